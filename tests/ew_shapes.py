"""The N x shape cases of the launch-against-float64 tests of the elementwise training launches (csrc/ew_common.h).

The map launches run a grid of at most 64 workgroups per image, each taking 256 lanes x 4 f32x4 per trip: an image above
64 * 256 * 4 * 4 = 262144 elements sends the grid-stride loop on a second trip.  SECOND_TRIP is the smallest 3-channel square image
that does (262848 elements, 65712 f32x4: the second trip is a partial one); it runs once per test, with one image."""
import pytest

SECOND_TRIP = (3, 296, 296)


def n_by_shape(shapes, Ns=(1, 7)):
    """parametrize("N,shape", ...): every N x shape under the ids two stacked parametrize decorators give, then N = 1 at SECOND_TRIP."""
    cases = [pytest.param(N, s, id=f"{N}-shape{i}") for i, s in enumerate(shapes) for N in Ns]
    return cases + [pytest.param(1, SECOND_TRIP, id=f"1-shape{len(shapes)}")]
