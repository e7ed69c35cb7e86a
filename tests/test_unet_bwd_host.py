"""models.unet_bwd.walk on the host: the skip-connection rule of the U-Net backwards on hand-built tapes with integer
"gradients".  No device, no kernels.

Every callback returns g + 1, and a "res" callback returns 100 * (its tape position) as the gradient of its x1, so each parked
gradient is a distinct multiple of 100 and the units count the callbacks run so far.  The two layouts are the tapes the training
forwards write for a DDPM Model(ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[8], resolution=16) and an EDM UNetModel
(channel_mult=(1, 2), num_res_blocks=1, attention at 8x8, resblock_updown=True): the EDM net resamples inside "res" entries
where the DDPM net has "down" / "up" entries."""
import pytest

from models.unet_bwd import walk


def res(x1=None):
    return ("res", None, "x0", x1)


def push(idx):
    return ("push", None, idx)


def skip(idx):
    return ("skip", None, idx)


ATTN, UP, DOWN, CAT = ("attn", None), ("up", None, "x"), ("down", None, "x"), "skip tensor"
DOWN_PATH = {"ddpm": [res(), push(1), DOWN, push(2), res(), ATTN, push(3)],
             "edm": [res(), push(1), res(), push(2), res(), ATTN, push(3)]}
UP_PATH = {"ddpm": [skip(3), res(CAT), ATTN, skip(2), res(CAT), ATTN, UP, skip(1), res(CAT), skip(0), res(CAT)],
           "edm": [skip(3), res(CAT), ATTN, skip(2), res(CAT), ATTN, res(), skip(1), res(CAT), skip(0), res(CAT)]}
MID = [res(), ATTN, res()]


def tape_of(net):
    return DOWN_PATH[net] + MID + UP_PATH[net]


def run(tape, g=0):
    """-> (result, log): log = [(position, kind, g handed in)] in call order."""
    log = []
    tape = [(e[0], i) + e[2:] for i, e in enumerate(tape)]      # the module slot, which walk() does not read, holds the position

    def cb(kind):
        def f(entry, g):
            pos = entry[1]
            log.append((pos, kind, g))
            return (g + 1, 100 * pos if entry[3] is not None else None) if kind == "res" else g + 1
        return f
    return walk(tape, g, cb("res"), cb("attn"), cb("up"), cb("down")), log


@pytest.mark.parametrize("net", ["ddpm", "edm"])
def test_walk_parks_and_adds_skip_gradients(net):
    tape = tape_of(net)
    out, log = run(tape, g=7)
    called = [i for i, e in enumerate(tape) if e[0] not in ("push", "skip")]
    # callbacks run once per entry in reverse tape order, each under its own kind
    assert [p for p, _, _ in log] == called[::-1]
    assert all(kind == tape[p][0] for p, kind, _ in log)
    g_in = {p: g for p, _, g in log}
    consumer = {tape[i - 1][2]: i for i, e in enumerate(tape) if e[0] == "res" and e[3] is not None}
    assert sorted(consumer) == [0, 1, 2, 3]
    # each push adds the gradient parked under its index exactly once, there: the callback before it (in tape order) is handed
    # what the callback after it returned plus 100 * (position of the consuming block)
    for q, e in enumerate(tape):
        if e[0] == "push":
            before, after = max(p for p in called if p < q), min(p for p in called if p > q)
            assert g_in[before] == g_in[after] + 1 + 100 * consumer[e[2]]
    # between two callbacks with no push between them nothing is added
    for a, b in zip(called, called[1:]):
        if not any(tape[q][0] == "push" for q in range(a, b)):
            assert g_in[a] == g_in[b] + 1
    # index 0 (the stem's output, which has no push entry) is added after the loop
    assert out == g_in[called[0]] + 1 + 100 * consumer[0]
    assert out == 7 + len(called) + 100 * sum(consumer.values())


def test_walk_ignores_an_index_no_block_consumed():
    tape = tape_of("ddpm")
    assert run(tape + [push(9)])[0] == run(tape)[0]        # (appended, so that the positions run() parks stay the same)
    # a down-path-only tape: nothing is parked, the pushes add nothing
    assert run(DOWN_PATH["edm"] + MID, g=5)[0] == 5 + 7


@pytest.mark.parametrize("bad", [
    [res(), push(1), skip(1), ATTN, res(CAT)],           # an entry between the skip and its concat block
    [res(), push(1), skip(1), res()],                    # a skip in front of a block that concatenates nothing
    [res(), push(1), res(CAT)],                          # a concat block without a skip entry
    [res(CAT)],                                          # ... at the start of the tape
    [skip(0)],
])
def test_walk_raises_on_a_misplaced_skip(bad):
    with pytest.raises(AssertionError):
        run(bad)
