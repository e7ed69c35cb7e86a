"""UniPC on the EDM nets on the device: dxmi_edm_unipc_stage through the checks of tests/test_hip_unipc_sample.py (the bounds are
stated there; the family below says what differs: the Karras preconditioning D0 = c_out F + c_skip x, FIRST's scaling and the second
output stream x_in), xc = NULL against dxmi_edm_dpm_stage, and replay against eager and batch invariance on the shrunken HIP
UNetModel with labels."""
import pytest
import torch

import test_hip_unipc_sample as tu
from test_hip_unipc_sample import DEV, MID, SENTINEL, SHAPES, STEPS, ops  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu


def diffusion():
    from models.cm.karras_diffusion import KarrasDenoiser
    return KarrasDenoiser()


class EDM(tu.Teacher):
    name, prefix, x_in = "edm", "EUT_", True

    def schedule(self, steps=STEPS, order=3, variant="bh1", corrector=True, clip=True):
        from models.cm.unipc_sample import edm_unipc_schedule
        return edm_unipc_schedule(diffusion(), steps, order, variant, corrector, clip_denoised=clip)

    def stage(self, tab, t, first=False, f=None, **kw):
        self.ops.edm_unipc_stage(self.ops.EDM_UNIPC_FIRST if first else self.ops.EDM_UNIPC_STEP, tab, t, model_out=f, **kw)

    def products(self, K, x, f):
        return K[self.c["COUT"]] * f, K[self.c["CSKIP"]] * x

    def make(self, K, x0, e):
        x = (x0 + float(K[self.c["SIGMA"]]) * e).float()
        return x, ((x0 - float(K[self.c["CSKIP"]]) * x) / float(K[self.c["COUT"]])).float()

    def parent(self, steps, order):
        from models.cm.dpm_sample import edm_dpm_schedule
        sch = edm_dpm_schedule(diffusion(), steps, order, solver_type="midpoint")
        return sch, lambda tab, t, f=None, **kw: self.ops.edm_dpm_stage(self.ops.EDM_DPM_STEP, tab, t, model_out=f, **kw)


@pytest.mark.parametrize("corrector", [True, False])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("N,CHW", SHAPES)
def test_stage_vs_fp64(ops, N, CHW, clip, corrector):
    tu.check_stage_vs_fp64(EDM(ops), N, CHW, clip, corrector)


@pytest.mark.parametrize("N,CHW", SHAPES)
def test_first_mode(ops, N, CHW):
    fam = EDM(ops)
    sch = fam.schedule()
    tab = sch.device_table(DEV)
    x = torch.randn(N, CHW, generator=torch.Generator().manual_seed(CHW))
    for row in (0, 3):
        xd, x_in, t = x.to(DEV).clone(), torch.full((N, CHW), SENTINEL, device=DEV), torch.full((N,), -1.0, device=DEV)
        ops.edm_unipc_stage(ops.EDM_UNIPC_FIRST, tab, t, row=row, x=xd, x_in=x_in)
        torch.cuda.synchronize()
        K = sch.table[row]
        want_x = x * K[ops.EUT_XSCALE]
        assert torch.equal(xd.cpu(), want_x) and torch.equal(x_in.cpu(), K[ops.EUT_CIN] * want_x)
        assert torch.equal(t.cpu(), torch.full((N,), float(K[ops.EUT_T])))


@pytest.mark.parametrize("through_ctl", [False, True])
@pytest.mark.parametrize("N,CHW", [(3, 75), (5, 3072)])
def test_unread_slots_and_state_are_not_read(ops, N, CHW, through_ctl):
    tu.check_unread_slots_and_state(EDM(ops), N, CHW, through_ctl)


def test_control_block_equals_by_value(ops):
    tu.check_control_block(EDM(ops))


def test_out_of_range_row_in_the_control_block(ops):
    tu.check_poisoned_row(EDM(ops))


def test_nan_stays_in_its_image(ops):
    tu.check_nan_stays_in_its_image(EDM(ops))


@pytest.mark.parametrize("N,CHW", [(3, 75), (5, 3072), (1, 263347)])
def test_without_xc_is_edm_dpm_stage(ops, N, CHW):
    tu.check_without_xc_is_the_parent(EDM(ops), N, CHW)


def test_malformed_calls(ops):
    from dxmi_hip import DxmiError
    fam = EDM(ops)
    sch = fam.schedule()
    tab = sch.device_table(DEV)
    x, f, xc, *d = (v.to(DEV) for v in tu.operands(fam, sch.table[MID], 4, 768, 2))
    t, out, hist = torch.empty(4, device=DEV), torch.empty(4, 768, device=DEV), torch.zeros(4, 4, 768, device=DEV)
    x_in = torch.empty(4, 768, device=DEV)
    step = lambda **kw: ops.edm_unipc_stage(ops.EDM_UNIPC_STEP, **dict(dict(tab=tab, t_out=t, row=MID, x=x, xc=xc, model_out=f, hist=hist,
                                                                            x_in=x_in, out=out), **kw))
    first = lambda **kw: ops.edm_unipc_stage(ops.EDM_UNIPC_FIRST, **dict(dict(tab=tab, t_out=t, row=0, x=x.clone(), x_in=x_in), **kw))
    bad = [lambda: step(row=STEPS), lambda: step(model_out=f[:3]), lambda: step(out=None), lambda: step(hist=hist[:3]),
           lambda: step(xc=x), lambda: step(xc=xc.double()), lambda: step(x_in=None),
           lambda: step(x_in=None, row=STEPS - 1, ctl=torch.zeros(4, dtype=torch.int32, device=DEV)), lambda: step(x_in=x_in[:3]),
           lambda: step(tab=tab[:, :16]), lambda: first(x=None), lambda: first(x_in=None), lambda: first(row=STEPS)]
    for i, call in enumerate(bad):
        with pytest.raises(DxmiError):
            call()
            pytest.fail(f"malformed call {i} was accepted")
    step()
    step(xc=None)
    step(row=STEPS - 1, x_in=None)
    first()
    torch.cuda.synchronize()


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("S", [6, 8])
def test_loop_with_analytic_network(ops, S, clip):
    from models.cm.unipc_sample import edm_unipc_sample
    tu.check_loop(EDM(ops), lambda net, shape, **kw: edm_unipc_sample(diffusion(), net, shape, **kw), S, clip)


# ------------------------------------------------------------------------------------------ the loop on the HIP UNetModel
SHAPE = (4, 3, 16, 16)
LABELS = [3, 871, 12, 500]


@pytest.fixture(scope="module")
def unet(ops):
    """The shrunken class-conditional UNetModel of tests/test_hip_edm.py with formula weights, in eval mode."""
    from test_hip_edm import TINY_KW, build
    net, diff, _ = build(TINY_KW)
    assert net.num_classes is not None
    return net, diff


def test_replay_equals_eager_on_the_unet(unet):
    from models.cm.unipc_sample import edm_unipc_sample, replay_graphs
    from test_hip_edm_dpm_sample import Counting
    net, diff = unet
    model = Counting(net)
    S = 6
    y = torch.tensor(LABELS, device=DEV)
    kw = dict(steps=S, device=DEV, model_kwargs={"y": y})
    torch.manual_seed(5)
    eager = edm_unipc_sample(diff, model, SHAPE, **kw).clone()
    assert model.calls == S and replay_graphs(model) == [] and all(torch.equal(v, y) for v in model.labels)
    assert torch.isfinite(eager).all() and eager.abs().max() <= 1 and eager.std() > 0
    model.calls = 0
    torch.manual_seed(5)
    first = edm_unipc_sample(diff, model, SHAPE, use_graph=True, **kw).clone()
    assert torch.equal(first, eager) and model.calls == 2                   # python ran for the warm-up row and the capture
    graphs = replay_graphs(model)
    assert len(graphs) == 1 and graphs[0].captures == 1 and graphs[0].replays == S - 2
    model.calls = 0
    torch.manual_seed(5)
    second = edm_unipc_sample(diff, model, SHAPE, use_graph=True, **kw)
    assert torch.equal(second, eager) and model.calls == 0 and graphs[0].captures == 1 and graphs[0].replays == 2 * S - 2
    # the labels are a static buffer: other labels through the same graph give what the eager loop gives for them
    y2 = torch.tensor(LABELS[::-1], device=DEV)
    torch.manual_seed(5)
    other = edm_unipc_sample(diff, model, SHAPE, use_graph=True, **dict(kw, model_kwargs={"y": y2}))
    assert other.data_ptr() == second.data_ptr()                            # the returned tensor is static
    other = other.clone()
    torch.manual_seed(5)
    assert model.calls == 0 and not torch.equal(other, eager)
    assert torch.equal(other, edm_unipc_sample(diff, model, SHAPE, **dict(kw, model_kwargs={"y": y2})))
    # the corrector is in the result
    torch.manual_seed(5)
    assert not torch.equal(edm_unipc_sample(diff, model, SHAPE, corrector=False, **kw), eager)


def test_batch_invariance_with_the_deterministic_generator(unet):
    from models.cm.random_util import get_generator
    from models.cm.unipc_sample import edm_unipc_sample
    net, diff = unet
    y = torch.tensor(LABELS, device=DEV)
    gen = get_generator("determ", 4, seed=(1 << 35) + 3)

    def run(done, rows, use_graph):
        gen.set_done_samples(done)
        out = edm_unipc_sample(diff, net, (rows.stop - rows.start, 3, 16, 16), steps=5, device=DEV, generator=gen,
                               model_kwargs={"y": y[rows]}, use_graph=use_graph).clone()
        assert gen.draw == 1                  # the solver draws x_T alone
        return out
    whole = run(0, slice(0, 4), False)
    parts = torch.cat([run(0, slice(0, 2), True), run(2, slice(2, 4), True)])
    assert torch.isfinite(whole).all() and whole.abs().max() <= 1 and whole.std() > 0.05
    for i in range(4):
        assert torch.equal(parts[i], whole[i]), i
    assert not torch.equal(whole[0], whole[1])
