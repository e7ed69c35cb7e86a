"""The tape API of both U-Nets (models/unet_bwd.py tape_api, bound in models/DxMI/unet_small_train.py and
models/cm/unet_train.py) against the autograd path, bit for bit, on 16x16 nets at batch 2:
train_backward(train_forward(...)) leaves the .grads of forward_with_grad(...).backward(v) in train mode with the same dropout
seeds; input_backward(input_forward(...)) is input_vjp and the dx of the full backward in eval mode; and a tape walked a second
time gives the first walk's result again (the walk changes nothing on the tape; callers drop it after one walk)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DDPM_KW = dict(ch=64, out_ch=3, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[8], dropout=0.1, in_channels=3, resolution=16)


def _ddpm():
    from models.DxMI import unet_small_train as mod
    from models.DxMI.unet_small import Model
    from oracle.weights import formula_tensor
    net = Model(**DDPM_KW)
    net.load_state_dict({k: formula_tensor(k, v.shape) for k, v in net.state_dict().items()})
    return mod, net.to(DEV), torch.tensor([37.0, 640.0], device=DEV), ()


def _edm(over):
    from models.cm import unet_train as mod
    from test_hip_edm import TINY_KW, build
    net = build(TINY_KW, dict(over, dropout=0.1))[0]
    cond = (torch.tensor([3, 871], device=DEV),) if net.num_classes is not None else ()
    return mod, net, torch.tensor([-89.17, 549.31], device=DEV), cond


class Case:
    """One net with its operands and, computed once, the autograd path's results in train and in eval mode."""

    def __init__(self, mod, net, t, cond):
        from dxmi_hip import ops
        ops.device_check()
        self.mod, self.net, self.t, self.cond = mod, net, t, cond
        gen = torch.Generator().manual_seed(41)
        self.x, self.v = (torch.randn(2, 3, 16, 16, generator=gen).to(DEV) for _ in range(2))
        net.dropout_seed = 1234
        self.ref = {train: self.autograd(train) for train in (True, False)}
        net.train()

    def reset(self):
        self.net.__dict__["_dropout_calls"] = 0

    def autograd(self, train):
        self.net.train(train)
        self.reset()
        for p in self.net.parameters():
            p.grad = None
        xg = self.x.clone().requires_grad_(True)
        out = self.mod.forward_with_grad(self.net, xg, self.t, *self.cond)
        out.backward(self.v)
        return out.detach(), xg.grad, [p.grad for p in self.net.parameters()], list(self.net.dropout_seeds_used)


@pytest.fixture(scope="module", params=["ddpm", "edm", "edm_plain"])
def case(request):
    from test_hip_edm import PLAIN
    return Case(*{"ddpm": _ddpm, "edm": lambda: _edm({}), "edm_plain": lambda: _edm(PLAIN)}[request.param]())


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and torch.equal(a, b))


def test_train_backward_is_the_autograd_backward(case):
    out, _, grads, seeds = case.ref[True]
    assert len(seeds) > 0 and any(g is not None and bool(g.abs().max() > 0) for g in grads)
    case.reset()
    with torch.no_grad():
        F, tape = case.mod.train_forward(case.net, case.x, case.t, *case.cond)
        got = case.mod.train_backward(tape, case.v)
    assert torch.equal(F, out) and list(case.net.dropout_seeds_used) == seeds
    assert len(got) == len(grads)
    bad = [n for (n, _), a, b in zip(case.net.named_parameters(), got, grads) if not same(a, b)]
    assert not bad, bad


def test_input_backward_is_input_vjp_and_the_full_dx(case):
    out, dx, _, _ = case.ref[False]
    mod, net = case.mod, case.net
    assert net.training                                     # dropout 0.1: the input-only path runs in eval and puts train back
    F, g = mod.input_vjp(net, case.x, case.t, case.v, *case.cond)
    F2, tape = mod.input_forward(net, case.x, case.t, *case.cond)
    assert net.training
    g2 = mod.input_backward(tape, case.v)
    assert torch.equal(F, out) and torch.equal(F2, out)
    assert g.dtype == torch.float32 and torch.equal(g, dx) and torch.equal(g2, dx)
    assert not torch.equal(out, case.ref[True][0])          # (the train-mode reference did apply dropout)


def test_second_walk_of_a_tape_repeats_the_first(case):
    mod, net = case.mod, case.net
    case.reset()
    with torch.no_grad():
        _, tape = mod.train_forward(net, case.x, case.t, *case.cond)
        first, second = mod.train_backward(tape, case.v), mod.train_backward(tape, case.v)
    assert all(same(a, b) for a, b in zip(first, second)) and all(same(a, b) for a, b in zip(first, case.ref[True][2]))
    _, tape = mod.input_forward(net, case.x, case.t, *case.cond)
    g1, g2 = mod.input_backward(tape, case.v), mod.input_backward(tape, case.v)
    assert torch.equal(g1, g2) and torch.equal(g1, case.ref[False][1])
