"""dxmi_hip.packs.WeightPacks on the three nets that keep packed bf16 weight sets: a set refreshed in place (plan replay) equals
one built from scratch bit for bit, its buffers keep their addresses across an in-place parameter update, ops.PACK_GENERATION moves
exactly when buffers do, entries a backward packs on demand go at every refresh, and a set that cannot be replayed is rebuilt."""
import pytest
import torch
import torch.nn as nn

from test_hip_edm import PLAIN, TINY_KW, build as build_cm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from dxmi_hip import ops as o
    o.device_check()
    return o


def _formula(net):
    from oracle.weights import formula_tensor
    net.load_state_dict({k: formula_tensor(k, v.shape) for k, v in net.state_dict().items()})
    return net.to(DEV).eval()


def _value():
    from models.modules import IGEBMEncoderV2
    net = _formula(IGEBMEncoderV2(in_chan=3, out_chan=1, use_spectral_norm=False, keepdim=False, out_activation="linear", nh=128))
    # 32x32: three stride-2 blocks, and the conv kernels take no map below 4x4
    return net, (lambda x: net(x)), (lambda: net.packed_transposed()), net.blocks[0].conv1.weight, 32


def _small():
    from models.DxMI.unet_small import Model
    from models.DxMI.unet_small_train import _pack_t, forward_with_grad
    # ch 128 x mult 2 = the 256-channel 16x16 AttnBlock (the derived entries); the concat ResnetBlocks of the up path: short_t pairs
    net = _formula(Model(ch=128, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[16], resolution=32, in_channels=3, out_ch=3,
                         dropout=0.0))
    t = torch.tensor([3.0, 900.0], device=DEV)
    return net, (lambda x: forward_with_grad(net, x, t)), (lambda: _pack_t(net)), net.mid.block_1.conv1.weight, 32


def _cm(over):
    from models.cm.unet_train import _pack_t, forward_with_grad
    net, _, _ = build_cm(TINY_KW, over)
    t = torch.tensor([700.0, -900.0], device=DEV)
    y = None if over else torch.tensor([5, 321], device=DEV)
    return net, (lambda x: forward_with_grad(net, x, t, y)), (lambda: _pack_t(net)), net.middle_block[0].in_layers[2].weight, 16


CASES = {"value": _value, "small_unet": _small, "cm_unet": lambda: _cm(None), "cm_unet_plain": lambda: _cm(PLAIN)}


@pytest.mark.parametrize("case", list(CASES))
def test_weight_packs(ops, monkeypatch, case):
    net, fwd, packed_t, both_sets_weight, res = CASES[case]()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, res, res, generator=g).to(DEV).requires_grad_(True)
    names = {id(m): n for n, m in net.named_modules()}

    def step():
        for p in net.parameters():
            p.grad = None
        fwd(x).float().square().mean().backward()

    def perturb():
        with torch.no_grad():
            for p in net.parameters():
                p.add_(torch.randn(p.shape, generator=g).to(DEV) * 0.01)      # in place: versions bump, addresses stay

    def buffers():
        """(set, module name, role[, member]) -> every device buffer of the two sets."""
        out = {}
        for name, d in (("f", net.packed()), ("t", packed_t())):
            for k, v in d.items():
                key = (name, k) if not isinstance(k, tuple) or k[0] not in names else (name, names[k[0]]) + k[1:]
                for j, e in enumerate(v if isinstance(v, tuple) else (v,)):
                    if isinstance(e, ops.PackedConvWeight):
                        out[key + (j,)] = e.buf
                    elif torch.is_tensor(e) and not isinstance(e, nn.Parameter):
                        out[key + (j,)] = e
                    else:
                        assert e is None or isinstance(e, (int, nn.Parameter)), (k, type(e))
        return out

    def snapshot():
        return {k: v.clone() for k, v in buffers().items()}

    def on_demand():
        pt = net._packs_t
        return {k if isinstance(k, str) else k[1] for k in pt.entries if k not in pt.planned}

    want_on_demand = {"value": set(), "small_unet": {"conv_in_t", "tproj_t", "dense1_t", "short_t"}}.get(case, {"conv_in_t", "skip_t"})

    def equals_fresh():
        """The sets as a step leaves them (on-demand entries included) against sets built from scratch of the same parameters."""
        step()
        assert on_demand() == want_on_demand
        have = snapshot()
        net._packs.forget()
        net._packs_t.forget()
        step()
        fresh = snapshot()
        assert set(have) == set(fresh) and len(fresh) > 10
        for k in fresh:
            assert torch.equal(have[k], fresh[k]), k

    step()                                          # full builds; the backward packs its on-demand entries
    assert on_demand() == want_on_demand

    # ---- unchanged parameters: nothing runs
    gen = ops.PACK_GENERATION
    pk, pkt = net.packed(), packed_t()
    assert net.packed() is pk and packed_t() is pkt and ops.PACK_GENERATION == gen

    # ---- in-place update: replayed into the same buffers, same generation, on-demand entries dropped
    perturb()
    net.refresh_packs()
    assert on_demand() == set()
    planned = buffers()
    assert ops.PACK_GENERATION == gen and net.packed() is pk and packed_t() is pkt
    held = {k: (v, v.data_ptr()) for k, v in planned.items()}
    perturb()
    net.refresh_packs()
    assert ops.PACK_GENERATION == gen
    assert {k: v.data_ptr() for k, v in buffers().items()} == {k: p for k, (_, p) in held.items()}
    equals_fresh()                                  # replayed == fresh, bit for bit
    net.prepare_capture()
    assert on_demand() == set()

    # ---- parameters moved: every buffer new (the old ones are still held), one generation per set
    held = buffers()
    gen = ops.PACK_GENERATION
    for p in net.parameters():
        p.data = p.data.clone()
    moved = buffers()
    assert ops.PACK_GENERATION == gen + 2
    old_ptrs = {v.data_ptr() for v in held.values()}
    assert set(moved) == set(held)
    for k, v in moved.items():
        assert v is not held[k] and v.data_ptr() not in old_ptrs, k

    # ---- replay switched off, then a packed source that has to be copied: every refresh is a full build
    def refused():
        for _ in range(2):
            gen = ops.PACK_GENERATION
            perturb()
            net.refresh_packs()
            assert ops.PACK_GENERATION == gen + 2
        equals_fresh()

    monkeypatch.setattr(ops, "PACK_PLAN_REPLAY", False)
    refused()
    monkeypatch.setattr(ops, "PACK_PLAN_REPLAY", True)
    perturb()
    gen = ops.PACK_GENERATION
    net.refresh_packs()
    assert ops.PACK_GENERATION == gen               # (back on the replay path)
    w = both_sets_weight
    w.data = w.data.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)
    assert not w.is_contiguous()
    net.refresh_packs()                             # moved: full build, which finds the source it cannot pack in place
    refused()
