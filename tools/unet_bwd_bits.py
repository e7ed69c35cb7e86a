"""Bits and library calls of the two U-Net backwards: python tools/unet_bwd_bits.py OUT.json

For each case: one forward and one full backward through forward_with_grad(...).backward(v), then one input_vjp.  Recorded: the
SHA-256 of the output, of dx and of every parameter gradient (net.parameters() order), of input_vjp's (F, g), and the ordered
dxmi_* entry points with their integer and float arguments seen during the backward and during input_vjp (a proxy in front of the
library object, as the host-cost mode of tools/edm_train_bench.py substitutes it), wgrad_branch regions and wgrad_join included.
OUT.json holds, per case, the hashes of the output and dx, the number of gradients and of calls, and one SHA-256 over the list of
gradient hashes and over each call list (small enough to keep under profiles/); OUT.detail.json holds the lists themselves, to
find where two runs part.  Run on two checkouts, the two OUT.json are equal exactly when both compute the same bits from the
same launches.  The tool uses only names both sides of such a comparison have: the nets, forward_with_grad and input_vjp.

Cases (N = 2, 16x16): the DDPM Model of tests/test_hip_likelihood.py in train and eval mode (dropout 0.1); the EDM TINY_KW net of
tests/test_hip_edm.py (scale-shift norm, resblock_updown, class-conditional, 4 heads) with dropout 0.1 in train and eval mode;
the same net with the PLAIN overrides."""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diffusion-by-maxentirl_amd"), os.path.join(ROOT, "tests")]
import torch
from dxmi_hip import _lib, ops

DEV = "cuda:0"
DDPM_KW = dict(ch=64, out_ch=3, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[8], dropout=0.1, in_channels=3, resolution=16)


class Recorder:
    """The library object with every call logged while `log` is a list: [name, the arguments that are no pointers]."""

    def __init__(self, real):
        self.real, self.log = real, None

    def __getattr__(self, name):
        f = getattr(self.real, name)
        types = _lib.SIGNATURES.get(name, (None, []))[1]
        keep = [i for i, t in enumerate(types)
                if isinstance(t, type) and issubclass(t, ctypes._SimpleCData) and t not in (ctypes.c_void_p, ctypes.c_char_p)]

        def call(*a):
            if self.log is not None:
                self.log.append([name, [getattr(a[i], "value", a[i]) for i in keep if i < len(a)]])
            return f(*a)
        return call


def install():
    rec = Recorder(_lib.load())
    _lib._lib = rec
    join, branch = ops.wgrad_join, ops.wgrad_branch

    def wgrad_join(*a, **kw):
        if rec.log is not None:
            rec.log.append(["wgrad_join", []])
        return join(*a, **kw)

    class wgrad_branch(branch):
        def __enter__(self):
            if rec.log is not None:
                rec.log.append(["wgrad_branch enter", []])
            return super().__enter__()

        def __exit__(self, *exc):
            if rec.log is not None:
                rec.log.append(["wgrad_branch exit", []])
            return super().__exit__(*exc)
    ops.wgrad_join, ops.wgrad_branch = wgrad_join, wgrad_branch
    return rec


def sha(t):
    return "none" if t is None else hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def ddpm_case(train):
    from models.DxMI import unet_small_train as mod
    from models.DxMI.unet_small import Model
    from oracle.weights import formula_tensor
    net = Model(**DDPM_KW)
    net.load_state_dict({k: formula_tensor(k, v.shape) for k, v in net.state_dict().items()})
    return mod, net.to(DEV).train(train), torch.tensor([37.0, 640.0]), ()


def edm_case(train, over):
    from models.cm import unet_train as mod
    from test_hip_edm import TINY_KW, build
    net = build(TINY_KW, dict(over, dropout=0.1))[0]
    cond = (torch.tensor([3, 871], device=DEV),) if net.num_classes is not None else ()
    return mod, net.train(train), torch.tensor([-89.17, 549.31]), cond


def run(rec, mod, net, t, cond):
    gen = torch.Generator().manual_seed(41)
    x, v = (torch.randn(2, 3, 16, 16, generator=gen).to(DEV) for _ in range(2))
    t = t.to(DEV)
    torch.manual_seed(0)
    net.dropout_seed = 1234
    net.__dict__["_dropout_calls"] = 0
    xg = x.clone().requires_grad_(True)
    out = mod.forward_with_grad(net, xg, t, *cond)
    rec.log = []
    out.backward(v)
    torch.cuda.synchronize()
    row = {"backward_calls": rec.log, "out": sha(out), "dx": sha(xg.grad), "grads": [sha(p.grad) for p in net.parameters()]}
    net.__dict__["_dropout_calls"] = 0
    rec.log = []
    F, g = mod.input_vjp(net, x, t, v, *cond)
    torch.cuda.synchronize()
    row.update(vjp_calls=rec.log, vjp_F=sha(F), vjp_g=sha(g), training_after=bool(net.training))
    rec.log = None
    return row


def main():
    from test_hip_edm import PLAIN
    rec = install()
    cases = {"ddpm_train": lambda: ddpm_case(True), "ddpm_eval": lambda: ddpm_case(False),
             "edm_train": lambda: edm_case(True, {}), "edm_eval": lambda: edm_case(False, {}),
             "edm_plain_train": lambda: edm_case(True, PLAIN), "edm_plain_eval": lambda: edm_case(False, PLAIN)}
    res = {}
    lists = ("grads", "backward_calls", "vjp_calls")
    digest = lambda v: hashlib.sha256(json.dumps(v, separators=(",", ":")).encode()).hexdigest()
    short = {}
    for name, make in cases.items():
        row = res[name] = run(rec, *make())
        short[name] = {k: ({"n": len(v), "sha256": digest(v)} if k in lists else v) for k, v in row.items()}
        print(name, len(row["backward_calls"]), "backward calls,", len(row["vjp_calls"]), "input_vjp calls, dx", row["dx"][:16], flush=True)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "unet_bwd_bits.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for path, what in ((out, short), (os.path.splitext(out)[0] + ".detail.json", res)):
        with open(path, "w") as f:      # one case per line
            f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in what.items()) + "\n}\n")


if __name__ == "__main__":
    main()
