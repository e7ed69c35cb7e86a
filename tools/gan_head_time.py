"""Time the launches of DMD2's GAN head at the ImageNet-64 size and the U-Net pass that stops at the bottleneck against
the full pass, on one GPU, in one process.

    python tools/gan_head_time.py [--out profiles/gan_head_time.json]

  head   C = 768, map 8, N = 16: dxmi_gan_conv4s2_fwd / _dgrad / _wgrad / _pack, the head's forward (features + logit loss), its full
         and its input-only backward; median and minimum of 30 calls after 5 warm-up calls, device events around each call;
  nets   the full-size ImageNet-64 EDM net (synthetic weights, dropout 0) at N = 16: input_forward against encoder_input_forward,
         forward + input backward of both, and the generator's whole GAN term (encoder forward, head, head input backward, encoder
         input backward); median and minimum of 10 calls after 3.
Prints one JSON line and writes it to --out, each entry [median, minimum] in microseconds.  The figures are stated as measured; no
test or threshold rests on them.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-by-maxentirl_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from dm_step_time import MODEL  # noqa: E402
from dxmi_hip import ops  # noqa: E402
from models.cm import unet_train as ut  # noqa: E402
from models.cm.gan_head import GANHead  # noqa: E402
from models.cm.script_util import create_model_and_diffusion  # noqa: E402

DEV = "cuda:0"
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gan_head_time.json"))
args = ap.parse_args()


def timed(fn, warm=5, reps=30):
    """-> (median, minimum) of `reps` calls in microseconds."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return round(statistics.median(ts), 1), round(min(ts), 1)

out = {}
N, C, m = 16, 768, 8
torch.manual_seed(0)
head = GANHead(C, m).to(DEV)
h = torch.randn(N, m, m, C, device=DEV).to(torch.bfloat16)
pk = head.packed()
dy = torch.randn(N, m // 2, m // 2, C, device=DEV).to(torch.bfloat16)
out["conv4s2_fwd_us"] = timed(lambda: ops.gan_conv4s2_fwd(h, pk["c0"], head.cls_pred_branch[0].bias))
out["conv4s2_dgrad_us"] = timed(lambda: ops.gan_conv4s2_dgrad(dy, pk["c0"]))
out["conv4s2_wgrad_us"] = timed(lambda: ops.gan_conv4s2_wgrad(h, dy))
out["conv4s2_pack_us"] = timed(lambda: ops.gan_conv4s2_pack(head.cls_pred_branch[0].weight, out=pk["c0"]))
sign = torch.ones(N, device=DEV)
def fwd():
    a2, saved = head.features(h)
    return head.logit_loss(a2, sign) + (saved,)
out["head_forward_us"] = timed(fwd)
lg, loss, saved = fwd()
assert torch.isfinite(lg).all()
out["head_backward_full_us"] = timed(lambda: head.backward(saved, sign, lg, sign, 1.0, params=True))
out["head_backward_input_us"] = timed(lambda: head.backward(saved, sign, lg, sign, 1.0, params=False))
d_h, grads = head.backward(saved, sign, lg, sign, 1.0, params=True)
assert all(torch.isfinite(g).all() for g in grads) and torch.isfinite(d_h.float()).all()
assert [tuple(g.shape) for g in grads] == [tuple(p.shape) for p in head.parameters()]
print("full-size head ok: logits", lg[:4].tolist())

net, _ = create_model_and_diffusion(**dict(MODEL, dropout=0.0))
net = net.to(DEV).eval()
x = torch.randn(N, 3, 64, 64, device=DEV)
t = torch.linspace(-800, 900, N, device=DEV)
y = torch.arange(N, device=DEV)
out["unet_input_forward_us"] = timed(lambda: ut.input_forward(net, x, t, y), 3, 10)
out["unet_encoder_input_forward_us"] = timed(lambda: ut.encoder_input_forward(net, x, t, y), 3, 10)
v = torch.randn(N, 3, 64, 64, device=DEV)
def full():
    F, tape = ut.input_forward(net, x, t, y)
    return ut.input_backward(tape, v)
def enc():
    hh, tape = ut.encoder_input_forward(net, x, t, y)
    return ut.encoder_input_backward(tape, hh)
out["unet_input_fwd_bwd_us"] = timed(full, 3, 10)
out["unet_encoder_input_fwd_bwd_us"] = timed(enc, 3, 10)
hh, tape = ut.encoder_input_forward(net, x, t, y)
assert tuple(hh.shape) == (N, 8, 8, 768)
def gen_term():
    hh, tape = ut.encoder_input_forward(net, x, t, y)
    a2, saved = head.features(hh)
    lg, loss = head.logit_loss(a2, sign)
    d_h, _ = head.backward(saved, sign, lg, sign, 1.0, params=False)
    return ut.encoder_input_backward(tape, d_h)
out["generator_gan_term_us"] = timed(gen_term, 3, 10)
print(json.dumps(out))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(out, open(args.out, "w"), indent=1)
