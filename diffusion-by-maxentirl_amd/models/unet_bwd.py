"""What the backward of the DDPM U-Net (models/DxMI/unet_small_train.py) and of the ADM / EDM U-Net (models/cm/unet_train.py) share.

Both training forwards leave a tape: a list of entries (kind, module, saved...), kind one of
  "res"   a residual block; slot 3 is x1, the skip tensor an up-path block concatenates to its input (None elsewhere);
  "attn", "up", "down"   an attention block, an upsample, a downsample;
  "push"  (., ., idx): the activation at this point was stored as hs[idx] (hs[0] is the stem's output and has no entry);
  "skip"  (., ., idx): the "res" entry that follows took hs[idx] as its x1;
  "tap"   (., .): the activation at this point was handed out by the forward (the EDM net's bottleneck, input_forward(tap=True));
          a cotangent given for it (walk's d_tap) joins the running gradient here.  A forward without a tap writes no such entry.
walk() runs the tape in reverse and owns the skip-connection rule: the x1 gradient of a concat block is parked under the index
its "skip" entry names and added where that activation was pushed.  Backward holds the state of one backward and the parts around
the walk that do not depend on the net: head, shortcut data gradient, stem, the rows of a concatenated dense layer, the
gradients in net.parameters() order.  tape_api() is the tape kept outside autograd, encoder_api() its form that stops at the bottleneck.  Nothing here asks which net it serves: the
GroupNorm, attention and resampling backwards and the embedding graphs stay in the nets' files and come in as callbacks.
"""
import torch

from dxmi_hip import ops
from dxmi_hip.packs import WeightPacks


def pack_t(net, build):
    """The transposed set of the net (dxmi_hip.packs.WeightPacks: cached on the net, refreshed with the parameters)."""
    if net._packs_t is None:
        net._packs_t = WeightPacks(net, build)
    return net._packs_t.get()


def up_sum(g):
    """transpose of nearest x2: sum over each 2x2 block (mean * 4, exact in bf16)."""
    out = ops.pool_act(g, True, ops.ACT_NONE)
    out.mul_(4.0)
    return out


def pool_t(g):
    """transpose of the 2x2 mean pool: every gradient value to its 4 sources, times 1/4."""
    out = ops.upsample2x(g)
    out.mul_(0.25)
    return out


def walk(tape, g, res_bwd, attn_bwd, up_bwd, down_bwd, d_tap=None):
    """The tape in reverse -> the gradient of hs[0].  res_bwd(entry, g) -> (d_x0, d_x1); the other callbacks (entry, g) -> g.
    d_tap: the cotangent of the tapped activation, added where the walk passes its "tap" entry (None: nothing is launched there)."""
    if d_tap is not None and not any(e[0] == "tap" for e in tape):
        raise ValueError("walk: a tap cotangent was given, but the forward that wrote this tape handed out no tap")
    gskip = {}
    i = len(tape) - 1
    while i >= 0:
        e = tape[i]
        kind = e[0]
        if kind == "res":
            g, d_x1 = res_bwd(e, g)
            if e[3] is not None:     # up-path block: (h, skip) concat; the preceding "skip" entry names the hs index
                if i == 0 or tape[i - 1][0] != "skip":
                    raise AssertionError("a concat block's tape entry must directly follow its skip entry")
                gskip[tape[i - 1][2]] = d_x1
                i -= 1
        elif kind == "attn":
            g = attn_bwd(e, g)
        elif kind == "up":
            g = up_bwd(e, g)
        elif kind == "down":
            g = down_bwd(e, g)
        elif kind == "push":         # h was stored as hs[idx]: the up path may have consumed it as a skip
            if e[2] in gskip:
                g = g + gskip.pop(e[2])
        elif kind == "tap":
            if d_tap is not None:
                if d_tap.shape != g.shape or d_tap.dtype != g.dtype:
                    raise ValueError(f"walk: the tap cotangent {tuple(d_tap.shape)} {d_tap.dtype} is not the tapped activation's "
                                     f"{tuple(g.shape)} {g.dtype}")
                g = g + d_tap
        elif kind == "skip":
            raise AssertionError("skip entry must directly precede the block that consumes it")
        i -= 1
    if 0 in gskip:
        g = g + gskip.pop(0)
    return g


class Backward:
    """One backward of ctx.net: the packs, the gradients found so far (parameter -> tensor) and `params`, False for an input-only
    walk (input_vjp): the data gradients alone, no weight, bias or embedding gradient is launched.  An autograd ctx has no
    input_only attribute, which means a full backward."""

    def __init__(self, ctx, build_packs_t):
        self.net = ctx.net
        self.pk, self.pkt = self.net.packed(), pack_t(self.net, build_packs_t)
        self.grads = {}
        self.params = not getattr(ctx, "input_only", False)

    def conv_wb(self, conv, x0, gy, k, x1=None, **kw):
        if not self.params:
            return
        dw, self.grads[conv.bias] = ops.conv2d_wgrad(x0, gy, k, in1=x1, with_bias=True, **kw)
        self.grads[conv.weight] = dw.reshape(conv.weight.shape)

    def head(self, conv_out, a_out, d_out):
        """out = conv_out(a_out) -> d a_out.  The gradient is padded to the 64 channels the packed conv_out has."""
        N, C, H, W = d_out.shape
        d_pad = torch.zeros((N, H, W, 64), dtype=torch.bfloat16, device=d_out.device)
        d_pad[..., :C] = d_out.permute(0, 2, 3, 1).to(torch.bfloat16)
        if self.params:
            with ops.wgrad_branch((a_out, d_pad)):       # (captured step: a parallel branch, joined in finish())
                wg = ops._conv2d_wgrad(a_out, d_pad, 3)
                self.grads[conv_out.weight] = wg[:C].contiguous()
            self.grads[conv_out.bias] = d_out.float().sum((0, 2, 3))
        return ops.conv2d(d_pad, self.pkt["conv_out"])

    def shortcut_dx(self, key, w, x0, x1, g, dxg0, dxg1):
        """Data gradient of a projection shortcut over the (x0, x1) concat, the GroupNorm dx of each source as the residual.
        The transposed fragments of `w`, split per concat source, are cached with the other packs under key + (C0,)."""
        C0 = x0.shape[3]
        w0t, w1t = self.net._packs_t.on_demand(key + (C0,), lambda: (
            ops.pack_conv_weight(w[:, :C0].contiguous(), transpose_flip=True),
            ops.pack_conv_weight(w[:, C0:].contiguous(), transpose_flip=True) if x1 is not None else None))
        d_x0 = ops.conv2d(g, w0t, residual=dxg0)
        return d_x0, (ops.conv2d(g, w1t, residual=dxg1) if x1 is not None else None)

    def stem(self, conv_in, x, g, want_dx):
        """g = the gradient of hs[0] = conv_in(x) -> dx (NCHW fp32), or None where the input takes no gradient."""
        if self.params:
            self.grads[conv_in.bias] = ops.colsum(g)
            self.grads[conv_in.weight] = ops.stem_conv_wgrad(x, g)
        if not want_dx:
            return None
        conv_in_t = self.net._packs_t.on_demand("conv_in_t", lambda: ops.pack_conv_weight(conv_in.weight, transpose_flip=True))
        return ops.conv2d(g, conv_in_t, out_nchw_f32=True)

    def dense_rows(self, linears, dw_cat, db_cat):
        """The gradients of the dense layers that were evaluated as one concatenated operator, handed back row block by row block."""
        off = 0
        for lin in linears:
            n = lin.weight.shape[0]
            self.grads[lin.weight], self.grads[lin.bias] = dw_cat[off:off + n], db_cat[off:off + n]
            off += n

    def finish(self, n_inputs, dx):
        """What the Function's backward returns: n_inputs non-parameter slots (dx in slot 1), then net.parameters() order."""
        out = (None, dx) + (None,) * (n_inputs - 2)
        if not self.params:
            return out
        ops.wgrad_join()
        return out + tuple(self.grads.get(prm) for prm in self.net.parameters())


class Tape:
    """What a training forward keeps for its backward, held outside autograd: it takes the place of the ctx for a caller that is an
    autograd node of its own around the network (the loss nodes), or that keeps no graph at all.  No input gradient is formed:
    such a caller differentiates the parameters only."""
    needs_input_grad = (False, False)
    input_only = False


class InputTape(Tape):
    """The tape of input_vjp: the backward walks it for the input gradient alone."""
    needs_input_grad = (False, True)
    input_only = True


class EncoderTape(Tape):
    """The tape of a forward that stops at the bottleneck (encoder_api): its backward starts from the bottleneck's cotangent."""
    encoder_only = True


class EncoderInputTape(InputTape):
    encoder_only = True


def _forward(fn, n_inputs, tape, net, x, t, cond):
    """fn.forward on `tape` in place of a ctx -> (output, tape); `cond` the conditioning after t, None where left out."""
    return fn.forward(tape, net, x, t, *cond, *(None,) * (n_inputs - 3 - len(cond))), tape


def _eval_forward(fn, n_inputs, tape, net, x, t, cond):
    """_forward with dropout off: eval mode under no_grad, the net's own mode restored."""
    was_training = net.training
    net.eval()
    try:
        with torch.no_grad():
            return _forward(fn, n_inputs, tape, net, x, t, cond)
    finally:
        net.train(was_training)


def encoder_api(fn, n_inputs):
    """-> (encoder_forward, encoder_backward, encoder_input_forward, encoder_input_backward): tape_api's functions for a net whose
    Function honours ctx.encoder_only, i.e. returns the bottleneck activation h (NHWC bf16) in place of the model output and takes
    its cotangent d_h (NHWC bf16) in backward.  The truncated tape has no "skip" entry, so walk() runs it unchanged."""

    def encoder_forward(net, x, t, *cond):
        """The training forward of `net` up to its bottleneck (dropout live in train mode; net.dropout_seeds_used lists the seeds of
        the sites that ran) -> (h, tape)."""
        return _forward(fn, n_inputs, EncoderTape(), net, x, t, cond)

    def encoder_backward(tape, d_h):
        """-> the gradients of net.parameters(), in that order; None for every parameter downstream of the bottleneck (the rows a
        concatenated dense operator holds for downstream blocks come back as exact zeros)."""
        return tuple(fn.backward(tape, d_h.contiguous())[n_inputs:])

    def encoder_input_forward(net, x, t, *cond):
        """encoder_forward in eval mode under no_grad (the net's own mode restored), its tape kept for encoder_input_backward."""
        return _eval_forward(fn, n_inputs, EncoderInputTape(), net, x, t, cond)

    def encoder_input_backward(tape, d_h):
        """-> dx (NCHW fp32) = d(d_h . h)/dx: the walk with no parameter-gradient launch.  A tape is walked once."""
        with torch.no_grad():
            return fn.backward(tape, d_h.contiguous())[1]

    return encoder_forward, encoder_backward, encoder_input_forward, encoder_input_backward


def tape_api(fn, n_inputs):
    """-> (train_forward, train_backward, input_forward, input_backward, input_vjp) of the autograd Function `fn`, whose forward
    takes (ctx, net, x, t, *cond, *params): n_inputs non-parameter inputs, `cond` the conditioning after t (None where left out)."""

    def train_forward(net, x, t, *cond):
        """The training forward of `net` (dropout applied in train mode; net.dropout_seeds_used lists its seeds) outside autograd
        -> (model output, tape).  Drop the tape where no backward follows."""
        return _forward(fn, n_inputs, Tape(), net, x, t, cond)

    def train_backward(tape, d_out):
        """The backward of train_forward -> the gradients of net.parameters(), in that order."""
        return tuple(fn.backward(tape, d_out)[n_inputs:])

    def input_forward(net, x, t, *cond, tap=False):
        """The first half of input_vjp -> (F, tape): the training forward with dropout off (eval mode, the net's own mode
        restored), its tape kept for input_backward.  For a caller whose cotangent is known only after this forward.
        tap=True (a net whose Function honours ctx.tap: the EDM U-Net): tape.bottleneck is the activation after middle_block
        (NHWC bf16), the tensor encoder_input_forward returns, from this same evaluation; F and every launch are unchanged."""
        tape = InputTape()
        if tap:
            tape.tap = True
        out = _eval_forward(fn, n_inputs, tape, net, x, t, cond)
        if tap and getattr(tape, "bottleneck", None) is None:
            raise NotImplementedError(f"input_forward(tap=True): {type(net).__name__} hands out no bottleneck")
        return out

    def input_backward(tape, v, d_tap=None):
        """The second half of input_vjp -> g = d(v . F)/dx for the tape of input_forward: the backward walk with its weight, bias
        and embedding launches switched off.  A tape is walked once; drop it afterwards.
        d_tap (a tape of input_forward(tap=True)): a second cotangent, of tape.bottleneck (NHWC bf16); it is added to the running
        gradient where the walk passes from the decoder into middle_block, so that g = d(v . F + d_tap . h)/dx comes out of one
        walk.  None: the walk of today, launch for launch."""
        if d_tap is not None:
            if not getattr(tape, "tap", False):
                raise ValueError("input_backward: d_tap needs the tape of input_forward(tap=True)")
            tape.d_tap = d_tap.contiguous()
        with torch.no_grad():
            return fn.backward(tape, v.contiguous().float())[1]

    def input_vjp(net, x, t, v, *cond):
        """The network output F at (x, t[, cond]) and g = d(v . F)/dx, the vector-Jacobian product of the network at v, with
        dropout off and no parameter gradient formed (the probability-flow likelihoods).  g is the dx the full backward of
        forward_with_grad returns, bit for bit.  The net's train / eval mode is left as it was."""
        out, tape = input_forward(net, x, t, *cond)
        return out, input_backward(tape, v)

    return train_forward, train_backward, input_forward, input_backward, input_vjp
