"""Autograd path of the DDPM U-Net on the gfx950 kernels (policy step of DxMI:
models/DxMI/trainer.py:361-389 back-propagates the sampler loss through `sample_step` into every
U-Net parameter; reference graph = torch autograd over models/DxMI/unet_small.py:292-332).

One torch.autograd.Function wraps the network.  forward() is the inference program plus saved bf16
NHWC activations (and one dropout seed per ResnetBlock in train mode) on a tape; backward() hands the
tape to models/unet_bwd.py (the reverse walk with its skip-connection rule, head, projection-shortcut
data gradient, stem, parameter order) and adds what is this net's own:
  conv data gradients   = the forward MFMA kernels on transpose-flipped weight fragments (stride-2:
                          over the zero-stuffed gradient; upsample: full-res gradient then 2x2 sum),
                          with the shortcut gradient fused as the epilogue residual;
  conv weight gradients = MFMA pixel-GEMM (ops.conv2d_wgrad, also strided / upsampled / 1x1);
  GroupNorm(+SiLU)      = ops.groupnorm_silu_bwd (dx split back into the two concat sources);
  attention             = ops.attention_bwd on the stacked qkv, one head; q / k / v are three convs,
                          so their weight and bias gradients are row blocks of one wgrad_branch launch;
  dropout               = ops.dropout with the forward's seed (no stored mask);
  temb MLP + temb_proj  = dense backward on the HIP kernels (ops.linear_bwd, ops.silu_bwd), the
                          pre-activations recomputed, every temb_proj as one concatenated operator.
Parameter gradients are returned in `net.parameters()` order as fp32 tensors.  train_forward /
train_backward / input_forward / input_backward / input_vjp keep the tape outside autograd.
"""
import torch
import torch.nn.functional as F

from dxmi_hip import graph as _graph
from dxmi_hip import ops

from ..unet_bwd import Backward, pack_t, tape_api, up_sum, walk


def _build_packs_t(net, ps):
    """Transpose-flipped fragments of every conv."""
    from .unet_small import AttnBlock, Downsample, Upsample
    for b in net._resblocks():
        ps.pack((id(b), "conv1"), b.conv1.weight, transpose_flip=True)
        ps.pack((id(b), "conv2"), b.conv2.weight, transpose_flip=True)
        if b.in_channels != b.out_channels:
            sc = b.conv_shortcut if b.use_conv_shortcut else b.nin_shortcut
            ps.entries[id(b), "short"] = sc.weight  # split per concat source at use time
    for m in net.modules():
        if isinstance(m, AttnBlock):
            ps.pack((id(m), "qkv"), ps.stage_cat([m.q.weight, m.k.weight, m.v.weight]), transpose_flip=True)
            ps.pack((id(m), "proj"), m.proj_out.weight, transpose_flip=True)
        elif isinstance(m, (Upsample, Downsample)):
            ps.pack((id(m), "conv"), m.conv.weight, transpose_flip=True)
    w = net.conv_out.weight
    ps.pack("conv_out", ps.stage((64,) + tuple(w.shape[1:]), lambda out: out[: w.shape[0]].copy_(w.detach()), zero=True), transpose_flip=True)


def _pack_t(net):
    return pack_t(net, _build_packs_t)


class _UNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, x, t, *params):
        pk = net.packed()
        x = x.contiguous().float()
        training, p_drop = net.training, net.dropout_p
        net.dropout_seeds_used = []
        emb = ops.timestep_embedding(t, net.ch, order=0)
        h1 = ops.linear(emb, pk["dense0"], net.temb.dense[0].bias, post_act=ops.ACT_SILU)
        s_temb = ops.linear(h1, pk["dense1"], net.temb.dense[1].bias, post_act=ops.ACT_SILU)
        tp = ops.linear(s_temb, pk["tproj"], pk["tproj_bias"])
        tape = []  # (kind, module, saved...)

        def res(b, x0, x1):
            a1 = ops.groupnorm_silu(x0, b.norm1.weight, b.norm1.bias, in1=x1, eps=1e-6, silu=True)
            off = pk[id(b), "toff"]
            h = ops.conv2d(a1, pk[id(b), "conv1"], bias=b.conv1.bias, addvec=tp[:, off:off + b.out_channels])
            a2 = ops.groupnorm_silu(h, b.norm2.weight, b.norm2.bias, eps=1e-6, silu=True)
            mask = None
            if training and p_drop > 0:
                # nn.Dropout (unet_small.py:129) as a counter-hash kernel: the backward regenerates the mask from the seed
                cap = _graph.current()
                if cap is None:
                    mask = net._next_dropout_seed()
                else:       # captured step: the seed is a host input of the graph, drawn per replay from the same counter hash
                    mask = cap.host_input(torch.int32, 1, lambda: [net._next_dropout_seed()])
                a2 = ops.dropout(a2, p_drop, mask)
            if b.in_channels != b.out_channels:
                sc_mod = b.conv_shortcut if b.use_conv_shortcut else b.nin_shortcut
                sc = ops.conv2d(x0, pk[id(b), "short"], in1=x1, bias=sc_mod.bias)
            else:
                sc = x0
            out = ops.conv2d(a2, pk[id(b), "conv2"], bias=b.conv2.bias, residual=sc)
            tape.append(("res", b, x0, x1, a1, h, a2, mask))
            return out

        def attn(m, xa):
            N, H, W, C = xa.shape
            hn = ops.groupnorm_silu(xa, m.norm.weight, m.norm.bias, eps=1e-6, silu=False)
            qkv = ops.conv2d(hn, pk[id(m), "qkv"], bias=pk[id(m), "qkv_bias"])
            a = ops.attention(qkv.view(N, H * W, 3 * C), heads=1, scale=float(int(C) ** (-0.5)))
            out = ops.conv2d(a.view(N, H, W, C), pk[id(m), "proj"], bias=m.proj_out.bias, residual=xa)
            tape.append(("attn", m, xa, hn, qkv, a))
            return out

        h = ops.conv2d(x, pk["conv_in"], bias=net.conv_in.bias) if pk["conv_in"].k27 else \
            ops.conv2d(ops.nchw_f32_to_nhwc_bf16(x), pk["conv_in"], bias=net.conv_in.bias)
        hs = [h]
        for i_level, lvl in enumerate(net.down):
            for i_block, blk in enumerate(lvl.block):
                h = res(blk, hs[-1], None)
                if len(lvl.attn) > 0:
                    h = attn(lvl.attn[i_block], h)
                tape.append(("push", None, len(hs)))
                hs.append(h)
            if i_level != net.num_resolutions - 1:
                ds = lvl.downsample
                hd = ops.conv2d(hs[-1], pk[id(ds), "conv"], bias=ds.conv.bias, stride=2, pad=0, pad_br=1)
                tape.append(("down", ds, hs[-1]))
                tape.append(("push", None, len(hs)))
                hs.append(hd)
        h = hs[-1]
        h = res(net.mid.block_1, h, None)
        h = attn(net.mid.attn_1, h)
        h = res(net.mid.block_2, h, None)
        for i_level in reversed(range(net.num_resolutions)):
            lvl = net.up[i_level]
            for i_block, blk in enumerate(lvl.block):
                skip_idx = len(hs) - 1
                skip = hs.pop()
                tape.append(("skip", None, skip_idx))
                h = res(blk, h, skip)
                if len(lvl.attn) > 0:
                    h = attn(lvl.attn[i_block], h)
            if i_level != 0:
                us = lvl.upsample
                tape.append(("up", us, h))
                h = ops.conv2d(h, pk[id(us), "conv"], bias=us.conv.bias, upsample=True)
        a_out = ops.groupnorm_silu(h, net.norm_out.weight, net.norm_out.bias, eps=1e-6, silu=True)
        eps = ops.conv2d(a_out, pk["conv_out"], bias=net.conv_out.bias, out_nchw_f32=True)
        ctx.net, ctx.tape, ctx.h_last, ctx.a_out, ctx.x, ctx.emb = net, tape, h, a_out, x, emb
        return eps

    @staticmethod
    def backward(ctx, d_eps):
        net = ctx.net
        bw = Backward(ctx, _build_packs_t)
        pk, pkt, grads, params, conv_wb = bw.pk, bw.pkt, bw.grads, bw.params, bw.conv_wb
        d_tp = torch.zeros((d_eps.shape[0], pk["tproj_bias"].numel()), dtype=torch.float32, device=d_eps.device) if params else None

        def gn_bwd(norm, xin, dy, **kw):
            dx0, dx1, grads[norm.weight], grads[norm.bias] = ops.groupnorm_silu_bwd(xin, dy, norm.weight, norm.bias, **kw)
            return dx0, dx1

        # ---- head: eps = conv_out(silu(gn(h_last)))
        g, _ = gn_bwd(net.norm_out, ctx.h_last, bw.head(net.conv_out, ctx.a_out, d_eps), silu=True)

        def res_bwd(entry, g):
            _, b, x0, x1, a1, h, a2, mask = entry
            conv_wb(b.conv2, a2, g, 3)
            d_a2 = ops.conv2d(g, pkt[id(b), "conv2"])
            if mask is not None:
                d_a2 = ops.dropout(d_a2, net.dropout_p, mask, out=d_a2)
            d_h, _ = gn_bwd(b.norm2, h, d_a2, silu=True)
            off = pk[id(b), "toff"]
            if params:
                d_tp[:, off:off + b.out_channels] = ops.colsum_per_image(d_h)
            conv_wb(b.conv1, a1, d_h, 3)
            d_a1 = ops.conv2d(d_h, pkt[id(b), "conv1"])
            if b.in_channels != b.out_channels:
                sc_mod = b.conv_shortcut if b.use_conv_shortcut else b.nin_shortcut
                conv_wb(sc_mod, x0, g, sc_mod.weight.shape[-1], x1=x1)
                dxg0, dxg1 = gn_bwd(b.norm1, x0, d_a1, in1=x1, silu=True)
                return bw.shortcut_dx((id(b), "short_t"), pkt[id(b), "short"], x0, x1, g, dxg0, dxg1)
            assert x1 is None
            return gn_bwd(b.norm1, x0, d_a1, add0=g, silu=True)

        def attn_bwd(entry, g):
            _, m, xa, hn, qkv, a = entry
            Nn, Hh, Ww, C = xa.shape
            conv_wb(m.proj_out, a.view(Nn, Hh, Ww, C), g, 1)
            d_a = ops.conv2d(g, pkt[id(m), "proj"])
            d_qkv = ops.attention_bwd(qkv.view(Nn, Hh * Ww, 3 * C), d_a.view(Nn, Hh * Ww, C), 1, float(int(C) ** (-0.5)))
            d_qkv = d_qkv.view(Nn, Hh, Ww, 3 * C)
            if params:
                with ops.wgrad_branch((hn, d_qkv)):
                    wq, bq = ops._conv2d_wgrad(hn, d_qkv, 1, with_bias=True)   # the bias gradient from the dY tiles the kernel stages anyway
                    for j, conv in enumerate((m.q, m.k, m.v)):
                        grads[conv.weight] = wq[j * C:(j + 1) * C].contiguous()
                        grads[conv.bias] = bq[j * C:(j + 1) * C].contiguous()
            d_hn = ops.conv2d(d_qkv, pkt[id(m), "qkv"])
            return gn_bwd(m.norm, xa, d_hn, add0=g, silu=False)[0]

        def up_bwd(entry, g):
            _, us, xin = entry
            conv_wb(us.conv, xin, g, 3, upsample=True)
            return up_sum(ops.conv2d(g, pkt[id(us), "conv"]))

        def down_bwd(entry, g):
            _, ds, xin = entry
            conv_wb(ds.conv, xin, g, 3, stride=2, pad=0)
            return ops.conv2d(g, pkt[id(ds), "conv"], pad=2, pad_br=0, upsample=2)

        dx = bw.stem(net.conv_in, ctx.x, walk(ctx.tape, g, res_bwd, attn_bwd, up_bwd, down_bwd), ctx.needs_input_grad[1])
        if params:
            # ---- temb MLP + all temb_proj layers (reference unet_small.py:296-299, :123): dense backward on the HIP kernels
            # (ops.linear_bwd: transposed-pack linear for dx, the 1x1 weight-gradient kernel for dW), pre-activations recomputed
            blocks = list(net._resblocks())
            d0, d1 = net.temb.dense
            e0 = ops.linear(ctx.emb, pk["dense0"], d0.bias)                        # pre-activation of dense[0]
            a0 = F.silu(e0)
            e1 = ops.linear(a0, pk["dense1"], d1.bias)
            s_t = F.silu(e1)
            tproj_t = net._packs_t.on_demand("tproj_t", lambda: ops.pack_conv_weight(torch.cat([b.temb_proj.weight for b in blocks], 0),
                                                                                     transpose_flip=True))
            dense1_t = net._packs_t.on_demand("dense1_t", lambda: ops.pack_conv_weight(d1.weight, transpose_flip=True))
            ds, dw_cat, db_cat = ops.linear_bwd(s_t, d_tp, tproj_t)
            bw.dense_rows([b.temb_proj for b in blocks], dw_cat, db_cat)
            de1 = ops.silu_bwd(e1, ds)
            da0, grads[d1.weight], grads[d1.bias] = ops.linear_bwd(a0, de1, dense1_t)
            de0 = ops.silu_bwd(e0, da0)
            _, grads[d0.weight], grads[d0.bias] = ops.linear_bwd(ctx.emb, de0, None, need_dx=False)
        return bw.finish(3, dx)


def forward_with_grad(net, x, t):
    return _UNetFn.apply(net, x, t, *ops.fast_parameters(net))


# the tape outside autograd (models.unet_bwd.tape_api): the loss node of models/DxMI/ddpm_train.py and the likelihood's input_vjp
train_forward, train_backward, input_forward, input_backward, input_vjp = tape_api(_UNetFn, 3)
