"""Autograd path of the ADM / EDM U-Net on the gfx950 kernels (policy step of DxMI on the EDM backbones:
models/DxMI/trainer.py:693-746 back-propagates the sampler loss through OpenAIDiffusion.sample_step into every
U-Net parameter; reference graph = torch autograd over models/cm/unet.py:761-790).

One torch.autograd.Function wraps the network.  forward() is the inference program of models/cm/unet.py (this
package) plus a tape of saved NHWC bf16 activations; backward() hands the tape to models/unet_bwd.py (the reverse walk with
its skip-connection rule, head, projection-shortcut data gradient, stem, parameter order) and adds what is this net's own:
  conv data gradients   = the forward MFMA kernels on transpose-flipped weight fragments (ResBlock(up) / Upsample:
                          full-resolution gradient then a 2x2 sum; stride-2 Downsample: zero-stuffed gradient);
  conv weight gradients = MFMA pixel-GEMM (ops.conv2d_wgrad), the bias gradient from the same launch;
  GroupNorm32 (+FiLM scale-shift, +SiLU) = ops.groupnorm_generic_bwd on the forward's saved statistics, which also returns
                          the per-image sums the scale / shift (= emb_layers output) gradients are formed from;
  attention             = ops.attention_bwd on the single qkv, any head count, with the forward's saved log-sum-exp;
  mean pool / nearest x2 = each other's transposes (unet_bwd.pool_t, unet_bwd.up_sum), in ResBlock(up / down) and in the
                          Upsample / Downsample without conv;
  time_embed, label_emb, emb_layers = dense backward on the HIP kernels (ops.linear_bwd, ops.silu_bwd), the pre-activations
                          recomputed, every emb_layers Linear as one concatenated operator.
Dropout (ResBlock out_layers: norm, SiLU, Dropout, conv; models/cm/unet.py) runs in train mode as the counter-hash kernel
dxmi_dropout_bf16 on the conv2 input: one seed per ResBlock per forward, kept on the tape with p, and the backward applies the same
(seed, p) to the gradient (no mask is stored).  With dropout 0, or in eval mode, nothing of it runs.  Inside a StepGraph capture
(dxmi_hip/graph.py) every site's seed is a host input of the graph, so a replayed step draws the seeds an eager step would draw.
Parameter gradients come back in net.parameters() order.  train_forward / train_backward / input_forward / input_backward /
input_vjp keep the tape outside autograd (input_forward(tap=True) also hands out the bottleneck, and input_backward(d_tap=...) takes
its cotangent in the same walk: SiDA's discriminator reads SiD's own evaluation of the fake net); encoder_forward / encoder_backward / encoder_input_forward / encoder_input_backward are
the same pass stopped at the bottleneck: the output of middle_block (NHWC bf16) and its cotangent take the place of the model
output, and no output_blocks / out launch is issued in either direction.
"""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from dxmi_hip import graph as _graph
from dxmi_hip import ops

from ..unet_bwd import Backward, encoder_api, pack_t, pool_t, tape_api, up_sum, walk


def _build_packs_t(net, ps):
    """Transpose-flipped fragments of every conv, and of the two dense operators the embedding backward differentiates through."""
    from .unet import AttentionBlock, Downsample, ResBlock, Upsample
    for m in net.modules():
        if isinstance(m, ResBlock):
            ps.pack((id(m), "conv1"), m.in_layers[2].weight, transpose_flip=True)
            ps.pack((id(m), "conv2"), m.out_layers[3].weight, transpose_flip=True)
        elif isinstance(m, AttentionBlock):
            C = m.channels
            ps.pack((id(m), "qkv"), m.qkv.weight.reshape(3 * C, C, 1, 1), transpose_flip=True)
            ps.pack((id(m), "proj"), m.proj_out.weight.reshape(C, C, 1, 1), transpose_flip=True)
        elif isinstance(m, Upsample) and m.use_conv:
            ps.pack((id(m), "conv"), m.conv.weight, transpose_flip=True)
        elif isinstance(m, Downsample) and m.use_conv:
            ps.pack((id(m), "conv"), m.op.weight, transpose_flip=True)
    w = net.out[2].weight
    ps.pack("conv_out", ps.stage((64,) + tuple(w.shape[1:]), lambda out: out[: w.shape[0]].copy_(w.detach()), zero=True), transpose_flip=True)
    ps.pack("emb_t", ps.stage_cat([m.emb_layers[1].weight for m in net.modules() if isinstance(m, ResBlock)]), transpose_flip=True)
    ps.pack("te2_t", net.time_embed[2].weight, transpose_flip=True)


def _pack_t(net):
    return pack_t(net, _build_packs_t)


# Training forward: GroupNorm on the producers' block statistics (streaming apply) where the inference path uses them; 0 = the generic
# statistics + apply pair everywhere (rounds 3-5).
STREAM_GN = os.environ.get("DXMI_TRAIN_STREAM_GN", "1") == "1"
# Training forward keeps the attention rows' log-sum-exp for the backward (dxmi_attention_fwd_lse / _bwd_lse); 0 = the backward recomputes it.
SAVE_LSE = os.environ.get("DXMI_ATTN_SAVE_LSE", "1") == "1"


def _next_dropout_seed(net):
    """32-bit seed of the next dropout site (ops.dropout_site_seed of the base seed and a running site counter).  The base is
    `net.dropout_seed` if set, else torch.initial_seed().  The counter lives on the net and is not part of a checkpoint: a run
    resumed with dropout > 0 draws the masks of a fresh net again, so it is not bit-exact with the run it continues."""
    feed = net.__dict__.get("_dropout_seed_feed")
    if feed is not None:    # seeds handed over by the caller (the target net of consistency_losses takes the online net's)
        if not feed:
            raise RuntimeError("dropout seed hand-over: the net has more dropout sites than seeds were handed to it")
        return feed.pop(0)
    base = torch.initial_seed() if getattr(net, "dropout_seed", None) is None else int(net.dropout_seed)
    n = net.__dict__.get("_dropout_calls", 0)
    net.__dict__["_dropout_calls"] = n + 1
    return ops.dropout_site_seed(base, n)


class _EDMUNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, x, timesteps, y, *params):
        from .unet import AttentionBlock, Downsample, ResBlock, Upsample
        p_drop = float(net.dropout) if net.training else 0.0
        cap = _graph.current() if p_drop > 0 else None
        net.dropout_seeds_used = []
        pk = net.packed()
        x = x.contiguous().float()
        sinus = ops.timestep_embedding(timesteps, net.model_channels, order=1)
        e0 = ops.linear(sinus, pk["te0"], net.time_embed[0].bias, post_act=ops.ACT_SILU)
        emb = ops.linear(e0, pk["te2"], net.time_embed[2].bias)
        if net.num_classes is not None:
            emb = emb + net.label_emb.weight[y]
        emb_all = ops.linear(emb, pk["emb_w"], pk["emb_b"], pre_act=ops.ACT_SILU)
        tape = []

        def conv_s(*a, **kw):
            """-> (out, BlockStats of out from the conv's epilogue | None)"""
            return ops.conv2d(*a, want_stats=True, **kw) if STREAM_GN else (ops.conv2d(*a, **kw), None)

        def gn_fwd(norm, xin, st=None, st1=None, **kw):
            """GroupNorm(+SiLU) + the statistics partials the backward reads (it then skips its own statistics pass over `xin`;
            autograd saves mean / rstd the same way).  With block statistics from the producer (st; round 6, as in
            forward_inference) the forward is the one-pass streaming apply and the partials are those sums converted
            (dxmi_gn_blockstats_to_generic); otherwise the generic statistics + apply pair, which leaves its partials."""
            sv = []
            out = ops.groupnorm_silu(xin, norm.weight, norm.bias, eps=norm.eps, saved=sv, stats=(st, st1), **kw)
            return out, (sv[0] if sv else None)

        def res(b, x0, x1, st0, st1):
            gn1, conv1, gn2, conv2 = b.in_layers[0], b.in_layers[2], b.out_layers[0], b.out_layers[3]
            a1, s1 = gn_fwd(gn1, x0, st0, st1, in1=x1, silu=True)
            a1p, xs = a1, x0
            if b.up:
                xs = ops.upsample2x(x0)
            elif b.down:
                a1p, xs = ops.pool_act(a1, True, ops.ACT_NONE), ops.pool_act(x0, True, ops.ACT_NONE)
            off, eo = pk[id(b), "eoff"], b.emb_layers[1].out_features
            e = emb_all[:, off:off + eo]
            if b.use_scale_shift_norm:
                h, sh = conv_s(a1p, pk[id(b), "conv1"], bias=conv1.bias, upsample=b.up)
                a2, s2 = gn_fwd(gn2, h, sh, silu=True, scale_shift=e)
            else:
                h, sh = conv_s(a1p, pk[id(b), "conv1"], bias=conv1.bias, upsample=b.up, addvec=e)
                a2, s2 = gn_fwd(gn2, h, sh, silu=True)
            drop = None
            if p_drop > 0:       # nn.Dropout of out_layers: the backward regenerates the mask from (seed, p)
                if cap is not None and net.__dict__.get("_dropout_seed_feed") is None:
                    # captured step: the seed is a host input of the graph (a device word, dxmi_dropout_bf16_dev), declared in site
                    # order; its producer advances the counter an eager forward advances
                    drop = (cap.host_input(torch.int32, 1, lambda: [_next_dropout_seed(net)]), p_drop)
                else:       # eager: a python int; seeds handed over by the caller are taken as they are (device words under capture)
                    drop = (_next_dropout_seed(net), p_drop)
                net.dropout_seeds_used.append(drop[0])
                a2 = ops.dropout(a2, p_drop, drop[0])
            if (id(b), "skip") in pk:
                xs = ops.conv2d(x0, pk[id(b), "skip"], in1=x1, bias=b.skip_connection.bias)
            out, so = conv_s(a2, pk[id(b), "conv2"], bias=conv2.bias, residual=xs)
            tape.append(("res", b, x0, x1, a1p, h, a2, s1, s2, drop))
            return out, (so if so is not None else stats_of(out))

        def attn(m, xa, sx):
            N, H, W, C = xa.shape
            hn, sn = gn_fwd(m.norm, xa, sx, silu=False)
            qkv = ops.conv2d(hn, pk[id(m), "qkv"], bias=m.qkv.bias)
            # the row log-sum-exp rides along (autograd's saved softmax statistics): the backward skips its own sweep for it
            a, lse = ops.attention(qkv.view(N, H * W, 3 * C), heads=m.num_heads, scale=1.0 / math.sqrt(C // m.num_heads), want_lse=True)
            lse = lse if SAVE_LSE else None
            out = ops.conv2d(a.view(N, H, W, C), pk[id(m), "proj"], bias=m.proj_out.bias, residual=xa)
            tape.append(("attn", m, xa, hn, qkv, a, sn, lse))
            return out, stats_of(out)

        def seq(mods, h, skip, sh, sskip):
            for m in mods:
                if isinstance(m, ResBlock):
                    h, sh = res(m, h, skip, sh, sskip)
                    skip = sskip = None
                elif isinstance(m, AttentionBlock):
                    h, sh = attn(m, h, sh)
                elif isinstance(m, Downsample):
                    tape.append(("down", m, h))
                    if m.use_conv:
                        h, sh = conv_s(h, pk[id(m), "conv"], bias=m.op.bias, stride=2, pad=1)
                    else:
                        h, sh = ops.pool_act(h, True, ops.ACT_NONE), None
                    sh = sh if sh is not None else stats_of(h)
                elif isinstance(m, Upsample):
                    tape.append(("up", m, h))
                    if m.use_conv:
                        h, sh = conv_s(h, pk[id(m), "conv"], bias=m.conv.bias, upsample=True)
                    else:
                        h, sh = ops.upsample2x(h), None
                    sh = sh if sh is not None else stats_of(h)
            return h, sh

        stats_of = net._stats_of if STREAM_GN else (lambda t: None)
        conv_in = net.input_blocks[0][0]
        h = ops.conv2d(x, pk["conv_in"], bias=conv_in.bias) if pk["conv_in"].k27 else \
            ops.conv2d(ops.nchw_f32_to_nhwc_bf16(x), pk["conv_in"], bias=conv_in.bias)
        sh = stats_of(h)
        hs = [(h, sh)]
        for i in range(1, len(net.input_blocks)):
            h, sh = seq(net.input_blocks[i], h, None, sh, None)
            tape.append(("push", None, len(hs)))
            hs.append((h, sh))
        h, sh = seq(net.middle_block, h, None, sh, None)
        ctx.net, ctx.tape, ctx.x, ctx.sinus, ctx.y, ctx.emb_all = net, tape, x, sinus, y, emb_all
        if getattr(ctx, "encoder_only", False):      # the pass that stops at the bottleneck (unet_bwd.encoder_api): NHWC bf16
            return h
        if getattr(ctx, "tap", False):               # input_forward(tap=True): the bottleneck is handed out, and the walk may take
            ctx.bottleneck = h                       # a cotangent for it where it passes this entry
            tape.append(("tap", None))
        for blk in net.output_blocks:
            tape.append(("skip", None, len(hs) - 1))
            skip, sskip = hs.pop()
            h, sh = seq(blk, h, skip, sh, sskip)
        gn = net.out[0]
        a_out, ctx.s_out = gn_fwd(gn, h, sh, silu=True)
        out = ops.conv2d(a_out, pk["conv_out"], bias=net.out[2].bias, out_nchw_f32=True)
        ctx.h_last, ctx.a_out = h, a_out
        return out

    @staticmethod
    def backward(ctx, d_out):
        from .unet import ResBlock
        net = ctx.net
        bw = Backward(ctx, _build_packs_t)
        pk, pkt, grads, params, conv_wb = bw.pk, bw.pkt, bw.grads, bw.params, bw.conv_wb
        emb_all = ctx.emb_all
        d_emb_all = torch.zeros(emb_all.shape, dtype=torch.float32, device=d_out.device) if params else None

        def gn_bwd(norm, xin, dy, *, in1=None, add0=None, add1=None, silu=True, scale_shift=None, fwd_stats=None):
            dx0, dx1, dg, db, d_ss = ops.groupnorm_generic_bwd(xin, dy, norm.weight, norm.bias, in1=in1, add0=add0, add1=add1,
                                                               eps=norm.eps, silu=silu, scale_shift=scale_shift, fwd_stats=fwd_stats)
            grads[norm.weight], grads[norm.bias] = dg, db
            return dx0, dx1, d_ss

        if getattr(ctx, "encoder_only", False):
            # the tape ends at the bottleneck and holds no "skip" entry: d_out is the gradient of middle_block's output, and the
            # rows of d_emb_all that belong to decoder blocks stay zero
            g = d_out
        else:
            # ---- head: out = conv(silu(gn(h_last)))
            g, _, _ = gn_bwd(net.out[0], ctx.h_last, bw.head(net.out[2], ctx.a_out, d_out), fwd_stats=ctx.s_out)

        def res_bwd(entry, g):
            _, b, x0, x1, a1p, h, a2, s1, s2, drop = entry
            gn1, conv1, gn2, conv2 = b.in_layers[0], b.in_layers[2], b.out_layers[0], b.out_layers[3]
            conv_wb(conv2, a2, g, 3)
            d_a2 = ops.conv2d(g, pkt[id(b), "conv2"])
            if drop is not None:
                d_a2 = ops.dropout(d_a2, drop[1], drop[0], out=d_a2)
            off, eo = pk[id(b), "eoff"], b.emb_layers[1].out_features
            if b.use_scale_shift_norm:
                d_h, _, d_ss = gn_bwd(gn2, h, d_a2, scale_shift=emb_all[:, off:off + eo], fwd_stats=s2)
                if params:
                    d_emb_all[:, off:off + eo] = d_ss
            else:
                d_h, _, _ = gn_bwd(gn2, h, d_a2, fwd_stats=s2)
                if params:
                    d_emb_all[:, off:off + eo] = ops.colsum_per_image(d_h)
            conv_wb(conv1, a1p, d_h, 3, upsample=b.up)
            d_a1 = ops.conv2d(d_h, pkt[id(b), "conv1"])
            if b.up:
                d_a1 = up_sum(d_a1)
            elif b.down:
                d_a1 = pool_t(d_a1)
            if (id(b), "skip") in pk:
                sk = b.skip_connection
                conv_wb(sk, x0, g, sk.weight.shape[-1], x1=x1)
                dxg0, dxg1, _ = gn_bwd(gn1, x0, d_a1, in1=x1, fwd_stats=s1)
                return bw.shortcut_dx((id(b), "skip_t"), sk.weight, x0, x1, g, dxg0, dxg1)
            assert x1 is None
            g_id = up_sum(g) if b.up else (pool_t(g) if b.down else g)
            d_x0, _, _ = gn_bwd(gn1, x0, d_a1, add0=g_id, fwd_stats=s1)
            return d_x0, None

        def attn_bwd(entry, g):
            _, m, xa, hn, qkv, a, sn, lse = entry
            Nn, Hh, Ww, C = xa.shape
            conv_wb(m.proj_out, a.view(Nn, Hh, Ww, C), g, 1)
            d_a = ops.conv2d(g, pkt[id(m), "proj"])
            d_qkv = ops.attention_bwd(qkv.view(Nn, Hh * Ww, 3 * C), d_a.view(Nn, Hh * Ww, C), m.num_heads,
                                      1.0 / math.sqrt(C // m.num_heads), o=a.view(Nn, Hh * Ww, C), lse=lse).view(Nn, Hh, Ww, 3 * C)
            conv_wb(m.qkv, hn, d_qkv, 1)
            d_hn = ops.conv2d(d_qkv, pkt[id(m), "qkv"])
            d_x, _, _ = gn_bwd(m.norm, xa, d_hn, add0=g, silu=False, fwd_stats=sn)
            return d_x

        def up_bwd(entry, g):
            _, m, xin = entry
            if not m.use_conv:
                return up_sum(g)
            conv_wb(m.conv, xin, g, 3, upsample=True)
            return up_sum(ops.conv2d(g, pkt[id(m), "conv"]))

        def down_bwd(entry, g):
            _, m, xin = entry
            if not m.use_conv:
                return pool_t(g)
            conv_wb(m.op, xin, g, 3, stride=2, pad=1)
            return ops.conv2d(g, pkt[id(m), "conv"], pad=1, pad_br=1, upsample=2)

        g = walk(ctx.tape, g, res_bwd, attn_bwd, up_bwd, down_bwd, d_tap=getattr(ctx, "d_tap", None))
        dx = bw.stem(net.input_blocks[0][0], ctx.x, g, ctx.needs_input_grad[1])
        if not params:
            return bw.finish(4, dx)

        # ---- embedding graph (models/cm/unet.py:775-779, :249): time_embed MLP, label embedding, every emb_layers Linear as one
        # operator — dense backward on the HIP kernels (ops.linear_bwd), pre-activations recomputed
        blocks = [m for m in net.modules() if isinstance(m, ResBlock)]
        l0, l2 = net.time_embed[0], net.time_embed[2]
        e0 = ops.linear(ctx.sinus, pk["te0"], l0.bias)
        a0 = F.silu(e0)
        emb = ops.linear(a0, pk["te2"], l2.bias)
        if net.num_classes is not None:
            emb = emb + net.label_emb.weight.detach()[ctx.y]
        s_e = F.silu(emb)
        ds, dw_cat, db_cat = ops.linear_bwd(s_e, d_emb_all, pkt["emb_t"])
        bw.dense_rows([b.emb_layers[1] for b in blocks], dw_cat, db_cat)
        d_emb = ops.silu_bwd(emb, ds)
        if net.num_classes is not None:
            grads[net.label_emb.weight] = torch.zeros_like(net.label_emb.weight).index_add_(0, ctx.y, d_emb)
        da0, grads[l2.weight], grads[l2.bias] = ops.linear_bwd(a0, d_emb, pkt["te2_t"])
        de0 = ops.silu_bwd(e0, da0)
        _, grads[l0.weight], grads[l0.bias] = ops.linear_bwd(ctx.sinus, de0, None, need_dx=False)
        return bw.finish(4, dx)


def forward_with_grad(net, x, timesteps, y=None):
    return _EDMUNetFn.apply(net, x, timesteps, y, *ops.fast_parameters(net))


# the tape outside autograd (models.unet_bwd.tape_api): the loss nodes of models.cm.karras_diffusion, score identity distillation's
# input_forward / input_backward on both denoisers and the likelihood's input_vjp
train_forward, train_backward, input_forward, input_backward, input_vjp = tape_api(_EDMUNetFn, 4)
# the same, stopped at the bottleneck: the classifier head of models.cm.gan_head reads the fake denoiser's middle_block output
encoder_forward, encoder_backward, encoder_input_forward, encoder_input_backward = encoder_api(_EDMUNetFn, 4)
