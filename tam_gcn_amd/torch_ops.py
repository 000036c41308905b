"""``torch.library`` registration of the hot-path ops whose interface is pure tensors (BASELINE.json north_star: "Python host
on PyTorch-ROCm registering custom ops through a thin C-ABI").  Each ``tamgcn::*`` op is a ``torch.library.custom_op`` whose
implementation launches the C ABI (through ``tam_gcn_amd.ops``), with a fake (meta) implementation so that export /
``torch.compile`` trace through it without a graph break, and -- for the differentiable ones -- ``register_autograd`` whose
backward is itself a registered op:

    tamgcn::ctrgc(x, A, alpha, w1, b1, w2, b2, w3, b3, w4, b4) -> y          reference models/ctrgcn.py:172-177
    tamgcn::ctrgc_backward(dy, x, A, alpha, w1, ..., b4) -> 11 gradients
    tamgcn::cross_entropy(logits, labels) -> (loss, g);  tamgcn::cross_entropy_backward(g, dloss) -> dlogits
    tamgcn::cross_entropy_opts(logits, target, weight | None, ignore_index, label_smoothing, reduction) -> (loss, g);
    tamgcn::cross_entropy_opts_backward(g, dloss, reduction) -> dlogits       torch.nn.CrossEntropyLoss's options
    tamgcn::pointwise_conv(x, w, b) -> y;  tamgcn::pointwise_conv_backward(dy, x, w) -> (dx, dw, db)
    tamgcn::head(x, W, b, M) -> logits;  tamgcn::head_backward(dlogits, x, W, M) -> (dx, dW, db)        models/ctrgcn.py:343-348
    tamgcn::head_pooled(x, rowmean, W, b, M): the same with the row means of x already taken by the producer of x
    tamgcn::dropout(x, state, site, p) -> (out, bits);  tamgcn::dropout_backward(dout, bits, p) -> dx      the device mask of dropout.py
    tamgcn::stream_derive(x, parent, mode) -> stream            feeder/feeder_nucla_gcn.py:119-127
    tamgcn::feeder_transform(raw, offsets, rot, idx, parent, V, time_steps, center_joint, mode) -> clips   :85-130
    tamgcn::guidance_reduce(h, M) -> (intensity, pooled, minmax);  tamgcn::guidance_weights(intensity, minmax, joints, k) -> weights;
    tamgcn::guidance_apply(weights, rgb | None, frames, H, W, want_map) -> (rgb * map, map)                 visual.py:53-87
    tamgcn::xmodal_head(f, f_rgb, W1, b1, bn_w, bn_b, running_mean, running_var, num_batches_tracked, W2, b2, Wc, bc, training,
                        momentum, eps) -> (logits, saved...);  tamgcn::xmodal_head_backward(...) -> 10 gradients
                                                 the cross-modal attention head, models/resnet_gcn_attention.py:60-70, :89-120; it updates the
                                                 BatchNorm buffers in place, so its autograd node is XModalHeadFn (below)

    tamgcn::tcn_gcn_unit_eval(x, xpart, params, geom) -> (out, xpart)   the whole eval-mode TCN_GCN_unit (:266-284) for small
                                                 batches, BatchNorm folded; registered by tam_gcn_amd/f2.py with the engine that uses it
    tamgcn::tcn_gcn_unit_eval_v25(x, xpart, params, geom) -> (out, xpart)   the same for 25 joints (tam_gcn_amd/f2v.py); xpart there
                                                 has frames of 28 floats
    tamgcn::tcn_gcn_unit_eval_vj(x, xpart, params, geom) -> (out, xpart)    the same for any joint count of f2v.JOINTS (17, 18, 25);
                                                 xpart has frames of (V + 3) & ~3 floats.  (_grouped twins of all three: f2.py, f2v.py)
    tamgcn::st_gcn_eval(x, params, geom) -> out  the whole eval-mode st_gcn block of ST-GCN (models/stgcn.py:67-99) for small
                                                 batches, both BatchNorms folded, two launches; registered by tam_gcn_amd/f2s.py

The TRAINING block-level nodes (unit_gcn / MultiScale_TemporalConv / TCN_GCN_unit / st_gcn) stay ``autograd.Function``s: they update
BatchNorm running statistics in place, keep ~20 intermediate tensors between forward and backward and take their
configuration from the nn.Module; the modules ``CTRGC``, ``CrossEntropyLoss``, the ST-GCN per-position classifier and the
model heads call the registered ops."""
from typing import Optional

import torch
from torch import Tensor

from . import ops
from .ops import S


def _c(t):
    return t.contiguous()


# ---------------------------------------------------------------------------------------------------------------
# CTRGC (single subset; A and alpha are inputs)
# ---------------------------------------------------------------------------------------------------------------
def _ctrgc_pack(x, A, alpha, w1, b1, w2, b2, w3, b3, w4, b4):
    N, Cin, T, V = x.shape
    Cout, R = w3.shape[0], w1.shape[0]
    W12 = torch.cat((w1.reshape(R, Cin), w2.reshape(R, Cin)))
    B12 = torch.cat((b1, b2))
    W3, W4 = w3.reshape(Cout, Cin).contiguous(), w4.reshape(1, Cout, R).contiguous()
    A3 = A.reshape(1, V, V).contiguous()
    al = alpha.reshape(1).to(torch.float32).contiguous()
    xs = S(x)
    xbar = ops.tmean(xs, Cin)
    pq, _ = ops.conv(S(xbar.view(1, Cin, N, V)), K=Cin, w=W12, bias=B12, M=2 * R)
    return dict(N=N, Cin=Cin, T=T, V=V, Cout=Cout, R=R, W12=W12, W3=W3, W4=W4, A3=A3, al=al, xs=xs, xbar=xbar,
                pq=pq.view(2 * R, N, V), b3=_c(b3), b4=b4.reshape(1, Cout).contiguous())


@torch.library.custom_op('tamgcn::ctrgc', mutates_args=())
def ctrgc(x: Tensor, A: Tensor, alpha: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, w3: Tensor, b3: Tensor,
          w4: Tensor, b4: Tensor) -> Tensor:
    p = _ctrgc_pack(_c(x), A, alpha, w1, b1, w2, b2, w3, b3, w4, b4)
    y, _, _ = ops.ctrgc_fwd(p['xs'], p['pq'], p['W3'], p['b3'], p['W4'], p['b4'], p['A3'], p['al'], p['Cin'], p['Cout'], 1, p['R'],
                            stats=False)
    return y


@ctrgc.register_fake
def _(x, A, alpha, w1, b1, w2, b2, w3, b3, w4, b4):
    return x.new_empty(x.shape[0], w3.shape[0], x.shape[2], x.shape[3])


@torch.library.custom_op('tamgcn::ctrgc_backward', mutates_args=())
def ctrgc_backward(dy: Tensor, x: Tensor, A: Tensor, alpha: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, w3: Tensor,
                   b3: Tensor, w4: Tensor, b4: Tensor) -> list[Tensor]:
    x = _c(x)
    p = _ctrgc_pack(x, A, alpha, w1, b1, w2, b2, w3, b3, w4, b4)       # x-bar and p, q are recomputed: a mean and a tiny GEMM
    N, Cin, T, V, Cout, R = p['N'], p['Cin'], p['T'], p['V'], p['Cout'], p['R']
    xs = p['xs']
    dx3, db3, dA, dW4, db4, dal, dpq = ops.ctrgc_bwd(xs, p['pq'], p['W3'], p['b3'], p['W4'], p['b4'], p['A3'], p['al'], Cin, Cout, 1, R,
                                                     S(_c(dy)))
    dpq4 = S(dpq.view(1, 2 * R, N, V))
    dW12 = ops.wgrad(dpq4, S(p['xbar'].view(1, Cin, N, V)), M=2 * R, K=Cin)
    dB12 = dpq.sum((1, 2))
    dW3 = ops.wgrad(S(dx3), xs, M=Cout, K=Cin)
    dxbar, _ = ops.conv(dpq4, K=2 * R, w=p['W12'], bias=None, M=Cin, wmode=1)
    dx, _ = ops.conv(S(dx3), K=Cout, w=p['W3'], bias=None, M=Cin, wmode=1, bcast=dxbar.view(Cin, N, V), bcast_scale=1.0 / T)
    return [dx, dA.reshape(A.shape), dal.reshape(alpha.shape).to(alpha.dtype), dW12[:R].reshape(w1.shape).clone(), dB12[:R].clone(),
            dW12[R:].reshape(w2.shape).clone(), dB12[R:].clone(), dW3.reshape(w3.shape), db3, dW4.reshape(w4.shape), db4.reshape(b4.shape)]


@ctrgc_backward.register_fake
def _(dy, x, A, alpha, w1, b1, w2, b2, w3, b3, w4, b4):
    return [torch.empty_like(t) for t in (x, A, alpha, w1, b1, w2, b2, w3, b3, w4, b4)]


def _ctrgc_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _ctrgc_bwd(ctx, dy):
    return tuple(torch.ops.tamgcn.ctrgc_backward(dy, *ctx.saved_tensors))


ctrgc.register_autograd(_ctrgc_bwd, setup_context=_ctrgc_setup)


# ---------------------------------------------------------------------------------------------------------------
# cross-entropy (mean reduction)
# ---------------------------------------------------------------------------------------------------------------
@torch.library.custom_op('tamgcn::cross_entropy', mutates_args=())
def cross_entropy(logits: Tensor, labels: Tensor) -> tuple[Tensor, Tensor]:
    return ops.ce_fwd(_c(logits), _c(labels))


@cross_entropy.register_fake
def _(logits, labels):
    return logits.new_empty(()), torch.empty_like(logits)


@torch.library.custom_op('tamgcn::cross_entropy_backward', mutates_args=())
def cross_entropy_backward(g: Tensor, dloss: Tensor) -> Tensor:
    return ops.ce_bwd(_c(g), dloss.to(torch.float32).contiguous())


@cross_entropy_backward.register_fake
def _(g, dloss):
    return torch.empty_like(g)


def _ce_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])


def _ce_bwd(ctx, dloss, dg):
    (g,) = ctx.saved_tensors
    return torch.ops.tamgcn.cross_entropy_backward(g, dloss), None


cross_entropy.register_autograd(_ce_bwd, setup_context=_ce_setup)


# ---------------------------------------------------------------------------------------------------------------
# cross-entropy with torch's options: class weights, ignore_index, label smoothing, the three reductions; target = class
# indices (N,) int64 or class probabilities (N, K) fp32.  g is the final gradient for dloss = 1.
# ---------------------------------------------------------------------------------------------------------------
@torch.library.custom_op('tamgcn::cross_entropy_opts', mutates_args=())
def cross_entropy_opts(logits: Tensor, target: Tensor, weight: Optional[Tensor], ignore_index: int, label_smoothing: float,
                       reduction: str) -> tuple[Tensor, Tensor]:
    return ops.ce_opts_fwd(_c(logits), _c(target), None if weight is None else _c(weight), ignore_index, label_smoothing, reduction)


@cross_entropy_opts.register_fake
def _(logits, target, weight, ignore_index, label_smoothing, reduction):
    return logits.new_empty((logits.shape[0],) if reduction == 'none' else ()), torch.empty_like(logits)


@torch.library.custom_op('tamgcn::cross_entropy_opts_backward', mutates_args=())
def cross_entropy_opts_backward(g: Tensor, dloss: Tensor, reduction: str) -> Tensor:
    dloss = dloss.to(torch.float32).contiguous()
    return ops.ce_opts_bwd_rows(_c(g), dloss) if reduction == 'none' else ops.ce_bwd(_c(g), dloss)


@cross_entropy_opts_backward.register_fake
def _(g, dloss, reduction):
    return torch.empty_like(g)


def _ce_opts_setup(ctx, inputs, output):
    ctx.reduction = inputs[5]
    ctx.save_for_backward(output[1])


def _ce_opts_bwd(ctx, dloss, dg):
    (g,) = ctx.saved_tensors
    return torch.ops.tamgcn.cross_entropy_opts_backward(g, dloss, ctx.reduction), None, None, None, None, None


cross_entropy_opts.register_autograd(_ce_opts_bwd, setup_context=_ce_opts_setup)


# ---------------------------------------------------------------------------------------------------------------
# 1x1 convolution with bias over (N, C, T, V)
# ---------------------------------------------------------------------------------------------------------------
@torch.library.custom_op('tamgcn::pointwise_conv', mutates_args=())
def pointwise_conv(x: Tensor, w: Tensor, b: Tensor) -> Tensor:
    x = _c(x)
    y, _ = ops.conv(S(x), K=x.shape[1], w=w.reshape(w.shape[0], -1).contiguous(), bias=_c(b), M=w.shape[0])
    return y


@pointwise_conv.register_fake
def _(x, w, b):
    return x.new_empty(x.shape[0], w.shape[0], x.shape[2], x.shape[3])


@torch.library.custom_op('tamgcn::pointwise_conv_backward', mutates_args=())
def pointwise_conv_backward(dy: Tensor, x: Tensor, w: Tensor) -> tuple[Tensor, Tensor, Tensor]:
    dy, x = _c(dy), _c(x)
    M, K = w.shape[0], x.shape[1]
    dw = ops.wgrad(S(dy), S(x), M=M, K=K).reshape(w.shape)
    db = dy.sum((0, 2, 3))
    dx, _ = ops.conv(S(dy), K=M, w=w.reshape(M, K).contiguous(), bias=None, M=K, wmode=1)
    return dx, dw, db


@pointwise_conv_backward.register_fake
def _(dy, x, w):
    return torch.empty_like(x), torch.empty_like(w), x.new_empty(w.shape[0])


def _pc_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])


def _pc_bwd(ctx, dy):
    x, w = ctx.saved_tensors
    return torch.ops.tamgcn.pointwise_conv_backward(dy, x, w)


pointwise_conv.register_autograd(_pc_bwd, setup_context=_pc_setup)


# ---------------------------------------------------------------------------------------------------------------
# head: mean over (m, t, v) then the classifier
# ---------------------------------------------------------------------------------------------------------------
@torch.library.custom_op('tamgcn::head', mutates_args=())
def head(x: Tensor, W: Tensor, b: Tensor, M: int) -> Tensor:
    pooled = ops.head_pool_fwd(_c(x), M)
    return ops.head_fc_fwd(pooled, _c(W), _c(b))


@head.register_fake
def _(x, W, b, M):
    return x.new_empty(x.shape[0] // M, W.shape[0])


@torch.library.custom_op('tamgcn::head_backward', mutates_args=())
def head_backward(dlogits: Tensor, x: Tensor, W: Tensor, M: int) -> tuple[Tensor, Tensor, Tensor]:
    x = _c(x)
    pooled = ops.head_pool_fwd(x, M)                                     # recomputed: one pass over the last block's output
    dW, db, dpooled = ops.head_fc_bwd(_c(dlogits), pooled, _c(W))
    return ops.head_pool_bwd(dpooled, M, x.shape[2], x.shape[3]), dW, db


@head_backward.register_fake
def _(dlogits, x, W, M):
    return torch.empty_like(x), torch.empty_like(W), x.new_empty(W.shape[0])


def _head_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.M = inputs[3]


def _head_bwd(ctx, dl):
    x, W = ctx.saved_tensors
    dx, dW, db = torch.ops.tamgcn.head_backward(dl, x, W, ctx.M)
    return dx, dW, db, None


head.register_autograd(_head_bwd, setup_context=_head_setup)


# the same head when the last block already produced the (N*M, C) row means of x in its final pass: x is an argument only
# for its gradient (the broadcast of d pooled), it is not read
def _pooled_of(rowmean, M):
    rowmean = _c(rowmean)
    if M == 1:                                           # one body per clip: the row means are the pooled features
        return rowmean
    NM, Cc = rowmean.shape
    return ops.head_pool_fwd(rowmean.view(NM, Cc, 1, 1), M)


@torch.library.custom_op('tamgcn::head_pooled', mutates_args=())
def head_pooled(x: Tensor, rowmean: Tensor, W: Tensor, b: Tensor, M: int) -> Tensor:
    return ops.head_fc_fwd(_pooled_of(rowmean, M), _c(W), _c(b))


@head_pooled.register_fake
def _(x, rowmean, W, b, M):
    return x.new_empty(x.shape[0] // M, W.shape[0])


@torch.library.custom_op('tamgcn::head_pooled_backward', mutates_args=())
def head_pooled_backward(dlogits: Tensor, rowmean: Tensor, W: Tensor, M: int, T: int, V: int) -> tuple[Tensor, Tensor, Tensor]:
    dW, db, dpooled = ops.head_fc_bwd(_c(dlogits), _pooled_of(rowmean, M), _c(W))
    return ops.head_pool_bwd(dpooled, M, T, V), dW, db


@head_pooled_backward.register_fake
def _(dlogits, rowmean, W, M, T, V):
    return rowmean.new_empty(rowmean.shape[0], rowmean.shape[1], T, V), torch.empty_like(W), rowmean.new_empty(W.shape[0])


def _headp_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[1], inputs[2])
    ctx.M, ctx.T, ctx.V = inputs[4], inputs[0].shape[2], inputs[0].shape[3]


def _headp_bwd(ctx, dl):
    rm, W = ctx.saved_tensors
    dx, dW, db = torch.ops.tamgcn.head_pooled_backward(dl, rm, W, ctx.M, ctx.T, ctx.V)
    return dx, None, dW, db, None


head_pooled.register_autograd(_headp_bwd, setup_context=_headp_setup)


# ---------------------------------------------------------------------------------------------------------------
# device dropout (the model heads; the st_gcn blocks carry theirs inside functional.StGcnFn)
# ---------------------------------------------------------------------------------------------------------------
def _rows4(x):
    """x as the (N, C, T, V) the row kernels walk: a 4-D tensor as it is, anything else as (shape[0], 1, 1, rest)."""
    x = _c(x)
    return x if x.dim() == 4 else x.view(x.shape[0], 1, 1, -1)


@torch.library.custom_op('tamgcn::dropout', mutates_args=())
def dropout(x: Tensor, state: Tensor, site: int, p: float) -> tuple[Tensor, Tensor]:
    x4 = _rows4(x)
    out, bits = ops.drop_add_act_fwd(S(x4), None, False, x4.shape[1], state, site, p)
    return out.view(x.shape), bits


@dropout.register_fake
def _(x, state, site, p):
    x4 = x if x.dim() == 4 else x.view(x.shape[0], 1, 1, -1)
    return torch.empty_like(x), x.new_empty(x4.shape[0], x4.shape[1], (x4.shape[2] * x4.shape[3] + 3) // 4, dtype=torch.uint8)


@torch.library.custom_op('tamgcn::dropout_backward', mutates_args=())
def dropout_backward(dout: Tensor, bits: Tensor, p: float) -> Tensor:
    d4 = _rows4(dout)
    dx, _, _ = ops.drop_add_act_bwd(d4, bits, False, p, None, None, None, None, want_dzr=False)
    return dx.view(dout.shape)


@dropout_backward.register_fake
def _(dout, bits, p):
    return torch.empty_like(dout)


def _dropout_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.p = inputs[3]


def _dropout_bwd(ctx, dout, _dbits):
    return torch.ops.tamgcn.dropout_backward(dout, ctx.saved_tensors[0], ctx.p), None, None, None


dropout.register_autograd(_dropout_bwd, setup_context=_dropout_setup)


# ---------------------------------------------------------------------------------------------------------------
# input side (no autograd)
# ---------------------------------------------------------------------------------------------------------------
@torch.library.custom_op('tamgcn::stream_derive', mutates_args=())
def stream_derive(x: Tensor, parent: Tensor, mode: int) -> Tensor:
    return ops.stream_derive(_c(x), parent, mode) if mode else x.clone()


@stream_derive.register_fake
def _(x, parent, mode):
    return torch.empty_like(x)


@torch.library.custom_op('tamgcn::feeder_transform', mutates_args=())
def feeder_transform(raw: Tensor, offsets: Tensor, rot: Tensor, idx: Tensor, parent: Tensor, V: int, time_steps: int,
                     center_joint: int, mode: int) -> Tensor:
    return ops.feeder_transform(raw, offsets, rot, idx, parent, V, time_steps, center_joint, mode)


@feeder_transform.register_fake
def _(raw, offsets, rot, idx, parent, V, time_steps, center_joint, mode):
    return raw.new_empty(offsets.shape[0] - 1, 3, time_steps, V, 1, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------
# skeleton guidance (tam_gcn_amd/guidance.py; no autograd: the callers run under no_grad)
# ---------------------------------------------------------------------------------------------------------------
@torch.library.custom_op('tamgcn::guidance_reduce', mutates_args=())
def guidance_reduce(h: Tensor, M: int) -> tuple[Tensor, Tensor, Tensor]:
    return ops.guidance_reduce(_c(h), M)


@guidance_reduce.register_fake
def _(h, M):
    NM, C_, Tp, V = h.shape
    N = NM // M
    parts = NM * ((Tp * V + 63) // 64)
    return (h.new_empty(N, Tp, V, M, dtype=torch.float32), h.new_empty(N, C_, dtype=torch.float32),
            h.new_empty(parts, 2, dtype=torch.float32))


@torch.library.custom_op('tamgcn::guidance_weights', mutates_args=())
def guidance_weights(intensity: Tensor, minmax: Tensor, joints: Tensor, k: int) -> Tensor:
    return ops.guidance_weights(_c(intensity), _c(minmax), _c(joints), k)


@guidance_weights.register_fake
def _(intensity, minmax, joints, k):
    return intensity.new_empty(intensity.shape[0], joints.shape[0], dtype=torch.float32)


@torch.library.custom_op('tamgcn::guidance_apply', mutates_args=())
def guidance_apply(weights: Tensor, rgb: Tensor | None, frames: int, H: int, W: int, want_map: bool) -> tuple[Tensor, Tensor]:
    """(rgb * map, map); a part that was not asked for (rgb None, want_map False) comes back with 0 elements"""
    out, wmap = ops.guidance_apply(_c(weights), None if rgb is None else _c(rgb), frames, H, W, want_map)
    return (weights.new_empty(0) if out is None else out), (weights.new_empty(0) if wmap is None else wmap)


@guidance_apply.register_fake
def _(weights, rgb, frames, H, W, want_map):
    N = weights.shape[0]
    out = weights.new_empty(0) if rgb is None else weights.new_empty(N, rgb.shape[1], H, W)
    return out, (weights.new_empty(N, 1, H, W) if want_map else weights.new_empty(0))


# ---------------------------------------------------------------------------------------------------------------
# cross-modal attention head (tam_gcn_amd/crossmodal.py; reference models/resnet_gcn_attention.py:60-70, :89-120): everything
# between the pooled skeleton feature f (N, D) / the image map f_rgb (N, R, H, W) and the logits, on libtamgcn_xmodal.so
# (include/tamgcn_xmodal.h) plus the core's head_fc.  Three new launches forward, four (five with d f) backward; the gated
# copy of the map is never written.  Besides the logits the forward returns what the backward reads (cross_entropy_opts does the
# same with g): pooled g, att, m (N, R), a1, xhat (N, Hd), invstd (Hd).
# ---------------------------------------------------------------------------------------------------------------
def _a16(t):
    """contiguous and 16-byte aligned, as include/tamgcn_xmodal.h asks of everything but the map (a parameter that is a view into
    a flat arena at an odd offset is copied)"""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _xm_dims(f, f_rgb, W1, W2, Wc, training):
    if f.dim() != 2 or f_rgb.dim() != 4 or f_rgb.shape[0] != f.shape[0]:
        raise ValueError(f'xmodal_head: f must be (N, D) and f_rgb (N, R, H, W) for the same N, got {tuple(f.shape)} and {tuple(f_rgb.shape)}')
    N, D = f.shape
    Hd, R, K = W1.shape[0], W2.shape[0], Wc.shape[0]
    if tuple(W1.shape) != (Hd, D) or tuple(W2.shape) != (R, Hd) or tuple(Wc.shape) != (K, R) or f_rgb.shape[1] != R:
        raise ValueError(f'xmodal_head: W1 {tuple(W1.shape)}, W2 {tuple(W2.shape)}, Wc {tuple(Wc.shape)} do not chain from D = {D} '
                         f'to the R = {f_rgb.shape[1]} channels of f_rgb')
    P = f_rgb.shape[2] * f_rgb.shape[3]
    if D % 4 or Hd % 4 or R % 4 or min(D, Hd, R) < 4:
        raise ValueError(f'xmodal_head: D = {D}, Hd = {Hd} and R = {R} must be positive multiples of 4')
    if P < 1 or K < 1:
        raise ValueError(f'xmodal_head: H * W = {P} and K = {K} must be at least 1')
    if N == 1 and training:
        raise ValueError(f'Expected more than 1 value per channel when training, got input size {torch.Size((N, Hd))}')
    if not 1 <= N <= 1024:
        raise ValueError(f'xmodal_head: N = {N} clips outside 1..1024')
    if N * R * P >= 2 ** 31:
        raise ValueError(f'xmodal_head: f_rgb has {N * R * P} elements, the limit is 2^31 - 1')
    return N, D, Hd, R, P, K


@torch.library.custom_op('tamgcn::xmodal_head', mutates_args=('running_mean', 'running_var', 'num_batches_tracked'))
def xmodal_head(f: Tensor, f_rgb: Tensor, W1: Tensor, b1: Tensor, bn_w: Tensor, bn_b: Tensor, running_mean: Tensor, running_var: Tensor,
                num_batches_tracked: Tensor, W2: Tensor, b2: Tensor, Wc: Tensor, bc: Tensor, training: bool, momentum: float,
                eps: float) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    from . import _xm_lib
    N, D, Hd, R, P, K = _xm_dims(f, f_rgb, W1, W2, Wc, training)
    for name, t in (('running_mean', running_mean), ('running_var', running_var)):
        if not (t.is_contiguous() and t.data_ptr() % 16 == 0 and tuple(t.shape) == (Hd,)):
            raise RuntimeError(f'xmodal_head: {name} must be a contiguous, 16-byte aligned ({Hd},) buffer: it is updated in place')
    if num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1:
        raise RuntimeError('xmodal_head: num_batches_tracked must be one int64')
    lib, p, st = _xm_lib.load(), ops._ptr, ops._stream()
    f, frgb = _a16(f), f_rgb.contiguous()                         # the map may start at any dword
    a1, xhat = f.new_empty(N, Hd), f.new_empty(N, Hd)
    mean, invstd = f.new_empty(Hd), f.new_empty(Hd)
    att, m, g = f.new_empty(N, R), f.new_empty(N, R), ops.empty(N, R, like=f)
    _xm_lib.check(lib.tamgcn_xm_hidden_fwd(p(f), p(_a16(W1)), p(_a16(b1)), p(_a16(bn_w)), p(_a16(bn_b)), p(running_mean), p(running_var),
                                           p(num_batches_tracked), N, D, Hd, int(training), momentum, eps, p(a1), p(xhat), p(mean), p(invstd), st),
                  'tamgcn_xm_hidden_fwd')
    _xm_lib.check(lib.tamgcn_xm_gate_fwd(p(a1), p(_a16(W2)), p(_a16(b2)), N, Hd, R, p(att), st), 'tamgcn_xm_gate_fwd')
    _xm_lib.check(lib.tamgcn_xm_pool_fwd(p(frgb), p(att), N, R, P, p(m), p(g), st), 'tamgcn_xm_pool_fwd')
    return ops.head_fc_fwd(g, _c(Wc), _c(bc)), g, att, m, a1, xhat, invstd


@xmodal_head.register_fake
def _(f, f_rgb, W1, b1, bn_w, bn_b, running_mean, running_var, num_batches_tracked, W2, b2, Wc, bc, training, momentum, eps):
    N, Hd, R = f.shape[0], W1.shape[0], W2.shape[0]
    return (f.new_empty(N, Wc.shape[0]), f.new_empty(N, R), f.new_empty(N, R), f.new_empty(N, R), f.new_empty(N, Hd), f.new_empty(N, Hd),
            f.new_empty(Hd))


@torch.library.custom_op('tamgcn::xmodal_head_backward', mutates_args=())
def xmodal_head_backward(dlogits: Tensor, f: Tensor, W1: Tensor, bn_w: Tensor, W2: Tensor, Wc: Tensor, g: Tensor, att: Tensor, m: Tensor,
                         a1: Tensor, xhat: Tensor, invstd: Tensor, H: int, W: int, training: bool, need_f: bool,
                         need_f_rgb: bool) -> list[Tensor]:
    """[df, df_rgb, dW1, db1, dbn_w, dbn_b, dW2, db2, dWc, dbc]; df / df_rgb have 0 elements when not asked for"""
    from . import _xm_lib
    lib, p, st = _xm_lib.load(), ops._ptr, ops._stream()
    N, D = f.shape
    Hd, R, P = W1.shape[0], W2.shape[0], H * W
    f, W1, W2 = _a16(f), _a16(W1), _a16(W2)
    dWc, dbc, dg = ops.head_fc_bwd(_c(dlogits), g, _c(Wc))
    dz2 = f.new_empty(N, R)
    df_rgb = f.new_empty(N, R, H, W) if need_f_rgb else f.new_empty(0)
    _xm_lib.check(lib.tamgcn_xm_pool_bwd(p(dg), p(m), p(att), N, R, P, p(dz2), p(df_rgb) if need_f_rgb else None, st), 'tamgcn_xm_pool_bwd')
    dW2, db2, da1 = torch.empty_like(W2), f.new_empty(R), f.new_empty(N, Hd)
    _xm_lib.check(lib.tamgcn_xm_gate_bwd(p(dz2), p(a1), p(W2), N, Hd, R, p(dW2), p(db2), p(da1), st), 'tamgcn_xm_gate_bwd')
    dgam, dbet, dW1, db1, dz1 = f.new_empty(Hd), f.new_empty(Hd), torch.empty_like(W1), f.new_empty(Hd), f.new_empty(N, Hd)
    df = f.new_empty(N, D) if need_f else f.new_empty(0)
    _xm_lib.check(lib.tamgcn_xm_hidden_bwd(p(da1), p(a1), p(xhat), p(invstd), p(_a16(bn_w)), p(f), p(W1), N, D, Hd, int(training), p(dgam), p(dbet),
                                           p(dW1), p(db1), p(dz1), p(df) if need_f else None, st), 'tamgcn_xm_hidden_bwd')
    return [df, df_rgb, dW1, db1, dgam, dbet, dW2, db2, dWc, dbc]


@xmodal_head_backward.register_fake
def _(dlogits, f, W1, bn_w, W2, Wc, g, att, m, a1, xhat, invstd, H, W, training, need_f, need_f_rgb):
    N, Hd, R = f.shape[0], W1.shape[0], W2.shape[0]
    return [torch.empty_like(f) if need_f else f.new_empty(0), f.new_empty(N, R, H, W) if need_f_rgb else f.new_empty(0), torch.empty_like(W1),
            f.new_empty(Hd), f.new_empty(Hd), f.new_empty(Hd), torch.empty_like(W2), f.new_empty(R), torch.empty_like(Wc),
            f.new_empty(Wc.shape[0])]


class XModalHeadFn(torch.autograd.Function):
    """logits = XModalHeadFn.apply(f, f_rgb, W1, ..., eps): the autograd node of tamgcn::xmodal_head.  torch.library refuses
    register_autograd on an operator that mutates its arguments, and this one updates the three BatchNorm buffers in its first
    kernel -- so, as for the training block nodes above, the node is an autograd.Function around the two registered ops.  d f and
    d f_rgb are computed only when those inputs require them."""

    @staticmethod
    def forward(ctx, f, f_rgb, W1, b1, bn_w, bn_b, running_mean, running_var, num_batches_tracked, W2, b2, Wc, bc, training, momentum, eps):
        logits, *saved = torch.ops.tamgcn.xmodal_head(f, f_rgb, W1, b1, bn_w, bn_b, running_mean, running_var, num_batches_tracked, W2, b2,
                                                      Wc, bc, training, momentum, eps)
        ctx.save_for_backward(f, W1, bn_w, W2, Wc, *saved)
        ctx.H, ctx.W, ctx.training = f_rgb.shape[2], f_rgb.shape[3], training
        return logits

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogits):
        need_f, need_f_rgb = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        df, df_rgb, dW1, db1, dgam, dbet, dW2, db2, dWc, dbc = torch.ops.tamgcn.xmodal_head_backward(
            dlogits, *ctx.saved_tensors, ctx.H, ctx.W, ctx.training, need_f, need_f_rgb)
        return (df if need_f else None, df_rgb if need_f_rgb else None, dW1, db1, dgam, dbet, None, None, None, dW2, db2, dWc, dbc,
                None, None, None)
