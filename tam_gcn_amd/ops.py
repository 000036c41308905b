"""Thin Python plumbing over the C ABI: device pointers out of torch tensors,
output allocation through torch's caching allocator, the current HIP stream.
No arithmetic happens here."""
import ctypes as C
import os
import threading

import torch

from . import _lib
from ._lib import Src, ConvDesc, WgradDesc, CtrgcDesc, ReduceDesc, TconvDesc, TCONV_MAXB

RELU = 1


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    if t is None:
        return None
    if not (t.is_cuda and t.is_contiguous()):
        raise RuntimeError('tam_gcn_amd: expected a contiguous HIP (cuda) tensor; there is no CPU path')
    if t.dtype not in (torch.float32, torch.int64, torch.int32, torch.float64, torch.uint8):
        raise RuntimeError(f'tam_gcn_amd: unsupported dtype {t.dtype}')
    return t.data_ptr()


class S:
    """A fused-prologue operand: value = act(c1*x1 + c2*x2 + c0) over (N, ctot, T, V)."""
    __slots__ = ('x1', 'x2', 'coef', 'coff', 'act', 'ctot')

    def __init__(self, x1, x2=None, coef=None, coff=0, act=0):
        self.x1, self.x2, self.coef, self.coff, self.act = x1, x2, coef, coff, act
        self.ctot = x1.shape[1]
        if x2 is not None and x2.shape != x1.shape:
            raise RuntimeError('tam_gcn_amd: x1/x2 geometry mismatch')
        if coef is not None and tuple(coef.shape) != (3, self.ctot):
            raise RuntimeError(f'tam_gcn_amd: coef shape {tuple(coef.shape)} != (3,{self.ctot})')

    def c(self):
        return Src(_ptr(self.x1), _ptr(self.x2), _ptr(self.coef), self.ctot, self.coff, self.act)


def _lib_():
    return _lib.load()


# Kernels index one launch's tensors with 32-bit element offsets inside a sample block and refuse tensors of >= 2^32
# elements; the V = 64, T = 512, C = 256 configuration at 256 clips has a 6.4e9-element x3.  Such calls are split over
# the clip dimension N (clips are independent; every tensor is contiguous in n) into launches below this bound.
CHUNK_ELEMS = int(os.environ.get("TAMGCN_CHUNK_ELEMS", str(2 ** 32 - 1)))


def n_chunks(N, per_clip):
    """[(n0, n1)] covering range(N) such that (n1 - n0) * per_clip <= CHUNK_ELEMS (at least one clip per chunk)."""
    c = max(1, CHUNK_ELEMS // max(1, per_clip))
    return [(i, min(N, i + c)) for i in range(0, N, c)]


def _slice_src(src, n0, n1):
    return S(src.x1[n0:n1], None if src.x2 is None else src.x2[n0:n1], src.coef, src.coff, src.act)


SLACK = 4          # floats readable behind every activation the ops allocate (see with_slack)


def empty(*shape, like):
    """fp32 tensor on like's device with SLACK floats of readable memory behind its last element."""
    n = 1
    for d_ in shape:
        n *= d_
    return torch.empty(n + SLACK, device=like.device, dtype=torch.float32)[:n].view(shape)


def empty_like(t):
    return empty(*t.shape, like=t)


def zeros_like(t):
    return empty(*t.shape, like=t).zero_()


def with_slack(t):
    """The 16-byte kernels may read up to 12 bytes past the last element of an activation whose rows (V joints) are not
    a multiple of 4 floats (the last 16-byte piece of the last frame).  Tensors from empty() carry that slack; a tensor
    that ends exactly at the end of its storage (a caller's input, an autograd-made gradient) is copied once."""
    if t is None or t.shape[-1] % 4 == 0:
        return t
    st = t.untyped_storage()
    if st.nbytes() - (t.storage_offset() + t.numel()) * t.element_size() >= 4 * SLACK:
        return t
    out = empty(*t.shape, like=t)
    out.copy_(t)
    return out


# ---------------------------------------------------------------------------
def conv(src, K, w, bias, M, KT=1, dil=1, stride=1, pad=0, wmode=0, up=1,
         y=None, ycoff=0, T_out=None, T_y=None, ostride=1, add1=None, add2=None,
         bcast=None, bcast_scale=0.0, mask=None, aux=None, aux_center=None, auxcoff=0, stats=False,
         post_coef=None, post_act=0, sign=None, sign_coff=0):
    """y (N, yctot, T_y, V); returns (y, stats_part [2][yctot][nparts] or None).
    post_coef [3][yctot] / post_act: eval-mode fusion, y = act(c1*(conv + bias) + c0 + adds).
    sign (N, C, ceil(T_y*V / 4)) uint8: sign bits in place of `mask` (tamgcn_conv_signmask; row m uses channel sign_coff + m).
    The library refuses the shapes signmask_supported() does not admit."""
    if src.x1.shape[-1] % 4:
        src = S(with_slack(src.x1), with_slack(src.x2), src.coef, src.coff, src.act)
    x = src.x1
    N, _, T_in, V = x.shape
    if T_out is None:
        T_out = (T_in + 2 * pad - dil * (KT - 1) - 1) // stride + 1
    if y is None:
        if T_y is None:
            T_y = T_out
        y = empty(N, M, T_y, V, like=x)
    else:
        T_y = y.shape[2]
    per_clip = max(x.shape[1] * T_in * V, y.shape[1] * T_y * V)
    if N > 1 and N * per_clip > CHUNK_ELEMS:
        if stats or mask is not None or aux is not None or sign is not None:
            raise RuntimeError('tam_gcn_amd: a convolution over >= 2^31 elements cannot carry BatchNorm moments / a mask')
        for n0, n1 in n_chunks(N, per_clip):
            conv(_slice_src(src, n0, n1), K, w, bias, M, KT, dil, stride, pad, wmode, up, y=y[n0:n1], ycoff=ycoff, T_out=T_out,
                 ostride=ostride, add1=None if add1 is None else add1[n0:n1], add2=None if add2 is None else add2[n0:n1],
                 bcast=None if bcast is None else bcast[:, n0:n1].contiguous(), bcast_scale=bcast_scale,
                 post_coef=post_coef, post_act=post_act)
        return y, None
    d = ConvDesc()
    d.src = src.c()
    d.N, d.K, d.T_in, d.V = N, K, T_in, V
    d.w, d.bias = _ptr(w), _ptr(bias)
    d.M, d.KT, d.dil, d.stride, d.pad = M, KT, dil, stride, pad
    d.wmode, d.up = wmode, up
    d.y, d.yctot, d.ycoff = _ptr(y), y.shape[1], ycoff
    d.T_out, d.T_y, d.ostride = T_out, T_y, ostride
    d.add1, d.add2, d.bcast, d.bcast_scale = _ptr(add1), _ptr(add2), _ptr(bcast), bcast_scale
    mc = None
    if mask is not None:
        mc = mask.c()
        d.mask = C.pointer(mc)
    if aux is not None:
        d.aux, d.aux_center, d.auxctot, d.auxcoff = _ptr(aux), _ptr(aux_center), aux.shape[1], auxcoff
    if post_coef is not None:
        d.post_coef, d.post_ctot = _ptr(post_coef), post_coef.shape[1]
    d.post_act = int(post_act)
    part = None
    lib = _lib_()
    if stats:
        nparts = lib.tamgcn_conv_nparts(C.byref(d))
        if nparts <= 0:
            raise RuntimeError('tamgcn_conv: no tiling for this shape')
        part = empty(2, y.shape[1], nparts, like=x)
        d.stats_part, d.stats_ctot, d.stats_coff = _ptr(part), y.shape[1], ycoff
    if sign is not None:
        _lib.check(lib.tamgcn_conv_signmask(C.byref(d), _ptr(sign), sign.shape[1], sign_coff, _stream()), 'tamgcn_conv_signmask')
    else:
        _lib.check(lib.tamgcn_conv(C.byref(d), _stream()), 'tamgcn_conv')
    return y, part


# ---------------------------------------------------------------------------
# ReLU sign bits (include/tamgcn.h: tamgcn_conv_signmask): the forward passes that save for a backward leave one bit per element
# of g and of the block output, and the backward reads those instead of the activations
SIGNBITS = os.environ.get('TAMGCN_SIGNBITS', '1') != '0'   # 0: the backward reads the activations' signs, as before (A/B, tests)


def sign_empty(N, C_, T, V, like):
    """The sign-bit array of an (N, C_, T, V) tensor: a byte per four consecutive floats of a row."""
    return torch.empty(N, C_, (T * V + 3) // 4, device=like.device, dtype=torch.uint8)


def signmask_shape_ok(N, K, M, T, V, split_mode=0):
    """Whether tamgcn_conv_signmask serves a stride-1 two-source 1x1 data gradient of K channels into M at (N, *, T, V): the
    CONSERVATIVE side of the library's rule (conv.hip: the LDS-DMA GEMM's shapes as in pair_supported, its eight-wave form,
    and not the bf16 split kernel that takes M >= 128 in split mode 1)."""
    if V % 4 or V > 32 or T * V < 64 or K % 16 or M % 16 or K > 512 or M > 512 or N * max(K, M) * T * V > CHUNK_ELEMS:
        return False
    if os.environ.get('TAMGCN_CONV_WAVES', '8') == '4':
        return False
    return split_mode == 0 or M < 128


def signmask_supported(tensors, N, K, M, T, V):
    """signmask_shape_ok() at the library's current split mode, and every operand contiguous and 16-byte aligned."""
    if not signmask_shape_ok(N, K, M, T, V, _lib_().tamgcn_get_split_mode()):
        return False
    return all(t is None or (t.is_cuda and t.is_contiguous() and t.data_ptr() % 16 == 0) for t in tensors)


# ---------------------------------------------------------------------------
# two stride-1 1x1 GEMMs that share a tensor as one launch (tamgcn_conv_pair / tamgcn_wgrad_pair)
TCN_PAIR = os.environ.get('TAMGCN_TCN_PAIR', '1') != '0'   # 0: MS-TCN's entry convs and plain 1x1 branch as two launches per direction (A/B, tests)


def pair_supported(tensors, N, chans, T, V):
    """Whether tamgcn_conv_pair / tamgcn_wgrad_pair serve this shape.  The library refuses what its LDS-DMA kernels do not run
    (conv.hip plan_conv: vec / flat / LB; wgrad.hip wgrad_glds_plan) and there is no entry point to ask it, so this is the
    CONSERVATIVE side of those rules -- everything it admits they admit: 16-byte rows (V % 4 == 0) of whole frames (V <= 32:
    a tile of 320 // V frames holds >= 64 columns, and so does a shorter clip with T * V >= 64), 16-byte aligned contiguous
    operands, channel counts in whole 16-row chunks, one launch for the batch.  chans <= 512 also keeps plan_conv's LDS bound
    (4 * (64 * 34 + 32 * 336 + 512 + 3 * 512) < 64 KB at the largest row tile) away from its frame-halving loop, so the plan
    -- frames per tile, hence moment partials -- is the same for M = M0, M1 and M0 + M1: what the row split's bit-identity
    with the two launches rests on.  Anything else takes the two launches."""
    if V % 4 or V > 32 or T * V < 64 or any(c % 16 or c > 512 for c in chans) or N * max(chans) * T * V > CHUNK_ELEMS:
        return False
    return all(t is None or (t.is_cuda and t.is_contiguous() and t.data_ptr() % 16 == 0) for t in tensors)


def conv_pair(src, w0, w1, bias0=None, bias1=None, y0=None, ycoff0=0, y1=None, ycoff1=0, stats=False):
    """y0[:, ycoff0:+M0] = w0 . src + bias0 and y1[:, ycoff1:+M1] = w1 . src + bias1 in one launch, w0 (M0, K, 1, 1),
    w1 (M1, K, 1, 1); returns (y0, part0, y1, part1), bit-identical to the two conv() calls."""
    if src.x1.shape[-1] % 4:                               # as conv(): the same kernels stream src (pair_supported admits no such V today)
        src = S(with_slack(src.x1), with_slack(src.x2), src.coef, src.coff, src.act)
    x = src.x1
    N, _, T, V = x.shape
    M0, M1, K = w0.shape[0], w1.shape[0], w0.shape[1]
    if w1.shape[1] != K:
        raise RuntimeError('tamgcn_conv_pair: the two weight matrices have the same K')
    d = _lib.ConvPairDesc()
    d.N, d.T, d.V, d.stride = N, T, V, 1
    d.src = src.c()
    d.w0, d.w1 = _ptr(w0), _ptr(w1)
    d.K, d.M0, d.M1 = K, M0, M1
    d.bias0, d.bias1 = _ptr(bias0), _ptr(bias1)
    if y0 is None:
        y0 = empty(N, M0, T, V, like=x)
    if y1 is None:
        y1 = empty(N, M1, T, V, like=x)
    if y0.shape[2:] != x.shape[2:] or y1.shape[2:] != x.shape[2:]:
        raise RuntimeError('tamgcn_conv_pair: destination geometry differs from the source (stride-1 1x1 only)')
    d.y0, d.yctot0, d.ycoff0 = _ptr(y0), y0.shape[1], ycoff0
    d.y1, d.yctot1, d.ycoff1 = _ptr(y1), y1.shape[1], ycoff1
    lib = _lib_()
    part0 = part1 = None
    if stats:
        cd = ConvDesc()                                    # the partial count is that of the single GEMM with the stacked rows
        cd.src = d.src
        cd.N, cd.K, cd.T_in, cd.V, cd.M, cd.KT, cd.dil, cd.stride, cd.up = N, K, T, V, M0 + M1, 1, 1, 1, 1
        cd.T_out, cd.T_y, cd.ostride = T, T, 1
        nparts = lib.tamgcn_conv_nparts(C.byref(cd))
        if nparts <= 0:
            raise RuntimeError('tamgcn_conv_pair: no tiling for this shape')
        part0 = empty(2, y0.shape[1], nparts, like=x)
        part1 = empty(2, y1.shape[1], nparts, like=x)
        d.stats_part0, d.stats_ctot0, d.stats_coff0 = _ptr(part0), y0.shape[1], ycoff0
        d.stats_part1, d.stats_ctot1, d.stats_coff1 = _ptr(part1), y1.shape[1], ycoff1
    _lib.check(lib.tamgcn_conv_pair(C.byref(d), _stream()), 'tamgcn_conv_pair')
    return y0, part0, y1, part1


def _wgrad_desc(gy, src, M, K, KT=1, dil=1, stride=1, pad=0):
    d = WgradDesc()
    d.gy, d.src = gy.c(), src.c()
    d.N, d.M, d.K, d.T_in, d.T_out, d.V = gy.x1.shape[0], M, K, src.x1.shape[2], gy.x1.shape[2], gy.x1.shape[3]
    d.KT, d.dil, d.stride, d.pad = KT, dil, stride, pad
    return d


def _wgrad_splits(d, nlaunch=1):
    """The ONE sizing rule of the weight-gradient launches (wgrad(), wgrad_pair(), wgrad_pair_nsplit()): slabs for descriptor
    d when nlaunch launches share the contraction -- aim at WGRAD_BLOCKS workgroups (tiles x splits; same tile rule as
    wgrad_tile() in csrc/wgrad.hip), never past tamgcn_wgrad_max_split."""
    M, K, KT = d.M, d.K, d.KT
    taps = KT > 1 and d.stride == 1 and d.T_in == d.T_out and (M > 32 or K > 32 or (d.V % 4 != 0 and (M > 16 or K > 16)))      # one window per tap on the LDS-DMA kernel
    if KT == 1 or taps:
        bm, bk = (64 if M <= 64 else 128), (64 if K <= 64 else 128)
    elif KT == 9:
        bm = bk = 32
    else:
        bm = bk = 32 if (M <= 32 and K <= 32) else 64
    tiles = ((M + bm - 1) // bm) * ((K + bk - 1) // bk) * (KT if taps else 1)
    per = max(1, (WGRAD_BLOCKS + tiles - 1) // tiles // nlaunch)
    return max(1, min(_lib_().tamgcn_wgrad_max_split(C.byref(d)), per))


def wgrad_pair_nsplit(gy0, gy1, src, M0, M1, K):
    """The split count at which wgrad_pair() is bit-identical to the two wgrad() launches, or None.  A row of dW sums its
    products chunk by chunk inside a split and the splits in a fixed order, whatever rows share its tile: the paired launch
    reproduces both single launches exactly when all three cut the contraction into the same number of splits."""
    ns = [_wgrad_splits(_wgrad_desc(gy, src, M, K)) for gy, M in ((gy0, M0 + M1), (gy0, M0), (gy1, M1))]
    return ns[0] if ns[0] == ns[1] == ns[2] else None


def wgrad_pair(gy0, gy1, src, M0, M1, K, rows=None, nsplit=None):
    """dW of two 1x1 convolutions of the same src in one launch: rows [0, M0) from gy0, rows [M0, M0 + M1) from gy1.
    Returns the (M0 + M1, K, 1, 1) gradient, or with rows = [m0, m1, ...] (summing to M0 + M1) one tensor per entry.
    nsplit: the slab count (None: wgrad()'s rule for M = M0 + M1; the library refuses one past tamgcn_wgrad_max_split)."""
    N, _, T, V = src.x1.shape
    M = M0 + M1
    if nsplit is None:
        nsplit = _wgrad_splits(_wgrad_desc(gy0, src, M, K))
    part = empty(nsplit, M, K, 1, like=src.x1)
    d = _lib.WgradPairDesc()
    d.gy0, d.gy1, d.src = gy0.c(), gy1.c(), src.c()
    d.N, d.M0, d.M1, d.K, d.T, d.V, d.stride = N, M0, M1, K, T, V, 1
    d.part, d.nsplit = _ptr(part), nsplit
    _lib.check(_lib_().tamgcn_wgrad_pair(C.byref(d), _stream()), 'tamgcn_wgrad_pair')
    if rows is not None:
        return reduce_sum(part, nsplit, chunks=[(m, K, 1, 1) for m in rows])
    if nsplit == 1:
        return part.view(M, K, 1, 1)
    return reduce_sum(part, nsplit).view(M, K, 1, 1)


# ---------------------------------------------------------------------------
# the MS-TCN second stage in one launch per direction (csrc/tconv.hip)
TCONV = os.environ.get('TAMGCN_TCONV', '1') != '0'         # 0: every branch through tamgcn_conv / tamgcn_maxpool_fwd (A/B, tests)


def tconv_supported(V, Cb, ks, dils, stride, T_in):
    """True when tamgcn_tconv_fwd / _bwd are built for this branch geometry (one kernel size for every branch)."""
    if not TCONV or not dils or len(dils) > TCONV_MAXB or any(k != ks[0] for k in ks):
        return False
    arr = (C.c_int * len(dils))(*[int(d_) for d_ in dils])
    return bool(_lib_().tamgcn_tconv_supported(V, Cb, int(ks[0]), len(dils), arr, stride, T_in))


def _tconv_desc(src, Cb, KT, dils, stride, ws, T_in, T_out, y, ycoff):
    d = TconvDesc()
    d.src = src.c()
    d.N, d.T_in, d.T_out, d.V, d.Cb, d.nb, d.KT, d.stride = src.x1.shape[0], T_in, T_out, src.x1.shape[3], Cb, len(dils), KT, stride
    for b, (dl, w) in enumerate(zip(dils, ws)):
        if tuple(w.shape[:3]) != (Cb, Cb, KT):
            raise RuntimeError(f'tamgcn_tconv: branch {b} weight {tuple(w.shape)}, expected ({Cb}, {Cb}, {KT}, 1)')
        d.dil[b], d.w[b] = int(dl), _ptr(w)
    d.y, d.yctot, d.ycoff = _ptr(y), y.shape[1], ycoff
    return d


def tconv_fwd(src, Cb, KT, dils, stride, ws, biases, pool, y, ycoff=0, stats=False):
    """Every temporal branch (and the pooled one) of an MS-TCN block: y[:, ycoff + b*Cb ...] for b < len(dils) (+ 1 with pool).
    src: S over (N, ctot, T_in, V) with the BatchNorm + ReLU prologue; returns the moment partials [2][yctot][nparts] or None."""
    N, _, T_in, V = src.x1.shape
    T_out = y.shape[2]
    if src.x1.shape[-1] % 4:
        src = S(with_slack(src.x1), None, src.coef, src.coff, src.act)
    d = _tconv_desc(src, Cb, KT, dils, stride, ws, T_in, T_out, y, ycoff)
    d.pool = int(bool(pool))
    for b, bi in enumerate(biases):
        d.bias[b] = _ptr(bi)
    lib = _lib_()
    part = None
    if stats:
        nparts = lib.tamgcn_tconv_nparts(C.byref(d), 0)
        if nparts <= 0:
            raise RuntimeError('tamgcn_tconv_fwd: no tiling for this shape')
        part = empty(2, y.shape[1], nparts, like=y)
        d.stats_part, d.stats_ctot = _ptr(part), y.shape[1]
    _lib.check(lib.tamgcn_tconv_fwd(C.byref(d), _stream()), 'tamgcn_tconv_fwd')
    return part


def tconv_bwd(gy, Cb, KT, dils, stride, ws, mask, center, dh, dcoff=0):
    """Data gradient of the temporal branches into dh[:, dcoff + b*Cb ...] (N, dctot, T_in, V), masked by relu(mask) > 0;
    returns the entry BatchNorm's backward moment partials [2][dctot][nparts]."""
    T_in, T_out = dh.shape[2], gy.x1.shape[2]
    if gy.x1.shape[-1] % 4:
        gy = S(with_slack(gy.x1), with_slack(gy.x2), gy.coef, gy.coff, gy.act)
        mask = S(with_slack(mask.x1), None, mask.coef, mask.coff, mask.act)
    d = _tconv_desc(gy, Cb, KT, dils, stride, ws, T_in, T_out, dh, dcoff)
    mc = mask.c()
    d.mask, d.center = C.pointer(mc), _ptr(center)
    lib = _lib_()
    nparts = lib.tamgcn_tconv_nparts(C.byref(d), 1)
    if nparts <= 0:
        raise RuntimeError('tamgcn_tconv_bwd: no tiling for this shape')
    part = empty(2, dh.shape[1], nparts, like=dh)
    d.stats_part, d.stats_ctot = _ptr(part), dh.shape[1]
    _lib.check(lib.tamgcn_tconv_bwd(C.byref(d), _stream()), 'tamgcn_tconv_bwd')
    return part


def tconv_wgrad_pays(V, Cb, stride):
    """Where the one-launch weight gradient of the temporal branches beats the per-branch launches (tools/tconv_bench.py,
    profiles/r04_tconv_bench.txt, 256 clips): 64-channel branches (129 vs 152 us, strided 176 vs 211), V = 25 except the
    16-channel stride-1 branches (0.9-1.35 ms vs 1.6-2.6 ms), V = 64 (1.30 vs 1.83 ms); at 16 / 32 channels and V = 20 the two
    are level (69 vs 74, 104 vs 104, 132 vs 126 us) and the per-branch launches stay."""
    if V > 32:
        return True
    if V % 4:
        return Cb >= 32 or stride > 1
    return Cb >= 64


def tconv_wgrad(gy, src, Cb, KT, dils, stride):
    """Weight gradients of every temporal branch in one launch: [dW_b (Cb, Cb, KT, 1) for b in branches].  gy: S over the
    gradient w.r.t. the concatenated output (two-source prologue), src: S over the forward's source (BatchNorm + ReLU)."""
    N, _, T_in, V = src.x1.shape
    T_out = gy.x1.shape[2]
    if V % 4:
        gy = S(with_slack(gy.x1), with_slack(gy.x2), gy.coef, gy.coff, gy.act)
        src = S(with_slack(src.x1), None, src.coef, src.coff, src.act)
    nb = len(dils)
    d = TconvDesc()
    d.src = gy.c()
    d.N, d.T_in, d.T_out, d.V, d.Cb, d.nb, d.KT, d.stride = N, T_in, T_out, V, Cb, nb, KT, stride
    for b, dl in enumerate(dils):
        d.dil[b] = int(dl)
    mc = src.c()
    d.mask = C.pointer(mc)
    lib = _lib_()
    mx = lib.tamgcn_tconv_wgrad_max_split(C.byref(d))
    if mx <= 0:
        raise RuntimeError('tamgcn_tconv_wgrad: no tiling for this shape')
    blocks = nb * (1 if Cb == 16 else (Cb // 32) ** 2)
    nsplit = max(1, min(mx, WGRAD_BLOCKS * 2 // blocks))
    part = empty(nsplit, nb, Cb, Cb, KT, like=gy.x1)
    d.y, d.yctot, d.ycoff = _ptr(part), nsplit, 0
    _lib.check(lib.tamgcn_tconv_wgrad(C.byref(d), _stream()), 'tamgcn_tconv_wgrad')
    return reduce_sum(part, nsplit, chunks=[(Cb, Cb, KT, 1)] * nb)


WGRAD_BLOCKS = int(os.environ.get('TAMGCN_WGRAD_BLOCKS', '512'))    # workgroups a weight gradient aims at (tiles x splits)


def wgrad(gy, src, M, K, KT=1, dil=1, stride=1, pad=0, rows=None):
    """Returns dW (M, K, KT, 1); with rows = [m0, m1, ...] (summing to M) a list of separate (m_i, K, KT, 1) tensors."""
    N, _, T_out, V = gy.x1.shape
    T_in = src.x1.shape[2]
    per_clip = max(gy.x1.shape[1] * T_out * V, src.x1.shape[1] * T_in * V)
    chunks = n_chunks(N, per_clip) if N * per_clip > CHUNK_ELEMS else [(0, N)]
    lib = _lib_()
    descs = []
    for n0, n1 in chunks:
        g_, s_ = (gy, src) if len(chunks) == 1 else (_slice_src(gy, n0, n1), _slice_src(src, n0, n1))
        descs.append((_wgrad_desc(g_, s_, M, K, KT, dil, stride, pad), g_, s_))
    splits = [_wgrad_splits(d, len(chunks)) for d, _, _ in descs]
    nsplit = sum(splits)                                   # every chunk's partial slabs sit in ONE array: one reduction
    part = empty(nsplit, M, K, KT, like=gy.x1)
    off = 0
    for (d, _, _), ns in zip(descs, splits):
        d.part, d.nsplit = part.data_ptr() + 4 * off * M * K * KT, ns
        _lib.check(lib.tamgcn_wgrad(C.byref(d), _stream()), 'tamgcn_wgrad')
        off += ns
    if rows is not None:
        return reduce_sum(part, nsplit, chunks=[(m, K, KT, 1) for m in rows])
    if nsplit == 1:
        return part.view(M, K, KT, 1)
    return reduce_sum(part, nsplit).view(M, K, KT, 1)


class ReduceBatch:
    """with ReduceBatch(): every reduce_sum() inside only registers its slabs and returns the (not yet filled) output;
    ONE tamgcn_reduce_multi launch on the stream current at exit fills them all.  The caller guarantees that nothing
    inside reads a reduced value and that every producer has been joined into that stream before the exit.

    The active batch is per THREAD: nn.DataParallel (the reference's multi-GPU mode, processor/io.py:86-87) runs one
    autograd thread per device and ctypes / torch calls release the GIL, so a process-global would let one device's
    reductions land in another device's batch."""
    _tls = threading.local()

    @staticmethod
    def active():
        return getattr(ReduceBatch._tls, 'active', None)

    def __enter__(self):
        self.items, self.prev = [], ReduceBatch.active()
        ReduceBatch._tls.active = self
        return self

    def __exit__(self, *exc):
        ReduceBatch._tls.active = self.prev
        if self.items and exc[0] is None:
            arr = (ReduceDesc * len(self.items))()
            for i, (part, nsplit, stride, off, count, scale, acc, out) in enumerate(self.items):
                arr[i] = ReduceDesc(part.data_ptr() + 4 * off, _ptr(out), nsplit, int(acc), stride, count, scale)
            _lib.check(_lib_().tamgcn_reduce_multi(arr, len(self.items), _stream()), 'tamgcn_reduce_multi')
        self.items = []
        return False


def reduce_sum(part, nsplit, scale=1.0, out=None, accumulate=False, chunks=None, immediate=False):
    """part [nsplit][...] -> sum over the leading dim (deferred to the enclosing ReduceBatch, if any).

    chunks = list of shapes: the reduced vector is delivered as that many SEPARATE tensors (consecutive pieces), so that
    gradients of parameters a kernel treats as one packed operand leave as tensors autograd can adopt without a copy."""
    count = part.numel() // nsplit
    if chunks is not None:
        outs, off = [], 0
        flat = part.view(nsplit, count)
        for shp in chunks:
            n = 1
            for d_ in shp:
                n *= d_
            o = torch.empty(shp, device=part.device, dtype=torch.float32)
            _reduce_piece(flat, nsplit, count, off, n, scale, o)
            outs.append(o)
            off += n
        assert off == count, 'reduce_sum: chunk shapes do not cover the slab'
        return outs
    if out is None:
        out = torch.empty(part.shape[1:], device=part.device, dtype=torch.float32)
    _reduce_piece(part, nsplit, count, 0, count, scale, out, accumulate, immediate)   # immediate: the value is read inside the batch
    return out


def _reduce_piece(part, nsplit, stride, off, count, scale, out, accumulate=False, immediate=False):
    rb = None if immediate else ReduceBatch.active()
    if rb is not None:
        rb.items.append((part, nsplit, stride, off, count, scale, accumulate, out))   # keeps `part` alive until the launch
        return
    src = C.c_void_p(part.data_ptr() + 4 * off)
    if nsplit > 128:                                       # the two-stage kernel reduces in place: on a private copy of the piece
        tmp = part.view(nsplit, stride)[:, off:off + count].contiguous()
        _lib.check(_lib_().tamgcn_reduce_sum(_ptr(tmp), nsplit, count, count, scale, int(accumulate), _ptr(out), _stream()),
                   'tamgcn_reduce_sum')
        return
    _lib.check(_lib_().tamgcn_reduce_sum(src, nsplit, stride, count, scale, int(accumulate), _ptr(out), _stream()),
               'tamgcn_reduce_sum')


# ---------------------------------------------------------------------------
def coef_diff(coef_d, coef_y, mode):
    """[3][C] prologue coefficients of diff = down(x) - bn(y) in one launch (include/tamgcn.h: tamgcn_coef_diff)."""
    out = torch.empty_like(coef_y)
    _lib.check(_lib_().tamgcn_coef_diff(_ptr(coef_d), _ptr(coef_y), _ptr(out), coef_y.shape[1], mode, _stream()), 'tamgcn_coef_diff')
    return out


# ---------------------------------------------------------------------------
def bn_fwd_finalize(part, part_coff, count, gamma, beta, rmean, rvar, nbt, momentum, eps, training,
                    coef, save, coff, C_):
    lib = _lib_()
    if part is not None:
        pctot, nparts = part.shape[1], part.shape[2]
    else:
        pctot, nparts = 0, 0
    _lib.check(lib.tamgcn_bn_fwd_finalize(_ptr(part), pctot, part_coff, nparts, float(count),
                                          _ptr(gamma), _ptr(beta), _ptr(rmean), _ptr(rvar), _ptr(nbt),
                                          momentum, eps, int(training), _ptr(coef), _ptr(save),
                                          coef.shape[1], coff, C_, _stream()), 'tamgcn_bn_fwd_finalize')


class BNBatch:
    """Collects BatchNorm finalisations whose partial sums are ready together and issues them as ONE launch per
    direction on the stream current at flush() (tamgcn_bn_*_finalize_multi)."""

    def __init__(self):
        self.f, self.b, self.keep = [], [], []

    def fwd(self, part, part_coff, count, gamma, beta, rmean, rvar, nbt, momentum, eps, training, coef, save, coff, C_):
        d = _lib.BnFwdDesc()
        d.part = _ptr(part)
        d.part_ctot, d.nparts = (part.shape[1], part.shape[2]) if part is not None else (0, 0)
        d.part_coff, d.count = part_coff, float(count)
        d.gamma, d.beta, d.running_mean, d.running_var, d.num_batches_tracked = _ptr(gamma), _ptr(beta), _ptr(rmean), _ptr(rvar), _ptr(nbt)
        d.momentum, d.eps, d.training = momentum, eps, int(training)
        d.coef, d.save, d.coef_ctot, d.coef_coff, d.C = _ptr(coef), _ptr(save), coef.shape[1], coff, C_
        self.f.append(d)
        self.keep += [part, coef, save]

    def bwd(self, part, part_coff, count, gamma, save, save_coff, training, dgamma, dbeta, dbias, coef, coff, C_):
        d = _lib.BnBwdDesc()
        d.part, d.part_ctot, d.part_coff, d.nparts, d.count = _ptr(part), part.shape[1], part_coff, part.shape[2], float(count)
        d.gamma, d.save, d.save_ctot, d.save_coff, d.training = _ptr(gamma), _ptr(save), save.shape[1], save_coff, int(training)
        d.dgamma, d.dbeta, d.dbias_conv = _ptr(dgamma), _ptr(dbeta), _ptr(dbias)
        d.coef, d.coef_ctot, d.coef_coff, d.C = _ptr(coef), coef.shape[1], coff, C_
        self.b.append(d)
        self.keep += [part, save, coef, dgamma, dbeta, dbias]

    def flush(self):
        lib = _lib_()
        if self.f:
            arr = (_lib.BnFwdDesc * len(self.f))(*self.f)
            _lib.check(lib.tamgcn_bn_fwd_finalize_multi(arr, len(self.f), _stream()), 'tamgcn_bn_fwd_finalize_multi')
        if self.b:
            arr = (_lib.BnBwdDesc * len(self.b))(*self.b)
            _lib.check(lib.tamgcn_bn_bwd_finalize_multi(arr, len(self.b), _stream()), 'tamgcn_bn_bwd_finalize_multi')
        self.f, self.b, self.keep = [], [], []


def bn_bwd_finalize(part, part_coff, count, gamma, save, save_coff, training, dgamma, dbeta, dbias, coef, coff, C_):
    lib = _lib_()
    _lib.check(lib.tamgcn_bn_bwd_finalize(_ptr(part), part.shape[1], part_coff, part.shape[2], float(count),
                                          _ptr(gamma), _ptr(save), save.shape[1], save_coff, int(training),
                                          _ptr(dgamma), _ptr(dbeta), _ptr(dbias), _ptr(coef), coef.shape[1], coff, C_,
                                          _stream()), 'tamgcn_bn_bwd_finalize')


# ---------------------------------------------------------------------------
def tmean(src, C_):
    N, _, T, V = src.x1.shape
    xbar = empty(C_, N, V, like=src.x1)
    sc = src.c()
    _lib.check(_lib_().tamgcn_tmean(C.byref(sc), N, C_, T, V, _ptr(xbar), _stream()), 'tamgcn_tmean')
    return xbar


def _ctrgc_desc(x, pq, w3, b3, w4, b4, A, alpha, Cin, Cout, S, R, E=None):
    N, _, T, V = x.x1.shape
    d = CtrgcDesc()
    d.N, d.Cin, d.Cout, d.S, d.R, d.T, d.V = N, Cin, Cout, S, R, T, V
    d.x = x.c()
    d.pq, d.w3, d.b3, d.w4, d.b4, d.A, d.alpha = (_ptr(pq), _ptr(w3), _ptr(b3), _ptr(w4), _ptr(b4), _ptr(A), _ptr(alpha))
    d.E = _ptr(E)
    return d


def ctrgc_route(V):
    """'fused'  V = 20: LDS-resident E tiles, x3 GEMM + VALU aggregation in one kernel;
    'stream' V = 25: x3 = W3 x through the pointwise GEMM (kept in HBM), aggregation / dE accumulation on MFMA with the joints padded
             to 32 in LDS, E and the dE tail from the per-(n, subset) kernels of the fused family;
    'tiled'  V in {32, 64}: the same with tiled E / tail kernels (E of one channel is 48 KB at V = 64);
    'vgen'   every other 2 <= V <= 32 (a user's skeleton): the stream route's kernels with V as a run-time argument
             (csrc/vgen.hip), joints padded to 16 or 32 in LDS."""
    k = _lib_().tamgcn_ctrgc_tiled_supported(int(V))
    if k == 1:
        return 'tiled'
    if k == 2 and V != 20:
        return 'stream'
    if V == 20:
        return 'fused'
    if _lib_().tamgcn_vgen_supported(int(V)) == 1:
        return 'vgen'
    raise RuntimeError(f'tam_gcn_amd: CTRGC is built for 2 <= V <= 32 joints and V = 64, got V = {V}')


def ctrgc_tiled(V):
    """True when CTRGC runs as x3 GEMM + MFMA aggregation kernels (routes 'tiled', 'stream' and 'vgen')."""
    return ctrgc_route(V) != 'fused'


def ctrgc_build_E(x, pq, w3, b3, w4, b4, A, alpha, Cin, Cout, S, R):
    """E (N, S, Cout, V, V) for every channel, once per layer; hand it to ctrgc_fwd / ctrgc_bwd_dx3."""
    N, _, T, V = x.x1.shape
    if R > 32 or R % 4:
        raise RuntimeError(f'tam_gcn_amd: CTRGC with R = {R} rel-channels is not built (multiples of 4 up to 32: in_channels <= 256 + 7)')
    d = _ctrgc_desc(x, pq, w3, b3, w4, b4, A, alpha, Cin, Cout, S, R)
    E = empty(N, S, Cout, V, V, like=x.x1)
    route = ctrgc_route(V)
    if route == 'tiled':
        _lib.check(_lib_().tamgcn_ctrgc_tiled_build_e(C.byref(d), _ptr(E), _stream()), 'tamgcn_ctrgc_tiled_build_e')
    elif route == 'vgen':
        _lib.check(_lib_().tamgcn_vgen_build_e(C.byref(d), _ptr(E), _stream()), 'tamgcn_vgen_build_e')
    else:
        _lib.check(_lib_().tamgcn_ctrgc_build_e(C.byref(d), _ptr(E), _stream()), 'tamgcn_ctrgc_build_e')
    return E


def _agg_entry(V, which):
    """The streaming entry point (agg_fwd / agg_bwd / de_acc) of V's route and its name: the templated kernels of the
    'stream' and 'tiled' routes, the run-time-V ones of 'vgen'."""
    name = ('tamgcn_vgen_' if ctrgc_route(V) == 'vgen' else 'tamgcn_ctrgc_tiled_') + which
    return getattr(_lib_(), name), name


def _x3_gemm(x, w3, b3, Cin, Cout, S):
    """x3 = conv3(x) of every subset as ONE pointwise GEMM: (N, S*Cout, T, V)."""
    x3, _ = conv(x, K=Cin, w=w3, bias=b3.reshape(-1), M=S * Cout)
    return x3


def ctrgc_fwd(x, pq, w3, b3, w4, b4, A, alpha, Cin, Cout, S, R, stats, keep_x3=False, E=None):
    """Returns (y, stats_part, x3); x3 (N,S*Cout,T,V) only when keep_x3 (for the backward)."""
    N, _, T, V = x.x1.shape
    d = _ctrgc_desc(x, pq, w3, b3, w4, b4, A, alpha, Cin, Cout, S, R, E)
    y = empty(N, Cout, T, V, like=x.x1)
    part = empty(2, Cout, N, like=x.x1) if stats else None
    if ctrgc_tiled(V):
        if E is None:
            E = ctrgc_build_E(x, pq, w3, b3, w4, b4, A, alpha, Cin, Cout, S, R)
        x3 = _x3_gemm(x, w3, b3, Cin, Cout, S)
        chunks = n_chunks(N, S * Cout * T * V)
        parts = []
        agg, name = _agg_entry(V, 'agg_fwd')
        for n0, n1 in chunks:                              # one launch unless x3 has >= 2^31 elements
            d.N = n1 - n0
            pc = None
            if stats:
                pc = part if len(chunks) == 1 else empty(2, Cout, n1 - n0, like=x.x1)
                parts.append(pc)
            _lib.check(agg(C.byref(d), _ptr(x3[n0:n1]), _ptr(E[n0:n1]), _ptr(y[n0:n1]), _ptr(pc), _stream()), name)
        if stats and len(chunks) > 1:
            part = torch.cat(parts, dim=2)
        return y, part, (x3 if keep_x3 else None)
    if E is None:
        E = ctrgc_build_E(x, pq, w3, b3, w4, b4, A, alpha, Cin, Cout, S, R)
        d.E = _ptr(E)
    x3 = empty(N, S * Cout, T, V, like=x.x1) if keep_x3 else None
    _lib.check(_lib_().tamgcn_ctrgc_fwd(C.byref(d), _ptr(y), _ptr(part), _ptr(x3), _stream()), 'tamgcn_ctrgc_fwd')
    return y, part, x3


def _dy_with_slack(dy):
    """The streaming kernels fetch dy in 16-byte pieces; where V % 4 != 0 the last piece of the last row reaches up to 12 bytes past
    the tensor (csrc/ctrgc_stream_body.h).  A gradient the ops allocated has that slack; a caller's cotangent that ends with its
    storage (the stand-alone CTRGC's, autograd's) is copied once."""
    if dy.x1.shape[-1] % 4 == 0:
        return dy
    x1, x2 = with_slack(dy.x1), with_slack(dy.x2)
    if x1 is dy.x1 and x2 is dy.x2:
        return dy
    return type(dy)(x1, x2, dy.coef, dy.coff, dy.act)


def ctrgc_bwd_dx3(x, pq, w3, b3, w4, b4, A, alpha, Cin, Cout, S, R, dy, E=None, per_subset=False):
    """dx3 (N,S*Cout,T,V) = E^T . dy, and db3 [S*Cout]."""
    N, _, T, V = x.x1.shape
    dy = _dy_with_slack(dy)
    d = _ctrgc_desc(x, pq, w3, b3, w4, b4, A, alpha, Cin, Cout, S, R, E)
    dyc = dy.c()
    dx3 = empty(N, S * Cout, T, V, like=x.x1)
    db3_part = empty(N, S * Cout, like=x.x1)
    if ctrgc_tiled(V):
        if E is None:
            E = ctrgc_build_E(x, pq, w3, b3, w4, b4, A, alpha, Cin, Cout, S, R)
        agg, name = _agg_entry(V, 'agg_bwd')
        for n0, n1 in n_chunks(N, S * Cout * T * V):
            d.N = n1 - n0
            dyc = _slice_src(dy, n0, n1).c()
            _lib.check(agg(C.byref(d), C.byref(dyc), _ptr(E[n0:n1]), _ptr(dx3[n0:n1]), _ptr(db3_part[n0:n1]), _stream()), name)
    else:
        if E is None:
            E = ctrgc_build_E(x, pq, w3, b3, w4, b4, A, alpha, Cin, Cout, S, R)
            d.E = _ptr(E)
        _lib.check(_lib_().tamgcn_ctrgc_bwd_dx3(C.byref(d), C.byref(dyc), _ptr(dx3), _ptr(db3_part), _stream()),
                   'tamgcn_ctrgc_bwd_dx3')
    return dx3, (reduce_sum(db3_part, N, chunks=[(Cout,)] * S) if per_subset else reduce_sum(db3_part, N))


def ctrgc_bwd_de_acc(dy, x3, Cout, S):
    """dE (N, S, Cout, V, V) = sum_t dy[n,c,t,u] x3[n,s*Cout+c,t,v]: the streaming accumulation of the dE chain.
    dy: an operand S(...) whose channels coff..coff+Cout are the gradient; x3 (N, S*Cout, T, V)."""
    N, _, T, V = x3.shape
    dy, x3 = _dy_with_slack(dy), with_slack(x3)
    d = CtrgcDesc()
    d.N, d.Cout, d.S, d.T, d.V = N, Cout, S, T, V
    dE = empty(N, S, Cout, V, V, like=x3)
    if ctrgc_route(V) != 'fused':
        acc, name = _agg_entry(V, 'de_acc')
        for n0, n1 in n_chunks(N, S * Cout * T * V):
            d.N = n1 - n0
            dyc = _slice_src(dy, n0, n1).c()
            _lib.check(acc(C.byref(d), C.byref(dyc), _ptr(x3[n0:n1]), _ptr(dE[n0:n1]), _stream()), name)
    else:
        dyc = dy.c()
        _lib.check(_lib_().tamgcn_ctrgc_bwd_de_acc(C.byref(d), C.byref(dyc), _ptr(x3), _ptr(dE), _stream()),
                   'tamgcn_ctrgc_bwd_de_acc')
    return dE


def ctrgc_bwd_de_tail(dE, pq, w4, b4, alpha, R, per_subset=False, groups=1):
    """dE (N, S, Cout, V, V) through E = alpha (W4 tanh(p_u - q_v) + b4) + A: dA [S,V,V], dw4 [S,Cout,R], db4 [S,Cout],
    dalpha [1], dpq [S*2*R,N,V], one per-(n, s) tail launch.  groups: channel groups per (n, subset) of the LDS-resident
    tail (V in {20, 25}); the per-workgroup fixed cost (D fill, dp/dq sums) equals ~1.4 channel chunks, so splitting did
    not pay (measured) and the model runs one."""
    N, S, Cout, V, _ = dE.shape
    d = CtrgcDesc()
    d.N, d.Cout, d.S, d.R, d.V = N, Cout, S, R, V
    d.pq, d.w4, d.b4, d.alpha = _ptr(pq), _ptr(w4), _ptr(b4), _ptr(alpha)
    like = dE
    ps = per_subset
    if ctrgc_route(V) == 'tiled':
        if groups != 1:
            raise RuntimeError('tam_gcn_amd: the tiled dE tail (V in {32, 64}) has no channel groups')
        NUC = _lib_().tamgcn_ctrgc_tiled_chunks(V)
        dA_part = empty(N, S, V, V, like=like)
        dw4_part = empty(N * NUC, S, Cout, R, like=like)
        db4_part = empty(N * NUC, S, Cout, like=like)
        dal_part = empty(N * S * NUC, 1, like=like)
        dpq = empty(NUC, S * 2 * R, N, V, like=like)
        _lib.check(_lib_().tamgcn_ctrgc_tiled_de_tail(C.byref(d), _ptr(dE), _ptr(dA_part), _ptr(dw4_part), _ptr(db4_part), _ptr(dal_part),
                                                      _ptr(dpq), _stream()), 'tamgcn_ctrgc_tiled_de_tail')
        return (reduce_sum(dA_part, N), reduce_sum(dw4_part, N * NUC, chunks=[(Cout, R, 1, 1)] * S if ps else None),
                reduce_sum(db4_part, N * NUC, chunks=[(Cout,)] * S if ps else None), reduce_sum(dal_part, N * S * NUC),
                reduce_sum(dpq, NUC, immediate=True))
    if R > 32:
        raise RuntimeError('tam_gcn_amd: CTRGC with R > 32 rel-channels is not built')
    G = groups
    dA_part = empty(N * G, S, V, V, like=like)
    dw4_part = empty(N, S, Cout, R, like=like)
    db4_part = empty(N, S, Cout, like=like)
    dal_part = empty(N * S * G, 1, like=like)
    dpq = empty(G, S * 2 * R, N, V, like=like)
    name = 'tamgcn_vgen_de_tail' if ctrgc_route(V) == 'vgen' else 'tamgcn_ctrgc_bwd_de_tail'
    _lib.check(getattr(_lib_(), name)(C.byref(d), _ptr(dE), _ptr(dA_part), _ptr(dw4_part), _ptr(db4_part),
                                      _ptr(dal_part), _ptr(dpq), G, _stream()), name)
    dpq = dpq[0] if G == 1 else reduce_sum(dpq, G, immediate=True)       # every group holds a partial dp / dq of its channels
    return (reduce_sum(dA_part, N * G), reduce_sum(dw4_part, N, chunks=[(Cout, R, 1, 1)] * S if ps else None),
            reduce_sum(db4_part, N, chunks=[(Cout,)] * S if ps else None), reduce_sum(dal_part, N * S * G), dpq)


def ctrgc_bwd_de(x, pq, w3, b3, w4, b4, A, alpha, Cin, Cout, S, R, dy, x3=None, per_subset=False):
    """The dE chain: dA [S,V,V], dw4 [S,Cout,R], db4 [S,Cout], dalpha [1], dpq [S*2*R,N,V]: a streaming accumulation of
    dE from dy and the x3 ctrgc_fwd kept (recomputed by one pointwise GEMM if it was not), then one per-(n, s) tail launch."""
    if x3 is None:                                          # the caller did not keep x3: one more pointwise GEMM
        x3 = _x3_gemm(x, w3, b3, Cin, Cout, S)
    dE = ctrgc_bwd_de_acc(dy, x3, Cout, S)
    return ctrgc_bwd_de_tail(dE, pq, w4, b4, alpha, R, per_subset=per_subset)


def ctrgc_bwd(x, pq, w3, b3, w4, b4, A, alpha, Cin, Cout, S, R, dy, x3=None, E=None):
    """Returns dx3 (N,S*Cout,T,V), db3 [S*Cout], dA [S,V,V], dw4 [S,Cout,R], db4 [S,Cout], dalpha [1], dpq [S*2*R,N,V]."""
    dy = _dy_with_slack(dy)                               # once for both chains
    dx3, db3 = ctrgc_bwd_dx3(x, pq, w3, b3, w4, b4, A, alpha, Cin, Cout, S, R, dy, E=E)
    dA, dw4, db4, dal, dpq = ctrgc_bwd_de(x, pq, w3, b3, w4, b4, A, alpha, Cin, Cout, S, R, dy, x3)
    return dx3, db3, dA, dw4, db4, dal, dpq


# ---------------------------------------------------------------------------
def gcn_tail_fwd(y, o, res, sign=None):
    """sign: None | list -- the sign bits of g are written too and appended to it."""
    N, _, T, V = y.x1.shape
    Cc = y.ctot
    g = empty(N, Cc, T, V, like=y.x1)
    yc, oc = y.c(), o.c()
    rc = res.c() if res is not None else None
    if sign is not None:
        bits = sign_empty(N, Cc, T, V, g)
        _lib.check(_lib_().tamgcn_gcn_tail_fwd_bits(C.byref(yc), C.byref(oc), C.byref(rc) if rc is not None else None,
                                                    N, Cc, T, V, _ptr(g), _ptr(bits), _stream()), 'tamgcn_gcn_tail_fwd_bits')
        sign.append(bits)
        return g
    _lib.check(_lib_().tamgcn_gcn_tail_fwd(C.byref(yc), C.byref(oc), C.byref(rc) if rc is not None else None,
                                           N, Cc, T, V, _ptr(g), _stream()), 'tamgcn_gcn_tail_fwd')
    return g


def gcn_tail_bwd(dg, g, o, o_save):
    N, Cc, T, V = g.shape
    dsum, doz = empty_like(g), empty_like(g)
    part = empty(2, Cc, N, like=g)
    oc = o.c()
    _lib.check(_lib_().tamgcn_gcn_tail_bwd(_ptr(dg), _ptr(g), C.byref(oc), _ptr(o_save), N, Cc, T, V, _ptr(dsum), _ptr(doz),
                                           _ptr(part), _stream()), 'tamgcn_gcn_tail_bwd')
    return dsum, doz, part


def gcn_tail_bwd_bits(dg, bits, o, o_save):
    """gcn_tail_bwd with the sign bits of g in place of g.  bits None: dg is dsum already (masked by its producer) and is
    returned as such -- g is not read and dsum is not written."""
    N, Cc, T, V = dg.shape
    dsum = empty_like(dg) if bits is not None else None
    doz = empty_like(dg)
    part = empty(2, Cc, N, like=dg)
    oc = o.c()
    _lib.check(_lib_().tamgcn_gcn_tail_bwd_bits(_ptr(dg), _ptr(bits), C.byref(oc), _ptr(o_save), N, Cc, T, V, _ptr(dsum), _ptr(doz),
                                                _ptr(part), _stream()), 'tamgcn_gcn_tail_bwd_bits')
    return (dsum if bits is not None else dg), doz, part


def gcn_mid_bwd(dsum, ddiff, y_pre, y_save, r_pre, r_save, want_dres):
    N, Cc, T, V = dsum.shape
    dyb = empty_like(dsum)
    dres = empty_like(dsum) if want_dres else None
    part = empty(4 if r_pre is not None else 2, Cc, N, like=dsum)
    _lib.check(_lib_().tamgcn_gcn_mid_bwd(_ptr(dsum), _ptr(ddiff), _ptr(y_pre), _ptr(y_save), _ptr(r_pre), _ptr(r_save), N, Cc, T, V,
                                          _ptr(dyb), _ptr(dres), _ptr(part), _stream()), 'tamgcn_gcn_mid_bwd')
    return dyb, dres, part


def maxpool_fwd(src, C_, stride, y, ycoff, stats):
    N, _, T_in, V = src.x1.shape
    T_out = y.shape[2]
    part = empty(2, y.shape[1], N, like=y) if stats else None
    sc = src.c()
    _lib.check(_lib_().tamgcn_maxpool_fwd(C.byref(sc), N, C_, T_in, V, stride, _ptr(y), y.shape[1], ycoff, T_out,
                                          _ptr(part), _stream()), 'tamgcn_maxpool_fwd')
    return part


def maxpool_post_fwd(src, C_, stride, y, ycoff, coef, add, relu):
    """Eval-mode pooled branch finished in place: y[:, ycoff:ycoff+C_] = act(c1 * maxpool(src) + c0 + add)."""
    N, _, T_in, V = src.x1.shape
    sc = src.c()
    _lib.check(_lib_().tamgcn_maxpool_post_fwd(C.byref(sc), N, C_, T_in, V, stride, _ptr(y), y.shape[1], ycoff, y.shape[2],
                                               _ptr(coef), _ptr(add), int(relu), _stream()), 'tamgcn_maxpool_post_fwd')


def maxpool_bwd(gy, src, src_save, C_, stride, d, dcoff):
    N, _, T_in, V = src.x1.shape
    T_out = gy.x1.shape[2]
    part = empty(2, d.shape[1], N, like=d)
    gc, sc = gy.c(), src.c()
    _lib.check(_lib_().tamgcn_maxpool_bwd(C.byref(gc), C.byref(sc), _ptr(src_save), N, C_, T_in, T_out, V, stride, _ptr(d),
                                          d.shape[1], dcoff, _ptr(part), _stream()), 'tamgcn_maxpool_bwd')
    return part


XBAR_FOLD = os.environ.get('TAMGCN_XBAR_FOLD', '1') != '0'    # 0: every block computes its own frame means (tamgcn_tmean)


def add_act_fwd(a, res, relu, C_, rowmean=False, xbar=False, sign=None):
    """sign: None | list -- with relu, the sign bits of the output are written too and appended to it.
    rowmean: also return the (N, C) means over (t, v) of the output (the model head's pooling input).
    xbar: also return the (C, N, V) means over t of the output (the next block's pooled joint-embedding input) -- or None
    where the fused form does not apply (V % 4 != 0, V > 64)."""
    N, _, T, V = a.x1.shape
    out = empty(N, C_, T, V, like=a.x1)
    rm = torch.empty(N, C_, device=out.device, dtype=torch.float32) if rowmean else None
    xb = None
    if xbar and not rowmean and XBAR_FOLD and V % 4 == 0 and V <= 64:
        xb = empty(C_, N, V, like=a.x1)
    ac = a.c()
    rc = res.c() if res is not None else None
    if sign is not None and relu:
        bits = sign_empty(N, C_, T, V, out)
        _lib.check(_lib_().tamgcn_add_act_fwd_bits(C.byref(ac), C.byref(rc) if rc is not None else None,
                                                   N, C_, T, V, _ptr(out), _ptr(rm), _ptr(xb), _ptr(bits), _stream()), 'tamgcn_add_act_fwd_bits')
        sign.append(bits)
    else:
        _lib.check(_lib_().tamgcn_add_act_fwd(C.byref(ac), C.byref(rc) if rc is not None else None, int(relu),
                                              N, C_, T, V, _ptr(out), _ptr(rm), _ptr(xb), _stream()), 'tamgcn_add_act_fwd')
    if xbar:
        return out, xb
    return (out, rm) if rowmean else out


def add_act_bwd(dout, out, relu, a_pre, a_save, r_pre, r_save, want_dz):
    N, Cc, T, V = dout.shape
    dz = empty_like(dout) if want_dz else None
    part = empty(4 if r_pre is not None else 2, Cc, N, like=dout)
    _lib.check(_lib_().tamgcn_add_act_bwd(_ptr(dout), _ptr(out), int(relu), _ptr(a_pre), _ptr(a_save), _ptr(r_pre), _ptr(r_save), N, Cc, T, V,
                                          _ptr(dz), _ptr(part), _stream()), 'tamgcn_add_act_bwd')
    return dz, part


def add_act_bwd_bits(dout, bits, a_pre, a_save, r_pre, r_save, want_dz):
    """add_act_bwd (relu = 1) with the sign bits of `out` in place of `out`."""
    N, Cc, T, V = dout.shape
    dz = empty_like(dout) if want_dz else None
    part = empty(4 if r_pre is not None else 2, Cc, N, like=dout)
    _lib.check(_lib_().tamgcn_add_act_bwd_bits(_ptr(dout), _ptr(bits), _ptr(a_pre), _ptr(a_save), _ptr(r_pre), _ptr(r_save), N, Cc, T, V,
                                               _ptr(dz), _ptr(part), _stream()), 'tamgcn_add_act_bwd_bits')
    return dz, part


# ---------------------------------------------------------------------------
# dropout inside the residual tail (include/tamgcn.h: tamgcn_drop_add_act_fwd has the draw)
DROP_MAX_ROW = 2 ** 22        # elements per (n, c) row: the group index shares a counter word with the site id
DROP_MAX_SITES = 4096


def dropout_consts(p):
    """(thr, scale) of a drop probability p in (0, 1): thr = floor(p 2^32) and scale = float32(1 / (1 - p)), both from fp64.
    The scale is returned as the Python float that holds the rounded fp32 value."""
    p = float(p)
    if not 0.0 < p < 1.0:
        raise ValueError(f'tam_gcn_amd: the device dropout takes 0 < p < 1, not p = {p!r}')
    import numpy as np
    return int(p * 4294967296.0), float(np.float32(1.0 / (1.0 - p)))


def _drop_check(T, V, site):
    if T * V > DROP_MAX_ROW:
        raise ValueError(f'tam_gcn_amd: the device dropout takes rows of at most 2^22 elements, not T * V = {T * V}')
    if not 0 <= int(site) < DROP_MAX_SITES:
        raise ValueError(f'tam_gcn_amd: dropout site {site} outside 0 .. {DROP_MAX_SITES - 1}')


def drop_add_act_fwd(a, res, relu, C_, state, site, p, keep_bits=True):
    """out = act(keep * a * scale + res) over (N, C_, T, V); returns (out, bits or None).  state: the int64 [2] = (seed, call)
    tensor of a DropoutStream, read on the device.  bits (ops.sign_empty's shape): sign nibble low, keep nibble high."""
    N, _, T, V = a.x1.shape
    thr, scale = dropout_consts(p)
    _drop_check(T, V, site)
    if state.dtype != torch.int64 or state.numel() != 2:
        raise RuntimeError('tam_gcn_amd: the dropout state is an int64 [2] tensor')
    out = empty(N, C_, T, V, like=a.x1)
    bits = sign_empty(N, C_, T, V, out) if keep_bits else None
    ac = a.c()
    rc = res.c() if res is not None else None
    _lib.check(_lib_().tamgcn_drop_add_act_fwd(C.byref(ac), C.byref(rc) if rc is not None else None, int(bool(relu)), N, C_, T, V,
                                               _ptr(state), int(site), thr, scale, _ptr(out), _ptr(bits), _stream()),
               'tamgcn_drop_add_act_fwd')
    return out, bits


def drop_add_act_bwd(dout, bits, relu, p, a_pre, a_save, r_pre, r_save, want_dzr):
    """(dza, dzr or None, part or None) of drop_add_act_fwd's backward; part [4 | 2][C][N] exists iff a_pre is given."""
    N, Cc, T, V = dout.shape
    _, scale = dropout_consts(p)
    dza = empty_like(dout)
    dzr = empty_like(dout) if (want_dzr or r_pre is not None) else None
    part = empty(4 if r_pre is not None else 2, Cc, N, like=dout) if a_pre is not None else None
    _lib.check(_lib_().tamgcn_drop_add_act_bwd(_ptr(dout), _ptr(bits), int(bool(relu)), scale, _ptr(a_pre), _ptr(a_save), _ptr(r_pre),
                                               _ptr(r_save), N, Cc, T, V, _ptr(dza), _ptr(dzr), _ptr(part), _stream()),
               'tamgcn_drop_add_act_bwd')
    return dza, dzr, part


def dropout_advance(state):
    """call += 1 on the device, in stream order."""
    _lib.check(_lib_().tamgcn_dropout_advance(_ptr(state), _stream()), 'tamgcn_dropout_advance')


def apply(src, C_, y=None, ycoff=0):
    N, _, T, V = src.x1.shape
    if y is None:
        y = empty(N, C_, T, V, like=src.x1)
    sc = src.c()
    _lib.check(_lib_().tamgcn_apply(C.byref(sc), N, C_, T, V, _ptr(y), y.shape[1], ycoff, _stream()), 'tamgcn_apply')
    return y


# ---------------------------------------------------------------------------
# stem / head of Model
def stem_stats(x5, dout=None, center=None):
    """x5 (N, C, T, V, M) -> partial sums [2][C*V*M][N] for the data_bn finalize (forward: moments; backward with dout)."""
    N, C_, T, V, M = x5.shape
    part = empty(2, C_ * V * M, N, like=x5)
    _lib.check(_lib_().tamgcn_stem_stats(_ptr(x5), _ptr(dout), _ptr(center), N, C_, T, V, M, _ptr(part), _stream()), 'tamgcn_stem_stats')
    return part


def stem_apply(x5, coef, dout=None):
    """forward: (N*M, C, T, V) = c1*x + c0 (permuted);  with dout: dx (N, C, T, V, M) = c1*dout + c2*x + c0."""
    N, C_, T, V, M = x5.shape
    out = empty(N * M, C_, T, V, like=x5) if dout is None else torch.empty_like(x5)
    _lib.check(_lib_().tamgcn_stem_apply(_ptr(x5), _ptr(dout), _ptr(coef), N, C_, T, V, M, _ptr(out), _stream()), 'tamgcn_stem_apply')
    return out


def head_pool_fwd(x, M):
    NM, C_, T, V = x.shape
    pooled = empty(NM // M, C_, like=x)
    _lib.check(_lib_().tamgcn_head_pool_fwd(_ptr(x), NM // M, C_, T, V, M, _ptr(pooled), _stream()), 'tamgcn_head_pool_fwd')
    return pooled


def head_pool_bwd(dpooled, M, T, V):
    N, C_ = dpooled.shape
    dx = empty(N * M, C_, T, V, like=dpooled)
    _lib.check(_lib_().tamgcn_head_pool_bwd(_ptr(dpooled), N, C_, T, V, M, _ptr(dx), _stream()), 'tamgcn_head_pool_bwd')
    return dx


def head_fc_fwd(pooled, W, b):
    N, C_ = pooled.shape
    K = W.shape[0]
    logits = empty(N, K, like=pooled)
    _lib.check(_lib_().tamgcn_head_fc_fwd(_ptr(pooled), _ptr(W), _ptr(b), N, C_, K, _ptr(logits), _stream()), 'tamgcn_head_fc_fwd')
    return logits


def head_fc_grouped(pooled, W, b, G):
    """pooled (G*N, C), W (G, K, C), b (G, K) -> scores (G, N, K): G heads in one launch (score_fuse's layout)."""
    GN, C_ = pooled.shape
    K = W.shape[1]
    scores = empty(G, GN // G, K, like=pooled)
    _lib.check(_lib_().tamgcn_head_fc_grouped(_ptr(pooled), _ptr(W), _ptr(b), G, GN // G, C_, K, _ptr(scores), _stream()), 'tamgcn_head_fc_grouped')
    return scores


def head_fc_bwd(dlogits, pooled, W):
    N, C_ = pooled.shape
    K = W.shape[0]
    dW, db, dpooled = torch.empty_like(W), empty(K, like=W), torch.empty_like(pooled)
    _lib.check(_lib_().tamgcn_head_fc_bwd(_ptr(dlogits), _ptr(pooled), _ptr(W), N, C_, K, _ptr(dW), _ptr(db), _ptr(dpooled), _stream()),
               'tamgcn_head_fc_bwd')
    return dW, db, dpooled


# ---------------------------------------------------------------------------
# input side: skeleton streams, the feeder's per-sample transform
STREAM_MODES = {'joint': 0, 'bone': 1, 'motion': 2, 'joint_motion': 2, 'bone_motion': 3}


def stream_derive(x5, parent, mode):
    """x5 (N, C, T, V, M) joint clips -> the 'bone' / 'motion' / 'bone_motion' stream (same shape); parent int32 [V]."""
    N, C_, T, V, M = x5.shape
    m = STREAM_MODES[mode] if isinstance(mode, str) else int(mode)
    if m == 0:
        return x5
    out = torch.empty_like(x5)
    _lib.check(_lib_().tamgcn_stream_derive(_ptr(x5), N, C_, T, V, M, _ptr(parent), m, _ptr(out), _stream()), 'tamgcn_stream_derive')
    return out


def stem_streams_eval(x5, parent, modes, coef):
    """x5 (N, C, T, V, M) joint clips, parent int32 [V], modes int32 [G] (STREAM_MODES values), coef (G, 3, C*V*M) eval-mode
    data_bn coefficients per model -> (G*N*M, C, T, V): stream_derive + stem_apply of every group in one launch."""
    N, C_, T, V, M = x5.shape
    G = modes.numel()
    if tuple(coef.shape) != (G, 3, C_ * V * M) or parent.numel() != V or parent.dtype != torch.int32 or modes.dtype != torch.int32:
        raise RuntimeError(f'tam_gcn_amd: stem_streams_eval: coef {tuple(coef.shape)} / parent / modes do not fit x {tuple(x5.shape)}, G = {G}')
    out = empty(G * N * M, C_, T, V, like=x5)
    _lib.check(_lib_().tamgcn_stem_streams_eval(_ptr(x5), _ptr(parent), _ptr(modes), _ptr(coef), G, N, C_, T, V, M, _ptr(out), _stream()),
               'tamgcn_stem_streams_eval')
    return out


def feeder_transform(raw, offsets, rot, idx, parent, V, time_steps, center_joint, mode):
    """raw (sum L, V, 3) fp64, offsets int64 [N+1], rot fp64 (N, 3, 3), idx int32 (N, time_steps) -> (N, 3, time_steps, V, 1) fp32."""
    N = offsets.numel() - 1
    m = STREAM_MODES[mode] if isinstance(mode, str) else int(mode)
    out = torch.empty(N, 3, time_steps, V, 1, device=raw.device, dtype=torch.float32)
    _lib.check(_lib_().tamgcn_feeder_transform(_ptr(raw), _ptr(offsets), _ptr(rot), _ptr(idx), _ptr(parent), N, V, time_steps,
                                               center_joint, m, _ptr(out), _stream()), 'tamgcn_feeder_transform')
    return out


def _want(t, name, dtype, shape=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == dtype):
        raise RuntimeError(f'tam_gcn_amd: {name} must be a contiguous {dtype} tensor on the GPU')
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f'tam_gcn_amd: {name} is {tuple(t.shape)}, expected {tuple(shape)}')


def feeder_draw(offsets, clip_ids, state, cossin, time_steps, train, labels=None):
    """The feeder's per-sample draws on the device (tamgcn_feeder_draw, include/tamgcn.h has the stream's definition).
    offsets int64 [n_clips + 1], clip_ids int64 [B] (taken modulo n_clips), state int64 [2] = (seed, call) read on the
    device and, on the train path, advanced by one after the draw; cossin fp64 (121, 2) (None allowed when train is
    false); labels int64 [n_clips] | None.  -> view fp64 (B, 3), rot fp64 (B, 3, 3), idx int32 (B, time_steps),
    labels int64 (B,) | None.  Shapes come from the arguments' shapes only: no host sync, capturable."""
    _want(offsets, 'offsets', torch.int64)
    _want(clip_ids, 'clip_ids', torch.int64)
    _want(state, 'state', torch.int64, (2,))
    n_clips, B = offsets.numel() - 1, clip_ids.numel()
    if offsets.dim() != 1 or clip_ids.dim() != 1:
        raise RuntimeError('tam_gcn_amd: feeder_draw takes 1-D offsets and clip_ids')
    if cossin is not None:
        _want(cossin, 'cossin', torch.float64, (121, 2))
    if labels is not None:
        _want(labels, 'labels', torch.int64, (n_clips,))
    dev = offsets.device
    view = torch.empty(B, 3, device=dev, dtype=torch.float64)
    rot = torch.empty(B, 3, 3, device=dev, dtype=torch.float64)
    idx = torch.empty(B, time_steps, device=dev, dtype=torch.int32)
    lab = torch.empty(B, device=dev, dtype=torch.int64) if labels is not None else None
    _lib.check(_lib_().tamgcn_feeder_draw(_ptr(offsets), n_clips, _ptr(clip_ids), B, _ptr(labels), _ptr(state), _ptr(cossin),
                                          time_steps, int(bool(train)), _ptr(view), _ptr(rot), _ptr(idx), _ptr(lab), _stream()),
               'tamgcn_feeder_draw')
    return view, rot, idx, lab


def feeder_transform_indexed(raw, offsets, clip_ids, rot, idx, parent, V, time_steps, center_joint, mode):
    """feeder_transform reading the resident split: raw (sum L, V, 3) fp64 and offsets int64 [n_clips + 1] of the WHOLE
    split, clip_ids int64 [B] (slot b transforms clip clip_ids[b] % n_clips), rot fp64 (B, 3, 3), idx int32
    (B, time_steps) with every entry inside its clip -> (B, 3, time_steps, V, 1) fp32."""
    _want(offsets, 'offsets', torch.int64)
    _want(clip_ids, 'clip_ids', torch.int64)
    n_clips, B = offsets.numel() - 1, clip_ids.numel()
    _want(raw, 'raw', torch.float64)
    _want(rot, 'rot', torch.float64, (B, 3, 3))
    _want(idx, 'idx', torch.int32, (B, time_steps))
    _want(parent, 'parent', torch.int32, (V,))
    m = STREAM_MODES[mode] if isinstance(mode, str) else int(mode)
    out = torch.empty(B, 3, time_steps, V, 1, device=raw.device, dtype=torch.float32)
    _lib.check(_lib_().tamgcn_feeder_transform_indexed(_ptr(raw), _ptr(offsets), n_clips, _ptr(clip_ids), _ptr(rot), _ptr(idx),
                                                       _ptr(parent), B, V, time_steps, center_joint, m, _ptr(out), _stream()),
               'tamgcn_feeder_transform_indexed')
    return out


# the feeder for fixed-shape arrays (csrc/clipfeeder.hip; include/tamgcn.h has the plan and the draw stream)
CLIP_SHIFT, CLIP_CHOOSE, CLIP_MOVE = 1, 2, 4


def clip_extent(raw):
    """raw (n_clips, C, T, V, M) fp32 resident split -> extent int32 (n_clips, 2) = (first valid frame, last valid frame + 1)."""
    _want(raw, 'raw', torch.float32)
    if raw.dim() != 5 or raw.numel() == 0:
        raise RuntimeError(f'tam_gcn_amd: clip_extent takes a non-empty (n_clips, C, T, V, M) array, got {tuple(raw.shape)}')
    n, C_, T, V, M = raw.shape
    out = torch.empty(n, 2, device=raw.device, dtype=torch.int32)
    _lib.check(_lib_().tamgcn_clip_extent(_ptr(raw), n, C_, T, V, M, _ptr(out), _stream()), 'tamgcn_clip_extent')
    return out


def clip_draw(extent, clip_ids, state, flags, T, W, num_node=0, candidates=None, labels=None):
    """One batch's draws on the device (tamgcn_clip_draw).  extent int32 (n_clips, 2), clip_ids int64 [B] (taken modulo
    n_clips), state int64 [2] = (seed, call) read on the device and advanced by one iff flags != 0; flags = CLIP_SHIFT |
    CLIP_CHOOSE | CLIP_MOVE.  With CLIP_MOVE: num_node nodes and candidates = (angle, scale, trans), three 1-D fp64 tensors.
    -> plan int32 (B, 3), draws int32 (B, 2), move_idx int32 (B, num_node, 4) | None, keys fp64 (B, num_node, 4) | None,
    labels int64 (B,) | None.  No host sync, capturable."""
    _want(extent, 'extent', torch.int32)
    _want(clip_ids, 'clip_ids', torch.int64)
    _want(state, 'state', torch.int64, (2,))
    if extent.dim() != 2 or extent.shape[1] != 2 or clip_ids.dim() != 1:
        raise RuntimeError('tam_gcn_amd: clip_draw takes extent (n_clips, 2) and 1-D clip_ids')
    n_clips, B, dev = extent.shape[0], clip_ids.numel(), extent.device
    if labels is not None:
        _want(labels, 'labels', torch.int64, (n_clips,))
    move_idx = keys = None
    cand, nc = (None, None, None), (0, 0, 0)
    if flags & CLIP_MOVE:
        if candidates is None or len(candidates) != 3:
            raise RuntimeError('tam_gcn_amd: clip_draw with CLIP_MOVE needs candidates = (angle, scale, trans)')
        for t, name in zip(candidates, ('angle candidates', 'scale candidates', 'translation candidates')):
            _want(t, name, torch.float64)
            if t.dim() != 1 or t.numel() < 1:
                raise RuntimeError(f'tam_gcn_amd: {name} must be a non-empty 1-D tensor')
        cand, nc = tuple(candidates), tuple(t.numel() for t in candidates)
        move_idx = torch.empty(B, num_node, 4, device=dev, dtype=torch.int32)
        keys = torch.empty(B, num_node, 4, device=dev, dtype=torch.float64)
    plan = torch.empty(B, 3, device=dev, dtype=torch.int32)
    draws = torch.empty(B, 2, device=dev, dtype=torch.int32)
    lab = torch.empty(B, device=dev, dtype=torch.int64) if labels is not None else None
    _lib.check(_lib_().tamgcn_clip_draw(_ptr(extent), n_clips, _ptr(clip_ids), B, _ptr(labels), _ptr(state), int(flags), T, W, num_node,
                                        nc[0], nc[1], nc[2], _ptr(cand[0]), _ptr(cand[1]), _ptr(cand[2]), _ptr(plan), _ptr(draws),
                                        _ptr(move_idx), _ptr(keys), _ptr(lab), _stream()), 'tamgcn_clip_draw')
    return plan, draws, move_idx, keys, lab


def clip_transform(raw, clip_ids, plan, W, node=None, keys=None):
    """The gather (tamgcn_clip_transform): raw (n_clips, C, T, V, M) fp32, clip_ids int64 [B] (taken modulo n_clips), plan int32
    (B, 3) = (src0, lo, hi); with the move node int32 [num_node] and keys fp64 (B, num_node, 4) -> (B, C, W, V, M) fp32."""
    _want(raw, 'raw', torch.float32)
    _want(clip_ids, 'clip_ids', torch.int64)
    if raw.dim() != 5 or raw.numel() == 0 or clip_ids.dim() != 1:
        raise RuntimeError(f'tam_gcn_amd: clip_transform takes a non-empty (n_clips, C, T, V, M) array and 1-D clip_ids, got {tuple(raw.shape)}')
    n, C_, T, V, M = raw.shape
    B = clip_ids.numel()
    _want(plan, 'plan', torch.int32, (B, 3))
    num_node = 0
    if (node is None) != (keys is None):
        raise RuntimeError('tam_gcn_amd: clip_transform takes node and keys together')
    if node is not None:
        _want(node, 'node', torch.int32)
        num_node = node.numel()
        if node.dim() != 1:
            raise RuntimeError('tam_gcn_amd: node must be 1-D')
        _want(keys, 'keys', torch.float64, (B, num_node, 4))
    out = torch.empty(B, C_, W, V, M, device=raw.device, dtype=torch.float32)
    _lib.check(_lib_().tamgcn_clip_transform(_ptr(raw), n, _ptr(clip_ids), _ptr(plan), _ptr(node), _ptr(keys), num_node, B, C_, T, W, V, M,
                                             _ptr(out), _stream()), 'tamgcn_clip_transform')
    return out


# the same feeder's crop-and-resize mode (include/tamgcn.h has the crop, the rotation and the resize)
CLIP_CROP_RANDOM, CLIP_ROT = 1, 2


def clip_crop_draw(extent, clip_ids, state, flags, p0, p1, min_crop=64, theta=0.3, labels=None):
    """One batch's crops and rotations on the device (tamgcn_clip_crop_draw).  extent int32 (n_clips, 2), clip_ids int64 [B]
    (taken modulo n_clips), state int64 [2] = (seed, call) read on the device and advanced by one iff flags != 0; flags =
    CLIP_CROP_RANDOM | CLIP_ROT; 0 < p0 <= p1 <= 1 (without CLIP_CROP_RANDOM the centre crop of share p0).
    -> crop int32 (B, 2) = (start, L), drawn fp64 (B, 4) = (p, a_x, a_y, a_z), rot fp32 (B, 3, 3) | None, labels int64 (B,) |
    None.  No host sync, capturable."""
    _want(extent, 'extent', torch.int32)
    _want(clip_ids, 'clip_ids', torch.int64)
    _want(state, 'state', torch.int64, (2,))
    if extent.dim() != 2 or extent.shape[1] != 2 or clip_ids.dim() != 1:
        raise RuntimeError('tam_gcn_amd: clip_crop_draw takes extent (n_clips, 2) and 1-D clip_ids')
    n_clips, B, dev = extent.shape[0], clip_ids.numel(), extent.device
    if labels is not None:
        _want(labels, 'labels', torch.int64, (n_clips,))
    crop = torch.empty(B, 2, device=dev, dtype=torch.int32)
    drawn = torch.empty(B, 4, device=dev, dtype=torch.float64)
    rot = torch.empty(B, 3, 3, device=dev, dtype=torch.float32) if flags & CLIP_ROT else None
    lab = torch.empty(B, device=dev, dtype=torch.int64) if labels is not None else None
    _lib.check(_lib_().tamgcn_clip_crop_draw(_ptr(extent), n_clips, _ptr(clip_ids), B, _ptr(labels), _ptr(state), int(flags), float(p0),
                                             float(p1), int(min_crop), float(theta), _ptr(crop), _ptr(drawn), _ptr(rot), _ptr(lab),
                                             _stream()), 'tamgcn_clip_crop_draw')
    return crop, drawn, rot, lab


def clip_resize(raw, clip_ids, crop, W, rot=None):
    """The crop-and-resize gather (tamgcn_clip_resize): raw (n_clips, C, T, V, M) fp32, clip_ids int64 [B] (taken modulo n_clips),
    crop int32 (B, 2) = (start, L) (clamped into the clip), rot fp32 (B, 3, 3) | None (C = 3) -> (B, C, W, V, M) fp32."""
    _want(raw, 'raw', torch.float32)
    _want(clip_ids, 'clip_ids', torch.int64)
    if raw.dim() != 5 or raw.numel() == 0 or clip_ids.dim() != 1:
        raise RuntimeError(f'tam_gcn_amd: clip_resize takes a non-empty (n_clips, C, T, V, M) array and 1-D clip_ids, got {tuple(raw.shape)}')
    n, C_, T, V, M = raw.shape
    B = clip_ids.numel()
    _want(crop, 'crop', torch.int32, (B, 2))
    if rot is not None:
        _want(rot, 'rot', torch.float32, (B, 3, 3))
    out = torch.empty(B, C_, W, V, M, device=raw.device, dtype=torch.float32)
    _lib.check(_lib_().tamgcn_clip_resize(_ptr(raw), n, _ptr(clip_ids), _ptr(crop), _ptr(rot), B, C_, T, W, V, M, _ptr(out), _stream()),
               'tamgcn_clip_resize')
    return out


# live and sliding-window inference (csrc/streaming.hip; include/tamgcn.h has the rings, the plan and every rule): a bank of S
# rings for S live feeds, feed s a ring of its own at s * (P cap R); counts / restart int32 [S] | None.  One ring is a bank of one feed.
STREAM_MAX_TS = 64            # time_steps of window_nucla
STREAM_MAX_K = 4096           # classes of window_vote / score_ema
BANK_MAX_FEEDS = 1024


def _bank_geometry(bank, what):
    """(S, P, cap, R, elem) of a bank tensor: fp64 (S, cap, V, 3) or fp32 (S, C, cap, V, M)."""
    if isinstance(bank, torch.Tensor) and bank.numel():
        if bank.dtype == torch.float64 and bank.dim() == 4 and bank.shape[3] == 3:
            return bank.shape[0], 1, bank.shape[1], bank.shape[2] * 3, 8
        if bank.dtype == torch.float32 and bank.dim() == 5:
            return bank.shape[0], bank.shape[1], bank.shape[2], bank.shape[3] * bank.shape[4], 4
    raise RuntimeError(f'tam_gcn_amd: {what} takes a non-empty fp64 (S, cap, V, 3) or fp32 (S, C, cap, V, M) bank, got '
                       f'{getattr(bank, "dtype", type(bank))} {tuple(getattr(bank, "shape", ()))}')


def _want_plan(plan):
    _want(plan, 'plan', torch.int64)
    if plan.dim() != 2 or plan.shape[1] != 2 or plan.shape[0] < 1:
        raise RuntimeError(f'tam_gcn_amd: plan is {tuple(plan.shape)}, expected (B, 2)')
    return plan.shape[0]


def window_vote(logits, plan, n_frames=None):
    """logits fp32 (B, K), plan int64 (B, 2) -> probs fp32 (B, K) = softmax rows, and with n_frames: frame_scores fp32
    (n_frames, K) = per frame the mean of the valid windows that cover it, frame_label int64 (n_frames,) (-1: uncovered);
    both None without n_frames."""
    _want(logits, 'logits', torch.float32)
    if logits.dim() != 2 or logits.numel() == 0:
        raise RuntimeError(f'tam_gcn_amd: window_vote takes non-empty (B, K) logits, got {tuple(logits.shape)}')
    B, K = logits.shape
    _want(plan, 'plan', torch.int64, (B, 2))
    probs = torch.empty_like(logits)
    fs = fl = None
    if n_frames is not None:
        fs = torch.empty(n_frames, K, device=logits.device, dtype=torch.float32)
        fl = torch.empty(n_frames, device=logits.device, dtype=torch.int64)
    _lib.check(_lib_().tamgcn_window_vote(_ptr(logits), _ptr(plan), B, K, n_frames or 0, _ptr(probs), _ptr(fs), _ptr(fl), _stream()),
               'tamgcn_window_vote')
    return probs, fs, fl


def _want_feeds(S, what, counts=None, restart=None):
    if not 1 <= S <= BANK_MAX_FEEDS:
        raise RuntimeError(f'tam_gcn_amd: {what}: S = {S} feeds outside 1..{BANK_MAX_FEEDS}')
    if counts is not None:
        _want(counts, 'counts', torch.int32, (S,))
    if restart is not None:
        _want(restart, 'restart', torch.int32, (S,))


def bank_push(frames, bank, state, counts=None, restart=None):
    """frames fp64 (S, n, V, 3) into bank fp64 (S, cap, V, 3), or fp32 (S, C, n, V, M) into fp32 (S, C, cap, V, M): feed s takes the
    first min(max(counts[s], 0), n) frames of its slice (all n without counts) at slots (count_s + i) % cap; a feed with
    restart[s] != 0 is forgotten first (count 0).  state int64 (S, 2) = (count, pushes) per feed, read and advanced on the
    device; a feed that takes nothing and is not restarted is not touched.  1 <= n <= cap.  No host sync, capturable."""
    S, P, cap, R, elem = _bank_geometry(bank, 'bank_push')
    _want(bank, 'bank', bank.dtype)
    _want(state, 'state', torch.int64, (S, 2))
    _want_feeds(S, 'bank_push', counts, restart)
    t = 1 if elem == 8 else 2                       # the time axis
    if not isinstance(frames, torch.Tensor) or frames.dim() != bank.dim() or frames.shape[:t] + frames.shape[t + 1:] != bank.shape[:t] + bank.shape[t + 1:]:
        raise RuntimeError(f'tam_gcn_amd: bank_push: frames {tuple(getattr(frames, "shape", ()))} do not fit the bank {tuple(bank.shape)}')
    _want(frames, 'frames', bank.dtype)
    _lib.check(_lib_().tamgcn_bank_push(_ptr(frames), S, frames.shape[t], P, R, elem, _ptr(bank), cap, _ptr(state), _ptr(counts), _ptr(restart),
                                        _stream()), 'tamgcn_bank_push')


def bank_plan(state, cap, B, L, hop, counts=None, rows=None):
    """-> plan int64 (S B, 2): row s B + j is ring_plan's row j on feed s (state int64 (S, 2)); (0, 0) rows for a feed with
    counts[s] <= 0.  rows > S B: that many rows, the tail (0, 0) (a padded last chunk).  No host sync, capturable."""
    _want(state, 'state', torch.int64)
    if state.dim() != 2 or state.shape[1] != 2:
        raise RuntimeError(f'tam_gcn_amd: bank_plan: state is {tuple(state.shape)}, expected (S, 2)')
    S = state.shape[0]
    _want_feeds(S, 'bank_plan', counts)
    rows = S * B if rows is None else rows
    if rows < S * B:
        raise RuntimeError(f'tam_gcn_amd: bank_plan: rows = {rows} below S B = {S * B}')
    plan = torch.empty(rows, 2, device=state.device, dtype=torch.int64)
    if rows > S * B:
        plan[S * B:].zero_()
    _lib.check(_lib_().tamgcn_bank_plan(_ptr(state), _ptr(counts), S, cap, B, L, hop, _ptr(plan), _stream()), 'tamgcn_bank_plan')
    return plan


def _bank_windows(bank, plan, B, what):
    """rows of the plan and of the output: the first S B are built, rows past them (a padded chunk) are zeros."""
    rows = _want_plan(plan)
    S = bank.shape[0]
    _want_feeds(S, what)
    if isinstance(B, bool) or not isinstance(B, int) or B < 1 or rows < S * B:
        raise RuntimeError(f'tam_gcn_amd: {what}: a plan of {rows} rows for S = {S} feeds of B = {B!r} windows')
    return S, rows


def bank_window_nucla(bank, plan, B, parent, time_steps, center_joint, mode):
    """bank fp64 (S, cap, V, 3), plan int64 (rows >= S B, 2), parent int32 [V] -> (rows, 3, time_steps, V, 1) fp32: window w < S B is
    window_nucla's window of plan row w on the ring of feed w // B; rows past S B are zeros."""
    _want(bank, 'bank', torch.float64)
    if bank.dim() != 4 or bank.shape[3] != 3 or bank.numel() == 0:
        raise RuntimeError(f'tam_gcn_amd: bank_window_nucla takes a non-empty (S, cap, V, 3) bank, got {tuple(bank.shape)}')
    S, rows = _bank_windows(bank, plan, B, 'bank_window_nucla')
    cap, V = bank.shape[1], bank.shape[2]
    _want(parent, 'parent', torch.int32, (V,))
    m = STREAM_MODES[mode] if isinstance(mode, str) else int(mode)
    out = torch.empty(rows, 3, time_steps, V, 1, device=bank.device, dtype=torch.float32)
    if rows > S * B:
        out[S * B:].zero_()
    _lib.check(_lib_().tamgcn_bank_window_nucla(_ptr(bank), S, cap, _ptr(plan), B, _ptr(parent), V, time_steps, center_joint, m, _ptr(out),
                                                _stream()), 'tamgcn_bank_window_nucla')
    return out


def bank_window_clip(bank, plan, B, W):
    """bank fp32 (S, C, cap, V, M), plan int64 (rows >= S B, 2) -> (rows, C, W, V, M) fp32: window w < S B is window_clip's window of
    plan row w on the ring of feed w // B; rows past S B are zeros."""
    _want(bank, 'bank', torch.float32)
    if bank.dim() != 5 or bank.numel() == 0:
        raise RuntimeError(f'tam_gcn_amd: bank_window_clip takes a non-empty (S, C, cap, V, M) bank, got {tuple(bank.shape)}')
    S, rows = _bank_windows(bank, plan, B, 'bank_window_clip')
    _, C_, cap, V, M = bank.shape
    out = torch.empty(rows, C_, W, V, M, device=bank.device, dtype=torch.float32)
    if rows > S * B:
        out[S * B:].zero_()
    _lib.check(_lib_().tamgcn_bank_window_clip(_ptr(bank), S, cap, _ptr(plan), B, C_, V, M, W, _ptr(out), _stream()), 'tamgcn_bank_window_clip')
    return out


def bank_ema(probs, plan, beta, ema, seen, restart=None):
    """probs fp32 (S B, K), plan int64 (S B, 2), ema fp64 (S, K) and seen int64 [S] updated in place: per feed, score_ema's update
    for its B windows, oldest first; restart[s] != 0: the feed's average reads as zeros and its seen as 0 first.
    -> out fp32 (S, K), label int64 [S] (-1 before a feed's first valid window), conf fp32 [S], advanced int32 [S] (seen moved)."""
    _want(ema, 'ema', torch.float64)
    if ema.dim() != 2 or ema.numel() == 0:
        raise RuntimeError(f'tam_gcn_amd: bank_ema takes a non-empty (S, K) average, got {tuple(ema.shape)}')
    S, K = ema.shape
    _want_feeds(S, 'bank_ema', None, restart)
    _want(seen, 'seen', torch.int64, (S,))
    _want(probs, 'probs', torch.float32)
    if probs.dim() != 2 or probs.shape[1] != K or probs.shape[0] < S or probs.shape[0] % S:
        raise RuntimeError(f'tam_gcn_amd: bank_ema: probs {tuple(probs.shape)} are not (S B, K) for S = {S}, K = {K}')
    B = probs.shape[0] // S
    _want(plan, 'plan', torch.int64, (S * B, 2))
    dev = probs.device
    out = torch.empty(S, K, device=dev, dtype=torch.float32)
    label = torch.empty(S, device=dev, dtype=torch.int64)
    conf = torch.empty(S, device=dev, dtype=torch.float32)
    advanced = torch.empty(S, device=dev, dtype=torch.int32)
    _lib.check(_lib_().tamgcn_bank_ema(_ptr(probs), _ptr(plan), _ptr(restart), S, B, K, float(beta), _ptr(ema), _ptr(seen), _ptr(out), _ptr(label),
                                       _ptr(conf), _ptr(advanced), _stream()), 'tamgcn_bank_ema')
    return out, label, conf, advanced


# one ring: the bank's ops on views with a leading feed axis of one (RingBank.feed(s) gives such rings)
def _one_feed(t):
    """A ring's tensor as the one-feed bank's (a view); what is no tensor goes on to the bank op's refusal."""
    return t[None] if isinstance(t, torch.Tensor) else t


def ring_push(frames, ring, state):
    """frames fp64 (n, V, 3) into ring fp64 (cap, V, 3), or fp32 (C, n, V, M) into fp32 (C, cap, V, M): slots (count + i) % cap;
    state int64 [2] = (count, pushes), read and advanced on the device.  1 <= n <= cap.  No host sync, capturable."""
    bank_push(_one_feed(frames), _one_feed(ring), _one_feed(state))


def ring_plan(state, cap, B, L, hop):
    """-> plan int64 (B, 2) = (start, L): window j ends (B - 1 - j) hop frames before the newest frame of the ring whose state
    is `state`; (0, 0) where the window starts before frame 0 or is overwritten.  No host sync, capturable."""
    return bank_plan(_one_feed(state), cap, B, L, hop)


def window_nucla(ring, plan, parent, time_steps, center_joint, mode):
    """ring fp64 (cap, V, 3), plan int64 (B, 2), parent int32 [V] -> (B, 3, time_steps, V, 1) fp32: feeder_transform's val path
    on every window (identity view, np.linspace indices), zeros for an invalid one."""
    return bank_window_nucla(_one_feed(ring), plan, _want_plan(plan), parent, time_steps, center_joint, mode)


def window_clip(ring, plan, W):
    """ring fp32 (C, cap, V, M), plan int64 (B, 2) -> (B, C, W, V, M) fp32: clip_resize's linear time-resize of every window
    (no rotation), zeros for an invalid one."""
    return bank_window_clip(_one_feed(ring), plan, _want_plan(plan), W)


def score_ema(probs, plan_row, beta, ema, seen):
    """probs fp32 [K], plan_row int64 [2], ema fp64 [K] and seen int64 [1] updated in place on the device (an invalid window moves
    nothing) -> out fp32 [K] = the average, label int64 [1] (-1 before the first valid window), conf fp32 [1]."""
    out, label, conf, _ = bank_ema(_one_feed(probs), _one_feed(plan_row), beta, _one_feed(ema), seen)
    return out[0], label, conf


def bank_decide(label, conf, advanced, state, threshold, hold, deb, log_rows, log_conf, log_count, restart=None):
    """The debounced decision of every feed and its log (include/tamgcn.h has the rule): label int64 [S], conf fp32 [S], advanced
    int32 [S] (bank_ema's), state int64 (S, 2) (the bank's), deb int64 (S, 3) = (stable, cand, run) updated in place, log_rows
    int64 (capacity, 3) = (feed, frame, label), log_conf fp32 [capacity], log_count int64 [2] = (written, dropped).  Events are
    appended in ascending feed order; a full log drops and counts.  No atomics, no host sync, capturable."""
    _want(label, 'label', torch.int64)
    if label.dim() != 1 or label.numel() == 0:
        raise RuntimeError(f'tam_gcn_amd: bank_decide takes labels [S], got {tuple(label.shape)}')
    S = label.numel()
    _want_feeds(S, 'bank_decide', None, restart)
    _want(conf, 'conf', torch.float32, (S,))
    _want(advanced, 'advanced', torch.int32, (S,))
    _want(state, 'state', torch.int64, (S, 2))
    _want(deb, 'deb', torch.int64, (S, 3))
    _want(log_rows, 'log_rows', torch.int64)
    if log_rows.dim() != 2 or log_rows.shape[1] != 3 or log_rows.shape[0] < 1 or log_rows.shape[0] >= 2 ** 31:
        raise RuntimeError(f'tam_gcn_amd: bank_decide: log_rows is {tuple(log_rows.shape)}, expected (capacity, 3)')
    cap = log_rows.shape[0]
    _want(log_conf, 'log_conf', torch.float32, (cap,))
    _want(log_count, 'log_count', torch.int64, (2,))
    _lib.check(_lib_().tamgcn_bank_decide(_ptr(label), _ptr(conf), _ptr(advanced), _ptr(restart), _ptr(state), S, float(threshold), int(hold),
                                          _ptr(deb), _ptr(log_rows), _ptr(log_conf), _ptr(log_count), cap, _stream()), 'tamgcn_bank_decide')


# ---------------------------------------------------------------------------
# loss of the harness step
def ce_fwd(logits, labels):
    N, K = logits.shape
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    g = torch.empty_like(logits)
    _lib.check(_lib_().tamgcn_ce_fwd(_ptr(logits), _ptr(labels), N, K, _ptr(loss), _ptr(g), _stream()), 'tamgcn_ce_fwd')
    return loss, g


def score_fuse(scores, weights, softmax, labels=None):
    """scores (S, N, K) f32, weights (S,) f32 -> fused (N, K), pred (N,) int64, class_stats (K, 2) int32 | None."""
    S_, N, K = scores.shape
    fused = torch.empty(N, K, device=scores.device, dtype=torch.float32)
    pred = torch.empty(N, device=scores.device, dtype=torch.int64)
    stats = torch.empty(K, 2, device=scores.device, dtype=torch.int32) if labels is not None else None
    _lib.check(_lib_().tamgcn_score_fuse(_ptr(scores), _ptr(weights), S_, N, K, int(bool(softmax)), _ptr(labels), _ptr(fused), _ptr(pred),
                                         _ptr(stats), _stream()), 'tamgcn_score_fuse')
    return fused, pred, stats


EVAL_MAX_TOPK = 4             # include/tamgcn.h TAMGCN_EVAL_MAX_TOPK
EVAL_COUNTS = 4 + EVAL_MAX_TOPK
SWEEP_MAX_ALPHAS = 16         # TAMGCN_SWEEP_MAX_ALPHAS


def eval_accumulate(logits, labels, counts, sums, confusion, topk, index=None, valid=None, scores=None, base=0):
    """One batch into an evaluation state (tamgcn_eval_accumulate, include/tamgcn.h has the state's layout and the rules).
    logits (B, K) fp32, labels (B) int64, index (B) int64 | None, valid int | 0-d / 1-element int32 tensor on the device |
    None (= B), topk a sequence of <= EVAL_MAX_TOPK ints.  One launch on the current stream, no synchronisation."""
    _want(logits, 'logits', torch.float32)
    if logits.dim() != 2:
        raise RuntimeError(f'tam_gcn_amd: eval_accumulate: logits must be (B, K), got {tuple(logits.shape)}')
    B, K = logits.shape
    _want(labels, 'labels', torch.int64, (B,))
    if index is not None:
        _want(index, 'index', torch.int64, (B,))
    _want(counts, 'counts', torch.int64, (EVAL_COUNTS,))
    _want(sums, 'sums', torch.float64, (2,))
    _want(confusion, 'confusion', torch.int32, (K, K))
    num_samples = 0
    if scores is not None:
        _want(scores, 'scores', torch.float32)
        if scores.dim() != 2 or scores.shape[1] != K:
            raise RuntimeError(f'tam_gcn_amd: eval_accumulate: scores must be (num_samples, {K}), got {tuple(scores.shape)}')
        num_samples = scores.shape[0]
    vdev, vhost = None, B
    if isinstance(valid, torch.Tensor):
        _want(valid, 'valid', torch.int32)
        if valid.numel() != 1:
            raise RuntimeError('tam_gcn_amd: eval_accumulate: valid must hold one int32')
        vdev = valid
    elif valid is not None:
        vhost = int(valid)
        if not 0 <= vhost <= B:
            raise RuntimeError(f'tam_gcn_amd: eval_accumulate: valid = {vhost} outside [0, {B}]')
    topk = [int(k) for k in topk]
    if len(topk) > EVAL_MAX_TOPK:
        raise RuntimeError(f'tam_gcn_amd: eval_accumulate: at most {EVAL_MAX_TOPK} top-k entries, got {len(topk)}')
    tk = (C.c_int * max(1, len(topk)))(*topk)
    _lib.check(_lib_().tamgcn_eval_accumulate(_ptr(logits), _ptr(labels), _ptr(index), B, K, vhost, _ptr(vdev), tk, len(topk), int(base),
                                              num_samples, _ptr(counts), _ptr(sums), _ptr(confusion), _ptr(scores), _stream()),
               'tamgcn_eval_accumulate')


def score_sweep(a, b, alphas, labels, softmax):
    """a, b (N, K) fp32, alphas <= SWEEP_MAX_ALPHAS floats, labels (N) int64 -> correct int32 [A] on the device:
    correct[i] = #{n : first arg max of tamgcn_score_fuse's (a, b) fused with weights (1, alphas[i]) == labels[n]}."""
    _want(a, 'a', torch.float32)
    _want(b, 'b', torch.float32, tuple(a.shape))
    if a.dim() != 2:
        raise RuntimeError(f'tam_gcn_amd: score_sweep: scores must be (N, K), got {tuple(a.shape)}')
    N, K = a.shape
    _want(labels, 'labels', torch.int64, (N,))
    alphas = [float(x) for x in alphas]
    if not 1 <= len(alphas) <= SWEEP_MAX_ALPHAS:
        raise RuntimeError(f'tam_gcn_amd: score_sweep: 1 .. {SWEEP_MAX_ALPHAS} alphas per launch, got {len(alphas)}')
    correct = torch.empty(len(alphas), device=a.device, dtype=torch.int32)
    al = (C.c_float * len(alphas))(*alphas)
    _lib.check(_lib_().tamgcn_score_sweep(_ptr(a), _ptr(b), al, len(alphas), N, K, int(bool(softmax)), _ptr(labels), _ptr(correct), _stream()),
               'tamgcn_score_sweep')
    return correct


def ce_bwd(g, dloss):
    N, K = g.shape
    dl = torch.empty_like(g)
    _lib.check(_lib_().tamgcn_ce_bwd(_ptr(g), _ptr(dloss), N, K, _ptr(dl), _stream()), 'tamgcn_ce_bwd')
    return dl


CE_REDUCTIONS = {'mean': 0, 'sum': 1, 'none': 2}          # include/tamgcn.h TAMGCN_CE_*


def ce_opts_fwd(logits, target, weight, ignore_index, label_smoothing, reduction):
    """logits (N, K) fp32; target (N,) int64 class indices or (N, K) fp32 class probabilities; weight (K,) fp32 | None;
    reduction a key of CE_REDUCTIONS -> loss (() or (N,)), g (N, K): tamgcn_ce_opts_fwd, one or two launches on the current
    stream, the workspace from torch's allocator."""
    N, K = logits.shape
    d = _lib.CeDesc()
    d.logits, d.weight = _ptr(logits), _ptr(weight)
    if target.dtype == torch.int64:
        d.labels = _ptr(target)
    else:
        d.probs = _ptr(target)
    d.ignore_index, d.label_smoothing, d.reduction, d.N, d.K = int(ignore_index), float(label_smoothing), CE_REDUCTIONS[reduction], N, K
    nbytes = _lib_().tamgcn_ce_opts_workspace_bytes(C.byref(d))
    if nbytes < 0:
        _lib.check(-1, 'tamgcn_ce_opts_workspace_bytes')
    ws = torch.empty(nbytes // 8, device=logits.device, dtype=torch.float64) if nbytes else None
    loss = torch.empty((N,) if reduction == 'none' else (), device=logits.device, dtype=torch.float32)
    g = torch.empty_like(logits)
    _lib.check(_lib_().tamgcn_ce_opts_fwd(C.byref(d), _ptr(loss), _ptr(g), _ptr(ws), _stream()), 'tamgcn_ce_opts_fwd')
    return loss, g


def ce_opts_bwd_rows(g, dloss):
    """dlogits[n][k] = g[n][k] * dloss[n]"""
    N, K = g.shape
    dl = torch.empty_like(g)
    _lib.check(_lib_().tamgcn_ce_opts_bwd_rows(_ptr(g), _ptr(dloss), N, K, _ptr(dl), _stream()), 'tamgcn_ce_opts_bwd_rows')
    return dl


def _optim_desc(fn, p, g, s0, s1, lr, step, scal, mode, momentum, dampening, nesterov, weight_decay, beta1, beta2, eps):
    for name, t in (('p', p), ('g', g), ('s0', s0), ('s1', s1), ('scal', scal)):
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f'tam_gcn_amd.{fn}: {name} must be fp32')
    if lr.dtype != torch.float32 or step.dtype != torch.int32:
        raise RuntimeError(f'tam_gcn_amd.{fn}: lr must be fp32 and step int32')
    if lr.numel() < 1 or step.numel() < 1 or scal.numel() < 2:
        raise RuntimeError(f'tam_gcn_amd.{fn}: lr and step need 1 element, scal 2')
    if g.numel() != p.numel() or any(t is not None and t.numel() != p.numel() for t in (s0, s1)):
        raise RuntimeError(f'tam_gcn_amd.{fn}: p, g and the state buffers differ in size')
    return _lib.OptimDesc(p.numel(), _ptr(p), _ptr(g), _ptr(s0), _ptr(s1), _ptr(lr), _ptr(step), _ptr(scal),
                          int(mode), int(bool(nesterov)), float(momentum), float(dampening), float(weight_decay), float(eps),
                          float(beta1), float(beta2))


def optim_step(p, g, s0, s1, lr, step, scal, mode, momentum=0.0, dampening=0.0, nesterov=False, weight_decay=0.0,
               beta1=0.9, beta2=0.999, eps=1e-8):
    """One in-place SGD (mode 0) or Adam (mode 1) update of the flat fp32 buffer p from g (tamgcn_optim_step).
    lr: (1,) fp32 and step: (1,) int32 device tensors, read (and step advanced) on the device; scal: (2,) fp32 scratch."""
    d = _optim_desc('optim_step', p, g, s0, s1, lr, step, scal, mode, momentum, dampening, nesterov, weight_decay,
                    beta1, beta2, eps)
    _lib.check(_lib_().tamgcn_optim_step(C.byref(d), _stream()), 'tamgcn_optim_step')


def optim_step_guarded(p, g, s0, s1, lr, step, scal, mode, partial, stat, skipped=None, max_norm=0.0, skip_nonfinite=False,
                       momentum=0.0, dampening=0.0, nesterov=False, weight_decay=0.0, beta1=0.9, beta2=0.999, eps=1e-8):
    """optim_step behind the gradient guard (tamgcn_optim_step_guarded): the L2 norm of g is reduced on the device in fp64,
    the update uses g * min(1, max_norm / (norm + 1e-6)) when max_norm > 0 (g itself keeps its values), and with
    skip_nonfinite a non-finite norm leaves p, s0, s1 and step untouched and advances skipped.
    partial: fp64 scratch, one element per workgroup of the reduction (2048 always suffices); stat: (3,) fp32 out
    [norm before clipping, coefficient, 1/0 finite]; skipped: (1,) int32 counter (needed with skip_nonfinite)."""
    d = _optim_desc('optim_step_guarded', p, g, s0, s1, lr, step, scal, mode, momentum, dampening, nesterov, weight_decay,
                    beta1, beta2, eps)
    if partial.dtype != torch.float64 or stat.dtype != torch.float32 or stat.numel() < 3:
        raise RuntimeError('tam_gcn_amd.optim_step_guarded: partial must be fp64, stat fp32 with 3 elements')
    if skipped is not None and (skipped.dtype != torch.int32 or skipped.numel() < 1):
        raise RuntimeError('tam_gcn_amd.optim_step_guarded: skipped must be int32 with 1 element')
    gd = _lib.GradGuard(float(max_norm), int(bool(skip_nonfinite)), _ptr(partial), partial.numel(), _ptr(stat), _ptr(skipped))
    _lib.check(_lib_().tamgcn_optim_step_guarded(C.byref(d), C.byref(gd), _stream()), 'tamgcn_optim_step_guarded')


# ---------------------------------------------------------------------------------------------------------------
# skeleton guidance (csrc/guidance.hip; tam_gcn_amd/guidance.py)
# ---------------------------------------------------------------------------------------------------------------
def guidance_reduce(h, M):
    """h (N*M, C, T', V) fp32, the block stack's output -> intensity (N, T', V, M), pooled (N, C), minmax (parts, 2): one read of h."""
    _want(h, 'h', torch.float32)
    if h.dim() != 4 or M < 1 or h.shape[0] % M:
        raise RuntimeError(f'tam_gcn_amd.guidance_reduce: h {tuple(h.shape)} is not (N*M, C, T, V) with M = {M}')
    NM, C_, Tp, V = h.shape
    N = NM // M
    parts = _lib_().tamgcn_guidance_parts(N, M, Tp, V)
    if parts < 1:
        raise RuntimeError(f'tam_gcn_amd.guidance_reduce: bad dims N={N} M={M} T={Tp} V={V}')
    intensity = torch.empty(N, Tp, V, M, device=h.device, dtype=torch.float32)
    pooled = torch.empty(N, C_, device=h.device, dtype=torch.float32)
    csum = torch.empty(parts, C_, device=h.device, dtype=torch.float32)
    minmax = torch.empty(parts, 2, device=h.device, dtype=torch.float32)
    _lib.check(_lib_().tamgcn_guidance_reduce(_ptr(h), N, M, C_, Tp, V, _ptr(intensity), _ptr(pooled), _ptr(csum), _ptr(minmax), _stream()),
               'tamgcn_guidance_reduce')
    return intensity, pooled, minmax


def guidance_weights(intensity, minmax, joints, k):
    """intensity (N, T', V, M), minmax (parts, 2) of the same call, joints int32 [J] on the device -> weights (N, J)."""
    _want(intensity, 'intensity', torch.float32)
    _want(minmax, 'minmax', torch.float32)
    _want(joints, 'joints', torch.int32)
    if intensity.dim() != 4 or minmax.dim() != 2 or minmax.shape[1] != 2 or joints.dim() != 1:
        raise RuntimeError('tam_gcn_amd.guidance_weights: intensity (N, T, V, M), minmax (parts, 2), joints (J,)')
    N, Tp, V, M = intensity.shape
    J = joints.numel()
    w = torch.empty(N, J, device=intensity.device, dtype=torch.float32)
    _lib.check(_lib_().tamgcn_guidance_weights(_ptr(intensity), _ptr(minmax), minmax.shape[0], N, Tp, V, M, _ptr(joints), J, int(k), _ptr(w),
                                               _stream()), 'tamgcn_guidance_weights')
    return w


def guidance_apply(weights, rgb, frames, H, W, want_map=False):
    """weights (N, J); rgb None | (N, Crgb, H, W) fp32 -> (rgb * resized map | None, the (N, 1, H, W) map | None)."""
    _want(weights, 'weights', torch.float32)
    if weights.dim() != 2:
        raise RuntimeError('tam_gcn_amd.guidance_apply: weights (N, J)')
    N, J = weights.shape
    out = wmap = None
    Crgb = 0
    if rgb is not None:
        _want(rgb, 'rgb', torch.float32)
        if rgb.dim() != 4 or rgb.shape[0] != N or tuple(rgb.shape[2:]) != (H, W):
            raise RuntimeError(f'tam_gcn_amd.guidance_apply: rgb is {tuple(rgb.shape)}, expected ({N}, Crgb, {H}, {W})')
        Crgb = rgb.shape[1]
        out = torch.empty(N, Crgb, H, W, device=weights.device, dtype=torch.float32)
    if want_map:
        wmap = torch.empty(N, 1, H, W, device=weights.device, dtype=torch.float32)
    _lib.check(_lib_().tamgcn_guidance_apply(_ptr(weights), N, J, int(frames), _ptr(rgb), Crgb, int(H), int(W), _ptr(out), _ptr(wmap), _stream()),
               'tamgcn_guidance_apply')
    return out, wmap
