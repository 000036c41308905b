"""numpy restatement of the clip feeder's crop-and-resize mode (tam_gcn_amd/feeder/clip_feeder.py with p_interval=,
csrc/clipfeeder.hip: tamgcn_clip_crop_draw and tamgcn_clip_resize; include/tamgcn.h has the contract): the crop and the
rotation's draws from the device's stream, the matrix in fp64, the resize and the rotation in fp64 on the exact source
position, with the rounding bound of every output element.  Test infrastructure: tests/test_clip_resize_ref_cpu.py holds it to
torch's own interpolate and matmul, tests/test_gpu_clip_resize.py holds the kernels to it."""
import numpy as np

from feeder_draws import philox4x32_10

CROP_RANDOM, ROT = 1, 2
_S32 = np.uint64(32)
EPS = 2.0 ** -24                # one fp32 rounding, relative (round to nearest: half an ulp, 2^-24 of the value at the most)

# The interpolation bound of an element whose exact source position src = (t + 0.5) L / W - 0.5 lies between frames i0 and
# i1 of the crop with values x0 and x1:
#
#     EPS (3 L D + 3 (|x0| + |x1|)),   D = the largest |difference| of neighbouring frames among frames i0 - 1 .. i0 + 2
#                                          (clamped into the crop)
#
# The kernel reaches its src through three fp32 roundings -- of scale = L / W (relative EPS; times t + 0.5 <= W: EPS L at the
# most), of the product scale (t + 0.5) (a value below L: EPS L) and of the subtraction of 0.5 (again below L: EPS L); t + 0.5
# itself is exact.  So its src is off by 3 EPS L at the most.  The interpolant is continuous and piecewise linear in src with
# slope x[i + 1] - x[i] on segment i (0 before the first frame's centre and after the last one's, where both sides clamp), so
# moving src by d moves the value by |d| times the steepest slope on the way: the exact segment's, or, when the rounded src
# falls on the other side of an integer, a neighbouring segment's -- hence D over frames i0 - 1 .. i0 + 2, and 3 EPS L D.
# From its src the kernel takes l1 = src - i0 exactly (src < 2^24 and i0 is its integer part), then rounds l0 = 1 - l1, the
# two products and their sum: three rounded operations on terms of |x0| + |x1| at the most (the rounding of l0 is half of one,
# and is counted into the three) -- 3 EPS (|x0| + |x1|).  The fp32 result IS the rounded sum, so no separate output rounding.
INTERP_SRC_ROUNDINGS = 3
INTERP_BLEND_ROUNDINGS = 3

# The rotation out[c] = R[c][0] y[0] + R[c][1] y[1] + R[c][2] y[2] in fp32 on the kernel's own fp32 R: the interpolation
# bounds b[k] of the y[k] go through |R| -- sum_k |R[c][k]| b[k] -- and the three products and two sums each round once: a
# product by EPS |R[c][k] y[k]|, the first sum by EPS (|p0| + |p1|), the second by EPS (|p0| + |p1| + |p2|) at the most, so
# every |p_k| is rounded three times at the most: 3 EPS sum_k |R[c][k]| (|y[k]| + b[k]), the b[k] inside standing for the
# second-order terms (the kernel's y, not the exact one, is what is multiplied).
ROT_ROUNDINGS = 3

# The device's rot (fp32) against the fp64 matrix of the same angles, in units of 2^-53 on top of the one fp32 rounding
# EPS |R|: a cos / sin is off by e ulp of a value below 1, e 2^-53 absolute (e = 2 on the device, 1 in the host's libm).  An
# entry of Rz Ry is one product of two of them (the other terms multiply an exact 0): 2 e + 1 with its rounding.  An entry of
# (Rz Ry) Rx has two such terms at the most, each that entry times a cos / sin: (2 e + 1) + e + 1 = 3 e + 2 per term, and the
# sum of the two (below 2 in magnitude) rounds by 2 more: 6 e + 6 per side, 18 + 12 = 30, and 2 more for the second-order
# terms and for the fp32 rounding being taken of the device's fp64 value instead of the reference's.
ROT_ULPS = 32
# two fp64 compositions of the same three matrices that differ in summation order or contraction (the restatement against
# torch.matmul): per product level 3 products (2^-53 each, |entries| <= 1) and two sums (below 2: 2^-52 each) = 7, the first
# level's error doubled on its way through the second (two non-zero terms): 21 per side, 42 for both.
MATMUL_ULPS = 42


def _mulhi(w, n):
    return ((w * np.asarray(n, dtype=np.uint64)) >> _S32).astype(np.int64)


def _block(seed, call, B, j):
    slot, zero = np.arange(B, dtype=np.uint64), np.zeros(B, dtype=np.uint64)
    counter = (zero + np.uint64(call & 0xFFFFFFFF), zero + np.uint64((call >> 32) & 0xFFFFFFFF), slot, zero + np.uint64(j))
    return philox4x32_10(counter, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def centre_crop(valid, p):
    """(bias, L) of the one-element interval: trunc((1 - p) valid / 2) in fp64, kept to (valid - 1) // 2 so that L >= 1."""
    bias = min(int((1.0 - float(p)) * valid / 2), (valid - 1) // 2)
    return bias, valid - 2 * bias


def crop_draws(seed, call, extents, flags, p0, p1, min_crop=64, theta=0.3):
    """Slot b of call `call` under `seed` for a clip of extent extents[b] = (begin, end).  -> crop int32 [B, 2] = (start, L),
    drawn fp64 [B, 4] = (p, a_x, a_y, a_z) (angles 0 without ROT)."""
    ext = np.asarray(extents, dtype=np.int64).reshape(-1, 2)
    B = len(ext)
    begin, valid = ext[:, 0], np.maximum(ext[:, 1] - ext[:, 0], 1)
    drawn = np.zeros((B, 4), dtype=np.float64)
    if flags & CROP_RANDOM:
        w = _block(seed, call, B, 0)
        u = w[0].astype(np.float64) * 2.0 ** -32
        p = np.float64(p0) + u * (np.float64(p1) - np.float64(p0))
        L = np.minimum(np.maximum(np.floor(valid.astype(np.float64) * p).astype(np.int64), min_crop), valid)
        bias = _mulhi(w[1], valid - L + 1)
    else:
        p = np.full(B, np.float64(p0))
        bias, L = (np.array(v, dtype=np.int64) for v in zip(*(centre_crop(int(v), p0) for v in valid)))
    drawn[:, 0] = p
    if flags & ROT:
        w = _block(seed, call, B, 1)
        for k in range(3):
            drawn[:, 1 + k] = np.float64(theta) * (2.0 * (w[k].astype(np.float64) * 2.0 ** -32) - 1.0)
    return np.stack([begin + bias, L], axis=1).astype(np.int32), drawn


def _mul3(a, b):
    return [[a[r][0] * b[0][c] + a[r][1] * b[1][c] + a[r][2] * b[2][c] for c in range(3)] for r in range(3)]


def axis_matrices(angles):
    """Rx, Rz, Rz of CTR-GCN's random_rot (feeders/tools.py _rot) for angles = (a_x, a_y, a_z), fp64."""
    ax, ay, az = (np.float64(a) for a in angles)
    one, zero = np.float64(1.0), np.float64(0.0)
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = [[one, zero, zero], [zero, cx, sx], [zero, -sx, cx]]
    ry = [[cy, zero, -sy], [zero, one, zero], [sy, zero, cy]]
    rz = [[cz, sz, zero], [-sz, cz, zero], [zero, zero, one]]
    return rx, ry, rz


def rot_matrix(angles):
    """R = (Rz Ry) Rx in fp64, every entry of a product summed over k = 0, 1, 2 left to right; (3, 3) fp64."""
    rx, ry, rz = axis_matrices(angles)
    return np.array(_mul3(_mul3(rz, ry), rx), dtype=np.float64)


def rot_bound(R64):
    """|device rot - R64| allowed, elementwise."""
    return EPS * np.abs(R64) + ROT_ULPS * 2.0 ** -53


def taps(L, W):
    """The exact source position of every output frame, in integers: src = ((2 t + 1) L - W) / (2 W), clamped at 0.
    -> i0, i1 int64 [W] (frames of the crop), l1 fp64 [W] (the weight of i1; l0 = 1 - l1)."""
    t = np.arange(W, dtype=np.int64)
    num = np.maximum((2 * t + 1) * L - W, 0)
    i0 = np.minimum(num // (2 * W), L - 1)
    i1 = np.minimum(i0 + 1, L - 1)
    l1 = (num - i0 * 2 * W).astype(np.float64) / np.float64(2 * W)
    return i0, i1, l1


def resize(clip, start, L, W, rot=None):
    """clip (C, T, V, M), the crop (start, L) as the kernel clamps it, rot (3, 3) or None (the fp32 matrix the kernel was given)
    -> (out fp64 (C, W, V, M), bound fp64 of the same shape): an fp32 result `got` passes iff |got - out| <= bound."""
    clip = np.asarray(clip, dtype=np.float64)
    C, T, V, M = clip.shape
    L = min(max(int(L), 1), T)
    start = min(max(int(start), 0), T - L)
    x = clip[:, start:start + L]
    i0, i1, l1 = taps(L, W)
    l1 = l1[None, :, None, None]
    x0, x1 = x[:, i0], x[:, i1]
    y = (1.0 - l1) * x0 + l1 * x1
    D = np.zeros_like(y)
    for k in (-1, 0, 1):                                                # segments (i0 + k, i0 + k + 1), clamped into the crop
        a, b = np.clip(i0 + k, 0, L - 1), np.clip(i0 + k + 1, 0, L - 1)
        D = np.maximum(D, np.abs(x[:, b] - x[:, a]))
    bound = EPS * (INTERP_SRC_ROUNDINGS * L * D + INTERP_BLEND_ROUNDINGS * (np.abs(x0) + np.abs(x1)))
    if rot is None:
        return y, bound
    assert C == 3
    R = np.asarray(rot, dtype=np.float64).reshape(3, 3)
    out = np.einsum('ck,ktvm->ctvm', R, y)
    aR = np.abs(R)
    rb = np.einsum('ck,ktvm->ctvm', aR, bound) + ROT_ROUNDINGS * EPS * np.einsum('ck,ktvm->ctvm', aR, np.abs(y) + bound)
    return out, rb


def check(got, want, bound, what='', exact=False):
    """got fp32 against resize()'s (want, bound), NaN-free; exact: bit-equal to want rounded to fp32 instead.  Returns the
    largest error / bound ratio (0.0 where every bound is 0 and met)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert not np.isnan(got).any() and not np.isnan(want).any(), f'{what}: NaN'
    if exact:
        assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32)), f'{what}: not bit-equal'
        return 0.0
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), f'{what}: an element misses its bound by a factor {float((err[err > bound] / np.maximum(bound[err > bound], 1e-300)).max()):.3f}'
    m = bound > 0
    return float((err[m] / bound[m]).max()) if m.any() else 0.0
