"""numpy restatement of the clip feeder (tam_gcn_amd/feeder/clip_feeder.py, csrc/clipfeeder.hip; include/tamgcn.h has the
contract): extents, the plan, the device's draw stream, the move's per-frame parameters and the gather in fp64, with the
rounding bound of every output element.  Test infrastructure: tests/test_clip_feeder_ref_cpu.py holds it to the reference's
recorded outputs (tests/golden/clip_feeder.npz), tests/test_gpu_clip_feeder.py holds the kernels to it."""
import numpy as np

from feeder_draws import philox4x32_10

SHIFT, CHOOSE, MOVE = 1, 2, 4
_S32 = np.uint64(32)

# The bound of a moved element, in units of 2^-53 (A + |t|) with A = (|x| + |y|) |s|.  Both sides start from the same bits
# of a, s, t_x, t_y (np.linspace restated operation for operation, no contraction) and differ from the exact
# cos(a) s x - sin(a) s y + t by: their cos / sin (e ulp of a value below 1: e 2^-53 absolute, times |s| (|x| + |y|)); the
# rounding of cos.s and sin.s; of the two products; of their sum; of the final addition -- (e + 4) A + |t| per side.  The host
# libm is good to 1 ulp, the device's sincos to 2: 5 + 6 = 11, and one more for the second-order terms and for the fp32
# rounding being taken of the device's fp64 value instead of the reference's.  (A side that contracts a product into an FMA
# only loses a term.)
MOVE_ULPS = 12


def default_candidates():
    """angles (degrees), scales, translations of the reference's random_move."""
    angles = np.array([a for a in np.arange(-175.0, 181.0, 5.0) if abs(a) not in (105.0, 110.0)])
    return angles, np.array([0.9, 1.0, 1.1]), np.array([-0.2, -0.1, 0.0, 0.1, 0.2])


def node_table(W, move_time):
    """round_half_even(arange(0, W, W / move_time)) with W appended."""
    return np.append(np.rint(np.arange(0, W, W / float(move_time))).astype(np.int64), W)


def extent(clip):
    """(begin, end) of a clip (C, T, V, M): first valid frame, last valid frame + 1; no valid frame: (0, T)."""
    valid = np.flatnonzero((np.asarray(clip) != 0).any(axis=(0, 2, 3)))
    return (int(valid[0]), int(valid[-1]) + 1) if valid.size else (0, clip.shape[1])


def fixed_offset(T, W):
    """d without random_choose: pad at the front, crop at the centre."""
    return (T - W) // 2 if T > W else 0


def plan(begin, end, T, W, bias, d):
    """output frame t is raw frame src0 + t for lo <= t < hi, zero elsewhere."""
    return d - bias + begin, max(0, bias - d), min(W, bias + (end - begin) - d)


def _mulhi(w, n):
    return ((w * np.uint64(n)) >> _S32).astype(np.int64)


def _block(seed, call, B, j):
    slot, zero = np.arange(B, dtype=np.uint64), np.zeros(B, dtype=np.uint64)
    counter = (zero + np.uint64(call & 0xFFFFFFFF), zero + np.uint64((call >> 32) & 0xFFFFFFFF), slot, zero + np.uint64(j))
    return philox4x32_10(counter, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def device_draws(seed, call, extents, T, W, flags, num_node=0, n_cand=(0, 0, 0)):
    """Slot b of call `call` under `seed` for a clip of extent extents[b] = (begin, end).  -> plan int32 [B, 3], shift int32
    [B, 2] = (bias, d), move int32 [B, num_node, 4] (None without MOVE)."""
    ext = np.asarray(extents, dtype=np.int64).reshape(-1, 2)
    B = len(ext)
    w = _block(seed, call, B, 0)
    begin, size = np.zeros(B, dtype=np.int64), np.full(B, T, dtype=np.int64)
    bias = np.zeros(B, dtype=np.int64)
    if flags & SHIFT:
        begin, size = ext[:, 0], ext[:, 1] - ext[:, 0]
        bias = np.array([int(_mulhi(w[0][b:b + 1], T - size[b] + 1)[0]) for b in range(B)], dtype=np.int64)
    if flags & CHOOSE:
        d = _mulhi(w[1], T - W + 1) if T > W else (-_mulhi(w[1], W - T + 1) if T < W else np.zeros(B, dtype=np.int64))
    else:
        d = np.full(B, fixed_offset(T, W), dtype=np.int64)
    pl = np.stack([d - bias + begin, np.maximum(0, bias - d), np.minimum(W, bias + size - d)], axis=1).astype(np.int32)
    move = None
    if flags & MOVE:
        move = np.zeros((B, num_node, 4), dtype=np.int32)
        for i in range(num_node):
            w = _block(seed, call, B, 1 + i)
            for q, n in enumerate((n_cand[0], n_cand[1], n_cand[2], n_cand[2])):
                move[:, i, q] = _mulhi(w[q], n)
    return pl, np.stack([bias, d], axis=1).astype(np.int32), move


def linspace(start, stop, n):
    """np.linspace(start, stop, n) operation for operation: k * ((stop - start) / (n - 1)) + start, last element stop."""
    if n <= 0:
        return np.zeros(0)
    if n == 1:
        return np.array([np.float64(start)])
    step = (np.float64(stop) - np.float64(start)) / np.float64(n - 1)
    out = np.arange(n, dtype=np.float64) * step + np.float64(start)
    out[-1] = stop
    return out


def move_rows(node, keys):
    """keys [num_node, 4] = (angle in degrees, scale, t_x, t_y) at the nodes -> a (radians), s, t_x, t_y per frame, [W] each."""
    W = int(node[-1])
    rows = np.zeros((4, W))
    for i in range(len(node) - 1):
        n0, n1 = int(node[i]), int(node[i + 1])
        for q in range(4):
            rows[q, n0:n1] = linspace(keys[i, q], keys[i + 1, q], n1 - n0)
    rows[0] = rows[0] * np.pi / 180
    return rows


def apply(clip, pl, W, node=None, keys=None):
    """clip (C, T, V, M) -> (out fp64 (C, W, V, M), bound fp64 of the same shape): an fp32 result `got` passes iff
    |got - out| <= bound.  bound is 0 where the element is a copy or a zero (bit-equal after the fp32 cast) and
    2^-24 |out| + MOVE_ULPS 2^-53 ((|x| + |y|) |s| + |t|) where it was moved."""
    clip = np.asarray(clip, dtype=np.float64)
    C, T, V, M = clip.shape
    src0, lo, hi = (int(v) for v in pl)
    lo, hi = max(lo, 0, -src0), min(hi, W, T - src0)
    out = np.zeros((C, W, V, M))
    if hi > lo:
        out[:, lo:hi] = clip[:, src0 + lo:src0 + hi]
    out = out.astype(np.float32).astype(np.float64)
    bound = np.zeros_like(out)
    if keys is not None:
        a, s, tx, ty = (r[:, None, None] for r in move_rows(node, np.asarray(keys, dtype=np.float64)))
        x, y = out[0].copy(), out[1].copy()
        out[0] = (np.cos(a) * s) * x + (-np.sin(a) * s) * y + tx
        out[1] = (np.sin(a) * s) * x + (np.cos(a) * s) * y + ty
        amp = (np.abs(x) + np.abs(y)) * np.abs(s)
        for c, t in ((0, tx), (1, ty)):
            bound[c] = 2.0 ** -24 * np.abs(out[c]) + MOVE_ULPS * 2.0 ** -53 * (amp + np.abs(t))
    return out, bound


def check(got, want, bound, what=''):
    """got fp32 against apply()'s (want, bound); NaN must sit where NaN is wanted.  Returns the largest error / bound ratio
    over the moved elements (0.0 when there are none)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    exact = bound == 0
    w32 = want.astype(np.float32)
    assert np.array_equal(got[exact].view(np.uint32), w32[exact].view(np.uint32)), f'{what}: copied / zero elements are not bit-equal'
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f'{what}: NaN pattern differs'
    m = ~exact & ~nan
    if not m.any():
        return 0.0
    err = np.abs(got[m].astype(np.float64) - want[m])
    ratio = float((err / bound[m]).max())
    assert ratio <= 1.0, f'{what}: a moved element misses its bound by a factor {ratio:.3f}'
    return ratio


def stream(x, parent, mode):
    """bone / motion / bone_motion of a joint batch (B, C, W, V, M) in fp32, as ops.stream_derive computes them."""
    x = np.asarray(x, dtype=np.float32)
    if mode == 'joint':
        return x
    bone = x - x[:, :, :, np.asarray(parent)]
    if mode == 'bone':
        return bone
    src = x if mode in ('motion', 'joint_motion') else bone
    out = np.zeros_like(x)
    out[:, :, :-1] = src[:, :, 1:] - src[:, :, :-1]
    return out
