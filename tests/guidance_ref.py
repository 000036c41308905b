"""float64 numpy restatement of the reference's visual.py:55-87 and models/resnet_gcn_attention.py:85 for any N, M, J, and the
rounding bars the device results (csrc/guidance.hip) are held to.

feature is the extract_feature layout (N, C, T', V, M); `from_h` turns the block stack's (N*M, C, T', V) into it.

DEFECTS are real mistakes one can make restating those lines; `defect=` plants one (tests/test_guidance_ref_cpu.py shows that each
fails the checks; nothing else uses the argument).  'no_tie_break' is a mistake of the KERNEL's rank counting, not of those lines
(a rank that counts larger values only): the stage case ties_t75 must tell it from the rule.

Bars (u = 2^-24; every one is a worst case of correct fp32 arithmetic, none is a measured value):
  intensity   I = sqrt(S), S a sum of C squares: S within (C + 1) u S in any order, the root halves that and rounds once:
              |dI| <= (C + 4) u I, fp64_bars.check with L = C and mag = I.
  pooled      a sum of L = T' V M terms and one division: fp64_bars.check with L = T' V M and mag = mean|h|.
  weights     with E = max over the call of the intensity bar (plus whatever the caller knows the intensities to be off by), min and
              max are within E as well.  f = 255 (I - min) / R, R = max - min: the numerator moves by <= 2 E, the denominator by
              <= 2 E, and f <= 255, so |df| <= 255 * 4 E / (R - 2 E) + 4 u 255 (the three fp32 operations).  That is the intensity
              bar amplified by 255 / R, which is why the inputs must keep R >= max / 4 (`conditioned`).  The mean of the k largest of
              a vector is 1-Lipschitz in the largest element-wise change (every order statistic is), the device adds in fp64 and
              rounds once, and / 127 rounds once:  |dw| <= (|df| + 2 u 255) / 127.  With max == min nothing is normalised:
              |dw| <= (E + 2 u max) / 127.  The person choice compares two means of f, each within |df|: it is a condition on the
              inputs that they differ by >= 100 |df| (or not at all, for a bitwise copy).
  map         the row position src = (y + 0.5) 225 / H - 0.5 in fp32 (two roundings of a number <= 225, one subtraction) is within
              3 u 225 of the exact one; the interpolated profile is continuous and piecewise linear in src, so the value moves by
              <= 3 u 225 * (the largest step between neighbouring rows around src), plus 4 u (|a| + |b|) for the blend itself.
"""
import numpy as np

U = 2.0 ** -24
MAP_ROWS, STRIPE = 225, 45
DEFECTS = ('k_smallest', 'per_sample_minmax', 'person_le', 'align_corners', 'stripe_columns')


def from_h(h, M):
    """(N*M, C, T', V) -> (N, C, T', V, M), Model.extract_feature's permutation"""
    NM, C, T, V = h.shape
    return np.ascontiguousarray(h.reshape(NM // M, M, C, T, V).transpose(0, 2, 3, 4, 1))


def pooled(feature):
    return np.asarray(feature, np.float64).mean((2, 3, 4))


def intensity(feature):
    f = np.asarray(feature, np.float64)
    return np.sqrt((f * f).sum(1))


def normalised(I, defect=None):
    """visual.py:57-59 on the whole call"""
    f = np.abs(np.asarray(I, np.float64))
    if defect == 'per_sample_minmax':
        out = f.copy()
        for n in range(f.shape[0]):
            if f[n].max() - f[n].min() != 0:
                out[n] = 255 * (f[n] - f[n].min()) / (f[n].max() - f[n].min())
        return out
    if f.max() - f.min() != 0:
        f = 255 * (f - f.min()) / (f.max() - f.min())
    return f


def persons(fs, defect=None):
    """visual.py:71-74: (N,) the person index per clip, and the two means (N, 2) (the second is the first when M == 1)"""
    N, T, V, M = fs.shape
    m0 = fs[:, :, :, 0].reshape(N, -1).mean(1)
    m1 = fs[:, :, :, 1].reshape(N, -1).mean(1) if M > 1 else m0
    pick = (m0 <= m1) if defect == 'person_le' else (m0 < m1)
    return np.where((M > 1) & pick, 1, 0), np.stack([m0, m1], 1)


def joint_weights(I, target_joints, k, defect=None):
    """visual.py:57-84 up to the / 127: (N, J)"""
    fs = normalised(I, defect)
    N, T, V, M = fs.shape
    who, _ = persons(fs, defect)
    w = np.zeros((N, len(target_joints)))
    for n in range(N):
        for j, v in enumerate(target_joints):
            if v < V:
                col = np.sort(fs[n, :, v, who[n]])
                top = col[:k] if defect == 'k_smallest' else col[::-1][:k]      # T' <= k: all of them
                w[n, j] = top.mean() / 127.0
                if defect == 'no_tie_break':             # rank = the number of larger values alone: a tie group across k enters whole
                    x = fs[n, :, v, who[n]]
                    rank = (x[None, :] > x[:, None]).sum(1)
                    w[n, j] = x[rank < min(k, T)].sum() / min(k, T) / 127.0
    return w


def stripe_rows(w, frames):
    """(N, 225): the value of every row of the reference's map (all its columns are equal), visual.py:67, 81-82"""
    N, J = w.shape
    rows = np.zeros((N, MAP_ROWS))
    for j in range(J):
        if STRIPE * (j + 1) <= STRIPE * frames and STRIPE * (j + 1) <= MAP_ROWS:
            rows[:, STRIPE * j:STRIPE * (j + 1)] = w[:, j:j + 1]
    return rows


def _src(H, in_size, defect=None):
    y = np.arange(H, dtype=np.float64)
    if defect == 'align_corners':
        return y * ((in_size - 1) / (H - 1) if H > 1 else 0.0)
    return np.maximum((y + 0.5) * in_size / H - 0.5, 0.0)


def _interp(rows, src):
    i0 = np.minimum(np.floor(src).astype(np.int64), rows.shape[-1] - 1)
    i1 = np.minimum(i0 + 1, rows.shape[-1] - 1)
    lam = src - i0
    return (1 - lam) * rows[..., i0] + lam * rows[..., i1]


def weight_map(w, frames, size, defect=None):
    """(N, 1, H, W): F.interpolate(map, size, mode='bilinear', align_corners=False), visual.py:86"""
    H, W = size
    rows = stripe_rows(w, frames)
    if defect == 'stripe_columns':                                   # the stripes written along the map's columns
        Wm = STRIPE * frames
        full = np.zeros((w.shape[0], MAP_ROWS, Wm))
        for j in range(w.shape[1]):
            if STRIPE * (j + 1) <= Wm:
                full[:, :, STRIPE * j:STRIPE * (j + 1)] = w[:, j, None, None]
        a = _interp(full.transpose(0, 2, 1), _src(H, MAP_ROWS)).transpose(0, 2, 1)       # rows
        return _interp(a, _src(W, Wm))[:, None]
    prof = _interp(rows, _src(H, MAP_ROWS, defect))                   # (N, H)
    return np.repeat(prof[:, None, :, None], W, axis=3)


def guidance(feature, rgb, target_joints=(3, 11, 7, 18, 14), k=15, frames=5, defect=None):
    """visual.py:55-87: (weights (N, J), map (N, 1, H, W), rgb * map)"""
    w = joint_weights(intensity(feature), target_joints, k, defect)
    wm = weight_map(w, frames, rgb.shape[-2:], defect)
    return w, wm, np.asarray(rgb, np.float64) * wm


# ---------------------------------------------------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------------------------------------------------
def intensity_bar_max(I, C, extra=0.0):
    """E: the largest intensity error of the call (the L = C rounding bar, plus an error the caller accounts for)"""
    return (C + 4) * U * float(np.max(I)) + extra


def conditioned(I):
    """max - min >= max / 4 (or exactly 0): the normalisation amplifies E by 255 / (max - min)"""
    R = float(np.max(I) - np.min(I))
    return R == 0.0 or R >= float(np.max(I)) / 4


def normalised_bar(I, E):
    R = float(np.max(I) - np.min(I))
    if R == 0.0:
        return E
    assert R > 4 * E
    return 255 * 4 * E / (R - 2 * E) + 4 * U * 255


def weights_bar(I, E):
    top = 255.0 if float(np.max(I) - np.min(I)) != 0.0 else float(np.max(I))
    return (normalised_bar(I, E) + 2 * U * top) / 127.0


def persons_decided(I, E):
    """the person choice of every clip is out of the bar's reach: the means differ by >= 100 bars, or the persons are copies"""
    fs = normalised(I)
    if fs.shape[3] == 1:
        return True
    _, means = persons(fs)
    gap = np.abs(means[:, 0] - means[:, 1])
    copies = np.array([np.array_equal(I[n, :, :, 0], I[n, :, :, 1]) for n in range(I.shape[0])])
    return bool(np.all(copies | (gap >= 100 * normalised_bar(I, E))))


def map_bar(w, frames, H, dw=0.0):
    """(N, H): the bar of every row of the resized map; dw: what the weights themselves may be off by"""
    rows = stripe_rows(w, frames)
    step = np.abs(np.diff(rows, axis=1))                              # (N, 224)
    step = np.concatenate([step[:, :1], step, step[:, -1:]], 1)       # step[i + 1] = |rows[i + 1] - rows[i]|
    src = _src(H, MAP_ROWS)
    i0 = np.minimum(np.floor(src).astype(np.int64), MAP_ROWS - 1)
    near = np.maximum(np.maximum(step[:, i0], step[:, i0 + 1]), step[:, np.minimum(i0 + 2, MAP_ROWS)])
    i1 = np.minimum(i0 + 1, MAP_ROWS - 1)
    # weights off by dw move every row by <= dw and every step by <= 2 dw
    return 3 * U * MAP_ROWS * (near + 2 * dw) + 4 * U * (np.abs(rows[:, i0]) + np.abs(rows[:, i1]) + 2 * dw) + dw
