"""fp64 references of the row-streaming kernels (csrc/elementwise.hip) and of the BatchNorm finalisers (csrc/bn.hip), one per
ENTRY POINT, with the magnitudes and operation counts of the bars their results are held to (fp64_bars.check).

Conventions of fp64_bars / ctrgc_ref: plain torch on the CPU; an operand is a dict {x1, x2, coef, coff, act} over ctot
channels (fp64_bars.src_value), the kernel reads channels coff .. coff + C of it.  Every function below takes a problem dict
`p` and a dtype and returns {output: Bar}: `val` the output evaluated in that dtype (float64: the reference; float32: what
a correct fp32 implementation delivers), `mag` the same expression on absolute values in float64 (ReLU and masks left out),
`L` the number of fp32 operations behind the prologue (fp64_bars adds 4 for the prologue act(c1*x1 + c2*x2 + c0)), `allow`
an additive allowance (tanh, excluded decisions), `keep` the elements that are checked (None: all), `eq`: the output must be
bit-equal to the float32 evaluation (one correctly rounded fp32 operation, or a select).

Moment slabs are (C, N) here, part[s][c][n] in the kernels: one row (n, c) of T*V elements per slot, never summed over n.
Their L is T*V times the terms per element plus the element's own operations (one exception, where that would pass 4096:
maxpool_bwd below), their mag the row sum of the element magnitudes; for a centred moment sum d * (x - mu) that is |d| * (|x| + |mu|), two terms per element (the subtraction, the fma).

tanh.  Device tanhf is a library routine.  `delta` is the allowance PER TANH, twice its largest measured absolute error
(TANHF_MEASURED below, profiles/ew_bn_bars.txt); through 1 - t^2 it becomes 2 |t| delta |dsum|.  The error of tanh's fp32
argument (the prologue's two roundings, <= 2 * 2^-24 * omag) passes through |tanh'| <= 1 and is carried by `mag`, which
therefore holds omag where the expression holds tanh.

Decisions.  The max-pool gradient decides on prologue values: x > 0, and which candidate of a window is the first maximum.
Where the fp64 margin of a decision (|x|; the gap to another candidate) is below the prologue's rounding bound of the values
compared, the element is left out of the comparison (`keep`), and what it could have received goes into the allowance of
its row's moments.  Candidates whose raw inputs are equal are equal in fp32 and in fp64: such ties stay in, and aten's
first-maximum rule decides them.  verify() fails a case that leaves out more than EXCLUDE_CAP of its elements."""
import collections

import numpy as np
import torch

import fp64_bars as B

F64, F32 = torch.float64, torch.float32
EXCLUDE_CAP = 1e-3
# largest |tanhf(x) - tanh(x)| of the device routine over the tanh arguments of the ledger's cases (measured through
# tamgcn_gcn_tail_fwd, tests/test_gpu_ew_forms.py::test_device_tanhf_error; profiles/ew_bn_bars.txt records the run)
TANHF_MEASURED = 1.0783e-07     # 1.81 * 2^-24, over 180128 arguments in [-2.770, 4.035]
TANHF_FINDING = 2.0 ** -22           # 4 ulp of 1.0: a larger measured error is a finding, the allowance is not widened

Bar = collections.namedtuple('Bar', 'val mag L allow keep eq', defaults=(0.0, None, False))


def lanes(L, vec):
    """row_geo in csrc/elementwise.hip: steps = ceil(L / 4) where the kernel walks float4 groups, else L;
    16 lanes up to 80 steps, 32 up to 160, 64 up to 447, the whole workgroup (256) from 448."""
    steps = (L + 3) // 4 if vec else L
    return 256 if steps >= 448 else 16 if steps <= 80 else 32 if steps <= 160 else 64


def _sv(s, C, dt, absval=False, act=None):
    if act is not None:
        s = dict(s, act=act)
    c0 = s.get('coff', 0)
    return B.src_value(s, dt, absval)[:, c0:c0 + C]


def _rows(x):
    """(N, C, T, V) -> (C, N): the sum of every (n, c) row"""
    return x.sum((2, 3)).t()


def _ch(v, dt=F64, absval=False):
    v = v.to(dt)
    return (v.abs() if absval else v)[None, :, None, None]


def _moment(d, dm, x, mu, k, dt, allow=None):
    """slots sum d and sum d * (x - mu) of one row each: d (dt) the element, dm its magnitude, k its operation count"""
    P = d.shape[2] * d.shape[3]
    xa = x.to(F64).abs() + _ch(mu, absval=True)
    a0 = 0.0 if allow is None else _rows(allow)
    a1 = 0.0 if allow is None else _rows(allow * xa)
    return (Bar(_rows(d), _rows(dm), P + k, a0),
            Bar(_rows(d * (x.to(dt) - _ch(mu, dt))), _rows(dm * xa), 2 * P + k, a1))


# ---------------------------------------------------------------------------------------------------------------------
# unit_gcn tail
# ---------------------------------------------------------------------------------------------------------------------
def gcn_tail_fwd(p, dt=F64, delta=0.0):
    """g = relu(y + tanh(o) + res).  After the prologues: tanhf (library, `allow`), the add of y, the add of res: k = 2
    with res, 1 without."""
    C = p['C']
    v = _sv(p['y'], C, dt) + torch.tanh(_sv(p['o'], C, dt))
    m = _sv(p['y'], C, F64, True) + _sv(p['o'], C, F64, True)
    if p.get('res') is not None:
        v = v + _sv(p['res'], C, dt)
        m = m + _sv(p['res'], C, F64, True)
    return dict(g=Bar(torch.relu(v), m, 2 if p.get('res') is not None else 1, delta))


def gcn_tail_bwd(p, dt=F64, delta=0.0):
    """dsum = dg where g > 0 (a select on the given g: bit-equal); doz = dsum * (1 - tanh(o)^2): t * t, 1 - .., the product:
    k = 3; part[0] = sum doz, part[1] = sum doz * (o_raw - o_save[0][coff + c]) per row."""
    C, o = p['C'], p['o']
    c0 = o.get('coff', 0)
    d = torch.where(p['g'] > 0, p['dg'], torch.zeros(())).to(dt)
    t = torch.tanh(_sv(o, C, dt))
    t64 = torch.tanh(_sv(o, C, F64))
    dm = p['dg'].to(F64).abs()
    z = d * (1 - t * t)
    zm = dm * (1 + t64 * t64 + _sv(o, C, F64, True))     # the argument's rounding: |d| 2 |t| |tanh'| (2 eps omag) <= 4 eps |d| omag
    za = 2 * t64.abs() * delta * dm
    s0, s1 = _moment(z, zm, o['x1'][:, c0:c0 + C], p['o_save'][0, c0:c0 + C], 3, dt, za)
    return dict(dsum=Bar(d, None, 0, eq=True), doz=Bar(z, zm, 3, za), s0=s0, s1=s1)


def gcn_mid_bwd(p, dt=F64, delta=0.0):
    """dyb = dsum - ddiff, dres = dsum + ddiff (one rounding each: bit-equal); slots sum dyb, sum dyb * (y_pre - y_save[0]),
    and with r_pre sum dres, sum dres * (r_pre - r_save[0]).  The summed element carries its one rounding: k = 1."""
    ds, dd = p['dsum'].to(dt), p['ddiff'].to(dt)
    m = p['dsum'].to(F64).abs() + p['ddiff'].to(F64).abs()
    out = dict(dyb=Bar(ds - dd, None, 0, eq=True))
    if p.get('want_dres'):
        out['dres'] = Bar(ds + dd, None, 0, eq=True)
    out['s0'], out['s1'] = _moment(ds - dd, m, p['y_pre'], p['y_save'][0], 1, dt)
    if p.get('r_pre') is not None:
        out['s2'], out['s3'] = _moment(ds + dd, m, p['r_pre'], p['r_save'][0], 1, dt)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# residual add (+ ReLU), its row means / frame means, its backward, apply, tmean
# ---------------------------------------------------------------------------------------------------------------------
def add_act_fwd(p, dt=F64, delta=0.0):
    """out = act(a + res): k = 1 with res, 0 without.  rowmean[n][c] = mean over the row (T*V adds, one division);
    xbar[c][n][v] = mean over t (T adds, the product with 1 / T and that reciprocal's rounding: + 2)."""
    C = p['C']
    v, m, k = _sv(p['a'], C, dt), _sv(p['a'], C, F64, True), 0
    if p.get('res') is not None:
        v, m, k = v + _sv(p['res'], C, dt), m + _sv(p['res'], C, F64, True), 1
    if p.get('relu'):
        v = torch.relu(v)
    T, V = v.shape[2], v.shape[3]
    out = dict(out=Bar(v, m, k))
    if p.get('rowmean'):
        out['rowmean'] = Bar(v.mean((2, 3)), m.mean((2, 3)), T * V + k + 1)
    if p.get('xbar'):
        out['xbar'] = Bar(v.mean(2).permute(1, 0, 2), m.mean(2).permute(1, 0, 2), T + k + 2)
    return out


def add_act_bwd(p, dt=F64, delta=0.0):
    """dz = dout where out > 0 (relu) or dout (a select: bit-equal, k = 0); slots sum dz, sum dz * (a_pre - a_save[0]) (0
    without a_pre), and with r_pre sum dz, sum dz * (r_pre - r_save[0])."""
    d = p['dout'].to(dt)
    if p.get('relu'):
        d = torch.where(p['out'] > 0, d, torch.zeros((), dtype=dt))
    m = p['dout'].to(F64).abs()
    out = {}
    if p.get('want_dz'):
        out['dz'] = Bar(d, None, 0, eq=True)
    zero = torch.zeros_like(p['dout'])
    mu0 = torch.zeros(d.shape[1])
    if p.get('a_pre') is not None:
        out['s0'], out['s1'] = _moment(d, m, p['a_pre'], p['a_save'][0], 0, dt)
    else:
        out['s0'] = _moment(d, m, zero, mu0, 0, dt)[0]
        out['s1'] = Bar(torch.zeros(d.shape[1], d.shape[0], dtype=dt), None, 0, eq=True)      # written, and exactly 0
    if p.get('r_pre') is not None:
        out['s2'], out['s3'] = _moment(d, m, p['r_pre'], p['r_save'][0], 0, dt)
    return out


def apply(p, dt=F64, delta=0.0):
    """y[:, ycoff : ycoff + C] = the prologue's value: k = 0"""
    return dict(y=Bar(_sv(p['src'], p['C'], dt), _sv(p['src'], p['C'], F64, True), 0))


def tmean(p, dt=F64, delta=0.0):
    """xbar[c][n][v] = mean over t: T adds and the division: k = T + 1"""
    C = p['C']
    v, m = _sv(p['src'], C, dt), _sv(p['src'], C, F64, True)
    return dict(xbar=Bar(v.mean(2).permute(1, 0, 2), m.mean(2).permute(1, 0, 2), v.shape[2] + 1))


# ---------------------------------------------------------------------------------------------------------------------
# the pooled branch: windows of three frames th = t * stride - 1 .. + 1 inside [0, T_in)
# ---------------------------------------------------------------------------------------------------------------------
def pool_T_out(T_in, stride):
    return (T_in - 1) // stride + 1


def _windows(T_in, stride):
    return [[tt for tt in (t * stride - 1, t * stride, t * stride + 1) if 0 <= tt < T_in] for t in range(pool_T_out(T_in, stride))]


def _pool(v, stride):
    return torch.stack([v[:, :, w].amax(2) for w in _windows(v.shape[2], stride)], 2)


def maxpool_fwd(p, dt=F64, delta=0.0):
    """y = max over the window (a select: k = 0); slots sum y and sum y^2 per output row (a product and an add per element)"""
    C = p['C']
    y, m = _pool(_sv(p['src'], C, dt), p['stride']), _pool(_sv(p['src'], C, F64, True), p['stride'])
    out = dict(y=Bar(y, m, 0))
    if p.get('stats'):
        P = y.shape[2] * y.shape[3]
        out['s0'], out['s1'] = Bar(_rows(y), _rows(m), P), Bar(_rows(y * y), _rows(m * m), 2 * P)
    return out


def maxpool_post_fwd(p, dt=F64, delta=0.0):
    """y = act(c1 * max + c0 [+ add]) with c1 = coef[0][ycoff + c], c0 = coef[2][ycoff + c]: the fma, the add: k = 2 / 1"""
    C, yc = p['C'], p['ycoff']
    c1, c0 = p['coef'][0, yc:yc + C], p['coef'][2, yc:yc + C]
    v = _ch(c1, dt) * _pool(_sv(p['src'], C, dt), p['stride']) + _ch(c0, dt)
    m = _ch(c1, F64, True) * _pool(_sv(p['src'], C, F64, True), p['stride']) + _ch(c0, F64, True)
    k = 1
    if p.get('add') is not None:
        a = p['add'][:, yc:yc + C]
        v, m, k = v + a.to(dt), m + a.to(F64).abs(), 2
    return dict(y=Bar(torch.relu(v) if p.get('relu') else v, m, k))


def maxpool_bwd(p, dt=F64, delta=0.0, last_max=False):
    """d[th] = sum of gy[t] over the windows t whose FIRST maximum is frame th, where x[th] > 0 (x and gy through their
    prologues): at most three terms, k = 2.  Slots sum d, sum d * (x_raw - src_save[0][coff + c]) per input row.
    last_max = True resolves ties to the last maximum instead (what the teeth test plants)."""
    C, src, gy, stride = p['C'], p['src'], p['gy'], p['stride']
    c0 = src.get('coff', 0)
    x, x64, xm = _sv(src, C, dt), _sv(src, C, F64), _sv(src, C, F64, True)
    g, gm = _sv(gy, C, dt), _sv(gy, C, F64, True)
    T_in = x.shape[2]
    raw = [src['x1'][:, c0:c0 + C]] + ([src['x2'][:, c0:c0 + C]] if src.get('x2') is not None else [])
    bound = 4 * B.EPS32 * xm if src.get('coef') is not None else torch.zeros_like(xm)      # plain values are exact
    excl = (_sv(src, C, F64, act=0).abs() < bound)                                        # the mask x > 0
    d, dm, gall = torch.zeros_like(x), torch.zeros_like(xm), torch.zeros_like(xm)
    for t, w in enumerate(_windows(T_in, stride)):
        xs = x[:, :, w]
        arg = (len(w) - 1 - xs.flip(2).argmax(2)) if last_max else xs.argmax(2)           # torch: the first maximal index
        for j, th in enumerate(w):
            win = (arg == j) & (x[:, :, th] > 0)
            d[:, :, th] += torch.where(win, g[:, :, t], torch.zeros((), dtype=dt))
            dm[:, :, th] += torch.where(win, gm[:, :, t], torch.zeros((), dtype=F64))
            gall[:, :, th] += gm[:, :, t]
            for t2 in w:
                if t2 != th:
                    tie = torch.ones_like(excl[:, :, th])
                    for r in raw:
                        tie &= r[:, :, th] == r[:, :, t2]
                    near = (x64[:, :, th] - x64[:, :, t2]).abs() < bound[:, :, th] + bound[:, :, t2]
                    excl[:, :, th] |= near & ~tie & (x64[:, :, th] > 0)
    keep = ~excl
    lost = torch.where(excl, gall, torch.zeros((), dtype=F64))
    s0, s1 = _moment(d, dm, src['x1'][:, c0:c0 + C], p['src_save'][0, c0:c0 + C], 2, dt, lost)
    P = T_in * x.shape[3]
    if s1.L > B.GLOBAL_MAX_L:
        # A row this long (the no-LDS case: 11000 elements) would leave the order-free bar at ~1e-3 * mag and fp64_bars.check would
        # drop its global bound: no missing term of size mag / P would show.  Such a row has the whole workgroup (lanes() = 256), and
        # every kernel of elementwise.hip adds a row up the same way: each lane its ceil(P / lanes) elements in turn, six xor-shuffle
        # steps inside a wave, then the row's four waves in turn (row_sum).  No partial sum passes through more additions than that
        # depth, so the slot is held to the depth in place of P (the centred moment keeps its two terms per element, both keep the
        # element's k = 2), and with L <= 4096 the global bound applies again.
        depth = -(-P // lanes(P, False)) + 6 + 3
        s0, s1 = s0._replace(L=depth + 2), s1._replace(L=2 * depth + 2)
    return dict(d=Bar(d, dm, 2, 0.0, keep), s0=s0, s1=s1)


KINDS = dict(gcn_tail_fwd=gcn_tail_fwd, gcn_tail_bwd=gcn_tail_bwd, gcn_mid_bwd=gcn_mid_bwd, add_act_fwd=add_act_fwd,
             add_act_bwd=add_act_bwd, apply=apply, tmean=tmean, maxpool_fwd=maxpool_fwd, maxpool_post_fwd=maxpool_post_fwd,
             maxpool_bwd=maxpool_bwd)


def tanh_args(kind, p):
    """the fp32 arguments tanh sees in problem p (None: the kernel has no tanh)"""
    return _sv(p['o'], p['C'], F32).flatten() if kind in ('gcn_tail_fwd', 'gcn_tail_bwd') else None


def evaluate(kind, p, dt=F32):
    return {n: b.val for n, b in KINDS[kind](p, dt).items()}


def ratio(got, bar):
    got = got.detach().to('cpu', F64)
    if bar.keep is not None:
        got = torch.where(bar.keep, got, bar.val)
    lim = B.elementwise_bar(bar.L, bar.mag) + bar.allow
    err = (got - bar.val).abs()
    r = torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return float(torch.nan_to_num(r, nan=float('inf')).max())


def verify(name, kind, p, got, delta=2 * TANHF_MEASURED):
    """Hold the outputs `got` ({name: tensor}, from whatever computed them) of one launch to their bars.  Returns
    {output: max err / bound} (0 for a bit-equal output); raises fp64_bars.BarError."""
    bars = KINDS[kind](p, F64, delta)
    exact = KINDS[kind](p, F32) if any(b.eq for b in bars.values()) else {}
    if set(got) != set(bars):
        raise B.BarError(f'{name}: outputs {sorted(got)} vs {sorted(bars)}')
    rat = {}
    for n, b in bars.items():
        g = got[n].detach().cpu()
        if b.eq:
            want = exact[n].val
            if g.dtype != F32 or g.shape != want.shape or not torch.equal(g, want):
                bad = int((g != want).sum()) if g.shape == want.shape else -1
                raise B.BarError(f'{name}: {n}: {bad} elements differ from the correctly rounded fp32 value')
            rat[n] = 0.0
            continue
        if b.keep is not None:
            out = int((~b.keep).sum())
            if out > EXCLUDE_CAP * b.keep.numel():
                raise B.BarError(f'{name}: {n}: {out} of {b.keep.numel()} decisions too close to call (cap {EXCLUDE_CAP:.1%})')
            if g.shape == b.val.shape:
                g = torch.where(b.keep, g.to(F64), b.val)
        rat[n] = ratio(g, b)
        B.check(f'{name}: {n}', g, b.val, b.mag, b.L, allow=b.allow)
    return rat


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm finalisers (numpy float64 on the fp32 partial sums: exact given them)
# ---------------------------------------------------------------------------------------------------------------------
ULP = 2.0 ** -23
CANCEL = 2.0 ** -50


def _np(t):
    return None if t is None else t.detach().cpu().numpy().astype(np.float64)


def _sums(part, coff, C):
    p = _np(part)[:, coff:coff + C]
    return p[0].sum(-1), p[1].sum(-1), np.abs(p[0]).sum(-1), np.abs(p[1]).sum(-1)


def bn_fwd(d):
    """{output: (ref, tol)} of one forward finalisation.  d: part (2, part_ctot, nparts) / part_coff / count, gamma, beta,
    running_mean, running_var (the values BEFORE the launch), nbt, momentum, eps (Python floats, handed over as fp32),
    training, C.  tol = 2^-23 |ref| + 2^-50 * the magnitude of what cancels in fp64: for what depends on var,
    (s2 / count) |d ref / d var|; for a sum of signed terms, the sum of their magnitudes."""
    C = d['C']
    mom, eps = float(np.float32(d['momentum'])), float(np.float32(d['eps']))
    g = _np(d.get('gamma')) if d.get('gamma') is not None else np.ones(C)
    b = _np(d.get('beta')) if d.get('beta') is not None else np.zeros(C)
    out = {}
    if d['training']:
        cnt = float(d['count'])
        s1, s2, a1, a2 = _sums(d['part'], d.get('part_coff', 0), C)
        mean = s1 / cnt
        var = np.maximum(s2 / cnt - mean * mean, 0.0)
        mcan, vcan = a1 / cnt, a2 / cnt + mean * mean
    else:
        mean, var = _np(d['running_mean']), _np(d['running_var'])
        mcan, vcan = np.zeros(C), np.zeros(C)
    inv = 1.0 / np.sqrt(var + eps)
    dinv = 0.5 * inv ** 3                                   # |d invstd / d var|

    def put(name, ref, cancel):
        out[name] = (ref, ULP * np.abs(ref) + CANCEL * cancel)
    put('c1', g * inv, vcan * np.abs(g) * dinv)
    put('c2', np.zeros(C), np.zeros(C))
    put('c0', b - mean * g * inv, np.abs(b) + np.abs(mean * g * inv) + mcan * np.abs(g) * inv + vcan * np.abs(mean * g) * dinv)
    put('mean', mean, mcan)
    put('invstd', inv, vcan * dinv)
    if d['training']:
        unb = var * cnt / (cnt - 1.0) if cnt > 1.0 else var
        if d.get('running_mean') is not None:
            rm = _np(d['running_mean'])
            put('running_mean', (1.0 - mom) * rm + mom * mean, np.abs(rm) + mom * (np.abs(mean) + mcan))
        if d.get('running_var') is not None:
            rv = _np(d['running_var'])
            put('running_var', (1.0 - mom) * rv + mom * unb, np.abs(rv) + mom * vcan * (cnt / (cnt - 1.0) if cnt > 1.0 else 1.0))
    return out


def bn_bwd(d):
    """{output: (ref, tol)} of one backward finalisation.  d: part / part_coff / count, gamma, save (2, save_ctot) /
    save_coff, training, C.  dbias_conv = c1 s1 + c2 mean count + c0 count cancels to rounding noise in training: its
    tolerance carries the magnitudes of the three terms."""
    C, cnt = d['C'], float(d['count'])
    s1, s2, a1, a2 = _sums(d['part'], d.get('part_coff', 0), C)
    sc = d.get('save_coff', 0)
    sv = _np(d['save'])[:, sc:sc + C]
    mean, inv = sv[0], sv[1]
    g = _np(d.get('gamma')) if d.get('gamma') is not None else np.ones(C)
    dg, a = s2 * inv, g * inv
    c1, c2, c0 = a, np.zeros(C), np.zeros(C)
    c0can = np.zeros(C)
    if d['training']:
        c2 = -a * inv * dg / cnt
        c0 = -a * s1 / cnt - c2 * mean
        c0can = np.abs(a) * a1 / cnt + np.abs(a * inv * inv * mean) * a2 / cnt
    out = {}

    def put(name, ref, cancel):
        out[name] = (ref, ULP * np.abs(ref) + CANCEL * cancel)
    put('c1', c1, 0.0)
    put('c2', c2, np.abs(a * inv * inv) * a2 / cnt)
    put('c0', c0, c0can)
    put('dgamma', dg, a2 * inv)
    put('dbeta', s1, a1)
    put('dbias_conv', c1 * s1 + c2 * (mean * cnt) + c0 * cnt, np.abs(c1) * a1 + np.abs(c2 * mean) * cnt + (np.abs(c0) + c0can) * cnt)
    return out


def bn_check(name, got, ref):
    """got {output: tensor / array of C values}, ref from bn_fwd / bn_bwd; returns {output: max err / tol}"""
    rat = {}
    for n, (r, tol) in ref.items():
        if n not in got:
            continue
        g = _np(got[n]) if torch.is_tensor(got[n]) else np.asarray(got[n], np.float64)
        err = np.abs(g - r)
        bad = ~(err <= tol)
        if bad.any():
            c = int(np.nonzero(bad)[0][0])
            raise B.BarError(f'{name}: {n}: {int(bad.sum())} of {len(r)} channels outside 2^-23 relative; first c = {c}: '
                             f'got {g[c]:.9g} ref {r[c]:.9g} tol {tol[c]:.3g}')
        rat[n] = float(np.max(np.where(tol > 0, err / np.maximum(tol, 1e-300), 0.0)))
    return rat
