"""fp64 reference of the three entry points of csrc/tconv.hip (tamgcn_tconv_fwd / _bwd / _wgrad), stated from the comment on
tamgcn_tconv_desc in include/tamgcn.h, the bars their results are held to, and a mirror of the host planners.

A problem `p` is a plain dict of CPU tensors and ints that mirrors the descriptor:

    N Cb T_in T_out V KT dils stride pool
    src    {x1 (N, ctot, T_in, V), coef [3][ctot] | None, coff, act = 1}    the forward's source
    w      [ (Cb, Cb, KT) per branch ]      bias  [ (Cb,) | None per branch ]
    y0     (N, yctot, T_out, V) what y holds before the launch;  ycoff
    gy     {x1, x2 | None, coef | None, coff, act = 0}  (N, gctot, T_out, V)    the gradient w.r.t. y
    mask   {x1 (N, mctot, T_in, V), coef | None, coff}   center (mctot,) | None   dh0 (N, dctot, T_in, V)   dcoff
    wsrc   the forward's source as tamgcn_tconv_wgrad reads it (d->mask there): {x1, coef | None, coff, act}

Every function evaluates in dtype dt, and with absval=True on magnitudes with ReLU and the mask left out (fp64_bars' `mag`).

ReLU and the mask need no flip allowance: the kernel decides them as fmaf(c1, x, c0) > 0, one rounding of the exact value, and
in float64 c1*x is exact and the addition of c0 rounds without changing the sign, so `c1*x + c0 > 0` in float64 decides
identically provided no fp32 result is subnormal -- min_abs_prologue(p) > 1e-30 is a checked condition of the inputs.  The
mask is therefore always decided in float64, whatever dt is."""
import torch

import fp64_bars as B
from ctrgc_ref import ratio

F64 = torch.float64
MAXB = 6
MAXLB = 512                                  # csrc/tconv.hip: TC_MAXLB


NAN = float('nan')


def _bc(c):
    return c[None, :, None, None]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _f(dt, absval):
    return (lambda t: t.to(dt).abs()) if absval else (lambda t: t.to(dt))


def nbr(p):
    return len(p['dils']) + (1 if p.get('pool') else 0)


def pool3(xv, stride, T_out):
    """max over the frames t*stride - 1 .. t*stride + 1 that exist (MaxPool2d((3,1), (stride,1), (1,0)) of a ReLU'd source)"""
    T_in = xv.shape[2]
    th = torch.arange(T_out) * stride
    out = xv[:, :, th]
    out = torch.maximum(out, xv[:, :, (th - 1).clamp_min(0)])           # th - 1 < 0 re-reads the centre frame
    return torch.maximum(out, xv[:, :, (th + 1).clamp_max(T_in - 1)])


def fwd(p, dt=F64, absval=False):
    """(y, s1, s2): y the whole (N, yctot, T_out, V) output starting from y0; s1 / s2 (N, nbr*Cb) the per-sample,
    per-channel sums of y and y^2 over the written channels (the pooled branch's included when pool is set)."""
    f = _f(dt, absval)
    Cb, KT, s, T_out, src = p['Cb'], p['KT'], p['stride'], p['T_out'], p['src']
    xv = B.src_value(src, dt, absval)
    vals = []
    for b, dil in enumerate(p['dils']):
        c = src['coff'] + b * Cb
        v = B.conv_taps(xv[:, c:c + Cb], f(p['w'][b]), KT, dil, s, (KT - 1) * dil // 2, 1, T_out)
        if p['bias'][b] is not None:
            v = v + _bc(f(p['bias'][b]))
        vals.append(v)
    if p.get('pool'):
        c = src['coff'] + len(p['dils']) * Cb
        vals.append(pool3(xv[:, c:c + Cb], s, T_out))
    val = torch.cat(vals, 1)
    y = f(p['y0']).clone()
    y[:, p['ycoff']:p['ycoff'] + val.shape[1]] = val
    return y, val.sum((2, 3)), (val * val).sum((2, 3))


def bwd(p, dt=F64, absval=False, up_shift=0):
    """(dh, s1, s2): dh the whole (N, dctot, T_in, V) gradient starting from dh0; s1 / s2 (N, nb*Cb) the per-sample sums of d
    and d * (h - center) (magnitudes: d * (|h| + |center|)).  up_shift != 0 plants a fault for the tests of the bars: the
    zero-upsampled gradient that many frames off."""
    f = _f(dt, absval)
    Cb, KT, s, T_in, gy, mk = p['Cb'], p['KT'], p['stride'], p['T_in'], p['gy'], p['mask']
    nb = len(p['dils'])
    gv = B.src_value(dict(gy, act=0), dt, absval)
    vals = []
    for b, dil in enumerate(p['dils']):
        c = gy['coff'] + b * Cb
        Wt = f(p['w'][b]).permute(1, 0, 2).flip(2)                       # [k][m][KT-1-tap]
        pad = (KT - 1) * dil - (KT - 1) * dil // 2
        vals.append(B.conv_taps(gv[:, c:c + Cb], Wt, KT, dil, 1, pad + up_shift, s, T_in))
    val = torch.cat(vals, 1)
    m0 = mk['coff']
    h = f(mk['x1'])[:, m0:m0 + nb * Cb]
    if not absval:
        mv = B.src_value(dict(mk, act=0, x2=None), F64)[:, m0:m0 + nb * Cb]
        val = torch.where(mv > 0, val, torch.zeros((), dtype=dt))
    ctr = _bc(f(p['center'])[m0:m0 + nb * Cb]) if p.get('center') is not None else torch.zeros((), dtype=dt)
    second = val * (h + ctr) if absval else val * (h - ctr)
    dh = f(p['dh0']).clone()
    dh[:, p['dcoff']:p['dcoff'] + nb * Cb] = val
    return dh, val.sum((2, 3)), second.sum((2, 3))


def _cut(s, c, n):
    """channels c .. c + n of an operand dict as an operand of their own"""
    return dict(s, x1=s['x1'][:, c:c + n], x2=None if s.get('x2') is None else s['x2'][:, c:c + n],
                coef=None if s.get('coef') is None else s['coef'][:, c:c + n], coff=0)


def wgrad(p, dt=F64, absval=False):
    """dW (nb, Cb, Cb, KT): fp64_bars.wgrad_eval per branch"""
    Cb, KT, s, gy, x = p['Cb'], p['KT'], p['stride'], p['gy'], p['wsrc']
    out = []
    for b, dil in enumerate(p['dils']):
        out.append(B.wgrad_eval(_cut(dict(gy, act=0), gy['coff'] + b * Cb, Cb), _cut(x, x['coff'] + b * Cb, Cb), Cb, Cb, KT, dil, s,
                                (KT - 1) * dil // 2, dt, absval))
    return torch.stack(out)


def min_abs_prologue(p):
    """min |c1*x + c0| over every operand a ReLU or the mask decides on: the forward's source channels (pool included),
    the backward's mask channels and the weight gradient's source channels"""
    worst = float('inf')
    nb = len(p['dils'])
    for s, n in ((p['src'], nbr(p)), (p['mask'], nb), (p['wsrc'], nb)):
        v = B.src_value(dict(s, act=0, x2=None), F64)[:, s['coff']:s['coff'] + n * p['Cb']]
        worst = min(worst, float(v.abs().min()))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------------------------------------------------
def _chk(rat, name, key, got, ref, mag, L, **kw):
    rat[key] = max(rat.get(key, 0.0), ratio(got, ref, mag, L))
    B.check(f'{name}: {key}', got, ref, mag, L, **kw)


def _moments(rat, name, tag, part, ch0, nch, N, refs, mags, Ls, Cbs, per_sample=True):
    """part [2][ctot][nparts] (NaN where never written) with slots n * (nparts / N) + unit.  Channels ch0 .. ch0 + nch must be
    finite in every slot, everything else the NaN it was; the slots of each sample, and all slots, are held to refs / mags
    (per moment: (N, nch)) at contraction lengths Ls[moment](count) evaluated per block of Cbs channels."""
    part = part.detach().cpu()
    nparts = part.shape[2]
    if nparts % N:
        raise B.BarError(f'{name}: {nparts} moment slots for {N} samples')
    rows = torch.zeros(part.shape, dtype=torch.bool)
    rows[:, ch0:ch0 + nch] = True
    B.check_untouched(f'{name}: {tag} moment slots of other channels', _bits(part), _bits(torch.full_like(part, NAN)), ~rows)
    w = part[:, ch0:ch0 + nch]
    if not bool(torch.isfinite(w).all()):
        bad = torch.nonzero(~torch.isfinite(w))[0].tolist()
        raise B.BarError(f'{name}: {tag} moment slot [moment, channel, slot] = {bad} of a written channel is not finite')
    per = w.double().reshape(2, nch, N, nparts // N).sum(-1).permute(0, 2, 1)          # [2][N][nch]
    for st in (0, 1):
        for lo, hi, Lc, cnt in Cbs:
            sl = slice(lo, hi)
            if per_sample:
                _chk(rat, name, f'{tag}.s{st + 1}.sample', per[st][:, sl], refs[st][:, sl], mags[st][:, sl], Ls[st](Lc, cnt),
                     global_bound=False)
            _chk(rat, name, f'{tag}.s{st + 1}.all', per[st][:, sl].sum(0), refs[st][:, sl].sum(0), mags[st][:, sl].sum(0),
                 Ls[st](Lc, cnt * N), global_bound=False)


def _no_stats(name, part):
    if part is not None:
        part = part.detach().cpu()
        B.check_untouched(f'{name}: moment slots with stats_part = NULL', _bits(part), _bits(torch.full_like(part, NAN)),
                          torch.ones(part.shape, dtype=torch.bool))


def check_fwd(name, p, y, part, stats=True, per_sample=True):
    """y (whole tensor) and part ([2][yctot][nparts], pre-filled with NaN; with stats=False it must still be all NaN) of a
    forward launch against the bars; returns {quantity: worst err / bar}."""
    rat = {}
    Cb, nb, N = p['Cb'], len(p['dils']), p['N']
    L = Cb * p['KT']
    ref, r1, r2 = fwd(p)
    mag, m1, m2 = fwd(p, absval=True)
    c0, c1, c2 = p['ycoff'], p['ycoff'] + nb * Cb, p['ycoff'] + nbr(p) * Cb
    keep = torch.ones(ref.shape, dtype=torch.bool)
    keep[:, c0:c2] = False
    B.check_untouched(f'{name}: y outside the written channels', y, p['y0'], keep)
    yc = y.detach().cpu()
    _chk(rat, name, 'y', yc[:, c0:c1], ref[:, c0:c1], mag[:, c0:c1], L)
    if p.get('pool'):
        _chk(rat, name, 'y.pool', yc[:, c1:c2], ref[:, c1:c2], mag[:, c1:c2], 0)
    if not stats:
        _no_stats(name, part)
        return rat
    cnt = p['T_out'] * p['V']
    blocks = [(0, nb * Cb, L, cnt)] + ([(nb * Cb, nbr(p) * Cb, 0, cnt)] if p.get('pool') else [])
    # sum y: (Lc + 4 + count) eps sum(mag);  sum y^2: (2 (Lc + 4) + 2 + count) eps sum(mag^2); fp64_bars.check adds the 4
    _moments(rat, name, 'fwd', part, c0, nbr(p) * Cb, N, (r1, r2), (m1, m2),
             (lambda Lc, n: Lc + n, lambda Lc, n: 2 * Lc + 6 + n), blocks, per_sample)
    return rat


def check_bwd(name, p, dh, part, stats=True, per_sample=True):
    rat = {}
    Cb, nb, N = p['Cb'], len(p['dils']), p['N']
    L = Cb * p['KT']
    ref, r1, r2 = bwd(p)
    mag, m1, m2 = bwd(p, absval=True)
    c0, c1 = p['dcoff'], p['dcoff'] + nb * Cb
    keep = torch.ones(ref.shape, dtype=torch.bool)
    keep[:, c0:c1] = False
    B.check_untouched(f'{name}: dh outside the written channels', dh, p['dh0'], keep)
    _chk(rat, name, 'dh', dh.detach().cpu()[:, c0:c1], ref[:, c0:c1], mag[:, c0:c1], L)
    if not stats:
        _no_stats(name, part)
        return rat
    cnt = p['T_in'] * p['V']
    # sum d: (Lc + 4 + count) eps sum(mag);  sum d (h - center): (Lc + 6 + count) eps sum(mag (|h| + |center|))
    _moments(rat, name, 'bwd', part, c0, nb * Cb, N, (r1, r2), (m1, m2), (lambda Lc, n: Lc + n, lambda Lc, n: Lc + 2 + n),
             [(0, nb * Cb, L, cnt)], per_sample)
    return rat


_WG_CACHE = {}


def wgrad_ref(p, key=None):
    """(ref, mag) of the weight gradient; cached under `key` (the reference does not depend on nsplit)"""
    if key is None or key not in _WG_CACHE:
        r = wgrad(p), wgrad(p, absval=True)
        if key is None:
            return r
        _WG_CACHE.clear()
        _WG_CACHE[key] = r
    return _WG_CACHE[key]


def check_wgrad(name, p, slabs, reduced=None, key=None):
    """slabs [nsplit][nb][Cb][Cb][KT], pre-filled with NaN: all finite, their float64 sum (and `reduced`, the device reduction
    of them) within the L = N*T_out*V bar"""
    rat = {}
    s = slabs.detach().cpu()
    if not bool(torch.isfinite(s).all()):
        bad = torch.nonzero(~torch.isfinite(s))[0].tolist()
        raise B.BarError(f'{name}: slab element {bad} is not finite ({int((~torch.isfinite(s)).sum())} are not)')
    ref, mag = wgrad_ref(p, key)
    L = p['N'] * p['T_out'] * p['V']
    _chk(rat, name, 'dW', s.double().sum(0), ref, mag, L)
    if reduced is not None:
        _chk(rat, name, 'dW.reduced', reduced.detach().cpu().reshape(ref.shape), ref, mag, L)
    return rat


# ---------------------------------------------------------------------------------------------------------------------
# the host planners of csrc/tconv.hip (tc_plan, tc_split, tw_plan), mirrored: which kernel form and how many moment slots /
# weight-gradient items a shape gets.  tests/test_tconv_ledger_cpu.py holds the mirror to the library's own answers.
# ---------------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def tc_plan(V, Cb, KT, span, stride, T_out):
    if V < 1 or Cb < 16 or (Cb not in (16, 32) and Cb % 64) or KT not in (3, 5) or T_out < 1:
        return None
    Vs, nsl = V, 1
    if V > 32:
        if V % 16:
            return None
        Vs, nsl = 16, V // 16
    Vp = (Vs + 3) & ~3
    BT = min(320 // Vs, T_out)
    while BT >= 1 and ((BT - 1) * stride + span + 1) * Vp > MAXLB:
        BT -= 1
    if BT < 1:
        return None
    mt = 1 if Cb == 16 else 2 if Cb == 32 else 4
    tiles = _cdiv(BT * Vs, 16)
    if _cdiv(tiles, 4) > 5:
        return None
    return dict(BT=BT, Vs=Vs, Vp=Vp, nsl=nsl, mt=mt, mh=Cb // (16 * mt), ct=3 if _cdiv(tiles, 4) <= 3 else 5, ntt=_cdiv(T_out, BT))


def tc_split(pl, N, nby):
    tiles = N * nby * pl['ntt'] * pl['nsl']
    tpw = max(1, min(8, (tiles + 256) // 512, pl['ntt']))
    tpw = max(1, min(tpw, pl['ntt']))
    ngrp = _cdiv(pl['ntt'], tpw)
    pl['tpw'] = _cdiv(pl['ntt'], ngrp)
    pl['ngrp'] = _cdiv(pl['ntt'], pl['tpw'])
    return pl


def tw_plan(V, Cb, KT, span, stride, T_out):
    if V < 1 or (Cb != 16 and Cb % 32) or KT not in (3, 5) or T_out < 1:
        return None
    Vs, nsl = V, 1
    if V > 32:
        if V % 16:
            return None
        Vs, nsl = 16, V // 16
    Vp = (Vs + 3) & ~3
    ktl = 1 if Cb == 16 else 2
    for cap in (320, 512):
        BT = min(max(160 // Vs, 1), T_out)
        while BT >= 1 and ((BT - 1) * stride + span + 1) * Vp > cap:
            BT -= 1
        if BT >= 1 and (BT >= 6 or BT == T_out or cap == 512):
            break
        if cap == 512:
            return None
    LB = ((BT - 1) * stride + span + 1) * Vp
    PG = ((((BT * Vs + 3) & ~3) + 31) & ~31) + 2
    if (PG - 2) // 4 > 64:
        return None
    return dict(BT=BT, LB=LB, Vs=Vs, Vp=Vp, nsl=nsl, ktl=ktl, ntt=_cdiv(T_out, BT))


def plan(case):
    """case = (N, Cb, T_in, V, KT, dils, stride) -> dict(fwd=, bwd=, wgrad= kernel symbols, nparts_fwd, nparts_bwd, max_split,
    tpw_fwd, tpw_bwd), or None where tamgcn_tconv_supported() says 0 or the weight gradient has no tiling"""
    N, Cb, T, V, KT, dils, s = case
    if not 1 <= len(dils) <= MAXB or s not in (1, 2) or T < 1 or any(d < 1 or ((KT - 1) * d) % 2 for d in dils):
        return None
    span, T2 = (KT - 1) * max(dils), (T - 1) // s + 1
    pf, pb, pw = tc_plan(V, Cb, KT, span, s, T2), tc_plan(V, Cb, KT, span, 1, T), tw_plan(V, Cb, KT, span, s, T2)
    if pf is None or pb is None or pw is None:
        return None
    out = {}
    for k, pl, d in (('fwd', pf, 'false'), ('bwd', pb, 'true')):
        tc_split(pl, N, len(dils) * pl['mh'])
        out[k] = f'tconv_kernel<{pl["mt"]}, {pl["ct"]}, {KT}, {d}>'
        out['nparts_' + k] = N * pl['ngrp'] * pl['nsl']
        out['tpw_' + k] = pl['tpw']
        out['plan_' + k] = pl
    out['wgrad'] = f'tconv_wgrad_kernel<{pw["ktl"]}, {pw["ktl"]}, {KT}>'
    out['max_split'] = N * pw['ntt'] * pw['nsl']
    out['plan_wgrad'] = pw
    return out
