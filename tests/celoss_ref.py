"""fp64 reference of the cross-entropy with torch's options (tamgcn_ce_opts_fwd, tamgcn_ce_opts_bwd_rows: csrc/celoss.hip) with the
bar every output is held to, the problems the CPU and the GPU tests share, and the planted mistakes the bars must reject.

Semantics (include/tamgcn.h), per row n: logp = l - lse(l), p = softmax(l), w_k the class weight (1 without weights),
Wsum = sum_k w_k, eps = label_smoothing.

    class indices y   a row is KEPT iff y_n != ignore_index (any integer, a valid class id included)
                      L_n = (1 - eps) w_y (-logp_y) + (eps / K) sum_k w_k (-logp_k);   0 on ignored rows
                      dL_n/dl_j = p_j c_n - (1 - eps) w_y [j = y] - (eps / K) w_j,  c_n = (1 - eps) w_y + (eps / K) Wsum;   0 on ignored rows
                      eps = 0 never evaluates the smoothing sum.  'mean' divides by W = sum of w_y over the kept rows.
                      A label outside [0, K) that is not ignore_index: the reduced loss is NaN, with 'none' that row's loss is NaN,
                      that row's gradient is 0, the row counts nothing towards W.
    probabilities t   t' = (1 - eps) t + eps / K;  L_n = -sum_k w_k t'_k logp_k;  dL_n/dl_j = p_j c_n - w_j t'_j,  c_n = sum_k w_k t'_k;
                      'mean' divides by N
    reduction         'none' (N,) L_n;  'sum' sum_n L_n;  'mean' sum_n L_n / W (or N);  g is the gradient for dloss = 1, division included
    backward          dlogits = g * dloss ('mean' / 'sum') or g[n][k] * dloss[n] ('none'): ONE fp32 product, bit-equal

The bars.  Every row's loss is L_n = sum_k a_nk (lse_n - l_nk) with coefficients a_nk >= 0 that add up to c_n, and every row's
gradient is g_nj = (p_nj c_n - a_nj) / D with D = W, N or 1.  The kernel takes the max and e_k = expf(l_k - max) in fp32 as
tamgcn_ce_fwd does and everything after them in fp64 (the shifted sum, its logarithm, p = e / s, the weighted sums, the division)
with one rounding to fp32 at the end, so what separates its result from the fp64 value is expf's error in lse and in p, scaled
by the coefficients they are multiplied with.  It does no more fp32 roundings than tamgcn_ce_fwd, whose bars therefore hold:

    lse     the project's bar of tamgcn_ce_fwd's loss, stemhead_ref.CE_LOSS_BAR = 2e-6 max(1, |loss|), is the bar of ONE lse - l_y term of
            coefficient 1 (c_n = 1, D = kept there), plus 2^-23 max|logit| for shifted logits (the roundings of m + log s and lse - l_y).
            An error d_n of lse_n moves L_n by c_n d_n, so
                row:      tol_n = CE_LOSS_BAR max(c_n, mag_n) + [shifted] 2^-23 max|logit| c_n,          mag_n = sum_k |a_nk| |lse_n - l_nk|
                reduced:  tol   = CE_LOSS_BAR max(cs, mag)    + [shifted] 2^-23 max|logit| cs,   cs = sum_n c_n / D,  mag = sum_n mag_n / D
            (`mag` is the loss's own expression on absolute values, as fp64_bars evaluates it; with default arguments cs = 1 and the bar is
            tamgcn_ce_fwd's).  The final rounding to fp32, 2^-25 |L|, is inside the relative part.
    p       tamgcn_ce_fwd's g = (p - onehot) / kept is held to stemhead_ref.CE_GRAD_BAR = 2e-7 by tests that keep every row of small
            batches: the bar of p's error at coefficient 1 (times the 1 / kept <= 1 it is multiplied with).  Here p is multiplied
            by c_n / D:                          tol_nj = CE_GRAD_BAR c_n / D.
            |g_nj| <= c_n / D (0 <= a_nj <= c_n), so the one final rounding, 2^-25 |g|, is 0.15 of the bar.
    exact   ignored and bad rows of g are bit-zero; ignored rows of a 'none' loss are bit-zero (c_n = mag_n = 0 gives tol_n = 0); all rows
            ignored gives 'sum' exactly 0; K = 1 gives loss 0 and g 0 exactly (lse = l_0, p = 1, and p c - a = c - c);  NaN where NaN
            is due: a bad label (reduced loss, that row of 'none'), 'mean' with W = 0 (no kept row, or kept weights that are all 0);
            with W = 0 the kept rows of g are 0 / 0 or x / 0: not finite.
No bar is taken from an error seen on the GPU: both constants are the project's, the scalings are the formulas' coefficients."""
import collections

import torch

import fp64_bars as B
from stemhead_ref import CE_GRAD_BAR, CE_LOSS_BAR

F64, F32 = torch.float64, torch.float32
REDUCTIONS = ('mean', 'sum', 'none')
# one mistake each (tests/test_celoss_ref_cpu.py plants them): the divisor taken as the kept count; ignored rows given the smoothing
# term; eps / (K - 1); the -(eps / K) w_j term of g dropped; Wsum replaced by K
FAULTS = ('count_divisor', 'ignored_smoothing', 'eps_k_minus_1', 'drop_wj', 'wsum_is_k')

Ref = collections.namedtuple('Ref', 'loss g loss_tol g_tol valid nan_loss w_zero')


# ---------------------------------------------------------------------------------------------------------------------
# the formulas
# ---------------------------------------------------------------------------------------------------------------------
def _softmax_parts(l, dt):
    """lse (N, 1) and p (N, K) by max-shift, in float64.  dt = float32 is the kernel's split: the max and exp(l - max) in fp32
    (one expf each), the sum, the logarithm and the quotient in fp64"""
    l = l.to(dt)
    m = l.max(1, keepdim=True).values
    e = torch.exp(l - m).to(F64)
    s = e.sum(1, keepdim=True)
    return m.to(F64) + torch.log(s), e / s


def ce_opts(p, dt=F64, fault=None):
    """p: logits (N, K) fp32, labels (N,) int64 | probs (N, K) fp32, weight (K,) fp32 | None, ignore_index, eps, reduction, shifted.
    Returns Ref: loss and g in float64 (dt = float32: lse and p taken in fp32 first, what a correct kernel delivers before its
    final rounding), their tolerances, the rows that carry a loss, whether the loss (or which rows of it) must be NaN, whether
    'mean' divides by W = 0."""
    assert fault in (None,) + FAULTS
    l32 = p['logits']
    N, K = (int(s) for s in l32.shape)
    eps, red = float(p['eps']), p['reduction']
    w = torch.ones(K, dtype=F64) if p.get('weight') is None else p['weight'].to(F64)
    lse, pr = _softmax_parts(l32, dt)
    l = l32.to(F64)
    ek = eps / (K - 1) if fault == 'eps_k_minus_1' else eps / K
    om = 1.0 - eps
    zero = torch.zeros((), dtype=F64)
    if p.get('labels') is not None:
        y, ign = p['labels'], int(p['ignore_index'])
        inrange = (y >= 0) & (y < K)
        valid = (y != ign) & inrange
        bad = (y != ign) & ~inrange
        yc = torch.where(valid, y, torch.zeros_like(y))
        vf = valid.to(F64)
        cy = om * w[yc] * vf
        Wsum = float(K) if fault == 'wsum_is_k' else w.sum()
        coef = cy + (ek * Wsum * vf if eps > 0 else 0.0)
        onehot = torch.zeros(N, K, dtype=F64).scatter_(1, yc[:, None], 1.0)
        nly = (lse - l.gather(1, yc[:, None]))[:, 0]
        L = torch.where(valid, cy * nly, zero)
        mag = torch.where(valid, cy.abs() * nly.abs(), zero)
        a = cy[:, None] * onehot
        if eps > 0:                                                         # eps = 0 never forms w_k (lse - l_k)
            sm, sma = (w * (lse - l)).sum(1), (w.abs() * (lse - l).abs()).sum(1)
            L = L + torch.where(valid, ek * sm, zero)
            mag = mag + torch.where(valid, ek * sma, zero)
            if fault != 'drop_wj':
                a = a + ek * w[None, :] * vf[:, None]
        g = pr * coef[:, None] - a
        if fault == 'ignored_smoothing' and eps > 0:
            skipped = (y == ign).to(F64)
            L = L + skipped * ek * sm
            g = g + skipped[:, None] * ek * (pr * Wsum - w[None, :])
        W = vf.sum() if fault == 'count_divisor' else (w[yc] * vf).sum()
    else:
        valid, bad = torch.ones(N, dtype=torch.bool), torch.zeros(N, dtype=torch.bool)
        tp = om * p['probs'].to(F64) + ek
        wt = w * tp
        coef = wt.sum(1)
        L, mag = (wt * (lse - l)).sum(1), (wt.abs() * (lse - l).abs()).sum(1)
        g = pr * coef[:, None] - wt
        W = torch.tensor(float(N), dtype=F64)
    D = W if red == 'mean' else torch.ones((), dtype=F64)
    w_zero = bool(D == 0)
    sh = 2.0 ** -23 * float(l32.abs().max()) if p.get('shifted') else 0.0
    g = g / D                                                               # D = 0: 0 / 0 or x / 0 on the kept rows
    g_tol = CE_GRAD_BAR * coef.abs() / (D if not w_zero else 1.0)
    if red == 'none':
        loss = torch.where(bad, torch.full((), float('nan'), dtype=F64), L)
        loss_tol = CE_LOSS_BAR * torch.maximum(coef.abs(), mag) + sh * coef.abs()
        nan_loss = bad
    else:
        loss = L.sum() / D
        if bool(bad.any()) or w_zero:                                       # W = 0: torch's mean of the w_y terms is 0 / 0 whatever the
            loss = loss * float('nan')                                      # smoothing terms add
        cs, mg = (coef.abs().sum() / D, mag.sum() / D) if not w_zero else (zero, zero)
        loss_tol = CE_LOSS_BAR * torch.maximum(cs, mg) + sh * cs
        nan_loss = bool(bad.any()) or w_zero
    if K == 1:
        loss_tol, g_tol = torch.zeros_like(loss_tol), torch.zeros_like(g_tol)
    return Ref(loss, g, loss_tol, g_tol, valid, nan_loss, w_zero)


def evaluate(p, dt=F32, fault=None):
    """{loss, g} as fp32 tensors: dt = float32 is a correct kernel's result, a `fault` one mistake in it"""
    r = ce_opts(p, dt, fault)
    keep = torch.ones_like(r.valid) if fault == 'ignored_smoothing' else r.valid           # x / 0 on the other rows is still 0
    g = torch.where(keep[:, None], r.g, torch.zeros((), dtype=F64))
    return dict(loss=r.loss.to(F32), g=g.to(F32))


def _ratio(err, tol):
    """max err / tol; a positive error at tol = 0 is infinite"""
    if err.numel() == 0:
        return 0.0
    rat = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return float(torch.nan_to_num(rat, nan=float('inf')).max())


def verify(name, p, got):
    """Hold got = {loss, g} (fp32 tensors from whatever computed them) to the bars.  Returns {output: max err / bound};
    raises fp64_bars.BarError."""
    r = ce_opts(p, F64)
    N, K = (int(s) for s in p['logits'].shape)
    loss, g = got['loss'].detach().cpu(), got['g'].detach().cpu()
    if loss.dtype != F32 or g.dtype != F32 or tuple(loss.shape) != tuple(r.loss.shape) or tuple(g.shape) != (N, K):
        raise B.BarError(f'{name}: loss {loss.dtype} {tuple(loss.shape)}, g {g.dtype} {tuple(g.shape)} vs float32 {tuple(r.loss.shape)}, {(N, K)}')
    out = {}
    # g: exact zeros outside the rows that carry a loss, the coefficient-scaled bar inside
    if bool((g[~r.valid] != 0).any()) or bool(torch.isnan(g[~r.valid]).any()):
        raise B.BarError(f'{name}: g: {int((g[~r.valid] != 0).sum())} non-zero elements on ignored or bad rows')
    gv = g[r.valid].to(F64)
    if r.w_zero:
        if bool(torch.isfinite(gv).any()):
            raise B.BarError(f'{name}: g: finite values on kept rows although the mean divides by W = 0')
    else:
        err, tol = (gv - r.g[r.valid]).abs(), r.g_tol[r.valid][:, None].expand_as(gv)
        if not bool((err <= tol).all()):                                    # NaN fails
            raise B.BarError(f'{name}: g: max err / bound = {_ratio(err, tol):.3g} (bound {CE_GRAD_BAR:.0e} c_n / D)')
        out['g'] = _ratio(err, tol)
    # loss
    lo = loss.to(F64)
    if p['reduction'] == 'none':
        nan = r.nan_loss
        if not bool(torch.isnan(lo[nan]).all()):
            raise B.BarError(f'{name}: loss: a bad row holds a number where NaN is due')
        err = (lo[~nan] - r.loss[~nan]).abs()
        if not bool((err <= r.loss_tol[~nan]).all()):
            i = int(torch.nonzero(~(err <= r.loss_tol[~nan]))[0])
            raise B.BarError(f'{name}: loss: row-level bar: |got - ref| = {float(err[i]):.3g} > {float(r.loss_tol[~nan][i]):.3g}')
        out['loss'] = _ratio(err, r.loss_tol[~nan])
    elif r.nan_loss:
        if not bool(torch.isnan(lo)):
            raise B.BarError(f'{name}: loss: {float(lo)} where NaN is due')
    else:
        err = (lo - r.loss).abs()
        if not bool(err <= r.loss_tol):
            raise B.BarError(f'{name}: loss: |{float(lo):.9g} - {float(r.loss):.9g}| = {float(err):.3g} > {float(r.loss_tol):.3g}')
        out['loss'] = _ratio(err.view(1), r.loss_tol.view(1))
    return out


def verify_bwd(name, reduction, g, dloss, got):
    """dlogits = g * dloss, one fp32 product per element, bit-equal"""
    g, dloss, got = g.detach().cpu(), dloss.detach().cpu(), got.detach().cpu()
    want = g * (dloss[:, None] if reduction == 'none' else dloss)
    if got.dtype != F32 or not torch.equal(got, want):
        raise B.BarError(f'{name}: dlogits: {int((got != want).sum())} elements differ from the fp32 product g * dloss')


# ---------------------------------------------------------------------------------------------------------------------
# problems (CPU tensors from a seed; shared by the CPU and the GPU tests)
# ---------------------------------------------------------------------------------------------------------------------
IGNORES = (-100, 0, 'K+5')
WEIGHTS = (None, 'uniform', 'zeros')
EPSILONS = (0.0, 0.1, 1.0)
# every option combination: 81 over class indices, 27 over probabilities
OPTIONS = [dict(target='index', weight=w, eps=e, reduction=r, ignore=i) for w in WEIGHTS for e in EPSILONS for r in REDUCTIONS for i in IGNORES] + \
          [dict(target='prob', weight=w, eps=e, reduction=r, ignore=-100) for w in WEIGHTS for e in EPSILONS for r in REDUCTIONS]

# (N, K) of the GPU ledger.  K: below, at and above one wave of 64 lanes, several passes of a lane, K = 1 (exact zeros).  N: around
# the 4 rows of a workgroup (1, 3, 4, 5), the 256 threads of the normaliser's and the reducer's row loops (255, 256, 257), and
# the 256 workgroups x 4 rows of one grid pass (1023, 1024, 1025; 2049: a third pass)
K_SWEEP = [(5, K) for K in (1, 2, 3, 10, 60, 63, 64, 65, 130, 400)]
N_SWEEP = [(N, 10) for N in (1, 3, 4, 255, 256, 257)] + [(N, 3) for N in (1023, 1024, 1025, 2049)]
SHAPES = K_SWEEP + N_SWEEP + [(257, 400), (256, 65), (3, 130)]
MAIN_SHAPES = [(5, 10), (257, 10), (5, 65), (3, 130)]                     # every option combination; the others take every fourth


def options_of(shape):
    if shape in MAIN_SHAPES:
        return list(OPTIONS)
    r = (shape[0] + shape[1]) % 4
    return [o for i, o in enumerate(OPTIONS) if i % 4 == r]


_BASE = {}


def _base(N, K):
    """the seeded raw material of shape (N, K), drawn once"""
    if (N, K) not in _BASE:
        g = torch.Generator().manual_seed(1000 * N + K)
        z = torch.randn(N, K, generator=g)
        shifted = z * 3.0 + 60.0
        r = N // 2
        shifted[r] = (torch.linspace(-80.0, 80.0, K) if K > 1 else torch.tensor([80.0]))[torch.randperm(K, generator=g)]
        uni = torch.rand(K, generator=g) * 1.9 + 0.1
        zeros = uni.clone()
        zeros[::3] = 0.0
        _BASE[(N, K)] = dict(plain=z * 3.0, shifted=shifted, y=torch.randint(0, K, (N,), generator=g), skip=torch.rand(N, generator=g) < 0.25,
                             probs=torch.softmax(torch.randn(N, K, generator=g) * 2.0, 1), uniform=uni, zeros=zeros, allzero=torch.zeros(K))
    return _BASE[(N, K)]


def problem(N, K, target='index', weight=None, eps=0.0, reduction='mean', ignore=-100, logits='plain', labels='quarter'):
    """logits: 'plain' N(0, 3^2) | 'shifted' (+60, row N // 2 spanning -80 .. 80).  labels: 'quarter' (about a quarter of the rows
    ignored) | 'bad' (and one label outside [0, K) that is not ignore_index) | 'allign' (every row ignored) | 'valid' (none).
    ignore: an integer or 'K+5'.  weight: None | 'uniform' U(0.1, 2) | 'zeros' (every third weight 0) | 'allzero'."""
    b = _base(N, K)
    ign = K + 5 if ignore == 'K+5' else int(ignore)
    p = dict(logits=b[logits], weight=None if weight is None else b[weight], eps=eps, reduction=reduction, ignore_index=ign,
             shifted=logits == 'shifted')
    if target == 'prob':
        p['probs'] = b['probs']
        return p
    y = b['y'].clone()
    if labels != 'valid':
        y[b['skip']] = ign
    if labels == 'allign':
        y[:] = ign
    if labels == 'bad':
        y[min(2, N - 1)] = K if N % 2 else -1
    p['labels'] = y
    return p


def option_name(o):
    return f"{o['target']}.w={o['weight']}.eps={o['eps']}.{o['reduction']}.ign={o['ignore']}"
