"""fp64 references of the stem, head, loss and score-fusion entry points (csrc/stemhead.hip, csrc/evalbody.h), one per ENTRY
POINT, with the magnitudes and operation counts of the bars their results are held to (fp64_bars.check).

Conventions of fp64_bars / ew_ref: plain torch or numpy on the CPU.  Every function takes a problem dict `p` of fp32 / integer
CPU tensors and a dtype and returns {output: Out}: `val` the output evaluated in that dtype (float64: the reference; float32:
what a correct fp32 implementation delivers), `mag` the same expression on absolute values in float64, `L` the number of fp32
operations of the bar (fp64_bars adds 4), and `how` the output is held:

    'bar'   |got - val| <= (L + 4) 2^-24 mag element by element, and fp64_bars' global 2e-6
    'eq'    bit-equal to the float32 evaluation (one correctly rounded operation per step, in the order the header states)
    'abs'   |got - val| <= tol (a number or a tensor): the project's own absolute bars of the loss and the softmax scores
    'nan'   every element NaN
    'zero'  every element exactly 0

The semantics restated (the header comments of stemhead.hip and evalbody.h), j = (m*V + v)*C + c the data_bn feature:

    stem_stats          part[0][j][n] = sum_t a, part[1][j][n] = sum_t a (b - center[j]); forward a = b = x, center = 0;
                        backward a = dout[(n*M+m), c, t, v], b = x[n, c, t, v, m]
    stem_apply          out[(n*M+m), c, t, v] = c1[j] x + c0[j]; backward dx[n, c, t, v, m] = c1[j] dout + c2[j] x + c0[j]
    stem_streams_eval   out[(g*N+n)*M+m, c, t, v] = c1_g[j] stream_{modes[g]}(x) + c0_g[j]; streams: joint, bone x - x[parent],
                        motion x[t+1] - x[t] (0 in the last frame), bone of motion
    head_pool_fwd/bwd   pooled[n][c] = mean over (m, t, v); dx[(n*M+m), c, :, :] = dpooled[n][c] / (M T V)
    head_fc_*           logits = pooled W^T + b; grouped: G heads; dW = dl^T pooled, db = sum_n dl, dpooled = dl W
    ce_fwd              mean over the kept rows (label in [0, K)) of lse - l_y; g = (softmax - onehot) / kept on kept rows, 0 on
                        the others; rows labelled -100 are skipped; any other label outside [0, K) makes the loss NaN; no kept
                        row: NaN
    ce_bwd              dlogits = g * (dloss * 1.0f)
    score_fuse          fused = sum_s w[s] (softmax? scores[s]), f = f + (w * x) with both roundings, pred = first arg max,
                        stats[k] = (correct, total) of the labels in [0, K)"""
import collections

import numpy as np
import torch

import fp64_bars as B

F64, F32 = torch.float64, torch.float32
IGNORE_INDEX = -100
CE_LOSS_BAR, CE_GRAD_BAR = 2e-6, 2e-7                 # tests/test_gpu_primitives.py::test_cross_entropy_against_torch
FUSE_BAR, FUSE_GAP, FUSE_CAP = 2e-6, 1e-5, 0.01       # tests/test_gpu_ensemble.py: the bar, the top-2 gap, the share left out

Out = collections.namedtuple('Out', 'val mag L how tol', defaults=(None, 0, 'bar', None))


def frame_index_f32(tv, V):
    """stem_apply_kernel's frame index, t = (int)(((float)tv + 0.5f) * (1.0f / (float)V)), replayed in numpy float32"""
    tv = np.asarray(tv)
    rV = np.float32(1.0) / np.float32(V)
    return ((tv.astype(np.float32) + np.float32(0.5)) * rV).astype(np.int32)


def _dims(x):
    return tuple(int(s) for s in x.shape)


def _feat(c, C, V, M):
    """a per-feature vector [J] broadcast over x (N, C, T, V, M)"""
    return c.view(M, V, C).permute(2, 1, 0)[None, :, None]


def _rows(t5):
    """(N, C, T, V, M) -> (J, N, T), j = (m*V + v)*C + c"""
    N, C, T, V, M = _dims(t5)
    return t5.permute(4, 3, 1, 0, 2).reshape(C * V * M, N, T)


def _to5(d, N, M):
    """(N*M, C, T, V) -> (N, C, T, V, M)"""
    NM, C, T, V = _dims(d)
    return d.view(N, M, C, T, V).permute(0, 2, 3, 4, 1)


def _to4(t5):
    """(N, C, T, V, M) -> (N*M, C, T, V)"""
    N, C, T, V, M = _dims(t5)
    return t5.permute(0, 4, 1, 2, 3).reshape(N * M, C, T, V)


# ---------------------------------------------------------------------------------------------------------------------
# stem
# ---------------------------------------------------------------------------------------------------------------------
def stem_stats(p, dt=F64):
    """p: x (N, C, T, V, M) [, dout (N*M, C, T, V), center [J]].  s0, s1 (J, N): L = T, the second moment's magnitude
    sum |a| (|b| + |mu|)."""
    x = p['x']
    N, C, T, V, M = _dims(x)
    b, bm = _rows(x.to(dt)), _rows(x.to(F64).abs())
    if p.get('dout') is None:
        a, am, mu, mum = b, bm, 0.0, 0.0
    else:
        d5 = _to5(p['dout'], N, M)
        a, am = _rows(d5.to(dt)), _rows(d5.to(F64).abs())
        mu, mum = p['center'].to(dt)[:, None, None], p['center'].to(F64).abs()[:, None, None]
    return dict(s0=Out(a.sum(2), am.sum(2), T), s1=Out((a * (b - mu)).sum(2), (am * (bm + mum)).sum(2), T))


def stem_apply(p, dt=F64):
    """p: x (N, C, T, V, M), coef (3, J) rows c1, c2, c0 [, dout (N*M, C, T, V)].  One fma (two in the backward): L = 1."""
    x, coef = p['x'], p['coef']
    N, C, T, V, M = _dims(x)
    c = [_feat(coef[r].to(dt), C, V, M) for r in range(3)]
    ca = [_feat(coef[r].to(F64).abs(), C, V, M) for r in range(3)]
    xa = x.to(F64).abs()
    if p.get('dout') is None:
        return dict(out=Out(_to4(c[0] * x.to(dt) + c[2]), _to4(ca[0] * xa + ca[2]), 1))
    d5 = _to5(p['dout'], N, M)
    return dict(dx=Out((c[0] * d5.to(dt) + c[1] * x.to(dt) + c[2]).contiguous(), (ca[0] * d5.to(F64).abs() + ca[1] * xa + ca[2]).contiguous(), 1))


def stream(x, parent, mode, absval=False):
    """the skeleton streams of a joint clip x (N, C, T, V, M): 0 joint, 1 bone, 2 motion, 3 bone of motion"""
    sub = (lambda a, b: a + b) if absval else (lambda a, b: a - b)
    x = x.abs() if absval else x
    par = torch.as_tensor(parent, dtype=torch.long)
    bone = sub(x, x[:, :, :, par]) if mode in (1, 3) else x
    if mode < 2:
        return bone
    d = torch.zeros_like(x)
    d[:, :, :-1] = sub(bone[:, :, 1:], bone[:, :, :-1])
    return d


def stem_streams_eval(p, dt=F64):
    """p: x (N, C, T, V, M), parent [V], modes [G], coef (G, 3, J).  At most three subtractions and the fma: L = 3."""
    x, coef = p['x'], p['coef']
    N, C, T, V, M = _dims(x)
    val, mag = [], []
    for g, mode in enumerate(p['modes']):
        c1, c0 = _feat(coef[g, 0].to(dt), C, V, M), _feat(coef[g, 2].to(dt), C, V, M)
        a1, a0 = _feat(coef[g, 0].to(F64).abs(), C, V, M), _feat(coef[g, 2].to(F64).abs(), C, V, M)
        val.append(_to4(c1 * stream(x.to(dt), p['parent'], mode) + c0))
        mag.append(_to4(a1 * stream(x.to(F64), p['parent'], mode, True) + a0))
    return dict(out=Out(torch.cat(val), torch.cat(mag), 3))


# ---------------------------------------------------------------------------------------------------------------------
# head
# ---------------------------------------------------------------------------------------------------------------------
def pool_fwd(p, dt=F64):
    """p: x (N*M, C, T, V), M.  M T V adds and the division: L = M T V + 1."""
    x, M = p['x'], p['M']
    NM, C, T, V = _dims(x)
    f = lambda t: t.view(NM // M, M, C, T * V).mean((1, 3))                 # noqa: E731
    return dict(pooled=Out(f(x.to(dt)), f(x.to(F64).abs()), M * T * V + 1))


def pool_bwd(p, dt=F64):
    """p: dpooled (N, C), M, T, V.  One division: L = 1."""
    d, M, T, V = p['dpooled'], p['M'], p['T'], p['V']
    N, C = _dims(d)
    v = d.to(dt) / torch.tensor(float(M * T * V), dtype=dt)
    f = lambda t: t[:, None, :, None, None].expand(N, M, C, T, V).reshape(N * M, C, T, V)      # noqa: E731
    return dict(dx=Out(f(v), f((d.to(F64) / float(M * T * V)).abs()), 1))


def fc_fwd(p, dt=F64):
    """p: pooled (N, C), W (K, C), b [K] | None.  C products and the bias: L = C + 1."""
    x, W, b = p['pooled'], p['W'], p.get('b')
    val, mag = x.to(dt) @ W.to(dt).t(), x.to(F64).abs() @ W.to(F64).abs().t()
    if b is not None:
        val, mag = val + b.to(dt), mag + b.to(F64).abs()
    return dict(logits=Out(val, mag, x.shape[1] + 1))


def fc_grouped(p, dt=F64):
    """p: pooled (G*N, C), W (G, K, C), b (G, K) | None -> scores (G, N, K): head g on rows g*N .. (g+1)*N"""
    x, W, b = p['pooled'], p['W'], p.get('b')
    G = W.shape[0]
    f = lambda xx, ww: torch.einsum('gnc,gkc->gnk', xx.view(G, -1, xx.shape[1]), ww)       # noqa: E731
    val, mag = f(x.to(dt), W.to(dt)), f(x.to(F64).abs(), W.to(F64).abs())
    if b is not None:
        val, mag = val + b.to(dt)[:, None], mag + b.to(F64).abs()[:, None]
    return dict(scores=Out(val, mag, x.shape[1] + 1))


def fc_bwd(p, dt=F64):
    """p: dl (N, K), pooled (N, C), W (K, C).  dW, db: L = N; dpooled: L = K."""
    dl, x, W = p['dl'], p['pooled'], p['W']
    N, K = _dims(dl)
    a = lambda t: t.to(F64).abs()                                           # noqa: E731
    return dict(dW=Out(dl.to(dt).t() @ x.to(dt), a(dl).t() @ a(x), N), db=Out(dl.to(dt).sum(0), a(dl).sum(0), N),
                dpooled=Out(dl.to(dt) @ W.to(dt), a(dl) @ a(W), K))


# ---------------------------------------------------------------------------------------------------------------------
# cross-entropy
# ---------------------------------------------------------------------------------------------------------------------
def ce_rows(labels, K):
    """(kept, bad) row masks: a label in [0, K); any other label than ignore_index"""
    kept = (labels >= 0) & (labels < K)
    return kept, ~kept & (labels != IGNORE_INDEX)


def ce_fwd(p, dt=F64):
    """p: logits (N, K) fp32, labels [N] int64, shifted (bool: logits far from 0).  The reference is taken on the fp32 logits.
    loss: 2e-6 max(1, |ref|), and for shifted logits + 2^-23 max|logit| (the roundings of m + log s and of lse - l_y, each
    half an ulp of a number of that size); g: 2e-7.  `mag` of the loss is max|logit|."""
    l, y = p['logits'].to(dt), p['labels']
    N, K = _dims(l)
    kept, bad = ce_rows(y, K)
    nk = int(kept.sum())
    m = l.max(1, keepdim=True).values
    e = torch.exp(l - m)
    s = e.sum(1, keepdim=True)
    lse = (m + torch.log(s))[:, 0]
    yc = torch.where(kept, y, torch.zeros_like(y))
    term = lse - l.gather(1, yc[:, None])[:, 0]
    onehot = torch.zeros_like(l).scatter_(1, yc[:, None], 1.0)
    g = torch.where(kept[:, None], (e / s - onehot) * (torch.tensor(1.0, dtype=dt) / max(nk, 1)), torch.zeros((), dtype=dt))
    lmax = float(p['logits'].abs().max())
    if nk == 0 or bool(bad.any()):
        loss = Out(torch.full((), float('nan'), dtype=dt), lmax, 0, 'nan')
    else:
        val = (term[kept].to(F64).sum() / nk).to(dt)                         # the terms are summed in fp64, as the header says
        tol = CE_LOSS_BAR * max(1.0, abs(float(val))) + (2.0 ** -23 * lmax if p.get('shifted') else 0.0)
        loss = Out(val, lmax, 0, 'zero' if K == 1 else 'abs', tol)           # K = 1: lse = l_y and softmax = 1, exactly
    gout = Out(g, None, 0, 'zero') if nk == 0 or K == 1 else Out(g, None, 0, 'abs', CE_GRAD_BAR)
    return dict(loss=loss, g=gout)


def ce_extra(name, p, got):
    """what does not depend on expf's accuracy: every kept row's gradient sums to 0 within (2K + 4) 2^-24 / kept (K roundings
    of the shifted sum, K of the quotients' sum, the reciprocal, the products), every other row is exactly 0"""
    y = p['labels']
    N, K = _dims(p['logits'])
    kept, _ = ce_rows(y, K)
    g = got['g'].detach().cpu()
    if bool(torch.isnan(g).any()):
        raise B.BarError(f'{name}: NaN in g')
    if bool((g[~kept] != 0).any()):
        raise B.BarError(f'{name}: {int((g[~kept] != 0).sum())} non-zero gradient elements on ignored or bad rows')
    nk = int(kept.sum())
    if nk == 0:
        return {}
    rs = (g[kept].to(F64).sum(1) * nk).abs()
    lim = (2 * K + 4) * B.EPS32
    if not bool((rs <= lim).all()):
        raise B.BarError(f'{name}: a kept row of g sums to {float(rs.max()):.3g} / kept, bound {lim:.3g} / kept')
    return dict(rowsum=float(rs.max()) / lim)


def ce_bwd(p, dt=F64):
    """p: g (N, K), dloss ().  One product: bit-equal."""
    return dict(dlogits=Out(p['g'].to(dt) * p['dloss'].to(dt), None, 0, 'eq'))


# ---------------------------------------------------------------------------------------------------------------------
# score fusion
# ---------------------------------------------------------------------------------------------------------------------
def first_argmax(f, last=False):
    a = f.detach().cpu().numpy()
    if last:
        return torch.from_numpy(a.shape[1] - 1 - np.argmax(a[:, ::-1], axis=1)).long()
    return torch.from_numpy(np.argmax(a, axis=1)).long()                    # numpy: the first occurrence


def class_stats(pred, labels, K):
    """(K, 2) int32: (correct, total) of the labels in [0, K)"""
    st = torch.zeros(K, 2, dtype=torch.int32)
    for n in range(labels.numel()):
        l = int(labels[n])
        if 0 <= l < K:
            st[l, 1] += 1
            st[l, 0] += int(int(pred[n]) == l)
    return st


def score_fuse(p, dt=F64, fma=False):
    """p: scores (S, N, K), w [S], softmax, labels [N] | None.  Raw scores: fused bit-equal to the sequential fp32
    f = f + (w * x) from f = 0; softmax: within 2e-6.  pred and stats are held by fuse_extra.  fma = True (float32 only) fuses
    the product into the add: one rounding where two are asked (what the teeth test plants)."""
    x, w = p['scores'].to(dt), p['w'].to(dt)
    S, N, K = _dims(x)
    if p['softmax']:
        x = torch.softmax(x, 2) if dt == F64 else _softmax32(x)
    f = torch.zeros(N, K, dtype=dt)
    for s in range(S):
        f = (f.double() + w[s].double() * x[s].double()).to(dt) if fma else f + w[s] * x[s]
    return dict(fused=Out(f, None, 0, 'abs', FUSE_BAR) if p['softmax'] else Out(f, None, 0, 'eq'))


def _softmax32(x):
    """max-shift softmax in fp32 steps: exp(x - max) * (1 / sum)"""
    e = torch.exp(x - x.max(2, keepdim=True).values)
    return e * (1.0 / e.sum(2, keepdim=True))


def fuse_excluded(p):
    """rows whose fp64 top-2 gap is within FUSE_GAP: an fp32 exp may order them differently"""
    f = score_fuse(p, F64)['fused'].val
    if f.shape[1] < 2:
        return torch.zeros(f.shape[0], dtype=torch.bool)
    top = f.topk(2, 1).values
    return (top[:, 0] - top[:, 1]) <= FUSE_GAP


def fuse_extra(name, p, got):
    """pred = the first arg max of the SAME fused scores, always; in softmax mode also the fp64 arg max wherever the top-2 gap
    exceeds 1e-5 (at most 1 % of the rows may be left out); stats = the counts of that pred"""
    K = p['scores'].shape[2]
    pred = got['pred'].detach().cpu()
    if pred.dtype != torch.int64 or not torch.equal(pred, first_argmax(got['fused'])):
        raise B.BarError(f'{name}: pred is not the first arg max of fused')
    if p['softmax']:
        out = fuse_excluded(p)
        if int(out.sum()) > FUSE_CAP * out.numel():
            raise B.BarError(f'{name}: {int(out.sum())} of {out.numel()} rows too close to call (cap {FUSE_CAP:.0%})')
        ref = first_argmax(score_fuse(p, F64)['fused'].val)
        if not torch.equal(pred[~out], ref[~out]):
            raise B.BarError(f'{name}: pred differs from the fp64 arg max on {int((pred[~out] != ref[~out]).sum())} clear rows')
    if p.get('labels') is not None:
        if 'stats' not in got or not torch.equal(got['stats'].detach().cpu(), class_stats(pred, p['labels'], K)):
            raise B.BarError(f'{name}: class statistics are not the counts of pred')
    elif 'stats' in got:
        raise B.BarError(f'{name}: statistics without labels')
    return {}


KINDS = dict(stem_stats=stem_stats, stem_apply=stem_apply, stem_streams_eval=stem_streams_eval, pool_fwd=pool_fwd, pool_bwd=pool_bwd,
             fc_fwd=fc_fwd, fc_grouped=fc_grouped, fc_bwd=fc_bwd, ce_fwd=ce_fwd, ce_bwd=ce_bwd, score_fuse=score_fuse)
EXTRA = dict(ce_fwd=ce_extra, score_fuse=fuse_extra)
EXTRA_OUTPUTS = dict(score_fuse=('pred', 'stats'))          # outputs that only EXTRA holds


def evaluate(kind, p, dt=F32):
    out = {n: o.val for n, o in KINDS[kind](p, dt).items()}
    if kind == 'score_fuse':
        out['pred'] = first_argmax(out['fused'])
        if p.get('labels') is not None:
            out['stats'] = class_stats(out['pred'], p['labels'], p['scores'].shape[2])
    return out


def ratio(got, o):
    lim = B.elementwise_bar(o.L, o.mag)
    err = (got.detach().to('cpu', F64) - o.val).abs()
    r = torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return float(torch.nan_to_num(r, nan=float('inf')).max())


def verify(name, kind, p, got):
    """Hold the outputs `got` ({name: tensor}, from whatever computed them) of one launch to their bars.  Returns
    {output: max err / bound} (0 for an exact output); raises fp64_bars.BarError."""
    bars = KINDS[kind](p, F64)
    exact = KINDS[kind](p, F32) if any(o.how == 'eq' for o in bars.values()) else {}
    extra = EXTRA_OUTPUTS.get(kind, ())
    if set(got) - set(extra) != set(bars):
        raise B.BarError(f'{name}: outputs {sorted(got)} vs {sorted(bars)}')
    rat = {}
    for n, o in bars.items():
        g = got[n].detach().cpu()
        if g.dtype != F32 or tuple(g.shape) != tuple(o.val.shape):
            raise B.BarError(f'{name}: {n}: {g.dtype} {tuple(g.shape)} vs float32 {tuple(o.val.shape)}')
        if o.how == 'eq':
            if not torch.equal(g, exact[n].val):
                raise B.BarError(f'{name}: {n}: {int((g != exact[n].val).sum())} elements differ from the correctly rounded fp32 value')
            rat[n] = 0.0
        elif o.how == 'nan':
            if not bool(torch.isnan(g).all()):
                raise B.BarError(f'{name}: {n}: {float(g.flatten()[0])} where NaN is due')
            rat[n] = 0.0
        elif o.how == 'zero':
            if bool((g != 0).any()):
                raise B.BarError(f'{name}: {n}: {int((g != 0).sum())} elements are not exactly 0')
            rat[n] = 0.0
        elif o.how == 'abs':
            err = (g.to(F64) - o.val).abs()
            if not bool((err <= o.tol).all()):                              # NaN fails
                raise B.BarError(f'{name}: {n}: max |got - ref| = {float(torch.nan_to_num(err, nan=float("inf")).max()):.3g} > {o.tol:.3g}')
            rat[n] = float(err.max()) / o.tol
        else:
            rat[n] = ratio(g, o)
            B.check(f'{name}: {n}', g, o.val, o.mag, o.L)
    if kind in EXTRA:
        rat.update(EXTRA[kind](name, p, got))
    return rat
