"""Torch restatement of the two f2s entry points (include/tamgcn.h "f2s": tamgcn_f2s_gcn, tamgcn_f2s_tcn) from the header's
formulas, in a chosen dtype, with the `absval` mode of tests/fp64_bars.py (every operand replaced by its magnitude, ReLU left
out: the `mag` of the rounding bars), the host-side fold of an st_gcn block written from the reference's lines
(models/stgcn.py:56-64, :75-99) independently of tam_gcn_amd.f2s._BlockST, and the stage cases of tests/test_gpu_f2s_stages.py.

Bars (derived, not tuned; fp64_bars.check(name, got, ref, mag, L)):
    gcn  L = 3 * (Cin + V)      sum_k [ sum_ci (.) sum_v (.) ] in either association order: a first-order bound of the nested sums
                                (K <= 3 partial results of Cin- and V-long sums, each rounded once more when it is re-used)
    tcn  L = KT * Cout + Cres   one sum over taps and channels, plus the residual's own (Cres = Cin | 1 | 0)

`defect=` evaluates a deliberately WRONG variant (tests/test_f2s_ref_cpu.py: the bars must reject each of them)."""
import zlib

import numpy as np
import torch

KT = 9
DEFECTS = ('bg_no_colsum', 'ae_transposed', 'tap_shift', 'stride_phase', 'drop_last_frame', 'res_unstrided')


def _f(t, dt, absval):
    t = t.to(dt)
    return t.abs() if absval else t


# ---------------------------------------------------------------------------------------------------------------------
# the two stages
# ---------------------------------------------------------------------------------------------------------------------
def gcn_eval(x, Ae, Wg, bg, dt=torch.float64, absval=False, defect=None):
    """h[n,c,t,w] = relu( sum_k sum_ci Wg[k][c][ci] * ( sum_v x[n,ci,t,v] * Ae[k][v][w] ) + bg[c][w] )"""
    x, Ae, Wg, bg = (_f(t, dt, absval) for t in (x, Ae, Wg, bg))
    if defect == 'ae_transposed':
        Ae = Ae.transpose(1, 2)
    xa = torch.einsum('nitv,kvw->nkitw', x, Ae)
    h = torch.einsum('kci,nkitw->nctw', Wg, xa) + bg[None, :, None, :]
    if not absval:
        h = torch.relu(h)
    if defect == 'drop_last_frame':
        h = h.clone()
        h[:, :, -1] = 0
    return h


def tcn_eval(h, Wt, bt, stride, rmode, x=None, Wr=None, br=None, dt=torch.float64, absval=False, defect=None):
    """out[n,c,tau,v] = relu( sum_tap sum_c' Wt[c][c'][tap] * h[n,c',tau*s - (KT-1)/2 + tap,v] + bt[c] + res ), frames outside
    [0, T) zero; res: rmode 0 nothing | 1 x[n,c,tau,v] | 2 sum_ci Wr[c][ci] x[n,ci,tau*s,v] + br[c]."""
    h, Wt, bt = (_f(t, dt, absval) for t in (h, Wt, bt))
    N, C, T, V = h.shape
    Wt = Wt.reshape(C, C, KT)
    T2 = (T - 1) // stride + 1
    tau = torch.arange(T2)
    out = torch.zeros(N, C, T2, V, dtype=dt)
    for tap in range(KT):
        fr = tau * stride - (KT - 1) // 2 + tap
        if defect == 'tap_shift':
            fr = fr + 1
        if defect == 'stride_phase' and stride == 2:
            fr = fr + 1
        ok = ((fr >= 0) & (fr < T)).to(dt)
        hs = h[:, :, fr.clamp(0, T - 1)] * ok[None, None, :, None]
        out += torch.einsum('cd,ndtv->nctv', Wt[:, :, tap], hs)
    out = out + bt[None, :, None, None]
    if rmode == 1:
        out = out + _f(x, dt, absval)
    elif rmode == 2:
        fr = tau if defect == 'res_unstrided' else tau * stride
        out = out + torch.einsum('ci,nitv->nctv', _f(Wr, dt, absval), _f(x, dt, absval)[:, :, fr]) + _f(br, dt, absval)[None, :, None, None]
    if not absval:
        out = torch.relu(out)
    if defect == 'drop_last_frame':
        out = out.clone()
        out[:, :, -1] = 0
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the fold (eval-mode BatchNorm: y = s * x + t, s = gamma / sqrt(var + eps), t = beta - mean * s)
# ---------------------------------------------------------------------------------------------------------------------
def bn_affine(sd, pfx, dt, eps=1e-5):
    s = sd[pfx + '.weight'].to(dt) / torch.sqrt(sd[pfx + '.running_var'].to(dt) + eps)
    return s, sd[pfx + '.bias'].to(dt) - sd[pfx + '.running_mean'].to(dt) * s


def fold_gcn(w, b, s1, t1, Ae, defect=None):
    """w (K*Cout, Cin), b (K*Cout): the 1 x 1 conv whose output channel k*Cout + c is subset k of channel c (:56-64); s1, t1:
    tcn.0 (:75).  bn(sum_k (w_k x + b_k) Ae_k) = sum_k (s1 w_k x) Ae_k + s1 sum_k b_k colsum(Ae_k) + t1."""
    K, V = Ae.shape[0], Ae.shape[-1]
    Cout = w.shape[0] // K
    Wg = w.reshape(K, Cout, -1) * s1[None, :, None]
    bk = b.reshape(K, Cout)
    if defect == 'bg_no_colsum':
        bg = (s1 * bk.sum(0) + t1)[:, None].expand(Cout, V)
    else:
        bg = s1[:, None] * torch.einsum('kc,kw->cw', bk, Ae.sum(1)) + t1[:, None]
    return Wg.contiguous(), bg.contiguous()


def fold_block(sd, pfx, Ae, rmode, dt=torch.float64, defect=None):
    """The f2s operands of the st_gcn block whose state is sd[pfx + ...]; rmode 'zero' | 'identity' | 'conv'."""
    Ae = Ae.to(dt)
    w = sd[pfx + '.gcn.conv.weight'].to(dt)
    s1, t1 = bn_affine(sd, pfx + '.tcn.0', dt)
    Wg, bg = fold_gcn(w.reshape(w.shape[0], -1), sd[pfx + '.gcn.conv.bias'].to(dt), s1, t1, Ae, defect)
    s2, t2 = bn_affine(sd, pfx + '.tcn.3', dt)
    wt = sd[pfx + '.tcn.2.weight'].to(dt)
    Cout = wt.shape[0]
    p = dict(Ae=Ae, Wg=Wg, bg=bg, Wt=(wt.reshape(Cout, Cout, -1) * s2[:, None, None]).contiguous(),
             bt=sd[pfx + '.tcn.2.bias'].to(dt) * s2 + t2, rmode={'zero': 0, 'identity': 1, 'conv': 2}[rmode], Wr=None, br=None)
    if rmode == 'conv':
        sr, tr = bn_affine(sd, pfx + '.residual.1', dt)
        wr = sd[pfx + '.residual.0.weight'].to(dt)
        p['Wr'] = wr.reshape(Cout, -1) * sr[:, None]
        p['br'] = sd[pfx + '.residual.0.bias'].to(dt) * sr + tr
    return p


def block_eval(x, p, stride, dt=torch.float64, defect=None):
    h = gcn_eval(x, p['Ae'], p['Wg'], p['bg'], dt, defect=defect)
    return tcn_eval(h, p['Wt'], p['bt'], stride, p['rmode'], x, p['Wr'], p['br'], dt, defect=defect)


# ---------------------------------------------------------------------------------------------------------------------
# stage cases: the smallest shapes at which the kernels can still go wrong
#   V: every residue mod 4, an exact 16-column tile, one joint past it, the upper bound;  K 1 and 3;  N' 1 and 3
# ---------------------------------------------------------------------------------------------------------------------
JOINTS = (3, 16, 17, 20, 25, 32)
GCN_CH = ((2, 16), (3, 64), (64, 64), (64, 128), (256, 256))
GCN_T = (1, 5, 33)


def _gcn_cases():
    out = {}
    for i, V in enumerate(JOINTS):
        for j, (ci, co) in enumerate(GCN_CH):
            T = 5 if ci == 256 else GCN_T[(i + j) % 3]
            K, N = (1, 3)[(i + j) % 2], (1, 3)[(i + j // 2) % 2]
            out[f'v{V}_k{K}_n{N}_c{ci}_{co}_t{T}'] = dict(V=V, K=K, N=N, Cin=ci, Cout=co, T=T, off=(i + j) % 3 == 2)
    return out


def _tcn_cases():
    combos = []
    for co in (16, 64):
        for T in (1, 3, 8, 9, 33):
            combos.append((co, T, 1, 1, co))                                         # identity residual
            combos.append((co, T, 2, 2, 3 if co == 16 else co // 2))                 # strided conv residual, Cin != Cout; T even and odd
            combos.append((co, T, 2, 0, co) if T in (3, 8, 33) else (co, T, 1, 2, co + 5))
    combos += [(256, 5, 1, 1, 256), (256, 5, 2, 2, 128), (256, 5, 2, 0, 256)]      # the longest contraction
    out = {}
    for i, (co, T, s, r, ci) in enumerate(combos):
        V, N = JOINTS[i % 6], (1, 3)[(i // 6 + i) % 2]
        out[f'v{V}_n{N}_c{co}_t{T}_s{s}_res{r}' + (f'_cin{ci}' if r == 2 else '')] = dict(V=V, N=N, Cin=ci, Cout=co, T=T, stride=s, rmode=r,
                                                                                       off=i % 3 == 2)
    return out


GCN_CASES, TCN_CASES = _gcn_cases(), _tcn_cases()


def _rand(r, *shape, scale=1.0):
    return torch.from_numpy((scale * r.standard_normal(shape)).astype(np.float32))


def problem(stage, c, defect=None):
    """Seeded fp32 operands of a case.  gcn: the folded Wg / bg come from raw conv / BatchNorm parameters through fold_gcn (so
    that a fold defect can be injected); Ae is a non-symmetric matrix with entries of both signs."""
    r = np.random.RandomState(zlib.crc32(repr((stage, sorted((k, int(v)) for k, v in c.items()))).encode()))
    V, N, Cin, Cout, T = c['V'], c['N'], c['Cin'], c['Cout'], c['T']
    if stage == 'gcn':
        K = c['K']
        Ae = _rand(r, K, V, V, scale=0.5)
        w, b = _rand(r, K * Cout, Cin, scale=Cin ** -0.5), _rand(r, K * Cout)
        s1, t1 = 1 + 0.2 * _rand(r, Cout), _rand(r, Cout, scale=0.3)
        Wg, bg = fold_gcn(w, b, s1, t1, Ae, defect)
        return dict(x=_rand(r, N, Cin, T, V), Ae=Ae, Wg=Wg, bg=bg)
    p = dict(h=_rand(r, N, Cout, T, V).abs(), Wt=_rand(r, Cout, Cout, KT, scale=(KT * Cout) ** -0.5), bt=_rand(r, Cout, scale=0.3),
             x=None, Wr=None, br=None)
    if c['rmode'] == 1:
        p['x'] = _rand(r, N, Cout, T, V)
    elif c['rmode'] == 2:
        p.update(x=_rand(r, N, Cin, T, V), Wr=_rand(r, Cout, Cin, scale=Cin ** -0.5), br=_rand(r, Cout, scale=0.3))
    return p


def evaluate(stage, c, p, dt=torch.float64, absval=False, defect=None):
    if stage == 'gcn':
        return gcn_eval(p['x'], p['Ae'], p['Wg'], p['bg'], dt, absval, defect)
    return tcn_eval(p['h'], p['Wt'], p['bt'], c['stride'], c['rmode'], p['x'], p['Wr'], p['br'], dt, absval, defect)


def bar_L(stage, c):
    if stage == 'gcn':
        return 3 * (c['Cin'] + c['V'])
    return KT * c['Cout'] + {0: 0, 1: 1, 2: c['Cin']}[c['rmode']]
