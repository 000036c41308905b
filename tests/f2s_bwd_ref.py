"""Torch restatement of the f2s backward and saliency entry points (include/tamgcn.h "f2s backward", "saliency":
tamgcn_f2s_tcn_bwd, tamgcn_f2s_gcn_bwd, tamgcn_saliency_joints, tamgcn_saliency_accumulate) from the header's formulas, in a
chosen dtype, with the `absval` mode of tests/fp64_bars.py (every operand replaced by its magnitude, the ReLU masks left out:
the `mag` of the rounding bars), the transposed fold written independently of tam_gcn_amd.f2s._BlockST, the body-part
bookkeeping of saliency.PartImportance as plain loops, and the stage cases of tests/test_gpu_f2s_bwd_stages.py (the forward's
own tables, tests/f2s_ref.py).

Bars (derived, not tuned; fp64_bars.check(name, got, ref, mag, L)):
    tcn_bwd          L = KT * Cout               one sum over taps and channels
    gcn_bwd          L = 3 * (Cout + V) + Cres   the forward's nested-sum bound with the channel roles swapped, plus the residual's
                                                 own sum (Cres = 0 | 1 | Cout)
    saliency_joints  L = C * T * M               one sum of magnitudes (the product c1 * dx0 rounds once: inside the bar's + 4)

`defect=` evaluates a deliberately WRONG variant (tests/test_f2s_bwd_ref_cpu.py: the bars must reject each of them)."""
import zlib

import numpy as np
import torch

import f2s_ref as R

KT = R.KT
DEFECTS = ('mask_wrong_tensor', 'taps_not_mirrored', 'stride_phase', 'ae_not_transposed', 'res_dropped', 'res_not_upsampled',
           'drop_last_frame')


def _f(t, dt, absval):
    t = t.to(dt)
    return t.abs() if absval else t


def _gz(gout, out, dt, absval, defect=None):
    """gout * [out > 0]; absval: |gout|"""
    g = _f(gout, dt, absval)
    if absval:
        return g
    src = gout if defect == 'mask_wrong_tensor' else out                      # the defect masks by the gradient's own sign
    return g * (src > 0).to(dt)


# ---------------------------------------------------------------------------------------------------------------------
# the two stages
# ---------------------------------------------------------------------------------------------------------------------
def tcn_bwd(gout, out, h, Wt, stride, dt=torch.float64, absval=False, defect=None):
    """dh[n,c',t,v] = [h[n,c',t,v] > 0] * sum_c sum_tap Wt[c][c'][tap] * gz[n,c,tau,v], tau = (t + (KT-1)/2 - tap) / s; terms with a
    non-integral tau or tau outside [0, T2) are zero.  Wt (Cout, Cout, KT) is the FORWARD's array."""
    gz = _gz(gout, out, dt, absval, defect)
    N, C, T, V = h.shape
    T2 = gz.shape[2]
    Wt = _f(Wt, dt, absval).reshape(C, C, KT)
    t = torch.arange(T)
    dh = torch.zeros(N, C, T, V, dtype=dt)
    for tap in range(KT):
        num = t - (KT - 1) // 2 + tap if defect == 'taps_not_mirrored' else t + (KT - 1) // 2 - tap
        if defect == 'stride_phase' and stride == 2:
            num = num + 1
        tau = torch.div(num, stride, rounding_mode='floor')
        ok = ((num % stride == 0) & (tau >= 0) & (tau < T2)).to(dt)
        gs = gz[:, :, tau.clamp(0, T2 - 1)] * ok[None, None, :, None]
        dh += torch.einsum('cd,nctv->ndtv', Wt[:, :, tap], gs)
    if not absval:
        dh = dh * (h > 0).to(dt)
    if defect == 'drop_last_frame':
        dh = dh.clone()
        dh[:, :, -1] = 0
    return dh


def gcn_bwd(dh, Ae, Wg, rmode, stride, gout=None, out=None, Wr=None, dt=torch.float64, absval=False, defect=None):
    """dx[n,ci,t,v] = sum_k sum_c Wg[k][c][ci] * ( sum_w Ae[k][v][w] * dh[n,c,t,w] ) + res; res: rmode 0 nothing | 1 gz[n,ci,t,v] |
    2 [t % s == 0] * sum_c Wr[c][ci] * gz[n,c,t/s,v].  Ae, Wg (K, Cout, Cin), Wr (Cout, Cin) are the FORWARD's arrays."""
    dh, Ae, Wg = (_f(t, dt, absval) for t in (dh, Ae, Wg))
    if defect == 'ae_not_transposed':
        Ae = Ae.transpose(1, 2)
    da = torch.einsum('kvw,nctw->nkctv', Ae, dh)
    dx = torch.einsum('kci,nkctv->nitv', Wg, da)
    T = dh.shape[2]
    if rmode and defect != 'res_dropped':
        gz = _gz(gout, out, dt, absval, defect)
        if rmode == 1:
            dx = dx + gz
        else:
            r = torch.einsum('ci,nctv->nitv', _f(Wr, dt, absval), gz)
            up = torch.zeros_like(dx)
            if defect == 'res_not_upsampled':
                up[:, :, :r.shape[2]] = r
            else:
                up[:, :, torch.arange(r.shape[2]) * stride] = r
            dx = dx + up
    if defect == 'drop_last_frame':
        dx = dx.clone()
        dx[:, :, -1] = 0
    assert dx.shape[2] == T
    return dx


def block_bwd(x, p, stride, gout, dt=torch.float64, defect=None):
    """(dx, dict(out, h)) of the block f2s_ref.block_eval(x, p, stride) for the output gradient gout."""
    h = R.gcn_eval(x, p['Ae'], p['Wg'], p['bg'], dt)
    out = R.tcn_eval(h, p['Wt'], p['bt'], stride, p['rmode'], x, p['Wr'], p['br'], dt)
    dh = tcn_bwd(gout, out, h, p['Wt'], stride, dt, defect=defect)
    return gcn_bwd(dh, p['Ae'], p['Wg'], p['rmode'], stride, gout, out, p['Wr'], dt, defect=defect), dict(out=out, h=h)


def fold_transposed(p):
    """The backward's operands from f2s_ref.fold_block's: wtb[c'][c][tap], wgb[k][ci][c], wrb[ci][c]."""
    C = p['Wt'].shape[0]
    return dict(Wtb=p['Wt'].reshape(C, C, KT).permute(1, 0, 2).contiguous(), Wgb=p['Wg'].permute(0, 2, 1).contiguous(),
                Wrb=None if p['Wr'] is None else p['Wr'].t().contiguous())


# ---------------------------------------------------------------------------------------------------------------------
# saliency
# ---------------------------------------------------------------------------------------------------------------------
def saliency_joints(dx0, c1, M, dt=torch.float64, absval=False):
    """dx0 (N*M, C, T, V), c1 [(m V + v) C + c] -> (sal (N, V) = sum_{m,c,t} |dxin|, dxin (N, C, T, V, M) = c1 * dx0)"""
    NM, C, T, V = dx0.shape
    N = NM // M
    c = _f(c1, dt, absval).reshape(M, V, C).permute(0, 2, 1)                  # (M, C, V)
    g = _f(dx0, dt, absval).reshape(N, M, C, T, V) * c[None, :, :, None, :]
    return g.abs().sum((1, 2, 3)), g.permute(0, 2, 3, 4, 1).contiguous()


def part_accumulate(count, total, sal, labels, parts, per_class):
    """One batch into the state (count: list of int per class, total: list of lists [class][part] of float), in batch order: a
    sample counts until its class holds per_class; its part value is the mean of its joints' saliency."""
    for i, k in enumerate(int(v) for v in labels):
        if not 0 <= k < len(count) or count[k] >= per_class:
            continue
        count[k] += 1
        for p, joints in enumerate(parts):
            total[k][p] += sum(float(sal[i][j]) for j in joints) / len(joints)


def part_importance(count, total):
    """Per class: the mean over its counted samples, divided by the class's largest part value (by 1 when that is 0); a class
    without a sample gives zeros."""
    res = []
    for n, row in zip(count, total):
        if n == 0:
            res.append([0.0] * len(row))
            continue
        mean = [v / n for v in row]
        top = max(mean)
        res.append([v / (top if top != 0 else 1.0) for v in mean])
    return res


# the reference's grouping of the 20 N-UCLA joints (tools/train_stgcn_group.py:272-278): neck + head, shoulder .. hand, hip .. foot
UCLA_PARTS = {'head': [2, 3], 'l_hand': [4, 5, 6, 7], 'r_hand': [8, 9, 10, 11], 'l_leg': [12, 13, 14, 15], 'r_leg': [16, 17, 18, 19]}


# ---------------------------------------------------------------------------------------------------------------------
# stage cases: the forward's own tables
#   tcn_bwd  every entry of TCN_CASES;  gcn_bwd  every entry of GCN_CASES (rmode 1 where Cin == Cout, else 0) and every rmode-2
#   entry of TCN_CASES at K = 3
# ---------------------------------------------------------------------------------------------------------------------
def _gcn_bwd_cases():
    out = {}
    for cid, c in R.GCN_CASES.items():
        out[cid + ('_res1' if c['Cin'] == c['Cout'] else '_res0')] = dict(c, stride=1, rmode=1 if c['Cin'] == c['Cout'] else 0)
    for cid, c in R.TCN_CASES.items():
        if c['rmode'] == 2:
            out[cid + '_k3'] = dict(c, K=3)
    return out


TCN_BWD_CASES = dict(R.TCN_CASES)
GCN_BWD_CASES = _gcn_bwd_cases()
SAL_CASES = {'n2_c3_t13_v20_m1': dict(N=2, C=3, T=13, V=20, M=1), 'n1_c3_t70_v18_m2': dict(N=1, C=3, T=70, V=18, M=2),
             'n3_c2_t5_v7_m1': dict(N=3, C=2, T=5, V=7, M=1), 'n2_c3_t64_v25_m2': dict(N=2, C=3, T=64, V=25, M=2)}


def _rand(r, *shape, scale=1.0):
    return torch.from_numpy((scale * r.standard_normal(shape)).astype(np.float32))


def problem(stage, c):
    """Seeded fp32 operands of a case (forward-layout weights: the caller transposes).  h and out are relu of normals, so about
    half of each mask is zero; Ae is a non-symmetric matrix with entries of both signs."""
    r = np.random.RandomState(zlib.crc32(repr((stage, sorted((k, int(v)) for k, v in c.items()))).encode()))
    if stage == 'sal':
        N, C, T, V, M = c['N'], c['C'], c['T'], c['V'], c['M']
        return dict(dx0=_rand(r, N * M, C, T, V), c1=1 + 0.5 * _rand(r, M * V * C))
    V, N, Cin, Cout, T, s = c['V'], c['N'], c['Cin'], c['Cout'], c['T'], c['stride']
    T2 = (T - 1) // s + 1
    p = dict(gout=_rand(r, N, Cout, T2, V), out=torch.relu(_rand(r, N, Cout, T2, V)))
    if stage == 'tcn_bwd':
        p.update(h=torch.relu(_rand(r, N, Cout, T, V)), Wt=_rand(r, Cout, Cout, KT, scale=(KT * Cout) ** -0.5))
        return p
    K = c['K']
    p.update(dh=_rand(r, N, Cout, T, V), Ae=_rand(r, K, V, V, scale=0.5), Wg=_rand(r, K, Cout, Cin, scale=Cin ** -0.5), Wr=None)
    if c['rmode'] == 2:
        p['Wr'] = _rand(r, Cout, Cin, scale=Cin ** -0.5)
    if c['rmode'] == 0:
        p['gout'] = p['out'] = None
    return p


def evaluate(stage, c, p, dt=torch.float64, absval=False, defect=None):
    if stage == 'tcn_bwd':
        return tcn_bwd(p['gout'], p['out'], p['h'], p['Wt'], c['stride'], dt, absval, defect)
    if stage == 'gcn_bwd':
        return gcn_bwd(p['dh'], p['Ae'], p['Wg'], c['rmode'], c['stride'], p['gout'], p['out'], p['Wr'], dt, absval, defect)
    return saliency_joints(p['dx0'], p['c1'], c['M'], dt, absval)[0]


def bar_L(stage, c):
    if stage == 'tcn_bwd':
        return KT * c['Cout']
    if stage == 'gcn_bwd':
        return 3 * (c['Cout'] + c['V']) + {0: 0, 1: 1, 2: c['Cout']}[c['rmode']]
    return c['C'] * c['T'] * c['M']
