"""fp64 references of the small-batch eval kernels (csrc/f2.hip: V = 20, csrc/f2v.hip: V = 25), one per STAGE, the bars their
results are held to (fp64_bars.check), the case tables of the ledger (tests/test_gpu_f2_stages.py) and a mirror of the
kernel geometry that decides which code path a case reaches (tests/test_f2_ref_cpu.py holds the mirror to the source text).

Conventions of fp64_bars.conv_eval and ctrgc_ref: plain torch on the CPU in a chosen dtype; absval=True evaluates the same
expression on magnitudes (ReLU left out, minus turned into plus): the `mag` of the bound (L + 4) * 2^-24 * mag.  Every
reference takes the tensors the kernel was GIVEN (a random E for gcn, a random sum / diff for gemm, a random h for tcn, a
random xpart for e), so no stage's rounding enters another stage's bar.

A problem `p` is a dict of CPU float32 tensors in the LOGICAL layout (joints contiguous, V per frame) plus the case's ints.
Parameters carry a leading group axis (G = 1 for a plain case); `sub(p, g)` is group g's problem: its parameters without
that axis and its rows [g N/G, (g+1) N/G) of every activation.

    gcn descriptor (stages e and gcn)   x (N, Cin, T, V)  xpart (N, ceil(T/4), Cin, V) | None  E (N, S, Cout, V, V)
        w12 (S*2R, Cin)  b12 (S*2R,)  w4 (S, Cout, R)  b4 (S, Cout)  A (S, V, V)  alpha (1,)  w3 (S*Cout, Cin)  b3 (S*Cout,)
        sy, ty (Cout,)  wd (Cout, Cin), bd (Cout,) | None
    gemm                                x (N, K, T, V)  add (N, M, T, V)  w (M, K)  b (M,)
    tcn                                 h (N, Cout, T, V)  x (N, Cin, T, V)  wt [nb] (Cb, Cb*ks) tap innermost  bt [nb] (Cb,)
        sp, tp (Cb,)  wr (Cout, Cin), br (Cout,) | None

The bars (derived; nothing here is a measured tolerance):

  e     L = R on E = alpha (W4 D + b4) + A, plus the allowance |alpha| sum_r |W4| (TANH_DELTA + delta): TANH_DELTA = 2^-20 is
        ctrgc_ref's bound of the same fast_tanh; delta = 2^-24 (|p| + |q|) for the rounded difference plus the rounding bounds
        of p and q themselves, (Cin + T + 4) 2^-24 mag(p | q) each (T terms of the mean and its scaling, Cin products, the
        bias); tanh is 1-Lipschitz.  alpha == 0: 0 * finite + A is A bit for bit.
  gcn   L = Cin + 3V (+ Cin with the convolutional residual) on the nested magnitude of sy sum E (W3 x + b3) + ty +- res.
  gemm  mode 0: relu(add + tanh(W x + b)): L = 0 on |add| + |tanh|, allowance TANH_DELTA + (K + 2) 2^-24 mag(W x + b);
        mode 1: L = K.  ReLU is 1-Lipschitz.
  tcn   temporal rows L = Cb*ks, pooled and plain rows L = 0, each + Cin with the convolutional residual.  The pooled maximum
        selects among exactly represented fp32 values over the frames that exist (padding is -inf, not 0).
        xpart is compared with the fp64 tile sums of the kernel's OWN out at L = 4.
No element is excluded anywhere."""
import ctypes as C

import torch

import fp64_bars as B
from ctrgc_ref import TANH_DELTA, ratio

F64 = torch.float64
NAN = float('nan')
S = 3

# ---- the kernel geometry this file mirrors (csrc/f2_common.h, f2.hip, f2v.hip; tests/test_f2_ref_cpu.py reads the source text)
BT = 4                    # frames of a tile (F2_BT)
HF = 15                   # frames of a halo tile (F2_HF)
KC = 128                  # K rows of a staged chunk of f2v_gcn (F2_KC)
VP25 = 28                 # floats of a frame in the f2v family's own buffers
PX = 36                   # xbar / pq pitch (F2_PX)
LDS_MAX = 160 * 1024
FAMILIES = {'f2': 20, 'f2v': 25}


def vp(V):
    return (V + 3) & ~3


def fv_e_lds(Cin, R, ntp, V=25):
    """FvHost<V>::fv_e_lds of csrc/f2v.hip (f2_e_lds of csrc/f2_common.h at FvGeo<V>'s pitches) in bytes"""
    Kp, R2p, Rp = (Cin + 15) & ~15, max(16, 2 * R), (R + 15) & ~15
    PD = ((V * vp(V) + 15) // 16) * 16 + 4
    return 4 * (Kp * PX + R2p * PX + 64 * PX + max(Rp * PD, ntp * Kp * vp(V)))


def e_phases(Cin, R, fam):
    """frame phases of the xbar sum: f2 always 4; f2v 4 unless four partial tiles do not fit LDS"""
    return 4 if fam == 'f2' or fv_e_lds(Cin, R, 4) <= LDS_MAX else 2


def halo(ks, dil, stride):
    return (BT - 1) * stride + (ks - 1) * dil + 1


def _f(dt, absval):
    return (lambda t: t.to(dt).abs()) if absval else (lambda t: t.to(dt))


def _bc(c):
    return c[None, :, None, None]


# ---------------------------------------------------------------------------------------------------------------------
# layouts of the V = 25 family: contiguous (.., 25) <-> frames of 28 floats
# ---------------------------------------------------------------------------------------------------------------------
def to_frames(t, V, fill=0.0):
    """(..., V) -> (..., VP) with the pad joints holding `fill` (V = 20: unchanged)"""
    P = vp(V)
    if P == V:
        return t.contiguous()
    out = torch.full(tuple(t.shape[:-1]) + (P,), fill, dtype=t.dtype, device=t.device)
    out[..., :V] = t
    return out


def from_frames(t, V):
    """(..., VP) -> ((..., V) contiguous, (..., VP - V) the pad joints)"""
    return t[..., :V].contiguous(), t[..., V:].contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def xbar(p, dt=F64, absval=False):
    """mean over T of x, or (sum over the tiles of xpart) / T when xpart is given: (N, Cin, V)"""
    f = _f(dt, absval)
    if p.get('xpart') is not None:
        return f(p['xpart']).sum(1) / p['T']
    return f(p['x']).sum(2) / p['T']


def pq(p, dt=F64, absval=False):
    """p, q (N, S, R, V) = W12 xbar + b12"""
    f = _f(dt, absval)
    R, Cin = p['R'], p['Cin']
    W, b = f(p['w12']).view(S, 2, R, Cin), f(p['b12']).view(S, 2, R)
    v = torch.einsum('sjrk,nkv->nsjrv', W, xbar(p, dt, absval)) + b[None, :, :, :, None]
    return v[:, :, 0], v[:, :, 1]


def e(p, dt=F64, absval=False):
    """E (N, S, Cout, V, V) = alpha (W4 tanh(p_u - q_v) + b4) + A;  L = R"""
    f = _f(dt, absval)
    p_, q_ = pq(p, dt)
    D = f(torch.tanh(p_.unsqueeze(-1) - q_.unsqueeze(-2)))
    return f(p['alpha']) * (torch.einsum('scr,nsruv->nscuv', f(p['w4']), D) + f(p['b4'])[None, :, :, None, None]) + f(p['A'])[None, :, None]


def e_tanh_delta(p):
    """bound of |D_kernel - D| (N, S, R, V, V)"""
    p_, q_ = pq(p)
    pm, qm = pq(p, absval=True)
    Lpq = p['Cin'] + p['T'] + 4
    dp = B.EPS32 * p_.abs() + Lpq * B.EPS32 * pm
    dq = B.EPS32 * q_.abs() + Lpq * B.EPS32 * qm
    return TANH_DELTA + dp.unsqueeze(-1) + dq.unsqueeze(-2)


def e_allow(p):
    return p['alpha'].double().abs() * torch.einsum('scr,nsruv->nscuv', p['w4'].double().abs(), e_tanh_delta(p))


def gcn(p, dt=F64, absval=False):
    """(sum, diff) (N, Cout, T, V) each"""
    f = _f(dt, absval)
    x, Cout = f(p['x']), p['Cout']
    N, _, T, V = x.shape
    x3 = (torch.einsum('mk,nktv->nmtv', f(p['w3']), x) + _bc(f(p['b3']))).view(N, S, Cout, T, V)
    z = torch.einsum('nscuv,nsctv->nctu', f(p['E']), x3)
    y = _bc(f(p['sy'])) * z + _bc(f(p['ty']))
    if p['res_mode'] == 0:
        res = torch.zeros_like(y)
    elif p['res_mode'] == 1:
        res = x
    else:
        res = torch.einsum('mk,nktv->nmtv', f(p['wd']), x) + _bc(f(p['bd']))
    return y + res, (res + y if absval else res - y)


def gcn_L(p, V):
    return p['Cin'] + 3 * V + (p['Cin'] if p['res_mode'] == 2 else 0)


def gemm_pre(p, dt=F64, absval=False):
    f = _f(dt, absval)
    return torch.einsum('mk,nktv->nmtv', f(p['w']), f(p['x'])) + _bc(f(p['b']))


def gemm(p, dt=F64, absval=False):
    f = _f(dt, absval)
    v = gemm_pre(p, dt, absval)
    if p['mode'] == 0:
        t = torch.tanh(gemm_pre(p, dt))
        v = f(p['add']) + (t.abs() if absval else t)
        return v if absval else torch.relu(v)
    if not absval:
        v = v.clone()
        v[:, :p['relu_rows']] = torch.relu(v[:, :p['relu_rows']])
    return v


def gemm_L(p):
    return 0 if p['mode'] == 0 else p['K']


def gemm_allow(p):
    if p['mode'] != 0:
        return 0.0
    return TANH_DELTA + (p['K'] + 2) * B.EPS32 * gemm_pre(p, absval=True)


def pool3(h, stride, T2):
    """max over the frames ts - 1, ts, ts + 1 that exist (the padding is -inf)"""
    N, Cc, T, V = h.shape
    pad = torch.full((N, Cc, 1, V), float('-inf'), dtype=h.dtype)
    hp = torch.cat((pad, h, pad), 2)
    ts = torch.arange(T2) * stride + 1
    return torch.maximum(torch.maximum(hp[:, :, ts - 1], hp[:, :, ts]), hp[:, :, ts + 1])


def tcn(p, dt=F64, absval=False):
    """out (N, Cout, T2, V)"""
    f = _f(dt, absval)
    Cb, nb, ks, s, T = p['Cb'], p['nb'], p['ks'], p['stride'], p['T']
    T2 = (T - 1) // s + 1
    h = f(p['h'])
    vals = []
    for b, d in enumerate(p['dils']):
        W = f(p['wt'][b]).view(Cb, Cb, ks)
        vals.append(B.conv_taps(h[:, b * Cb:(b + 1) * Cb], W, ks, d, s, ((ks - 1) * d) // 2, 1, T2) + _bc(f(p['bt'][b])))
    m = pool3(p['h'].to(dt)[:, nb * Cb:(nb + 1) * Cb], s, T2)                 # selected on the real values
    vals.append(_bc(f(p['sp'])) * f(m) + _bc(f(p['tp'])))
    vals.append(h[:, (nb + 1) * Cb:, ::s])
    out = torch.cat(vals, 1)
    if p['res_mode'] == 1:
        out = out + f(p['x'])
    elif p['res_mode'] == 2:
        out = out + torch.einsum('mk,nktv->nmtv', f(p['wr']), f(p['x'])[:, :, ::s]) + _bc(f(p['br']))
    return out if absval else torch.relu(out)


def tcn_rows(p):
    """[(name, channel slice, L)]: the contraction length differs per branch kind"""
    Cb, nb = p['Cb'], p['nb']
    r = p['Cin'] if p['res_mode'] == 2 else 0
    return [('temporal', slice(0, nb * Cb), Cb * p['ks'] + r), ('pooled', slice(nb * Cb, (nb + 1) * Cb), r),
            ('plain', slice((nb + 1) * Cb, (nb + 2) * Cb), r)]


def tile_sums(out, dt=F64, absval=False):
    """(N, C, T2, V) -> (N, ceil(T2/4), C, V): sums over each four-frame tile; a ragged last tile sums its real frames"""
    o = _f(dt, absval)(out)
    N, Cc, T2, V = o.shape
    o = torch.cat((o, torch.zeros(N, Cc, (-T2) % BT, V, dtype=dt)), 2)
    return o.view(N, Cc, -1, BT, V).sum(3).permute(0, 2, 1, 3).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# checks: every output of a stage against its bar; return {output: (worst err / bar, tanh-attributable error | None)}
# ---------------------------------------------------------------------------------------------------------------------
def _chk(name, key, got, ref, mag, L, allow=0.0):
    B.check(f'{name}: {key}', got, ref, mag, L, allow=allow)
    return ratio(got, ref, mag, L, allow)


def check_e(name, p, got):
    ref, mag = e(p), e(p, absval=True)
    if float(p['alpha']) == 0.0:
        if not torch.equal(got.cpu(), p['A'][None, :, None].expand_as(ref).float()):
            raise B.BarError(f'{name}: alpha == 0 but E is not A bit for bit')
    r = _chk(name, 'E', got, ref, mag, p['R'], e_allow(p))
    # the error per tanh that the rounding of the R-term sum does not explain (test_gpu_ctrgc_routes.tanh_attributable)
    w = float(p['alpha'].abs()) * p['w4'].double().abs().sum(-1)[None, :, :, None, None]
    over = ((got.cpu().double() - ref).abs() - B.elementwise_bar(p['R'], mag)).clamp_min(0)
    ta = float((over / w).max()) if float(p['alpha']) != 0.0 else 0.0
    return {'E': (r, ta)}


def check_gcn(name, p, got_sum, got_diff, V):
    (rs, rd), (ms, md) = gcn(p), gcn(p, absval=True)
    L = gcn_L(p, V)
    return {'sum': (_chk(name, 'sum', got_sum, rs, ms, L), None), 'diff': (_chk(name, 'diff', got_diff, rd, md, L), None)}


def check_gemm(name, p, got):
    ref, mag, al = gemm(p), gemm(p, absval=True), gemm_allow(p)
    r = _chk(name, 'out', got, ref, mag, gemm_L(p), al)
    ta = None
    if p['mode'] == 0:
        ta = float(((got.cpu().double() - ref).abs() - B.elementwise_bar(0, mag)).clamp_min(0).max())
    return {'out': (r, ta)}


def check_tcn(name, p, got_out, got_xpart):
    ref, mag = tcn(p), tcn(p, absval=True)
    out = {}
    for key, sl, L in tcn_rows(p):
        out[key] = (_chk(name, key, got_out[:, sl], ref[:, sl], mag[:, sl], L), None)
    if got_xpart is not None:
        out['xpart'] = (_chk(name, 'xpart', got_xpart, tile_sums(got_out.cpu()), tile_sums(got_out.cpu(), absval=True), BT), None)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the ledger's tables.  N <= 3 and T <= 9 except where a row of the table asks for more.  `off`: the weight arrays start one
# float past a 16-byte boundary (the scalar A-fragment path at a row length that would otherwise take the vector path); the
# run must be bit-equal to the aligned one.  `G`: the grouped twin runs too, on G groups.
# ---------------------------------------------------------------------------------------------------------------------
def _c(**kw):
    kw.setdefault('N', 2)
    kw.setdefault('G', 1)
    kw.setdefault('off', False)
    if kw['G'] > 1:                                              # two groups: two samples each, so that sample / (N / G) is a real division
        kw['N'] = 4 if kw['G'] == 2 else 3
    return kw


def _e(Cin, R, Cout, T, src='x', alpha=0.7, **kw):
    return _c(Cin=Cin, R=R, Cout=Cout, T=T, src=src, alpha=alpha, res_mode=0, **kw)


E_CASES = {
    'cin3_r8_t5': _e(3, 8, 16, 5, G=2),
    'cin3_r1_t1': _e(3, 1, 16, 1),
    'cin16_r4_t3': _e(16, 4, 48, 3, off=True),
    'cin40_r12_t4': _e(40, 12, 16, 4),
    'cin40_r20_t33': _e(40, 20, 16, 33, N=1),
    'cin64_r16_t5': _e(64, 16, 48, 5, off=True, G=3),
    'cin64_r24_t4': _e(64, 24, 16, 4),
    'cin16_r28_t3': _e(16, 28, 16, 3, G=2),                        # four row tiles, the last one half empty
    'cin64_r32_t3': _e(64, 32, 16, 3, off=True),
    'cin256_r8_t4': _e(256, 8, 16, 4, N=1),                       # f2v: four frame phases (just under the LDS cap)
    'cin256_r16_t5': _e(256, 16, 16, 5, N=1, off=True),           # f2v: two frame phases
    'cin64_r8_alpha0': _e(64, 8, 16, 4, alpha=0.0),
    'cin40_r20_alpha0_xpart': _e(40, 20, 16, 6, src='xpart', alpha=0.0),
    'cin256_r16_xpart_t18': _e(256, 16, 16, 18, src='xpart', N=1),
    'cin256_r8_xpart_t35': _e(256, 8, 16, 35, src='xpart', N=1),
    'cin3_r12_xpart_t2_grouped': _e(3, 12, 16, 2, src='xpart', G=2),
}
for _T in (1, 2, 3, 4, 9, 10, 11, 12, 17, 18, 19, 20, 33, 34, 35, 36):
    E_CASES[f'xpart_t{_T}'] = _e(16 if _T % 2 else 40, 8 if _T % 3 else 20, 16, _T, src='xpart', N=1, G=3 if _T in (3, 19, 35) else 2 if _T in (2, 10, 12) else 1)


def _g(Cin, Cout, res_mode, T, **kw):
    return _c(Cin=Cin, Cout=Cout, res_mode=res_mode, T=T, R=8, src='x', alpha=0.7, **kw)


GCN_CASES = {
    'cin3_res0_t5': _g(3, 16, 0, 5, G=2),
    'cin3_res2_t1': _g(3, 16, 2, 1),
    'cin16_res1_t3': _g(16, 16, 1, 3, off=True),
    'cin16_res2_t9': _g(16, 48, 2, 9, off=True, G=3),
    'cin40_res0_t4': _g(40, 16, 0, 4),
    'cin40_res2_t5': _g(40, 48, 2, 5, G=2),
    'cin64_res0_t9': _g(64, 48, 0, 9, off=True),
    'cin64_res2_t3': _g(64, 16, 2, 3),
    'cin48_res1_t4': _g(48, 48, 1, 4, G=2),
    'cin128_res2_t5': _g(128, 16, 2, 5, N=1),                     # f2v: one K chunk exactly
    'cin144_res0_t5': _g(144, 16, 0, 5, N=1, off=True),           # a chunk plus 16 rows
    'cin200_res2_t3': _g(200, 16, 2, 3, N=1),                     # scalar-path tail in the second chunk
    'cin256_res0_t5': _g(256, 16, 0, 5, N=1),                     # two full chunks
}


def _m(K, M, mode, relu_rows, T, **kw):
    return _c(K=K, M=M, mode=mode, relu_rows=relu_rows, T=T, **kw)


GEMM_CASES = {
    'k16_m16_mode0_t5': _m(16, 16, 0, 0, 5, G=2),
    'k40_m48_mode0_t3': _m(40, 48, 0, 0, 3, G=3),
    'k48_m48_mode0_t9': _m(48, 48, 0, 0, 9, off=True),
    'k256_m16_mode0_t6': _m(256, 16, 0, 0, 6, N=1),
    'k16_m48_relu0_t7': _m(16, 48, 1, 0, 7),
    'k40_m48_relu8_t5': _m(40, 48, 1, 8, 5, G=3),
    'k48_m48_relu24_t2': _m(48, 48, 1, 24, 2, off=True, G=2),
    'k256_m48_relu48_t9': _m(256, 48, 1, 48, 9, N=1, off=True),
    'k40_m16_relu16_t1': _m(40, 16, 1, 16, 1),
    'k256_m16_relu8_t5': _m(256, 16, 1, 8, 5, N=1),
    'k16_m48_relu32_t4': _m(16, 48, 1, 32, 4),
}


def _t(nb, Cb, ks, dils, stride, T, res_mode, Cin=None, xpart=True, **kw):
    Cout = (nb + 2) * Cb
    return _c(nb=nb, Cb=Cb, ks=ks, dils=tuple(dils), stride=stride, T=T, res_mode=res_mode, Cout=Cout,
              Cin=Cout if Cin is None else Cin, xpart=xpart, **kw)


TCN_CASES = {
    'nb2_cb16_k5_s2_res0_t9': _t(2, 16, 5, (1, 2), 2, 9, 0, G=2),                  # wr / br absent in a grouped launch
    'nb2_cb16_k5_s2_res2_cin3_t8': _t(2, 16, 5, (2, 1), 2, 8, 2, Cin=3, G=2),
    'nb1_cb16_k9_s2_res2_cin40_t3': _t(1, 16, 9, (1,), 2, 3, 2, Cin=40),
    'nb1_cb32_k9_s2_res2_cin64_t2': _t(1, 32, 9, (1,), 2, 2, 2, Cin=64, off=True),
    'nb1_cb48_k7_s2_res0_t1': _t(1, 48, 7, (1,), 2, 1, 0, xpart=False),
    'nb2_cb16_k3_s1_res1_t5': _t(2, 16, 3, (1, 5), 1, 5, 1, G=3),
    'nb2_cb32_k5_s1_res1_t5': _t(2, 32, 5, (1, 2), 1, 5, 1, xpart=False),
    'nb3_cb16_k9_s1_res2_cin40_t5': _t(3, 16, 9, (1, 1, 1), 1, 5, 2, Cin=40),
    'nb4_cb16_k1_s1_res2_cin64_t1': _t(4, 16, 1, (1, 1, 1, 1), 1, 1, 2, Cin=64, off=True, G=2),
    'nb4_cb64_k3_s1_res2_cin3_t5': _t(4, 64, 3, (1, 2, 3, 5), 1, 5, 2, Cin=3, N=1),
    'nb1_cb64_k7_s1_res0_t5': _t(1, 64, 7, (1,), 1, 5, 0, N=1, off=True),
    'nb1_cb16_k3_s2_res0_t5': _t(1, 16, 3, (1,), 2, 5, 0),                          # three output frames: a ragged tile of 3
    'nb3_cb48_k3_s1_res1_t1': _t(3, 48, 3, (5, 1, 2), 1, 1, 1, N=1),
}

AT_LIMIT = {1: ((3, 5), (5, 2), (9, 1)), 2: ((5, 2), (9, 1))}     # (ks, dil) whose next dilation no longer fits the halo tile

STAGES = {'e': E_CASES, 'gcn': GCN_CASES, 'gemm': GEMM_CASES, 'tcn': TCN_CASES}


# ---------------------------------------------------------------------------------------------------------------------
# which code paths a case reaches (the conditions of the kernels, mirrored)
# ---------------------------------------------------------------------------------------------------------------------
def _vec(name, rowlen, off):
    """an `off` case runs twice, aligned and offset by one float: both fragment paths at a row length that is a multiple of 16"""
    if rowlen % 16:
        return {f'{name}:scalar'}
    return {f'{name}:vec', f'{name}:scalar'} if off else {f'{name}:vec'}


def _bt(T):
    return f'ragged{T % BT}'


def paths(stage, c, fam):
    P = set()
    off, G = c['off'], c['G']
    P.add('grouped' if G > 1 else 'plain')
    if stage == 'e':
        Cin, R, T = c['Cin'], c['R'], c['T']
        R2p = max(16, 2 * R)
        nrt = -(-R2p // 16)
        P |= _vec('w12', Cin, off) | _vec('w4', R, off) | {f'nrt{nrt}', f'nparts{4 // nrt}', f'kblocks{min(4, -(-Cin // 16))}',
              f'phases{e_phases(Cin, R, fam)}', f'xsrc:{c["src"]}', 'alpha0' if c['alpha'] == 0 else 'alpha'}
        if R > 16:
            P.add('w4:second')
        if Cin % 16:
            P.add('w12:ktail')
        if c['src'] == 'x':
            P.add(f'T{T}' if T <= 5 else 'framestep' if T > 32 else 'T')
        else:
            ntt, ntp = -(-T // BT), e_phases(Cin, R, fam)
            tpg = -(-ntt // ntp)
            P |= {f'tiles{ntt}', _bt(T)}
            if any(g * tpg >= ntt for g in range(ntp)):
                P.add('xpart:emptygroup')
            if ntt % tpg:
                P.add('xpart:raggedgroup')
    elif stage == 'gcn':
        Cin = c['Cin']
        P |= _vec('w3', Cin, off) | {f'res{c["res_mode"]}', _bt(c['T'])}
        if Cin % 16:
            P.add('w3:ktail')
        if c['res_mode'] == 2:
            P |= _vec('wd', Cin, off)
        Kp = (Cin + 15) & ~15
        if fam == 'f2v':
            P.add(f'chunks{-(-Kp // KC)}')
            if Kp > KC and Kp % KC:
                P.add('chunk:partial')
            if Cin > KC and Cin % 16:
                P.add('chunk:scalartail')
    elif stage == 'gemm':
        K, M, rr = c['K'], c['M'], c['relu_rows']
        P |= _vec('w', K, off) | {f'mode{c["mode"]}', _bt(c['T']), f'kblocks{min(4, -(-K // 16))}'}
        if K % 16:
            P.add('w:ktail')
        if c['mode'] == 1:
            P.add('relu:none' if rr == 0 else 'relu:all' if rr == M else 'relu:midtile' if rr % 16 else 'relu:tileedge')
    else:
        s, ks = c['stride'], c['ks']
        T2 = (c['T'] - 1) // s + 1
        P |= {f'nb{c["nb"]}', f'Cb{c["Cb"]}', f'stride{s}', f'res{c["res_mode"]}@s{s}', _bt(T2),
              'xpart:given' if c['xpart'] else 'xpart:null', 'pooled', 'plain', 'temporal'}
        P |= _vec('wt', c['Cb'] * ks, off)
        for d in c['dils']:
            P.add(f'k{ks}d{d}@s{s}')
            if (ks, d) in AT_LIMIT[s]:
                P.add(f'atlimit:k{ks}d{d}@s{s}')
        if c['res_mode'] == 2:
            P |= _vec('wr', c['Cin'], off) | {f'wr:cin{c["Cin"]}'}
        if c['T'] % s == 0 and s == 2:
            P.add('pool:lastframe')                              # frame ts + 1 of the last output frame exists
        if G > 1 and c['res_mode'] != 2:
            P.add('grouped:wr_absent')
    return P


def required_paths(fam):
    """What the ledger's table must reach at least once per family."""
    req = {
        'e': {'w12:vec', 'w12:scalar', 'w12:ktail', 'w4:vec', 'w4:scalar', 'w4:second', 'nrt1', 'nrt2', 'nrt3', 'nrt4',
              'nparts4', 'nparts2', 'nparts1', 'kblocks1', 'kblocks3', 'kblocks4', 'phases4', 'xsrc:x', 'xsrc:xpart', 'alpha0', 'alpha',
              'T1', 'T3', 'T4', 'T5', 'framestep', 'tiles1', 'tiles3', 'tiles5', 'tiles9', 'ragged0', 'ragged1', 'ragged2', 'ragged3',
              'xpart:emptygroup', 'xpart:raggedgroup', 'grouped', 'plain'},
        'gcn': {'w3:vec', 'w3:scalar', 'w3:ktail', 'wd:vec', 'wd:scalar', 'res0', 'res1', 'res2', 'ragged0', 'ragged1', 'ragged3',
                'grouped', 'plain'},
        'gemm': {'w:vec', 'w:scalar', 'w:ktail', 'mode0', 'mode1', 'relu:none', 'relu:all', 'relu:midtile', 'relu:tileedge',
                 'ragged0', 'ragged1', 'ragged2', 'ragged3', 'kblocks1', 'kblocks3', 'kblocks4', 'grouped', 'plain'},
        'tcn': {'nb1', 'nb2', 'nb3', 'nb4', 'Cb16', 'Cb32', 'Cb48', 'Cb64', 'stride1', 'stride2', 'res0@s2', 'res1@s1', 'res2@s1',
                'res2@s2', 'k1d1@s1', 'k3d1@s1', 'k3d5@s1', 'k5d2@s1', 'k7d1@s1', 'k9d1@s1', 'k5d2@s2', 'k9d1@s2',
                'atlimit:k3d5@s1', 'atlimit:k5d2@s1', 'atlimit:k9d1@s1', 'atlimit:k5d2@s2', 'atlimit:k9d1@s2', 'wr:cin3', 'wr:cin40',
                'wr:cin64', 'wr:vec', 'wr:scalar', 'wt:vec', 'wt:scalar', 'xpart:given', 'xpart:null', 'ragged0', 'ragged1', 'ragged2',
                'ragged3', 'pool:lastframe', 'grouped', 'plain', 'grouped:wr_absent'},
    }
    if fam == 'f2v':
        req['e'] |= {'phases2'}
        req['gcn'] |= {'chunks1', 'chunks2', 'chunk:partial', 'chunk:scalartail'}
    return req


# ---------------------------------------------------------------------------------------------------------------------
# seeded problems
# ---------------------------------------------------------------------------------------------------------------------
def _rn(g, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=g) * scale + shift


def problem(stage, c, V, seed):
    g = torch.Generator().manual_seed(seed)
    G, N, T = c['G'], c['N'], c['T']
    p = dict(c, V=V)
    if stage in ('e', 'gcn'):
        Cin, Cout, R = c['Cin'], c['Cout'], c['R']
        p['x'] = _rn(g, N, Cin, T, V, shift=0.5)
        # NOT the tile sums of x: which operand the kernel reads shows in the result
        p['xpart'] = _rn(g, N, -(-T // BT), Cin, V, scale=2.0, shift=1.0) if c['src'] == 'xpart' else None
        p['E'] = _rn(g, N, S, Cout, V, V, scale=0.3)
        p['w12'] = _rn(g, G, S * 2 * R, Cin, scale=Cin ** -0.5)
        p['b12'] = _rn(g, G, S * 2 * R, scale=0.5)
        p['w4'] = _rn(g, G, S, Cout, R, scale=max(R, 1) ** -0.5)
        p['b4'] = _rn(g, G, S, Cout, scale=0.3)
        p['A'] = _rn(g, G, S, V, V, scale=0.3)
        p['alpha'] = torch.full((G, 1), float(c['alpha'])) * (1 + 0.25 * torch.arange(G).float()[:, None])
        p['w3'] = _rn(g, G, S * Cout, Cin, scale=Cin ** -0.5)
        p['b3'] = _rn(g, G, S * Cout, scale=0.3)
        p['sy'] = _rn(g, G, Cout, scale=0.3, shift=1.0)
        p['ty'] = _rn(g, G, Cout, scale=0.3)
        p['wd'] = _rn(g, G, Cout, Cin, scale=Cin ** -0.5) if c['res_mode'] == 2 else None
        p['bd'] = _rn(g, G, Cout, scale=0.3) if c['res_mode'] == 2 else None
    elif stage == 'gemm':
        K, M = c['K'], c['M']
        p['x'] = _rn(g, N, K, T, V)
        p['add'] = _rn(g, N, M, T, V)
        p['w'] = _rn(g, G, M, K, scale=K ** -0.5)
        p['b'] = _rn(g, G, M, scale=0.3)
    else:
        Cb, nb, ks, Cin, Cout = c['Cb'], c['nb'], c['ks'], c['Cin'], c['Cout']
        h = _rn(g, N, Cout, T, V)
        h[:, nb * Cb:(nb + 1) * Cb] = -h[:, nb * Cb:(nb + 1) * Cb].abs() - 0.125   # a zero-padded maximum would win at the clip ends
        p['h'] = h
        p['x'] = _rn(g, N, Cin, T, V)
        p['wt'] = [_rn(g, G, Cb, Cb * ks, scale=(Cb * ks) ** -0.5) for _ in range(nb)]
        p['bt'] = [_rn(g, G, Cb, scale=0.3) for _ in range(nb)]
        p['sp'] = -(0.5 + torch.rand(G, Cb, generator=g))
        p['tp'] = _rn(g, G, Cb, scale=0.3, shift=1.0)
        p['wr'] = _rn(g, G, Cout, Cin, scale=Cin ** -0.5) if c['res_mode'] == 2 else None
        p['br'] = _rn(g, G, Cout, scale=0.3) if c['res_mode'] == 2 else None
    return p


PARAMS = {'e': ('w12', 'b12', 'w4', 'b4', 'A', 'alpha', 'w3', 'b3', 'sy', 'ty', 'wd', 'bd'),
          'gemm': ('w', 'b'), 'tcn': ('wt', 'bt', 'sp', 'tp', 'wr', 'br')}
PARAMS['gcn'] = PARAMS['e']
ACTS = {'e': ('x', 'xpart', 'E'), 'gcn': ('x', 'xpart', 'E'), 'gemm': ('x', 'add'), 'tcn': ('h', 'x')}


def sub(stage, p, g):
    """group g's problem: G = 1, its own parameters (no group axis) and sample rows"""
    G = p['G']
    npg = p['N'] // G
    q = dict(p, G=1, N=npg)
    for k in PARAMS[stage]:
        v = p[k]
        q[k] = None if v is None else [t[g] for t in v] if isinstance(v, list) else v[g]
    for k in ACTS[stage]:
        if p.get(k) is not None:
            q[k] = p[k][g * npg:(g + 1) * npg]
    return q


# ---------------------------------------------------------------------------------------------------------------------
# ctypes descriptors from a case and a dict of device tensors (a name absent or None: a NULL pointer)
# ---------------------------------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else t.data_ptr()


def gcn_desc(lib, c, V, t):
    return lib.F2GcnDesc(N=c['N'], Cin=c['Cin'], Cout=c['Cout'], T=c['T'], V=V, S=c.get('S', S), R=c['R'], res_mode=c['res_mode'],
                         **{k: _ptr(t.get(k)) for k in ('x', 'w12', 'b12', 'w4', 'b4', 'A', 'alpha', 'w3', 'b3', 'sy', 'ty', 'wd', 'bd',
                                                        'E', 'sum', 'diff', 'xpart')})


def gemm_desc(lib, c, V, t):
    return lib.F2GemmDesc(N=c['N'], K=c['K'], M=c['M'], T=c['T'], V=V, mode=c['mode'], relu_rows=c['relu_rows'],
                          **{k: _ptr(t.get(k)) for k in ('x', 'w', 'b', 'add', 'out')})


def tcn_desc(lib, c, V, t):
    d = lib.F2TcnDesc(N=c['N'], Cin=c['Cin'], Cout=c['Cout'], T=c['T'], V=V, stride=c['stride'], Cb=c['Cb'], nb=c['nb'], ks=c['ks'],
                      res_mode=c['res_mode'], **{k: _ptr(t.get(k)) for k in ('h', 'sp', 'tp', 'x', 'wr', 'br', 'out', 'xpart')})
    for i in range(min(c['nb'], 4)):
        d.dil[i] = c['dils'][i]
        d.wt[i] = _ptr(t['wt'][i])
        d.bt[i] = _ptr(t['bt'][i])
    return d


DESC = {'e': gcn_desc, 'gcn': gcn_desc, 'gemm': gemm_desc, 'tcn': tcn_desc}


def entry(lib, fam, stage, grouped):
    return getattr(lib, f'tamgcn_{fam}_{stage}{"_grouped" if grouped else ""}')


def launch(lib, fam, stage, d, groups=None, stream=None):
    st = C.c_void_p(stream)
    fn = entry(lib, fam, stage, groups is not None)
    return fn(C.byref(d), st) if groups is None else fn(C.byref(d), groups, st)
