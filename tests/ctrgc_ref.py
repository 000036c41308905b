"""fp64 references of the CTRGC kernels (csrc/ctrgc.hip, ctrgc_de.hip, ctrgc_tiled.hip), one per KERNEL, and the bars their
results are held to (fp64_bars.check).

Convention of fp64_bars.conv_eval: every function is plain torch on the CPU in a chosen dtype; absval=True evaluates the same
expression with every operand replaced by its magnitude (ReLU left out, minus signs turned into plus, 1 - D^2 into 1 + D^2):
the `mag` of the rounding bound (L + 4) * 2^-24 * mag.  The reference of a linear kernel takes the tensors the kernel was
GIVEN (a random E, a random x3, a random dE), so one kernel's rounding never enters another kernel's bar.

Tensors: pq (S*2*R, N, V) rows [(s*2 + which)*R + r], which = 0 for p and 1 for q; w4 (S, Cout, R); b4 (S, Cout); A (S, V, V);
alpha (1,); E, dE (N, S, Cout, V, V); x3, dx3 (N, S*Cout, T, V); dy an operand dict of fp64_bars.src_value plus 'coff'.
D[n,s,r,u,v] = tanh(p[n,s,r,u] - q[n,s,r,v]).

The tanh allowance.  The kernels' fast_tanh is 1 - 2 / (exp(2x) + 1) from a hardware exp2 and a hardware reciprocal, 1 ulp
each: the exponent's relative error is <= (|2x| + 1) * 2^-23, which the factor 2e / (e + 1)^2 <= 1/2 weighs down to
<= 0.8 * 2^-23 wherever it matters; the quotient carries <= 2 ulp on a value <= 2 (4 * 2^-23); the subtraction 2^-24: about
5.3 * 2^-23 = 6.3e-7 < TANH_DELTA = 2^-20 absolute per tanh.  The fp32 difference p - q in front of it is off by
<= 2^-24 (|p| + |q|), and tanh' <= 1.  Both travel through the magnitude expression of whatever contains D."""
import torch

import fp64_bars as B

TANH_DELTA = 2.0 ** -20
F64 = torch.float64


def _f(dt, absval):
    return (lambda t: t.to(dt).abs()) if absval else (lambda t: t.to(dt))


def split_pq(pq, S, R, dt=F64):
    """p, q (N, S, R, V) out of pq (S*2*R, N, V)"""
    _, N, V = pq.shape
    x = pq.to(dt).view(S, 2, R, N, V)
    return x[:, 0].permute(2, 0, 1, 3), x[:, 1].permute(2, 0, 1, 3)


def D_of(pq, S, R, dt=F64):
    p, q = split_pq(pq, S, R, dt)
    return torch.tanh(p.unsqueeze(-1) - q.unsqueeze(-2))                      # (N, S, R, V, V)


def tanh_delta(pq, S, R):
    """Element-wise bound of |D_kernel - D| (N, S, R, V, V): the approximation and the rounded difference."""
    p, q = split_pq(pq, S, R)
    return TANH_DELTA + B.EPS32 * (p.abs().unsqueeze(-1) + q.abs().unsqueeze(-2))


# ---------------------------------------------------------------------------------------------------------------------
def E(pq, w4, b4, A, alpha, S, R, dt=F64, absval=False):
    """E[n,s,c,u,v] = alpha (sum_r W4[s,c,r] D[n,s,r,u,v] + b4[s,c]) + A[s,u,v];  L = R"""
    f = _f(dt, absval)
    D = f(D_of(pq, S, R, dt))
    return f(alpha) * (torch.einsum('scr,nsruv->nscuv', f(w4), D) + f(b4)[None, :, :, None, None]) + f(A)[None, :, None]


def E_allow(pq, w4, alpha, S, R):
    return alpha.double().abs() * torch.einsum('scr,nsruv->nscuv', w4.double().abs(), tanh_delta(pq, S, R))


def _x3v(x3, S, dt, absval):
    N, SC, T, V = x3.shape
    return _f(dt, absval)(x3).view(N, S, SC // S, T, V)


def dy_value(dy, Cout, dt=F64, absval=False):
    """The prologue'd dy over its Cout-channel slice (N, Cout, T, V)."""
    c0 = dy.get('coff', 0)
    return B.src_value(dy, dt, absval)[:, c0:c0 + Cout]


def agg_fwd(E_, x3, S, dt=F64, absval=False):
    """y[n,c,t,u] = sum_s sum_v E[n,s,c,u,v] x3[n,s,c,t,v] (L = S*V) and its per-channel moments sum y, sum y^2
    (L = N*T*V + S*V)"""
    f = _f(dt, absval)
    y = torch.einsum('nscuv,nsctv->nctu', f(E_), _x3v(x3, S, dt, absval))
    return y, y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))


def dx3(E_, dy, S, dt=F64, absval=False):
    """dx3[n,s*Cout+c,t,v] = sum_u E[n,s,c,u,v] dy[n,c,t,u] (L = V) and db3[s*Cout+c] = sum_{n,t,v} dx3 (L = N*T*V + V)"""
    N, _, Cout, V, _ = E_.shape
    g = torch.einsum('nscuv,nctu->nsctv', _f(dt, absval)(E_), dy_value(dy, Cout, dt, absval))
    g = g.reshape(N, S * Cout, g.shape[3], V)
    return g, g.sum((0, 2, 3))


def dE(dy, x3, S, dt=F64, absval=False):
    """dE[n,s,c,u,v] = sum_t dy[n,c,t,u] x3[n,s,c,t,v];  L = T"""
    xv = _x3v(x3, S, dt, absval)
    return torch.einsum('nctu,nsctv->nscuv', dy_value(dy, xv.shape[2], dt, absval), xv)


TAIL_OUTPUTS = ('dA', 'db4', 'dW4', 'dalpha', 'dpq')


def tail(dE_, pq, w4, b4, alpha, S, R, dt=F64, absval=False):
    """dE through E = alpha (W4 D + b4) + A:
       dA[s,u,v] = sum_{n,c} dE                          db4[s,c] = alpha sum_{n,u,v} dE
       dW4[s,c,r] = alpha sum_{n,u,v} dE D_r             dalpha = sum dE (W4 D + b4)
       g = alpha (1 - D^2) sum_c W4[c,r] dE;  dp = sum_v g;  dq = -sum_u g;  dpq in pq's layout"""
    f = _f(dt, absval)
    N, _, Cout, V, _ = dE_.shape
    g_, W, b, al = f(dE_), f(w4), f(b4), f(alpha)
    D = D_of(pq, S, R, dt)
    dA = g_.sum((0, 2))
    db_raw = g_.sum((0, 3, 4))
    dW_raw = torch.einsum('nscuv,nsruv->scr', g_, f(D))
    dalpha = ((W * dW_raw).sum() + (b * db_raw).sum()).reshape(1)
    dD = torch.einsum('scr,nscuv->nsruv', W, g_)
    g = al * ((1 + D * D) if absval else (1 - D * D)) * dD
    dp, dq = g.sum(-1), g.sum(-2)                                           # (N, S, R, V)
    if not absval:
        dq = -dq
    dpq = torch.stack([dp, dq], 2).permute(1, 2, 3, 0, 4).reshape(S * 2 * R, N, V)
    return dict(dA=dA, db4=al * db_raw, dW4=al * dW_raw, dalpha=dalpha, dpq=dpq)


def tail_allow(dE_, pq, w4, alpha, S, R):
    """The tanh allowance of the tail outputs that contain D (zero for dA, db4): delta through the magnitude expression;
    for dp / dq |d(1 - D^2)| <= 2 delta."""
    N, _, Cout, V, _ = dE_.shape
    a, W, al = dE_.double().abs(), w4.double().abs(), float(alpha.double().abs())
    dl = tanh_delta(pq, S, R)
    dW_raw = torch.einsum('nscuv,nsruv->scr', a, dl)
    g = al * 2 * dl * torch.einsum('scr,nscuv->nsruv', W, a)
    dpq = torch.stack([g.sum(-1), g.sum(-2)], 2).permute(1, 2, 3, 0, 4).reshape(S * 2 * R, N, V)
    return dict(dA=0.0, db4=0.0, dW4=al * dW_raw, dalpha=(W * dW_raw).sum().reshape(1), dpq=dpq)


def tail_L(dE_, R):
    """Contraction length per tail output, counted from dE's nonzero pattern (adding exact zeros is exact in fp32, so the
    bound (L_nz + 4) * 2^-24 * mag stays a worst case; for a dense dE these are N*Cout, N*V^2, N*V^2, N*S*Cout*V^2*(R+1)
    and Cout*V)."""
    nz = (dE_ != 0).double()
    dD = nz.sum(2)                                                          # (N, S, V, V): terms of one dG element
    return dict(dA=int(nz.sum((0, 2)).max()), db4=int(nz.sum((0, 3, 4)).max()), dW4=int(nz.sum((0, 3, 4)).max()),
                dalpha=int(nz.sum()) * (R + 1), dpq=int(max(dD.sum(-1).max(), dD.sum(-2).max())))


def check_tail(name, got, dE_, pq, w4, b4, alpha, S, R):
    """got: dict of the five tail outputs.  Every output against its bar; returns {output: max err/bound}."""
    ref = tail(dE_, pq, w4, b4, alpha, S, R)
    mag = tail(dE_, pq, w4, b4, alpha, S, R, absval=True)
    allow, L = tail_allow(dE_, pq, w4, alpha, S, R), tail_L(dE_, R)
    out = {}
    for k in TAIL_OUTPUTS:
        out[k] = ratio(got[k], ref[k], mag[k], L[k], allow[k])
        B.check(f'{name}: {k}', got[k], ref[k], mag[k], L[k], allow=allow[k])
    return out


def ratio(got, ref, mag, L, allow=0.0):
    """max over the elements of |got - ref| / bound (what B.check holds <= 1); NaN -> inf"""
    err = (got.detach().to('cpu', F64) - ref).abs()
    lim = B.elementwise_bar(L, mag) + allow
    r = torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    r = torch.nan_to_num(r, nan=float('inf'))
    return float(r.max())


# ---------------------------------------------------------------------------------------------------------------------
# the sparse dE of the tail cases
# ---------------------------------------------------------------------------------------------------------------------
def tail_u_edges(V):
    """First and last u, and both sides of every u-chunk edge of the tiled tail (chunks of 512 / V rows; none at V < 32)."""
    us = {0, V - 1}
    if V >= 32:
        ut = 512 // V
        for e in range(ut, V, ut):
            us |= {e - 1, e}
    return sorted(us)


def sparse_dE(N, S, Cout, V, R, seed):
    """dE that is zero except, per (subset, 16-channel tile), at one seeded (clip, channel of the tile) x every u of
    tail_u_edges with v alternating between the first and the last joint, plus the two remaining corners: few enough
    entries that dalpha's nonzero products number <= 4096."""
    g = torch.Generator().manual_seed(seed)
    d = torch.zeros(N, S, Cout, V, V)
    us = tail_u_edges(V)
    for s in range(S):
        for c0 in range(0, Cout, 16):
            n = int(torch.randint(0, N, (1,), generator=g))
            c = c0 + int(torch.randint(0, 16, (1,), generator=g))
            uv = [(u, (0, V - 1)[i % 2]) for i, u in enumerate(us)] + [(us[0], V - 1), (us[-1], (V - 1, 0)[(len(us) - 1) % 2])]
            for u, v in sorted(set(uv)):
                d[n, s, c, u, v] = (0.5 + float(torch.rand((), generator=g))) * (1 if float(torch.rand((), generator=g)) < 0.5 else -1)
    assert int((d != 0).sum()) * (R + 1) <= 4096, 'sparse dE: too many nonzero products for the dalpha bar'
    return d
