"""fp64 references of the GEMM-family descriptors (tamgcn_conv, tamgcn_wgrad, the slab reductions) and the rounding bars
their results are held to.

A reference is evaluated twice in float64: once on the operands (`ref`) and once on their absolute values (`mag`: the same
expression with every input, coefficient and weight replaced by its magnitude, ReLU and masks left out).  An fp32 result
that sums L products in any order, each product of fp32-rounded operands, is within

    |got - ref| <= (L + 4) * 2^-24 * mag

element by element (the +4 covers the fp32 prologue act(c1*x1 + c2*x2 + c0), the bias, the post-affine and the residual
adds).  In split-bf16 mode every product is three bf16 products (3L), and the dropped lo*lo term and the operand
representation add 2^-15 * mag.  The bound is a worst case -- correct arithmetic cannot fail it -- yet a single missing,
extra or misplaced term of size ~mag/L breaks it whenever L is below ~4000.  Where L <= 4096 the result is also held to a
global bound, max|got - ref| / max|ref| <= 2e-6 (exact) / 3e-5 (split)."""
import numpy as np
import torch

EPS32 = 2.0 ** -24
SPLIT_DROP = 2.0 ** -15
GLOBAL_BAR = {False: 2e-6, True: 3e-5}
GLOBAL_MAX_L = 4096


class BarError(AssertionError):
    pass


def elementwise_bar(L, mag, split=False):
    return ((3 * L if split else L) + 4) * EPS32 * mag + (SPLIT_DROP * mag if split else 0.0)


def check(name, got, ref, mag, L, split=False, global_bound=True, allow=0.0):
    """Raise BarError unless got is within the element-wise rounding bound of ref (and, for L <= 4096, the global bound).
    got: any tensor (any device / dtype); ref, mag: float64 CPU tensors of the same shape; L: contraction length; allow: an
    element-wise additive allowance (a float64 tensor of that shape or a number) for an error source that is no fp32
    rounding of the sum, such as an approximated tanh inside an operand: it widens both bounds by exactly that much."""
    got = got.detach().to('cpu', torch.float64)
    if tuple(got.shape) != tuple(ref.shape):
        raise BarError(f'{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}')
    err = (got - ref).abs()
    lim = elementwise_bar(L, mag, split) + allow
    bad = ~(err <= lim)                                   # NaN fails
    if bool(bad.any()):
        idx = tuple(int(i) for i in np.unravel_index(int(torch.nonzero(bad.flatten())[0]), tuple(got.shape)))
        raise BarError(f'{name}: {int(bad.sum())} of {got.numel()} elements outside the L = {L} rounding bound '
                       f'({"split" if split else "exact"}); first at {idx}: got {float(got[idx]):.9g} '
                       f'ref {float(ref[idx]):.9g} bound {float(lim[idx]):.3g}')
    if global_bound and L <= GLOBAL_MAX_L:
        scale = float(ref.abs().max())
        over = (err - allow).clamp_min(0.0)                   # what the allowance does not explain
        rel = float(over.max()) / scale if scale > 0 else float(over.max())
        if rel > GLOBAL_BAR[split]:
            raise BarError(f'{name}: max|err|/max|ref| = {rel:.3g} > {GLOBAL_BAR[split]:.0e} (L = {L})')
    return float(err.max())


def check_untouched(name, got, before, keep):
    """Elements where `keep` is True must hold exactly what they held before the launch."""
    g, b = got.detach().cpu()[keep], before.detach().cpu()[keep]
    if not torch.equal(g, b):
        raise BarError(f'{name}: {int((g != b).sum())} elements outside the written region changed')


# ---------------------------------------------------------------------------------------------------------------------
# descriptor semantics (include/tamgcn.h) evaluated with torch on the CPU in a chosen dtype
# ---------------------------------------------------------------------------------------------------------------------
def _bc(c):
    return c[None, :, None, None]


def src_value(s, dt, absval=False):
    """act(c1*x1 + c2*x2 + c0) over all ctot channels of an operand dict {x1, x2, coef, act}."""
    f = (lambda t: t.to(dt).abs()) if absval else (lambda t: t.to(dt))
    x1, x2, cf = s['x1'], s.get('x2'), s.get('coef')
    if cf is None:
        v = f(x1)
    else:
        c = f(cf)
        v = _bc(c[0]) * f(x1) + _bc(c[2])
        if x2 is not None:
            v = v + _bc(c[1]) * f(x2)
    if s.get('act', 0) == 1 and not absval:
        v = torch.relu(v)
    return v


def conv_taps(xv, W, KT, dil, stride, pad, up, T_out):
    """y[n,m,t,v] = sum_k sum_tap W[m,k,tap] * X[n,k,th,v] with th = t*stride - pad + tap*dil over an input upsampled by
    `up` (th must be a multiple of up and reads frame th/up); zero outside [0, T_in)."""
    N, K, T_in, V = xv.shape
    y = torch.zeros(N, W.shape[0], T_out, V, dtype=xv.dtype)
    t = torch.arange(T_out)
    for tap in range(KT):
        th = t * stride - pad + tap * dil
        ok = th >= 0
        if up > 1:
            ok = ok & (th % up == 0)
            th = torch.div(th, up, rounding_mode='floor')
        ok = ok & (th < T_in)
        xs = xv[:, :, th.clamp(0, T_in - 1), :] * ok.to(xv.dtype)[None, None, :, None]
        y += torch.einsum('mk,nktv->nmtv', W[:, :, tap], xs)
    return y


def conv_eval(p, dt=torch.float64, absval=False):
    """The tamgcn_conv descriptor `p` (a dict of CPU tensors and ints) evaluated in dtype dt.  Returns (y, s1, s2): y the
    whole (N, yctot, T_y, V) output, starting from p['y0'] (what the launch does not write keeps y0); s1 / s2 the
    per-channel moments (M,) that the stats partial sums add up to (None without stats).  add1 / add2 = 'y' alias y0."""
    def f(t):
        return None if t is None else (t.to(dt).abs() if absval else t.to(dt))
    K, M, KT = p['K'], p['M'], p.get('KT', 1)
    src = p['src']
    c0 = src.get('coff', 0)
    xv = src_value(src, dt, absval)[:, c0:c0 + K]
    w = f(p['w'])
    w = w[..., 0] if w.dim() == 4 else w
    W = w.permute(1, 0, 2).flip(2) if p.get('wmode', 0) == 1 else w     # wmode 1: w[k][m][KT-1-tap] (the data gradient)
    y0 = p['y0']
    T_out, ostride, ycoff = p['T_out'], p.get('ostride', 1), p.get('ycoff', 0)
    acc = conv_taps(xv, W, KT, p.get('dil', 1), p.get('stride', 1), p.get('pad', 0), p.get('up', 1), T_out)
    tsel = torch.arange(T_out) * ostride

    def region(t, coff=ycoff):                                          # channels coff..coff+M, the written frames
        return t[:, coff:coff + M][:, :, tsel]
    val = acc
    if p.get('bias') is not None:
        val = val + _bc(f(p['bias']))
    if p.get('post_coef') is not None:
        pc = f(p['post_coef'])
        val = _bc(pc[0, ycoff:ycoff + M]) * val + _bc(pc[2, ycoff:ycoff + M])
    if p.get('bcast') is not None:
        val = val + f(p['bcast']).permute(1, 0, 2)[:, :, None, :] * (abs(p['bcast_scale']) if absval else p['bcast_scale'])
    for k in ('add1', 'add2'):
        a = p.get(k)
        if a is not None:
            val = val + region(f(y0 if isinstance(a, str) else a))
    if p.get('post_act', 0) == 1 and not absval:
        val = torch.relu(val)
    if p.get('mask') is not None and not absval:
        mk = p['mask']
        mv = region(src_value(mk, dt), mk.get('coff', 0))
        val = torch.where(mv > 0, val, torch.zeros((), dtype=dt))
    y = f(y0).clone()
    y[:, ycoff:ycoff + M, tsel] = val
    s1 = s2 = None
    if p.get('stats'):
        s1 = val.sum((0, 2, 3))
        x2 = val
        if p.get('aux') is not None:
            ac = p.get('auxcoff', 0)
            aux, ctr = region(f(p['aux']), ac), _bc(f(p['aux_center'])[ac:ac + M])
            x2 = aux + ctr if absval else aux - ctr
        s2 = (val * x2).sum((0, 2, 3))
    return y, s1, s2


def wgrad_eval(gy, src, M, K, KT=1, dil=1, stride=1, pad=0, dt=torch.float64, absval=False):
    """dW[m,k,tap] = sum_{n,t,v} gy(n,m,t,v) * x(n,k, t*stride + tap*dil - pad, v) over the prologue'd operands."""
    g = src_value(gy, dt, absval)[:, gy.get('coff', 0):gy.get('coff', 0) + M]
    x = src_value(src, dt, absval)[:, src.get('coff', 0):src.get('coff', 0) + K]
    T_out, T_in = g.shape[2], x.shape[2]
    out = torch.zeros(M, K, KT, dtype=dt)
    t = torch.arange(T_out)
    for tap in range(KT):
        th = t * stride + tap * dil - pad
        ok = (th >= 0) & (th < T_in)
        xs = x[:, :, th.clamp(0, T_in - 1)] * ok.to(dt)[None, None, :, None]
        out[:, :, tap] = torch.einsum('nmtv,nktv->mk', g, xs)
    return out
