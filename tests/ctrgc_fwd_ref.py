"""The fused V = 20 CTRGC forward (tamgcn_ctrgc_fwd, csrc/ctrgc.hip): its fp64 reference, the bars its results are held to, a
pure-Python mirror of the host dispatch and the case table of the ledger (tests/test_gpu_ctrgc_fwd_forms.py).

The forward takes E as an OPERAND (N, S, Cout, V*V): the cases feed it a seeded random E, so tanh and the E builder (pinned by
tests/test_gpu_ctrgc_routes.py) stay out of the bound.  Convention of fp64_bars: every expression is evaluated twice in float64,
on the operands (`ref`) and on their magnitudes (`mag`), and an fp32 result is held to (L + 4) * 2^-24 * mag element by element.

    x3[n, s*Cout + c, t, v] = sum_k W3[s*Cout + c, k] x[n, coff + k, t, v] + b3[s*Cout + c]               L = Cin
    y[n, c, t, u]           = sum_s sum_v E[n, s, c, u, v] x3[n, s*Cout + c, t, v]                        L = Cin + S*V
        mag_y = sum |E| mag_x3: the aggregation's own rounding is (S V) eps mag_y, the rounded x3 it consumes adds
        sum |E| (Cin + 1) eps mag_x3 = (Cin + 1) eps mag_y; the +4 of check() covers the rest
    part[0][c][n], part[1][c][n] = sum, sum of squares of THE DEVICE'S OWN STORED y over the (n, c) row    L = T*V
        magnitudes sum |y| and sum y^2: with y itself pinned, the moment bar stays at summation depth

No element is excluded anywhere: the forward has no ReLU, max or tanh.

A problem is a dict of CPU fp32 tensors: x (N, ctot, T, V) with the operand in channels coff .. coff + Cin (every other channel
NaN), w3 (S*Cout, Cin), b3 (S*Cout,), E (N, S, Cout, V, V), and the ints coff, Cin, Cout, S."""
import torch

import fp64_bars as B
from ctrgc_ref import ratio

F64 = torch.float64
V = 20
NAN = float('nan')
G20 = 'Geo<20, 8, 2, 8, 16>'
G20W = 'Geo<20, 16, 2, 8, 32>'

# form -> the symbol tamgcn_note_kernel writes for it, and the template instantiation the host launches
SYM = {
    'res16_3': f'ctrgc_fwd_kernel<{G20W}, 3>',
    'res16_1': f'ctrgc_fwd_kernel<{G20W}, 1>',
    'res8_3': f'ctrgc_fwd_kernel<{G20}, 3>',
    'res8_1': f'ctrgc_fwd_kernel<{G20}, 1>',
    'l2': f'ctrgc_fwd_kernel<{G20W}, 3, E from L2>',
    'fwd2': f'ctrgc_fwd2_kernel<{G20W}, 3>',
}
INSTANTIATION = {
    'res16_3': f'ctrgc_fwd_kernel<{G20W}, 3>',
    'res16_1': f'ctrgc_fwd_kernel<{G20W}, 1>',
    'res8_3': f'ctrgc_fwd_kernel<{G20}, 3>',
    'res8_1': f'ctrgc_fwd_kernel<{G20}, 1>',
    'l2': f'ctrgc_fwd_kernel<{G20W}, 3, false>',
    'fwd2': f'ctrgc_fwd2_kernel<{G20W}, 3, 2>',
}
SBK = {'res16_3': 32, 'res16_1': 32, 'res8_3': 16, 'res8_1': 16, 'l2': 32, 'fwd2': 16}      # input channels per GEMM stage
DEFAULT_MODE = 1                                                                              # TAMGCN_CTRGC_FWD2 unset
BT = 16                                                                                       # frames per chunk


# ---------------------------------------------------------------------------------------------------------------------
# the host dispatch of tamgcn_ctrgc_fwd (tests/test_ctrgc_fwd_ref_cpu.py holds it to the source text)
# ---------------------------------------------------------------------------------------------------------------------
def fwd_ct(Cout):
    return 8 if Cout % 16 else 16


def form_key(mode, Cin, Cout, S, x_aligned=True, w3_aligned=True):
    ct = fwd_ct(Cout)
    al16 = x_aligned and w3_aligned
    two = ct == 16 and S == 3 and mode != 0 and (Cin >= 64 or mode >= 2)
    if two and Cin % 16 == 0 and al16 and (mode == 2 or (mode == 1 and Cin >= 256)):
        return 'fwd2'
    if two:
        return 'l2'
    if ct == 16:
        return 'res16_3' if S == 3 else 'res16_1'
    return 'res8_3' if S == 3 else 'res8_1'


def form(mode, Cin, Cout, S, x_aligned=True, w3_aligned=True):
    """The symbol tamgcn_last_kernel() reports after tamgcn_ctrgc_fwd in a process whose TAMGCN_CTRGC_FWD2 is `mode`."""
    return SYM[form_key(mode, Cin, Cout, S, x_aligned, w3_aligned)]


# ---------------------------------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------------------------------
TS = (1, 15, 16, 17, 33, 40)        # one short chunk; one frame short of a chunk; one chunk; 16 + 1; 16 + 16 + 1; 16 + 16 + 8
NS = (1, 3, 9)                      # a grid of 8 ceil(N / 8) clip slots: 7 idle, 5 idle, a second group of eight with 7 idle
CO16, CO8 = (16, 32, 48), (8, 24, 40)
CASES = {}


def shape_key(c):
    return (f'N{c["N"]}_Ci{c["Cin"]}_Co{c["Cout"]}_T{c["T"]}_S{c["S"]}' + ('_sl' if c['sl'] else '') + ('_xoff' if c['xoff'] else '')
            + ('_w3off' if c['w3off'] else ''))


def _add(mode, fk, N, Cin, Cout, T, S=3, sl=0, xoff=0, w3off=0, xform=False):
    c = dict(mode=mode, form=fk, sym=SYM[fk], N=N, Cin=Cin, Cout=Cout, T=T, S=S, sl=sl, xoff=xoff, w3off=w3off, xform=xform)
    cid = f'm{mode}_{fk}_{shape_key(c)}' + ('_x' if xform else '')
    assert cid not in CASES, cid
    assert form_key(mode, Cin, Cout, S, not xoff, not w3off) == fk, cid
    assert N <= 9 and T <= 40 and Cout <= 48, cid
    CASES[cid] = c


def _grid(mode, fk, S, couts, variants, n=12):
    """n cases over T x N x Cout x variants, thinned: T in turn, the other three on strides that do not repeat with it"""
    nv = len(variants)
    for i in range(n):
        v = dict(variants[(i + i // nv) % nv])
        if i % 4 == 3 and not v.get('xoff'):
            v.setdefault('sl', 1)
        _add(mode, fk, NS[(i + i // 6) % 3], Cout=couts[(2 * i + i // 6) % 3], T=TS[i % 6], S=S, **v)


# ---- mode 1 (the default; the pytest process itself)
_grid(1, 'res16_3', 3, CO16, [dict(Cin=3), dict(Cin=35), dict(Cin=48)])           # 35: a K tail of 3 inside the second stage; 48 = 32 + 16
_grid(1, 'res16_1', 1, CO16, [dict(Cin=3), dict(Cin=80), dict(Cin=96)])
_grid(1, 'l2', 3, CO16, [dict(Cin=64), dict(Cin=72), dict(Cin=128), dict(Cin=260),  # 72: a tail of 8; 260: >= 256, no multiple of 16
                         dict(Cin=256, w3off=1), dict(Cin=256, xoff=1)])            # the al16 fallback of the fwd2 route
for _i in range(12):                                                                # fwd2: Cin = 256 at every T, plain and as a slice
    _add(1, 'fwd2', NS[(_i + _i // 6) % 3], 256, CO16[(2 * _i + _i // 6) % 3], TS[_i % 6], sl=_i // 6)
_add(1, 'fwd2', 3, 272, 32, 33)                                                     # nk = 17
_grid(1, 'res8_3', 3, CO8, [dict(Cin=3), dict(Cin=16), dict(Cin=20), dict(Cin=64)])  # 20: a tail of 4 behind a 16-channel stage
_grid(1, 'res8_1', 1, CO8, [dict(Cin=3), dict(Cin=16), dict(Cin=20), dict(Cin=64)])
# ---- mode 2 (child): fwd2 at nk = 1, 2, 3, 5; the E-from-L2 form where fwd2 does not apply
for _i, (_Cin, _T) in enumerate([(16, 1), (32, 17), (48, 33), (80, 40), (16, 33), (32, 40), (48, 1), (80, 17)]):
    _add(2, 'fwd2', NS[_i % 3], _Cin, CO16[(_i + _i // 3) % 3], _T)
_add(2, 'fwd2', 3, 32, 32, 17, sl=1)
_add(2, 'l2', 3, 3, 16, 15)
_add(2, 'l2', 1, 20, 48, 33)
_add(2, 'l2', 9, 16, 32, 17, w3off=1)
# ---- mode 3 (child): the E-from-L2 form everywhere
for _N, _Cin, _Cout, _T in [(1, 3, 32, 15), (3, 16, 48, 17), (9, 48, 16, 33), (3, 256, 32, 40)]:
    _add(3, 'l2', _N, _Cin, _Cout, _T)
# ---- mode 0 (child): the resident-E form at Cin mode 1 never sends there
_add(0, 'res16_3', 3, 64, 32, 33)
_add(0, 'res16_3', 1, 256, 48, 33)
# ---- the three 16-channel S = 3 forms on the SAME operands, once per mode that serves the shape (every mode does): their
# outputs' digests are compared across the processes
XFORM = [(3, 16, 17), (1, 64, 40), (9, 256, 17), (1, 256, 40)]                     # N, Cin, T at Cout = 48
for _mode in (0, 1, 2, 3):
    for _N, _Cin, _T in XFORM:
        _add(_mode, form_key(_mode, _Cin, 48, 3), _N, _Cin, 48, _T, xform=True)


def cases_of(mode):
    return [cid for cid, c in CASES.items() if c['mode'] == mode]


def features(c):
    """The paths of its kernel a case reaches (tests/test_ctrgc_fwd_ref_cpu.py holds the table to required_paths)."""
    f = set()
    fk, Cin, T, N = c['form'], c['Cin'], c['T'], c['N']
    nchunks = -(-T // BT)
    if fk == 'fwd2':
        nk = Cin // 16
        f |= {f'nk={nk}'} if nk in (1, 2, 16) else {'nk odd >= 3'} if nk % 2 else set()
    else:
        sbk = SBK[fk]
        if Cin % sbk:
            f.add('K tail inside the first stage' if Cin < sbk else 'K tail behind a full stage')
        if c['w3off']:
            f.add('w3off')
        if c['xoff']:
            f.add('xoff')
    if T < BT:
        f.add('T < 16')
    if T > BT and T % BT == 1:
        f.add('one-frame last chunk')
    if nchunks >= 3:
        f.add('three chunks')
    if c['sl']:
        f.add('x slice')
    f |= {f'N={N}', f'Cout={c["Cout"]}', f'S={c["S"]}'}
    return f


required_paths = {
    'fwd2': ['nk=1', 'nk=2', 'nk odd >= 3', 'nk=16', 'T < 16', 'one-frame last chunk', 'three chunks', 'x slice', 'N=1', 'N=9'],
    'res16_3': ['K tail inside the first stage', 'K tail behind a full stage'],
    'res16_1': ['K tail inside the first stage', 'K tail behind a full stage'],
    'l2': ['K tail inside the first stage', 'K tail behind a full stage', 'w3off', 'xoff'],
    'res8_3': ['K tail inside the first stage', 'K tail behind a full stage', 'Cout=8'],
    'res8_1': ['K tail inside the first stage', 'K tail behind a full stage', 'Cout=8', 'S=1'],
}


# ---------------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------------
def _rnd(shape, g, lo=-1.0, hi=1.0):
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def seed_of(c):
    """From the shape alone: the cases of one shape in different modes get the same operands."""
    return sum(map(ord, shape_key(c)))


def make_problem(N, Cin, Cout, T, S, sl, seed):
    g = torch.Generator().manual_seed(seed)
    ctot, coff = (Cin + 8, 4) if sl else (Cin, 0)
    x = torch.full((N, ctot, T, V), NAN)
    x[:, coff:coff + Cin] = _rnd((N, Cin, T, V), g)
    return dict(x=x, w3=_rnd((S * Cout, Cin), g) * (1.0 / Cin ** 0.5), b3=_rnd((S * Cout,), g) * 0.1,
                E=_rnd((N, S, Cout, V, V), g) * 0.5, coff=coff, Cin=Cin, Cout=Cout, S=S)


def problem(cid, which=0):
    """Operands A (which = 0) or B (1) of case cid."""
    c = CASES[cid]
    return make_problem(c['N'], c['Cin'], c['Cout'], c['T'], c['S'], c['sl'], 2 * seed_of(c) + which)


# ---------------------------------------------------------------------------------------------------------------------
# reference and bars
# ---------------------------------------------------------------------------------------------------------------------
def reference(p, dt=F64, absval=False):
    """(x3 (N, S*Cout, T, V), y (N, Cout, T, V)) in dtype dt; absval: the same expressions on magnitudes."""
    f = (lambda t: t.to(dt).abs()) if absval else (lambda t: t.to(dt))
    x = f(p['x'][:, p['coff']:p['coff'] + p['Cin']])
    x3 = torch.einsum('ok,nktv->notv', f(p['w3']), x) + f(p['b3'])[None, :, None, None]
    N, _, T, _ = x3.shape
    y = torch.einsum('nscuv,nsctv->nctu', f(p['E']), x3.view(N, p['S'], p['Cout'], T, V))
    return x3, y


def moments(y, dt=F64, absval=False):
    """part (2, Cout, N) of a y (N, Cout, T, V): [0][c][n] = sum over the (n, c) row, [1][c][n] = sum of squares"""
    y = y.to(dt)
    return torch.stack([(y.abs() if absval else y).sum((2, 3)).t(), (y * y).sum((2, 3)).t()])


def evaluate(p, dt):
    """What a launch with both output pointers delivers, from torch on the CPU in dtype dt: {y, x3, part}"""
    x3, y = reference(p, dt)
    return dict(y=y, x3=x3, part=moments(y, dt))


def verify(name, p, got):
    """Hold got = {y, x3 or None, part or None} (from whatever computed it) to the bars; returns {quantity: max err / bound}."""
    x3r, yr = reference(p)
    x3m, ym = reference(p, absval=True)
    Cin, S = p['Cin'], p['S']
    T = yr.shape[2]
    todo = [('y', got['y'], yr, ym, Cin + S * V)]
    if got.get('x3') is not None:
        todo.insert(0, ('x3', got['x3'], x3r, x3m, Cin))
    if got.get('part') is not None:
        yd = got['y'].detach().to('cpu', F64)                     # the moments of the y that was stored
        todo.append(('part', got['part'], moments(yd), moments(yd, absval=True), T * V))
    rat = {}
    for q, g, ref, mag, L in todo:
        rat[q] = ratio(g, ref, mag, L)                          # ctrgc_ref's: max err / bound, NaN -> inf
        B.check(f'{name}: {q}', g, ref, mag, L)
    return rat
