"""-m gpu: the ledger of the CTRGC backward, E-builder and streaming kernels (csrc/ctrgc.hip, ctrgc_de.hip, ctrgc_tiled.hip).
Every case is one kernel launch on operands the test made (a random E, a random x3, a random or sparse dE), the kernel
symbol the host dispatch must pick for it (tamgcn_last_kernel() after the launch) and the fp64 reference of THAT kernel
(tests/ctrgc_ref.py) at fp32-rounding bars (tests/fp64_bars.py), plus: two identical launches bit-equal; dy as a
two-operand channel slice act(c1 x1 + c2 x2 + c0) of a wider tensor whose other channels are NaN; every streamed operand
with NaN in the allocator's slack floats behind it.

tests/test_ctrgc_ref_cpu.py (CPU) checks that the reference's formulas are autograd's, that an fp32 torch evaluation of every
case below passes its bars, that subtly wrong results do not, and that every instantiation the three sources dispatch to is
pinned here or by the forward ledger (tests/test_gpu_ctrgc_fwd_forms.py), run by another test (ELSEWHERE) or listed in
UNREACHABLE with the reason no case launches it; both of those lists are empty.

Run with -s to see the measured err / bound ratios (profiles/ctrgc_route_bars.txt records one run)."""
import ctypes as C

import pytest
import torch

import ctrgc_fwd_ref as FR_
import ctrgc_ref as R_
import fp64_bars as B

G20 = 'Geo<20, 8, 2, 8, 16>'
G20W = 'Geo<20, 16, 2, 8, 32>'
NAN = float('nan')

CASES = {}


def _add(kind, sym, **kw):
    cid = kind + ('f' if kw.get('abi') == 'fused' else '') + '_' + '_'.join(f'{k}{v}' for k, v in kw.items() if k not in ('forms', 'abi'))
    assert cid not in CASES, cid
    CASES[cid] = dict(kind=kind, sym=sym, **kw)


# ---- streaming kernels: (N, Cout, T, S) per V.  T = 33: a full 32-frame chunk + one ragged frame; 31: one short chunk;
# 64: two full chunks; 7 / 33 at V = 25: T*V % 4 != 0 (the last 16-byte piece of a row runs into the next (n, c) row);
# V = 20 is built and exported but no op routes to it: pinned through the ABI
STREAM = {25: [(2, 16, 33, 3), (3, 16, 31, 3), (1, 48, 1, 1), (2, 16, 64, 3), (2, 16, 7, 3)],
          32: [(2, 16, 33, 3), (1, 16, 32, 1)],
          64: [(1, 16, 40, 3), (1, 32, 33, 1)],
          20: [(2, 16, 33, 3), (1, 16, 7, 1)]}
for _V, _shapes in STREAM.items():
    for _i, (_N, _C, _T, _S) in enumerate(_shapes):
        _forms = ('plain', 'two', 'relu') if (_V, _i) == (25, 0) else ('plain', 'two')
        _add('aggfwd', f'ctrgc_agg_fwd_kernel<{_V}, {_S}>', V=_V, N=_N, C=_C, T=_T, S=_S)
        _add('aggbwd', f'ctrgc_agg_bwd_kernel<{_V}, {_S}>', V=_V, N=_N, C=_C, T=_T, S=_S, forms=_forms)
        _add('deacc', f'ctrgc_de_acc_mfma_kernel<{_V}, {_S}>', V=_V, N=_N, C=_C, T=_T, S=_S, forms=_forms, abi='tiled')
# ---- the fused V = 20 backward: N in {1, 3, 9} (the grid is padded to 8 clips), Cout 24 = the 8-channel tile only,
# T around the 16-frame chunk; the ragged T with the two-operand dy
for _N, _C, _T, _S in [(1, 16, 1, 3), (3, 24, 15, 3), (9, 16, 17, 1), (3, 48, 40, 3), (1, 16, 16, 1), (3, 24, 17, 1)]:
    _add('dx3', f'ctrgc_bwd_dx3_kernel<{G20}, {_S}>', V=20, N=_N, C=_C, T=_T, S=_S, forms=('plain', 'two'))
for _N, _C, _T, _S in [(2, 16, 1, 3), (2, 48, 17, 1), (1, 16, 40, 3), (3, 16, 17, 3), (1, 48, 40, 1)]:
    _add('deacc', f'ctrgc_de_acc_kernel<AccGeo<20, {_S}>>', V=20, N=_N, C=_C, T=_T, S=_S, forms=('plain', 'two'), abi='fused')
# V = 25 of the same kernel (8-frame chunks, scalar loads): the ops route V = 25 to the MFMA kernel; pinned through the ABI
for _N, _C, _T, _S in [(2, 16, 9, 3), (1, 16, 17, 1)]:
    _add('deacc', f'ctrgc_de_acc_kernel<AccGeo<25, {_S}>>', V=25, N=_N, C=_C, T=_T, S=_S, forms=('plain', 'two'), abi='fused')
# ---- E builders: V x R x S x Cout thinned, every value of every factor at least twice
for _V, _R, _S, _C in [(20, 4, 3, 16), (20, 20, 3, 16), (20, 32, 1, 48), (25, 8, 3, 48), (25, 20, 1, 16), (25, 32, 3, 16),
                       (32, 4, 1, 48), (32, 8, 3, 16), (32, 32, 3, 16), (64, 4, 3, 16), (64, 8, 1, 16), (64, 20, 3, 16),
                       (64, 32, 1, 48)]:
    _add('E', f'ctrgc_E_kernel<{_V}>' if _V < 32 else f'ctrgc_E_tiled_kernel<{_V}>', V=_V, R=_R, S=_S, C=_C, N=2)
# ---- dE tails: the five forms of tamgcn_ctrgc_bwd_de_tail by V, R and pointer alignment, the tiled tail by V and RT
TAIL_DMA1, TAIL_DMA2 = 'ctrgc_de_tail_kernel<20, 1, 0>', 'ctrgc_de_tail_kernel<20, 2, 1>'
for _V, _R, _S, _N, _C, _sym, _kw in [
        (20, 4, 3, 1, 16, TAIL_DMA1, {}), (20, 8, 1, 3, 48, TAIL_DMA1, {}),
        (20, 12, 3, 3, 16, 'ctrgc_de_tail_reg_kernel<20, 1>', {}), (20, 16, 1, 1, 48, 'ctrgc_de_tail_reg_kernel<20, 1>', {}),
        (20, 20, 3, 1, 48, TAIL_DMA2, {}), (20, 32, 1, 3, 16, TAIL_DMA2, {}),
        (20, 8, 3, 1, 16, 'ctrgc_de_tail_reg_kernel<20, 1>', dict(w4off=1)),     # w4 one float into its storage: not 16-byte aligned
        (20, 32, 3, 1, 16, 'ctrgc_de_tail_reg_kernel<20, 2>', dict(w4off=1)),    # the only way to <20, 2>
        (20, 8, 3, 3, 32, TAIL_DMA1, dict(groups=2)),
        (25, 8, 3, 3, 16, 'ctrgc_de_tail_reg_kernel<25, 1>', {}), (25, 32, 1, 1, 48, 'ctrgc_de_tail_reg_kernel<25, 2>', {}),
        (32, 4, 3, 3, 16, 'ctrgc_de_tail_tiled_kernel<32, 1>', {}), (32, 8, 1, 1, 48, 'ctrgc_de_tail_tiled_kernel<32, 1>', {}),
        (32, 20, 3, 1, 48, 'ctrgc_de_tail_tiled_kernel<32, 2>', {}), (32, 32, 1, 3, 16, 'ctrgc_de_tail_tiled_kernel<32, 2>', {}),
        (64, 4, 1, 1, 48, 'ctrgc_de_tail_tiled_kernel<64, 1>', {}), (64, 8, 3, 3, 16, 'ctrgc_de_tail_tiled_kernel<64, 1>', {}),
        (64, 20, 3, 1, 16, 'ctrgc_de_tail_tiled_kernel<64, 2>', {}), (64, 32, 1, 1, 48, 'ctrgc_de_tail_tiled_kernel<64, 2>', {})]:
    _add('tail', _sym, V=_V, R=_R, S=_S, N=_N, C=_C, **_kw)

# The six forward instantiations of ctrgc.hip (the 8-channel tile included: ops.ctrgc_fwd(..., E=E) reaches it at Cout % 16 == 8)
# are pinned by the forward ledger, tests/test_gpu_ctrgc_fwd_forms.py, through the table of tests/ctrgc_fwd_ref.py: symbol-checked
# there, at the derived bars.  FWD_PINNED: instantiation -> the symbol the dispatch reports for it, for every form that table runs.
FWD_PINNED = {FR_.INSTANTIATION[k]: FR_.SYM[k] for k in sorted({c['form'] for c in FR_.CASES.values()})}
# instantiations another test of the suite runs without checking the symbol, and instantiations no case launches, with the reason
ELSEWHERE = {}
UNREACHABLE = {}
PINNED = {c['sym'] for c in CASES.values()} | set(FWD_PINNED)


# ---------------------------------------------------------------------------------------------------------------------
# problems: CPU tensors from the case's seed (shared with the CPU test, which evaluates them in fp32 torch)
# ---------------------------------------------------------------------------------------------------------------------
def _rnd(shape, g, lo=-1.0, hi=1.0):
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def seed_of(cid):
    return sum(map(ord, cid))


def make_dy(form, N, Cout, T, V, g):
    """'plain': one tensor of Cout channels; 'two' / 'relu': act(c1 x1 [+ c2 x2] + c0), c0 != 0, channels 4..4+Cout of
    Cout + 8, the other channels NaN."""
    if form == 'plain':
        return dict(x1=_rnd((N, Cout, T, V), g))
    ctot, coff = Cout + 8, 4
    outside = torch.ones(ctot, dtype=torch.bool)
    outside[coff:coff + Cout] = False
    d = dict(coef=_rnd((3, ctot), g, 0.5, 1.5) * torch.where(_rnd((3, ctot), g) < 0, -1.0, 1.0), coff=coff)
    for k in ('x1', 'x2') if form == 'two' else ('x1',):
        d[k] = _rnd((N, ctot, T, V), g)
        d[k][:, outside] = NAN
    if form == 'relu':
        d['act'] = 1
    return d


def _params(c, g):
    S, R, Cout, N, V = c['S'], c['R'], c['C'], c['N'], c['V']
    return dict(pq=_rnd((S * 2 * R, N, V), g), w4=_rnd((S, Cout, R), g) * (1.0 / R ** 0.5), b4=_rnd((S, Cout), g) * 0.1,
                A=_rnd((S, V, V), g) * 0.3, alpha=torch.tensor([0.7]))


def problem(cid):
    c = CASES[cid]
    g = torch.Generator().manual_seed(seed_of(cid))
    N, Cout, V, S = c['N'], c['C'], c['V'], c['S']
    k = c['kind']
    if k == 'E':
        return _params(c, g)
    if k == 'tail':
        p = _params(c, g)
        p['dE'] = dict(dense=_rnd((N, S, Cout, V, V), g), sparse=R_.sparse_dE(N, S, Cout, V, c['R'], seed_of(cid)))
        return p
    T = c['T']
    p = {}
    if k in ('aggfwd', 'aggbwd', 'dx3'):
        p['E'] = _rnd((N, S, Cout, V, V), g)
    if k in ('aggfwd', 'deacc'):
        p['x3'] = _rnd((N, S * Cout, T, V), g)
    if k != 'aggfwd':
        p['dy'] = {f: make_dy(f, N, Cout, T, V, g) for f in c['forms']}
    return p


def evaluate(cid, p, dt):
    """Every output of case cid from ctrgc_ref in dtype dt: {name: tensor}; per dy form / dE kind the name is prefixed."""
    c = CASES[cid]
    k, S = c['kind'], c['S']
    if k == 'E':
        return dict(E=R_.E(p['pq'], p['w4'], p['b4'], p['A'], p['alpha'], S, c['R'], dt))
    if k == 'tail':
        return {f'{kind}.{n}': v for kind, d in p['dE'].items()
                for n, v in R_.tail(d, p['pq'], p['w4'], p['b4'], p['alpha'], S, c['R'], dt).items()}
    if k == 'aggfwd':
        return dict(zip(('y', 's1', 's2'), R_.agg_fwd(p['E'], p['x3'], S, dt)))
    out = {}
    for f, dy in p['dy'].items():
        if k == 'deacc':
            out[f'{f}.dE'] = R_.dE(dy, p['x3'], S, dt)
        else:
            out[f'{f}.dx3'], out[f'{f}.db3'] = R_.dx3(p['E'], dy, S, dt)
    return out


def verify(cid, p, got):
    """Hold `got` (the dict evaluate() returns, from whatever computed it) to the bars; returns {name: max err / bound}."""
    c = CASES[cid]
    k, S, N, V = c['kind'], c['S'], c['N'], c['V']
    rat = {}

    def chk(name, ref, mag, L, allow=0.0, **kw):
        rat[name] = R_.ratio(got[name], ref, mag, L, allow)
        B.check(f'{cid}: {name}', got[name], ref, mag, L, allow=allow, **kw)
    if k == 'E':
        a = (p['pq'], p['w4'], p['b4'], p['A'], p['alpha'], S, c['R'])
        chk('E', R_.E(*a), R_.E(*a, absval=True), c['R'], R_.E_allow(p['pq'], p['w4'], p['alpha'], S, c['R']))
    elif k == 'tail':
        for kind, d in p['dE'].items():
            r = R_.check_tail(f'{cid} [{kind} dE]', {n: got[f'{kind}.{n}'] for n in R_.TAIL_OUTPUTS}, d, p['pq'], p['w4'], p['b4'],
                              p['alpha'], S, c['R'])
            rat.update({f'{kind}.{n}': v for n, v in r.items()})
    elif k == 'aggfwd':
        ref, mag = R_.agg_fwd(p['E'], p['x3'], S), R_.agg_fwd(p['E'], p['x3'], S, absval=True)
        P = N * c['T'] * V
        assert P <= 4000, 'moments: too many elements per channel for the bar to bite'
        chk('y', ref[0], mag[0], S * V)
        chk('s1', ref[1], mag[1], P + S * V)
        chk('s2', ref[2], mag[2], P + S * V)
    else:
        for f, dy in p['dy'].items():
            if k == 'deacc':
                chk(f'{f}.dE', R_.dE(dy, p['x3'], S), R_.dE(dy, p['x3'], S, absval=True), c['T'])
            else:
                ref, mag = R_.dx3(p['E'], dy, S), R_.dx3(p['E'], dy, S, absval=True)
                P = N * c['T'] * V
                assert P <= 4000, 'db3: too many elements per channel for the bar to bite'
                chk(f'{f}.dx3', ref[0], mag[0], V)
                chk(f'{f}.db3', ref[1], mag[1], P + V)
    return rat


# ---------------------------------------------------------------------------------------------------------------------
# GPU runners
# ---------------------------------------------------------------------------------------------------------------------
def _dev(t, off=0):
    """A device copy from ops.empty with NaN in the slack floats behind it (off: that many floats into its storage)."""
    from tam_gcn_amd import ops
    if t is None:
        return None
    like = torch.empty(0, device='cuda:0')
    base = ops.empty(t.numel() + off, like=like)
    flat = torch.empty(0, device='cuda:0').set_(base.untyped_storage())
    assert flat.numel() == t.numel() + off + ops.SLACK
    flat.fill_(NAN)
    out = base[off:].view(t.shape)
    out.copy_(t)
    return out


def _sdev(s):
    from tam_gcn_amd.ops import S
    return S(_dev(s['x1']), _dev(s.get('x2')), _dev(s.get('coef')), s.get('coff', 0), s.get('act', 0))


def _out(*shape):
    from tam_gcn_amd import ops
    return ops.empty(*shape, like=torch.empty(0, device='cuda:0')).fill_(NAN)


def _desc(c):
    from tam_gcn_amd import _lib
    d = _lib.CtrgcDesc()
    d.N, d.Cin, d.Cout, d.S, d.R, d.T, d.V = c['N'], 1, c['C'], c['S'], c.get('R', 0), c.get('T', 1), c['V']
    return d


def _launch(name, sym, *args):
    from tam_gcn_amd import _lib, ops
    lib = _lib.load()
    _lib.check(getattr(lib, name)(*args, ops._stream()), name)
    got = lib.tamgcn_last_kernel().decode()
    assert got == sym, f'{name}: dispatched {got}, ledger says {sym}'


def run_once(cid, p):
    """Launch case cid once: the dict evaluate() returns, as device tensors."""
    from helpers import record_kernels
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S as Src
    c = CASES[cid]
    k, N, Cout, S, V, sym = c['kind'], c['N'], c['C'], c['S'], c['V'], c['sym']
    d = _desc(c)
    out = {}
    if k == 'E':
        x = Src(torch.empty(N, 1, 1, V, device='cuda:0'))
        a = {n: _dev(v) for n, v in p.items()}
        with record_kernels() as rec:
            out['E'] = ops.ctrgc_build_E(x, a['pq'], None, None, a['w4'], a['b4'], a['A'], a['alpha'], 1, Cout, S, c['R'])
        assert [s for _, s in rec.seen] == [sym], f'{cid}: dispatched {rec.seen}, ledger says {sym}'
    elif k == 'tail':
        a = {n: _dev(p[n]) for n in ('pq', 'b4', 'alpha')}
        w4 = _dev(p['w4'], c.get('w4off', 0))
        assert (w4.data_ptr() % 16 != 0) == bool(c.get('w4off'))
        tail_abi = 'tamgcn_ctrgc_tiled_de_tail' if V >= 32 else 'tamgcn_ctrgc_bwd_de_tail'
        for kind, dE in p['dE'].items():
            with record_kernels() as rec:
                res = ops.ctrgc_bwd_de_tail(_dev(dE), a['pq'], w4, a['b4'], a['alpha'], c['R'], groups=c.get('groups', 1))
            seen = [s for n, s in rec.seen if n == tail_abi]
            assert seen == [sym], f'{cid}: dispatched {rec.seen}, ledger says {sym}'
            out.update({f'{kind}.{n}': v for n, v in zip(R_.TAIL_OUTPUTS, (res[0], res[2], res[1], res[3], res[4]))})
    elif k == 'aggfwd':
        x3, E = _dev(p['x3']), _dev(p['E'])
        y, part = _out(N, Cout, c['T'], V), _out(2, Cout, N)
        _launch('tamgcn_ctrgc_tiled_agg_fwd', sym, C.byref(d), x3.data_ptr(), E.data_ptr(), y.data_ptr(), part.data_ptr())
        out.update(y=y, s1=part[0].double().sum(-1), s2=part[1].double().sum(-1))
    else:
        E, x3 = _dev(p.get('E')), _dev(p.get('x3'))
        for f, dy in p['dy'].items():
            s = _sdev(dy)
            sc = s.c()
            if k == 'deacc':
                dE = _out(N, S, Cout, V, V)
                _launch('tamgcn_ctrgc_tiled_de_acc' if c['abi'] == 'tiled' else 'tamgcn_ctrgc_bwd_de_acc', sym, C.byref(d), C.byref(sc),
                        x3.data_ptr(), dE.data_ptr())
                out[f'{f}.dE'] = dE
                continue
            dx3, part = _out(N, S * Cout, c['T'], V), _out(N, S * Cout)
            if k == 'aggbwd':
                _launch('tamgcn_ctrgc_tiled_agg_bwd', sym, C.byref(d), C.byref(sc), E.data_ptr(), dx3.data_ptr(), part.data_ptr())
            else:
                x = torch.empty(N, 1, c['T'], V, device='cuda:0')
                d.x, d.E = Src(x).c(), E.data_ptr()
                _launch('tamgcn_ctrgc_bwd_dx3', sym, C.byref(d), C.byref(sc), dx3.data_ptr(), part.data_ptr())
            out[f'{f}.dx3'], out[f'{f}.db3'] = dx3, part.double().sum(0)
    torch.cuda.synchronize()
    return out


def shape_of(c):
    return ' '.join(f'{k}={c[k]}' for k in ('V', 'N', 'C', 'T', 'S', 'R', 'groups', 'w4off') if k in c)


def tanh_attributable(p, c, got):
    """max over E's elements of (|err| - rounding bound)+ / (|alpha| sum_r |W4|): the error per tanh that rounding of the
    R-term sum does not explain, against TANH_DELTA = 2^-20"""
    a = (p['pq'], p['w4'], p['b4'], p['A'], p['alpha'], c['S'], c['R'])
    err = (got.detach().cpu().double() - R_.E(*a)).abs() - B.elementwise_bar(c['R'], R_.E(*a, absval=True))
    w = float(p['alpha'].abs()) * p['w4'].double().abs().sum(-1)[None, :, :, None, None]
    return float((err.clamp_min(0) / w).max())


@pytest.mark.gpu
@pytest.mark.parametrize('cid', list(CASES))
def test_ctrgc_route(cid):
    c, p = CASES[cid], problem(cid)
    got = run_once(cid, p)
    again = run_once(cid, p)
    rat = verify(cid, p, got)
    line = f'ROUTE {cid} | {c["sym"]} | {shape_of(c)} | ' + ' '.join(f'{n}={v:.3f}' for n, v in rat.items())
    if c['kind'] == 'E':
        line += f' | tanh-attributable {tanh_attributable(p, c, got["E"]):.3e}'
    print(line)
    for n in got:
        assert torch.equal(got[n], again[n]), f'{cid}: {n}: two identical launches differ'
