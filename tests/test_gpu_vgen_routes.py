"""-m gpu: the ledger of the run-time-V CTRGC kernels (csrc/vgen.hip), built like tests/test_gpu_ctrgc_routes.py and on its
helpers.  Every case is one launch through the raw ABI on operands the test made, the kernel symbol the dispatch must pick
(tamgcn_last_kernel()) and the fp64 reference of THAT kernel (tests/ctrgc_ref.py, V-generic einsums) at the fp32-rounding
bars of tests/fp64_bars.py; two identical launches bit-equal; dy as a two-operand channel slice of a wider tensor whose other
channels are NaN; NaN in the slack floats behind every streamed operand.

Joint counts: 3 (VP = 16, almost all pad), 16 (an exact tile, no pads), 17 (one joint past a tile), 18, 23, 31: both padded
widths and every residue mod 4.  The streaming shapes are the V = 25 list of the templated ledger (a full 32-frame chunk plus a
ragged frame, a short chunk, T = 1, two chunks, T*V % 4 != 0 for odd V), thinned so that every V and every shape appears at
least twice.  At V = 25 and V = 32 the new entry points run beside the templated kernels on one shape each, and at V = 20, 25 and
32 the three streaming kernels of both families (one body, csrc/ctrgc_stream_body.h, under two geometry policies) must give
the same bits on every streaming shape of that list (BITEQ).

tests/test_vgen_cpu.py (CPU) checks that every instantiation vgen.hip dispatches to is launched here, that an fp32 torch
evaluation of every case passes its bars and that subtly wrong results do not.  Run with -s for the err / bound ratios."""
import ctypes as C

import pytest
import torch

import ctrgc_ref as R_
import test_gpu_ctrgc_routes as L

VS = (3, 16, 17, 18, 23, 31)
SHAPES = L.STREAM[25]                       # (N, Cout, T, S)
PAIRS = {3: (0, 2, 4), 16: (1, 3), 17: (0, 2, 4), 18: (1, 3), 23: (0, 4), 31: (1, 2, 3)}

CASES = {}


def _add(kind, sym, **kw):
    cid = kind + '_' + '_'.join(f'{k}{v}' for k, v in kw.items() if k != 'forms')
    assert cid not in CASES, cid
    CASES[cid] = dict(kind=kind, sym=sym, **kw)


def vp(V):
    return 16 if V <= 16 else 32


for _V, _idx in PAIRS.items():
    for _i in _idx:
        _N, _C, _T, _S = SHAPES[_i]
        _forms = ('plain', 'two', 'relu') if (_V, _i) == (17, 0) else ('plain', 'two')
        _add('aggfwd', f'vgen_agg_fwd_kernel<{vp(_V)}, {_S}>', V=_V, N=_N, C=_C, T=_T, S=_S)
        _add('aggbwd', f'vgen_agg_bwd_kernel<{vp(_V)}, {_S}>', V=_V, N=_N, C=_C, T=_T, S=_S, forms=_forms)
        _add('deacc', f'vgen_de_acc_kernel<{vp(_V)}, {_S}>', V=_V, N=_N, C=_C, T=_T, S=_S, forms=_forms)
for _V, _R, _S, _C in [(3, 4, 3, 16), (3, 32, 1, 48), (16, 20, 3, 16), (16, 4, 1, 48), (17, 32, 3, 16), (17, 20, 1, 48),
                       (18, 4, 3, 48), (18, 32, 1, 16), (23, 20, 3, 16), (23, 4, 1, 48), (31, 32, 3, 16), (31, 20, 1, 48)]:
    _add('E', 'vgen_E_kernel', V=_V, R=_R, S=_S, C=_C, N=2)
# tails: R <= 16 is RT = 1, above RT = 2; V = 31 at R = 32 stages the dE chunk in three column windows (one and three channel chunks)
for _V, _R, _S, _N, _C, _kw in [(3, 4, 3, 1, 16, {}), (16, 8, 1, 3, 48, {}), (17, 12, 3, 3, 16, {}), (17, 32, 1, 1, 48, {}),
                                (18, 20, 3, 1, 16, {}), (23, 32, 3, 3, 16, {}), (31, 32, 1, 3, 16, {}), (31, 8, 3, 1, 48, {}), (31, 32, 3, 1, 48, {}),
                                (17, 8, 3, 3, 32, dict(groups=2))]:
    _add('tail', f'vgen_de_tail_kernel<{1 if _R <= 16 else 2}>', V=_V, R=_R, S=_S, N=_N, C=_C, **_kw)
PINNED = {c['sym'] for c in CASES.values()}

# the templated kernels' own ledger cases the new entry points are run beside (tests/test_gpu_ctrgc_routes.py CASES)
CROSS = ['aggfwd_V25_N2_C16_T33_S3', 'aggbwd_V25_N2_C16_T33_S3', 'deacc_V25_N2_C16_T33_S3', 'E_V25_R8_S3_C48_N2', 'tail_V25_R8_S3_N3_C16',
         'aggfwd_V32_N2_C16_T33_S3', 'aggbwd_V32_N2_C16_T33_S3', 'deacc_V32_N2_C16_T33_S3', 'E_V32_R32_S3_C16_N2', 'tail_V32_R32_S1_N3_C16']

# the streaming kernels exist in both families for V = 20, 25 and 32: every shape of the V = 25 list, every dy form; the case
# carries both symbols (sym: the templated kernel, vsym: the run-time-V one)
STREAM_KINDS = ('aggfwd', 'aggbwd', 'deacc')
TEMPLATED = dict(aggfwd='ctrgc_agg_fwd_kernel', aggbwd='ctrgc_agg_bwd_kernel', deacc='ctrgc_de_acc_mfma_kernel')
VGEN = dict(aggfwd='vgen_agg_fwd_kernel', aggbwd='vgen_agg_bwd_kernel', deacc='vgen_de_acc_kernel')
BITEQ = {}
for _V in (20, 25, 32):
    for _N, _C, _T, _S in SHAPES:
        for _k in STREAM_KINDS:
            BITEQ[f'both_{_k}_V{_V}_N{_N}_C{_C}_T{_T}_S{_S}'] = dict(
                kind=_k, sym=f'{TEMPLATED[_k]}<{_V}, {_S}>', vsym=f'{VGEN[_k]}<{vp(_V)}, {_S}>', V=_V, N=_N, C=_C, T=_T, S=_S,
                forms=('plain', 'two', 'relu'), abi='tiled')


# ---------------------------------------------------------------------------------------------------------------------
# problems, references and bars: the templated ledger's functions on this table
# ---------------------------------------------------------------------------------------------------------------------
class _table:
    """Run a function of tests/test_gpu_ctrgc_routes.py on this module's case table (its functions look cases up by id)."""
    def __enter__(self):
        self.saved = L.CASES
        L.CASES = {**L.CASES, **CASES, **BITEQ}

    def __exit__(self, *exc):
        L.CASES = self.saved


def problem(cid):
    with _table():
        return L.problem(cid)


def evaluate(cid, p, dt):
    with _table():
        return L.evaluate(cid, p, dt)


def verify(cid, p, got):
    with _table():
        return L.verify(cid, p, got)


# ---------------------------------------------------------------------------------------------------------------------
# GPU runner: every kind through the raw vgen ABI
# ---------------------------------------------------------------------------------------------------------------------
def run_once(c, p, abi='tamgcn_vgen'):
    """Launch case c (a dict of this table's form) once through tamgcn_vgen_*: the dict evaluate() returns, on the device.
    The three streaming entry points of the templated family take the same arguments: abi='tamgcn_ctrgc_tiled' runs those."""
    k, N, Cout, S, V, sym = c['kind'], c['N'], c['C'], c['S'], c['V'], c['sym']
    assert abi == 'tamgcn_vgen' or k in STREAM_KINDS
    d = L._desc(c)
    out = {}
    if k == 'E':
        a = {n: L._dev(v) for n, v in p.items()}
        d.pq, d.w4, d.b4, d.A, d.alpha = (a[n].data_ptr() for n in ('pq', 'w4', 'b4', 'A', 'alpha'))
        E = L._out(N, S, Cout, V, V)
        L._launch('tamgcn_vgen_build_e', sym, C.byref(d), E.data_ptr())
        out['E'] = E
    elif k == 'tail':
        a = {n: L._dev(p[n]) for n in ('pq', 'w4', 'b4', 'alpha')}
        d.pq, d.w4, d.b4, d.alpha = (a[n].data_ptr() for n in ('pq', 'w4', 'b4', 'alpha'))
        G, R = c.get('groups', 1), c['R']
        for kind, dE in p['dE'].items():
            dEd = L._dev(dE)
            dA, dw4, db4, dal, dpq = L._out(N * G, S, V, V), L._out(N, S, Cout, R), L._out(N, S, Cout), L._out(N * S * G), L._out(G, S * 2 * R, N, V)
            L._launch('tamgcn_vgen_de_tail', sym, C.byref(d), dEd.data_ptr(), dA.data_ptr(), dw4.data_ptr(), db4.data_ptr(), dal.data_ptr(),
                      dpq.data_ptr(), G)
            res = dict(dA=dA.double().sum(0), db4=db4.double().sum(0), dW4=dw4.double().sum(0), dalpha=dal.double().sum().reshape(1),
                       dpq=dpq.double().sum(0))           # the partial slabs, summed here in fp64
            out.update({f'{kind}.{n}': res[n] for n in R_.TAIL_OUTPUTS})
            out[f'{kind}.raw'] = torch.cat([t.flatten() for t in (dA, dw4, db4, dal, dpq)])
    elif k == 'aggfwd':
        x3, E = L._dev(p['x3']), L._dev(p['E'])
        y, part = L._out(N, Cout, c['T'], V), L._out(2, Cout, N)
        L._launch(f'{abi}_agg_fwd', sym, C.byref(d), x3.data_ptr(), E.data_ptr(), y.data_ptr(), part.data_ptr())
        out.update(y=y, s1=part[0].double().sum(-1), s2=part[1].double().sum(-1))
        out['raw'] = part
    else:
        E, x3 = L._dev(p.get('E')), L._dev(p.get('x3'))
        for f, dy in p['dy'].items():
            s = L._sdev(dy)
            sc = s.c()
            if k == 'deacc':
                dE = L._out(N, S, Cout, V, V)
                L._launch(f'{abi}_de_acc', sym, C.byref(d), C.byref(sc), x3.data_ptr(), dE.data_ptr())
                out[f'{f}.dE'] = dE
                continue
            dx3, part = L._out(N, S * Cout, c['T'], V), L._out(N, S * Cout)
            L._launch(f'{abi}_agg_bwd', sym, C.byref(d), C.byref(sc), E.data_ptr(), dx3.data_ptr(), part.data_ptr())
            out[f'{f}.dx3'], out[f'{f}.db3'], out[f'{f}.raw'] = dx3, part.double().sum(0), part
    torch.cuda.synchronize()
    return out


def _results(got):
    return {n: v for n, v in got.items() if not n.endswith('raw')}


@pytest.mark.gpu
@pytest.mark.parametrize('cid', list(CASES))
def test_vgen_route(cid):
    c, p = CASES[cid], problem(cid)
    got = run_once(c, p)
    again = run_once(c, p)
    rat = verify(cid, p, _results(got))
    line = f'VGEN {cid} | {c["sym"]} | {L.shape_of(c)} | ' + ' '.join(f'{n}={v:.3f}' for n, v in rat.items())
    if c['kind'] == 'E':
        line += f' | tanh-attributable {L.tanh_attributable(p, c, got["E"]):.3e}'
    print(line)
    for n in got:
        assert torch.equal(got[n], again[n]), f'{cid}: {n}: two identical launches differ'


def vgen_twin(c):
    """The case of the templated ledger as the run-time-V entry points see it: same operands, the vgen symbol."""
    k, V, S = c['kind'], c['V'], c['S']
    sym = {'aggfwd': f'vgen_agg_fwd_kernel<{vp(V)}, {S}>', 'aggbwd': f'vgen_agg_bwd_kernel<{vp(V)}, {S}>',
           'deacc': f'vgen_de_acc_kernel<{vp(V)}, {S}>', 'E': 'vgen_E_kernel'}.get(k) or f'vgen_de_tail_kernel<{1 if c["R"] <= 16 else 2}>'
    return dict(c, sym=sym)


@pytest.mark.gpu
@pytest.mark.parametrize('cid', CROSS)
def test_vgen_beside_the_templated_kernel(cid):
    """V = 25 and V = 32: the new entry points on a case of the templated ledger, both held to that case's bars (each within
    its own bar of the fp64 reference; bit-equality is not asked: the tail sums its columns in another order)."""
    c, p = L.CASES[cid], L.problem(cid)
    old = L.run_once(cid, p)
    new = _results(run_once(vgen_twin(c), p))
    assert set(new) == set(old)
    ro, rn = L.verify(cid, p, old), L.verify(cid, p, new)
    if c['kind'] in STREAM_KINDS:
        for n in new:
            assert torch.equal(new[n], old[n]), f'{cid}: {n}: the two families differ'
    print(f'VGEN-CROSS {cid} | templated ' + ' '.join(f'{n}={v:.3f}' for n, v in ro.items()) + ' | vgen ' + ' '.join(f'{n}={v:.3f}' for n, v in rn.items()))


@pytest.mark.gpu
@pytest.mark.parametrize('cid', list(BITEQ))
def test_vgen_same_bits_as_the_templated_kernel(cid):
    """The streaming kernels are one body under a compile-time-V and a run-time-V policy: the same sums in the same order.  y,
    dx3, dE and the moment / db3 partial slabs of the two entry points must be the same words, on every streaming shape of the
    V = 25 list at V = 20, 25 and 32 and for every dy form (plain, two-operand slice between NaN channels, relu)."""
    c = BITEQ[cid]
    p = problem(cid)
    tpl = run_once(c, p, abi='tamgcn_ctrgc_tiled')
    vgn = run_once(dict(c, sym=c['vsym']), p)
    assert set(tpl) == set(vgn) and tpl
    for n in tpl:
        assert not torch.isnan(tpl[n]).any(), f'{cid}: {n}: NaN in the templated kernel\'s output'
        assert torch.equal(tpl[n], vgn[n]), f'{cid}: {n}: {int((tpl[n] != vgn[n]).sum())} words differ between the two policies'
