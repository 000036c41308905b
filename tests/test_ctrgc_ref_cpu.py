"""CPU: the CTRGC route ledger (tests/test_gpu_ctrgc_routes.py) stays complete, its fp64 references (tests/ctrgc_ref.py) are
autograd's formulas, an fp32 torch evaluation of every GPU case stays inside every bar, and the bars have teeth."""
import glob
import os
import re

import pytest
import torch

import ctrgc_ref as CR
import fp64_bars as B
import test_gpu_ctrgc_routes as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tam_gcn_amd', 'csrc')
GEO = {'G20': L.G20, 'G20W': L.G20W}


# ---------------------------------------------------------------------------------------------------------------------
# ledger completeness
# ---------------------------------------------------------------------------------------------------------------------
def source_symbols():
    """The kernel instantiation behind every literal dispatch site of csrc/ctrgc*.hip, as '<kernel><template arguments>'."""
    found = []
    for path in sorted(glob.glob(os.path.join(CSRC, 'ctrgc*.hip'))):
        src = open(path).read()
        found += [f'ctrgc_de_acc_kernel<AccGeo<{v}, {s}>>' for v, s in re.findall(r'\bDE_ACC_CASE\((\d+), (\d+)\)', src)]
        found += [f'ctrgc_de_tail_kernel<{v}, {rt}, {int(dbr == "true")}>'
                  for v, rt, dbr in re.findall(r'\bDE_TAIL_CASE\((\d+), (\d+), (true|false)\)', src)]
        found += [f'ctrgc_de_tail_reg_kernel<{v}, {rt}>' for v, rt in re.findall(r'\bDE_TAIL_REG_CASE\((\d+), (\d+)\)', src)]
        found += [f'{k}<{v}, {s}>' for k, v, s in re.findall(r'\bTL_CASE\((\w+), (\d+), (\d+),', src)]
        found += [f'ctrgc_de_tail_tiled_kernel<{v}, {rt}>' for v, rt in re.findall(r'\bTL_TAIL_CASE\((\d+), (\d+)\)', src)]
        found += [f'{k}<{GEO[g]}, {s}>' for k, g, s in re.findall(r'\bCTRGC_LAUNCH\((\w+), (G20W?), (\d+),', src)]
        for k, args in re.findall(r'(?:hipLaunchKernelGGL\(\(|tg_launch_lds<)(ctrgc_\w+)<([^<>()]*)>', src):   # launches outside the macros
            args = [a.strip() for a in args.split(',')]
            if all(re.fullmatch(r'\d+|true|false|G20W?', a) for a in args):                     # a macro's own launch has parameter names
                found.append(f'{k}<{", ".join(GEO.get(a, a) for a in args)}>')
    return found


def test_every_dispatch_site_is_pinned_elsewhere_or_unreachable():
    found = source_symbols()
    assert len(found) >= 50, sorted(found)                               # the extraction itself still works
    found = set(found)
    assert {'ctrgc_E_kernel<25>', 'ctrgc_E_tiled_kernel<32>', f'ctrgc_bwd_dx3_kernel<{L.G20}, 1>'} <= found
    missing = sorted(k for k in found if k not in L.PINNED and k not in L.ELSEWHERE and k not in L.UNREACHABLE)
    assert not missing, f'CTRGC instantiations without a ledger case, ELSEWHERE or UNREACHABLE entry: {missing}'
    stale = sorted(k for k in list(L.PINNED) + list(L.ELSEWHERE) + list(L.UNREACHABLE) if k not in found)
    assert not stale, f'ledger entries for instantiations the sources no longer have: {stale}'
    both = sorted(k for k in list(L.UNREACHABLE) + list(L.ELSEWHERE) if k in L.PINNED)
    assert not both, f'listed as unreachable / elsewhere but pinned by a case: {both}'
    assert all(L.UNREACHABLE.values()) and all(L.ELSEWHERE.values())
    # the fused forward: all six instantiations of ctrgc.hip, each through a case of the forward ledger that asserts the symbol
    # the dispatch reports for it -- none is merely run elsewhere, none is unreachable
    fwd = {k for k in found if k.startswith(('ctrgc_fwd_kernel<', 'ctrgc_fwd2_kernel<'))}
    assert len(fwd) == 6 and fwd == set(L.FWD_PINNED), sorted(fwd ^ set(L.FWD_PINNED))
    assert not [k for k in list(L.ELSEWHERE) + list(L.UNREACHABLE) if 'fwd' in k]
    import ctrgc_fwd_ref as FR
    for inst, sym in L.FWD_PINNED.items():
        assert any(c['sym'] == sym and FR.INSTANTIATION[c['form']] == inst for c in FR.CASES.values()), inst
    assert not any(k in L.FWD_PINNED for c in L.CASES.values() for k in (c['sym'],))


def test_case_table_covers_what_it_promises():
    t = [c for c in L.CASES.values() if c['kind'] == 'tail']
    assert {c['S'] for c in t} == {1, 3} and {c['N'] for c in t} == {1, 3} and {16, 48} <= {c['C'] for c in t}
    e = [c for c in L.CASES.values() if c['kind'] == 'E']
    for key, vals in (('V', (20, 25, 32, 64)), ('R', (4, 8, 20, 32)), ('S', (1, 3)), ('C', (16, 48))):
        for v in vals:
            assert sum(c[key] == v for c in e) >= 2, (key, v)
    d = [c for c in L.CASES.values() if c['kind'] == 'dx3']
    assert {c['N'] for c in d} == {1, 3, 9} and {c['C'] for c in d} == {16, 24, 48} and {c['T'] for c in d} == {1, 15, 16, 17, 40}
    assert all(c['N'] <= 9 and c['C'] <= 48 and c.get('T', 1) <= 70 for c in L.CASES.values())
    for V in (20, 25, 32, 64):                                            # the sparse dE touches both sides of every chunk edge
        us = CR.tail_u_edges(V)
        assert us[0] == 0 and us[-1] == V - 1 and len(us) == (2 if V < 32 else 2 * (V // (512 // V)))
    d = CR.sparse_dE(3, 3, 48, 64, 20, 5)
    nz = d != 0
    assert bool(nz.view(3, 3, 3, 16, 64, 64).any(3).any(0).flatten(2).any(2).all()), 'a (subset, channel tile) without an entry'
    assert bool(nz[..., 0].any() and nz[..., 63].any() and nz[..., 0, :].any() and nz[..., 63, :].any())
    assert set(torch.nonzero(nz.any(0).any(0).any(0).any(-1)).flatten().tolist()) == set(CR.tail_u_edges(64))


# ---------------------------------------------------------------------------------------------------------------------
# the reference's gradient formulas are autograd's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,V', [(1, 20), (3, 20), (1, 25), (3, 25)])
def test_reference_gradients_equal_autograd_of_the_fp64_forward(S, V):
    g = torch.Generator().manual_seed(S * 100 + V)
    N, Cout, T, R = 2, 16, 5, 8
    r = lambda *s: (torch.rand(s, generator=g, dtype=torch.float64) * 2 - 1)                 # noqa: E731
    pq, w4, b4, A, alpha = r(S * 2 * R, N, V), r(S, Cout, R) * 0.35, r(S, Cout) * 0.1, r(S, V, V) * 0.3, torch.tensor([0.7], dtype=torch.float64)
    x3 = r(N, S * Cout, T, V)
    for t in (pq, w4, b4, A, alpha, x3):
        t.requires_grad_(True)
    E = CR.E(pq, w4, b4, A, alpha, S, R)
    E.retain_grad()
    y, _, _ = CR.agg_fwd(E, x3, S)
    ctot = Cout + 8
    dy = dict(x1=r(N, ctot, T, V), x2=r(N, ctot, T, V), coef=r(3, ctot), coff=4)
    (y * CR.dy_value(dy, Cout)).sum().backward()
    E_, x3_ = E.detach(), x3.detach()
    det = [t.detach() for t in (pq, w4, b4, alpha)]

    def same(name, a, b):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), name
    same('dx3', CR.dx3(E_, dy, S)[0], x3.grad)
    dE = CR.dE(dy, x3_, S)
    same('dE', dE, E.grad)
    t = CR.tail(dE, det[0], det[1], det[2], det[3], S, R)
    same('dA', t['dA'], A.grad)
    same('db4', t['db4'], b4.grad)
    same('dW4', t['dW4'], w4.grad)
    same('dalpha', t['dalpha'], alpha.grad)
    same('dpq', t['dpq'], pq.grad)


# ---------------------------------------------------------------------------------------------------------------------
# the reference alone stays inside every bar: an fp32 torch evaluation of every GPU case, dense and sparse
# ---------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _case(cid):
    if cid not in _CACHE:
        p = L.problem(cid)
        _CACHE[cid] = (p, L.evaluate(cid, p, torch.float32))
    return _CACHE[cid]


@pytest.mark.parametrize('cid', list(L.CASES))
def test_checker_accepts_fp32_torch(cid):
    p, got = _case(cid)
    rat = L.verify(cid, p, got)
    assert rat and max(rat.values()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the checker rejects what a subtly wrong kernel would deliver (each on the smallest case that has the feature)
# ---------------------------------------------------------------------------------------------------------------------
F32 = torch.float32
RAGGED = 'V25_N2_C16_T33_S3'                                      # T = 33: chunks 32 + 1 of the streaming kernels


def _rejects(cid, p, got, **over):
    L.verify(cid, p, got)                                          # the unmutated fp32 evaluation passes ...
    with pytest.raises(B.BarError):
        L.verify(cid, p, dict(got, **over))                        # ... the mutated one does not


def _ext_dy(dy):
    """dy with one more frame whose prologue'd value is c0 (x1 = x2 = 0): what a row past T holds if the constant leaks."""
    d = dict(dy)
    for k in ('x1', 'x2'):
        d[k] = torch.cat([dy[k], torch.zeros_like(dy[k][:, :, :1])], 2)
    return d


def test_rejects_a_dropped_ragged_chunk():
    cid = 'aggfwd_' + RAGGED
    p, got = _case(cid)
    y = got['y'].clone()
    y[:, :, 32:] = 0
    _rejects(cid, p, got, y=y)
    cid = 'deacc_' + RAGGED
    p, got = _case(cid)
    dy = {k: (v[:, :, :32] if k in ('x1', 'x2') else v) for k, v in p['dy']['two'].items()}
    _rejects(cid, p, got, **{'two.dE': CR.dE(dy, p['x3'][:, :, :32], 3, F32)})


def test_rejects_the_prologue_constant_leaking_into_rows_past_T():
    cid = 'deacc_' + RAGGED
    p, got = _case(cid)
    x3 = p['x3']                                                   # the frame behind a row's last one is the next row's first
    nxt = x3.flatten(0, 1).roll(-1, 0).view_as(x3)[:, :, :1]
    leak = CR.dE(_ext_dy(p['dy']['two']), torch.cat([x3, nxt], 2), 3, F32)
    _rejects(cid, p, got, **{'two.dE': leak})
    cid = 'aggbwd_' + RAGGED
    p, got = _case(cid)
    _, db3 = CR.dx3(p['E'], _ext_dy(p['dy']['two']), 3, F32)  # E^T c0 of ONE row past T summed into db3
    _rejects(cid, p, got, **{'two.db3': db3})


def test_rejects_E_transposed_and_subsets_swapped():
    cid = 'dx3_V20_N1_C16_T1_S3'
    p, got = _case(cid)
    for f in ('plain', 'two'):
        dx3, db3 = CR.dx3(p['E'].transpose(-1, -2), p['dy'][f], 3, F32)
        _rejects(cid, p, got, **{f'{f}.dx3': dx3})
    Esw = p['E'][:, [1, 0, 2]]
    _rejects(cid, p, got, **{'plain.dx3': CR.dx3(Esw, p['dy']['plain'], 3, F32)[0]})
    cid = 'aggfwd_' + RAGGED
    p, got = _case(cid)
    N, SC, T, V = p['x3'].shape
    xsw = p['x3'].view(N, 3, SC // 3, T, V)[:, [0, 2, 1]].reshape(N, SC, T, V)
    y, s1, s2 = CR.agg_fwd(p['E'], xsw, 3, F32)
    _rejects(cid, p, got, y=y)
    _rejects(cid, p, got, s1=s1)


def _tail_one(cid, p, kind, name, val):
    """Only output `name` of the `kind` dE against its own bar."""
    c = L.CASES[cid]
    a = (p['dE'][kind], p['pq'], p['w4'], p['b4'], p['alpha'], c['S'], c['R'])
    ref, mag = CR.tail(*a)[name], CR.tail(*a, absval=True)[name]
    B.check(f'{cid} [{kind}] {name}', val, ref, mag, CR.tail_L(a[0], c['R'])[name],
            allow=CR.tail_allow(a[0], a[1], a[2], a[4], c['S'], c['R'])[name])


def _tail_with(cid, p, kind, dE):
    c = L.CASES[cid]
    return CR.tail(dE, p['pq'], p['w4'], p['b4'], p['alpha'], c['S'], c['R'], F32)


def test_rejects_a_missing_channel_tile_in_dA_and_sparse_dalpha():
    cid = 'tail_V20_R8_S1_N3_C48'
    p, got = _case(cid)
    for kind, name in (('dense', 'dA'), ('sparse', 'dalpha'), ('sparse', 'dA')):
        dE = p['dE'][kind].clone()
        dE[:, :, 16:32] = 0
        _tail_one(cid, p, kind, name, got[f'{kind}.{name}'])
        with pytest.raises(B.BarError):
            _tail_one(cid, p, kind, name, _tail_with(cid, p, kind, dE)[name])


def test_rejects_dq_sign_and_a_missing_tanh_derivative():
    cid = 'tail_V20_R4_S3_N1_C16'
    c = L.CASES[cid]
    p, got = _case(cid)
    S, R = c['S'], c['R']
    for kind in ('dense', 'sparse'):
        dpq = got[f'{kind}.dpq'].clone().view(S, 2, R, c['N'], c['V'])
        dpq[:, 1] = -dpq[:, 1]
        _rejects(cid, p, got, **{f'{kind}.dpq': dpq.view(S * 2 * R, c['N'], c['V'])})
        dD = p['alpha'] * torch.einsum('scr,nscuv->nsruv', p['w4'], p['dE'][kind])           # (1 - D^2) replaced by 1
        flat = torch.stack([dD.sum(-1), -dD.sum(-2)], 2).permute(1, 2, 3, 0, 4).reshape(S * 2 * R, c['N'], c['V'])
        _rejects(cid, p, got, **{f'{kind}.dpq': flat})


def test_rejects_tanh_off_by_1e_5():
    for cid in ('E_V20_R4_S3_C16_N2', 'E_V64_R32_S1_C48_N2'):
        p, got = _case(cid)
        off = (p['alpha'] * p['w4'].sum(-1) * 1e-5)[None, :, :, None, None]
        _rejects(cid, p, got, E=got['E'] + off)
    cid = 'tail_V20_R4_S3_N1_C16'                                                             # and in the sparse dW4
    p, got = _case(cid)
    dW = got['sparse.dW4'] + 1e-5 * p['alpha'] * p['dE']['sparse'].sum((0, 3, 4))[:, :, None]
    _tail_one(cid, p, 'sparse', 'dW4', got['sparse.dW4'])
    with pytest.raises(B.BarError):
        _tail_one(cid, p, 'sparse', 'dW4', dW)


def test_rejects_pad_joints_holding_a_copy_of_the_last_joint():
    cid = 'aggfwd_V25_N1_C48_T1_S1'
    p, got = _case(cid)
    E, x3 = p['E'], p['x3'].view(1, 1, 48, 1, 25)
    y = got['y'] + 7 * torch.einsum('nscu,nsct->nctu', E[..., 24], x3[..., 24])               # joints 25..31 = joint 24, in both images
    _rejects(cid, p, got, y=y)


def test_rejects_a_missing_u_chunk_in_the_tiled_dpq_sum():
    cid = 'tail_V32_R4_S3_N3_C16'
    c = L.CASES[cid]
    p, got = _case(cid)
    S, R = c['S'], c['R']
    for kind in ('dense', 'sparse'):
        dE = p['dE'][kind].clone()
        dE[:, :, :, 16:] = 0                                                                   # the second chunk of 16 rows
        part = _tail_with(cid, p, kind, dE)['dpq'].view(S, 2, R, c['N'], c['V'])
        dpq = got[f'{kind}.dpq'].clone().view(S, 2, R, c['N'], c['V'])
        dpq[:, 1] = part[:, 1]                                                                 # dq without that chunk's rows
        _rejects(cid, p, got, **{f'{kind}.dpq': dpq.view(S * 2 * R, c['N'], c['V'])})


def test_rejects_nan_and_the_allowance_leaves_old_callers_alone():
    cid = 'E_V20_R4_S3_C16_N2'
    p, got = _case(cid)
    bad = got['E'].clone()
    bad[1, 2, 3, 4, 5] = float('nan')
    _rejects(cid, p, got, E=bad)
    ref = torch.ones(4, dtype=torch.float64)
    B.check('allow', ref + 1e-3, ref, ref, 4, allow=1e-3)
    B.check('allow', ref + 1e-3, ref, ref, 4, allow=torch.full((4,), 1e-3, dtype=torch.float64))
    with pytest.raises(B.BarError):
        B.check('no allowance', ref + 1e-3, ref, ref, 4)
