"""CPU: the run-time-V CTRGC family (csrc/vgen.hip).  Its GPU ledger (tests/test_gpu_vgen_routes.py) launches every
instantiation the source dispatches to; an fp32 torch evaluation of every GPU case stays inside every bar; the bars reject what
a kernel that mishandles a run-time V would deliver; the entry points refuse what they are not built for before any HIP call;
the route table and the two shipped graphs."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ctrgc_ref as CR
import fp64_bars as B
import test_gpu_vgen_routes as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tam_gcn_amd', 'csrc')
F32 = torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# ledger completeness
# ---------------------------------------------------------------------------------------------------------------------
def source_symbols():
    """The kernel instantiation behind every literal dispatch site of csrc/vgen.hip."""
    src = open(os.path.join(CSRC, 'vgen.hip')).read()
    found = [f'{k}<{vp}, {s}>' for k, vp, s in re.findall(r'\bVG_CASE\((\w+), (\d+), (\d+),', src)]
    found += [f'vgen_de_tail_kernel<{rt}>' for rt in re.findall(r'\bVG_TAIL_CASE\((\d+)\)', src)]
    found += re.findall(r'tg_launch_lds<(vgen_\w+)>\(', src)                       # launches outside the macros, no template arguments
    return found


def test_every_dispatch_site_is_launched_by_a_ledger_case():
    found = source_symbols()
    assert len(found) == 15 and len(set(found)) == 15, sorted(found)       # 3 streaming kernels x 2 VP x 2 S, 2 tails, E
    assert {'vgen_E_kernel', 'vgen_agg_fwd_kernel<16, 1>', 'vgen_de_tail_kernel<2>'} <= set(found)
    assert set(found) == L.PINNED, set(found) ^ L.PINNED
    assert not glob_matches_ctrgc_ledger()


def glob_matches_ctrgc_ledger():
    """vgen.hip must stay outside the glob of the templated ledger (tests/test_ctrgc_ref_cpu.py: csrc/ctrgc*.hip)."""
    import fnmatch
    return fnmatch.fnmatch('vgen.hip', 'ctrgc*.hip')


def test_case_table_covers_what_the_ledger_promises():
    st = [c for c in L.CASES.values() if c['kind'] in ('aggfwd', 'aggbwd', 'deacc')]
    for kind in ('aggfwd', 'aggbwd', 'deacc'):
        k = [c for c in st if c['kind'] == kind]
        for V in L.VS:
            assert sum(c['V'] == V for c in k) >= 2, (kind, V)
        for N, Cout, T, S in L.SHAPES:
            assert sum((c['N'], c['C'], c['T'], c['S']) == (N, Cout, T, S) for c in k) >= 2, (kind, T)
        if kind != 'aggfwd':
            assert all({'plain', 'two'} <= set(c['forms']) for c in k) and sum('relu' in c['forms'] for c in k) == 1
    assert {v % 4 for v in L.VS} == {0, 1, 2, 3} and {L.vp(v) for v in L.VS} == {16, 32} and 16 in L.VS and 17 in L.VS
    e = [c for c in L.CASES.values() if c['kind'] == 'E']
    assert {c['V'] for c in e} == set(L.VS) and {c['R'] for c in e} == {4, 20, 32} and {c['S'] for c in e} == {1, 3}
    assert {c['C'] for c in e} == {16, 48} and all(c['N'] == 2 for c in e)
    t = [c for c in L.CASES.values() if c['kind'] == 'tail']
    assert {4, 8, 12, 20, 32} <= {c['R'] for c in t} and {c['N'] for c in t} == {1, 3} and {c['S'] for c in t} == {1, 3}
    assert all(c['N'] <= 3 and c['C'] <= 48 and c.get('T', 1) <= 64 for c in L.CASES.values())
    assert all(cid in L.L.CASES for cid in L.CROSS) and {L.L.CASES[cid]['V'] for cid in L.CROSS} == {25, 32}


# ---------------------------------------------------------------------------------------------------------------------
# bars are achievable: an fp32 torch evaluation of every GPU case
# ---------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _case(cid):
    if cid not in _CACHE:
        p = L.problem(cid)
        _CACHE[cid] = (p, L.evaluate(cid, p, F32))
    return _CACHE[cid]


@pytest.mark.parametrize('cid', list(L.CASES))
def test_checker_accepts_fp32_torch(cid):
    p, got = _case(cid)
    rat = L.verify(cid, p, got)
    assert rat and max(rat.values()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# bars have teeth
# ---------------------------------------------------------------------------------------------------------------------
RAGGED = 'V17_N2_C16_T33_S3'                                      # T = 33: chunks 32 + 1; T*V = 561 is odd


def _rejects(cid, p, got, **over):
    L.verify(cid, p, got)
    with pytest.raises(B.BarError):
        L.verify(cid, p, dict(got, **over))


def _ext_dy(dy):
    """dy with one more frame whose prologue'd value is c0 (x1 = x2 = 0): what a row past T holds if the constant leaks."""
    d = dict(dy)
    for k in ('x1', 'x2'):
        d[k] = torch.cat([dy[k], torch.zeros_like(dy[k][:, :, :1])], 2)
    return d


def test_rejects_pad_joints_holding_a_copy_of_the_last_joint():
    for cid, V in (('aggfwd_V17_N1_C48_T1_S1', 17), ('aggfwd_V3_N1_C48_T1_S1', 3)):
        p, got = _case(cid)
        E, x3 = p['E'], p['x3'].view(1, 1, 48, 1, V)
        npad = L.vp(V) - V                                         # the pads of both LDS images = joint V - 1
        y = got['y'] + npad * torch.einsum('nscu,nsct->nctu', E[..., V - 1], x3[..., V - 1])
        _rejects(cid, p, got, y=y)
    cid = 'deacc_V17_N1_C48_T1_S1'                                 # a pad row u = 17 stored over (u = 16, v = 0)'s neighbour: any
    p, got = _case(cid)                                            # single element of dE replaced by the last joint's
    dE = got['plain.dE'].clone()
    dE[:, :, :, 0, 16] = dE[:, :, :, 16, 16]
    _rejects(cid, p, got, **{'plain.dE': dE})


def test_rejects_a_dropped_ragged_frame():
    cid = 'aggfwd_' + RAGGED
    p, got = _case(cid)
    y = got['y'].clone()
    y[:, :, 32:] = 0
    _rejects(cid, p, got, y=y)
    _, s1, s2 = CR.agg_fwd(p['E'], p['x3'][:, :, :32], 3, F32)     # the frame written but left out of the moments
    _rejects(cid, p, got, s1=s1)
    _rejects(cid, p, got, s2=s2)
    cid = 'deacc_' + RAGGED
    p, got = _case(cid)
    dy = {k: (v[:, :, :32] if k in ('x1', 'x2') else v) for k, v in p['dy']['two'].items()}
    _rejects(cid, p, got, **{'two.dE': CR.dE(dy, p['x3'][:, :, :32], 3, F32)})
    cid = 'aggbwd_' + RAGGED
    p, got = _case(cid)
    dx3 = got['two.dx3'].clone()
    dx3[:, :, 32:] = 0
    _rejects(cid, p, got, **{'two.dx3': dx3})


def test_rejects_the_prologue_constant_leaking_into_frames_past_T():
    cid = 'deacc_' + RAGGED
    p, got = _case(cid)
    x3 = p['x3']                                                   # the frame behind a row's last one is the next row's first
    nxt = x3.flatten(0, 1).roll(-1, 0).view_as(x3)[:, :, :1]
    leak = CR.dE(_ext_dy(p['dy']['two']), torch.cat([x3, nxt], 2), 3, F32)
    _rejects(cid, p, got, **{'two.dE': leak})
    cid = 'aggbwd_' + RAGGED
    p, got = _case(cid)
    _, db3 = CR.dx3(p['E'], _ext_dy(p['dy']['two']), 3, F32)       # E^T c0 of ONE row past T summed into db3
    _rejects(cid, p, got, **{'two.db3': db3})


@pytest.mark.parametrize('V,shape', [(17, 'N2_C16_T33_S3'), (16, 'N3_C16_T31_S3'), (31, 'N2_C16_T64_S3'), (3, 'N2_C16_T7_S3')])
def test_rejects_one_contraction_step_too_few(V, shape):
    """(V + 3) / 4 steps of four joints; one fewer loses the joints from 4 ((V + 3) / 4 - 1) on."""
    keep = 4 * ((V + 3) // 4 - 1)
    assert 0 <= keep < V
    cid = f'aggfwd_V{V}_{shape}'
    p, got = _case(cid)
    y, s1, s2 = CR.agg_fwd(p['E'][..., :keep], p['x3'][..., :keep], 3, F32)
    _rejects(cid, p, got, y=y)
    cid = f'aggbwd_V{V}_{shape}'
    p, got = _case(cid)
    E = p['E'].clone()
    E[..., keep:, :] = 0                                           # the backward contracts over u
    _rejects(cid, p, got, **{'plain.dx3': CR.dx3(E, p['dy']['plain'], 3, F32)[0]})


def test_rejects_a_tail_that_loses_a_column_window():
    """V = 31, R = 32 stages dE in column windows: the columns of the last one missing from dA, dW4 and dp / dq."""
    cid = 'tail_V31_R32_S1_N3_C16'
    c = L.CASES[cid]
    p, got = _case(cid)
    dE = p['dE']['dense'].clone().flatten(3)
    dE[..., 736:] = 0
    part = CR.tail(dE.view_as(p['dE']['dense']), p['pq'], p['w4'], p['b4'], p['alpha'], c['S'], c['R'], F32)
    for n in ('dA', 'dW4', 'dpq'):
        _rejects(cid, p, got, **{f'dense.{n}': part[n]})


# ---------------------------------------------------------------------------------------------------------------------
# the ABI without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def _lib():
    from tam_gcn_amd import build, _lib
    build.build()
    lib = C.CDLL(_lib.LIB_PATH)
    lib.tamgcn_last_error.restype = C.c_char_p
    return lib, _lib


def test_support_queries():
    lib, _ = _lib()
    assert [lib.tamgcn_vgen_supported(v) for v in (2, 17, 32)] == [1, 1, 1]
    assert [lib.tamgcn_vgen_supported(v) for v in (1, 33, 0, -5, 64)] == [0, 0, 0, 0, 0]
    for V in range(2, 33):
        for R in range(4, 33, 4):
            for S in (1, 3):
                assert 0 < lib.tamgcn_vgen_lds_bytes(S, V, R) <= 160 * 1024, (S, V, R)
    assert lib.tamgcn_vgen_lds_bytes(3, 31, 32) >= 4 * (32 * 31 * 31 + 2 * 32 * 31)        # the E builder's D and p, q
    for S, V, R in ((2, 17, 8), (3, 1, 8), (3, 33, 8), (3, 17, 6), (3, 17, 36), (3, 17, 0)):
        assert lib.tamgcn_vgen_lds_bytes(S, V, R) == -1, (S, V, R)
    # the existing queries keep their answers
    assert lib.tamgcn_ctrgc_tiled_supported(17) == 0 and lib.tamgcn_ctrgc_lds_bytes(3, 40, 8) == -1
    assert lib.tamgcn_ctrgc_lds_bytes(3, 17, 8) == -1
    assert [lib.tamgcn_ctrgc_tiled_supported(v) for v in (20, 25, 32, 64)] == [2, 2, 1, 1]
    assert lib.tamgcn_version() == 401


def test_entry_points_reject_bad_arguments_without_touching_the_gpu():
    lib, _lib_mod = _lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    src = _lib_mod.Src()
    src.x1, src.ctot, src.coff = p, 16, 0

    def calls(d):
        r = C.byref(d)
        return [('tamgcn_vgen_build_e', (r, p, None)), ('tamgcn_vgen_agg_fwd', (r, p, p, p, p, None)),
                ('tamgcn_vgen_agg_bwd', (r, C.byref(src), p, p, p, None)), ('tamgcn_vgen_de_acc', (r, C.byref(src), p, p, None)),
                ('tamgcn_vgen_de_tail', (r, p, p, p, p, p, p, 1, None))]

    def desc(**kw):
        d = _lib_mod.CtrgcDesc()
        d.N, d.Cin, d.Cout, d.S, d.R, d.T, d.V = 1, 1, 16, 3, 8, 4, 17
        d.pq = d.w4 = d.b4 = d.A = d.alpha = p
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for name, args in calls(desc()):                                       # null descriptor / pointers first
        fn = getattr(lib, name)
        assert fn(*([None] * len(args))) < 0 and name.encode() in lib.tamgcn_last_error(), name
    for V in (0, 1, 33, 40):
        for name, args in calls(desc(V=V)):
            assert getattr(lib, name)(*args) < 0, (name, V)
            msg = lib.tamgcn_last_error()
            assert name.encode() in msg and f'V={V}'.encode() in msg, (name, V, msg)
    for kw, what in ((dict(S=2), b'S=2'), (dict(Cout=24), b'Cout=24'), (dict(N=0), b'N=0')):
        for name, args in calls(desc(**kw)):
            assert getattr(lib, name)(*args) < 0, (name, kw)
            msg = lib.tamgcn_last_error()
            assert name.encode() in msg and what in msg, (name, kw, msg)
    for R in (0, 6, 36):
        for name, args in calls(desc(R=R)):
            if name in ('tamgcn_vgen_build_e', 'tamgcn_vgen_de_tail'):
                assert getattr(lib, name)(*args) < 0 and name.encode() in lib.tamgcn_last_error() and f'R={R}'.encode() in lib.tamgcn_last_error()
    for name, args in calls(desc(N=1 << 20, Cout=1 << 12)):                # N * Cout = 2^32 workgroups
        if name in ('tamgcn_vgen_agg_fwd', 'tamgcn_vgen_agg_bwd', 'tamgcn_vgen_de_acc'):
            assert getattr(lib, name)(*args) < 0 and b'grid' in lib.tamgcn_last_error(), name
    d = desc()
    assert lib.tamgcn_vgen_de_tail(C.byref(d), p, p, p, p, p, p, 3, None) < 0 and b'groups=3' in lib.tamgcn_last_error()
    src.ctot = 8                                                           # dy narrower than Cout
    assert lib.tamgcn_vgen_agg_bwd(C.byref(d), C.byref(src), p, p, p, None) < 0 and b'tamgcn_vgen_agg_bwd: dy has 8 channels' in lib.tamgcn_last_error()


def test_route_table():
    from tam_gcn_amd import ops
    assert [ops.ctrgc_route(v) for v in (2, 16, 17, 18, 31)] == ['vgen'] * 5
    assert ops.ctrgc_route(20) == 'fused' and ops.ctrgc_route(25) == 'stream'
    assert ops.ctrgc_route(32) == 'tiled' and ops.ctrgc_route(64) == 'tiled'
    for v in (1, 33, 40):
        with pytest.raises(RuntimeError, match=f'got V = {v}'):
            ops.ctrgc_route(v)
    assert all(ops.ctrgc_tiled(v) for v in (2, 17, 25, 31, 32, 64)) and not ops.ctrgc_tiled(20)


# ---------------------------------------------------------------------------------------------------------------------
# the shipped graphs
# ---------------------------------------------------------------------------------------------------------------------
COCO_PARENTS = (None, 0, 0, 1, 2, 0, 0, 5, 6, 7, 8, 5, 6, 11, 12, 13, 14)
OPENPOSE_INWARD = [(4, 3), (3, 2), (7, 6), (6, 5), (13, 12), (12, 11), (10, 9), (9, 8), (11, 5), (8, 2), (5, 1), (2, 1), (0, 1), (15, 0),
                   (14, 0), (17, 15), (16, 14)]


def _is_tree(links, V):
    adj = {i: set() for i in range(V)}
    for i, j in links:
        adj[i].add(j)
        adj[j].add(i)
    seen, todo = {0}, [0]
    while todo:
        for k in adj[todo.pop()]:
            if k not in seen:
                seen.add(k)
                todo.append(k)
    return len(set(map(frozenset, links))) == V - 1 and len(seen) == V


@pytest.mark.parametrize('name,V,root,links', [('coco', 17, 0, [(k, p) for k, p in enumerate(COCO_PARENTS) if p is not None]),
                                               ('openpose', 18, 1, OPENPOSE_INWARD)])
def test_shipped_graph(name, V, root, links):
    import importlib
    mod = importlib.import_module(f'tam_gcn_amd.graph.{name}')
    g = mod.Graph()
    assert mod.num_node == g.num_node == V
    assert g.A.shape == (3, V, V) and g.A.dtype == np.float64
    assert np.array_equal(g.A[0], np.eye(V))
    for s in (1, 2):
        col = g.A[s].sum(0)
        assert np.all((np.abs(col) < 1e-12) | (np.abs(col - 1) < 1e-12)), col
    assert len(g.inward) == V - 1 and set(g.inward) == set(links) and set(g.outward) == {(j, i) for i, j in links}
    assert _is_tree(g.inward, V)
    assert [k for k in range(V) if k not in {i for i, _ in g.inward}] == [root]          # every joint but the root has a parent
    assert g.A[1][:, root].sum() == 0                                                    # nothing flows inward from the root
    assert np.array_equal(g.A, mod.Graph(labeling_mode='spatial').get_adjacency_matrix())


def test_a_users_own_graph_class_is_the_extension_point():
    """Any class whose instance has .A of shape (3, V, V) builds a model: here one defined in this file, 11 joints."""
    from tam_gcn_amd.models.ctrgcn import Model
    m = Model(num_class=5, num_point=11, num_person=1, graph='test_vgen_cpu.ChainGraph', in_channels=3)
    assert tuple(m.l1.gcn1.PA.shape) == (3, 11, 11)


class ChainGraph:
    def __init__(self, **_):
        from tam_gcn_amd.graph import tools
        V = 11
        inward = [(k, k - 1) for k in range(1, V)]
        self.A = tools.get_spatial_graph(V, [(i, i) for i in range(V)], inward, [(j, i) for i, j in inward])
