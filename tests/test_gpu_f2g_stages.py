"""-m gpu: the ledger of the small-batch eval kernels (tests/test_gpu_f2_stages.py, tests/f2_ref.py) run on the f2g family --
csrc/f2g.hip, the joint count a kernel argument -- at V in {8, 9, 16, 19, 22, 23, 28}: all six frame pitches, 1, 2, 3 and 4
live lanes in a frame's last 16-byte piece, the whole-tile case 16 and the LDS edge 28.  Every stage and every case of
tests/f2g_cases.py through test_gpu_f2_stages.ledger_case (the buffer layout is f2v's, so its harness drives the family
unchanged): NaN guards around every operand, NaN pad joints in every padded input, exact-zero pad joints of E / sum / diff /
xpart, the weights-one-float-off run, the kernel symbol, the derived fp64 rounding bars, no element excluded.  Then two more
runs of the same problem: bit-equal.

Then the refusals: every f2g entry point refuses V = 7 and 29 on the host -- the launch counter (the last kernel symbol)
unchanged, no byte written.

Then f2g against f2v at 17, 18 and 25 joints, stage by stage on the same operands: every output buffer has f2v's bits."""
import pytest
import torch

import f2_ref as R
import f2g_cases as T
import test_gpu_f2_stages as L

pytestmark = pytest.mark.gpu

from tam_gcn_amd import _lib                                                       # noqa: E402

FAM = 'f2g'


def _params(stage):
    return [(cid, V) for cid in T.STAGES[stage] for V in T.JOINTS]


def _case(monkeypatch, stage, cid, V):
    monkeypatch.setitem(R.FAMILIES, FAM, V)
    monkeypatch.setitem(R.STAGES, stage, T.STAGES[stage])
    assert T.STAGES[stage][cid]['G'] == 1
    L.ledger_case(stage, cid, FAM)
    q = R.sub(stage, R.problem(stage, T.STAGES[stage][cid], V, L._seed(cid)), 0)
    a, b = L.run(stage, FAM, q), L.run(stage, FAM, q)
    for k in a:
        assert torch.equal(L._bits(a[k]), L._bits(b[k])), f'{cid} V = {V}: {k}: two runs differ'


@pytest.mark.parametrize('cid, V', _params('e'))
def test_e(cid, V, monkeypatch):
    _case(monkeypatch, 'e', cid, V)


@pytest.mark.parametrize('cid, V', _params('gcn'))
def test_gcn(cid, V, monkeypatch):
    _case(monkeypatch, 'gcn', cid, V)


@pytest.mark.parametrize('cid, V', _params('gemm'))
def test_gemm(cid, V, monkeypatch):
    _case(monkeypatch, 'gemm', cid, V)


@pytest.mark.parametrize('cid, V', _params('tcn'))
def test_tcn(cid, V, monkeypatch):
    _case(monkeypatch, 'tcn', cid, V)


# ---------------------------------------------------------------------------------------------------------------------
# joint counts outside the range: refused on the host before any launch.  The operands are real buffers sized for the joint
# count the descriptor names, so an entry point that accepted one would run on memory it may touch.
# ---------------------------------------------------------------------------------------------------------------------
_BASE = {'e': dict(R.GCN_CASES['cin16_res2_t9'], G=1, N=2), 'gcn': dict(R.GCN_CASES['cin16_res2_t9'], G=1, N=2),
         'gemm': dict(R.GEMM_CASES['k48_m48_mode0_t9'], G=1, N=2), 'tcn': dict(R.TCN_CASES['nb2_cb16_k5_s2_res2_cin3_t8'], G=1, N=2)}


@pytest.mark.parametrize('V', [7, 29])
@pytest.mark.parametrize('stage', list(_BASE))
def test_joint_counts_outside_the_range_are_refused(stage, V, monkeypatch):
    lib = _lib.load()
    # a launch of ANOTHER stage at a served joint count first: its symbol must still be the last one after the refusal
    other = 'gemm' if stage != 'gemm' else 'tcn'
    oc = next(iter(T.STAGES[other]))
    monkeypatch.setitem(R.FAMILIES, FAM, 9)
    L.run(other, FAM, R.sub(other, R.problem(other, T.STAGES[other][oc], 9, 1), 0))
    before = lib.tamgcn_last_kernel()
    assert before == f'f2g_{other}_kernel'.encode()
    monkeypatch.setitem(R.FAMILIES, FAM, V)
    p = R.sub(stage, R.problem(stage, _BASE[stage], V, 2), 0)
    bufs, d, _ = L.prepare(stage, FAM, p)
    assert d.V == V
    rc = R.launch(lib, FAM, stage, d, None, torch.cuda.current_stream().cuda_stream)
    msg = lib.tamgcn_last_error()
    assert rc != 0, f'f2g_{stage} V = {V}: accepted'
    assert f'tamgcn_f2g_{stage}: V={V} '.encode() in msg and b'8 <= V <= 28' in msg, msg
    assert lib.tamgcn_last_kernel() == before, lib.tamgcn_last_kernel()
    torch.cuda.synchronize()
    for name, whole, was, keep in bufs.items:                      # nothing was written anywhere, outputs included
        assert torch.equal(L._bits(whole), was), name


# ---------------------------------------------------------------------------------------------------------------------
# f2g against f2v at the joint counts both serve (17, 18, 25): the two families are one body under two geometry policies
# (csrc/f2x_body.h), so on the same operands every buffer the next stage reads -- E, sum, diff, g / h (the gemm outputs of
# mode 0 / 1), out, xpart -- comes out with the same bits, pad columns included (the NaN pad joints of the padded inputs give
# the same NaN bits in gemm's pad columns: the comparison is of the words).  The smallest rows of tests/f2_ref.py's tables that
# reach the vector and the scalar weight-row path and a K tail; an `off` row also one float off the 16-byte boundary; gcn
# also at Cin = 200, which crosses the K chunk.
# ---------------------------------------------------------------------------------------------------------------------
_SAME = {'e': ('cin3_r1_t1', 'cin40_r12_t4', 'cin16_r4_t3'),
         'gcn': ('cin3_res2_t1', 'cin40_res0_t4', 'cin16_res1_t3', 'cin200_res2_t3'),
         'gemm': ('k40_m16_relu16_t1', 'k16_m48_relu32_t4', 'k48_m48_mode0_t9'),
         'tcn': ('nb2_cb16_k5_s2_res2_cin3_t8', 'nb1_cb16_k9_s2_res2_cin40_t3', 'nb1_cb32_k9_s2_res2_cin64_t2', 'nb2_cb16_k3_s1_res1_t5')}
_OUTS = {'e': ('E',), 'gcn': ('sum', 'diff'), 'gemm': ('out',), 'tcn': ('out', 'xpart')}


def _words(stage, fam, p, off):
    """one launch -> {output buffer: its words, the whole allocation the next stage reads}"""
    lib = _lib.load()
    bufs, d, t = L.prepare(stage, fam, p, off)
    rc = R.launch(lib, fam, stage, d, None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (fam, stage, lib.tamgcn_last_error())
    assert lib.tamgcn_last_kernel() == f'{fam}_{stage}_kernel'.encode(), lib.tamgcn_last_kernel()
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:                                    # a device fault: nothing more is launched in this session
        pytest.exit(f'{fam}_{stage}: {err}', returncode=3)
    bufs.check(f'{fam}_{stage}')
    return {k: L._bits(t[k]) for k in _OUTS[stage] if t.get(k) is not None}


@pytest.mark.parametrize('V', [17, 18, 25])
@pytest.mark.parametrize('stage, cid', [(s, c) for s, cs in _SAME.items() for c in cs])
def test_stage_outputs_have_the_bits_of_f2v(stage, cid, V, monkeypatch):
    monkeypatch.setitem(R.FAMILIES, FAM, V)
    monkeypatch.setitem(R.FAMILIES, 'f2v', V)
    c = R.STAGES[stage][cid]
    q = R.sub(stage, R.problem(stage, c, V, L._seed(cid)), 0)
    assert max(t.numel() for t in q.values() if torch.is_tensor(t)) <= 256 * 33 * 28
    for off in ((False, True) if c['off'] else (False,)):
        g, v = _words(stage, FAM, q, off), _words(stage, 'f2v', q, off)
        assert set(g) == set(v) and g, (stage, cid)
        for k in g:
            assert g[k].shape == v[k].shape and torch.equal(g[k], v[k]), f'{stage} {cid} V = {V} off = {off}: {k} differs from f2v'
