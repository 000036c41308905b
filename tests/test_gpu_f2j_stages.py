"""-m gpu: the ledger of the small-batch eval kernels (tests/test_gpu_f2_stages.py, tests/f2_ref.py) run on the f2v family at
17 and 18 joints -- the instantiations csrc/f2v.hip adds for graph.coco and graph.openpose.  Every stage and every case of
the table, through test_gpu_f2_stages.ledger_case with the family's joint count switched (the kernel symbols it pins are free
of V): NaN guards around every operand, NaN pad joints (columns V..19) in every padded input, exact-zero pad joints of E / sum
/ diff / xpart, the weights-one-float-off run, grouped equal to plain bit for bit, the derived fp64 rounding bars, no element
excluded.  V = 18 is the joint count with TWO live lanes in a frame's last 16-byte piece; the block input's rows have a pitch
of T*17 or T*18 floats.

Then the refusals: every f2v entry point refuses V = 19, 16 and 20 on the host -- the launch counter (the last kernel symbol)
unchanged, no byte written."""
import pytest
import torch

import f2_ref as R
import test_gpu_f2_stages as L

pytestmark = pytest.mark.gpu

from tam_gcn_amd import _lib                                                       # noqa: E402

JOINTS = (17, 18)


def _params(stage):
    return [(cid, V) for cid in R.STAGES[stage] for V in JOINTS]


def _case(monkeypatch, stage, cid, V):
    monkeypatch.setitem(R.FAMILIES, 'f2v', V)
    assert R.vp(V) == 20
    L.ledger_case(stage, cid, 'f2v')


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
# joint counts outside the list: refused on the host before any launch.  The operands are real buffers sized for the joint
# count the descriptor names, so an entry point that accepted one would run on memory it may touch.
# ---------------------------------------------------------------------------------------------------------------------
_BASE = {'e': dict(R.GCN_CASES['cin16_res2_t9'], G=1, N=2), 'gcn': dict(R.GCN_CASES['cin16_res2_t9'], G=1, N=2),
         'gemm': dict(R.GEMM_CASES['k48_m48_mode0_t9'], G=1, N=2), 'tcn': dict(R.TCN_CASES['nb2_cb16_k5_s2_res2_cin3_t8'], G=1, N=2)}


@pytest.mark.parametrize('grouped', [False, True], ids=['plain', 'grouped'])
@pytest.mark.parametrize('V', [19, 16, 20])
@pytest.mark.parametrize('stage', list(_BASE))
def test_other_joint_counts_are_refused(stage, V, grouped, monkeypatch):
    lib = _lib.load()
    # a launch of ANOTHER stage at a served joint count first: its symbol must still be the last one after the refusal
    other = 'gemm' if stage != 'gemm' else 'tcn'
    oc = next(iter(R.STAGES[other]))
    monkeypatch.setitem(R.FAMILIES, 'f2v', 17)
    L.run(other, 'f2v', R.sub(other, R.problem(other, R.STAGES[other][oc], 17, 1), 0))
    before = lib.tamgcn_last_kernel()
    monkeypatch.setitem(R.FAMILIES, 'f2v', V)
    groups = 2 if grouped else None
    c = _BASE[stage]
    p = R.problem(stage, dict(c, G=2), V, 2) if grouped else R.sub(stage, R.problem(stage, c, V, 2), 0)
    bufs, d, _ = L.prepare(stage, 'f2v', p)
    assert d.V == V
    rc = R.launch(lib, 'f2v', stage, d, groups, torch.cuda.current_stream().cuda_stream)
    msg = lib.tamgcn_last_error()
    assert rc != 0, f'f2v_{stage} V = {V}: accepted'
    assert f'V={V}'.encode() in msg and b'V = 17, V = 18, V = 25' in msg, msg
    assert lib.tamgcn_last_kernel() == before, lib.tamgcn_last_kernel()
    torch.cuda.synchronize()
    for name, whole, was, keep in bufs.items:                      # nothing was written anywhere, outputs included
        assert torch.equal(L._bits(whole), was), name
