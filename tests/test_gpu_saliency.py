"""-m gpu: gradient saliency (tam_gcn_amd/saliency.py) on the f2s family's forward + backward chain (csrc/f2s_bwd.hip) through whole
ST-GCN models.

  * teacher-forced: per block, the fp64 restatement (tests/f2s_bwd_ref.py) applied to the GPU's OWN gout, out and h must reproduce the
    GPU's dx within the stage bars -- the masks are identical by construction, so a ReLU flip cannot excuse a miss.  The trace
    holds no dh, so the two stages are held together: the gcn_bwd bar on the fp64 dh, plus the tcn_bwd bar on dh carried through
    gcn_bwd's magnitudes (a linear map: an error of dh within its bar moves dx by at most that much).
  * end to end, against the fp64 oracle (autograd, eval mode), the fp64 fixture written from the reference's model and the
    general path: relative L2 <= 5e-2 and cosine >= 0.999 -- the flip-robust bars of tests/test_gpu_model.py (a ReLU whose
    pre-activation is ~0 may flip in fp32 and moves single entries; the reference's own fp32 run against its fp64 run gives
    5.2e-7 / 3.9e-4 relative L2 on the two fixture cases).
  * seeding, state, launch structure, graph capture, the registered operator, PartImportance.
`pytest -s` prints the figures."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import f2s_bwd_ref as RB                                                            # noqa: E402
import fp64_bars as B                                                               # noqa: E402
from cases import STGCN_MODEL_CASES                                                 # noqa: E402
from params import make_input, make_labels                                          # noqa: E402
from tam_gcn_amd import f2, f2s, saliency                                           # noqa: E402
from tam_gcn_amd.models import stgcn as M                                           # noqa: E402
from tam_gcn_amd.models import ctrgcn as CM                                         # noqa: E402
from test_stgcn_oracle import fill_stgcn_                                           # noqa: E402
from test_gpu_f2j import _counted, _general                                         # noqa: E402
from test_gpu_f2s import MODELS, _model, _sd64, _oracle, _bits                      # noqa: E402

DEV = 'cuda:0'
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'saliency.npz'))
BOUND = 1024                   # the routing tests set the bound themselves: they test the routing, not the measured value
FAMILY = ('tamgcn_f2s_tcn_bwd', 'tamgcn_f2s_gcn_bwd')


@pytest.fixture(autouse=True)
def _bound(monkeypatch):
    monkeypatch.setattr(f2s, 'F2S_BWD_MAX_FRAMES', BOUND)
    monkeypatch.setattr(f2s, 'F2S_MAX_FRAMES', BOUND)
    monkeypatch.setenv('TAMGCN_F2', '1')


def _fixture_model(margs):
    m = M.Model(**margs)
    fill_stgcn_(m.state_dict(), seed=77)
    return m.to(DEV).eval()


def _oracle_grad(m, x, labels, V):
    """fp64 autograd through the oracle in eval mode: d sum_n logits[n, labels[n]] / dx, and the logits"""
    xd = x.double().requires_grad_(True)
    logits = _oracle(xd, _sd64(m), V)[0]
    (g,) = torch.autograd.grad(torch.gather(logits, 1, labels.view(-1, 1)).sum(), xd)
    return g, logits.detach()


def _bars(name, got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.double().reshape(-1)
    rel = float((got - ref).norm() / ref.norm())
    cos = float((got * ref).sum() / (got.norm() * ref.norm()))
    print(f'\n{name}: relative L2 {rel:.3e}, cosine {cos:.9f}')
    assert rel <= 5e-2 and cos >= 0.999, (name, rel, cos)


def _sal_of(g5):
    return g5.abs().sum((1, 2, 4))


def _spy(monkeypatch):
    calls = []
    real = f2s.FusedEvalST.saliency_pass
    monkeypatch.setattr(f2s.FusedEvalST, 'saliency_pass', lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    return calls


# ---------------------------------------------------------------------------------------------------------------------
# every block of a family run, teacher-forced on the GPU's own tensors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', STGCN_MODEL_CASES, ids=[c[0] for c in STGCN_MODEL_CASES])
def test_every_block_teacher_forced(case):
    tag, margs, shape = case
    m = _fixture_model(margs)
    x = make_input(shape, seed=21).to(DEV)
    lab = make_labels(shape[0], margs['num_class'], seed=22).to(DEV)
    trace = []
    g = saliency.input_gradient(m, x, lab, trace=trace)
    assert g.shape == x.shape and len(trace) == 10
    blocks = m.__dict__['_tamgcn_f2s']._blocks
    for i, (b, s) in enumerate(zip(blocks, trace)):
        gout, out, h, dx = (s[k].cpu() for k in ('gout', 'out', 'h', 'dx'))
        if i < 9:
            assert trace[i + 1]['dx'] is s['gout']                                    # block i's gout IS block i + 1's dx
        Wt, Wg, Ae = b.Wt.cpu().view(b.Cout, b.Cout, 9), b.Wg.cpu(), b.Ae.cpu()
        Wr = None if b.Wr is None else b.Wr.cpu()
        c = dict(Cout=b.Cout, V=b.V, rmode=b.rmode)
        dh = RB.tcn_bwd(gout, out, h, Wt, b.stride)
        dh_mag = RB.tcn_bwd(gout, out, h, Wt, b.stride, absval=True)
        ref = RB.gcn_bwd(dh, Ae, Wg, b.rmode, b.stride, gout, out, Wr)
        mag = RB.gcn_bwd(dh, Ae, Wg, b.rmode, b.stride, gout, out, Wr, absval=True)
        carried = RB.gcn_bwd(B.elementwise_bar(RB.bar_L('tcn_bwd', c), dh_mag), Ae, Wg, 0, b.stride, absval=True)
        err = B.check(f'{tag} block {i}', dx, ref, mag, RB.bar_L('gcn_bwd', c), allow=carried)
        assert 0.02 < float((out > 0).float().mean()) < 0.98 and 0.02 < float((h > 0).float().mean()) < 0.98
        print(f'\n{tag} block {i} ({b.Cin} -> {b.Cout}, stride {b.stride}, res {b.rmode}): max|err| {err:.3e} (max|ref| {float(ref.abs().max()):.3e})')
    # the stem's end: dxin = c1 * dx0, summed per joint
    coef = m.data_bn.__dict__['_tamgcn_eval_cache']['stem'][1][0].cpu()
    sal_ref, dxin_ref = RB.saliency_joints(trace[0]['dx'].cpu(), coef[0], shape[4])
    sal_mag, dxin_mag = RB.saliency_joints(trace[0]['dx'].cpu(), coef[0], shape[4], absval=True)
    B.check(f'{tag} dxin', g, dxin_ref, dxin_mag, 1)
    B.check(f'{tag} sal', saliency.joint_saliency(m, x, lab), sal_ref, sal_mag, shape[1] * shape[2] * shape[4])


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', STGCN_MODEL_CASES, ids=[c[0] for c in STGCN_MODEL_CASES])
def test_against_the_oracle_the_fixture_and_the_general_path(case, monkeypatch):
    tag, margs, shape = case
    m = _fixture_model(margs)
    x = make_input(shape, seed=21)
    lab = make_labels(shape[0], margs['num_class'], seed=22)
    ref, _ = _oracle_grad(m, x, lab, margs['num_point'])
    fix, fix_sal = torch.from_numpy(GOLD[f'{tag}/dx64']), torch.from_numpy(GOLD[f'{tag}/saliency'])
    calls = _spy(monkeypatch)
    xd, ld = x.to(DEV), lab.to(DEV)
    g = saliency.input_gradient(m, xd, ld)
    s = saliency.joint_saliency(m, xd, ld)
    assert len(calls) == 2 and g.shape == xd.shape and s.shape == (shape[0], shape[3])
    with _general():
        gg = saliency.input_gradient(m, xd, ld)
        sg = saliency.joint_saliency(m, xd, ld)
    assert len(calls) == 2, 'TAMGCN_F2=0 is the general path'
    for name, got, want in (('family / oracle', g, ref), ('family / fixture', g, fix), ('general / oracle', gg, ref), ('family / general', g, gg.cpu()),
                            ('saliency family / oracle', s, _sal_of(ref)), ('saliency family / fixture', s, fix_sal),
                            ('saliency general / oracle', sg, _sal_of(ref)), ('saliency family / general', s, sg.cpu())):
        _bars(f'{tag} {name}', got, want)


GEOMETRIES = [('coco', (2, 3, 13, 17, 1)), ('openpose', (1, 3, 20, 18, 2)), ('ntu', (1, 3, 20, 25, 2)), ('ucla', (2, 13, 60))]


@pytest.mark.parametrize('name, shape', GEOMETRIES, ids=[f'{n}_{"x".join(map(str, s))}' for n, s in GEOMETRIES])
def test_other_geometries_against_the_oracle(name, shape, monkeypatch):
    m = _model(name)
    V = MODELS[name]['num_point']
    x = make_input(shape, seed=21)
    lab = make_labels(shape[0], MODELS[name]['num_class'], seed=22)
    ref, _ = _oracle_grad(m, x, lab, V)
    calls = _spy(monkeypatch)
    g = saliency.input_gradient(m, x.to(DEV), lab.to(DEV))
    s = saliency.joint_saliency(m, x.to(DEV), lab.to(DEV))
    assert len(calls) == 2 and g.shape == x.shape and s.shape == (shape[0], V)
    _bars(f'{name} {shape} gradient', g, ref)
    ref5 = ref if ref.dim() == 5 else ref.view(shape[0], shape[1], V, -1).permute(0, 3, 1, 2).unsqueeze(-1)
    _bars(f'{name} {shape} saliency', s, _sal_of(ref5))


def test_seeding():
    m = _model('ucla')
    x = make_input((3, 3, 16, 20, 1), seed=4).to(DEV)
    lab = torch.tensor([7, 0, 3], device=DEV)
    g = saliency.input_gradient(m, x, lab)
    one_hot = torch.nn.functional.one_hot(lab, 10).float()
    assert torch.equal(_bits(saliency.input_gradient(m, x, dlogits=one_hot)), _bits(g))
    with torch.no_grad():
        top = m(x).argmax(1)
    assert torch.equal(_bits(saliency.input_gradient(m, x)), _bits(saliency.input_gradient(m, x, top)))
    assert torch.equal(_bits(saliency.joint_saliency(m, x)), _bits(saliency.joint_saliency(m, x, top)))
    # a linear functional of the logits: the gradient is linear in the seed
    w = make_input((3, 10), seed=9).to(DEV)
    gw = saliency.input_gradient(m, x, dlogits=w)
    with _general():
        _bars('dlogits family / general', gw, saliency.input_gradient(m, x, dlogits=w).cpu())
    with pytest.raises(ValueError, match='not both'):
        saliency.input_gradient(m, x, lab, dlogits=w)
    with pytest.raises(ValueError, match='dlogits must be'):
        saliency.input_gradient(m, x, dlogits=w[:, :4])


def test_state_is_left_alone_and_followed():
    m = _model('coco')
    x = make_input((2, 3, 20, 17, 1), seed=21)
    lab = make_labels(2, 10, seed=22)
    xd, ld = x.to(DEV), lab.to(DEV)
    with torch.no_grad():
        before = m(xd)
    g0 = saliency.input_gradient(m, xd, ld)
    with _general():
        saliency.input_gradient(m, xd, ld)
        saliency.joint_saliency(m, xd, ld)
    saliency.joint_saliency(m, xd, ld)
    assert all(p.grad is None for p in m.parameters()) and xd.grad is None and not xd.requires_grad
    with torch.no_grad():
        assert torch.equal(_bits(m(xd)), _bits(before))
    _bars('coco', g0, _oracle_grad(m, x, lab, 17)[0])
    with torch.no_grad():
        m.edge_importance[3].mul_(1.3)                       # in place
        m.st_gcn_networks[6].tcn[2].bias.add_(0.3)
    g1 = saliency.input_gradient(m, xd, ld)
    assert float((g1 - g0).abs().max()) > 1e-3 * float(g0.abs().max())
    _bars('coco after an in-place change', g1, _oracle_grad(m, x, lab, 17)[0])
    m2 = _model('coco')
    with torch.no_grad():
        for p in m2.parameters():
            p.mul_(0.9)
    m.load_state_dict(m2.state_dict())
    g2 = saliency.input_gradient(m, xd, ld)
    assert float((g2 - g1).abs().max()) > 1e-3 * float(g1.abs().max())
    _bars('coco after load_state_dict', g2, _oracle_grad(m, x, lab, 17)[0])


def test_launch_structure_and_routing():
    m = _model('openpose')
    V, P = 18, 2
    x = make_input((1, 3, 20, V, P), seed=9).to(DEV)
    lab = torch.tensor([5], device=DEV)
    saliency.joint_saliency(m, x, lab)                                              # fold, coefficient cache
    _, cnt = _counted(lambda: saliency.joint_saliency(m, x, lab))
    last_fwd = max(i for i, n in enumerate(cnt.names) if n == 'tamgcn_f2s_tcn')
    assert [n for n in cnt.names[:last_fwd + 1] if n.startswith('tamgcn_f2s_')] == ['tamgcn_f2s_gcn', 'tamgcn_f2s_tcn'] * 10
    back = cnt.names[last_fwd + 1:]
    fam = [n for n in back if n.startswith('tamgcn_f2s_')]
    assert fam == list(FAMILY) * 10, fam
    assert len(back) - len(fam) <= 8, back
    assert back[-1] == 'tamgcn_saliency_joints'
    trace = []
    saliency.input_gradient(m, x, lab, trace=trace)
    assert [tuple(s['dx'].shape[1:3]) for s in trace] == [(3, 20)] + [(64, 20)] * 4 + [(128, 10)] * 3 + [(256, 5)] * 2   # reverse block order fills it
    big = make_input((BOUND // (P * 8) + 1, 3, 8, V, P), seed=3).to(DEV)           # one clip over the bound: the general path
    _, cnt = _counted(lambda: saliency.joint_saliency(m, big, None))
    assert not any(n in FAMILY for n in cnt.names)
    _, cnt = _counted(lambda: saliency.joint_saliency(m, big[:-1], None))
    assert sum(n in FAMILY for n in cnt.names) == 20
    h = m.st_gcn_networks[3].register_forward_hook(lambda mod, i, o: None)          # a hook would not fire inside the engine
    _, cnt = _counted(lambda: saliency.joint_saliency(m, x, lab))
    h.remove()
    assert not any(n in FAMILY for n in cnt.names)
    c = CM.Model(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial')).to(DEV).eval()
    xc = make_input((1, 3, 16, 20, 1), seed=2).to(DEV)
    (sc, cnt) = _counted(lambda: saliency.joint_saliency(c, xc, None))
    assert not any(n in FAMILY for n in cnt.names) and sc.shape == (1, 20) and bool(torch.isfinite(sc).all())
    assert all(p.grad is None for p in c.parameters())
    trace = []
    saliency.input_gradient(c, xc, trace=trace)
    assert trace == []


def test_captured_in_a_graph_on_one_stream():
    m = _model('ucla')
    xs = make_input((2, 3, 24, 20, 1), seed=4).to(DEV)
    ys = torch.tensor([1, 8], device=DEV)
    x2 = make_input((2, 3, 24, 20, 1), seed=5).to(DEV)
    y2 = torch.tensor([3, 3], device=DEV)
    eager = [saliency.joint_saliency(m, a, b).clone() for a, b in ((xs, ys), (x2, y2))]
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        saliency.joint_saliency(m, xs, ys)
    torch.cuda.current_stream().wait_stream(st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        out = saliency.joint_saliency(m, xs, ys)
    for _ in range(2):
        graph.replay()
        assert torch.equal(_bits(out), _bits(eager[0]))
    xs.copy_(x2)
    ys.copy_(y2)
    graph.replay()
    assert torch.equal(_bits(out), _bits(eager[1]))


def test_block_gradient_is_a_registered_operator():
    m = _model('ucla')
    eng = f2s.FusedEvalST(m)
    blocks = eng._packed(torch.device(DEV))
    for i, cin in ((0, 3), (2, 64), (4, 64), (8, 256)):
        b = blocks[i]
        x = make_input((2, cin, 11, 20), seed=3 + i).to(DEV)
        out, h = torch.ops.tamgcn.st_gcn_eval_fwd(x, b.params, b.geom)
        assert torch.equal(out, torch.ops.tamgcn.st_gcn_eval(x, b.params, b.geom)) and h.shape == (2, b.Cout, 11, 20)
        gout = make_input(tuple(out.shape), seed=11).to(DEV)
        dx = torch.ops.tamgcn.st_gcn_eval_bwd(gout, out, h, b.bparams, b.geom)
        assert dx.shape == x.shape
        torch.library.opcheck(torch.ops.tamgcn.st_gcn_eval_bwd.default, (gout, out, h, b.bparams, b.geom), test_utils=('test_schema', 'test_faketensor'))
        torch.library.opcheck(torch.ops.tamgcn.st_gcn_eval_fwd.default, (x, b.params, b.geom), test_utils=('test_schema', 'test_faketensor'))
    b = blocks[0]
    z = torch.zeros(1, 64, 8, 20)
    with pytest.raises(RuntimeError, match='no CPU path'):
        torch.ops.tamgcn.st_gcn_eval_bwd(z, z, z, b.bparams, b.geom)
    with pytest.raises(RuntimeError, match='outside the f2s kernels'):
        torch.ops.tamgcn.st_gcn_eval_bwd(z.to(DEV), z.to(DEV), z.to(DEV), b.bparams, [3, 5, 1, 0])
    kt5 = _model('ucla')
    kt5.st_gcn_networks[2] = M.st_gcn(64, 64, (5, 3), 1).to(DEV).eval()             # outside the family: the general path, no error
    xk = make_input((1, 3, 12, 20, 1), seed=2).to(DEV)
    s, cnt = _counted(lambda: saliency.joint_saliency(kt5, xk))
    assert kt5.__dict__.get('_tamgcn_f2s') is False and not any(n in FAMILY for n in cnt.names) and s.shape == (1, 20)
    with pytest.raises(f2.Unsupported):
        f2s.FusedEvalST(kt5)._packed(torch.device(DEV))


def test_part_importance(tmp_path):
    m = _model('ucla')
    imp = saliency.PartImportance(m, 10, per_class=2)
    labels = ([0, 0, 0, 1], [1, 1, 2, 0], [2, 2, 2, 3])                              # classes 0, 1, 2 reach the cap in mid-batch
    count, total = [0] * 10, [[0.0] * 5 for _ in range(10)]
    parts = list(RB.UCLA_PARTS.values())
    for i, lab in enumerate(labels):
        x = make_input((4, 3, 16, 20, 1), seed=30 + i).to(DEV)
        ld = torch.tensor(lab, device=DEV)
        imp.update(x, ld)
        RB.part_accumulate(count, total, saliency.joint_saliency(m, x, ld).double().cpu().tolist(), lab, parts, 2)
    got = imp.compute()
    want = RB.part_importance(count, total)
    assert imp.count.cpu().tolist() == count == [2, 2, 2, 1] + [0] * 6
    assert list(got) == list(range(10)) and list(got[0]) == list(RB.UCLA_PARTS)
    for k in range(10):
        for p, name in enumerate(RB.UCLA_PARTS):
            assert abs(got[k][name] - want[k][p]) <= 1e-12 * max(1.0, abs(want[k][p])), (k, name)
        assert max(got[k].values()) == (1.0 if count[k] else 0.0)
    path = tmp_path / 'group_weights.json'
    assert imp.to_json(str(path)) == got
    back = json.load(open(path))
    assert {int(k): v for k, v in back.items()} == got
    imp.reset()
    assert imp.compute() == {k: {n: 0.0 for n in RB.UCLA_PARTS} for k in range(10)}
