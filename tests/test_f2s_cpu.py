"""CPU: the host side of the ST-GCN small-batch eval family (csrc/f2s.hip, tam_gcn_amd/f2s.py) -- what it serves and refuses,
decided before any HIP call, and the parameter-state key that drives the re-fold."""
import ctypes as C

import pytest
import torch

from params import fill_state_                                                      # noqa: E402
from tam_gcn_amd import _lib, f2, f2s
from tam_gcn_amd.models import stgcn as M

UCLA = dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
CPU = torch.device('cpu')


def test_supported_over_the_range_and_just_outside_it():
    s = _lib.load().tamgcn_f2s_supported
    for V in (2, 3, 17, 20, 25, 32):
        for K in (1, 2, 3):
            for cin, cout in ((1, 16), (2, 64), (3, 64), (64, 128), (255, 256), (256, 256)):
                for stride in (1, 2):
                    assert s(V, K, cin, cout, 9, stride) == 1, (V, K, cin, cout, stride)
    ok = (20, 3, 64, 64, 9, 1)
    assert s(*ok) == 1
    for i, bad in ((0, 1), (0, 33), (0, 0), (1, 0), (1, 4), (2, 0), (2, 257), (3, 0), (3, 24), (3, 8), (3, 272), (4, 1), (4, 3), (4, 5),
                   (4, 11), (5, 0), (5, 3)):
        g = list(ok)
        g[i] = bad
        assert s(*g) == 0, g


def _descs():
    one = (C.c_float * 4)()
    p = C.addressof(one)
    g = dict(N=1, Cin=16, Cout=16, T=4, V=20, K=3, x=p, Ae=p, wg=p, bg=p, h=p)
    t = dict(N=1, Cin=16, Cout=16, T=4, V=20, KT=9, stride=1, res_mode=0, h=p, wt=p, bt=p, x=None, wr=None, br=None, out=p)
    return one, g, t


@pytest.mark.parametrize('change', [dict(x=None), dict(h=None), dict(Cout=24), dict(V=33), dict(K=4), dict(N=0), dict(Cin=257)],
                         ids=['null_x', 'null_h', 'cout24', 'v33', 'k4', 'n0', 'cin257'])
def test_gcn_entry_point_refuses_before_any_hip_call(change):
    lib = _lib.load()
    one, g, _ = _descs()
    d = _lib.F2sGcnDesc(**dict(g, **change))
    assert lib.tamgcn_f2s_gcn(C.byref(d), None) != 0
    assert b'tamgcn_f2s_gcn' in lib.tamgcn_last_error(), lib.tamgcn_last_error()
    assert lib.tamgcn_f2s_gcn(None, None) != 0 and b'tamgcn_f2s_gcn' in lib.tamgcn_last_error()


@pytest.mark.parametrize('change', [dict(h=None), dict(out=None), dict(wt=None), dict(Cout=24), dict(V=33), dict(KT=5), dict(stride=3),
                                    dict(res_mode=1), dict(res_mode=2), dict(res_mode=3), dict(N=0)],
                         ids=['null_h', 'null_out', 'null_wt', 'cout24', 'v33', 'kt5', 'stride3', 'identity_without_x', 'conv_without_wr',
                              'res_mode3', 'n0'])
def test_tcn_entry_point_refuses_before_any_hip_call(change):
    lib = _lib.load()
    one, _, t = _descs()
    d = _lib.F2sTcnDesc(**dict(t, **change))
    assert lib.tamgcn_f2s_tcn(C.byref(d), None) != 0
    assert b'tamgcn_f2s_tcn' in lib.tamgcn_last_error(), lib.tamgcn_last_error()
    assert lib.tamgcn_f2s_tcn(None, None) != 0 and b'tamgcn_f2s_tcn' in lib.tamgcn_last_error()


def test_k4_is_refused_by_the_gcn_entry_point_with_its_geometry_in_the_message():
    lib = _lib.load()
    one, g, _ = _descs()
    d = _lib.F2sGcnDesc(**dict(g, K=4))
    assert lib.tamgcn_f2s_gcn(C.byref(d), None) != 0 and b'K=4' in lib.tamgcn_last_error()


def _model(**kw):
    m = M.Model(**dict(UCLA, **kw))
    fill_state_(m.state_dict(), seed=42)
    return m.eval()


def test_engine_refuses_a_train_mode_model():
    m = _model().train()
    with pytest.raises(ValueError, match='eval'):
        f2s.FusedEvalST(m)


def test_engine_folds_on_the_cpu_and_refuses_what_the_kernels_do_not_serve():
    m = _model()
    blocks = f2s.FusedEvalST(m)._packed(CPU)
    assert len(blocks) == 10 and [b.geom for b in blocks][:5] == [[3, 9, 1, 0]] + [[3, 9, 1, 1]] * 3 + [[3, 9, 2, 2]]
    assert tuple(blocks[0].bg.shape) == (64, 20) and tuple(blocks[4].Wr.shape) == (128, 64)
    Ae = m.A * m.edge_importance[1]
    with pytest.raises(f2.Unsupported, match='temporal kernel size 5'):
        f2s._BlockST(M.st_gcn(64, 64, (5, 3)).eval(), Ae, CPU)
    with pytest.raises(f2.Unsupported, match='multiple of 16'):
        f2s._BlockST(M.st_gcn(64, 24, (9, 3)).eval(), Ae, CPU)
    with pytest.raises(f2.Unsupported, match='33 joints'):
        f2s._BlockST(M.st_gcn(64, 64, (9, 3)).eval(), torch.ones(3, 33, 33), CPU)
    with pytest.raises(f2.Unsupported, match='4 subsets'):
        f2s._BlockST(M.st_gcn(64, 64, (9, 4)).eval(), torch.ones(4, 20, 20), CPU)
    m.st_gcn_networks[2] = M.st_gcn(64, 64, (5, 3)).eval()
    with pytest.raises(f2.Unsupported):
        f2s.FusedEvalST(m)._packed(CPU)


def test_no_edge_importance_weighting_folds_the_plain_adjacency():
    m = _model(edge_importance_weighting=False)
    blocks = f2s.FusedEvalST(m)._packed(CPU)
    assert torch.equal(blocks[3].Ae, m.A)


def test_state_key_sees_every_kind_of_state_change():
    m = _model()
    eng = f2s.FusedEvalST(m)
    b0 = eng._packed(CPU)
    assert eng._packed(CPU) is b0                                # nothing changed: no re-fold
    k = eng._state_key()
    with torch.no_grad():
        m.edge_importance[4].mul_(1.25)                          # in place
    k1 = eng._state_key()
    assert k1 != k
    b1 = eng._packed(CPU)
    assert b1 is not b0 and not torch.equal(b1[4].Ae, b0[4].Ae) and torch.equal(b1[3].Ae, b0[3].Ae)
    m2 = _model()
    with torch.no_grad():
        for p in m2.parameters():
            p.mul_(0.9)
    m.load_state_dict(m2.state_dict())
    k2 = eng._state_key()
    assert k2 != k1
    with torch.no_grad():
        m.st_gcn_networks[6].tcn[3].running_var.add_(0.5)        # running statistics
    assert eng._state_key() != k2
    b3 = eng._packed(CPU)
    assert not torch.equal(b3[6].Wt, b1[6].Wt)


def test_routing_bound_and_switch():
    assert f2s.F2S_MAX_FRAMES >= 0 and f2s.enabled is f2.enabled


def test_model_forward_on_a_cpu_tensor_still_raises():
    m = _model()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            m(torch.zeros(1, 3, 8, 20, 1))
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            m.extract_feature(torch.zeros(1, 3, 8, 20, 1))
    with pytest.raises(RuntimeError, match='no CPU path'):
        torch.ops.tamgcn.st_gcn_eval(torch.zeros(1, 3, 8, 20), [torch.zeros(1)] * 7, [3, 9, 1, 0])
