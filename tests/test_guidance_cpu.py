"""tam_gcn_amd.guidance without a GPU: argument checks, the refusals, and the registered operators' fake implementations."""
import pytest
import torch

from tam_gcn_amd import guidance, torch_ops              # noqa: F401
from tam_gcn_amd.models import ctrgcn as M, stgcn

UCLA = dict(num_class=10, num_point=20, num_person=1, graph='tam_gcn_amd.graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))


def test_refusals():
    m = M.Model(**UCLA).eval()
    x = torch.zeros(1, 3, 16, 20, 1)
    with pytest.raises(RuntimeError, match='no CPU'):
        guidance.pooled_feature(m, x)
    with pytest.raises(RuntimeError, match='requires grad'):
        guidance.joint_intensity(m, x.clone().requires_grad_(True))
    g = guidance.SkeletonGuidance(m)
    assert g.target_joints == (3, 11, 7, 18, 14) and g.temporal_positions == 15 and g.temporal_rgb_frames == 5
    with pytest.raises(RuntimeError, match='no CPU'):
        g.apply(x, torch.zeros(1, 3, 8, 8))
    for bad in (dict(target_joints=()), dict(target_joints=(0, 1, 2, 3, 4, 5)), dict(target_joints=(-1,)), dict(temporal_positions=0)):
        with pytest.raises(ValueError):
            guidance.SkeletonGuidance(m, **bad)
    st = stgcn.Model(in_channels=3, num_class=10, num_point=20, num_person=1, graph='tam_gcn_amd.graph.ucla.Graph',
                     graph_args=dict(labeling_mode='spatial'))
    with pytest.raises(TypeError):
        guidance.pooled_feature(st, x)
    with pytest.raises(TypeError):
        guidance.SkeletonGuidance(st)


def test_fake_implementations_give_the_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        h = torch.empty(6, 256, 13, 20)
        inten, pooled, minmax = torch.ops.tamgcn.guidance_reduce(h, 2)
        assert inten.shape == (3, 13, 20, 2) and pooled.shape == (3, 256) and minmax.shape == (6 * 5, 2)
        w = torch.ops.tamgcn.guidance_weights(inten, minmax, torch.empty(5, dtype=torch.int32), 15)
        assert w.shape == (3, 5)
        out, wm = torch.ops.tamgcn.guidance_apply(w, torch.empty(3, 15, 224, 224), 5, 224, 224, True)
        assert out.shape == (3, 15, 224, 224) and wm.shape == (3, 1, 224, 224)
        out, wm = torch.ops.tamgcn.guidance_apply(w, None, 5, 7, 5, True)
        assert out.numel() == 0 and wm.shape == (3, 1, 7, 5)
