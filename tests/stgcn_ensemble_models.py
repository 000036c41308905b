"""Models shared by tests/test_stgcn_ensemble_cpu.py and tests/test_gpu_stgcn_ensemble.py (not a test file).

Model g of an ST-GCN ensemble: tests/test_gpu_f2s.py's MODELS with fill_stgcn_(state, seed=42 + g).  Every tensor then differs
between the groups, edge_importance included (so Ae = A * edge_importance does too): a wrong group pointer is a wrong result.
tests/test_stgcn_ensemble_cpu.py::test_seeded_models_stay_tame holds, with the fp64 oracle, that every such model's logits stay
finite and within 10x of group 0's in max|.|."""
import functools

import torch

from tam_gcn_amd.models import stgcn as M
from test_stgcn_oracle import fill_stgcn_

SP = dict(labeling_mode='spatial')
# tests/test_gpu_f2s.py's MODELS (restated: that module is marked gpu and patches the routing bound per test)
MODELS = {
    'ucla': dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=SP),
    'openpose': dict(num_class=12, num_point=18, num_person=2, graph='tam_gcn_amd.graph.openpose.Graph', graph_args=SP),
    'coco': dict(num_class=10, num_point=17, num_person=1, graph='tam_gcn_amd.graph.coco.Graph', graph_args=SP),
    'ntu': dict(num_class=60, num_point=25, num_person=2, graph='graph.ntu_rgb_d.Graph', graph_args=SP),
    'tree7': dict(in_channels=2, num_class=6, num_point=7, num_person=1, graph='tam_gcn_amd.graph.synthetic.Graph',
                  graph_args=dict(num_node=7, arity=2)),
}
STREAMS = ['joint', 'bone', 'motion', 'bone_motion']


@functools.lru_cache(maxsize=None)
def _state(name, g):
    m = M.Model(**MODELS[name])
    fill_stgcn_(m.state_dict(), seed=42 + g)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def model(name, g):
    """Group g's model of `name`, eval mode, on the CPU."""
    m = M.Model(**MODELS[name])
    m.load_state_dict(_state(name, g))
    return m.eval()


def sd64(m):
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in m.state_dict().items()}
