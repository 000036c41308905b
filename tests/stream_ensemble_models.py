"""Models and references shared by tests/test_stream_ensemble_cpu.py and tests/test_gpu_stream_ensemble.py (not a test file).

Model g of an ensemble: the seeded state of tests/golden/params.py with the golden running statistics of the case (seeded
ones are the statistics of nothing: tests/test_gpu_f2.py::_model), every floating PARAMETER (not buffer) multiplied
elementwise by 1 + EPS*u, u uniform in (-1, 1) from seed g.  All groups then differ in every tensor: a wrong group pointer
is a wrong result.  tests/test_stream_ensemble_cpu.py::test_perturbed_models_stay_tame holds, with the fp64 oracle, that
max|activation| after l10 of every such model stays within 10x of the unperturbed model's (measured: 0.83x .. 1.26x at
EPS = 0.02 for g = 0..3, both cases), so 0.02 did not have to be halved."""
import os

import numpy as np
import torch

from cases import MODEL_CASES, MODEL_PARAM_SEED
from params import fill_state_
from tam_gcn_amd.models import ctrgcn as M
from oracle import ctrgcn_oracle as O

EPS = 0.02
_GOLD = None


def gold():
    global _GOLD
    if _GOLD is None:
        _GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'models.npz'))
    return _GOLD


def base_model(tag, **over):
    """The golden-statistics model of case `tag` (train mode, on the CPU)."""
    margs = dict(next(c for c in MODEL_CASES if c[0] == tag)[1], **over)
    m = M.Model(**margs)
    sd = m.state_dict()
    fill_state_(sd, seed=MODEL_PARAM_SEED)
    g = gold()
    with torch.no_grad():
        for k in sd:
            key = f'{tag}/evalbuf/{k}'
            if 'running_' in k and key in g.files and tuple(g[key].shape) == tuple(sd[k].shape):
                sd[k].copy_(torch.from_numpy(g[key]))
    return m


def perturbed_model(tag, g, eps=EPS, **over):
    m = base_model(tag, **over)
    gen = torch.Generator().manual_seed(g)
    with torch.no_grad():
        for p in m.parameters():
            if p.is_floating_point():
                p.mul_(1 + eps * (2 * torch.rand(p.shape, generator=gen) - 1))
    return m


def state64(m):
    return {k: (v.detach().clone().double().cpu() if v.is_floating_point() else v.clone().cpu()) for k, v in m.state_dict().items()}


def derive(x, parent, stream):
    """Plain-torch restatement of the four stream derivations on (N, C, T, V, M), any dtype: bone x[v] - x[parent[v]], motion
    x[t+1] - x[t] with the last frame 0, bone_motion the motion of bone."""
    def bone(d):
        return d - d[:, :, :, list(parent)]

    def motion(d):
        out = torch.zeros_like(d)
        out[:, :, :-1] = d[:, :, 1:] - d[:, :, :-1]
        return out
    return {'joint': lambda d: d, 'bone': bone, 'motion': motion, 'joint_motion': motion, 'bone_motion': lambda d: motion(bone(d))}[stream](x)


def l10_absmax(m, x):
    """max|activation| after l10 of model m (fp64 oracle, eval mode)."""
    sd = state64(m)
    h, _, _ = O._stem(x.double(), sd, m.num_point, False)
    for i in range(1, 11):
        h = O.tcn_gcn_unit(h, sd, f'l{i}', O._STRIDES.get(i, 1), residual=(i != 1), training=False)
    return float(h.abs().max())


def oracle_scores(models, streams, parent, x):
    """fp64: per model the oracle's eval logits on its stream derived in fp64 -> (G, N, K)."""
    return torch.stack([O.model_forward(derive(x.double(), parent, s), state64(m), m.num_point, training=False)
                        for m, s in zip(models, streams)])
