"""Golden vectors for gradient saliency (tam_gcn_amd/saliency.py).  Runs ONLY where a checkout of the reference is at hand:
imports the reference's models/stgcn.py + graph/ucla.py and writes data only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_saliency.py <path to the reference checkout>

For every STGCN_MODEL_CASES entry (state fill_stgcn_ seed 77, input seed 21, labels seed 22), in eval mode: the true-class input
gradient (torch.gather(output, 1, label).sum().backward(), the reference's tools/train_stgcn_group.py:300-305) from an fp32 and
an fp64 copy of the model, and the (N, V) joint saliency data.grad.abs().sum((1, 2, 4)) of the fp64 run (:309).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from params import fill_state_, make_input, make_labels  # noqa: E402
from cases import STGCN_MODEL_CASES  # noqa: E402


def fill_stgcn_(sd, seed):
    """make_golden_stgcn.py's: fill_state_, edge_importance ~ 1 + 0.1 N(0,1), the buffer A kept"""
    A = sd['A'].clone()
    fill_state_(sd, seed)
    r = np.random.RandomState(seed + 17)
    with torch.no_grad():
        for k in sorted(sd.keys()):
            if k.startswith('edge_importance'):
                sd[k].copy_(torch.from_numpy((1 + 0.1 * r.standard_normal(tuple(sd[k].shape))).astype(np.float32)))
        sd['A'].copy_(A)


def _grad(m, x, lab):
    x = x.clone().requires_grad_(True)
    m.eval()
    out = m(x)
    torch.gather(out, 1, lab.unsqueeze(1)).squeeze().sum().backward()
    assert all(p.grad is not None for p in m.parameters())                   # the reference's way leaves these behind
    return x.grad.detach()


def main(ref):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    from models import stgcn as R            # the reference's
    torch.set_num_threads(8)
    out = {}
    for tag, margs, shape in STGCN_MODEL_CASES:
        m = R.Model(**margs)
        fill_stgcn_(m.state_dict(), seed=77)
        x = make_input(shape, seed=21)
        lab = make_labels(shape[0], margs['num_class'], seed=22)
        g32 = _grad(m, x, lab)
        g64 = _grad(m.double(), x.double(), lab)
        out[f'{tag}/labels'] = lab.numpy()
        out[f'{tag}/dx32'] = g32.numpy()
        out[f'{tag}/dx64'] = g64.numpy()
        out[f'{tag}/saliency'] = g64.abs().sum((1, 2, 4)).numpy()
        rel = float((g32.double() - g64).norm() / g64.norm())
        cos = float((g32.double() * g64).sum() / (g32.double().norm() * g64.norm()))
        print(f'{tag}: fp32 against fp64 relative L2 {rel:.3e}, cosine {cos:.9f}')
    np.savez_compressed(os.path.join(HERE, 'saliency.npz'), **out)
    print('saliency.npz', len(out), 'arrays')


if __name__ == '__main__':
    main(sys.argv[1])
