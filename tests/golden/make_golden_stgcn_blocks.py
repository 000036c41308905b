"""fp64 pin for the ST-GCN teacher-forced block test (tests/stgcn_block_ref.py).  Runs ONLY in the build container: imports
the reference's models/stgcn.py + graph/ and writes data only -- the reference Model in .double(), train mode, on the
seeded state and input of each case: logits, loss and the input gradient.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stgcn_blocks.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from params import make_input, make_labels             # noqa: E402
from make_golden_stgcn import fill_stgcn_, R           # noqa: E402  (puts the reference on sys.path; R = its models.stgcn)
import graph.ntu_rgb_d                                  # noqa: E402,F401  (reference's)

# the cases of tests/stgcn_block_ref.py that have a graph in the reference (openpose_t18 has none)
_SP = dict(labeling_mode='spatial')
CASES = [('ucla_t13', dict(in_channels=3, num_class=4, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=_SP), (2, 3, 13, 20, 1)),
         ('ntu25_t20', dict(in_channels=3, num_class=4, num_point=25, num_person=1, graph='graph.ntu_rgb_d.Graph', graph_args=_SP), (4, 3, 20, 25, 1))]


def main():
    out = {}
    for tag, margs, shape in CASES:
        m = R.Model(**margs)
        fill_stgcn_(m.state_dict(), seed=77)
        m = m.double().train()
        x = make_input(shape, seed=21).double().requires_grad_(True)
        lab = make_labels(shape[0], margs['num_class'], seed=22)
        logits = m(x)
        loss = torch.nn.functional.cross_entropy(logits, lab)
        loss.backward()
        out[f'{tag}/logits_train64'] = logits.detach().numpy()
        out[f'{tag}/loss64'] = loss.detach().numpy()
        out[f'{tag}/dx64'] = x.grad.numpy()
        print(tag, 'loss', float(loss.detach()))
    np.savez_compressed(os.path.join(HERE, 'stgcn_blocks64.npz'), **out)
    print('stgcn_blocks64.npz', len(out), 'arrays')


if __name__ == '__main__':
    main()
