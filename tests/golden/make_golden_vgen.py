"""Golden-vector generator for a joint count outside {20, 25, 64}: V = 17, the COCO skeleton.  Like make_golden.py it runs ONLY
in the build container: it imports the reference's own CTRGC, unit_gcn and TCN_GCN_unit (through make_golden.py, which knows where
the read-only reference checkout is), hands them A from tam_gcn_amd.graph.coco and writes *data only* into tests/golden/vgen.npz.  No reference source travels.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vgen.py

Per case (cases_vgen.py) the fixture holds the input, the state the modules ran with -- fill_state_(seed = tag_seed(tag)): every
parameter and buffer drawn so that nothing is at its degenerate initial value (alpha = 0, BatchNorm weights of 1e-6, zero
running statistics); regenerable from the seed, so it is stored as one digest per tensor --, the train-mode output, every
gradient of sum(y * cot), the buffers after the step and the eval-mode output.  tests/test_oracle_vs_golden_vgen.py holds
oracle/ctrgcn_oracle.py to it: the oracle the GPU tests of the run-time-V kernels rely on, pinned to the reference at a V
outside the ones it was checked at.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from params import fill_state_, make_input, digest  # noqa: E402
from cases import NEEDS_A, tag_seed                 # noqa: E402
from cases_vgen import VGEN_MODULE_CASES            # noqa: E402
from make_golden import put, run_module, np32, R    # noqa: E402  (R: the reference's models.ctrgcn)

sys.path.insert(0, ROOT)
from tam_gcn_amd.graph import coco                  # noqa: E402

torch.set_num_threads(8)
torch.manual_seed(0)


def put_state(out, tag, m):
    """Digests of the state run_module is about to give m: one fill of a copy (PA is filled relative to its initial value,
    and the buffers move during the step)."""
    ref = copy.deepcopy(m).state_dict()
    fill_state_(ref, seed=tag_seed(tag))
    out[f'{tag}/state_keys'] = np.array(list(ref.keys()))
    out[f'{tag}/state_digest'] = np.stack([digest(v) for v in ref.values()])


def main():
    out = {}
    A3 = coco.Graph().A
    out['A'] = A3
    for tag, kind, kw, shape, xseed in VGEN_MODULE_CASES:
        V = shape[-1]
        assert V == A3.shape[-1] == 17
        cls = getattr(R, kind)
        x = make_input(shape, xseed)
        put(out, f'{tag}/x', x)
        if kind == 'CTRGC':
            m = cls(**kw)
            put_state(out, tag, m)
            A = torch.from_numpy(A3[1].astype(np.float32))
            A = (A + 0.05 * make_input((V, V), 5)).requires_grad_(True)
            alpha = torch.tensor([0.6], requires_grad=True)
            run_module(m, x, out, tag, extra_fwd=lambda mod, xx: mod(xx, A, alpha))
            out[f'{tag}/A'] = np32(A)
            out[f'{tag}/dA'] = np32(A.grad)
            out[f'{tag}/dalpha'] = np32(alpha.grad)
        else:
            assert kind in NEEDS_A
            kw = dict(kw)
            cin, cout = kw.pop('in_channels'), kw.pop('out_channels')
            m = cls(cin, cout, A3, **kw)
            put_state(out, tag, m)
            run_module(m, x, out, tag)
    path = os.path.join(HERE, 'vgen.npz')
    np.savez_compressed(path, **out)
    print('vgen.npz', len(out), 'arrays', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
