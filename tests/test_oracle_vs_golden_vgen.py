"""Pins the oracle (oracle/ctrgcn_oracle.py) to the reference at a joint count outside the ones tests/test_oracle_vs_golden.py
checks it at: V = 17, the COCO skeleton (tam_gcn_amd.graph.coco), against tests/golden/vgen.npz, which
tests/golden/make_golden_vgen.py wrote by running the reference's own CTRGC, unit_gcn and TCN_GCN_unit.  The GPU tests of the
run-time-V kernels (tests/test_gpu_vgen_model.py) compare against this oracle."""
import os

import numpy as np
import pytest
import torch

from cases_vgen import VGEN_MODULE_CASES
from helpers import COT_SEED, NEEDS_A, M, tag_seed, fill_state_, make_input, digest, oracle_run, assert_close
from tam_gcn_amd.graph import coco

RTOL, ATOL = 2e-4, 2e-5                     # tests/test_oracle_vs_golden.py's
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vgen.npz')


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def build_module(kind, kw):
    cls = getattr(M, kind)
    if kind in NEEDS_A:
        kw = dict(kw)
        cin, cout = kw.pop('in_channels'), kw.pop('out_channels')
        return cls(cin, cout, coco.Graph().A, **kw)
    return cls(**kw)


def ctrgc_extras(V):
    A = torch.from_numpy(coco.Graph().A[1].astype(np.float32)) + 0.05 * make_input((V, V), 5)
    return A.requires_grad_(True), torch.tensor([0.6], requires_grad=True)


def test_fixture_is_small_and_was_made_on_this_graph(gold):
    assert os.path.getsize(GOLD) < 1024 * 1024
    assert np.array_equal(gold['A'], coco.Graph().A)
    assert {k.split('/')[0] for k in gold.files if '/' in k} == {c[0] for c in VGEN_MODULE_CASES}
    assert [(c[1], c[3]) for c in VGEN_MODULE_CASES] == [('CTRGC', (2, 64, 13, 17)), ('unit_gcn', (2, 3, 13, 17)), ('TCN_GCN_unit', (2, 64, 13, 17))]


@pytest.mark.parametrize('case', VGEN_MODULE_CASES, ids=[c[0] for c in VGEN_MODULE_CASES])
def test_module_case(case, gold):
    tag, kind, kw, shape, xseed = case
    mod = build_module(kind, kw)
    fill_state_(mod.state_dict(), seed=tag_seed(tag))
    # the product module has the reference's keys and the state the reference ran with
    assert list(mod.state_dict().keys()) == list(gold[f'{tag}/state_keys'])
    np.testing.assert_allclose(np.stack([digest(v) for v in mod.state_dict().values()]), gold[f'{tag}/state_digest'], rtol=1e-6, atol=1e-6)
    sd = {'m.' + k: v.detach().clone() for k, v in mod.state_dict().items()}
    pnames = [k for k, _ in mod.named_parameters()]
    for k in pnames:
        sd['m.' + k].requires_grad_(True)
    x = make_input(shape, xseed)
    assert_close('x', x, gold, f'{tag}/x', 0, 0)
    x.requires_grad_(True)
    extras = ctrgc_extras(shape[-1]) if kind == 'CTRGC' else None
    y = oracle_run(kind, kw, sd, x, True, extras)
    cot = make_input(tuple(y.shape), COT_SEED)
    (y * cot).sum().backward()
    assert_close('y', y, gold, f'{tag}/y', RTOL, ATOL)
    assert_close('dx', x.grad, gold, f'{tag}/dx', RTOL * 5, ATOL * 5)
    for k in pnames:
        g = sd['m.' + k].grad
        assert g is not None, k
        scale = float(g.abs().max()) + 1e-6
        assert_close(f'grad {k}', g, gold, f'{tag}/grad/{k}', 2e-3, 2e-4 * max(1.0, scale))
    for k, _ in mod.named_buffers():
        assert_close(f'buf {k}', sd['m.' + k].detach().float(), gold, f'{tag}/buf_after/{k}', 1e-4, 1e-5)
    if kind == 'CTRGC':
        A, alpha = extras
        np.testing.assert_allclose(A.detach().numpy(), gold[f'{tag}/A'], rtol=0, atol=0)
        np.testing.assert_allclose(A.grad.numpy(), gold[f'{tag}/dA'], rtol=2e-3, atol=2e-4)
        np.testing.assert_allclose(alpha.grad.numpy(), gold[f'{tag}/dalpha'], rtol=2e-3, atol=2e-3)
    with torch.no_grad():
        sde = {k: v.detach() for k, v in sd.items()}
        ye = oracle_run(kind, kw, sde, x.detach(), False, tuple(t.detach() for t in extras) if extras else None)
    assert_close('y_eval', ye, gold, f'{tag}/y_eval', RTOL, ATOL)
