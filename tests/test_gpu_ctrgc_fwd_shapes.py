"""-m gpu: the fused CTRGC forward at the layer shapes the training step runs (l1 l2 l5 l6 l8 l9 of the N-UCLA model, 8 clips)
and at ragged frame counts (T = 20: chunks 16 + 4, T = 40: 16 + 16 + 8), per dispatch form: y, the kept x3 and the BatchNorm
partial moments, slot by slot, against the fp64 reference of the forward ledger at its derived rounding bars
(tests/ctrgc_fwd_ref.py; E as the call built it), and two identical launches bit-equal.  The default dispatch runs in this
process; TAMGCN_CTRGC_FWD2 = 2 (ctrgc_fwd2_kernel wherever it applies) and 3 (E from L2, register-staged operands everywhere)
are read once per process, so each runs this file in a child of its own."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import ctrgc_fwd_ref as FR              # noqa: E402
from params import make_input          # noqa: E402

# name, Cin, Cout, T
STEP_SHAPES = [('l1', 3, 64, 64), ('l2', 64, 64, 64), ('l5', 64, 128, 64), ('l6', 128, 128, 32), ('l8', 128, 256, 32),
               ('l9', 256, 256, 16)]
RAGGED = [('c64-T20', 64, 64, 20), ('c64-T40', 64, 64, 40), ('c256-T20', 256, 256, 20), ('c256-T40', 256, 256, 40)]
N, V, S_ = 8, 20, 3


def reference(x, pq, W3, B3, W4, B4, A, alpha, Cout, R):
    """fp64: x3 = W3 x + b3 per subset, E = alpha (W4 tanh(p_u - q_v) + b4) + A, y = sum_s sum_v E_s x3_s"""
    x, pq, W3, B3, W4, B4, A, alpha = (t.double() for t in (x, pq, W3, B3, W4, B4, A, alpha))
    x3 = torch.einsum('oc,nctv->notv', W3, x) + B3[None, :, None, None]
    y = 0
    for s in range(S_):
        p = pq[(2 * s) * R:(2 * s + 1) * R].permute(1, 0, 2)
        q = pq[(2 * s + 1) * R:(2 * s + 2) * R].permute(1, 0, 2)
        D = torch.tanh(p.unsqueeze(-1) - q.unsqueeze(-2))
        E = alpha * (torch.einsum('cr,nruv->ncuv', W4[s], D) + B4[s][None, :, None, None]) + A[s][None, None]
        y = y + torch.einsum('ncuv,nctv->nctu', E, x3[:, s * Cout:(s + 1) * Cout])
    return y, x3


@pytest.mark.parametrize('case', STEP_SHAPES + RAGGED, ids=lambda c: c[0])
def test_ctrgc_fwd_step_shapes(case):
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    _, Cin, Cout, T = case
    R = 8 if Cin == 3 else Cin // 8
    x = make_input((N, Cin, T, V), 1)
    pq = make_input((S_ * 2 * R, N, V), 2)
    W3 = make_input((S_ * Cout, Cin), 4) * (1.0 / Cin ** 0.5)
    B3 = make_input((S_ * Cout,), 5) * 0.1
    W4 = make_input((S_, Cout, R), 6) * (1.0 / R ** 0.5)
    B4 = make_input((S_, Cout), 7) * 0.1
    A = make_input((S_, V, V), 8) * 0.3
    alpha = torch.tensor([0.7])
    y, x3 = reference(x, pq, W3, B3, W4, B4, A, alpha, Cout, R)
    d = torch.device('cuda:0')
    t = lambda z: z.to(d).contiguous()
    args = (S(t(x)), t(pq), t(W3), t(B3), t(W4), t(B4), t(A), t(alpha), Cin, Cout, S_, R)
    yg, part, x3g = ops.ctrgc_fwd(*args, stats=True, keep_x3=True)
    ey = float((yg.double().cpu() - y).abs().max() / y.abs().max())
    ex = float((x3g.double().cpu() - x3).abs().max() / x3.abs().max())
    print(f'{case[0]}: y max|err|/max|ref| {ey:.3e}, x3 {ex:.3e}')
    # y, x3 and every moment slot at the forward ledger's derived bars (tests/ctrgc_fwd_ref.py), against the E the call built --
    # read back through ops.ctrgc_build_E, so that tanh stays out of the bound; the E builder has its own ledger
    Eg = ops.ctrgc_build_E(*args)
    rat = FR.verify(case[0], dict(x=x, w3=W3, b3=B3, E=Eg.cpu().view(N, S_, Cout, V, V), coff=0, Cin=Cin, Cout=Cout, S=S_),
                    dict(y=yg, x3=x3g, part=part))
    print(f'{case[0]}: err / bar ' + ' '.join(f'{k}={v:.3f}' for k, v in rat.items()))
    yg2, part2, x3g2 = ops.ctrgc_fwd(*args, stats=True, keep_x3=True)
    assert torch.equal(yg2, yg) and torch.equal(x3g2, x3g) and torch.equal(part2, part), 'two identical launches differ'
    y0, _, none = ops.ctrgc_fwd(*args, stats=False)                        # the inference form (no x3 store) computes the same y
    assert none is None and torch.equal(y0, yg)


@pytest.mark.parametrize('mode', ['2', '3'])
def test_ctrgc_fwd_step_shapes_forms(mode):
    if os.environ.get('TAMGCN_CTRGC_FWD2') is not None:
        pytest.skip('already inside a child run')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-m', 'gpu', '-x', '-q', '-k', 'test_ctrgc_fwd_step_shapes and not forms'],
                         cwd=root, env=dict(os.environ, TAMGCN_CTRGC_FWD2=mode), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1000:]
    assert f'{len(STEP_SHAPES) + len(RAGGED)} passed' in out.stdout, out.stdout[-1000:]
