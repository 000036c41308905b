"""-m gpu: ReLU sign bits through the modules -- TAMGCN_SIGNBITS on against off, bit for bit.

  units        TCN_GCN_unit forward + backward at N = 2, T = 8: 64->64 (identity residual: the masked-GEMM route (a)), 64->128
               stride 2 (route (b), convolutional residual), 3->64 without residual (route (a): g has 64 channels), 64->64 at
               V = 25 (route (b): no 16-byte groups).  Output, dx, every parameter gradient and BatchNorm buffer are equal, and
               the launches of each route are the designed ones (counted through the library's call log);
  captured     one CapturedStep replay against its eager twin and against the eager step with the switch off;
  four streams four models forked over four streams at 2 clips each against the same models on one stream;
  stand-alone  unit_gcn and MultiScale_TemporalConv receive a gradient from autograd that is NOT masked: their gradients equal
               the switch-off result (no module assumes a masked input)."""
import copy
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
BITS_ABI = ('tamgcn_gcn_tail_fwd_bits', 'tamgcn_gcn_tail_bwd_bits', 'tamgcn_add_act_fwd_bits', 'tamgcn_add_act_bwd_bits',
            'tamgcn_conv_signmask')
PLAIN_ABI = ('tamgcn_gcn_tail_fwd', 'tamgcn_gcn_tail_bwd', 'tamgcn_add_act_fwd', 'tamgcn_add_act_bwd')


def _rand(gen, *shape, scale=1.0):
    return (torch.rand(shape, generator=gen) * 2 - 1) * scale


def _perturbed(m, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for prm in m.parameters():                               # biases and norms off their initial constants
            prm.add_(_rand(gen, *prm.shape, scale=0.1).to(prm.device))
    return m


def _run(m, x, dout, on, monkeypatch, grad_in=True):
    """(out, dx, grads, buffers, ABI call names, tail forms) of one forward + backward with the switch `on`."""
    from helpers import record_kernels
    from tam_gcn_amd import ops
    monkeypatch.setattr(ops, 'SIGNBITS', on)
    forms = []
    real = ops.gcn_tail_bwd_bits

    def tail(dg, bits, *a, **kw):
        forms.append('a' if bits is None else 'b')
        return real(dg, bits, *a, **kw)
    monkeypatch.setattr(ops, 'gcn_tail_bwd_bits', tail)
    xg = x.clone().requires_grad_(grad_in)
    with record_kernels() as rec:
        out = m(xg)
        out.backward(dout)
        torch.cuda.synchronize()
    monkeypatch.setattr(ops, 'gcn_tail_bwd_bits', real)
    names = [n for n, _ in rec.seen]
    return (out.detach(), xg.grad, {k: v.grad for k, v in m.named_parameters()}, {k: v.clone() for k, v in m.named_buffers()},
            names, forms)


def _assert_equal_runs(a, b):
    assert torch.equal(a[0], b[0]), 'output'
    assert (a[1] is None and b[1] is None) or torch.equal(a[1], b[1]), 'dx'
    assert a[2].keys() == b[2].keys() and len(a[2]) > 0
    for k in a[2]:
        assert a[2][k] is not None and torch.equal(a[2][k], b[2][k]), f'gradient of {k}'
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), f'buffer {k}'


UNITS = [
    ('c64_identity', dict(cin=64, cout=64, stride=1, residual=True, V=20), 'a'),
    ('c64_c128_stride2', dict(cin=64, cout=128, stride=2, residual=True, V=20), 'b'),
    ('c3_c64_no_residual', dict(cin=3, cout=64, stride=1, residual=False, V=20), 'a'),
    ('c64_identity_v25', dict(cin=64, cout=64, stride=1, residual=True, V=25), 'b'),
]


@pytest.mark.parametrize('name,cfg,route', UNITS, ids=[u[0] for u in UNITS])
def test_unit_with_the_switch_on_and_off(name, cfg, route, monkeypatch):
    from helpers import A_BY_V
    from tam_gcn_amd.models import ctrgcn as M
    N, T, V = 2, 8, cfg['V']
    torch.manual_seed(11)
    m_on = _perturbed(M.TCN_GCN_unit(cfg['cin'], cfg['cout'], A_BY_V[V], stride=cfg['stride'], residual=cfg['residual']).to(DEV).train(), 12)
    m_off = copy.deepcopy(m_on)
    gen = torch.Generator().manual_seed(13)
    x = _rand(gen, N, cfg['cin'], T, V).to(DEV)
    T2 = (T - 1) // cfg['stride'] + 1
    dout = _rand(gen, N, cfg['cout'], T2, V).to(DEV)
    on = _run(m_on, x, dout, True, monkeypatch)
    off = _run(m_off, x, dout, False, monkeypatch)
    _assert_equal_runs(on, off)
    # the launches of the route: one for one against today's, and the designed forms
    n_on, n_off = on[4], off[4]
    assert len(n_on) == len(n_off), 'the switch changes which launches run, not how many'
    assert not [n for n in n_off if n in BITS_ABI] and off[5] == []
    assert [n_off.count(n) for n in PLAIN_ABI] == [1, 1, 1, 1]
    assert [n_on.count(n) for n in PLAIN_ABI] == [0, 0, 0, 0]
    assert [n_on.count(n) for n in BITS_ABI[:4]] == [1, 1, 1, 1]
    assert n_on.count('tamgcn_conv_signmask') == (1 if route == 'a' else 0)
    assert n_on.count('tamgcn_conv') + n_on.count('tamgcn_conv_signmask') == n_off.count('tamgcn_conv')
    assert on[5] == [route]


def test_stand_alone_modules_never_assume_a_masked_gradient(monkeypatch):
    """unit_gcn and MultiScale_TemporalConv as their own autograd nodes: the upstream gradient is dense (not masked by g > 0)."""
    from helpers import A_BY_V
    from tam_gcn_amd.models import ctrgcn as M
    N, T, V = 2, 8, 20
    gen = torch.Generator().manual_seed(21)
    torch.manual_seed(22)
    x = _rand(gen, N, 64, T, V).to(DEV)
    dout = _rand(gen, N, 64, T, V).to(DEV)
    assert (dout != 0).all()
    for mod in (M.unit_gcn(64, 64, A_BY_V[V]), M.MultiScale_TemporalConv(64, 64, kernel_size=5, dilations=[1, 2])):
        m_on = _perturbed(mod.to(DEV).train(), 23)
        m_off = copy.deepcopy(m_on)
        on = _run(m_on, x, dout, True, monkeypatch)
        off = _run(m_off, x, dout, False, monkeypatch)
        _assert_equal_runs(on, off)
        assert 'tamgcn_conv_signmask' not in on[4] and 'a' not in on[5], 'a gradient from autograd was taken as masked'
        assert not [n for n in off[4] if n in BITS_ABI]
    # chained through autograd (two nodes): nothing crosses the node boundary
    torch.manual_seed(24)
    seq_on = _perturbed(torch.nn.Sequential(M.unit_gcn(64, 64, A_BY_V[V]), M.MultiScale_TemporalConv(64, 64, kernel_size=5, dilations=[1, 2])).to(DEV).train(), 25)
    seq_off = copy.deepcopy(seq_on)
    on = _run(seq_on, x, dout, True, monkeypatch)
    off = _run(seq_off, x, dout, False, monkeypatch)
    _assert_equal_runs(on, off)
    assert 'tamgcn_conv_signmask' not in on[4] and on[5] == ['b']


# ---------------------------------------------------------------------------------------------------------------------
# captured step, four streams
# ---------------------------------------------------------------------------------------------------------------------
MARGS = dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))


def _model(seed):
    from params import fill_state_
    from tam_gcn_amd.models.ctrgcn import Model
    m = Model(**MARGS)
    fill_state_(m.state_dict(), seed=seed)
    return m.to(DEV).train()


def test_captured_step_equals_its_eager_twin_and_the_switch_off_step(monkeypatch):
    from params import make_input, make_labels
    from tam_gcn_amd import ops
    from tam_gcn_amd.distributed import ParamArena
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.optim import FusedSGD
    from tam_gcn_amd.training import CapturedStep
    B, T, V = 2, 16, 20
    batches = [(make_input((B, 3, T, V, 1), 3 + i).to(DEV), make_labels(B, 10, 103 + i).to(DEV)) for i in range(2)]
    runs = {}
    for mode, on in (('graph', True), ('eager', True), ('eager_off', False)):
        monkeypatch.setattr(ops, 'SIGNBITS', on)
        m = _model(0)
        arena = ParamArena(m)
        bucket = arena.grad_bucket()
        opt = FusedSGD(arena, bucket, lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4)
        step = CapturedStep(m, CrossEntropyLoss(), opt, arena, bucket, *batches[0], eager=(mode != 'graph'))
        losses = [step.step(x, y).clone() for x, y in batches]
        torch.cuda.synchronize()
        bn = [t.clone() for mod in m.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)
              for t in (mod.running_mean, mod.running_var)]
        runs[mode] = (torch.stack(losses).cpu(), arena.flat.cpu(), bucket.flat.cpu(), [t.cpu() for t in bn])
    ref = runs['eager_off']
    for mode in ('graph', 'eager'):
        got = runs[mode]
        assert torch.equal(got[0], ref[0]), (mode, got[0], ref[0])
        assert torch.equal(got[1], ref[1]), f'{mode}: parameters'
        assert torch.equal(got[2], ref[2]), f'{mode}: gradients'
        assert all(torch.equal(a, b) for a, b in zip(got[3], ref[3])), f'{mode}: running statistics'


def test_four_forked_model_streams_equal_one_stream(monkeypatch):
    """Four independent models at 2 clips each, forward and (through autograd) backward on four streams, against the same
    models on the current stream: losses and every gradient equal, sign bits on."""
    from params import make_input, make_labels
    from tam_gcn_amd import ops, functional as Fm
    from tam_gcn_amd.functional import CrossEntropyLoss
    monkeypatch.setattr(ops, 'SIGNBITS', True)
    B, T, V = 2, 16, 20
    x, lab = make_input((B, 3, T, V, 1), 7).to(DEV), make_labels(B, 10, 107).to(DEV)
    ce = CrossEntropyLoss()
    res = {}
    for fork in (True, False):
        models = [_model(s) for s in range(4)]
        pool = [torch.cuda.Stream(DEV) for _ in range(4)] if fork else []
        cur = torch.cuda.current_stream(DEV)
        losses = []
        for i, m in enumerate(models):
            if fork:
                pool[i].wait_stream(cur)
                with Fm.model_stream(pool[i]):
                    losses.append(ce(m(x), lab))
            else:
                losses.append(ce(m(x), lab))
        for st in pool:
            cur.wait_stream(st)
        total = losses[0] + losses[1] + losses[2] + losses[3]
        total.backward()
        torch.cuda.synchronize()
        res[fork] = (torch.stack([l.detach() for l in losses]).cpu(), [p.grad.cpu() for m in models for p in m.parameters()])
    assert torch.equal(res[True][0], res[False][0])
    assert len(res[True][1]) == len(res[False][1]) > 0
    for i, (a, b) in enumerate(zip(res[True][1], res[False][1])):
        assert torch.equal(a, b), f'gradient {i}'
