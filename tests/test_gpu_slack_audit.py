"""-m gpu: the host's half of the read-slack contract ("Read slack behind streamed activations"), on real launches.

Every scenario runs under slack_audit.SlackAuditor three times: with friendly operands (ops.empty: 16 bytes behind them), and
with the two hostile kinds a caller can hand in --
  a  exact-size storage            torch.empty(n).view(shape)          (ops.with_slack must copy it)
  b  one float into its storage    torch.empty(n + 1)[1:].view(shape)  (unaligned, and it ends with its storage)
-- as inputs, as explicit cotangents of backward(cot), and as the cotangents autograd makes itself ((y * w).sum().backward()).
Every hostile tensor has 4 <= (4 n) % 512 <= 496 (slack_audit.assert_hostile_size): tight for the torch storage, which is what
ops.with_slack and the auditor judge, but with physical bytes behind it in the allocator's block, so that even a kernel the
table wrongly calls `guarded` cannot reach unmapped memory here.

Asserted: no SlackError, no unresolved pointer; hostile results equal the friendly ones bit for bit where the two runs launched
the same kernels (tamgcn_last_kernel), and within test_large_tensor_chunking_matches_single_launch's bars where alignment
picked another kernel form; every hostile input keeps its bits; nothing is copied at V = 20; a Model train step copies no
more tensors than it was handed; every entry point that owns a `stream` pointer was launched with a ragged row (EXCEPTIONS
lists the ones that cannot be, each with its reason); and with ops.with_slack disabled the stand-alone CTRGC backward at the
shape of the fault this audit was written after raises before anything is launched."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import slack_audit as S                                                            # noqa: E402
from helpers import A_BY_V                                                          # noqa: E402
from params import fill_state_, make_input, make_labels                             # noqa: E402
from tam_gcn_amd import ops                                                         # noqa: E402

DEV = torch.device('cuda:0')
KINDS = ('friendly', 'a', 'b')
# what test_large_tensor_chunking_matches_single_launch allows where another kernel form ran: (relative to max |ref|, absolute)
BAR_Y, BAR_DX, BAR_GRAD = (1e-6, 0.0), (1e-5, 0.0), (2e-5, 1e-7)


def _graph(V):
    if V in A_BY_V:
        return A_BY_V[V]
    from tam_gcn_amd.graph import coco, openpose, synthetic
    if V == 17:
        return coco.Graph().A
    if V == 18:
        return openpose.Graph().A
    return synthetic.Graph(num_node=V, arity=2).A


def _operand(src, kind):
    """src's values in a tensor of the given kind (see the module's docstring)."""
    n = src.numel()
    if kind == 'friendly':
        t = ops.empty(*src.shape, like=src)
    else:
        S.assert_hostile_size(n)
        t = torch.empty(n, device=src.device).view(src.shape) if kind == 'a' else torch.empty(n + 1, device=src.device)[1:].view(src.shape)
        st = t.untyped_storage()
        assert st.nbytes() == (t.storage_offset() + n) * 4 and t.is_contiguous()
    t.copy_(src)
    return t


def _rand(seed, *shape, scale=1.0):
    return (make_input(shape, seed) * scale).to(DEV)


# =====================================================================================================================
# scenarios: name, V, inputs {name: tensor}, run(ins) -> {quantity: tensor}
# =====================================================================================================================
class Case:
    train_step = False

    def __init__(self, name, V, inputs, run):
        self.name, self.V, self._inputs, self.run = name, V, inputs, run

    @functools.cached_property
    def inputs(self):
        return self._inputs()


def _module_results(m, y, x, extras=()):
    res = {'y': y.detach()}
    if x.grad is not None:
        res['dx'] = x.grad
    for name, e in extras:
        res['grad ' + name] = e.grad
    for k, p in m.named_parameters():
        if p.grad is not None:
            res['grad ' + k] = p.grad
    for k, b in m.named_buffers():
        res['buffer ' + k] = b.detach().clone()
    return res


def module_case(name, V, build, xshape, cotshape, seed, autograd=False, extras=None, call=None):
    """forward + backward of a module built by build() on x (xshape) with the cotangent `cot` given to backward(), or -- autograd
    -- made by autograd from (y * w).sum()."""
    @functools.lru_cache(maxsize=None)
    def module():
        torch.manual_seed(seed)
        m = build()
        fill_state_(m.state_dict(), seed=seed)
        return m.to(DEV).train()

    def inputs():
        d = {'x': _rand(seed + 1, *xshape)}
        d['w' if autograd else 'cot'] = _rand(seed + 2, *cotshape)
        return d

    def run(ins):
        m = copy.deepcopy(module())
        x = ins['x'].requires_grad_(True)
        ex = extras() if extras else ()
        y = call(m, x, *[e for _, e in ex]) if call else m(x, *[e for _, e in ex])
        assert tuple(y.shape) == tuple(cotshape), (name, tuple(y.shape))
        if autograd:
            (y * ins['w']).sum().backward()
        else:
            y.backward(ins['cot'])
        return _module_results(m, y, x, ex)
    return Case(name + (' autograd-cot' if autograd else ''), V, inputs, run)


def _unit(cin, cout, stride, V, N, T, autograd=False, seed=30):
    from tam_gcn_amd.models import ctrgcn as M
    To = (T - 1) // stride + 1
    return module_case(f'TCN_GCN_unit {cin}->{cout} s{stride} V{V} N{N} T{T}', V,
                       lambda: M.TCN_GCN_unit(cin, cout, _graph(V), stride=stride), (N, cin, T, V), (N, cout, To, V), seed, autograd)


def _ctrgc_extras(V):
    def make():
        A = (torch.from_numpy(_graph(V)[1].astype(np.float32)) + 0.05 * make_input((V, V), 5)).to(DEV).requires_grad_(True)
        return (('A', A), ('alpha', torch.tensor([0.6], device=DEV, requires_grad=True)))
    return make


def _standalone(kind, V, N, T, autograd=False):
    from tam_gcn_amd.models import ctrgcn as M
    if kind == 'CTRGC':
        return module_case(f'CTRGC 32->64 V{V}', V, lambda: M.CTRGC(32, 64), (N, 32, T, V), (N, 64, T, V), 40, autograd, extras=_ctrgc_extras(V))
    if kind == 'unit_gcn':
        return module_case(f'unit_gcn 32->64 V{V}', V, lambda: M.unit_gcn(32, 64, _graph(V)), (N, 32, T, V), (N, 64, T, V), 41, autograd)
    if kind == 'unit_tcn':
        return module_case(f'unit_tcn 32->64 s2 V{V}', V, lambda: M.unit_tcn(32, 64, kernel_size=9, stride=2), (N, 32, T, V),
                           (N, 64, (T - 1) // 2 + 1, V), 42, autograd)
    return module_case(f'MultiScale_TemporalConv 32->64 V{V}', V,
                       lambda: M.MultiScale_TemporalConv(32, 64, kernel_size=5, stride=1, dilations=[1, 2]), (N, 32, T, V), (N, 64, T, V), 43, autograd)


def _st_gcn(V, N, T, dropout_p):
    from tam_gcn_amd.models import stgcn as M

    def extras():
        return (('Ae', _rand(7, 3, V, V, scale=0.3).requires_grad_(True)),)

    def call(m, x, Ae):
        if dropout_p:
            from tam_gcn_amd import dropout
            dropout.enable(m, seed=99).set_state(99, 3)
        return m(x, Ae)[0]
    return module_case(f'st_gcn 32->32 k9 V{V} dropout {dropout_p}', V, lambda: M.st_gcn(32, 32, (9, 3), 1, dropout=dropout_p, residual=True),
                       (N, 32, T, V), (N, 32, T, V), 44, extras=extras, call=call)


NTU = dict(num_class=7, num_point=25, num_person=1, graph='graph.ntu_rgb_d.Graph', graph_args=dict(labeling_mode='spatial'))
COCO = dict(num_class=7, num_point=17, num_person=1, graph='tam_gcn_amd.graph.coco.Graph', graph_args=dict(labeling_mode='spatial'))
TREE23 = dict(num_class=7, num_point=23, num_person=1, graph='tam_gcn_amd.graph.synthetic.Graph', graph_args=dict(num_node=23, arity=2))
OPENPOSE = dict(num_class=7, num_point=18, num_person=1, graph='tam_gcn_amd.graph.openpose.Graph', graph_args=dict(labeling_mode='spatial'))
UCLA = dict(num_class=7, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))


@functools.lru_cache(maxsize=None)
def _model(kind, cfg_name):
    from tam_gcn_amd.models import ctrgcn, stgcn
    cfg = dict(globals()[cfg_name])
    if kind == 'stgcn':
        cfg.update(edge_importance_weighting=True)
        m = stgcn.Model(**cfg)
    else:
        m = ctrgcn.Model(**cfg)
    fill_state_(m.state_dict(), seed=3)
    return m.to(DEV)


def _train_step(kind, cfg_name, N, T):
    V = globals()[cfg_name]['num_point']

    def inputs():
        return {'x': make_input((N, 3, T, V, 1), 11).to(DEV)}

    def run(ins):
        from tam_gcn_amd.functional import CrossEntropyLoss
        m = copy.deepcopy(_model(kind, cfg_name)).train()
        x = ins['x'].requires_grad_(True)
        logits = m(x)
        loss = CrossEntropyLoss()(logits, make_labels(N, 7, 5).to(DEV))
        loss.backward()
        res = {'y': logits.detach(), 'dx': x.grad}
        res.update({'grad ' + k: p.grad for k, p in m.named_parameters() if p.grad is not None})
        return res
    c = Case(f'{kind} Model train step {cfg_name} N{N} T{T}', V, inputs, run)
    c.train_step = True
    return c


def _eval_forward(kind, cfg_name, N, T, family):
    """Model.forward in eval mode: through the general path (TAMGCN_F2=0) or the small-batch family that takes this V."""
    V = globals()[cfg_name]['num_point']

    def inputs():
        return {'x': make_input((N, 3, T, V, 1), 12).to(DEV)}

    def run(ins):
        import os
        m = copy.deepcopy(_model(kind, cfg_name)).eval()
        old = os.environ.get('TAMGCN_F2')
        os.environ['TAMGCN_F2'] = '1' if family else '0'
        try:
            with torch.no_grad():
                return {'y': m(ins['x'])}
        finally:
            if old is None:
                del os.environ['TAMGCN_F2']
            else:
                os.environ['TAMGCN_F2'] = old
    return Case(f'{kind} Model eval {cfg_name} {"family" if family else "general path"} N{N} T{T}', V, inputs, run)


def _saliency(cfg_name, N, T):
    V = globals()[cfg_name]['num_point']

    def run(ins):
        from tam_gcn_amd import saliency
        m = copy.deepcopy(_model('stgcn', cfg_name)).eval()
        lab = make_labels(N, 7, 6).to(DEV)
        return {'dx': saliency.input_gradient(m, ins['x'], labels=lab), 'y': saliency.joint_saliency(m, ins['x'], labels=lab)}
    return Case(f'saliency stgcn {cfg_name} N{N} T{T}', V, lambda: {'x': make_input((N, 3, T, V, 1), 13).to(DEV)}, run)


def _guidance(cfg_name, N, T):
    V = globals()[cfg_name]['num_point']

    def run(ins):
        from tam_gcn_amd import guidance
        m = copy.deepcopy(_model('ctrgcn', cfg_name)).eval()
        return {'y': guidance.joint_intensity(m, ins['x']), 'pooled': guidance.pooled_feature(m, ins['x'])}
    return Case(f'guidance ctrgcn {cfg_name} N{N} T{T}', V, lambda: {'x': make_input((N, 3, T, V, 1), 14).to(DEV)}, run)


def _ring_window(cfg_name, T):
    """Two feeds pushed into a RingBank, their newest window built on the device (torch.empty: tight) and fed to the model."""
    V = globals()[cfg_name]['num_point']

    def run(ins):
        from tam_gcn_amd.streaming import RingBank
        m = copy.deepcopy(_model('ctrgcn', cfg_name)).eval()
        bank = RingBank(2, T + 3, prep='clip', V=V, C=3, M=1, device=DEV)
        bank.push(ins['frames'])
        plan = ops.bank_plan(bank.state, bank.capacity, 1, T, 1)
        win = ops.bank_window_clip(bank.buf, plan, 1, T)
        with torch.no_grad():
            return {'y': m(win), 'window': win}
    return Case(f'RingBank window -> Model {cfg_name} T{T}', V, lambda: {'frames': make_input((2, 3, T, V, 1), 15).to(DEV)}, run)


def _clip_feeder(cfg_name, T):
    V = globals()[cfg_name]['num_point']

    def run(ins):
        from tam_gcn_amd.feeder.clip_feeder import Feeder
        m = copy.deepcopy(_model('ctrgcn', cfg_name)).eval()
        data = make_input((5, 3, T + 2, V, 1), 16).numpy()
        fd = Feeder(None, None, data=data, labels=np.arange(5) % 7, window_size=T, device=DEV)
        x, _, _ = fd.batch([0, 3, 4])
        with torch.no_grad():
            return {'y': m(x), 'batch': x}
    return Case(f'clip feeder batch -> Model {cfg_name} T{T}', V, lambda: {}, run)


def _ensemble(cfg_name, N, T):
    V = globals()[cfg_name]['num_point']

    def run(ins):
        from tam_gcn_amd.inference import StreamEnsemble
        models = []
        for g in range(2):
            m = copy.deepcopy(_model('ctrgcn', cfg_name)).eval()
            fill_state_(m.state_dict(), seed=3 + g)
            models.append(m)
        ens = StreamEnsemble(models, ['joint', 'bone'], arrangement='grouped')
        with torch.no_grad():
            return {'y': ens(ins['x'])}
    return Case(f'StreamEnsemble grouped {cfg_name} N{N} T{T}', V, lambda: {'x': make_input((N, 3, T, V, 1), 17).to(DEV)}, run)


def _custom_ops(V, N, T):
    """torch.ops.tamgcn.* called directly on a caller's tensors: ctrgc, pointwise_conv, head, dropout."""
    def inputs():
        return {'x': _rand(50, N, 32, T, V), 'cot': _rand(51, N, 64, T, V), 'cot_pc': _rand(52, N, 48, T, V), 'cot_drop': _rand(53, N, 32, T, V)}

    def run(ins):
        from tam_gcn_amd import torch_ops                                         # noqa: F401  (registers the ops)
        from tam_gcn_amd.models import ctrgcn as M
        res = {}
        torch.manual_seed(9)
        c = M.CTRGC(32, 64)
        fill_state_(c.state_dict(), seed=54)
        c = c.to(DEV)
        A, alpha = [e for _, e in _ctrgc_extras(V)()]
        x = ins['x'].requires_grad_(True)
        y = c(x, A, alpha)
        y.backward(ins['cot'])
        res.update({'y': y.detach(), 'dx': x.grad.clone(), 'grad A': A.grad, 'grad alpha': alpha.grad})
        x.grad = None
        w, b = _rand(55, 48, 32, 1, 1, scale=0.2).requires_grad_(True), _rand(56, 48, scale=0.2).requires_grad_(True)
        y = torch.ops.tamgcn.pointwise_conv(x, w, b)
        y.backward(ins['cot_pc'])
        res.update({'y pointwise': y.detach(), 'dx pointwise': x.grad.clone(), 'grad w': w.grad, 'grad b': b.grad})
        x.grad = None
        W, hb = _rand(57, 7, 32, scale=0.2).requires_grad_(True), _rand(58, 7, scale=0.2).requires_grad_(True)
        logits = torch.ops.tamgcn.head(x, W, hb, 1)
        logits.backward(_rand(59, N, 7))
        res.update({'y head': logits.detach(), 'dx head': x.grad.clone(), 'grad W': W.grad})
        x.grad = None
        state = torch.tensor([99, 3], dtype=torch.int64, device=DEV)
        out, bits = torch.ops.tamgcn.dropout(x, state, 0, 0.25)
        out.backward(ins['cot_drop'])
        res.update({'y dropout': out.detach(), 'dx dropout': x.grad.clone(), 'keep bits': bits})
        return res
    return Case(f'tamgcn custom ops V{V}', V, inputs, run)


def _direct_ops(V, N, T):
    """The ops wrappers no module reaches with a caller's tensor: each on the caller's tensors as they are."""
    C_ = 32

    def inputs():
        return {'x': _rand(60, N, C_, T, V), 'g': _rand(61, N, C_, T, V), 'x3': _rand(62, N, 3 * C_, T, V)}

    def run(ins):
        x, g, x3 = ins['x'], ins['g'], ins['x3']
        Sx, Sg = ops.S(x), ops.S(g)
        res = {}
        w = _rand(63, C_, C_, 1, 1, scale=0.2)
        res['y conv'] = ops.conv(Sx, K=C_, w=w, bias=None, M=C_)[0]
        w5 = _rand(64, C_, C_, 5, 1, scale=0.2)
        res['y conv k5'] = ops.conv(Sx, K=C_, w=w5, bias=None, M=C_, KT=5, pad=2)[0]
        res['grad wgrad'] = ops.wgrad(Sg, Sx, C_, C_)
        res['grad wgrad k5'] = ops.wgrad(Sg, Sx, C_, C_, KT=5, pad=2)
        res['y tmean'] = ops.tmean(Sx, C_)
        res['y add_act'] = ops.add_act_fwd(Sx, Sg, True, C_)
        yp = ops.empty(N, C_, T, V, like=x)
        ops.maxpool_fwd(Sx, C_, 1, yp, 0, False)
        res['y maxpool'] = yp
        dE = ops.ctrgc_bwd_de_acc(Sg, x3, C_, 3)
        res['grad dE'] = dE
        return res
    return Case(f'ops wrappers V{V}', V, inputs, run)


def _cases():
    return [
        # TCN_GCN_unit, the stream route (V = 25) and the vgen route (V = 17, 23: V % 4 = 1, 3; V = 18: V % 4 = 2)
        _unit(64, 64, 1, 25, 3, 7), _unit(32, 64, 2, 25, 3, 9), _unit(64, 64, 1, 25, 3, 7, autograd=True),
        _unit(64, 64, 1, 17, 3, 7), _unit(32, 64, 2, 23, 3, 9), _unit(32, 32, 1, 18, 3, 7), _unit(32, 64, 2, 17, 3, 9, autograd=True),
        _unit(3, 48, 1, 20, 3, 7),                     # the control: nothing copied, nothing ragged (48 channels: a hostile size)
        # stand-alone modules with a caller's cotangent
        _standalone('CTRGC', 25, 3, 7), _standalone('CTRGC', 17, 3, 7, autograd=True), _standalone('unit_gcn', 25, 3, 7),
        _standalone('unit_gcn', 23, 3, 7, autograd=True), _standalone('unit_tcn', 25, 3, 9), _standalone('MultiScale_TemporalConv', 25, 3, 7),
        _standalone('MultiScale_TemporalConv', 17, 3, 9, autograd=True),
        _st_gcn(25, 3, 7, 0), _st_gcn(25, 3, 7, 0.25),
        # models
        _train_step('ctrgcn', 'NTU', 3, 9), _train_step('ctrgcn', 'COCO', 3, 9), _train_step('stgcn', 'NTU', 3, 9),
        _eval_forward('ctrgcn', 'NTU', 3, 9, False), _eval_forward('stgcn', 'NTU', 3, 9, False),
        _eval_forward('ctrgcn', 'NTU', 3, 9, True), _eval_forward('ctrgcn', 'COCO', 3, 9, True), _eval_forward('ctrgcn', 'OPENPOSE', 3, 9, True), _eval_forward('ctrgcn', 'TREE23', 3, 9, True),
        _eval_forward('stgcn', 'NTU', 3, 9, True), _eval_forward('ctrgcn', 'UCLA', 2, 6, True),
        _ensemble('NTU', 3, 9),
        _saliency('NTU', 3, 9), _guidance('NTU', 3, 9), _ring_window('NTU', 9), _clip_feeder('NTU', 9),
        _custom_ops(25, 3, 7), _direct_ops(25, 3, 7), _direct_ops(17, 3, 9),
    ]


CASES = _cases()

# entry points that own a `stream` pointer and are not launched with a ragged row here: why
EXCEPTIONS = {
    'tamgcn_conv_signmask': 'refused by the library unless V % 4 == 0 (conv.hip: tamgcn_conv_signmask)',
    'tamgcn_conv_pair': 'ops.pair_supported admits V % 4 == 0 only: functional takes the two launches at a ragged V',
    'tamgcn_f2_e': 'f2 is built for V = 20 only', 'tamgcn_f2_gcn': 'f2 is built for V = 20 only', 'tamgcn_f2_tcn': 'f2 is built for V = 20 only',
    'tamgcn_f2_e_grouped': 'f2 is built for V = 20 only', 'tamgcn_f2_gcn_grouped': 'f2 is built for V = 20 only',
    'tamgcn_f2_tcn_grouped': 'f2 is built for V = 20 only',
}


# =====================================================================================================================
# the runs
# =====================================================================================================================
_RUNS = {}


def _audit(case, kind):
    """(results, auditor, the hostile inputs and their sources) of one run, once per process."""
    key = (case.name, kind)
    if key not in _RUNS:
        src = case.inputs
        with S.SlackAuditor() as aud:
            ins = {k: _operand(v, kind) for k, v in src.items()}
            res = case.run(ins)
            torch.cuda.synchronize()
        kept = all(torch.equal(ins[k].detach(), src[k]) for k in src)
        _RUNS[key] = (res, aud, kept, [tuple(v.shape) for v in src.values()])
    return _RUNS[key]


def _close(name, got, ref, bar):
    got, ref = got.detach().double(), ref.detach().double()
    assert got.shape == ref.shape, name
    scale = float(ref.abs().max()) + 1e-6
    err = float((got - ref).abs().max())
    assert err <= bar[0] * scale + bar[1], f'{name}: max-abs-err {err:.3e} > {bar[0]:g} * {scale:.3e} + {bar[1]:g}'


def _bar(q):
    if q.startswith('grad'):
        return BAR_GRAD
    return BAR_DX if q.startswith('dx') else BAR_Y


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_scenario_is_clean_and_hostile_equals_friendly(case):
    ref, aud0, _, _ = _audit(case, 'friendly')
    assert aud0.unresolved == [], aud0.unresolved[:3]
    assert aud0.launches, 'nothing was launched'
    for kind in ('a', 'b') if case.inputs else ():
        res, aud, kept, shapes = _audit(case, kind)              # a SlackError would have been raised here
        assert aud.unresolved == [], (kind, aud.unresolved[:3])
        assert kept, f'kind {kind}: a hostile input changed'
        assert set(res) == set(ref)
        same = aud.kernels() == aud0.kernels()
        print(f'{case.name} kind {kind}: {len(aud.launches)} launches, {len(aud.ragged_entries())} ragged entry points, '
              f'copies {aud.copies}, kernels {"same" if same else "differ"}')
        for q in sorted(ref):
            if ref[q] is None:
                assert res[q] is None
            elif same or not ref[q].is_floating_point():
                assert torch.equal(res[q], ref[q]), f'kind {kind}: {q} differs from the friendly run (same kernels)'
            else:
                _close(f'kind {kind}: {q}', res[q], ref[q], _bar(q))
        # what was copied is what was handed in (or a cotangent autograd made of such a shape): never a tensor of the ops' own
        handed = set(shapes) | {tuple(v.shape) for v in ref.values() if v is not None}
        assert all(shape in handed for shape, _ in aud.copies), aud.copies
        if case.V % 4 == 0:
            assert aud.copies == [] and not aud.ragged_entries()
        if case.train_step:
            assert len(aud.copies) <= len(shapes), aud.copies
    if case.V % 4 == 0:
        assert aud0.copies == [] and not aud0.ragged_entries()
    # the friendly run copies only what torch itself made on the way (a cotangent from autograd), never an operand of its own
    made = {tuple(v.shape) for v in ref.values() if v is not None}
    assert all(shape in made for shape, _ in aud0.copies), aud0.copies


def _write_report(path, owners, per_case):
    """profiles/slack_audit.txt: the classification table, scenario x entry point, the copies per scenario."""
    cols = sorted(owners)
    out = ['classification of every const float* of include/tamgcn.h (tests/slack_audit.py)', '']
    for (owner, name), e in sorted(S.CLASSES.items()):
        note = {S.STREAM: f'row length from {e.v}; {e.why}', S.FLAT: e.why,
                S.GUARDED: '; '.join(f'csrc/{f}: {t}' for f, t in e.cites) + (f'  ({e.why})' if e.why else '')}[e.cls]
        out.append(f'{e.cls:8} {owner}: {name:12} {note}')
    out += ['', 'entry points that own a stream pointer (columns of the matrix below)', '']
    out += [f'  {i:2}  {c}: {", ".join(owners[c])}' + (f'   -- EXCEPTION: {EXCEPTIONS[c]}' if c in EXCEPTIONS else '') for i, c in enumerate(cols)]
    out += ['', 'scenario x entry point: R = launched with a ragged row (V % 4 != 0) under the audit, in any of the three runs', '',
            ' ' * 66 + ' '.join(f'{i:2}' for i in range(len(cols)))]
    for name, (ran, copies) in per_case.items():
        out.append(f'{name[:64]:64}  ' + ' '.join(' R' if c in ran else ' .' for c in cols))
    out += ['', "copies ops.with_slack made per scenario and run (friendly / a / b): count, then shape @ call site of the hostile runs' copies", '']
    for name, (ran, copies) in per_case.items():
        sites = sorted({f'{shape} @ {site}' for k in ('a', 'b') for shape, site in copies.get(k, [])})
        out.append(f'{name[:64]:64}  ' + ' / '.join(str(len(copies[k])) if k in copies else '-' for k in KINDS) + ('   ' + '; '.join(sites) if sites else ''))
    with open(path, 'w') as f:
        f.write('\n'.join(out) + '\n')


def test_every_stream_entry_point_ran_ragged():
    import os
    owners = S.stream_owners()
    assert set(EXCEPTIONS) <= set(owners), 'an exception for an entry point that owns no stream pointer'
    ran, per_case = set(), {}
    for case in CASES:
        mine, copies = set(), {}
        for kind in KINDS if case.inputs else ('friendly',):
            aud = _audit(case, kind)[1]
            mine |= aud.ragged_entries()
            copies[kind] = aud.copies
        per_case[case.name] = (mine, copies)
        ran |= mine
    if os.environ.get('TAMGCN_SLACK_REPORT'):                   # a path: the tables of profiles/slack_audit.txt go there
        _write_report(os.environ['TAMGCN_SLACK_REPORT'], owners, per_case)
    missing = sorted(set(owners) - ran - set(EXCEPTIONS))
    assert not missing, f'never launched with a ragged row under the audit: {missing}'
    stale = sorted(set(EXCEPTIONS) & ran)
    assert not stale, f'listed as exceptions but launched ragged: {stale}'


def test_without_with_slack_the_ctrgc_backward_is_stopped_before_the_launch(monkeypatch):
    """The fault this audit was written after: a caller's cotangent (2, 128, 6, 25) -- 300 granules of 512 bytes, nothing behind
    it -- reaching the aggregation backward.  With ops.with_slack disabled the auditor must stop it; nothing is launched."""
    from tam_gcn_amd.models import ctrgcn as M
    monkeypatch.setattr(ops, 'with_slack', lambda t: t)
    torch.manual_seed(1)
    c = M.CTRGC(64, 128).to(DEV)
    A, alpha = [e for _, e in _ctrgc_extras(25)()]
    x = ops.empty(2, 64, 6, 25, like=A).copy_(_rand(70, 2, 64, 6, 25)).requires_grad_(True)
    n = 2 * 128 * 6 * 25
    assert (4 * n) % 512 == 0
    cot = torch.zeros(n, device=DEV).view(2, 128, 6, 25)
    with S.SlackAuditor() as aud:
        y = c(x, A, alpha)
        torch.cuda.synchronize()
        with pytest.raises(S.SlackError) as ei:
            y.backward(cot)
        torch.cuda.synchronize()
        assert aud.violations == [(len(aud.launches), ei.value)], 'something was launched after the violation'
        assert not any(e['entry'].endswith('agg_bwd') for e in aud.launches)
    e = ei.value
    assert e.entry == 'tamgcn_ctrgc_tiled_agg_bwd' and e.role == 'dy.x1' and e.shape == (2, 128, 6, 25) and e.behind == 0
