"""-m gpu: the side-stream schedule, checked two independent ways ("The stream schedule and how it is checked").

  A  the audit      every scenario runs once under stream_audit.Recorder; the happens-before checker must find no hazard, the
                    scenario must really have forked (a launch on a side stream), every library pointer must have an extent,
                    and the launches of the intended route must be in the trace.  Teeth without a racy GPU run: wait edges
                    are deleted from a recorded trace and the checker must name the consumer.
  B  serial/concurrent   every forking scenario with functional.USE_SIDE_STREAMS False and True: outputs, input gradients,
                    parameter gradients, BatchNorm buffers and saved sign bits are torch.equal (the kernels are deterministic
                    and the schedule changes no summation order).
  C  delay injection     the concurrent run again with a torch.cuda._sleep of 3x the scenario's serial duration behind every
                    fork / refork -- on the side stream (late_side: a consumer on main without a join reads too early) or on
                    main (late_main: a side launch without a refork reads before main wrote) -- still equal to the serial bits.
                    A toy of torch ops shows the mechanism catching a missing wait.

Scenarios: TCN_GCN_unit forward + backward at N = 2, T = 16 (64->64 identity residual, 64->128 stride 2 with both
convolutional residuals, the 3->64 first layer), each with ops.tconv_supported as it is and forced off (the per-branch path with
mark / wait), ops.TCN_PAIR and ops.SIGNBITS on and off at V = 20, and at V = 25 where the pair and sign-mask routes are refused;
the launch-fused eval forward; a block, a stand-alone unit_gcn and a stand-alone MS-TCN whose input needs no gradient; an st_gcn block with device dropout (it does not fork:
audited and compared all the same); the small N-UCLA Model through CapturedStep(eager=True), with accumulation, and with the
recorder active during graph capture; and one use of every other hand-written fork / join pair of the package."""
import contextlib
import copy
import functools
import itertools
import json
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fork_sites                                                                   # noqa: E402
import stream_audit as A                                                            # noqa: E402
from params import fill_state_, make_input, make_labels                             # noqa: E402
from tam_gcn_amd import functional as Fn, ops                                       # noqa: E402

DEV = torch.device('cuda:0')
N, T = 2, 16
REPORT = os.environ.get('TAMGCN_AUDIT_REPORT')                # a path: the figures of profiles/stream_schedule_audit.txt go there
_LINES = {}


def _report(key, line):
    _LINES[key] = line
    if REPORT:
        with open(REPORT, 'w') as f:
            f.write('\n'.join(_LINES[k] for k in sorted(_LINES)) + '\n')


@contextlib.contextmanager
def patched(*triples):
    old = [(o, a, getattr(o, a)) for o, a, _ in triples]
    for o, a, v in triples:
        setattr(o, a, v)
    try:
        yield
    finally:
        for o, a, v in reversed(old):
            setattr(o, a, v)


def _rand(gen, *shape, scale=1.0):
    return (torch.rand(shape, generator=gen) * 2 - 1) * scale


# =====================================================================================================================
# scenarios
# =====================================================================================================================
class Scenario:
    forks = True                                           # False: the code under it has no fork site (audited all the same)
    compare = True                                         # False: audit only (captures; pairs USE_SIDE_STREAMS does not govern)
    steps = 1                                              # serial time is divided by it: a block's chain lies within one step
    fork_select = None                                     # delay injection: which Fork objects (by creation index) get delays
    present, absent = (), ()                               # ABI entry points that must / must not be in the trace

    def run(self):
        raise NotImplementedError


class Unit(Scenario):
    """TCN_GCN_unit forward + backward."""

    def __init__(self, cin, cout, stride, V, tconv=True, pair=True, bits=True, grad_in=True, residual=True):
        self.cfg = dict(cin=cin, cout=cout, stride=stride, V=V, tconv=tconv, pair=pair, bits=bits, grad_in=grad_in, residual=residual)
        self.name = f'unit {cin}->{cout} s{stride} V{V} tconv{int(tconv)} pair{int(pair)} bits{int(bits)}' + \
            ('' if grad_in else ' no-dx') + ('' if residual else ' no-res')
        self.expect_bits = bits
        pair_runs = pair and V % 4 == 0 and stride == 1
        self.present = ['tamgcn_tconv_fwd', 'tamgcn_tconv_bwd'] if tconv else ['tamgcn_maxpool_fwd']
        self.absent = [] if tconv else ['tamgcn_tconv_fwd', 'tamgcn_tconv_bwd', 'tamgcn_tconv_wgrad']
        self.present += ['tamgcn_conv_pair', 'tamgcn_wgrad_pair'] if pair_runs else []
        self.absent += [] if pair_runs else ['tamgcn_conv_pair', 'tamgcn_wgrad_pair']
        self.present += ['tamgcn_add_act_fwd_bits', 'tamgcn_gcn_tail_bwd_bits'] if bits else ['tamgcn_add_act_fwd', 'tamgcn_gcn_tail_bwd']
        self.absent += [] if bits else ['tamgcn_add_act_fwd_bits', 'tamgcn_conv_signmask']
        if V % 4:
            self.absent += ['tamgcn_conv_signmask']
        elif bits and stride == 1:
            self.present += ['tamgcn_conv_signmask']

    @functools.cached_property
    def parts(self):
        from helpers import A_BY_V
        from tam_gcn_amd.models import ctrgcn as M
        c = self.cfg
        torch.manual_seed(11)
        m = M.TCN_GCN_unit(c['cin'], c['cout'], A_BY_V[c['V']], stride=c['stride'], residual=c['residual']).to(DEV).train()
        gen = torch.Generator().manual_seed(12)
        with torch.no_grad():
            for prm in m.parameters():                     # biases and norms off their initial constants
                prm.add_(_rand(gen, *prm.shape, scale=0.1).to(DEV))
        x = _rand(gen, N, c['cin'], T, c['V']).to(DEV)
        dout = _rand(gen, N, c['cout'], (T - 1) // c['stride'] + 1, c['V']).to(DEV)
        return m, x, dout

    def run(self):
        m0, x, dout = self.parts
        c = self.cfg
        m = copy.deepcopy(m0)
        bits = []
        real_sign = ops.sign_empty

        def sign_empty(*a, **kw):
            t = real_sign(*a, **kw)
            bits.append(t)
            return t
        patches = [(ops, 'TCN_PAIR', c['pair']), (ops, 'SIGNBITS', c['bits']), (ops, 'sign_empty', sign_empty)]
        if not c['tconv']:
            patches.append((ops, 'tconv_supported', lambda *a, **kw: False))
        with patched(*patches):
            xg = x.clone().requires_grad_(c['grad_in'])
            out = m(xg)
            out.backward(dout)
        res = {'out': out.detach()}
        if c['grad_in']:
            res['dx'] = xg.grad
        for k, p in m.named_parameters():
            assert p.grad is not None, k
            res['grad ' + k] = p.grad
        for k, b in m.named_buffers():
            res['buffer ' + k] = b.detach()
        if self.expect_bits is not None:
            assert bool(bits) == self.expect_bits
        for i, b in enumerate(bits):
            res[f'sign bits {i}'] = b
        return res


class EvalUnit(Unit):
    """The launch-fused eval forward (functional._tcn_forward_eval), without autograd."""

    def __init__(self, cin, cout, stride, V):
        super().__init__(cin, cout, stride, V)
        self.name = f'eval-fused {cin}->{cout} s{stride} V{V}'
        self.present, self.absent = ['tamgcn_maxpool_post_fwd'], ['tamgcn_add_act_fwd', 'tamgcn_tconv_fwd']

    def run(self):
        m0, x, _ = self.parts
        m = copy.deepcopy(m0).eval()
        with torch.no_grad():
            out = m(x)
        return {'out': out}


class Standalone(Unit):
    """unit_gcn / MultiScale_TemporalConv as their own autograd nodes, 64 -> 128 (stride 2), with an input that needs no gradient:
    the need_dx = False form of gcn_backward, the need_dg = need_dxres = False form of tcn_backward."""

    def __init__(self, kind):
        super().__init__(64, 128, 2 if kind == 'MultiScale_TemporalConv' else 1, 20, grad_in=False)
        self.kind, self.name, self.expect_bits = kind, f'stand-alone {kind} 64->128 no-dx', None
        if kind == 'unit_gcn':
            self.present, self.absent = ['tamgcn_ctrgc_bwd_dx3', 'tamgcn_gcn_mid_bwd'], ['tamgcn_tconv_fwd', 'tamgcn_add_act_fwd_bits']
        else:
            self.present, self.absent = ['tamgcn_tconv_fwd', 'tamgcn_tconv_bwd'], ['tamgcn_ctrgc_fwd', 'tamgcn_gcn_tail_bwd_bits']

    @functools.cached_property
    def parts(self):
        from helpers import A_BY_V
        from tam_gcn_amd.models import ctrgcn as M
        torch.manual_seed(21)
        if self.kind == 'unit_gcn':
            m = M.unit_gcn(64, 128, A_BY_V[20])
        else:
            m = M.MultiScale_TemporalConv(64, 128, kernel_size=5, stride=2, dilations=[1, 2])
        m = m.to(DEV).train()
        gen = torch.Generator().manual_seed(22)
        with torch.no_grad():
            for prm in m.parameters():
                prm.add_(_rand(gen, *prm.shape, scale=0.1).to(DEV))
        s = self.cfg['stride']
        return m, _rand(gen, N, 64, T, 20).to(DEV), _rand(gen, N, 128, (T - 1) // s + 1, 20).to(DEV)


class StGcnDropout(Scenario):
    """One st_gcn block with device dropout, forward + backward.  ST-GCN blocks have no fork site."""
    forks = False
    name = 'st_gcn 64->64 k9 dropout'
    present = ['tamgcn_drop_add_act_fwd', 'tamgcn_drop_add_act_bwd']

    @functools.cached_property
    def parts(self):
        from tam_gcn_amd.models import stgcn as M
        blk = M.st_gcn(64, 64, (9, 3), 1, dropout=0.25, residual=True)
        fill_state_(blk.state_dict(), seed=5)
        gen = torch.Generator().manual_seed(6)
        return blk.to(DEV).train(), _rand(gen, N, 64, T, 20).to(DEV), (_rand(gen, 3, 20, 20) * 0.3).to(DEV), _rand(gen, N, 64, T, 20).to(DEV)

    def run(self):
        from tam_gcn_amd import dropout
        blk0, x, Ae, dout = self.parts
        blk = copy.deepcopy(blk0)
        stream = dropout.enable(blk, seed=99)
        stream.set_state(99, 3)
        xg, Ag = x.clone().requires_grad_(True), Ae.clone().requires_grad_(True)
        y = blk(xg, Ag)[0]
        y.backward(dout)
        res = {'out': y.detach(), 'dx': xg.grad, 'dA': Ag.grad}
        res.update({'grad ' + k: p.grad for k, p in blk.named_parameters()})
        res.update({'buffer ' + k: b.detach() for k, b in blk.named_buffers()})
        return res


MARGS = dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
BLOCKS = 10                                                # TCN_GCN_units of the model; each makes 2 Forks forward and 2 backward


def _batches(k):
    return [(make_input((N, 3, T, 20, 1), 3 + i).to(DEV), make_labels(N, 10, 103 + i).to(DEV)) for i in range(k)]


@functools.lru_cache(maxsize=None)
def _seeded_model():
    from tam_gcn_amd.models.ctrgcn import Model
    m = Model(**MARGS)
    fill_state_(m.state_dict(), seed=0)
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def _eval_model():
    """The N-UCLA model with the golden running statistics (seeded ones are the statistics of nothing), never run itself."""
    import stream_ensemble_models as SM
    return SM.base_model('ucla_t52').to(DEV).eval()


def _train_setup():
    from tam_gcn_amd.distributed import ParamArena
    from tam_gcn_amd.optim import FusedSGD
    m = copy.deepcopy(_seeded_model()).train()
    arena = ParamArena(m)
    bucket = arena.grad_bucket()
    return m, arena, bucket, FusedSGD(arena, bucket, lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4)


class ModelSteps(Scenario):
    """The small N-UCLA Model through CapturedStep(eager=True)."""
    present = ['tamgcn_optim_step', 'tamgcn_ctrgc_bwd_dx3', 'tamgcn_tconv_bwd']
    # delays at the forks of l5 (64 -> 128, stride 2) in the first step only: its two Forks of the forward and its two of the
    # backward, among the 4 * BLOCKS Fork objects of a step (every fork of the model would take a minute)
    fork_select = staticmethod(lambda i: i in (8, 9, 4 * BLOCKS - 10, 4 * BLOCKS - 9))

    def __init__(self, accum):
        self.accum, self.steps = accum, 2
        self.name = f'model eager 2 steps accum{accum}'

    def run(self):
        from tam_gcn_amd.functional import CrossEntropyLoss
        from tam_gcn_amd.training import CapturedStep
        m, arena, bucket, opt = _train_setup()
        batches = _batches(2)
        step = CapturedStep(m, CrossEntropyLoss(), opt, arena, bucket, *batches[0], eager=True, accum_steps=self.accum)
        losses = [step.step(x, y).clone() for x, y in batches]
        res = {'parameters': arena.flat.clone(), 'gradients': bucket.flat.clone(), 'losses': torch.stack(losses)}
        res.update({'buffer ' + k: b.detach().clone() for k, b in m.named_buffers()})
        return res


class CaptureStep(Scenario):
    """CapturedStep's constructor with the recorder active: the warm-up steps on its side stream (training.py's fork / join
    pair), then the graph capture, which executes nothing -- what is recorded is the Python schedule, with
    functional._side_ok on its capture branch."""
    compare = False
    name = 'model CapturedStep warm-up and capture'
    present = ['tamgcn_optim_step', 'tamgcn_ctrgc_bwd_dx3']

    def run(self):
        from tam_gcn_amd.functional import CrossEntropyLoss
        from tam_gcn_amd.training import CapturedStep
        m, arena, bucket, opt = _train_setup()
        batches = _batches(1)
        seen = []
        real = Fn._side_ok

        def side_ok(device, main):
            ok = real(device, main)
            seen.append((torch.cuda.is_current_stream_capturing(), ok))
            return ok
        # functional._MODEL_STREAMS never forgets a stream, and torch hands out streams from a pool of 32 that wraps around: in
        # a long-lived process (the whole suite) the default capture stream can alias a stream some earlier caller ran a model
        # on, and the captured step then runs its branches in order -- slower, never a race.  The scenario is about the capture
        # branch of _side_ok, so it runs with the registry of a fresh process and reports whether that alias was there.
        stale = set(Fn._MODEL_STREAMS)
        with patched((Fn, '_MODEL_STREAMS', set()), (Fn, '_side_ok', side_ok)):
            step = CapturedStep(m, CrossEntropyLoss(), opt, arena, bucket, *batches[0])
        dcs = torch.cuda.graph.default_capture_stream
        _report('note capture stream', f'note   the default capture stream was registered as a model stream by earlier work in the process: '
                f'{(DEV.index, dcs.cuda_stream) in stale} ({len(stale)} streams registered)')
        assert (True, True) in seen and (True, False) not in seen, 'the blocks fork during capture, from the capture stream'
        self.keep = step
        return {}


class GraphedSplit(Scenario):
    """inference.GraphedForward with split = 2: its warm-up pair and the model-stream pairs inside the capture."""
    compare, forks = False, True
    name = 'GraphedForward split 2'

    def run(self):
        from tam_gcn_amd.inference import GraphedForward
        m = copy.deepcopy(_eval_model())
        x = make_input((128, 3, T, 20, 1), 5).to(DEV)
        fast = GraphedForward(m, split=2)
        with torch.no_grad():
            out = fast(x)
        self.keep = fast
        return {'out': out}


class EnsembleStreams(Scenario):
    """inference.StreamEnsemble with its models side by side on their own streams (wait pair and record_stream)."""
    compare = False
    name = 'StreamEnsemble on streams'
    present = ['tamgcn_stream_derive', 'tamgcn_score_fuse']

    def run(self):
        from tam_gcn_amd.inference import StreamEnsemble
        models = [copy.deepcopy(_eval_model()) for g in range(2)]
        ens = StreamEnsemble(models, ['joint', 'bone'], arrangement='streams')
        x = make_input((2, 3, 13, 20, 1), seed=1).to(DEV)
        with torch.no_grad():
            f1 = ens.predict(x)[0]
            f2 = ens.predict(x)[0]                         # the second call reuses the side streams' blocks
        assert torch.equal(f1, f2)
        return {'fused': f2}


class LiveCapture(Scenario):
    """streaming.LiveBank's constructor: warm-up on a side stream, then the capture."""
    compare = False
    name = 'LiveBank warm-up and capture'
    present = ['tamgcn_bank_push', 'tamgcn_bank_ema']

    def run(self):
        from tam_gcn_amd.streaming import LiveBank, RingBank
        model = copy.deepcopy(_eval_model())
        self.keep = LiveBank(model, RingBank(2, 12, prep='nucla', V=20, device=DEV), window=8, beta=0.8)
        return {}


class FeederCapture(Scenario):
    """feeder.GraphedBatch's constructor: one batch on a side stream, then the capture."""
    compare = False
    name = 'GraphedBatch warm-up and capture'
    present = ['tamgcn_feeder_draw', 'tamgcn_feeder_transform_indexed']

    def __init__(self, root):
        self.root = root

    def run(self):
        from tam_gcn_amd.feeder.feeder_nucla_gcn import Feeder, GraphedBatch
        rng = np.random.default_rng(11)
        dd = []
        for k, n in enumerate((9, 31, 60, 17)):
            name = f'a{1 + k % 6:02d}_s{k:02d}_e00_v01'
            clip = rng.normal(size=(1, 20, 3)) + 0.05 * np.cumsum(rng.normal(size=(n, 20, 3)), axis=0)
            os.makedirs(os.path.join(self.root, name), exist_ok=True)
            with open(os.path.join(self.root, name, name + '.json'), 'w') as f:
                json.dump({'skeletons': clip.tolist()}, f)
            dd.append({'file_name': name, 'label': 1 + k % 10})
        fd = Feeder(self.root, 'train', data_dict=dd, seed=7)
        self.keep = GraphedBatch(fd, 4)
        return {}


UNITS = []
for cin, cout, stride, residual in ((64, 64, 1, True), (64, 128, 2, True), (3, 64, 1, False)):
    for tconv, pair, bits in itertools.product((True, False), repeat=3):
        UNITS.append(Unit(cin, cout, stride, 20, tconv, pair, bits, residual=residual))
    for tconv in (True, False):
        UNITS.append(Unit(cin, cout, stride, 25, tconv, residual=residual))
UNITS.append(Unit(64, 128, 2, 20, grad_in=False))
UNITS.append(Unit(64, 128, 2, 20, tconv=False, grad_in=False))
UNITS += [Standalone('unit_gcn'), Standalone('MultiScale_TemporalConv')]
COMPARED = UNITS + [EvalUnit(64, 128, 2, 20), EvalUnit(64, 64, 1, 25), StGcnDropout(), ModelSteps(1), ModelSteps(2)]
AUDITED = COMPARED + [CaptureStep(), GraphedSplit(), EnsembleStreams(), LiveCapture()]
TEETH = next(s for s in UNITS if s.name == 'unit 64->128 s2 V20 tconv0 pair1 bits1')
ids = lambda s: s.name                                                               # noqa: E731


# =====================================================================================================================
# A: the audit
# =====================================================================================================================
_AUDITS = {}


def audit(sc):
    """(recorder, report) of one recorded run of the scenario, cached."""
    got = _AUDITS.get(sc.name)
    if got is None:
        with patched((Fn, 'USE_SIDE_STREAMS', True)):
            if sc.compare:
                sc.run()                                   # warm-up: lazily built caches and the allocator's pools
            torch.cuda.synchronize()
            main = torch.cuda.current_stream().cuda_stream
            with A.Recorder() as rec:
                sc.run()
                torch.cuda.synchronize()
        rep = A.Checker().run(rec.trace, main=main)
        got = _AUDITS[sc.name] = (rec, rep)
        _report('audit ' + sc.name, f'audit  {sc.name:58s} launches {rep.launches:5d} (side {rep.side_launches:4d})  accesses {rep.accesses:6d}  '
                f'cross-stream pairs {rep.pairs:6d}  hazards {len(rep.hazards)}  waived {len(rep.waived)}')
    return got


def _check_audit(sc):
    rec, rep = audit(sc)
    assert rep.hazards == [], '\n'.join(repr(h) for h in rep.hazards[:8])
    assert rec.unresolved == [], rec.unresolved[:5]
    assert rec.mismatch == [], rec.mismatch[:5]
    assert all(e['resolved'] for e in rec.launches())
    labels = {e['label'] for e in rec.launches()}
    assert not [n for n in sc.present if n not in labels], (sorted(labels), sc.present)
    assert not [n for n in sc.absent if n in labels], sc.absent
    if sc.forks:
        assert rep.side_launches > 0, 'the scenario did not fork'
    else:
        assert rep.side_launches == 0 and not rec.fork_sites()
    return rec, rep


@pytest.mark.parametrize('sc', AUDITED, ids=ids)
def test_audit_finds_no_hazard(sc):
    _check_audit(sc)


def test_audit_of_the_feeder_capture(tmp_path):
    _check_audit(FeederCapture(str(tmp_path)))


def test_recorder_sees_aten_work_inside_a_custom_backward():
    """The coverage canary: an ATen op issued by a custom autograd.Function's backward, on a side stream, is in the trace
    with its stream, and the checker sees the race it makes."""
    class Canary(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            ctx.side = torch.cuda.Stream()
            return x * 2

        @staticmethod
        def backward(ctx, g):
            ctx.side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(ctx.side):
                r = torch.special.bessel_j0(g)
            torch.cuda.current_stream().wait_stream(ctx.side)
            return r

    x0 = torch.ones(4096, device=DEV, requires_grad=True)
    with A.Recorder() as rec:
        Canary.apply(x0 * 3.0).sum().backward()             # the multiplication's backward reads the canary's result on main
        torch.cuda.synchronize()
    hits = rec.launches('aten::special_bessel_j0')
    assert len(hits) == 1 and hits[0]['stream'] != torch.cuda.current_stream().cuda_stream
    assert A.Checker().run(rec.trace).hazards == []
    cut = A.drop(rec.trace, lambda e: e['op'] == 'wait_stream' and e['other'] == hits[0]['stream'])
    hz = A.Checker().run(cut).hazards
    assert any(h.earlier.label == 'aten::special_bessel_j0' and h.kind == 'read-after-write' for h in hz), hz


def _cut(trace, method, site):
    """The trace without the wait edges the Fork call `method` at `site` produced, and how many were cut."""
    out = A.drop(trace, lambda e: e['op'] in A.WAIT_OPS and e.get('via') == (method, site))
    return out, len(trace) - len(out)


# every partial join of functional.py: (function, method, k-th call) -> what deleting its wait edges must show in the TEETH block's
# trace: (ABI entry point of the consumer, its operand) -- or None where the wait is redundant (DESIGN.md says why for each)
PARTIAL_JOINS = {
    ('_gcn_backward', 'join', 0): ('tamgcn_conv', 'd.bcast'),                       # dxbar from side 1 feeds the dx conv
    ('_gcn_backward', 'refork', 0): None,                                           # side 0 gets no work before the next refork
    ('_gcn_backward', 'refork', 1): ('tamgcn_wgrad', 'd.gy.x1'),                    # W3's weight gradient reads dx3
    ('_gcn_backward', 'refork', 2): None,                                           # Wd's operands were complete before refork 1
    ('_tcn_backward', 'wait', 0): ('tamgcn_bn_bwd_finalize_multi', 'descs[1].part'),   # branch 1's moments (and its dh slice)
    ('_tcn_backward', 'refork', 0): ('tamgcn_wgrad_pair', None),                    # Win / Wl read dh and coefb_h ... (stride 2: tamgcn_wgrad)
    ('_tcn_backward', 'refork', 1): None,                                           # Wr's operands were complete before the first fork
    ('tcn_forward', 'refork', 0): ('tamgcn_conv', 'd.src.x1'),                      # branch 1 reads h_pre and coef_h
}


@pytest.mark.parametrize('key', list(PARTIAL_JOINS), ids=lambda k: f'{k[0]}.{k[1]}#{k[2]}')
def test_deleting_a_partial_join_names_its_consumer(key):
    rec, rep = audit(TEETH)
    assert rep.hazards == []
    site = fork_sites.site(*key)
    cut, n = _cut(rec.trace, key[1], site)
    assert n >= 1, f'{key} at {site} produced no wait edge in the recorded block'
    hz = A.Checker().run(cut).hazards
    want = PARTIAL_JOINS[key]
    if want is None:
        assert hz == [], f'{key} is listed as redundant, but deleting it shows: {hz[:3]}'
        return
    assert hz, f'deleting {key} at {site} shows no hazard'
    label, role = want
    if key == ('_tcn_backward', 'refork', 0):
        label = 'tamgcn_wgrad'                             # the TEETH block is strided: two launches, not the paired one
    assert any(h.later.label == label and (role is None or h.later.role == role) for h in hz), [repr(h) for h in hz[:6]]
    assert all(any(c.startswith('functional.py:') for c in h.later.chain) for h in hz)


def test_every_partial_join_has_a_teeth_case():
    keys = {(fn, attr) for fn, attr, _ in fork_sites.functional_sites() if attr in ('refork', 'join', 'wait')}
    have = {(fn, attr) for fn, attr, _ in PARTIAL_JOINS}
    assert keys == have
    for fn, attr in keys:
        n = len([1 for f, a, _ in fork_sites.functional_sites() if (f, a) == (fn, attr)])
        assert {k for f, a, k in PARTIAL_JOINS if (f, a) == (fn, attr)} == set(range(n))


def test_every_fork_site_is_in_some_scenarios_trace(tmp_path):
    seen, waits = set(), set()
    for sc in AUDITED + [FeederCapture(str(tmp_path))]:
        rec, _ = audit(sc)
        seen |= rec.fork_sites()
        waits |= rec.wait_sites()
    want = {(attr, f'functional.py:{line}') for _, attr, line in fork_sites.functional_sites()}
    assert want - seen == set(), sorted(want - seen)
    other = {f'{f}:{line}' for f, line in fork_sites.other_sites()}
    assert other - waits == set(), sorted(other - waits)


def test_every_waiver_is_hit():
    hit = set()
    for sc in AUDITED:
        hit |= audit(sc)[1].waivers_hit
    assert hit == set(range(len(A.WAIVERS))) and len(A.WAIVERS) <= A.MAX_WAIVERS


# =====================================================================================================================
# B and C: serial against concurrent, and with delays
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def cycles_per_ms():
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cycles = 50_000_000
    e0.record()
    torch.cuda._sleep(cycles)
    e1.record()
    torch.cuda.synchronize()
    cpm = cycles / e0.elapsed_time(e1)
    _report('calibration', f'calibration  torch.cuda._sleep: {cpm:.0f} cycles per millisecond ({cycles} cycles in {cycles / cpm:.2f} ms)')
    return cpm


_SERIAL = {}


def serial(sc):
    """(results, milliseconds per step) of the scenario with the side streams off.  The first run is the reference (and the
    warm-up); two more are timed with events and the shorter one counts -- the span includes the host, and one stall of the
    host would size every sleep of the scenario.  All three must agree bit for bit (what every comparison below rests on)."""
    got = _SERIAL.get(sc.name)
    if got is None:
        with patched((Fn, 'USE_SIDE_STREAMS', False)):
            first = sc.run()
            torch.cuda.synchronize()
            ms = []
            for _ in range(2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                again = sc.run()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
                _same(first, again, 'two serial runs')
        got = _SERIAL[sc.name] = (first, min(ms) / sc.steps)
    return got


def _same(a, b, what):
    assert a.keys() == b.keys() and len(a) > 0
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), f'{what}: {k} differs'


@pytest.mark.parametrize('sc', COMPARED, ids=ids)
def test_serial_equals_concurrent(sc):
    want, _ = serial(sc)
    with patched((Fn, 'USE_SIDE_STREAMS', True)):
        got = sc.run()
        torch.cuda.synchronize()
    _same(want, got, 'side streams on against off')


class Delays:
    """A torch.cuda._sleep behind every fork and refork of the selected Fork objects: on the forked side streams (late_side) or
    on the main stream (late_main)."""

    def __init__(self, mode, cycles, select=None):
        self.mode, self.cycles, self.select, self.count, self.made = mode, int(cycles), select, 0, 0

    def _inject(self, fk, ks):
        if self.select is not None and not self.select(fk._audit_index):
            return
        if self.mode == 'late_side':
            for k in ks:
                with torch.cuda.stream(fk.side[k]):
                    torch.cuda._sleep(self.cycles)
        else:
            with torch.cuda.stream(fk.main):
                torch.cuda._sleep(self.cycles)
        self.count += 1

    def __enter__(self):
        me = self
        init, on, refork = Fn.Fork.__init__, Fn.Fork.on, Fn.Fork.refork

        def __init__(fk, *a, **kw):
            init(fk, *a, **kw)
            fk._audit_index = me.made
            me.made += 1

        def on_(fk, i):
            k = i % len(fk.side) if fk.side else None
            fresh = bool(fk.side) and k not in fk.used
            ctx = on(fk, i)
            if fresh:
                me._inject(fk, [k])
            return ctx

        def refork_(fk):
            refork(fk)
            if fk.side and fk.used:
                me._inject(fk, sorted(fk.used))
        self._ctx = patched((Fn.Fork, '__init__', __init__), (Fn.Fork, 'on', on_), (Fn.Fork, 'refork', refork_))
        self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        return self._ctx.__exit__(*exc)


@pytest.mark.parametrize('mode', ['late_side', 'late_main'])
@pytest.mark.parametrize('sc', [s for s in COMPARED if s.forks], ids=ids)
def test_delayed_concurrent_equals_serial(sc, mode):
    want, ms = serial(sc)
    sleep_ms = 3.0 * ms                                    # outlasts any chain inside a block
    cycles = sleep_ms * cycles_per_ms()
    t0 = time.perf_counter()
    with patched((Fn, 'USE_SIDE_STREAMS', True)), Delays(mode, cycles, sc.fork_select) as d:
        got = sc.run()
        torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    _report(f'delay {sc.name} {mode}', f'delay  {sc.name:58s} {mode:9s}  serial {ms:7.3f} ms/step  sleep {sleep_ms:7.3f} ms = {int(cycles):10d} cycles  '
            f'x {d.count:3d} forks  run {1e3 * wall:7.1f} ms')
    assert d.count > 0, 'no fork was delayed'
    _same(want, got, f'{mode}: delayed side streams against serial')


def _runs_beside_current(s, cycles, sleep_ms):
    """Whether work on stream `s` overlaps work on the current stream: a sleep on `s` must not hold a small launch here back."""
    main = torch.cuda.current_stream()
    if s.cuda_stream == main.cuda_stream:
        return False
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
    x = torch.zeros(64, device=DEV) + 1.0
    e1.record()
    torch.cuda.synchronize()
    del x
    return e0.elapsed_time(e1) < 0.25 * sleep_ms


def test_delay_mechanism_catches_a_missing_wait_on_a_toy():
    """Producer on a side stream, consumer on main, torch ops only.  With the producer delayed, a missing wait_stream makes the
    consumer read too early: the bits differ from the serial run.  With the wait they are equal."""
    sleep_ms = 20.0                                        # far above the serial duration of three small launches
    cycles = int(sleep_ms * cycles_per_ms())
    # The runtime multiplexes streams onto a few hardware queues, and two streams on one queue run in submission order: a
    # delay there shows nothing.  Take a stream that demonstrably runs beside the current one.
    side = next((s for s in (torch.cuda.Stream() for _ in range(8)) if _runs_beside_current(s, cycles, sleep_ms)), None)
    assert side is not None, 'none of eight fresh streams runs beside the current stream'
    main = torch.cuda.current_stream()
    forked = [_runs_beside_current(s, cycles, sleep_ms) for s in Fn._side_streams(DEV, main, 2)]
    _report('note side streams', f'note   the side streams of the current stream run beside it (a delay on them can show a race): {forked}')

    def toy(concurrent, wait):
        a = torch.zeros(1 << 16, device=DEV)
        torch.cuda.synchronize()
        main = torch.cuda.current_stream()
        if not concurrent:
            a.add_(1.0)
            return (a * 2.0).clone()
        side.wait_stream(main)                             # fork
        with torch.cuda.stream(side):
            torch.cuda._sleep(cycles)                      # late_side
            a.add_(1.0)                                    # the producer
        if wait:
            main.wait_stream(side)                         # join
        b = a * 2.0                                        # the consumer on main
        torch.cuda.synchronize()
        return b

    want = toy(False, True)
    assert torch.equal(toy(True, True), want)
    assert not torch.equal(toy(True, False), want), 'the delayed producer did not lose the race: the mechanism has no teeth'
