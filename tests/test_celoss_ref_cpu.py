"""CPU: the fp64 restatement of the cross-entropy options (tests/celoss_ref.py) is torch.nn.functional.cross_entropy over the
whole option product; a correct fp32 evaluation of the GPU ledger's problems passes every bar and one planted mistake does not;
the entry points refuse bad arguments before any HIP call; the Python layer refuses what it cannot run."""
import ctypes as C
import itertools

import pytest
import torch
import torch.nn.functional as F

import celoss_ref as R
import fp64_bars as B

F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------------
# the restatement is torch's
# ---------------------------------------------------------------------------------------------------------------------
def _torch(p):
    l = p['logits'].double().requires_grad_(True)
    w = None if p.get('weight') is None else p['weight'].double()
    tgt = p['labels'] if p.get('labels') is not None else p['probs'].double()
    loss = F.cross_entropy(l, tgt, weight=w, ignore_index=p['ignore_index'], reduction=p['reduction'], label_smoothing=p['eps'])
    loss.sum().backward()                                                    # unit upstream gradient
    return loss.detach(), l.grad


@pytest.mark.parametrize('shape', [(7, 5), (12, 10), (3, 1), (6, 65)])
def test_reference_equals_torch_over_the_option_product(shape):
    N, K = shape
    worst = [0.0, 0.0]
    cases = [dict(o) for o in R.OPTIONS]
    cases += [dict(o, weight='allzero') for o in R.OPTIONS if o['weight'] == 'uniform']
    cases += [dict(o, labels='allign') for o in R.OPTIONS if o['target'] == 'index']
    cases += [dict(o, labels='valid') for o in R.OPTIONS if o['target'] == 'index' and o['weight'] == 'zeros']
    assert len(R.OPTIONS) == 81 + 27
    for o in cases:
        p = R.problem(N, K, **o)
        r = R.ce_opts(p, F64)
        loss, grad = _torch(p)
        assert loss.shape == r.loss.shape, o
        nan = torch.isnan(loss)
        assert bool((torch.isnan(r.loss) == nan).all()), (o, loss, r.loss)
        assert bool(((r.loss - loss).abs()[~nan] <= 1e-12 * loss.abs()[~nan].clamp_min(1.0)).all()), (o, loss, r.loss)
        worst[0] = max(worst[0], float(((r.loss - loss).abs()[~nan]).max()) if bool((~nan).any()) else 0.0)
        if p['reduction'] == 'mean':
            assert bool(nan) == r.nan_loss == r.w_zero, o                   # all ignored, or kept weights that sum to 0: NaN, as torch
        if r.w_zero:
            continue                                                         # x / 0: torch's gradient is as undefined as ours
        assert bool((r.g[~r.valid] == 0).all()) and bool((grad[~r.valid] == 0).all()), o
        assert bool(((r.g - grad).abs() <= 1e-14).all()), (o, float((r.g - grad).abs().max()))
        worst[1] = max(worst[1], float((r.g - grad).abs().max()))
        if o.get('labels') == 'allign' and p['reduction'] != 'mean':
            assert bool((r.loss == 0).all())                                 # sum 0, none all zeros
    assert worst[0] <= 1e-12 and worst[1] <= 1e-14
    if K >= 5:                                                               # kept rows whose weights are all 0 among classes that have one:
        for eps in (0.0, 0.1):                                               # the smoothing terms are positive, the mean is NaN all the same
            p = R.problem(N, K, weight='zeros', eps=eps, labels='valid')
            p['labels'] = p['labels'] // 3 * 3
            r = R.ce_opts(p, F64)
            assert r.w_zero and bool(torch.isnan(r.loss)) and bool(torch.isnan(_torch(p)[0])), eps


def test_eps_zero_never_forms_zero_times_infinity():
    p = R.problem(6, 5, weight='zeros', labels='valid')
    p['logits'] = p['logits'].clone()
    p['logits'][:, 0] = float('-inf')                                        # w_0 = 0 and -logp_0 = inf
    p['labels'] = p['labels'].clamp_min(1)
    r = R.ce_opts(p, F64)
    assert bool(torch.isfinite(r.loss)) and bool(torch.isfinite(r.g).all())
    assert abs(float(r.loss) - float(_torch(p)[0])) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# the bars are achievable and have teeth, on the problems the GPU tests run
# ---------------------------------------------------------------------------------------------------------------------
def test_shape_ledger_covers_what_it_promises():
    assert {K for _, K in R.SHAPES} >= {1, 2, 3, 10, 60, 63, 64, 65, 130, 400}
    assert {N for N, _ in R.SHAPES} >= {1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049}
    assert set(R.MAIN_SHAPES) <= set(R.SHAPES) and len(set(R.SHAPES)) == len(R.SHAPES)
    for s in R.SHAPES:                                                        # every value of every option at every shape
        opts = R.options_of(s)
        for key in ('target', 'weight', 'eps', 'reduction'):
            assert {o[key] for o in opts} == {o[key] for o in R.OPTIONS}, (s, key)
        assert {o['ignore'] for o in opts} == set(R.IGNORES)
    assert all(N * K <= 257 * 400 for N, K in R.SHAPES)


@pytest.mark.parametrize('shape', R.MAIN_SHAPES + [(5, 1), (1025, 3), (5, 400)])
def test_checker_accepts_a_correct_fp32_evaluation(shape):
    for o, lg, lb in itertools.product(R.options_of(shape), ('plain', 'shifted'), ('quarter', 'bad', 'allign')):
        if o['target'] == 'prob' and lb != 'quarter':
            continue
        p = R.problem(*shape, logits=lg, labels=lb, **o)
        rat = R.verify(f'{shape} {R.option_name(o)} {lg} {lb}', p, R.evaluate(p, torch.float32))
        assert all(v <= 1.0 for v in rat.values())


FAULT_OPTIONS = dict(count_divisor=dict(weight='uniform', eps=0.0, reductions=('mean',)),
                     ignored_smoothing=dict(weight=None, eps=0.1, reductions=R.REDUCTIONS),
                     eps_k_minus_1=dict(weight=None, eps=0.1, reductions=R.REDUCTIONS),
                     drop_wj=dict(weight='uniform', eps=0.1, reductions=R.REDUCTIONS),
                     wsum_is_k=dict(weight='uniform', eps=0.1, reductions=R.REDUCTIONS))


@pytest.mark.parametrize('fault', R.FAULTS)
def test_bars_reject_one_mistake(fault):
    assert set(FAULT_OPTIONS) == set(R.FAULTS)
    fo = FAULT_OPTIONS[fault]
    for shape in ((257, 10), (5, 65)):
        for red in fo['reductions']:
            for ign in R.IGNORES:
                p = R.problem(*shape, weight=fo['weight'], eps=fo['eps'], reduction=red, ignore=ign)
                name = f'{fault} {shape} {red} ign={ign}'
                R.verify(name, p, R.evaluate(p, torch.float32))              # the same evaluation without the mistake passes
                with pytest.raises(B.BarError):
                    R.verify(name, p, R.evaluate(p, torch.float32, fault=fault))
    if fault == 'eps_k_minus_1':                                             # the probability targets smooth with eps / K too
        p = R.problem(257, 10, target='prob', eps=0.1)
        with pytest.raises(B.BarError):
            R.verify(fault, p, R.evaluate(p, torch.float32, fault=fault))


def test_bars_reject_wrong_exact_facts():
    p = R.problem(257, 10, weight='uniform', eps=0.1, reduction='none', labels='bad')
    got = R.evaluate(p, torch.float32)
    R.verify('exact', p, got)
    r = R.ce_opts(p)
    ignored = int(torch.nonzero(p['labels'] == -100)[0])
    badrow = int(torch.nonzero(r.nan_loss)[0])
    g = got['g'].clone(); g[ignored, 3] = 1e-30
    with pytest.raises(B.BarError):
        R.verify('exact', p, dict(got, g=g))                                 # an ignored row of g that is not bit-zero
    g = got['g'].clone(); g[badrow, 0] = 1e-30
    with pytest.raises(B.BarError):
        R.verify('exact', p, dict(got, g=g))                                 # a bad row
    loss = got['loss'].clone(); loss[badrow] = 0.0
    with pytest.raises(B.BarError):
        R.verify('exact', p, dict(got, loss=loss))                           # a bad row's loss that is not NaN
    p1 = R.problem(5, 1, eps=0.1, weight='uniform', labels='valid')
    got = R.evaluate(p1, torch.float32)
    assert float(got['loss']) == 0.0 and bool((got['g'] == 0).all())
    with pytest.raises(B.BarError):
        R.verify('K=1', p1, dict(got, loss=torch.tensor(1e-30)))
    gd = torch.randn(4, 64, generator=torch.Generator().manual_seed(0))
    R.verify_bwd('bwd', 'none', gd, torch.tensor([1.5, 0.3, -2.0, 0.7]), gd * torch.tensor([1.5, 0.3, -2.0, 0.7])[:, None])
    with pytest.raises(B.BarError):
        R.verify_bwd('bwd', 'mean', gd, torch.tensor(0.3), (gd.double() * 0.3).float())     # 0.3 is not the fp32 0.3


# ---------------------------------------------------------------------------------------------------------------------
# the ABI without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def _lib():
    from tam_gcn_amd import build, _lib
    build.build()
    lib = C.CDLL(_lib.LIB_PATH)
    lib.tamgcn_last_error.restype = C.c_char_p
    lib.tamgcn_ce_opts_workspace_bytes.restype = C.c_longlong
    return lib, _lib


def test_symbols_and_version():
    lib, mod = _lib()
    assert lib.tamgcn_version() == 401 == mod.ABI_VERSION
    for name in ('tamgcn_ce_opts_workspace_bytes', 'tamgcn_ce_opts_fwd', 'tamgcn_ce_opts_bwd_rows'):
        assert hasattr(lib, name) and name in mod.SIGNATURES, name
    assert C.sizeof(mod.CeDesc) == 64                                        # 4 pointers, int64, double, 3 ints (+ padding)
    from tam_gcn_amd import ops
    assert ops.CE_REDUCTIONS == dict(mean=0, sum=1, none=2)


def test_entry_points_reject_bad_arguments_without_touching_the_gpu():
    lib, mod = _lib()
    buf = (C.c_float * 64)()
    ptr = C.addressof(buf)

    def desc(**kw):
        d = mod.CeDesc()
        d.logits, d.labels, d.weight = ptr, ptr, ptr
        d.ignore_index, d.label_smoothing, d.reduction, d.N, d.K = -100, 0.1, 0, 4, 3
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def both(d, what):
        """the size query and the launch refuse d with their own name and `what` in the message"""
        assert lib.tamgcn_ce_opts_workspace_bytes(C.byref(d)) == -1
        msg = lib.tamgcn_last_error()
        assert b'tamgcn_ce_opts_workspace_bytes' in msg and what in msg, msg
        assert lib.tamgcn_ce_opts_fwd(C.byref(d), ptr, ptr, ptr, None) < 0
        msg = lib.tamgcn_last_error()
        assert b'tamgcn_ce_opts_fwd' in msg and what in msg, msg

    assert lib.tamgcn_ce_opts_workspace_bytes(None) == -1 and b'tamgcn_ce_opts_workspace_bytes: null descriptor' in lib.tamgcn_last_error()
    assert lib.tamgcn_ce_opts_fwd(None, ptr, ptr, ptr, None) < 0 and b'tamgcn_ce_opts_fwd: null descriptor' in lib.tamgcn_last_error()
    both(desc(logits=None), b'null logits')
    both(desc(probs=ptr), b'got both')
    both(desc(labels=None), b'got neither')
    both(desc(N=0), b'N=0')
    both(desc(K=-2), b'K=-2')
    both(desc(label_smoothing=1.5), b'label_smoothing=1.5')
    both(desc(label_smoothing=-0.25), b'label_smoothing=-0.25')
    both(desc(label_smoothing=float('nan')), b'label_smoothing=')
    both(desc(reduction=3), b'reduction=3')
    both(desc(N=1 << 20, K=1 << 11), b'N*K=2147483648')
    d = desc()
    assert lib.tamgcn_ce_opts_fwd(C.byref(d), None, ptr, ptr, None) < 0 and b'tamgcn_ce_opts_fwd: null loss' in lib.tamgcn_last_error()
    assert lib.tamgcn_ce_opts_fwd(C.byref(d), ptr, None, ptr, None) < 0 and b'tamgcn_ce_opts_fwd: null g' in lib.tamgcn_last_error()
    assert lib.tamgcn_ce_opts_fwd(C.byref(d), ptr, ptr, None, None) < 0 and b'null workspace (reduction=0 needs 32 bytes)' in lib.tamgcn_last_error()
    # the size query: 8 N for the reduced forms, nothing for 'none'; weights and probabilities are optional
    assert lib.tamgcn_ce_opts_workspace_bytes(C.byref(desc())) == 32
    assert lib.tamgcn_ce_opts_workspace_bytes(C.byref(desc(reduction=1, N=1000, weight=None))) == 8000
    assert lib.tamgcn_ce_opts_workspace_bytes(C.byref(desc(reduction=2, labels=None, probs=ptr))) == 0
    assert lib.tamgcn_ce_opts_workspace_bytes(C.byref(desc(N=(1 << 31) - 1, K=1, label_smoothing=1.0))) == 8 * ((1 << 31) - 1)
    # the row-scaled backward
    for args, what in (((None, ptr, 4, 3, ptr, None), b'null g'), ((ptr, None, 4, 3, ptr, None), b'null dloss'),
                       ((ptr, ptr, 4, 3, None, None), b'null dlogits'), ((ptr, ptr, 0, 3, ptr, None), b'N=0'),
                       ((ptr, ptr, 4, 0, ptr, None), b'K=0'), ((ptr, ptr, 1 << 16, 1 << 15, ptr, None), b'N*K=2147483648')):
        assert lib.tamgcn_ce_opts_bwd_rows(*args) < 0
        msg = lib.tamgcn_last_error()
        assert b'tamgcn_ce_opts_bwd_rows' in msg and what in msg, msg


# ---------------------------------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------------------------------
def test_module_refuses_what_it_cannot_run():
    from tam_gcn_amd.functional import CrossEntropyLoss
    with pytest.raises(ValueError, match="unknown reduction 'batchmean'"):
        CrossEntropyLoss(reduction='batchmean')
    for eps in (-0.1, 1.5):
        with pytest.raises(ValueError, match='label_smoothing'):
            CrossEntropyLoss(label_smoothing=eps)
    for w in (torch.ones(3, 2), torch.ones(3, dtype=F64), [1.0, 2.0]):
        with pytest.raises(ValueError, match='weight must be a'):
            CrossEntropyLoss(weight=w)
    ce = CrossEntropyLoss(weight=torch.ones(5), ignore_index=2, reduction='sum', label_smoothing=0.1)
    assert 'weight' in dict(ce.named_buffers()) and (ce.ignore_index, ce.reduction, ce.label_smoothing) == (2, 'sum', 0.1)
    assert dict(CrossEntropyLoss().named_buffers()) == {} and CrossEntropyLoss().weight is None
    l, y = torch.randn(4, 5), torch.tensor([0, 1, 2, 3])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ce(l, y)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        CrossEntropyLoss()(l, y)
    for bl, by in ((l.double(), y), (l[0], y), (l, y.int()), (l, y[:3]), (l, torch.rand(4, 4)), (l, torch.rand(4, 5).double())):
        with pytest.raises(RuntimeError, match='expected'):
            ce(bl, by)
