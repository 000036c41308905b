"""-m gpu: every CTR-GCN module a caller can construct alone, on the HIP path, against a teacher-forced fp64 reference at
fp32-rounding bars -- the layer tests/test_gpu_blocks.py is for the fused block and tests/test_gpu_stgcn_blocks.py for ST-GCN.
CTRGC (torch.ops.tamgcn.ctrgc), unit_gcn (UnitGCNFn), TemporalConv / unit_tcn (ConvBNFn) and MultiScale_TemporalConv (MSTCNFn)
each have Python composition code of their own in tam_gcn_amd/functional.py; the kernels under them are pinned form by form,
this file is what catches a wrong COMPOSITION of right kernels: the dxbar / T broadcast of CTRGC's backward, dg + dxres of the
stand-alone MS-TCN, the per-branch fallbacks of _tcn_backward, a residual kernel wider than one, no final ReLU, a backward
through eval-mode BatchNorm, and the forms of each node that depend on what the caller asks a gradient for.

Cases, teachers, bars and judge() are tests/ctrgcn_module_ref.py (tests/test_ctrgcn_modules_cpu.py shows the bars bite).  Every
case runs in both arithmetic modes and with BatchNorm in train and in eval mode (CTRGC has none: once per arithmetic mode).
-s prints one line per case with err / bar of every quantity; profiles/ctrgcn_module_bars.txt holds one full run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import ctrgcn_module_ref as R                                                   # noqa: E402
from helpers import record_kernels                                              # noqa: E402

DEV = torch.device('cuda:0')
MODES = pytest.mark.parametrize('mode', [1, 0], ids=['split_bf16_bwd', 'exact_f32'])
RUNS = [(tag, bn) for tag in R.CASES for bn in (('train',) if R.kind_of(tag) == 'CTRGC' else ('train', 'eval'))]
SEEN = {}                                             # tag -> [set of ABI entry points launched by one forward + backward]


def _split_mode(mode):
    from tam_gcn_amd import _lib
    lib = _lib.load()
    prev = lib.tamgcn_get_split_mode()
    lib.tamgcn_set_split_mode(mode)
    return lambda: lib.tamgcn_set_split_mode(prev)


def _module(tag, training=True):
    return R.build(tag).to(DEV).train(training)


def _frozen(mod, what):
    """Names of the parameters variant `what` freezes: 'all', 'graph' (PA and alpha) or 'bn' (the BatchNorm affines)."""
    names = [k for k, _ in mod.named_parameters()]
    if what == 'all':
        return set(names)
    if what == 'graph':
        return {k for k in names if k.split('.')[-1] in ('PA', 'alpha')}
    if what == 'bn':
        return {(k + '.' if k else '') + a for k, m in mod.named_modules() if isinstance(m, torch.nn.BatchNorm2d) for a in ('weight', 'bias')}
    return set()


def _run(mod, tag, t, x_grad=True, freeze=None, backward=True, emit=False):
    """One forward + backward of the module at the teacher's input, its buffers put back to the seeded state first (an earlier
    train-mode run moved them): {quantity: tensor} as ctrgcn_module_ref.evaluate gives, plus 'rowmean' with emit."""
    pristine = R.module(tag).state_dict()
    with torch.no_grad():
        for k, buf in mod.named_buffers():
            buf.copy_(pristine[k].to(buf.dtype))
    frozen = _frozen(mod, freeze)
    for k, p in mod.named_parameters():
        p.grad = None
        p.requires_grad_(k not in frozen)
    x = t.x.float().to(DEV).contiguous().requires_grad_(x_grad)
    ex = R.extras(tag, torch.float32, DEV, grad=freeze not in ('all', 'graph'))
    q = {}
    try:
        with record_kernels() as rec:
            if ex is not None:
                y = mod(x, ex[0], ex[1])
            elif emit:
                y, q['rowmean'] = mod(x, emit_pool=True)
            else:
                y = mod(x)
            if backward:
                y.backward(R.cot(tag).to(DEV))
            torch.cuda.synchronize()
        SEEN.setdefault(tag, []).append({name for name, _ in rec.seen})
        q.update({'y': y.detach(), 'dx': x.grad, 'requires_grad': y.requires_grad})
        if ex is not None:
            for name, e in zip(('dA', 'dalpha'), ex):
                if isinstance(e, torch.Tensor):
                    q[name] = e.grad
        q.update({'grad/' + k: p.grad for k, p in mod.named_parameters()})
        q.update({'buf/' + k: b.detach().clone() for k, b in mod.named_buffers()})
    finally:
        for p in mod.parameters():
            p.requires_grad_(True)
    return q


def _same(a, b, skip=()):
    """Bit-equality of two runs' quantities (None where a gradient was not asked for), those in `skip` aside."""
    bad = [k for k in a if k not in skip and not ((a[k] is None and b.get(k) is None) or (
        a[k] is not None and b.get(k) is not None and (a[k] == b[k] if isinstance(a[k], bool) else torch.equal(a[k], b[k]))))]
    assert a.keys() == b.keys() and not bad, f'differ: {bad}'


@MODES
@pytest.mark.parametrize('tag,bn', RUNS, ids=[f'{R.case_id(t)}-{b}' for t, b in RUNS])
def test_module_teacher_forced(tag, bn, mode):
    """Output, dx, every parameter gradient, dA / dalpha and the BatchNorm buffers after the forward against the fp64 teacher.
    bn = 'eval': the backward on running statistics, the buffers bit-equal before and after."""
    training = bn == 'train'
    t = R.teacher(tag, training)
    mod = _module(tag, training)
    restore = _split_mode(mode)
    try:
        got = _run(mod, tag, t)
    finally:
        restore()
    ratios, misses = R.judge(got, t, mode, buffers=training)
    print(R.line(f'{tag} mode {mode} bn {bn} nudges {t.tries} worst {max(ratios.values()):.2g}', ratios))
    assert not misses, f'{tag} mode {mode} bn {bn}: ' + '; '.join(misses)
    if not training:
        pristine = R.module(tag).state_dict()
        assert all(torch.equal(got['buf/' + k].cpu(), pristine[k]) for k, _ in mod.named_buffers()), 'buffers changed in eval mode'


FORM_CASES = ['gcn 64->64 v20', 'ms 64 k5 identity', 'ms 64->128 s2 rk3', 'tconv 32 k5 s2 d2', 'ctrgc 64->64 v20', 'unit 64->64 s1',
              'unit 64->128 s2']
FIXED_A = {R.CASES[t][3]['partner']: t for t in R.CASES if 'partner' in R.CASES[t][3]}


@MODES
@pytest.mark.parametrize('tag', FORM_CASES, ids=R.case_id)
def test_forms_of_the_node(tag, mode):
    """The branches of each autograd node that depend on what the caller asks for.  Every form runs the same kernels on the same
    operands as the full run for what it still computes (functional.py: need_dx / need_dg / need_dxres only skip launches,
    a frozen parameter's gradient is computed and dropped by autograd), so bit-equality is asked everywhere."""
    t = R.teacher(tag, True)
    mod = _module(tag)
    grads = [k for k in t.q if k.startswith('grad/')]
    restore = _split_mode(mode)
    try:
        full = _run(mod, tag, t)
        R.verify(full, t, mode)
        # (a) the same run twice: side streams, no atomics
        _same(full, _run(mod, tag, t))
        # (b) the input asks for no gradient (TCN_GCN_unit: the form of block l1 in a training step)
        nox = _run(mod, tag, t, x_grad=False)
        assert nox['dx'] is None
        _same(full, nox, skip=('dx',))
        # (c) frozen parameters keep grad None; dx and the remaining gradients do not move
        for what in ('all', 'graph', 'bn'):
            frozen = {'grad/' + k for k in _frozen(mod, what)}
            if R.kind_of(tag) == 'CTRGC' and what != 'bn':
                frozen |= {'dA', 'dalpha'}
            if not frozen:
                continue                              # nothing of that kind in this module
            fr = _run(mod, tag, t, freeze=what)
            assert all(fr[k] is None for k in frozen), f'{what}: a frozen parameter has a gradient'
            assert all(fr[k] is not None for k in grads if k not in frozen)
            _same(full, fr, skip=frozen)
        # (d) adaptive=False on the same A: nothing reaches A, nothing else moves
        if tag in FIXED_A:
            fmod = _module(FIXED_A[tag])
            fx = _run(fmod, FIXED_A[tag], t)
            pa = {k for k in full if k.endswith('PA')}
            assert pa and not any(k.endswith('PA') for k in fx)
            _same({k: v for k, v in full.items() if k not in pa}, fx)
            for m in fmod.modules():
                if hasattr(m, 'adaptive'):
                    assert not m.A.requires_grad and m.A.grad is None
        # (f) TCN_GCN_unit(emit_pool=True): the same output and gradients, the row means of the output beside it
        if R.kind_of(tag) == 'TCN_GCN_unit':
            em = _run(mod, tag, t, emit=True)
            rm = em.pop('rowmean')
            _same(full, em)
            ref = t.q['y'].mean((2, 3))
            err = float((rm.detach().cpu().double() - ref).abs().max() / ref.abs().max())
            assert tuple(rm.shape) == tuple(ref.shape) and err <= R.REL_Y, f'row means {err:.2e}'
        # (e) nothing requires a gradient, grad mode on, eval mode: the output of torch.no_grad()
        mod.eval()
        te = R.teacher(tag, False) if R.kind_of(tag) != 'CTRGC' else t
        on = _run(mod, tag, te, x_grad=False, freeze='all', backward=False)
        with torch.no_grad():
            off = _run(mod, tag, te, x_grad=False, freeze='all', backward=False)
        assert not on['requires_grad'] and torch.equal(on['y'], off['y'])
        assert R._relerr(on['y'], te.q['y']) <= R.REL_Y
    finally:
        restore()


def _routes(names):
    tcn = 'tamgcn_maxpool_bwd' in names               # an MS-TCN backward ran (its pooled branch always takes this entry point)
    fused, pair = 'tamgcn_tconv_bwd' in names, 'tamgcn_wgrad_pair' in names
    return {r for r, on in (('fused temporal route (tamgcn_tconv_bwd)', fused), ('per-branch fallback', tcn and not fused),
                            ('tamgcn_wgrad_pair', pair), ('two-launch route', tcn and not pair)) if on}


def test_the_table_reaches_all_four_routes():
    """The ABI launches of the whole case table, recorded by the tests above (a case they did not run is run here): the fused
    temporal route, the per-branch fallback, the paired weight gradient and the two-launch route each serve at least one case,
    so a later planner change cannot empty a branch of _tcn_backward of its test without notice."""
    for tag in R.CASES:
        if tag not in SEEN:
            _run(_module(tag), tag, R.teacher(tag, True))
    seen = {}
    for tag, runs in SEEN.items():
        for names in runs:
            for r in _routes(names):
                seen.setdefault(r, set()).add(tag)
    for r, tags in sorted(seen.items()):
        print(f'route {r}: {sorted(tags)}')
    assert set(seen) == {'fused temporal route (tamgcn_tconv_bwd)', 'per-branch fallback', 'tamgcn_wgrad_pair', 'two-launch route'}, seen
    assert 'ms 64 k3k5' in seen['per-branch fallback']           # unequal kernel sizes: ops.tconv_supported is false
    assert 'ms 64->128 s2 rk1' in seen['two-launch route']       # stride 2: no paired launch
    # the temporal branches' weight gradient: per branch where ops.tconv_wgrad_pays is false (16-channel branches at V = 20),
    # one launch where it pays (32-channel branches at V = 25)
    assert not any('tamgcn_tconv_wgrad' in n for n in SEEN['ms 64 k5 nores']) and all('tamgcn_tconv_bwd' in n for n in SEEN['ms 64 k5 nores'])
    assert all('tamgcn_tconv_wgrad' in n for n in SEEN['ms 128 v25 s2 nores'])
    assert any('tamgcn_conv_pair' in n for n in SEEN['ms 64 k5 identity'])
