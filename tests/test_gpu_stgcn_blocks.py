"""-m gpu: every ST-GCN training block on the HIP path, ALONE, against a teacher-forced fp64 reference at fp32-rounding bars --
the layer tests/test_gpu_blocks.py is for CTR-GCN.  functional.StGcnFn is a hand-written forward and backward that drives the
CTRGC kernels with alpha = 0 and R = 4, ctrgc_bwd_de for dA alone, the k x 1 data gradient with up = stride, a ReLU mask and
fused BatchNorm moments, add_act_bwd with and without the tail, part[2:4] for the residual BatchNorm, an ostride write into a
zeroed buffer and two element counts when the block strides: this file is what catches a wrong COMPOSITION of right kernels.

Cases, teachers, bars and verify() are tests/stgcn_block_ref.py (tests/test_stgcn_blocks_cpu.py shows the bars bite):
three ten-block models (V = 20, 25 and the run-time-V route at 18; T 13/7/4, 20/10/5, 18/9/5), in both arithmetic modes, with
BatchNorm in train AND eval mode; eight isolated blocks with temporal kernels 1, 3, 5 and 9, T below the kernel width, T = 1
and T2 = 1; and the forms of the node (no tail, no dx, no dA, run twice).  Output, dx, d(A * importance), every parameter
gradient and the BatchNorm buffers after the forward are judged.  -s prints one line per block with err / bar of every
quantity; profiles/stgcn_block_bars.txt holds one full run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import stgcn_block_ref as R                                                     # noqa: E402
from cases import tag_seed                                                      # noqa: E402
from params import fill_state_                                                  # noqa: E402
from tam_gcn_amd import functional as Fn                                        # noqa: E402

DEV = torch.device('cuda:0')
MODES = pytest.mark.parametrize('mode', [1, 0], ids=['split_bf16_bwd', 'exact_f32'])


def _f32(t):
    return t.detach().float().to(DEV).contiguous()


def _params(blk, tail=True):
    p = [blk.gcn.conv.weight, blk.gcn.conv.bias, blk.tcn[0].weight, blk.tcn[0].bias, blk.tcn[2].weight, blk.tcn[2].bias,
         blk.tcn[3].weight, blk.tcn[3].bias]
    if tail and blk._rmode == 'conv':
        p += [blk.residual[0].weight, blk.residual[0].bias, blk.residual[1].weight, blk.residual[1].bias]
    return p


def _reset(blk, b):
    """The module's parameters' gradients cleared and its buffers put back to the block's fixture: an earlier train-mode run of the
    same module moved the running statistics, and every teacher starts from the fixture's."""
    for p in blk.parameters():
        p.grad = None
    with torch.no_grad():
        for k, buf in blk.named_buffers():
            buf.copy_(b.sd[k].to(buf.dtype))


def _run(blk, b, t, tail=True, x_grad=True, A_grad=True):
    """One forward + backward of the module at the teacher's input: (y, dx, dAe, {param: grad}, buffers after)."""
    _reset(blk, b)
    x = _f32(t.x).requires_grad_(x_grad)
    Ae = _f32(b.Ae).requires_grad_(A_grad)
    y = blk(x, Ae)[0] if tail else Fn.StGcnFn.run(blk, False, x, Ae, *_params(blk, False))
    y.backward(_f32(b.cot))
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in blk.named_parameters() if tail or not k.startswith('residual.')}
    bufs = {k: v.detach().clone() for k, v in blk.named_buffers() if tail or not k.startswith('residual.')}
    return y.detach(), x.grad, Ae.grad, grads, bufs


def _split_mode(mode):
    from tam_gcn_amd import _lib
    lib = _lib.load()
    prev = lib.tamgcn_get_split_mode()
    lib.tamgcn_set_split_mode(mode)
    return lambda: lib.tamgcn_set_split_mode(prev)


@pytest.fixture(scope='module')
def models():
    return {}


@pytest.mark.parametrize('bn', ['train', 'eval'])
@MODES
@pytest.mark.parametrize('case', list(R.TRACE_CASES))
def test_every_block_teacher_forced(case, mode, bn, models):
    """Each st_gcn_networks[i] of a Model on the fp32 cast of its fp64 teacher input, topology and cotangent.  bn = 'eval': the
    only run of this node's backward on running statistics (the saliency path has kernels of its own)."""
    training = bn == 'train'
    if case not in models:
        models[case] = R.trace(case)[0].to(DEV)
    m = models[case].train(training)
    failures = []
    restore = _split_mode(mode)
    try:
        for i in range(10):
            b, t = R.block(case, i), R.teacher(case, i, training)
            blk = m.st_gcn_networks[i]
            got = _run(blk, b, t)
            if not training:
                assert all(torch.equal(v.cpu(), b.sd[k].to(v.dtype)) for k, v in got[4].items()), f'block {i}: buffers changed in eval mode'
            ratios, misses = R.judge(got[:4] + (got[4] if training else None,), t, mode)
            print(R.line(f'{case} {i} mode {mode} bn {bn} nudges {t.tries} worst {max(ratios.values()):.2g}', ratios))
            failures += [f'block {i} {s}' for s in misses]
    finally:
        restore()
    assert not failures, f'{case} mode {mode} bn {bn}: ' + '; '.join(failures)


def _isolated(tag):
    b = R.block('isolated', tag)
    blk = b.build()
    fill_state_(blk.state_dict(), seed=tag_seed(tag))
    return b, blk.to(DEV).train()


@MODES
@pytest.mark.parametrize('tag', list(R.ISOLATED), ids=[R.iso_id(t) for t in R.ISOLATED])
def test_isolated_block(tag, mode):
    """Train mode.  The first training runs of temporal kernels 1, 3 and 5, of T2 = 1 and of T below the kernel width."""
    b, blk = _isolated(tag)
    t = R.teacher('isolated', tag, True)
    restore = _split_mode(mode)
    try:
        ratios = R.verify(_run(blk, b, t), t, mode)
    finally:
        restore()
    print(R.line(f'isolated {R.iso_id(tag)} mode {mode} bn train nudges {t.tries} worst {max(ratios.values()):.2g}', ratios))


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


@MODES
@pytest.mark.parametrize('tag', [R.FORM_BLOCK, 'k5 64->128 s2'], ids=R.iso_id)
def test_forms_of_the_node(tag, mode):
    """The branches of StGcnFn that depend on what the caller asks for: (a) tail = False against its own teacher; (b) / (c) a
    gradient not asked for leaves every other one bit-equal; (d) nothing in the node depends on the run (no atomics)."""
    b, blk = _isolated(tag)
    restore = _split_mode(mode)
    try:
        # (a) the Dropout form: bn2(conv(relu(bn1(gcn(x))))), no residual, no final ReLU
        t0 = R.teacher('isolated', tag, True, tail=False)
        ratios = R.verify(_run(blk, b, t0, tail=False), t0, mode)
        print(R.line(f'isolated {R.iso_id(tag)} mode {mode} bn train tail 0 nudges {t0.tries} worst {max(ratios.values()):.2g}', ratios))
        t = R.teacher('isolated', tag, True)
        full = _run(blk, b, t)
        # (d) the same run twice: every output, gradient and buffer bit-equal
        again = _run(blk, b, t)
        assert all(_same(u, v) for u, v in zip(full, again)), 'two identical runs differ'
        # (b) no gradient asked for x: dAe and every parameter gradient unchanged
        nox = _run(blk, b, t, x_grad=False)
        assert nox[1] is None and _same(nox[2], full[2]) and _same(nox[3], full[3]) and _same(nox[0], full[0])
        # (c) no gradient asked for A: dx and every parameter gradient unchanged, nothing reaches A
        noa = _run(blk, b, t, A_grad=False)
        assert noa[2] is None and _same(noa[1], full[1]) and _same(noa[3], full[3]) and _same(noa[0], full[0])
    finally:
        restore()
