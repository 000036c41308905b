"""CPU: the bars of tests/stgcn_block_ref.py shown to bite, before anyone trusts a green tests/test_gpu_stgcn_blocks.py.

  * the fp32 oracle (ref32) is inside every bar, for every (case, block, train / eval) and every isolated block, both modes;
  * six subtly wrong evaluations of a block, each in fp64 so that only the planted error is present, FAIL verify() -- on every
    block the error can occur in, the block where it is smallest named with -s;
  * the fp64 trace of the two cases the reference has a graph for matches the reference's own fp64 run (tests/golden/
    stgcn_blocks64.npz), the pin the GPU test's teachers stand on."""
import pytest
import torch
import torch.nn.functional as F

import stgcn_block_ref as R
from oracle.ctrgcn_oracle import BN_EPS, BN_MOMENTUM

ALL_BLOCKS = [(c, i) for c in R.TRACE_CASES for i in range(10)] + [('isolated', t) for t in R.ISOLATED]


@pytest.mark.parametrize('case', R.PINNED)
def test_trace_matches_the_reference_fp64_run(case):
    R.trace(case)                                    # asserts logits 1e-9, loss 1e-10, dx 1e-9 * max(1, max|dx|)


@pytest.mark.parametrize('case', list(R.TRACE_CASES) + ['isolated'])
def test_fp32_oracle_is_inside_every_bar(case):
    blocks = [(i, tr, True) for i in range(10) for tr in (True, False)] if case != 'isolated' else \
        [(t, True, tail) for t in list(R.ISOLATED) + [R.FORM_BLOCK] for tail in (True, False)]
    for i, training, tail in blocks:
        t = R.teacher(case, i, training, tail)
        for mode in (1, 0):
            ratios = R.verify(R.ref32(case, i, training, tail)[1:6], t, mode)
            # bar >= 4 x the fp32 oracle's own error on everything under a relative bar, so these sit at or below 0.25
            print(R.line(f'{case} {i} mode {mode} bn {"train" if training else "eval"} tail {int(tail)} nudges {t.tries} worst {max(ratios.values()):.2g}', ratios))


# ---------------------------------------------------------------------------------------------------------------------
# the block once more, from plain tensor arithmetic, with a switch for each planted error
# ---------------------------------------------------------------------------------------------------------------------
class _ResConvLate(torch.autograd.Function):
    """The strided 1 x 1 residual convolution whose data gradient lands one frame late (frames s*t2 + 1)."""

    @staticmethod
    def forward(ctx, x, w, b, s):
        ctx.save_for_backward(x, w)
        ctx.s = s
        return F.conv2d(x, w, b, stride=(s, 1))

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        s, T, T2 = ctx.s, x.shape[2], dy.shape[2]
        g = torch.einsum('oc,notv->nctv', w[:, :, 0, 0], dy)
        dx = torch.zeros_like(x)
        idx = torch.arange(T2) * s + 1
        dx[:, :, idx[idx < T]] = g[:, :, idx < T]
        dw = torch.einsum('notv,nctv->oc', dy, x[:, :, ::s][:, :, :T2]).reshape(w.shape)
        return dx, dw, dy.sum((0, 2, 3)), None


def _bn(x, sd, pfx, training, eps=BN_EPS, biased=False, bwd_cnt=None):
    g, b = sd[pfx + '.weight'].view(1, -1, 1, 1), sd[pfx + '.bias'].view(1, -1, 1, 1)
    rm, rv = sd[pfx + '.running_mean'], sd[pfx + '.running_var']
    if not training:
        return (x - rm.view(1, -1, 1, 1)) * (rv.view(1, -1, 1, 1) + eps).rsqrt() * g + b
    n = x.numel() // x.shape[1]
    mean, var = x.mean((0, 2, 3), keepdim=True), x.var((0, 2, 3), unbiased=False, keepdim=True)
    with torch.no_grad():
        rm.mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * mean.flatten())
        rv.mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * var.flatten() * (1.0 if biased else n / (n - 1)))
        sd[pfx + '.num_batches_tracked'] += 1
    if bwd_cnt is None:
        return (x - mean) * (var + eps).rsqrt() * g + b
    # dx = g * istd * (dy' - sum(dy') / cnt - xh * sum(dy' * xh) / cnt), dy' = the gradient at xh: mean and istd held constant,
    # the two projections written out with the planted count
    istd = (var + eps).rsqrt().detach()
    xh = (x - mean.detach()) * istd
    proj = _Projected.apply(xh, bwd_cnt)
    return proj * g + b


class _Projected(torch.autograd.Function):
    """Identity on the normalised activation whose backward is BatchNorm's two projections with the count `cnt`."""

    @staticmethod
    def forward(ctx, xh, cnt):
        ctx.save_for_backward(xh)
        ctx.cnt = cnt
        return xh.clone()

    @staticmethod
    def backward(ctx, d):
        xh, = ctx.saved_tensors
        return d - d.sum((0, 2, 3), keepdim=True) / ctx.cnt - xh * (d * xh).sum((0, 2, 3), keepdim=True) / ctx.cnt, None


def _mutable(mut):
    def fwd(x, sd, Ae, stride, rmode, training, tail):
        assert tail
        N, _, T, V = x.shape
        K = Ae.size(0)
        wrong_cnt = N * T * V if mut == 'bn_count' else None
        if rmode == 'zero':
            res = 0
        elif rmode == 'identity':
            res = x
        else:
            w, b = sd['residual.0.weight'], sd['residual.0.bias']
            r = _ResConvLate.apply(x, w, b, stride) if mut == 'res_late' else F.conv2d(x, w, b, stride=(stride, 1))
            res = _bn(r, sd, 'residual.1', training, biased=mut == 'biased_var:residual.1', bwd_cnt=wrong_cnt)
        h = F.conv2d(x, sd['gcn.conv.weight'], sd['gcn.conv.bias'])
        h = h.view(N, K, h.shape[1] // K, T, V)
        if mut == 'dA_frame':                        # the last frame's products never reach dAe
            y = torch.cat([torch.einsum('nkctv,kvw->nctw', h[:, :, :, :-1], Ae), torch.einsum('nkctv,kvw->nctw', h[:, :, :, -1:], Ae.detach())], 2)
        else:
            y = torch.einsum('nkctv,kvw->nctw', h, Ae)
        y = torch.relu(_bn(y, sd, 'tcn.0', training, eps=1e-4 if mut == 'bn1_eps' else BN_EPS, biased=mut == 'biased_var:tcn.0'))
        w = sd['tcn.2.weight']
        pad = (w.shape[2] - 1) // 2
        z = F.conv2d(y, w, sd['tcn.2.bias'], stride=(stride, 1), padding=(pad, 0))
        if mut == 'last_tap':
            # T odd, stride 2: the last output frame is centred on input frame T - 1 and every later tap reads padding, so the
            # last tap that reads data there is the centre one: the frame loop's bound off by one (t_in < T - 1)
            assert stride == 2 and T % 2 == 1
            z = torch.cat([z[:, :, :-1], (z[:, :, -1] - torch.einsum('oc,ncv->nov', w[:, :, pad, 0], y[:, :, T - 1])).unsqueeze(2)], 2)
        z = _bn(z, sd, 'tcn.3', training, biased=mut == 'biased_var:tcn.3', bwd_cnt=wrong_cnt)
        return torch.relu(z + res)
    return fwd


def _applies(mut, case, i):
    b = R.block(case, i)
    T = b.x.shape[2]
    if mut in ('bn_count', 'res_late'):
        return b.stride == 2
    if mut == 'last_tap':
        return b.stride == 2 and T % 2 == 1
    if mut == 'dA_frame':
        return T > 1                                 # with one frame there is no dAe left at all
    if mut == 'biased_var:residual.1':
        return b.rmode == 'conv'
    return True


def test_the_plain_restatement_is_the_oracle():
    """No switch set: the restatement the mutants are planted in reproduces every teacher to fp64 rounding."""
    for case, i in ALL_BLOCKS:
        for training in (True, False) if case != 'isolated' else (True,):
            t = R.teacher(case, i, training)
            ratios = R.verify(R.evaluate(R.block(case, i), t.x, training, True, fwd=_mutable(None)), t, 0)
            assert max(ratios.values()) <= 1e-4, (case, i, training, ratios)


MUTANTS = ['bn_count', 'biased_var:tcn.0', 'biased_var:tcn.3', 'biased_var:residual.1', 'dA_frame', 'last_tap', 'bn1_eps', 'res_late']


@pytest.mark.parametrize('mut', MUTANTS)
def test_a_subtly_wrong_block_fails(mut):
    """1 bn_count: a stride-2 block's second and residual BatchNorm backward normalised by N*T*V instead of N*T2*V;
    2 biased_var:<bn>: running_var updated with the biased variance (each of the block's BatchNorms in turn);
    3 dA_frame: dAe accumulated over all frames but the last;  4 last_tap: see the comment in _mutable;
    5 bn1_eps: tcn.0 eps 1e-4 instead of 1e-5;  6 res_late: the residual's strided data gradient written one frame late.
    Judged in the split mode's bars, the wider ones, on EVERY block the error can occur in."""
    weakest, escaped, below = None, [], []
    for case, i in ALL_BLOCKS:
        if not _applies(mut, case, i):
            continue
        t = R.teacher(case, i, True)
        ratios, misses = R.judge(R.evaluate(R.block(case, i), t.x, True, True, fwd=_mutable(mut)), t, 1)
        q = max(ratios, key=ratios.get)
        if not misses and mut == 'bn1_eps' and _eps_size(case, i) < EPS_VISIBLE:
            below.append(f'{case} {i}: size {_eps_size(case, i):.2g}, worst {q} at {ratios[q]:.3g} of its bar')
            continue
        if not misses:
            escaped.append(f'{case} {i}: worst {q} at {ratios[q]:.3g} of its bar')
        if weakest is None or ratios[q] < weakest[0]:
            weakest = (ratios[q], case, i, q)
    assert weakest is not None
    print(f'mutant {mut}: smallest on {weakest[1]} {weakest[2]}, caught by {weakest[3]} at {weakest[0]:.3g} x its bar')
    for b in below:
        print(f'mutant {mut}: below what fp32 bars on a block\'s outputs can see -- {b}')
    assert not escaped, f'mutant {mut} passes verify: ' + '; '.join(escaped)


# bn1_eps is the one planted error that is not caught on every block, and no bar is loose for it.  eps 1e-4 for 1e-5 scales
# channel c of bn1's output by sqrt((var_c + 1e-5) / (var_c + 1e-4)) = 1 - 4.5e-5 / var_c: at its SOURCE the error is 1.5e-5 to
# 9e-5, 3 to 18 x REL_Y.  ReLU is positively homogeneous and the train-mode BatchNorm behind the temporal convolution removes
# whatever part of that rescale its output channels share, so only the spread of 4.5e-5 / var_c over the channels (and beta,
# which is not rescaled) reaches y.  Where the gcn output's variance is 1.6 or more in every channel (blocks 4, 6, 7, 9 of the
# three models, whose input is a sum of two normalised branches) that remainder is 0.2-0.5 of REL_Y on y and 0.7-0.97 of it on
# tcn.3.running_mean: fp32 rounding level, which no test of a block's outputs at fp32 bars can tell from rounding.  The
# assertion therefore holds the mutant to every block where its size at the source is at least an order above the bar it has to
# cross behind that BatchNorm, 10 x REL_Y; the others are printed.
EPS_VISIBLE = 10 * R.REL_Y


def _eps_size(case, i):
    b, t = R.block(case, i), R.teacher(case, i, True)
    N, _, T, V = t.x.shape
    h = F.conv2d(t.x, b.sd['gcn.conv.weight'], b.sd['gcn.conv.bias']).view(N, b.Ae.size(0), -1, T, V)
    var = torch.einsum('nkctv,kvw->nctw', h, b.Ae).var((0, 2, 3), unbiased=False)
    return float(4.5e-5 / var.min())
