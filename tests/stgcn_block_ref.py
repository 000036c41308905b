"""Cases, fp64 teachers, bars and verify() of the ST-GCN teacher-forced block tests -- no GPU code.  Shared by
tests/test_gpu_stgcn_blocks.py (the HIP path against the teachers) and tests/test_stgcn_blocks_cpu.py (the bars shown to bite).

Every st_gcn block is judged ALONE: its input is the fp64 oracle activation at that depth (or a seeded input for the isolated
blocks), its upstream gradient the fp64 cotangent, its topology the fp64 product A * importance.  The teacher loop is the one of
tests/test_gpu_blocks.py (its docstring has the conditioning argument): the input is nudged by a seeded 1e-3-relative
perturbation until every ReLU input of the fp64 run is at least MARGIN from zero, so no mask can differ between the teacher and
an fp32 evaluation and max-norm bars at fp32 rounding level apply to every entry.  There is no max-pool in ST-GCN, so only
the ReLU margin applies.

Bars.  bars() starts from the constants of tests/test_gpu_blocks.py and widens a bar to 4 x the error of the fp32 oracle
(ref32: the same evaluation in fp32 torch on the CPU) on the same quantity of the same block where that is larger, capped at
REL_VEC_SPLIT.  The factor 4 allows for the kernels summing in another order than torch's CPU kernels; the widening never looks
at a GPU result."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from cases import COT_SEED, tag_seed
from params import fill_state_, make_input, make_labels
from oracle import stgcn_oracle as SO
from oracle.ctrgcn_oracle import _bn
from tam_gcn_amd.models import stgcn as M
from test_stgcn_oracle import fill_stgcn_, A as A_UCLA
from test_gpu_blocks import _Monitor, MARGIN, MAX_TRIES, REL_Y, REL_G, REL_VEC_SPLIT

_SP = dict(labeling_mode='spatial')


def _margs(num_point, graph):
    return dict(in_channels=3, num_class=4, num_point=num_point, num_person=1, graph=graph, graph_args=_SP)


# tag -> (Model kwargs, x (N, C, T, V, M)); frames per stage 13/7/4, 20/10/5, 18/9/5
TRACE_CASES = {
    'ucla_t13': (_margs(20, 'graph.ucla.Graph'), (2, 3, 13, 20, 1)),
    'ntu25_t20': (_margs(25, 'graph.ntu_rgb_d.Graph'), (4, 3, 20, 25, 1)),
    # the reference has no OpenPose graph: the same oracle code on the product's graph, not pinned to a fixture
    'openpose_t18': (_margs(18, 'tam_gcn_amd.graph.openpose.Graph'), (2, 3, 18, 18, 1)),
}
PINNED = ('ucla_t13', 'ntu25_t20')
PARAM_SEED, X_SEED, LABEL_SEED = 77, 21, 22

# tag -> (temporal kernel, Cin, Cout, stride, residual, frames T); V = 20, N = 2
ISOLATED = {
    'k3 64->64 s1': (3, 64, 64, 1, True, 13),
    'k5 64->128 s2': (5, 64, 128, 2, True, 13),
    'k1 64->128 s2': (1, 64, 128, 2, True, 13),
    'k1 64->64 s1': (1, 64, 64, 1, True, 6),
    'k3 3->64 nores': (3, 3, 64, 1, False, 13),
    'k5 128->128 s1': (5, 128, 128, 1, True, 3),      # T below the kernel width
    'k9 64->64': (9, 64, 64, 1, True, 1),             # one frame
    'k9 64->128 s2': (9, 64, 128, 2, True, 2),        # T2 = 1
}
FORM_BLOCK = 'k9 64->64 s1'                           # the block of the node-form checks, with 'k5 64->128 s2'
_FORM = {FORM_BLOCK: (9, 64, 64, 1, True, 13)}
ISO_N, ISO_V, ISO_X_SEED, ISO_IMP_SEED = 2, 20, 50, 31
# input seed per isolated block, should one have no teacher in MAX_TRIES nudges (none needed so far)
ISO_SEED_OVERRIDE = {}

ZERO_GRAD = 1e-9                                      # an fp64 bias gradient below this is exactly zero in exact arithmetic
MATRICES = ('gcn.conv.weight', 'tcn.2.weight', 'residual.0.weight')
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stgcn_blocks64.npz')


def iso_id(tag):
    return tag.replace('->', '_').replace(' ', '_')


def rmode_of(cin, cout, stride, residual):
    if not residual:
        return 'zero'
    return 'identity' if cin == cout and stride == 1 else 'conv'


class Block:
    """One block's fp64 problem: state-dict (keys as the module's), topology A * importance, input, cotangent."""

    def __init__(self, tag, sd, Ae, x, cot, stride, rmode, build):
        self.tag, self.sd, self.Ae, self.x, self.cot, self.stride, self.rmode, self.build = tag, sd, Ae, x, cot, stride, rmode, build


class Teacher(tuple):
    """(x, y, dx, dAe, {param: grad}, buffers_after, tries); .key = (case, i, training, tail) for the bars' ref32 lookup."""
    x, y, dx, dAe, grads, buffers, tries = (property(lambda s, j=j: s[j]) for j in range(7))


_TRACES, _BLOCKS, _TEACHERS, _REF32 = {}, {}, {}, {}


def trace(case):
    """fp64 oracle run of the whole model, every block boundary, topology and cotangent retained:
    (model, state-dict, [(i, x_in, out, A * importance)])."""
    if case in _TRACES:
        return _TRACES[case]
    margs, shape = TRACE_CASES[case]
    m = M.Model(**margs)
    fill_stgcn_(m.state_dict(), seed=PARAM_SEED)
    sd = {k: (v.detach().clone().double() if v.is_floating_point() else v.clone()) for k, v in m.state_dict().items()}
    for k, v in sd.items():
        if v.is_floating_point() and 'running' not in k and k != 'A':
            v.requires_grad_(True)
    x = make_input(shape, seed=X_SEED).double().requires_grad_(True)
    lab = make_labels(shape[0], margs['num_class'], seed=LABEL_SEED)
    N, C, T, V, Mp = x.shape
    h = _bn(x.permute(0, 4, 3, 1, 2).contiguous().view(N * Mp, V * C, T), sd, 'data_bn', True)        # SO._blocks
    h = h.view(N, Mp, V, C, T).permute(0, 1, 3, 4, 2).contiguous().view(N * Mp, C, T, V)
    rec = []
    for i, (_, stride, res) in enumerate(SO.PLAN):
        xin, Ae = h, sd['A'] * sd[f'edge_importance.{i}']
        xin.retain_grad(); Ae.retain_grad()
        h = SO.st_gcn(xin, sd, f'st_gcn_networks.{i}', Ae, stride, res, True)
        h.retain_grad()
        rec.append((i, xin, h, Ae))
    logits = F.conv2d(F.avg_pool2d(h, h.size()[2:]).view(N, Mp, -1, 1, 1).mean(dim=1), sd['fcn.weight'], sd['fcn.bias']).view(N, -1)
    loss = F.cross_entropy(logits, lab)
    loss.backward()
    if case in PINNED:                               # the teacher is the reference: its own fp64 run, stored as fixtures
        gold = np.load(GOLD)
        assert np.abs(logits.detach().numpy() - gold[f'{case}/logits_train64']).max() <= 1e-9
        assert abs(float(loss.detach()) - float(gold[f'{case}/loss64'])) <= 1e-10
        assert np.abs(x.grad.numpy() - gold[f'{case}/dx64']).max() <= 1e-9 * max(1.0, np.abs(gold[f'{case}/dx64']).max())
    with torch.no_grad():                            # the traced run moved the running statistics: the blocks start from the fixture's
        ref = m.state_dict()
        for k, v in sd.items():
            if 'running' in k or k.endswith('num_batches_tracked'):
                v.copy_(ref[k])
    _TRACES[case] = (m, sd, rec)
    return _TRACES[case]


def _isolated(tag):
    kt, cin, cout, stride, residual, T = ISOLATED[tag] if tag in ISOLATED else _FORM[tag]
    build = lambda: M.st_gcn(cin, cout, (kt, 3), stride, residual=residual)      # noqa: E731
    blk = build()
    fill_state_(blk.state_dict(), seed=tag_seed(tag))
    sd = {k: (v.detach().clone().double() if v.is_floating_point() else v.clone()) for k, v in blk.state_dict().items()}
    Ae = (A_UCLA * (1 + 0.1 * make_input((3, ISO_V, ISO_V), seed=ISO_IMP_SEED))).double()
    x = make_input((ISO_N, cin, T, ISO_V), ISO_SEED_OVERRIDE.get(tag, ISO_X_SEED)).double()
    T2 = (T - 1) // stride + 1
    cot = make_input((ISO_N, cout, T2, ISO_V), seed=COT_SEED).double()
    return Block(tag, sd, Ae, x, cot, stride, rmode_of(cin, cout, stride, residual), build)


def block(case, i):
    """The fp64 problem of block i of a trace case, or of the isolated block i (a tag) for case 'isolated'."""
    if (case, i) not in _BLOCKS:
        if case == 'isolated':
            _BLOCKS[(case, i)] = _isolated(i)
        else:
            m, sd, rec = trace(case)
            _, xin, hout, Ae = rec[i]
            pfx = f'st_gcn_networks.{i}.'
            bsd = {k[len(pfx):]: v.detach().clone() for k, v in sd.items() if k.startswith(pfx)}
            _BLOCKS[(case, i)] = Block(f'{case}[{i}]', bsd, Ae.detach().clone(), xin.detach().clone(), hout.grad.detach().clone(),
                                       SO.PLAN[i][1], SO.PLAN[i][2], None)
    return _BLOCKS[(case, i)]


def forward(x, sd, Ae, stride, rmode, training, tail=True):
    """The oracle's block; tail False: bn2(conv(relu(bn1(gcn(x))))) -- no residual, no final ReLU (st_gcn with an active Dropout)."""
    sd = {'m.' + k: v for k, v in sd.items()}
    if tail:
        return SO.st_gcn(x, sd, 'm', Ae, stride, rmode, training)
    y = torch.relu(_bn(SO.conv_temporal_graphical(x, sd, 'm.gcn', Ae), sd, 'm.tcn.0', training))
    w = sd['m.tcn.2.weight']
    y = F.conv2d(y, w, sd['m.tcn.2.bias'], stride=(stride, 1), padding=((w.shape[2] - 1) // 2, 0))
    return _bn(y, sd, 'm.tcn.3', training)


def evaluate(b, x, training, tail, dtype=torch.float64, fwd=forward):
    """One forward + backward of block b at input x in `dtype`: (y, dx, dAe, {param: grad}, buffers_after)."""
    sd = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in b.sd.items()}
    for k, v in sd.items():
        if v.is_floating_point() and 'running' not in k and (tail or not k.startswith('residual.')):
            v.requires_grad_(True)
    x = x.detach().clone().to(dtype).requires_grad_(True)
    Ae = b.Ae.detach().clone().to(dtype).requires_grad_(True)
    y = fwd(x, sd, Ae, b.stride, b.rmode, training, tail)
    y.backward(b.cot.to(dtype))
    grads = {k: v.grad for k, v in sd.items() if v.requires_grad}
    bufs = {k: v.detach() for k, v in sd.items() if not v.requires_grad and (tail or not k.startswith('residual.'))}
    return y.detach(), x.grad, Ae.grad, grads, bufs


def teacher(case, i, training, tail=True):
    """Well-conditioned fp64 teacher of a block: Teacher(x, y, dx, dAe, {param: grad}, buffers_after, tries)."""
    key = (case, i, bool(training), bool(tail))
    if key in _TEACHERS:
        return _TEACHERS[key]
    b = block(case, i)
    scale = float(b.x.abs().max())
    salt = tag_seed(b.tag) if case == 'isolated' else 100 * i
    for t in range(MAX_TRIES):
        x = b.x if t == 0 else b.x + 1e-3 * scale * make_input(tuple(b.x.shape), seed=9000 + salt + t).double()
        sd = {k: v.detach().clone() for k, v in b.sd.items()}
        with torch.no_grad(), _Monitor() as mon:
            forward(x, sd, b.Ae, b.stride, b.rmode, training, tail)
        if mon.relu_min >= MARGIN:
            break
    else:
        raise AssertionError(f'{b.tag}: no teacher with ReLU margin >= {MARGIN} in {MAX_TRIES} tries')
    out = Teacher((x.detach(),) + evaluate(b, x, training, tail) + (t,))
    out.key = key
    _TEACHERS[key] = out
    return out


def ref32(case, i, training, tail=True):
    """The same evaluation, at the teacher's input, in fp32 torch on the CPU: the reference's own rounding error."""
    key = (case, i, bool(training), bool(tail))
    if key not in _REF32:
        t = teacher(case, i, training, tail)
        out = Teacher((t.x.float(),) + evaluate(block(case, i), t.x, training, tail, torch.float32) + (t.tries,))
        out.key = key
        _REF32[key] = out
    return _REF32[key]


def quantities(t):
    """{name: tensor} of everything verify() judges: y, dx, dAe, grad/<param>, buf/<buffer>."""
    q = {'y': t[1], 'dx': t[2], 'dAe': t[3]}
    q.update({'grad/' + k: v for k, v in t[4].items()})
    if t[5] is not None:
        q.update({'buf/' + k: v for k, v in t[5].items()})
    return q


def _relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, f'{tuple(a.shape)} vs {tuple(b.shape)}'
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def bars(mode, quantity, ref32_err):
    """The relative (to max|ref|) max-abs bar of a quantity in arithmetic mode 0 (exact fp32 GEMMs) or 1 (bf16-split backward)."""
    if quantity == 'y' or quantity.startswith('buf/'):
        base = REL_Y
    elif quantity in ('dx', 'dAe') or quantity[len('grad/'):] in MATRICES:
        base = REL_G[mode]
    else:                                             # per-channel vectors: BatchNorm gamma / beta, conv biases
        base = REL_G[0] if mode == 0 else REL_VEC_SPLIT
    return min(max(base, 4 * ref32_err), REL_VEC_SPLIT)


def _zero_bias(q, ref):
    return q.endswith('bias') and float(ref.abs().max()) < ZERO_GRAD


def ref32_errors(t):
    """{quantity: relative error of the fp32 oracle}, the quantities under a relative bar only."""
    tq, rq = quantities(t), quantities(ref32(*t.key))
    return {q: _relerr(rq[q], tq[q]) for q in tq if not q.endswith('num_batches_tracked') and not _zero_bias(q, tq[q])}


def verify(got, t, mode):
    """got: (y, dx, dAe, {param: grad}, buffers or None) of an evaluation at the teacher's input.  Returns {quantity: err / bar}
    (buffers None: not judged); raises with the full list of misses, not at the first one."""
    ratios, misses = judge(got, t, mode)
    if misses:
        raise AssertionError(f'{t.key} mode {mode}: ' + '; '.join(misses))
    return ratios


def judge(got, t, mode):
    """verify() without the raise: ({quantity: err / bar}, [misses])."""
    tq, gq = quantities(t), quantities((None,) + tuple(got))
    r32 = ref32_errors(t)
    ratios, misses = {}, []
    for q, ref in tq.items():
        if q.startswith('buf/') and got[4] is None:
            continue
        g = gq.get(q)
        if g is None:
            misses.append(f'{q}: missing')
            continue
        if q.endswith('num_batches_tracked'):
            ratios[q] = 0.0 if int(g) == int(ref) else float('inf')
        elif _zero_bias(q, ref):
            # bias of a conv that feeds a train-mode BatchNorm: exactly zero in exact arithmetic
            wq = q[:-4] + 'weight'
            scale = float(tq[wq].abs().max()) if wq in tq else 1.0
            ratios[q] = float(g.detach().abs().max()) / (1e-4 * max(scale, 1e-3))
        else:
            ratios[q] = _relerr(g, ref) / bars(mode, q, r32[q])
        if not ratios[q] <= 1.0:
            misses.append(f'{q}: err/bar {ratios[q]:.3g}')
    return ratios, misses


def line(head, ratios):
    return head + ' | ' + ' '.join(f'{q}={r:.2g}' for q, r in ratios.items())
