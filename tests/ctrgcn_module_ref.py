"""Cases, fp64 teachers, bars, judge() and verify() of the teacher-forced tests of the stand-alone CTR-GCN modules -- no GPU code.
Shared by tests/test_gpu_ctrgcn_modules.py (the HIP path against the teachers) and tests/test_ctrgcn_modules_cpu.py (the bars
shown to bite, the cases shown to meet their conditions).  The layer tests/stgcn_block_ref.py is for ST-GCN, here for everything of
tam_gcn_amd/models/ctrgcn.py a caller can construct alone: CTRGC, unit_gcn, TemporalConv, unit_tcn, MultiScale_TemporalConv
(and TCN_GCN_unit, for the forms of its node only: tests/test_gpu_blocks.py pins its arithmetic).

Teachers.  oracle/ctrgcn_oracle.py in float64 on the module's seeded state (fill_state_ with tag_seed), a seeded input and a
seeded cotangent: output, dx, every parameter gradient, the BatchNorm buffers after the forward, and dA / dalpha for CTRGC.  The
conditioning loop is the one of tests/test_gpu_blocks.py (its docstring has the argument): the input is nudged by seeded
1e-3-relative perturbations until every ReLU input and every max-pool runner-up of the fp64 run is at least MARGIN away, so no
mask can differ between the teacher and any fp32 evaluation and max-norm bars apply to every entry.  A case that found no
teacher in MAX_TRIES would get another input seed in SEED_OVERRIDE, never a wider margin.

Bars.  bars() starts from the constants of tests/test_gpu_blocks.py -- REL_Y for outputs and buffers, REL_G[mode] for dx, dA and
weight matrices, REL_G[0] / REL_VEC_SPLIT for per-channel vectors, REL_SCALAR for the one-element alpha, REL_SCALE_INV for the
gamma of the max-pool branch's entry BatchNorm in train mode -- and widens a bar to 4 x the error of the fp32 oracle (ref32: the same
evaluation in fp32 torch on the CPU) on the same quantity of the same case where that is larger, the widening capped at
REL_VEC_SPLIT.  It never looks at a GPU result.  The bias of a convolution in front of a train-mode BatchNorm keeps the
exactly-zero rule.

A wrong small term must not hide.  share() is max|dx - dx without the term| / max|dx| in fp64 for the additive terms of dx
that a max-norm bar could swallow (CTRGC's p / q path, the residual paths); share_terms() names the terms of each case and the
CPU test holds each to >= SHARE_FACTOR x the case's dx bar in the looser mode.  SCALE rescales seeded parameters where a share
would otherwise be too small.

restated() is the same arithmetic once more from the oracle's primitives with a switch per detached path (for share()) and per
planted fault (for the CPU test); with no switch it reproduces the teachers to fp64 rounding, which the CPU test asserts."""
import numpy as np
import torch
import torch.nn.functional as F

from cases import COT_SEED, NEEDS_A, tag_seed
from params import fill_state_, make_input
from helpers import oracle_run
from oracle import ctrgcn_oracle as O
from tam_gcn_amd.graph import ucla, ntu_rgb_d, coco
from tam_gcn_amd.models import ctrgcn as M
from test_gpu_blocks import _Monitor, MARGIN, MAX_TRIES, REL_Y, REL_G, REL_VEC_SPLIT, REL_SCALAR, REL_SCALE_INV

A_BY_V = {20: ucla.Graph().A, 25: ntu_rgb_d.Graph().A, 17: coco.Graph().A}     # the fused, stream and vgen CTRGC routes
X_SEED, A_SEED = 50, 5
SEED_OVERRIDE = {}                                    # input seed per case, should one have no teacher in MAX_TRIES nudges (none needed)
ZERO_GRAD = 1e-9                                      # an fp64 bias gradient below this is exactly zero in exact arithmetic
SHARE_FACTOR = 100


def _ms(cin, cout, **kw):
    return dict(in_channels=cin, out_channels=cout, **kw)


# tag -> (kind, constructor kwargs, x shape (N, C, T, V), options).  Options: A / alpha of a CTRGC call ('tensor' | None, 'tensor' |
# float), partner = the adaptive=True case whose seeded state and PA an adaptive=False case shares.
CASES = {
    # CTRGC: graph subset 1 + noise as A, alpha 0.6 (tests/helpers.ctrgc_extras)
    'ctrgc 3->64 v20': ('CTRGC', _ms(3, 64), (2, 3, 8, 20), {}),
    'ctrgc 64->64 v20': ('CTRGC', _ms(64, 64), (2, 64, 13, 20), {}),
    'ctrgc 64->128 v25': ('CTRGC', _ms(64, 128), (2, 64, 6, 25), {}),
    'ctrgc 64->64 v17': ('CTRGC', _ms(64, 64), (2, 64, 7, 17), {}),
    'ctrgc 64->64 v20 noA': ('CTRGC', _ms(64, 64), (2, 64, 8, 20), dict(A=None, alpha=0.6)),
    'ctrgc 64->64 v20 t1': ('CTRGC', _ms(64, 64), (2, 64, 1, 20), {}),
    # unit_gcn: residual conv / identity / zero; adaptive=False on the PA of its partner
    'gcn 3->64 v20': ('unit_gcn', _ms(3, 64), (2, 3, 13, 20), {}),
    'gcn 64->128 v25': ('unit_gcn', _ms(64, 128), (2, 64, 6, 25), {}),
    'gcn 64->64 v20': ('unit_gcn', _ms(64, 64), (2, 64, 13, 20), {}),
    'gcn 64->64 v17': ('unit_gcn', _ms(64, 64), (2, 64, 7, 17), {}),
    'gcn 64->64 v20 zero': ('unit_gcn', _ms(64, 64, residual=False), (2, 64, 7, 20), {}),
    'gcn 64->64 v20 fixedA': ('unit_gcn', _ms(64, 64, adaptive=False), (2, 64, 13, 20), dict(partner='gcn 64->64 v20')),
    # TemporalConv / unit_tcn
    'utcn 64->128 k1 s2': ('unit_tcn', _ms(64, 128, kernel_size=1, stride=2), (2, 64, 13, 20), {}),      # ostride write into a zeroed dx
    'tconv 32 k5 s2 d2': ('TemporalConv', _ms(32, 32, kernel_size=5, stride=2, dilation=2), (2, 32, 13, 20), {}),
    'utcn 64 k9 s1': ('unit_tcn', _ms(64, 64, kernel_size=9, stride=1), (2, 64, 12, 20), {}),
    'tconv 32 k5 t3': ('TemporalConv', _ms(32, 32, kernel_size=5, stride=1, dilation=1), (2, 32, 3, 20), {}),   # T below the kernel width
    'utcn 64 k9 t1': ('unit_tcn', _ms(64, 64, kernel_size=9, stride=1), (2, 64, 1, 20), {}),             # one frame
    'utcn 64->128 k9 s2 t2': ('unit_tcn', _ms(64, 128, kernel_size=9, stride=2), (2, 64, 2, 20), {}),    # T_out = 1
    # MultiScale_TemporalConv
    'ms 64 k5 nores': ('MultiScale_TemporalConv', _ms(64, 64, kernel_size=5, dilations=[1, 2], residual=False), (2, 64, 13, 20), {}),
    'ms 64 k5 identity': ('MultiScale_TemporalConv', _ms(64, 64, kernel_size=5, dilations=[1, 2]), (2, 64, 13, 20), {}),
    'ms 64->128 s2 rk1': ('MultiScale_TemporalConv', _ms(64, 128, kernel_size=5, stride=2, dilations=[1, 2]), (2, 64, 13, 20), {}),
    'ms 64->128 s2 rk3': ('MultiScale_TemporalConv', _ms(64, 128, kernel_size=5, stride=2, dilations=[1, 2], residual_kernel_size=3),
                          (2, 64, 13, 20), {}),
    'ms 48 defaults': ('MultiScale_TemporalConv', _ms(48, 48), (2, 48, 11, 20), {}),                      # k = 3, dilations [1, 2, 3, 4]
    'ms 64 k3k5': ('MultiScale_TemporalConv', _ms(64, 64, kernel_size=[3, 5], dilations=[1, 2]), (2, 64, 13, 20), {}),   # no fused temporal route
    'ms 64->128 v25 s1': ('MultiScale_TemporalConv', _ms(64, 128, kernel_size=5, dilations=[1, 2]), (2, 64, 9, 25), {}),  # conv residual at stride 1
    'ms 128 v25 s2 nores': ('MultiScale_TemporalConv', _ms(128, 128, kernel_size=5, stride=2, dilations=[1, 2], residual=False),
                            (2, 128, 8, 25), {}),
    # TCN_GCN_unit: only for the forms of its node
    'unit 64->64 s1': ('TCN_GCN_unit', _ms(64, 64, stride=1), (2, 64, 13, 20), {}),
    'unit 64->128 s2': ('TCN_GCN_unit', _ms(64, 128, stride=2), (2, 64, 13, 20), {}),
    'unit 64->64 fixedA': ('TCN_GCN_unit', _ms(64, 64, stride=1, adaptive=False), (2, 64, 13, 20), dict(partner='unit 64->64 s1')),
}

# seeded parameters rescaled after fill_state_ so that a share (below) is not too small: tag -> {parameter: factor}
SCALE = {}


def case_id(tag):
    return tag.replace('->', '_').replace(' ', '_')


def kind_of(tag):
    return CASES[tag][0]


def rmode_of(tag):
    """The residual mode of the case's own residual path ('conv' | 'identity' | 'zero'), None for a kind without one."""
    kind, kw, _, _ = CASES[tag]
    cin, cout, s = kw['in_channels'], kw['out_channels'], kw.get('stride', 1)
    if kind == 'unit_gcn':
        return 'zero' if not kw.get('residual', True) else ('identity' if cin == cout else 'conv')
    if kind in ('MultiScale_TemporalConv', 'TCN_GCN_unit'):
        return 'zero' if not kw.get('residual', True) else ('identity' if cin == cout and s == 1 else 'conv')
    return None


def share_terms(tag):
    """The additive terms of the case's dx that its CPU test holds to SHARE_FACTOR x the dx bar."""
    kind, r = kind_of(tag), rmode_of(tag)
    if kind == 'CTRGC':
        return ('pq',)
    if kind == 'unit_gcn':
        return ('pq', 'down') if r != 'zero' else ('pq',)
    if kind == 'MultiScale_TemporalConv':
        return ('res',) if r != 'zero' else ()
    if kind == 'TCN_GCN_unit':
        return ('pq', 'unit_res') if r != 'zero' else ('pq',)
    return ()


_MODS, _COT, _TEACHERS, _REF32 = {}, {}, {}, {}


def build(tag):
    """A fresh module of the case on the CPU with its seeded state (the GPU test moves it to the device)."""
    kind, kw, shape, opt = CASES[tag]
    kw = dict(kw)
    cls = getattr(M, kind)
    if kind in NEEDS_A:
        cin, cout = kw.pop('in_channels'), kw.pop('out_channels')
        mod = cls(cin, cout, A_BY_V[shape[-1]], **kw)
    else:
        mod = cls(**kw)
    seed_tag = opt.get('partner', tag)
    fill_state_(mod.state_dict(), seed=tag_seed(seed_tag))
    with torch.no_grad():
        for k, f in SCALE.get(seed_tag, {}).items():
            mod.get_parameter(k).mul_(f)
    if 'partner' in opt:                              # adaptive=False: the fixed graph is the partner's PA
        pa = dict(build(opt['partner']).named_parameters())
        for k, p in pa.items():
            if k.endswith('PA'):
                owner = mod.get_submodule(k[:-3]) if '.' in k else mod
                owner.A = p.detach().clone()
    return mod


def module(tag):
    if tag not in _MODS:
        _MODS[tag] = build(tag)
    return _MODS[tag]


def extras(tag, dtype=torch.float64, device='cpu', grad=True):
    """(A, alpha) of a CTRGC call, None for every other kind."""
    kind, _, shape, opt = CASES[tag]
    if kind != 'CTRGC':
        return None
    V = shape[-1]
    A, alpha = opt.get('A', 'tensor'), opt.get('alpha', 'tensor')
    if A == 'tensor':
        A = (torch.from_numpy(A_BY_V[V][1].astype(np.float32)) + 0.05 * make_input((V, V), A_SEED)).to(dtype).to(device).requires_grad_(grad)
    if alpha == 'tensor':
        alpha = torch.tensor([0.6], dtype=dtype, device=device).requires_grad_(grad)
    return A, alpha


def state(tag, dtype):
    """(oracle state-dict with the 'm.' prefix, parameter names, buffer names) of the case in `dtype`."""
    mod = module(tag)
    sd = {'m.' + k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in mod.state_dict().items()}
    for k, sub in mod.named_modules():                # adaptive=False: the fixed graph in the oracle's PA slot, no gradient
        if isinstance(sub, M.unit_gcn) and not sub.adaptive:
            sd['m.' + (k + '.' if k else '') + 'PA'] = sub.A.detach().clone().to(dtype)
    return sd, [k for k, _ in mod.named_parameters()], [k for k, _ in mod.named_buffers()]


def oracle_forward(tag, sd, x, training, ex, **_):
    kind, kw, _, _ = CASES[tag]
    return oracle_run(kind, kw, sd, x, training, ex)


def cot(tag):
    """The seeded cotangent of the case (float32 values, as the input)."""
    if tag not in _COT:
        sd, _, _ = state(tag, torch.float64)
        with torch.no_grad():
            y = oracle_forward(tag, sd, x0(tag), True, extras(tag, grad=False))
        _COT[tag] = make_input(tuple(y.shape), COT_SEED)
    return _COT[tag]


def x0(tag):
    return make_input(CASES[tag][2], SEED_OVERRIDE.get(tag, X_SEED)).double()


def evaluate(tag, x, training, dtype=torch.float64, fwd=oracle_forward, **sw):
    """One forward + backward of the case at input x in `dtype`: {quantity: tensor} with y, dx, dA, dalpha, grad/<parameter>,
    buf/<buffer> (the buffers after the forward)."""
    sd, pnames, bnames = state(tag, dtype)
    for k in pnames:
        sd['m.' + k].requires_grad_(True)
    x = x.detach().clone().to(dtype).requires_grad_(True)
    ex = extras(tag, dtype)
    y = fwd(tag, sd, x, training, ex, **sw)
    y.backward(cot(tag).to(dtype))
    q = {'y': y.detach(), 'dx': x.grad}
    if ex is not None:
        if isinstance(ex[0], torch.Tensor):
            q['dA'] = ex[0].grad
        if isinstance(ex[1], torch.Tensor):
            q['dalpha'] = ex[1].grad
    q.update({'grad/' + k: sd['m.' + k].grad for k in pnames})
    q.update({'buf/' + k: sd['m.' + k].detach() for k in bnames})
    return q


class Teacher:
    """x: the well-conditioned input; q: {quantity: fp64 tensor}; tries: nudges it took; key = (tag, training)."""

    def __init__(self, key, x, q, tries):
        self.key, self.x, self.q, self.tries = key, x, q, tries


def teacher(tag, training):
    key = (tag, bool(training))
    if key in _TEACHERS:
        return _TEACHERS[key]
    base = x0(tag)
    scale = float(base.abs().max())
    ex = extras(tag, grad=False)
    for t in range(MAX_TRIES):
        x = base if t == 0 else base + 1e-3 * scale * make_input(tuple(base.shape), seed=9000 + tag_seed(tag) + t).double()
        sd, _, _ = state(tag, torch.float64)
        with torch.no_grad(), _Monitor() as mon:
            oracle_forward(tag, sd, x, training, ex)
        if mon.relu_min >= MARGIN and mon.pool_gap >= MARGIN:
            break
    else:
        raise AssertionError(f'{tag}: no teacher with ReLU / max-pool margin >= {MARGIN} in {MAX_TRIES} tries')
    _TEACHERS[key] = Teacher(key, x.detach(), evaluate(tag, x, training), t)
    return _TEACHERS[key]


def ref32(tag, training):
    """The same evaluation, at the teacher's input, in fp32 torch on the CPU: the reference's own rounding error."""
    key = (tag, bool(training))
    if key not in _REF32:
        _REF32[key] = evaluate(tag, teacher(tag, training).x, training, torch.float32)
    return _REF32[key]


def _relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, f'{tuple(a.shape)} vs {tuple(b.shape)}'
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _pool_entry_gamma(tag, q, training):
    """grad/<gamma of the BatchNorm in front of the max-pool>, train mode: that branch ends in another train-mode BatchNorm, which
    removes the scale gamma sets (see REL_SCALE_INV).  On running statistics nothing cancels and the vector bar holds."""
    kind, kw, _, _ = CASES[tag]
    if not training or kind not in ('MultiScale_TemporalConv', 'TCN_GCN_unit'):
        return False
    nb = len(kw.get('dilations', [1, 2, 3, 4] if kind == 'MultiScale_TemporalConv' else [1, 2]))
    return q == 'grad/' + ('tcn1.' if kind == 'TCN_GCN_unit' else '') + f'branches.{nb}.1.weight'


def base_bar(tag, mode, quantity, ref, training=True):
    if quantity == 'y' or quantity.startswith('buf/'):
        return REL_Y
    if ref.numel() == 1:                              # alpha: ONE heavily cancelling sum over every (n, s, c, u, v)
        return REL_SCALAR
    if _pool_entry_gamma(tag, quantity, training):
        return REL_SCALE_INV
    if quantity in ('dx', 'dA') or ref.dim() >= 2:    # activations' gradients, the graph, weight matrices
        return REL_G[mode]
    return REL_G[0] if mode == 0 else REL_VEC_SPLIT   # per-channel vectors: BatchNorm gamma / beta, conv biases


def bars(tag, mode, quantity, ref, ref32_err, training=True):
    """The relative (to max|ref|) max-abs bar of a quantity in arithmetic mode 0 (exact fp32 GEMMs) or 1 (bf16-split backward)."""
    return max(base_bar(tag, mode, quantity, ref, training), min(4 * ref32_err, REL_VEC_SPLIT))


def _zero_bias(q, ref):
    return q.endswith('bias') and float(ref.abs().max()) < ZERO_GRAD


def ref32_errors(t):
    """{quantity: relative error of the fp32 oracle}, the quantities under a relative bar only."""
    r = ref32(*t.key)
    return {q: _relerr(r[q], v) for q, v in t.q.items() if not q.endswith('num_batches_tracked') and not _zero_bias(q, v)}


def judge(got, t, mode, buffers=True):
    """got: {quantity: tensor} of an evaluation at the teacher's input.  ({quantity: err / bar}, [misses]); buffers False: the
    BatchNorm buffers are not judged (eval mode: the caller holds them to bit-equality instead)."""
    tag = t.key[0]
    r32 = ref32_errors(t)
    ratios, misses = {}, []
    for q, ref in t.q.items():
        if q.startswith('buf/') and not buffers:
            continue
        g = got.get(q)
        if g is None:
            misses.append(f'{q}: missing')
            continue
        if q.endswith('num_batches_tracked'):
            ratios[q] = 0.0 if int(g) == int(ref) else float('inf')
        elif _zero_bias(q, ref):
            # bias of a conv that feeds a train-mode BatchNorm: exactly zero in exact arithmetic
            wq = q[:-4] + 'weight'
            scale = float(t.q[wq].abs().max()) if wq in t.q else 1.0
            ratios[q] = float(g.detach().abs().max()) / (1e-4 * max(scale, 1e-3))
        else:
            ratios[q] = _relerr(g, ref) / bars(tag, mode, q, ref, r32[q], t.key[1])
        if not ratios[q] <= 1.0:
            misses.append(f'{q}: err/bar {ratios[q]:.3g}')
    return ratios, misses


def verify(got, t, mode, buffers=True):
    """judge() that raises with the full list of misses, not at the first one.  Returns {quantity: err / bar}."""
    ratios, misses = judge(got, t, mode, buffers)
    if misses:
        raise AssertionError(f'{t.key} mode {mode}: ' + '; '.join(misses))
    return ratios


def line(head, ratios):
    return head + ' | ' + ' '.join(f'{q}={r:.2g}' for q, r in ratios.items())


def widened(t, mode):
    """{quantity: (fp32-oracle error, bar)} of the quantities whose bar is above its base constant."""
    tag, out = t.key[0], {}
    for q, e in ref32_errors(t).items():
        b = bars(tag, mode, q, t.q[q], e, t.key[1])
        if b > base_bar(tag, mode, q, t.q[q], t.key[1]):
            out[q] = (e, b)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the modules once more from the oracle's primitives, with a switch per detached path (cut) and per planted fault
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ('pq_scale', 'identity_dropped', 'biased_var', 'res_late', 'dilation')


def _gscale(x, f):
    """x, with the gradient that flows back through it scaled by f."""
    return x.detach() if f == 0.0 else x.detach() * (1 - f) + x * f


class _ConvLate(torch.autograd.Function):
    """A strided k x 1 convolution whose data gradient lands one frame late."""

    @staticmethod
    def forward(ctx, x, w, b, s, pad, d):
        ctx.save_for_backward(x, w)
        ctx.cfg = (s, pad, d)
        return F.conv2d(x, w, b, stride=(s, 1), padding=(pad, 0), dilation=(d, 1))

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        s, pad, d = ctx.cfg
        with torch.enable_grad():
            xx, ww = x.detach().requires_grad_(True), w.detach().requires_grad_(True)
            y = F.conv2d(xx, ww, None, stride=(s, 1), padding=(pad, 0), dilation=(d, 1))
            dx, dw = torch.autograd.grad(y, (xx, ww), dy)
        late = torch.zeros_like(dx)
        late[:, :, 1:] = dx[:, :, :-1]
        return late, dw, dy.sum((0, 2, 3)), None, None, None


def _r_bn(x, sd, pfx, training, fault):
    if not (training and fault == 'biased_var'):
        return O._bn(x, sd, pfx, training)
    rm, rv = sd[pfx + '.running_mean'], sd[pfx + '.running_var']
    rmc, rvc = rm.detach().clone(), rv.detach().clone()
    y = F.batch_norm(x, rmc, rvc, sd[pfx + '.weight'], sd[pfx + '.bias'], training=True, momentum=O.BN_MOMENTUM, eps=O.BN_EPS)
    dims = [i for i in range(x.dim()) if i != 1]
    with torch.no_grad():
        rv.copy_((1 - O.BN_MOMENTUM) * rv + O.BN_MOMENTUM * x.detach().var(dims, unbiased=False))
        rm.copy_(rmc)
        sd[pfx + '.num_batches_tracked'] += 1
    return y


def _r_ctrgc(x, sd, pfx, A, alpha, cut, fault):
    T = x.shape[2]
    f = 0.0 if cut == 'pq' else ((T - 1) / T if fault == 'pq_scale' else 1.0)
    xq = x if f == 1.0 else _gscale(x, f)
    p = O._conv(xq, sd, pfx + '.conv1').mean(-2)
    q = O._conv(xq, sd, pfx + '.conv2').mean(-2)
    x3 = O._conv(x, sd, pfx + '.conv3')
    E = O._conv(torch.tanh(p.unsqueeze(-1) - q.unsqueeze(-2)), sd, pfx + '.conv4') * alpha
    if A is not None:
        E = E + A[None, None]
    return torch.einsum('ncuv,nctv->nctu', E, x3)


def _r_unit_gcn(x, sd, pfx, training, cut, fault, zero=False):
    PA, alpha = sd[pfx + '.PA'], sd[pfx + '.alpha']
    y = None
    for i in range(PA.shape[0]):
        z = _r_ctrgc(x, sd, f'{pfx}.convs.{i}', PA[i], alpha, cut, fault)
        y = z if y is None else z + y
    y = _r_bn(y, sd, pfx + '.bn', training, fault)
    xr = x.detach() if cut == 'down' else x
    if zero:                                          # residual=False: down(x) = 0
        res = None
    elif (pfx + '.down.0.weight') in sd:
        res = _r_bn(O._conv(xr, sd, pfx + '.down.0'), sd, pfx + '.down.1', training, fault)
    else:
        res = xr
    diff = (res - y) if res is not None else (0 - y)
    off = torch.tanh(_r_bn(O._conv(diff, sd, pfx + '.offset_conv.0'), sd, pfx + '.offset_conv.1', training, fault))
    return torch.relu(y + off + res) if res is not None else torch.relu(y + off)


def _r_tconv(x, sd, pfx, k, s, d, training, fault, late=False):
    pad = (k + (k - 1) * (d - 1) - 1) // 2
    if late:
        h = _ConvLate.apply(x, sd[pfx + '.conv.weight'], sd[pfx + '.conv.bias'], s, pad, d)
    else:
        h = O._conv(x, sd, pfx + '.conv', s, pad, d)
    return _r_bn(h, sd, pfx + '.bn', training, fault)


def _r_ms_tcn(x, sd, pfx, ks, s, dils, training, rmode, rk, cut, fault):
    nb = len(dils)
    ks = ks if isinstance(ks, (list, tuple)) else [ks] * nb
    outs = []
    for b, (k, d) in enumerate(zip(ks, dils)):
        h = torch.relu(_r_bn(O._conv(x, sd, f'{pfx}.branches.{b}.0'), sd, f'{pfx}.branches.{b}.1', training, fault))
        if fault == 'dilation' and b == 1:
            d = d + 1                                 # k odd: the padding of d + 1 keeps the output length
        outs.append(_r_tconv(h, sd, f'{pfx}.branches.{b}.3', k, s, d, training, fault))
    h = torch.relu(_r_bn(O._conv(x, sd, f'{pfx}.branches.{nb}.0'), sd, f'{pfx}.branches.{nb}.1', training, fault))
    h = F.max_pool2d(h, kernel_size=(3, 1), stride=(s, 1), padding=(1, 0))
    outs.append(_r_bn(h, sd, f'{pfx}.branches.{nb}.4', training, fault))
    outs.append(_r_bn(O._conv(x, sd, f'{pfx}.branches.{nb + 1}.0', s), sd, f'{pfx}.branches.{nb + 1}.1', training, fault))
    out = torch.cat(outs, dim=1)
    xr = x.detach() if cut == 'res' or (fault == 'identity_dropped' and rmode == 'identity') else x
    if rmode == 'identity':
        out = out + xr
    elif rmode == 'conv':
        out = out + _r_tconv(xr, sd, pfx + '.residual', rk, s, 1, training, fault, late=fault == 'res_late' and s == 2)
    return out


def restated(tag, sd, x, training, ex, cut=None, fault=None):
    kind, kw, _, _ = CASES[tag]
    s = kw.get('stride', 1)
    if kind == 'CTRGC':
        return _r_ctrgc(x, sd, 'm', ex[0], ex[1], cut, fault)
    if kind == 'unit_gcn':
        return _r_unit_gcn(x, sd, 'm', training, cut, fault, zero=rmode_of(tag) == 'zero')
    if kind == 'TemporalConv':
        return _r_tconv(x, sd, 'm', kw['kernel_size'], s, kw.get('dilation', 1), training, fault)
    if kind == 'unit_tcn':
        return _r_tconv(x, sd, 'm', kw.get('kernel_size', 9), s, 1, training, fault)
    if kind == 'MultiScale_TemporalConv':
        return _r_ms_tcn(x, sd, 'm', kw.get('kernel_size', 3), s, kw.get('dilations', [1, 2, 3, 4]), training, rmode_of(tag),
                         kw.get('residual_kernel_size', 1), cut, fault)
    if kind == 'TCN_GCN_unit':
        g = _r_unit_gcn(x, sd, 'm.gcn1', training, cut, fault)
        y = _r_ms_tcn(g, sd, 'm.tcn1', 5, s, [1, 2], training, 'zero', 1, None, fault)
        r, xr = rmode_of(tag), (x.detach() if cut == 'unit_res' else x)
        if r == 'conv':
            y = y + _r_tconv(xr, sd, 'm.residual', 1, s, 1, training, fault, late=fault == 'res_late' and s == 2)
        elif r == 'identity':
            y = y + xr
        return torch.relu(y)
    raise KeyError(kind)


def fault_applies(fault, tag):
    """Whether the planted fault changes anything in the case."""
    kind, kw, shape, _ = CASES[tag]
    if fault == 'pq_scale':
        return kind in ('CTRGC', 'unit_gcn', 'TCN_GCN_unit')      # T = 1: (T - 1) / T = 0, the whole term is lost
    if fault == 'identity_dropped':
        return kind == 'MultiScale_TemporalConv' and rmode_of(tag) == 'identity'
    if fault == 'biased_var':
        return kind != 'CTRGC'                        # train mode only
    if fault == 'res_late':
        return kind in ('MultiScale_TemporalConv', 'TCN_GCN_unit') and rmode_of(tag) == 'conv' and kw.get('stride', 1) == 2
    if fault == 'dilation':
        return kind in ('MultiScale_TemporalConv', 'TCN_GCN_unit')
    raise KeyError(fault)


def share(tag, term, training=True):
    """max|dx - dx with the term's path detached| / max|dx| at the teacher's input, fp64."""
    t = teacher(tag, training)
    dx = t.q['dx']
    cutdx = evaluate(tag, t.x, training, fwd=restated, cut=term)['dx']
    return float((dx - cutdx).abs().max() / dx.abs().max())
