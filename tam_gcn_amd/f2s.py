"""Small-batch eval-mode engine for ST-GCN (models.stgcn.Model): every st_gcn block as TWO launches of the f2s kernel family
(csrc/f2s.hip: tamgcn_f2s_gcn, tamgcn_f2s_tcn; include/tamgcn.h "f2s") instead of the ~10 training-size launches of the
general eval path (functional.StGcnFn: four zero fills, A * importance, its transpose, an E tensor that repeats one matrix for
every sample and channel, the CTRGC forward, the k x 1 conv, the residual conv, add_act).

In eval mode the topology is static and both BatchNorms fold into the neighbouring weights, HERE, once per parameter state
(f2.FusedEval's state key: a cheap version check per call re-folds after an optimiser step, load_state_dict, an in-place
edge_importance update or a train-mode forward):

    gcn   h = relu( sum_k (Wg_k x) Ae_k + bg )      Ae = A * edge_importance;  Wg = s1 * gcn.conv.weight;
                                                     bg[c][w] = s1[c] sum_k b[k Cout + c] sum_v Ae[k][v][w] + t1[c]
                                                     (the conv bias is added BEFORE the joint contraction, so it reaches joint w
                                                     through the column sums of Ae: a (Cout, V) table, not a (Cout) vector)
    tcn   out = relu( Wt * h + bt + res )            Wt = s2 * tcn.2.weight, bt = s2 b + t2;  res = 0 | x | Wr x[::stride] + br

    eng = FusedEvalST(model)          # model.eval(); any graph of 2..32 joints, 1..3 subsets
    logits = eng(x)                   # x (N, C, T, V, M) or (N, T, V*C) on the GPU, under torch.no_grad()

`stgcn.Model.forward` / `extract_feature` route here by themselves in eval mode without autograd for batches of at most
F2S_MAX_FRAMES clip-persons x frames (N * M * T; TAMGCN_F2S_MAX_FRAMES overrides it, TAMGCN_F2=0 switches the routing off;
measured: profiles/f2s_infer_bench.txt).  Limits: temporal kernel 9 only, V <= 32, K <= 3, Cout % 16 == 0.  No CPU path, no
fallback inside: `Unsupported` is raised before anything is launched.

A multi-stream ensemble of G ST-GCN models of one geometry (inference.StreamEnsemble) runs as ONE launch sequence:
`GroupedEvalST` stacks the folded tensors of the G models on a leading group axis and runs the fused stem, ten
tamgcn::st_gcn_eval_grouped (the same two kernels with a group offset on their parameter pointers: tamgcn_f2s_gcn_grouped,
tamgcn_f2s_tcn_grouped; include/tamgcn.h "f2s grouped"), one pool and one grouped fc -- 23 launches whatever G is, bit-equal
per group to that model's own FusedEvalST (measured: profiles/stgcn_ensemble_bench.txt).

The same engine serves gradient saliency (tam_gcn_amd.saliency; reference tools/train_stgcn_group.py:264-356).  In eval mode a
block is piecewise linear in its input with these static folded weights, so its DATA gradient is again two launches
(csrc/f2s_bwd.hip: tamgcn_f2s_tcn_bwd, tamgcn_f2s_gcn_bwd; include/tamgcn.h "f2s backward"), masked by the two ReLUs as the
forward's own h and out record them; no weight gradient is computed and no parameter's .grad is touched:

    tcn_bwd   dh = [h > 0] * ( Wt^T (*) gz ),  gz = gout * [out > 0]       Wtb[c'][c][tap] = Wt[c][c'][tap]
    gcn_bwd   dx = sum_k Wg_k^T (dh Ae_k^T) + res                           Wgb[k][ci][c] = Wg[k][c][ci];  res = 0 | gz | Wrb gz on the
                                                                            frames t % stride == 0,  Wrb[ci][c] = Wr[c][ci]

The transposed operands are folded with the others, under the same state key and re-fold.  `FusedEvalST.saliency_pass` runs
stem, 10 x (gcn, tcn) keeping every (out, h), head, the seed (head_fc_bwd, head_pool_bwd), 10 x (tcn_bwd, gcn_bwd) in reverse
and tamgcn_saliency_joints, all on the current stream without a host synchronisation.  saliency.input_gradient /
joint_saliency route here for inputs of at most F2S_BWD_MAX_FRAMES clip-persons x frames (TAMGCN_F2S_BWD_MAX_FRAMES overrides
it; measured: profiles/f2s_saliency_bench.txt)."""
import ctypes as C
import os
from typing import List, Tuple

import torch
from torch import Tensor

from . import _lib
from . import functional as Fn
from .f2 import FusedEval, GroupedEval, Unsupported, enabled, _affine, _fold, _opt

__all__ = ['FusedEvalST', 'GroupedEvalST', 'Unsupported', 'F2S_MAX_FRAMES', 'F2S_BWD_MAX_FRAMES', 'enabled']

# N*M*T up to which stgcn.Model.forward routes here: the largest measured clip-persons x frames at which the family beats the
# general eval path both eager and under graph replay at every measured joint count (17, 18, 20, 25); it loses at 1200 (25
# joints), 1664 (20) and 2048 (17)  (profiles/f2s_infer_bench.txt)
F2S_MAX_FRAMES = int(os.environ.get('TAMGCN_F2S_MAX_FRAMES', '1024'))
# N*M*T up to which saliency.input_gradient / joint_saliency take the family's forward + backward chain instead of autograd
# through the general path: the largest clip-persons x frames measured at every joint count (17, 20, 25) at which the family's
# median is below the general path's by more than the spread of the alternating repeats at each of them; at 3072 it loses at
# 20 joints  (profiles/f2s_saliency_bench.txt)
F2S_BWD_MAX_FRAMES = int(os.environ.get('TAMGCN_F2S_BWD_MAX_FRAMES', '2048'))
KT = 9                                                                     # the temporal kernel the kernels are built for


class _BlockST:
    """Folded tensors and geometry of one st_gcn block; Ae (K, V, V) = A * edge_importance of that block."""

    def __init__(self, blk, Ae, device):
        conv = blk.gcn.conv
        K, V = int(Ae.shape[0]), int(Ae.shape[-1])
        Cin, Cout = blk.in_channels, blk.out_channels
        tconv = blk.tcn[2]
        kt, stride = int(tconv.kernel_size[0]), int(tconv.stride[0])
        if kt != KT:
            raise Unsupported(f'st_gcn with temporal kernel size {kt} (the f2s kernels are built for {KT})')
        if Cout % 16:
            raise Unsupported(f'st_gcn({Cin}, {Cout}): output channels must be a multiple of 16')
        if V > 32:
            raise Unsupported(f'{V} joints (the f2s kernels serve V <= 32)')
        if K > 3:
            raise Unsupported(f'{K} subsets (the f2s kernels serve K <= 3)')
        if blk.gcn.kernel_size != K or blk.gcn._cfg != (1, 1, 1, 0) or conv.out_channels != K * Cout:
            raise Unsupported('ConvTemporalGraphical other than the 1 x 1 form over the graph\'s subsets')
        if not _lib.load().tamgcn_f2s_supported(V, K, Cin, Cout, kt, stride):
            raise Unsupported(f'st_gcn({Cin}, {Cout}, stride {stride}) on {V} joints, {K} subsets')
        Ae = Ae.detach().to(device=device, dtype=torch.float32)
        s1, t1 = _affine(Fn.BN(blk.tcn[0]))
        w = conv.weight.detach().reshape(K, Cout, Cin)
        b = conv.bias.detach().reshape(K, Cout) if conv.bias is not None else w.new_zeros(K, Cout)
        self.Ae = Ae.contiguous()
        self.Wg = (w * s1[None, :, None]).contiguous()
        self.bg = (s1[:, None] * (b.t() @ Ae.sum(1)) + t1[:, None]).contiguous()             # (Cout, V)
        self.Wt, self.bt = _fold(tconv.weight.reshape(Cout, Cout * kt), tconv.bias, Fn.BN(blk.tcn[3]))
        self.rmode = {'zero': 0, 'identity': 1, 'conv': 2}[blk._rmode]
        self.Wr = self.br = None
        if self.rmode == 2:
            r = blk.residual
            if r[0].kernel_size != (1, 1):
                raise Unsupported('residual conv other than 1 x 1')
            self.Wr, self.br = _fold(r[0].weight.reshape(Cout, Cin), r[0].bias, Fn.BN(r[1]))
        self.Cin, self.Cout, self.K, self.V, self.stride = Cin, Cout, K, V, stride
        none = self.bt.new_empty(0)
        # the registered op's arguments: tensors in this order (an absent one is an empty tensor), geometry as integers
        self.params = [self.Ae, self.Wg, self.bg, self.Wt, self.bt, none if self.Wr is None else self.Wr, none if self.br is None else self.br]
        self.geom = [K, kt, stride, self.rmode]
        # the data gradient's operands (tamgcn::st_gcn_eval_bwd): the same weights with the contraction index innermost
        self.Wtb = self.Wt.view(Cout, Cout, kt).permute(1, 0, 2).contiguous()
        self.Wgb = self.Wg.permute(0, 2, 1).contiguous()
        self.Wrb = None if self.Wr is None else self.Wr.t().contiguous()
        self.bparams = [self.Ae, self.Wgb, self.Wtb, none if self.Wrb is None else self.Wrb]


class FusedEvalST(FusedEval):
    """f2.FusedEval's state key and re-fold on models.stgcn.Model: the blocks are model.st_gcn_networks, the operator is
    tamgcn::st_gcn_eval, the head reads fcn's weight as (num_class, 256)."""
    FAMILY = 'f2s'

    def __init__(self, model):
        if model.training:
            raise ValueError('FusedEvalST: put the model in eval() mode first')
        if not hasattr(model, 'st_gcn_networks') or not hasattr(model, 'edge_importance'):
            raise Unsupported('FusedEvalST serves models.stgcn.Model')
        self.V = model.num_point
        super().__init__(model)

    def _packed(self, device):
        key = self._state_key()
        if self._blocks is None or key != self._key:
            m = self.model
            with torch.no_grad():
                self._blocks = [_BlockST(blk, m.A * imp, device) for blk, imp in zip(m.st_gcn_networks, m.edge_importance)]
            self._key = self._state_key()
        return self._blocks

    def _block(self, b, x, st=None, xpart=None, want_xpart=False):
        return torch.ops.tamgcn.st_gcn_eval(x, b.params, b.geom)

    def blocks(self, x):
        """(N, C, T, V, M) or (N, T, V*C) -> (N*M, 256, T/4, V), N, M   (reference models/stgcn.py:172-189)"""
        m = self.model
        if torch.is_grad_enabled() and any(p.requires_grad for p in m.parameters()):
            raise RuntimeError('FusedEvalST is an inference path: call it under torch.no_grad()')
        if m.training:
            raise RuntimeError('FusedEvalST: the model went back to train() mode')
        if not x.is_cuda or x.dtype != torch.float32:
            raise RuntimeError('FusedEvalST: expected a float32 HIP (cuda) tensor; there is no CPU path')
        if x.dim() == 3:
            N, T, VC = x.shape
            x = x.view(N, T, m.num_point, -1).permute(0, 3, 1, 2).contiguous().unsqueeze(-1)
        N, C_, T, V, M = x.shape
        if V != self.V:
            raise Unsupported(f'{V} joints (the model has {self.V})')
        blocks = self._packed(x.device)
        h = Fn.StemFn.run(m.data_bn, x.contiguous(), m.data_bn.weight, m.data_bn.bias)
        for b in blocks:
            h = self._block(b, h)
        return h, N, M

    def __call__(self, x):
        h, N, M = self.blocks(x)
        m = self.model                                         # eval mode: drop_out is the identity
        return torch.ops.tamgcn.head(h, m.fcn.weight.view(m.fcn.weight.size(0), -1), m.fcn.bias, M)

    forward = __call__

    def saliency_pass(self, x, labels=None, dlogits=None, trace=None, want_dxin=True):
        """(sal (N, V), dxin (N, C, T, V, M) | None, logits (N, K)) for x (N, C, T, V, M): the gradient of sum(dlogits * logits) --
        dlogits (N, K), or one-hot of labels (N) int64, or one-hot of the arg max of the logits (taken on the device) -- with respect
        to x, and its magnitude summed per joint.  trace: a list that receives, per block in forward order, dict(gout, out, h, dx).
        Everything runs on the current stream; nothing synchronises with the host."""
        from . import ops
        m = self.model
        if m.training:
            raise RuntimeError('FusedEvalST: the model went back to train() mode')
        if not x.is_cuda or x.dtype != torch.float32:
            raise RuntimeError('FusedEvalST: expected a float32 HIP (cuda) tensor; there is no CPU path')
        N, C_, T, V, M = x.shape
        if V != self.V:
            raise Unsupported(f'{V} joints (the model has {self.V})')
        with torch.no_grad():
            blocks = self._packed(x.device)
            x = x.contiguous()
            bn = Fn.BN(m.data_bn)
            J = C_ * V * M
            if bn.C != J:
                raise RuntimeError(f'tam_gcn_amd: data_bn has {bn.C} features, input gives {J}')
            coef, _ = Fn._eval_cached(m.data_bn, 'stem', [bn], lambda: Fn._eval_coefs([(bn, 0)], J, x))
            a = ops.stem_apply(x, coef)
            kept = []
            for b in blocks:
                a, h = torch.ops.tamgcn.st_gcn_eval_fwd(a, b.params, b.geom)
                kept.append((a, h))
            W = m.fcn.weight.detach().view(m.fcn.weight.size(0), -1).contiguous()
            pooled = ops.head_pool_fwd(a, M)
            logits = ops.head_fc_fwd(pooled, W, m.fcn.bias.detach().contiguous())
            if dlogits is None:
                lab = logits.argmax(1) if labels is None else labels.to(device=x.device, dtype=torch.int64).view(N)
                dlogits = torch.zeros_like(logits).scatter_(1, lab.view(N, 1), 1.0)
            elif tuple(dlogits.shape) != tuple(logits.shape):
                raise ValueError(f'dlogits must be {tuple(logits.shape)}, got {tuple(dlogits.shape)}')
            dlogits = dlogits.to(device=x.device, dtype=torch.float32).contiguous()
            _, _, dpooled = ops.head_fc_bwd(dlogits, pooled, W)
            g = ops.head_pool_bwd(dpooled, M, a.shape[2], V)
            steps = [None] * len(blocks)
            for i in range(len(blocks) - 1, -1, -1):
                out, h = kept[i]
                dx = torch.ops.tamgcn.st_gcn_eval_bwd(g, out, h, blocks[i].bparams, blocks[i].geom)
                steps[i] = dict(gout=g, out=out, h=h, dx=dx)
                g = dx
            if trace is not None:
                trace.extend(steps)
            sal = torch.empty(N, V, device=x.device)
            dxin = torch.empty_like(x) if want_dxin else None
            _lib.check(_lib.load().tamgcn_saliency_joints(g.data_ptr(), coef.data_ptr(), N, C_, T, V, M, sal.data_ptr(),
                                                       None if dxin is None else dxin.data_ptr(),
                                                       C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)), 'tamgcn_saliency_joints')
        return sal, dxin, logits


# ----------------------------------------------------------------------------------------------------------------------
# The block as a registered operator: pure tensors in, a pure tensor out, a fake implementation for tracing / export.
#   params: Ae [K][V][V] (A * edge_importance), Wg [K][Cout][Cin], bg [Cout][V], Wt [Cout][Cout*KT] (tap innermost), bt [Cout],
#           Wr [Cout][Cin], br [Cout] (the residual conv, folded; both empty if there is none)      -- include/tamgcn.h "f2s"
#   geom:   K, KT, stride, block residual (0 none | 1 identity | 2 conv)
# x (N, Cin, T, V) -> out (N, Cout, (T - 1) // stride + 1, V).  Two launches.
# ----------------------------------------------------------------------------------------------------------------------
def _st_gcn_fwd(name, x, params, geom, groups=None):
    """groups None: the plain entry points on one model's params; else the grouped ones on params stacked on a leading group axis."""
    if not x.is_cuda or x.dtype != torch.float32:
        raise RuntimeError(f'{name}: expected a float32 HIP (cuda) tensor; there is no CPU path')
    if x.dim() != 4 or len(params) != 7 or len(geom) != 4:
        raise RuntimeError(f'{name}: expected x (N, C, T, V), 7 tensors and 4 integers, got {tuple(x.shape)}, {len(params)}, {len(geom)}')
    lib = _lib.load()
    K, kt, stride, rmode = geom
    N, Cin, T, V = x.shape
    ga, sfx = (), ''                                         # the grouped entry points take `groups` after the descriptor
    if groups is not None:
        if groups < 1 or N % groups:
            raise RuntimeError(f'{name}: {N} samples are not a multiple of groups = {groups}')
        if any(t.dim() < 1 or t.shape[0] != groups for t in params):
            raise RuntimeError(f'{name}: every tensor of params needs a leading axis of groups = {groups}')
        ga, sfx = (groups,), '_grouped'
        full = params
        params = [t[0] for t in params]                      # group 0's: the shapes below are per group
    Ae, Wg, bg, Wt, bt, Wr, br = (t.contiguous() for t in params)
    Cout = bt.shape[0]
    if not (2 <= V <= 32 and 1 <= K <= 3 and 1 <= Cin <= 256 and 16 <= Cout <= 256 and Cout % 16 == 0 and kt == KT and stride in (1, 2)):
        raise RuntimeError(f'{name}: V={V} K={K} Cin={Cin} Cout={Cout} KT={kt} stride={stride} is outside the f2s kernels '
                           '(2 <= V <= 32, K <= 3, Cin <= 256, Cout % 16 == 0, Cout <= 256, KT == 9, stride 1 | 2)')
    if tuple(Ae.shape) != (K, V, V) or tuple(Wg.shape) != (K, Cout, Cin) or tuple(bg.shape) != (Cout, V) or Wt.numel() != Cout * Cout * kt:
        raise RuntimeError(f'{name}: parameter shapes {[tuple(t.shape) for t in params]} do not fit x {tuple(x.shape)}, geom {list(geom)}')
    if rmode == 2 and (tuple(Wr.shape) != (Cout, Cin) or br.numel() != Cout) or rmode == 1 and (Cin != Cout or stride != 1):
        raise RuntimeError(f'{name}: residual mode {rmode} does not fit Cin={Cin} Cout={Cout} stride={stride}')
    if groups is not None:                                   # the whole stacked arrays: group g's follows group 0's densely
        Ae, Wg, bg, Wt, bt, Wr, br = (t.contiguous() for t in full)
    x = x.contiguous()
    dev = x.device
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    h = torch.empty(N, Cout, T, V, device=dev)
    g = _lib.F2sGcnDesc(N=N, Cin=Cin, Cout=Cout, T=T, V=V, K=K, x=x.data_ptr(), Ae=Ae.data_ptr(), wg=Wg.data_ptr(), bg=bg.data_ptr(),
                        h=h.data_ptr())
    _lib.check(getattr(lib, 'tamgcn_f2s_gcn' + sfx)(C.byref(g), *ga, st), 'tamgcn_f2s_gcn' + sfx)
    out = torch.empty(N, Cout, (T - 1) // stride + 1, V, device=dev)
    t = _lib.F2sTcnDesc(N=N, Cin=Cin, Cout=Cout, T=T, V=V, KT=kt, stride=stride, res_mode=rmode, h=h.data_ptr(), wt=Wt.data_ptr(),
                        bt=bt.data_ptr(), x=x.data_ptr() if rmode else None, wr=_opt(Wr) if rmode == 2 else None,
                        br=_opt(br) if rmode == 2 else None, out=out.data_ptr())
    _lib.check(getattr(lib, 'tamgcn_f2s_tcn' + sfx)(C.byref(t), *ga, st), 'tamgcn_f2s_tcn' + sfx)
    return out, h


@torch.library.custom_op('tamgcn::st_gcn_eval', mutates_args=())
def st_gcn_eval(x: Tensor, params: List[Tensor], geom: List[int]) -> Tensor:
    return _st_gcn_fwd('tamgcn::st_gcn_eval', x, params, geom)[0]


@st_gcn_eval.register_fake
def _(x, params, geom):
    N, _, T, V = x.shape
    return x.new_empty(N, params[4].shape[0], (T - 1) // geom[2] + 1, V)


# The same two launches, returning the gcn's h as well: what the data gradient needs to keep (its two ReLU masks).
@torch.library.custom_op('tamgcn::st_gcn_eval_fwd', mutates_args=())
def st_gcn_eval_fwd(x: Tensor, params: List[Tensor], geom: List[int]) -> Tuple[Tensor, Tensor]:
    return _st_gcn_fwd('tamgcn::st_gcn_eval_fwd', x, params, geom)


@st_gcn_eval_fwd.register_fake
def _(x, params, geom):
    N, _, T, V = x.shape
    Cout = params[4].shape[0]
    return x.new_empty(N, Cout, (T - 1) // geom[2] + 1, V), x.new_empty(N, Cout, T, V)


# ----------------------------------------------------------------------------------------------------------------------
# The grouped block: `groups` models of one geometry in the same two launches (include/tamgcn.h "f2s grouped").
#   x      (groups*n, Cin, T, V): rows [g n, (g+1) n) are group g's samples
#   params the seven tensors above, EVERY one stacked on a new leading group axis (an absent one: no elements)
#   geom   as above, shared by all groups
# Group g's slice of the result is bit-equal to st_gcn_eval on group g's slice and parameters.
# ----------------------------------------------------------------------------------------------------------------------
@torch.library.custom_op('tamgcn::st_gcn_eval_grouped', mutates_args=())
def st_gcn_eval_grouped(x: Tensor, params: List[Tensor], geom: List[int], groups: int) -> Tensor:
    return _st_gcn_fwd('tamgcn::st_gcn_eval_grouped', x, params, geom, groups)[0]


@st_gcn_eval_grouped.register_fake
def _(x, params, geom, groups):
    N, _, T, V = x.shape
    return x.new_empty(N, params[4].shape[1], (T - 1) // geom[2] + 1, V)


# ----------------------------------------------------------------------------------------------------------------------
# The block's data gradient as a registered operator (include/tamgcn.h "f2s backward").
#   gout (N, Cout, T2, V): the gradient of the block's output;  out (N, Cout, T2, V), h (N, Cout, T, V): st_gcn_eval_fwd's results
#   params: Ae [K][V][V], Wgb [K][Cin][Cout], Wtb [Cout][Cout][KT], Wrb [Cin][Cout] (empty if there is no residual conv)
#   geom:   the forward's
# -> dx (N, Cin, T, V).  Two launches.
# ----------------------------------------------------------------------------------------------------------------------
@torch.library.custom_op('tamgcn::st_gcn_eval_bwd', mutates_args=())
def st_gcn_eval_bwd(gout: Tensor, out: Tensor, h: Tensor, params: List[Tensor], geom: List[int]) -> Tensor:
    name = 'tamgcn::st_gcn_eval_bwd'
    if not (gout.is_cuda and out.is_cuda and h.is_cuda) or not (gout.dtype == out.dtype == h.dtype == torch.float32):
        raise RuntimeError(f'{name}: expected float32 HIP (cuda) tensors; there is no CPU path')
    if h.dim() != 4 or len(params) != 4 or len(geom) != 4:
        raise RuntimeError(f'{name}: expected h (N, C, T, V), 4 tensors and 4 integers, got {tuple(h.shape)}, {len(params)}, {len(geom)}')
    lib = _lib.load()
    K, kt, stride, rmode = geom
    Ae, Wgb, Wtb, Wrb = (t.contiguous() for t in params)
    N, Cout, T, V = h.shape
    Cin = Wgb.shape[1] if Wgb.dim() == 3 else 0
    if not (2 <= V <= 32 and 1 <= K <= 3 and 1 <= Cin <= 256 and 16 <= Cout <= 256 and Cout % 16 == 0 and kt == KT and stride in (1, 2)):
        raise RuntimeError(f'{name}: V={V} K={K} Cin={Cin} Cout={Cout} KT={kt} stride={stride} is outside the f2s kernels '
                           '(2 <= V <= 32, K <= 3, Cin <= 256, Cout % 16 == 0, Cout <= 256, KT == 9, stride 1 | 2)')
    T2 = (T - 1) // stride + 1
    if tuple(gout.shape) != (N, Cout, T2, V) or tuple(out.shape) != (N, Cout, T2, V):
        raise RuntimeError(f'{name}: gout {tuple(gout.shape)} and out {tuple(out.shape)} must be {(N, Cout, T2, V)} for h {tuple(h.shape)}, stride {stride}')
    if tuple(Ae.shape) != (K, V, V) or tuple(Wgb.shape) != (K, Cin, Cout) or Wtb.numel() != Cout * Cout * kt:
        raise RuntimeError(f'{name}: parameter shapes {[tuple(t.shape) for t in params]} do not fit h {tuple(h.shape)}, geom {list(geom)}')
    if rmode == 2 and tuple(Wrb.shape) != (Cin, Cout) or rmode == 1 and (Cin != Cout or stride != 1) or rmode not in (0, 1, 2):
        raise RuntimeError(f'{name}: residual mode {rmode} does not fit Cin={Cin} Cout={Cout} stride={stride}')
    gout, out, h = gout.contiguous(), out.contiguous(), h.contiguous()
    dev = h.device
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    dh = torch.empty(N, Cout, T, V, device=dev)
    t = _lib.F2sTcnBwdDesc(N=N, Cout=Cout, T=T, V=V, KT=kt, stride=stride, gout=gout.data_ptr(), out=out.data_ptr(), h=h.data_ptr(),
                           wtb=Wtb.data_ptr(), dh=dh.data_ptr())
    _lib.check(lib.tamgcn_f2s_tcn_bwd(C.byref(t), st), 'tamgcn_f2s_tcn_bwd')
    dx = torch.empty(N, Cin, T, V, device=dev)
    g = _lib.F2sGcnBwdDesc(N=N, Cin=Cin, Cout=Cout, T=T, V=V, K=K, stride=stride, res_mode=rmode, dh=dh.data_ptr(), Ae=Ae.data_ptr(),
                           wgb=Wgb.data_ptr(), gout=gout.data_ptr() if rmode else None, out=out.data_ptr() if rmode else None,
                           wrb=Wrb.data_ptr() if rmode == 2 else None, dx=dx.data_ptr())
    _lib.check(lib.tamgcn_f2s_gcn_bwd(C.byref(g), st), 'tamgcn_f2s_gcn_bwd')
    return dx


@st_gcn_eval_bwd.register_fake
def _(gout, out, h, params, geom):
    N, _, T, V = h.shape
    return h.new_empty(N, params[1].shape[1], T, V)


# ----------------------------------------------------------------------------------------------------------------------
# G models as one launch sequence
# ----------------------------------------------------------------------------------------------------------------------
def _model_fields(m):
    """The geometry all ST-GCN models of a group must share, as (name, value) pairs (f2.GroupedEval reads the first, second and
    fourth by position); each block's geometry is compared after folding (f2.stack_blocks)."""
    if not hasattr(m, 'st_gcn_networks') or not hasattr(m, 'edge_importance'):
        raise Unsupported('GroupedEvalST serves models.stgcn.Model')
    V = getattr(m, 'num_point', None)
    cin = m.st_gcn_networks[0].in_channels
    return [('num_point', V), ('num_class', m.fcn.out_channels), ('in_channels', cin),
            ('num_person', m.data_bn.num_features // (cin * V) if V else None), ('subsets', int(m.A.shape[0])),
            ('block plan', [(b.in_channels, b.out_channels, int(b.tcn[2].stride[0]), b._rmode) for b in m.st_gcn_networks])]


class GroupedEvalST(GroupedEval):
    """f2.GroupedEval on G models.stgcn.Model of one geometry: a fused stem (tamgcn_stem_streams_eval), TWO grouped launches per
    block (tamgcn::st_gcn_eval_grouped), one pool and one grouped fc -- 23 launches whatever G is.

        eng = GroupedEvalST(models)                     # all in eval() mode, on one device
        scores = eng(x, parent, modes)                  # x (N, C, T, V, M) JOINT clips; modes int32 [G] on the device
                                                        # -> (G, N, K): model g on stream modes[g] of x

    The models share num_point, num_class, in_channels, num_person, the number of subsets and the block plan; every model has its
    own edge_importance, so Ae = A * edge_importance differs per group like every other folded tensor.  Each model keeps its own
    FusedEvalST for the folding and the state key; stacking, the in-place re-fold of one model's slice, keep_alive and
    check_input are GroupedEval's."""
    NAME = 'GroupedEvalST'
    LABEL = 'st_gcn block {}'
    FAMILY = 'f2s'
    _fields = staticmethod(_model_fields)

    def _family(self, V):
        if not 2 <= V <= 32:
            raise Unsupported(f'{V} joints (the f2s kernels serve 2 <= V <= 32)')
        self._blk = torch.ops.tamgcn.st_gcn_eval_grouped
        return FusedEvalST

    @staticmethod
    def _fc(m):
        return m.fcn.weight.detach().view(m.fcn.weight.size(0), -1), m.fcn.bias.detach()

    def run(self, x, parent, modes, stacked):
        """x already checked (check_input), stacked = self._packed(x.device): the launches alone."""
        from . import ops
        G = len(self.models)
        h = ops.stem_streams_eval(x, parent, modes, self._coef)
        for params, geom in stacked:
            h = self._blk(h, params, geom, G)
        pooled = ops.head_pool_fwd(h, self.M)                      # (G*N, C): the single model's per-row arithmetic
        return ops.head_fc_grouped(pooled, self._fcw, self._fcb, G)
