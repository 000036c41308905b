"""Small-batch eval-mode engine for 25-joint (NTU-RGB+D) models: tam_gcn_amd.f2's engine on the f2v kernel family
(csrc/f2v.hip: tamgcn_f2v_e / _f2v_gcn / _f2v_gemm x 2 / _f2v_tcn, five launches per TCN_GCN_unit).

    eng = FusedEvalV(model)           # model.eval(); V = 25 joints, the block plan of models.ctrgcn.Model
    logits = eng(x)                   # x (N, C, T, 25, M) on the GPU, under torch.no_grad()

The folding of eval-mode BatchNorm (`f2._Block`), the parameter-state key and the re-fold are f2's, inherited; what is new
is the registered operator that runs one block.  A block's input and output are contiguous (N, C, T, 25); E, the four
workspaces and the frame sums, which live inside the operator, have frames of 28 floats (include/tamgcn.h, the f2v comment).

`Model.forward` routes here by itself in eval mode without autograd for batches of at most F2V_MAX_FRAMES clip-persons x
frames (N * M * T; an NTU clip is 300 frames and two persons, so the bound is in frames and not in clips; TAMGCN_F2V_MAX_FRAMES
overrides it, TAMGCN_F2=0 switches both families off).  No CPU path, no fallback inside: `Unsupported` is raised before
anything is launched."""
import ctypes as C
import os
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import _lib, ops
from .f2 import FusedEval, Unsupported, enabled, _opt

__all__ = ['FusedEvalV', 'Unsupported', 'F2V_MAX_FRAMES', 'enabled']

F2V_MAX_FRAMES = int(os.environ.get('TAMGCN_F2V_MAX_FRAMES', '1024'))      # N*M*T up to which Model.forward routes here
V, VP = 25, 28                                                            # joints; floats per frame of the family's own buffers


class FusedEvalV(FusedEval):
    V = V
    FAMILY = 'f2v'

    def _block(self, b, x, st=None, xpart=None, want_xpart=False):
        out, xp = torch.ops.tamgcn.tcn_gcn_unit_eval_v25(x, xpart, b.params, b.geom)
        return (out, xp) if want_xpart else out


# ----------------------------------------------------------------------------------------------------------------------
# The block as a registered operator: f2.tcn_gcn_unit_eval's arguments (params / geom as documented there) at V = 25.
# Returns (out (N, Cout, T2, 25), xpart (N, ceil(T2/4), Cout, 28)): xpart[..., :25] = per-tile (four frames) frame sums of
# out, xpart[..., 25:] = 0 -- the next block's `xpart` argument.
# ----------------------------------------------------------------------------------------------------------------------
@torch.library.custom_op('tamgcn::tcn_gcn_unit_eval_v25', mutates_args=())
def tcn_gcn_unit_eval_v25(x: Tensor, xpart: Optional[Tensor], params: List[Tensor], geom: List[int]) -> Tuple[Tensor, Tensor]:
    lib = _lib.load()
    if not x.is_cuda or x.dtype != torch.float32:
        raise RuntimeError('tamgcn::tcn_gcn_unit_eval_v25: expected a float32 HIP (cuda) tensor; there is no CPU path')
    if x.dim() != 4 or x.shape[3] != V:
        raise RuntimeError(f'tamgcn::tcn_gcn_unit_eval_v25: expected (N, C, T, {V}), got {tuple(x.shape)}')
    x = ops.with_slack(x.contiguous())                           # the last 16-byte piece of the last frame reads 12 bytes past it
    (W12, B12, W3, B3, W4, B4, PA, alpha, sy, ty, Wd, bd, Wo, bo, We, be, sp, tp, Wr, br), rest = params[:20], params[20:]
    R, gmode, Cb, nb, ks, stride, rmode = geom[:7]
    dils = geom[7:7 + nb]
    N, Cin, T, _ = x.shape
    Cout = W3.shape[0] // 3
    dev = x.device
    if xpart is not None:
        if tuple(xpart.shape) != (N, (T + 3) // 4, Cin, VP):
            raise RuntimeError(f'tamgcn::tcn_gcn_unit_eval_v25: xpart {tuple(xpart.shape)}, expected {(N, (T + 3) // 4, Cin, VP)}')
        xpart = xpart.contiguous()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    E = torch.empty(N, 3, Cout, V, VP, device=dev)
    ws = torch.empty(4, N, Cout, T, VP, device=dev)              # y + res, res - y, g, h
    sm, df, g, h = ws[0], ws[1], ws[2], ws[3]
    d = _lib.F2GcnDesc(N=N, Cin=Cin, Cout=Cout, T=T, V=V, S=3, R=R, res_mode=gmode,
                       x=x.data_ptr(), w12=W12.data_ptr(), b12=B12.data_ptr(), w4=W4.data_ptr(), b4=B4.data_ptr(),
                       A=PA.data_ptr(), alpha=alpha.data_ptr(), w3=W3.data_ptr(), b3=B3.data_ptr(),
                       sy=sy.data_ptr(), ty=ty.data_ptr(), wd=_opt(Wd), bd=_opt(bd),
                       E=E.data_ptr(), sum=sm.data_ptr(), diff=df.data_ptr(), xpart=_opt(xpart))
    _lib.check(lib.tamgcn_f2v_e(C.byref(d), st), 'tamgcn_f2v_e')
    _lib.check(lib.tamgcn_f2v_gcn(C.byref(d), st), 'tamgcn_f2v_gcn')
    q = _lib.F2GemmDesc(N=N, K=Cout, M=Cout, T=T, V=V, mode=0, relu_rows=0, x=df.data_ptr(), w=Wo.data_ptr(), b=bo.data_ptr(),
                        add=sm.data_ptr(), out=g.data_ptr())
    _lib.check(lib.tamgcn_f2v_gemm(C.byref(q), st), 'tamgcn_f2v_gemm')
    q = _lib.F2GemmDesc(N=N, K=Cout, M=Cout, T=T, V=V, mode=1, relu_rows=(nb + 1) * Cb, x=g.data_ptr(), w=We.data_ptr(),
                        b=be.data_ptr(), add=None, out=h.data_ptr())
    _lib.check(lib.tamgcn_f2v_gemm(C.byref(q), st), 'tamgcn_f2v_gemm')
    T2 = (T - 1) // stride + 1
    out = ops.empty(N, Cout, T2, V, like=x)                      # the next block's input: with the slack its reads need
    xp = torch.empty(N, (T2 + 3) // 4, Cout, VP, device=dev)     # per-tile frame sums: the next block's xbar
    t = _lib.F2TcnDesc(N=N, Cin=Wr.shape[1] if rmode == 2 else Cin, Cout=Cout, T=T, V=V, stride=stride, Cb=Cb, nb=nb, ks=ks,
                       res_mode=rmode, h=h.data_ptr(), sp=sp.data_ptr(), tp=tp.data_ptr(), x=x.data_ptr(), wr=_opt(Wr), br=_opt(br),
                       out=out.data_ptr(), xpart=xp.data_ptr())
    for i in range(nb):
        t.dil[i] = dils[i]
        t.wt[i] = rest[2 * i].data_ptr()
        t.bt[i] = rest[2 * i + 1].data_ptr()
    _lib.check(lib.tamgcn_f2v_tcn(C.byref(t), st), 'tamgcn_f2v_tcn')
    return out, xp


@tcn_gcn_unit_eval_v25.register_fake
def _(x, xpart, params, geom):
    N, _, T, V_ = x.shape
    Cout = params[2].shape[0] // 3
    T2 = (T - 1) // geom[5] + 1
    return x.new_empty(N, Cout, T2, V_), x.new_empty(N, (T2 + 3) // 4, Cout, VP)
