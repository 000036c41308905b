"""Small-batch eval-mode engines for models whose joint count is no multiple of four: tam_gcn_amd.f2's engine on the f2v
kernel family (csrc/f2v.hip: tamgcn_f2v_e / _f2v_gcn / _f2v_gemm x 2 / _f2v_tcn, five launches per TCN_GCN_unit).  The
kernels are instantiated for the joint counts of JOINTS: 25 (NTU-RGB+D), 17 (graph.coco: COCO / YOLO-pose keypoints) and
18 (graph.openpose).

    eng = FusedEvalV(model)           # model.eval(); V = 25 joints, the block plan of models.ctrgcn.Model
    logits = eng(x)                   # x (N, C, T, 25, M) on the GPU, under torch.no_grad()
    eng = FusedEvalJ(model)           # the same for every other joint count of JOINTS (17, 18)

The folding of eval-mode BatchNorm (`f2._Block`), the parameter-state key and the re-fold are f2's, inherited; what is new
is the registered operator that runs one block.  A block's input and output are contiguous (N, C, T, 25); E, the four
workspaces and the frame sums, which live inside the operator, have frames of 28 floats (include/tamgcn.h, the f2v comment).

`Model.forward` routes here by itself in eval mode without autograd for batches of at most F2V_MAX_FRAMES clip-persons x
frames (N * M * T; an NTU clip is 300 frames and two persons, so the bound is in frames and not in clips; TAMGCN_F2V_MAX_FRAMES
overrides it, TAMGCN_F2=0 switches both families off).  17- and 18-joint models are routed to FusedEvalJ up to
F2J_MAX_FRAMES clip-persons x frames (TAMGCN_F2J_MAX_FRAMES; measured: profiles/f2j_infer_bench.txt).  No CPU path, no
fallback inside: `Unsupported` is raised before anything is launched."""
import os
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from .f2 import FusedEval, Unsupported, enabled, _unit

__all__ = ['FusedEvalV', 'FusedEvalJ', 'JOINTS', 'Unsupported', 'F2V_MAX_FRAMES', 'F2J_MAX_FRAMES', 'enabled']

F2V_MAX_FRAMES = int(os.environ.get('TAMGCN_F2V_MAX_FRAMES', '1024'))      # N*M*T up to which Model.forward routes here
V, VP = 25, 28                                                            # joints; floats per frame of the family's own buffers
JOINTS = (17, 18, 25)                                                     # FV_JOINTS of csrc/f2v.hip (tests/test_f2j_cpu.py holds it to the source)
# N*M*T up to which Model.forward routes 17- / 18-joint models to FusedEvalJ: the last measured win over the general eval
# path in BOTH graph replay and eager, for both joint counts (profiles/f2j_infer_bench.txt)
F2J_MAX_FRAMES = int(os.environ.get('TAMGCN_F2J_MAX_FRAMES', '1024'))


def _vp(v):
    return (v + 3) & ~3


class FusedEvalV(FusedEval):
    V = V
    FAMILY = 'f2v'

    def _block(self, b, x, st=None, xpart=None, want_xpart=False):
        out, xp = torch.ops.tamgcn.tcn_gcn_unit_eval_v25(x, xpart, b.params, b.geom)
        return (out, xp) if want_xpart else out


class FusedEvalJ(FusedEval):
    """The engine for every joint count of JOINTS other than 25 (which stays FusedEvalV's): V is the model's."""
    FAMILY = 'f2v'

    def __init__(self, model):
        if model.training:
            raise ValueError('FusedEvalJ: put the model in eval() mode first')
        v = getattr(model, 'num_point', None)
        if v not in JOINTS or v == V:
            raise Unsupported(f'{v} joints (FusedEvalJ serves V in {tuple(j for j in JOINTS if j != V)} of the f2v kernels\' '
                              f'joint counts {JOINTS}; 25 joints: FusedEvalV, 20: f2.FusedEval)')
        self.V = v
        super().__init__(model)

    def _block(self, b, x, st=None, xpart=None, want_xpart=False):
        out, xp = torch.ops.tamgcn.tcn_gcn_unit_eval_vj(x, xpart, b.params, b.geom)
        return (out, xp) if want_xpart else out


# ----------------------------------------------------------------------------------------------------------------------
# The block as a registered operator: f2.tcn_gcn_unit_eval's arguments (params / geom as documented there) at V = 25.
# Returns (out (N, Cout, T2, 25), xpart (N, ceil(T2/4), Cout, 28)): xpart[..., :25] = per-tile (four frames) frame sums of
# out, xpart[..., 25:] = 0 -- the next block's `xpart` argument.
# ----------------------------------------------------------------------------------------------------------------------
@torch.library.custom_op('tamgcn::tcn_gcn_unit_eval_v25', mutates_args=())
def tcn_gcn_unit_eval_v25(x: Tensor, xpart: Optional[Tensor], params: List[Tensor], geom: List[int]) -> Tuple[Tensor, Tensor]:
    return _unit('f2v', x, xpart, params, geom, None)


@tcn_gcn_unit_eval_v25.register_fake
def _(x, xpart, params, geom):
    N, _, T, V_ = x.shape
    Cout = params[2].shape[0] // 3
    T2 = (T - 1) // geom[5] + 1
    return x.new_empty(N, Cout, T2, V_), x.new_empty(N, (T2 + 3) // 4, Cout, VP)


# The grouped block at V = 25 (f2.tcn_gcn_unit_eval_grouped's arguments: every tensor of params stacked on a leading group axis).
@torch.library.custom_op('tamgcn::tcn_gcn_unit_eval_v25_grouped', mutates_args=())
def tcn_gcn_unit_eval_v25_grouped(x: Tensor, xpart: Optional[Tensor], params: List[Tensor], geom: List[int], groups: int) -> Tuple[Tensor, Tensor]:
    return _unit('f2v', x, xpart, params, geom, groups)


@tcn_gcn_unit_eval_v25_grouped.register_fake
def _(x, xpart, params, geom, groups):
    N, _, T, V_ = x.shape
    Cout = params[2].shape[1] // 3
    T2 = (T - 1) // geom[5] + 1
    return x.new_empty(N, Cout, T2, V_), x.new_empty(N, (T2 + 3) // 4, Cout, VP)


# ----------------------------------------------------------------------------------------------------------------------
# The same two operators for any joint count V of JOINTS (x (N, C, T, V)): out (N, Cout, T2, V), xpart (N, ceil(T2/4), Cout,
# VP) with VP = (V + 3) & ~3 and xpart[..., V:] = 0.
# ----------------------------------------------------------------------------------------------------------------------
@torch.library.custom_op('tamgcn::tcn_gcn_unit_eval_vj', mutates_args=())
def tcn_gcn_unit_eval_vj(x: Tensor, xpart: Optional[Tensor], params: List[Tensor], geom: List[int]) -> Tuple[Tensor, Tensor]:
    return _unit('f2v', x, xpart, params, geom, None, JOINTS, '_vj')


@tcn_gcn_unit_eval_vj.register_fake
def _(x, xpart, params, geom):
    N, _, T, V_ = x.shape
    Cout = params[2].shape[0] // 3
    T2 = (T - 1) // geom[5] + 1
    return x.new_empty(N, Cout, T2, V_), x.new_empty(N, (T2 + 3) // 4, Cout, _vp(V_))


@torch.library.custom_op('tamgcn::tcn_gcn_unit_eval_vj_grouped', mutates_args=())
def tcn_gcn_unit_eval_vj_grouped(x: Tensor, xpart: Optional[Tensor], params: List[Tensor], geom: List[int], groups: int) -> Tuple[Tensor, Tensor]:
    return _unit('f2v', x, xpart, params, geom, groups, JOINTS, '_vj')


@tcn_gcn_unit_eval_vj_grouped.register_fake
def _(x, xpart, params, geom, groups):
    N, _, T, V_ = x.shape
    Cout = params[2].shape[1] // 3
    T2 = (T - 1) // geom[5] + 1
    return x.new_empty(N, Cout, T2, V_), x.new_empty(N, (T2 + 3) // 4, Cout, _vp(V_))
