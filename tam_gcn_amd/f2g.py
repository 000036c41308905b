"""Small-batch eval-mode engine for CTR-GCN models of ANY joint count 8 <= V <= 28: tam_gcn_amd.f2's engine on the f2g kernel
family (csrc/f2g.hip: tamgcn_f2g_e / _f2g_gcn / _f2g_gemm x 2 / _f2g_tcn, five launches per TCN_GCN_unit).  The kernels take
the joint count as an argument and are instantiated per frame pitch VP = (V + 3) & ~3 only, so a 21-joint hand skeleton,
SHREC's 22 joints, SMPL's 24, Halpe's 26 or a 16-joint MPII / H36M layout get the same five launches per block that the
dedicated families give 20 (f2), 25, 17 and 18 joints (f2v).

    eng = FusedEvalG(model)           # model.eval(); V = model.num_point in JOINTS_RANGE
    logits = eng(x)                   # x (N, C, T, V, M) on the GPU, under torch.no_grad()

The folding of eval-mode BatchNorm (`f2._Block`), the parameter-state key and the re-fold are f2's, inherited; the buffer
layout is f2v's (a block's input and output contiguous (N, C, T, V); E, the workspaces and the frame sums in frames of VP
floats).  The engine accepts every joint count of the range, 17, 18, 20 and 25 included (the run-time-V kernels against the
templated ones at the same V: profiles/f2g_infer_bench.txt); `Model.forward` routes here only the joint counts that have no
dedicated family, in eval mode without autograd, for at most F2G_MAX_FRAMES clip-persons x frames (N * M * T;
TAMGCN_F2G_MAX_FRAMES overrides it, TAMGCN_F2=0 switches every small-batch family off).  No CPU path, no fallback inside:
`Unsupported` is raised before anything is launched."""
import os
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from .f2 import FusedEval, Unsupported, enabled, _unit

__all__ = ['FusedEvalG', 'JOINTS_RANGE', 'DEDICATED', 'Unsupported', 'F2G_MAX_FRAMES', 'enabled']

JOINTS_RANGE = (8, 28)                                                    # FG_VMIN, FG_VMAX of csrc/f2g.hip (tamgcn_f2g_supported)
DEDICATED = (17, 18, 20, 25)                                              # joint counts Model.forward keeps on f2 / f2v
# N*M*T up to which Model.forward routes here: the last measured win over the general eval path in BOTH graph replay and
# eager, at every measured joint count (16, 21, 28: profiles/f2g_infer_bench.txt; at 1024 the family loses under replay at 28)
F2G_MAX_FRAMES = int(os.environ.get('TAMGCN_F2G_MAX_FRAMES', '512'))
_JOINTS = tuple(range(JOINTS_RANGE[0], JOINTS_RANGE[1] + 1))


def _vp(v):
    return (v + 3) & ~3


class FusedEvalG(FusedEval):
    """The engine for any joint count of JOINTS_RANGE: V is the model's."""
    FAMILY = 'f2g'

    def __init__(self, model):
        if model.training:
            raise ValueError('FusedEvalG: put the model in eval() mode first')
        v = getattr(model, 'num_point', None)
        if not isinstance(v, int) or not JOINTS_RANGE[0] <= v <= JOINTS_RANGE[1]:
            raise Unsupported(f'{v} joints (FusedEvalG serves {JOINTS_RANGE[0]} <= V <= {JOINTS_RANGE[1]}, f2g.JOINTS_RANGE)')
        self.V = v
        super().__init__(model)

    def _block(self, b, x, st=None, xpart=None, want_xpart=False):
        out, xp = torch.ops.tamgcn.tcn_gcn_unit_eval_vg(x, xpart, b.params, b.geom)
        return (out, xp) if want_xpart else out


# ----------------------------------------------------------------------------------------------------------------------
# The block as a registered operator: f2.tcn_gcn_unit_eval's arguments (params / geom as documented there) for x (N, C, T, V),
# 8 <= V <= 28.  Returns (out (N, Cout, T2, V), xpart (N, ceil(T2/4), Cout, VP)) with VP = (V + 3) & ~3 and xpart[..., V:] = 0.
# ----------------------------------------------------------------------------------------------------------------------
@torch.library.custom_op('tamgcn::tcn_gcn_unit_eval_vg', mutates_args=())
def tcn_gcn_unit_eval_vg(x: Tensor, xpart: Optional[Tensor], params: List[Tensor], geom: List[int]) -> Tuple[Tensor, Tensor]:
    if x.dim() == 4 and x.shape[3] not in _JOINTS:                # (the kernels would refuse it too; this names the range)
        raise RuntimeError(f'tamgcn::tcn_gcn_unit_eval_vg: expected (N, C, T, V) with {JOINTS_RANGE[0]} <= V <= {JOINTS_RANGE[1]}, '
                           f'got {tuple(x.shape)}')
    return _unit('f2g', x, xpart, params, geom, None, _JOINTS, '_vg')


@tcn_gcn_unit_eval_vg.register_fake
def _(x, xpart, params, geom):
    N, _, T, V_ = x.shape
    Cout = params[2].shape[0] // 3
    T2 = (T - 1) // geom[5] + 1
    return x.new_empty(N, Cout, T2, V_), x.new_empty(N, (T2 + 3) // 4, Cout, _vp(V_))
