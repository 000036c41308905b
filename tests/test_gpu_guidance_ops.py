"""-m gpu: the registered guidance operators (tam_gcn_amd/torch_ops.py: tamgcn::guidance_reduce, guidance_weights,
guidance_apply): schema and fake-tensor checks by torch.library.opcheck, as tests/test_gpu_torch_ops.py does for the others, and
tracing without a graph break."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from params import make_input                           # noqa: E402
from tam_gcn_amd import torch_ops                        # noqa: E402,F401

DEV = 'cuda:0'
UTILS = ('test_schema', 'test_faketensor')


def test_opcheck():
    h = make_input((4, 20, 5, 25), 3).to(DEV)
    torch.library.opcheck(torch.ops.tamgcn.guidance_reduce.default, (h, 2), test_utils=UTILS)
    torch.library.opcheck(torch.ops.tamgcn.guidance_reduce.default, (h, 1), test_utils=UTILS)
    inten, pooled, minmax = torch.ops.tamgcn.guidance_reduce(h, 2)
    assert inten.shape == (2, 5, 25, 2) and pooled.shape == (2, 20) and minmax.shape == (4 * 2, 2)
    joints = torch.tensor([3, 11, 30], dtype=torch.int32, device=DEV)
    torch.library.opcheck(torch.ops.tamgcn.guidance_weights.default, (inten, minmax, joints, 15), test_utils=UTILS)
    w = torch.ops.tamgcn.guidance_weights(inten, minmax, joints, 15)
    assert w.shape == (2, 3) and bool((w[:, 2] == 0).all())
    rgb = make_input((2, 3, 9, 7), 4).to(DEV)
    for args in ((w, rgb, 5, 9, 7, False), (w, rgb, 5, 9, 7, True), (w, None, 5, 9, 7, True)):
        torch.library.opcheck(torch.ops.tamgcn.guidance_apply.default, args, test_utils=UTILS)
    out, wm = torch.ops.tamgcn.guidance_apply(w, rgb, 5, 9, 7, True)
    assert out.shape == rgb.shape and wm.shape == (2, 1, 9, 7) and torch.equal(out, rgb * wm)
    none, wm2 = torch.ops.tamgcn.guidance_apply(w, None, 5, 9, 7, True)
    assert none.numel() == 0 and torch.equal(wm, wm2)


def test_traces_without_a_graph_break():
    h = make_input((2, 20, 5, 20), 5).to(DEV)
    rgb = make_input((2, 1, 8, 8), 6).to(DEV)
    joints = torch.tensor([3, 11], dtype=torch.int32, device=DEV)

    def f(h, rgb, joints):
        inten, pooled, minmax = torch.ops.tamgcn.guidance_reduce(h, 1)
        w = torch.ops.tamgcn.guidance_weights(inten, minmax, joints, 3)
        return torch.ops.tamgcn.guidance_apply(w, rgb, 5, 8, 8, False)[0] + pooled.sum()

    eager = f(h, rgb, joints)
    compiled = torch.compile(f, backend='eager', fullgraph=True)(h, rgb, joints)      # fullgraph: any graph break raises
    assert torch.equal(eager, compiled)
