"""-m gpu: the small-batch eval-mode kernel family for 25-joint (NTU-RGB+D) models (csrc/f2v.hip, tam_gcn_amd/f2v.py).

Bars (the V = 20 family's, tests/test_gpu_f2.py): every block, fed the fp64 oracle's own input for that block
(teacher-forced), within 4 x 1.21e-6 of max|ref| (1.21e-6: the worst block this file printed on the MI355X once the per-stage
ledger, test_gpu_f2_stages.py, was green); logits within 1e-4 max|ref| of the fp64 oracle with the same argmax; logits within
1e-3 of the reference's golden eval logits; logits and features within 2e-5 (relative) of the general eval path.  An fp32
torch evaluation of the same blocks stays below 5.5e-7 (logits 2.7e-6) on the three shapes: the logits bars are 30x the
reference's own rounding, the block bar 9x.  `pytest -s` prints the measured ratios."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cases import MODEL_CASES, MODEL_PARAM_SEED, MODEL_X_SEED                      # noqa: E402
from params import fill_state_, make_input                                        # noqa: E402
from tam_gcn_amd import f2, f2v, _lib                                               # noqa: E402
from tam_gcn_amd.models import ctrgcn as M                                          # noqa: E402
from oracle import ctrgcn_oracle as O                                               # noqa: E402

DEV = 'cuda:0'
TAG = 'ntu_t20'


def _model(gold, **over):
    """ntu_t20's seeded parameters with the fixture's `evalbuf` running statistics wherever the shapes match (the seeded
    statistics are not the statistics of anything: the eval-mode activations grow tenfold per block with them, see
    test_gpu_f2._model)."""
    margs = dict(next(c for c in MODEL_CASES if c[0] == TAG)[1], **over)
    m = M.Model(**margs)
    sd = m.state_dict()
    fill_state_(sd, seed=MODEL_PARAM_SEED)
    with torch.no_grad():
        for k in sd:
            key = f'{TAG}/evalbuf/{k}'
            if 'running_' in k and key in gold.files and tuple(gold[key].shape) == tuple(sd[k].shape):
                sd[k].copy_(torch.from_numpy(gold[key]))
    return m, margs


def _rel(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


class _general:
    """Model.forward on the general eval path (what TAMGCN_F2=0 selects)."""

    def __enter__(self):
        self.old = os.environ.get('TAMGCN_F2')
        os.environ['TAMGCN_F2'] = '0'

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ['TAMGCN_F2']
        else:
            os.environ['TAMGCN_F2'] = self.old


@pytest.mark.parametrize('shape', [(2, 3, 20, 25, 2), (1, 3, 13, 25, 1), (1, 3, 30, 25, 2)], ids=['t20_case', 't13_ragged_one_person', 't30'])
def test_every_block_against_the_fp64_oracle(shape, golden_models):
    """Frames per depth 20 -> 10 -> 5, 13 -> 7 -> 4 and 30 -> 15 -> 8: every residue of T*25 mod 4 at every stride, odd T
    under stride 2, ragged last tiles of 1, 2 and 3 frames, one and two persons, 1, 2 and 4 clip-persons."""
    m, margs = _model(golden_models, num_person=shape[4])
    sd64 = {k: (v.detach().clone().double() if v.is_floating_point() else v.clone()) for k, v in m.state_dict().items()}
    x = make_input(shape, seed=MODEL_X_SEED)
    h, N, Mp = O._stem(x.double(), sd64, 25, False)
    ins, outs = [], []
    for i in range(1, 11):
        ins.append(h)
        h = O.tcn_gcn_unit(h, sd64, f'l{i}', O._STRIDES.get(i, 1), residual=(i != 1), training=False)
        outs.append(h)
    m = m.to(DEV).eval()
    eng = f2v.FusedEvalV(m)
    blocks = eng._packed(torch.device(DEV))
    errs = []
    for i, (b, xin, ref) in enumerate(zip(blocks, ins, outs), 1):
        got = eng._block(b, xin.float().to(DEV).contiguous()).double().cpu()
        assert got.shape == ref.shape, (i, got.shape, ref.shape)
        assert bool(torch.isfinite(got).all()), f'l{i}'
        errs.append(_rel(got, ref))
    print(f'\n{shape}: block error / max|ref|: ' + ' '.join(f'l{i}={e:.2e}' for i, e in enumerate(errs, 1)))
    for i, e in enumerate(errs, 1):
        assert e <= 4 * 1.21e-6, f'l{i}: {e:.3e} of max|ref|'          # measured worst: 1.21e-6 (l9 of t30)
    with torch.no_grad():
        logits = eng(x.to(DEV)).double().cpu()
    ref = O.model_forward(x.double(), sd64, 25, training=False)
    print(f'{shape}: logits error / max|ref| = {_rel(logits, ref):.2e}')
    assert float((logits - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    assert torch.equal(logits.argmax(1), ref.argmax(1))


def test_golden_logits_and_the_general_path(monkeypatch, golden_models):
    """The case shape with every evalbuf statistic (test_gpu_model.py's eval section): the fixture's eval logits to 1e-3 (the
    fp64 oracle sits 4.9e-6 from them at logit scale 4.0), the general path to 2e-5; both through Model.forward."""
    tag, margs, shape = next(c for c in MODEL_CASES if c[0] == TAG)
    m, _ = _model(golden_models)
    m = m.to(DEV).eval()
    x = make_input(shape, seed=MODEL_X_SEED).to(DEV)
    calls = []
    real = f2v.FusedEvalV.blocks
    monkeypatch.setattr(f2v.FusedEvalV, 'blocks', lambda self, x: (calls.append(1), real(self, x))[1])
    with torch.no_grad():
        a = m(x)
        fa, _ = m.extract_feature(x)
        assert len(calls) == 2
        with _general():
            b = m(x)
            fb, _ = m.extract_feature(x)
    assert len(calls) == 2
    gold = golden_models[f'{tag}/logits_eval']
    print(f'\nlogits: |f2v - golden| = {np.abs(a.cpu().numpy() - gold).max():.2e}, f2v vs general {_rel(a, b):.2e}, features {_rel(fa, fb):.2e}')
    assert np.abs(a.cpu().numpy() - gold).max() <= 1e-3
    assert np.array_equal(a.cpu().numpy().argmax(1), gold.argmax(1))
    assert _rel(a, b) <= 2e-5
    assert fa.shape == fb.shape and _rel(fa, fb) <= 2e-5


def test_full_length_clip_against_the_general_path(golden_models):
    """(1, 3, 300, 25, 2): 75-tile grids, 300 -> 150 -> 75 frames (rows of 75 * 25 floats: unaligned).  The engine is called
    directly, whatever the routing bound is."""
    m, _ = _model(golden_models)
    m = m.to(DEV).eval()
    x = make_input((1, 3, 300, 25, 2), seed=4).to(DEV)
    eng = f2v.FusedEvalV(m)
    with torch.no_grad():
        a = eng(x)
        fa = eng.blocks(x)[0]
        with _general():
            b = m(x)
            fb = m._blocks(x)[0]
    print(f'\nT = 300: logits vs general {_rel(a, b):.2e}, features {_rel(fa, fb):.2e}')
    assert bool(torch.isfinite(a).all())
    assert _rel(a, b) <= 2e-5
    assert fa.shape == fb.shape and _rel(fa, fb) <= 2e-5


@pytest.mark.parametrize('which, T', [(1, 7), (4, 7), (4, 6)], ids=['identity_t7', 'stride2_conv_t7', 'stride2_conv_t6'])
def test_nan_before_the_input_and_in_its_slack_reaches_nothing(which, T, golden_models):
    """The input is a slice of a NaN-filled buffer: NaN in front of it (the slice starts 3 floats in: dword-aligned only) and in
    the 4 slack floats behind it, which the last 16-byte piece of the last frame reads.  Same bits as on a clean copy."""
    m, _ = _model(golden_models)
    m = m.to(DEV).eval()
    b = f2v.FusedEvalV(m)._packed(torch.device(DEV))[which]
    data = make_input((2, 64, T, 25), seed=3).to(DEV)
    n = data.numel()
    buf = torch.full((3 + n + 4,), float('nan'), device=DEV)
    buf[3:3 + n] = data.view(-1)
    dirty = buf[3:3 + n].view(data.shape)
    assert dirty.data_ptr() % 16 == 12 and bool(torch.isnan(buf[3 + n:]).all())
    clean, cxp = torch.ops.tamgcn.tcn_gcn_unit_eval_v25(data, None, b.params, b.geom)
    got, gxp = torch.ops.tamgcn.tcn_gcn_unit_eval_v25(dirty, None, b.params, b.geom)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(gxp).all())
    assert torch.equal(got, clean) and torch.equal(gxp, cxp)
    assert bool(torch.isnan(buf[:3]).all()) and bool(torch.isnan(buf[3 + n:]).all())


def test_model_forward_routes_small_eval_batches_here(monkeypatch, golden_models):
    m, margs = _model(golden_models)
    m = m.to(DEV).eval()
    x = make_input((1, 3, 16, 25, 2), seed=2).to(DEV)
    calls = []
    real = f2v.FusedEvalV.blocks
    monkeypatch.setattr(f2v.FusedEvalV, 'blocks', lambda self, x: (calls.append(1), real(self, x))[1])
    with torch.no_grad():
        m(x)
        m.extract_feature(x)
        assert len(calls) == 2
        assert m._f2(x) is None and m._f2v(x) is not None
        T = 8
        big = make_input((f2v.F2V_MAX_FRAMES // (2 * T) + 1, 3, T, 25, 2), seed=3).to(DEV)
        assert m._f2v(big[:-1]) is not None and m._f2v(big) is None
        m(big)                                              # over the bound (clip-persons x frames): general path
        assert len(calls) == 2
        monkeypatch.setenv('TAMGCN_F2', '0')
        m(x)
        assert len(calls) == 2
        monkeypatch.setenv('TAMGCN_F2', '1')
        h = m.l3.register_forward_hook(lambda mod, i, o: None)
        m(x)                                                # a forward hook would not fire inside the engine
        assert len(calls) == 2
        h.remove()
        m(x)
        assert len(calls) == 3
    m(x)                                                    # grad mode: general path (autograd)
    assert len(calls) == 3
    m.train()
    with torch.no_grad():
        m(x)
    assert len(calls) == 3


def _pair(m, x):
    with torch.no_grad():
        a = m(x)
        with _general():
            b = m(x)
    assert _rel(a, b) <= 2e-5
    return a


def test_refolds_after_every_kind_of_state_change(golden_models):
    m, _ = _model(golden_models)
    m = m.to(DEV).eval()
    x = make_input((1, 3, 20, 25, 2), seed=MODEL_X_SEED).to(DEV)
    a0 = _pair(m, x)
    assert m.__dict__.get('_tamgcn_f2v')
    with torch.no_grad():
        m.l3.tcn1.branches[0][1].weight.mul_(1.5)
        m.l6.gcn1.convs[1].conv4.bias.add_(0.3)
    a1 = _pair(m, x)
    assert float((a1 - a0).abs().max()) > 0
    m2, _ = _model(golden_models)
    with torch.no_grad():
        for p in m2.parameters():
            p.mul_(0.9)
    m.load_state_dict(m2.state_dict())
    a2 = _pair(m, x)
    assert float((a2 - a1).abs().max()) > 1e-3 * float(a1.abs().max())


def test_refolds_after_a_flat_arena_step(golden_models):
    from tam_gcn_amd.distributed import ParamArena, SGDNesterov
    m, _ = _model(golden_models)
    m = m.to(DEV).eval()
    arena = ParamArena(m)
    bucket = arena.grad_bucket()
    opt = SGDNesterov(arena.params, lr=0.05, momentum=0.9, weight_decay=1e-4, arena=arena, bucket=bucket)
    x = make_input((1, 3, 20, 25, 2), seed=MODEL_X_SEED).to(DEV)
    a0 = _pair(m, x)
    g = torch.Generator().manual_seed(3)
    for p in arena.params:
        p.grad = (torch.randn(p.shape, generator=g) * p.detach().abs().mean().cpu()).to(DEV)
    bucket.pack()
    opt.step()
    a1 = _pair(m, x)
    assert float((a1 - a0).abs().max()) > 1e-3 * float(a0.abs().max())


def test_graph_replay_and_launch_count(golden_models):
    """GraphedForward captures this path: replay = eager bit for bit, two eager runs are bit-equal; 50 family launches per
    forward and at most 56 ABI launches in all, as for V = 20."""
    from tam_gcn_amd.inference import GraphedForward
    m, _ = _model(golden_models)
    m = m.to(DEV).eval()
    fast = GraphedForward(m)
    for shape in ((1, 3, 13, 25, 2), (2, 3, 20, 25, 2)):
        x = make_input(shape, seed=shape[2]).to(DEV)
        with torch.no_grad():
            ref = m(x)
            assert torch.equal(m(x), ref)
        assert torch.equal(fast(x).clone(), ref)
        assert torch.equal(fast(x).clone(), ref)

    class Count:
        def __init__(self, lib):
            self.lib, self.n, self.names = lib, 0, []

        def __getattr__(self, name):
            fn = getattr(self.lib, name)
            if not name.startswith('tamgcn_') or name in ('tamgcn_last_error',):
                return fn

            def w(*args):
                self.n += 1
                self.names.append(name)
                return fn(*args)
            return w
    real = _lib.load()
    cnt = Count(real)
    _lib._lib = cnt
    try:
        with torch.no_grad():
            m(make_input((1, 3, 20, 25, 2), seed=9).to(DEV))
    finally:
        _lib._lib = real
    assert cnt.n <= 56, (cnt.n, cnt.names)
    assert sum(n.startswith('tamgcn_f2v_') for n in cnt.names) == 50
    assert not any(n.startswith('tamgcn_f2_') for n in cnt.names)


def test_block_is_a_registered_operator(golden_models):
    """torch.ops.tamgcn.tcn_gcn_unit_eval_v25: schema and fake-tensor checks on a stride-1 identity block and a stride-2 block with
    convolutional residuals; the second output holds the frame sums of the first over tiles of four frames."""
    m, _ = _model(golden_models)
    m = m.to(DEV).eval()
    blocks = f2v.FusedEvalV(m)._packed(torch.device(DEV))
    x = make_input((2, 64, 11, 25), seed=3).to(DEV)
    for b in (blocks[1], blocks[4]):
        torch.library.opcheck(torch.ops.tamgcn.tcn_gcn_unit_eval_v25.default, (x, None, b.params, b.geom),
                              test_utils=('test_schema', 'test_faketensor'))
    for b, shp in ((blocks[1], (2, 64, 11, 25)), (blocks[4], (2, 128, 6, 25))):
        out, xp = torch.ops.tamgcn.tcn_gcn_unit_eval_v25(x, None, b.params, b.geom)
        T2 = shp[2]
        assert tuple(out.shape) == shp and tuple(xp.shape) == (2, (T2 + 3) // 4, shp[1], 28)
        assert float(xp[..., 25:].abs().max()) == 0.0
        pad = torch.zeros(2, shp[1], (-T2) % 4, 25, device=DEV)
        want = torch.cat((out, pad), 2).view(2, shp[1], -1, 4, 25).sum(3).permute(0, 2, 1, 3)
        assert float((xp[..., :25] - want).abs().max()) <= 1e-6 * float(out.abs().max()) * 4
        # the next block takes those sums instead of reading its input again: same E to rounding, so the same output
        nb = blocks[2] if b is blocks[1] else blocks[5]
        o1, _ = torch.ops.tamgcn.tcn_gcn_unit_eval_v25(out, xp, nb.params, nb.geom)
        o2, _ = torch.ops.tamgcn.tcn_gcn_unit_eval_v25(out, None, nb.params, nb.geom)
        assert _rel(o1, o2) <= 1e-5


def test_engine_argument_guards(golden_models):
    m, _ = _model(golden_models)
    with pytest.raises(ValueError):
        f2v.FusedEvalV(m.to(DEV))                           # train mode
    m.eval()
    eng = f2v.FusedEvalV(m)
    x = make_input((1, 3, 12, 25, 2), seed=1)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='no CPU path'):
            eng(x)
        with pytest.raises(f2.Unsupported):
            eng(make_input((1, 3, 12, 20, 2), seed=1).to(DEV))
    with pytest.raises(RuntimeError, match='no_grad'):
        eng(x.to(DEV))
    lib = _lib.load()
    d = _lib.F2GemmDesc(N=1, K=64, M=64, T=8, V=20, mode=1, relu_rows=0, x=1 << 20, w=1 << 20, b=1 << 20, add=None, out=1 << 20)
    assert lib.tamgcn_f2v_gemm(C.byref(d), None) != 0 and b'V = 25' in lib.tamgcn_last_error()
