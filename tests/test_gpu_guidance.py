"""-m gpu: tam_gcn_amd.guidance end to end (pooled_feature, joint_intensity, SkeletonGuidance) on the models of
tests/guidance_models.py: N-UCLA clips of 52 and 128 frames (T' = 13 and 32: either side of the top-15 rule), NTU with two persons,
COCO (17 joints: target joint 18 does not exist), a 21-joint synthetic graph (the f2g family) and 33 clips (above f2.F2_MAX_CLIPS:
the general route).

Bars.  The guidance kernels read the block stack's output h, which the existing suites pin on their own; so
  (a) against guidance_ref applied to the model's OWN extract_feature(x)[0] in fp64, the results are held to the stage bars of
      tests/test_gpu_guidance_stages.py unchanged (that is also "pooled_feature == extract_feature(x)[0].mean((2, 3, 4))" and the
      same for joint_intensity, to their bars), and
  (b) against the fp64 oracle (oracle/ctrgcn_oracle.py, then guidance_ref) and against the reference's recorded maps
      (tests/golden/guidance.npz), the intensity error E of those bars grows by what the features differ: the channel L2 norm is
      1-Lipschitz, so an intensity moves by at most the L2 norm over channels of (h - h_oracle) in its column, and the largest such
      norm D is MEASURED per case and added to E -- after asserting max|h - h_oracle| <= 1e-4 max|h_oracle|, the bar the eval
      families' logits are held to (tests/test_gpu_f2.py), so that the allowance cannot hide a broken forward.  For the recorded
      maps the reference's own float32 steps add their bar once more (tests/test_guidance_ref_cpu.py).
The two routes (the small-batch family, and the general path that TAMGCN_F2=0 selects) are each held to (a) and (b), and to each
other with D measured between them."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_bars as B                                   # noqa: E402
import guidance_models as GM                            # noqa: E402
import guidance_ref as R                                # noqa: E402
from tam_gcn_amd import guidance, f2                    # noqa: E402
from tam_gcn_amd.models import ctrgcn as M              # noqa: E402

DEV = 'cuda:0'
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'guidance.npz')
FEATURE_BAR = 1e-4


class _general:
    """the general eval path (what TAMGCN_F2=0 selects)"""

    def __enter__(self):
        self.old = os.environ.get('TAMGCN_F2')
        os.environ['TAMGCN_F2'] = '0'

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ['TAMGCN_F2']
        else:
            os.environ['TAMGCN_F2'] = self.old


class _family:
    def __enter__(self):
        pass

    def __exit__(self, *exc):
        pass


def _model(tag):
    m = M.Model(**GM.CASES[tag][0])
    m.load_state_dict(GM.settled_state(tag)[0])
    return m.to(DEV).eval()


def _served_by_family(m, x):
    with torch.no_grad():
        return any(e is not None for e in (m._f2(x), m._f2v(x), m._f2j(x), m._f2g(x)))


def _np(t):
    return t.detach().double().cpu().numpy()


def _within(name, got, ref, bar):
    err = np.abs(_np(got) - ref)
    assert got.shape == ref.shape and np.all(err <= bar), f'{name}: {float(np.max(err / np.maximum(bar, 1e-300))):.3g} bars'


def _column_norm(a, b):
    """the largest L2 norm over channels of a - b, (N, C, T', V, M) each"""
    return float(np.sqrt(((a - b) ** 2).sum(1)).max())


def _run(tag, m, x, image):
    g = guidance.SkeletonGuidance(m, GM.TARGETS, GM.K, GM.FRAMES)
    with torch.no_grad():
        feat = m.extract_feature(x)[0]
    res = dict(feature=_np(feat), pooled=guidance.pooled_feature(m, x), I=guidance.joint_intensity(m, x), w=g.joint_weights(x),
               map=g.weight_map(x, image.shape[-2:]), out=g.apply(x, image))
    for k in ('pooled', 'I', 'w', 'map', 'out'):
        assert not res[k].requires_grad and res[k].dtype == torch.float32
    return res


def _check_own_features(tag, res, image):
    """(a): the stage bars, against guidance_ref of the model's own features"""
    f = res['feature']
    N, C, T, V, Mp = f.shape
    I = R.intensity(f)
    B.check(f'{tag}: joint_intensity', res['I'], torch.from_numpy(I), torch.from_numpy(I), C)
    B.check(f'{tag}: pooled_feature', res['pooled'], torch.from_numpy(R.pooled(f)), torch.from_numpy(np.abs(f).mean((2, 3, 4))), T * V * Mp)
    E = R.intensity_bar_max(I, C)
    assert R.conditioned(I) and R.persons_decided(I, E)
    w = R.joint_weights(I, GM.TARGETS, GM.K)
    dw = R.weights_bar(I, E)
    _within(f'{tag}: joint_weights', res['w'], w, dw)
    H = image.shape[2]
    mbar = R.map_bar(w, GM.FRAMES, H, dw)[:, None, :, None]
    wm = R.weight_map(w, GM.FRAMES, image.shape[-2:])
    _within(f'{tag}: weight_map', res['map'], wm, mbar)
    img = _np(image)
    _within(f'{tag}: apply', res['out'], img * wm, np.abs(img) * mbar + 2 * R.U * np.abs(img * wm))


def _check_against(tag, res, image, ref, what):
    """(b): against a reference whose features differ from the model's by a measured column norm D"""
    f, fr = res['feature'], ref['feature']
    assert np.abs(f - fr).max() <= FEATURE_BAR * np.abs(fr).max(), f'{tag}: features against {what}'
    D = _column_norm(f, fr)
    I = ref['I']
    E = R.intensity_bar_max(I, f.shape[1], extra=D)
    assert R.conditioned(I) and R.persons_decided(I, E), f'{tag}: the inputs do not meet the conditions'
    assert np.all(np.abs(_np(res['I']) - I) <= (f.shape[1] + 4) * R.U * I + D)
    dw = R.weights_bar(I, E)
    _within(f'{tag}: joint_weights against {what}', res['w'], ref['w'], dw)
    mbar = R.map_bar(ref['w'], GM.FRAMES, image.shape[2], dw)[:, None, :, None]
    _within(f'{tag}: weight_map against {what}', res['map'], ref['map'], mbar)
    img = _np(image)
    _within(f'{tag}: apply against {what}', res['out'], ref['out'], np.abs(img) * mbar + 2 * R.U * np.abs(ref['out']))
    return D, dw


@pytest.mark.parametrize('tag', list(GM.CASES))
def test_both_routes_against_the_oracle_and_each_other(tag):
    m, x, image = _model(tag), GM.clip(tag).to(DEV), GM.rgb(tag).to(DEV)
    ref = GM.reference(tag)
    family = _served_by_family(m, x)
    assert family == (tag != 'ucla_big')                                  # 33 clips: above F2_MAX_CLIPS, the general route
    assert f2.F2_MAX_CLIPS < 33
    got = {}
    for route, ctx in (('family', _family()), ('general', _general())):
        if route == 'family' and not family:
            continue
        with ctx:
            assert _served_by_family(m, x) == (route == 'family')
            res = got[route] = _run(tag, m, x, image)
        _check_own_features(f'{tag}/{route}', res, image)
        D, dw = _check_against(f'{tag}/{route}', res, image, ref, 'the fp64 oracle')
        print(f'\nguidance {tag}/{route}: feature column norm against the oracle {D:.3e}, weights bar {dw:.3e}, '
              f'max|dw| {float(np.abs(_np(res["w"]) - ref["w"]).max()):.3e}')
    if len(got) == 2:                                                     # the two routes, each other's reference
        a, b = got['family'], got['general']
        I = R.intensity(b['feature'])
        dw = R.weights_bar(I, R.intensity_bar_max(I, b['feature'].shape[1], extra=_column_norm(a['feature'], b['feature'])))
        _within(f'{tag}: routes', a['w'], _np(b['w']), 2 * dw)
        mbar = R.map_bar(_np(b['w']), GM.FRAMES, image.shape[2], 2 * dw)[:, None, :, None]
        _within(f'{tag}: routes, map', a['map'], _np(b['map']), mbar)


@pytest.mark.parametrize('tag,key', [('ucla_t52', 't52'), ('ucla_t128_one', 't128')])
def test_the_reference_recorded_maps(tag, key):
    gold = np.load(GOLD)
    x = GM.clip(tag)
    assert np.array_equal(x.numpy(), gold[f'{key}/x'])
    m = _model(tag)
    fix = gold[f'{key}/feature'].astype(np.float64)
    with torch.no_grad():
        f = _np(m.extract_feature(x.to(DEV))[0])
    assert np.abs(f - fix).max() <= FEATURE_BAR * np.abs(fix).max()
    I = R.intensity(fix)
    C = fix.shape[1]
    assert R.conditioned(I)
    dw = R.weights_bar(I, R.intensity_bar_max(I, C, extra=_column_norm(f, fix)))          # this side
    dw += R.weights_bar(I, R.intensity_bar_max(I, C)) + 16 * R.U * 255 / 127                # the reference's float32 steps
    w = R.joint_weights(I, GM.TARGETS, GM.K)
    g = guidance.SkeletonGuidance(m)                                      # the defaults are visual.py's
    H, W = gold[f'{key}/map'].shape
    wm = g.weight_map(x.to(DEV), (H, W))
    assert wm.shape == (1, 1, H, W)
    recorded = gold[f'{key}/map'].astype(np.float64)
    mbar = R.map_bar(w, 5, H, dw)[0][:, None]
    _within(f'{tag}: recorded map', wm[0, 0], recorded, mbar)
    # the image the reference multiplied (visual.py:87) is not stored (3 MB of noise): it is make_input of the stored shape and seed
    from params import make_input
    shape = tuple(int(v) for v in gold[f'{key}/rgb_shape'])
    assert shape == (1, 15, H, W) and int(gold[f'{key}/seeds'][1]) == GM.CASES[tag][3]
    image = make_input(shape[1:], seed=int(gold[f'{key}/seeds'][2]), lo=0.0, hi=1.0)[None]
    want = image.double().numpy() * recorded                              # rgb_weighted, from the reference's own map
    _within(f'{tag}: recorded map applied', g.apply(x.to(DEV), image.to(DEV)), want,
            image.double().numpy() * mbar + 2 * R.U * np.abs(want))


def _capture(fn, *static):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        fn(*static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn(*static)
    return graph, out


@pytest.mark.parametrize('route', ['family', 'general'])
def test_host_free_capturable_and_bit_reproducible(route):
    tag = 'ucla_t52'
    m = _model(tag)
    g = guidance.SkeletonGuidance(m)
    x, image = GM.clip(tag).to(DEV), GM.rgb(tag).to(DEV)
    x2 = (GM.clip(tag) * 0.7 + 0.1).to(DEV)
    image2 = (1 - GM.rgb(tag)).to(DEV)
    with (_family() if route == 'family' else _general()):
        assert _served_by_family(m, x) == (route == 'family')
        first = g.apply(x, image)
        assert torch.equal(first, g.apply(x, image))                      # two eager runs
        assert torch.equal(guidance.pooled_feature(m, x), guidance.pooled_feature(m, x))
        fresh = guidance.SkeletonGuidance(m)          # its host-to-device copy (the target joints) is in the constructor ...
        torch.cuda.set_sync_debug_mode('error')                           # a synchronising call inside raises
        try:
            again = fresh.apply(x, image)             # ... so its very first call already neither synchronises nor copies
            f = guidance.pooled_feature(m, x)
            I = guidance.joint_intensity(m, x)
            wm = g.weight_map(x, (7, 5))
        finally:
            torch.cuda.set_sync_debug_mode('default')
        assert torch.equal(first, again) and f.shape == (1, 256) and I.shape == (1, 13, 20, 1) and wm.shape == (1, 1, 7, 5)
        eager2 = g.apply(x2, image2)
        xs, rs = x.clone(), image.clone()
        graph, out = _capture(g.apply, xs, rs)
        graph.replay()
        assert torch.equal(out, first)
        xs.copy_(x2)
        rs.copy_(image2)
        graph.replay()
        assert torch.equal(out, eager2) and not torch.equal(out, first)


def test_train_mode_input_forms_and_refusals():
    tag = 'ucla_t52'
    m = _model(tag)
    g = guidance.SkeletonGuidance(m)
    x, image = GM.clip(tag).to(DEV), GM.rgb(tag).to(DEV)
    ref = g.joint_weights(x)
    x3 = x[..., 0].permute(0, 2, 3, 1).contiguous().view(1, 52, 60)       # the (N, T, V*C) form
    assert torch.equal(g.joint_weights(x3), ref)
    # train mode (the frozen backbone of the cross-modal trainer): works under no_grad semantics on the general path; with
    # BatchNorm momentum 0 the running statistics stay, so only batch statistics enter -- finite, same shapes, no autograd
    m.train()
    for b in m.modules():
        if isinstance(b, torch.nn.modules.batchnorm._BatchNorm):
            b.momentum = 0.0
    seen, real = [], m._block_stack
    m._block_stack = lambda inp: (seen.append(real(inp)), seen[-1])[1]      # the h this very call reduced
    f = guidance.pooled_feature(m, x)
    h = seen[-1][0].double().cpu()
    out = g.apply(x, image)
    del m._block_stack
    assert f.shape == (1, 256) and not f.requires_grad and bool(torch.isfinite(out).all())
    B.check('train mode: pooled_feature', f, h.mean((2, 3)), h.abs().mean((2, 3)), 13 * 20)
    m.eval()
    with pytest.raises(RuntimeError, match='requires grad'):
        guidance.pooled_feature(m, x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match='requires grad'):
        g.apply(x.clone().requires_grad_(True), image)
    with pytest.raises(RuntimeError, match='no CPU'):
        guidance.joint_intensity(m, x.cpu())
    with pytest.raises(ValueError):
        guidance.SkeletonGuidance(m, target_joints=(0, 1, 2, 3, 4, 5))     # 45 * 6 > 225
    from tam_gcn_amd.models import stgcn
    st = stgcn.Model(in_channels=3, num_class=10, num_point=20, num_person=1, graph='tam_gcn_amd.graph.ucla.Graph',
                     graph_args=dict(labeling_mode='spatial'))
    with pytest.raises(TypeError):
        guidance.pooled_feature(st.to(DEV).eval(), x)
    with pytest.raises(TypeError):
        guidance.SkeletonGuidance(st)
