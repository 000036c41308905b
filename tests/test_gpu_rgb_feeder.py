"""-m gpu: the RGB feeder (tam_gcn_amd/feeder/rgb_feeder.py, csrc/rgb/) against its numpy restatement (tests/rgb_feeder_ref.py)
and the reference's recorded outputs (tests/golden/rgb_feeder.npz).  Every comparison is exact: the resample is integer
arithmetic, a batch is a table lookup (and with row_scale one fp32 multiplication).  Nothing here imports PIL or reads the
reference."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import rgb_feeder_ref as R                                                           # noqa: E402
from tam_gcn_amd.crossmodal import ResNet_GCN_Attention                              # noqa: E402
from tam_gcn_amd.feeder import rgb_feeder as F                                       # noqa: E402
from tam_gcn_amd.feeder.clip_feeder import Feeder as ClipFeeder                      # noqa: E402
from tam_gcn_amd.feeder.feeder_nucla_gcn import GraphedBatch                         # noqa: E402
from tam_gcn_amd.models.ctrgcn import Model                                          # noqa: E402

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rgb_feeder.npz'))
DEV = torch.device('cuda:0')
SEED_HI = 2 ** 32 + 12345                       # a seed whose high word is not zero
UCLA = dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ids(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


def _random(seed, n, H, W):
    return np.random.RandomState(seed).randint(0, 256, size=(n, H, W, 3), dtype=np.uint8)


# ---- resize -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,H,W,S', [(1, 37, 53, 16), (1, 7, 9, 24), (2, 20, 24, 24), (2, 24, 20, 24), (2, 24, 24, 24), (1, 480, 640, 224),
                                     (3, 37, 53, 16)],
                         ids=['down7taps', 'up_clamped', 'h_skipped', 'v_skipped', 'both_skipped', '480x640', 'three_images'])
def test_resize_equals_the_restatement(n, H, W, S):
    src = _random(100 * H + W + n, n, H, W)
    got = F.resize(_dev(src), (S, S))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, S, S, 3)
    assert torch.equal(got.cpu(), torch.from_numpy(R.resize(src, S)))


def test_resize_rounds_the_ends_of_the_range_as_the_restatement_does():
    H, W, S = 37, 53, 16
    board = (((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2) * 255).astype(np.uint8)
    src = np.stack([np.full((H, W, 3), 255, dtype=np.uint8), np.zeros((H, W, 3), dtype=np.uint8), np.repeat(board[:, :, None], 3, axis=2)])
    want = R.resize(src, S)
    assert (want[0] == 255).all() and (want[1] == 0).all() and 0 < want[2].min() and want[2].max() < 255
    assert torch.equal(F.resize(_dev(src), (S, S)).cpu(), torch.from_numpy(want))
    up = np.ascontiguousarray(src[:, :7, :9])
    assert torch.equal(F.resize(_dev(up), (24, 24)).cpu(), torch.from_numpy(R.resize(up, 24)))


# ---- batch ------------------------------------------------------------------------------------------------------------------
def _batch_case(S, Fr, n, ids, flip=None, missing=None, mode=0, row_scale=None, seed=0):
    store, table = _random(seed + S, n, S, S), R.lut()
    args = (_dev(store), _ids(ids), _dev(table), Fr, None if flip is None else _dev(np.asarray(flip, dtype=np.int32)),
            None if missing is None else _dev(np.asarray(missing, dtype=np.uint8)), mode, None if row_scale is None else _dev(row_scale))
    got, lab = F.batch(*args)
    again, _ = F.batch(*args)
    assert lab is None and torch.equal(got, again)                                   # two calls are bit-equal
    want = R.batch(store, ids, table, Fr, flip, missing, mode, row_scale)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    return got.cpu(), torch.from_numpy(want)


def test_batch_at_the_model_size_with_flips_and_wrapped_ids():
    got, want = _batch_case(224, 5, 4, [5, 2, 2], flip=[1, 0, 1])                    # an id >= n, a repeated id
    assert torch.equal(got, want)
    assert torch.equal(got[:, :3], got[:, 12:15]) and not torch.equal(got[0], got[1])


@pytest.mark.parametrize('S', [6, 4, 1, 12], ids=['scalar6', 'vector4', 'scalar1', 'vector12'])
def test_batch_scalar_and_vector_forms(S):
    for flip in (None, [0, 1, 1, 0, 1]):
        got, want = _batch_case(S, 1, 3, [0, -1, 4, 1, 2], flip=flip)
        assert torch.equal(got, want)
    got, want = _batch_case(S, 3, 3, [2, 0], flip=[1, 0])
    assert torch.equal(got, want)


@pytest.mark.parametrize('S', [6, 8], ids=['scalar', 'vector'])
def test_batch_missing_modes_and_row_scale(S):
    missing, ids = [0, 1, 0], [1, 0, 2, 4]
    for mode in (0, 1):
        got, want = _batch_case(S, 2, 3, ids, flip=[1, 1, 0, 0], missing=missing, mode=mode)
        assert torch.equal(got, want)
        if mode == 0:
            assert not got[0].any() and not got[3].any() and got[1].any()
        else:
            assert torch.equal(got[0, :3], torch.from_numpy(R.lut()[:, 0])[:, None, None].expand(3, S, S))
    scale = np.random.RandomState(S).uniform(0.0, 1.0, size=(4, S)).astype(np.float32)
    scale[2, 1] = 0.0
    plain, _ = _batch_case(S, 2, 3, ids)
    got, want = _batch_case(S, 2, 3, ids, row_scale=scale)
    assert torch.equal(got, want) and torch.equal(got, plain * torch.from_numpy(scale)[:, None, :, None])
    got, want = _batch_case(S, 2, 3, ids, missing=missing, mode=0, row_scale=np.full((4, S), np.inf, dtype=np.float32))
    assert not got[0].any() and torch.isinf(got[1]).any()                             # zeros stay exact zeros


def test_batch_labels_ride_along():
    store, labels = _random(1, 3, 4, 4), torch.tensor([7, 8, 9], dtype=torch.int64, device=DEV)
    _, lab = F.batch(_dev(store), _ids([2, 0, 4, -1]), _dev(R.lut()), 1, labels=labels)
    assert lab.tolist() == [9, 7, 8, 9]


# ---- the feeder: draws --------------------------------------------------------------------------------------------------------
def _feeder(n=5, H=20, W=31, S=8, **kw):
    kw.setdefault('device', DEV)
    return F.RGBFeeder(_random(7, n, H, W), np.arange(n) * 2 + 1, size=S, **kw), R.resize(_random(7, n, H, W), S)


def test_batch_device_flips_equal_the_philox_restatement():
    fd, store = _feeder(temporal_rgb_frames=2, random_flip=True, seed=SEED_HI)
    assert torch.equal(fd._raw.cpu(), torch.from_numpy(store))
    ids = [0, 3, 3, 9, -2, 1, 4, 2, 0]
    fd.manual_seed(SEED_HI, 2 ** 32 + 5)                                             # a call counter whose high word is not zero
    for k in range(3):
        x, y = fd.batch_device(_ids(ids))
        want = R.flips(SEED_HI, 2 ** 32 + 5 + k, len(ids))
        assert torch.equal(fd.last_draws['flip'].cpu(), torch.from_numpy(want))
        assert torch.equal(x.cpu(), torch.from_numpy(R.batch(store, ids, R.lut(), 2, want)))
        assert y.tolist() == [(i % 5) * 2 + 1 for i in ids]
    assert fd.rng_state() == (SEED_HI, 2 ** 32 + 8)
    assert 0 < int(torch.from_numpy(R.flips(SEED_HI, 2 ** 32 + 5, 64)).sum()) < 64


@pytest.mark.parametrize('train,random_flip', [(True, True), (True, False), (False, True)])
def test_the_counter_moves_iff_train_and_random_flip(train, random_flip):
    fd, store = _feeder(train=train, random_flip=random_flip, seed=11)
    x, _ = fd.batch_device(_ids([1, 2]))
    drawn = train and random_flip
    assert fd.rng_state() == (11, 1 if drawn else 0) and fd.train_val == ('train' if drawn else 'val')
    assert (fd.last_draws['flip'] is not None) == drawn
    if not drawn:
        assert torch.equal(x.cpu(), torch.from_numpy(R.batch(store, [1, 2], R.lut(), 1)))
    state = fd.rng_state()
    a, _ = fd.batch_device(_ids([4, 0, 3]))
    fd.set_rng_state(state)
    b, _ = fd.batch_device(_ids([4, 0, 3]))
    assert torch.equal(a, b)


def test_host_batch_draws_as_the_reference_does_and_refusals():
    fd, store = _feeder(random_flip=True, random_crop=True)
    np.random.seed(3)
    x, y, idx = fd.batch([0, 6, 2, 2])
    np.random.seed(3)
    want = [1 if np.random.random() < 0.5 else 0 for _ in range(4)]
    assert idx == [0, 1, 2, 2] and fd.last_draws['flip'].tolist() == want and fd.rng_state() == (0, 0)
    assert torch.equal(x.cpu(), torch.from_numpy(R.batch(store, idx, R.lut(), 1, want)))
    with pytest.raises(ValueError, match='row_scale'):
        fd.batch_device(_ids([0]), row_scale=torch.ones(1, 8, device=DEV))
    with pytest.raises(ValueError, match='int64'):
        fd.batch_device([0, 1])
    plain, _ = _feeder()
    with pytest.raises(ValueError, match='row_scale'):
        plain.batch_device(_ids([0]), row_scale=torch.ones(2, 8, device=DEV))
    scratch = torch.zeros(1, device=DEV)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='outside graph capture'):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            scratch.add_(1.0)
            fd.manual_seed(1)
    assert fd.rng_state() == (0, 0)


def test_images_of_differing_sizes_are_grouped():
    rs = np.random.RandomState(2)
    shapes = [(20, 31), (8, 8), (20, 31), (5, 12), (8, 30), (1, 1)]
    images = [rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in shapes]
    missing = np.array([False] * 5 + [True])
    fd = F.RGBFeeder(images, [0, 1, 2, 3, 4, 5], size=8, missing=missing, missing_as='black', device=DEV)
    for i in range(5):
        assert torch.equal(fd._raw[i].cpu(), torch.from_numpy(R.resize(images[i], 8))), i
    x, _ = fd.batch_device(_ids([5, 1]))
    assert torch.equal(x[0].cpu(), torch.from_numpy(R.lut()[:, 0])[:, None, None].expand(3, 8, 8))


# ---- the fixture ------------------------------------------------------------------------------------------------------------
def test_feeder_equals_the_recorded_reference_outputs():
    Fr = int(GOLD['F'])
    for name in GOLD['names']:
        src, S = GOLD[f'{name}/src'], int(GOLD[f'{name}/size'])
        images = [src, np.zeros((1, 1, 3), dtype=np.uint8)]
        fd = F.RGBFeeder(images, [0, 1], size=S, temporal_rgb_frames=Fr, missing=np.array([False, True]), missing_as='zeros', device=DEV)
        assert torch.equal(fd._raw[0].cpu(), torch.from_numpy(GOLD[f'{name}/resized']))
        x, _ = fd.batch_device(_ids([0, 1]))
        assert tuple(x.shape) == (2, 3 * Fr, S, S)
        assert torch.equal(x[0].reshape(-1)[_ids(GOLD[f'{name}/idx'])].cpu(), torch.from_numpy(GOLD[f'{name}/sample'])), name
        assert bool(GOLD['absent/all_zero']) and not x[1].any()                      # tools.py:246
        one = F.RGBFeeder([src], [0], size=S, device=DEV)
        fl, _ = F.batch(one._raw, _ids([0]), one._lut, 1, flip=torch.ones(1, dtype=torch.int32, device=DEV))
        assert torch.equal(fl.reshape(-1)[_ids(GOLD[f'flip/{name}/idx'])].cpu(), torch.from_numpy(GOLD[f'flip/{name}/sample'])), name


# ---- fusion -----------------------------------------------------------------------------------------------------------------
def _clips(n, T=20, V=20):
    x = np.random.RandomState(4).uniform(-1.0, 1.0, size=(n, 3, T, V, 1)).astype(np.float32)
    x[:, :, :2] = 0
    x[:, :, T - 3:] = 0
    return x


def _fusion(n=6, S=28, Fr=5, seed=21):
    labels = np.arange(n) % 10
    mk = lambda: ClipFeeder(None, None, data=_clips(n), labels=labels, random_shift=True, random_choose=True, random_move=True,   # noqa: E731
                            window_size=16, device=DEV, seed=seed)
    rgb = F.RGBFeeder(_random(9, n, 30, 40), labels, size=S, temporal_rgb_frames=Fr, random_flip=True, seed=seed + 1, device=DEV)
    return F.FusionFeeder(mk(), rgb), mk()


def test_graphed_fusion_batch_equals_eager_and_the_skeleton_feeder_alone():
    fusion, alone = _fusion()
    B, ids = 4, [[5, 0, 7, 2], [1, 1, 3, -1]]
    fusion.skeleton.manual_seed(21, 3)
    fusion.rgb.manual_seed(22, 9)
    alone.manual_seed(21, 3)
    assert fusion.rng_state() == (21, 3, 22, 9)
    gb = GraphedBatch(fusion, B)                                                     # as it stands; consumes no draws of either
    assert fusion.rng_state() == (21, 3, 22, 9) and fusion.skeleton.rng_state() == (21, 3) and fusion.rgb.rng_state() == (22, 9)
    replays = []
    for k in range(2):
        (xg, xr), y = gb(_ids(ids[k]))
        replays.append((xg.clone(), xr.clone(), y.clone(), fusion.last_draws['rgb']['flip'].clone()))
    assert fusion.rng_state() == (21, 5, 22, 11)
    fusion.set_rng_state((21, 3, 22, 9))
    for k in range(2):
        (xg, xr), y = fusion.batch_device(_ids(ids[k]))
        sk, ys = alone.batch_device(_ids(ids[k]))
        assert torch.equal(xg, replays[k][0]) and torch.equal(xr, replays[k][1]) and torch.equal(y, replays[k][2])
        assert torch.equal(xg, sk) and torch.equal(y, ys)                            # the skeleton half: the skeleton feeder alone
        flip = R.flips(22, 9 + k, B)
        assert torch.equal(replays[k][3].cpu(), torch.from_numpy(flip))
        assert torch.equal(xr.cpu(), torch.from_numpy(R.batch(fusion.rgb._raw.cpu().numpy(), ids[k], R.lut(), 5, flip)))
    assert not torch.equal(replays[0][0], replays[1][0])
    (xg, xr), y = fusion.batch([0, 1])
    assert tuple(xg.shape) == (2, 3, 16, 20, 1) and tuple(xr.shape) == (2, 15, 28, 28) and y.tolist() == [0, 1]


def test_fusion_refuses_feeders_that_do_not_match():
    fusion, alone = _fusion()
    short = F.RGBFeeder(_random(9, 5, 8, 8), np.arange(5), size=8, device=DEV)
    with pytest.raises(ValueError, match='samples'):
        F.FusionFeeder(alone, short)
    other = F.RGBFeeder(_random(9, 6, 8, 8), np.arange(6)[::-1].copy(), size=8, device=DEV)
    with pytest.raises(ValueError, match='labels'):
        F.FusionFeeder(alone, other)
    with pytest.raises(TypeError):
        F.FusionFeeder(alone, alone)


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_cross_modal_model_trains_on_a_fusion_batch():
    torch.manual_seed(5)
    fusion, _ = _fusion()
    trunk = nn.Conv2d(15, 8, 4, stride=4)                                            # 28 x 28 -> a 7 x 7 map of 8 channels
    model = ResNet_GCN_Attention(Model(**UCLA), trunk, num_class=10, gcn_dim=256, rgb_dim=8, freeze_gcn=False).to(DEV).train()
    (x_gcn, x_rgb), y = fusion.batch_device(_ids([0, 3]))
    logits = model(x_gcn, x_rgb)
    assert tuple(logits.shape) == (2, 10) and torch.isfinite(logits).all()
    nn.functional.cross_entropy(logits, y).backward()
    for k, p in model.named_parameters():
        if k.startswith('gcn.'):                                  # the CTR-GCN's own classifier is not on the path: no gradient there
            assert p.grad is None or torch.isfinite(p.grad).all(), k
        else:                                                     # gradients reach the trunk and the head
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert float(model.resnet.weight.grad.abs().max()) > 0
    assert any(p.grad is not None and float(p.grad.abs().max()) > 0 for p in model.gcn.parameters())
