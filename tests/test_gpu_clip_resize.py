"""-m gpu: the clip feeder's crop-and-resize mode (tam_gcn_amd/feeder/clip_feeder.py with p_interval=; csrc/clipfeeder.hip:
tamgcn_clip_crop_draw, tamgcn_clip_resize) against its numpy restatement (tests/clip_resize_ref.py).

The crop's integers and the drawn fp64 values are compared exactly; the device's fp32 matrix against the fp64 matrix of the same
angles within clip_resize_ref.rot_bound.  A batch is compared with the restatement fed the batch's own ``last_draws``, every
element within the bound derived in clip_resize_ref -- EPS (3 L D + 3 (|x0| + |x1|)) for the interpolation, carried through |R|
with three more roundings for the rotation -- and bit for bit where the arithmetic is exact: slots with L = W or L = 2 W and no
rotation, and the two-channel case, whose clips hold small integers and whose crops stand in a dyadic ratio to the window.  The
largest error met is printed as a fraction of the bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_feeder_ref as R0                                                         # noqa: E402
import clip_resize_ref as R                                                          # noqa: E402
from tam_gcn_amd import ops                                                          # noqa: E402
from tam_gcn_amd.feeder import clip_feeder as CF                                     # noqa: E402
from tam_gcn_amd.feeder.clip_feeder import Feeder                                    # noqa: E402
from tam_gcn_amd.feeder.feeder_nucla_gcn import GraphedBatch                         # noqa: E402

DEV = torch.device('cuda:0')
SEED_HI = 2 ** 32 + 12345                       # a seed whose high word is not zero
WINDOWS = (1, 8, 12, 16, 24)

# name -> ((C, T, V, M), [(begin, valid frames) | None = no valid frame], B, windows).  V M = 3: every 16-byte span crosses a
# frame; 10, 17, 50: some do, and source frames are 16-byte aligned on some frames only; W V M % 4 != 0 at W = 1 (and for V M =
# 17 at every W that is not a multiple of 4): the dword kernels.  The two-channel clips keep L in a dyadic ratio to every window.
CASES = {
    'vm3': ((3, 12, 3, 1), [(0, 12), (2, 8), (5, 2), (11, 1), (0, 6), None], 3, WINDOWS),
    'vm10': ((3, 13, 5, 2), [(0, 13), (3, 8), (6, 2), (0, 1), (1, 5), None], 3, WINDOWS),
    'c2': ((2, 12, 17, 1), [(0, 12), (3, 6), (4, 3), None, (6, 6), (9, 3)], 3, WINDOWS),
    'vm50': ((3, 12, 25, 2), [(0, 12), (1, 8), (7, 2), (4, 1), (0, 7), None], 3, WINDOWS),
    'ntu': ((3, 300, 25, 2), [(0, 300), (40, 128), (0, 64), (131, 19)], 2, (64,)),
}
_DATA = {}


def _data(name):
    if name not in _DATA:
        shape, layout, _, _ = CASES[name]
        rng = np.random.default_rng(sum(shape))
        if shape[0] == 2:
            x = rng.integers(-8, 9, size=(len(layout),) + shape).astype(np.float32)
            x[:, :, :, 0] = 1.0                                          # no frame inside the extent is all zero
        else:
            x = rng.uniform(-1.0, 1.0, size=(len(layout),) + shape).astype(np.float32)
        for i, span in enumerate(layout):
            begin, n = span if span is not None else (0, 0)
            x[i][:, :begin] = 0
            x[i][:, begin + n:] = 0
        _DATA[name] = x
    return _DATA[name]


def _extents(name):
    T = CASES[name][0][1]
    return np.array([(0, T) if s is None else (s[0], s[0] + s[1]) for s in CASES[name][1]], dtype=np.int64)


def _feeder(data, **kw):
    return Feeder(None, None, data=data, labels=np.arange(len(data)) * 3 + 1, device=DEV, **kw)


def _ids(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


def _flags(fd):
    return (R.CROP_RANDOM if len(fd.p_interval) == 2 else 0) | (R.ROT if fd.random_rot else 0)


def _check_draws(fd, ext, seed, call, what):
    """fd.last_draws against the restatement's draws for clips of extents ext; returns (crop, rot) as numpy."""
    flags = _flags(fd)
    wc, wd = R.crop_draws(seed, call, ext, flags, fd.p_interval[0], fd.p_interval[-1], fd.min_crop, fd.rot_theta)
    crop, drawn = fd.last_draws['crop'].cpu().numpy(), fd.last_draws['drawn'].cpu().numpy()
    assert crop.dtype == np.int32 and np.array_equal(crop, wc), (what, crop.tolist(), wc.tolist())
    assert drawn.dtype == np.float64 and np.array_equal(drawn.view(np.int64), wd.view(np.int64)), what
    rot = fd.last_draws['rot']
    if not flags & R.ROT:
        assert rot is None
        return crop, None
    rot = rot.cpu().numpy()
    assert rot.dtype == np.float32 and rot.shape == (len(ext), 3, 3)
    for b in range(len(ext)):
        R64 = R.rot_matrix(wd[b, 1:])
        assert (np.abs(rot[b].astype(np.float64) - R64) <= R.rot_bound(R64)).all(), f'{what}: rot of slot {b}'
    return crop, rot


def _check_batch(data, ids, W, out, crop, rot, what, exact_all=False):
    got = out.cpu().numpy()
    assert got.shape == (len(ids), data.shape[1], W, data.shape[3], data.shape[4]) and got.dtype == np.float32
    worst, n_exact = 0.0, 0
    for b, i in enumerate(ids):
        L = int(crop[b, 1])
        exact = exact_all or (rot is None and L in (W, 2 * W))
        want, bound = R.resize(data[i % len(data)], crop[b, 0], L, W, None if rot is None else rot[b])
        worst = max(worst, R.check(got[b], want, bound, f'{what} slot {b} (start, L) = {crop[b].tolist()}', exact=exact))
        n_exact += exact
    return worst, n_exact


def test_the_cases_cover_every_relation_of_crop_and_window():
    """With p_interval = [1.0] a slot's L is its clip's valid length: between them the three-channel cases meet every relation
    of L and W (the two exact ones included), and both kernel widths."""
    seen = set()
    for name, (shape, _, _, windows) in CASES.items():
        if shape[0] != 3:
            continue
        for W in windows:
            for L in np.diff(_extents(name), axis=1).ravel():
                seen |= {'L=1'} if L == 1 else set()
                seen.add('L=W' if L == W else 'L=2W' if L == 2 * W else 'L<W' if L < W else 'L>W')
    assert seen == {'L=1', 'L=W', 'L=2W', 'L<W', 'L>W'}
    assert {(W * 17) % 4 != 0 for W in WINDOWS} == {True, False} and (1 * 50) % 4 != 0 and (8 * 50) % 4 == 0


@pytest.mark.parametrize('min_crop', [1, 4, 64])
@pytest.mark.parametrize('T', [12, 300])
def test_crop_draws_exact(T, min_crop):
    """ops.clip_crop_draw on extents of every kind -- leading zero frames, no valid frame ((0, T)), one frame -- both interval
    forms, with and without the rotation, negative and over-range clip_ids, a call counter above 2^32."""
    rng = np.random.default_rng(T + min_crop)
    n_clips = 41
    begin = rng.integers(0, T, size=n_clips)
    end = begin + 1 + rng.integers(0, T - begin)
    begin[:3], end[:3] = (0, T - 1, 5), (T, T, 5 + min(64, T - 5))
    ext = np.stack([begin, end], axis=1).astype(np.int32)
    ids = rng.integers(-2 * n_clips, 3 * n_clips, size=70)
    ids[:5] = (0, 1, 2, -1, n_clips)
    labels = torch.arange(n_clips, dtype=torch.int64, device=DEV) * 3 + 1
    dext = torch.from_numpy(ext).to(DEV)
    for seed, call in ((0, 0), (SEED_HI, 2 ** 32 + 5)):
        for flags, p0, p1 in ((0, 1.0, 1.0), (0, 0.95, 0.95), (0, 0.5, 0.5), (R.ROT, 0.95, 0.95), (R.CROP_RANDOM, 0.5, 1.0),
                              (R.CROP_RANDOM | R.ROT, 0.5, 1.0), (R.CROP_RANDOM | R.ROT, 0.1, 0.2)):
            state = torch.tensor([seed, call], dtype=torch.int64, device=DEV)
            crop, drawn, rot, lab = ops.clip_crop_draw(dext, _ids(ids.tolist()), state, flags, p0, p1, min_crop, 0.3, labels=labels)
            clip = ids % n_clips
            wc, wd = R.crop_draws(seed, call, ext[clip], flags, p0, p1, min_crop, 0.3)
            assert crop.dtype == torch.int32 and np.array_equal(crop.cpu().numpy(), wc), (flags, p0)
            assert np.array_equal(drawn.cpu().numpy().view(np.int64), wd.view(np.int64)), (flags, p0)
            assert lab.tolist() == (clip * 3 + 1).tolist()
            assert (rot is None) == (not flags & R.ROT)
            if rot is not None:
                got = rot.cpu().numpy().astype(np.float64)
                want = np.stack([R.rot_matrix(a) for a in wd[:, 1:]])
                assert (np.abs(got - want) <= R.rot_bound(want)).all()
            assert state.tolist() == [seed, call + (1 if flags else 0)]        # advanced on the device iff something is drawn


MODES = [dict(p_interval=[1.0]), dict(p_interval=[0.95]), dict(p_interval=[0.5]), dict(p_interval=[0.5, 1], min_crop=1),
         dict(p_interval=[0.5, 1], min_crop=4, random_rot=True), dict(p_interval=[0.5, 1], random_rot=True),
         dict(p_interval=[1.0], random_rot=True, rot_theta=3.0)]


@pytest.mark.parametrize('name,W', [(n, W) for n, c in CASES.items() for W in c[3]])
def test_batch_device_against_the_restatement(name, W):
    data, ext = _data(name), _extents(name)
    (C, T, V, M), _, B, _ = CASES[name]
    assert [list(R0.extent(c)) for c in data] == ext.tolist()
    batches = [list(range(k, k + B)) for k in range(0, len(data), B)]
    batches[-1] = [i - 2 * len(data) if k % 2 else i + len(data) for k, i in enumerate(batches[-1])]       # negative, over-range
    worst, n_exact = 0.0, 0
    for mode in MODES:
        if C == 2 and (mode.get('random_rot') or (mode['p_interval'] != [1.0] and (mode.get('min_crop') != 1 or W not in (1, 8, 16)))):
            continue                                                     # two channels: L / W dyadic, so that the arithmetic is exact
        fd = _feeder(data, window_size=W, seed=SEED_HI, **mode)
        random = len(mode['p_interval']) == 2 or mode.get('random_rot', False)
        assert fd.train_val == ('train' if random else 'val') and fd.W == W
        for call, ids in enumerate(batches):
            out, lab = fd.batch_device(_ids(ids))
            assert lab.tolist() == [3 * (i % len(data)) + 1 for i in ids]
            what = f'{name} W={W} {mode} batch {call}'
            crop, rot = _check_draws(fd, ext[[i % len(data) for i in ids]], SEED_HI, call if random else 0, what)
            if C == 2 and len(mode['p_interval']) == 1:
                assert all(L in (12, 6, 3) for L in crop[:, 1].tolist())
            w, e = _check_batch(data, ids, W, out, crop, rot, what, exact_all=(C == 2))
            worst, n_exact = max(worst, w), n_exact + e
            assert fd.rng_state() == (SEED_HI, call + 1 if random else 0)
    print(f'{name} W={W}: worst element at {worst:.3f} of its bound, {n_exact} slots bit-equal')


def test_resize_clamps_any_crop_into_the_clip():
    """Whatever crop holds -- a start before or past the clip, L <= 0 or above T -- the frames read are the clip's own."""
    data = _data('vm50')
    crop = np.array([[-5, 4], [9, 40], [3, 0], [2 ** 31 - 1, 2 ** 31 - 1], [-2 ** 31, -2 ** 31], [11, 1]], dtype=np.int32)
    ids = list(range(6))
    raw = torch.from_numpy(data).to(DEV)
    for W in (8, 1):
        out = ops.clip_resize(raw, _ids(ids), torch.from_numpy(crop).to(DEV), W)
        _check_batch(data, ids, W, out, crop, None, f'clamp W={W}')


@pytest.mark.parametrize('stream', ['bone', 'motion', 'bone_motion'])
def test_streams_are_derived_last(stream):
    data, parent = _data('vm10'), [0, 0, 1, 1, 3]
    kw = dict(window_size=8, seed=21, p_interval=[0.5, 1], min_crop=2, random_rot=True)
    joint, fd = _feeder(data, **kw), _feeder(data, stream=stream, parent=parent, **kw)
    ids = [0, 1, 4, 2, -1]
    x, _ = joint.batch_device(_ids(ids))
    y, _ = fd.batch_device(_ids(ids))
    for k in ('crop', 'drawn', 'rot'):
        assert torch.equal(joint.last_draws[k], fd.last_draws[k])
    x, y = x.cpu().numpy(), y.cpu().numpy()
    assert np.array_equal(y, R0.stream(x, parent, stream)) and not np.array_equal(x, y)


def test_two_calls_give_the_same_bits_and_the_state_resumes():
    data = _data('vm50')
    fd = _feeder(data, window_size=8, seed=31, p_interval=[0.5, 1], min_crop=3, random_rot=True)
    v = _ids([2, 0, 3, 1, 1])
    outs = [fd.batch_device(v)[0].clone() for _ in range(3)]
    assert fd.rng_state() == (31, 3) and not torch.equal(outs[0], outs[1])
    fd.manual_seed(31)
    for want in outs:
        assert torch.equal(fd.batch_device(v)[0].view(torch.int32), want.view(torch.int32))
    resumed = _feeder(data, window_size=8, p_interval=[0.5, 1], min_crop=3, random_rot=True)
    resumed.set_rng_state((31, 1))
    assert torch.equal(resumed.batch_device(v)[0].view(torch.int32), outs[1].view(torch.int32)) and resumed.rng_state() == (31, 2)
    crop, rot = fd.last_draws['crop'], fd.last_draws['rot']
    a, b = (ops.clip_resize(fd._raw, v, crop, 8, rot) for _ in range(2))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(ValueError, match='int64'):
        fd.batch_device([0, 1])


def test_host_batch_draws_as_the_published_pipeline_does():
    """batch() under np.random.seed / torch.manual_seed: per sample np.random.rand(1), np.random.randint(0, valid - L + 1), then
    torch.zeros(3).uniform_(-theta, theta); the matrix in fp64 from the fp32 angles, rounded once; the same resize kernel."""
    data, ext = _data('vm50'), _extents('vm50')
    ids = [0, 1, 4, 5, 2]
    fd = _feeder(data, window_size=8, p_interval=[0.5, 1], min_crop=3, random_rot=True)
    np.random.seed(7)
    torch.manual_seed(7)
    out, lab, idx = fd.batch(ids)
    assert idx == ids and lab.tolist() == [3 * i + 1 for i in ids] and fd.rng_state() == (0, 0)
    np.random.seed(7)
    torch.manual_seed(7)
    crops, drawn, rots = [], [], []
    for i in ids:
        valid = int(ext[i, 1] - ext[i, 0])
        p = np.random.rand(1) * (1 - 0.5) + 0.5
        L = int(np.minimum(np.maximum(int(np.floor(valid * p[0])), 3), valid))
        bias = np.random.randint(0, valid - L + 1)
        ang = torch.zeros(3).uniform_(-0.3, 0.3)
        crops.append([ext[i, 0] + bias, L])
        drawn.append([float(p[0])] + [float(a) for a in ang])
        rots.append(R.rot_matrix(ang.double().numpy()).astype(np.float32))
    assert fd.last_draws['crop'].cpu().tolist() == crops
    assert np.array_equal(fd.last_draws['drawn'].cpu().numpy().view(np.int64), np.array(drawn).view(np.int64))
    rot = fd.last_draws['rot'].cpu().numpy()
    assert np.array_equal(rot.view(np.uint32), np.stack(rots).view(np.uint32))
    _check_batch(data, ids, 8, out, np.array(crops), rot, 'host batch')
    val = _feeder(data, window_size=8, p_interval=[0.95])                # nothing random: batch() and batch_device() agree
    a, b = val.batch(ids)[0], val.batch_device(_ids(ids))[0]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and val.last_draws['rot'] is None
    assert val.last_draws['crop'].cpu().tolist() == [[int(ext[i, 0]) + CF.crop_of(int(ext[i, 1] - ext[i, 0]), 0.95)[0],
                                                      CF.crop_of(int(ext[i, 1] - ext[i, 0]), 0.95)[1]] for i in ids]


def test_graphed_batch_replays_draw_anew():
    data, ext = _data('vm50'), _extents('vm50')
    kw = dict(window_size=8, seed=SEED_HI, p_interval=[0.5, 1], min_crop=2, random_rot=True)
    fg, fe = _feeder(data, **kw), _feeder(data, **kw)
    ids = [0, 1, 2, 3, 4, 5, -1]
    gb = GraphedBatch(fg, len(ids))
    assert fg.rng_state() == (SEED_HI, 0)                       # building it consumed no draws
    xs = []
    for call in range(3):
        x, y = gb(_ids(ids))
        ex, ey = fe.batch_device(_ids(ids))
        assert torch.equal(x.view(torch.int32), ex.view(torch.int32)) and torch.equal(y, ey)
        crop, rot = _check_draws(fg, ext[[i % 6 for i in ids]], SEED_HI, call, f'replay {call}')
        _check_batch(data, ids, 8, x, crop, rot, f'replay {call}')
        xs.append(x.clone())
    assert not torch.equal(xs[0], xs[1]) and not torch.equal(xs[1], xs[2])
    assert fg.rng_state() == (SEED_HI, 3) == fe.rng_state()
    fv = _feeder(data, window_size=8, p_interval=[0.95])         # nothing random: replays repeat, the counter stays
    gv = GraphedBatch(fv, 3)
    a = gv(_ids([0, 1, 3]))[0].clone()
    assert torch.equal(a.view(torch.int32), gv(_ids([0, 1, 3]))[0].view(torch.int32)) and fv.rng_state() == (0, 0)


TREE5 = dict(num_class=4, num_point=5, num_person=1, graph='tam_gcn_amd.graph.synthetic.Graph', graph_args=dict(num_node=5, arity=2))


def _tiny():
    rng = np.random.default_rng(29)
    data = rng.uniform(-1.0, 1.0, size=(5, 3, 20, 5, 1)).astype(np.float32)
    data[1][:, 14:] = 0
    return data, [3, 1, 0, 1, 2]


def test_captured_eval_takes_the_centre_crop_and_refuses_the_random_one():
    from params import fill_state_
    from tam_gcn_amd.evaluation import CapturedEval
    from tam_gcn_amd.models.ctrgcn import Model
    data, labels = _tiny()
    fd = Feeder(None, None, data=data, labels=labels, window_size=8, p_interval=[0.95], split='val', device=DEV)
    assert fd.train_val == 'val'
    m = Model(**TREE5)
    fill_state_(m.state_dict(), seed=0)
    m = m.to(DEV).eval()
    res = CapturedEval(m, fd, 2, topk=(1,)).run().compute()
    assert res['count'] == 5 and res['batches'] == 3 and res['bad_labels'] == 0 and res['bad_index'] == 0
    want = np.zeros((5, 4), dtype=np.float32)
    for idx in ([0, 1], [2, 3], [4, 0]):
        x, _, _ = fd.batch(idx)
        with torch.no_grad():
            want[idx[0]:idx[0] + 2] = m(x).cpu().numpy()[:5 - idx[0]]
    assert np.isfinite(want).all() and np.array_equal(res['scores'], want), float(np.abs(res['scores'] - want).max())
    for kw in (dict(p_interval=[0.5, 1], min_crop=4), dict(p_interval=[0.95], random_rot=True)):
        with pytest.raises(ValueError, match='train split'):
            CapturedEval(m, Feeder(None, None, data=data, labels=labels, window_size=8, device=DEV, **kw), 2)


def test_graphed_batch_feeds_captured_step():
    """A tiny CTR-GCN at (2, 3, 8, 5, 1) fed by GraphedBatch for two steps: finite losses, the counter moved twice."""
    from params import fill_state_, make_input, make_labels
    from tam_gcn_amd.distributed import ParamArena
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.models.ctrgcn import Model
    from tam_gcn_amd.optim import FusedSGD
    from tam_gcn_amd.training import CapturedStep
    data, labels = _tiny()
    m = Model(**TREE5)
    fill_state_(m.state_dict(), seed=0)
    m = m.to(DEV).train()
    arena = ParamArena(m)
    bucket = arena.grad_bucket()
    opt = FusedSGD(arena, bucket, lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4)
    fd = Feeder(None, None, data=data, labels=labels, window_size=8, p_interval=[0.5, 1], min_crop=4, random_rot=True, device=DEV, seed=2024)
    x0, y0 = make_input((2, 3, 8, 5, 1), 3).to(DEV), make_labels(2, 4, 103).to(DEV)
    train = CapturedStep(m, CrossEntropyLoss(), opt, arena, bucket, x0, y0)
    gb = GraphedBatch(fd, 2)
    losses = torch.stack([train.step(*gb(_ids(v))).clone() for v in ([0, 1], [4, 2])]).cpu()
    assert torch.isfinite(losses).all() and fd.rng_state() == (2024, 2), losses


@pytest.mark.parametrize('kw,match', [
    (dict(p_interval=[0.5, 1], window_size=-1), 'window_size'), (dict(p_interval=[0.5, 1], random_shift=True), 'excludes'),
    (dict(p_interval=[0.5, 1], random_choose=True), 'excludes'), (dict(p_interval=[0.95], random_move=True), 'excludes'),
    (dict(random_rot=True), 'needs p_interval'), (dict(p_interval=[0.5, 1], random_rot=True, data='c2'), 'three channels'),
    (dict(p_interval=[0.1, 0.5, 1]), 'p_interval'), (dict(p_interval=[0.0, 1]), 'p_interval'), (dict(p_interval=[0.6, 0.5]), 'p_interval'),
    (dict(p_interval=[0.5, 1.5]), 'p_interval'), (dict(p_interval=[0.5, 1], rot_theta=-0.1), 'rot_theta'),
    (dict(p_interval=[0.5, 1], rot_theta=float('nan')), 'rot_theta'), (dict(p_interval=[0.5, 1], min_crop=0), 'min_crop'),
    (dict(p_interval=[0.5, 1], min_crop=2.5), 'min_crop'),
])
def test_argument_rules(kw, match):
    kw = dict(window_size=8, **kw) if 'window_size' not in kw else dict(kw)
    data = _data(kw.pop('data', 'vm50'))
    with pytest.raises(ValueError, match=match):
        _feeder(data, **kw)
