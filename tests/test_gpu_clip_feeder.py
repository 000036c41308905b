"""-m gpu: the clip feeder (tam_gcn_amd/feeder/clip_feeder.py, csrc/clipfeeder.hip) against its numpy restatement
(tests/clip_feeder_ref.py) and the reference's recorded outputs (tests/golden/clip_feeder.npz).

Extents and draws are compared exactly.  A batch is compared with the restatement fed the batch's own ``last_draws``: copied and
zero elements bit for bit, a moved element r within

    |dev - r| <= 2^-24 |r| + MOVE_ULPS 2^-53 ((|x| + |y|) |s| + |t|),     MOVE_ULPS = 12.

The first term is the one fp32 rounding of the result.  The second was proposed with the constant 8; the derivation written out
at clip_feeder_ref.MOVE_ULPS gives 11 -- per side the cos / sin error (1 ulp on the host, 2 on the device), the roundings of
cos.s / sin.s, of the two products, of their sum and of the final addition: 5 + 6 -- and one more for the second-order terms, so
the derived 12 is what is asserted.  The largest error met is printed as a fraction of that bound."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_feeder_ref as R                                                          # noqa: E402
from tam_gcn_amd import ops                                                          # noqa: E402
from tam_gcn_amd.feeder.clip_feeder import Feeder                                    # noqa: E402
from tam_gcn_amd.feeder.feeder_nucla_gcn import GraphedBatch                         # noqa: E402

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'clip_feeder.npz'))
CASES = [tuple(int(v) for v in row) for row in GOLD['cases']]
DEV = torch.device('cuda:0')
SEED_HI = 2 ** 32 + 12345                       # a seed whose high word is not zero
A, B_ = GOLD['A/clips'], GOLD['B/clips']        # (5, 3, 12, 5, 2) and (5, 2, 7, 3, 1): zero borders, none, all zeros, -0.0, NaN
PARENT5 = [0, 0, 1, 1, 3]
IDS = [0, 1, 2, 3, 4, 4, -1, 7, -6, 12, 3]      # repeated, negative, >= n_clips
CAND = R.default_candidates()
_NTU = {}


def _ntu():
    """Three (3, 300, 25, 2) clips: a 40-frame lead-in and a zero tail, no zero frame, a short island."""
    if not _NTU:
        rng = np.random.default_rng(3)
        x = rng.uniform(-1.0, 1.0, size=(3, 3, 300, 25, 2)).astype(np.float32)
        x[0][:, :40] = 0
        x[0][:, 221:] = 0
        x[2][:, :131] = 0
        x[2][:, 150:] = 0
        _NTU['x'] = x
    return _NTU['x']


def _feeder(data, flags=0, **kw):
    return Feeder(None, None, data=data, labels=np.arange(len(data)) * 3 + 1, random_shift=bool(flags & 1),
                  random_choose=bool(flags & 2), random_move=bool(flags & 4), device=DEV, **kw)


def _ids(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


def _keys(move):
    return np.stack([c[move[..., q]] for q, c in enumerate((CAND[0], CAND[1], CAND[2], CAND[2]))], axis=-1)


def _check_batch(fd, data, ids, out, what):
    """out (joint stream) against the restatement fed fd.last_draws; returns the worst error / bound ratio."""
    draws = {k: (None if v is None else v.cpu().numpy()) for k, v in fd.last_draws.items()}
    got = out.cpu().numpy()
    assert got.shape == (len(ids), data.shape[1], fd.W, data.shape[3], data.shape[4]) and got.dtype == np.float32
    node = R.node_table(fd.W, fd.move_time) if fd.random_move else None
    worst = 0.0
    for b, i in enumerate(ids):
        keys = _keys(draws['move'][b]) if fd.random_move else None
        want, bound = R.apply(data[i % len(data)], draws['plan'][b], fd.W, node, keys)
        worst = max(worst, R.check(got[b], want, bound, f'{what} slot {b}'))
    return worst


@pytest.mark.parametrize('name', ['A', 'B', 'ntu'])
def test_extent_exact(name):
    data = {'A': A, 'B': B_}.get(name)
    data = _ntu() if data is None else data                  # B: T V M = 21, the scalar path; the others read 16 bytes
    ext = ops.clip_extent(torch.from_numpy(data).to(DEV))
    assert ext.dtype == torch.int32 and ext.cpu().tolist() == [list(R.extent(c)) for c in data]
    if name == 'A':
        assert ext.cpu().tolist() == [[3, 10], [0, 12], [0, 12], [1, 10], [6, 8]]
    if name == 'ntu':
        assert ext.cpu().tolist() == [[40, 221], [0, 300], [131, 150]]


@pytest.mark.parametrize('flags', range(8))
@pytest.mark.parametrize('T,W,mt', [(12, 8, 1), (12, 16, 3), (12, 12, 1), (7, 1, 3), (300, 64, 8)])
def test_draws_exact(T, W, mt, flags):
    rng = np.random.default_rng(T + W)
    n_clips = 37
    begin = rng.integers(0, T, size=n_clips)
    end = begin + 1 + rng.integers(0, T - begin)
    begin[:2], end[:2] = (0, T - 1), (T, T)                   # size T: bias has one value; size 1: the widest range
    ext = np.stack([begin, end], axis=1).astype(np.int32)
    ids = rng.integers(-2 * n_clips, 3 * n_clips, size=70)
    ids[:4] = (0, 1, 1, -1)
    node = R.node_table(W, mt)
    cand = tuple(torch.from_numpy(c).to(DEV) for c in CAND)
    labels = torch.arange(n_clips, dtype=torch.int64, device=DEV) * 3 + 1
    for seed, call in ((0, 0), (SEED_HI, 2 ** 32 + 5)):
        state = torch.tensor([seed, call], dtype=torch.int64, device=DEV)
        plan, shift, move, keys, lab = ops.clip_draw(torch.from_numpy(ext).to(DEV), _ids(ids.tolist()), state, flags, T, W, len(node),
                                                     cand if flags & 4 else None, labels=labels)
        clip = ids % n_clips
        wp, ws, wm = R.device_draws(seed, call, ext[clip], T, W, flags, len(node), tuple(len(c) for c in CAND))
        assert plan.dtype == torch.int32 and np.array_equal(plan.cpu().numpy(), wp)
        assert np.array_equal(shift.cpu().numpy(), ws)
        assert lab.tolist() == (clip * 3 + 1).tolist()
        if flags & 4:
            assert move.dtype == torch.int32 and np.array_equal(move.cpu().numpy(), wm)
            assert np.array_equal(keys.cpu().numpy().view(np.int64), _keys(wm).view(np.int64))
        else:
            assert move is None and keys is None
        assert state.tolist() == [seed, call + (1 if flags else 0)]        # advanced on the device iff a flag is set


@pytest.mark.parametrize('flags', range(8))
@pytest.mark.parametrize('ws', [8, 12, 16, -1])
def test_batch_device_small_clips(ws, flags):
    worst = 0.0
    for mt in (1, 3):
        fd = _feeder(A, flags, window_size=ws, move_time=mt, seed=SEED_HI)
        assert fd.train_val == ('train' if flags else 'val') and fd.W == (ws if ws > 0 else 12) and len(fd) == 5
        for call in range(2):
            out, lab = fd.batch_device(_ids(IDS))
            assert lab.tolist() == [3 * (i % 5) + 1 for i in IDS]
            ext = np.array([R.extent(A[i % 5]) for i in IDS])
            wp, wsft, wm = R.device_draws(SEED_HI, call, ext, 12, fd.W, flags, len(fd.node), tuple(len(c) for c in CAND))
            assert np.array_equal(fd.last_draws['plan'].cpu().numpy(), wp) and np.array_equal(fd.last_draws['shift'].cpu().numpy(), wsft)
            assert (fd.last_draws['move'] is None) if wm is None else np.array_equal(fd.last_draws['move'].cpu().numpy(), wm)
            worst = max(worst, _check_batch(fd, A, IDS, out, f'W={ws} flags={flags} move_time={mt}'))
            assert fd.rng_state() == (SEED_HI, (call + 1) if flags else 0)
        fd.manual_seed(SEED_HI, 1)                                       # the same state: the same bits
        again, _ = fd.batch_device(_ids(IDS))
        assert torch.equal(again.view(torch.int32), out.view(torch.int32))
    print(f'W={ws} flags={flags}: worst moved element at {worst:.3f} of its bound')


@pytest.mark.parametrize('flags', range(8))
def test_batch_device_one_frame_window(flags):
    """(C, T, V, M) = (2, 7, 3, 1), W = 1: rows of 3 floats (the scalar kernels), move_time 3 with empty segments."""
    for mt in (1, 3):
        fd = _feeder(B_, flags, window_size=1, move_time=mt, seed=9)
        out, _ = fd.batch_device(_ids(IDS))
        _check_batch(fd, B_, IDS, out, f'W=1 flags={flags} move_time={mt}')


@pytest.mark.parametrize('ws', [100, 99, 21])
def test_batch_device_many_frames_per_tile(ws):
    """V M = 3: a tile of 1024 (W = 100, 16-byte accesses) or 256 (W = 99, scalar) elements spans more than the 64 frames whose
    move parameters the transform stages in LDS, so they are computed per thread; W = 21 is staged and ends inside a tile.  T = 7
    is padded to W at a drawn position."""
    for flags, mt in ((7, 3), (6, 8), (4, 1)):
        fd = _feeder(B_, flags, window_size=ws, move_time=mt, seed=13)
        out, _ = fd.batch_device(_ids(IDS))
        _check_batch(fd, B_, IDS, out, f'W={ws} flags={flags} move_time={mt}')
        assert np.array_equal(fd.last_draws['plan'].cpu().numpy(),
                              R.device_draws(13, 0, np.array([R.extent(B_[i % 5]) for i in IDS]), 7, ws, flags, len(fd.node), (68, 3, 5))[0])


@pytest.mark.parametrize('flags', [0, 7])
def test_batch_device_ntu_shape(flags):
    data = _ntu()
    fd = _feeder(data, flags, window_size=64, seed=4)
    ids = [2, 0, 1, 5, -1]
    out, lab = fd.batch_device(_ids(ids))
    assert tuple(out.shape) == (5, 3, 64, 25, 2) and lab.tolist() == [7, 1, 4, 7, 7]
    worst = _check_batch(fd, data, ids, out, f'ntu flags={flags}')
    print(f'ntu flags={flags}: worst moved element at {worst:.3f} of its bound')


@pytest.mark.parametrize('stream', ['bone', 'motion', 'bone_motion'])
def test_streams_are_derived_last(stream):
    joint = _feeder(A, 7, window_size=8, seed=21)
    fd = _feeder(A, 7, window_size=8, seed=21, stream=stream, parent=PARENT5)
    x, _ = joint.batch_device(_ids(IDS))
    y, _ = fd.batch_device(_ids(IDS))
    for k in ('plan', 'shift', 'move'):
        assert torch.equal(joint.last_draws[k], fd.last_draws[k])
    x, y = x.cpu().numpy(), y.cpu().numpy()
    want = R.stream(x, PARENT5, stream)
    keep = ~np.isnan(want)
    assert np.array_equal(np.isnan(y), ~keep) and np.array_equal(y[keep], want[keep])
    assert not np.array_equal(x[keep], y[keep])


_HOST = {}


@pytest.mark.parametrize('k', range(len(CASES)))
def test_host_batch_against_the_reference(k):
    """batch() under random.seed / np.random.seed: the reference's draws, and its outputs within the bound."""
    s, j, ws, flags, mt, seed = CASES[k]
    data = GOLD[f'{chr(s)}/clips']
    key = (s, ws, flags, mt)
    if key not in _HOST:
        _HOST[key] = _feeder(data, flags, window_size=ws, move_time=mt)
    fd = _HOST[key]
    random.seed(seed)
    np.random.seed(seed)
    out, lab, idx = fd.batch([j])
    assert idx == [j] and lab.tolist() == [3 * j + 1] and fd.rng_state() == (0, 0)
    assert fd.last_draws['shift'].cpu().numpy().tolist() == [GOLD[f'case{k}/shift'].tolist()]
    node = keys = None
    if flags & 4:
        assert np.array_equal(fd.last_draws['move'].cpu().numpy()[0], GOLD[f'case{k}/move'])
        node, keys = R.node_table(fd.W, mt), _keys(GOLD[f'case{k}/move'])
    _, bound = R.apply(data[j], fd.last_draws['plan'].cpu().numpy()[0], fd.W, node, keys)
    ratio = R.check(out.cpu().numpy()[0], GOLD[f'case{k}/out'], bound, f'case {k}')
    print(f'case {k}: worst moved element at {ratio:.3f} of its bound')


def test_graphed_batch_replays_draw_anew():
    fg, fe = (_feeder(A, 7, window_size=8, move_time=3, seed=SEED_HI) for _ in range(2))
    gb = GraphedBatch(fg, len(IDS))
    assert fg.rng_state() == (SEED_HI, 0)                       # building it consumed no draws
    ext = np.array([R.extent(A[i % 5]) for i in IDS])
    xs = []
    for call in range(2):
        x, y = gb(_ids(IDS))
        ex, ey = fe.batch_device(_ids(IDS))
        assert torch.equal(x.view(torch.int32), ex.view(torch.int32)) and torch.equal(y, ey)
        wp, ws, wm = R.device_draws(SEED_HI, call, ext, 12, 8, 7, len(fg.node), tuple(len(c) for c in CAND))
        for name, want in (('plan', wp), ('shift', ws), ('move', wm)):
            assert np.array_equal(fg.last_draws[name].cpu().numpy(), want), (call, name)
        _check_batch(fg, A, IDS, x, f'replay {call}')
        xs.append(x.clone())
    assert not torch.equal(xs[0].view(torch.int32), xs[1].view(torch.int32))
    assert fg.rng_state() == (SEED_HI, 2) == fe.rng_state()
    fv = _feeder(A, 0, window_size=8)                            # no random flag: replays repeat, the counter stays
    gv = GraphedBatch(fv, 3)
    a = gv(_ids([0, 1, 3]))[0].clone()
    assert torch.equal(a.view(torch.int32), gv(_ids([0, 1, 3]))[0].view(torch.int32)) and fv.rng_state() == (0, 0)


def test_resume_and_argument_checks():
    fd = _feeder(A, 7, window_size=8, seed=31)
    v = _ids([2, 0, 3, 1, 1])
    for _ in range(3):
        fd.batch_device(v)
    state = fd.rng_state()
    assert state == (31, 3)
    resumed = _feeder(A, 7, window_size=8)
    resumed.set_rng_state(state)
    assert torch.equal(fd.batch_device(v)[0].view(torch.int32), resumed.batch_device(v)[0].view(torch.int32))
    assert resumed.rng_state() == (31, 4) and resumed.seed == 31
    with pytest.raises(ValueError, match='int64'):
        fd.batch_device([0, 1])
    with pytest.raises(ValueError, match='int64'):
        fd.batch_device(torch.zeros(2, dtype=torch.int32, device=DEV))


def test_loads_the_data_tools_files(tmp_path):
    """data_path a .npy (memory-mapped or not, fp64 on disk converted to fp32), label_path a .pkl of (names, labels) or a .npy;
    debug keeps the first 100 samples; __getitem__ and top_k as on the reference's feeders."""
    import pickle
    np.save(tmp_path / 'data.npy', A.astype(np.float64))
    names, labels = [f'S{k:03d}' for k in range(5)], [4, 0, 2, 2, 1]
    with open(tmp_path / 'label.pkl', 'wb') as f:
        pickle.dump((names, labels), f)
    np.save(tmp_path / 'label.npy', np.array(labels))
    want = _feeder(A, 0, window_size=8).batch(range(5))[0]
    for label_path, use_mmap in (('label.pkl', True), ('label.pkl', False), ('label.npy', True)):
        fd = Feeder(str(tmp_path / 'data.npy'), str(tmp_path / label_path), window_size=8, use_mmap=use_mmap, split='test', device=DEV)
        assert len(fd) == 5 and fd.label == labels and fd.split == 'test' and fd._raw.dtype == torch.float32
        assert fd.sample_name == (names if label_path.endswith('.pkl') else [str(k) for k in range(5)])
        out, lab, idx = fd.batch(range(5))
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)) and lab.tolist() == labels and idx == [0, 1, 2, 3, 4]
    sample, label, index = fd[6]                                      # taken modulo the split's size
    assert index == 1 and label == 0 and np.array_equal(sample, want[1].cpu().numpy())
    score = np.eye(5)[labels]
    score[0] = [1, 0, 0, 0, 0.5]                                       # sample 0: label 4 is second
    assert fd.top_k(score, 1) == 0.8 and fd.top_k(score, 2) == 1.0
    big = np.zeros((103, 2, 4, 3, 1), dtype=np.float32)
    assert len(Feeder(None, None, data=big, labels=np.arange(103), debug=True, device=DEV)) == 100
    assert Feeder(None, None, data=A, labels=labels, normalization=True, device=DEV).train_val == 'val'


COCO = dict(num_class=10, num_point=17, num_person=1, graph='tam_gcn_amd.graph.coco.Graph', graph_args=dict(labeling_mode='spatial'))


def test_captured_eval_runs_on_a_clip_feeder():
    """A 17-joint model over a deterministic clip feeder of 5 clips, B = 2: the scores are the model's eager logits on
    feeder.batch() of the same padded batches, bit for bit (the last batch is padded with sample 0, as CapturedEval does)."""
    from params import fill_state_
    from tam_gcn_amd.evaluation import CapturedEval
    from tam_gcn_amd.models.ctrgcn import Model
    rng = np.random.default_rng(17)
    data = rng.uniform(-1.0, 1.0, size=(5, 3, 20, 17, 1)).astype(np.float32)
    data[1][:, 12:] = 0
    fd = Feeder(None, None, data=data, labels=[3, 1, 4, 1, 5], window_size=16, split='val', device=DEV)
    assert fd.train_val == 'val'
    m = Model(**COCO)
    fill_state_(m.state_dict(), seed=0)
    m = m.to(DEV).eval()
    res = CapturedEval(m, fd, 2, topk=(1,)).run().compute()
    assert res['count'] == 5 and res['batches'] == 3 and res['bad_labels'] == 0 and res['bad_index'] == 0
    want = np.zeros((5, 10), dtype=np.float32)
    for idx in ([0, 1], [2, 3], [4, 0]):
        x, _, _ = fd.batch(idx)
        with torch.no_grad():
            want[idx[0]:idx[0] + 2] = m(x).cpu().numpy()[:5 - idx[0]]
    assert np.isfinite(want).all() and np.array_equal(res['scores'], want), float(np.abs(res['scores'] - want).max())
    with pytest.raises(ValueError, match='train split'):
        CapturedEval(m, _feeder(data, 2, window_size=16), 2)


def test_graphed_batch_feeds_captured_step():
    """train.step(*gb(idx)) for two steps == CapturedStep(eager=True) fed eager batch_device calls of a second feeder with
    the same seed: losses bit for bit."""
    from params import fill_state_, make_input, make_labels
    from tam_gcn_amd.distributed import ParamArena
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.models.ctrgcn import Model
    from tam_gcn_amd.optim import FusedSGD
    from tam_gcn_amd.training import CapturedStep
    rng = np.random.default_rng(23)
    data = rng.uniform(-1.0, 1.0, size=(6, 3, 24, 20, 1)).astype(np.float32)
    data[0][:, :5] = 0
    labels = [0, 3, 9, 2, 2, 7]
    x0, y0 = make_input((8, 3, 16, 20, 1), 3).to(DEV), make_labels(8, 10, 103).to(DEV)
    vectors = [_ids(v) for v in ([0, 1, 2, 3, 4, 5, 1, 0], [5, 5, 2, 0, 3, 0, 2, 4])]
    losses = {}
    for mode in ('graph', 'eager'):
        m = Model(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
        fill_state_(m.state_dict(), seed=0)
        m = m.to(DEV).train()
        arena = ParamArena(m)
        bucket = arena.grad_bucket()
        opt = FusedSGD(arena, bucket, lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4)
        fd = Feeder(None, None, data=data, labels=labels, random_shift=True, random_choose=True, random_move=True, window_size=16,
                    device=DEV, seed=2024)
        train = CapturedStep(m, CrossEntropyLoss(), opt, arena, bucket, x0, y0, eager=(mode == 'eager'))
        feed = GraphedBatch(fd, 8) if mode == 'graph' else fd.batch_device
        losses[mode] = torch.stack([train.step(*feed(v)).clone() for v in vectors]).cpu()
        assert fd.rng_state() == (2024, 2)
    assert torch.isfinite(losses['graph']).all()
    assert torch.equal(losses['graph'], losses['eager']), (losses['graph'], losses['eager'])
