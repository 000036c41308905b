"""-m gpu: the feeder's device-side train path -- tamgcn_feeder_draw against its numpy restatement (tests/feeder_draws.py)
bit for bit, the view matrix against view_matrix(), Feeder.batch_device against the feeder oracle fed the device's own
draws (<= 2e-6, the bar of tests/test_gpu_feeder.py's train path: the 3x3 product's fp64 summation order) and against
the host-draw kernel on the same draws (bit-identical: one device body), the val path against the reference's vectors
(bit-exact), slot independence, HIP graph capture (GraphedBatch), resuming the stream, and the captured batch feeding
CapturedStep."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import feeder_draws as FD                                                           # noqa: E402
from oracle import feeder_oracle as FO                                              # noqa: E402
from tam_gcn_amd import ops                                                         # noqa: E402
from tam_gcn_amd.feeder.feeder_nucla_gcn import Feeder, GraphedBatch, view_matrix   # noqa: E402

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'feeder.npz'))
PICKS = {'val': [0, 7, 123, 463], 'train': [0, 11, 500, 1019]}
DEV = torch.device('cuda:0')
TS = 52
SEED_HI = 2 ** 32 + 12345                       # a seed whose high word is not zero
STREAMS = [('train', None, 'joint'), ('train_bone', None, 'bone'), ('train_motion', None, 'motion'),
           ('train', 'bone_motion', 'bone_motion')]


def _dataset(tmp_path, split):
    dd = []
    for i in PICKS[split]:
        name = str(GOLD[f'{split}/{i}/name'])
        os.makedirs(tmp_path / name, exist_ok=True)
        with open(tmp_path / name / (name + '.json'), 'w') as f:
            json.dump({'skeletons': GOLD[f'{split}/{i}/raw'].tolist()}, f)
        dd.append({'file_name': name, 'label': int(GOLD[f'{split}/{i}/label']) + 1})
    return dd


def _synthetic(tmp_path, lengths, seed=11):
    """Seeded clips of the given lengths (a walk around a random pose, so that min and max differ per coordinate)."""
    rng = np.random.default_rng(seed)
    dd = []
    for k, n in enumerate(lengths):
        name = f'a{1 + k % 6:02d}_s{k:02d}_e00_v01'
        clip = rng.normal(size=(1, 20, 3)) + 0.05 * np.cumsum(rng.normal(size=(n, 20, 3)), axis=0)
        os.makedirs(tmp_path / name, exist_ok=True)
        with open(tmp_path / name / (name + '.json'), 'w') as f:
            json.dump({'skeletons': clip.tolist()}, f)
        dd.append({'file_name': name, 'label': 1 + k % 10})
    return dd


def _state(seed, call):
    return torch.tensor([seed, call], dtype=torch.int64, device=DEV)


def _cossin():
    import math
    return torch.tensor([[math.cos(math.radians(a)), math.sin(math.radians(a))] for a in range(-60, 61)],
                        dtype=torch.float64, device=DEV)


def _ragged_table(seed=5, n_clips=300):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 1001, size=n_clips)
    lens[:4] = (1, 1000, 2, 999)
    return lens, torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(DEV)


@pytest.mark.parametrize('seed', [0, SEED_HI])
@pytest.mark.parametrize('call', [0, 1, 2 ** 32 + 5])
@pytest.mark.parametrize('B', [1, 4, 256])
def test_draws_bit_for_bit(B, call, seed):
    lens, offsets = _ragged_table()
    n_clips = len(lens)
    rng = np.random.default_rng(B + 7)
    ids = rng.integers(0, 3 * n_clips, size=B)              # beyond n_clips: taken modulo, as batch() does for repeat
    ids[0] = 1                                              # the 1000-frame clip
    if B > 1:
        ids[1], ids[2], ids[3] = 0, n_clips + 1, -1         # a 1-frame clip; the modulo; Python's sign rule
    labels = torch.arange(n_clips, dtype=torch.int64, device=DEV) * 3 + 1
    state = _state(seed, call)
    view, rot, idx, lab = ops.feeder_draw(offsets, torch.from_numpy(ids).to(DEV), state, _cossin(), TS, True, labels=labels)
    clip = ids % n_clips
    agx, agy, s, want_idx, _ = FD.draws(seed, call, lens[clip], TS)
    view, idx = view.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(view[:, 0].astype(np.int64), agx) and np.array_equal(view[:, 0], agx.astype(np.float64))
    assert np.array_equal(view[:, 1].astype(np.int64), agy) and np.array_equal(view[:, 1], agy.astype(np.float64))
    assert np.array_equal(np.ascontiguousarray(view[:, 2]).view(np.int64), s.view(np.int64)), 's differs in its fp64 bits'
    assert idx.dtype == np.int32 and np.array_equal(idx, want_idx)
    assert lab.tolist() == (clip * 3 + 1).tolist()
    assert state.tolist() == [seed, call + 1]               # advanced on the device, after the draw read it
    # the view matrix: entries <= 1.5 in magnitude, from at most two products and one sum of fp64 values, each rounding
    # <= 2^-53 relative; 16 units in the last place of 1.5 is 3.6e-15
    want_rot = np.stack([view_matrix(int(x), int(y), float(z)) for x, y, z in zip(agx, agy, s)])
    err = float(np.abs(rot.cpu().numpy() - want_rot).max())
    assert err <= 4e-15, f'view matrix differs from view_matrix() by {err:.3e}'


def test_val_draws_are_numpy_linspace_and_the_identity():
    lens = np.arange(1, 4097)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(DEV)
    state = _state(9, 4)
    view, rot, idx, lab = ops.feeder_draw(offsets, torch.arange(4096, dtype=torch.int64, device=DEV), state, None, TS, False)
    assert lab is None
    idx = idx.cpu().numpy()
    for L in lens:
        assert np.array_equal(idx[L - 1], np.linspace(0, L - 1, TS).astype(int)), L
    assert torch.equal(view.cpu(), torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand(4096, 3))
    assert torch.equal(rot.cpu(), torch.eye(3, dtype=torch.float64).expand(4096, 3, 3))
    assert state.tolist() == [9, 4]                         # the val path consumes nothing of the stream


def _check_against_oracle_and_host_path(fd, raws, indices, stream):
    """batch_device's data <= 2e-6 of the oracle fed the device's own draws; bit-identical to tamgcn_feeder_transform given
    the same draws and a host-gathered copy of the same clips.  Returns the largest difference to the oracle."""
    n = len(raws)
    out, lab = fd.batch_device(torch.tensor(indices, dtype=torch.int64, device=DEV))
    view, rot, idx = (fd.last_draws[k] for k in ('view', 'rot', 'idx'))
    assert tuple(out.shape) == (len(indices), 3, TS, 20, 1) and out.dtype == torch.float32 and out.is_cuda
    assert lab.dtype == torch.int64 and lab.tolist() == [fd.label[i % n] for i in indices]
    v, ix, got = view.cpu().numpy(), idx.cpu().numpy(), out.cpu().numpy()
    worst = 0.0
    for b, i in enumerate(indices):
        raw = raws[i % n]
        assert ix[b].min() >= 0 and ix[b].max() < len(raw)
        want = FO.transform(raw, int(v[b, 0]), int(v[b, 1]), float(v[b, 2]), ix[b], stream)
        worst = max(worst, float(np.abs(got[b] - want).max()))
    assert worst <= 2e-6, f'{stream}: largest difference to the oracle {worst:.3e}'
    gathered = np.concatenate([raws[i % n] for i in indices], axis=0)
    offs = np.concatenate([[0], np.cumsum([len(raws[i % n]) for i in indices])]).astype(np.int64)
    host = ops.feeder_transform(torch.from_numpy(np.ascontiguousarray(gathered)).to(DEV), torch.from_numpy(offs).to(DEV),
                                rot, idx, fd._parent, 20, TS, 1, stream)
    assert torch.equal(host, out), f'{stream}: the indexed kernel and the gathered-copy kernel differ'
    return worst


@pytest.mark.parametrize('label_path,stream_arg,stream', STREAMS)
def test_batch_device_data(label_path, stream_arg, stream, tmp_path):
    dd = _dataset(tmp_path, 'train')
    fd = Feeder(str(tmp_path), label_path, data_dict=dd, stream=stream_arg, seed=77)
    assert fd.stream == stream
    raws = [GOLD[f'train/{i}/raw'] for i in PICKS['train']]
    worst = 0.0
    for indices in ([0, 1, 2, 3], [3, 3, 0, 6, 9, 1, 2, 4]):
        worst = max(worst, _check_against_oracle_and_host_path(fd, raws, indices, stream))
    print(f'{stream}: largest difference to the oracle {worst:.3e}')
    assert fd.rng_state() == (77, 2)


def test_batch_device_data_synthetic_clips(tmp_path):
    """Lengths the fixture does not have (1, 2 and 333 frames among them) and a batch wider than the split."""
    lengths = [1, 2, 17, 40, 200, 333, 52, 5, 64, 100, 3, 29]
    dd = _synthetic(tmp_path, lengths)
    fd = Feeder(str(tmp_path), 'train', data_dict=dd, seed=SEED_HI)
    raws = fd.data
    assert [len(r) for r in raws] == lengths
    rng = np.random.default_rng(2)
    worst = _check_against_oracle_and_host_path(fd, raws, rng.integers(0, 40, size=64).tolist(), 'joint')
    print(f'synthetic clips: largest difference to the oracle {worst:.3e}')


@pytest.mark.parametrize('label_path', ['val', 'val_bone', 'val_motion', 'val_bone_motion'])
def test_val_path_bit_exact(label_path, tmp_path):
    dd = _dataset(tmp_path, 'val')
    fd = Feeder(str(tmp_path), label_path, data_dict=dd)
    out, lab = fd.batch_device(torch.arange(4, dtype=torch.int64, device=DEV))
    host, host_lab, _ = fd.batch(range(4))
    assert torch.equal(out, host) and torch.equal(lab, host_lab)
    assert lab.tolist() == [int(GOLD[f'val/{i}/label']) for i in PICKS['val']]
    for k, i in enumerate(PICKS['val']):
        assert np.array_equal(out[k].cpu().numpy(), GOLD[f'{label_path}/{i}/data']), (label_path, i)
    assert fd.rng_state() == (0, 0)


def test_slots_not_neighbours(tmp_path):
    dd = _dataset(tmp_path, 'train')
    fd = Feeder(str(tmp_path), 'train', data_dict=dd, seed=5)

    def at_call_zero(indices):
        fd.manual_seed(5, 0)
        out, _ = fd.batch_device(torch.tensor(indices, dtype=torch.int64, device=DEV))
        return out.clone(), fd.last_draws['view'].clone()
    a, va = at_call_zero([0, 1, 2, 3])
    b, vb = at_call_zero([0, 3, 3, 3])
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])          # same clip, same slot, other neighbours
    assert torch.equal(va, vb)                                          # the view belongs to the slot
    for i, j in ((1, 2), (1, 3), (2, 3)):                               # one clip in three slots: three views
        assert not torch.equal(vb[i], vb[j]) and not torch.equal(b[i], b[j])
    c, _ = at_call_zero([0, 1, 2, 3])
    assert torch.equal(a, c)                                            # and the stream is reproducible


def test_graphed_batch_replays_equal_eager_calls(tmp_path):
    dd = _dataset(tmp_path, 'train')
    fg = Feeder(str(tmp_path), 'train', data_dict=dd, seed=SEED_HI)
    fe = Feeder(str(tmp_path), 'train', data_dict=dd, seed=SEED_HI)
    gb = GraphedBatch(fg, 8)                    # capture refuses a host synchronisation or a pageable upload
    assert fg.rng_state() == (SEED_HI, 0)       # building it consumed no draws
    vectors = [torch.tensor(v, dtype=torch.int64, device=DEV) for v in
               ([0, 1, 2, 3, 0, 1, 2, 3], [3, 3, 2, 9, 1, 0, 5, 6], [7, 2, 2, 1, 0, 0, 3, 4])]
    for v in vectors:
        x, y = gb(v)
        ex, ey = fe.batch_device(v)
        assert torch.equal(x, ex) and torch.equal(y, ey)
        for k in ('view', 'rot', 'idx'):
            assert torch.equal(fg.last_draws[k], fe.last_draws[k]), k
    assert fg.rng_state() == (SEED_HI, 3) and fe.rng_state() == (SEED_HI, 3)
    x1 = gb(vectors[0])[0].clone()
    x2 = gb(vectors[0])[0].clone()
    assert not torch.equal(x1, x2)              # the counter advanced on the device between the replays
    assert fg.rng_state() == (SEED_HI, 5)
    fg.manual_seed(424242)                      # after the capture: the graph reads the state on every replay
    fresh = Feeder(str(tmp_path), 'train', data_dict=dd, seed=424242)
    x, y = gb(vectors[1])
    ex, ey = fresh.batch_device(vectors[1])
    assert torch.equal(x, ex) and torch.equal(y, ey)
    with pytest.raises(ValueError, match='8 elements'):
        gb(vectors[0][:4])


def test_resume_and_seed_inside_capture(tmp_path):
    dd = _dataset(tmp_path, 'train')
    fd = Feeder(str(tmp_path), 'train', data_dict=dd, seed=31)
    v = torch.tensor([2, 0, 3, 1, 1], dtype=torch.int64, device=DEV)
    for _ in range(3):
        fd.batch_device(v)
    state = fd.rng_state()
    assert state == (31, 3)
    resumed = Feeder(str(tmp_path), 'train', data_dict=dd)
    resumed.set_rng_state(state)
    a, b = fd.batch_device(v)[0], resumed.batch_device(v)[0]
    assert torch.equal(a, b)
    assert resumed.rng_state() == (31, 4) and resumed.seed == 31
    scratch = torch.zeros(1, device=DEV)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='outside graph capture'):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            scratch.add_(1.0)
            fd.manual_seed(1)
    with pytest.raises(ValueError, match='int64'):
        fd.batch_device([0, 1])


def test_graphed_batch_feeds_captured_step(tmp_path):
    """train.step(*gb(idx)) for three steps == CapturedStep(eager=True) fed eager batch_device calls of a second Feeder
    with the same seed: losses bit for bit."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    from params import fill_state_, make_input, make_labels
    from tam_gcn_amd.models.ctrgcn import Model
    from tam_gcn_amd.distributed import ParamArena
    from tam_gcn_amd.optim import FusedSGD
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.training import CapturedStep
    dd = _dataset(tmp_path, 'train')
    x0, y0 = make_input((8, 3, TS, 20, 1), 3).to(DEV), make_labels(8, 10, 103).to(DEV)
    vectors = [torch.tensor(v, dtype=torch.int64, device=DEV) for v in
               ([0, 1, 2, 3, 3, 2, 1, 0], [1, 1, 2, 0, 3, 0, 2, 3], [3, 0, 0, 1, 2, 2, 1, 3])]
    losses = {}
    for mode in ('graph', 'eager'):
        m = Model(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
        fill_state_(m.state_dict(), seed=0)
        m = m.to(DEV).train()
        arena = ParamArena(m)
        bucket = arena.grad_bucket()
        opt = FusedSGD(arena, bucket, lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4)
        fd = Feeder(str(tmp_path), 'train', data_dict=dd, seed=2024)
        train = CapturedStep(m, CrossEntropyLoss(), opt, arena, bucket, x0, y0, eager=(mode == 'eager'))
        feed = GraphedBatch(fd, 8) if mode == 'graph' else fd.batch_device
        losses[mode] = torch.stack([train.step(*feed(v)).clone() for v in vectors]).cpu()
        assert fd.rng_state() == (2024, 3)
    assert torch.isfinite(losses['graph']).all()
    assert torch.equal(losses['graph'], losses['eager']), (losses['graph'], losses['eager'])
