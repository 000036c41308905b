"""-m gpu: the kernels of csrc/streaming.hip and the classes of tam_gcn_amd.streaming against tests/streaming_ref.py, against the
feeders' own kernels on materialised copies of the windows (bit for bit), and end to end against the model's direct forward."""
import numpy as np
import pytest
import torch

import clip_resize_ref
import streaming_ref as R
import stream_ensemble_models as SM
from oracle import feeder_oracle
from tam_gcn_amd import ops
from tam_gcn_amd.feeder.feeder_nucla_gcn import BONE_PARENT
from tam_gcn_amd.inference import default_parent
from tam_gcn_amd.streaming import FrameRing, LiveClassifier, SlidingWindow

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
SENTINEL = -7.0


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.tensor(a, dtype=dtype, device=DEV)


def _walk(rng, n, V=20):
    """n frames of (V, 3) joints that move like a skeleton: a pose plus a random walk."""
    return rng.normal(size=(1, V, 3)) + 0.05 * np.cumsum(rng.normal(size=(n, V, 3)), axis=0)


# ---- ring ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', [('nucla', 20, 3, 1), ('nucla', 5, 3, 1), ('clip', 17, 3, 1), ('clip', 25, 3, 2), ('clip', 20, 2, 1)],
                         ids=['nucla_v20_16B', 'nucla_v5_8B', 'clip_v17_4B', 'clip_v25x2_4B', 'clip_v20_16B'])
def test_ring_push_equals_the_ring_model(layout):
    prep, V, C, M = layout
    cap, rng = 16, np.random.default_rng(1)
    if prep == 'nucla':
        seq = rng.normal(size=(38, V, 3))
        ring = torch.full((cap, V, 3), SENTINEL, dtype=torch.float64, device=DEV)
    else:
        seq = rng.normal(size=(38, C, V, M)).astype(np.float32)                 # frame-major here, (C, n, V, M) when pushed
        ring = torch.full((C, cap, V, M), SENTINEL, dtype=torch.float32, device=DEV)
    state = torch.zeros(2, dtype=torch.int64, device=DEV)
    model, at = R.Ring(cap), 0
    for pushes, n in enumerate((5, 7, 9, 1, 16), 1):                            # the third push wraps inside itself
        chunk = seq[at:at + n]
        at += n
        model.push(chunk)
        ops.ring_push(_dev(chunk if prep == 'nucla' else chunk.transpose(1, 0, 2, 3)), ring, state)
        assert state.tolist() == [at, pushes] == [model.count, model.pushes]
        got = ring.cpu().numpy() if prep == 'nucla' else ring.cpu().numpy().transpose(1, 0, 2, 3)
        for s in range(cap):
            if model.slots[s] is None:
                assert (got[s] == SENTINEL).all(), f'slot {s} was never written'
            else:
                assert np.array_equal(got[s], model.slots[s]), (at, s)


def test_frame_ring_casts_counts_and_resets():
    ring = FrameRing(16, prep='nucla', V=20, device=DEV)
    x = torch.randn(5, 20, 3, device=DEV, dtype=torch.float32)
    ring.push(x)
    assert ring.count == 5 and torch.equal(ring.buf[:5], x.double()) and not ring.buf[5:].any()
    with pytest.raises(ValueError, match='outside 1..capacity'):
        ring.push(torch.zeros(17, 20, 3, device=DEV))
    with pytest.raises(RuntimeError, match='no CPU path'):
        ring.push(torch.zeros(2, 20, 3))
    ring.reset()
    assert ring.count == 0 and not ring.buf.any()


def test_ring_plan_equals_plan_live():
    for count in (5, 12, 17, 40):
        state = torch.tensor([count, 3], dtype=torch.int64, device=DEV)
        got = ops.ring_plan(state, 16, 3, 9, 4).cpu().numpy()
        want = R.plan_live(count, 16, 3, 9, 4)
        assert np.array_equal(got, want), (count, got, want)
    assert not R.plan_live(5, 16, 3, 9, 4).any() and not R.plan_live(40, 16, 3, 9, 4)[0].any()      # before frame 0; overwritten


# ---- windows ------------------------------------------------------------------------------------------------------------
def _feeder_transform(windows, TS, stream):
    """ops.feeder_transform (the feeder's own kernel) on materialised copies of the windows, identity view, val indices."""
    offs = np.concatenate([[0], np.cumsum([len(w) for w in windows])]).astype(np.int64)
    rot = np.tile(np.eye(3), (len(windows), 1, 1))
    idx = np.stack([feeder_oracle.val_indices(len(w), TS) for w in windows]).astype(np.int32)
    return ops.feeder_transform(_dev(np.concatenate(windows)), _dev(offs), _dev(rot), _dev(idx), _dev(BONE_PARENT, torch.int32), 20, TS, 1, stream)


@pytest.fixture(scope='module')
def nucla_seq():
    return _walk(np.random.default_rng(2), 23)


@pytest.mark.parametrize('stream', R.STREAMS)
def test_window_nucla_equals_the_feeder_kernel_and_the_oracle(nucla_seq, stream):
    seq = nucla_seq
    parent = _dev(BONE_PARENT, torch.int32)
    ring = FrameRing(16, prep='nucla', V=20, device=DEV)                      # 23 frames through 16 slots: frames 7 .. 22 remain
    ring.push(_dev(seq[:16]))
    ring.push(_dev(seq[16:]))
    whole = _dev(seq)                                                           # the offline form: cap = length, no wrap
    for TS, rows, src, cap in ((52, [(22, 1), (5, 9), (0, 23), (0, 0), (14, 9)], whole, 23), (8, [(5, 9), (0, 0)], whole, 23),
                               (52, [(10, 9), (0, 0), (7, 16), (22, 1)], ring.buf, 16), (8, [(12, 9)], ring.buf, 16)):
        got = ops.window_nucla(src, _dev(rows, torch.int64), parent, TS, 1, stream).cpu().numpy()
        assert got.shape == (len(rows), 3, TS, 20, 1) and np.isfinite(got).all()                  # L = 1 included
        valid = [(s, L) for s, L in rows if L]
        direct = _feeder_transform([seq[s:s + L] for s, L in valid], TS, stream).cpu().numpy()
        k = 0
        for b, (s, L) in enumerate(rows):
            if not L:
                assert not got[b].any(), (TS, b)
                continue
            assert np.array_equal(got[b], direct[k]), (TS, s, L, cap, float(np.abs(got[b] - direct[k]).max()))
            want = R.window_nucla(seq[s:s + L], stream, TS)
            assert np.array_equal(got[b], want), (TS, s, L, cap, float(np.abs(got[b] - want).max()))
            k += 1


@pytest.mark.parametrize('C,V,M', [(3, 17, 1), (3, 25, 2), (3, 20, 1)], ids=['v17', 'v25x2', 'v20_16B'])
def test_window_clip_equals_clip_resize_and_its_reference(C, V, M):
    rng = np.random.default_rng(3)
    W = 8
    seq = rng.uniform(-1.0, 1.0, size=(C, 23, V, M)).astype(np.float32)
    ring = FrameRing(16, prep='clip', V=V, C=C, M=M, device=DEV)
    ring.push(_dev(seq[:, :16]))
    ring.push(_dev(seq[:, 16:]))
    for rows, src in (([(22, 1), (3, 5), (9, 8), (0, 0), (10, 13)], _dev(seq)), ([(11, 8), (0, 0), (9, 13), (14, 5)], ring.buf)):
        got = ops.window_clip(src, _dev(rows, torch.int64), W).cpu().numpy()
        assert got.shape == (len(rows), C, W, V, M)
        for b, (s, L) in enumerate(rows):
            if not L:
                assert not got[b].any()
                continue
            crop = seq[:, s:s + L]
            direct = ops.clip_resize(_dev(crop[None]), _dev([0], torch.int64), _dev([[0, L]], torch.int32), W).cpu().numpy()[0]
            assert np.array_equal(got[b], direct), (s, L, float(np.abs(got[b] - direct).max()))
            want, bound = R.window_clip(seq, s, L, W)
            clip_resize_ref.check(got[b], want, bound, what=f'window ({s}, {L})')
            if L == W:
                assert np.array_equal(got[b], crop)


# ---- scores -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(R.VOTE_CASES))
def test_window_vote_is_inside_the_bound(name):
    logits, plan, frames = R.vote_case(name)
    B, K = logits.shape
    probs, scores, label, cover = R.vote(logits, plan, frames)
    gp, gs, gl = (t.cpu().numpy() for t in ops.window_vote(_dev(logits), _dev(plan), n_frames=frames))
    assert gp.dtype == np.float32 and gs.dtype == np.float32 and gl.dtype == np.int64
    err = np.abs(gp.astype(np.float64) - probs)
    assert (err <= R.score_bound(probs, K, 0)).all(), float((err / R.score_bound(probs, K, 0)).max())
    bound = R.score_bound(scores, K, cover[:, None])
    err = np.abs(gs.astype(np.float64) - scores)
    assert (err <= bound).all(), float((err / bound).max())
    assert (cover == 0).sum() >= 2 and not gs[cover == 0].any() and (gl[cover == 0] == -1).all()
    decided = R.top2_gap(scores) > 2 * R.score_bound(np.sort(scores, axis=1)[:, -1], K, cover)
    assert decided[cover > 0].all()                                             # every covered frame: the seeds see to it
    assert np.array_equal(gl[cover > 0], label[cover > 0])
    only, none, none2 = ops.window_vote(_dev(logits), _dev(plan))                # probabilities alone
    assert none is None and none2 is None and np.array_equal(only.cpu().numpy(), gp)


@pytest.mark.parametrize('beta', [0.0, 0.8])
def test_score_ema_is_inside_the_bound(beta):
    K, steps = 10, 12
    rows = R.softmax(R.vote_logits(steps, K, 7)).astype(np.float32)
    valid = [s not in (0, 5) for s in range(steps)]
    want = R.ema(rows, valid, beta)
    ema = torch.zeros(K, dtype=torch.float64, device=DEV)
    seen = torch.zeros(1, dtype=torch.int64, device=DEV)
    probs = _dev(rows)
    for s in range(steps):
        row = _dev([33 + s, 9] if valid[s] else [0, 0], torch.int64)
        out, label, conf = ops.score_ema(probs[s], row, beta, ema, seen)
        e, n, lab = want[s]
        assert int(seen) == n and int(label) == lab, (s, int(seen), int(label))
        bound = R.ema_bound(e, K, max(n, 1))
        got = ema.cpu().numpy()
        assert (np.abs(got - e) <= bound).all(), (s, float((np.abs(got - e) / bound).max()))
        assert np.array_equal(out.cpu().numpy(), got.astype(np.float32))
        assert float(conf) == (float(out[lab]) if lab >= 0 else 0.0)
    assert int(seen) == 10 and want[0][2] == -1


# ---- the classes ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ucla_model():
    return SM.base_model('ucla_t52').to(DEV).eval()


def _direct_nucla(model, seq, rows, TS=52, stream='joint'):
    """model(x) on the windows ops.feeder_transform builds from materialised frames; zeros for an invalid row."""
    x = torch.zeros(len(rows), 3, TS, 20, 1, device=DEV)
    valid = [b for b, (s, L) in enumerate(rows) if L]
    if valid:
        x[valid] = _feeder_transform([seq[rows[b][0]:rows[b][0] + rows[b][1]] for b in valid], TS, stream)
    with torch.no_grad():
        return model(x)


@pytest.mark.parametrize('length', [70, 63], ids=['two_full_chunks', 'padded_chunk'])
def test_sliding_window_equals_the_direct_forward_nucla(ucla_model, length):
    seq = _walk(np.random.default_rng(4), 70)[:length]
    sw = SlidingWindow(ucla_model, window=20, hop=8, prep='nucla', batch_windows=4)
    res = sw.run(_dev(seq))
    plan = R.plan_offline(length, 20, 8)
    n = len(plan)
    assert np.array_equal(res.plan.cpu().numpy(), plan) and res.window_logits.shape == (n, 10)
    rows = [tuple(r) for r in plan.tolist()] + [(0, 0)] * (-n % 4)
    want = torch.cat([_direct_nucla(ucla_model, seq, rows[c:c + 4]) for c in range(0, len(rows), 4)])[:n]
    assert torch.isfinite(want).all() and torch.equal(res.window_logits, want), float((res.window_logits - want).abs().max())
    probs, scores, label, cover = R.vote(want.cpu().numpy(), plan, length)
    assert cover.min() >= 1 and res.frame_scores.shape == (length, 10) and res.frame_label.shape == (length,)
    assert (np.abs(res.window_probs.cpu().numpy() - probs) <= R.score_bound(probs, 10, 0)).all()
    assert (np.abs(res.frame_scores.cpu().numpy() - scores) <= R.score_bound(scores, 10, cover[:, None])).all()
    again = sw.run(torch.from_numpy(seq))                                       # from the host, and twice the same bits
    assert torch.equal(again.window_logits, res.window_logits) and torch.equal(again.frame_scores, res.frame_scores)


COCO = dict(num_class=10, num_point=17, num_person=1, graph='tam_gcn_amd.graph.coco.Graph', graph_args=dict(labeling_mode='spatial'))


def test_sliding_window_equals_the_direct_forward_clip():
    from params import fill_state_
    from tam_gcn_amd.models.ctrgcn import Model
    m = Model(**COCO)
    fill_state_(m.state_dict(), seed=0)
    m = m.to(DEV).eval()
    seq = np.random.default_rng(5).uniform(-1.0, 1.0, size=(3, 70, 17, 1)).astype(np.float32)
    W = 16
    res = SlidingWindow(m, window=20, hop=8, prep='clip', window_size=W, stream='bone', batch_windows=4).run(_dev(seq))
    plan = R.plan_offline(70, 20, 8)
    parent = _dev(default_parent(m.graph), torch.int32)
    want = []
    for c in range(0, len(plan), 4):
        x = torch.cat([ops.clip_resize(_dev(seq[None, :, s:s + L]), _dev([0], torch.int64), _dev([[0, L]], torch.int32), W) for s, L in plan[c:c + 4].tolist()])
        with torch.no_grad():
            want.append(m(ops.stream_derive(x, parent, 'bone')))
    want = torch.cat(want)
    assert len(plan) == 8 and torch.isfinite(want).all()
    assert torch.equal(res.window_logits, want), float((res.window_logits - want).abs().max())


def test_live_classifier(ucla_model):
    model = ucla_model
    seq = _walk(np.random.default_rng(6), 84)
    frames = _dev(seq)
    live = LiveClassifier(model, FrameRing(64, prep='nucla', V=20, device=DEV), window=20, beta=0.8, frames_per_step=2)
    eager = LiveClassifier(model, FrameRing(64, prep='nucla', V=20, device=DEV), window=20, beta=0.8, frames_per_step=2, eager=True)
    assert live.captures == 1
    rows, valid = [], []
    for s in range(40):                                                         # 80 frames through 64 slots
        out = [t.clone() for t in live.step(frames[2 * s:2 * s + 2])]
        ref = eager.step(frames[2 * s:2 * s + 2])
        for a, b in zip(out, ref):
            assert torch.equal(a, b), s                                         # the replayed chain and the eager one: the same bits
        label, conf, smoothed, logits = out
        count = 2 * s + 2
        if s < 9:
            assert int(label) == -1 and float(conf) == 0.0 and not smoothed.any() and int(live.seen) == 0, s
            rows.append(np.zeros(10, dtype=np.float32))
            valid.append(False)
            continue
        want = _direct_nucla(model, seq, [(count - 20, 20)])
        assert torch.equal(logits, want), (s, float((logits - want).abs().max()))
        rows.append(R.softmax(want.cpu().numpy())[0].astype(np.float32))
        valid.append(True)
        e, n, lab = R.ema(np.stack(rows), valid, 0.8)[-1]
        assert int(live.seen) == n == s - 8
        # the device's fp32 probabilities and the reference's are roundings of two softmax chains, each inside score_bound of the
        # exact value (<= 1): they differ by twice that at the most, and the average is a convex combination of them
        slack = 2 * R.score_bound(1.0, 10, 0)
        assert (np.abs(live.ema.cpu().numpy() - e) <= R.ema_bound(e, 10, n) + slack).all(), s
        assert int(label) == int(np.argmax(smoothed.cpu().numpy())) and float(conf) == float(smoothed[int(label)])
    assert live.ring.count == 80 and live.captures == 1
    # an in-place edit of one parameter: the next step sees it, through a new capture
    with torch.no_grad():
        model.fc.bias.add_(0.5)
    try:
        _, _, _, logits = live.step(frames[80:82])
        assert live.captures == 2
        want = _direct_nucla(model, seq, [(62, 20)])
        assert torch.equal(logits, want)
        model.train()
        with pytest.raises(RuntimeError, match='train'):
            live.step(frames[82:84])
        model.eval()
        # the eager chain inside an outer capture: no synchronisation, no shape that depends on the host
        eager.step(frames[80:82])
        before = eager.ring.count
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outer = eager.step(frames[82:84])
        assert eager.ring.count == before                                       # captured, not run
        g.replay()
        assert eager.ring.count == before + 2 and int(outer[0]) >= 0
        assert torch.equal(outer[3], live.step(frames[82:84])[3])            # both saw the same 84 frames
    finally:
        model.eval()
        with torch.no_grad():
            model.fc.bias.sub_(0.5)
    live.reset()
    assert live.ring.count == 0 and int(live.seen) == 0 and not live.ema.any()


def test_live_classifier_two_windows_per_step(ucla_model):
    """hop_windows = 2, hop = 4, four frames per step through 32 slots: both windows go through the model as one batch of two, an
    invalid older window as zeros, and the average counts the valid ones, oldest first."""
    seq = _walk(np.random.default_rng(8), 32)
    frames = _dev(seq)
    live = LiveClassifier(ucla_model, FrameRing(32, prep='nucla', V=20, device=DEV), window=20, hop_windows=2, hop=4, beta=0.5, frames_per_step=4)
    seen, e = 0, np.zeros(10)
    for s in range(8):
        label, conf, smoothed, logits = live.step(frames[4 * s:4 * s + 4])
        count = 4 * s + 4
        rows = [tuple(r) for r in R.plan_live(count, 32, 2, 20, 4).tolist()]
        assert rows == [(count - 24, 20) if count >= 24 else (0, 0), (count - 20, 20) if count >= 20 else (0, 0)]
        want = _direct_nucla(ucla_model, seq, rows)
        assert logits.shape == (2, 10) and torch.equal(logits, want), s
        for j, (_, L) in enumerate(rows):
            if L:
                p = R.softmax(want[j:j + 1].cpu().numpy())[0].astype(np.float32).astype(np.float64)
                e = p if seen == 0 else 0.5 * e + 0.5 * p
                seen += 1
        assert int(live.seen) == seen == (0, 0, 0, 0, 1, 3, 5, 7)[s]
        assert int(label) == (int(np.argmax(e)) if seen else -1)
        assert (np.abs(live.ema.cpu().numpy() - e) <= R.ema_bound(e, 10, max(seen, 1)) + 2 * R.score_bound(1.0, 10, 0)).all(), s
