"""-m gpu: the bank of frame rings (the tamgcn_bank_* kernels of csrc/streaming.hip, tam_gcn_amd.streaming.RingBank / LiveBank)
against tests/streambank_ref.py, against the single-ring ops on every feed's own views (bit for bit), and end to end against one
independent LiveClassifier per feed that is stepped only on the feed's own ticks."""
import collections
import functools

import numpy as np
import pytest
import torch

import streaming_ref as R
import streambank_ref as BR
import stream_ensemble_models as SM
from tam_gcn_amd import ops
from tam_gcn_amd.feeder.feeder_nucla_gcn import BONE_PARENT
from tam_gcn_amd.inference import StreamEnsemble
from tam_gcn_amd.streaming import FrameRing, LiveBank, LiveClassifier, RingBank

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
SENTINEL = -7.0


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.tensor(a, dtype=dtype, device=DEV)


def _flags(v):
    return None if v is None else _dev(list(v), torch.int32)


def _walk(rng, n, V=20):
    return rng.normal(size=(1, V, 3)) + 0.05 * np.cumsum(rng.normal(size=(n, V, 3)), axis=0)


# ---- 1. push ------------------------------------------------------------------------------------------------------------
# (counts, restart) per tick for S = 3, n = 2, cap = 5: 0, 1 and 2 frames on different feeds of one tick, counts outside 0..n,
# a restart on a tick where the feed pushes (tick 3, feed 1) and one where it does not (tick 5, feed 2), None = all / none.
PUSH_TICKS = [((2, 1, 0), None), ((2, 0, 2), None), ((1, 5, -1), (0, 0, 0)), ((2, 2, 2), (0, 1, 0)), ((0, 2, 2), None),
              ((2, 1, 0), (0, 0, 1)), (None, None)]


@pytest.mark.parametrize('layout', [('nucla', 20, 3, 1), ('nucla', 5, 3, 1), ('clip', 17, 3, 1), ('clip', 20, 3, 1), ('clip', 25, 3, 2)],
                         ids=['nucla_v20_16B', 'nucla_v5_8B', 'clip_v17_4B', 'clip_v20_16B', 'clip_v25x2_4B'])
def test_bank_push_equals_the_reference_and_ring_push_per_feed(layout):
    prep, V, C, M = layout
    S, cap, n, rng = 3, 5, 2, np.random.default_rng(11)
    nucla = prep == 'nucla'
    shape, dtype = ((S, cap, V, 3), torch.float64) if nucla else ((S, C, cap, V, M), torch.float32)
    bank = torch.full(shape, SENTINEL, dtype=dtype, device=DEV)
    state = torch.zeros(S, 2, dtype=torch.int64, device=DEV)
    alone = [(torch.full(shape[1:], SENTINEL, dtype=dtype, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)) for _ in range(S)]
    model = BR.Bank(S, cap)
    for t, (counts, restart) in enumerate(PUSH_TICKS):
        fr = rng.normal(size=(S, n, V, 3)) if nucla else rng.normal(size=(S, n, C, V, M)).astype(np.float32)      # (feed, frame, ...)
        takes = [BR.take(counts, s, n) for s in range(S)]
        model.push([list(fr[s]) for s in range(S)], counts, restart)
        sent = fr.copy()
        for s in range(S):
            sent[s, takes[s]:] = np.nan                                         # what is not taken is never read
        before = bank.clone()
        ops.bank_push(_dev(sent if nucla else sent.transpose(0, 2, 1, 3, 4)), bank, state, _flags(counts), _flags(restart))
        assert np.array_equal(state.cpu().numpy(), model.state()), (t, state.tolist())
        assert not torch.isnan(bank).any(), t
        for s in range(S):
            if restart is not None and restart[s]:
                alone[s][1].zero_()                                             # forgotten, not cleared
            if takes[s]:
                one = fr[s, :takes[s]]
                ops.ring_push(_dev(one if nucla else one.transpose(1, 0, 2, 3)), *alone[s])
            else:
                assert torch.equal(bank[s], before[s]), (t, s)                  # a feed that takes nothing is untouched
            assert torch.equal(bank[s], alone[s][0]) and torch.equal(state[s], alone[s][1]), (t, s)
            got = bank[s].cpu().numpy() if nucla else bank[s].cpu().numpy().transpose(1, 0, 2, 3)
            for slot, want in enumerate(model.rings[s].slots):
                if want is not None:
                    assert np.array_equal(got[slot], want), (t, s, slot)
    assert (model.state()[:, 0] > 0).all() and state[:, 0].tolist() == [11, 7, 2]


def test_ring_bank_pushes_resets_and_hands_out_feeds():
    bank = RingBank(3, 8, prep='nucla', V=20, device=DEV)
    x = torch.randn(3, 2, 20, 3, device=DEV, dtype=torch.float32)
    bank.push(x, counts=_flags((2, 0, 1)))
    assert bank.counts == [2, 0, 1] and torch.equal(bank.buf[0, :2], x[0].double()) and not bank.buf[1].any() and not bank.buf[2, 1:].any()
    buf, state = bank.feed(2)
    ops.ring_push(x[2].double().contiguous(), buf, state)                       # the single-ring op on a feed's views
    assert bank.counts == [2, 0, 3] and torch.equal(bank.buf[2, 1:3], x[2].double())
    bank.push(x, restart=torch.tensor([0, 0, 1]))
    assert bank.counts == [4, 2, 2] and bank.state[:, 1].tolist() == [2, 1, 1]
    bank.reset([0])
    assert bank.counts == [0, 2, 2] and not bank.buf[0].any()
    bank.reset()
    assert bank.counts == [0, 0, 0] and not bank.buf.any()
    with pytest.raises(ValueError, match='outside 1..capacity'):
        bank.push(torch.zeros(3, 9, 20, 3, device=DEV))
    with pytest.raises(ValueError, match='counts'):
        bank.push(x, counts=torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match='no CPU path'):
        bank.push(torch.zeros(3, 2, 20, 3))
    with pytest.raises(ValueError, match='outside 0..2'):
        bank.feed(3)


# ---- 2. plan ------------------------------------------------------------------------------------------------------------
def test_bank_plan_equals_plan_live_per_feed():
    counts = [5, 12, 17, 40, 17]                                                # before frame 0; partly; the oldest overwritten (twice); idle
    state = _dev([[c, 3] for c in counts], torch.int64)
    took = (1, 2, 1, 1, 0)
    got = ops.bank_plan(state, 16, 3, 9, 4, _flags(took)).cpu().numpy()
    want = np.concatenate([R.plan_live(c, 16, 3, 9, 4) if k else np.zeros((3, 2), dtype=np.int64) for c, k in zip(counts, took)])
    assert np.array_equal(got, want), (got, want)
    assert not want[:3].any() and not want[6].any() and want[7:9].all() and not want[9].any() and want[10:12].all() and not want[12:].any()
    padded = ops.bank_plan(state, 16, 3, 9, 4, rows=18).cpu().numpy()            # no counts: every feed plans; a padded tail
    assert np.array_equal(padded[12:15], R.plan_live(17, 16, 3, 9, 4)) and not padded[15:].any() and np.array_equal(padded[:12], want[:12])


# ---- 3. windows ---------------------------------------------------------------------------------------------------------
# plan rows (B = 3 per feed) for feeds that hold frames 7..22, 0..11 and 0..15 of their sequences in 16 slots
WINDOW_ROWS = [(10, 9), (0, 0), (7, 16), (3, 9), (11, 1), (0, 0), (0, 16), (0, 0), (5, 8)]
FILL = (23, 12, 16)


@pytest.mark.parametrize('stream', R.STREAMS)
def test_bank_window_nucla_equals_window_nucla_per_feed(stream):
    rng = np.random.default_rng(12)
    bank = RingBank(3, 16, prep='nucla', V=20, device=DEV)
    for s, length in enumerate(FILL):
        seq = _dev(_walk(rng, length))
        for at in range(0, length, 16):
            ops.ring_push(seq[at:at + 16].contiguous(), *bank.feed(s))
    assert bank.counts == list(FILL)
    parent = _dev(BONE_PARENT, torch.int32)
    plan = _dev(WINDOW_ROWS + [(0, 0), (0, 0)], torch.int64)                     # two rows of padding
    for TS in (52, 8):
        got = ops.bank_window_nucla(bank.buf, plan, 3, parent, TS, 1, stream)
        assert got.shape == (11, 3, TS, 20, 1) and not got[9:].any()
        for s in range(3):
            want = ops.window_nucla(bank.feed(s)[0], plan[3 * s:3 * s + 3], parent, TS, 1, stream)
            assert torch.equal(got[3 * s:3 * s + 3], want), (TS, s)
            assert want[[b for b in range(3) if WINDOW_ROWS[3 * s + b][1]]].abs().sum() > 0
            assert not want[[b for b in range(3) if not WINDOW_ROWS[3 * s + b][1]]].any()


@pytest.mark.parametrize('C,V,M', [(3, 17, 1), (3, 20, 1), (2, 25, 2)], ids=['v17', 'v20_16B', 'v25x2'])
def test_bank_window_clip_equals_window_clip_per_feed(C, V, M):
    rng = np.random.default_rng(13)
    bank = RingBank(3, 16, prep='clip', V=V, C=C, M=M, device=DEV)
    for s, length in enumerate(FILL):
        seq = _dev(rng.uniform(-1.0, 1.0, size=(C, length, V, M)).astype(np.float32))
        for at in range(0, length, 16):
            ops.ring_push(seq[:, at:at + 16].contiguous(), *bank.feed(s))
    plan = _dev(WINDOW_ROWS, torch.int64)
    got = ops.bank_window_clip(bank.buf, plan, 3, 8)
    assert got.shape == (9, C, 8, V, M)
    for s in range(3):
        want = ops.window_clip(bank.feed(s)[0], plan[3 * s:3 * s + 3], 8)
        assert torch.equal(got[3 * s:3 * s + 3], want), s
        assert want[[b for b in range(3) if WINDOW_ROWS[3 * s + b][1]]].abs().sum() > 0


# ---- 4. the averages ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [0.0, 0.8])
def test_bank_ema_equals_score_ema_per_feed(beta):
    S, B, K, ticks = 3, 2, 10, 6
    rows = R.softmax(R.vote_logits(ticks * S * B, K, 21)).astype(np.float32).reshape(ticks, S * B, K)
    rows[1, 2, :] = 0.0
    rows[1, 2, [3, 7]] = 0.5                                                    # a tie on feed 1's first window: the first arg max
    # valid[t][s][j]; feed 1 skips ticks 0 and 3 entirely, feed 2 restarts at tick 4 (with a valid window) and feed 0 at tick 5
    # (without one)
    valid = np.ones((ticks, S, B), dtype=bool)
    valid[0, 1] = valid[3, 1] = False
    valid[2, 0, 0] = valid[4, 2, 0] = valid[1, 1, 1] = False
    valid[5, 0] = False
    restarts = {4: (0, 0, 1), 5: (1, 0, 0)}
    ema = torch.zeros(S, K, dtype=torch.float64, device=DEV)
    seen = torch.zeros(S, dtype=torch.int64, device=DEV)
    alone = [(torch.zeros(K, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)) for _ in range(S)]
    ref = BR.Averages(S, K, beta)
    for t in range(ticks):
        plan = _dev([(3 + t, 4) if v else (0, 0) for v in valid[t].reshape(-1)], torch.int64)
        probs = _dev(rows[t])
        restart = restarts.get(t)
        before = seen.clone()
        out, label, conf, adv = ops.bank_ema(probs, plan, beta, ema, seen, _flags(restart))
        want = ref.tick(rows[t].reshape(S, B, K), valid[t], restart)
        for s in range(S):
            if restart is not None and restart[s]:
                alone[s][0].zero_()
                alone[s][1].zero_()
                before[s] = 0
            for j in range(B):
                o1, l1, c1 = ops.score_ema(probs[s * B + j], plan[s * B + j], beta, *alone[s])
            assert torch.equal(ema[s], alone[s][0]) and int(seen[s]) == int(alone[s][1]) == want[s][1], (t, s)
            assert torch.equal(out[s], o1) and int(label[s]) == int(l1) == want[s][2] and float(conf[s]) == float(c1), (t, s)
            assert bool(adv[s]) == want[s][3] == (int(seen[s]) > int(before[s])), (t, s)
        if t == 1:
            assert int(label[1]) == 3 and float(conf[1]) == 0.5                 # feed 1's first valid window is the tied row
    assert seen.tolist() == [0, 7, 3]
    tie = _dev(np.array([[0.0, 0.5, 0.0, 0.5]], dtype=np.float32))
    _, label, conf, _ = ops.bank_ema(tie, _dev([(0, 4)], torch.int64), 0.0, torch.zeros(1, 4, dtype=torch.float64, device=DEV),
                                     torch.zeros(1, dtype=torch.int64, device=DEV))
    assert int(label) == 1 and float(conf) == 0.5


# ---- 5 .. 9. LiveBank against one LiveClassifier per feed ---------------------------------------------------------------------
Tick = collections.namedtuple('Tick', 'frames counts restart taken')
Played = collections.namedtuple('Played', 'outs seen advanced counts')


def _ticks(prep, seqs, n, sched):
    """sched: [(counts | None, restart | None)] -> [Tick]: feed s is offered the next n frames of its own sequence and takes the first
    counts[s]; the rest of its slice is NaN."""
    S, at, out = len(seqs), [0] * len(seqs), []
    for counts, restart in sched:
        offered, taken = [], []
        for s in range(S):
            c = BR.take(counts, s, n)
            f = seqs[s][at[s]:at[s] + n].copy() if prep == 'nucla' else seqs[s][:, at[s]:at[s] + n].copy()
            taken.append(f[:c] if prep == 'nucla' else f[:, :c])
            if prep == 'nucla':
                f[c:] = np.nan
            else:
                f[:, c:] = np.nan
            offered.append(f)
            at[s] += c
        out.append(Tick(_dev(np.stack(offered)), counts, restart, taken))
    return out


def _play(live, ticks):
    """Step `live` through the ticks: clones of every tick's outputs, seen and the feeds' frame counts after it, and which feeds'
    seen advanced (a restarted feed's counts from 0)."""
    outs, seens, adv, counts = [], [], [], []
    for tk in ticks:
        before = live.seen.clone()
        if tk.restart is not None:
            before[torch.tensor(tk.restart, device=DEV) != 0] = 0
        out = live.step(tk.frames, _flags(tk.counts), _flags(tk.restart))
        outs.append(type(out)(*[None if v is None else v.clone() for v in out]))
        seens.append(live.seen.clone())
        adv.append((live.seen > before).cpu().numpy())
        counts.append(live.bank.state[:, 0].cpu().numpy())
    return Played(outs, seens, np.stack(adv), np.stack(counts))


def _play_alone(model, prep, V, ticks, cap, kw):
    """One eager LiveClassifier per feed on its own FrameRing, stepped only on the feed's ticks with the frames it took and
    reset() where it restarts -> per tick, per feed (label, conf, smoothed, logits | None: the feed did not step)."""
    S = len(ticks[0].taken)
    per = [max(BR.take(tk.counts, s, tk.frames.shape[1 if prep == 'nucla' else 2]) for tk in ticks) for s in range(S)]
    alone = [LiveClassifier(model, FrameRing(cap, prep=prep, V=V, device=DEV), frames_per_step=per[s], eager=True, **kw) for s in range(S)]
    K = alone[0].num_class
    idle = (torch.full((1,), -1, dtype=torch.int64, device=DEV), torch.zeros(1, device=DEV), torch.zeros(K, device=DEV))
    last, out = [idle] * S, []
    for tk in ticks:
        row = []
        for s in range(S):
            if tk.restart is not None and tk.restart[s]:
                alone[s].reset()
                last[s] = idle
            n_s = tk.taken[s].shape[0 if prep == 'nucla' else 1]
            if n_s:
                assert n_s == per[s]
                label, conf, smoothed, logits = (v.clone() for v in alone[s].step(_dev(tk.taken[s])))
                last[s] = (label, conf, smoothed)
                row.append((label, conf, smoothed, logits))
            else:
                row.append(last[s] + (None,))
        out.append(row)
    return out, [int(a.seen) for a in alone]


def _same(played, want, what):
    active = 0
    for t, (out, row) in enumerate(zip(played.outs, want)):
        for s, (label, conf, smoothed, logits) in enumerate(row):
            assert int(out.label[s]) == int(label) and float(out.conf[s]) == float(conf), (what, t, s, int(out.label[s]), int(label))
            assert torch.equal(out.smoothed[s], smoothed), (what, t, s)
            if logits is not None:
                assert torch.equal(out.logits[s], logits), (what, t, s, float((out.logits[s] - logits).abs().max()))
                active += 1
    return active


def _same_outs(a, b, what):
    for t, (x, y) in enumerate(zip(a.outs, b.outs)):
        for name, u, v in zip(x._fields, x, y):
            assert (u is None and v is None) or torch.equal(u, v), (what, t, name)
        assert torch.equal(a.seen[t], b.seen[t]), (what, t)


@functools.lru_cache(maxsize=None)
def _ucla():
    return SM.base_model('ucla_t52').to(DEV).eval()


def _nucla_seqs(S, total, seed):
    rng = np.random.default_rng(seed)
    return [_walk(rng, total) for _ in range(S)]


# 14 ticks, S = 3, window 8, one frame per tick: feed 1 skips ticks 2, 3 and 10; feed 2 restarts in mid-run, at tick 9 (with a
# frame), after two valid windows: its average, seen and stable label are forgotten and it has no valid window again.  Tick 6
# passes no counts at all.
def _sched_a():
    return [((1, 0 if t in (2, 3, 10) else 1, 1) if t != 6 else None, (0, 0, 1) if t == 9 else None) for t in range(14)]


# every advanced tick is confident and decides at once: each feed's first valid window is an event whatever the model says (the
# run counting and the threshold are held to the reference on hand-written scores below)
THRESHOLD, HOLD = 0.0, 1


@pytest.fixture(scope='module')
def case_a():
    """LiveBank (graph and eager) and the independent classifiers on schedule A, with the decision log on: shared by the
    comparison, the log and the resume tests.  Nothing in it is modified afterwards."""
    model = _ucla()
    ticks = _ticks('nucla', _nucla_seqs(3, 14, 31), 1, _sched_a())
    kw = dict(window=8, beta=0.8)
    live = LiveBank(model, RingBank(3, 12, prep='nucla', V=20, device=DEV), threshold=THRESHOLD, hold=HOLD, **kw)
    eager = LiveBank(model, RingBank(3, 12, prep='nucla', V=20, device=DEV), threshold=THRESHOLD, hold=HOLD, eager=True, **kw)
    played, played_eager = _play(live, ticks), _play(eager, ticks)
    want, seen = _play_alone(model, 'nucla', 20, ticks, 12, kw)
    return dict(model=model, ticks=ticks, kw=kw, live=live, eager=eager, played=played, played_eager=played_eager, want=want, seen=seen)


def test_live_bank_equals_independent_classifiers(case_a):
    c = case_a
    active = _same(c['played'], c['want'], 'graph')
    assert active == 3 * 14 - 3                                                  # every feed on every tick it took a frame
    _same_outs(c['played'], c['played_eager'], 'graph against eager')
    assert c['live'].captures == 1 and c['eager'].captures == 0
    assert c['played'].seen[-1].tolist() == c['seen'] == [7, 4, 0]
    labels = torch.stack([o.label for o in c['played'].outs]).cpu().numpy()
    assert (labels[:7, 0] == -1).all() and (labels[7:, 0] >= 0).all()            # feed 0: its first valid window at tick 7
    assert (labels[:9, 1] == -1).all() and (labels[9:, 1] >= 0).all()            # feed 1: two ticks later, and tick 10 repeats tick 9
    assert (labels[7:9, 2] >= 0).all() and (labels[9:, 2] == -1).all()           # feed 2 restarted at tick 9
    assert not c['played'].outs[9].smoothed[2].any() and float(c['played'].outs[9].conf[2]) == 0.0


def test_live_bank_two_frames_per_step_and_two_windows():
    """frames_per_step = 2 with counts of 1 on feed 1 throughout and a skipping feed 0; hop_windows = 2, hop = 3."""
    model = _ucla()
    sched = [((0 if t in (1, 5) else 2, 1, 2), (0, 0, 1) if t == 6 else None) for t in range(12)]
    ticks = _ticks('nucla', _nucla_seqs(3, 24, 32), 2, sched)
    kw = dict(window=8, hop_windows=2, hop=3, beta=0.5)
    live = LiveBank(model, RingBank(3, 12, prep='nucla', V=20, device=DEV), frames_per_step=2, **kw)
    eager = LiveBank(model, RingBank(3, 12, prep='nucla', V=20, device=DEV), frames_per_step=2, eager=True, **kw)
    played = _play(live, ticks)
    want, seen = _play_alone(model, 'nucla', 20, ticks, 12, kw)
    assert _same(played, want, 'n = 2, B = 2') == 3 * 12 - 2
    _same_outs(played, _play(eager, ticks), 'graph against eager')
    assert live.captures == 1 and played.seen[-1].tolist() == seen and min(seen) >= 2
    assert played.outs[0].logits.shape == (3, 2, 10) and played.outs[0].stable is None


# ---- 6. other families ----------------------------------------------------------------------------------------------------
COCO = dict(num_class=10, num_point=17, num_person=1, graph='tam_gcn_amd.graph.coco.Graph', graph_args=dict(labeling_mode='spatial'))
SCHED_2 = [((1, 0 if t in (2, 7) else 1), (0, 1) if t == 3 else None) for t in range(14)]


def _coco():
    from params import fill_state_
    from tam_gcn_amd.models.ctrgcn import Model
    m = Model(**COCO)
    fill_state_(m.state_dict(), seed=0)
    return m.to(DEV).eval(), 'clip', 17, dict(window=8, beta=0.8, window_size=16, stream='bone')


def _stgcn():
    from test_stgcn_oracle import fill_stgcn_
    from tam_gcn_amd.models import stgcn
    m = stgcn.Model(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
    fill_stgcn_(m.state_dict(), seed=42)
    return m.to(DEV).eval(), 'nucla', 20, dict(window=8, beta=0.8)


def _two_streams():
    models = [SM.perturbed_model('ucla_t52', g).to(DEV).eval() for g in range(2)]
    return StreamEnsemble(models, ('joint', 'bone')), 'nucla', 20, dict(window=8, beta=0.8)


@pytest.mark.parametrize('make', [_coco, _stgcn, _two_streams], ids=['coco_clip', 'stgcn_nucla', 'two_stream_ensemble'])
def test_live_bank_on_other_families(make):
    model, prep, V, kw = make()
    rng = np.random.default_rng(33)
    seqs = _nucla_seqs(2, 14, 33) if prep == 'nucla' else [rng.uniform(-1.0, 1.0, size=(3, 14, V, 1)).astype(np.float32) for _ in range(2)]
    ticks = _ticks(prep, seqs, 1, SCHED_2)
    live = LiveBank(model, RingBank(2, 12, prep=prep, V=V, device=DEV), **kw)
    played = _play(live, ticks)
    want, seen = _play_alone(model, prep, V, ticks, 12, kw)
    assert _same(played, want, make.__name__) == 2 * 14 - 2
    assert live.captures == 1 and played.seen[-1].tolist() == seen and min(seen) >= 1


# ---- 7. chunking ------------------------------------------------------------------------------------------------------------
def test_live_bank_chunks_are_the_default_pass():
    model = _ucla()
    sched = [((1, 1, 0 if t in (0, 5) else 1, 1, 1), (0, 0, 0, 1, 0) if t == 2 else None) for t in range(11)]
    ticks = _ticks('nucla', _nucla_seqs(5, 11, 34), 1, sched)
    kw = dict(window=8, beta=0.8)
    whole = LiveBank(model, RingBank(5, 12, prep='nucla', V=20, device=DEV), **kw)
    split = LiveBank(model, RingBank(5, 12, prep='nucla', V=20, device=DEV), chunk_windows=2, **kw)
    assert (whole.chunks, whole.chunk) == (1, 5) and (split.chunks, split.chunk) == (3, 2)               # the last chunk is padded
    a, b = _play(whole, ticks), _play(split, ticks)
    _same_outs(a, b, 'one pass against three chunks')
    assert split.captures == 1 and int(a.seen[-1].min()) >= 1 and torch.isfinite(a.outs[-1].logits).all()


# ---- 8. the decision log ------------------------------------------------------------------------------------------------------
def _gpu_sequences(played):
    labels = torch.stack([o.label for o in played.outs]).cpu().numpy()
    confs = torch.stack([o.conf for o in played.outs]).cpu().numpy()
    stable = torch.stack([o.stable for o in played.outs]).cpu().numpy()
    return labels, confs, stable


def test_decision_log_equals_the_reference_on_the_devices_own_scores(case_a):
    c = case_a
    labels, confs, stable = _gpu_sequences(c['played'])
    restarts = [tk.restart or (0, 0, 0) for tk in c['ticks']]
    want_stable, rows, rc, dropped = BR.decide(labels, confs, c['played'].advanced, THRESHOLD, HOLD, counts=c['played'].counts, restarts=restarts)
    assert np.array_equal(stable, want_stable), (stable, want_stable)
    ev = c['live'].events()
    assert ev.rows.dtype == torch.int64 and ev.conf.dtype == torch.float32
    assert np.array_equal(ev.rows.numpy(), rows) and np.array_equal(ev.conf.numpy(), rc) and ev.dropped == dropped == 0
    assert rows[:2].tolist() == [[0, 7, int(stable[7, 0])], [2, 7, int(stable[7, 2])]]             # tick 7: feeds 0 and 2, ascending
    assert [r for r in rows.tolist() if r[0] == 1][0] == [1, 7, int(stable[9, 1])]                 # feed 1's eighth frame came at tick 9
    assert (stable[9:, 2] == -1).all()                                           # the restart forgot feed 2's decision
    again = c['eager'].events()                                                  # a second run: the same log
    assert torch.equal(again.rows, ev.rows) and torch.equal(again.conf, ev.conf) and again.dropped == 0


@pytest.mark.parametrize('S,capacity', [(6, 3), (300, 4096), (1024, 700)], ids=['one_wave', 'two_waves_no_drop', 'every_feed_drops'])
def test_bank_decide_equals_the_reference_on_hand_written_scores(S, capacity):
    """Labels of two classes, confidences at, just below and above the threshold, feeds that do not advance and feeds that restart:
    the run counting, conf == threshold, the scan over the feeds (across threads and waves) and the full log."""
    thr, hold, ticks, rng = 0.6, 2, 7, np.random.default_rng(41)
    at = np.float32(thr)
    labels = rng.integers(3, 5, size=(ticks, S))
    confs = rng.choice(np.array([at, np.nextafter(at, np.float32(0)), np.float32(0.9)], dtype=np.float32), size=(ticks, S), p=[.4, .2, .4])
    adv = rng.random((ticks, S)) < 0.8
    restarts = (rng.random((ticks, S)) < 0.1).astype(np.int32)
    counts = np.cumsum(rng.integers(0, 3, size=(ticks, S)), axis=0) + 1
    want_stable, rows, rc, dropped = BR.decide(labels, confs, adv, thr, hold, counts=counts, restarts=restarts, capacity=capacity)
    deb = _dev([[-1, -1, 0]] * S, torch.int64)
    log_rows = torch.full((capacity, 3), -9, dtype=torch.int64, device=DEV)
    log_conf = torch.zeros(capacity, dtype=torch.float32, device=DEV)
    log_count = torch.zeros(2, dtype=torch.int64, device=DEV)
    for t in range(ticks):
        state = _dev(np.stack([counts[t], counts[t]], axis=1).astype(np.int64))
        ops.bank_decide(_dev(labels[t].astype(np.int64)), _dev(confs[t]), _dev(adv[t].astype(np.int32)), state, thr, hold, deb, log_rows, log_conf,
                        log_count, _dev(restarts[t]))
        assert np.array_equal(deb[:, 0].cpu().numpy(), want_stable[t]), t
    written, lost = log_count.tolist()
    assert written == len(rows) and lost == dropped and (dropped > 0) == (capacity != 4096) and written > 0
    assert np.array_equal(log_rows[:written].cpu().numpy(), rows) and np.array_equal(log_conf[:written].cpu().numpy(), rc)
    assert (log_rows[written:] == -9).all()


def test_a_full_log_drops_and_counts_and_clears_without_a_capture(case_a):
    c = case_a
    live = LiveBank(c['model'], RingBank(3, 12, prep='nucla', V=20, device=DEV), threshold=THRESHOLD, hold=HOLD, log_capacity=2, **c['kw'])
    played = _play(live, c['ticks'])
    _same_outs(played, c['played'], 'log_capacity = 2')
    labels, confs, _ = _gpu_sequences(played)
    restarts = [tk.restart or (0, 0, 0) for tk in c['ticks']]
    _, rows, rc, dropped = BR.decide(labels, confs, played.advanced, THRESHOLD, HOLD, counts=played.counts, restarts=restarts, capacity=2)
    ev = live.events()
    full = c['live'].events()
    assert len(ev.rows) == 2 and ev.dropped == dropped == len(full.rows) - 2 >= 1
    assert np.array_equal(ev.rows.numpy(), rows) and np.array_equal(ev.conf.numpy(), rc) and torch.equal(ev.rows, full.rows[:2])
    live.clear_events()
    ev = live.events()
    assert len(ev.rows) == 0 and ev.dropped == 0
    out = live.step(c['ticks'][-1].frames)
    assert live.captures == 1 and out.stable.shape == (3,)


# ---- 9. resume ------------------------------------------------------------------------------------------------------------------
def test_live_bank_resumes_from_its_state_dict(case_a):
    c = case_a
    mk = lambda: LiveBank(c['model'], RingBank(3, 12, prep='nucla', V=20, device=DEV), threshold=THRESHOLD, hold=HOLD, **c['kw'])      # noqa: E731
    first = mk()
    head = _play(first, c['ticks'][:9])
    sd = first.state_dict()
    assert sorted(sd) == ['buf', 'deb', 'ema', 'log_conf', 'log_count', 'log_rows', 'seen', 'state']
    resumed = mk()
    resumed.load_state_dict(sd)
    tail = _play(resumed, c['ticks'][9:])
    for t, (x, y) in enumerate(zip(tail.outs, c['played'].outs[9:])):
        for name, u, v in zip(x._fields, x, y):
            assert torch.equal(u, v), (t, name)
    ev, full = resumed.events(), c['live'].events()
    assert torch.equal(ev.rows, full.rows) and torch.equal(ev.conf, full.conf) and ev.dropped == full.dropped
    assert resumed.captures == 1 and len(head.outs) == 9
    with pytest.raises(ValueError, match='keys'):
        resumed.load_state_dict({'ema': sd['ema']})
