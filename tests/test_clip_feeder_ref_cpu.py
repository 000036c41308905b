"""The clip feeder's numpy restatement (tests/clip_feeder_ref.py) against the reference's recorded outputs
(tests/golden/clip_feeder.npz, written by tests/golden/make_golden_clip_feeder.py), the draw stream's coverage, the node tables,
and the feeder's host-side pieces and argument checks -- none of which needs a GPU."""
import os

import numpy as np
import pytest

import clip_feeder_ref as R
from tam_gcn_amd.feeder import clip_feeder as CF

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'clip_feeder.npz'))
CASES = [tuple(int(v) for v in row) for row in GOLD['cases']]
CAND = (GOLD['angles'], GOLD['scales'], GOLD['trans'])


def _case(k):
    s, j, ws, flags, mt, seed = CASES[k]
    clip = GOLD[f'{chr(s)}/clips'][j]
    return clip, (ws if ws > 0 else clip.shape[1]), flags, mt, seed


def _keys(move):
    return np.stack([c[move[:, q]] for q, c in enumerate((CAND[0], CAND[1], CAND[2], CAND[2]))], axis=1)


def test_the_fixture_covers_what_it_should():
    assert len(CASES) >= 40
    assert {c[3] for c in CASES} == set(range(8)) and {c[4] for c in CASES} == {1, 3}
    assert {c[2] for c in CASES} == {8, 12, 16, -1, 1, 9}
    assert np.isnan(GOLD['A/clips'][4]).sum() == 1 and np.signbit(GOLD['A/clips'][3][:, 10]).all()


def test_default_candidates_are_the_reference_s():
    for mine in (R.default_candidates(), CF.default_candidates()):
        assert len(mine[0]) == 68
        for a, b in zip(mine, CAND):
            assert np.array_equal(np.asarray(a, dtype=np.float64), b)


@pytest.mark.parametrize('k', range(len(CASES)))
def test_restatement_against_the_reference(k):
    """With the recorded draws: the plan reproduces shift and window exactly (copied and zero elements bit-equal after the fp32
    cast), moved elements within the bound of clip_feeder_ref.MOVE_ULPS."""
    clip, W, flags, mt, _ = _case(k)
    T = clip.shape[1]
    bias, d = (int(v) for v in GOLD[f'case{k}/shift'])
    begin, end = R.extent(clip) if flags & R.SHIFT else (0, T)
    if not flags & R.CHOOSE:
        assert d == R.fixed_offset(T, W)
    if not flags & R.SHIFT:
        assert bias == 0
    pl = R.plan(begin, end, T, W, bias, d)
    assert pl == CF.make_plan(begin, end, T, W, bias, d)
    node = keys = None
    if flags & R.MOVE:
        node = R.node_table(W, mt)
        move = GOLD[f'case{k}/move']
        assert move.shape == (len(node), 4)
        keys = _keys(move)
    want, bound = R.apply(clip, pl, W, node, keys)
    ref = GOLD[f'case{k}/out']
    assert ref.shape == want.shape
    ratio = R.check(ref.astype(np.float32), want, bound, f'case {k}')
    if flags & R.MOVE:
        # every frame of the window is moved: the reference's padding comes out as (t_x, t_y, 0, ...)
        assert (bound[:2][~np.isnan(bound[:2])] > 0).any() or not np.any(want[:2])
        assert (bound[2:] == 0).all()
        print(f'case {k}: worst moved element at {ratio:.3f} of its bound')
    else:
        assert (bound == 0).all()


def test_extent_rules():
    clips = GOLD['A/clips']
    assert [R.extent(c) for c in clips] == [(3, 10), (0, 12), (0, 12), (1, 10), (6, 8)]
    for c in clips:                                     # the reference's own expression (tools.py:122-124)
        valid = (c != 0).sum(axis=3).sum(axis=2).sum(axis=0) > 0
        if valid.any():
            assert R.extent(c) == (int(valid.argmax()), int(len(valid) - valid[::-1].argmax()))


def test_draw_stream_reaches_every_candidate_and_both_ends_of_every_range():
    B, T, W = 4096, 12, 8
    ext = np.tile(np.array([[2, 9]]), (B, 1))           # size 7: bias on 0 .. 5; crop on 0 .. 4
    node = R.node_table(W, 1)
    pl, shift, move = R.device_draws(0, 0, ext, T, W, 7, len(node), (68, 3, 5))
    assert set(shift[:, 0].tolist()) == set(range(6)) and set(shift[:, 1].tolist()) == set(range(5))
    assert [sorted(set(move[..., q].ravel().tolist())) for q in range(4)] == [list(range(68)), [0, 1, 2], list(range(5)), list(range(5))]
    for b in (0, 1, 4095):
        assert tuple(pl[b]) == R.plan(2, 9, T, W, int(shift[b, 0]), int(shift[b, 1]))
    _, pad, _ = R.device_draws(0, 0, ext, T, 16, 2)     # padding: -p on -(W - T) .. 0; no shift: bias 0
    assert set(pad[:, 1].tolist()) == set(range(-4, 1)) and not pad[:, 0].any()
    pl0, sh0, mv0 = R.device_draws(0, 0, ext, T, W, 0)  # no flag: the centre crop
    assert mv0 is None and (sh0 == [0, 2]).all() and (pl0 == [2, 0, 8]).all()
    a = R.device_draws(5, 1, ext[:7], T, W, 7, 2, (68, 3, 5))
    b = R.device_draws(5, 2, ext[:7], T, W, 7, 2, (68, 3, 5))
    assert not np.array_equal(a[2], b[2])               # the call is part of the counter


def test_node_tables():
    assert R.node_table(10, 4).tolist() == [0, 2, 5, 8, 10] == CF.node_table(10, 4).tolist()     # 2.5 -> 2, 7.5 -> 8
    assert R.node_table(12, 1).tolist() == [0, 12]
    assert R.node_table(1, 3).tolist() == [0, 0, 1, 1]                                             # empty segments
    for W in (1, 7, 8, 12, 16, 52, 64, 300):
        for mt in range(1, 9):
            want = np.append(np.arange(0, W, W * 1.0 / mt).round().astype(int), W)                # reference tools.py:79-80
            assert R.node_table(W, mt).tolist() == want.tolist() == CF.node_table(W, mt).tolist()
            assert len(want) <= 10 and want[0] == 0 and (np.diff(want) >= 0).all()


def test_linspace_restated_bit_for_bit():
    rng = np.random.default_rng(0)
    for n in (1, 2, 3, 7, 8, 64, 300):
        for start, stop in [(-175.0, 180.0), (0.9, 1.1), (0.2, -0.2), (1.0, 1.0)] + rng.uniform(-180, 180, size=(8, 2)).tolist():
            assert np.array_equal(R.linspace(start, stop, n).view(np.int64), np.linspace(start, stop, n).view(np.int64)), (start, stop, n)
    assert R.linspace(1.0, 2.0, 0).size == 0


def test_moved_padding_is_the_translation():
    node, keys = R.node_table(4, 1), np.array([[90.0, 1.1, 0.1, -0.2], [90.0, 1.1, 0.1, -0.2]])
    want, bound = R.apply(np.zeros((3, 2, 1, 1)), (0, 0, 0), 4, node, keys)
    assert np.array_equal(want[0].ravel(), [0.1] * 4) and np.array_equal(want[1].ravel(), [-0.2] * 4) and not want[2].any()


def _feeder(**kw):
    args = dict(data_path=None, label_path=None, data=np.zeros((4, 3, 6, 5, 1), dtype=np.float32), labels=np.arange(4))
    args.update(kw)
    return CF.Feeder(**args)


@pytest.mark.parametrize('kw,match', [
    (dict(move_time=0), 'move_time'), (dict(move_time=9), 'move_time'), (dict(move_time=True), 'move_time'),
    (dict(window_size=2.5), 'window_size'), (dict(stream='velocity'), 'unknown stream'), (dict(stream='bone'), 'needs parent'),
    (dict(stream='motion', parent=[0, 0, 1, 5, 2]), 'needs parent'), (dict(stream='bone', parent=[0, 0, 1]), 'needs parent'),
    (dict(angle_candidate=[]), 'angle_candidate'), (dict(scale_candidate=[1.0, float('nan')]), 'scale_candidate'),
    (dict(transform_candidate=[[0.1]]), 'transform_candidate'), (dict(seed=-1), 'seed'), (dict(seed=1.5), 'seed'),
    (dict(data=np.zeros((4, 3, 6, 5))), r'\(N, C, T, V, M\)'), (dict(labels=np.arange(3)), 'labels'),
    (dict(labels=np.zeros(4)), 'labels'), (dict(data=np.zeros((4, 1, 6, 5, 1)), random_move=True), 'random_move'),
])
def test_constructor_refuses_before_it_touches_the_device(kw, match):
    with pytest.raises(ValueError, match=match):
        _feeder(**kw)


def test_ops_wrappers_refuse_host_tensors():
    import torch
    from tam_gcn_amd import ops
    with pytest.raises(RuntimeError, match='raw must be'):
        ops.clip_extent(torch.zeros(2, 3, 4, 5, 1))
    with pytest.raises(RuntimeError, match='extent must be'):
        ops.clip_draw(torch.zeros(2, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), 0, 4, 4)
    with pytest.raises(RuntimeError, match='raw must be'):
        ops.clip_transform(torch.zeros(2, 3, 4, 5, 1), torch.zeros(1, dtype=torch.int64), torch.zeros(1, 3, dtype=torch.int32), 4)


def test_abi_refuses_bad_arguments_without_a_launch():
    import ctypes as C
    from tam_gcn_amd import _lib
    lib = _lib.load()
    one = (C.c_float * 64)()
    p = C.addressof(one)
    assert lib.tamgcn_clip_extent(None, 1, 3, 4, 5, 1, p, None) < 0 and b'tamgcn_clip_extent' in lib.tamgcn_last_error()
    assert lib.tamgcn_clip_extent(p, 0, 3, 4, 5, 1, p, None) < 0 and b'bad dims' in lib.tamgcn_last_error()
    assert lib.tamgcn_clip_draw(p, 1, p, 1, None, p, 8, 4, 4, 0, 0, 0, 0, None, None, None, p, p, None, None, None, None) < 0
    assert b'flags' in lib.tamgcn_last_error()
    assert lib.tamgcn_clip_draw(p, 1, p, 1, None, p, 4, 4, 4, 17, 1, 1, 1, None, None, None, p, p, p, None, None, None) < 0
    assert b'num_node' in lib.tamgcn_last_error()
    assert lib.tamgcn_clip_transform(p, 1, p, p, p, None, 2, 1, 3, 4, 4, 5, 1, p, None) < 0 and b'go together' in lib.tamgcn_last_error()
    assert lib.tamgcn_clip_transform(p, 1, p, p, p, p, 2, 1, 1, 4, 4, 5, 1, p, None) < 0 and b'channels 0 and 1' in lib.tamgcn_last_error()
