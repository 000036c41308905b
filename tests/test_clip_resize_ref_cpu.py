"""The crop-and-resize restatement (tests/clip_resize_ref.py) against torch's own interpolate and matmul on the CPU, the ranges
and recorded values of its draws, and the library's two entry points' argument checks -- none of which needs a GPU."""
import numpy as np
import pytest
import torch

import clip_resize_ref as R
from tam_gcn_amd.feeder import clip_feeder as CF

# (L, W): one frame, fewer and more frames than the window, the two exact ratios, windows of one frame, the NTU lengths
SHAPES = [(1, 8), (5, 8), (13, 8), (8, 8), (16, 8), (2, 1), (7, 1), (1, 1),
          (300, 64), (299, 64), (257, 64), (37, 64), (64, 64), (103, 20), (1000, 64)]


def _interpolate(x, W):
    """CTR-GCN's valid_crop_resize on a crop x (C, L, V, M): (C V M, L) rows resized by F.interpolate to (C V M, W)."""
    C, L, V, M = x.shape
    t = torch.from_numpy(x).permute(0, 2, 3, 1).contiguous().view(C * V * M, L)[None, None]
    y = torch.nn.functional.interpolate(t, size=(C * V * M, W), mode='bilinear', align_corners=False).squeeze()
    return y.contiguous().view(C, V, M, W).permute(0, 3, 1, 2).contiguous().numpy()


@pytest.mark.parametrize('L,W', SHAPES)
def test_restatement_against_torch_interpolate(L, W):
    rng = np.random.default_rng(1000 * L + W)
    x = rng.uniform(-1.0, 1.0, size=(3, L + 5, 5, 2)).astype(np.float32)
    want, bound = R.resize(x, 3, L, W)
    assert want.shape == (3, W, 5, 2)
    ratio = R.check(_interpolate(x[:, 3:3 + L], W), want, bound, f'L={L} W={W}')
    print(f'L={L} W={W}: torch at {ratio:.3f} of the bound')
    if L == W:
        assert np.array_equal(want, x[:, 3:3 + L].astype(np.float64))
    if L == 2 * W:
        assert np.array_equal(want, (x[:, 3:3 + L:2].astype(np.float64) + x[:, 4:3 + L:2]) / 2)


def test_taps_are_torch_s_index_pairs_and_weights():
    """area_pixel_compute_source_index in fp64: src = max(scale (t + 0.5) - 0.5, 0), i0 = int(src), i1 = i0 + (i0 < L - 1)."""
    for L, W in SHAPES + [(12, 24), (12, 16), (3, 7)]:
        i0, i1, l1 = R.taps(L, W)
        src = np.maximum((np.arange(W) + 0.5) * (L / W) - 0.5, 0)
        near = np.abs(src - np.rint(src)) < 1e-9                      # fp64 src at an integer: either side is right
        assert np.array_equal(i0[~near], np.minimum(src.astype(np.int64), L - 1)[~near])
        assert np.array_equal(i1, np.minimum(i0 + 1, L - 1))
        assert (np.abs(i0 + l1 - src) < 1e-9)[i0 < L - 1].all() and (l1 >= 0).all() and (l1 < 1).all()
        assert i0.min() >= 0 and i1.max() <= L - 1


def test_resize_clamps_the_crop_into_the_clip():
    x = np.arange(2 * 6 * 1 * 1, dtype=np.float32).reshape(2, 6, 1, 1)
    for start, L in ((-3, 4), (4, 9), (9, 0), (0, 99), (2, -1)):
        want, _ = R.resize(x, start, L, 5)
        assert want.min() >= x.min() and want.max() <= x.max()
    assert np.array_equal(R.resize(x, 5, 9, 6)[0], x)                 # L -> 6, start -> 0: the clip itself


def test_rotation_bound_carries_the_interpolation_bound():
    rng = np.random.default_rng(5)
    x = rng.uniform(-1.0, 1.0, size=(3, 9, 2, 1)).astype(np.float32)
    y, by = R.resize(x, 0, 9, 4)
    ident, bi = R.resize(x, 0, 9, 4, np.eye(3, dtype=np.float32))
    assert np.array_equal(ident, y) and (bi >= by).all() and (bi <= by + 3.1 * R.EPS * (np.abs(y) + by)).all()
    rot = CF.rot_matrix((0.3, -0.2, 0.1))
    out, bo = R.resize(x, 0, 9, 4, rot)
    got = np.einsum('ck,ktvm->ctvm', rot, y.astype(np.float32))       # fp32 products and sums, some order
    R.check(got.astype(np.float32), out, bo, 'einsum in fp32')


def _torch_rot(angles):
    """CTR-GCN's _rot for one clip, in fp64: rz.matmul(ry).matmul(rx)."""
    a = torch.tensor(angles, dtype=torch.float64)
    c, s, one, zero = a.cos(), a.sin(), torch.ones((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    rx = torch.stack([torch.stack([one, zero, zero]), torch.stack([zero, c[0], s[0]]), torch.stack([zero, -s[0], c[0]])])
    ry = torch.stack([torch.stack([c[1], zero, -s[1]]), torch.stack([zero, one, zero]), torch.stack([s[1], zero, c[1]])])
    rz = torch.stack([torch.stack([c[2], s[2], zero]), torch.stack([-s[2], c[2], zero]), torch.stack([zero, zero, one])])
    return rz.matmul(ry).matmul(rx).numpy()


def test_matrix_against_torch_matmul():
    rng = np.random.default_rng(11)
    for angles in [(0.0, 0.0, 0.0), (0.3, 0.3, 0.3), (-0.3, 0.0, 0.3), (1.0, -2.0, 3.0)] + rng.uniform(-0.3, 0.3, size=(32, 3)).tolist():
        mine, ref = R.rot_matrix(angles), _torch_rot(angles)
        assert mine.dtype == np.float64 and np.abs(mine - ref).max() <= R.MATMUL_ULPS * 2.0 ** -53, angles
        assert np.abs(mine @ mine.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(mine) - 1) < 1e-14
        host = CF.rot_matrix(angles)                                   # the feeder's host path: the same arithmetic, rounded once
        assert host.dtype == np.float32 and np.array_equal(host.view(np.uint32), mine.astype(np.float32).view(np.uint32))
        assert (np.abs(host - mine) <= R.rot_bound(mine)).all()
    assert np.array_equal(R.rot_matrix((0.0, 0.0, 0.0)), np.eye(3))


@pytest.mark.parametrize('valid', [1, 63, 64, 65, 300])
def test_draws_stay_in_range(valid):
    B = 2048
    ext = np.tile(np.array([[7, 7 + valid]]), (B, 1))
    for p0, p1, min_crop in ((0.5, 1.0, 64), (0.5, 1.0, 1), (0.01, 0.02, 4), (1.0, 1.0, 64), (0.5, 1.0, 1000)):
        crop, drawn = R.crop_draws(3, 9, ext, R.CROP_RANDOM, p0, p1, min_crop)
        start, L = crop[:, 0].astype(np.int64), crop[:, 1].astype(np.int64)
        assert (drawn[:, 0] >= p0).all() and (drawn[:, 0] <= p1).all() and not drawn[:, 1:].any()
        assert (L >= 1).all() and (L <= valid).all() and (start >= 7).all() and (start + L <= 7 + valid).all()
        assert np.array_equal(L, np.minimum(np.maximum(np.floor(valid * drawn[:, 0]).astype(np.int64), min_crop), valid))
        if min_crop > valid:
            assert (L == valid).all() and (start == 7).all()           # min_crop > valid: the whole extent
        if valid == 300 and (p0, p1, min_crop) == (0.5, 1.0, 64):
            assert L.min() == 150 and L.max() == 299 and (start - 7).min() == 0 and (start - 7 + L).max() == 300
    for p in (1.0, 0.95, 0.5, 0.01, 1e-9):
        crop, drawn = R.crop_draws(3, 9, ext[:2], 0, p, p)
        bias, L = crop[0, 0] - 7, crop[0, 1]
        assert (bias, L) == R.centre_crop(valid, p) == CF.crop_of(valid, p) and L >= 1 and bias >= 0 and 2 * bias + L == valid
        assert (drawn[:, 0] == p).all() and (crop[0] == crop[1]).all()
    assert R.centre_crop(300, 0.95) == (7, 286) and R.centre_crop(300, 1.0) == (0, 300)      # int((1 - 0.95) 300 / 2) = 7
    assert R.centre_crop(1, 0.5) == (0, 1) and R.centre_crop(2, 1e-9) == (0, 2) and R.centre_crop(3, 1e-9) == (1, 1)


def test_angles_cover_the_interval():
    _, drawn = R.crop_draws(1, 0, np.tile(np.array([[0, 10]]), (4096, 1)), R.ROT, 1.0, 1.0, 64, 0.3)
    a = drawn[:, 1:]
    assert (drawn[:, 0] == 1.0).all() and (a >= -0.3).all() and (a < 0.3).all()
    assert a.min() < -0.299 and a.max() > 0.299 and abs(a.mean()) < 0.01
    assert abs(np.corrcoef(a.T)[0, 1]) < 0.05 and abs(np.corrcoef(a.T)[1, 2]) < 0.05
    assert not R.crop_draws(1, 0, [(0, 10)], R.ROT, 1.0, 1.0, 64, 0.0)[1][:, 1:].any()


def test_recorded_draws():
    """(seed, call) = (2^32 + 12345, 2^32 + 5), p_interval [0.5, 1], min_crop 64, theta 0.3: the stream's definition, pinned."""
    ext = [(0, 300), (40, 221), (0, 64), (3, 4)]
    crop, drawn = R.crop_draws(2 ** 32 + 12345, 2 ** 32 + 5, ext, R.CROP_RANDOM | R.ROT, 0.5, 1.0, 64, 0.3)
    assert crop.dtype == np.int32 and crop.tolist() == [[3, 259], [70, 121], [0, 64], [3, 1]]
    want = [['0x1.bb460acf00000p-1', '0x1.c40b5d0333333p-3', '-0x1.d9fb343199999p-3', '-0x1.05eab30b33333p-2'],
            ['0x1.58df928f00000p-1', '0x1.2f56f410ccccdp-2', '0x1.7347bc0999999p-3', '0x1.0664e74000000p-6'],
            ['0x1.da92402d00000p-1', '-0x1.dfd9793333333p-9', '-0x1.df50332000000p-5', '0x1.1d5b611c00000p-2'],
            ['0x1.a0a4a06100000p-1', '-0x1.9bf6aa5333333p-3', '-0x1.01df8cf8ccccdp-2', '0x1.3239b17a66666p-2']]
    assert [[float(v).hex() for v in row] for row in drawn] == want
    assert R.rot_matrix(drawn[0, 1:]).astype(np.float32).view(np.uint32).tolist() == [
        [1064374636, 3197584540, 1042612626], [1048324533, 1064200450, 1049194673], [3194675570, 3193583304, 1064509722]]
    only_crop = R.crop_draws(2 ** 32 + 12345, 2 ** 32 + 5, ext, R.CROP_RANDOM, 0.5, 1.0, 64, 0.3)
    assert np.array_equal(only_crop[0], crop) and np.array_equal(only_crop[1][:, 0], drawn[:, 0])       # block 0 is the crop's alone
    other = R.crop_draws(2 ** 32 + 12345, 2 ** 32 + 6, ext, R.CROP_RANDOM | R.ROT, 0.5, 1.0, 64, 0.3)
    assert not np.array_equal(other[1], drawn)                                                          # the call is part of the counter


def _feeder(**kw):
    args = dict(data_path=None, label_path=None, data=np.zeros((4, 3, 6, 5, 1), dtype=np.float32), labels=np.arange(4), window_size=4)
    args.update(kw)
    return CF.Feeder(**args)


@pytest.mark.parametrize('kw,match', [
    (dict(p_interval=[0.5, 1], window_size=-1), 'window_size'), (dict(p_interval=[0.95], window_size=0), 'window_size'),
    (dict(p_interval=[0.5, 1], random_shift=True), 'excludes'), (dict(p_interval=[0.5, 1], random_choose=True), 'excludes'),
    (dict(p_interval=[0.95], random_move=True), 'excludes'),
    (dict(random_rot=True), 'needs p_interval'), (dict(p_interval=[0.5, 1], random_rot=True, data=np.zeros((4, 2, 6, 5, 1))), 'three channels'),
    (dict(p_interval=[]), 'p_interval'), (dict(p_interval=[0.1, 0.5, 1]), 'p_interval'), (dict(p_interval=[0.0, 1]), 'p_interval'),
    (dict(p_interval=[0.6, 0.5]), 'p_interval'), (dict(p_interval=[0.5, 1.5]), 'p_interval'), (dict(p_interval=[float('nan')]), 'p_interval'),
    (dict(p_interval=0.5), 'p_interval'), (dict(p_interval=['a']), 'p_interval'),
    (dict(p_interval=[0.5, 1], rot_theta=-0.1), 'rot_theta'), (dict(p_interval=[0.5, 1], rot_theta=float('inf')), 'rot_theta'),
    (dict(rot_theta=float('nan')), 'rot_theta'), (dict(rot_theta='0.3'), 'rot_theta'),
    (dict(p_interval=[0.5, 1], min_crop=0), 'min_crop'), (dict(min_crop=2.5), 'min_crop'), (dict(min_crop=True), 'min_crop'),
])
def test_constructor_refuses_before_it_touches_the_device(kw, match):
    with pytest.raises(ValueError, match=match):
        _feeder(**kw)


def test_ops_wrappers_refuse_host_tensors():
    from tam_gcn_amd import ops
    i64, i32 = torch.zeros(1, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='extent must be'):
        ops.clip_crop_draw(torch.zeros(2, 2, dtype=torch.int32), i64, torch.zeros(2, dtype=torch.int64), 0, 0.5, 1.0)
    with pytest.raises(RuntimeError, match='raw must be'):
        ops.clip_resize(torch.zeros(2, 3, 4, 5, 1), i64, i32, 4)


def test_abi_exports_the_entry_points_and_refuses_bad_arguments_without_a_launch():
    import ctypes as C
    from tam_gcn_amd import _lib
    lib = _lib.load()
    assert lib.tamgcn_version() == 401 == _lib.ABI_VERSION
    one = (C.c_float * 64)()
    p = C.addressof(one)
    err = lib.tamgcn_last_error

    def draw(extent=p, n_clips=1, ids=p, B=1, labels=None, state=p, flags=3, p0=0.5, p1=1.0, min_crop=64, theta=0.3, crop=p, drawn=p,
             rot=p, labels_out=None):
        return lib.tamgcn_clip_crop_draw(extent, n_clips, ids, B, labels, state, flags, p0, p1, min_crop, theta, crop, drawn, rot, labels_out, None)

    for kw in (dict(extent=None), dict(ids=None), dict(state=None), dict(crop=None), dict(drawn=None)):
        assert draw(**kw) < 0 and b'tamgcn_clip_crop_draw: null pointer' in err(), kw
    for kw, what in ((dict(B=0), b'bad dims'), (dict(B=-1), b'bad dims'), (dict(n_clips=0), b'bad dims'), (dict(flags=4), b'flags'),
                     (dict(flags=-1), b'flags'), (dict(p0=0.0), b'p0'), (dict(p0=0.7, p1=0.6), b'p0'), (dict(p1=1.5), b'p0'),
                     (dict(p0=float('nan')), b'p0'), (dict(min_crop=0), b'min_crop'), (dict(theta=-1.0), b'theta'),
                     (dict(theta=float('inf')), b'theta'), (dict(theta=float('nan')), b'theta'), (dict(rot=None), b'needs rot'),
                     (dict(labels=p), b'go together'), (dict(labels_out=p), b'go together')):
        assert draw(**kw) < 0 and what in err(), (kw, err())

    def resize(raw=p, n_clips=1, ids=p, crop=p, rot=None, B=1, C_=3, T=4, W=4, V=5, M=1, out=p):
        return lib.tamgcn_clip_resize(raw, n_clips, ids, crop, rot, B, C_, T, W, V, M, out, None)

    for kw in (dict(raw=None), dict(ids=None), dict(crop=None), dict(out=None)):
        assert resize(**kw) < 0 and b'tamgcn_clip_resize: null pointer' in err(), kw
    for kw in (dict(B=0), dict(n_clips=0), dict(C_=0), dict(T=0), dict(W=0), dict(W=-4), dict(V=0), dict(M=-1)):
        assert resize(**kw) < 0 and b'bad dims' in err(), kw
    assert resize(T=2 ** 30, V=2) < 0 and b'2^30' in err()
    assert resize(rot=p, C_=2) < 0 and b'three channels' in err()
