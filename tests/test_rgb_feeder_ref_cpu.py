"""The RGB feeder without a GPU: the numpy restatement (tests/rgb_feeder_ref.py) against Pillow and against the recorded fixture
(tests/golden/rgb_feeder.npz, made from the reference by make_golden_rgb_feeder.py), the host-side tables of
tam_gcn_amd/feeder/rgb_feeder.py, and the derivation of libtamgcn_rgb.so's binding from include/tamgcn_rgb.h."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import rgb_feeder_ref as R
from tam_gcn_amd import _abi, _lib, _rgb_lib, _xm_lib, build
from tam_gcn_amd.feeder import rgb_feeder as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rgb_feeder.npz')


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def test_restatement_equals_pil_byte_for_byte():
    Image = pytest.importorskip('PIL.Image')
    for H, W, S in R.PIL_SHAPES:
        img = np.random.RandomState(1000 * H + W).randint(0, 256, size=(H, W, 3), dtype=np.uint8)
        want = np.asarray(Image.fromarray(img).resize((S, S), Image.BILINEAR))
        assert np.array_equal(R.resize(img, S), want), (H, W, S)
        # on the same images the flip commutes with the resize
        flipped = np.asarray(Image.fromarray(img).transpose(Image.FLIP_LEFT_RIGHT).resize((S, S), Image.BILINEAR))
        assert np.array_equal(R.resize(img, S)[:, ::-1], flipped), (H, W, S)


def test_feeder_tables_equal_the_restatement():
    for n_in, n_out in {(W, S) for _, W, S in R.PIL_SHAPES} | {(H, S) for H, _, S in R.PIL_SHAPES} | {(1, 5), (5, 1), (1000, 3)}:
        a, b = F.pil_bilinear_tables(n_in, n_out), R.tables(n_in, n_out)
        assert a[0].dtype == np.int32 and a[1].dtype == np.int32
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (n_in, n_out)
        assert a[0].shape[1] <= _rgb_lib.MAX_TAPS or n_in > 31 * n_out
        lo, cnt = a[1][:, 0], a[1][:, 1]
        assert (lo >= 0).all() and (cnt >= 1).all() and (lo + cnt <= n_in).all() and (cnt <= a[0].shape[1]).all()
        assert (np.abs(a[0].sum(axis=1) - (1 << 22)) <= a[0].shape[1]).all()          # 255 * sum < 2^31


def test_restatement_equals_the_fixture(golden):
    Fr = int(golden['F'])
    table = R.lut()
    for name in golden['names']:
        src, S = golden[f'{name}/src'], int(golden[f'{name}/size'])
        store = R.resize(src, S)
        assert np.array_equal(store, golden[f'{name}/resized']), name
        out = R.batch(store[None], [0], table, Fr)
        assert out.shape == (1, 3 * Fr, S, S)
        assert np.array_equal(out.reshape(-1)[golden[f'{name}/idx']], golden[f'{name}/sample']), name
        fl = R.batch(store[None], [0], table, 1, flip=[1])
        assert np.array_equal(fl.reshape(-1)[golden[f'flip/{name}/idx']], golden[f'flip/{name}/sample']), name
    assert bool(golden['absent/all_zero']) and str(golden['absent/dtype']) == 'float32'
    shape = tuple(int(v) for v in golden['absent/shape'])
    gone = R.batch(np.zeros((1, shape[1], shape[2], 3), dtype=np.uint8), [0], table, Fr, missing=[1], missing_mode=0)
    assert gone.shape == (1,) + shape and not gone.any()
    black = R.batch(np.full((1, 4, 4, 3), 9, dtype=np.uint8), [0], table, 1, missing=[1], missing_mode=1)
    assert np.array_equal(black[0], np.broadcast_to(table[:, 0][:, None, None], (3, 4, 4)))


def test_normalise_table_equals_totensor_and_normalize_in_torch():
    table = F.normalise_table()
    assert table.dtype == torch.float32 and tuple(table.shape) == (3, 256) and table.is_contiguous()
    pic = torch.arange(256, dtype=torch.uint8).view(1, 256, 1).expand(16, 256, 3).contiguous()       # HWC, byte v in column v
    t = pic.permute(2, 0, 1).contiguous().to(torch.float32).div(255)                                 # ToTensor
    mean, std = torch.as_tensor(F.IMAGENET_MEAN, dtype=torch.float32), torch.as_tensor(F.IMAGENET_STD, dtype=torch.float32)
    t = t.clone().sub_(mean[:, None, None]).div_(std[:, None, None])                                 # Normalize
    for row in range(16):
        assert torch.equal(t[:, row, :], table)
    assert np.array_equal(table.numpy(), R.lut())
    other = F.normalise_table((0.5, 0.25, 0.0), (0.5, 2.0, 1.0))
    assert torch.equal(other[2], torch.arange(256, dtype=torch.float32).div(255))
    with pytest.raises(ValueError):
        F.normalise_table((0, 0, 0), (1, 0, 1))


def test_mirror_symmetry_of_the_tables_and_the_refusal_that_follows():
    for W in range(2, 700):
        assert F.tables_mirror_symmetric(*F.pil_bilinear_tables(W, 224), W), W
    coef, bounds = F.pil_bilinear_tables(53, 16)
    assert F.tables_mirror_symmetric(coef, bounds, 53)
    bent = coef.copy()
    bent[3, 1] += 1
    assert not F.tables_mirror_symmetric(bent, bounds, 53)
    # a table that is not symmetric resamples a flipped row to something else than the flipped resample
    row = np.random.RandomState(5).randint(0, 256, size=(1, 53, 3), dtype=np.uint8)
    assert np.array_equal(R.resample_axis(row[:, ::-1], 1, coef, bounds), R.resample_axis(row, 1, coef, bounds)[:, ::-1])
    far = coef.copy()
    far[3, 1] += 1 << 16                                                   # 255 * 2^16 >> 22 = 3: enough to move a byte
    assert not F.tables_mirror_symmetric(far, bounds, 53)
    big = np.zeros((1, 53, 3), dtype=np.uint8)
    big[0, bounds[3, 0] + 1] = 255
    assert not np.array_equal(R.resample_axis(big[:, ::-1], 1, far, bounds), R.resample_axis(big, 1, far, bounds)[:, ::-1])


def test_the_feeder_refuses_a_flip_over_an_asymmetric_table(monkeypatch):
    """the ValueError is raised before anything touches the device"""
    real = F.pil_bilinear_tables

    def bent(n_in, n_out):
        coef, bounds = real(n_in, n_out)
        if n_in == 53:
            coef = coef.copy()
            coef[3, 1] += 1
        return coef, bounds
    monkeypatch.setattr(F, 'pil_bilinear_tables', bent)
    images = [np.zeros((37, 53, 3), dtype=np.uint8), np.zeros((16, 16, 3), dtype=np.uint8), np.zeros((20, 31, 3), dtype=np.uint8)]
    with pytest.raises(ValueError, match=r'widths \[53\]'):
        F.RGBFeeder(images, [0, 1, 2], size=16, random_flip=True, train=True)
    for kw in (dict(size=0), dict(temporal_rgb_frames=0), dict(missing_as='grey'), dict(seed=-1)):
        with pytest.raises(ValueError):
            F.RGBFeeder(images, [0, 1, 2], **{'size': 16, **kw})
    with pytest.raises(ValueError, match='labels'):
        F.RGBFeeder(images, [0, 1], size=16)
    with pytest.raises(ValueError, match='image 1'):
        F.RGBFeeder([images[0], images[1].astype(np.float32)], [0, 1], size=16)


def test_the_header_derives_and_the_other_bindings_are_untouched():
    structs, funcs, rets, defines = _abi.parse_abi(_rgb_lib.RGB_HEADER)
    classes, sigs, defs = _lib.derive(_rgb_lib.RGB_HEADER, ())
    assert structs == {} and classes == {} and defs['TAMGCN_RGB_VERSION'] == _rgb_lib.RGB_VERSION == defines['TAMGCN_RGB_VERSION'] == 1
    assert defs['TAMGCN_RGB_MAX_TAPS'] == _rgb_lib.MAX_TAPS == 64
    assert set(sigs) == set(_rgb_lib.SIGNATURES) == {'tamgcn_rgb_version', 'tamgcn_rgb_last_error', 'tamgcn_rgb_resize', 'tamgcn_rgb_draw',
                                                    'tamgcn_rgb_batch'}
    assert sigs['tamgcn_rgb_last_error'] == (C.c_char_p, []) and sigs['tamgcn_rgb_version'] == (C.c_int, [])
    v, i, ll, f = C.c_void_p, C.c_int, C.c_longlong, C.c_float
    assert sigs['tamgcn_rgb_resize'] == (i, [v, i, i, i, i, i, v, v, i, v, v, i, v, v, v])
    assert sigs['tamgcn_rgb_draw'] == (i, [v, i, v, v])
    assert sigs['tamgcn_rgb_batch'] == (i, [v, ll, i, v, i, v, v, v, i, v, i, v, v, v, v])
    kinds = {d.name: (d.kind, d.base) for d in funcs['tamgcn_rgb_batch']}
    assert kinds['store'] == ('r', 'unsigned char') and kinds['out'] == ('w', 'float') and kinds['stream'] == ('stream', 'void')
    assert all(fn.startswith('tamgcn_rgb_') for fn in sigs)
    assert not set(sigs) & set(_lib.SIGNATURES) and not set(sigs) & set(_xm_lib.SIGNATURES)
    assert len(_lib.SIGNATURES) == 137 and _xm_lib.XM_VERSION == 1
    assert 'libtamgcn_rgb.so' in build.RGB_LIB and not set(build.RGB_SRC) & (set(build.SRC) | set(build.XM_SRC))


@pytest.fixture(scope='module')
def rgb():
    build.build(verbose=False)
    return _rgb_lib.load()


def test_the_library_exports_every_declared_symbol(rgb):
    assert not build.needs_build_rgb() and not build.needs_build_xmodal() and not build.needs_build()
    raw = C.CDLL(build.RGB_LIB)
    for name in _rgb_lib.SIGNATURES:
        assert hasattr(raw, name), name
    assert rgb.tamgcn_rgb_version() == _rgb_lib.RGB_VERSION == 1


def test_every_entry_point_refuses_bad_arguments_before_any_launch(rgb):
    """no GPU is needed: a refused call returns before it touches the runtime.  q is an address-like integer that is never read."""
    q, r, s, odd = 0x10000, 0x20000, 0x30000, 0x10002
    err = lambda: rgb.tamgcn_rgb_last_error().decode()                    # noqa: E731

    def resize(src=q, n=1, H0=8, W0=8, Ho=4, Wo=4, ch=q, bh=q, Kh=5, cv=q, bv=q, Kv=5, tmp=r, dst=s):
        return rgb.tamgcn_rgb_resize(src, n, H0, W0, Ho, Wo, ch, bh, Kh, cv, bv, Kv, tmp, dst, None)
    for kw, word in ((dict(src=None), 'NULL'), (dict(dst=None), 'NULL'), (dict(n=0), 'n = 0'), (dict(Wo=0), 'Wo = 0'), (dict(Kh=65), 'Kh = 65'),
                     (dict(Kv=0), 'Kv = 0'), (dict(ch=None), 'go together'), (dict(bv=None), 'go together'), (dict(ch=None, bh=None), 'W0 = 8'),
                     (dict(cv=None, bv=None), 'H0 = 8'), (dict(tmp=None), 'tmp'), (dict(dst=q), 'overlap'), (dict(tmp=q), 'overlap'),
                     (dict(n=4096, H0=1024, W0=1024), '2^31')):
        assert resize(**kw) == -1 and 'tamgcn_rgb_resize' in err() and word in err(), (kw, err())

    def draw(state=q, B=4, flip=r):
        return rgb.tamgcn_rgb_draw(state, B, flip, None)
    for kw, word in ((dict(state=None), 'NULL'), (dict(flip=None), 'NULL'), (dict(B=0), 'B = 0'), (dict(state=q + 4), 'aligned'),
                     (dict(flip=odd), 'aligned')):
        assert draw(**kw) == -1 and 'tamgcn_rgb_draw' in err() and word in err(), (kw, err())

    def batch(store=q, n=3, S=8, ids=r, B=2, lut=s, flip=None, missing=None, mode=0, row_scale=None, Fr=1, labels=None, labels_out=None, out=q):
        return rgb.tamgcn_rgb_batch(store, n, S, ids, B, lut, flip, missing, mode, row_scale, Fr, labels, labels_out, out, None)
    for kw, word in ((dict(store=None), 'NULL'), (dict(ids=None), 'NULL'), (dict(lut=None), 'NULL'), (dict(out=None), 'NULL'), (dict(n=0), 'n = 0'),
                     (dict(S=0), 'S = 0'), (dict(B=0), 'B = 0'), (dict(Fr=0), 'F = 0'), (dict(B=65536, S=256), '2^31'), (dict(mode=2), 'missing_mode'),
                     (dict(labels=q), 'go together'), (dict(labels_out=q), 'go together'), (dict(ids=odd), 'aligned'), (dict(out=odd), 'aligned'),
                     (dict(row_scale=odd), 'aligned'), (dict(flip=odd), 'aligned')):
        assert batch(**kw) == -1 and 'tamgcn_rgb_batch' in err() and word in err(), (kw, err())


def test_a_missing_library_is_an_error_not_a_fallback(monkeypatch, tmp_path):
    monkeypatch.setattr(_rgb_lib, '_rgb', None)
    monkeypatch.setenv('TAMGCN_RGB_LIB', str(tmp_path / 'absent.so'))
    with pytest.raises(_lib.TamgcnLibraryError, match='not built'):
        _rgb_lib.load()


def test_load_images_on_a_temporary_directory(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    a, b = R.smooth_images(3, 1, 9, 13)[0], R.smooth_images(4, 1, 6, 5)[0]
    Image.fromarray(a).save(tmp_path / 'a.png')
    Image.fromarray(b).save(tmp_path / 'b.jpg', quality=95)
    Image.fromarray(a[:, :, 0]).save(tmp_path / 'grey.png')               # mode L: convert('RGB') makes three equal channels
    (tmp_path / 'broken.png').write_bytes(b'not an image')
    images, missing = F.load_images(str(tmp_path), ['a', 'b', 'absent', 'grey', 'broken'])
    assert missing.dtype == np.bool_ and missing.tolist() == [False, False, True, False, True]
    assert all(im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3 and im.flags['C_CONTIGUOUS'] for im in images)
    assert np.array_equal(images[0], a)
    with Image.open(tmp_path / 'b.jpg') as im:
        assert np.array_equal(images[1], np.asarray(im.convert('RGB'))) and images[1].shape == (6, 5, 3)
    assert np.array_equal(images[3], np.repeat(a[:, :, :1], 3, axis=2))
    assert images[2].shape == (1, 1, 3) and not images[2].any() and not images[4].any()


def test_philox_flips_are_a_fair_deterministic_stream():
    a = R.flips(7, 3, 4096)
    assert a.dtype == np.int32 and set(np.unique(a)) == {0, 1} and np.array_equal(a, R.flips(7, 3, 4096))
    assert abs(int(a.sum()) - 2048) < 4 * 32                              # four standard deviations of Binomial(4096, 1/2)
    assert not np.array_equal(a, R.flips(7, 4, 4096)) and not np.array_equal(a, R.flips(8, 3, 4096))
    assert np.array_equal(R.flips(7, 3, 8), a[:8])
