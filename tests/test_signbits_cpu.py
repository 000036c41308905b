"""ReLU sign bits without a GPU: the bit layout as a numpy statement (the reference the GPU tests import) and the route
predicate of TCN_GCN_unit's backward.

Layout (include/tamgcn.h, tamgcn_conv_signmask): an (N, C, T, V) tensor has N*C rows of L = T*V floats; a row has
ceil(L / 4) bytes; byte i holds the elements 4i .. 4i+3 in bits 0 .. 3, bits 4 .. 7 are 0; a bit is 1 iff the element is > 0
(-0.0, +0.0 and NaN give 0)."""
import numpy as np
import pytest


def row_bytes(L):
    return (L + 3) // 4


def pack_bits(x, ge=False):
    """x (N, C, T, V) float32 -> (N, C, ceil(T*V / 4)) uint8.  ge: the DEFECT `>= 0` in place of `> 0` (defect variants only)."""
    x = np.asarray(x, dtype=np.float32)
    N, C, T, V = x.shape
    L = T * V
    with np.errstate(invalid='ignore'):
        on = (x >= 0) if ge else (x > 0)
    on = on.reshape(N, C, L)
    pad = np.zeros((N, C, 4 * row_bytes(L)), dtype=bool)
    pad[:, :, :L] = on
    g = pad.reshape(N, C, row_bytes(L), 4).astype(np.uint8)
    return (g[..., 0] | (g[..., 1] << 1) | (g[..., 2] << 2) | (g[..., 3] << 3)).astype(np.uint8)


def unpack_bits(bits, T, V):
    """(N, C, ceil(T*V / 4)) uint8 -> (N, C, T, V) bool."""
    bits = np.asarray(bits, dtype=np.uint8)
    N, C, nb = bits.shape
    L = T * V
    assert nb == row_bytes(L)
    on = np.stack([(bits >> k) & 1 for k in range(4)], axis=-1).reshape(N, C, 4 * nb)[:, :, :L]
    return on.astype(bool).reshape(N, C, T, V)


def shift_one_group(bits):
    """The DEFECT of a bit array addressed one group late: byte i of a row holds what belongs to byte i - 1."""
    return np.roll(np.asarray(bits), 1, axis=-1)


def special_values():
    """What a ReLU output can hold around the mask's edge: exact zeros of both signs, a denormal, a NaN, ordinary values."""
    return np.array([0.0, -0.0, 1e-45, np.nan, 1.5, -2.25, 3.0e-3, -7.0], dtype=np.float32)


@pytest.mark.parametrize('shape', [(2, 5, 4, 20), (2, 5, 3, 25), (1, 3, 90, 20), (1, 1, 1, 1)])
def test_pack_and_unpack_are_inverse_and_sized(shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape).astype(np.float32)
    x.reshape(-1)[:8] = special_values()[:x.size][:8] if x.size >= 8 else special_values()[:x.size]
    b = pack_bits(x)
    N, C, T, V = shape
    assert b.shape == (N, C, row_bytes(T * V)) and b.dtype == np.uint8
    assert 16 * b.nbytes <= x.nbytes + 16 * 4 * N * C          # at most 1/16 of the tensor (+ the partial last group of a row)
    assert (b >> 4).max() == 0
    with np.errstate(invalid='ignore'):
        assert np.array_equal(unpack_bits(b, T, V), x > 0)


def test_zero_signs_denormal_and_nan():
    x = special_values().reshape(1, 1, 1, 8)
    on = unpack_bits(pack_bits(x), 1, 8).reshape(-1)
    assert on.tolist() == [False, False, True, False, True, False, True, False]
    # the defect variants differ from the layout on this very input
    assert unpack_bits(pack_bits(x, ge=True), 1, 8).reshape(-1).tolist() != on.tolist()
    assert not np.array_equal(shift_one_group(pack_bits(x)), pack_bits(x))


def test_partial_last_group_uses_the_low_bits():
    x = np.ones((1, 1, 3, 25), dtype=np.float32)              # L = 75: 18 whole groups and three elements
    b = pack_bits(x)
    assert b.shape[-1] == 19 and b[0, 0, :18].tolist() == [15] * 18 and b[0, 0, 18] == 7


# The blocks of the unit tests.  The GEMM in question is the data gradient of the MS-TCN's plain 1x1 branch: K = Cb = Cout / 4
# channels of the block's output gradient into M = Cin = Cout channels of g (the unit_gcn output the MS-TCN reads)
ROUTES = [
    ('64->64 identity', dict(stride=1, N=2, Cb=16, Cin=64, T=8, V=20), 'a'),
    ('64->128 stride 2', dict(stride=2, N=2, Cb=32, Cin=128, T=8, V=20), 'b'),       # the GEMM writes every other frame of dg
    ('3->64 no residual', dict(stride=1, N=2, Cb=16, Cin=64, T=8, V=20), 'a'),       # g has 64 channels whatever x has
    ('24 channels', dict(stride=1, N=2, Cb=6, Cin=24, T=8, V=20), 'b'),              # not whole 16-row chunks
    ('64->64 V=25', dict(stride=1, N=2, Cb=16, Cin=64, T=8, V=25), 'b'),             # rows of 25 floats: no 16-byte groups
    ('128->128', dict(stride=1, N=2, Cb=32, Cin=128, T=8, V=20), 'a'),
    ('256->256', dict(stride=1, N=256, Cb=64, Cin=256, T=13, V=20), 'a'),
    ('short clip', dict(stride=1, N=2, Cb=16, Cin=64, T=2, V=20), 'b'),              # 40 columns: below the GEMM's tile
]


@pytest.mark.parametrize('name,kw,want', ROUTES, ids=[r[0] for r in ROUTES])
def test_route_predicate(name, kw, want):
    from tam_gcn_amd import functional as F
    assert F.signmask_route(have_bits=True, **kw) == want
    assert F.signmask_route(have_bits=False, **kw) is None     # TAMGCN_SIGNBITS=0: today's kernels
    # split mode 1 sends data gradients into >= 128 channels to the bf16 split kernel, which has no mask mode
    want1 = 'b' if (want == 'a' and kw['Cin'] >= 128) else want
    assert F.signmask_route(have_bits=True, split_mode=1, **kw) == want1

