"""tamgcn_conv_pair / tamgcn_wgrad_pair refuse bad descriptors before any HIP call, with a message that names the entry point
(no GPU needed).  The refusals that print descriptor fields double as a check of the binding's struct layouts: the values
the library reads back are the ones the ctypes structs were given."""
import ctypes as C
import importlib

import pytest


@pytest.fixture(scope='module')
def lib():
    from tam_gcn_amd import build, _lib
    build.build()
    return _lib.load()


_buf = (C.c_float * 64)()           # a 16-byte aligned host address: the checks never dereference it


def _addr():
    a = C.addressof(_buf)
    return a + (-a) % 16


def _src(ctot, coff=0, two=False):
    from tam_gcn_amd import _lib
    p = _addr()
    return _lib.Src(p, p if two else None, p if two else None, ctot, coff, 0)


def _conv_desc():
    """A descriptor every argument check accepts: (N, Cin, Cb, T, V) = (3, 64, 16, 20, 20), three stacked entry branches."""
    from tam_gcn_amd import _lib
    p = _addr()
    d = _lib.ConvPairDesc()
    d.N, d.T, d.V, d.stride = 3, 20, 20, 1
    d.w0 = d.w1 = d.y0 = d.y1 = p
    d.src = _src(64)
    d.K, d.M0, d.M1 = 64, 48, 16
    d.yctot0, d.ycoff0, d.yctot1, d.ycoff1 = 48, 0, 64, 48
    return d


def _wgrad_desc():
    from tam_gcn_amd import _lib
    d = _lib.WgradPairDesc()
    d.gy0, d.gy1, d.src = _src(48, two=True), _src(64, 48, two=True), _src(64)
    d.N, d.M0, d.M1, d.K, d.T, d.V, d.stride = 3, 48, 16, 64, 20, 20, 1
    d.part, d.nsplit = _addr(), 1
    return d


def _refused(lib, fn, d, text=None):
    rc = getattr(lib, fn)(C.byref(d) if d is not None else None, None)
    msg = lib.tamgcn_last_error()
    assert rc < 0, (fn, rc)
    assert fn.encode() + b':' in msg, msg
    if text:
        assert text.encode() in msg, msg


def test_null_descriptors_are_refused(lib):
    _refused(lib, 'tamgcn_conv_pair', None, 'null descriptor')
    _refused(lib, 'tamgcn_wgrad_pair', None, 'null descriptor')
    for field in ('w0', 'w1', 'y0', 'y1'):
        d = _conv_desc()
        setattr(d, field, None)
        _refused(lib, 'tamgcn_conv_pair', d, 'null pointer')
    d = _wgrad_desc()
    d.part = None
    _refused(lib, 'tamgcn_wgrad_pair', d, 'null pointer')


def test_the_library_reads_the_fields_the_binding_wrote(lib):
    """Struct layouts: distinct values in every integer field in front of and behind the embedded tamgcn_src structs come
    back in the refusals that print them."""
    d = _conv_desc()
    d.N, d.T, d.V, d.K, d.M0, d.M1 = -7, 11, 13, 17, 23, 29
    _refused(lib, 'tamgcn_conv_pair', d, 'bad dims N=-7 T=11 V=13 K=17 M0=23 M1=29')
    d = _conv_desc()
    d.stride = 5
    _refused(lib, 'tamgcn_conv_pair', d, 'stride 5')
    w = _wgrad_desc()
    w.N, w.M0, w.M1, w.K, w.T, w.V, w.nsplit = -7, 23, 29, 17, 11, 13, 31
    _refused(lib, 'tamgcn_wgrad_pair', w, 'bad dims N=-7 M0=23 M1=29 K=17 T=11 V=13 nsplit=31')
    w = _wgrad_desc()
    w.stride = 5
    _refused(lib, 'tamgcn_wgrad_pair', w, 'stride 5')


def test_an_empty_second_part_is_refused(lib):
    d = _conv_desc()
    d.M1 = 0
    _refused(lib, 'tamgcn_conv_pair', d, 'M1 = 0')
    d = _wgrad_desc()
    d.M1 = 0
    _refused(lib, 'tamgcn_wgrad_pair', d, 'M1 = 0')


def test_a_contraction_off_the_chunk_is_refused(lib):
    d = _conv_desc()
    d.K = 56                            # chunks of 16 contraction rows
    _refused(lib, 'tamgcn_conv_pair', d, 'multiple of the chunk')
    d = _wgrad_desc()
    d.M0 = 44                           # the gradient operand is fetched in pieces of eight rows
    _refused(lib, 'tamgcn_wgrad_pair', d, '8-row pieces')


def test_a_strided_pair_is_refused(lib):
    d = _conv_desc()
    d.stride = 2
    _refused(lib, 'tamgcn_conv_pair', d, 'stride 2')
    w = _wgrad_desc()
    w.stride = 2
    _refused(lib, 'tamgcn_wgrad_pair', w, 'stride 2')


def test_a_slice_out_of_range_is_refused(lib):
    d = _conv_desc()
    d.ycoff1 = 49                       # 49 + 16 > 64 channels of the second destination
    _refused(lib, 'tamgcn_conv_pair', d, 'destination slice out of range')
    d = _conv_desc()
    d.yctot0 = 47
    _refused(lib, 'tamgcn_conv_pair', d, 'destination slice out of range')
    d = _conv_desc()
    d.src.coff = 1
    _refused(lib, 'tamgcn_conv_pair', d, 'source channel slice out of range')
    w = _wgrad_desc()
    w.gy1.coff = 49
    _refused(lib, 'tamgcn_wgrad_pair', w, 'channel slice out of range')


def test_moments_for_one_part_only_are_refused(lib):
    d = _conv_desc()
    d.stats_part0 = _addr()
    _refused(lib, 'tamgcn_conv_pair', d, 'moments')
    d = _conv_desc()
    d.stats_part0 = d.stats_part1 = _addr()
    d.stats_ctot0, d.stats_coff0, d.stats_ctot1, d.stats_coff1 = 48, 0, 64, 49
    _refused(lib, 'tamgcn_conv_pair', d, 'moment slice out of range')


def test_too_many_splits_are_refused(lib):
    from tam_gcn_amd import _lib
    w = _wgrad_desc()
    sd = _lib.WgradDesc()
    sd.gy, sd.src = w.gy0, w.src
    sd.N, sd.M, sd.K, sd.T_in, sd.T_out, sd.V, sd.KT, sd.dil, sd.stride, sd.pad = 3, 64, 64, 20, 20, 20, 1, 1, 1, 0
    w.nsplit = lib.tamgcn_wgrad_max_split(C.byref(sd)) + 1
    _refused(lib, 'tamgcn_wgrad_pair', w, 'exceeds tamgcn_wgrad_max_split')


def test_a_one_source_gradient_operand_is_refused(lib):
    w = _wgrad_desc()
    w.gy1.x2 = None
    _refused(lib, 'tamgcn_wgrad_pair', w, 'two-source prologue')


def test_the_switch_is_read_when_the_op_layer_is_imported(monkeypatch):
    """TAMGCN_TCN_PAIR=0 at import selects the two-launch path; unset, the paired one; a change of the variable afterwards does
    nothing until the module is executed again."""
    from tam_gcn_amd import ops
    try:
        monkeypatch.setenv('TAMGCN_TCN_PAIR', '0')
        importlib.reload(ops)
        assert ops.TCN_PAIR is False
        monkeypatch.delenv('TAMGCN_TCN_PAIR')
        assert ops.TCN_PAIR is False                # read once: not followed
        importlib.reload(ops)
        assert ops.TCN_PAIR is True
        monkeypatch.setenv('TAMGCN_TCN_PAIR', '1')
        importlib.reload(ops)
        assert ops.TCN_PAIR is True
    finally:
        monkeypatch.undo()
        importlib.reload(ops)


def test_the_pairing_predicate_admits_only_what_the_kernels_serve():
    """ops.pair_supported() is the conservative side of the library's plan (its docstring): shapes off the LDS-DMA kernels
    take the two launches instead of reaching a refusal."""
    from tam_gcn_amd import ops

    class T_:                                        # stands in for a 16-byte aligned contiguous device tensor
        is_cuda = True

        def __init__(self, ptr=256):
            self._p = ptr

        def is_contiguous(self):
            return True

        def data_ptr(self):
            return self._p
    ok = (T_(), None)
    assert ops.pair_supported(ok, 256, (64, 64), 64, 20)
    assert not ops.pair_supported(ok, 256, (64, 64), 64, 25)            # rows not whole 16-byte slots
    assert not ops.pair_supported(ok, 256, (64, 64), 8, 64)             # joint slices
    assert not ops.pair_supported(ok, 2, (64, 64), 3, 20)               # fewer than 64 columns
    assert not ops.pair_supported(ok, 2, (40, 64), 16, 20)              # K not in whole chunks
    assert not ops.pair_supported(ok, 2, (64, 1024), 16, 20)            # past the LDS bound the plan's tile rests on
    assert not ops.pair_supported((T_(260),), 2, (64, 64), 16, 20)      # misaligned operand
    assert not ops.pair_supported(ok, 2 ** 20, (512, 512), 64, 20)      # the batch would be split over launches
