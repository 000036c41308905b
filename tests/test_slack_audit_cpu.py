"""The read-slack audit without a GPU (tests/slack_audit.py; DESIGN.md, "Read slack behind streamed activations"): the
classification table against the header and the kernel sources, the checker's teeth on a stand-in library with CPU tensors,
and ops.with_slack itself."""
import ctypes as C

import pytest
import torch

import slack_audit as S
import stream_audit as A
from tam_gcn_amd import _lib, ops


# =====================================================================================================================
# completeness
# =====================================================================================================================
def test_every_const_float_pointer_has_one_class():
    assert S.classification_problems() == []
    want = S.float_read_pointers()
    assert len(want) == len(set(want)) == len(S.CLASSES)
    assert {e.cls for e in S.CLASSES.values()} == {S.STREAM, S.GUARDED, S.FLAT}


def test_the_table_covers_the_binding():
    """Every `r` float pointer of _lib.SIGNATURES and of the ctypes structs: the header is the binding (completeness_problems), and
    the table is the header."""
    assert A.completeness_problems(_lib) == []
    structs, funcs = A.parse_header()
    n = 0
    for name, (_, argtypes) in _lib.SIGNATURES.items():
        for ct, d in zip(argtypes, funcs[name]):
            if ct is C.c_void_p and d.kind == 'r' and d.base == 'float':
                assert (name, d.name) in S.CLASSES, (name, d.name)
                n += 1
            if A._is_pointer_type(ct) and ct._type_ is _lib.Src:
                assert all((name, f'{d.name}.{f}') in S.CLASSES for f in ('x1', 'x2', 'coef')), (name, d.name)
                n += 3
            if A._is_pointer_type(ct) and ct._type_ is C.c_float:       # a host array of floats (tamgcn_score_sweep's alphas)
                assert S.CLASSES[(name, d.name)].cls == S.FLAT
                n += 1
    for h, cls in _lib.STRUCTS.items():
        if h == 'tamgcn_src':
            continue
        for (fname, ct), d in zip(cls._fields_, structs[h]):
            base = ct._type_ if A._is_array_type(ct) else ct
            if base is C.c_void_p and d.kind == 'r' and d.base == 'float':
                assert (h, fname) in S.CLASSES, (h, fname)
                n += 1
            if base is _lib.Src or (A._is_pointer_type(base) and base._type_ is _lib.Src):
                assert all((h, f'{fname}.{f}') in S.CLASSES for f in ('x1', 'x2', 'coef')), (h, fname)
                n += 3
    assert n == len(S.CLASSES)


def test_a_new_header_pointer_without_a_class_is_reported(tmp_path):
    text = open(A.HEADER).read()
    text = text.replace('int tamgcn_tmean(', 'int tamgcn_new_stream_op(const float* fresh, int V, void* stream);\nint tamgcn_tmean(')
    text = text.replace('    const float* pq;  ', '    const float* extra;\n    const float* pq;  ')
    p = tmp_path / 'tamgcn.h'
    p.write_text(text)
    structs, funcs = A.parse_header(str(p))
    bad = S.classification_problems(structs=structs, funcs=funcs)
    assert any('tamgcn_new_stream_op: fresh has no slack class' in b for b in bad), bad
    assert any('tamgcn_ctrgc_desc: extra has no slack class' in b for b in bad), bad
    assert len(bad) == 2


def test_a_wrong_citation_or_a_stale_entry_is_reported():
    classes = dict(S.CLASSES)
    classes[('tamgcn_apply', 'src.x1')] = S.guarded(('elementwise.hip', 'no such guard in the file'))
    classes[('tamgcn_apply', 'gone')] = S.flat('x')
    classes[('tamgcn_vgen_agg_fwd', 'x3')] = S.stream('arg:nothing', 'x')
    classes[('tamgcn_tmean', 'src.x2')] = S.guarded()
    bad = S.classification_problems(classes)
    assert len(bad) == 4
    assert any("'no such guard in the file' is not in csrc/elementwise.hip" in b for b in bad)
    assert any('tamgcn_apply: gone is classified but is no const float*' in b for b in bad)
    assert any('stream without a row-length source' in b for b in bad)
    assert any('guarded without a citation' in b for b in bad)


def test_stream_owners_are_launching_entry_points():
    owners = S.stream_owners()
    _, funcs = A.parse_header()
    assert owners and all(any(d.kind == 'stream' for d in funcs[fn]) for fn in owners)
    assert owners['tamgcn_vgen_de_acc'] == ['dy.x1', 'dy.x2', 'x3']
    assert owners['tamgcn_conv'] == ['d.src.x1', 'd.src.x2']
    assert 'tamgcn_conv_nparts' not in owners and 'tamgcn_wgrad' not in owners


# =====================================================================================================================
# the checker's teeth
# =====================================================================================================================
class FakeLib:
    """Counts calls; refuses an argument list the real ctypes signature would refuse."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('tamgcn_'):
            raise AttributeError(name)
        argtypes = _lib.SIGNATURES[name][1]

        def fn(*args):
            assert len(args) == len(argtypes), name
            for a, ct in zip(args, argtypes):
                ct.from_param(a)
            self.calls.append(name)
            return 0
        return fn


N, CH, T = 2, 16, 6


def _desc(V, n=N):
    d = _lib.CtrgcDesc()
    d.N, d.Cin, d.Cout, d.S, d.R, d.T, d.V = n, CH, CH, 1, 8, T, V
    return d


def _agg_fwd(aud, x3, V, n=N):
    """tamgcn_vgen_agg_fwd on x3 (n, CH, T, V): x3 is a stream pointer whose row length is d.V."""
    E = torch.zeros(n, 1, CH, V, V)
    y = torch.zeros(n, CH, T, V)
    return aud.lib.tamgcn_vgen_agg_fwd(C.byref(_desc(V, n)), x3.data_ptr(), E.data_ptr(), y.data_ptr(), None, None)


def _tight(V, n=N):
    return torch.zeros(n * CH * T * V).view(n, CH, T, V)


def test_tight_tensor_at_ragged_v_raises_before_the_call():
    fake = FakeLib()
    with S.SlackAuditor(lib=fake) as aud:
        with pytest.raises(S.SlackError) as ei:
            _agg_fwd(aud, _tight(25), 25)
    e = ei.value
    assert (e.entry, e.role, e.shape, e.behind) == ('tamgcn_vgen_agg_fwd', 'x3', (N, CH, T, 25), 0)
    assert fake.calls == [] and aud.launches == []          # the call count is unchanged by the raise
    assert _lib._lib is None or not hasattr(_lib._lib, 'calls')


def test_tight_tensor_at_v20_passes():
    fake = FakeLib()
    with S.SlackAuditor(lib=fake) as aud:
        assert _agg_fwd(aud, _tight(20), 20) == 0
    assert fake.calls == ['tamgcn_vgen_agg_fwd']
    assert [(e['entry'], e['ragged'], e['roles']) for e in aud.launches] == [('tamgcn_vgen_agg_fwd', False, {})]
    assert aud.unresolved == []


def test_ops_empty_at_ragged_v_passes():
    fake = FakeLib()
    with S.SlackAuditor(lib=fake) as aud:
        x3 = ops.empty(N, CH, T, 25, like=torch.zeros(1))
        assert _agg_fwd(aud, x3, 25) == 0
    assert fake.calls == ['tamgcn_vgen_agg_fwd']
    assert aud.launches[0]['ragged'] and aud.launches[0]['roles'] == {'x3': 4 * ops.SLACK}
    assert aud.ragged_entries() == {'tamgcn_vgen_agg_fwd'}


def test_one_float_into_a_storage_that_ends_with_the_tensor_raises():
    fake = FakeLib()
    n = N * CH * T * 25
    x3 = torch.zeros(n + 1)[1:].view(N, CH, T, 25)
    with S.SlackAuditor(lib=fake) as aud:
        with pytest.raises(S.SlackError) as ei:
            _agg_fwd(aud, x3, 25)
    assert ei.value.behind == 0 and fake.calls == []


def test_clip_slices():
    fake = FakeLib()
    slack = ops.empty(3, CH, T, 25, like=torch.zeros(1))
    tight = torch.zeros(3 * CH * T * 25).view(3, CH, T, 25)
    per = CH * T * 25 * 4
    with S.SlackAuditor(lib=fake) as aud:
        assert _agg_fwd(aud, slack[0:2], 25, n=2) == 0      # the rest of the parent lies behind it
        assert _agg_fwd(aud, slack[1:3], 25, n=2) == 0      # the parent's last clips: the parent's own slack
        assert _agg_fwd(aud, tight[0:2], 25, n=2) == 0      # a tight parent, but its last clip lies behind the slice
        with pytest.raises(S.SlackError) as ei:
            _agg_fwd(aud, tight[1:3], 25, n=2)              # the parent's last clips and tight
    assert [e['roles']['x3'] for e in aud.launches] == [per + 16, 16, per]
    assert ei.value.shape == (2, CH, T, 25) and ei.value.behind == 0
    assert len(fake.calls) == 3


def test_an_offset_into_a_tensor_counts():
    """A raw address inside a seen tensor (part.data_ptr() + off): the tensor that contains it is the holder."""
    fake = FakeLib()
    tight = torch.zeros(3 * CH * T * 25).view(3, CH, T, 25)
    slack = ops.empty(3, CH, T, 25, like=tight)
    per = CH * T * 25 * 4
    E, y = torch.zeros(2, 1, CH, 25, 25), torch.zeros(2, CH, T, 25)
    with S.SlackAuditor(lib=fake) as aud:
        p = slack.data_ptr() + per
        assert aud.lib.tamgcn_vgen_agg_fwd(C.byref(_desc(25)), p, E.data_ptr(), y.data_ptr(), None, None) == 0
        p = tight.data_ptr() + per
        with pytest.raises(S.SlackError):
            aud.lib.tamgcn_vgen_agg_fwd(C.byref(_desc(25)), p, E.data_ptr(), y.data_ptr(), None, None)
    assert len(fake.calls) == 1 and aud.unresolved == []


def test_an_unresolved_pointer_is_reported():
    fake = FakeLib()
    x3 = _tight(25)
    addr = x3.untyped_storage().data_ptr()                  # the storage's address: no tensor was seen there
    E, y = torch.zeros(N, 1, CH, 25, 25), torch.zeros(N, CH, T, 25)
    with S.SlackAuditor(lib=fake) as aud:
        assert aud.lib.tamgcn_vgen_agg_fwd(C.byref(_desc(25)), addr, E.data_ptr(), y.data_ptr(), None, None) == 0
    assert aud.unresolved == [('tamgcn_vgen_agg_fwd', 'x3', addr)]
    assert aud.launches[0]['roles'] == {'x3': None}


def test_descriptor_sources_and_guarded_pointers():
    """tamgcn_conv: src.x1 / src.x2 are stream pointers with the row length of the descriptor; add1 is guarded and may be tight."""
    fake = FakeLib()
    x = ops.empty(N, CH, T, 25, like=torch.zeros(1))
    x2 = _tight(25)
    y, add1 = ops.empty(N, CH, T, 25, like=x), _tight(25)
    w = torch.zeros(CH, CH)
    d = _lib.ConvDesc()
    d.N, d.K, d.T_in, d.V, d.M, d.KT, d.dil, d.stride, d.up = N, CH, T, 25, CH, 1, 1, 1, 1
    d.T_out = d.T_y = T
    d.ostride = 1
    d.w, d.y, d.yctot, d.add1 = w.data_ptr(), y.data_ptr(), CH, add1.data_ptr()
    with S.SlackAuditor(lib=fake) as aud:
        d.src = _lib.Src(x.data_ptr(), None, None, CH, 0, 0)
        assert aud.lib.tamgcn_conv(C.byref(d), None) == 0
        d.src = _lib.Src(x.data_ptr(), x2.data_ptr(), None, CH, 0, 0)
        with pytest.raises(S.SlackError) as ei:
            aud.lib.tamgcn_conv(C.byref(d), None)
        d.V, d.T_in = 20, T                                  # the same pointers under a row length of 20: nothing to ask
        assert aud.lib.tamgcn_conv(C.byref(d), None) == 0
    assert (ei.value.entry, ei.value.role) == ('tamgcn_conv', 'd.src.x2')
    assert aud.launches[0]['roles'] == {'d.src.x1': 16} and fake.calls == ['tamgcn_conv', 'tamgcn_conv']


def test_source_parameters_take_v_from_the_descriptor_beside_them():
    fake = FakeLib()
    dy = _tight(25)
    E, dx3 = torch.zeros(N, 1, CH, 25, 25), torch.zeros(N, CH, T, 25)
    with S.SlackAuditor(lib=fake) as aud:
        src = _lib.Src(dy.data_ptr(), None, None, CH, 0, 0)  # a tensor is seen when its address is taken under the audit
        with pytest.raises(S.SlackError) as ei:
            aud.lib.tamgcn_ctrgc_tiled_agg_bwd(C.byref(_desc(25)), C.byref(src), E.data_ptr(), dx3.data_ptr(), None, None)
        assert aud.lib.tamgcn_ctrgc_bwd_dx3(C.byref(_desc(20)), C.byref(src), dx3.data_ptr(), None, None) == 0    # guarded
    assert (ei.value.entry, ei.value.role) == ('tamgcn_ctrgc_tiled_agg_bwd', 'dy.x1')
    assert fake.calls == ['tamgcn_ctrgc_bwd_dx3']


def test_the_audit_restores_what_it_patched():
    before = (_lib._lib, ops._ptr, ops.with_slack, torch.Tensor.data_ptr)
    with S.SlackAuditor(lib=FakeLib()):
        assert ops.with_slack is not before[2] and torch.Tensor.data_ptr is not before[3]
    assert (_lib._lib, ops._ptr, ops.with_slack, torch.Tensor.data_ptr) == before


def test_copies_are_recorded():
    with S.SlackAuditor(lib=FakeLib()) as aud:
        ops.with_slack(_tight(25))
        ops.with_slack(_tight(20))
        ops.with_slack(ops.empty(N, CH, T, 25, like=torch.zeros(1)))
    assert len(aud.copies) == 1 and aud.copies[0][0] == (N, CH, T, 25) and aud.copies[0][1].startswith('test_slack_audit_cpu.py:')


def test_hostile_size_helper():
    assert S.assert_hostile_size(2 * 16 * 6 * 25) == 4800
    with pytest.raises(AssertionError):
        S.assert_hostile_size(2 * 128 * 6 * 25)               # 300 * 512 bytes: the shape of the fault the audit was written after
    with pytest.raises(AssertionError):
        S.assert_hostile_size(125)                            # 500 bytes: 12 behind it in the block


# =====================================================================================================================
# ops.with_slack
# =====================================================================================================================
def _behind(t):
    return t.untyped_storage().nbytes() - (t.storage_offset() + t.numel()) * t.element_size()


def test_with_slack_copies_a_tight_ragged_tensor():
    t = torch.arange(N * CH * T * 25, dtype=torch.float32).view(N, CH, T, 25)
    out = ops.with_slack(t)
    assert out.data_ptr() != t.data_ptr() and out.shape == t.shape and out.is_contiguous()
    assert torch.equal(out, t) and _behind(out) == 16


def test_with_slack_keeps_a_tensor_that_has_the_bytes():
    for extra in (4, 5, 100):
        n = N * CH * T * 25
        t = torch.zeros(n + extra)[:n].view(N, CH, T, 25)
        assert ops.with_slack(t).data_ptr() == t.data_ptr()
    t = ops.empty(N, CH, T, 25, like=torch.zeros(1))
    assert ops.with_slack(t) is t
    n = N * CH * T * 25
    t = torch.zeros(n + 3)[:n].view(N, CH, T, 25)             # 12 bytes: not enough
    assert ops.with_slack(t).data_ptr() != t.data_ptr()


@pytest.mark.parametrize('V', [4, 16, 20, 32])
def test_with_slack_never_copies_whole_rows(V):
    t = torch.zeros(N * CH * T * V).view(N, CH, T, V)
    assert ops.with_slack(t) is t
    u = torch.zeros(N * CH * T * V + 1)[1:].view(N, CH, T, V)
    assert ops.with_slack(u) is u


def test_with_slack_copies_an_offset_view_that_ends_with_its_storage():
    n = N * CH * T * 25
    base = torch.arange(n + 7, dtype=torch.float32)
    t = base[7:].view(N, CH, T, 25)
    out = ops.with_slack(t)
    assert out.data_ptr() != t.data_ptr() and torch.equal(out, t) and _behind(out) == 16
    last = torch.arange(3 * CH * T * 25, dtype=torch.float32).view(3, CH, T, 25)[1:]
    out = ops.with_slack(last)
    assert out.data_ptr() != last.data_ptr() and torch.equal(out, last)
    first = torch.zeros(3 * CH * T * 25).view(3, CH, T, 25)[:2]
    assert ops.with_slack(first).data_ptr() == first.data_ptr()


def test_with_slack_passes_none_through():
    assert ops.with_slack(None) is None
