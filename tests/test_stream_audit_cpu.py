"""The stream-schedule checker on synthetic traces, and the header parser / derived binding against include/tamgcn.h and
tam_gcn_amd/_lib.py.  No GPU: the checker is pure Python, the traces are written by hand in the vocabulary of
functional.Fork (fork = side.wait_stream(main), join = main.wait_stream(side), mark / wait = event record / wait)."""
import ctypes as C
import os
import types

import pytest

import stream_audit as A
from stream_audit import Checker, launch, record, wait, wait_stream, sync, event_sync, protect, drop

MAIN, S0, S1 = 0, 0x10, 0x20
X, Y, Z, W = (0x100000, 0x101000), (0x200000, 0x201000), (0x300000, 0x300800), (0x400000, 0x400100)


def rd(buf, role='in'):
    return (buf[0], buf[1], role)


def wr(buf, role='out'):
    return (buf[0], buf[1], role)


def hazards(trace, **kw):
    return Checker(waivers=[]).run(trace, **kw).hazards


# ---------------------------------------------------------------------------------------------------------------------
# fork / join
# ---------------------------------------------------------------------------------------------------------------------
def _fork_join(fork=True, join=True):
    t = [launch(MAIN, 'f.py:1', writes=[wr(X)], label='produce_x')]
    if fork:
        t.append(wait_stream(S0, MAIN, via=('on', 'f.py:2')))
    t.append(launch(S0, 'f.py:3', reads=[rd(X)], writes=[wr(Y)], label='side_work'))
    if join:
        t.append(wait_stream(MAIN, S0, via=('__exit__', 'f.py:4')))
    t.append(launch(MAIN, 'f.py:5', reads=[rd(Y)], writes=[wr(Z)], label='consume_y'))
    return t


def test_fork_and_join_order_everything():
    rep = Checker(waivers=[]).run(_fork_join())
    assert rep.hazards == [] and rep.launches == 3 and rep.side_launches == 1 and rep.accesses == 5 and rep.pairs == 2


def test_missing_join_is_a_read_after_write():
    hz = hazards(_fork_join(join=False))
    assert len(hz) == 1
    h = hz[0]
    assert h.kind == 'read-after-write' and (h.earlier.site, h.later.site) == ('f.py:3', 'f.py:5')
    assert h.earlier.role == 'out' and h.later.role == 'in' and h.earlier.stream == S0 and h.later.stream == MAIN
    assert 'f.py:3' in repr(h) and 'f.py:5' in repr(h) and 'consume_y' in repr(h)


def test_missing_fork_is_a_read_after_write_on_the_side():
    hz = hazards(_fork_join(fork=False))
    assert [(h.kind, h.earlier.site, h.later.site) for h in hz] == [('read-after-write', 'f.py:1', 'f.py:3')]


def test_deleting_the_join_edge_from_a_clean_trace_shows_the_consumer():
    clean = _fork_join()
    assert hazards(clean) == []
    cut = drop(clean, lambda e: e['op'] in A.WAIT_OPS and e.get('via') == ('__exit__', 'f.py:4'))
    assert len(cut) == len(clean) - 1
    assert [h.later.site for h in hazards(cut)] == ['f.py:5']


def _refork(refork=True):
    """main writes Y AFTER the fork; the side stream reads it: only a refork orders that."""
    t = [launch(MAIN, 'f.py:1', writes=[wr(X)]),
         wait_stream(S0, MAIN, via=('on', 'f.py:2')),
         launch(S0, 'f.py:3', reads=[rd(X)], writes=[wr(Z)]),
         launch(MAIN, 'f.py:4', reads=[rd(X)], writes=[wr(Y)], label='late_producer')]
    if refork:
        t.append(wait_stream(S0, MAIN, via=('refork', 'f.py:5')))
    t += [launch(S0, 'f.py:6', reads=[rd(Y)], writes=[wr(W)], label='late_side_reader'),
          wait_stream(MAIN, S0, via=('__exit__', 'f.py:7'))]
    return t


def test_refork_orders_what_main_wrote_after_the_fork():
    assert hazards(_refork()) == []
    hz = hazards(_refork(refork=False))
    assert [(h.kind, h.earlier.site, h.later.site, h.later.stream) for h in hz] == [('read-after-write', 'f.py:4', 'f.py:6', S0)]


def test_partial_join_through_mark_and_wait():
    """mark() after the side stream's first launch, wait() on main: the marked prefix is ordered, the suffix is not."""
    t = [launch(MAIN, 'f.py:1', writes=[wr(X)]),
         wait_stream(S0, MAIN),
         launch(S0, 'f.py:2', reads=[rd(X)], writes=[wr(Y, 'dh_slice')], label='data_gradient'),
         record(S0, 'ev'),
         launch(S0, 'f.py:3', reads=[rd(X)], writes=[wr(Z, 'dW_part')], label='weight_gradient'),
         wait(MAIN, 'ev'),
         launch(MAIN, 'f.py:4', reads=[rd(Y)], label='reads_marked_prefix')]
    assert hazards(t) == []
    t2 = t + [launch(MAIN, 'f.py:5', reads=[rd(Z)], label='reads_suffix')]
    hz = hazards(t2)
    assert [(h.earlier.role, h.later.site) for h in hz] == [('dW_part', 'f.py:5')]
    t3 = t + [wait_stream(MAIN, S0), launch(MAIN, 'f.py:5', reads=[rd(Z)])]
    assert hazards(t3) == []
    # without the wait even the prefix is unordered
    hz = hazards(drop(t, lambda e: e['op'] == 'wait'))
    assert [(h.earlier.role, h.later.site) for h in hz] == [('dh_slice', 'f.py:4')]


def test_a_wait_on_an_event_merges_the_clock_at_the_record_not_later():
    t = [record(S0, 'early'),
         launch(S0, 'f.py:1', writes=[wr(X)]),
         wait(MAIN, 'early'),
         launch(MAIN, 'f.py:2', reads=[rd(X)])]
    assert len(hazards(t)) == 1
    # the same event recorded again after the launch: the wait sees the later record
    t.insert(2, record(S0, 'early'))
    assert hazards(t) == []


def test_write_write_on_disjoint_and_on_overlapping_slices():
    base, L = 0x500000, 0x400
    fork = [launch(MAIN, 'f.py:1', writes=[wr(X)]), wait_stream(S0, MAIN), wait_stream(S1, MAIN)]
    branches = [launch(MAIN, 'f.py:2', writes=[(base, base + L, 'y')], label='branch0'),
                launch(S0, 'f.py:3', writes=[(base + L, base + 2 * L, 'y')], label='branch1'),
                launch(S1, 'f.py:4', writes=[(base + 2 * L, base + 3 * L, 'y')], label='branch2')]
    join = [wait_stream(MAIN, S0), wait_stream(MAIN, S1), launch(MAIN, 'f.py:5', reads=[(base, base + 3 * L, 'cat')])]
    rep = Checker(waivers=[]).run(fork + branches + join)
    assert rep.hazards == [] and rep.side_launches == 2
    branches[2] = launch(S1, 'f.py:4', writes=[(base + 2 * L - 4, base + 3 * L, 'y')], label='branch2')
    hz = hazards(fork + branches + join)
    assert [(h.kind, h.earlier.site, h.later.site, h.hi - h.lo) for h in hz] == [('write-after-write', 'f.py:3', 'f.py:4', 4)]
    # ranges that only touch do not overlap
    branches[2] = launch(S1, 'f.py:4', writes=[(base + 2 * L, base + 3 * L, 'y')])
    assert hazards(fork + branches + join) == []


def test_write_after_read_through_address_reuse():
    """A block freed on main while a side stream still reads it, handed out again and written on main."""
    t = [launch(MAIN, 'f.py:1', writes=[wr(X, 'old_tensor')]),
         wait_stream(S0, MAIN),
         launch(S0, 'f.py:2', reads=[rd(X, 'old_tensor')], writes=[wr(Y)], label='slow_side_reader'),
         launch(MAIN, 'f.py:3', writes=[(X[0], X[0] + 0x40, 'new_tensor')], label='writer_of_the_reused_block')]
    hz = hazards(t)
    assert [(h.kind, h.earlier.role, h.later.role) for h in hz] == [('write-after-read', 'old_tensor', 'new_tensor')]
    t.insert(3, wait_stream(MAIN, S0))
    assert hazards(t) == []


def test_record_stream_shields_the_recorded_stream_only():
    t = [launch(S0, 'f.py:1', writes=[wr(X)]),
         wait_stream(MAIN, S0),
         protect(MAIN, *X),
         launch(MAIN, 'f.py:2', reads=[rd(X)]),
         launch(S0, 'f.py:3', writes=[wr(X)], label='reuse_on_the_owner')]
    assert hazards(t) == []
    assert len(hazards(drop(t, lambda e: e['op'] == 'protect'))) == 1
    t[2] = protect(S1, *X)
    assert len(hazards(t)) == 1


def test_two_forks_in_sequence_reuse_a_side_stream():
    """The second fork's wait orders the side stream behind main's consumers of the first fork's results: what makes the
    side stream's allocator pool safe to reuse (functional._side_streams)."""
    def two(second_fork):
        t = [launch(MAIN, 'f.py:1', writes=[wr(X)]),
             wait_stream(S0, MAIN, via=('on', 'f.py:2')),
             launch(S0, 'f.py:3', reads=[rd(X)], writes=[wr(Y, 'side_owned')]),
             wait_stream(MAIN, S0, via=('__exit__', 'f.py:4')),
             launch(MAIN, 'f.py:5', reads=[rd(Y, 'side_owned')], writes=[wr(Z)], label='consumer_on_main')]
        if second_fork:
            t.append(wait_stream(S0, MAIN, via=('on', 'f.py:6')))
        t += [launch(S0, 'f.py:7', writes=[wr(Y, 'side_owned_again')], label='next_tenant'),
              wait_stream(MAIN, S0, via=('__exit__', 'f.py:8')),
              launch(MAIN, 'f.py:9', reads=[rd(Y)])]
        return t
    assert hazards(two(True)) == []
    hz = hazards(two(False))
    assert [(h.kind, h.earlier.site, h.later.site) for h in hz] == [('write-after-read', 'f.py:5', 'f.py:7')]


def test_synchronise_is_a_barrier():
    racy = [launch(S0, 'f.py:1', writes=[wr(X)]), launch(MAIN, 'f.py:2', reads=[rd(X)])]
    assert len(hazards(racy)) == 1
    assert hazards([racy[0], sync(None), racy[1]]) == []
    assert hazards([racy[0], sync(S0), racy[1]]) == []                       # the host waited for the producer's stream
    assert len(hazards([racy[0], sync(S1), racy[1]])) == 1                   # ... not for some other stream
    assert hazards([racy[0], record(S0, 'e'), event_sync('e'), racy[1]]) == []
    assert len(hazards([record(S0, 'e'), racy[0], event_sync('e'), racy[1]])) == 1
    # a stream first used after the barrier starts behind it too
    assert hazards([racy[0], sync(None), launch(S1, 'f.py:3', writes=[wr(X)])]) == []


def test_read_read_is_never_a_hazard():
    t = [launch(MAIN, 'f.py:1', reads=[rd(X)]), launch(S0, 'f.py:2', reads=[rd(X)]), launch(S1, 'f.py:3', reads=[rd(X)])]
    rep = Checker(waivers=[]).run(t)
    assert rep.hazards == [] and rep.pairs == 0


def test_same_stream_is_always_ordered_and_transitivity_holds():
    t = [launch(S0, 'f.py:1', writes=[wr(X)]), launch(S0, 'f.py:2', writes=[wr(X)]), launch(S0, 'f.py:3', reads=[rd(X)])]
    assert hazards(t) == []
    # S0 -> S1 -> MAIN: main never waited for S0 itself
    t = [launch(S0, 'f.py:1', writes=[wr(X)]), wait_stream(S1, S0), launch(S1, 'f.py:2', writes=[wr(Y)]),
         wait_stream(MAIN, S1), launch(MAIN, 'f.py:3', reads=[rd(X), rd(Y)])]
    assert hazards(t) == []


def test_forgetting_covered_accesses_does_not_hide_a_hazard():
    """The checker drops an access once a later ordered write covers it; a racing reader must still be reported."""
    t = [launch(MAIN, 'f.py:1', writes=[wr(X)]), launch(MAIN, 'f.py:2', writes=[wr(X)]),
         launch(S0, 'f.py:3', reads=[(X[0] + 8, X[0] + 16, 'in')])]
    hz = hazards(t)
    assert [(h.earlier.site, h.later.site) for h in hz] == [('f.py:2', 'f.py:3')]
    # many steps over the same buffers stay cheap and clean
    step = _fork_join()
    rep = Checker(waivers=[]).run(step * 200)
    assert rep.hazards == [] and rep.launches == 600


def test_ranges_larger_than_the_page_index():
    big = (0x10000000, 0x10000000 + (1 << 28))
    t = [launch(S0, 'f.py:1', writes=[(big[0], big[1], 'arena')]), launch(MAIN, 'f.py:2', reads=[(big[0] + (1 << 27), big[0] + (1 << 27) + 4, 'w')])]
    assert len(hazards(t)) == 1
    t = [launch(S0, 'f.py:1', writes=[(big[0] + 64, big[0] + 68, 'w')]), launch(MAIN, 'f.py:2', reads=[(big[0], big[1], 'arena')])]
    assert len(hazards(t)) == 1


def test_waivers_are_keyed_by_sites_and_roles_capped_and_must_be_hit():
    t = _fork_join(join=False)
    w = [(('f.py:3', 'out'), ('f.py:5', 'in'), 'synthetic: disjoint by construction')]
    rep = Checker(waivers=w).run(t)
    assert rep.hazards == [] and len(rep.waived) == 1 and rep.waivers_hit == {0}
    rep = Checker(waivers=[(('f.py:3', 'other_role'), ('f.py:5', 'in'), 'wrong role')]).run(t)
    assert len(rep.hazards) == 1 and rep.waivers_hit == set()
    with pytest.raises(ValueError, match='at most'):
        Checker(waivers=w * (A.MAX_WAIVERS + 1))
    assert len(A.WAIVERS) <= A.MAX_WAIVERS
    assert all(len(x) == 3 and isinstance(x[2], str) and x[2].strip() for x in A.WAIVERS)


def test_unknown_trace_entries_are_refused():
    with pytest.raises(ValueError, match='unknown op'):
        Checker(waivers=[]).run([dict(op='wait_all')])


# ---------------------------------------------------------------------------------------------------------------------
# the header and the binding derived from it
# ---------------------------------------------------------------------------------------------------------------------
def test_every_pointer_of_the_binding_is_classified_by_the_header():
    from tam_gcn_amd import _lib
    structs, funcs = A.parse_header()
    assert A.completeness_problems(_lib, structs, funcs) == []
    assert set(funcs) == set(_lib.SIGNATURES)
    assert set(structs) == set(_lib.STRUCTS)


def test_header_parser_reads_const_as_read_and_plain_as_write():
    structs, funcs = A.parse_header()
    kinds = {d.name: d.kind for d in structs['tamgcn_src']}
    assert kinds == dict(x1='r', x2='r', coef='r', ctot='scalar', coff='scalar', act='scalar')
    conv = {d.name: d for d in structs['tamgcn_conv_desc']}
    assert conv['src'].kind == 'struct' and conv['src'].base == 'tamgcn_src'
    assert conv['mask'].kind == 'desc' and conv['mask'].base == 'tamgcn_src' and conv['mask'].const
    assert (conv['y'].kind, conv['stats_part'].kind, conv['w'].kind, conv['add1'].kind, conv['bcast_scale'].kind) == \
        ('w', 'w', 'r', 'r', 'scalar')
    tc = {d.name: d for d in structs['tamgcn_tconv_desc']}
    assert (tc['w'].count, tc['w'].kind, tc['bias'].count, tc['dil'].count, tc['dil'].kind) == (6, 'r', 6, 6, 'scalar')
    fin = {d.name: d.kind for d in funcs['tamgcn_bn_fwd_finalize']}
    assert (fin['part'], fin['gamma'], fin['running_mean'], fin['num_batches_tracked'], fin['coef'], fin['save'], fin['stream']) == \
        ('r', 'r', 'w', 'w', 'w', 'w', 'stream')
    assert [d.kind for d in funcs['tamgcn_reduce_sum']] == ['w', 'scalar', 'scalar', 'scalar', 'scalar', 'scalar', 'w', 'stream']
    assert funcs['tamgcn_version'] == [] and [d.kind for d in funcs['tamgcn_conv_nparts']] == ['desc']
    assert [d.kind for d in funcs['tamgcn_drop_add_act_fwd']][7:11] == ['r', 'scalar', 'scalar', 'scalar']   # state, site, thr, scale
    assert {d.name: d.kind for d in funcs['tamgcn_ring_push']}['ring'] == 'w'


def test_an_unclassified_pointer_fails_the_completeness_check(tmp_path):
    from tam_gcn_amd import _lib
    structs, funcs = A.parse_header()

    def variant(**changes):
        ns = {k: v for k, v in vars(_lib).items()}
        ns.update(changes)
        m = types.ModuleType(_lib.__name__)
        m.__dict__.update(ns)
        return m

    class Src(C.Structure):                                   # a pointer field the header does not have
        _fields_ = list(_lib.Src._fields_) + [('x3', C.c_void_p)]
    Src.__module__ = _lib.__name__
    bad = A.completeness_problems(variant(Src=Src, STRUCTS=dict(_lib.STRUCTS, tamgcn_src=Src)), structs, funcs)
    assert any('Src.x3' in b for b in bad), bad

    class Extra(C.Structure):                                 # a structure of the binding without a header struct
        _fields_ = [('p', C.c_void_p)]
    Extra.__module__ = _lib.__name__
    assert any('Extra' in b for b in A.completeness_problems(variant(Extra=Extra), structs, funcs))
    sigs = dict(_lib.SIGNATURES)
    res, args = sigs['tamgcn_coef_diff']
    sigs['tamgcn_coef_diff'] = (res, list(args) + [C.c_void_p])                    # one more pointer than the header declares
    assert any('tamgcn_coef_diff' in b for b in A.completeness_problems(variant(SIGNATURES=sigs), structs, funcs))
    sigs = dict(_lib.SIGNATURES)
    sigs['tamgcn_new_entry'] = (C.c_int, [C.c_void_p, C.c_void_p])
    assert any('tamgcn_new_entry' in b for b in A.completeness_problems(variant(SIGNATURES=sigs), structs, funcs))
    sigs = dict(_lib.SIGNATURES)
    res, args = sigs['tamgcn_tmean']
    sigs['tamgcn_tmean'] = (res, [args[0], C.c_void_p] + list(args[2:]))           # a pointer where the header has an int
    assert any('tamgcn_tmean argument 1' in b for b in A.completeness_problems(variant(SIGNATURES=sigs), structs, funcs))
    # and the other way round: a header that loses a field or gains an entry point
    text = open(A.HEADER).read()
    p = tmp_path / 'tamgcn.h'
    p.write_text(text.replace('    const float* bcast;', '    ', 1))
    s2, f2 = A.parse_header(str(p))
    assert any('ConvDesc' in b for b in A.completeness_problems(_lib, s2, f2))
    p.write_text(text.replace('int tamgcn_conv(', 'int tamgcn_conv2(const float* a, void* stream);\nint tamgcn_conv(', 1))
    s2, f2 = A.parse_header(str(p))
    assert any('tamgcn_conv2' in b for b in A.completeness_problems(_lib, s2, f2))
    p.write_text(text.replace('int tamgcn_conv(', 'float** tamgcn_conv(', 1).replace('const float* w0;', 'const float** w0;', 1))
    with pytest.raises(ValueError):
        A.parse_header(str(p))


def test_channel_slices_of_a_descriptor():
    """The extent refinement: channels [coff, coff + cuse) of a (N, ctot, L) tensor are one range per sample."""
    got = A._planes(0x1000, 2, 8, 2, 3, 10)
    assert got == [(0x1000 + 4 * 20, 0x1000 + 4 * 50), (0x1000 + 4 * 100, 0x1000 + 4 * 130)]
    a = A._planes(0, 2, 96, 0, 32, 320)
    b = A._planes(0, 2, 96, 32, 32, 320)
    assert all(x[1] <= y[0] or y[1] <= x[0] for x in a for y in b)
    assert A._planes(0, 2, 96, 0, 96, 320) == [(0, 4 * 96 * 320), (4 * 96 * 320, 8 * 96 * 320)]


def test_range_registry():
    r = A._Ranges()
    r.add(100, 200)
    r.add(300, 400)
    assert r.find(150) == (100, 200) and r.find(200) is None and r.find(99) is None and r.find(399) == (300, 400)
    r.add(150, 320)                                           # a new allocation evicts what it overlaps
    assert r.find(120) is None and r.find(350) is None and r.find(319) == (150, 320)
    r.purge(0, 1000)
    assert r.starts == [] and r.end == {}


def test_dispatch_mode_sees_aten_work_inside_a_custom_backward():
    """The recorder's coverage canary, CPU side: with autograd's worker threads off, a TorchDispatchMode installed by the
    caller sees the ATen ops a custom autograd.Function issues in its backward."""
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode

    class Canary(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 2

        @staticmethod
        def backward(ctx, g):
            return torch.special.bessel_j0(g)                 # an op nothing else in this test issues

    seen = []

    class Mode(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(func._schema.name)
            return func(*args, **(kwargs or {}))

    x = torch.ones(4, requires_grad=True)
    with torch.autograd.set_multithreading_enabled(False), Mode():
        Canary.apply(x).sum().backward()
    assert 'aten::special_bessel_j0' in seen


def test_fork_call_sites_are_found_in_the_source():
    """The GPU scenarios assert coverage by call-site line; the list of sites comes from the source, not from a table."""
    import fork_sites
    sites = fork_sites.functional_sites()
    kinds = {}
    for fn, attr, _line in sites:
        kinds.setdefault(attr, set()).add(fn)
    assert kinds['join'] == {'_gcn_backward'} and kinds['mark'] == {'_tcn_backward'} and kinds['wait'] == {'_tcn_backward'}
    assert kinds['refork'] == {'_gcn_backward', 'tcn_forward', '_tcn_backward'}
    assert {'gcn_forward', '_gcn_backward', 'tcn_forward', '_tcn_forward_eval', '_tcn_backward'} == kinds['on']
    other = fork_sites.other_sites()
    assert {f for f, _ in other} == {'training.py', 'inference.py', 'streaming.py', os.path.join('feeder', 'feeder_nucla_gcn.py')}
