"""Happens-before audit of the side-stream schedule ("The stream schedule and how it is checked").

Three parts, test-side only:

  header     parse_header() lives in the package (tam_gcn_amd/_abi.py) and is re-exported here: it reads every struct field
             and every parameter of every entry point of include/tamgcn.h, with `const T*` = read and `T*` = write.
             tam_gcn_amd/_lib.py derives its ctypes classes (_lib.STRUCTS) and signatures from the same parse;
             completeness_problems() checks a binding against a parse and lists every pointer that has no classification.
  Checker    pure Python over a trace (a list of dicts, see the constructors launch() .. protect() below): vector clocks
             per stream and one for the host; a hazard is a pair of accesses on different streams whose byte ranges
             overlap, at least one of them a write, where the earlier one in host order does not happen-before the later.
  Recorder   a context manager that produces such a trace from a real run: it wraps the loaded library, ops._ptr, the
             ordering primitives of torch.cuda and the methods of functional.Fork, and sees ATen work through a
             TorchDispatchMode.  It needs torch; the two parts above do not.  The wrapped library, ops._ptr, the address ->
             extent map and the walk over a call's descriptors are LibraryTap, shared with slack_audit.SlackAuditor.
"""
import bisect
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tam_gcn_amd._abi import BASE_TYPES, HEADER, Decl, _parse_decl, parse_header  # noqa: E402,F401  (re-exported)

PKG = os.path.join(ROOT, 'tam_gcn_amd') + os.sep


# =====================================================================================================================
# the binding against the header
# =====================================================================================================================
def _is_struct(t):
    return isinstance(t, type) and issubclass(t, C.Structure)


def _is_pointer_type(t):
    return isinstance(t, type) and issubclass(t, C._Pointer)


def _is_array_type(t):
    return isinstance(t, type) and issubclass(t, C.Array)


def completeness_problems(lib_module, structs=None, funcs=None):
    """Every way in which a pointer of the ctypes binding `lib_module` (tam_gcn_amd._lib) lacks a read / write
    classification from the header: an empty list means every pointer field of every structure and every pointer
    parameter of every declared entry point is classified."""
    if structs is None:
        structs, funcs = parse_header()
    bad = []
    struct_map = {h: c.__name__ for h, c in lib_module.STRUCTS.items()}     # header struct -> ctypes class of the binding
    by_class = {v: k for k, v in struct_map.items()}
    classes = {n: c for n, c in vars(lib_module).items() if _is_struct(c) and c.__module__ == lib_module.__name__}
    for n in classes:
        if n not in by_class:
            bad.append(f'_lib.{n}: no header struct mapped to it (_lib.STRUCTS)')
    for h, n in struct_map.items():
        if h not in structs:
            bad.append(f'_lib.STRUCTS: {h} is not a struct of tamgcn.h')
        if classes.get(n) is not lib_module.STRUCTS[h]:
            bad.append(f'_lib.STRUCTS: {h} is not the module attribute _lib.{n}')
    for h in structs:
        if h not in struct_map:
            bad.append(f'tamgcn.h struct {h}: no ctypes class mapped (_lib.STRUCTS)')

    def match(where, ct, d):
        """ctypes type `ct` against header declaration `d` (None: missing)."""
        if d is None:
            bad.append(f'{where}: not in tamgcn.h')
            return
        if _is_array_type(ct):
            if d.count != ct._length_:
                bad.append(f'{where}: array of {ct._length_}, header says {d.count}')
            ct = ct._type_
        elif d.count:
            bad.append(f'{where}: header has an array, the binding a single value')
        if ct is C.c_void_p:
            if d.kind not in ('r', 'w', 'stream'):
                bad.append(f'{where}: a device pointer in the binding, {d!r} in the header: unclassified')
        elif _is_pointer_type(ct) and _is_struct(ct._type_):
            want = by_class.get(ct._type_.__name__)
            if d.kind != 'desc' or d.base != want:
                bad.append(f'{where}: pointer to {ct._type_.__name__}, header has {d!r}')
            elif not d.const:
                bad.append(f'{where}: descriptor pointer is not const in the header')
        elif _is_pointer_type(ct):                          # a host array (dilations, top-k list): read-only by contract
            if d.kind != 'r':
                bad.append(f'{where}: host array in the binding, header has {d!r}')
        elif _is_struct(ct):
            if d.kind != 'struct' or d.base != by_class.get(ct.__name__):
                bad.append(f'{where}: struct {ct.__name__} by value, header has {d!r}')
        elif d.kind != 'scalar':
            bad.append(f'{where}: scalar in the binding, header has {d!r}')

    for h, n in struct_map.items():
        if h not in structs or n not in classes:
            continue
        hf = {d.name: d for d in structs[h]}
        cf = list(classes[n]._fields_)
        if [f[0] for f in cf] != [d.name for d in structs[h]]:
            bad.append(f'_lib.{n}: fields {[f[0] for f in cf]} differ from {h}: {[d.name for d in structs[h]]}')
        for name, ct in cf:
            match(f'_lib.{n}.{name}', ct, hf.get(name))
    sigs = lib_module.SIGNATURES
    for name in funcs:
        if name not in sigs:
            bad.append(f'{name}: declared in tamgcn.h, not in _lib.SIGNATURES')
    for name, (_, argtypes) in sigs.items():
        if name not in funcs:
            bad.append(f'{name}: in _lib.SIGNATURES, not declared in tamgcn.h')
            continue
        params = funcs[name]
        if len(params) != len(argtypes):
            bad.append(f'{name}: {len(argtypes)} arguments in the binding, {len(params)} in the header')
            continue
        for i, (ct, d) in enumerate(zip(argtypes, params)):
            match(f'{name} argument {i} ({d.name})', ct, d)
    return bad


# =====================================================================================================================
# traces
# =====================================================================================================================
def launch(stream, site, reads=(), writes=(), label='', **extra):
    """One unit of device work.  reads / writes: [(lo, hi, role)] byte ranges [lo, hi)."""
    acc = [(lo, hi, 'r', role) for lo, hi, role in reads] + [(lo, hi, 'w', role) for lo, hi, role in writes]
    return dict(op='launch', stream=stream, site=site, label=label, acc=acc, **extra)


def record(stream, event, **extra):
    return dict(op='record', stream=stream, event=event, **extra)


def wait(stream, event, **extra):
    return dict(op='wait', stream=stream, event=event, **extra)


def wait_stream(stream, other, **extra):
    """`stream` waits for everything enqueued on `other` so far (an event record on `other`, then a wait)."""
    return dict(op='wait_stream', stream=stream, other=other, **extra)


def sync(stream=None, **extra):
    """The host blocks until `stream` (None: every stream) has drained."""
    return dict(op='sync', stream=stream, **extra)


def event_sync(event, **extra):
    return dict(op='event_sync', event=event, **extra)


def protect(stream, lo, hi, **extra):
    """Tensor.record_stream: the allocator will not hand [lo, hi) out again before `stream`'s work so far is done."""
    return dict(op='protect', stream=stream, lo=lo, hi=hi, **extra)


WAIT_OPS = ('wait', 'wait_stream')


def drop(trace, pred):
    """A copy of the trace without the entries pred(entry) selects (trace-edit teeth: delete a wait edge)."""
    return [e for e in trace if not pred(e)]


class Access:
    __slots__ = ('stream', 'tick', 'lo', 'hi', 'write', 'site', 'role', 'label', 'chain', 'index', 'dead', 'protected')

    def __repr__(self):
        return f'{"write" if self.write else "read"} of {self.role} by {self.label or "?"} at {self.site} on stream {self.stream:#x}'


class Hazard:
    __slots__ = ('earlier', 'later', 'lo', 'hi')

    def __init__(self, earlier, later):
        self.earlier, self.later = earlier, later
        self.lo, self.hi = max(earlier.lo, later.lo), min(earlier.hi, later.hi)

    @property
    def kind(self):
        return {(True, True): 'write-after-write', (True, False): 'read-after-write', (False, True): 'write-after-read'}[
            (self.earlier.write, self.later.write)]

    def key(self):
        return (self.earlier.site, self.earlier.role, self.later.site, self.later.role)

    def __repr__(self):
        return f'{self.kind}: {self.later!r} is not ordered after the {self.earlier!r} ({self.hi - self.lo} bytes at {self.lo:#x})'


# (site, role) of the earlier access, (site, role) of the later one, the argument in one sentence.  Only for pairs that are
# disjoint by index arithmetic the descriptors do not expose; at most MAX_WAIVERS, each must be hit by a scenario.
WAIVERS = []
MAX_WAIVERS = 6


class Report:
    def __init__(self):
        self.hazards, self.waived = [], []
        self.launches = self.accesses = self.pairs = 0
        self.side_launches = 0
        self.waivers_hit = set()

    def __repr__(self):
        return f'<{self.launches} launches, {self.accesses} accesses, {self.pairs} cross-stream pairs, {len(self.hazards)} hazards, ' \
               f'{len(self.waived)} waived>'


class Checker:
    """Vector clocks: VC[s][t] = the last tick of stream t that stream s's next work is ordered after; H is the host's.
    Every entry is issued by the host, so the issuing stream first merges H.  An event record copies the stream's clock;
    a wait merges it; wait_stream is both; a synchronise merges the stream's clock (all clocks) into H."""
    PAGE = 12
    BIG = 1 << 14                                          # pages above which a range is kept in one list

    def __init__(self, waivers=None):
        self.waivers = list(WAIVERS if waivers is None else waivers)
        if len(self.waivers) > MAX_WAIVERS:
            raise ValueError(f'{len(self.waivers)} waivers: at most {MAX_WAIVERS} -- refine the extents instead')

    def run(self, trace, main=None):
        """main: the stream that counts as the main one for Report.side_launches (None: the stream of the first launch)."""
        rep = Report()
        VC, H, events = {}, {}, {}
        pages, big = {}, []
        seen = set()
        shielded = []                                      # (stream, lo, hi) under Tensor.record_stream, until the next full synchronise

        def clock(s):
            vc = VC.get(s)
            if vc is None:
                vc = VC[s] = {}
            for k, v in H.items():
                if vc.get(k, 0) < v:
                    vc[k] = v
            return vc

        def merge(dst, src):
            for k, v in src.items():
                if dst.get(k, 0) < v:
                    dst[k] = v

        def candidates(lo, hi):
            p0, p1 = lo >> self.PAGE, (hi - 1) >> self.PAGE
            out = {}
            for a in big:
                out[id(a)] = a
            if p1 - p0 >= self.BIG:
                for lst in pages.values():
                    for a in lst:
                        out[id(a)] = a
            else:
                for p in range(p0, p1 + 1):
                    for a in pages.get(p, ()):
                        out[id(a)] = a
            return [a for a in out.values() if not a.dead]

        def store(a):
            p0, p1 = a.lo >> self.PAGE, (a.hi - 1) >> self.PAGE
            if p1 - p0 >= self.BIG:
                big.append(a)
                return
            for p in range(p0, p1 + 1):
                lst = pages.get(p)
                if lst is None:
                    pages[p] = [a]
                else:
                    if len(lst) > 64:
                        lst[:] = [x for x in lst if not x.dead]
                    lst.append(a)

        for index, e in enumerate(trace):
            op = e['op']
            if op == 'launch':
                s = e['stream']
                vc = clock(s)
                vc[s] = vc.get(s, 0) + 1
                rep.launches += 1
                if main is None:
                    main = s
                if s != main:
                    rep.side_launches += 1
                fresh = []
                for lo, hi, mode, role in e['acc']:
                    if hi <= lo:
                        continue
                    b = Access()
                    b.stream, b.tick, b.lo, b.hi, b.write = s, vc[s], lo, hi, mode == 'w'
                    b.site, b.role, b.label, b.chain = e.get('site'), role, e.get('label', ''), e.get('chain', ())
                    b.index, b.dead = index, False
                    b.protected = any(st == s and l < hi and h > lo for st, l, h in shielded)
                    rep.accesses += 1
                    for a in candidates(lo, hi):
                        if a.hi <= lo or a.lo >= hi:
                            continue
                        ordered = a.stream == s or vc.get(a.stream, 0) >= a.tick
                        if a.stream != s and (a.write or b.write):
                            rep.pairs += 1
                            if not ordered and not a.protected:
                                hz = Hazard(a, b)
                                if hz.key() not in seen:
                                    seen.add(hz.key())
                                    w = self._waiver(hz)
                                    if w is None:
                                        rep.hazards.append(hz)
                                    else:
                                        rep.waivers_hit.add(w)
                                        rep.waived.append(hz)
                        # an access that the new one covers and is ordered after can be forgotten: whatever conflicts with
                        # it conflicts with the new one, and is ordered after it if it is ordered after the new one
                        if ordered and lo <= a.lo and a.hi <= hi and (b.write or (not a.write and a.stream == s)):
                            a.dead = True
                    fresh.append(b)
                for b in fresh:
                    store(b)
            elif op == 'record':
                events[e['event']] = dict(clock(e['stream']))
            elif op == 'wait':
                ev = events.get(e['event'])
                if ev is not None:
                    merge(clock(e['stream']), ev)
            elif op == 'wait_stream':
                snap = dict(clock(e['other']))
                merge(clock(e['stream']), snap)
            elif op == 'sync':
                if e.get('stream') is None:
                    for s in list(VC):
                        merge(H, clock(s))
                    pages.clear()                          # everything so far is ordered before everything to come
                    del big[:]
                    del shielded[:]
                else:
                    merge(H, clock(e['stream']))
            elif op == 'event_sync':
                ev = events.get(e['event'])
                if ev is not None:
                    merge(H, ev)
            elif op == 'protect':
                shielded.append((e['stream'], e['lo'], e['hi']))
                for a in candidates(e['lo'], e['hi']):
                    if a.stream == e['stream'] and a.lo < e['hi'] and a.hi > e['lo']:
                        a.protected = True
            elif op != 'note':
                raise ValueError(f'trace entry {index}: unknown op {op!r}')
        return rep

    def _waiver(self, hz):
        for i, (early, late, _why) in enumerate(self.waivers):
            if (hz.earlier.site, hz.earlier.role) == tuple(early) and (hz.later.site, hz.later.role) == tuple(late):
                return i
        return None


# =====================================================================================================================
# the recorder
# =====================================================================================================================
class _Ranges:
    """Disjoint byte ranges, looked up by a contained address."""

    def __init__(self):
        self.starts, self.end = [], {}

    def purge(self, lo, hi):
        i = bisect.bisect_left(self.starts, lo)
        if i > 0 and self.end[self.starts[i - 1]] > lo:
            i -= 1
        j = i
        while j < len(self.starts) and self.starts[j] < hi:
            del self.end[self.starts[j]]
            j += 1
        del self.starts[i:j]

    def add(self, lo, hi):
        if self.end.get(lo) == hi:
            return False
        self.purge(lo, hi)
        bisect.insort(self.starts, lo)
        self.end[lo] = hi
        return True

    def find(self, p):
        i = bisect.bisect_right(self.starts, p) - 1
        if i >= 0:
            lo = self.starts[i]
            if self.end[lo] > p:
                return lo, self.end[lo]
        return None


def _planes(base, k, ctot, coff, cuse, inner, esz=4):
    """Channels [coff, coff + cuse) of a [k][ctot][inner] array: k ranges."""
    return [(base + esz * (j * ctot + coff) * inner, base + esz * (j * ctot + coff + cuse) * inner) for j in range(k)]


FORK_METHODS = ('on', 'refork', 'mark', 'wait', 'join', '__exit__')
FACTORIES = ('aten::empty', 'aten::new_empty', 'aten::empty_like', 'aten::empty_strided', 'aten::new_empty_strided')


class LibraryTap:
    """What every audit of a real run shares (Recorder below, slack_audit.SlackAuditor): the loaded library behind a proxy whose
    tamgcn_* calls go through self._call(name, fn, args), ops._ptr reporting the tensors it is given, the map from a device
    address to the extent of the tensor, storage or allocator block that holds it, and the walk over an entry point's
    arguments and descriptors that lists every device pointer of the call with its role."""

    SNAP_EVERY = 200

    def __init__(self, lib=None):
        self.unresolved = []
        self._tensors, self._storages, self._blocks = _Ranges(), _Ranges(), _Ranges()
        self._snap_age = 0
        self._saved = []
        self._lib_given = lib                              # a stand-in for the loaded library (CPU tests)

    # ---- extents ----------------------------------------------------------------------------------------------------
    def _extent(self, p):
        """(hi, resolved) of the allocation piece that starts at device address p."""
        hit = self._tensors.find(p)                        # a registered tensor: its start, or an offset into it
        if hit is not None:
            return hit[1], True
        hit = self._storages.find(p)
        if hit is not None:
            return hit[1], True
        # tensors made before the recording began (workspaces and folded weights cached by earlier callers): the allocator's
        # own blocks, from a snapshot that is retaken on a miss and every SNAP_EVERY launches (blocks split and merge)
        hit = self._blocks.find(p) if self._snap_age < self.SNAP_EVERY else None
        if hit is None:
            self._snapshot()
            hit = self._blocks.find(p)
        if hit is not None:
            return hit[1], True
        return p + 4, False

    def _snapshot(self):
        """The allocator's blocks in use, once per miss: a snapshot walks every segment of the process."""
        import torch
        got = []
        for seg in torch.cuda.memory_snapshot():
            a = seg['address']
            for b in seg['blocks']:
                ba = b.get('address', a)
                if b.get('state') != 'inactive':
                    got.append((ba, ba + b['size']))
                a = ba + b['size']
        got.sort()
        self._blocks = _Ranges()
        self._blocks.starts = [lo for lo, _ in got]
        self._blocks.end = dict(got)
        self._snap_age = 0

    def _register_tensor(self, t):
        n = t.numel() * t.element_size()
        if n:
            self._tensors.add(t.data_ptr(), t.data_ptr() + n)

    def _register_storage(self, t, fresh):
        st = t.untyped_storage()
        lo, n = st.data_ptr(), st.nbytes()
        if n and lo:
            if self._storages.add(lo, lo + n) or fresh:
                self._tensors.purge(lo, lo + n)

    def _walk(self, hname, obj, prefix, raw, fname):
        def get(nm, obj=obj):
            return getattr(obj, nm)
        for d in self._structs[hname]:
            v = getattr(obj, d.name)
            role = f'{prefix}.{d.name}'
            if d.kind in ('r', 'w'):
                vals = list(v) if d.count else [v]
                for k, p in enumerate(vals):
                    if p:
                        raw.append((p, d.kind, role if not d.count else f'{role}[{k}]', hname, get, d.name))
            elif d.kind == 'struct':
                self._walk_src(d.base, v, role, raw, hname, get, d.name)
            elif d.kind == 'desc':
                if v:
                    self._walk_src(d.base, v.contents, role, raw, hname, get, d.name)

    def _walk_src(self, base, obj, role, raw, owner, owner_get, owner_field):
        if base != 'tamgcn_src':
            self._walk(base, obj, role, raw, None)
            return
        for d in self._structs[base]:
            p = getattr(obj, d.name)
            if d.kind in ('r', 'w') and p:
                # container 'src:<owner struct>': refined by the owner's geometry of this source
                raw.append((p, d.kind, f'{role}.{d.name}', 'src:' + owner, (owner_get, obj), (owner_field, d.name)))

    def _pointers(self, name, params, args):
        """(stream, [(address, mode, role, container, getter, field)], arg): every device pointer of one call; arg(name) is the
        value of a parameter."""
        raw = []
        argmap = {d.name: a for d, a in zip(params, args)}

        def arg(nm):
            v = argmap[nm]
            return v.value if hasattr(v, 'value') else v

        stream = 0
        for d, a, ct in zip(params, args, self._lib_mod.SIGNATURES[name][1]):
            if d.kind == 'stream':
                stream = (a.value if hasattr(a, 'value') else a) or 0
            elif d.kind in ('r', 'w'):
                if ct is not C.c_void_p:
                    continue                               # a host array
                p = (a.value if hasattr(a, 'value') else a) or 0
                if p:
                    raw.append((p, d.kind, d.name, name, arg, d.name))
            elif d.kind == 'desc' and a is not None:
                if isinstance(a, C.Array):
                    objs = list(a)
                    n = argmap.get('n')
                    if n is not None:
                        objs = objs[:arg('n')]
                elif hasattr(a, '_obj'):
                    objs = [a._obj]
                else:
                    objs = [a.contents]
                for k, obj in enumerate(objs):
                    prefix = d.name if len(objs) == 1 else f'{d.name}[{k}]'
                    self._walk(d.base, obj, prefix, raw, name)
        return stream, raw, arg

    def _call(self, name, fn, args):
        return fn(*args)

    def _install_library(self):
        """The proxy in place of the loaded library and the reporting ops._ptr; both are undone by _restore()."""
        from tam_gcn_amd import _lib, ops
        tap = self
        self._lib_mod = _lib
        self._structs, self._funcs = parse_header()
        bad = completeness_problems(_lib, self._structs, self._funcs)
        if bad:
            raise AssertionError('unclassified pointers: ' + '; '.join(bad[:5]))
        before = _lib._lib
        real = self._lib_given if self._lib_given is not None else _lib.load()
        self._real = real

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(real, name)
                if not name.startswith('tamgcn_'):
                    return fn

                def call(*args):
                    return tap._call(name, fn, args)
                return call

        self._saved.append((_lib, '_lib', real if self._lib_given is None else before))
        _lib._lib = Proxy()
        real_ptr = ops._ptr

        def _ptr(t):
            p = real_ptr(t)
            if t is not None:
                tap._register_tensor(t)
                tap._register_storage(t, False)
            return p
        self._patch(ops, '_ptr', _ptr)

    def _patch(self, owner, attr, new):
        self._saved.append((owner, attr, getattr(owner, attr)))
        setattr(owner, attr, new)

    def _restore(self):
        for owner, attr, old in reversed(self._saved):
            setattr(owner, attr, old)
        self._saved = []


class Recorder(LibraryTap):
    """with Recorder() as rec: ... ; rec.trace is the host-order trace, rec.unresolved the library pointers without an extent,
    rec.mismatch the descriptors whose channel-slice geometry did not fit the tensor's extent."""

    def __init__(self, sync_first=True):
        LibraryTap.__init__(self)
        self.trace, self.mismatch = [], []
        self.forks = []                                    # (method, call site) of every functional.Fork call that did something
        self._via, self._quiet = [], 0
        self._events, self._keep = {}, []
        self._sync_first = sync_first

    # ---- where ------------------------------------------------------------------------------------------------------
    def _where(self):
        """(innermost tam_gcn_amd frame as 'file:line', every tam_gcn_amd frame inside-out)."""
        f, chain = sys._getframe(1), []
        while f is not None:
            fn = f.f_code.co_filename
            if fn.startswith(PKG):
                chain.append(f'{fn[len(PKG):]}:{f.f_lineno}')
            f = f.f_back
        return (chain[0] if chain else None), tuple(chain)

    def _log(self, entry):
        site, chain = self._where()
        entry.setdefault('site', site)
        entry['chain'] = chain
        if self._via:
            entry['via'] = self._via[-1]
        self.trace.append(entry)

    # ---- library launches -------------------------------------------------------------------------------------------
    def _call(self, name, fn, args):
        params = self._funcs.get(name)
        if params is None or not any(d.kind == 'stream' for d in params):
            return fn(*args)
        stream, raw, _ = self._pointers(name, params, args)
        acc, ok = [], True
        for p, mode, role, container, get, field in raw:
            hi, res = self._extent(p)
            if not res:
                ok = False
                self.unresolved.append((name, role, p))
            for lo2, hi2 in self._refine(name, container, get, field, p, hi, role):
                acc.append((lo2, hi2, mode, role))
        rc = fn(*args)
        self._snap_age += 1
        if rc == 0:
            self._log(dict(op='launch', stream=stream, label=name, acc=acc, resolved=ok))
        return rc

    # ---- channel slices ---------------------------------------------------------------------------------------------
    # geometry of a tamgcn_src inside a descriptor: owner struct -> field -> (N, channels used, elements per channel)
    SRC_GEOM = {
        'tamgcn_conv_desc': {'src': lambda g: (g('N'), g('K'), g('T_in') * g('V')),
                             'mask': lambda g: (g('N'), g('M'), g('T_y') * g('V'))},
        'tamgcn_wgrad_desc': {'gy': lambda g: (g('N'), g('M'), g('T_out') * g('V')),
                              'src': lambda g: (g('N'), g('K'), g('T_in') * g('V'))},
        'tamgcn_conv_pair_desc': {'src': lambda g: (g('N'), g('K'), g('T') * g('V'))},
        'tamgcn_wgrad_pair_desc': {'gy0': lambda g: (g('N'), g('M0'), g('T') * g('V')),
                                   'gy1': lambda g: (g('N'), g('M1'), g('T') * g('V')),
                                   'src': lambda g: (g('N'), g('K'), g('T') * g('V'))},
    }
    # tamgcn_tconv_desc: the same fields mean different tensors per entry point: (channels of src, frames of src, channels of
    # mask, frames of mask, channels of y, frames of y); None: not a sliced tensor there
    TCONV = {
        'tamgcn_tconv_fwd': lambda g: dict(src=((g('nb') + (1 if g('pool') else 0)) * g('Cb'), g('T_in')),
                                           y=((g('nb') + (1 if g('pool') else 0)) * g('Cb'), g('T_out'))),
        'tamgcn_tconv_bwd': lambda g: dict(src=(g('nb') * g('Cb'), g('T_out')), mask=(g('nb') * g('Cb'), g('T_in')),
                                           y=(g('nb') * g('Cb'), g('T_in'))),
        'tamgcn_tconv_wgrad': lambda g: dict(src=(g('nb') * g('Cb'), g('T_out')), mask=(g('nb') * g('Cb'), g('T_in'))),
    }

    def _refine(self, fname, container, get, field, p, hi, role):
        """The byte ranges of one pointer: the whole extent [p, hi), or the channel slices its descriptor states."""
        try:
            out = self._slices(fname, container, get, field, p, hi)
        except (KeyError, AttributeError, ZeroDivisionError):
            out = None
        if not out:
            return [(p, hi)]
        if any(lo < p or h > hi + 16 or h <= lo for lo, h in out):
            self.mismatch.append((fname, role, p, hi, out[:2]))
            return [(p, hi)]
        return [(lo, min(h, hi)) for lo, h in out]

    def _slices(self, fname, container, get, field, p, hi):
        if container.startswith('src:'):
            owner = container[4:]
            owner_get, src = get
            ofield, sfield = field
            if sfield not in ('x1', 'x2'):
                return None
            if owner == 'tamgcn_tconv_desc':
                geo = self.TCONV[fname](owner_get).get(ofield)
                if geo is None:
                    return None
                N, cuse, L = owner_get('N'), geo[0], geo[1] * owner_get('V')
            else:
                N, cuse, L = self.SRC_GEOM[owner][ofield](owner_get)
            return _planes(p, N, src.ctot, src.coff, cuse, L)
        g = get
        if container == 'tamgcn_conv_desc':
            if field in ('y', 'add1', 'add2'):
                return _planes(p, g('N'), g('yctot'), g('ycoff'), g('M'), g('T_y') * g('V'))
            if field == 'aux':
                return _planes(p, g('N'), g('auxctot'), g('auxcoff'), g('M'), g('T_y') * g('V'))
            if field == 'stats_part':
                ctot = g('stats_ctot')
                return _planes(p, 2, ctot, g('stats_coff'), g('M'), (hi - p) // (8 * ctot))
        if container == 'tamgcn_conv_pair_desc':
            for i in '01':
                if field == 'y' + i:
                    return _planes(p, g('N'), g('yctot' + i), g('ycoff' + i), g('M' + i), g('T') * g('V'))
                if field == 'stats_part' + i:
                    ctot = g('stats_ctot' + i)
                    return _planes(p, 2, ctot, g('stats_coff' + i), g('M' + i), (hi - p) // (8 * ctot))
        if container == 'tamgcn_tconv_desc' and field == 'y':
            geo = self.TCONV[fname](g).get('y')
            if geo is not None:
                return _planes(p, g('N'), g('yctot'), g('ycoff'), geo[0], geo[1] * g('V'))
        if container == 'tamgcn_tconv_desc' and field == 'stats_part':
            geo = self.TCONV[fname](g).get('y')
            if geo is not None:
                ctot = g('stats_ctot')
                return _planes(p, 2, ctot, g('ycoff'), geo[0], (hi - p) // (8 * ctot))
        if container in ('tamgcn_bn_fwd_desc', 'tamgcn_bn_bwd_desc', 'tamgcn_bn_fwd_finalize', 'tamgcn_bn_bwd_finalize'):
            if field == 'part':
                return _planes(p, 2, g('part_ctot'), g('part_coff'), g('C'), g('nparts'))
            if field == 'coef':
                return _planes(p, 3, g('coef_ctot'), g('coef_coff'), g('C'), 1)
            if field == 'save':
                if 'bwd' in container:
                    return _planes(p, 2, g('save_ctot'), g('save_coff'), g('C'), 1)
                return _planes(p, 2, g('coef_ctot'), g('coef_coff'), g('C'), 1)
        if container in ('tamgcn_maxpool_fwd', 'tamgcn_maxpool_post_fwd'):
            if field in ('y', 'add'):
                return _planes(p, g('N'), g('yctot'), g('ycoff'), g('C'), g('T_out') * g('V'))
            if field == 'stats_part':
                return _planes(p, 2, g('yctot'), g('ycoff'), g('C'), (hi - p) // (8 * g('yctot')))
            if field == 'coef':
                return _planes(p, 3, g('yctot'), g('ycoff'), g('C'), 1)
        if container == 'tamgcn_maxpool_bwd':
            if field == 'd':
                return _planes(p, g('N'), g('dctot'), g('dcoff'), g('C'), g('T_in') * g('V'))
            if field == 'part':
                return _planes(p, 2, g('dctot'), g('dcoff'), g('C'), (hi - p) // (8 * g('dctot')))
        if container == 'tamgcn_apply' and field == 'y':
            return _planes(p, g('N'), g('yctot'), g('ycoff'), g('C'), g('T') * g('V'))
        return None

    # ---- ATen work --------------------------------------------------------------------------------------------------
    def _aten(self, func, args, kwargs, out):
        import torch
        schema = func._schema
        name = schema.name
        acc, seen_w = [], []

        def span(t):
            lo = t.data_ptr()
            n = 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
            return lo, lo + n * t.element_size()

        def tensors(v):
            if isinstance(v, torch.Tensor):
                yield v
            elif isinstance(v, (list, tuple)):
                for x in v:
                    if isinstance(x, torch.Tensor):
                        yield x

        cpu_in = cpu_out = False
        for i, sa in enumerate(schema.arguments):
            v = args[i] if i < len(args) else (kwargs or {}).get(sa.name)
            wr = sa.alias_info is not None and sa.alias_info.is_write
            for t in tensors(v):
                if not t.is_cuda:
                    cpu_in = True
                    continue
                if t.numel() == 0:
                    continue
                self._register_storage(t, False)
                lo, hi = span(t)
                acc.append((lo, hi, 'w' if wr else 'r', f'{name}:{sa.name}'))
                if wr:
                    seen_w.append(t)
        view = False
        outs = [out] if isinstance(out, torch.Tensor) else (list(out) if isinstance(out, (list, tuple)) else [])
        fresh = []
        for j, v in enumerate(outs):
            ai = schema.returns[j].alias_info if j < len(schema.returns) else None
            for t in tensors(v):
                if ai is not None and not ai.is_write:
                    view = True
                elif ai is None:
                    if not t.is_cuda:
                        cpu_out = True
                    elif t.numel():
                        fresh.append(t)
        if view:
            return
        for t in fresh:
            self._register_storage(t, True)
        if name == 'aten::record_stream':
            t, s = args[0], args[1]
            if t.is_cuda and t.numel():
                st = t.untyped_storage()
                if not hasattr(s, 'cuda_stream'):
                    s = torch.cuda.Stream(stream_id=s.stream_id, device_index=s.device_index, device_type=s.device_type)
                self._log(dict(op='protect', stream=s.cuda_stream, lo=st.data_ptr(), hi=st.data_ptr() + st.nbytes()))
            return
        if any(name == f or name.startswith(f + '.') for f in FACTORIES):
            return
        for t in fresh:
            lo, hi = span(t)
            acc.append((lo, hi, 'w', f'{name}:out'))
        if not acc:
            return
        stream = torch.cuda.current_stream().cuda_stream
        self._log(dict(op='launch', stream=stream, label=name, acc=acc, resolved=True, aten=True))
        if name == 'aten::_local_scalar_dense' or (cpu_out and not cpu_in) or \
                (name == 'aten::copy_' and not args[0].is_cuda and args[1].is_cuda):
            self._log(dict(op='sync', stream=stream))       # a blocking read on the host: the stream has drained

    # ---- installation -----------------------------------------------------------------------------------------------
    def __enter__(self):
        import torch
        from torch.utils._python_dispatch import TorchDispatchMode
        from tam_gcn_amd import functional
        rec = self
        self._install_library()

        def prim(owner, attr, make):
            orig = getattr(owner, attr)

            def wrapped(*a, **kw):
                if rec._quiet:
                    return orig(*a, **kw)
                rec._quiet += 1
                try:
                    res = orig(*a, **kw)
                finally:
                    rec._quiet -= 1
                e = make(res, *a, **kw)
                if e is not None:
                    rec._log(e)
                return res
            self._patch(owner, attr, wrapped)

        def evid(ev):
            k = id(ev)
            if k not in rec._events:
                rec._events[k] = len(rec._events) + 1
                rec._keep.append(ev)                       # alive: the id is not handed out again
            return rec._events[k]

        St, Ev = torch.cuda.Stream, torch.cuda.Event
        cur = lambda: torch.cuda.current_stream().cuda_stream                    # noqa: E731
        prim(St, 'wait_stream', lambda r, self_, other: wait_stream(self_.cuda_stream, other.cuda_stream))
        prim(St, 'wait_event', lambda r, self_, ev: wait(self_.cuda_stream, evid(ev)))
        prim(St, 'record_event', lambda r, self_, event=None: record(self_.cuda_stream, evid(r)))
        prim(St, 'synchronize', lambda r, self_: sync(self_.cuda_stream))
        prim(Ev, 'record', lambda r, self_, stream=None: record(cur() if stream is None else stream.cuda_stream, evid(self_)))
        prim(Ev, 'wait', lambda r, self_, stream=None: wait(cur() if stream is None else stream.cuda_stream, evid(self_)))
        prim(Ev, 'synchronize', lambda r, self_: event_sync(evid(self_)))
        prim(torch.cuda, 'synchronize', lambda r, device=None: sync(None))
        # a capture executes nothing: what was issued inside it is the graph's own schedule (audited as such) and cannot
        # race with what the host issues after the capture has ended
        prim(torch.cuda.CUDAGraph, 'capture_end', lambda r, self_: sync(None, note='capture_end'))

        def fork_method(attr):
            orig = getattr(functional.Fork, attr)

            def wrapped(self_, *a, **kw):
                f = sys._getframe(1)
                site = f'{f.f_code.co_filename[len(PKG):]}:{f.f_lineno}' if f.f_code.co_filename.startswith(PKG) else None
                before = len(rec.trace)
                rec._via.append((attr, site))
                try:
                    res = orig(self_, *a, **kw)
                finally:
                    rec._via.pop()
                rec.forks.append((attr, site, bool(self_.side), len(rec.trace) - before))
                return res
            self._patch(functional.Fork, attr, wrapped)
        for attr in FORK_METHODS:
            fork_method(attr)

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                out = func(*args, **(kwargs or {}))
                rec._aten(func, args, kwargs, out)
                return out

        self._mt = torch.autograd.set_multithreading_enabled(False)
        self._mt.__enter__()
        if self._sync_first and torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
            torch.cuda.synchronize()                       # (logged) everything before the recording is ordered before it
        self._mode = Mode()
        self._mode.__enter__()
        return self

    def __exit__(self, *exc):
        self._mode.__exit__(*exc)
        self._mt.__exit__(*exc)
        self._restore()
        self._keep = []
        return False

    # ---- queries ----------------------------------------------------------------------------------------------------
    def launches(self, label=None):
        return [e for e in self.trace if e['op'] == 'launch' and (label is None or e['label'] == label)]

    def fork_sites(self):
        """{(method, 'file:line')} of the functional.Fork calls that ran with side streams on."""
        return {(m, s) for m, s, on, _ in self.forks if on and s is not None}

    def wait_sites(self):
        """{'file:line'} of every wait_stream / wait_event issued directly from the package (not through Fork)."""
        return {e['site'] for e in self.trace if e['op'] in WAIT_OPS and 'via' not in e and e.get('site')}
