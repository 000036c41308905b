"""ctypes binding of libtamgcn.so, derived at import from include/tamgcn.h (the only declaration of the C ABI).

Every struct of the header becomes a ctypes.Structure named by class_name() (tamgcn_conv_desc -> ConvDesc), every entry point a
row of SIGNATURES, TAMGCN_VERSION and TAMGCN_TCONV_MAXB become ABI_VERSION and TCONV_MAXB.  The one thing the header cannot say is
kept here by hand: HOST_ARRAYS.  Importing this module reads the header only; load() opens the shared object.

The product path has no CPU fallback: if the shared object is missing or does
not export the ABI, importing the op layer raises (fail loudly).
"""
import ctypes as C
import os

from ._abi import HEADER, parse_abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libtamgcn.so')

SCALARS = {'unsigned char': C.c_ubyte, 'long long': C.c_longlong, 'unsigned': C.c_uint, 'int': C.c_int,
           'float': C.c_float, 'double': C.c_double, 'char': C.c_char}

# (entry point, parameter): a `const T*` that is an array on the host and is bound as POINTER(T); every other pointer that is
# not a descriptor is a device address and travels as an integer (c_void_p)
HOST_ARRAYS = (('tamgcn_tconv_supported', 'dil'), ('tamgcn_eval_accumulate', 'topk'), ('tamgcn_score_sweep', 'alphas'))


def class_name(struct):
    """tamgcn_f2s_tcn_bwd_desc -> F2sTcnBwdDesc."""
    return ''.join(p.capitalize() for p in struct[len('tamgcn_'):].split('_'))


def _ctype(d, classes, host_array=False):
    """The ctypes type of one header declaration."""
    if d.kind == 'desc':
        t = C.POINTER(classes[d.base])
    elif d.kind == 'struct':
        t = classes[d.base]
    elif d.ptr:
        t = C.POINTER(SCALARS[d.base]) if host_array else C.c_void_p
    elif d.base in SCALARS:
        t = SCALARS[d.base]
    else:
        raise ValueError(f'no ctypes type for {d!r}')
    return t * d.count if d.count else t


def derive(path=HEADER, host_arrays=HOST_ARRAYS):
    """(STRUCTS, SIGNATURES, defines) of the header at `path`: {struct name: ctypes.Structure subclass} in header order,
    {entry point: (restype, [argtypes])} and the header's integer #defines."""
    try:
        structs, funcs, rets, defines = parse_abi(path)
        classes = {h: type(class_name(h), (C.Structure,), {'__module__': __name__}) for h in structs}
        for h, fields in structs.items():
            classes[h]._fields_ = [(d.name, _ctype(d, classes)) for d in fields]
        for fn, param in host_arrays:
            if not any(d.name == param and d.kind == 'r' and d.base != 'void' for d in funcs.get(fn, ())):
                raise ValueError(f'HOST_ARRAYS: {fn} has no `const T*` parameter {param}')
        sigs = {}
        for fn, params in funcs.items():
            ret = rets[fn]
            if ret.ptr and (ret.base, ret.const) != ('char', True):
                raise ValueError(f'no ctypes return type for {ret!r} of {fn}')
            res = C.c_char_p if ret.ptr else _ctype(ret, classes)
            sigs[fn] = (res, [_ctype(d, classes, (fn, d.name) in host_arrays) for d in params])
    except ValueError as e:
        raise ValueError(f'{path}: {e}') from e
    return classes, sigs, defines


STRUCTS, SIGNATURES, _defines = derive()
for _h in STRUCTS:                            # Src, ConvDesc, ... as module attributes
    globals()[class_name(_h)] = STRUCTS[_h]
ABI_VERSION = _defines['TAMGCN_VERSION']      # what load() demands of tamgcn_version()
TCONV_MAXB = _defines['TAMGCN_TCONV_MAXB']


class TamgcnLibraryError(RuntimeError):
    pass


_lib = None


def load():
    """Load libtamgcn.so and bind every ABI symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64.so (SONAME libamdhip64.so.7) and finds it by file name
    # through an RPATH; libtamgcn.so asks for libamdhip64.so.7.  If we were loaded first the
    # process would end up with TWO HIP runtimes (ours from /opt/rocm, torch's bundled one) and
    # our launches fail with "no ROCm-capable device".  Loading torch first makes the dynamic
    # loader satisfy our DT_NEEDED with torch's already-loaded runtime (same SONAME).
    import torch  # noqa: F401
    path = os.environ.get('TAMGCN_LIB', LIB_PATH)      # instrumented side builds (tools/), same ABI
    if not os.path.exists(path):
        raise TamgcnLibraryError(
            f'{path} not found: the HIP extension is not built.  Run '
            '`python -m tam_gcn_amd.build` (needs hipcc, gfx950).  There is no CPU fallback.')
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise TamgcnLibraryError(f'{path} does not export {name}') from e
        fn.restype = res
        fn.argtypes = args
    got = lib.tamgcn_version()
    if got != ABI_VERSION:                             # a stale or side-built library with the same symbol set would be
        raise TamgcnLibraryError(                      # called with the wrong struct layouts and corrupt device memory
            f'{path} reports ABI version {got}, this binding is written for {ABI_VERSION}: rebuild with '
            '`python -m tam_gcn_amd.build --force`')
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().tamgcn_last_error()
        raise RuntimeError(f'{what} failed ({rc}): {msg.decode(errors="replace") if msg else "?"}')
