"""ctypes binding of libtamgcn_xmodal.so, the extension library of the cross-modal head, derived at import from
include/tamgcn_xmodal.h by the same code that derives the core binding (_lib.derive).  The core ABI (include/tamgcn.h, its
version, _lib.SIGNATURES) is untouched.  Importing this module reads the header only; load() opens the shared object.

There is no fallback: a missing or stale library raises."""
import ctypes as C
import os

from . import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
XM_HEADER = os.path.normpath(os.path.join(_HERE, '..', 'include', 'tamgcn_xmodal.h'))
XM_LIB_PATH = os.path.join(_HERE, 'libtamgcn_xmodal.so')

STRUCTS, SIGNATURES, _defines = _lib.derive(XM_HEADER, ())
XM_VERSION = _defines['TAMGCN_XM_VERSION']      # what load() demands of tamgcn_xm_version()

_xm = None


def load():
    """Load libtamgcn_xmodal.so and bind every symbol of its header; raises if anything is missing."""
    global _xm
    if _xm is not None:
        return _xm
    import torch  # noqa: F401  (first, as in _lib.load: one HIP runtime per process, torch's)
    path = os.environ.get('TAMGCN_XM_LIB', XM_LIB_PATH)
    if not os.path.exists(path):
        raise _lib.TamgcnLibraryError(
            f'{path} not found: the cross-modal extension library is not built.  Run '
            '`python -m tam_gcn_amd.build` (needs hipcc, gfx950).  There is no CPU fallback.')
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise _lib.TamgcnLibraryError(f'{path} does not export {name}') from e
        fn.restype = res
        fn.argtypes = args
    got = lib.tamgcn_xm_version()
    if got != XM_VERSION:
        raise _lib.TamgcnLibraryError(
            f'{path} reports version {got}, this binding is written for {XM_VERSION}: rebuild with '
            '`python -m tam_gcn_amd.build --force`')
    _xm = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().tamgcn_xm_last_error()
        raise RuntimeError(f'{what} failed ({rc}): {msg.decode(errors="replace") if msg else "?"}')
