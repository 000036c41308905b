"""ctypes binding of libtamgcn_rgb.so, the extension library of the RGB feeder, derived at import from include/tamgcn_rgb.h by
the same code that derives the core binding (_lib.derive).  The core ABI (include/tamgcn.h, its version, _lib.SIGNATURES) and
the cross-modal extension's are untouched.  Importing this module reads the header only; load() opens the shared object.

There is no fallback: a missing or stale library raises."""
import ctypes as C
import os

from . import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
RGB_HEADER = os.path.normpath(os.path.join(_HERE, '..', 'include', 'tamgcn_rgb.h'))
RGB_LIB_PATH = os.path.join(_HERE, 'libtamgcn_rgb.so')

STRUCTS, SIGNATURES, _defines = _lib.derive(RGB_HEADER, ())
RGB_VERSION = _defines['TAMGCN_RGB_VERSION']    # what load() demands of tamgcn_rgb_version()
MAX_TAPS = _defines['TAMGCN_RGB_MAX_TAPS']

_rgb = None


def load():
    """Load libtamgcn_rgb.so and bind every symbol of its header; raises if anything is missing."""
    global _rgb
    if _rgb is not None:
        return _rgb
    import torch  # noqa: F401  (first, as in _lib.load: one HIP runtime per process, torch's)
    path = os.environ.get('TAMGCN_RGB_LIB', RGB_LIB_PATH)
    if not os.path.exists(path):
        raise _lib.TamgcnLibraryError(
            f'{path} not found: the RGB feeder\'s extension library is not built.  Run '
            '`python -m tam_gcn_amd.build` (needs hipcc, gfx950).  There is no CPU fallback.')
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise _lib.TamgcnLibraryError(f'{path} does not export {name}') from e
        fn.restype = res
        fn.argtypes = args
    got = lib.tamgcn_rgb_version()
    if got != RGB_VERSION:
        raise _lib.TamgcnLibraryError(
            f'{path} reports version {got}, this binding is written for {RGB_VERSION}: rebuild with '
            '`python -m tam_gcn_amd.build --force`')
    _rgb = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().tamgcn_rgb_last_error()
        raise RuntimeError(f'{what} failed ({rc}): {msg.decode(errors="replace") if msg else "?"}')
