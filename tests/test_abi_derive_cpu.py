"""The binding tam_gcn_amd/_lib.py derives from include/tamgcn.h: its struct layouts against the C++ compiler's, and the
derivation rules one by one on a small header of every form the real one uses.  No GPU, nothing loaded into Python."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

from tam_gcn_amd import _abi, _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_derived_layouts_match_the_compiler(tmp_path):
    """sizeof and every offsetof, as the library's own host compiler lays the header's structs out, against the ctypes classes:
    nothing else ties a derived class to the C++ struct the kernels' launchers read."""
    cc = shutil.which(build._hipcc())
    if cc is None:
        pytest.skip('no hipcc on this machine (a prebuilt libtamgcn.so on a GPU machine): nothing to lay the structs out with')
    structs, _ = _abi.parse_header()
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "tamgcn.h"', 'int main() {']
    for h, fields in structs.items():
        lines.append(f'    std::printf("{h} %zu\\n", sizeof({h}));')
        lines += [f'    std::printf("{h}.{d.name} %zu\\n", offsetof({h}, {d.name}));' for d in fields]
    lines += ['    return 0;', '}']
    src, exe = tmp_path / 'layout.cpp', tmp_path / 'layout'
    src.write_text('\n'.join(lines) + '\n')
    subprocess.run([cc, '-x', 'c++', '-std=c++17', '-I', os.path.dirname(_abi.HEADER), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    want = {}
    for h, cls in _lib.STRUCTS.items():
        want[h] = C.sizeof(cls)
        want.update({f'{h}.{name}': getattr(cls, name).offset for name, _ in cls._fields_})
    assert len(_lib.STRUCTS) == 20 and len(want) > 300
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    assert C.sizeof(_lib.GradGuard) == 40 and C.sizeof(_lib.CeDesc) == 64


RULES_HEADER = '''
#ifdef __cplusplus
extern "C" {
#endif
#define TAMGCN_VERSION 7
#define TAMGCN_N 3            /* an array count */
typedef struct tamgcn_in_ner {
    const float* x;
    int c;
} tamgcn_in_ner;
typedef struct tamgcn_every_form_desc {
    int i; unsigned u; unsigned char b; long long ll; float f; double d; char ch;
    const float* rd;
    float* wr;
    void* stream;
    tamgcn_in_ner by_value;
    const tamgcn_in_ner* by_pointer;
    int x[TAMGCN_N];
    const float* w[TAMGCN_N];
} tamgcn_every_form_desc;
int tamgcn_run(const tamgcn_every_form_desc* d, const int* sizes, const float* dev, float* out, int n, void* stream);
long long tamgcn_bytes(const tamgcn_every_form_desc* d);
const char* tamgcn_text(void);
#ifdef __cplusplus
}
#endif
'''


def test_derivation_rules_one_by_one(tmp_path):
    p = tmp_path / 'tamgcn.h'
    p.write_text(RULES_HEADER)
    structs, sigs, defines = _lib.derive(str(p), host_arrays=(('tamgcn_run', 'sizes'),))
    assert defines == dict(TAMGCN_VERSION=7, TAMGCN_N=3)
    assert [c.__name__ for c in structs.values()] == ['InNer', 'EveryFormDesc'] and list(structs) == ['tamgcn_in_ner', 'tamgcn_every_form_desc']
    Inner, Desc = structs.values()
    assert issubclass(Inner, C.Structure) and Inner._fields_ == [('x', C.c_void_p), ('c', C.c_int)]
    f = dict(Desc._fields_)
    assert list(f) == ['i', 'u', 'b', 'll', 'f', 'd', 'ch', 'rd', 'wr', 'stream', 'by_value', 'by_pointer', 'x', 'w']
    assert (f['i'], f['u'], f['b'], f['ll'], f['f'], f['d'], f['ch']) == \
        (C.c_int, C.c_uint, C.c_ubyte, C.c_longlong, C.c_float, C.c_double, C.c_char)
    assert f['rd'] is C.c_void_p and f['wr'] is C.c_void_p and f['stream'] is C.c_void_p      # device pointers travel as integers
    assert f['by_value'] is Inner
    assert issubclass(f['by_pointer'], C._Pointer) and f['by_pointer']._type_ is Inner
    assert issubclass(f['x'], C.Array) and (f['x']._type_, f['x']._length_) == (C.c_int, 3)
    assert issubclass(f['w'], C.Array) and (f['w']._type_, f['w']._length_) == (C.c_void_p, 3)
    assert list(sigs) == ['tamgcn_run', 'tamgcn_bytes', 'tamgcn_text']
    res, args = sigs['tamgcn_run']
    assert res is C.c_int and len(args) == 6
    assert args[0]._type_ is Desc and args[1]._type_ is C.c_int and issubclass(args[1], C._Pointer)      # descriptor, host array
    assert args[2:] == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    assert sigs['tamgcn_bytes'][0] is C.c_longlong and sigs['tamgcn_bytes'][1][0]._type_ is Desc
    assert sigs['tamgcn_text'] == (C.c_char_p, [])
    # without the hand-kept entry the same parameter is a device pointer
    assert _lib.derive(str(p), host_arrays=())[1]['tamgcn_run'][1][1] is C.c_void_p
    # a stale HOST_ARRAYS entry: no such entry point, no such parameter, not const, not typed
    for stale in (('tamgcn_gone', 'sizes'), ('tamgcn_run', 'gone'), ('tamgcn_run', 'out'), ('tamgcn_run', 'n')):
        with pytest.raises(ValueError, match='HOST_ARRAYS'):
            _lib.derive(str(p), host_arrays=(stale,))
    p.write_text(RULES_HEADER.replace('float* out', 'const void* out'))
    with pytest.raises(ValueError, match='HOST_ARRAYS'):
        _lib.derive(str(p), host_arrays=(('tamgcn_run', 'out'),))
    # the header is the one place: a new parameter changes the signature, a new struct gets a class named by the rule
    p.write_text(RULES_HEADER.replace('int n, void* stream', 'int n, double scale, void* stream')
                 .replace('typedef struct tamgcn_every', 'typedef struct tamgcn_f9_new_desc { int k; } tamgcn_f9_new_desc;\ntypedef struct tamgcn_every'))
    structs, sigs, _ = _lib.derive(str(p), host_arrays=())
    assert sigs['tamgcn_run'][1][4:] == [C.c_int, C.c_double, C.c_void_p]
    assert structs['tamgcn_f9_new_desc'].__name__ == 'F9NewDesc' and structs['tamgcn_f9_new_desc']._fields_ == [('k', C.c_int)]
    # what the parser does not understand is an error that names the file, never a guessed layout
    for bad in (RULES_HEADER.replace('float* wr;', 'float** wr;'), RULES_HEADER.replace('int c;', 'size_t c;'),
                RULES_HEADER.replace('} tamgcn_in_ner;', '} tamgcn_inner_t;'), RULES_HEADER.replace('long long tamgcn_bytes', 'void* tamgcn_bytes'),
                RULES_HEADER + 'static const int tamgcn_k = 3;\n'):
        p.write_text(bad)
        with pytest.raises(ValueError, match=re.escape(str(p))):
            _lib.derive(str(p), host_arrays=())
    # the real header through the same rules: the three host arrays, the three return types that are not int, the constants
    host = {(fn, i): ct for fn, (_, args) in _lib.SIGNATURES.items() for i, ct in enumerate(args)
            if issubclass(ct, C._Pointer) and not issubclass(ct._type_, C.Structure)}
    assert {k: ct._type_ for k, ct in host.items()} == \
        {('tamgcn_tconv_supported', 4): C.c_int, ('tamgcn_eval_accumulate', 7): C.c_int, ('tamgcn_score_sweep', 2): C.c_float}
    other = {fn: res for fn, (res, _) in _lib.SIGNATURES.items() if res is not C.c_int}
    assert other == dict(tamgcn_last_error=C.c_char_p, tamgcn_last_kernel=C.c_char_p, tamgcn_ce_opts_workspace_bytes=C.c_longlong)
    assert (_lib.ABI_VERSION, _lib.TCONV_MAXB, len(_lib.SIGNATURES)) == (401, 6, 137)
    assert all(getattr(_lib, c.__name__) is c for c in _lib.STRUCTS.values())
    # and importing the binding reads the header only: no torch, no shared object
    code = ('import sys, tam_gcn_amd._lib as L; assert "torch" not in sys.modules; assert L._lib is None; '
            'assert "libtamgcn" not in open("/proc/self/maps").read(); print(len(L.STRUCTS), len(L.SIGNATURES))')
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ['20', '137'], r.stderr
