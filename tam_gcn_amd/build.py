"""Build libtamgcn.so and its extension libraries libtamgcn_xmodal.so and libtamgcn_rgb.so (HIP, gfx950 only) in-tree with hipcc.

    python -m tam_gcn_amd.build [--force]

The shared objects are git-ignored but travel to the GPU box with the
snapshot; nothing is JIT-compiled at import time.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = ['lib.hip', 'conv.hip', 'wgrad.hip', 'reduce.hip', 'bn.hip', 'elementwise.hip', 'dropout.hip', 'ctrgc.hip', 'ctrgc_de.hip', 'ctrgc_tiled.hip', 'vgen.hip', 'stemhead.hip', 'celoss.hip', 'feeder.hip', 'clipfeeder.hip', 'streaming.hip', 'f2.hip', 'f2v.hip', 'f2g.hip', 'f2s.hip', 'f2s_bwd.hip', 'saliency.hip', 'guidance.hip', 'tconv.hip', 'optim.hip', 'evalmeter.hip']
LIB = os.path.join(HERE, 'libtamgcn.so')
# the cross-modal head (crossmodal.py): a library and a header (include/tamgcn_xmodal.h) of its own, the core ABI stays as it is
XM_SRC = ['xm_lib.hip', 'xm_hidden.hip', 'xm_gate.hip', 'xm_pool.hip']
XM_LIB = os.path.join(HERE, 'libtamgcn_xmodal.so')
# the RGB feeder (feeder/rgb_feeder.py): likewise a library and a header (include/tamgcn_rgb.h) of its own
RGB_SRC = ['rgb_lib.hip', 'rgb_resize.hip', 'rgb_batch.hip']
RGB_LIB = os.path.join(HERE, 'libtamgcn_rgb.so')
ARCH = 'gfx950'


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return 'hipcc'


def sources():
    return [os.path.join(HERE, 'csrc', s) for s in SRC]


def needs_build():
    if not os.path.exists(LIB):
        return True
    csrc = os.path.join(HERE, 'csrc')
    deps = sources() + [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith('.h')] + [os.path.join(HERE, '..', 'include', 'tamgcn.h')]
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in deps)


def xm_sources():
    return [os.path.join(HERE, 'csrc', 'xmodal', s) for s in XM_SRC]


def needs_build_xmodal():
    if not os.path.exists(XM_LIB):
        return True
    xm = os.path.join(HERE, 'csrc', 'xmodal')
    deps = xm_sources() + [os.path.join(xm, h) for h in os.listdir(xm) if h.endswith('.h')] + \
        [os.path.join(HERE, 'csrc', 'common.h'), os.path.join(HERE, '..', 'include', 'tamgcn.h'), os.path.join(HERE, '..', 'include', 'tamgcn_xmodal.h')]
    t = os.path.getmtime(XM_LIB)
    return any(os.path.getmtime(d) > t for d in deps)


def build_xmodal(force=False, verbose=True):
    """libtamgcn_xmodal.so from csrc/xmodal/*.hip."""
    if not force and not needs_build_xmodal():
        return XM_LIB
    return _compile_and_link(xm_sources(), XM_LIB, '.o', (), verbose)


def rgb_sources():
    return [os.path.join(HERE, 'csrc', 'rgb', s) for s in RGB_SRC]


def needs_build_rgb():
    if not os.path.exists(RGB_LIB):
        return True
    rgb = os.path.join(HERE, 'csrc', 'rgb')
    deps = rgb_sources() + [os.path.join(rgb, h) for h in os.listdir(rgb) if h.endswith('.h')] + \
        [os.path.join(HERE, 'csrc', 'common.h'), os.path.join(HERE, 'csrc', 'feeder_common.h'),
         os.path.join(HERE, '..', 'include', 'tamgcn.h'), os.path.join(HERE, '..', 'include', 'tamgcn_rgb.h')]
    t = os.path.getmtime(RGB_LIB)
    return any(os.path.getmtime(d) > t for d in deps)


def build_rgb(force=False, verbose=True):
    """libtamgcn_rgb.so from csrc/rgb/*.hip."""
    if not force and not needs_build_rgb():
        return RGB_LIB
    return _compile_and_link(rgb_sources(), RGB_LIB, '.o', (), verbose)


def build(force=False, verbose=True, out=None, defines=()):
    """The three libraries; returns LIB.  out/defines: instrumented side builds for tools/ (e.g. -DTAMGCN_TRACE) of the core
    library alone; the product is LIB."""
    if out is None:
        build_xmodal(force, verbose)
        build_rgb(force, verbose)
        if not force and not needs_build():
            return LIB
    return _compile_and_link(sources(), out or LIB, '.o' if out is None else '.side.o', defines, verbose)


def _compile_and_link(srcs, lib, osuffix, defines, verbose):
    objs = []
    procs = []
    for s in srcs:
        o = os.path.splitext(s)[0] + osuffix
        objs.append(o)
        cmd = [_hipcc(), f'--offload-arch={ARCH}', '-O3', '-std=c++17', '-fPIC', *[f'-D{d}' for d in defines], '-c', s, '-o', o]
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode:
            raise RuntimeError('hipcc failed: ' + ' '.join(cmd) + '\n' + out.decode(errors='replace'))
    cmd = [_hipcc(), f'--offload-arch={ARCH}', '-shared', '-fPIC', '-o', lib] + objs
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode:
        raise RuntimeError('link failed: ' + ' '.join(cmd) + '\n' + r.stdout.decode(errors='replace'))
    if verbose:
        print(f'[tam_gcn_amd.build] built {lib}')
    return lib


if __name__ == '__main__':
    build(force='--force' in sys.argv)
