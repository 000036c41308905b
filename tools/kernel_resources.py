"""Static resources of the kernels of one csrc/*.hip, compiled for gfx950 (no GPU needed):

    python tools/kernel_resources.py ctrgc.hip [--filter ctrgc_fwd] [--src PATH] [-DNAME ...] [--waits]

Per kernel, from hipcc's -Rpass-analysis=kernel-resource-usage remarks: VGPR, AGPR, VGPR spills, scratch bytes per lane and
occupancy (waves per SIMD); from the assembly (-S): static counts of v_mfma*, other v_*, ds_*, scratch_*, s_barrier and
`s_waitcnt vmcnt(0)`.  --waits lists every vmcnt(0) with the instruction in front of it.

Checks (exit status 1 when one fails):
  * kernels named by --spill-free REGEX must have scratch 0, spills 0, no scratch_* instruction;
  * ctrgc_fwd2_kernel's first wait of the next frame chunk leaves exactly the copy-out's stores in flight and assumes their
    number per wave.  The kernel prints it as the assembly comment `cg_fwd2_copyout_stores n=<N>`; the kernel text must hold
    exactly N 16-byte global stores (block placement scatters them, so they are counted over the whole kernel: the
    copy-out has the only ones) and one marker.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tam_gcn_amd', 'csrc')
ARCH = 'gfx950'


def hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc'):
        if c and os.path.exists(c):
            return c
    return 'hipcc'


def demangle(names):
    for tool in ('/opt/rocm/llvm/bin/llvm-cxxfilt', 'llvm-cxxfilt', 'c++filt'):
        try:
            r = subprocess.run([tool], input='\n'.join(names), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
        except OSError:
            continue
        if r.returncode == 0:
            return dict(zip(names, r.stdout.splitlines()))
    return {n: n for n in names}


def short(name):
    """ctrgc_fwd_kernel<Geo<20,16,2,8,32>,3,false>(...) -> without the argument list and the anonymous namespace"""
    name = name.replace('(anonymous namespace)::', '').replace('void ', '')
    depth = 0
    for i, ch in enumerate(name):
        depth += ch == '<'
        depth -= ch == '>'
        if ch == '(' and depth == 0:
            return name[:i]
    return name


def compile_one(src, defines):
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, 'k.s')
        cmd = [hipcc(), f'--offload-arch={ARCH}', '-O3', '-std=c++17', '--offload-device-only', '-S',
               '-Rpass-analysis=kernel-resource-usage', *defines, '-I', os.path.join(ROOT, 'include'), src, '-o', asm]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode:
            sys.exit('hipcc failed:\n' + r.stderr)
        with open(asm) as f:
            return r.stderr, f.read()


def parse_remarks(text):
    res, cur = {}, None
    keys = {'VGPRs': 'vgpr', 'AGPRs': 'agpr', 'ScratchSize [bytes/lane]': 'scratch', 'Occupancy [waves/SIMD]': 'occ',
            'VGPRs Spill': 'spill', 'SGPRs Spill': 'sspill', 'LDS Size [bytes/block]': 'lds', 'SGPRs': 'sgpr'}
    for line in text.splitlines():
        m = re.search(r'remark: .*Function Name: (\S+)', line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r'remark: [^ ]* +([A-Za-z][A-Za-z \[\]/]*): (\d+)', line)
        if m and cur is not None and m.group(1) in keys:
            cur[keys[m.group(1)]] = int(m.group(2))
    return res


def kernel_bodies(asm):
    """mangled name -> list of instruction lines (comments kept: the markers are comments)"""
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r'^(_Z\w+):', line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if line.startswith('.Lfunc_end'):
            cur = None
        elif cur is not None:
            s = line.strip()
            if s and not s.startswith('.'):
                cur.append(s)
    return out


def instr(line):
    return line.split(';')[0].strip()


def counts(body):
    c = dict(mfma=0, valu=0, ds=0, scratch=0, barrier=0, vm0=0, gload=0, gstore=0)
    for line in body:
        i = instr(line)
        if not i:
            continue
        op = i.split()[0]
        if op.startswith('v_mfma'):
            c['mfma'] += 1
        elif op.startswith('v_'):
            c['valu'] += 1
        elif op.startswith('ds_'):
            c['ds'] += 1
        elif op.startswith('scratch_'):
            c['scratch'] += 1
        elif op == 's_barrier':
            c['barrier'] += 1
        elif op.startswith('global_load') or op.startswith('buffer_load'):
            c['gload'] += 1
        elif op.startswith('global_store') or op.startswith('buffer_store'):
            c['gstore'] += 1
        if op == 's_waitcnt' and re.search(r'vmcnt\(0\)', i):
            c['vm0'] += 1
    return c


def waits(body):
    """every `s_waitcnt vmcnt(0)` with the nearest instruction in front of it and the next vector-memory / LDS consumer"""
    ins = [instr(x) for x in body if instr(x)]
    rows = []
    for k, i in enumerate(ins):
        if i.startswith('s_waitcnt') and 'vmcnt(0)' in i:
            prev = next((p for p in reversed(ins[:k]) if re.match(r'(global|scratch|buffer)_', p)), '-')
            rows.append((k, i, prev.split()[0], ins[k + 1] if k + 1 < len(ins) else '-'))
    return rows


def check_fwd2_stores(name, body):
    """returns a list of error strings"""
    errs = []
    marks = [int(m.group(1)) for line in body for m in [re.search(r'cg_fwd2_copyout_stores n=(\d+)', line)] if m]
    if not marks:
        return errs
    ins = [instr(x) for x in body if instr(x)]
    n = sum(1 for i in ins if i.startswith('global_store_dwordx4'))
    # a store the whole wave skips is a store vmcnt never counted: a branch on an empty exec mask straight in front of one
    skipped = sum(1 for k, i in enumerate(ins) if i.startswith('global_store_dwordx4') and any(p.startswith('s_cbranch_execz') for p in ins[max(0, k - 3):k]))
    print(f'  {name}: {n} global_store_dwordx4 in the kernel, the next chunk\'s first wait assumes {marks[0]} per wave '
          f'({len(marks)} marker{"s" if len(marks) > 1 else ""}; {skipped} stores straight behind an s_cbranch_execz)')
    if len(marks) != 1 or n != marks[0]:
        errs.append(f'{name}: {n} 16-byte store instructions, {len(marks)} marker(s) naming {marks}: the copy-out was merged, split or duplicated')
    return errs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('source')
    ap.add_argument('--src', help='path of the source file (default: csrc/<source>)')
    ap.add_argument('--filter', default='', help='regex on the demangled kernel name')
    ap.add_argument('--spill-free', default='', help='regex: these kernels must be free of scratch')
    ap.add_argument('--waits', action='store_true')
    ap.add_argument('-D', action='append', default=[], dest='defs')
    a = ap.parse_args()
    src = a.src or os.path.join(CSRC, a.source)
    remarks, asm = compile_one(src, ['-D' + d for d in a.defs] + ['-I', CSRC])
    res, bodies = parse_remarks(remarks), kernel_bodies(asm)
    names = demangle(list(res))
    errs = []
    hdr = f'{"kernel":64s} {"VGPR":>4s} {"AGPR":>4s} {"spill":>5s} {"scr B":>5s} {"occ":>3s} {"LDS":>6s} | {"mfma":>4s} {"valu":>5s} {"ds":>4s} {"scr":>3s} {"bar":>3s} {"vm0":>3s} {"gld":>3s} {"gst":>3s}'
    print(hdr)
    rows = []
    for mangled, r in res.items():
        nm = short(names[mangled])
        if a.filter and not re.search(a.filter, nm):
            continue
        body = bodies.get(mangled, [])
        c = counts(body)
        print(f'{nm[:64]:64s} {r.get("vgpr", -1):4d} {r.get("agpr", -1):4d} {r.get("spill", -1):5d} {r.get("scratch", -1):5d} {r.get("occ", -1):3d} '
              f'{r.get("lds", -1):6d} | {c["mfma"]:4d} {c["valu"]:5d} {c["ds"]:4d} {c["scratch"]:3d} {c["barrier"]:3d} {c["vm0"]:3d} {c["gload"]:3d} {c["gstore"]:3d}')
        rows.append((nm, body))
        if a.spill_free and re.search(a.spill_free, nm):
            if r.get('scratch', 0) or r.get('spill', 0) or c['scratch']:
                errs.append(f'{nm}: scratch {r.get("scratch")} B/lane, {r.get("spill")} spills, {c["scratch"]} scratch_* instructions')
    print('store-count check (ctrgc_fwd2_kernel):')
    for nm, body in rows:
        errs += check_fwd2_stores(nm, body)
    if a.waits:
        for nm, body in rows:
            print(f'vmcnt(0) waits of {nm}:')
            for k, i, prev, nxt in waits(body):
                print(f'  @{k:5d}  {i:40s} last vector-memory op in front: {prev:24s} next: {nxt}')
    for e in errs:
        print('FAIL ' + e)
    return 1 if errs else 0


if __name__ == '__main__':
    sys.exit(main())
