"""GPU-box tool: the fused CTRGC forward of two builds of libtamgcn.so side by side.

    python tools/ctrgc_fwd_ab.py OTHER_LIB [rounds]       e.g. the parent commit's library (tam_gcn_amd.build.build(out=...))

Part 1, bits: for every TAMGCN_CTRGC_FWD2 mode (a child process per library and mode: both are read once per process) the
forward runs at the six layer shapes of the training step (256 clips) and at T = 20 / T = 40 on the same seeded inputs; y, the
kept x3 and stats_part are compared through their SHA-256 (equal digests of the raw bytes = torch.equal).
Part 2, time: `rounds` interleaved rounds of HIP-event timings (us per launch, x3 kept, moments on) at the six layer shapes, the
protocol of profiles/r04_ctrgc_fwd_pipeline_ab.txt.  A shape counts as faster when the product's slower round beats the other
library's faster round."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [('l1', 3, 64, 64), ('l2', 64, 64, 64), ('l5', 64, 128, 64), ('l6', 128, 128, 32), ('l8', 128, 256, 32), ('l9', 256, 256, 16)]
RAGGED = [('c64-T20', 64, 64, 20), ('c64-T40', 64, 64, 40), ('c256-T20', 256, 256, 20), ('c256-T40', 256, 256, 40)]
N, V = 256, 20


def child(what):
    import torch
    sys.path.insert(0, ROOT)
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    dev = torch.device('cuda:0')
    out = {}
    for nm, Cin, Cout, T in (SHAPES + RAGGED if what == 'bits' else SHAPES):
        g = torch.Generator(device='cpu').manual_seed(1234 + Cin + T)
        r = lambda *s: torch.randn(*s, generator=g).to(dev)
        R = 8 if Cin == 3 else Cin // 8
        x = r(N, Cin, T, V); pq = r(6 * R, N, V)
        W3 = r(3 * Cout, Cin) * 0.1; B3 = r(3 * Cout); W4 = r(3, Cout, R) * 0.1; B4 = r(3, Cout)
        A = r(3, V, V) * 0.1; al = torch.tensor([0.5], device=dev)
        E = ops.ctrgc_build_E(S(x), pq, W3, B3, W4, B4, A, al, Cin, Cout, 3, R)
        fn = lambda: ops.ctrgc_fwd(S(x), pq, W3, B3, W4, B4, A, al, Cin, Cout, 3, R, stats=True, keep_x3=True, E=E)
        if what == 'bits':
            y, part, x3 = fn()
            torch.cuda.synchronize()
            out[nm] = [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16] for t in (y, x3, part)]
        else:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[nm] = e0.elapsed_time(e1) * 100.0                         # us per launch
    print('AB_RESULT ' + json.dumps(out), flush=True)


def run(lib, mode, what):
    env = dict(os.environ)
    env.pop('TAMGCN_CTRGC_FWD2', None)
    if lib:
        env['TAMGCN_LIB'] = lib
    if mode is not None:
        env['TAMGCN_CTRGC_FWD2'] = mode
    p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', what], env=env, capture_output=True, text=True, timeout=240)
    if p.returncode:
        sys.exit(f'child failed (lib {lib}, mode {mode}, {what}): rc {p.returncode}\n' + p.stdout[-1500:] + p.stderr[-1500:])
    return json.loads(next(l for l in p.stdout.splitlines() if l.startswith('AB_RESULT '))[10:])


def main():
    other, rounds = os.path.abspath(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 2
    print(f'bits: y / x3 / stats_part of the product build against {os.path.basename(other)}, per TAMGCN_CTRGC_FWD2 mode')
    bad = 0
    for mode in (None, '0', '2', '3'):
        a, b = run(None, mode, 'bits'), run(other, mode, 'bits')
        for nm in a:
            eq = [x == y for x, y in zip(a[nm], b[nm])]
            bad += not all(eq)
            print(f'  mode {mode or "default":7s} {nm:9s} ' + '  '.join(f'{k} {"equal" if e else "DIFFERENT"}' for k, e in zip(('y', 'x3', 'stats_part'), eq)), flush=True)
    print(f'bits: {"all bit-identical" if not bad else str(bad) + " cases differ"}')
    print(f'time: us per launch (x3 kept, moments), {rounds} interleaved rounds; default dispatch, then modes 2 and 3 (one form at every shape it serves)')
    for mode in (None, '2', '3'):
        res = {'other': [], 'product': []}
        for _ in range(rounds):
            res['other'].append(run(other, mode, 'time'))
            res['product'].append(run(None, mode, 'time'))
        for nm, *_ in SHAPES:
            o, p = [r[nm] for r in res['other']], [r[nm] for r in res['product']]
            verdict = 'faster' if max(p) < min(o) else ('slower' if min(p) > max(o) else 'within the spread')
            print(f'  mode {mode or "default":7s} {nm:3s} other ' + ' / '.join(f'{v:6.1f}' for v in o) + '   product ' + ' / '.join(f'{v:6.1f}' for v in p)
                  + f'   {verdict} ({(1 - sum(p) / sum(o)) * 100:+.1f} %)', flush=True)
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--child':
        child(sys.argv[2])
    else:
        sys.exit(main())
