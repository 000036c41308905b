"""GPU-box tool: what training from user code costs (profiles/captured_step.txt, profiles/guarded_step.txt).

    python tools/captured_step_bench.py time [batch] [steps]   eager step (CapturedStep(eager=True)) vs CapturedStep replay at
                                                               N-UCLA x 64 frames, alternated twice; optimiser-only wall time
    python tools/captured_step_bench.py opt [n]                n x FusedSGD.step, n x FusedAdam.step, then n x SGDNesterov.step on
                                                               the N-UCLA arena -- run it under rocprofv3 --kernel-trace --stats
    python tools/captured_step_bench.py report <kernel_trace.csv> [n]   per-step kernel time of each optimiser from that trace
    python tools/captured_step_bench.py guard [batch] [steps]  captured step with FusedSGD plain (A) and with max_grad_norm +
                                                               skip_nonfinite (B), one process, legs A, B, A, B
    python tools/captured_step_bench.py optguard [n]           n x FusedSGD.step plain, then n x guarded, on the N-UCLA arena
                                                               -- run it under rocprofv3 --kernel-trace --stats
    python tools/captured_step_bench.py reportguard <kernel_trace.csv> [n]   per-step kernel time of both from that trace

In the `opt` trace, the fused optimisers' kernels are named optim_*; every kernel after the last of them belongs to
SGDNesterov.step (the tool launches nothing else after it).
"""
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

MARGS = dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
T_FRAMES, V = 64, 20


def _setup(opt_kind='sgd', seed=0, **guard):
    import torch
    from params import fill_state_
    from tam_gcn_amd.models.ctrgcn import Model
    from tam_gcn_amd.distributed import ParamArena, SGDNesterov
    from tam_gcn_amd.optim import FusedSGD, FusedAdam
    m = Model(**MARGS)
    fill_state_(m.state_dict(), seed=seed)
    m = m.to('cuda:0').train()
    arena = ParamArena(m)
    bucket = arena.grad_bucket()
    if opt_kind == 'sgd':
        opt = FusedSGD(arena, bucket, lr=0.01, momentum=0.9, nesterov=True, weight_decay=1e-4, **guard)
    elif opt_kind == 'adam':
        opt = FusedAdam(arena, bucket, lr=1e-3, weight_decay=1e-4)
    else:
        opt = SGDNesterov(arena.params, lr=0.01, momentum=0.9, weight_decay=1e-4, arena=arena, bucket=bucket)
    return m, arena, bucket, opt


def _timed(fn, k):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k


def time_steps(batch=256, steps=20):
    import torch
    from params import make_input, make_labels
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.training import CapturedStep
    x = make_input((batch, 3, T_FRAMES, V, 1), 4).to('cuda:0')
    y = make_labels(batch, 10, 5).to('cuda:0')
    runs = {}
    for name, eager in (('eager', True), ('captured', False)):
        m, arena, bucket, opt = _setup('sgd')
        runs[name] = CapturedStep(m, CrossEntropyLoss(), opt, arena, bucket, x, y, eager=eager)
    print(f'N-UCLA model, batch {batch}, {T_FRAMES} frames, {V} joints, FusedSGD; {steps} timed steps after 3 warm-up steps')
    for rnd in range(2):
        for name, st in runs.items():
            _timed(lambda: st.step(x, y), 3)
            ms = 1e3 * _timed(lambda: st.step(x, y), steps)
            print(f'  round {rnd}: {name:8s} {ms:8.3f} ms/step')
    for kind in ('sgd', 'sgdnesterov', 'adam'):
        _, arena, bucket, opt = _setup(kind)
        bucket.flat.normal_(0, 0.01)
        _timed(opt.step, 10)
        us = 1e6 * _timed(opt.step, 200)
        print(f'  optimiser alone, wall time per step (launch included, 200 steps): {type(opt).__name__:12s} {us:8.1f} us'
              f'  ({arena.total} floats)')


def opt_trace(n=100):
    import torch
    opts = [_setup(k) for k in ('sgd', 'adam', 'sgdnesterov')]
    for _, _, bucket, _ in opts:
        bucket.flat.normal_(0, 0.01)
    torch.cuda.synchronize()
    for _, _, _, opt in opts:
        for _ in range(n):
            opt.step()
        torch.cuda.synchronize()
    print(f'opt: {n} steps each of FusedSGD, FusedAdam, SGDNesterov ({opts[0][1].total} floats)')


GUARD = dict(max_grad_norm=4.0, skip_nonfinite=True)


def guard_steps(batch=256, steps=20):
    """The guarded step against the plain one, interleaved in one process.  The yardstick is the run's own noise: the
    guarded legs' mean is compared with the plain legs' mean, and the difference with the spread between the two plain legs."""
    from params import make_input, make_labels
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.training import CapturedStep
    x = make_input((batch, 3, T_FRAMES, V, 1), 4).to('cuda:0')
    y = make_labels(batch, 10, 5).to('cuda:0')
    runs = {}
    for name, guard in (('A plain', {}), ('B guarded', GUARD)):
        m, arena, bucket, opt = _setup('sgd', **guard)
        runs[name] = (CapturedStep(m, CrossEntropyLoss(), opt, arena, bucket, x, y), opt)
    print(f'N-UCLA model, batch {batch}, {T_FRAMES} frames, {V} joints, captured step, FusedSGD plain (A) vs '
          f'max_grad_norm={GUARD["max_grad_norm"]} + skip_nonfinite (B); {steps} timed steps after 3 warm-up steps per leg')
    ms = {name: [] for name in runs}
    for rnd in range(2):
        for name, (st, _) in runs.items():
            _timed(lambda: st.step(x, y), 3)
            ms[name].append(1e3 * _timed(lambda: st.step(x, y), steps))
            print(f'  leg {rnd}: {name:10s} {ms[name][-1]:8.3f} ms/step')
    a, b = ms['A plain'], ms['B guarded']
    spread, diff = abs(a[0] - a[1]), sum(b) / 2 - sum(a) / 2
    opt = runs['B guarded'][1]
    print(f'  spread between the two A legs {1e3 * spread:8.1f} us;  mean(B) - mean(A) {1e3 * diff:+8.1f} us  '
          f'({"within" if abs(diff) <= spread else "OUTSIDE"} the spread)')
    print(f'  last guarded step: grad_norm {float(opt.grad_norm):.4f}, clip_coef {float(opt.clip_coef):.4f}, '
          f'skipped_steps {opt.skipped_steps}')
    for name, guard in (('plain', {}), ('guarded', GUARD)):
        _, arena, bucket, opt = _setup('sgd', **guard)
        bucket.flat.normal_(0, 0.01)
        _timed(opt.step, 10)
        us = 1e6 * _timed(opt.step, 200)
        print(f'  optimiser alone, wall time per step (launch included, 200 steps): FusedSGD {name:8s} {us:8.1f} us')


def optguard_trace(n=100):
    import torch
    opts = [_setup('sgd'), _setup('sgd', **GUARD)]
    for _, _, bucket, _ in opts:
        bucket.flat.normal_(0, 0.01)
    torch.cuda.synchronize()
    for _, _, _, opt in opts:
        for _ in range(n):
            opt.step()
        torch.cuda.synchronize()
    print(f'optguard: {n} steps each of FusedSGD plain and guarded ({opts[0][1].total} floats)')


def report_guard(path, n=100):
    rows = list(csv.DictReader(open(path)))
    per = {}
    for r in rows:
        k = r['Kernel_Name']
        if 'optim_' in k or 'grad_sumsq' in k:
            short = k.replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0][:70]
            per.setdefault(short, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    groups = {'FusedSGD plain': ('optim_prologue_kernel', 'optim_update_kernel'),
              'FusedSGD guarded': ('grad_sumsq_kernel', 'optim_guard_prologue_kernel', 'optim_update_guarded_kernel')}
    for name, keys in groups.items():
        mine = {k: v for k, v in per.items() if k.split('<')[0] in keys}
        tot = sum(sum(v) for v in mine.values()) / n
        print(f'{name:17s} {tot:8.2f} us of kernel time per step ({sum(len(v) for v in mine.values())} launches over {n} steps)')
        for short, ds in sorted(mine.items(), key=lambda kv: -sum(kv[1])):
            print(f'    {len(ds):5d} x {sum(ds) / len(ds):8.2f} us  (min {min(ds):.2f}, max {max(ds):.2f})  {short}')


def report(path, n=100):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    dur = [(r['Kernel_Name'], (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3) for r in rows]
    last = max(i for i, (k, _) in enumerate(dur) if 'optim_' in k)
    adam = min(i for i, (k, _) in enumerate(dur) if 'optim_update_kernel<1' in k) - 1      # its prologue comes first
    groups = {'FusedSGD': [(k, d) for k, d in dur[:adam] if 'optim_' in k],
              'FusedAdam': [(k, d) for k, d in dur[adam:last + 1] if 'optim_' in k],
              'SGDNesterov': dur[last + 1:]}
    for name, ks in groups.items():
        per = {}
        for k, d in ks:
            short = k.replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0][:70]
            per.setdefault(short, []).append(d)
        tot = sum(d for _, d in ks) / n
        print(f'{name:12s} {tot:8.2f} us of kernel time per step ({len(ks)} launches over {n} steps)')
        for short, ds in sorted(per.items(), key=lambda kv: -sum(kv[1])):
            print(f'    {len(ds):5d} x {sum(ds) / len(ds):8.2f} us  {short}')


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'time'
    if mode == 'time':
        time_steps(*(int(a) for a in sys.argv[2:4]))
    elif mode == 'opt':
        opt_trace(*(int(a) for a in sys.argv[2:3]))
    elif mode == 'guard':
        guard_steps(*(int(a) for a in sys.argv[2:4]))
    elif mode == 'optguard':
        optguard_trace(*(int(a) for a in sys.argv[2:3]))
    elif mode == 'reportguard':
        report_guard(sys.argv[2], *(int(a) for a in sys.argv[3:4]))
    elif mode == 'report':
        report(sys.argv[2], *(int(a) for a in sys.argv[3:4]))
    else:
        raise SystemExit(__doc__)
