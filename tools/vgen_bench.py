"""GPU-box tool: what the run-time-V CTRGC kernels (csrc/vgen.hip) cost (profiles/vgen_bench.txt).

    python tools/vgen_bench.py kernels [rounds] [launches]   (a) each vgen kernel beside its templated counterpart at V = 25 and V = 32, NTU
                                                             layer shapes (C, T) = (64, 300), (128, 150), (256, 75), 16 clip-persons, S = 3,
                                                             R = C / 8, through the raw ABI on the same operands
    python tools/vgen_bench.py step [batch] [steps] [rounds] (b) one training step (forward + CE + backward + FusedSGD) of the COCO model
                                                             (17 joints, 64 frames), eager and captured
    python tools/vgen_bench.py                               both

Every figure is device-event time per launch (or host time around a synchronise per step) after a warm-up; A and B alternate in
one process, `rounds` legs each; printed: the median leg and the spread (min .. max) of the legs.
"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

LAYERS = ((64, 300), (128, 150), (256, 75))
N_CLIPS, S = 16, 3


def _events(fn, k):
    """us per call of fn over k back-to-back calls, by device events"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / k


def _ab(legs_a, legs_b):
    ma, mb = statistics.median(legs_a), statistics.median(legs_b)
    return (f'{ma:9.1f} ({min(legs_a):.1f} .. {max(legs_a):.1f})   {mb:9.1f} ({min(legs_b):.1f} .. {max(legs_b):.1f})   {mb / ma:5.2f}x')


def kernels(rounds=5, launches=10):
    import torch
    from tam_gcn_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device('cuda:0')
    like = torch.empty(0, device=dev)
    g = torch.Generator().manual_seed(1)

    def rnd(*shape, scale=1.0):
        t = ops.empty(*shape, like=like)
        t.copy_((torch.rand(shape, generator=g) * 2 - 1) * scale)
        return t
    print(f'(a) run-time-V kernels beside the templated ones: {N_CLIPS} clip-persons, S = {S}, R = C / 8; us per launch, device events, '
          f'{launches} launches per leg, {rounds} alternated legs each: median (min .. max)')
    print(f'{"V":>3} {"C":>4} {"T":>4}  {"kernel":8s} {"templated":>28s} {"run-time V":>30s}   ratio   symbols')
    for V in (25, 32):
        tiled = V == 32
        for Cout, T in LAYERS:
            R = Cout // 8
            N = N_CLIPS
            d = _lib.CtrgcDesc()
            d.N, d.Cin, d.Cout, d.S, d.R, d.T, d.V = N, 1, Cout, S, R, T, V
            pq, w4, b4 = rnd(S * 2 * R, N, V), rnd(S, Cout, R, scale=R ** -0.5), rnd(S, Cout, scale=0.1)
            A, alpha = rnd(S, V, V, scale=0.3), torch.tensor([0.7], device=dev)
            d.pq, d.w4, d.b4, d.A, d.alpha = (t.data_ptr() for t in (pq, w4, b4, A, alpha))
            x3, dyt = rnd(N, S * Cout, T, V), rnd(N, Cout, T, V)
            E, dE = ops.empty(N, S, Cout, V, V, like=like), ops.empty(N, S, Cout, V, V, like=like)
            y, dx3 = ops.empty(N, Cout, T, V, like=like), ops.empty(N, S * Cout, T, V, like=like)
            part, db3 = ops.empty(2, Cout, N, like=like), ops.empty(N, S * Cout, like=like)
            NUC = lib.tamgcn_ctrgc_tiled_chunks(V) if tiled else 1
            dA, dw4, db4 = ops.empty(N, S, V, V, like=like), ops.empty(N * NUC, S, Cout, R, like=like), ops.empty(N * NUC, S, Cout, like=like)
            dal, dpq = ops.empty(N * S * NUC, like=like), ops.empty(NUC, S * 2 * R, N, V, like=like)
            dy = ops.S(dyt).c()
            st = ops._stream()
            r, p = C.byref(d), (lambda t: t.data_ptr())
            if tiled:
                old_tail = lambda: lib.tamgcn_ctrgc_tiled_de_tail(r, p(dE), p(dA), p(dw4), p(db4), p(dal), p(dpq), st)      # noqa: E731
            else:
                old_tail = lambda: lib.tamgcn_ctrgc_bwd_de_tail(r, p(dE), p(dA), p(dw4), p(db4), p(dal), p(dpq), 1, st)     # noqa: E731
            pairs = [
                ('E', lambda: (lib.tamgcn_ctrgc_tiled_build_e if tiled else lib.tamgcn_ctrgc_build_e)(r, p(E), st),
                 lambda: lib.tamgcn_vgen_build_e(r, p(E), st)),
                ('agg_fwd', lambda: lib.tamgcn_ctrgc_tiled_agg_fwd(r, p(x3), p(E), p(y), p(part), st),
                 lambda: lib.tamgcn_vgen_agg_fwd(r, p(x3), p(E), p(y), p(part), st)),
                ('agg_bwd', lambda: lib.tamgcn_ctrgc_tiled_agg_bwd(r, C.byref(dy), p(E), p(dx3), p(db3), st),
                 lambda: lib.tamgcn_vgen_agg_bwd(r, C.byref(dy), p(E), p(dx3), p(db3), st)),
                ('de_acc', lambda: lib.tamgcn_ctrgc_tiled_de_acc(r, C.byref(dy), p(x3), p(dE), st),
                 lambda: lib.tamgcn_vgen_de_acc(r, C.byref(dy), p(x3), p(dE), st)),
                ('de_tail', old_tail, lambda: lib.tamgcn_vgen_de_tail(r, p(dE), p(dA), p(dw4), p(db4), p(dal), p(dpq), 1, st)),
            ]
            for name, old, new in pairs:
                syms = []
                for fn in (old, new):
                    rc = fn()
                    if rc:
                        raise RuntimeError(f'{name}: {lib.tamgcn_last_error().decode()}')
                    syms.append(lib.tamgcn_last_kernel().decode())
                    _events(fn, 3)
                la, lb = [], []
                for _ in range(rounds):
                    la.append(_events(old, launches))
                    lb.append(_events(new, launches))
                print(f'{V:3d} {Cout:4d} {T:4d}  {name:8s} {_ab(la, lb)}   {syms[0]} | {syms[1]}')
            del x3, dyt, E, dE, y, dx3
    torch.cuda.synchronize()


COCO = dict(num_class=10, num_point=17, num_person=1, graph='tam_gcn_amd.graph.coco.Graph', graph_args=dict(labeling_mode='spatial'))


def step(batch=256, steps=10, rounds=3):
    import torch
    from params import fill_state_, make_input, make_labels
    from tam_gcn_amd.distributed import ParamArena
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.models.ctrgcn import Model
    from tam_gcn_amd.optim import FusedSGD
    from tam_gcn_amd.training import CapturedStep
    T = 64
    x = make_input((batch, 3, T, 17, 1), 4).to('cuda:0')
    y = make_labels(batch, 10, 5).to('cuda:0')
    runs = {}
    for name, eager in (('eager', True), ('captured', False)):
        m = Model(**COCO)
        fill_state_(m.state_dict(), seed=0)
        m = m.to('cuda:0').train()
        arena = ParamArena(m)
        bucket = arena.grad_bucket()
        opt = FusedSGD(arena, bucket, lr=0.01, momentum=0.9, nesterov=True, weight_decay=1e-4)
        runs[name] = CapturedStep(m, CrossEntropyLoss(), opt, arena, bucket, x, y, eager=eager)

    def timed(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / k
    print(f'(b) COCO model (17 joints, route vgen), batch {batch}, {T} frames: forward + CE + backward + FusedSGD; ms per step, host clock around a '
          f'synchronise, {steps} steps per leg after 3 warm-up steps, {rounds} alternated legs each: median (min .. max)')
    legs = {name: [] for name in runs}
    for _ in range(rounds):
        for name, st in runs.items():
            timed(lambda: st.step(x, y), 3)
            legs[name].append(timed(lambda: st.step(x, y), steps))
    for name, l in legs.items():
        print(f'    {name:9s} {statistics.median(l):8.3f} ms/step ({min(l):.3f} .. {max(l):.3f})   {batch / statistics.median(l) * 1e3:9.0f} clips/s')


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'both'
    args = [int(a) for a in sys.argv[2:]]
    if mode in ('kernels', 'both'):
        kernels(*(args if mode == 'kernels' else ()))
    if mode in ('step', 'both'):
        step(*(args if mode == 'step' else ()))
    if mode not in ('kernels', 'step', 'both'):
        raise SystemExit(__doc__)
