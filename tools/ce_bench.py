"""GPU-box tool: what the cross-entropy options cost (profiles/ce_options_bench.txt).

    python tools/ce_bench.py [--out FILE] [--rounds R] [--iters I] [--steps S]

Loss forward + backward at (N, K) = (256, 10), (256, 60), (1024, 400), as one graph replay and eagerly, six legs alternated in
one process for R rounds of I iterations each (median and min .. max of the rounds' means, wall clock around a device
synchronise):

    default    torch.ops.tamgcn.cross_entropy                         CrossEntropyLoss()
    opts-def   torch.ops.tamgcn.cross_entropy_opts, default options   the new kernels doing the default loss's work
    opts       the same with class weights, label_smoothing = 0.1 and a quarter of the rows ignored
    opts-ls    the new kernels with label_smoothing = 0.1 and the ignored rows, no class weights
    aten-ls    torch.nn.functional.cross_entropy on the device with opts-ls's options
    aten       the same with opts's options (where torch refuses to capture a leg, the tool says so and times it eagerly only)

Then one N-UCLA batch-256 CapturedStep with CrossEntropyLoss() against the same step with label_smoothing = 0.1, legs A, B, A, B,
..., S steps each; the difference of the legs' medians is compared with the spread of each leg's own rounds.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

SHAPES = ((256, 10), (256, 60), (1024, 400))
MARGS = dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
T_FRAMES, V = 64, 20


def _timed(fn, k):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k


def _legs(N, K, dev):
    """{name: fn(logits) -> loss} on seeded inputs"""
    import torch
    import torch.nn.functional as F
    from tam_gcn_amd.functional import CrossEntropyLoss
    import tam_gcn_amd.torch_ops  # noqa: F401
    g = torch.Generator().manual_seed(N + K)
    y = torch.randint(0, K, (N,), generator=g)
    yi = y.clone()
    yi[torch.rand(N, generator=g) < 0.25] = -100
    w = (torch.rand(K, generator=g) * 1.9 + 0.1).to(dev)
    y, yi = y.to(dev), yi.to(dev)
    default, opts = CrossEntropyLoss(), CrossEntropyLoss(weight=w, label_smoothing=0.1).to(dev)
    opts_ls = CrossEntropyLoss(label_smoothing=0.1)
    logits = (torch.randn(N, K, generator=g) * 3).to(dev)
    return logits, {'default': lambda l: default(l, y),
                    'opts-def': lambda l: torch.ops.tamgcn.cross_entropy_opts(l, y, None, -100, 0.0, 'mean')[0],
                    'opts': lambda l: opts(l, yi),
                    'opts-ls': lambda l: opts_ls(l, yi),
                    'aten-ls': lambda l: F.cross_entropy(l, yi, label_smoothing=0.1),
                    'aten': lambda l: F.cross_entropy(l, yi, weight=w, label_smoothing=0.1)}


def loss_legs(rounds, iters, say):
    import torch
    dev = torch.device('cuda:0')
    for N, K in SHAPES:
        logits, legs = _legs(N, K, dev)
        runs = {}
        for name, f in legs.items():
            l = logits.clone().requires_grad_(True)

            def fwd_bwd(f=f, l=l):
                l.grad = None
                f(l).backward()
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(3):
                    fwd_bwd()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(graph):
                    fwd_bwd()
                replay = graph.replay
            except Exception as e:                              # noqa: BLE001  -- reported, and the leg runs eagerly only
                say(f'N = {N}, K = {K}: leg {name!r} cannot be captured into a graph: {type(e).__name__}: {str(e).splitlines()[0]}')
                replay = None
                torch.cuda.synchronize()
            runs[name] = (replay, fwd_bwd)
        say(f'loss forward + backward, N = {N}, K = {K}: {rounds} rounds x {iters} iterations per leg, legs alternated; us per iteration')
        for mode, idx in (('graph replay', 0), ('eager', 1)):
            live = [name for name in runs if runs[name][idx] is not None]
            us = {name: [] for name in live}
            for name in live:
                _timed(runs[name][idx], 20)
            for _ in range(rounds):
                for name in live:
                    us[name].append(1e6 * _timed(runs[name][idx], iters))
            for name, v in us.items():
                say(f'  {mode:12s} {name:9s} median {statistics.median(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}')
            for ours, theirs in (('opts', 'aten'), ('opts-ls', 'aten-ls')):
                if theirs in us:
                    a, o = statistics.median(us[theirs]), statistics.median(us[ours])
                    say(f'  {mode:12s} {ours} against {theirs}: {o - a:+.2f} us ({"no slower" if o <= a else "SLOWER"})')
                else:
                    say(f'  {mode:12s} {ours} against {theirs}: no such leg ({theirs} is not capturable, see above)')


def captured_step(rounds, steps, say, batch=256):
    import torch
    from params import fill_state_, make_input, make_labels
    from tam_gcn_amd.distributed import ParamArena
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.models.ctrgcn import Model
    from tam_gcn_amd.optim import FusedSGD
    from tam_gcn_amd.training import CapturedStep
    dev = torch.device('cuda:0')
    x = make_input((batch, 3, T_FRAMES, V, 1), 4).to(dev)
    y = make_labels(batch, 10, 5).to(dev)
    runs = {}
    for name, kw in (('A default', {}), ('B label_smoothing=0.1', dict(label_smoothing=0.1))):
        m = Model(**MARGS)
        fill_state_(m.state_dict(), seed=0)
        m = m.to(dev).train()
        arena = ParamArena(m)
        bucket = arena.grad_bucket()
        opt = FusedSGD(arena, bucket, lr=0.01, momentum=0.9, nesterov=True, weight_decay=1e-4)
        runs[name] = CapturedStep(m, CrossEntropyLoss(**kw).to(dev), opt, arena, bucket, x, y)
    say(f'N-UCLA model, batch {batch}, {T_FRAMES} frames, {V} joints, captured step, FusedSGD; {rounds} rounds x {steps} timed steps per leg '
        f'after 3 warm-up steps, legs alternated; ms per step')
    ms = {name: [] for name in runs}
    for rnd in range(rounds):
        for name, st in runs.items():
            _timed(lambda: st.step(x, y), 3)
            ms[name].append(1e3 * _timed(lambda: st.step(x, y), steps))
            say(f'  round {rnd}: {name:24s} {ms[name][-1]:8.3f}')
    a, b = ms['A default'], ms['B label_smoothing=0.1']
    spread = max(max(a) - min(a), max(b) - min(b))
    diff = statistics.median(b) - statistics.median(a)
    say(f'  median A {statistics.median(a):.3f}, median B {statistics.median(b):.3f}: B - A = {1e3 * diff:+.1f} us; the larger spread of a leg\'s own '
        f'rounds is {1e3 * spread:.1f} us ({"within" if abs(diff) <= spread else "OUTSIDE"} the spread)')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=2000)
    ap.add_argument('--steps', type=int, default=20)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/ce_bench.py measures on the GPU; none found')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f'tools/ce_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}')
    loss_legs(a.rounds, a.iters, say)
    captured_step(a.rounds, a.steps, say)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
