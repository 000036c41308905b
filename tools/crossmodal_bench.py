"""GPU-box tool: the cross-modal attention head alone (profiles/xmodal_head_bench.txt).

    python tools/crossmodal_bench.py [--out FILE] [--rounds R] [--iters I] [--stats KERNEL_STATS_CSV]
    python tools/crossmodal_bench.py trace N STEPS

CrossModalHead (num_class 10, gcn_dim 256, rgb_dim 2048) on a (N, 2048, 7, 7) map at N = 16, 32, 64 against the torch composition of
the same modules (attention_transform(f), f_rgb * att, adaptive_avg_pool2d, classifier), train mode, eagerly and as one graph
replay.  Three kinds of call:

    fwd           forward under no_grad
    fwd+bwd       forward + backward, gradients for the parameters only (the frozen trunk: d f_rgb is not computed by the device
                  head; torch computes what autograd asks for)
    fwd+bwd+drgb  the same with d f_rgb (a trunk that trains)

Legs `hip` and `torch` alternated in one process for R rounds of I calls each: median and min .. max of the rounds' means, wall
clock around a device synchronise.

`trace N STEPS` runs STEPS eager fwd+bwd+drgb calls of the device head and nothing else: run it under
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/crossmodal_bench.py trace 16 200`, a run of its
own, and hand the kernel_stats.csv it writes to --stats: the report then lists every kernel of the head with its mean time and,
for the two streaming kernels, the bytes they must move over that time (pool_fwd reads the map, 4 N R P bytes; pool_bwd with
d f_rgb writes it)."""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, R, HW, K = 256, 2048, 7, 10
BATCHES = (16, 32, 64)


def _timed(fn, k):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k


class TorchHead:
    """the reference's composition over the modules of a CrossModalHead"""

    def __init__(self, head):
        self.at, self.cl = head.attention_transform, head.classifier

    def __call__(self, f, f_rgb):
        import torch
        att = self.at(f).unsqueeze(-1).unsqueeze(-1)
        return self.cl(torch.flatten(torch.nn.functional.adaptive_avg_pool2d(f_rgb * att, (1, 1)), 1))


def _problem(N, dev):
    import copy
    import torch
    from tam_gcn_amd.crossmodal import CrossModalHead
    torch.manual_seed(N)
    head = CrossModalHead(K, D, R).to(dev).train()
    twin = copy.deepcopy(head)
    g = torch.Generator().manual_seed(N + 1)
    f = torch.randn(N, D, generator=g).to(dev)
    f_rgb = torch.relu(torch.randn(N, R, HW, HW, generator=g)).to(dev)
    dl = (torch.randn(N, K, generator=g) / N).to(dev)
    return head, twin, f, f_rgb, dl


def _calls(net, params, f, f_rgb, dl):
    import torch
    frg = f_rgb.clone().requires_grad_(True)

    def fwd():
        with torch.no_grad():
            net(f, f_rgb)

    def fwd_bwd(x=f_rgb):
        for p in params:
            p.grad = None
        frg.grad = None
        net(f, x).backward(dl)
    return {'fwd': fwd, 'fwd+bwd': fwd_bwd, 'fwd+bwd+drgb': lambda: fwd_bwd(frg)}


def head_legs(rounds, iters, say):
    import torch
    dev = torch.device('cuda:0')
    for N in BATCHES:
        head, twin, f, f_rgb, dl = _problem(N, dev)
        legs = {'hip': _calls(head, list(head.parameters()), f, f_rgb, dl),
                'torch': _calls(TorchHead(twin), list(twin.parameters()), f, f_rgb, dl)}
        say(f'N = {N}, map ({N}, {R}, {HW}, {HW}) = {4 * N * R * HW * HW / 1e6:.1f} MB: {rounds} rounds x {iters} calls per leg, legs alternated; '
            f'us per call')
        for kind in ('fwd', 'fwd+bwd', 'fwd+bwd+drgb'):
            runs = {}
            for leg in legs:
                fn = legs[leg][kind]
                side = torch.cuda.Stream(dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    for _ in range(3):
                        fn()
                torch.cuda.current_stream(dev).wait_stream(side)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                try:
                    with torch.cuda.graph(graph):
                        fn()
                    replay = graph.replay
                except Exception as e:                          # noqa: BLE001  -- reported, and the leg runs eagerly only
                    say(f'  {kind}: leg {leg!r} cannot be captured: {type(e).__name__}: {str(e).splitlines()[0]}')
                    replay = None
                    torch.cuda.synchronize()
                runs[leg] = (fn, replay)
            for mode, idx in (('eager', 0), ('graph replay', 1)):
                live = [leg for leg in runs if runs[leg][idx] is not None]
                us = {leg: [] for leg in live}
                for leg in live:
                    _timed(runs[leg][idx], 20)
                for _ in range(rounds):
                    for leg in live:
                        us[leg].append(1e6 * _timed(runs[leg][idx], iters))
                med = {leg: statistics.median(v) for leg, v in us.items()}
                txt = '   '.join(f'{leg} median {med[leg]:8.2f} ({min(us[leg]):.2f} .. {max(us[leg]):.2f})' for leg in live)
                verdict = ''
                if len(live) == 2:
                    verdict = f'   hip / torch = {med["hip"] / med["torch"]:.2f} ({"faster" if med["hip"] < med["torch"] else "SLOWER"})'
                say(f'  {kind:13s} {mode:12s} {txt}{verdict}')


def trace(N, steps):
    import torch
    dev = torch.device('cuda:0')
    head, _, f, f_rgb, dl = _problem(N, dev)
    call = _calls(head, list(head.parameters()), f, f_rgb, dl)['fwd+bwd+drgb']
    for _ in range(steps):
        call()
    torch.cuda.synchronize()


def kernel_report(path, N, say):
    say(f'kernel times from a separate rocprofv3 --kernel-trace --stats run of `trace {N} STEPS` (eager fwd+bwd+drgb calls of the device head)')
    moved = {'xm_pool_fwd_kernel': 4 * N * R * HW * HW + 12 * N * R, 'xm_pool_bwd_kernel': 4 * N * R * HW * HW + 16 * N * R}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row['Name']
            if 'xm_' not in name and 'head_fc' not in name:
                continue
            us = float(row['AverageNs']) / 1e3
            short = name.split('(')[0].replace('void ', '').strip()
            extra = ''
            for k, b in moved.items():
                if k in name:
                    extra = f'   {b / 1e6:.2f} MB -> {b / us / 1e3:.0f} GB/s'
            say(f'  {short:60s} calls {int(row["Calls"]):6d}   mean {us:8.2f} us   min {float(row["MinNs"]) / 1e3:8.2f}{extra}')


def main():
    if len(sys.argv) > 1 and sys.argv[1] == 'trace':
        return trace(int(sys.argv[2]), int(sys.argv[3]))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--stats')
    ap.add_argument('--stats-batch', type=int, default=16)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/crossmodal_bench.py measures on the GPU; none found')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f'tools/crossmodal_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}')
    head_legs(a.rounds, a.iters, say)
    if a.stats:
        kernel_report(a.stats, a.stats_batch, say)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
