"""GPU-box tool: what the device dropout of tam_gcn_amd/dropout.py costs or saves (profiles/stgcn_dropout_bench.txt).

    python tools/dropout_bench.py time [batch] [steps] [rounds] [out]
        ST-GCN N-UCLA model, dropout = 0.5 in every block and the head, 52 and 64 frames.  Four legs in ONE process: a captured
        step and an eager step, each with the torch tail (dropout.enable not called: the parent commit's path) and with the device
        path.  3 warm-up steps per leg, then `rounds` (>= 5) alternated rounds of `steps` timed steps; median and min .. max of
        the rounds.  The table is printed and written to `out` (default profiles/stgcn_dropout_bench.txt).
    python tools/dropout_bench.py trace [batch] [steps]
        `steps` eager device-path steps at 52 frames, then at 64 -- run it under rocprofv3 --kernel-trace --stats
    python tools/dropout_bench.py report <kernel_trace.csv> [batch] [steps] [out]
        time of drop_add_act_fwd_kernel / drop_add_act_bwd_kernel per step from that trace, and the bytes the two kernels need
        (computed from the shapes: every operand read or written once) over that time; appended to `out` when given

The reference's Model hands its `dropout` argument to the head only (models/stgcn.py:121, :141-150); the published network
drops in every block, so the tool sets the blocks' probability itself.
"""
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

MARGS = dict(in_channels=3, num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
FRAMES, V, P = (52, 64), 20, 0.5
# (channels, temporal stride, residual) of the ten blocks
PLAN = [(64, 1, None)] + [(64, 1, 'identity')] * 3 + [(128, 2, 'conv')] + [(128, 1, 'identity')] * 2 + [(256, 2, 'conv')] + \
    [(256, 1, 'identity')] * 2
DEFAULT_OUT = os.path.join(ROOT, 'profiles', 'stgcn_dropout_bench.txt')


def _setup(device_path, seed=0):
    from params import fill_state_
    from tam_gcn_amd import dropout
    from tam_gcn_amd.distributed import ParamArena
    from tam_gcn_amd.models.stgcn import Model
    from tam_gcn_amd.optim import FusedSGD
    m = Model(**MARGS, dropout=P)
    fill_state_(m.state_dict(), seed=seed)
    for blk in m.st_gcn_networks:
        blk._dropout = blk.tcn[4].p = P
    m = m.to('cuda:0').train()
    if device_path:
        dropout.enable(m, seed=1234)
    arena = ParamArena(m)
    bucket = arena.grad_bucket()
    return m, arena, bucket, FusedSGD(arena, bucket, lr=0.01, momentum=0.9, nesterov=True, weight_decay=1e-4)


def _batch(batch, frames):
    from params import make_input, make_labels
    return make_input((batch, 3, frames, V, 1), 4).to('cuda:0'), make_labels(batch, 10, 5).to('cuda:0')


def _timed(fn, k):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k


def time_steps(batch=256, steps=10, rounds=5, out=DEFAULT_OUT):
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.training import CapturedStep
    rounds = max(5, rounds)
    lines = [f'ST-GCN N-UCLA model, batch {batch}, {V} joints, dropout {P} in every block and the head, FusedSGD; per leg 3 warm-up '
             f'steps, then {rounds} alternated rounds of {steps} timed steps (ms/step: median, min .. max of the rounds)']
    for frames in FRAMES:
        x, y = _batch(batch, frames)
        legs = {}
        for kind, eager in (('captured', False), ('eager', True)):
            for which, device_path in (('torch tail', False), ('device', True)):
                m, arena, bucket, opt = _setup(device_path)
                legs[(kind, which)] = CapturedStep(m, CrossEntropyLoss(), opt, arena, bucket, x, y, eager=eager)
        ms = {name: [] for name in legs}
        for name, st in legs.items():
            _timed(lambda: st.step(x, y), 3)
        for _ in range(rounds):
            for name, st in legs.items():
                ms[name].append(1e3 * _timed(lambda: st.step(x, y), steps))
        lines.append(f'{frames} frames')
        med = {name: statistics.median(v) for name, v in ms.items()}
        for (kind, which), v in ms.items():
            lines.append(f'  {kind + ", " + which:22s} {med[(kind, which)]:8.3f}   {min(v):8.3f} .. {max(v):8.3f}')
        for kind in ('captured', 'eager'):
            a, b = med[(kind, 'torch tail')], med[(kind, 'device')]
            spread = max(max(ms[(kind, w)]) - min(ms[(kind, w)]) for w in ('torch tail', 'device'))
            lines.append(f'  {kind}: device - torch tail = {b - a:+.3f} ms/step ({100 * (b - a) / a:+.1f} %), '
                         f'largest spread of a leg {spread:.3f} ms')
        del legs
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if out:
        with open(out, 'w') as f:
            f.write(text)


def trace(batch=256, steps=5):
    import torch
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.training import CapturedStep
    for frames in FRAMES:
        x, y = _batch(batch, frames)
        m, arena, bucket, opt = _setup(True)
        st = CapturedStep(m, CrossEntropyLoss(), opt, arena, bucket, x, y, eager=True)
        for _ in range(steps):
            st.step(x, y)
        torch.cuda.synchronize()
    print(f'trace: {steps} eager device-path steps at each of {FRAMES} frames, batch {batch}')


def step_bytes(batch, frames):
    """(forward, backward) bytes one training step's drop_add_act launches need: every operand once.  Forward: z_pre, the
    residual operand if any, out, the bits (a byte per four floats).  Backward: dout, the bits, z_pre, r_pre for a conv
    residual, dza, dzr where there is a residual.  The head's (N, 256) launch is included."""
    fwd = bwd = 0
    t = frames
    for c, s, res in PLAN:
        t = (t - 1) // s + 1
        e = batch * c * t * V
        fwd += e * (4 + (4 if res else 0) + 4) + e // 4
        bwd += e * (4 + 4 + (4 if res == 'conv' else 0) + 4 + (4 if res else 0)) + e // 4
    e = batch * 256
    return fwd + 8 * e + e // 4, bwd + 8 * e + e // 4


def report(path, batch=256, steps=5, out=None):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp']))
    lines = [f'kernel times from a separate rocprofv3 --kernel-trace run of `trace {batch} {steps}` (eager device-path steps)']
    for key, which in (('drop_add_act_fwd_kernel', 0), ('drop_add_act_bwd_kernel', 1)):
        d = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows if key in r['Kernel_Name']]
        per = len(PLAN) + 1
        assert len(d) == len(FRAMES) * steps * per, (key, len(d))
        for i, frames in enumerate(FRAMES):
            us = sum(d[i * steps * per:(i + 1) * steps * per]) / steps
            nbytes = step_bytes(batch, frames)[which]
            lines.append(f'  {frames} frames  {key:24s} {us:9.1f} us per step over {per} launches, {nbytes / 1e6:9.1f} MB needed '
                         f'-> {nbytes / us / 1e6:6.2f} TB/s')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if out:
        with open(out, 'a') as f:
            f.write(text)


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'time'
    if mode == 'time':
        time_steps(*(int(a) for a in sys.argv[2:5]), *sys.argv[5:6])
    elif mode == 'trace':
        trace(*(int(a) for a in sys.argv[2:4]))
    elif mode == 'report':
        report(sys.argv[2], *(int(a) for a in sys.argv[3:5]), *sys.argv[5:6])
    else:
        raise SystemExit(__doc__)
