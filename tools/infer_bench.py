"""GPU-box tool: forward-only throughput (eval mode, no_grad) of the N-UCLA or the NTU-RGB+D model at a few batch sizes -- what
the inference-only callers (cross-modal attention, ensemble eval, visualisation) see.  Eager launches and HIP-graph replay.
    python tools/infer_bench.py [--model ctrgcn|stgcn] [--graph ucla|ntu|coco|openpose|synthetic] [--t T] [--ab R] [batch ...]     (default ctrgcn, ucla, T = 64, batches 1 16 256)
--graph synthetic --joints V [--persons M]: graph.synthetic's binary tree of V joints (default 21), M persons (default 1) -- a
skeleton of any joint count; CTR-GCN models of 8..28 joints without a dedicated family take the f2g kernels (tam_gcn_amd/f2g.py,
TAMGCN_F2G_MAX_FRAMES).
--f2g R: the run-time-V family (f2g.FusedEvalG, called directly) against whatever Model.forward routes to (f2 / f2v at 17, 18,
20, 25 joints), alternating within this process, R timings each, eager and HIP-graph replay.
--model stgcn: models.stgcn.Model on the same graphs; its small-batch family is tam_gcn_amd/f2s.py (TAMGCN_F2S_MAX_FRAMES).
--graph ntu: 25 joints, 2 persons (a batch of B clips is 2B clip-persons); coco: 17 joints, 1 person; openpose: 18 joints, 2
persons (the skeletons a pose estimator hands over: graph.coco, graph.openpose).
Batches of at most TAMGCN_F2_MAX_CLIPS clips (ucla) / TAMGCN_F2V_MAX_FRAMES (ntu) / TAMGCN_F2J_MAX_FRAMES (coco, openpose)
clip-persons x frames take the small-batch kernel family (tam_gcn_amd/f2.py, f2v.py); TAMGCN_F2=0 puts them on the general eval
path for comparison.
--ab R: the family against the general path of the same process, alternating, R timings each (median [min .. max]); the
family is forced on whatever the routing bound says (that bound is what this mode is for).
--ensemble G [--ab R]: a G-stream ensemble (joint, bone, motion, bone-motion, ... models of one architecture, fused scores) for
one joint batch, every arrangement under HIP-graph replay, alternating within this process, R timings each (default 7):
    (a) serial    stream_derive x (G - 1), the G models' own forwards one after another, score_fuse -- one graph
    (b) streams   the same with the G models on G streams inside the graph (functional.model_stream)
    (c) grouped   inference.StreamEnsemble(arrangement='grouped'): one grouped launch sequence
then GraphedForward(StreamEnsemble(...)) with its default arrangement, and (a) and (c) launched from Python (eager): both
carry the host cost of G parameter-state keys per call.  --model stgcn --ensemble G: the same for ST-GCN models (f2s.GroupedEvalST).
--model stgcn --saliency [--ab R]: gradient saliency (tam_gcn_amd/saliency.py) of the true class, (N, V) per batch, alternating in
this process, R timings each (default 5):
    A  general   eval-mode Model.forward in grad mode and torch.autograd.grad of the gathered score with respect to x (the only
                 way without the f2s backward kernels), then |.| summed per joint -- eager
    B  family    saliency.joint_saliency on the f2s forward + backward chain, forced on whatever the routing bound says -- eager and
                 under HIP-graph replay
--guidance [--ab R]: skeleton guidance (tam_gcn_amd/guidance.py; the reference's visual.py:53-87) on N-UCLA clips (1 and 16 x 3 x 52 x
20 x 1 with rgb (N, 15, 224, 224)) and one NTU clip (1 x 3 x 300 x 25 x 2), alternating in this process, R timings each (default 7):
    A  host tail   the reference's shape of it: extract_feature, the torch ops, .cpu().numpy(), np.partition in two Python loops,
                   F.interpolate and the multiply -- eager only (it synchronises, so it cannot be captured)
    B  device      SkeletonGuidance.apply -- eager and under HIP-graph replay
then the three launches on their own (back to back on one stream between two events: the larger of the cost of issuing the operator from
Python and the kernel time; a kernel trace, a run of its own, gives the kernel time itself) and the apply kernel's bytes per second (rgb read + out written).  --guidance --kernels runs
only those launches, 20 of each per shape, for a run under rocprofv3 --kernel-trace --stats."""
import os, statistics, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tam_gcn_amd.models.ctrgcn import Model
dev = torch.device('cuda:0')
torch.manual_seed(0)
args = sys.argv[1:]
T, graph, ab, ens_g, model, sal, joints, persons, vs_g, guid, only_kernels = 64, 'ucla', 0, 0, 'ctrgcn', False, 21, 1, 0, False, False
while args and args[0].startswith('--'):
    if args[0] == '--saliency':
        sal, args = True, args[1:]
        continue
    if args[0] in ('--guidance', '--kernels'):                 # --kernels implies --guidance
        guid, only_kernels, args = True, only_kernels or args[0] == '--kernels', args[1:]
        continue
    if args[0] == '--t':
        T = int(args[1])
    elif args[0] == '--graph':
        graph = args[1]
    elif args[0] == '--ab':
        ab = int(args[1])
    elif args[0] == '--model' and args[1] in ('ctrgcn', 'stgcn'):
        model = args[1]
    elif args[0] == '--ensemble':
        ens_g = int(args[1])
    elif args[0] == '--joints':
        joints = int(args[1])
    elif args[0] == '--persons':
        persons = int(args[1])
    elif args[0] == '--f2g':
        vs_g = int(args[1])
    else:
        sys.exit(__doc__)
    args = args[2:]
if model == 'stgcn':
    from tam_gcn_amd.models.stgcn import Model
if graph == 'ntu':
    V, P = 25, 2
    m = Model(num_class=60, num_point=25, num_person=2, graph='graph.ntu_rgb_d.Graph', graph_args=dict(labeling_mode='spatial'))
elif graph == 'coco':
    V, P = 17, 1
    m = Model(num_class=10, num_point=17, num_person=1, graph='tam_gcn_amd.graph.coco.Graph', graph_args=dict(labeling_mode='spatial'))
elif graph == 'openpose':
    V, P = 18, 2
    m = Model(num_class=12, num_point=18, num_person=2, graph='tam_gcn_amd.graph.openpose.Graph', graph_args=dict(labeling_mode='spatial'))
elif graph == 'synthetic':
    V, P = joints, persons
    m = Model(num_class=10, num_point=V, num_person=P, graph='tam_gcn_amd.graph.synthetic.Graph', graph_args=dict(num_node=V, arity=2))
elif graph != 'ucla':
    sys.exit(__doc__)
else:
    V, P = 20, 1
    m = Model(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
m = m.to(dev).eval()
with torch.no_grad():
    for k, p in m.named_parameters():
        if k.endswith('alpha'):
            p.fill_(0.5)
n = 50


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def capture(x, fn=None):
    fn = fn or m
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y = fn(x)
    torch.cuda.current_stream().wait_stream(s); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = fn(x)
    g.replay(); torch.cuda.synchronize()
    return g, y


def ensemble_bench(G, batches, R):
    import copy
    from tam_gcn_amd import ops, functional as Fn
    from tam_gcn_amd.inference import GraphedForward, StreamEnsemble
    names = ['joint', 'bone', 'motion', 'bone_motion']
    streams = [names[g % 4] for g in range(G)]
    models = [m]
    gen = torch.Generator().manual_seed(1)
    for g in range(1, G):                                  # the same architecture, every parameter its own
        mg = copy.deepcopy(m)
        with torch.no_grad():
            for p in mg.parameters():
                p.mul_((1 + 0.02 * (2 * torch.rand(p.shape, generator=gen) - 1)).to(dev))
        models.append(mg.eval())
    ens = StreamEnsemble(models, streams, arrangement='grouped')
    auto = StreamEnsemble(models, streams)
    side = [torch.cuda.Stream(device=dev) for _ in range(G)]

    def serial(x):
        ys = [mg(ops.stream_derive(x, ens.parent, s)) for mg, s in zip(models, streams)]
        return ops.score_fuse(torch.stack(ys), ens.weights, False)[0]

    def on_streams(x):
        cur = torch.cuda.current_stream(dev)
        ys = []
        for st, mg, s in zip(side, models, streams):
            st.wait_stream(cur)
            with Fn.model_stream(st):
                ys.append(mg(ops.stream_derive(x, ens.parent, s)))
        for st in side:
            cur.wait_stream(st)
        return ops.score_fuse(torch.stack(ys), ens.weights, False)[0]

    def graphed(fn, x):
        s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                fn(x)
        torch.cuda.current_stream().wait_stream(s); torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = fn(x)
        g.replay(); torch.cuda.synchronize()
        return g, y

    print(f'ensemble of {G} ({", ".join(streams)}), graph = {graph} (V = {V}, M = {P}), T = {T}; {R} alternating timings of {n} calls: '
          'median [min .. max]', flush=True)
    for B in batches:
        x = torch.rand(B, 3, T, V, P, device=dev) * 2 - 1
        with torch.no_grad():
            gf = GraphedForward(auto)                       # what a user gets: the default arrangement under GraphedForward
            ya = gf(x)
            arr = {'(a) serial, graph ': graphed(serial, x), '(b) streams, graph': graphed(on_streams, x), '(c) grouped, graph': graphed(ens, x),
                   'GraphedForward(StreamEnsemble), default arrangement': (next(iter(gf._graphs.values()))[0], ya)}
            ref = arr['(a) serial, graph '][1]
            for k, (g, y) in arr.items():
                d = float((y - ref).abs().max()) / float(ref.abs().max())
                assert d <= 1e-4, (k, d)
            times = {k: [] for k in list(arr) + ['(a) serial, eager ', '(c) grouped, eager', 'StreamEnsemble default, eager']}
            for _ in range(R):
                for k, (g, _) in arr.items():
                    times[k].append(timed(g.replay))
                times['(a) serial, eager '].append(timed(lambda: serial(x)))
                times['(c) grouped, eager'].append(timed(lambda: ens(x)))
                times['StreamEnsemble default, eager'].append(timed(lambda: auto(x)))
        for k, v in times.items():
            print(f'batch {B:3d} x {P} x {T}  {k}: {statistics.median(v) * 1e3:7.3f} ms [{min(v) * 1e3:7.3f} .. {max(v) * 1e3:7.3f}]', flush=True)
        a, b, c = (times[k] for k in list(arr)[:3])
        best, which = min((statistics.median(a), 'a'), (statistics.median(b), 'b'))
        spread = max(max(a) - min(a), max(b) - min(b), max(c) - min(c))
        gain = best - statistics.median(c)
        print(f'      (c) against the better of (a), (b) = ({which}): {statistics.median(c) / best:5.2f}x of its time, '
              f'{gain * 1e3:+.3f} ms; largest [min .. max] spread of the three {spread * 1e3:.3f} ms: (c) '
              + ('WINS by more than the spread' if gain > spread else 'does NOT win (not below the better one by more than the spread)'), flush=True)


def saliency_bench(batches, R):
    from tam_gcn_amd import f2s, saliency
    f2s.F2S_BWD_MAX_FRAMES = 1 << 40
    print(f'saliency, model = stgcn, graph = {graph} (V = {V}, M = {P}), T = {T}; {R} alternating timings of {n} calls: median [min .. max]', flush=True)
    for B in batches:
        x = torch.rand(B, 3, T, V, P, device=dev) * 2 - 1
        lab = torch.randint(0, 10, (B,), device=dev)

        def general():
            xd = x.detach().requires_grad_(True)
            (g,) = torch.autograd.grad(torch.gather(m(xd), 1, lab.unsqueeze(1)).sum(), xd)
            return g.abs().sum((1, 2, 4))

        def family():
            return saliency.joint_saliency(m, x, lab)
        for _ in range(3):
            ya, yb = general(), family()
        s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            family()
        torch.cuda.current_stream().wait_stream(s); torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            yg = family()
        g.replay(); torch.cuda.synchronize()
        assert torch.equal(yg, yb)
        d = float((ya - yb).abs().max()) / float(ya.abs().max())
        times = {'A general, eager': [], 'B family, eager ': [], 'B family, graph ': []}
        for _ in range(R):
            times['A general, eager'].append(timed(general))
            times['B family, eager '].append(timed(family))
            times['B family, graph '].append(timed(g.replay))
        for k, v in times.items():
            print(f'batch {B:4d} x {P} x {T} ({B * P * T:6d} frames)  {k}: {statistics.median(v) * 1e3:7.3f} ms [{min(v) * 1e3:7.3f} .. {max(v) * 1e3:7.3f}]', flush=True)
        a, b = times['A general, eager'], times['B family, eager ']
        spread = max(max(a) - min(a), max(b) - min(b))
        gain = statistics.median(a) - statistics.median(b)
        print(f'      family vs general saliency: {d:.1e} relative;  eager family {statistics.median(b) / statistics.median(a):5.2f}x of the general path\'s time, '
              f'{gain * 1e3:+.3f} ms; larger [min .. max] spread {spread * 1e3:.3f} ms: the family '
              + ('WINS by more than the spread' if gain > spread else 'does NOT win by more than the spread'), flush=True)


def f2g_bench(batches, R):
    from tam_gcn_amd import f2, f2v, f2g
    f2.F2_MAX_CLIPS = f2v.F2V_MAX_FRAMES = f2v.F2J_MAX_FRAMES = f2g.F2G_MAX_FRAMES = 1 << 40
    eng = f2g.FusedEvalG(m)
    print(f'f2g (V at run time) against the routed family, graph = {graph} (V = {V}, M = {P}), T = {T}; {R} alternating timings of {n} calls: '
          'median [min .. max]', flush=True)
    for B in batches:
        x = torch.rand(B, 3, T, V, P, device=dev) * 2 - 1
        with torch.no_grad():
            routed = next((type(e).FAMILY for e in (m._f2(x), m._f2v(x), m._f2j(x), m._f2g(x)) if e is not None), 'general')
            runs = {}
            for name, fn in ((routed, m), ('f2g', eng)):
                for _ in range(3):
                    fn(x)
                g, y = capture(x, fn)
                runs[name] = (fn, g, y, {'eager': [], 'graph': []})
            for _ in range(R):
                for name, (fn, g, y, r) in runs.items():
                    r['eager'].append(timed(lambda: fn(x)))
                    r['graph'].append(timed(g.replay))
        ys = [v[2] for v in runs.values()]
        for name, (fn, g, y, r) in runs.items():
            print(f'batch {B:4d} x {P} x {T} ({B * P * T:6d} frames) {name:7s}: ' + '   '.join(
                f'{k} {statistics.median(v) * 1e3:7.3f} ms [{min(v) * 1e3:7.3f} .. {max(v) * 1e3:7.3f}]' for k, v in r.items()), flush=True)
        a, b = runs[routed][3]['graph'], runs['f2g'][3]['graph']
        print(f'      f2g vs {routed} logits: {float((ys[1] - ys[0]).abs().max()) / float(ys[0].abs().max()):.1e} relative;  '
              f'replay: f2g takes {statistics.median(b) / statistics.median(a):5.3f}x of the {routed} time', flush=True)


def guidance_bench(R):
    import numpy as np
    import torch.nn.functional as F
    from tam_gcn_amd import guidance
    ucla = dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
    ntu = dict(num_class=60, num_point=25, num_person=2, graph='graph.ntu_rgb_d.Graph', graph_args=dict(labeling_mode='spatial'))
    targets, k, frames = (3, 11, 7, 18, 14), 15, 5
    print(f'guidance: {R} alternating timings of {n} calls each: median [min .. max]', flush=True)
    for margs, shape in ((ucla, (1, 3, 52, 20, 1)), (ucla, (16, 3, 52, 20, 1)), (ntu, (1, 3, 300, 25, 2))):
        mm = Model(**margs).to(dev)
        with torch.no_grad():
            for name, p in mm.named_parameters():
                if name.endswith('alpha'):
                    p.fill_(0.5)
        x = torch.rand(*shape, device=dev) * 2 - 1
        rgb = torch.rand(shape[0], 15, 224, 224, device=dev)
        for b in mm.modules():                            # running statistics of this input: features of a sensible size
            if isinstance(b, torch.nn.modules.batchnorm._BatchNorm):
                b.momentum = 1.0
        with torch.no_grad():
            mm.train()(x)
        mm.eval()
        g = guidance.SkeletonGuidance(mm, targets, k, frames)

        def host_tail():
            with torch.no_grad():
                _, feat = mm.extract_feature(x)
            f = np.abs(((feat * feat).sum(dim=1) ** 0.5).cpu().numpy())
            if f.max() - f.min() != 0:
                f = 255 * (f - f.min()) / (f.max() - f.min())
            N, _, V_, M_ = f.shape
            canvas = np.zeros((N, 1, 225, 45 * frames))
            for i in range(N):
                who = 1 if M_ > 1 and f[i, :, :, 0].mean() < f[i, :, :, 1].mean() else 0
                for j, v in enumerate(targets):
                    if v < V_ and 45 * (j + 1) <= canvas.shape[3]:
                        col = f[i, :, v, who]
                        canvas[i, 0, 45 * j:45 * (j + 1), :] = -np.partition(-col, min(k, len(col) - 1))[:k].mean()
            wm = F.interpolate(torch.from_numpy(canvas).float().to(dev) / 127.0, size=rgb.shape[-2:], mode='bilinear', align_corners=False)
            return rgb * wm

        def device():
            return g.apply(x, rgb)
        if only_kernels:
            with torch.no_grad():
                h, N, M_ = mm._block_stack(x)
                for _ in range(20):
                    inten, pooled, minmax = torch.ops.tamgcn.guidance_reduce(h, M_)
                    w = torch.ops.tamgcn.guidance_weights(inten, minmax, g._joints_on(dev), k)
                    torch.ops.tamgcn.guidance_apply(w, rgb, frames, 224, 224, False)
            torch.cuda.synchronize()
            print(f'{shape}: 20 calls of each launch', flush=True)
            continue
        for _ in range(3):
            ya, yb = host_tail(), device()
        gr, yg = capture(x, lambda _: device())
        assert torch.equal(yg, yb)
        d = float((ya - yb).abs().max()) / float(ya.abs().max())
        times = {'A host tail, eager': [], 'B device, eager   ': [], 'B device, graph   ': []}
        for _ in range(R):
            times['A host tail, eager'].append(timed(host_tail))
            times['B device, eager   '].append(timed(device))
            times['B device, graph   '].append(timed(gr.replay))
        tag = f'{margs["num_point"]} joints, x {shape}, rgb {tuple(rgb.shape)}'
        for name, v in times.items():
            print(f'{tag}  {name}: {statistics.median(v) * 1e3:7.3f} ms [{min(v) * 1e3:7.3f} .. {max(v) * 1e3:7.3f}]', flush=True)
        a, b = times['A host tail, eager'], times['B device, eager   ']
        spread = max(max(a) - min(a), max(b) - min(b))
        gain = statistics.median(a) - statistics.median(b)
        print(f'      device vs host tail: {d:.1e} relative;  eager device path {statistics.median(b) / statistics.median(a):5.2f}x of the host tail\'s time, '
              f'{gain * 1e3:+.3f} ms; larger [min .. max] spread {spread * 1e3:.3f} ms: the device path '
              + ('WINS by more than the spread' if gain > spread else 'does NOT win by more than the spread'), flush=True)
        # the three launches on their own
        with torch.no_grad():
            h, N, M_ = mm._block_stack(x)
            inten, pooled, minmax = torch.ops.tamgcn.guidance_reduce(h, M_)
            jt = g._joints_on(dev)
            w = torch.ops.tamgcn.guidance_weights(inten, minmax, jt, k)
            H, W = rgb.shape[-2:]
            reps = 200
            for name, fn, nbytes in (('guidance_reduce (2 launches)', lambda: torch.ops.tamgcn.guidance_reduce(h, M_), h.numel() * 4),
                                     ('guidance_weights', lambda: torch.ops.tamgcn.guidance_weights(inten, minmax, jt, k), inten.numel() * 4),
                                     ('guidance_apply', lambda: torch.ops.tamgcn.guidance_apply(w, rgb, frames, H, W, False), 2 * rgb.numel() * 4)):
                for _ in range(5):
                    fn()
                best = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(reps):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    best.append(e0.elapsed_time(e1) / reps * 1e-3)
                t = statistics.median(best)
                print(f'      {name:30s} {t * 1e6:8.2f} us per call back to back [{min(best) * 1e6:.2f} .. {max(best) * 1e6:.2f}]   '
                      f'{nbytes / 1e6:8.3f} MB moved: {nbytes / t / 1e12:6.3f} TB/s', flush=True)


if guid:
    guidance_bench(ab or 7)
    sys.exit(0)
if vs_g:
    if model != 'ctrgcn':
        sys.exit('--f2g: the family serves --model ctrgcn')
    f2g_bench([int(v) for v in args] or (1, 16), vs_g)
    sys.exit(0)
if sal:
    if model != 'stgcn':
        sys.exit('--saliency: the family serves --model stgcn')
    saliency_bench([int(v) for v in args] or (1, 16), ab or 5)
    sys.exit(0)
if ens_g:
    ensemble_bench(ens_g, [int(v) for v in args] or (1, 4), ab or 7)
    sys.exit(0)
print(('model = stgcn, ' if model == 'stgcn' else '') + f'graph = {graph} (V = {V}, M = {P}), T = {T}, TAMGCN_F2 = {os.environ.get("TAMGCN_F2", "1")}', flush=True)
for B in ([int(v) for v in args] or (1, 16, 256)):
    x = torch.rand(B, 3, T, V, P, device=dev) * 2 - 1
    with torch.no_grad():
        if ab:
            if model == 'stgcn':
                from tam_gcn_amd import f2s
                f2s.F2S_MAX_FRAMES = 1 << 40
            elif graph == 'ntu':
                from tam_gcn_amd import f2v
                f2v.F2V_MAX_FRAMES = 1 << 40
            elif graph in ('coco', 'openpose'):
                from tam_gcn_amd import f2v
                f2v.F2J_MAX_FRAMES = 1 << 40
            elif graph == 'synthetic':
                from tam_gcn_amd import f2, f2v, f2g
                f2.F2_MAX_CLIPS = f2v.F2V_MAX_FRAMES = f2v.F2J_MAX_FRAMES = f2g.F2G_MAX_FRAMES = 1 << 40
            else:
                from tam_gcn_amd import f2
                f2.F2_MAX_CLIPS = 1 << 40
            runs, keep = {}, []
            for on in ('1', '0'):
                os.environ['TAMGCN_F2'] = on
                for _ in range(3):
                    m(x)
                g, y = capture(x)
                keep.append((g, y))
                runs[on] = (g, {'eager': [], 'graph': []})
            for _ in range(ab):
                for on in ('1', '0'):
                    os.environ['TAMGCN_F2'] = on
                    g, r = runs[on]
                    r['eager'].append(timed(lambda: m(x)))
                    r['graph'].append(timed(g.replay))
            d = float((keep[0][1] - keep[1][1]).abs().max()) / float(keep[1][1].abs().max())
            for on, name in (('1', 'family '), ('0', 'general')):
                r = runs[on][1]
                print(f'batch {B:4d} x {P} x {T} ({B * P * T:6d} frames) {name}: ' + '   '.join(
                    f'{k} {statistics.median(v) * 1e3:7.3f} ms [{min(v) * 1e3:7.3f} .. {max(v) * 1e3:7.3f}]' for k, v in r.items()), flush=True)
            print(f'      family vs general logits: {d:.1e} relative', flush=True)
            continue
        for _ in range(3):
            y = m(x)
        eager = timed(lambda: m(x))
        g, y = capture(x)
        graph_t = timed(g.replay)
        extra = ''
        for sp in ([int(v) for v in os.environ.get('INFER_SPLITS', '').split(',') if v] if B >= 16 else []):
            from tam_gcn_amd.inference import GraphedForward
            fast = GraphedForward(m, split=sp)
            ys = fast(x); torch.cuda.synchronize()
            assert float((ys - y).abs().max()) <= 1e-4 * float(y.abs().max()), float((ys - y).abs().max())   # (slices of <= 32 clips take the f2 kernels)
            dt = timed(lambda: fast(x))
            extra += f'   split {sp}: {dt * 1e3:6.2f} ms ({B / dt:8.0f} clips/s)'
    print(f'batch {B:4d}: eager {eager * 1e3:7.2f} ms ({B / eager:9.0f} clips/s)   hip graph {graph_t * 1e3:7.2f} ms ({B / graph_t:9.0f} clips/s)' + extra, flush=True)
