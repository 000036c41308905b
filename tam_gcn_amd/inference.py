"""HIP-graph replay of the eval-mode forward for the inference-only callers (the ensemble evaluation
loop ensemble/ensemble_ctrgcn_resnet_eval.py:147-183, the frozen backbone of models/resnet_gcn_attention.py:82-85,
visual.py:53-55).  Those loops call model(data) with one batch shape over and over; at small batches the launch-fused
eval path is bound by its ~118 launches, and a captured graph replays them without the host in between (batch 1: 4.3 ms
eager -> 2.8 ms, tools/infer_bench.py).

    fast = GraphedForward(model)            # model.eval(), parameters frozen for the lifetime of the capture
    for data, ... in loader:
        logits = fast(data.float().cuda())  # first call per input shape captures, later calls replay

The output tensor is the graph's static buffer: it is overwritten by the next call with the same shape (clone it to keep
it).  Parameter VALUES may change between calls (the graph reads them through their pointers; the eval path's folded
BatchNorm coefficients are keyed on parameter versions, so re-capture with .reset() after loading a new state dict).

A multi-stream ensemble (the published four-stream accuracies: joint, bone, joint-motion and bone-motion models whose scores
are summed) as ONE call on the joint clips:

    ens = StreamEnsemble([joint, bone, motion, bone_motion])       # eval() models of one architecture: all models.ctrgcn.Model
                                                                   # or all models.stgcn.Model
    with torch.no_grad():
        fused = ens(x)                                             # (N, K); GraphedForward(ens) captures it
        fused, pred, scores = ens.predict(x)                       # + arg max (N) and the per-stream scores (G, N, K)"""
import torch
from torch import nn

from . import ops

__all__ = ['GraphedForward', 'StreamEnsemble']

# where models.ctrgcn.Model keeps its small-batch engines: f2.FusedEval, f2v.FusedEvalV, f2v.FusedEvalJ, f2g.FusedEvalG (one slot
# per class), and models.stgcn.Model its f2s.FusedEvalST
ENGINE_SLOTS = ('_tamgcn_f2', '_tamgcn_f2v', '_tamgcn_f2j', '_tamgcn_f2g', '_tamgcn_f2s')


class GraphedForward:
    """split (default 1): eval-mode BatchNorm uses the running statistics, so a batch may be cut into `split` slices that run
    side by side on their own HIP streams inside the graph (functional.model_stream) and land in one output tensor -- kernels that
    wait for operands leave room that another slice's kernels fill (four models side by side in one graph run 23 % faster than
    one after the other: DESIGN.md §3 lessons).  Measured on the N-UCLA model: 256 clips 9.36 -> 8.74 ms, 512 clips 17.8 -> 16.5 ms
    with split = 4.  Slices are kept at >= 64 clips (smaller ones would take the latency-oriented f2 kernels, which lose on
    throughput); only tensor-valued methods (forward)."""

    def __init__(self, model, method='forward', max_shapes=8, split=1):
        if model.training:
            raise ValueError('GraphedForward: put the model in eval() mode first (train mode updates running statistics)')
        self.model, self.method, self.max_shapes, self.split = model, method, max_shapes, int(split)
        self._graphs = {}
        self._streams = None

    def reset(self):
        self._graphs.clear()

    def _capture(self, x):
        # A wrapped object that routes differently when its forward is replayed as a graph (StreamEnsemble) is told so for
        # the warm-up calls AND the capture: the warm-up must take the route the capture takes.
        told = hasattr(self.model, '_tamgcn_graphed')
        if told:
            before, self.model._tamgcn_graphed = self.model._tamgcn_graphed, True
        try:
            return self._capture_told(x)
        finally:
            if told:
                self.model._tamgcn_graphed = before

    def _capture_told(self, x):
        fn = getattr(self.model, self.method)
        static_in = x.clone()
        with torch.no_grad():
            s = torch.cuda.Stream(device=x.device)
            s.wait_stream(torch.cuda.current_stream(x.device))
            with torch.cuda.stream(s):                       # warm-up off the capture: allocator, side streams, cached coefficients
                for _ in range(2):
                    fn(static_in)
            torch.cuda.current_stream(x.device).wait_stream(s)
            g = torch.cuda.CUDAGraph()
            nsl = max(1, min(self.split, x.shape[0] // 64))
            if nsl > 1:
                from . import functional as Fn
                if self._streams is None:
                    self._streams = [torch.cuda.Stream(device=x.device) for _ in range(self.split)]
                parts = static_in.chunk(nsl)
                with torch.cuda.graph(g):
                    cur = torch.cuda.current_stream(x.device)
                    outs = []
                    for st, xp in zip(self._streams, parts):
                        st.wait_stream(cur)
                        with Fn.model_stream(st):
                            outs.append(fn(xp))
                    for st in self._streams[:len(parts)]:
                        cur.wait_stream(st)
                    out = torch.cat(outs)
            else:
                with torch.cuda.graph(g):
                    out = fn(static_in)
        # The graph reads the eval path's folded BatchNorm coefficients through their pointers, and those tensors are
        # owned by the per-module caches (functional._eval_cached): an eager forward after a parameter change evicts
        # them.  This entry keeps them alive, so a replay without reset() reads stale coefficients, never freed memory.
        keep = [dict(m.__dict__['_tamgcn_eval_cache']) for m in self.model.modules() if '_tamgcn_eval_cache' in m.__dict__]
        for slot in ENGINE_SLOTS:                            # small batches: the folded weights of tam_gcn_amd.f2 / f2v, likewise
            eng = self.model.__dict__.get(slot)
            if eng:
                keep.append(eng._blocks)
        hook = getattr(self.model, '_tamgcn_keep_alive', None)   # a wrapped object with folded tensors of its own (StreamEnsemble)
        if hook is not None:
            keep.append(hook())
        return g, static_in, out, keep

    def __call__(self, x):
        if not x.is_cuda:
            raise RuntimeError('GraphedForward: expected a HIP (cuda) tensor; there is no CPU path')
        key = (tuple(x.shape), x.dtype, x.device.index)
        ent = self._graphs.get(key)
        if ent is None:
            if len(self._graphs) >= self.max_shapes:
                self._graphs.pop(next(iter(self._graphs)))
            ent = self._graphs[key] = self._capture(x)
        g, static_in, out, _ = ent
        static_in.copy_(x)
        g.replay()
        return out


def default_parent(graph):
    """0-based bone parent of every joint from a graph's 1-based parent table (tam_gcn_amd.graph.*: 0 marks the root); the
    root is its own parent, so its bone is 0."""
    return [v if p == 0 else p - 1 for v, p in enumerate(graph.parents)]


class StreamEnsemble(nn.Module):
    """The fused class scores of G models, model g fed stream `streams[g]` of the JOINT clips x.

    streams   names of ops.STREAM_MODES ('joint', 'bone', 'motion' = 'joint_motion', 'bone_motion'), one per model
    weights   G floats (default ones), kept in a device tensor: fused = sum_g weights[g] * scores_g (softmax=True: of the
              softmax-normalised scores), ensemble.fuse's arithmetic
    parent    int32 [V] tensor or sequence: 0-based bone parent of every joint.  Default: from the models' graph.parents with
              the root as its own parent.  The reference N-UCLA feeder's bone table is feeder.feeder_nucla_gcn.BONE_PARENT;
              passing it reproduces that feeder's bone stream.

    x is (N, C, T, V, M) or (N, T, V*C), float32 on the GPU, under torch.no_grad().  forward(x) -> fused (N, K);
    predict(x) -> (fused, pred int64 (N), scores (G, N, K)).

    Small inputs (CTR-GCN: G*N*M <= f2.F2_MAX_CLIPS at V = 20, G*N*M*T <= f2v.F2V_MAX_FRAMES at V = 25 and <=
    f2v.F2J_MAX_FRAMES at V = 17, 18; ST-GCN: G*N*M*T <= f2s.F2S_MAX_FRAMES at any V <= 32; TAMGCN_F2 != 0; no forward
    hooks on any sub-module) run as ONE grouped launch sequence (f2.GroupedEval: 54 launches whatever G is; f2s.GroupedEvalST:
    24 with the score fusion).  Anything else runs each model's own forward on its derived stream (ops.stream_derive) and fuses the scores: the
    same result to rounding, at any size.  The models are all CTR-GCN or all ST-GCN: a mix is refused.

    arrangement (None: by measurement, profiles/stream_ensemble_bench.txt) | 'grouped' | 'streams' | 'serial'.  Launched from
    Python the grouped sequence is the fastest (54 launches against 216).  Inside a HIP-graph capture (GraphedForward(ens)) the
    launches cost nothing; there the grouped sequence does NOT beat what was possible before it: with one clip-person per
    model (N-UCLA batch 1) it ties with the G models' own forwards on G streams (functional.model_stream) inside that
    arrangement's own spread, only steadier, and beyond (N-UCLA batch 4; NTU batch 1, two persons) the G streams are 7-11 %
    faster: kernels of different models fill each other's tails, which one grouped launch per stage cannot.  So None takes
    'streams' for a call made by GraphedForward (its warm-up calls and its capture alike) with N*M > 1, and 'grouped'
    otherwise.  A capture made by hand (torch.cuda.graph around ens(x)) gets no such switch: pass arrangement= there.  The
    routes agree bit for bit where the grouped one applies.

    ST-GCN ensembles were measured on their own (profiles/stgcn_ensemble_bench.txt, four models, HIP-graph replay, medians of 7
    alternating rounds whose [min .. max] spread is at most 0.009 ms) and the measurement gives the SAME rule.  One clip-person per
    model (N-UCLA batch 1): grouped 0.625 ms, G streams 0.701 ms, serial 1.821 ms -- the grouped pass wins by 11 %, outside the
    spread.  Beyond: N-UCLA batch 4 grouped 1.376 ms against 1.180 ms on G streams, NTU batch 1 (two persons) 1.233 ms against
    1.109 ms -- the streams are 14 % and 10 % faster.  So None takes 'streams' under GraphedForward with N*M > 1 and 'grouped'
    otherwise, as above.  Launched from Python the grouped sequence takes 0.79 / 1.39 / 1.24 ms against 1.83 / 2.44 / 2.04 ms for
    the models one after another."""

    def __init__(self, models, streams=('joint', 'bone', 'motion', 'bone_motion'), weights=None, softmax=False, parent=None,
                 arrangement=None):
        super().__init__()
        from . import f2, f2s
        models, streams = list(models), list(streams)
        if len(streams) != len(models):
            raise ValueError(f'StreamEnsemble: {len(models)} models but {len(streams)} streams')
        for s in streams:
            if s not in ops.STREAM_MODES:
                raise ValueError(f'StreamEnsemble: unknown stream {s!r} (one of {sorted(ops.STREAM_MODES)})')
        if arrangement not in (None, 'grouped', 'streams', 'serial'):
            raise ValueError(f'StreamEnsemble: arrangement {arrangement!r} (None, "grouped", "streams" or "serial")')
        self.arrangement = arrangement
        self._side = None                                      # G HIP streams, made by the first call that takes 'streams'
        self._tamgcn_graphed = False                           # set by GraphedForward around its warm-up and capture
        weights = [1.0] * len(models) if weights is None else [float(w) for w in weights]
        if len(weights) != len(models):
            raise ValueError(f'StreamEnsemble: {len(models)} models but {len(weights)} weights')
        st = [hasattr(m, 'st_gcn_networks') for m in models]   # models.stgcn.Model: the f2s family and its own bound
        if any(st) and not all(st):
            raise ValueError('StreamEnsemble: a mix of ST-GCN and CTR-GCN models (model '
                             f'{st.index(not st[0])} is not of model 0\'s architecture); every model must be of one architecture')
        self._st = bool(st) and st[0]
        try:                                                   # ValueError: train mode, devices, differing geometry
            self._eng = (f2s.GroupedEvalST if self._st else f2.GroupedEval)(models)
        except f2.Unsupported:
            self._eng = None                                   # outside both families: every call takes the per-model route
            if any(m.training for m in models):
                raise ValueError('StreamEnsemble: put every model in eval() mode first')
        V = models[0].num_point
        if parent is None:
            parent = default_parent(models[0].graph)
        parent = [int(p) for p in (parent.tolist() if torch.is_tensor(parent) else parent)]
        if len(parent) != V or any(p < 0 or p >= V for p in parent):
            raise ValueError(f'StreamEnsemble: parent must hold {V} joint indices in [0, {V})')
        dev = next(models[0].parameters()).device
        self.models = nn.ModuleList(models)
        self.streams, self.softmax = streams, bool(softmax)
        self.register_buffer('weights', torch.tensor(weights, dtype=torch.float32, device=dev), persistent=False)
        self.register_buffer('parent', torch.tensor(parent, dtype=torch.int32, device=dev), persistent=False)
        self.register_buffer('modes', torch.tensor([ops.STREAM_MODES[s] for s in streams], dtype=torch.int32, device=dev), persistent=False)
        self.train(False)

    def _tamgcn_keep_alive(self):
        keep = [] if self._eng is None else self._eng.keep_alive()
        for m in self.models:
            for slot in ENGINE_SLOTS:
                eng = m.__dict__.get(slot)
                if eng:
                    keep.append(eng._blocks)
        return keep

    def _grouped(self, x5):
        """(the grouped engine, its stacked folded tensors) if this call is one for it, else (None, None)."""
        from . import f2, f2s, f2v
        eng = self._eng
        none = (None, None)
        if eng is None or not f2.enabled():
            return none
        G, (N, _, T, V, M) = len(self.models), x5.shape
        if V != eng.V or M != eng.M:
            return none
        if self._st:
            if G * N * M * T > f2s.F2S_MAX_FRAMES:
                return none
        elif (G * N * M > f2.F2_MAX_CLIPS) if V == 20 else (G * N * M * T > (f2v.F2V_MAX_FRAMES if V == 25 else f2v.F2J_MAX_FRAMES)):
            return none
        for mod in self.modules():
            if mod._forward_hooks or mod._forward_pre_hooks:
                return none
        try:
            return eng, eng._packed(x5.device)                 # folding and geometry checks, before anything is launched:
        except f2.Unsupported:                                 # the one walk over the models' state keys of this call
            self._eng = None
            return none

    def predict(self, x):
        if torch.is_grad_enabled():
            raise RuntimeError('StreamEnsemble is an inference path: call it under torch.no_grad()')
        if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32:
            raise RuntimeError('StreamEnsemble: expected a float32 HIP (cuda) tensor; there is no CPU path')
        if any(m.training for m in self.models):
            raise RuntimeError('StreamEnsemble: a model went back to train() mode')
        V = self.models[0].num_point
        if x.dim() == 3:
            N, T, VC = x.shape
            x = x.view(N, T, V, -1).permute(0, 3, 1, 2).unsqueeze(-1)
        if x.dim() != 5 or x.shape[3] != V:
            raise RuntimeError(f'StreamEnsemble: expected (N, C, T, {V}, M) or (N, T, {V}*C), got {tuple(x.shape)}')
        x = x.contiguous()
        arr = self.arrangement or ('streams' if self._tamgcn_graphed and x.shape[0] * x.shape[4] > 1 else 'grouped')
        eng, stacked = self._grouped(x) if arr == 'grouped' else (None, None)
        if eng is not None:
            scores = eng.run(x, self.parent, self.modes, stacked)
        elif arr == 'streams':
            scores = self._on_streams(x)
        else:
            scores = torch.stack([m(ops.stream_derive(x, self.parent, s)) for m, s in zip(self.models, self.streams)])
        fused, pred, _ = ops.score_fuse(scores, self.weights, self.softmax)
        return fused, pred, scores

    def _on_streams(self, x):
        """Each model's own forward on its derived stream, the G of them side by side on G HIP streams."""
        from . import functional as Fn
        if self._side is None:                                 # (GraphedForward's warm-up calls come here before its capture)
            self._side = [torch.cuda.Stream(device=x.device) for _ in self.models]
        cur = torch.cuda.current_stream(x.device)
        ys = []
        for st, m, s in zip(self._side, self.models, self.streams):
            st.wait_stream(cur)
            with Fn.model_stream(st):
                y = m(ops.stream_derive(x, self.parent, s))
            y.record_stream(cur)
            ys.append(y)
        for st in self._side:
            cur.wait_stream(st)
        return torch.stack(ys)

    def forward(self, x):
        return self.predict(x)[0]
