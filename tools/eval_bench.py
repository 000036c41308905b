"""GPU-box tool: what a val epoch costs from user code (profiles/captured_eval.txt).

    python tools/eval_bench.py [clips] [batch] [rounds]     default 464 clips (the N-UCLA val split's size), batch 64 (the
                                                            reference's test batch), 7 rounds

One process, the three forms alternated A, B, C, A, B, C, ... (a round each), wall time of a whole epoch per form, every leg
ending with its metrics on the host:
  A  the reference-shaped host loop (processor/recognition_rgb.py:71-101) on the API without evaluation.py: Feeder.batch,
     model(x), CrossEntropyLoss, loss.item(), output.cpu().numpy(), label.cpu().numpy(), then numpy metrics
  B  CapturedEval.run().compute()
  C  B right after a parameter changed (an in-place write that bumps a parameter's version): the forward graph is captured again
The split is synthetic (seeded random-walk skeletons of 20..80 frames); the model is the seeded N-UCLA model in eval() mode.
"""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

MARGS = dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))


def _split(path, n, seed=11):
    import numpy as np
    rng = np.random.default_rng(seed)
    dd = []
    for k in range(n):
        name = f'a{1 + k % 6:02d}_s{k:03d}_e00_v03'
        frames = int(rng.integers(20, 81))
        clip = rng.normal(size=(1, 20, 3)) + 0.05 * np.cumsum(rng.normal(size=(frames, 20, 3)), axis=0)
        os.makedirs(os.path.join(path, name), exist_ok=True)
        with open(os.path.join(path, name, name + '.json'), 'w') as f:
            json.dump({'skeletons': clip.tolist()}, f)
        dd.append({'file_name': name, 'label': 1 + (3 * k) % 10})
    return dd


def host_loop(model, fd, B, loss_fn):
    import numpy as np
    import torch
    n, K = len(fd), MARGS['num_class']
    loss_value, result_frag, label_frag = [], [], []
    with torch.no_grad():
        for b in range(0, n, B):
            data, label, _ = fd.batch(range(b, min(b + B, n)))
            output = model(data)
            loss = loss_fn(output, label)
            loss_value.append(loss.item())
            result_frag.append(output.cpu().numpy())
            label_frag.append(label.cpu().numpy())
    result, label = np.concatenate(result_frag), np.concatenate(label_frag)
    predict_label = np.argmax(result, axis=1)
    conf = np.zeros((K, K), dtype=np.int64)
    np.add.at(conf, (label, predict_label), 1)
    rank = result.argsort()
    top5 = sum(l in rank[i, -5:] for i, l in enumerate(label)) / len(label)
    return {'loss': float(np.mean(loss_value)), 'top1': float(np.sum(predict_label == label) / len(label)), 'top5': top5, 'confusion': conf}


def main(clips=464, batch=64, rounds=7):
    import numpy as np
    import torch
    from params import fill_state_
    from tam_gcn_amd.evaluation import CapturedEval
    from tam_gcn_amd.feeder.feeder_nucla_gcn import Feeder
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.models.ctrgcn import Model
    dev = torch.device('cuda:0')
    with tempfile.TemporaryDirectory() as path:
        fd = Feeder(path, 'val', data_dict=_split(path, clips), device=dev)
    m = Model(**MARGS)
    fill_state_(m.state_dict(), seed=3)
    m = m.to(dev).train()
    x, _, _ = fd.batch(range(min(clips, 64)))
    for _ in range(40):                                          # running statistics of these inputs, not of the seed
        m(x)
    m.eval()
    ce = CrossEntropyLoss()
    ev = CapturedEval(m, fd, batch)
    legs = {'A': lambda: host_loop(m, fd, batch, ce), 'B': lambda: ev.run().compute()}

    def changed():
        with torch.no_grad():
            m.fc.bias.mul_(1.0)                                  # same values, new version: the state key moves
        return ev.run().compute()
    legs['C'] = changed
    for fn in legs.values():                                     # one untimed pass each
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    last = {}
    for _ in range(rounds):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = fn()
            times[k].append((time.perf_counter() - t0) * 1e3)
    a, b = last['A'], last['B']
    same = (np.array_equal(a['confusion'], b['confusion']) and a['top1'] == b['top1'] and a['top5'] == b['topk'][5])
    print(f'N-UCLA model, {clips} clips, batch {batch} ({-(-clips // batch)} batches), {rounds} rounds alternated A, B, C after one untimed pass each; '
          f'{ev.captures} forward captures in all')
    names = {'A': 'host loop (Feeder.batch, model, CrossEntropyLoss, .item(), .cpu().numpy(), numpy metrics)',
             'B': 'CapturedEval.run().compute()', 'C': 'CapturedEval.run().compute() after a parameter change (re-capture)'}
    for k in legs:
        t = sorted(times[k])
        print(f'  {k}  median {statistics.median(t):8.2f} ms/epoch   min {t[0]:8.2f}   max {t[-1]:8.2f}   {names[k]}')
    print(f'  A and B agree on the confusion matrix, top-1 and top-5: {same}; loss A {a["loss"]:.6f}  B {b["loss"]:.6f} '
          f'(A\'s last batch is {clips % batch or batch} clips, B\'s is padded to {batch})')


if __name__ == '__main__':
    main(*[int(v) for v in sys.argv[1:4]])
