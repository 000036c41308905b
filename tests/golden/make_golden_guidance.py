"""Golden vectors for skeleton guidance (tam_gcn_amd/guidance.py).  Runs ONLY where a checkout of the reference is at hand: it
runs the reference's OWN visual.visualize_fusion_effect (not a copy of it) and writes data only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_guidance.py <path to the reference checkout>

visual.py imports a data feeder, OpenCV and matplotlib at module level; none of them takes part in the arithmetic between
extract_feature and the plot, so four stand-ins go into sys.modules before `import visual`:
    cv2                           an empty module
    feeder.feeder_nucla_fusion    a Feeder whose [0] returns the case's seeded ((x_ske, x_rgb), label, index)
    matplotlib, matplotlib.pyplot imshow records its argument, everything else does nothing
The second recorded image is weight_resized[0, 0] (visual.py:89), shape (224, 224).

Per case (T = 52: T' = 13 <= 15, the mean of all frames; T = 128: T' = 32 > 15, a real top-15): the reference Model's state is
fill_state_(seed) followed by one train-mode pass over the case's clip with every BatchNorm's momentum at 1 (make_golden.py's way to
realistic running statistics: plain fill_state_ statistics give intensities around 1e9), saved to a temporary file that
visualize_fusion_effect loads as weights_path.  Stored: the clip x, the seeds (state, clip, rgb) and the rgb shape (the rgb tensor is
make_input(rgb_shape[1:], rgb_seed, 0, 1): 3 MB of uniform noise are not stored; tests/test_gpu_guidance.py rebuilds it), the
recorded map, and the reference model's extract_feature output for the clip.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from params import fill_state_, make_input  # noqa: E402

MARGS = dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'), in_channels=3)
RGB_SHAPE = (15, 224, 224)
# tag -> (frames, state seed, clip seed, rgb seed)
CASES = {'t52': (52, 61, 62, 63), 't128': (128, 71, 72, 73)}


def _stubs(current, shown):
    cv2 = types.ModuleType('cv2')
    feeder_mod = types.ModuleType('feeder.feeder_nucla_fusion')

    class Feeder:
        def __init__(self, **kw):
            pass

        def __getitem__(self, i):
            return (current['x_ske'], current['x_rgb']), 0, i
    feeder_mod.Feeder = Feeder
    mpl = types.ModuleType('matplotlib')
    plt = types.ModuleType('matplotlib.pyplot')

    def nothing(*a, **k):
        return None
    plt.__getattr__ = lambda name: nothing
    plt.imshow = lambda img, *a, **k: shown.append(np.array(img, copy=True))
    mpl.pyplot = plt
    sys.modules.update({'cv2': cv2, 'feeder.feeder_nucla_fusion': feeder_mod, 'matplotlib': mpl, 'matplotlib.pyplot': plt})


def main(ref):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    current, shown = {}, []
    _stubs(current, shown)
    import visual                            # the reference's
    from models import ctrgcn as R           # the reference's
    torch.set_num_threads(8)
    out = {}
    for tag, (T, state_seed, x_seed, rgb_seed) in CASES.items():
        x = make_input((1, 3, T, 20, 1), seed=x_seed)
        rgb = make_input(RGB_SHAPE, seed=rgb_seed, lo=0.0, hi=1.0)
        m = R.Model(**MARGS)
        fill_state_(m.state_dict(), seed=state_seed)
        bns = [mod for mod in m.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)]
        for b in bns:
            b.momentum = 1.0
        m.train()
        with torch.no_grad():
            m(x)
        for b in bns:
            b.momentum = 0.1
        m.eval()
        with torch.no_grad():
            feat = m.extract_feature(x)[1]
        current['x_ske'], current['x_rgb'] = x[0].numpy(), rgb.numpy()
        del shown[:]
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, 'state.pt')
            torch.save(m.state_dict(), path)
            cwd = os.getcwd()
            os.chdir(tmp)                    # visualize_fusion_effect writes its figure file name into the working directory
            try:
                visual.visualize_fusion_effect('unused', path)
            finally:
                os.chdir(cwd)
        assert len(shown) == 3 and shown[1].shape == RGB_SHAPE[1:], [s.shape for s in shown]
        wmap = shown[1].astype(np.float32)
        assert float(np.abs(wmap - wmap[:, :1]).max()) <= 1e-6 * float(wmap.max()), 'the columns of the map are not constant'
        inten = (feat.double() ** 2).sum(1).sqrt()
        print(f'{tag}: feature {tuple(feat.shape)}, intensity {float(inten.min()):.4g} .. {float(inten.max()):.4g}, '
              f'map rows {float(wmap.min()):.4g} .. {float(wmap.max()):.4g}')
        out[f'{tag}/x'] = x.numpy()
        out[f'{tag}/seeds'] = np.array([state_seed, x_seed, rgb_seed], dtype=np.int64)
        out[f'{tag}/rgb_shape'] = np.array((1,) + RGB_SHAPE, dtype=np.int64)
        out[f'{tag}/map'] = wmap
        out[f'{tag}/feature'] = feat.numpy()
    np.savez_compressed(os.path.join(HERE, 'guidance.npz'), **out)
    print('guidance.npz', len(out), 'arrays', os.path.getsize(os.path.join(HERE, 'guidance.npz')), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
