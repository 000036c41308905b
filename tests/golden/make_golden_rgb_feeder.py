"""Golden vectors for the RGB feeder (tam_gcn_amd/feeder/rgb_feeder.py).  Runs ONLY in the build container.

Smooth synthetic images are written as PNGs into a temporary directory and loaded by the reference's own
feeder.tools.load_rgb_images (tools.py:216-246) with temporal_rgb_frames = 5; one name has no file, which gives the reference's
float zeros.  torchvision is not installed in the build container, so this script installs a STAND-IN torchvision.transforms of
four classes -- Compose, Resize, ToTensor, Normalize -- written to torchvision's arithmetic on PIL and torch:

    Resize((h, w))    img.resize((w, h), Image.BILINEAR)                 (torchvision's default interpolation on a PIL image)
    ToTensor          uint8 HWC -> CHW, .to(float32).div(255)
    Normalize         tensor.clone().sub_(mean[:, None, None]).div_(std[:, None, None]),  mean / std as float32 tensors

PIL itself is the real one.  The flip case (feeder_nucla_resnet.py:57-63: open, convert('RGB'), transpose(FLIP_LEFT_RIGHT),
transform) is made with the same PIL calls and the same three transforms DIRECTLY, not through the reference, and is labelled
'flip/...'.  What is stored is data only: the sources, PIL's resized bytes, and of each float output 4096 seeded elements with
their flat indices; of the absent file's output its shape and whether it is all zero.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rgb_feeder.py
"""
import contextlib
import io
import os
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

from params import sample_indices           # noqa: E402
from rgb_feeder_ref import smooth_images    # noqa: E402


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class Resize:
    def __init__(self, size):
        self.size = size

    def __call__(self, img):
        h, w = self.size
        return img.resize((w, h), Image.BILINEAR)


class ToTensor:
    def __call__(self, pic):
        a = torch.from_numpy(np.array(pic, np.uint8, copy=True))
        return a.view(pic.size[1], pic.size[0], 3).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


class Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, t):
        t = t.clone()
        mean, std = torch.as_tensor(self.mean, dtype=t.dtype), torch.as_tensor(self.std, dtype=t.dtype)
        return t.sub_(mean[:, None, None]).div_(std[:, None, None])


tv = types.ModuleType('torchvision')
tvt = types.ModuleType('torchvision.transforms')
for cls in (Compose, Resize, ToTensor, Normalize):
    setattr(tvt, cls.__name__, cls)
tv.transforms = tvt
sys.modules['torchvision'], sys.modules['torchvision.transforms'] = tv, tvt

from feeder import tools      # noqa: E402  (reference's)

F = 5
# (name, H, W, size): a downscale with 7 taps, an upscale to the model's size, an upscale with clamped windows
CASES = [('down', 37, 53, 16), ('up224', 60, 80, 224), ('tiny', 7, 9, 24)]


def main():
    out = {'F': np.int64(F), 'names': np.array([c[0] for c in CASES])}
    with tempfile.TemporaryDirectory() as root:
        for k, (name, H, W, S) in enumerate(CASES):
            src = smooth_images(1000 + k, 1, H, W)[0]
            Image.fromarray(src).save(os.path.join(root, name + '.png'))
            with Image.open(os.path.join(root, name + '.png')) as im:
                assert np.array_equal(np.asarray(im.convert('RGB')), src)
                resized = np.asarray(im.convert('RGB').resize((S, S), Image.BILINEAR))
            got = tools.load_rgb_images(root, name, F, size=S)
            assert got.shape == (3 * F, S, S) and got.dtype == np.float32, (got.shape, got.dtype)
            idx = sample_indices(got.size, f'rgb_feeder/{name}')
            out[f'{name}/src'], out[f'{name}/size'], out[f'{name}/resized'] = src, np.int64(S), resized
            out[f'{name}/idx'], out[f'{name}/sample'] = idx, got.reshape(-1)[idx].copy()
            # feeder_nucla_resnet.py:57-63, the train path's flip, with the same calls directly
            with Image.open(os.path.join(root, name + '.png')) as im:
                rgb = im.convert('RGB').transpose(Image.FLIP_LEFT_RIGHT)
            fl = Compose([Resize((S, S)), ToTensor(), Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])])(rgb).numpy()
            idx = sample_indices(fl.size, f'rgb_feeder/flip/{name}')
            out[f'flip/{name}/idx'], out[f'flip/{name}/sample'] = idx, fl.reshape(-1)[idx].copy()
        with contextlib.redirect_stdout(io.StringIO()):                 # the reference prints a warning for the absent file
            gone = tools.load_rgb_images(root, 'absent', F, size=24)
        out['absent/shape'] = np.array(gone.shape, dtype=np.int64)
        out['absent/all_zero'] = np.bool_(not gone.any())
        out['absent/dtype'] = np.array(str(gone.dtype))
    path = os.path.join(HERE, 'rgb_feeder.npz')
    np.savez_compressed(path, **out)
    print('rgb_feeder.npz', len(CASES), 'cases', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
