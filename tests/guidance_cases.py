"""The seeded cases of tests/test_gpu_guidance_stages.py (the raw guidance ABI against guidance_ref) and their two conditions,
kept apart from the GPU file so that tests/test_guidance_ref_cpu.py can check the conditions without a GPU.

Between them the cases take: (N, M) in {(1, 1), (2, 2), (3, 1)}; C in {1, 20, 256}; T' in {1, 13, 15, 16, 17, 75} (k = 15: both sides
of T' <= k and the edge); V in {2, 17, 20, 25, 32}; J in {1, 5}; a target joint >= V; (H, W) in {(224, 224), (7, 5), (225, 225),
(448, 3)}; Crgb in {1, 15}; an rgb view whose data pointer is only 4-byte aligned; a constant feature map (max == min); repeated
values inside a joint's column with a group of them across the k-th place (ties); person 1 a bitwise copy of person 0; the person
choice either way.

A feature map of independent noise has channel norms that all but coincide (256 terms average out), and the normalisation would
amplify rounding by 255 / (max - min) without bound: every column is scaled by its own factor in 0.3 .. 1.5, and a person's
columns by `person_gain`."""
import numpy as np
import torch

import guidance_ref as R

K = 15
UCLA_TARGETS = (3, 11, 7, 18, 14)

# special: const | ties | copy (clip 1's person 1 is a copy of its person 0)
CASES = {
    'ucla_t13':      dict(N=1, M=1, C=256, T=13, V=20, targets=UCLA_TARGETS, size=(224, 224), Crgb=15),
    'ntu_t16_2p':    dict(N=2, M=2, C=20, T=16, V=25, targets=UCLA_TARGETS, size=(7, 5), Crgb=1, person_gain=((1.0, 1.6), (1.6, 1.0))),
    'tiny':          dict(N=3, M=1, C=1, T=1, V=2, targets=(1,), size=(448, 3), Crgb=1),
    'coco_t15_copy': dict(N=2, M=2, C=20, T=15, V=17, targets=UCLA_TARGETS, size=(225, 225), Crgb=15, special='copy',
                          person_gain=((1.0, 1.6), (1.0, 1.0))),
    'v32_t17_unaligned': dict(N=1, M=1, C=256, T=17, V=32, targets=(3, 31, 7, 18, 14), size=(224, 224), Crgb=1, misaligned=True),
    'ties_t75':      dict(N=3, M=1, C=20, T=75, V=25, targets=(24,), size=(7, 5), Crgb=1, special='ties'),
    'const':         dict(N=2, M=2, C=20, T=13, V=20, targets=UCLA_TARGETS, size=(7, 5), Crgb=1, special='const'),
    'frames_2':      dict(N=2, M=2, C=1, T=16, V=20, targets=UCLA_TARGETS, size=(224, 224), Crgb=1, frames=2,
                          person_gain=((1.6, 1.0), (1.0, 1.6))),
}


def problem(c, seed=0):
    """h (N*M, C, T', V) fp32 and rgb (N, Crgb, H, W) fp32 (CPU tensors) with the fp64 references of every stage"""
    N, M, C, T, V = c['N'], c['M'], c['C'], c['T'], c['V']
    r = np.random.RandomState(1000 + seed + 7 * C + 13 * T + 17 * V)
    h = r.uniform(-1, 1, size=(N, M, C, T, V)) * r.uniform(0.3, 1.5, size=(N, M, 1, T, V))
    gain = np.asarray(c.get('person_gain', np.ones((N, M))), np.float64)
    h = h * gain[:, :, None, None, None]
    special = c.get('special')
    if special == 'const':
        h[:] = 0.37
    if special == 'ties':
        h = h[:, :, :, np.arange(T) % 7]      # 7 distinct frames, 10 or 11 copies of each: equal values lie across the k-th place
    if special == 'copy':
        h[1, 1] = h[1, 0]
    h = torch.from_numpy(np.ascontiguousarray(h.reshape(N * M, C, T, V)).astype(np.float32))
    H, W = c['size']
    rgb = torch.from_numpy(r.uniform(-1, 1, size=(N, c['Crgb'], H, W)).astype(np.float32))
    feat = R.from_h(h.double().numpy(), M)
    I = R.intensity(feat)
    frames = c.get('frames', 5)
    w = R.joint_weights(I, c['targets'], K)
    wmap = R.weight_map(w, frames, (H, W))
    return dict(h=h, rgb=rgb, M=M, C=C, targets=c['targets'], k=K, frames=frames, size=(H, W), I=I, pooled=R.pooled(feat),
                pooled_mag=np.abs(feat).mean((2, 3, 4)), w=w, map=wmap, out=rgb.double().numpy() * wmap,
                misaligned=bool(c.get('misaligned')), special=special)


def assert_conditions(cid, p):
    """Two discontinuities are conditions on the inputs, decided on the fp64 reference: the normalisation's amplification is bounded
    (max - min >= max / 4, or exactly 0) and no person choice is within reach of rounding (>= 100 bars apart, or a bitwise copy)."""
    I = p['I']
    assert R.conditioned(I), f'{cid}: max - min = {float(I.max() - I.min()):.4g} < max / 4 = {float(I.max()) / 4:.4g}'
    if p['special'] == 'const':
        assert float(I.max() - I.min()) < 1e-12 * float(I.max())     # in fp64 to its rounding; bit-equal on the device
    E = R.intensity_bar_max(I, p['C'])
    assert R.persons_decided(I, E), f'{cid}: a person choice is within 100 bars'
