"""The end-to-end cases of tests/test_gpu_guidance.py: de-degenerated models (params.fill_state_) whose running statistics are those
of the case's own input -- one train-mode pass of the fp64 oracle with BatchNorm momentum 1, the way tests/golden/make_golden.py
prepares its eval cases (seeded running statistics push the eval-mode features to 1e9) -- and the fp64 references of every guidance
output, computed once per case on the CPU."""
import functools

import numpy as np
import torch

import guidance_ref as R
from params import fill_state_, make_input
from oracle import ctrgcn_oracle as O

G = 'tam_gcn_amd.graph.'
UCLA = dict(num_class=10, num_point=20, num_person=1, graph=G + 'ucla.Graph', graph_args=dict(labeling_mode='spatial'))
NTU = dict(num_class=12, num_point=25, num_person=2, graph=G + 'ntu_rgb_d.Graph', graph_args=dict(labeling_mode='spatial'))
COCO = dict(num_class=10, num_point=17, num_person=1, graph=G + 'coco.Graph', graph_args=dict(labeling_mode='spatial'))
TREE21 = dict(num_class=9, num_point=21, num_person=2, graph=G + 'synthetic.Graph', graph_args=dict(num_node=21, arity=2))

# tag -> (model arguments, input shape, state seed, input seed, rgb (Crgb, H, W));  big: one clip more than f2.F2_MAX_CLIPS (32)
CASES = {
    'ucla_t52':  (UCLA, (1, 3, 52, 20, 1), 61, 62, (15, 224, 224)),
    'ucla_t128': (UCLA, (2, 3, 128, 20, 1), 71, 72, (3, 56, 60)),
    'ucla_t128_one': (UCLA, (1, 3, 128, 20, 1), 71, 72, (15, 224, 224)),     # the fixture's t128 clip alone (clip 0 of ucla_t128)
    'ntu_t20':   (NTU, (1, 3, 20, 25, 2), 81, 82, (3, 32, 30)),
    'coco_t16':  (COCO, (1, 3, 16, 17, 1), 83, 84, (1, 7, 5)),
    'tree21':    (TREE21, (1, 3, 16, 21, 2), 85, 86, (3, 32, 30)),
    'ucla_big':  (UCLA, (33, 3, 16, 20, 1), 87, 88, (1, 16, 12)),
}
TARGETS, K, FRAMES = (3, 11, 7, 18, 14), 15, 5


def clip(tag):
    margs, shape, _, x_seed, _ = CASES[tag]
    x = make_input(shape, seed=x_seed)
    if shape[4] == 2:
        x[..., 1] = 0.4 * x[..., 1] + 0.2            # the second person moves less: the two persons' mean intensities lie apart
    return x


def rgb(tag):
    N = CASES[tag][1][0]
    return make_input((N,) + CASES[tag][4], seed=CASES[tag][3] + 100, lo=0.0, hi=1.0)


@functools.lru_cache(maxsize=None)
def settled_state(tag):
    """the model's fp32 CPU state with running statistics of clip(tag), and the same values in fp64 for the oracle"""
    from tam_gcn_amd.models import ctrgcn as M
    margs, shape, state_seed, _, _ = CASES[tag]
    sd = M.Model(**margs).state_dict()
    fill_state_(sd, seed=state_seed)
    sd64 = {k: (v.detach().clone().double() if v.is_floating_point() else v.detach().clone()) for k, v in sd.items()}
    old, O.BN_MOMENTUM = O.BN_MOMENTUM, 1.0
    try:
        with torch.no_grad():
            O.model_blocks(clip(tag).double(), sd64, margs['num_point'], training=True)
    finally:
        O.BN_MOMENTUM = old
    for k in sd:
        if 'running_' in k:
            sd[k].copy_(sd64[k].float())
            sd64[k] = sd[k].double()                   # both sides hold exactly the fp32 values
    return sd, sd64


@functools.lru_cache(maxsize=None)
def reference(tag):
    """fp64: feature (N, C, T', V, M) of the oracle, intensity, pooled, weights, map and rgb * map"""
    margs = CASES[tag][0]
    _, sd64 = settled_state(tag)
    with torch.no_grad():
        feat = O.model_extract_feature(clip(tag).double(), sd64, margs['num_point'], training=False)[0].numpy()
    I = R.intensity(feat)
    w = R.joint_weights(I, TARGETS, K)
    image = rgb(tag).double().numpy()
    wmap = R.weight_map(w, FRAMES, image.shape[-2:])
    return dict(feature=feat, I=I, pooled=R.pooled(feat), pooled_mag=np.abs(feat).mean((2, 3, 4)), w=w, map=wmap, out=image * wmap)
