"""tests/guidance_ref.py, the fp64 restatement the guidance kernels are held to, against the reference itself: it reproduces both
recorded weight maps of tests/golden/guidance.npz (the reference's own visual.visualize_fusion_effect) from the recorded features,
to the rounding of the reference's float32 steps; it agrees with a loop-and-np.partition form of the same rule and with torch's
own bilinear resize on seeded three-clip, two-person data; and each of guidance_ref.DEFECTS fails those checks.  The seeded inputs
of tests/test_gpu_guidance_stages.py meet that file's two conditions (checked here, without a GPU)."""
import os

import numpy as np
import pytest
import torch

import guidance_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'guidance.npz')
TARGETS, K, FRAMES = (3, 11, 7, 18, 14), 15, 5


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def check_fixture(gold, tag, defect=None):
    """the reference's recorded map from its recorded feature.  Its float32 steps: the intensity (a torch sum of C squares and a
    root: E), the normalisation and the mean of <= 15 float32 values (guidance_ref's weights bar, plus 16 u 255 / 127 for that
    float32 mean), the bilinear resize (the map bar)."""
    feat = gold[f'{tag}/feature']
    I = R.intensity(feat)
    assert R.conditioned(I)
    E = R.intensity_bar_max(I, feat.shape[1])
    dw = R.weights_bar(I, E) + 16 * R.U * 255 / 127
    w = R.joint_weights(I, TARGETS, K, defect)
    H, W = gold[f'{tag}/map'].shape
    got = R.weight_map(w, FRAMES, (H, W), defect)[0, 0]
    bar = R.map_bar(R.joint_weights(I, TARGETS, K), FRAMES, H, dw)[0][:, None]
    err = np.abs(got - gold[f'{tag}/map'].astype(np.float64))
    assert np.all(err <= bar), f'{tag}: {float((err / bar).max()):.3g} bars'
    return float((err / bar).max())


def seeded_intensity():
    """(3, 16, 20, 2), whole numbers 0 .. 255 with both ends present: the normalisation is exact (f = I), sums of whole numbers
    are exact, values repeat inside every column (ties).  Clip 0: person 1 is stronger; clip 1: person 0 is; clip 2: person 1 is
    person 0 with its joints rolled by one -- the two means are EQUAL while the columns differ, which tells < from <=."""
    r = np.random.RandomState(11)
    I = r.randint(20, 200, size=(3, 16, 20, 2)).astype(np.float64)
    I[0, :, :, 1] += 40
    I[1, :, :, 0] += 40
    I[2, :, :, 1] = np.roll(I[2, :, :, 0], 1, axis=1)
    I[0, 0, 0, 0], I[1, 3, 5, 1] = 0, 255
    return I


def loop_form(I, targets, k, frames, size):
    """the rule as loops over clips and joints with np.partition, and torch's own resize in float64"""
    f = np.abs(I)
    if f.max() - f.min() != 0:
        f = 255 * (f - f.min()) / (f.max() - f.min())
    N, T, V, M = f.shape
    canvas = np.zeros((N, 1, R.MAP_ROWS, R.STRIPE * frames))
    for n in range(N):
        who = 1 if M > 1 and f[n, :, :, 0].mean() < f[n, :, :, 1].mean() else 0
        for j, v in enumerate(targets):
            if v >= V:
                continue
            col = f[n, :, v, who]
            part = np.partition(-col, min(k, len(col) - 1))
            if R.STRIPE * (j + 1) <= canvas.shape[3]:
                canvas[n, 0, R.STRIPE * j:R.STRIPE * (j + 1), :] = -part[:k].mean()
    canvas = torch.from_numpy(canvas) / 127.0
    return torch.nn.functional.interpolate(canvas, size=size, mode='bilinear', align_corners=False).numpy()


def check_seeded(defect=None):
    I = seeded_intensity()
    worst = 0.0
    for targets, k, frames, size in (((3, 11, 7, 18, 14), 15, 5, (224, 224)), ((3, 25, 7), 5, 2, (7, 5)), ((0,), 20, 5, (448, 3)),
                                     ((3, 11, 7, 18, 14), 15, 5, (225, 225))):
        want = loop_form(I, targets, k, frames, size)
        got = R.weight_map(R.joint_weights(I, targets, k, defect), frames, size, defect)
        assert got.shape == want.shape
        err = float(np.abs(got - want).max())
        assert err <= 1e-12 * max(1.0, float(np.abs(want).max())), (targets, size, err)
        worst = max(worst, err)
    return worst


@pytest.mark.parametrize('tag', ['t52', 't128'])
def test_reproduces_the_reference_recorded_map(gold, tag):
    feat = gold[f'{tag}/feature']
    assert feat.shape == (1, 256, {'t52': 13, 't128': 32}[tag], 20, 1)       # one case on each side of T' <= 15
    assert check_fixture(gold, tag) <= 1.0


def test_agrees_with_the_loop_form_and_torch_resize():
    check_seeded()
    r = np.random.RandomState(5)
    feat = r.standard_normal((3, 20, 7, 20, 2))
    t = torch.from_numpy(feat)
    assert np.allclose(R.intensity(feat), ((t * t).sum(dim=1) ** 0.5).numpy(), rtol=1e-14, atol=0)
    assert np.allclose(R.pooled(feat), t.mean((2, 3, 4)).numpy(), rtol=1e-12, atol=1e-15)
    h = np.ascontiguousarray(feat.transpose(0, 4, 1, 2, 3)).reshape(6, 20, 7, 20)
    assert np.array_equal(R.from_h(h, 2), feat)
    const = np.full((2, 4, 20, 1), 3.5)                                   # max == min: nothing is normalised
    assert np.array_equal(R.joint_weights(const, (3, 25), 15), np.array([[3.5 / 127, 0.0]] * 2))


@pytest.mark.parametrize('defect', R.DEFECTS)
def test_each_defect_fails_the_checks(gold, defect):
    failed = 0
    for chk in (lambda: check_fixture(gold, 't52', defect), lambda: check_fixture(gold, 't128', defect), lambda: check_seeded(defect)):
        try:
            chk()
        except AssertionError:
            failed += 1
    assert failed >= 1, defect
    want_fixture = {'k_smallest': 't128', 'stripe_columns': 't52'}.get(defect)
    if want_fixture:                # these two are visible in the reference's own maps (224 rows from 225 hide align_corners)
        with pytest.raises(AssertionError):
            check_fixture(gold, want_fixture, defect)


def test_the_stage_inputs_meet_their_conditions():
    """tests/test_gpu_guidance_stages.py asserts these on the GPU box before it looks at a device result; here for every case
    without one."""
    import guidance_cases as S
    for cid, c in S.CASES.items():
        S.assert_conditions(cid, S.problem(c))
    got = {k: {c[k] for c in S.CASES.values()} for k in ('C', 'T', 'V', 'size', 'Crgb')}
    assert got['C'] >= {1, 20, 256} and got['T'] >= {1, 13, 15, 16, 17, 75} and got['V'] >= {2, 17, 20, 25, 32}
    assert got['size'] >= {(224, 224), (7, 5), (225, 225), (448, 3)} and got['Crgb'] >= {1, 15}
    assert {(c['N'], c['M']) for c in S.CASES.values()} >= {(1, 1), (2, 2), (3, 1)}
    assert {len(c['targets']) for c in S.CASES.values()} >= {1, 5}


def test_the_ties_case_tells_a_rank_without_tie_break():
    """ties_t75 has 7 distinct frames in 75 (10 or 11 copies of each value in every column) and k = 15: the copies of the second
    largest value lie across the 15th place.  Rank counting that breaks no ties takes all of them and is off by far more than the
    weights bar; on a case without such a group (ucla_t13) it cannot be told from the rule."""
    import guidance_cases as S
    p = S.problem(S.CASES['ties_t75'])
    col = p['I'][0, :, p['targets'][0], 0]
    vals, counts = np.unique(col, return_counts=True)
    assert len(vals) == 7 and counts[-1] < S.K < counts[-1] + counts[-2]           # the group of the second largest straddles k
    bar = R.weights_bar(p['I'], R.intensity_bar_max(p['I'], p['C']))
    bad = R.joint_weights(p['I'], p['targets'], S.K, defect='no_tie_break')
    assert np.all(np.abs(bad - p['w']) > 100 * bar), (np.abs(bad - p['w']).min(), bar)
    q = S.problem(S.CASES['ucla_t13'])
    assert np.abs(R.joint_weights(q['I'], q['targets'], S.K, defect='no_tie_break') - q['w']).max() <= 1e-12
