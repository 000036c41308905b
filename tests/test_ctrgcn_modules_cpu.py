"""CPU: the case table and the bars of tests/ctrgcn_module_ref.py shown to hold and to bite, before anyone trusts a green
tests/test_gpu_ctrgcn_modules.py.

  * every case finds its well-conditioned fp64 teacher within MAX_TRIES nudges, in train and in eval mode;
  * every additive term of dx that a max-norm bar could swallow is at least SHARE_FACTOR x the case's dx bar (looser mode);
  * the fp32 oracle (ref32) is inside every bar, for every case, train / eval, both modes;
  * the restatement the faults are planted in reproduces every teacher to fp64 rounding;
  * five subtly wrong evaluations, each in fp64 so that only the planted error is present, FAIL judge() on every case the error
    can occur in, the case where it is smallest named with -s."""
import pytest
import torch

import ctrgcn_module_ref as R

BNS = lambda tag: (True,) if R.kind_of(tag) == 'CTRGC' else (True, False)      # noqa: E731  CTRGC has no BatchNorm


def test_the_table_holds_what_the_routes_need():
    """The shapes stay at the smallest where the route still exists, and every kind, residual mode and joint count is there."""
    kinds = {R.kind_of(t) for t in R.CASES}
    assert kinds == {'CTRGC', 'unit_gcn', 'TemporalConv', 'unit_tcn', 'MultiScale_TemporalConv', 'TCN_GCN_unit'}
    for tag, (kind, kw, shape, _) in R.CASES.items():
        assert shape[0] == 2 and shape[2] <= 13 and shape[3] in (20, 25, 17), tag
        assert kw['in_channels'] in (3, 32, 48, 64, 128) and kw['out_channels'] in (32, 48, 64, 128), tag
    for kind in ('CTRGC', 'unit_gcn'):
        assert {s[3] for k, _, s, _ in R.CASES.values() if k == kind} == {20, 25, 17}
    for kind in ('unit_gcn', 'MultiScale_TemporalConv'):
        assert {R.rmode_of(t) for t in R.CASES if R.kind_of(t) == kind} == {'conv', 'identity', 'zero'}
    assert any(s[2] == 1 for k, _, s, _ in R.CASES.values() if k == 'CTRGC')


@pytest.mark.parametrize('tag', list(R.CASES), ids=R.case_id)
def test_every_case_finds_its_teacher(tag):
    """A condition of the table, not a measurement: teacher() raises when MAX_TRIES nudges leave a ReLU input or a max-pool
    runner-up closer than MARGIN.  Adaptive=False cases compute what their partner computes."""
    for training in BNS(tag):
        t = R.teacher(tag, training)
        assert t.tries < R.MAX_TRIES
        assert all(torch.isfinite(v.double()).all() for v in t.q.values())
        if not training:
            sd, _, bnames = R.state(tag, torch.float64)
            assert all(torch.equal(t.q['buf/' + k], sd['m.' + k]) for k in bnames), 'an eval-mode teacher moved a buffer'
    partner = R.CASES[tag][3].get('partner')
    if partner:
        a, b = R.evaluate(tag, R.x0(tag), True), R.evaluate(partner, R.x0(partner), True)
        assert torch.equal(a['y'], b['y']) and torch.equal(a['dx'], b['dx'])
        assert not any(q.endswith('PA') for q in a) and any(q.endswith('PA') for q in b)


@pytest.mark.parametrize('tag', [t for t in R.CASES if R.share_terms(t)], ids=R.case_id)
def test_no_term_of_dx_is_below_what_the_bar_sees(tag):
    for training in BNS(tag):
        t = R.teacher(tag, training)
        bar = R.bars(tag, 1, 'dx', t.q['dx'], R.ref32_errors(t)['dx'])
        for term in R.share_terms(tag):
            s = R.share(tag, term, training)
            print(f'{tag} bn {"train" if training else "eval"}: share of {term} in dx {s:.3g} = {s / bar:.0f} x the dx bar {bar:.1e}')
            assert s >= R.SHARE_FACTOR * bar, (tag, training, term, s, bar)


@pytest.mark.parametrize('tag', list(R.CASES), ids=R.case_id)
def test_fp32_oracle_is_inside_every_bar(tag):
    for training in BNS(tag):
        t = R.teacher(tag, training)
        for mode in (1, 0):
            ratios = R.verify(R.ref32(tag, training), t, mode)
            # bar >= 4 x the fp32 oracle's own error on everything under a relative bar, so these sit at or below 0.25
            print(R.line(f'{tag} mode {mode} bn {"train" if training else "eval"} nudges {t.tries} worst {max(ratios.values()):.2g}', ratios))
            for q, (e, b) in R.widened(t, mode).items():
                print(f'{tag} mode {mode} bn {"train" if training else "eval"}: {q} widened to {b:.2e} from the fp32 oracle\'s {e:.2e}')


@pytest.mark.parametrize('tag', list(R.CASES), ids=R.case_id)
def test_the_plain_restatement_is_the_oracle(tag):
    """No switch set: the restatement the faults are planted in reproduces the teacher to fp64 rounding."""
    for training in BNS(tag):
        t = R.teacher(tag, training)
        ratios = R.verify(R.evaluate(tag, t.x, training, fwd=R.restated), t, 0)
        assert max(ratios.values()) <= 1e-4, (tag, training, ratios)


@pytest.mark.parametrize('fault', R.FAULTS)
def test_a_subtly_wrong_module_fails(fault):
    """pq_scale: the p / q term of CTRGC's dx scaled by (T - 1) / T;  identity_dropped: the identity residual's gradient left out
    of the MS-TCN's dx;  biased_var: running_var updated with the biased variance (EVERY running_var of the case must miss);
    res_late: a stride-2 residual convolution's data gradient written one frame late;  dilation: the second temporal branch's
    dilation off by one.  Judged in the split mode's bars, the wider ones, on EVERY case the error can occur in."""
    weakest, escaped, n = None, [], 0
    for tag in R.CASES:
        if not R.fault_applies(fault, tag):
            continue
        n += 1
        t = R.teacher(tag, True)
        ratios, misses = R.judge(R.evaluate(tag, t.x, True, fwd=R.restated, fault=fault), t, 1)
        if fault == 'biased_var':
            seen = {q: r for q, r in ratios.items() if q.endswith('running_var')}
            assert seen, tag
            q = min(seen, key=seen.get)               # the running_var the fault shows least in
            if not seen[q] > 1.0:
                escaped.append(f'{tag}: {q} at {seen[q]:.3g} of its bar')
        else:
            q = max(ratios, key=ratios.get)
            if fault in ('pq_scale', 'identity_dropped', 'res_late'):
                q = 'dx'                              # the quantity the fault is in
            if not ratios[q] > 1.0:
                escaped.append(f'{tag}: {q} at {ratios[q]:.3g} of its bar')
        if weakest is None or ratios[q] < weakest[0]:
            weakest = (ratios[q], tag, q)
    assert n > 0
    print(f'fault {fault}: on {n} cases, smallest on {weakest[1]}, caught by {weakest[2]} at {weakest[0]:.3g} x its bar')
    assert not escaped, f'fault {fault} passes judge(): ' + '; '.join(escaped)
