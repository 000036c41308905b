"""The fp64 references of the small-batch eval stages (tests/f2_ref.py) without a GPU: anchored to the fp64 oracle on block
geometries the stock model never has, their mirrored constants held to the source text of csrc/f2_common.h, f2x_body.h, f2.hip and f2v.hip, the ledger's
table held to the list of code paths it must reach, and the bars shown to pass a correct fp32 evaluation and to fail three
planted defects (a dropped tap, a zero-padded pooled maximum, the floor division of the p/q row tiles)."""
import os
import re

import pytest
import torch

import fp64_bars as B
import f2_ref as R
from oracle import ctrgcn_oracle as O

F64 = torch.float64
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tam_gcn_amd', 'csrc')


# ---------------------------------------------------------------------------------------------------------------------
# anchor: e -> gcn -> gemm 0 -> gemm 1 -> tcn composed in float64 == oracle.tcn_gcn_unit(training=False)
# ---------------------------------------------------------------------------------------------------------------------
#            V   N  T  Cin Cout R   nb Cb  ks dils        stride gcn-res block-res
GEOMETRIES = {
    'r12_k7_conv_conv':        (20, 2, 5, 40, 48, 12, 1, 16, 7, (1,), 1, 2, 2),
    'r20_k9_s2_identity_conv': (25, 1, 9, 48, 48, 20, 1, 16, 9, (1,), 2, 1, 2),
    'r1_cin3_k3d5_zero_zero':  (25, 2, 5, 3, 64, 1, 2, 16, 3, (1, 5), 1, 0, 0),
    'r24_nb3_identity':        (20, 1, 6, 80, 80, 24, 3, 16, 3, (1, 2, 3), 1, 1, 1),
    'r4_nb4_k1_s2_conv_zero':  (20, 2, 8, 16, 96, 4, 4, 16, 1, (1, 1, 1, 1), 2, 2, 0),
    'r32_cb48_k5d2_s2':        (25, 1, 9, 64, 144, 32, 1, 48, 5, (2,), 2, 2, 2),
}


def _state(geo, seed):
    V, N, T, Cin, Cout, Rr, nb, Cb, ks, dils, stride, gres, bres = geo
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def rn(*s, scale=1.0, shift=0.0):
        return torch.randn(*s, generator=g, dtype=F64) * scale + shift

    def conv(pfx, o, i, k=1):
        sd[pfx + '.weight'] = rn(o, i, k, 1, scale=(i * k) ** -0.5)
        sd[pfx + '.bias'] = rn(o, scale=0.3)

    def bn(pfx, c):
        sd[pfx + '.weight'], sd[pfx + '.bias'] = rn(c, scale=0.2, shift=1.0), rn(c, scale=0.2)
        sd[pfx + '.running_mean'], sd[pfx + '.running_var'] = rn(c, scale=0.3), torch.rand(c, generator=g, dtype=F64) + 0.5
    sd['b.gcn1.PA'], sd['b.gcn1.alpha'] = rn(3, V, V, scale=0.3), rn(1, shift=0.8, scale=0.1)
    for i in range(3):
        conv(f'b.gcn1.convs.{i}.conv1', Rr, Cin); conv(f'b.gcn1.convs.{i}.conv2', Rr, Cin)
        conv(f'b.gcn1.convs.{i}.conv3', Cout, Cin); conv(f'b.gcn1.convs.{i}.conv4', Cout, Rr)
    bn('b.gcn1.bn', Cout)
    if gres == 2:
        conv('b.gcn1.down.0', Cout, Cin); bn('b.gcn1.down.1', Cout)
    conv('b.gcn1.offset_conv.0', Cout, Cout); bn('b.gcn1.offset_conv.1', Cout)
    for b in range(nb + 2):
        conv(f'b.tcn1.branches.{b}.0', Cb, Cout); bn(f'b.tcn1.branches.{b}.1', Cb)
        if b < nb:
            conv(f'b.tcn1.branches.{b}.3.conv', Cb, Cb, ks); bn(f'b.tcn1.branches.{b}.3.bn', Cb)
    bn(f'b.tcn1.branches.{nb}.4', Cb)
    if bres == 2:
        conv('b.residual.conv', Cout, Cin); bn('b.residual.bn', Cout)
    return sd, rn(N, Cin, T, V)


def _affine(sd, pfx):
    s = sd[pfx + '.weight'] / torch.sqrt(sd[pfx + '.running_var'] + O.BN_EPS)
    return s, sd[pfx + '.bias'] - sd[pfx + '.running_mean'] * s


def _fold(sd, conv, bnp):
    s, t = _affine(sd, bnp)
    w = sd[conv + '.weight']
    return w.reshape(w.shape[0], -1) * s[:, None], sd[conv + '.bias'] * s + t


@pytest.mark.parametrize('name', list(GEOMETRIES))
def test_composed_stages_equal_the_oracle_block(name):
    geo = GEOMETRIES[name]
    V, N, T, Cin, Cout, Rr, nb, Cb, ks, dils, stride, gres, bres = geo
    sd, x = _state(geo, seed=11 + len(name))
    if gres == 0:
        # the oracle's tcn_gcn_unit always gives unit_gcn a residual: the zero-residual unit_gcn is composed here from the
        # oracle's own unit_gcn_noresidual and ms_tcn (TCN_GCN_unit: relu(tcn1(gcn1(x)) + residual(x)))
        y = O.ms_tcn(O.unit_gcn_noresidual(x, sd, 'b.gcn1', False), sd, 'b.tcn1', ks, stride, dils, False, 'zero')
        ref = torch.relu(y + (x if bres == 1 else 0))
    else:
        ref = O.tcn_gcn_unit(x, sd, 'b', stride, residual=bres != 0, training=False, kernel_size=ks, dilations=dils)
    cat = torch.cat
    p = dict(N=N, T=T, Cin=Cin, Cout=Cout, R=Rr, res_mode=gres, x=x, xpart=None, A=sd['b.gcn1.PA'], alpha=sd['b.gcn1.alpha'])
    cv = lambda i, k: sd[f'b.gcn1.convs.{i}.{k}.weight'][:, :, 0, 0]
    cb = lambda i, k: sd[f'b.gcn1.convs.{i}.{k}.bias']
    p['w12'] = cat([cat((cv(i, 'conv1'), cv(i, 'conv2'))) for i in range(3)])
    p['b12'] = cat([cat((cb(i, 'conv1'), cb(i, 'conv2'))) for i in range(3)])
    p['w4'], p['b4'] = torch.stack([cv(i, 'conv4') for i in range(3)]), torch.stack([cb(i, 'conv4') for i in range(3)])
    p['w3'], p['b3'] = cat([cv(i, 'conv3') for i in range(3)]), cat([cb(i, 'conv3') for i in range(3)])
    p['sy'], p['ty'] = _affine(sd, 'b.gcn1.bn')
    if gres == 2:
        p['wd'], p['bd'] = _fold(sd, 'b.gcn1.down.0', 'b.gcn1.down.1')
    p['E'] = R.e(p)
    sm, df = R.gcn(p)
    wo, bo = _fold(sd, 'b.gcn1.offset_conv.0', 'b.gcn1.offset_conv.1')
    g = R.gemm(dict(mode=0, relu_rows=0, K=Cout, M=Cout, x=df, add=sm, w=wo, b=bo))
    ent = [_fold(sd, f'b.tcn1.branches.{b}.0', f'b.tcn1.branches.{b}.1') for b in range(nb + 2)]
    h = R.gemm(dict(mode=1, relu_rows=(nb + 1) * Cb, K=Cout, M=Cout, x=g, w=cat([w for w, _ in ent]), b=cat([b for _, b in ent])))
    q = dict(N=N, T=T, Cin=Cin, Cout=Cout, Cb=Cb, nb=nb, ks=ks, dils=dils, stride=stride, res_mode=bres, h=h, x=x)
    tw = [_fold(sd, f'b.tcn1.branches.{b}.3.conv', f'b.tcn1.branches.{b}.3.bn') for b in range(nb)]
    q['wt'], q['bt'] = [w for w, _ in tw], [b for _, b in tw]
    q['sp'], q['tp'] = _affine(sd, f'b.tcn1.branches.{nb}.4')
    if bres == 2:
        q['wr'], q['br'] = _fold(sd, 'b.residual.conv', 'b.residual.bn')
    got = R.tcn(q)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-11 * float(ref.abs().max())


def test_xpart_path_is_the_mean_of_the_tiles():
    """e() on the tile sums of x equals e() on x (1e-13), and on other tile sums it does not: the operand matters."""
    c = R.E_CASES['xpart_t11']
    p = R.sub('e', R.problem('e', c, 20, 3), 0)
    own = dict(p, xpart=R.tile_sums(p['x']).float())
    a, b = R.e(dict(p, xpart=None)), R.e(own)
    assert float((a - b).abs().max()) <= 1e-6 * float(a.abs().max())          # (the float32 tile sums)
    assert float((a - R.e(p)).abs().max()) > 1e-2 * float(a.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# the mirrored constants against the source text
# ---------------------------------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, name):
    m = re.search(r'\b' + name + r'\s*=\s*([0-9]+)\b', text)
    assert m, name
    return int(m.group(1))


def _defined_once(name, home, others):
    """the value of a constant that f2_common.h (or another one file) defines and no other source of the family does"""
    for text in others:
        assert not re.search(r'\b' + name + r'\s*=[^=]', text), f'{name} is defined a second time'
    return _const(home, name)


def test_mirrored_constants_match_the_kernels():
    f2, fv, fg, cm, body = (_src(n) for n in ('f2.hip', 'f2v.hip', 'f2g.hip', 'f2_common.h', 'f2x_body.h'))
    rest = (f2, fv, fg, body)
    assert _defined_once('F2_BT', cm, rest) == R.BT
    assert _defined_once('F2_HF', cm, rest) == R.HF
    assert _defined_once('F2_PX', cm, rest) == R.PX
    assert _defined_once('F2_KC', cm, rest) == R.KC
    for text in rest + (cm,):                                      # the per-family copies of those constants are gone
        assert not re.search(r'\bF[VG]_(NT|BT|G|KC|HF|PX|CT|LDS_MAX)\b', text)
    assert _defined_once('F2_V', f2, (fv, fg, cm, body)) == R.FAMILIES['f2']
    assert _defined_once('FV_V', fv, (f2, fg, cm, body)) == R.FAMILIES['f2v']
    assert 'VP = (V + 3) & ~3' in fv and R.vp(25) == R.VP25 == 28 and R.vp(20) == 20
    assert 'F2_LDS_MAX = 160 * 1024' in cm and R.LDS_MAX == 160 * 1024
    for text in (f2, fv, fg):                                      # one cap, by its name, in front of every launch that can pass it
        assert 'lds <= F2_LDS_MAX' in text and '160 * 1024' not in text
    assert '160 * 1024' not in body
    # the halo guard and the formula that switches f2v_e between 4 and 2 frame phases, as f2_ref restates them: one copy each
    assert '(F2_BT - 1) * d->stride + (d->ks - 1) * d->dil[b] + 1 <= F2_HF' in cm
    for text in rest:
        assert 'd->dil[b] + 1 <=' not in text and 'R2p = 2 * R' not in text
    for frag in ('EC = V * VP', 'ECT = (EC + 15) / 16', 'PD = ECT * 16 + 4',
                 'static constexpr size_t fv_e_lds(int Cin, int R, int ntp) { return f2_e_lds(Cin, R, ntp, GV::VP, GV::PD); }',
                 'a.ntp = fv_e_lds(a.Cin, a.R, 4) <= F2_LDS_MAX ? 4 : 2;'):
        assert frag in fv, frag
    for frag in ('constexpr size_t f2_e_lds(int Cin, int R, int ntp, int VP, int PD) {',
                 'const int Kp = (Cin + 15) & ~15, R2p = 2 * R < 16 ? 16 : 2 * R, Rp = (R + 15) & ~15;',
                 'const size_t d = (size_t)Rp * PD, xp = (size_t)ntp * Kp * VP;',
                 'return sizeof(float) * ((size_t)Kp * F2_PX + (size_t)R2p * F2_PX + 64 * F2_PX + (d > xp ? d : xp));'):
        assert frag in cm, frag
    # the p/q product: row tiles rounded UP (2R = 24 needs two, 40 three, 56 four), K parts = 4 / row tiles -- in f2's body and
    # in the one body f2v and f2g share
    for text in (f2, body):
        assert 'nrt = (R2p + 15) / 16, nparts = 4 / nrt' in text
    for text in (fv, fg, cm):
        assert 'nparts' not in text


def test_f2v_e_phase_switch_sides():
    assert R.fv_e_lds(256, 8, 4) <= R.LDS_MAX < R.fv_e_lds(256, 16, 4)
    assert R.e_phases(256, 8, 'f2v') == 4 and R.e_phases(256, 16, 'f2v') == 2
    assert R.fv_e_lds(256, 32, 2) <= R.LDS_MAX
    assert all(R.e_phases(c['Cin'], c['R'], 'f2') == 4 for c in R.E_CASES.values())


# ---------------------------------------------------------------------------------------------------------------------
# the table reaches every listed path; every case is one the host accepts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fam', list(R.FAMILIES))
def test_table_reaches_every_path(fam):
    req = R.required_paths(fam)
    for stage, cases in R.STAGES.items():
        got = set()
        for c in cases.values():
            got |= R.paths(stage, c, fam)
        assert not req[stage] - got, (stage, sorted(req[stage] - got))
        n_grouped = sum(c['G'] > 1 for c in cases.values())
        assert n_grouped * 7 >= 2 * len(cases), (stage, n_grouped, len(cases))    # groups on about a third of every stage
        assert {c['G'] for c in cases.values()} >= {1, 2, 3}


def test_table_values_of_the_issue():
    E, Gc, M, Tc = (R.STAGES[k].values() for k in ('e', 'gcn', 'gemm', 'tcn'))
    assert {c['Cin'] for c in E} >= {3, 16, 40, 64, 256} and {c['R'] for c in E} >= {1, 4, 8, 12, 16, 20, 24, 32}
    assert {c['Cout'] for c in E} == {16, 48} and {c['T'] for c in E if c['src'] == 'x'} >= {1, 3, 4, 5, 33}
    assert {c['T'] for c in E if c['src'] == 'xpart'} >= set(range(1, 5)) | set(range(9, 13)) | set(range(17, 21)) | set(range(33, 37))
    assert {c['Cin'] for c in Gc} >= {3, 16, 40, 64, 128, 144, 200, 256} and {c['T'] for c in Gc} >= {1, 3, 4, 5, 9}
    for mode in (0, 1, 2):
        assert len({c['Cin'] for c in Gc if c['res_mode'] == mode}) > 1
    assert {c['K'] for c in M} == {16, 40, 48, 256} and {c['M'] for c in M} == {16, 48}
    assert {c['relu_rows'] for c in M if c['mode'] == 1} >= {0, 8, 24, 16, 48}
    assert {c['nb'] for c in Tc} == {1, 2, 3, 4} and {c['Cb'] for c in Tc} == {16, 32, 48, 64}
    assert {c['T'] for c in Tc if c['stride'] == 2} >= {1, 2, 3, 8, 9} and {c['T'] for c in Tc if c['stride'] == 1} >= {1, 5}
    for c in Tc:
        assert c['Cout'] == (c['nb'] + 2) * c['Cb'] and len(c['dils']) == c['nb'] and c['ks'] % 2 == 1
        assert all(R.halo(c['ks'], d, c['stride']) <= R.HF for d in c['dils'])
        assert c['res_mode'] != 1 or (c['Cin'] == c['Cout'] and c['stride'] == 1)
    for s, pairs in R.AT_LIMIT.items():
        for ks, d in pairs:
            assert R.halo(ks, d, s) <= R.HF < R.halo(ks, d + 1, s)
    for c in list(E) + list(Gc):
        assert c['res_mode'] != 1 or c['Cin'] == c['Cout']
    for cases in R.STAGES.values():
        for c in cases.values():
            assert c['N'] % c['G'] == 0 and c['N'] <= 4 and (c['T'] <= 9 or c in E)


# ---------------------------------------------------------------------------------------------------------------------
# the bars: a correct fp32 evaluation passes every one of them; planted defects fail
# ---------------------------------------------------------------------------------------------------------------------
F32 = torch.float32


def _fp32(stage, p):
    if stage == 'e':
        return R.check_e('fp32', p, R.e(p, F32))
    if stage == 'gcn':
        return R.check_gcn('fp32', p, *R.gcn(p, F32), p['V'])
    if stage == 'gemm':
        return R.check_gemm('fp32', p, R.gemm(p, F32))
    out = R.tcn(p, F32)
    return R.check_tcn('fp32', p, out, R.tile_sums(out, F32))


@pytest.mark.parametrize('stage', list(R.STAGES))
def test_fp32_evaluation_passes_every_bar(stage):
    """torch's float32 evaluation of the same expressions (another summation order, an accurate tanh) is inside every bar of
    every case of the table: the derivations hold for correct arithmetic."""
    for i, (cid, c) in enumerate(R.STAGES[stage].items()):
        V = (20, 25)[i % 2]
        p = R.problem(stage, c, V, seed=100 + i)
        for g in range(c['G']):
            _fp32(stage, R.sub(stage, p, g))


def test_planted_defects_fail_the_bars():
    # a dropped tap
    c = R.TCN_CASES['nb2_cb16_k3_s1_res1_t5']
    p = R.sub('tcn', R.problem('tcn', c, 20, 1), 0)
    good = R.tcn(p, F32)
    R.check_tcn('good', p, good, None)
    w = p['wt'][0].clone().view(c['Cb'], c['Cb'], c['ks'])
    w[:, 3, 2] = 0                                                # one input channel's last tap of the dilation-1 branch
    with pytest.raises(B.BarError, match='temporal'):
        R.check_tcn('tap', p, R.tcn(dict(p, wt=[w.view(c['Cb'], -1), p['wt'][1]]), F32), None)
    # the pooled maximum over zero padding instead of the frames that exist
    lo, hi = c['nb'] * c['Cb'], (c['nb'] + 1) * c['Cb']
    bad = good.clone()
    T2 = good.shape[2]
    hz = torch.cat((torch.zeros_like(p['h'][:, lo:hi, :1]), p['h'][:, lo:hi], torch.zeros_like(p['h'][:, lo:hi, :1])), 2)
    m = torch.stack([hz[:, :, t:t + 3].amax(2) for t in range(0, T2 * c['stride'], c['stride'])], 2)
    bad[:, lo:hi] = torch.relu(p['sp'][None, :, None, None] * m + p['tp'][None, :, None, None] + p['x'][:, lo:hi])
    assert torch.equal(bad[:, lo:hi, 1:-1], good[:, lo:hi, 1:-1])  # only the clip ends differ
    with pytest.raises(B.BarError, match='pooled'):
        R.check_tcn('pool0', p, bad, None)
    # the p/q row tiles rounded down: q rows 16.. of 2R = 24 never multiplied (here: left at their bias)
    c = R.E_CASES['cin40_r12_t4']
    p = R.sub('e', R.problem('e', c, 25, 2), 0)
    R.check_e('good', p, R.e(p, F32))
    w12 = p['w12'].clone().view(3, 24, -1)
    w12[:, 16:] = 0
    with pytest.raises(B.BarError):
        R.check_e('nrt', p, R.e(dict(p, w12=w12.view(72, -1)), F32))
