"""Case table of the V = 17 (COCO) fixture, shared by make_golden_vgen.py (reference side) and
tests/test_oracle_vs_golden_vgen.py (oracle side).  Pure data: (tag, kind, ctor kwargs, x shape (N, C, T, V), x seed)."""

VGEN_MODULE_CASES = [
    ('vgen_ctrgc_64_64',     'CTRGC',        dict(in_channels=64, out_channels=64),                           (2, 64, 13, 17), 11),
    ('vgen_gcn_3_64',        'unit_gcn',     dict(in_channels=3, out_channels=64),                            (2, 3, 13, 17),  12),
    ('vgen_unit_64_128_s2',  'TCN_GCN_unit', dict(in_channels=64, out_channels=128, stride=2, residual=True), (2, 64, 13, 17), 16),
]
