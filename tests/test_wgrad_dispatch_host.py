"""Host only: `expected_wgrad_kernel` of tests/test_gpu_wgrad_layers.py -- the restatement of the weight-gradient cascade
of backward_walk (csrc/api_training.hip) the launch-probe assertions of that file rest on -- against a hand-written table
of what every case of the file must launch in a default process and under the backward switches.  Needs neither a GPU nor
the library."""
from tests import test_gpu_wgrad_layers as layers
from tests.test_gpu_wgrad_layers import (FAMILIES, MB1, MB1_2, MB4, MB4_2, MB4_P, PAIR, PAIR_2, PROBES, REDUCE32, REDUCE64,
                                         S2C, S2D, S2RC, S2RD, TAP, TAP_2, UPFULL, VALU_C, VALU_D, X3)

# launches per family in a default process, derived by hand from the layer lists and the predicates (families not named:
# none); the 2-D modules list their layers first to last
DEFAULT = {
    # 128 -> 64 | 64 -> 64 (plain x0) | 64 -> 64 (width 33: w & 3) | two-source 64 -> 8
    'op_128_64_8_b1_n2_5x33': {MB4: 3, MB1_2: 1},
    # 128 -> 64 and the first 64 -> 64 (x0 carries no certificate) exact; three certified 64 -> 64 and the last layer split
    'op_128_64_8_b2_n3_5x36': {MB4: 2, X3: 4},
    'op_128_64_5_b2_n3_3x68': {MB4: 2, X3: 4},
    'op_128_64_8_b0_n2_4x31': {MB4: 1, MB1: 1},
    # one residual block: only its second convolution has certified operands (the last layer's second source is x0)
    'op_128_64_8_b1_n3_3x32': {MB4: 2, X3: 1, MB1_2: 1},
    'op_128_64_8_b1_n2_3x64': {MB4: 2, X3: 1, MB1_2: 1},
    'op_32_16_6_b1_n3_5x33': {MB1: 3, MB1_2: 1},
    # 64 -> 32 and 32 -> 32: Cout 32 is neither 64 nor <= 16; 32 -> 8 is
    'op_64_32_8_b1_n2_5x36': {VALU_C: 3, MB1_2: 1},
    # native route: x0 is certified, but width 13 keeps the exact kernels; layer 0 = three single-plane launches
    'matching_64_b1_n2_4x13_shard2+4': {MB4: 5, MB1_2: 1},
    'matching_64_b1_n2_3x36': {X3: 3, MB4: 3},
    # 12 -> 64 partial group | 256 -> 64, two 64 -> 64, 64 -> 8 on quarter width 36: split
    'embedding_b1_n2_20x144': {MB4_P: 1, X3: 4},
    # quarter width 33: exact
    'embedding_b1_n3_12x130': {MB4_P: 1, MB4: 3, MB1: 1},
    'contraction_4_n2_9x11x65': {S2C: 1, PAIR: 1},
    'contraction_8_n2_17x12x70': {S2C: 1, TAP: 1},
    'contraction_16_n1_7x9x65': {S2C: 1, TAP: 1},
    'contraction_32_n2_17x11x66': {S2C: 1, TAP: 1},
    'contraction_8_n2_16x62x72': {S2RC: 1, TAP: 1},
    'contraction_8_n2_16x62x70': {S2C: 1, TAP: 1},
    'expansion_12_n2_5x3x17': {S2D: 1, PAIR_2: 1},
    'expansion_16_n2_3x4x33': {S2D: 1, PAIR_2: 1},
    'expansion_32_n2_3x4x33': {S2D: 1, TAP_2: 1},
    'expansion_8_n2_8x31x36': {S2RD: 1, PAIR_2: 1},
    # smoothing <pair>; four stride-2 convolutions; their smoothing layers <tap>; four k4 transposed layers + the half-size
    # one; smoothing behind the skip sums at 64, 32, 16 channels <tap,2src> and at 8 <pair,2src>; the full-size layer
    'regularization_8_n1_16x16x32': {PAIR: 1, S2C: 4, TAP: 4, S2D: 5, TAP_2: 3, PAIR_2: 1, UPFULL: 1},
}


def counts(case, switches):
    return {k: v for k, v in layers.expected_counts(layers.case_layers(case), switches).items() if v}


def with_reductions(families):
    out = dict(families)
    valu = sum(v for k, v in families.items() if k in (VALU_C, VALU_D))
    mfma = sum(families.values()) - valu
    if mfma:
        out[REDUCE32] = mfma
    if valu:
        out[REDUCE64] = valu
    return out


def test_names_do_not_contain_each_other():
    for a in PROBES:
        for b in PROBES:
            assert a == b or a not in b, (a, b)


def test_default_process_matches_the_hand_written_table():
    ids = [layers.case_id(c) for c in layers.CASES]
    assert len(set(ids)) == len(ids) and set(ids) == set(DEFAULT)
    for case in layers.CASES:
        assert counts(case, {}) == with_reductions(DEFAULT[layers.case_id(case)]), layers.case_id(case)
    reached = set().union(*DEFAULT.values())
    assert reached == set(FAMILIES) - {MB4_2, VALU_D}     # (docstring of the GPU file: why these two are not)


def test_every_parameter_belongs_to_one_layer():
    for case in layers.CASES:
        module, lst = layers.make_module(case), layers.case_layers(case)
        prefixes = [L['prefix'] for L in lst]
        assert len(set(prefixes)) == len(prefixes)
        seen = {layers.layer_of(name, lst)['prefix'] for name, _ in module.named_parameters()}
        assert seen == set(prefixes), layers.case_id(case)


def test_table_reaches_the_edges_it_names():
    ops = [c[1] for c in layers.CASES if c[0] == 'op']
    assert {31, 32, 33, 36, 64, 68} <= {a[5] for a in ops}
    assert all(2 <= a[3] <= 3 and 3 <= a[4] <= 5 for a in ops)
    # rolling kernel: exactly 512 units by default, a partial R_TY block, widths % 4 == 0 on both grids; the neighbour not
    for kind, a in layers.CASES:
        name = layers.case_id((kind, a))
        if S2RC in DEFAULT[name] or S2RD in DEFAULT[name]:
            small = a[2:] if kind == 'expansion' else tuple((v + 1) // 2 for v in a[2:])
            assert a[1] * small[0] * -(-small[1] // 2) * -(-small[2] // 32) == 512
            assert small[1] % 2 == 1 and small[2] % 4 == 0 and (2 * small[2]) % 4 == 0
    assert sum(1 for v in DEFAULT.values() if S2RC in v or S2RD in v) == 2
    # wgrad3d_mfma: h = 6, w = 33 and 35, d = 5 and 9, batch 2
    smooth = [layers.case_layers(c)[1] for c in layers.CASES if c[0] == 'contraction']
    assert {(5, 6, 33), (9, 6, 35), (9, 6, 33)} <= {(L['d'], L['h'], L['w']) for L in smooth}


def test_wgrad2d_x3_off_keeps_the_exact_kernels():
    switches = {'PDS_WGRAD2D_X3': '0'}
    assert counts(layers.CASES[1], switches) == with_reductions({MB4: 5, MB1_2: 1})           # op_128_64_8_b2_n3_5x36
    assert counts(layers.CASES[9], switches) == with_reductions({MB4: 5, MB1_2: 1})           # matching_64_b1_n2_3x36
    assert counts(layers.CASES[10], switches) == with_reductions({MB4_P: 1, MB4: 3, MB1: 1})  # embedding_b1_n2_20x144
    for case in layers.CASES:
        if X3 not in DEFAULT[layers.case_id(case)]:
            assert counts(case, switches) == with_reductions(DEFAULT[layers.case_id(case)])


def test_rolling_switches():
    never, always = {'PDS_WGRAD3D_S2_ROLLING': '0'}, {'PDS_WGRAD3D_S2_ROLLING': '2'}
    for case in layers.CASES:
        want = dict(DEFAULT[layers.case_id(case)])
        for rolling, plain in ((S2RC, S2C), (S2RD, S2D)):
            if rolling in want:
                want[plain] = want.get(plain, 0) + want.pop(rolling)
        assert counts(case, never) == with_reductions(want), layers.case_id(case)
    # =2: every layer of the right shape, however small.  Of the small cases only the hourglass has such layers: its
    # first stride-2 convolution (8 -> 16, widths 32 / 16, two sources), the last expansion's 16 -> 8 and the 8 -> 4
    # half-size layer.  Everywhere else a width is not a multiple of 4, or the big grid has 6, 16 or more channels.
    census = dict(DEFAULT['regularization_8_n1_16x16x32'])
    census.update({S2C: 3, S2RC: 1, S2D: 3, S2RD: 2})
    for case in layers.CASES:
        name = layers.case_id(case)
        want = census if name.startswith('regularization') else DEFAULT[name]
        assert counts(case, always) == with_reductions(want), name


def test_valu_switches():
    switches = {'PDS_WGRAD3D_MFMA': '0', 'PDS_WGRAD3D_S2_MFMA': '0'}
    for case in layers.CASES:
        name, want = layers.case_id(case), None
        if case[0] == 'contraction':
            want = {VALU_C: 2}
        elif case[0] == 'expansion':
            want = {VALU_D: 1, VALU_C: 1}
        elif case[0] == 'regularization':
            want = {VALU_C: 13, VALU_D: 6}      # 1 + 4 x 2 + 4 convolutions; 4 + 2 transposed ones
        else:
            want = DEFAULT[name]                # the 2-D layers do not look at these switches
        assert counts(case, switches) == with_reductions(want), name
    # one switch alone
    only3d = counts(layers.CASES[12], {'PDS_WGRAD3D_MFMA': '0'})                               # contraction_4_n2_9x11x65
    assert only3d == with_reductions({S2C: 1, VALU_C: 1})
    only_s2 = counts(layers.CASES[22], {'PDS_WGRAD3D_S2_MFMA': '0'})                           # the census
    assert only_s2 == with_reductions({PAIR: 1, VALU_C: 4, TAP: 4, VALU_D: 6, TAP_2: 3, PAIR_2: 1})
