"""Host only: the restatement of the data-gradient / InstanceNorm-backward dispatch in tests/test_gpu_dgrad_layers.py
(`expected_in_bwd_route`, `expected_bwd_data_variant`, `expected_stride1`) -- what the launch-probe assertions of that file
rest on -- against a hand-written table of what every case must launch in a default process and under each backward
switch.  Needs neither a GPU nor the library."""
from tests import test_gpu_conv2d_layers as conv2d
from tests import test_gpu_dgrad_layers as layers
from tests.test_gpu_dgrad_layers import (CHANNEL_SUM, DATA1, DATA2, FLIP, GRAD_ADD, GRAD_REDUCE_D, IN_PLANE, IN_TWOPASS,
                                         KS16, PROBES, T8X)
from tests.test_gpu_switches import BACKWARD_SWITCHES

X3B, X3F, DIRECT = conv2d.X3B, conv2d.X3F, conv2d.DIRECT
C84, C81, C44, C42 = ('bwd_data2<conv,cb8,ocg4>', 'bwd_data2<conv,cb8,ocg1>', 'bwd_data2<conv,cb4,ocg4>',
                      'bwd_data2<conv,cb4,ocg2>')
D4V0, D4V1, D3V1 = ('bwd_data2<deconv4,cb4,ocg2,vec0>', 'bwd_data2<deconv4,cb4,ocg2,vec1>',
                    'bwd_data2<deconv3,cb4,ocg1,vec1>')

# launches per probe name in a default process, derived by hand from the launchers' constants (names not listed: none),
# and, for bwd_data2 and channel_sum, the workgroups of that launch
DEFAULT = {
    # pairs 36: pw 64, ry 1, 31 row blocks per parity: 2 * 16 * 2 * 31 = 1984 units of 8 channels; x 4 waves / 4 per workgroup
    's2_8_16_n2_16x62x72': ({IN_PLANE: 1, C84: 1, GRAD_ADD: 1}, {C84: 1984}),
    # pairs 65: two segments, 32 row blocks: 2 * 16 * 2 * 32 * 2 = 4096 units: ocg 1, 1024 workgroups
    's2_8_16_n2_16x64x130': ({IN_PLANE: 1, C81: 1, GRAD_ADD: 1}, {C81: 1024}),
    # 7 * 2 * 5 = 70 units per channel block < 512: cb 4, two blocks, 140 units x ocg 4
    's2_8_16_n1_7x9x65': ({IN_PLANE: 1, C44: 1, GRAD_ADD: 1}, {C44: 140}),
    # pairs 8: pw 8, 8 rows per wave, one row block: 2 * 9 * 2 = 36 units x ocg 2 (Cout 8 < 16) = 72 waves
    's2_4_8_n2_9x11x15': ({IN_PLANE: 1, C42: 1, GRAD_ADD: 1}, {C42: 18}),
    # pairs 11: pw 16, 4 rows per wave, 4 rows per parity: 2 * 5 * 2 = 20 units x 2
    's2_4_8_n2_5x7x21': ({IN_PLANE: 1, C42: 1, GRAD_ADD: 1}, {C42: 10}),
    # pairs 18: pw 32, 2 rows per wave, 3 rows per parity: 2 blocks: 2 * 5 * 2 * 2 = 40 units x 2; output 3 x 3 x 18 = 162
    # elements per group, not a multiple of 4: two-pass
    's2_4_8_n2_5x6x35': ({IN_TWOPASS: 1, C42: 1, GRAD_ADD: 1}, {C42: 20}),
    # 6 channels: two blocks of 4; pairs 7: pw 8: 2 * 5 * 2 * 1 = 20 per block, 40 units x 2
    's2_6_8_n2_5x7x13': ({IN_PLANE: 1, C42: 1, GRAD_ADD: 1}, {C42: 20}),
    's2_4_8_n2_5x7x21_2src': ({IN_PLANE: 1, C42: 1, GRAD_ADD: 2}, {C42: 10}),
    # pairs 17: pw 32, 2 rows per wave, 2 row blocks: 2 * 3 * 2 = 12 per block; 12 * 2 < 512: cb 4, 48 units x ocg 2
    'd4_16_8_n2_3x4x33': ({IN_PLANE: 1, D4V0: 1, GRAD_ADD: 1}, {D4V0: 24}),
    'd4_16_8_n2_3x4x34': ({IN_PLANE: 1, D4V1: 1, GRAD_ADD: 1}, {D4V1: 24}),
    # bare: dz is the caller's misaligned view; channel_sum over 6 * 8 * 68 = 3264 positions: one split, 8 channels
    'd4_16_8_n2_3x4x34_bare_offset': ({CHANNEL_SUM: 1, D4V0: 1, GRAD_ADD: 1}, {D4V0: 24, CHANNEL_SUM: 8}),
    # pairs 9: pw 16, 4 rows per wave, 2 row blocks: 2 * 4 * 2 = 16 units, Cout 1 < 8: ocg 1: 4 workgroups
    'd3_4_1_n2_4x5x18_bare': ({CHANNEL_SUM: 1, D3V1: 1, GRAD_ADD: 1}, {D3V1: 4, CHANNEL_SUM: 1}),
    # plane 165, not a multiple of 4: two-pass; odd width: 2 entries x 2 blocks, no certificate
    'c1_128_64_n2_1x5x33': ({IN_TWOPASS: 1, FLIP: 1, X3B: 4, GRAD_ADD: 1}, {}),
    'c1_128_64_n2_1x5x36': ({IN_PLANE: 1, FLIP: 1, X3F: 2, GRAD_ADD: 1}, {}),
    'c1_64_64_n2_2x5x36': ({IN_PLANE: 1, FLIP: 1, X3F: 1, GRAD_ADD: 1}, {}),
    'c1_64_64_n2_2x6x36_heavy': ({IN_PLANE: 1, FLIP: 1, X3F: 1, GRAD_ADD: 1}, {}),
    'c1_64_64_n2_2x6x36_heavy_bare': ({CHANNEL_SUM: 1, FLIP: 1, X3F: 1, GRAD_ADD: 1}, {CHANNEL_SUM: 64}),
    'c3_8_8_n2_3x6x34': ({IN_PLANE: 1, FLIP: 1, T8X: 1, GRAD_ADD: 1}, {}),
    'c3_16_16_n2_3x5x20': ({IN_PLANE: 1, FLIP: 1, KS16: 1, GRAD_ADD: 1}, {}),
    'c3_16_16_n2_3x5x20_2src': ({IN_PLANE: 1, FLIP: 1, KS16: 1, GRAD_ADD: 2}, {}),
    'c3_8_8_n2_3x5x7': ({IN_TWOPASS: 1, FLIP: 1, T8X: 1, GRAD_ADD: 1}, {}),
    'c3_8_8_n2_5x80x96': ({IN_TWOPASS: 1, FLIP: 1, T8X: 1, GRAD_ADD: 1}, {}),
    # dz has 3 channels: no MFMA tiling (Cin % 4 != 0)
    'c1_3_3_n2_1x128x516_pp': ({IN_TWOPASS: 1, FLIP: 1, DIRECT: 1, GRAD_ADD: 1}, {}),
    'c1_8_3_n2_2x6x8_pp_offset': ({IN_TWOPASS: 1, FLIP: 1, DIRECT: 1, GRAD_ADD: 1}, {}),
    # 9216 positions: two splits x 3 channels
    'c1_8_3_n2_1x96x96_bare': ({CHANNEL_SUM: 1, FLIP: 1, DIRECT: 1, GRAD_ADD: 1}, {CHANNEL_SUM: 6}),
}
# under PDS_BWD_DATA_V2=0: 4 input channels per thread, 256 positions of a plane per workgroup
V1 = {
    's2_8_16_n2_16x62x72': ('bwd_data1<conv,k3,s2>', 18 * 16 * 2 * 2),
    's2_8_16_n2_16x64x130': ('bwd_data1<conv,k3,s2>', 33 * 16 * 2 * 2),
    's2_8_16_n1_7x9x65': ('bwd_data1<conv,k3,s2>', 3 * 7 * 1 * 2),
    's2_4_8_n2_9x11x15': ('bwd_data1<conv,k3,s2>', 1 * 9 * 2 * 1),
    's2_4_8_n2_5x7x21': ('bwd_data1<conv,k3,s2>', 1 * 5 * 2 * 1),
    's2_4_8_n2_5x6x35': ('bwd_data1<conv,k3,s2>', 1 * 5 * 2 * 1),
    's2_6_8_n2_5x7x13': ('bwd_data1<conv,k3,s2>', 1 * 5 * 2 * 2),
    's2_4_8_n2_5x7x21_2src': ('bwd_data1<conv,k3,s2>', 1 * 5 * 2 * 1),
    'd4_16_8_n2_3x4x33': ('bwd_data1<deconv,k4>', 1 * 3 * 2 * 4),
    'd4_16_8_n2_3x4x34': ('bwd_data1<deconv,k4>', 1 * 3 * 2 * 4),
    'd4_16_8_n2_3x4x34_bare_offset': ('bwd_data1<deconv,k4>', 1 * 3 * 2 * 4),
    'd3_4_1_n2_4x5x18_bare': ('bwd_data1<deconv,k3>', 1 * 4 * 2 * 1),
}


def shown(case, switches):
    counts, workgroups = layers.expected_counts(case, switches)
    return {k: v for k, v in counts.items() if v}, workgroups


def test_names_do_not_contain_each_other():
    assert len(set(PROBES)) == len(PROBES)
    for a in PROBES:
        for b in PROBES:
            assert a == b or a not in b, (a, b)
    # ... nor do the names the library gives the two exact / split 8 -> 8 kernels confuse the two probes
    assert 'conv3d_t8<' in 'conv3d_t8<guarded>' and 'conv3d_t8<' not in 'conv3d_t8x<guarded>'
    assert 'conv3d_t8x' in 'conv3d_t8x<exact>' and 'conv3d_t8x' not in 'conv3d_t8<exact>'


def test_default_process_matches_the_hand_written_table():
    ids = [c['id'] for c in layers.CASES]
    assert len(set(ids)) == len(ids) and set(ids) == set(DEFAULT)
    for c in layers.CASES:
        assert shown(c, {}) == DEFAULT[c['id']], c['id']
    reached = set().union(*(d[0] for d in DEFAULT.values()))
    assert {IN_PLANE, IN_TWOPASS, CHANNEL_SUM, FLIP, GRAD_ADD, C84, C81, C44, C42, D4V0, D4V1, D3V1} <= reached
    # (docstring of the GPU file: why these are not reached in a default process)
    assert not reached & (set(DATA1) | {GRAD_REDUCE_D})
    assert not {n for n in DATA2 if 'deconv' in n and 'cb8' in n} & reached


def test_the_intermediate_values_of_the_variant():
    by_id = {c['id']: c for c in layers.CASES}
    v = layers.expected_bwd_data_variant(by_id['s2_8_16_n2_16x64x130'], {})
    assert (v['pw'], v['ry'], v['segs'], v['yblocks'], v['cb'], v['ocg'], v['units']) == (64, 1, 2, 32, 8, 1, 4096)
    v = layers.expected_bwd_data_variant(by_id['s2_8_16_n1_7x9x65'], {})
    assert (v['pw'], v['ry'], v['segs'], v['yblocks'], v['cb'], v['ocg'], v['units']) == (64, 1, 1, 5, 4, 4, 140)
    assert [layers.expected_bwd_data_variant(by_id[k], {})['ry'] for k in
            ('s2_4_8_n2_9x11x15', 's2_4_8_n2_5x7x21', 's2_4_8_n2_5x6x35', 's2_8_16_n2_16x62x72')] == [8, 4, 2, 1]
    v = layers.expected_bwd_data_variant(by_id['d4_16_8_n2_3x4x33'], {})
    assert (v['pw'], v['ry'], v['yblocks'], v['cb'], v['ocg'], v['units'], v['vec']) == (32, 2, 2, 4, 2, 48, False)
    assert layers.expected_bwd_data_variant(by_id['d4_16_8_n2_3x4x34'], {}, aligned=False)['vec'] is False


def test_in_bwd_routes_and_tiles():
    by_id = {c['id']: c for c in layers.CASES}
    assert layers.expected_in_bwd_route(by_id['c1_3_3_n2_1x128x516_pp'], {}) == (IN_TWOPASS, 64)    # ceil(66048 / 1024) = 65
    assert layers.expected_in_bwd_route(by_id['c3_8_8_n2_5x80x96'], {}) == (IN_TWOPASS, 8)          # 38400 > 36864
    assert layers.expected_in_bwd_route(by_id['c3_8_8_n2_3x6x34'], {})[0] == IN_PLANE               # 612 = 4 * 153
    assert layers.expected_in_bwd_route(by_id['c3_8_8_n2_3x5x7'], {})[0] == IN_TWOPASS              # 105
    aligned = dict(by_id['c1_8_3_n2_2x6x8_pp_offset'], offset=False)
    assert layers.expected_counts(aligned, {})[0][IN_PLANE] == 1
    assert all(c['n'] == 2 and c['cout'] >= 3 for c in layers.CASES if c['norm'] and c['id'] != 's2_8_16_n1_7x9x65')


def test_backward_switches():
    for switches in BACKWARD_SWITCHES:
        for c in layers.CASES:
            counts, workgroups = DEFAULT[c['id']]
            counts, workgroups = dict(counts), dict(workgroups)
            if switches.get('PDS_IN_BWD_PLANE') == '0' and IN_PLANE in counts:
                counts[IN_TWOPASS] = counts.pop(IN_PLANE)
            if switches.get('PDS_BWD_DATA_V2') == '0' and c['id'] in V1:
                old = [k for k in counts if k.startswith('bwd_data2')][0]
                del counts[old], workgroups[old]
                counts[V1[c['id']][0]] = 1
                workgroups[V1[c['id']][0]] = V1[c['id']][1]
            assert shown(c, switches) == (counts, workgroups), (c['id'], switches)
    assert {'PDS_BWD_DATA_V2': '0'} in BACKWARD_SWITCHES and {'PDS_IN_BWD_PLANE': '0'} in BACKWARD_SWITCHES
