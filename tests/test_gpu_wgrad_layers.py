"""GPU (-m gpu): every weight-gradient kernel of the backward pass alone, one parameter tensor at a time, against fp64.

No entry point runs the backward of a single layer, so a "layer" here is one parameter tensor of the smallest module
that contains it: ContractionBlock3d / ExpansionBlock3d through pds_contraction_block_fwd/_bwd and
pds_expansion_block_fwd/_bwd called directly (the test owns every buffer), pds.MatchingOperation, the native training
route of pds.Matching, pds.Embedding and pds.Regularization through autograd.

Every case
  1. counts the launches of all weight-gradient families with the launch probe, one run per name, and asserts that
     every family recorded exactly what `expected_wgrad_kernel` predicts for the layers of the module -- the predicted
     families their launches, every other family none -- and that exactly one reduction followed each launch;
  2. (C entry points) pre-fills the gradient buffers and the backward workspace with NaN bytes; every gradient is finite
     afterwards and pds_nonfinite_statistics does not move;
  3. compares every parameter gradient (weights, and the bias / gamma / beta gradients that come with the same call)
     with CPU fp64 autograd through oracle/pds_oracle.py: err = max|g - g64| / max|g64| <= max(F, 3 * e32), e32 = the
     same distance of the CPU fp32 autograd of the case, computed here at run time.  Weight tensors served by
     wgrad2d_x3 also meet the mean-relative form, mean|g - g64| / mean|g64| <= max(F_MEAN, 3 x the CPU fp32 mean);
  4. holds the input gradients to the REL_TOL of tests/test_gpu_backward.py (they are not this file's subject).

Dispatch (csrc/api_training.hip backward_walk, in this order; `expected_wgrad_kernel` restates it):
  wgrad2d_mfma_supported   kernel depth 1, stride 1, Cout == 64 or <= 16, Cin <= 64 or Cin % 64 == 0.  Inside
                           launch_wgrad2d_mfma: wgrad2d_x3 when input(s) and dz carry range certificates, Cin % 64 == 0
                           and W % 4 == 0 (wgrad2d_x3_supported; PDS_WGRAD2D_X3=0 turns it off), else the exact kernel:
                           <mb4,partial> (Cout 64, Cin < 64, one source), <mb4> / <mb4,2src> (Cout 64), <mb1> /
                           <mb1,2src> (Cout <= 16);
  wgrad3d_mfma_supported   convolution, kernel depth 3, stride 1 (PDS_WGRAD3D_MFMA=0: off): <pair> for Cin <= 8, else
                           <tap>, ",2src" with a second source.  Channel counts play no part;
  wgrad_up_full_mfma       the transposed 3 x 4 x 4 layer, Cin <= 4 -> 1 (PDS_WGRAD3D_S2_MFMA=0: off);
  wgrad3d_s2_mfma          stride-2 convolutions and k4 transposed convolutions (PDS_WGRAD3D_S2_MFMA=0: off); inside its
                           launcher wgrad3d_s2r takes the layers whose big grid has 4 or 8 channels and whose small grid
                           at most 16, both widths % 4 == 0, no second source on a transposed layer, from
                           n * d * ceil(h / R_TY) * ceil(w / R_TWG) >= 512 small-grid units (R_TY = 2, R_TWG = 32;
                           PDS_WGRAD3D_S2_ROLLING=0: never, =2: however small);
  bwd_weight<conv|deconv>  everything else (VALU, fp64 partials, weight_reduce).

Shapes (from the constants of the kernels).  wgrad2d_*: TWG = 32 positions per segment, CG = 64 input channels per
grid.y: widths 31, 32, 33, 36, 64, 68 (33 cannot take the split kernel, 36 and 68 can; 33, 36, 68 end in a partly
filled segment), 128 -> 64 (grid.y = 2), 256 -> 64 (grid.y = 4, the Embedding), 64 -> 8, 64 -> 5, 16 -> 16, 16 -> 6, the
12-channel partial group, batch 2-3 and heights 3-5.  wgrad3d_mfma: TY = 4 rows x TWG = 32 columns per step; h = 6
(partial row block), w = 33 / 35 (a second segment of 1 / 3), d = 5 / 9, batch 2; wgrad3d_plan gives such small volumes
chunks of one plane (the first zc with columns * ceil(d / zc) <= 768 / pairs), except the 64 -> 64 layer (pairs = 16,
slots = 48, columns = 8, d = 9: zc = 2, five chunks, the last one partial).  The 8 / 6 / 4-plane chunks need
columns * chunks >= 3 * 768 / pairs and are reached by the full-size tests only.  wgrad3d_s2_mfma: 32 small-grid
positions per item; small width 33 (two segments), big widths 65 / 66 / 70, odd big-grid d, h, w (7, 9, 65: the last
plane, row and column have one contributing tap).  wgrad3d_s2r: the smallest default-route volume is 512 units =
batch 2 x 8 planes x ceil(31 / 2) = 16 row blocks (the last one partial) x 2 segments (small width 36); the
neighbouring small width 35 (big 70) lands on wgrad3d_s2_mfma.

Families and a case whose probe shows them alone among the families that could serve the same layer:
  wgrad2d_mfma<mb4>          op_128_64_8_b1_n2_5x33 (all three 64-output layers), matching_64_b1_n2_4x13_shard2+4
  wgrad2d_mfma<mb4,partial>  embedding_b1_n2_20x144, embedding_b1_n3_12x130
  wgrad2d_mfma<mb1>          op_128_64_8_b0_n2_4x31, op_32_16_6_b1_n3_5x33
  wgrad2d_mfma<mb1,2src>     op_128_64_8_b1_n2_5x33, matching_64_b1_n2_4x13_shard2+4 (odd width, disparity shard)
  wgrad2d_mfma<mb4,2src>     NOT REACHABLE: the only two-source 2-D layer of any module is the last, Cout <= 16
  wgrad2d_x3                 op_128_64_8_b2_n3_5x36, op_128_64_5_b2_n3_3x68, matching_64_b1_n2_3x36 (two-source form too)
  wgrad3d_mfma<pair>         contraction_4_n2_9x11x65            wgrad3d_mfma<tap>       contraction_8/16/32_*
  wgrad3d_mfma<pair,2src>    expansion_12_*, expansion_16_*      wgrad3d_mfma<tap,2src>  expansion_32_n2_3x4x33
  wgrad3d_s2_mfma<conv>      contraction_4/8/16/32_*             wgrad3d_s2_mfma<deconv> expansion_12/16/32_*
  wgrad3d_s2r<conv>          contraction_8_n2_16x62x72           wgrad3d_s2r<deconv>     expansion_8_n2_8x31x36
  wgrad_up_full_mfma         regularization_8_n1_16x16x32 (the census)
  bwd_weight<conv>           op_64_32_8_b1_n2_5x36 (features 32)  bwd_weight<deconv>      only under
                             PDS_WGRAD3D_MFMA=0 PDS_WGRAD3D_S2_MFMA=0 (every 3-D case then)
Not covered, because no entry point builds it: single 2-D layers with a per-volume InstanceNorm, the two-source stride-2
convolution of the rolling kernel by default (HAS_B: Regularization only, whose smallest volumes stay below 512 units;
the census reaches it under PDS_WGRAD3D_S2_ROLLING=2), a 6-channel single-source pair layer (ContractionBlock3d(3) is not
a shape of the network), accumulate = 1 in any launcher, and the 8 / 6 / 4-plane chunks of wgrad3d_plan.

e32 floors (tools/wgrad_e32_floors.py on the CPU; max over the parameter tensors of the case, max-relative | mean-relative
of the weight tensors).  F and F_MEAN only guard against an e32 that happens to be near zero: the largest value of either
column rounded up to one significant digit -- per group of cases, because the hourglass (InstanceNorm over two voxels at
its deepest level) sits three orders of magnitude above every single block, and one floor for all would hold the blocks
to 6e-3, looser than the 2e-3 this file was written to tighten:
  op_128_64_8_b1_n2_5x33     12 tensors  e32 1.7e-07 .. 1.1e-06 | mean 4.5e-07 .. 4.9e-07
  op_128_64_8_b2_n3_5x36     20 tensors  e32 1.7e-07 .. 1.0e-06 | mean 5.6e-07 .. 6.9e-07
  op_128_64_5_b2_n3_3x68     20 tensors  e32 1.6e-07 .. 1.2e-06 | mean 5.4e-07 .. 6.8e-07
  op_128_64_8_b0_n2_4x31      4 tensors  e32 1.9e-07 .. 6.2e-07 | mean 2.8e-07 .. 2.8e-07
  op_128_64_8_b1_n3_3x32     12 tensors  e32 1.3e-07 .. 8.4e-07 | mean 4.3e-07 .. 4.8e-07
  op_128_64_8_b1_n2_3x64     12 tensors  e32 1.7e-07 .. 1.4e-06 | mean 4.4e-07 .. 4.8e-07
  op_32_16_6_b1_n3_5x33      12 tensors  e32 1.1e-07 .. 1.6e-06 | mean 4.0e-07 .. 4.8e-07
  op_64_32_8_b1_n2_5x36      12 tensors  e32 2.3e-07 .. 1.1e-06 | mean 4.2e-07 .. 4.8e-07
  matching_64_b1_n2_4x13_shard2+4  12 tensors  e32 1.0e-07 .. 8.3e-07 | mean 4.1e-07 .. 4.4e-07
  matching_64_b1_n2_3x36     12 tensors  e32 2.0e-07 .. 6.3e-07 | mean 4.2e-07 .. 4.6e-07
  embedding_b1_n2_20x144     20 tensors  e32 1.3e-07 .. 1.0e-06 | mean 4.7e-07 .. 6.9e-07
  embedding_b1_n3_12x130     20 tensors  e32 1.1e-07 .. 1.1e-06 | mean 4.6e-07 .. 6.5e-07
  contraction_4_n2_9x11x65      8 tensors  e32 1.4e-07 .. 8.9e-07 | mean 2.4e-07 .. 2.4e-07
  contraction_8_n2_17x12x70     8 tensors  e32 2.6e-07 .. 1.0e-06 | mean 3.9e-07 .. 4.6e-07
  contraction_16_n1_7x9x65      8 tensors  e32 2.3e-07 .. 6.6e-07 | mean 3.0e-07 .. 4.1e-07
  contraction_32_n2_17x11x66    8 tensors  e32 2.7e-07 .. 2.5e-06 | mean 9.1e-07 .. 9.6e-07
  contraction_8_n2_16x62x72     8 tensors  e32 5.1e-07 .. 3.8e-06 | mean 4.7e-07 .. 8.6e-07
  contraction_8_n2_16x62x70     8 tensors  e32 3.5e-07 .. 2.8e-06 | mean 4.5e-07 .. 8.4e-07
  expansion_12_n2_5x3x17      8 tensors  e32 1.6e-07 .. 2.2e-06 | mean 1.6e-07 .. 2.5e-07
  expansion_16_n2_3x4x33      8 tensors  e32 1.7e-07 .. 3.2e-06 | mean 1.9e-07 .. 3.3e-07
  expansion_32_n2_3x4x33      8 tensors  e32 2.6e-07 .. 2.5e-06 | mean 4.4e-07 .. 5.1e-07
  expansion_8_n2_8x31x36      8 tensors  e32 2.8e-07 .. 1.1e-05 | mean 2.7e-07 .. 3.9e-07
  regularization_8_n1_16x16x32   74 tensors  e32 1.0e-06 .. 5.8e-03 | mean 6.5e-06 .. 8.8e-05
    2-D modules: largest e32 1.59e-06 -> F = 2e-06;  largest mean 6.88e-07 -> F_MEAN = 7e-07
    3-D blocks:  largest e32 1.09e-05 -> F = 2e-05;  largest mean 9.64e-07 -> F_MEAN = 1e-06
    hourglass:   largest e32 5.82e-03 -> F = 6e-03;  largest mean 8.80e-05 -> F_MEAN = 9e-05
"""
import ctypes

import pytest
import torch

from oracle import pds_oracle as oracle
from tests import helpers
from tests.test_gpu_conv3d_layers import active_switches

pytestmark = pytest.mark.gpu
REL_TOL = 2e-3          # input gradients: the bound of tests/test_gpu_backward.py
# the floors of the docstring's table, per group of cases
GROUPS = {'op': '2-D modules', 'matching': '2-D modules', 'embedding': '2-D modules', 'contraction': '3-D blocks',
          'expansion': '3-D blocks', 'regularization': 'hourglass'}
F_FLOOR = {'2-D modules': 2e-6, '3-D blocks': 2e-5, 'hourglass': 6e-3}
F_MEAN = {'2-D modules': 7e-7, '3-D blocks': 1e-6, 'hourglass': 9e-5}

MB4, MB4_2, MB4_P = 'wgrad2d_mfma<mb4>', 'wgrad2d_mfma<mb4,2src>', 'wgrad2d_mfma<mb4,partial>'
MB1, MB1_2 = 'wgrad2d_mfma<mb1>', 'wgrad2d_mfma<mb1,2src>'
X3 = 'wgrad2d_x3'
PAIR, PAIR_2, TAP, TAP_2 = 'wgrad3d_mfma<pair>', 'wgrad3d_mfma<pair,2src>', 'wgrad3d_mfma<tap>', 'wgrad3d_mfma<tap,2src>'
S2C, S2D = 'wgrad3d_s2_mfma<conv>', 'wgrad3d_s2_mfma<deconv>'
S2RC, S2RD = 'wgrad3d_s2r<conv>', 'wgrad3d_s2r<deconv>'
UPFULL = 'wgrad_up_full_mfma'
VALU_C, VALU_D = 'bwd_weight<conv>', 'bwd_weight<deconv>'
REDUCE32, REDUCE64 = 'wgrad_reduce_f32', 'weight_reduce'
# (the probe matches by substring: no name of these tuples contains another)
FAMILIES = (MB4, MB4_2, MB4_P, MB1, MB1_2, X3, PAIR, PAIR_2, TAP, TAP_2, S2C, S2D, S2RC, S2RD, UPFULL, VALU_C, VALU_D)
PROBES = FAMILIES + (REDUCE32, REDUCE64)
R_TY, R_TWG = 2, 32     # csrc/wgrad3d_s2r.hip


# ---- the dispatch, restated --------------------------------------------------------------------------------------------
def layer(prefix, transposed, kd, stride, cin, cout, n, d, h, w, two_src=False, certified=False, launches=1):
    """One tape layer: input geometry [n, cin, d, h, w]; `certified`: every source and dz carry a range certificate."""
    return dict(prefix=prefix, transposed=transposed, kd=kd, stride=stride, cin=cin, cout=cout, n=n, d=d, h=h, w=w,
                two_src=two_src, certified=certified, launches=launches)


def expected_wgrad_kernel(L, switches):
    """The weight-gradient family backward_walk (csrc/api_training.hip) picks for a layer under the switches."""

    def value(name):
        return switches.get(name, '')[:1]

    cin, cout, two = L['cin'], L['cout'], L['two_src']
    # wgrad2d_mfma_supported, then wgrad2d_x3_supported inside launch_wgrad2d_mfma
    if (not L['transposed'] and L['kd'] == 1 and L['stride'] == 1 and (cin % 64 == 0 or cin <= 64)
            and (cout == 64 or cout <= 16)):
        if (value('PDS_WGRAD2D_X3') != '0' and cin % 64 == 0 and L['w'] % 4 == 0 and L['certified']
                and 64 * L['d'] * L['h'] * L['w'] < 1 << 31):
            return X3
        if cout == 64 and cin < 64 and not two:
            return MB4_P
        if cout == 64:
            return MB4_2 if two else MB4
        return MB1_2 if two else MB1
    # wgrad3d_mfma_supported (same-size output: padding 1)
    if (value('PDS_WGRAD3D_MFMA') != '0' and not L['transposed'] and L['kd'] == 3 and L['stride'] == 1
            and L['d'] * L['h'] * L['w'] * 16 < 1 << 31):
        if cin <= 8:
            return PAIR_2 if two else PAIR
        return TAP_2 if two else TAP
    s2 = value('PDS_WGRAD3D_S2_MFMA') != '0'
    # wgrad_up_full_mfma_supported
    if s2 and L['transposed'] and L['kd'] == 3 and not two and cin <= 4 and cout == 1:
        return UPFULL
    # wgrad3d_s2_mfma_supported, then wgrad3d_s2_rolling_supported inside launch_wgrad3d_s2_mfma
    if s2 and ((L['transposed'] and L['kd'] == 4) or (not L['transposed'] and L['kd'] == 3 and L['stride'] == 2)):
        if L['transposed']:
            small = (cin, L['d'], L['h'], L['w'])
            big = (cout, 2 * L['d'], 2 * L['h'], 2 * L['w'])
        else:
            small = (cout, (L['d'] + 1) // 2, (L['h'] + 1) // 2, (L['w'] + 1) // 2)
            big = (cin, L['d'], L['h'], L['w'])
        mode = value('PDS_WGRAD3D_S2_ROLLING')
        units = L['n'] * small[1] * -(-small[2] // R_TY) * -(-small[3] // R_TWG)
        rolling = (mode != '0' and big[0] in (4, 8) and small[0] <= 16 and big[3] % 4 == 0 and small[3] % 4 == 0
                   and not (L['transposed'] and two) and big[1] * big[2] * big[3] * 8 < 1 << 31
                   and (mode == '2' or units >= 512))
        if rolling:
            return S2RD if L['transposed'] else S2RC
        return S2D if L['transposed'] else S2C
    return VALU_D if L['transposed'] else VALU_C


def expected_counts(layers, switches):
    counts = {name: 0 for name in PROBES}
    for L in layers:
        family = expected_wgrad_kernel(L, switches)
        counts[family] += L['launches']
        counts[REDUCE64 if family in (VALU_C, VALU_D) else REDUCE32] += L['launches']
    return counts


# ---- the layer lists of the modules (csrc/api_regularization.hip, api_matching.hip, api_embedding.hip) -----------------
def contraction_layers(features, n, d, h, w, prefix='', shortcut=False):
    half = ((d + 1) // 2, (h + 1) // 2, (w + 1) // 2)
    return [layer(prefix + '_downsampling_2x', False, 3, 2, features, 2 * features, n, d, h, w, two_src=shortcut),
            layer(prefix + '_smoothing', False, 3, 1, 2 * features, 2 * features, n, *half)]


def expansion_layers(features, n, d, h, w, prefix=''):
    return [layer(prefix + '_upsampling_2x', True, 4, 2, features, features // 2, n, d, h, w),
            layer(prefix + '_smoothing', False, 3, 1, features // 2, features // 2, n, 2 * d, 2 * h, 2 * w, two_src=True)]


def regularization_layers(features, n, d, h, w):
    layers = [layer('_smoothing', False, 3, 1, features, features, n, d, h, w)]
    c, g = features, (d, h, w)
    for i in range(4):
        layers += contraction_layers(c, n, *g, prefix='_contraction_blocks.%d.' % i, shortcut=True)
        c, g = 2 * c, tuple((v + 1) // 2 for v in g)
    for i in range(4):
        layers += expansion_layers(c, n, *g, prefix='_expansion_blocks.%d.' % i)
        c, g = c // 2, tuple(2 * v for v in g)
    layers.append(layer('_upsample_to_halfsize', True, 4, 2, c, c // 2, n, *g))
    layers.append(layer('_upsample_to_fullsize', True, 3, 1, c // 2, 1, n, *(2 * v for v in g)))
    return layers


def operation_tail_layers(features, cout, blocks, n, d, h, w, x0_certified):
    """operation_tail: x0 carries a certificate only on the native route (l0_combine records it); every normalised
    tensor and every residual sum does."""
    m, layers, cur = '_matching_operation_modules', [], x0_certified
    for r in range(blocks):
        layers.append(layer('%s.%d.convolutions.0' % (m, 1 + r), False, 1, 1, features, features, n, d, h, w,
                            certified=cur))
        layers.append(layer('%s.%d.convolutions.1' % (m, 1 + r), False, 1, 1, features, features, n, d, h, w,
                            certified=True))
        if r + 1 < blocks:
            cur = True
    layers.append(layer('%s.%d' % (m, 1 + blocks), False, 1, 1, features, cout, n, d, h, w, two_src=blocks > 0,
                        certified=cur))
    return layers


def operation_layers(features, cout, blocks, n, h, w):
    first = layer('_matching_operation_modules.0', False, 1, 1, 2 * features, features, n, 1, h, w)
    return [first] + operation_tail_layers(features, cout, blocks, n, 1, h, w, False)


def matching_layers(features, cout, blocks, n, h, w, planes):
    """Native route: layer 0 through its factorisation -- three single-plane launches on rows of w + 1 columns, plain
    sources (matching_backward) -- then operation_tail over the disparity planes."""
    first = layer('_matching_operation_modules.0', False, 1, 1, features, features, n, 1, h, w + 1, launches=3)
    return operation_tail_layers(features, cout, blocks, n, planes, h, w, True) + [first]


def embedding_layers(blocks, n, h, w, features=64, shortcut=8, image=3):
    h2, w2, h4, w4 = (h + 1) // 2, (w + 1) // 2, ((h + 1) // 2 + 1) // 2, ((w + 1) // 2 + 1) // 2
    m = '_embedding_modules'
    layers = [layer(m + '.1', False, 1, 1, 4 * image, features, n, 1, h2, w2),
              layer(m + '.2', False, 1, 1, 4 * features, features, n, 1, h4, w4, certified=True)]
    for r in range(blocks):
        for j in range(2):
            layers.append(layer('%s.%d.convolutions.%d' % (m, 3 + r, j), False, 1, 1, features, features, n, 1, h4, w4,
                                certified=True))
    layers.append(layer('_shortcut', False, 1, 1, features, shortcut, n, 1, h4, w4, certified=blocks > 0))
    return layers


# ---- the case table ------------------------------------------------------------------------------------------------------
# kind, arguments:
#   contraction  (features, n, d, h, w)                  input grid
#   expansion    (features, n, d, h, w)                  input (small) grid
#   op           (features, signature features, residual blocks, n, h, w)
#   matching     (features, residual blocks, n, h, w, maximum disparity, shard)
#   embedding    (residual blocks, n, H, W)              image size
#   regularization (features, n, d, h, w)
CASES = [
    ('op', (64, 8, 1, 2, 5, 33)),           # width 33: no split kernel; <mb4> grid.y = 2 and 1, <mb1,2src>
    ('op', (64, 8, 2, 3, 5, 36)),           # width 36: wgrad2d_x3 (one and two sources), partial second segment
    ('op', (64, 5, 2, 3, 3, 68)),           # width 68: a partial third segment; 64 -> 5 on the split kernel
    ('op', (64, 8, 0, 2, 4, 31)),           # width 31; no residual block: <mb1> with one plain source
    ('op', (64, 8, 1, 3, 3, 32)),           # width 32: exactly one segment
    ('op', (64, 8, 1, 2, 3, 64)),           # width 64: exactly two
    ('op', (16, 6, 1, 3, 5, 33)),           # 32 -> 16, 16 -> 16, 16 -> 6: the <mb1> forms, Cout % 4 != 0
    ('op', (32, 8, 1, 2, 5, 36)),           # features 32: bwd_weight<conv>; 32 -> 8 two-source <mb1,2src>
    ('matching', (64, 1, 2, 4, 13, 7, (2, 4))),   # native route, odd width, disparity shard: <mb1,2src>, 3 x <mb4> at w + 1
    ('matching', (64, 1, 2, 3, 36, 7, None)),     # native route on a width the split kernel takes: two-source wgrad2d_x3
    ('embedding', (1, 2, 20, 144)),         # 12-channel partial group on 72 columns; 256 -> 64 (grid.y = 4) split
    ('embedding', (1, 3, 12, 130)),         # ... on 65 columns; quarter width 33: exact kernels, grid.y = 4
    ('contraction', (4, 2, 9, 11, 65)),     # -> (5, 6, 33): s2 conv on an odd big grid; 8 -> 8 <pair>
    ('contraction', (8, 2, 17, 12, 70)),    # -> (9, 6, 35): 16 -> 16 <tap>; big width 70 keeps the rolling kernel out
    ('contraction', (16, 1, 7, 9, 65)),     # -> (4, 5, 33): 16 -> 32 s2 conv, odd big grid (7, 9, 65)
    ('contraction', (32, 2, 17, 11, 66)),   # -> (9, 6, 33): 32 -> 64 s2 conv; 64 -> 64 <tap>, two-plane chunks
    ('contraction', (8, 2, 16, 62, 72)),    # -> (8, 31, 36): 512 units, the rolling kernel by default
    ('contraction', (8, 2, 16, 62, 70)),    # -> (8, 31, 35): 512 units, small width 35: wgrad3d_s2_mfma<conv>
    ('expansion', (12, 2, 5, 3, 17)),       # 12 -> 6 k4; 6 -> 6 <pair,2src> at (10, 6, 34)
    ('expansion', (16, 2, 3, 4, 33)),       # 16 -> 8 k4: dz has 8 channels, small width 33, big 66; 8 -> 8 <pair,2src>
    ('expansion', (32, 2, 3, 4, 33)),       # 32 -> 16 k4; 16 -> 16 <tap,2src>
    ('expansion', (8, 2, 8, 31, 36)),       # 8 -> 4 k4 on 512 units: the rolling kernel by default; 4 -> 4 <pair,2src>
    ('regularization', (8, 1, 16, 16, 32)),   # the smallest volume the hourglass accepts: the census
]


def case_id(case):
    kind, a = case
    if kind == 'op':
        return 'op_%d_%d_%d_b%d_n%d_%dx%d' % (2 * a[0], a[0], a[1], a[2], a[3], a[4], a[5])
    if kind == 'matching':
        shard = '_shard%d+%d' % a[6] if a[6] else ''
        return 'matching_%d_b%d_n%d_%dx%d%s' % (a[0], a[1], a[2], a[3], a[4], shard)
    if kind == 'embedding':
        return 'embedding_b%d_n%d_%dx%d' % a
    return '%s_%d_n%d_%dx%dx%d' % ((kind,) + tuple(a))


def case_layers(case):
    kind, a = case
    if kind == 'op':
        return operation_layers(*a)
    if kind == 'matching':
        features, blocks, n, h, w, maximum, shard = a
        return matching_layers(features, 8, blocks, n, h, w, shard[1] if shard else maximum + 1)
    if kind == 'embedding':
        return embedding_layers(*a)
    return {'contraction': contraction_layers, 'expansion': expansion_layers,
            'regularization': regularization_layers}[kind](*a)


def make_module(case):
    import practicaldeepstereo_nips2018_amd as pds
    kind, a = case
    seed = 100 + CASES.index(case)
    if kind in ('op', 'matching'):
        cout, blocks = (a[1], a[2]) if kind == 'op' else (8, a[1])
        return helpers.seeded(lambda: pds.MatchingOperation(2 * a[0], a[0], cout, blocks), seed)
    if kind == 'embedding':
        return helpers.seeded(lambda: pds.Embedding(number_of_residual_blocks=a[0]), seed)
    factory = {'contraction': pds.ContractionBlock3d, 'expansion': pds.ExpansionBlock3d,
               'regularization': pds.Regularization}[kind]
    return helpers.seeded(lambda: factory(a[0]), seed)


def make_inputs(case):
    """-> (inputs, upstream weights), CPU fp32."""
    kind, a = case
    g = torch.Generator().manual_seed(7000 + CASES.index(case))

    def randn(*shape):
        return torch.randn(*shape, generator=g)

    if kind == 'op':
        features, cout, _, n, h, w = a
        return [randn(n, 2 * features, h, w)], [randn(n, cout, h, w)]
    if kind == 'matching':
        features, _, n, h, w, maximum, shard = a
        planes = shard[1] if shard else maximum + 1
        return [randn(n, features, h, w), randn(n, features, h, w)], [randn(n, 8, planes, h, w)]
    if kind == 'embedding':
        _, n, h, w = a
        h4, w4 = ((h + 1) // 2 + 1) // 2, ((w + 1) // 2 + 1) // 2
        return [torch.rand(n, 3, h, w, generator=g) * 255], [randn(n, 64, h4, w4), randn(n, 8, h4, w4)]
    features, n, d, h, w = a
    if kind == 'contraction':
        half = (n, 2 * features, (d + 1) // 2, (h + 1) // 2, (w + 1) // 2)
        return [randn(n, features, d, h, w)], [randn(*half), randn(*half)]
    if kind == 'expansion':
        big = (n, features // 2, 2 * d, 2 * h, 2 * w)
        return [randn(n, features, d, h, w), randn(*big)], [randn(*big)]
    return [randn(n, features, d, h, w), randn(n, features, h, w)], [randn(n, 2 * d, 4 * h, 4 * w)]


def cpu_gradients(case, module, inputs, weights, dtype):
    """CPU autograd of sum(outputs * upstream weights) in `dtype` through the oracle -> (parameter gradients by the
    module's parameter names, input gradients; None for an input that takes none)."""
    kind, a = case
    p = {'_m.' + k: v.detach().to(dtype).requires_grad_(True) for k, v in module.state_dict().items()}
    leaves = [t.detach().clone().to(dtype).requires_grad_(kind != 'embedding') for t in inputs]
    if kind == 'op':
        outputs = [oracle.matching_operation(p, '_m', leaves[0], a[2])]
    elif kind == 'matching':
        begin, count = a[6] if a[6] else (0, a[5] + 1)
        full = oracle.matching(leaves[0], leaves[1], a[5], lambda x: oracle.matching_operation(p, '_m', x, a[1]))
        outputs = [full[:, :, begin:begin + count]]
    elif kind == 'embedding':
        outputs = list(oracle.embedding(p, '_m', leaves[0], number_of_residual_blocks=a[0]))
    elif kind == 'contraction':
        outputs = list(oracle.contraction_block_3d(p, '_m', leaves[0]))
    elif kind == 'expansion':
        outputs = [oracle.expansion_block_3d(p, '_m', leaves[0], leaves[1])]
    else:
        outputs = [oracle.regularization(p, '_m', leaves[0], leaves[1])]
    sum((o * w.to(dtype)).sum() for o, w in zip(outputs, weights)).backward()
    return ({k[3:]: v.grad.double() for k, v in p.items()},
            [t.grad.double() if t.grad is not None else None for t in leaves])


def distance(got, want):
    """(max-relative, mean-relative) distance of a gradient tensor from the fp64 one."""
    delta = (got.double() - want).abs()
    return (float(delta.max() / want.abs().max().clamp_min(1e-30)),
            float(delta.mean() / want.abs().mean().clamp_min(1e-30)))


def layer_of(name, layers):
    for L in layers:
        if name.startswith(L['prefix'] + '.'):
            return L
    raise KeyError(name)


# ---- the GPU side --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def count_launches(lib, name, run, capacity=64):
    """Launches whose probe name contains `name` during `run` (the hourglass has 19 reductions: room for 64)."""
    from practicaldeepstereo_nips2018_amd import _lib
    _lib.check(lib.pds_probe_begin(name.encode(), capacity), 'pds_probe_begin')
    try:
        result = run()
        torch.cuda.synchronize()
    finally:
        count = lib.pds_probe_end(None, None, capacity)
    assert 0 <= count < capacity, lib.pds_last_error()
    return count, result


def nan_bytes(count, dev):
    return torch.full((max(int(count), 256),), 0xFF, dtype=torch.uint8, device=dev)


def block_runner(case, module, inputs, weights, dev):
    """ContractionBlock3d / ExpansionBlock3d through the C entry points: every buffer is the test's, the gradient
    buffers and the backward workspace are NaN before the call."""
    from practicaldeepstereo_nips2018_amd import _lib
    from practicaldeepstereo_nips2018_amd.regularization import _block_params
    lib = _lib.load()
    kind, (features, n, d, h, w) = case
    first = module._downsampling_2x if kind == 'contraction' else module._upsampling_2x
    p0, p1 = _block_params(first), _block_params(module._smoothing)
    xs = [t.to(dev).contiguous() for t in inputs]
    ups = [t.to(dev).contiguous() for t in weights]
    stream = _lib.stream_handle(dev)
    sizes = ((lib.pds_contraction_block_workspace_bytes, lib.pds_contraction_block_bwd_workspace_bytes)
             if kind == 'contraction' else
             (lib.pds_expansion_block_workspace_bytes, lib.pds_expansion_block_bwd_workspace_bytes))

    def run():
        fws = torch.empty(max(int(sizes[0](n, features, d, h, w)), 256), dtype=torch.uint8, device=dev)
        bws = nan_bytes(sizes[1](n, features, d, h, w), dev)
        grads = {id(q): torch.full_like(q, float('nan')) for q in module.parameters()}
        g0, g1 = _block_params(first, lambda q: grads[id(q)]), _block_params(module._smoothing, lambda q: grads[id(q)])
        grad_inputs = [torch.full_like(t, float('nan')) for t in xs]
        if kind == 'contraction':
            outs = [torch.empty_like(ups[0]), torch.empty_like(ups[1])]
            _lib.check(lib.pds_contraction_block_fwd(ctypes.byref(p0), ctypes.byref(p1), _lib.ptr(xs[0]), _lib.ptr(outs[0]),
                                                     _lib.ptr(outs[1]), n, features, d, h, w, _lib.ptr(fws), fws.numel(),
                                                     stream), 'pds_contraction_block_fwd')
            _lib.check(lib.pds_contraction_block_bwd(ctypes.byref(p0), ctypes.byref(p1), ctypes.byref(g0), ctypes.byref(g1),
                                                     _lib.ptr(xs[0]), _lib.ptr(ups[0]), _lib.ptr(ups[1]),
                                                     _lib.ptr(grad_inputs[0]), n, features, d, h, w, _lib.ptr(fws),
                                                     fws.numel(), _lib.ptr(bws), bws.numel(), stream),
                       'pds_contraction_block_bwd')
        else:
            outs = [torch.empty_like(ups[0])]
            _lib.check(lib.pds_expansion_block_fwd(ctypes.byref(p0), ctypes.byref(p1), _lib.ptr(xs[0]), _lib.ptr(xs[1]),
                                                   _lib.ptr(outs[0]), n, features, d, h, w, _lib.ptr(fws), fws.numel(),
                                                   stream), 'pds_expansion_block_fwd')
            _lib.check(lib.pds_expansion_block_bwd(ctypes.byref(p0), ctypes.byref(p1), ctypes.byref(g0), ctypes.byref(g1),
                                                   _lib.ptr(xs[0]), _lib.ptr(xs[1]), _lib.ptr(ups[0]),
                                                   _lib.ptr(grad_inputs[0]), _lib.ptr(grad_inputs[1]), n, features, d, h, w,
                                                   _lib.ptr(fws), fws.numel(), _lib.ptr(bws), bws.numel(), stream),
                       'pds_expansion_block_bwd')
        torch.cuda.synchronize()
        return {name: grads[id(q)] for name, q in module.named_parameters()}, grad_inputs

    return run


def module_runner(case, module, inputs, weights, dev):
    """The modules that own their buffers, through autograd."""
    import practicaldeepstereo_nips2018_amd as pds
    kind, a = case
    net = module
    if kind == 'matching':
        net = pds.Matching(a[5], module)
        assert module.supports_native_training()
        net.set_disparity_shard(a[6])
    ups = [t.to(dev) for t in weights]

    def run():
        for q in module.parameters():
            q.grad = None
        xs = [t.to(dev).requires_grad_(kind != 'embedding') for t in inputs]
        outputs = net(*xs)
        outputs = outputs if isinstance(outputs, tuple) else (outputs,)
        sum((o * u).sum() for o, u in zip(outputs, ups)).backward()
        torch.cuda.synchronize()
        return {name: q.grad.detach() for name, q in module.named_parameters()}, [t.grad for t in xs]

    return run


_worst = {}    # family -> (err / gate, case): printed by the last test


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_wgrad_layers_against_fp64(dev, case):
    from practicaldeepstereo_nips2018_amd import _lib
    lib = _lib.load()
    kind = case[0]
    module = make_module(case)
    inputs, weights = make_inputs(case)
    want, want_inputs = cpu_gradients(case, module, inputs, weights, torch.float64)
    theirs, _ = cpu_gradients(case, module, inputs, weights, torch.float32)
    module = module.to(dev)
    runner = block_runner if kind in ('contraction', 'expansion') else module_runner
    run = runner(case, module, inputs, weights, dev)
    torch.cuda.synchronize()
    nonfinite_before = lib.pds_nonfinite_statistics(0)

    counts, result = {}, None
    for name in PROBES:
        counts[name], result = count_launches(lib, name, run)
    grads, grad_inputs = result
    switches = active_switches()
    layers = case_layers(case)
    expected = expected_counts(layers, switches)
    print('wgrad case %s: launches %s' % (case_id(case), {k: v for k, v in counts.items() if v}))

    # 1. which kernels ran
    assert counts == expected, 'launches %s, expected %s' % ({k: v for k, v in counts.items() if v},
                                                            {k: v for k, v in expected.items() if v})
    # 2. nothing stale
    for name, g in grads.items():
        assert bool(torch.isfinite(g).all()), 'gradient of %s left unwritten or non-finite' % name
    for g in grad_inputs:
        assert g is None or bool(torch.isfinite(g).all()), 'input gradient left unwritten or non-finite'
    assert lib.pds_nonfinite_statistics(0) == nonfinite_before
    # 3. values
    failures = []
    for name, g in grads.items():
        family = expected_wgrad_kernel(layer_of(name, layers), switches)
        err, err_mean = distance(g.cpu(), want[name])
        e32, e32_mean = distance(theirs[name], want[name])
        gate, gate_mean = max(F_FLOOR[GROUPS[kind]], 3.0 * e32), max(F_MEAN[GROUPS[kind]], 3.0 * e32_mean)
        print('    %-58s %-26s err %.2e  e32 %.2e  gate %.2e  x%.2f   mean %.2e (fp32 %.2e)'
              % (name, family, err, e32, gate, err / gate, err_mean, e32_mean))
        if err / gate > _worst.get(family, (0.0, ''))[0]:
            _worst[family] = (err / gate, case_id(case) + ' ' + name)
        if not err <= gate:
            failures.append((name, family, err, gate))
        if family == X3 and name.endswith('.weight') and g.dim() == 4 and not err_mean <= gate_mean:
            failures.append((name, family + ' mean', err_mean, gate_mean))
    assert not failures, failures
    # 4. input gradients
    for g, w64 in zip(grad_inputs, want_inputs):
        if w64 is not None:
            assert distance(g.cpu(), w64)[0] <= REL_TOL


def test_zz_report_worst_ratio_per_family(dev):
    """Prints, per family, the largest err / gate seen by the cases above (nothing to assert beyond what they did)."""
    for family in sorted(_worst):
        print('worst err / gate  %-26s x%.2f  (%s)' % ((family,) + _worst[family]))
    assert all(ratio <= 1.0 for ratio, _ in _worst.values())
