"""GPU (-m gpu): every data-gradient and InstanceNorm-backward kernel of the backward pass alone, one block at a time,
against fp64.

pds_conv_block_tape_fwd / pds_conv_block_bwd run ONE block (convolution kd 1 | 3, stride 1 | 2, or transposed convolution
kd 3 | 4; with or without InstanceNorm; per-volume or per-plane statistics; one or two plain sources) forward and through
backward_walk (csrc/api_training.hip) on a one-layer tape.  The test owns every buffer.

Every case
  1. counts the launches of every probe name of PROBES during the backward call, one run per name, and asserts that
     exactly the names `expected_counts` predicts launched, the predicted number of times, and every other name not at
     all; for bwd_data2 also that the launch had the predicted number of workgroups (ceil(units * ocg / 4));
  2. pre-fills every gradient buffer and the backward workspace with NaN bytes before each run: everything is finite
     afterwards, pds_nonfinite_statistics does not move, and two runs give the same bits (every reduction of
     csrc/backward.hip is two-stage in a fixed order; the atomicMax of the range certificate is order-independent);
  3. compares dx (both sources' gradients where there are two; they must be two buffers), dbias, dgamma and dbeta with
     CPU fp64 autograd of the same block built from torch.nn.functional, LeakyReLU slope and InstanceNorm eps taken from
     oracle/pds_oracle.py: err = max|g - g64| / max|g64| <= max(F, 3 * e32), and for dx also the mean-relative form
     mean|g - g64| / mean|g64| <= max(F_MEAN, 3 * e32_mean); e32 = the same distance of the CPU fp32 autograd of the
     case, computed here at run time.  Where the probe shows that a split-operand forward kernel served the stride-1
     data gradient (SPLIT_FORWARD) the gate of dx is that kernel's own forward bound of tests/test_gpu_range_safety.py,
     max(REL_TOL, 3 * e32) as max-relative and max(REL_TOL_MEAN, 3 * e32) for mean|g - g64| / max|g64|.

Dispatch, restated (csrc/api_training.hip backward_walk, csrc/backward.hip):
  expected_in_bwd_route    launch_in_bwd: per-volume groups of at most 36864 elements are viewed as one plane of
                           d * h * w; a (viewed) per-plane group takes in_bwd_plane when PDS_IN_BWD_PLANE != 0, the plane
                           has at most 36864 elements, a multiple of 4, and g, raw and dz are 16-byte aligned; else
                           in_bwd_twopass (tiles per plane = ceil(plane / 1024) capped at 64).  A per-volume group of
                           depth 1 counts as per-plane.  A bare layer has no InstanceNorm: channel_sum instead, with
                           max(1, min(volume / 4096, 2048 / C)) splits.
  expected_bwd_data_variant  launch_bwd_data2 (stride-2 convolutions and transposed layers unless PDS_BWD_DATA_V2=0):
                           pairs = ceil(Wi / 2); pw = 64 halved while pw > 8 and pw / 2 >= pairs; ry = 64 / pw rows per
                           wave; segs = ceil(pairs / pw); yblocks = ceil(rows / ry), rows = Hi (transposed) or
                           ceil(Hi / 2) per parity; cb = 8 when Cin % 8 == 0 and per_cb * Cin / 8 >= 512, else 4, with
                           per_cb = N * Di * (1 | 2) * yblocks * segs; units = per_cb * ceil(Cin / cb); ocg doubles
                           from 1 while ocg < 4, units * ocg < 4096 and Cout >= 8 * ocg; VEC (transposed only):
                           Wo % 4 == 0 and dz 16-byte aligned.  Under PDS_BWD_DATA_V2=0: bwd_data1<...>.
  expected_stride1         stride-1 convolutions: flip_weights, then the forward kernels on dz with its certificate.
                           kd 1 with Cin > 64, Cin % 64 == 0: 64-channel blocks -- W % 2 == 0 and Cout % 4 == 0: one
                           certified launch per block over the batch (channel slice of dx, ConvExtra::out_batch_channels);
                           else one un-certified launch per batch entry and block.  The kernel of each launch is that of
                           tests/test_gpu_conv2d_layers.py `dispatch` (bare, plain source: conv2d_t8w never) or, kd 3,
                           of `dispatch3d` below (csrc/api.hip conv_block).
  grad_add                 once per source (the caller's buffers are never adopted); grad_reduce_d never (no entry point
                           below the hourglass builds a source broadcast along D).

Variant -> case (ids of the table below):
  bwd_data2<conv,cb8,ocg4> ry1          s2_8_16_n2_16x62x72        bwd_data2<conv,cb8,ocg1> segs 2   s2_8_16_n2_16x64x130
  bwd_data2<conv,cb4,ocg4> odd extents  s2_8_16_n1_7x9x65          bwd_data2<conv,cb4,ocg2> ry8      s2_4_8_n2_9x11x15
  ... ry4 (width 21)                    s2_4_8_n2_5x7x21           ... ry2 (width 35)                s2_4_8_n2_5x6x35
  partial channel block (nch 2)         s2_6_8_n2_5x7x13           two sources                       s2_4_8_n2_5x7x21_2src
  bwd_data2<deconv4,cb4,ocg2,vec0>      d4_16_8_n2_3x4x33, d4_16_8_n2_3x4x34_bare_offset (dz off by one float)
  bwd_data2<deconv4,cb4,ocg2,vec1>      d4_16_8_n2_3x4x34          bwd_data2<deconv3,cb4,ocg1,vec1>  d3_4_1_n2_4x5x18_bare
  bwd_data1<conv,k3,s2> / <deconv,k4> / <deconv,k3>   the same cases under PDS_BWD_DATA_V2=0 only
  stride 1, per entry and block         c1_128_64_n2_1x5x33        channel slices                    c1_128_64_n2_1x5x36
  certified 64 -> 64                    c1_64_64_n2_2x5x36         heavy-tailed dz                   c1_64_64_n2_2x6x36_heavy(_bare)
  3-D 8 -> 8 (conv3d_t8x)               c3_8_8_n2_3x6x34           3-D 16 -> 16 (conv3d_ks<fp16>)    c3_16_16_n2_3x5x20(_2src)
  in_bwd_plane per plane                c1_64_64_n2_2x5x36         per volume, flattened             c3_8_8_n2_3x6x34
  in_bwd_twopass d*h*w % 4 != 0         c3_8_8_n2_3x5x7            above 36864 elements              c3_8_8_n2_5x80x96
  tile cap 64 (plane 66048)             c1_3_3_n2_1x128x516_pp     g off by one float                c1_8_3_n2_2x6x8_pp_offset
  channel_sum one split / several       d3_4_1_n2_4x5x18_bare / c1_64_64_n2_2x6x36_heavy_bare (864) ; c1_8_3_n2_1x96x96_bare (9216: 2 splits)
Not reachable, with the reason:
  bwd_data1<conv,k1,s1>, <conv,k3,s1>   backward_walk sends every stride-1 convolution to the forward kernels (conv_block
                                        falls back to conv_direct itself); launch_bwd_data never sees stride 1.
  bwd_data2<...,ocg1> by units >= 4096  only through Cout < 8 at small shapes, except s2_8_16_n2_16x64x130.
  bwd_data2<deconv*,cb8,*>              needs per_cb * Cin / 8 >= 512 transposed units: full-size hourglass levels only;
                                        the kernel body is shared with the cb4 instantiation.
  conv3d_nx / conv3d_mfma as the data-gradient kernel   16 -> 16 from 100 000 voxels / above 30 000: forward files cover them.
  grad_reduce_d                         see above.

e32 floors (tools/dgrad_e32_floors.py on the CPU; largest value over the gradient tensors of the case, max-relative |
mean-relative of dx).  F / F_MEAN only guard against an e32 that happens to be near zero: the largest value of the column
over the group rounded up to one significant digit:
  s2_8_16_n2_16x62x72              4 tensors  e32 1.3e-07 .. 1.8e-06 | dx mean 1.2e-07
  s2_8_16_n2_16x64x130             4 tensors  e32 1.2e-07 .. 2.5e-06 | dx mean 1.2e-07
  s2_8_16_n1_7x9x65                4 tensors  e32 7.8e-08 .. 3.9e-07 | dx mean 1.0e-07
  s2_4_8_n2_9x11x15                4 tensors  e32 6.5e-08 .. 4.7e-07 | dx mean 1.1e-07
  s2_4_8_n2_5x7x21                 4 tensors  e32 1.3e-07 .. 5.0e-07 | dx mean 1.2e-07
  s2_4_8_n2_5x6x35                 4 tensors  e32 5.1e-08 .. 3.2e-07 | dx mean 1.0e-07
  s2_6_8_n2_5x7x13                 4 tensors  e32 5.0e-08 .. 3.0e-07 | dx mean 1.2e-07
  s2_4_8_n2_5x7x21_2src            5 tensors  e32 1.1e-07 .. 3.9e-07 | dx mean 1.1e-07
  d4_16_8_n2_3x4x33                4 tensors  e32 1.4e-07 .. 3.2e-06 | dx mean 3.1e-07
  d4_16_8_n2_3x4x34                4 tensors  e32 2.2e-07 .. 8.8e-07 | dx mean 3.1e-07
  d4_16_8_n2_3x4x34_bare_offset    2 tensors  e32 9.6e-07 .. 1.1e-06 | dx mean 3.1e-07
  d3_4_1_n2_4x5x18_bare            2 tensors  e32 1.2e-07 .. 2.1e-07 | dx mean 9.3e-08
  c1_128_64_n2_1x5x33              4 tensors  e32 9.1e-08 .. 6.6e-07 | dx mean 2.1e-07
  c1_128_64_n2_1x5x36              4 tensors  e32 9.4e-08 .. 4.3e-07 | dx mean 2.1e-07
  c1_64_64_n2_2x5x36               4 tensors  e32 7.2e-08 .. 5.8e-07 | dx mean 2.1e-07
  c1_64_64_n2_2x6x36_heavy         4 tensors  e32 1.2e-07 .. 8.8e-07 | dx mean 2.0e-07
  c1_64_64_n2_2x6x36_heavy_bare    2 tensors  e32 3.5e-07 .. 3.9e-07 | dx mean 1.6e-07
  c3_8_8_n2_3x6x34                 4 tensors  e32 5.8e-08 .. 5.7e-07 | dx mean 2.1e-07
  c3_16_16_n2_3x5x20               4 tensors  e32 1.3e-07 .. 5.5e-07 | dx mean 2.8e-07
  c3_16_16_n2_3x5x20_2src          5 tensors  e32 1.1e-07 .. 6.6e-07 | dx mean 2.9e-07
  c3_8_8_n2_3x5x7                  4 tensors  e32 8.8e-08 .. 5.4e-07 | dx mean 2.1e-07
  c3_8_8_n2_5x80x96                4 tensors  e32 7.1e-08 .. 2.9e-06 | dx mean 2.2e-07
  c1_3_3_n2_1x128x516_pp           4 tensors  e32 7.9e-08 .. 1.8e-05 | dx mean 1.0e-07
  c1_8_3_n2_2x6x8_pp_offset        4 tensors  e32 5.3e-08 .. 1.9e-06 | dx mean 1.2e-07
  c1_8_3_n2_1x96x96_bare           2 tensors  e32 2.0e-07 .. 6.9e-07 | dx mean 8.6e-08
    3-D layers: largest e32 3.17e-06 -> F = 4e-06;  largest dx mean 3.11e-07 -> F_MEAN = 4e-07
    2-D layers: largest e32 1.77e-05 -> F = 2e-05;  largest dx mean 2.13e-07 -> F_MEAN = 3e-07
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import pds_oracle as oracle
from tests import test_gpu_conv2d_layers as conv2d
from tests.test_gpu_conv3d_layers import active_switches
from tests.test_gpu_range_safety import REL_TOL, REL_TOL_MEAN

pytestmark = pytest.mark.gpu
F_FLOOR = {'2-D layers': 2e-5, '3-D layers': 4e-6}     # the floors of the docstring's table, per group of cases
F_MEAN = {'2-D layers': 3e-7, '3-D layers': 4e-7}

IN_PLANE, IN_TWOPASS = 'in_bwd_plane', 'in_bwd_twopass'
CHANNEL_SUM, FLIP, GRAD_ADD, GRAD_REDUCE_D = 'channel_sum', 'flip_weights', 'grad_add', 'grad_reduce_d'
DATA1 = ('bwd_data1<conv,k1,s1>', 'bwd_data1<conv,k3,s1>', 'bwd_data1<conv,k3,s2>', 'bwd_data1<deconv,k3>',
         'bwd_data1<deconv,k4>')
DATA2 = tuple(['bwd_data2<conv,cb%d,ocg%d>' % (cb, ocg) for cb in (4, 8) for ocg in (1, 2, 4)]
              + ['bwd_data2<deconv%d,cb%d,ocg%d,vec%d>' % (kd, cb, ocg, vec)
                 for kd in (3, 4) for cb in (4, 8) for ocg in (1, 2, 4) for vec in (0, 1)])
T8X, T8, NX, KS16, KS32, MFMA3, DIRECT3 = ('conv3d_t8x', 'conv3d_t8<', 'conv3d_nx', 'conv3d_ks<fp16>', 'conv3d_ks<fp32>',
                                           'conv3d_mfma', 'conv_direct<3d>')
FORWARD3D = (T8X, T8, NX, KS16, KS32, MFMA3, DIRECT3)
# (the probe matches by substring: no name of PROBES contains another -- 'conv3d_t8<' is the exact kernel's
# "conv3d_t8<exact>" / "conv3d_t8<guarded>", which "conv3d_t8x<...>" does not contain)
PROBES = (IN_PLANE, IN_TWOPASS, CHANNEL_SUM, FLIP, GRAD_ADD, GRAD_REDUCE_D) + DATA1 + DATA2 + conv2d.FAMILIES + FORWARD3D
SPLIT_FORWARD = (conv2d.X3F, conv2d.T8, conv2d.T8W, T8X, NX, KS16)
PLANE_LIMIT = 1024 * 9 * 4      # kPlaneThreads * kPlaneQuads * 4 (csrc/backward.hip)


# ---- the case table ------------------------------------------------------------------------------------------------------
def case(name, kind, cin, cout, n, d, h, w, norm=True, per_plane=0, two=False, offset=False, heavy=False):
    """kind: 'c1' convolution kd 1 (the D axis is a stack of planes), 'c3' kd 3 stride 1, 's2' kd 3 stride 2, 'd3' / 'd4'
    transposed kd 3 / 4.  Input geometry [n, cin, d, h, w].  offset: grad_out is a view one float into its buffer.
    heavy: a few entries of the upstream gradient are about 1e3 times the bulk."""
    transposed = kind in ('d3', 'd4')
    kd = {'c1': 1, 'c3': 3, 's2': 3, 'd3': 3, 'd4': 4}[kind]
    return dict(id=name, kind=kind, transposed=transposed, kd=kd, stride=2 if kind in ('s2', 'd4') else 1, cin=cin,
                cout=cout, n=n, d=d, h=h, w=w, norm=norm, per_plane=per_plane, two=two, offset=offset, heavy=heavy,
                group='2-D layers' if kind == 'c1' else '3-D layers')


CASES = [
    # ---- strided convolution: conv_s2_bwd_data2 ------------------------------------------------------------------------
    case('s2_8_16_n2_16x62x72', 's2', 8, 16, 2, 16, 62, 72),          # cb8 ocg4 ry1; 1984 units
    case('s2_8_16_n2_16x64x130', 's2', 8, 16, 2, 16, 64, 130),        # cb8 ocg1 segs 2; 4096 units; one live pair in seg 1
    case('s2_8_16_n1_7x9x65', 's2', 8, 16, 1, 7, 9, 65),              # 70 units per channel block: cb4; ocg4; all odd
    case('s2_4_8_n2_9x11x15', 's2', 4, 8, 2, 9, 11, 15),              # ry8; ocg2
    case('s2_4_8_n2_5x7x21', 's2', 4, 8, 2, 5, 7, 21),                # ry4
    case('s2_4_8_n2_5x6x35', 's2', 4, 8, 2, 5, 6, 35),                # ry2
    case('s2_6_8_n2_5x7x13', 's2', 6, 8, 2, 5, 7, 13),                # partial channel block (nch 2)
    case('s2_4_8_n2_5x7x21_2src', 's2', 4, 8, 2, 5, 7, 21, two=True),  # one dx for both sources
    # ---- transposed convolution: deconv_bwd_data2 ------------------------------------------------------------------------
    case('d4_16_8_n2_3x4x33', 'd4', 16, 8, 2, 3, 4, 33),              # cb4 ocg2 ry2; Wo 66: VEC off
    case('d4_16_8_n2_3x4x34', 'd4', 16, 8, 2, 3, 4, 34),              # Wo 68: VEC on
    case('d4_16_8_n2_3x4x34_bare_offset', 'd4', 16, 8, 2, 3, 4, 34, norm=False, offset=True),   # dz misaligned: VEC off
    case('d3_4_1_n2_4x5x18_bare', 'd3', 4, 1, 2, 4, 5, 18, norm=False),   # the up layer: Cout < 8: ocg1; Wo 36: VEC
    # ---- stride 1 through the forward kernels ----------------------------------------------------------------------------
    case('c1_128_64_n2_1x5x33', 'c1', 128, 64, 2, 1, 5, 33, per_plane=1),     # odd width: per entry and block
    case('c1_128_64_n2_1x5x36', 'c1', 128, 64, 2, 1, 5, 36, per_plane=1),     # channel slices, batch 2
    case('c1_64_64_n2_2x5x36', 'c1', 64, 64, 2, 2, 5, 36, per_plane=1),       # certified, W % 4 == 0; in_bwd_plane
    case('c1_64_64_n2_2x6x36_heavy', 'c1', 64, 64, 2, 2, 6, 36, per_plane=1, heavy=True),
    case('c1_64_64_n2_2x6x36_heavy_bare', 'c1', 64, 64, 2, 2, 6, 36, norm=False, heavy=True),
    case('c3_8_8_n2_3x6x34', 'c3', 8, 8, 2, 3, 6, 34),                        # per volume, 612 elements: flattened plane
    case('c3_16_16_n2_3x5x20', 'c3', 16, 16, 2, 3, 5, 20),
    case('c3_16_16_n2_3x5x20_2src', 'c3', 16, 16, 2, 3, 5, 20, two=True),
    # ---- InstanceNorm backward routes ------------------------------------------------------------------------------------
    case('c3_8_8_n2_3x5x7', 'c3', 8, 8, 2, 3, 5, 7),                          # 105 elements: % 4 != 0: two-pass
    case('c3_8_8_n2_5x80x96', 'c3', 8, 8, 2, 5, 80, 96),                      # 38400 > 36864 per volume: two-pass
    case('c1_3_3_n2_1x128x516_pp', 'c1', 3, 3, 2, 1, 128, 516, per_plane=1),  # plane 66048 > 65536: 65 tiles capped at 64
    case('c1_8_3_n2_2x6x8_pp_offset', 'c1', 8, 3, 2, 2, 6, 8, per_plane=1, offset=True),   # g misaligned: two-pass
    # ---- bare layers: channel_sum ------------------------------------------------------------------------------------
    case('c1_8_3_n2_1x96x96_bare', 'c1', 8, 3, 2, 1, 96, 96, norm=False),     # volume 9216: two splits
]


def case_id(c):
    return c['id']


def out_geom(c):
    if c['transposed']:
        return ((2 if c['kd'] == 4 else 1) * c['d'], 2 * c['h'], 2 * c['w'])
    if c['stride'] == 2:
        return ((c['d'] + 1) // 2, (c['h'] + 1) // 2, (c['w'] + 1) // 2)
    return (c['d'], c['h'], c['w'])


def _ceil(a, b):
    return -(-a // b)


def _off(switches, name):
    return switches.get(name, '')[:1] == '0'


# ---- the dispatch, restated ----------------------------------------------------------------------------------------------
def expected_in_bwd_route(c, switches, aligned=True):
    """launch_in_bwd (csrc/backward.hip) -> (probe name, tiles per plane of the two-pass route)."""
    do, ho, wo = out_geom(c)
    plane, depth, per_plane = ho * wo, do, bool(c['per_plane'])
    tiles = min(max(_ceil(plane, 1024), 1), 64)
    if not per_plane and do * plane <= PLANE_LIMIT:     # the flattened view
        plane, depth, per_plane = do * plane, 1, True
    per_plane = per_plane or do == 1
    if (not _off(switches, 'PDS_IN_BWD_PLANE') and per_plane and plane % 4 == 0 and plane <= PLANE_LIMIT and aligned):
        return IN_PLANE, tiles
    return IN_TWOPASS, tiles


def channel_sum_splits(c):
    do, ho, wo = out_geom(c)
    return max(1, min(do * ho * wo // 4096, 2048 // max(c['cout'], 1)))


def expected_bwd_data_variant(c, switches, aligned=True):
    """launch_bwd_data / launch_bwd_data2 (csrc/backward.hip) for a stride-2 convolution or a transposed layer."""
    t, kd = c['transposed'], c['kd']
    if _off(switches, 'PDS_BWD_DATA_V2'):
        name = 'bwd_data1<deconv,k%d>' % kd if t else 'bwd_data1<conv,k3,s2>'
        return dict(name=name, workgroups=_ceil(c['h'] * c['w'], 256) * c['d'] * c['n'] * _ceil(c['cin'], 4))
    pairs, pw = (c['w'] + 1) // 2, 64
    while pw > 8 and pw // 2 >= pairs:
        pw //= 2
    ry, segs = 64 // pw, _ceil(pairs, pw)
    rows = c['h'] if t else (c['h'] + 1) // 2
    yblocks = _ceil(rows, ry)
    cb = 8 if c['cin'] % 8 == 0 else 4
    per_cb = c['n'] * c['d'] * (1 if t else 2) * yblocks * segs
    if cb == 8 and per_cb * (c['cin'] // 8) < 512:
        cb = 4
    units = per_cb * _ceil(c['cin'], cb)
    ocg = 1
    while ocg < 4 and units * ocg < 4096 and c['cout'] >= 8 * ocg:
        ocg *= 2
    vec = bool(t and out_geom(c)[2] % 4 == 0 and aligned)
    name = ('bwd_data2<deconv%d,cb%d,ocg%d,vec%d>' % (kd, cb, ocg, vec)) if t else 'bwd_data2<conv,cb%d,ocg%d>' % (cb, ocg)
    return dict(name=name, pw=pw, ry=ry, segs=segs, yblocks=yblocks, cb=cb, ocg=ocg, units=units, vec=vec,
                workgroups=_ceil(units * ocg, 4))


def dispatch3d(n, cin, cout, d, h, w, certified, switches):
    """conv_block (csrc/api.hip) for a bare stride-1 kd-3 layer on a plain source: conv3d_t8 (8 -> 8; the split kernel
    conv3d_t8x with a certificate), conv3d_ks (Cin = Cout in 16, 32, 64, up to 30 000 voxels; 4 channels per wave = Cin
    16 in the split form with a certificate; ks_plan keeps Cin 128 out at these widths), conv3d_nx (certified 16 -> 16
    from 100 000 voxels), conv3d_mfma (Cin % 4 == 0, Cin >= 8), conv_direct."""
    volume = d * h * w
    if cin == 8 and cout == 8 and not _off(switches, 'PDS_CONV3D_T8'):
        forced = switches.get('PDS_CONV3D_T8X', '')[:1] == '2'
        return T8X if (certified or forced) and not _off(switches, 'PDS_CONV3D_T8X') else T8
    limit = int(switches.get('PDS_CONV3D_KS_LIMIT', 30000))
    if cin in (16, 32, 64) and cout == cin and volume <= limit and not _off(switches, 'PDS_CONV3D_KS'):
        split = cin == 16 and certified and not _off(switches, 'PDS_CONV3D_KSX')
        return KS16 if split else KS32
    if cin == 16 and cout == 16 and certified and volume >= 100000 and not _off(switches, 'PDS_CONV3D_NX'):
        return NX
    return MFMA3 if cin % 4 == 0 and cin >= 8 else DIRECT3


def expected_stride1(c, switches):
    """The stride-1 branch of backward_walk -> {forward probe name: launches} (flip_weights aside)."""
    n, cin, cout, d, h, w = c['n'], c['cin'], c['cout'], c['d'], c['h'], c['w']
    if c['kd'] == 3:
        return {dispatch3d(n, cout, cin, d, h, w, True, switches): 1}

    def kernel2d(batch, channels, certified):
        k = conv2d.dispatch(conv2d.BOUND if certified else conv2d.PLAIN, batch, cout, channels, d, h, w, False, switches)
        return conv2d.T8 if k == conv2d.T8W else k      # (the full-width form wants a normalised source: dz is plain)

    if cin > 64 and cin % 64 == 0:
        if w % 2 == 0 and cout % 4 == 0:
            return {kernel2d(n, 64, True): cin // 64}
        return {kernel2d(1, 64, False): n * (cin // 64)}
    return {kernel2d(n, cin, True): 1}


def expected_counts(c, switches):
    """-> ({probe name: launches} over PROBES, {probe name: workgroups} where the case predicts them)."""
    counts, workgroups = {name: 0 for name in PROBES}, {}
    aligned = not c['offset']
    if c['norm']:
        counts[expected_in_bwd_route(c, switches, aligned)[0]] = 1
    else:
        counts[CHANNEL_SUM] = 1
        workgroups[CHANNEL_SUM] = c['cout'] * channel_sum_splits(c)
    if not c['transposed'] and c['stride'] == 1:
        counts[FLIP] = 1
        for name, launches in expected_stride1(c, switches).items():
            counts[name] += launches
    else:
        # (a bare layer's dz is the caller's gradient; behind an InstanceNorm it is an arena buffer, always aligned)
        v = expected_bwd_data_variant(c, switches, aligned or c['norm'])
        counts[v['name']] = 1
        workgroups[v['name']] = v['workgroups']
    counts[GRAD_ADD] = 2 if c['two'] else 1
    return counts, workgroups


# ---- inputs and the CPU reference --------------------------------------------------------------------------------------
def make_inputs(c):
    """-> dict of CPU fp32 tensors: x, x2 (or None), weight, bias, gamma, beta, up (the upstream gradient)."""
    g = torch.Generator().manual_seed(11000 + [k['id'] for k in CASES].index(c['id']))
    n, cin, cout, d, h, w, kd = c['n'], c['cin'], c['cout'], c['d'], c['h'], c['w'], c['kd']
    if c['transposed']:
        weight = torch.randn(cin, cout, kd, 4, 4, generator=g) / (cin * kd * 4) ** 0.5
    else:
        weight = torch.randn(cout, cin, kd, 3, 3, generator=g) / (cin * kd * 9) ** 0.5
    t = dict(x=torch.randn(n, cin, d, h, w, generator=g), x2=None, weight=weight,
             bias=torch.randn(cout, generator=g) * 0.1, gamma=torch.rand(cout, generator=g) + 0.5,
             beta=torch.randn(cout, generator=g) * 0.2)
    if c['two']:
        t['x2'] = torch.randn(n, cin, d, h, w, generator=g)
    up = torch.randn(n, cout, *out_geom(c), generator=g)
    if c['heavy']:      # in the manner of heavy_tailed_weights (tests/test_gpu_range_safety.py): a few entries ~1e3 x the bulk
        idx = torch.randperm(up.numel(), generator=g)[:12]
        mag = torch.exp(torch.rand(12, generator=g) * (torch.log(torch.tensor(2000.0)) - torch.log(torch.tensor(500.0)))
                        + torch.log(torch.tensor(500.0)))
        up.view(-1)[idx] = mag * (torch.randint(0, 2, (12,), generator=g) * 2 - 1).float()
    t['up'] = up
    return t


def block(c, x, weight, bias, gamma, beta):
    """The block in the dtype of its arguments (reference network_blocks.py:37-85): (transposed) convolution, then --
    with an InstanceNorm -- LeakyReLU and the normalisation over each plane or volume."""
    if c['transposed']:
        z = F.conv_transpose3d(x, weight, bias, stride=(2 if c['kd'] == 4 else 1, 2, 2), padding=1)
    else:
        z = F.conv3d(x, weight, bias, stride=1 if c['kd'] == 1 else c['stride'], padding=(c['kd'] // 2, 1, 1))
    if not c['norm']:
        return z
    t = F.leaky_relu(z, oracle.LEAKY_SLOPE)
    dims = (3, 4) if c['per_plane'] else (2, 3, 4)
    mean = t.mean(dim=dims, keepdim=True)
    var = t.var(dim=dims, unbiased=False, keepdim=True)
    return (t - mean) / torch.sqrt(var + oracle.IN_EPS) * gamma.view(1, -1, 1, 1, 1) + beta.view(1, -1, 1, 1, 1)


def cpu_gradients(c, t, dtype):
    """CPU autograd of sum(block(x + x2) * up) in `dtype` -> {'dx', 'dx2', 'dbias', 'dgamma', 'dbeta'} (fp64 tensors)."""
    leaf = {k: t[k].detach().to(dtype).requires_grad_(True) for k in ('x', 'x2', 'weight', 'bias', 'gamma', 'beta')
            if t[k] is not None}
    x = leaf['x'] + leaf['x2'] if c['two'] else leaf['x']
    (block(c, x, leaf['weight'], leaf['bias'], leaf['gamma'], leaf['beta']) * t['up'].to(dtype)).sum().backward()
    out = {'dx': leaf['x'].grad.double(), 'dbias': leaf['bias'].grad.double()}
    if c['two']:
        out['dx2'] = leaf['x2'].grad.double()
    if c['norm']:
        out['dgamma'], out['dbeta'] = leaf['gamma'].grad.double(), leaf['beta'].grad.double()
    return out


def distance(got, want):
    """(max-relative, mean-relative, mean error relative to the maximum) distance of a gradient from the fp64 one."""
    delta = (got.double() - want).abs()
    top = want.abs().max().clamp_min(1e-30)
    return (float(delta.max() / top), float(delta.mean() / want.abs().mean().clamp_min(1e-30)), float(delta.mean() / top))


_reference = {}


def reference(c):
    """The inputs and both CPU references of a case, computed once and shared (never modified)."""
    if c['id'] not in _reference:
        t = make_inputs(c)
        _reference[c['id']] = (t, cpu_gradients(c, t, torch.float64), cpu_gradients(c, t, torch.float32))
    return _reference[c['id']]


# ---- the GPU side --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def count_launches(lib, name, run, capacity=16):
    """-> (launches whose probe name contains `name` during `run`, their workgroup counts, the result of `run`)."""
    from practicaldeepstereo_nips2018_amd import _lib
    workgroups = (ctypes.c_int * capacity)()
    _lib.check(lib.pds_probe_begin(name.encode(), capacity), 'pds_probe_begin')
    try:
        result = run()
        torch.cuda.synchronize()
    finally:
        count = lib.pds_probe_end(None, workgroups, capacity)
    assert 0 <= count < capacity, lib.pds_last_error()
    return count, list(workgroups[:count]), result


def nan_bytes(count, dev):
    return torch.full((max(int(count), 256),), 0xFF, dtype=torch.uint8, device=dev)


def layer_runner(c, t, dev):
    """Runs the block forward once; -> a closure that runs its backward into fresh NaN-filled buffers."""
    from practicaldeepstereo_nips2018_amd import _lib
    lib = _lib.load()
    stream = _lib.stream_handle(dev)
    g = {k: (v.to(dev).contiguous() if v is not None else None) for k, v in t.items()}
    shape = (int(c['transposed']), c['n'], c['cin'], c['cout'], c['d'], c['h'], c['w'], c['kd'], c['stride'],
             c['per_plane'])
    flags = (int(c['norm']), int(c['two']))
    params = _lib.ConvBlockParams()
    params.weight, params.bias = g['weight'].data_ptr(), g['bias'].data_ptr()
    if c['norm']:
        params.gamma, params.beta = g['gamma'].data_ptr(), g['beta'].data_ptr()
    fws = torch.empty(max(int(lib.pds_conv_block_tape_workspace_bytes(*(shape + flags))), 256), dtype=torch.uint8,
                      device=dev)
    bytes_bwd = int(lib.pds_conv_block_bwd_workspace_bytes(*(shape + flags)))
    assert bytes_bwd > 0, lib.pds_last_error()
    out = torch.full_like(g['up'], float('nan'))
    x2 = _lib.ptr(g['x2']) if c['two'] else None
    _lib.check(lib.pds_conv_block_tape_fwd(ctypes.byref(params), _lib.ptr(g['x']), x2, _lib.ptr(out), *shape,
                                           _lib.ptr(fws), fws.numel(), stream), 'pds_conv_block_tape_fwd')
    torch.cuda.synchronize()
    if c['offset']:     # the upstream gradient as a view one float into its buffer: 4-byte, not 16-byte aligned
        store = torch.empty(g['up'].numel() + 1, device=dev)
        up = store[1:].view_as(g['up'])
        up.copy_(g['up'])
        assert up.data_ptr() % 16 == 4
    else:
        up = g['up']
        assert up.data_ptr() % 16 == 0

    def run():
        bws = nan_bytes(bytes_bwd, dev)
        grads = {k: torch.full_like(g[k], float('nan')) for k in ('weight', 'bias', 'gamma', 'beta', 'x')}
        if c['two']:
            grads['x2'] = torch.full_like(g['x2'], float('nan'))
        gp = _lib.ConvBlockParams()
        gp.weight, gp.bias = grads['weight'].data_ptr(), grads['bias'].data_ptr()
        if c['norm']:
            gp.gamma, gp.beta = grads['gamma'].data_ptr(), grads['beta'].data_ptr()
        _lib.check(lib.pds_conv_block_bwd(ctypes.byref(params), ctypes.byref(gp), _lib.ptr(g['x']), x2, _lib.ptr(up),
                                          _lib.ptr(grads['x']), _lib.ptr(grads['x2']) if c['two'] else None, *shape,
                                          _lib.ptr(fws), fws.numel(), _lib.ptr(bws), bws.numel(), stream),
                   'pds_conv_block_bwd')
        torch.cuda.synchronize()
        got = {'dx': grads['x'], 'dbias': grads['bias'], 'dweight': grads['weight']}
        if c['two']:
            got['dx2'] = grads['x2']
        if c['norm']:
            got['dgamma'], got['dbeta'] = grads['gamma'], grads['beta']
        return got

    return run, out


_worst = {}    # probe name -> (err / gate, case and tensor): printed by the last test


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_dgrad_layer_against_fp64(dev, c):
    from practicaldeepstereo_nips2018_amd import _lib
    lib = _lib.load()
    t, want, theirs = reference(c)
    run, out = layer_runner(c, t, dev)
    nonfinite_before = lib.pds_nonfinite_statistics(0)
    # the forward the tape follows is the block of the reference (not this file's subject: the normalised-output bound
    # of the forward files, 5 x 2e-5, relative to the largest entry)
    x64 = (t['x'].double() + t['x2'].double()) if c['two'] else t['x'].double()
    want_out = block(c, x64, *(t[k].double() for k in ('weight', 'bias', 'gamma', 'beta')))
    assert distance(out.cpu(), want_out)[0] <= 1e-4

    counts, seen_workgroups, first, got = {}, {}, None, None
    for name in PROBES:
        counts[name], seen_workgroups[name], got = count_launches(lib, name, run)
        first = first or got
    switches = active_switches()
    expected, expected_workgroups = expected_counts(c, switches)
    print('dgrad case %s: launches %s' % (c['id'], {k: v for k, v in counts.items() if v}))

    # 1. which kernels ran
    assert counts == expected, 'launches %s, expected %s' % ({k: v for k, v in counts.items() if v},
                                                            {k: v for k, v in expected.items() if v})
    for name, workgroups in expected_workgroups.items():
        assert seen_workgroups[name] == [workgroups], (name, seen_workgroups[name], workgroups)
    # 2. nothing stale; deterministic
    for name in got:
        assert bool(torch.isfinite(got[name]).all()), '%s left unwritten or non-finite' % name
        assert torch.equal(got[name], first[name]), '%s differs between two runs' % name
    assert lib.pds_nonfinite_statistics(0) == nonfinite_before
    if c['two']:
        assert got['dx'].data_ptr() != got['dx2'].data_ptr()
    # 3. values
    served = [k for k in conv2d.FAMILIES + FORWARD3D if counts[k]] or [k for k in DATA1 + DATA2 if counts[k]]
    norm_route = [k for k in (IN_PLANE, IN_TWOPASS, CHANNEL_SUM) if counts[k]]
    split = any(k in SPLIT_FORWARD for k in served)
    floor, floor_mean = F_FLOOR[c['group']], F_MEAN[c['group']]
    failures = []
    for name in sorted(want):
        err, err_mean, err_mean_top = distance(got[name].cpu(), want[name])
        e32, e32_mean, e32_mean_top = distance(theirs[name], want[name])
        dx = name.startswith('dx')
        if dx and split:
            gate, second, gate_second = max(REL_TOL, 3.0 * e32), err_mean_top, max(REL_TOL_MEAN, 3.0 * e32_mean_top)
        else:
            gate, second, gate_second = max(floor, 3.0 * e32), err_mean, max(floor_mean, 3.0 * e32_mean)
        print('    %-7s %-34s err %.2e  e32 %.2e  gate %.2e  x%.2f   mean %.2e (fp32 %.2e, gate %.2e)'
              % (name, '+'.join(served if dx else norm_route), err, e32, gate, err / gate, second,
                 e32_mean_top if dx and split else e32_mean, gate_second))
        for kernel in (served if dx else norm_route):
            ratio = max(err / gate, second / gate_second if dx else 0.0)
            if ratio > _worst.get(kernel, (0.0, ''))[0]:
                _worst[kernel] = (ratio, c['id'] + ' ' + name)
        if not err <= gate:
            failures.append((name, err, gate))
        if dx and not second <= gate_second:
            failures.append((name + ' mean', second, gate_second))
    assert not failures, failures


def test_zz_report_worst_ratio_per_kernel(dev):
    """Prints, per probe name, the largest err / gate seen by the cases above (nothing to assert beyond what they did)."""
    for kernel in sorted(_worst):
        print('worst err / gate  %-36s x%.2f  (%s)' % ((kernel,) + _worst[kernel]))
    assert all(ratio <= 1.0 for ratio, _ in _worst.values())
