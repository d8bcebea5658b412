"""GPU (-m gpu): the fused Matching forward (pds_matching_fwd, csrc/api_matching.hip matching_pipeline) at every
configuration and plane-range edge it branches on, against the fp64 oracle, with the route proved by launch probes.

pds_matching_workspace_bytes / pds_matching_fwd are called through ctypes; the test owns every buffer.  Parameters come
from helpers.seeded(lambda: pds.MatchingOperation(2 * F, F, S, R), seed).native_params(), the descriptors from a seeded
CPU generator (the batch entries differ), weights_resident = 0.  Reference: oracle.matching over
oracle.matching_operation(..., number_of_residual_blocks=R) in fp64 on the CPU, restricted to the planes of the case.

Every case of CASES (F, S, R, batch, h, w, d_begin, d_count)
  1. route: counts the launches of every name of PROBES, one run per name, and asserts exactly the counts
     `expected_route` predicts -- a Python restatement of matching_pipeline's predicates (fused, columns, cb8_level, the
     block walk) and of conv_block's dispatch order (csrc/api.hip), rider suffixes included, under the switches of the
     process (active_switches), so the file can run under tests/test_gpu_switches.py;
  2. initialisation: workspace pre-filled with 0xFF bytes, output with NaN, before each run: everything finite afterwards,
     pds_nonfinite_statistics does not move, two runs agree bit for bit, a run on a zero-filled workspace agrees bit for
     bit, and the guard bytes behind the workspace_bytes the library asked for are untouched;
  3. values: err = max|out - ref64| / max(1, max|ref64|) <= max(REL_TOL, 3 * e32) and
     mean|out - ref64| / max(1, max|ref64|) <= max(REL_TOL_MEAN, 3 * e32_mean), REL_TOL / REL_TOL_MEAN the Matching-chain
     figures of tests/test_gpu_range_safety.py (2e-5, 6e-7), e32 the same distances of the CPU fp32 oracle of the case,
     computed here at run time against the reference, never against the HIP output.
test_shards_concatenate_to_the_whole_range: concatenated shards equal the whole range bit for bit.

Words of the workspace that a kernel reads before "its own" launch writes them (read off the launchers, not found by
running): the only counters in the Matching arena are the nine tile-queue words behind conv2d_x3's packed weights
(csrc/conv2d_x3.hip launch_conv2d_x3: "A.queue = L.packed + total", nine atomics per launch, reset by the last workgroup to
leave).  With weights_resident = 0 every conv2d_x3 layer pushes a pack job of total + 16 words in the collect walk and
multi_pack_kernel zeroes words total .. total + 11 (csrc/pack.hip: "e >= J.total - 16"), pack_wscale_kernel writes 12 / 13,
all in the one packing launch that precedes the first layer; words 14 / 15 are never read.  conv2d_t8 / conv2d_t8w,
the Winograd kernels, conv2d_mfma and the glue kernels partition their work statically: no persistent-tile counter.
g2buf is read at unwritten columns by l1_column_terms (has_d false), conv2d_mfma SRC 2 / 3 and materialize_l0 (disparity
beyond w): every such load is discarded by a select before use.

Found while reading: with d_begin > 0 at a cb8 shape the run walk carved (d_begin + d_count) padding columns for the
blocked H rows where the planning walk (no d_begin) had counted d_count, and wrote past workspace_bytes;
matching_pipeline now forms t1 on the fly only for d_begin == 0 (level 1 is bit-identical).  The shard test holds that
at 16 x 32 with the guard bytes.

e32 floors (tools/matching_e32_floors.py on the CPU: max-relative | mean-relative distance of the fp32 oracle from fp64,
|ref| max, seconds for both oracles):
  planes_f64_s8_r2_n1_4x72_d0+66       e32 9.0e-07 | 1.1e-07   |ref| max  4.55   gates 2.0e-05 | 6.0e-07    1.3 s
  planes_f64_s8_r2_n1_16x32_d0+66      e32 6.6e-07 | 9.1e-08   |ref| max  4.62   gates 2.0e-05 | 6.0e-07    0.3 s
  planes_f64_s8_r2_n2_16x16_d0+6       e32 6.4e-07 | 1.1e-07   |ref| max  3.77   gates 2.0e-05 | 6.0e-07    0.0 s
  planes_f64_s8_r2_n1_70x6_d0+4        e32 6.2e-07 | 1.1e-07   |ref| max  3.90   gates 2.0e-05 | 6.0e-07    0.0 s
  planes_f64_s8_r2_n2_9x21_d3+4        e32 7.4e-07 | 1.2e-07   |ref| max  3.35   gates 2.0e-05 | 6.0e-07    0.0 s
  planes_f64_s8_r2_n1_6x4_d7+3         e32 6.6e-07 | 1.9e-07   |ref| max  2.69   gates 2.0e-05 | 6.0e-07    0.0 s
  planes_f64_s8_r2_n1_5x7_d6+4         e32 8.3e-07 | 1.9e-07   |ref| max  2.94   gates 2.0e-05 | 6.0e-07    0.0 s
  planes_f64_s8_r2_n1_5x7_d1+1         e32 8.7e-07 | 2.0e-07   |ref| max  2.51   gates 2.0e-05 | 6.1e-07    0.0 s
  planes_f64_s8_r2_n1_3x1_d0+3         e32 7.0e-06 | 1.7e-06   |ref| max  1.03   gates 2.1e-05 | 5.1e-06    0.0 s
  blocks_f64_s8_r0_n1_9x21_d0+7        e32 4.5e-07 | 6.6e-08   |ref| max  1.24   gates 2.0e-05 | 6.0e-07    0.0 s
  blocks_f64_s8_r0_n1_16x64_d0+7       e32 3.2e-07 | 5.2e-08   |ref| max  1.48   gates 2.0e-05 | 6.0e-07    0.0 s
  blocks_f64_s8_r1_n2_9x21_d0+7        e32 5.6e-07 | 8.3e-08   |ref| max  2.91   gates 2.0e-05 | 6.0e-07    0.0 s
  blocks_f64_s8_r1_n1_16x32_d0+7       e32 5.7e-07 | 9.5e-08   |ref| max  2.67   gates 2.0e-05 | 6.0e-07    0.0 s
  blocks_f64_s8_r3_n1_9x21_d0+7        e32 8.8e-07 | 1.6e-07   |ref| max  4.38   gates 2.0e-05 | 6.0e-07    0.0 s
  blocks_f64_s8_r3_n2_16x32_d0+7       e32 6.9e-07 | 1.1e-07   |ref| max  5.36   gates 2.0e-05 | 6.0e-07    0.1 s
  blocks_f64_s8_r4_n1_16x16_d0+6       e32 1.0e-06 | 1.7e-07   |ref| max  5.66   gates 2.0e-05 | 6.0e-07    0.0 s
  widths_f8_s8_r2_n2_9x21_d0+7         e32 4.4e-07 | 6.4e-08   |ref| max  4.60   gates 2.0e-05 | 6.0e-07    0.0 s
  widths_f16_s8_r1_n1_9x21_d0+7        e32 7.2e-07 | 1.1e-07   |ref| max  2.62   gates 2.0e-05 | 6.0e-07    0.0 s
  widths_f12_s8_r2_n1_9x21_d0+7        e32 7.6e-07 | 1.0e-07   |ref| max  3.73   gates 2.0e-05 | 6.0e-07    0.0 s
  widths_f64_s64_r0_n1_9x20_d0+5       e32 6.0e-07 | 6.3e-08   |ref| max  1.32   gates 2.0e-05 | 6.0e-07    0.0 s
  widths_f64_s64_r1_n1_9x21_d0+5       e32 8.6e-07 | 1.0e-07   |ref| max  3.04   gates 2.0e-05 | 6.0e-07    0.0 s
  widths_f64_s16_r2_n1_9x21_d0+7       e32 8.1e-07 | 1.3e-07   |ref| max  4.04   gates 2.0e-05 | 6.0e-07    0.0 s
  widths_f32_s8_r2_n1_6x10_d0+4        e32 9.6e-07 | 1.7e-07   |ref| max  3.17   gates 2.0e-05 | 6.0e-07    0.0 s
    largest e32 7.00e-06 | 1.69e-06: 3 * e32 exceeds the flat 2e-05 | 6e-07 of the Matching chain; both oracles of the whole table: 2.2 s
so the flat figures govern every case but w = 1, whose InstanceNorm planes hold three values each (3 x 1): there the gate
follows the fp32 oracle's own distance.
Measured on an MI355X in a default process (every case on the route `expected_route` predicts; e32 as computed on that host
at run time, which is why the gate is not taken from the table above):
  planes_f64_s8_r2_n1_4x72_d0+66       err 8.46e-07 (e32 6.11e-07)   mean 1.15e-07 (e32 9.00e-08)
  planes_f64_s8_r2_n1_16x32_d0+66      err 8.91e-07 (e32 6.62e-07)   mean 1.24e-07 (e32 9.05e-08)
  planes_f64_s8_r2_n2_16x16_d0+6       err 1.04e-06 (e32 6.38e-07)   mean 1.56e-07 (e32 1.10e-07)
  planes_f64_s8_r2_n1_70x6_d0+4        err 8.36e-07 (e32 6.17e-07)   mean 1.48e-07 (e32 1.05e-07)
  planes_f64_s8_r2_n2_9x21_d3+4        err 1.15e-06 (e32 7.39e-07)   mean 1.97e-07 (e32 1.18e-07)
  planes_f64_s8_r2_n1_6x4_d7+3         err 7.25e-07 (e32 6.85e-07)   mean 1.80e-07 (e32 1.90e-07)
  planes_f64_s8_r2_n1_5x7_d6+4         err 1.13e-06 (e32 7.27e-07)   mean 2.31e-07 (e32 1.60e-07)
  planes_f64_s8_r2_n1_5x7_d1+1         err 1.32e-06 (e32 8.79e-07)   mean 2.58e-07 (e32 1.88e-07)
  planes_f64_s8_r2_n1_3x1_d0+3         err 1.02e-05 (e32 1.86e-05)   mean 2.42e-06 (e32 3.51e-06)
  blocks_f64_s8_r0_n1_9x21_d0+7        err 9.32e-07 (e32 4.12e-07)   mean 9.42e-08 (e32 5.92e-08)
  blocks_f64_s8_r0_n1_16x64_d0+7       err 1.27e-06 (e32 3.25e-07)   mean 9.98e-08 (e32 5.22e-08)
  blocks_f64_s8_r1_n2_9x21_d0+7        err 9.78e-07 (e32 5.58e-07)   mean 1.50e-07 (e32 8.28e-08)
  blocks_f64_s8_r1_n1_16x32_d0+7       err 1.09e-06 (e32 5.66e-07)   mean 1.44e-07 (e32 9.46e-08)
  blocks_f64_s8_r3_n1_9x21_d0+7        err 1.48e-06 (e32 9.85e-07)   mean 2.03e-07 (e32 1.41e-07)
  blocks_f64_s8_r3_n2_16x32_d0+7       err 9.35e-07 (e32 6.89e-07)   mean 1.49e-07 (e32 1.08e-07)
  blocks_f64_s8_r4_n1_16x16_d0+6       err 1.05e-06 (e32 9.98e-07)   mean 1.72e-07 (e32 1.41e-07)
  widths_f8_s8_r2_n2_9x21_d0+7         err 4.93e-07 (e32 4.43e-07)   mean 6.04e-08 (e32 6.45e-08)
  widths_f16_s8_r1_n1_9x21_d0+7        err 8.04e-07 (e32 6.66e-07)   mean 9.26e-08 (e32 9.38e-08)
  widths_f12_s8_r2_n1_9x21_d0+7        err 7.16e-07 (e32 5.94e-07)   mean 9.45e-08 (e32 9.44e-08)
  widths_f64_s64_r0_n1_9x20_d0+5       err 8.73e-07 (e32 4.32e-07)   mean 1.02e-07 (e32 5.71e-08)
  widths_f64_s64_r1_n1_9x21_d0+5       err 1.19e-06 (e32 6.00e-07)   mean 1.43e-07 (e32 8.71e-08)
  widths_f64_s16_r2_n1_9x21_d0+7       err 1.14e-06 (e32 7.81e-07)   mean 1.72e-07 (e32 1.11e-07)
  widths_f32_s8_r2_n1_6x10_d0+4        err 8.92e-07 (e32 6.76e-07)   mean 1.66e-07 (e32 1.25e-07)
"""
import ctypes

import pytest
import torch

from oracle import pds_oracle as oracle
from tests import helpers
from tests import test_gpu_conv2d_layers as conv2d
from tests.test_gpu_conv3d_layers import active_switches
from tests.test_gpu_range_safety import REL_TOL, REL_TOL_MEAN

pytestmark = pytest.mark.gpu

# ---- probe names ---------------------------------------------------------------------------------------------------------
L0_STACK, L0_COLFIX, L1_COLTERMS, L1_BLOCKED, L1_STACK = ('l0_stack_inputs', 'l0_column_fix', 'l1_column_terms',
                                                          'l1_blocked', 'l1_stack_inputs')
L0_COMBINE, PAD_LEFT1 = 'l0_combine<fwd>', 'pad_left1'
L1_PLANES, L1_COLS_STORE, L1_COLS_STATS = 'l1_combine<planes>', 'l1_combine<cols,store>', 'l1_combine<cols,stats>'
MAT_SUM, MAT_L0 = 'materialize<sum>', 'materialize_l0'
GLUE = (L0_STACK, L0_COLFIX, L1_COLTERMS, L1_BLOCKED, L1_STACK, L0_COMBINE, PAD_LEFT1, L1_PLANES, L1_COLS_STORE,
        L1_COLS_STATS, MAT_SUM, MAT_L0)
X3F_FORMS = tuple('%s[%s>%s]' % (conv2d.X3F, i, o) for i in ('p', 'cb8', 'l1') for o in ('p', 'cb8'))
MFMA_FORMS = tuple('%s[%s]' % (mb, src) for mb in (conv2d.MB1, conv2d.MB4) for src in ('a', 'a+b', 'l0', 'a+l0'))
# (the probe matches by substring: no name of PROBES contains another -- tests/test_matching_routes_host.py)
PROBES = GLUE + X3F_FORMS + MFMA_FORMS + (conv2d.X3B, conv2d.W4, conv2d.W6, conv2d.W16, conv2d.T8W, conv2d.T8,
                                          conv2d.DIRECT)

# ---- the case table: (group, F, S, R, batch, h, w, d_begin, d_count, the branch it reaches) ------------------------------
CASES = [
    ('planes', 64, 8, 2, 1, 4, 72, 0, 66, 'second l1_combine launch with d0 = 64 inside the image; columns, planar'),
    ('planes', 64, 8, 2, 1, 16, 32, 0, 66, 'cb8 level 2 across two launches; planes with d > w + 1; pad 66 > w'),
    ('planes', 64, 8, 2, 2, 16, 16, 0, 6, 'smallest cb8 shape, batch 2'),
    ('planes', 64, 8, 2, 1, 70, 6, 0, 4, 'h > 64: corr0 spills into a second workgroup; w % 4 != 0 store path'),
    ('planes', 64, 8, 2, 2, 9, 21, 3, 4, 'shard without d = 0'),
    ('planes', 64, 8, 2, 1, 6, 4, 7, 3, 'shard wholly beyond w + 1 (count == 0, zeroing must still happen)'),
    ('planes', 64, 8, 2, 1, 5, 7, 6, 4, 'd = 6..9 straddles w and w + 1'),
    ('planes', 64, 8, 2, 1, 5, 7, 1, 1, 'the single plane d = 1'),
    ('planes', 64, 8, 2, 1, 3, 1, 0, 3, 'w = 1'),
    ('blocks', 64, 8, 0, 1, 9, 21, 0, 7, 'conv2d_mfma<mb1> SRC 2, odd width'),
    ('blocks', 64, 8, 0, 1, 16, 64, 0, 7, 'the same where the default operation would take conv2d_t8w'),
    ('blocks', 64, 8, 1, 2, 9, 21, 0, 7, 'SRC 3, planar'),
    ('blocks', 64, 8, 1, 1, 16, 32, 0, 7, 'SRC 3 behind the on-the-fly first 64 -> 64 launch'),
    ('blocks', 64, 8, 3, 1, 9, 21, 0, 7, 'buffer rotation, planar'),
    ('blocks', 64, 8, 3, 2, 16, 32, 0, 7, 'buffer rotation with out_cb8'),
    ('blocks', 64, 8, 4, 1, 16, 16, 0, 6, 'the rotation goes round a second time'),
    ('widths', 8, 8, 2, 2, 9, 21, 0, 7, 'column form, one output-channel group'),
    ('widths', 16, 8, 1, 1, 9, 21, 0, 7, 'column form, SRC 3'),
    ('widths', 12, 8, 2, 1, 9, 21, 0, 7, 'fused, whole-plane form in a default process'),
    ('widths', 64, 64, 0, 1, 9, 20, 0, 5, 'conv2d_mfma<mb4> SRC 2 on an even width (Winograd must decline)'),
    ('widths', 64, 64, 1, 1, 9, 21, 0, 5, 'conv2d_mfma<mb4> SRC 3'),
    ('widths', 64, 16, 2, 1, 9, 21, 0, 7, 'conv2d_mfma<mb1> SRC 1'),
    ('widths', 32, 8, 2, 1, 6, 10, 0, 4, 'unfused sequence (l0_combine, pad_left1, conv_direct)'),
]

# (F, S, R, batch, h, w, planes, shards as (d_begin, d_count))
SHARD_CASES = [
    (64, 8, 2, 1, 9, 21, 12, ((0, 5), (5, 7))),
    (64, 8, 2, 1, 4, 72, 66, ((0, 64), (64, 2))),     # the l1_combine launch boundary and the shard boundary coincide
    (64, 8, 2, 1, 4, 72, 66, ((0, 33), (33, 33))),    # ... and fall differently
    (8, 8, 2, 1, 9, 21, 8, ((0, 3), (3, 5))),
    (64, 8, 2, 1, 16, 32, 16, ((0, 8), (8, 8))),      # cb8 shape: a shard with d_begin > 0 must stay inside its workspace
]

GUARD_BYTES = 1 << 16


def case_id(c):
    return '%s_f%d_s%d_r%d_n%d_%dx%d_d%d+%d' % c[:9]


def shard_id(c):
    return 'f%d_s%d_r%d_n%d_%dx%d_%dplanes_%s' % (c[:7] + ('_'.join('%d+%d' % s for s in c[7]),))


def _ceil(a, b):
    return -(-a // b)


# ---- the route, restated -------------------------------------------------------------------------------------------------
def conv_name(switches, n, cin, cout, d, h, w, affine, a='plain', b=None, l0=False, sets=0, extras=False, x3_in='p',
              x3_out='p'):
    """conv_block's kernel choice (csrc/api.hip: conv2d_t8, then conv2d_x3 unless the layer carries Matching extras, then
    conv2d_mfma -- in the Winograd domain where conv2d_wino_eligible -- else conv_direct) -> the probe name of the launch.
    a: None (layer-0 terms only) | 'plain' (no certificate) | 'bounded' (plain, certified) | 'normed' (deferred
    InstanceNorm, certified); b: None | 'bounded' (the plain residual sum)."""

    def off(name):
        return switches.get(name, '')[:1] == '0'

    a_bounded, a_scale = a in ('bounded', 'normed'), a == 'normed'
    # conv2d_t8_supported (+ "no statistics wanted") and c2t8_wide
    if (not affine and not off('PDS_CONV2D_T8') and cin == 64 and cout == 8 and not l0 and sets == 0 and a_bounded
            and n * 64 * d * h * w < 1 << 29 and n * d * _ceil(h, 16) * _ceil(w, 32) < 1 << 30):
        wide = not off('PDS_CONV2D_T8W') and a_scale and w % 4 == 0 and 64 <= w <= 352 and h >= 8
        return conv2d.T8W if wide else conv2d.T8
    # conv2d_x3_supported and x3_use_fp16
    if (not extras and not off('PDS_X3') and cout == 64 and cin % 16 == 0 and 48 <= cin <= 256 and b is None and not l0
            and sets == 0 and d * h * w * 8 < 1 << 30 and n * d < 1 << 20):
        if a_bounded and not off('PDS_X3_FP16'):
            return '%s[%s>%s]' % (conv2d.X3F, x3_in, x3_out)
        return conv2d.X3B
    # conv2d_mfma_supported
    if (cin % 4 == 0 and cin <= 256 and (cout == 64 or cout <= 16) and 4 * d * h * w < 1 << 31 and d <= 65535
            and n <= 65535 and not (l0 and h * (w + 2) * cin >= 1 << 31)):
        # conv2d_wino_eligible
        if (not off('PDS_WINOGRAD') and cout == 64 and b is None and not l0 and (sets == 0 or (sets == d and sets <= 8))
                and w % 2 == 0 and w >= 2):
            if conv2d.wino16_preferred(h, w, switches):
                return conv2d.W16
            return conv2d.W6 if conv2d.wino_rows(n, d, h, w, switches) == 6 else conv2d.W4
        src = ('l0' if a is None else 'a+l0') if l0 else ('a+b' if b else 'a')
        return '%s[%s]' % (conv2d.MB4 if cout == 64 else conv2d.MB1, src)
    assert not extras, 'conv_block: fused Matching extras need the conv2d MFMA kernel'
    return conv2d.DIRECT


def mfma_supported(cin, cout, n, d, h, w):
    return (cin % 4 == 0 and cin <= 256 and (cout == 64 or cout <= 16) and 4 * d * h * w < 1 << 31 and d <= 65535
            and n <= 65535)


def expected_route(case, switches):
    """matching_pipeline (inference walk) -> ({probe name: launches} over PROBES, facts for the printout)."""
    _, F, S, R, n, h, w, d0, dc, _ = case
    counts = {name: 0 for name in PROBES}

    def off(name):
        return switches.get(name, '')[:1] == '0'

    def launch(name, times=1):
        counts[name] += times

    def conv(*args, **kwargs):
        launch(conv_name(switches, *args, **kwargs))

    fused = (not off('PDS_MATCHING_FUSED') and mfma_supported(F, F, n, dc, h, w) and mfma_supported(F, S, n, dc, h, w))
    columns = not off('PDS_MATCHING_COLUMNS') and fused and R >= 1 and F % 8 == 0
    l0_planes, l0_pad = (2, 2) if columns else (3, 1)
    facts = dict(fused=fused, columns=columns, cb8_level=0, on_the_fly=False)
    launch(L0_STACK)
    if fused:
        conv(n, F, F, l0_planes, h, w + l0_pad, False, sets=l0_planes, extras=True)
    else:
        for _ in range(3):
            launch(PAD_LEFT1)
            conv(n, F, F, 1, h, w + 1, False)
    if columns:
        launch(L0_COLFIX)        # (two padding columns of A to zero even where no plane of the call reads G2)
    if not fused:
        # operation_tail on the stored x0 (plain, certified by l0_combine)
        launch(L0_COMBINE)
        cur = 'bounded'
        for r in range(R):
            conv(n, F, F, dc, h, w, True, a=cur)
            conv(n, F, F, dc, h, w, True, a='normed')
            if r + 1 < R:
                launch(MAT_SUM)
                cur = 'bounded'
        if R > 0:
            conv(n, F, S, dc, h, w, False, a='normed', b='bounded')
        else:
            conv(n, F, S, dc, h, w, False, a='bounded')
        return counts, facts
    if R == 0:
        conv(n, F, S, dc, h, w, False, a=None, l0=True, extras=True)
        return counts, facts
    # cb8_level: channel-blocked tensors need F = 64, whole 16 x 16 tiles and conv2d_x3 in its fp16 form
    level = int(switches.get('PDS_MATCHING_CB8', 2))
    x3_fp16 = conv_name(switches, n, F, F, dc, h, w, True, a='bounded').startswith(conv2d.X3F)
    cb8_level = level if (F == 64 and h % 16 == 0 and w % 16 == 0 and x3_fp16) else 0
    if columns:
        per_row = dc - (1 if d0 == 0 else 0)
        if _ceil(h * per_row, 64) + (_ceil(h, 64) if d0 == 0 else 0) > 0:
            launch(L1_COLTERMS)
        conv(n, F, F, 2, h, w + 2, False, sets=2, extras=True)
    else:
        launch(L1_STACK)
        conv(n, 2 * F, F, 5, h, w + 2, False, sets=5, extras=True)
    on_the_fly = columns and cb8_level >= 2 and d0 == 0
    if on_the_fly:
        launch(L1_BLOCKED)
    launch(L1_COLS_STATS if on_the_fly else L1_COLS_STORE if columns else L1_PLANES, _ceil(dc, 64))
    facts.update(cb8_level=cb8_level, on_the_fly=on_the_fly)
    conv(n, F, F, dc, h, w, True, a='normed', x3_in='l1' if on_the_fly else 'p')
    if R == 1:
        conv(n, F, S, dc, h, w, False, a='normed', l0=True, extras=True)
        return counts, facts
    launch(MAT_L0)
    for r in range(1, R):
        blocked = cb8_level >= 1
        conv(n, F, F, dc, h, w, True, a='bounded', x3_out='cb8' if blocked else 'p')
        conv(n, F, F, dc, h, w, True, a='normed', x3_in='cb8' if blocked else 'p')
        if r + 1 < R:
            launch(MAT_SUM)
    conv(n, F, S, dc, h, w, False, a='normed', b='bounded')
    return counts, facts


# ---- inputs and the CPU references ---------------------------------------------------------------------------------------
def make_operation(F, S, R, seed):
    import practicaldeepstereo_nips2018_amd as pds
    return helpers.seeded(lambda: pds.MatchingOperation(2 * F, F, S, R), seed)


def make_inputs(F, n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, F, h, w, generator=g), torch.randn(n, F, h, w, generator=g)


def cpu_signatures(op, R, left, right, d0, dc, dtype):
    p = {k: v.to(dtype) for k, v in helpers.prefixed(op.state_dict(), 'op').items()}
    with torch.no_grad():
        return oracle.matching(left.to(dtype), right.to(dtype), d0 + dc - 1,
                               lambda x: oracle.matching_operation(p, 'op', x, number_of_residual_blocks=R),
                               plane_range=(d0, dc))


def distance(got, want):
    """(max, mean) of |got - want| relative to max(1, max|want|)."""
    delta = (got.double() - want).abs()
    top = max(1.0, float(want.abs().max()))
    return float(delta.max()) / top, float(delta.mean()) / top


_reference = {}


def reference(case):
    """(operation, left, right, fp64 signatures, (e32, e32_mean)) of a case, computed once and never modified."""
    key = case_id(case)
    if key not in _reference:
        _, F, S, R, n, h, w, d0, dc, _ = case
        index = [case_id(c) for c in CASES].index(key)
        op = make_operation(F, S, R, 100 + index)
        left, right = make_inputs(F, n, h, w, 200 + index)
        want = cpu_signatures(op, R, left, right, d0, dc, torch.float64)
        _reference[key] = (op, left, right, want,
                           distance(cpu_signatures(op, R, left, right, d0, dc, torch.float32), want))
    return _reference[key]


# ---- the GPU side --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def count_launches(lib, name, run, capacity=32):
    from practicaldeepstereo_nips2018_amd import _lib
    _lib.check(lib.pds_probe_begin(name.encode(), capacity), 'pds_probe_begin')
    try:
        result = run()
        torch.cuda.synchronize()
    finally:
        count = lib.pds_probe_end(None, None, capacity)
    assert 0 <= count < capacity, lib.pds_last_error()
    return count, result


def matching_runner(op, left, right, dev):
    """-> run(d_begin, d_count, fill): one pds_matching_fwd into a NaN-filled output and a workspace of exactly the bytes
    the library asks for, every byte `fill`, followed by GUARD_BYTES of the same; returns (signatures, guard intact)."""
    from practicaldeepstereo_nips2018_amd import _lib
    lib = _lib.load()
    op = op.to(dev)
    params, keep = op.native_params()
    lg, rg = left.to(dev).contiguous(), right.to(dev).contiguous()
    n, _, h, w = left.shape
    S = op.number_of_signature_features

    def run(d0, dc, fill=0xFF):
        need = int(lib.pds_matching_workspace_bytes(ctypes.byref(params), n, h, w, dc))
        assert need > 0, lib.pds_last_error()
        ws = torch.full((need + GUARD_BYTES,), fill, dtype=torch.uint8, device=dev)
        out = torch.full((n, S, dc, h, w), float('nan'), device=dev)
        _lib.check(lib.pds_matching_fwd(ctypes.byref(params), _lib.ptr(lg), _lib.ptr(rg), _lib.ptr(out), n, h, w, d0, dc,
                                        _lib.ptr(ws), need, 0, _lib.stream_handle(dev)), 'pds_matching_fwd')
        torch.cuda.synchronize()
        return out, bool((ws[need:] == fill).all()), (op, keep, lg, rg)   # (params points into the module's tensors)

    return run


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_matching_route_against_fp64(dev, case):
    from practicaldeepstereo_nips2018_amd import _lib
    lib = _lib.load()
    _, F, S, R, n, h, w, d0, dc, note = case
    op, left, right, want, (e32, e32_mean) = reference(case)
    run = matching_runner(op, left, right, dev)
    nonfinite_before = lib.pds_nonfinite_statistics(0)

    counts, first, out = {}, None, None
    for name in PROBES:
        counts[name], (out, guard_intact, _) = count_launches(lib, name, lambda: run(d0, dc))
        assert guard_intact, 'a kernel wrote behind the workspace_bytes the library asked for (probe run %s)' % name
        first = out if first is None else first
    expected, facts = expected_route(case, active_switches())
    seen = {k: v for k, v in counts.items() if v}
    finite = bool(torch.isfinite(out).all())
    err, err_mean = distance(out.cpu(), want) if finite else (float('nan'), float('nan'))
    gate, gate_mean = max(REL_TOL, 3.0 * e32), max(REL_TOL_MEAN, 3.0 * e32_mean)
    print('matching route %s (%s): %s  launches %s  err %.2e (e32 %.2e, gate %.2e)  mean %.2e (e32 %.2e, gate %.2e)'
          % (case_id(case), note, facts, seen, err, e32, gate, err_mean, e32_mean, gate_mean))

    # 1. route
    assert counts == expected, 'launches %s, expected %s' % (seen, {k: v for k, v in expected.items() if v})
    # 2. initialisation
    assert out.shape == want.shape
    assert finite, 'output positions left unwritten or non-finite'
    assert lib.pds_nonfinite_statistics(0) == nonfinite_before
    assert torch.equal(out, first), 'two runs differ'
    zeroed, guard_intact, _ = run(d0, dc, fill=0)
    assert guard_intact
    assert torch.equal(zeroed, out), 'the result depends on what the workspace held before the call'
    # 3. values
    assert err <= gate, (err, gate)
    assert err_mean <= gate_mean, (err_mean, gate_mean)


@pytest.mark.parametrize('case', SHARD_CASES, ids=shard_id)
def test_shards_concatenate_to_the_whole_range(dev, case):
    """the planes are independent, so shards computed by separate calls and concatenated equal the whole
    range bit for bit -- also where a shard boundary falls on or beside l1_combine's 64-plane launch boundary."""
    F, S, R, n, h, w, planes, shards = case
    index = SHARD_CASES.index(case)
    run = matching_runner(make_operation(F, S, R, 300 + index), *make_inputs(F, n, h, w, 400 + index), dev)
    whole, guard_intact, _ = run(0, planes)
    assert guard_intact and bool(torch.isfinite(whole).all())
    assert sum(count for _, count in shards) == planes
    parts = []
    for begin, count in shards:
        part, guard_intact, _ = run(begin, count)
        assert guard_intact, 'shard (%d, %d) wrote behind the workspace_bytes the library asked for' % (begin, count)
        parts.append(part)
    assert torch.equal(torch.cat(parts, dim=2), whole)
