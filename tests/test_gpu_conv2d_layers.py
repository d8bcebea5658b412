"""GPU (-m gpu): every 2-D convolution kernel behind conv_block alone, one layer at a time, against an fp64 convolution.

One block of MatchingOperation / Embedding (Conv2d 3 x 3 -> LeakyReLU(0.1) -> InstanceNorm2d, reference
network_blocks.py:47-58; kernel depth 1, so the D axis is a stack of independent planes) through the three ways a layer
is entered:
  plain           pds_conv_block_fwd on a plain tensor of unknown range;
  chained         pds_conv_block_chained_fwd: the input sits behind a deferred InstanceNorm (raw producer output x 37 + 5,
                  the loader applies the folded coefficients x^ = scale * x + shift, per (n, c) or per (n, c, d));
  chained+bound   ... with the range certificate x_bound = max |x^| that lets the fp16-split forms run.

Every case
  1. counts the launches of all ten 2-D kernel families with the launch probe and asserts that the intended one -- and
     no other -- ran (a layer that silently lands on a fallback passes every numeric check);
  2. pre-fills the output and the coefficient outputs with NaN and asserts that none is left and everything is finite;
  3. compares the raw output with an fp64 F.conv2d of x^ (+ LeakyReLU(0.1) when the block has an InstanceNorm) and, then,
     the normalised output scale * raw + shift;
  4. compares the returned folded coefficients with the fp64 statistics, per plane or per volume as the case says.

Dispatch (csrc/api.hip conv_block, in this order; `dispatch` below restates the predicates):
  conv2d_t8      bare (no InstanceNorm behind it) 64 -> 8 layers whose source carries a range certificate: the full-width
                 form conv2d_t8w for a normalised source on rows of 64 .. 352 columns, W % 4 == 0, H >= 8 (c2t8_wide; 6-row
                 tiles up to W = 256, 8-row tiles beyond, c2t8w_rows), else tiles of 16 x 32 (conv2d_t8<tile>);
  conv2d_x3      Cin % 16 == 0, 48 <= Cin <= 256, Cout == 64 (conv2d_x3_supported): <fp16> with a certificate, else <bf16>;
  conv2d_mfma    Cin % 4 == 0, Cin <= 256, Cout == 64 or Cout <= 16 (conv2d_mfma_supported).  Cout == 64 on an even width
                 runs in the Winograd domain (conv2d_wino_eligible): conv2d_wino16 where 16 x 16 tiles cover the plane with
                 fewer workgroups than 4 x 64 ones and W % 4 == 0 (conv2d_wino16_preferred), else conv2d_wino<6r> for
                 launches of more than 256 four-row tiles that fit fewer rounds of six-row tiles (wino_rows), else
                 conv2d_wino<4r>.  Otherwise the direct kernel: conv2d_mfma<mb4> (Cout == 64) or conv2d_mfma<mb1>;
  conv_direct    everything else (Cin % 4 != 0, Cin > 256, Cout in 17 .. 63): two channels x one pixel per thread below
                 256 Ki (pixels x channel blocks of 8), eight channels x four pixels from there on.

Kernel-selection switches (tests/test_gpu_switches.py runs this file under each of them): `expected_kernel` derives the
kernel a case must land on from the PDS_* variables of the process; the numeric checks never depend on them.

Neither entry point can build the riders of the fused Matching path: the two-source forms (skip add in the loader:
conv2d_t8 / conv2d_t8w <TWO>, conv2d_mfma SRC 1), the layer-0 terms (conv2d_mfma SRC 2 / 3), per-plane weight sets, and
the channel-blocked and on-the-fly layer-1 sources of conv2d_x3.  tests/test_gpu_matching_routes.py holds them, through
pds_matching_fwd at every configuration that reaches one, against fp64 and with the rider named in the launch probe;
`test_matching_launch_census` below only counts the launches of the default operation.  Still not covered: side outputs
(ConvExtra::side_out: no walk sets it), conv2d_t8<tile> on a plain certified source through these entry points, and
channel-slice outputs (the stride-1 data gradients of tests/test_gpu_dgrad_layers.py reach those).

Tolerance: the project's single-layer bound (tests/test_gpu_conv_block.py), max-abs <= 2e-5 on the O(1) raw output, was
stated for K = 576 products per output; the 256-channel layers sum 2 304.  The gate of a case is therefore
max(2e-5, 3 * e32), e32 = the max-abs distance from fp64 of the CPU fp32 F.conv2d (+ LeakyReLU) of the same case --
measured against the reference, never against the HIP output.  The normalised output and the folded coefficients
(relative to max(1, |reference|)) are gated at 5 x that, as in tests/test_gpu_conv3d_layers.py.  The split-operand
kernels (conv2d_x3<fp16>, conv2d_t8<tile>, conv2d_t8w) also meet a mean-abs gate, max(6e-7, 3 x the mean-abs error of
the same CPU fp32 run): 6e-7 is the project's K = 576 figure (tests/test_gpu_conv_block.py).

e32 floors (tools/conv2d_e32_floors.py on the CPU, torch fp32 F.conv2d; K = 9 * Cin products per output; smallest and
largest value over the cases of that channel count, max-abs | mean-abs):
    Cin =   3 (K =   27): 5.9e-07 .. 1.2e-06 | 2.6e-08 .. 4.0e-08      3 * e32 <= 3.7e-06 | 1.2e-07
    Cin =   6 (K =   54): 5.0e-07 .. 7.6e-07 | 4.0e-08 .. 5.0e-08      3 * e32 <= 2.3e-06 | 1.5e-07
    Cin =   8 (K =   72): 3.4e-07 .. 7.9e-07 | 3.9e-08 .. 5.5e-08      3 * e32 <= 2.4e-06 | 1.7e-07
    Cin =  12 (K =  108): 1.2e-06 .. 2.4e-06 | 6.6e-08 .. 7.5e-08      3 * e32 <= 7.1e-06 | 2.3e-07
    Cin =  16 (K =  144): 1.5e-06 .. 2.5e-06 | 6.4e-08 .. 9.0e-08      3 * e32 <= 7.5e-06 | 2.7e-07
    Cin =  32 (K =  288): 3.1e-07 .. 2.8e-06 | 2.9e-08 .. 1.6e-07      3 * e32 <= 8.3e-06 | 4.9e-07
    Cin =  48 (K =  432): 1.5e-06 .. 1.5e-06 | 1.0e-07 .. 1.0e-07      3 * e32 <= 4.5e-06 | 3.1e-07
    Cin =  64 (K =  576): 9.8e-07 .. 1.8e-06 | 8.5e-08 .. 2.2e-07      3 * e32 <= 5.3e-06 | 6.6e-07
    Cin = 128 (K = 1152): 1.2e-06 .. 1.2e-06 | 9.7e-08 .. 9.7e-08      3 * e32 <= 3.6e-06 | 2.9e-07
    Cin = 256 (K = 2304): 9.2e-07 .. 1.1e-06 | 9.4e-08 .. 9.5e-08      3 * e32 <= 3.2e-06 | 2.9e-07
    Cin = 260 (K = 2340): 1.3e-06 .. 1.3e-06 | 1.2e-07 .. 1.2e-07      3 * e32 <= 3.9e-06 | 3.6e-07
so the flat 2e-5 governs the max-abs gate of every case of the table, the K = 2 304 layers included: the floor follows
the number of outputs the maximum is taken over and their magnitude, not K -- the CPU sums in blocks.  The mean-abs gate
is the flat 6e-7 for every split-operand case too: the one mean above 2e-7 (2.2e-7, a bare 64 -> 32 layer) belongs to
conv_direct, which carries no mean gate; the split-operand cases (64, 128 and 256 channels) stay at or below 1.8e-7,
3 x that 5.3e-7.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from practicaldeepstereo_nips2018_amd import _lib
from tests.test_gpu_conv3d_layers import active_switches, count_launches

pytestmark = pytest.mark.gpu
TOL = 2e-5
TOL_MEAN = 6e-7

X3B, X3F = 'conv2d_x3<bf16>', 'conv2d_x3<fp16>'
W4, W6, W16 = 'conv2d_wino<4r>', 'conv2d_wino<6r>', 'conv2d_wino16'
MB4, MB1 = 'conv2d_mfma<mb4>', 'conv2d_mfma<mb1>'
T8W, T8 = 'conv2d_t8w', 'conv2d_t8<tile>'
DIRECT = 'conv_direct<2d>'
# (the probe matches by substring: no name of this tuple contains another, so nothing has to be subtracted)
FAMILIES = (X3B, X3F, W4, W6, W16, MB4, MB1, T8W, T8, DIRECT)
SPLIT_OPERAND = (X3F, T8, T8W)
PLAIN, CHAINED, BOUND = 'plain', 'chained', 'chained+bound'

# kernel (default process), entry, n, cin, cout, d, h, w, x_per_plane, per_plane, affine, note
CASES = [
    # ---- conv2d_x3<bf16>: no range certificate; tiles of 16 x 32 on eight persistent queues ------------------------------
    (X3B, PLAIN, 1, 64, 64, 1, 16, 32, 0, 1, True, 'a single tile: seven of the eight queues empty'),
    (X3B, PLAIN, 1, 64, 64, 3, 17, 33, 0, 1, True, 'one row and one column over, 3 planes'),
    (X3B, CHAINED, 1, 64, 64, 2, 20, 36, 0, 1, True, 'deferred norm without a bound: bf16 with NORM, per-volume input'),
    (X3B, CHAINED, 1, 64, 64, 2, 20, 36, 1, 1, True, 'deferred norm without a bound: bf16 with NORM, per-plane input'),
    (X3B, PLAIN, 1, 48, 64, 1, 9, 20, 0, 0, True, 'Cin 48: three K-steps, the fewest it takes'),
    (X3B, PLAIN, 1, 256, 64, 1, 9, 20, 0, 1, True, 'Cin 256 = CMAX'),
    (X3B, PLAIN, 1, 64, 64, 2, 12, 40, 0, 1, False, 'bare'),
    # ---- conv2d_x3<fp16>: certified ----------------------------------------------------------------------------------
    (X3F, BOUND, 1, 256, 64, 2, 9, 20, 1, 1, True, 'Cin 256 = CMAX coefficients in the LDS; K = 2 304'),
    (X3F, BOUND, 1, 64, 64, 1, 16, 32, 1, 1, True, 'a single tile'),
    (X3F, BOUND, 1, 64, 64, 11, 33, 65, 1, 1, True, '11 planes of 9 tiles: uneven queues, one row / column over'),
    (X3F, BOUND, 1, 128, 64, 3, 12, 40, 0, 0, True, 'Cin 128, per-volume statistics in and out'),
    (X3F, BOUND, 2, 64, 64, 2, 12, 40, 1, 1, False, 'bare, batch 2'),
    # ---- conv_direct: what no MFMA tiling covers -----------------------------------------------------------------------
    (DIRECT, PLAIN, 1, 260, 64, 1, 5, 10, 0, 1, True, 'the first Cin beyond conv2d_x3 and conv2d_mfma (both stop at 256)'),
    (DIRECT, PLAIN, 1, 3, 32, 2, 9, 11, 0, 1, True, 'Cin % 4 != 0, Cout in 17 .. 63'),
    (DIRECT, PLAIN, 1, 6, 6, 2, 6, 10, 0, 1, True, '6 -> 6'),
    (DIRECT, PLAIN, 1, 64, 32, 1, 7, 12, 0, 1, False, '64 -> 32, bare: Cout between the two MFMA forms'),
    (DIRECT, CHAINED, 2, 6, 6, 3, 6, 10, 1, 1, True, 'deferred norm in the loader, per-plane input, batch 2'),
    (DIRECT, PLAIN, 1, 64, 32, 3, 7, 12, 0, 0, True, 'per-volume statistics'),
    (DIRECT, BOUND, 1, 3, 20, 2, 210, 209, 0, 1, True, '8 channels x 4 pixels per thread (263 340 >= 256 Ki), partial block'),
    # ---- conv2d_wino<4r>: Cin below conv2d_x3, even width, tiles of 4 x 64 -----------------------------------------------
    (W4, PLAIN, 1, 12, 64, 1, 7, 130, 0, 0, True, 'Cin 12 (space-to-depth layer), 3 tile columns, per-volume statistics'),
    (W4, CHAINED, 1, 12, 64, 2, 7, 62, 1, 1, True, 'a.scale form, ragged width (w % 4 != 0), height 7'),
    (W4, PLAIN, 1, 32, 64, 2, 12, 64, 0, 1, True, 'Cin 32, one full tile column, height 12'),
    (W4, CHAINED, 2, 32, 64, 1, 12, 62, 0, 1, True, 'a.scale form, Cin 32, batch 2, per-volume input'),
    (W4, BOUND, 1, 16, 64, 3, 7, 64, 1, 0, True, 'Cin 16; a certificate changes nothing below 48 channels'),
    (W4, PLAIN, 1, 32, 64, 3, 12, 130, 0, 1, False, 'bare, 3 tile columns'),
    # ---- conv2d_wino<6r>: more than 256 four-row tiles that fit 256 six-row ones -----------------------------------------
    (W6, PLAIN, 2, 12, 64, 48, 11, 62, 0, 1, True, '96 planes: 288 four-row tiles, 192 six-row ones; w % 4 != 0'),
    (W6, CHAINED, 2, 12, 64, 48, 11, 62, 1, 1, True, 'the same layer behind a deferred norm'),
    # ---- conv2d_wino16: 16 x 16 tiles where they cover the plane with fewer workgroups ---------------------------------
    (W16, PLAIN, 2, 16, 64, 2, 40, 72, 0, 1, True, '15 tiles against 20 wide ones, ragged on both axes'),
    (W16, PLAIN, 1, 16, 64, 1, 16, 48, 0, 0, True, 'exact tiling'),
    (W16, CHAINED, 1, 32, 64, 1, 24, 20, 0, 0, True, 'a.scale form, one partial tile column'),
    (W16, PLAIN, 1, 16, 64, 1, 8, 4, 0, 1, True, 'width 4: the smallest'),
    (W16, PLAIN, 1, 32, 64, 8, 16, 48, 0, 1, False, 'bare, 8 planes'),
    # ---- conv2d_mfma<mb4>: Cout 64 on an odd width -------------------------------------------------------------------
    (MB4, PLAIN, 1, 12, 64, 2, 8, 33, 0, 1, True, 'Cin 12, width 33'),
    (MB4, CHAINED, 1, 32, 64, 1, 9, 7, 0, 0, True, 'Cin 32, width 7, deferred norm'),
    (MB4, PLAIN, 1, 32, 64, 3, 5, 1, 0, 1, True, 'width 1'),
    (MB4, CHAINED, 2, 12, 64, 1, 6, 33, 1, 1, True, 'Cin 12, batch 2, deferred norm'),
    # ---- conv2d_mfma<mb1>: Cout <= 16 ------------------------------------------------------------------------------------
    (MB1, PLAIN, 1, 64, 8, 3, 10, 40, 0, 1, False, '64 -> 8 without a certificate'),
    (MB1, CHAINED, 1, 64, 8, 2, 10, 24, 1, 1, False, '64 -> 8 behind a deferred norm without a bound, width 24'),
    (MB1, BOUND, 1, 64, 8, 2, 9, 33, 1, 1, True, '64 -> 8 certified but normed: conv2d_t8 declines; width 33'),
    (MB1, PLAIN, 1, 8, 5, 2, 7, 24, 0, 1, True, 'Cout 5: channel guards in the epilogue and the partials'),
    (MB1, PLAIN, 1, 8, 1, 1, 9, 33, 0, 0, True, 'Cout 1'),
    (MB1, CHAINED, 1, 16, 13, 2, 6, 130, 1, 1, True, 'Cout 13, width 130'),
    (MB1, PLAIN, 2, 64, 16, 1, 5, 24, 0, 1, True, '64 -> 16, batch 2'),
    # ---- conv2d_t8w: bare certified 64 -> 8 behind a deferred norm, full-width rows ----------------------------------------
    (T8W, BOUND, 1, 64, 8, 2, 8, 64, 1, 1, False, 'W 64, H 8: the smallest; 6-row tiles, ragged'),
    (T8W, BOUND, 1, 64, 8, 3, 13, 100, 0, 1, False, 'W 100, H 13, per-volume input'),
    (T8W, BOUND, 1, 64, 8, 1, 20, 256, 1, 1, False, 'W 256: the widest row of the <8, 6, 1> form'),
    (T8W, BOUND, 1, 64, 8, 2, 8, 260, 1, 1, False, 'W 260: the first row of the <11, 8, 2> form, one 8-row tile'),
    (T8W, BOUND, 2, 64, 8, 1, 13, 352, 1, 1, False, 'W 352 = C2W_MAXW, batch 2, ragged against 8-row tiles'),
    (T8W, BOUND, 1, 64, 8, 1, 20, 260, 0, 1, False, 'W 260, H 20'),
    # ---- conv2d_t8<tile>: the same layer where the full-width form declines ------------------------------------------------
    (T8, BOUND, 1, 64, 8, 2, 21, 36, 1, 1, False, 'W 36: narrower than 64'),
    (T8, BOUND, 1, 64, 8, 1, 9, 66, 1, 1, False, 'W 66: w % 4 != 0'),
    (T8, BOUND, 1, 64, 8, 1, 8, 356, 1, 1, False, 'W 356: beyond C2W_MAXW'),
    (T8, BOUND, 1, 64, 8, 2, 7, 64, 0, 1, False, 'H 7 at W 64: below the 8 rows of the full-width form'),
    (T8, BOUND, 1, 64, 8, 1, 16, 32, 1, 1, False, 'exactly one tile'),
    (T8, BOUND, 1, 64, 8, 1, 17, 33, 1, 1, False, 'one row and one column over'),
    (T8, BOUND, 2, 64, 8, 1, 10, 50, 1, 1, False, 'ragged 50 columns, batch 2'),
]


def case_id(c):
    return '%s_%s_n%d_%dto%d_d%d_%dx%d_xpp%d_pp%d_%s' % (c[0].replace('<', '_').replace('>', ''), c[1].replace('+', '_'),
                                                          c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9],
                                                          'in' if c[10] else 'bare')


def _ceil(a, b):
    return (a + b - 1) // b


def wino16_preferred(h, w, switches):
    """conv2d_wino16_preferred (csrc/conv2d_wino16.hip)."""
    if switches.get('PDS_WINO_TILE16', '')[:1] == '0' or w % 4 != 0 or w < 4:
        return False
    return _ceil(h, 16) * _ceil(w, 16) < _ceil(h, 4) * _ceil(w, 64)


def wino_rows(n, d, h, w, switches):
    """wino_rows (csrc/conv2d_wino.hip): rounds of workgroups over 256 CUs x rows per tile."""
    if switches.get('PDS_WINO_ROWS6', '')[:1] == '0':
        return 4
    planes, tx = n * d, _ceil(w, 64)
    t4 = _ceil(planes * tx * _ceil(h, 4), 256) * 4
    t6 = _ceil(planes * tx * _ceil(h, 6), 256) * 6
    return 6 if t6 < t4 else 4


def dispatch(entry, n, cin, cout, d, h, w, affine, switches):
    """The 2-D kernel family conv_block (csrc/api.hip:168-170) picks for a single-source layer of an entry point."""

    def off(name):
        return switches.get(name, '')[:1] == '0'

    bounded, a_scale = entry == BOUND, entry != PLAIN
    # conv2d_t8_supported (+ "no statistics wanted") and c2t8_wide
    if (not affine and not off('PDS_CONV2D_T8') and cin == 64 and cout == 8 and bounded
            and n * 64 * d * h * w < 1 << 29 and n * d * _ceil(h, 16) * _ceil(w, 32) < 1 << 30):
        wide = not off('PDS_CONV2D_T8W') and a_scale and w % 4 == 0 and 64 <= w <= 352 and h >= 8
        return T8W if wide else T8
    # conv2d_x3_supported and x3_use_fp16
    if (not off('PDS_X3') and cout == 64 and cin % 16 == 0 and 48 <= cin <= 256 and d * h * w * 8 < 1 << 30
            and n * d < 1 << 20):
        return X3F if bounded and not off('PDS_X3_FP16') else X3B
    # conv2d_mfma_supported
    if (cin % 4 == 0 and cin <= 256 and (cout == 64 or cout <= 16) and 4 * d * h * w < 1 << 31 and d <= 65535
            and n <= 65535):
        # conv2d_wino_eligible (its Cin and size limits are those of conv2d_mfma_supported)
        if not off('PDS_WINOGRAD') and cout == 64 and w % 2 == 0 and w >= 2:
            if wino16_preferred(h, w, switches):
                return W16
            return W6 if wino_rows(n, d, h, w, switches) == 6 else W4
        return MB4 if cout == 64 else MB1
    return DIRECT


def expected_kernel(case, switches):
    """The kernel family the case must land on under the switches of the process (none: its first column)."""
    _, entry, n, cin, cout, d, h, w, _, _, affine, _ = case
    return dispatch(entry, n, cin, cout, d, h, w, affine, switches)


def make_case(case, index):
    """Inputs of a case (CPU tensors): raw producer output, its folded coefficients, the block's parameters."""
    _, _, n, cin, cout, d, h, w, xpp, _, _, _ = case
    g = torch.Generator().manual_seed(9000 + index)
    x = torch.randn(n, cin, d, h, w, generator=g) * 37.0 + 5.0
    groups_in = (n, cin, d if xpp else 1, 1, 1)
    x_scale = (torch.rand(groups_in, generator=g) + 0.5) / 37.0
    x_shift = torch.randn(groups_in, generator=g) * 0.2 - 5.0 * x_scale
    weight = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    gamma = torch.rand(cout, generator=g) + 0.5
    beta = torch.randn(cout, generator=g) * 0.2
    # the fp32 normalised input the loader forms (one fma per element); the plain entry is handed this tensor itself
    xhat = torch.addcmul(x_shift.expand_as(x), x_scale.expand_as(x), x)
    return x, x_scale, x_shift, xhat, weight, bias, gamma, beta


def conv(xhat, weight, bias, affine, dtype):
    """The planes of [n, cin, d, h, w] through F.conv2d in `dtype` (+ LeakyReLU(0.1) in front of an InstanceNorm)."""
    n, cin, d, h, w = xhat.shape
    planes = xhat.to(dtype).permute(0, 2, 1, 3, 4).reshape(n * d, cin, h, w)
    y = F.conv2d(planes, weight.to(dtype), bias.to(dtype), padding=1)
    y = y.reshape(n, d, -1, h, w).permute(0, 2, 1, 3, 4)
    return F.leaky_relu(y, 0.1) if affine else y


def reference(xhat, weight, bias, gamma, beta, per_plane, affine):
    """-> fp64 raw, normalised output, folded scale and shift [n, cout, d or 1, 1, 1] (None for a bare convolution)."""
    raw = conv(xhat, weight, bias, affine, torch.float64)
    if not affine:
        return raw, None, None, None
    dims = (3, 4) if per_plane else (2, 3, 4)
    mean = raw.mean(dim=dims, keepdim=True)
    var = raw.var(dim=dims, unbiased=False, keepdim=True)
    scale = gamma.double().view(1, -1, 1, 1, 1) / torch.sqrt(var + 1e-5)
    shift = beta.double().view(1, -1, 1, 1, 1) - mean * scale
    return raw, raw * scale + shift, scale, shift


def fp32_floor(xhat, weight, bias, affine, want_raw):
    """e32: how far the CPU's own fp32 convolution of the case is from fp64 (max-abs, mean-abs)."""
    delta = (conv(xhat, weight, bias, affine, torch.float32).double() - want_raw).abs()
    return float(delta.max()), float(delta.mean())


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def launches_by_family(lib, run):
    """Launches of each 2-D kernel family in `run` (one run per probe name: the probe matches one substring at a time)
    and the result of the last run."""
    counts, result = {}, None
    for name in FAMILIES:
        counts[name], result = count_launches(lib, name, run)
    return counts, result


def run_layer(dev, case, x, x_scale, x_shift, xhat, bound, weight, bias, gamma, beta):
    """-> a closure that runs the layer once into fresh NaN-filled outputs and returns (raw, scale, shift) on the GPU."""
    lib = _lib.load()
    _, entry, n, cin, cout, d, h, w, xpp, per_plane, affine, _ = case
    tensors = [t.to(dev).contiguous() for t in (weight, bias, gamma, beta)]
    params = _lib.ConvBlockParams()
    params.weight, params.bias = tensors[0].data_ptr(), tensors[1].data_ptr()
    if affine:
        params.gamma, params.beta = tensors[2].data_ptr(), tensors[3].data_ptr()
    ws = torch.empty(int(lib.pds_conv_block_workspace_bytes(n, cin, cout, d, h, w, 1, 1, per_plane)), dtype=torch.uint8,
                     device=dev)
    plain = entry == PLAIN
    xg = (xhat if plain else x).to(dev).contiguous()
    sg = None if plain else x_scale.reshape(-1).to(dev).contiguous()
    hg = None if plain else x_shift.reshape(-1).to(dev).contiguous()
    bg = bound.reshape(1).to(dev) if bound is not None else None
    groups = n * cout * (d if per_plane else 1)

    def opt(t):
        return _lib.ptr(t) if t is not None else None

    def run():
        raw = torch.full((n, cout, d, h, w), float('nan'), device=dev)
        scale = torch.full((groups,), float('nan'), device=dev) if affine else None
        shift = torch.full((groups,), float('nan'), device=dev) if affine else None
        if plain:
            _lib.check(lib.pds_conv_block_fwd(ctypes.byref(params), _lib.ptr(xg), _lib.ptr(raw), opt(scale), opt(shift),
                                              n, cin, cout, d, h, w, 1, 1, per_plane, _lib.ptr(ws), ws.numel(),
                                              _lib.stream_handle(dev)), 'pds_conv_block_fwd')
        else:
            _lib.check(lib.pds_conv_block_chained_fwd(ctypes.byref(params), _lib.ptr(xg), _lib.ptr(sg), _lib.ptr(hg), xpp,
                                                      opt(bg), _lib.ptr(raw), opt(scale), opt(shift), n, cin, cout, d, h,
                                                      w, 1, 1, per_plane, _lib.ptr(ws), ws.numel(),
                                                      _lib.stream_handle(dev)), 'pds_conv_block_chained_fwd')
        return raw, scale, shift, (tensors, xg, sg, hg, bg, ws)   # (the inputs stay alive until the run is synchronised)

    return run


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_conv2d_layer_against_fp64(dev, case):
    lib = _lib.load()
    kernel, entry, n, cin, cout, d, h, w, xpp, per_plane, affine, note = case
    x, x_scale, x_shift, xhat, weight, bias, gamma, beta = make_case(case, CASES.index(case))
    bound = xhat.abs().max() if entry == BOUND else None
    counts, (raw, scale, shift, _) = launches_by_family(
        lib, run_layer(dev, case, x, x_scale, x_shift, xhat, bound, weight, bias, gamma, beta))
    raw = raw.cpu()

    want_raw, want_normed, want_scale, want_shift = reference(xhat, weight, bias, gamma, beta, per_plane, affine)
    e32, e32_mean = fp32_floor(xhat, weight, bias, affine, want_raw)
    tol, tol_mean = max(TOL, 3.0 * e32), max(TOL_MEAN, 3.0 * e32_mean)
    assert raw.shape == want_raw.shape
    finite = bool(torch.isfinite(raw).all())
    err = float((raw.double() - want_raw).abs().max()) if finite else float('nan')
    err_mean = float((raw.double() - want_raw).abs().mean()) if finite else float('nan')
    err_n = err_scale = err_shift = 0.0
    coefficients_finite = True
    if affine:
        scale, shift = scale.cpu().double().view(want_scale.shape), shift.cpu().double().view(want_shift.shape)
        coefficients_finite = bool(torch.isfinite(scale).all() and torch.isfinite(shift).all())
        err_n = float((raw.double() * scale + shift - want_normed).abs().max()) if finite else float('nan')
        err_scale = float(((scale - want_scale).abs() / want_scale.abs().clamp(min=1.0)).max())
        err_shift = float(((shift - want_shift).abs() / want_shift.abs().clamp(min=1.0)).max())
    print('conv2d layer %s (%s): launches %s  e32 %.2e (mean %.2e)  gate %.2e (mean %.2e)  raw err %.3g (mean %.3g)  '
          'normalised err %.3g  scale err %.3g  shift err %.3g'
          % (case_id(case), note, {k: v for k, v in counts.items() if v}, e32, e32_mean, tol, tol_mean, err, err_mean,
             err_n, err_scale, err_shift))

    # 1. which kernel ran
    want_kernel = expected_kernel(case, active_switches())
    assert counts[want_kernel] > 0, 'expected %s, launches: %s' % (want_kernel, counts)
    others = {k: v for k, v in counts.items() if k != want_kernel and v}
    assert not others, 'expected only %s, launches: %s' % (want_kernel, counts)
    # 2. every output position written
    assert not torch.isnan(raw).any(), 'output positions left unwritten'
    assert finite, 'non-finite output'
    assert coefficients_finite, 'InstanceNorm coefficients left unwritten or non-finite'
    # 3. values
    assert err <= tol, (err, tol)
    if kernel in SPLIT_OPERAND:
        assert err_mean <= tol_mean, (err_mean, tol_mean)
    if affine:
        assert err_n <= 5 * tol, (err_n, 5 * tol)
        # 4. folded InstanceNorm coefficients
        assert err_scale <= 5 * tol, (err_scale, 5 * tol)
        assert err_shift <= 5 * tol, (err_shift, 5 * tol)


# ---- launch census of the fused Matching path ------------------------------------------------------------------------
# switches that move a 2-D layer of Matching to another kernel, or change the layers the fused path is made of
CENSUS_SWITCHES = ('PDS_X3', 'PDS_X3_FP16', 'PDS_WINOGRAD', 'PDS_WINO_TILE16', 'PDS_WINO_ROWS6', 'PDS_MATCHING_FUSED',
                   'PDS_MATCHING_COLUMNS', 'PDS_MATCHING_CB8', 'PDS_CONV2D_T8', 'PDS_CONV2D_T8W')
CENSUS = {
    # descriptor shape: launches per family in a default process (families not named: none)
    (1, 64, 16, 64): {W4: 2, X3F: 3, T8W: 1},
    (1, 64, 9, 21): {MB4: 2, X3F: 3, T8: 1},
}


@pytest.mark.parametrize('shape', sorted(CENSUS), ids=lambda s: 'x'.join(map(str, s)))
def test_matching_launch_census(dev, shape):
    """Which 2-D kernels pds.Matching(7, pds.MatchingOperation()) launches under no_grad (eight disparity planes, two
    residual blocks).  Derived from matching_pipeline (csrc/api_matching.hip) in a default process -- fused, column form:

      "const int l0_planes = columns ? 2 : 3;" / "const Geom g3{batch, F, l0_planes, h, l0_rs};" with l0_rs = w + 2,
      "e3.plane_weight_sets = l0_planes;  y3 = conv_block(c, plain_src(x3), no_src(), g3, p3, F, ...)": layer 0 is one 64 -> 64
        launch over two planes of h x (w + 2).  Per-plane weight sets are Matching extras, so conv2d_x3 is passed over
        (csrc/api.hip: "!(extra && extra->matching_extras()) && conv2d_x3_supported(L)"): at w + 2 = 66 (even, 66 % 4 != 0,
        16 four-row tiles) the layer runs on conv2d_wino<4r>, at w + 2 = 23 (odd) on conv2d_mfma<mb4>;
      "const Geom g2{batch, F, 2, h, w + 2};  e2.plane_weight_sets = 2;  y4 = conv_block(c, plain_src(x2), none, g2, p2, F,
        ...)": layer 1 (first convolution of block 0) has the same geometry and lands on the same kernel;
      "DT t2 = on_the_fly ? conv_block(c, t1.src(), none, g, P.blocks[1], ..., &fly) : conv_block(c, t1.src(), none, g,
        P.blocks[1], F, 1, 1, 1);" and, for r = 1, "t1 = conv_block(c, cur.src(), none, g, P.blocks[2 * r], ...);
        t2 = conv_block(c, t1.src(), none, g, P.blocks[2 * r + 1], ...)": three certified 64 -> 64 layers over the eight
        planes, conv2d_x3<fp16> (t1 and t2 carry the bound in_finalize writes, the residual sum the one carve_amax gives it);
      "conv_block(c, t2.src(), cur.src(), g, P.last, P.signature_features, 1, 1, 1, signatures);": the bare two-source
        64 -> 8 layer, both sources certified: conv2d_t8w on rows of 64 columns and 16 rows, conv2d_t8<tile> at 9 x 21.
    Nothing reaches conv_direct.  The two-source, layer-0 and channel-blocked riders these launches carry cannot be built
    through the single-layer entry points above: tests/test_gpu_matching_routes.py names each in the launch probe and
    holds its numeric side against fp64, for this operation and for the other block counts and widths.

    Under a switch of CENSUS_SWITCHES the fused path is made of other layers (three or five planes in the first two
    launches, an unfused first layer) or its layers move to other kernels: the census is printed, and only what holds
    whatever the path is asserted -- PDS_CONV2D_T8W=0 sends the 64 -> 8 layer to conv2d_t8<tile>, PDS_CONV2D_T8=0 to
    conv2d_mfma<mb1>, and nothing reaches conv_direct."""
    import practicaldeepstereo_nips2018_amd as pds
    lib = _lib.load()
    torch.manual_seed(0)
    module = pds.Matching(7, pds.MatchingOperation()).to(dev).eval()
    g = torch.Generator().manual_seed(17)
    left, right = torch.randn(*shape, generator=g).to(dev), torch.randn(*shape, generator=g).to(dev)

    def run():
        with torch.no_grad():
            return module(left, right)

    counts, signatures = launches_by_family(lib, run)
    switches = active_switches()
    moved = sorted(k for k in switches if k in CENSUS_SWITCHES)
    print('matching census %s: launches %s%s' % (shape, {k: v for k, v in counts.items() if v},
                                                 '  (switches: %s)' % ', '.join(moved) if moved else ''))
    assert bool(torch.isfinite(signatures).all())
    assert counts[DIRECT] == 0, counts
    if not moved:
        assert counts == dict({k: 0 for k in FAMILIES}, **CENSUS[shape]), counts
        return
    last = T8W if T8W in CENSUS[shape] else T8
    if switches.get('PDS_CONV2D_T8', '')[:1] == '0':
        last = MB1
    elif switches.get('PDS_CONV2D_T8W', '')[:1] == '0':
        last = T8
    for name in (T8W, T8, MB1):
        assert counts[name] == (1 if name == last else 0), (last, counts)
