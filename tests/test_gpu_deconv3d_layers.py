"""GPU (-m gpu): every transposed 3-D kernel of the Regularization hourglass alone, one layer at a time, against an fp64
transposed convolution.

pds_deconv_block_chained_fwd (ABI v7) runs one transposed block (ConvTranspose3d -> LeakyReLU(0.1) -> InstanceNorm3d, or
the bare ConvTranspose3d of the last layer; reference network_blocks.py:37-44, 75-85) through deconv_block of csrc/api.hip,
the dispatch of the module walks.  kd = 4 is kernel 4, stride 2, padding 1 (output 2D x 2H x 2W); kd = 3 is kernel
(3, 4, 4), stride (1, 2, 2), padding 1 (output D x 2H x 2W).  The inputs follow tests/test_gpu_conv3d_layers.py: the raw
producer output is far from unit scale (x 37, + 5) and the folded per-(n, c) coefficients bring it back,
x^ = scale * x + shift.  A case has one of three source kinds: PLAIN (x_scale NULL, the input is x^ itself), CHAINED
(behind the deferred InstanceNorm, no range certificate) and CERT (chained, with the certificate max |x^|).  Only a
certified source may run an fp16-split form.

Every case, in this order,
  1. counts the launches of all seven transposed kernel families with the launch probe and asserts that the expected one
     -- and no other -- ran (a layer that silently lands on the generic kernel, or a split layer that silently runs on
     the fp32 pipe, passes every numeric check);
  2. pre-fills the output with NaN and asserts that none is left, and that everything is finite;
  3. compares the raw output with fp64 F.conv_transpose3d (+ LeakyReLU when normed);
  4. compares the normalised output scale * raw + shift with fp64;
  5. compares the returned folded coefficients with the fp64 statistics.
(4 and 5 do not exist for a bare layer: it has no statistics, and is given NULL for scale / shift.)

Dispatch (csrc/api.hip deconv_block, in this order):
  deconv3d_cell   k4, 8 -> 4 (tiles of 32 x 4 x 2 CELLS, 1024 persistent workgroups over the batch) and 16 -> 8 (tiles of
                  64 x 2 x 2 cells, 512 workgroups); an input of D x H x W has (D + 1) x (H + 1) x (W + 1) cells, so the
                  "exact" shapes are one short of a multiple of the tile.  <fp16> behind a certified source, else <fp32>.
  deconv3d_ks     k4, Cin in {16, 32, 64, 128}, up to 30 000 INPUT voxels (a fixed limit: PDS_CONV3D_KS_LIMIT governs the
                  convolutions only); single-row tiles of 16 / 32 / 64 cells (nb 1 / 2 / 4).  <fp16> behind a certified
                  source, else <fp32>.
  deconv3d_gemm   the transposed modes of conv3d_mfma.hip, Cin a multiple of 4: <k4> and <k3>; plans by input geometry:
                  rows <= 16, <= 32, wider, and from 100 000 input voxels 64-wide tiles, or 80-wide ones where the width
                  divides by 80.  From 64 tiles on the launch is re-mapped over the 8 compute dies, 8 * ceil(tiles / 8)
                  workgroups.
  deconv_direct   everything else (here: Cin = 6); 4 output channels per workgroup from 1024 workgroups on, else 1.

Kernel-selection switches (tests/test_gpu_switches.py runs this file under each of them): `expected_kernel` derives the
family a case must land on from the PDS_* variables of the process; the numeric checks never depend on them.

Tolerance: the project's single-layer bound, max-abs <= 2e-5 on the O(1) raw output; the gate of a case is
max(2e-5, 3 * e32), e32 = the max-abs distance from fp64 of the CPU fp32 F.conv_transpose3d (+ LeakyReLU) of the same case
-- measured against the reference, never against the HIP output.  The normalised output and the folded coefficients
(relative to max(1, |reference|)) are gated at 5 x the gate, as in tests/test_gpu_conv3d_layers.py.

e32 floors (tools/deconv3d_e32_floors.py on the CPU, torch fp32 F.conv_transpose3d; an output sums Cin * 8 products for
k4, Cin * 4 or Cin * 8 for k3; smallest and largest value over the cases of that channel count):
    Cin =   4: 5.4e-7 .. 1.1e-6      Cin =  24: 2.0e-6
    Cin =   6: 5.2e-7 .. 1.3e-6      Cin =  32: 1.2e-6 .. 2.5e-6
    Cin =   8: 7.1e-7 .. 1.2e-6      Cin =  64: 2.1e-6 .. 3.2e-6
    Cin =  12: 8.7e-7                Cin = 128: 1.8e-6 .. 2.7e-6
    Cin =  16: 1.2e-6 .. 2.1e-6
so 3 * e32 <= 9.7e-6 and the flat 2e-5 governs every case of the table.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from practicaldeepstereo_nips2018_amd import _lib
from tests.test_gpu_conv3d_layers import active_switches, count_launches

pytestmark = pytest.mark.gpu
TOL = 2e-5

CELL16, CELL32 = 'deconv3d_cell<fp16>', 'deconv3d_cell<fp32>'
KS16, KS32 = 'deconv3d_ks<fp16>', 'deconv3d_ks<fp32>'
GEMM4, GEMM3, DIRECT = 'deconv3d_gemm<k4>', 'deconv3d_gemm<k3>', 'deconv_direct'
FAMILIES = (CELL16, CELL32, KS16, KS32, GEMM4, GEMM3, DIRECT)
PLAIN, CHAINED, CERT = 'plain', 'chained', 'cert'

# kernel (default configuration), n, cin, cout, kd, d, h, w (of the INPUT), source kind, normed, note
CASES = [
    # ---- deconv3d_cell 8 -> 4: tiles of 32 x 4 x 2 cells, 1024 persistent workgroups over the batch ------------------
    (CELL32, 1, 8, 4, 4, 3, 7, 31, PLAIN, True, 'exact tiling, 4 tiles on 8 workgroups (half idle); plain source'),
    (CELL32, 1, 8, 4, 4, 3, 7, 31, CHAINED, True, 'exact tiling; deferred InstanceNorm, no certificate'),
    (CELL16, 1, 8, 4, 4, 3, 7, 31, CERT, True, 'exact tiling; split form'),
    (CELL16, 1, 8, 4, 4, 4, 8, 32, CERT, True, 'one cell in the last tile on every axis'),
    (CELL16, 2, 8, 4, 4, 5, 9, 40, CERT, True, 'ragged, batch 2'),
    (CELL32, 2, 8, 4, 4, 5, 9, 40, CHAINED, True, 'ragged, batch 2, no certificate'),
    (CELL16, 8, 8, 4, 4, 15, 23, 95, CERT, True, '144 tiles on 128 persistent workgroups per entry: second lap'),
    # ---- deconv3d_cell 16 -> 8: tiles of 64 x 2 x 2 cells, 512 workgroups ----------------------------------------------
    (CELL32, 1, 16, 8, 4, 3, 3, 63, PLAIN, True, 'exact tiling; plain source'),
    (CELL32, 1, 16, 8, 4, 3, 3, 63, CHAINED, True, 'exact tiling; no certificate'),
    (CELL16, 1, 16, 8, 4, 3, 3, 63, CERT, True, 'exact tiling; split form'),
    (CELL16, 1, 16, 8, 4, 2, 5, 64, CERT, True, 'one cell in a second tile column'),
    (CELL16, 8, 16, 8, 4, 11, 23, 63, CERT, True, '72 tiles on 64 workgroups per entry'),
    (CELL32, 8, 16, 8, 4, 11, 23, 63, CHAINED, True, '72 tiles on 64 workgroups per entry, no certificate'),
    # ---- deconv3d_ks -----------------------------------------------------------------------------------------------
    (KS16, 1, 32, 16, 4, 3, 5, 15, CERT, True, 'nb 1 exact; split form'),
    (KS32, 1, 32, 16, 4, 3, 5, 15, CHAINED, True, 'nb 1 exact; no certificate'),
    (KS32, 1, 32, 16, 4, 3, 5, 15, PLAIN, True, 'nb 1 exact; plain source'),
    (KS16, 1, 32, 16, 4, 4, 6, 16, CERT, True, '17 cells: one in the second block, nb 2'),
    (KS16, 2, 64, 32, 4, 3, 4, 31, CERT, True, 'nb 2 exact, batch 2'),
    (KS32, 1, 64, 32, 4, 2, 5, 40, CHAINED, True, 'nb 4 ragged'),
    (KS16, 1, 128, 64, 4, 2, 3, 6, CERT, True, '16 channels per wave'),
    (KS32, 1, 128, 64, 4, 2, 2, 33, CHAINED, True, 'nb 4'),
    (KS16, 1, 32, 16, 4, 10, 50, 60, CERT, True, 'exactly 30 000 input voxels: the largest volume deconv3d_ks serves'),
    (GEMM4, 1, 32, 16, 4, 10, 50, 61, CERT, True, '30 500 voxels: above the deconv3d_ks limit'),
    # ---- deconv3d_gemm<k4>: the plans of choose_plan_deconv ------------------------------------------------------------
    (GEMM4, 1, 12, 6, 4, 3, 5, 9, CERT, True, 'rows <= 16; 16-channel K chunk overhanging Cin = 12'),
    (GEMM4, 1, 24, 12, 4, 4, 6, 20, CHAINED, True, 'rows <= 32; 16-channel K chunks overhanging Cin = 24'),
    (GEMM4, 2, 4, 2, 4, 3, 7, 40, PLAIN, True, 'rows > 32, batch 2; plain source'),
    (GEMM4, 1, 4, 2, 4, 10, 100, 100, CERT, True, 'exactly 100 000 voxels: 64-wide tiles, 250 tiles behind the re-mapping'),
    (GEMM4, 1, 4, 2, 4, 8, 125, 160, CHAINED, True, 'width / 80: the 80-wide plan'),
    # ---- deconv3d_gemm<k3> -----------------------------------------------------------------------------------------
    (GEMM3, 1, 4, 1, 3, 6, 9, 21, CERT, False, 'bare 4 -> 1'),
    (GEMM3, 1, 8, 1, 3, 5, 8, 40, PLAIN, False, 'bare 8 -> 1; plain source'),
    (GEMM3, 1, 8, 4, 3, 3, 6, 18, CHAINED, True, 'with InstanceNorm'),
    # ---- deconv_direct -----------------------------------------------------------------------------------------------
    (DIRECT, 1, 6, 3, 4, 3, 5, 7, CERT, True, 'one output channel per workgroup'),
    (DIRECT, 2, 6, 3, 4, 64, 32, 32, CHAINED, True, '1024 blocks: the four-channel form with a partial channel block'),
    (DIRECT, 1, 6, 1, 3, 4, 5, 9, PLAIN, False, 'bare, kd 3'),
]


def case_id(c):
    return '%s_n%d_%dto%d_k%d_%dx%dx%d_%s%s' % (c[0].replace('<', '_').replace('>', ''), c[1], c[2], c[3], c[4], c[5], c[6],
                                                c[7], c[8], '' if c[9] else '_bare')


def expected_kernel(case, switches):
    """The kernel family the case must land on: the intended one, unless a switch of this process turns it off -- then
    what the dispatch of csrc/api.hip deconv_block leaves.  (PDS_CONV3D_KS_LIMIT does not govern the transposed layers.)"""
    kernel, cin, cout, source = case[0], case[2], case[3], case[8]

    def off(name):
        return switches.get(name, '')[:1] == '0'

    if kernel in (CELL16, CELL32):
        if off('PDS_DECONV_CELL'):
            # 16 -> 8 is a deconv3d_ks shape (every 16 -> 8 case of the table is below its volume limit); 8 -> 4 is not
            kernel = GEMM4 if (cin, cout) == (8, 4) else (KS16 if source == CERT else KS32)
        elif kernel == CELL16 and off('PDS_DECONV_CELL_X'):
            return CELL32
    if kernel in (KS16, KS32):
        if off('PDS_CONV3D_KS'):
            return GEMM4
        if kernel == KS16 and off('PDS_CONV3D_KSX'):
            return KS32
    return kernel


def make_case(case, index):
    """Inputs of a case (CPU tensors): raw producer output, its folded coefficients, the block's parameters."""
    _, n, cin, cout, kd, d, h, w, _, normed, _ = case
    g = torch.Generator().manual_seed(7000 + index)
    x = torch.randn(n, cin, d, h, w, generator=g) * 37.0 + 5.0
    x_scale = (torch.rand(n, cin, 1, 1, 1, generator=g) + 0.5) / 37.0
    x_shift = torch.randn(n, cin, 1, 1, 1, generator=g) * 0.2 - 5.0 * x_scale
    weight = torch.randn(cin, cout, kd, 4, 4, generator=g) * (cin * 8) ** -0.5
    bias = torch.randn(cout, generator=g) * 0.1
    gamma = torch.rand(cout, generator=g) + 0.5
    beta = torch.randn(cout, generator=g) * 0.2
    # the fp32 normalised input the loader forms (one fma per element)
    xhat = torch.addcmul(x_shift.expand_as(x), x_scale.expand_as(x), x)
    return x, x_scale, x_shift, xhat, weight, bias, gamma, beta


def deconv(xhat, weight, bias, kd, normed, dtype):
    y = F.conv_transpose3d(xhat.to(dtype), weight.to(dtype), bias.to(dtype), stride=(2 if kd == 4 else 1, 2, 2), padding=1)
    return F.leaky_relu(y, 0.1) if normed else y


def reference(xhat, weight, bias, gamma, beta, kd, normed):
    """-> fp64 raw (LeakyReLU(deconv) when normed), normalised, folded scale and shift per (n, c) (None when bare)."""
    raw = deconv(xhat, weight, bias, kd, normed, torch.float64)
    if not normed:
        return raw, None, None, None
    mean = raw.mean(dim=(2, 3, 4), keepdim=True)
    var = raw.var(dim=(2, 3, 4), unbiased=False, keepdim=True)
    scale = gamma.double().view(1, -1, 1, 1, 1) / torch.sqrt(var + 1e-5)
    shift = beta.double().view(1, -1, 1, 1, 1) - mean * scale
    return raw, raw * scale + shift, scale.reshape(-1), shift.reshape(-1)


def fp32_floor(xhat, weight, bias, kd, normed, want_raw):
    """e32: how far the CPU's own fp32 transposed convolution of the case is from fp64."""
    return float((deconv(xhat, weight, bias, kd, normed, torch.float32).double() - want_raw).abs().max())


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def launches_by_family(lib, run):
    """Launches of each transposed kernel family in `run` (one run per probe name: the probe matches one substring at a
    time; no name of FAMILIES contains another) and the result of the last run."""
    counts, result = {}, None
    for name in FAMILIES:
        counts[name], result = count_launches(lib, name, run)
    return counts, result


def run_layer(dev, case, x, x_scale, x_shift, xhat, bound, weight, bias, gamma, beta):
    """-> a closure that runs the layer once into fresh NaN-filled outputs and returns (raw, scale, shift) on the GPU."""
    lib = _lib.load()
    _, n, cin, cout, kd, d, h, w, source, normed, _ = case
    od = 2 * d if kd == 4 else d
    tensors = [t.to(dev).contiguous() for t in (weight, bias, gamma, beta)]
    params = _lib.ConvBlockParams()
    params.weight, params.bias = tensors[0].data_ptr(), tensors[1].data_ptr()
    if normed:
        params.gamma, params.beta = tensors[2].data_ptr(), tensors[3].data_ptr()
    ws = torch.empty(int(lib.pds_deconv_block_workspace_bytes(n, cin, cout, d, h, w, kd)), dtype=torch.uint8, device=dev)
    plain = source == PLAIN
    xg = (xhat if plain else x).to(dev).contiguous()
    sg = None if plain else x_scale.reshape(-1).to(dev).contiguous()
    hg = None if plain else x_shift.reshape(-1).to(dev).contiguous()
    bg = bound.reshape(1).to(dev) if bound is not None else None

    def opt(t):
        return _lib.ptr(t) if t is not None else None

    def run():
        raw = torch.full((n, cout, od, 2 * h, 2 * w), float('nan'), device=dev)
        scale = torch.full((n * cout,), float('nan'), device=dev) if normed else None
        shift = torch.full((n * cout,), float('nan'), device=dev) if normed else None
        _lib.check(lib.pds_deconv_block_chained_fwd(ctypes.byref(params), _lib.ptr(xg), opt(sg), opt(hg), opt(bg),
                                                    _lib.ptr(raw), opt(scale), opt(shift), n, cin, cout, d, h, w, kd,
                                                    _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev)),
                   'pds_deconv_block_chained_fwd')
        return raw, scale, shift, (tensors, xg, sg, hg, bg, ws)   # (the inputs stay alive until the run is synchronised)

    return run


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_deconv3d_layer_against_fp64(dev, case):
    lib = _lib.load()
    kernel, n, cin, cout, kd, d, h, w, source, normed, note = case
    x, x_scale, x_shift, xhat, weight, bias, gamma, beta = make_case(case, CASES.index(case))
    bound = xhat.abs().max() if source == CERT else None
    counts, (raw, scale, shift, _) = launches_by_family(
        lib, run_layer(dev, case, x, x_scale, x_shift, xhat, bound, weight, bias, gamma, beta))
    raw = raw.cpu()

    want_raw, want_normed, want_scale, want_shift = reference(xhat, weight, bias, gamma, beta, kd, normed)
    e32 = fp32_floor(xhat, weight, bias, kd, normed, want_raw)
    tol = max(TOL, 3.0 * e32)
    assert raw.shape == want_raw.shape
    finite = bool(torch.isfinite(raw).all())
    err = float((raw.double() - want_raw).abs().max()) if finite else float('nan')
    err_n = err_scale = err_shift = 0.0
    if normed:
        scale, shift = scale.cpu().double(), shift.cpu().double()
        normed_out = raw.double() * scale.view(n, cout, 1, 1, 1) + shift.view(n, cout, 1, 1, 1)
        err_n = float((normed_out - want_normed).abs().max()) if finite else float('nan')
        err_scale = float(((scale - want_scale).abs() / want_scale.abs().clamp(min=1.0)).max())
        err_shift = float(((shift - want_shift).abs() / want_shift.abs().clamp(min=1.0)).max())
    print('deconv3d layer %s (%s): launches %s  e32 %.2e  gate %.2e  raw err %.3g  normalised err %.3g  scale err %.3g  '
          'shift err %.3g' % (case_id(case), note, {k: v for k, v in counts.items() if v}, e32, tol, err, err_n,
                              err_scale, err_shift))

    # 1. which kernel ran
    want_kernel = expected_kernel(case, active_switches())
    assert counts[want_kernel] > 0, 'expected %s, launches: %s' % (want_kernel, counts)
    others = {k: v for k, v in counts.items() if k != want_kernel and v}
    assert not others, 'expected only %s, launches: %s' % (want_kernel, counts)
    # 2. every output position written
    assert not torch.isnan(raw).any(), 'output positions left unwritten'
    assert finite, 'non-finite output'
    # 3. values
    assert err <= tol, (err, tol)
    if normed:
        # 4. normalised output
        assert err_n <= 5 * tol, (err_n, 5 * tol)
        # 5. folded InstanceNorm coefficients (NaN-pre-filled: an unwritten one fails here)
        assert err_scale <= 5 * tol, (err_scale, 5 * tol)
        assert err_shift <= 5 * tol, (err_shift, 5 * tol)


def test_every_family_is_expected_somewhere():
    """Each of the seven probe names is the expected family of at least one case in the default configuration."""
    assert {expected_kernel(c, {}) for c in CASES} == set(FAMILIES)
    assert all(expected_kernel(c, {}) == c[0] for c in CASES)
