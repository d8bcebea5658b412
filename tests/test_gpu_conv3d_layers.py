"""GPU (-m gpu): every 3-D kernel of the Regularization hourglass alone, one layer at a time, against an fp64 convolution.

pds_conv_block_chained_fwd(kd = 3, per_plane = 0) runs one block (Conv3d -> LeakyReLU(0.1) -> InstanceNorm3d, reference
network_blocks.py:61-72) behind a deferred InstanceNorm, the way the hourglass chains its layers: the raw producer output
is far from unit scale (x 37, + 5), the loader applies the folded per-(n, c) coefficients x^ = scale * x + shift.  With a
range certificate (x_bound) the fp16-split forms run (conv3d_nx, conv3d_t8x, the 4-channels-per-wave stride-1 form of
conv3d_ks); without one the exact-fp32 forms (conv3d_t8, conv3d_ks on the fp32 pipe, conv3d_mfma).

Every case
  1. counts the launches of all five kernel families with the launch probe and asserts that the intended one -- and no
     other -- ran (a layer that silently lands on the exact-fp32 fallback passes every numeric check);
  2. pre-fills the output with NaN and asserts that none is left;
  3. compares the raw output and the normalised output scale * raw + shift with fp64;
  4. compares the returned folded coefficients with the fp64 statistics.

Dispatch (csrc/api.hip conv_block, in this order): conv3d_t8 takes every 8 -> 8 stride-1 layer (certified: the split
kernel of conv3d_t8x.hip); conv3d_ks takes Cin in {16, 32, 64, 128} up to an OUTPUT volume of 30 000 voxels (Cin = 128 at
stride 1 only for rows of at most 16 columns, never at stride 2); conv3d_nx takes certified 16 -> 16 stride-1 layers from
100 000 output voxels; conv3d_mfma takes the rest.  conv3d_nx tiles are 2 x 4 x 64 voxels, so 100 000 voxels are at least
196 tiles: the "fewer than 64 tiles" branch of its launch (no re-mapping over the 8 compute dies) cannot be reached
through the dispatch.  What can go wrong in the re-mapping is the tail -- 8 * ceil(tiles / 8) workgroups for `tiles` tiles
-- so the table has tile counts that divide by 8 (208, 224, 288) and that do not (250, 270, 350).

Kernel-selection switches (tests/test_gpu_switches.py runs this file under each of them): `expected_kernel` derives the
kernel a case must land on from the PDS_* variables of the process; the numeric checks never depend on them.

Tolerance: the project's single-layer bound (tests/test_gpu_conv_block.py), max-abs <= 2e-5 on the O(1) raw output and
5 x that on the normalised output.  That bound was stated for K = 576 products per output; the 128-channel layers sum
3 456.  The gate of a case is therefore max(2e-5, 3 * e32), e32 = the max-abs distance from fp64 of the CPU fp32
F.conv3d (+ LeakyReLU) of the same case -- measured against the reference, never against the HIP output.  The folded
coefficients are gated at 5 x the gate relative to max(1, |reference|): the rounding of the O(1) raw values enters the
variance as 2 sigma * err, and the coefficient as gamma / sigma^2 times that -- the same factor the project puts on the
normalised output.

e32 floors (tools/conv3d_e32_floors.py on the CPU, torch fp32 F.conv3d; K = 27 * Cin products per output; smallest and
largest value over the cases of that channel count):
    Cin =   8 (K =  216): 7.0e-7 .. 3.3e-6      3 * e32 <= 9.9e-6
    Cin =  16 (K =  432): 1.6e-6 .. 5.5e-6      3 * e32 <= 1.7e-5
    Cin =  32 (K =  864): 1.8e-6 .. 3.6e-6      3 * e32 <= 1.1e-5
    Cin =  64 (K = 1728): 1.4e-6 .. 1.8e-6      3 * e32 <= 5.6e-6
    Cin = 128 (K = 3456): 6.4e-7 .. 8.6e-7      3 * e32 <= 2.6e-6
so the flat 2e-5 governs every case of the table, the 128-channel layers included: the floor follows the number of
output voxels (the maximum is taken over more of them) and their magnitude, not K -- the CPU sums in blocks.
"""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from practicaldeepstereo_nips2018_amd import _lib

pytestmark = pytest.mark.gpu
TOL = 2e-5

NX, KS, T8, T8X, MFMA = 'conv3d_nx', 'conv3d_ks', 'conv3d_t8', 'conv3d_t8x', 'conv3d_mfma'
FAMILIES = (NX, KS, T8, T8X, MFMA)

# kernel, n, cin, cout, d, h, w (of the INPUT), stride, certified (x_bound given), note
CASES = [
    # ---- conv3d_nx: 16 -> 16, stride 1, certified, >= 100 000 voxels; tiles of 2 x 4 x 64 --------------------------------
    (NX, 1, 16, 16, 16, 52, 128, 1, True, 'exact tiling, 208 tiles'),
    (NX, 1, 16, 16, 15, 54, 125, 1, True, 'ragged on all three axes, 224 tiles'),
    (NX, 1, 16, 16, 10, 100, 100, 1, True, 'exactly 100 000 voxels; 250 tiles: 6 idle workgroups behind the re-mapping'),
    (MFMA, 1, 16, 16, 10, 100, 99, 1, True, '99 000 voxels: below the conv3d_nx threshold, above conv3d_ks'),
    (NX, 2, 16, 16, 11, 96, 96, 1, True, 'batch 2, 288 tiles per entry'),
    (NX, 1, 16, 16, 27, 100, 40, 1, True, 'rows narrower than a tile: every tile partial in x; 350 tiles'),
    (NX, 1, 16, 16, 9, 36, 321, 1, True, 'one column in the last tile of a row; odd D; 270 tiles'),
    (MFMA, 1, 16, 16, 15, 54, 125, 1, False, 'the ragged conv3d_nx layer without a certificate'),
    # ---- conv3d_ks, stride 1 (ks_plan: nb = 1 / 2 / 4 for rows <= 16 / <= 32 / wider) ------------------------------------
    (KS, 1, 16, 16, 6, 20, 40, 1, True, 'Cin 16, nb 4, ragged row; split form'),
    (KS, 1, 16, 16, 6, 20, 40, 1, False, 'Cin 16, nb 4: fp32 form'),
    (KS, 1, 32, 32, 5, 9, 24, 1, True, 'Cin 32, nb 2, ragged row; split form'),
    (KS, 1, 32, 32, 5, 9, 24, 1, False, 'Cin 32, nb 2: fp32 form'),
    (KS, 2, 32, 32, 3, 5, 33, 1, True, 'Cin 32, batch 2, 33 columns: one in the third 16-column block'),
    (KS, 1, 64, 64, 4, 6, 12, 1, True, 'Cin 64, nb 1 (8 channels per wave: fp32 form with or without a certificate)'),
    (KS, 1, 64, 64, 3, 5, 37, 1, False, 'Cin 64, nb 4, ragged'),
    (KS, 1, 128, 128, 2, 3, 6, 1, True, 'Cin 128: rows of at most 16 columns'),
    (KS, 1, 128, 128, 3, 2, 16, 1, False, 'Cin 128, a full 16-column row'),
    (MFMA, 1, 128, 128, 2, 4, 20, 1, True, 'Cin 128 with wider rows: no conv3d_ks configuration'),
    (KS, 1, 32, 32, 10, 50, 60, 1, True, 'exactly 30 000 voxels: the largest volume conv3d_ks serves'),
    (MFMA, 1, 32, 32, 10, 50, 61, 1, True, '30 500 voxels: above the conv3d_ks limit'),
    # ---- conv3d_ks, stride 2 (always the fp32 form) ------------------------------------------------------------------
    (KS, 1, 16, 32, 11, 17, 70, 2, True, '16 -> 32, odd D / H, output rows of 35 (nb 4)'),
    (KS, 1, 16, 32, 11, 17, 70, 2, False, '16 -> 32 without a certificate'),
    (KS, 1, 32, 64, 9, 13, 40, 2, True, '32 -> 64, odd D / H, output rows of 20 (nb 2)'),
    (KS, 2, 64, 128, 5, 7, 22, 2, True, '64 -> 128, odd D / H, output rows of 11 (nb 1), batch 2'),
    (KS, 1, 64, 128, 4, 6, 24, 2, False, '64 -> 128, even sizes'),
    # ---- conv3d_t8 / conv3d_t8x: 8 -> 8 at full signature resolution; tiles of 2 x 4 x 32 or 48 ---------------------------
    (T8X, 1, 8, 8, 6, 8, 64, 1, True, 'width / 32: EXACT form, 32-column tiles'),
    (T8, 1, 8, 8, 6, 8, 64, 1, False, 'width / 32, no certificate: exact-fp32 kernel'),
    (T8X, 1, 8, 8, 4, 8, 96, 1, True, 'width / 48: EXACT form, 48-column tiles'),
    (T8, 1, 8, 8, 4, 8, 96, 1, False, 'width / 48, no certificate'),
    (T8X, 1, 8, 8, 5, 10, 80, 1, True, 'width 80 (48-column tiles, 16 spare), odd D, H % 4 = 2: guarded form'),
    (T8, 1, 8, 8, 5, 10, 80, 1, False, 'width 80, no certificate'),
    (T8X, 2, 8, 8, 3, 7, 50, 1, True, 'ragged 50 columns (32-column tiles), batch 2'),
    (T8, 2, 8, 8, 3, 7, 50, 1, False, 'ragged 50 columns, batch 2, no certificate'),
    (T8X, 1, 8, 8, 2, 4, 32, 1, True, 'one tile: seven of the eight persistent workgroups idle'),
    (T8X, 1, 8, 8, 19, 94, 100, 1, True, '960 tiles over 512 persistent workgroups, ragged on all axes'),
    (T8, 1, 8, 8, 19, 94, 100, 1, False, '960 tiles, no certificate'),
    # ---- conv3d_mfma: what every PDS_*=0 switch falls back to --------------------------------------------------------
    (MFMA, 1, 8, 16, 9, 13, 42, 2, True, '8 -> 16 stride 2 (c0.down), odd D / H, output rows of 21'),
    (MFMA, 1, 8, 16, 20, 100, 200, 2, False, '8 -> 16 stride 2 over 100 000 output voxels: 16-wide tiles'),
    (MFMA, 2, 16, 16, 7, 50, 90, 1, True, '16 -> 16 between the conv3d_ks and conv3d_nx volumes, batch 2'),
]

def case_id(c):
    return '%s_n%d_%dto%d_%dx%dx%d_s%d_%s' % (c[0][7:], c[1], c[2], c[3], c[4], c[5], c[6], c[7], 'cert' if c[8] else 'nocert')


def output_volume(case):
    d, h, w, stride = case[4], case[5], case[6], case[7]
    return ((d + 1) // 2) * ((h + 1) // 2) * ((w + 1) // 2) if stride == 2 else d * h * w


def active_switches(environ=None):
    """The kernel-selection variables the library honours: only under PDS_DEBUG_SWITCHES=1 (csrc/common.hpp)."""
    environ = os.environ if environ is None else environ
    if not environ.get('PDS_DEBUG_SWITCHES', '').startswith('1'):
        return {}
    return {k: v for k, v in environ.items() if k.startswith('PDS_')}


def expected_kernel(case, switches):
    """The kernel family the case must land on: the intended one, unless a switch of this process turns it off -- then
    the fallback the dispatch of csrc/api.hip leaves (the exact-fp32 conv3d_t8 for conv3d_t8x, conv3d_mfma otherwise)."""
    kernel = case[0]

    def off(name):
        return switches.get(name, '')[:1] == '0'

    if kernel in (T8, T8X):
        if off('PDS_CONV3D_T8'):
            return MFMA
        if kernel == T8X and off('PDS_CONV3D_T8X'):
            return T8
        if kernel == T8 and switches.get('PDS_CONV3D_T8X', '')[:1] == '2':
            return T8X   # the split kernel (range-safe bf16 form) also for an un-certified single source
        return kernel
    if kernel == KS:
        limit = int(switches.get('PDS_CONV3D_KS_LIMIT', 30000))
        if off('PDS_CONV3D_KS') or output_volume(case) > limit:
            return MFMA
        return KS
    if kernel == NX:
        limit = int(switches.get('PDS_CONV3D_KS_LIMIT', 30000))
        if not off('PDS_CONV3D_KS') and output_volume(case) <= limit:
            return KS
        return MFMA if off('PDS_CONV3D_NX') else NX
    return kernel


def make_case(case, index):
    """Inputs of a case (CPU tensors): raw producer output, its folded coefficients, the block's parameters."""
    _, n, cin, cout, d, h, w, stride, certified, _ = case
    g = torch.Generator().manual_seed(5000 + index)
    x = torch.randn(n, cin, d, h, w, generator=g) * 37.0 + 5.0
    x_scale = (torch.rand(n, cin, 1, 1, 1, generator=g) + 0.5) / 37.0
    x_shift = torch.randn(n, cin, 1, 1, 1, generator=g) * 0.2 - 5.0 * x_scale
    weight = torch.randn(cout, cin, 3, 3, 3, generator=g) / (cin * 27) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    gamma = torch.rand(cout, generator=g) + 0.5
    beta = torch.randn(cout, generator=g) * 0.2
    # the fp32 normalised input the loader forms (one fma per element)
    xhat = torch.addcmul(x_shift.expand_as(x), x_scale.expand_as(x), x)
    return x, x_scale, x_shift, xhat, weight, bias, gamma, beta


def reference(xhat, weight, bias, gamma, beta, stride, dtype=torch.float64):
    """-> raw (LeakyReLU(conv)), normalised, folded scale and shift per (n, c); all in `dtype`."""
    y = F.conv3d(xhat.to(dtype), weight.to(dtype), bias.to(dtype), stride=stride, padding=1)
    raw = F.leaky_relu(y, 0.1)
    mean = raw.double().mean(dim=(2, 3, 4), keepdim=True)
    var = raw.double().var(dim=(2, 3, 4), unbiased=False, keepdim=True)
    scale = gamma.double().view(1, -1, 1, 1, 1) / torch.sqrt(var + 1e-5)
    shift = beta.double().view(1, -1, 1, 1, 1) - mean * scale
    return raw, raw.double() * scale + shift, scale.reshape(-1), shift.reshape(-1)


def fp32_floor(xhat, weight, bias, stride, want_raw):
    """e32: how far the CPU's own fp32 convolution of the case is from fp64."""
    y = F.leaky_relu(F.conv3d(xhat, weight, bias, stride=stride, padding=1), 0.1)
    return float((y.double() - want_raw).abs().max())


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def count_launches(lib, name, run):
    _lib.check(lib.pds_probe_begin(name.encode(), 16), 'pds_probe_begin')
    try:
        result = run()
        torch.cuda.synchronize()
    finally:
        count = lib.pds_probe_end(None, None, 16)
    assert count >= 0, lib.pds_last_error()
    return count, result


def launches_by_family(lib, run):
    """Launches of each 3-D kernel family in `run` (one run per probe name: the probe matches one substring at a time;
    'conv3d_t8' also matches 'conv3d_t8x', so the split kernel's count is subtracted) and the result of the last run."""
    counts, result = {}, None
    for name in FAMILIES:
        counts[name], result = count_launches(lib, name, run)
    counts[T8] -= counts[T8X]
    return counts, result


def run_layer(dev, case, x, x_scale, x_shift, bound, weight, bias, gamma, beta):
    """-> a closure that runs the layer once into fresh NaN-filled outputs and returns (raw, scale, shift) on the GPU."""
    lib = _lib.load()
    _, n, cin, cout, d, h, w, stride, certified, _ = case
    od, oh, ow = ((d + 1) // 2, (h + 1) // 2, (w + 1) // 2) if stride == 2 else (d, h, w)
    tensors = [t.to(dev).contiguous() for t in (weight, bias, gamma, beta)]
    params = _lib.ConvBlockParams()
    params.weight, params.bias = tensors[0].data_ptr(), tensors[1].data_ptr()
    params.gamma, params.beta = tensors[2].data_ptr(), tensors[3].data_ptr()
    ws = torch.empty(int(lib.pds_conv_block_workspace_bytes(n, cin, cout, d, h, w, 3, stride, 0)), dtype=torch.uint8,
                     device=dev)
    xg, sg, hg = x.to(dev), x_scale.reshape(-1).to(dev).contiguous(), x_shift.reshape(-1).to(dev).contiguous()
    bg = bound.reshape(1).to(dev) if bound is not None else None

    def run():
        raw = torch.full((n, cout, od, oh, ow), float('nan'), device=dev)
        scale = torch.full((n * cout,), float('nan'), device=dev)
        shift = torch.full((n * cout,), float('nan'), device=dev)
        _lib.check(lib.pds_conv_block_chained_fwd(ctypes.byref(params), _lib.ptr(xg), _lib.ptr(sg), _lib.ptr(hg), 0,
                                                  _lib.ptr(bg) if bg is not None else None, _lib.ptr(raw),
                                                  _lib.ptr(scale), _lib.ptr(shift), n, cin, cout, d, h, w, 3, stride, 0,
                                                  _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev)),
                   'pds_conv_block_chained_fwd')
        return raw, scale, shift, (tensors, xg, sg, hg, bg, ws)   # (the inputs stay alive until the run is synchronised)

    return run


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_conv3d_layer_against_fp64(dev, case):
    lib = _lib.load()
    kernel, n, cin, cout, d, h, w, stride, certified, note = case
    x, x_scale, x_shift, xhat, weight, bias, gamma, beta = make_case(case, CASES.index(case))
    bound = xhat.abs().max() if certified else None
    counts, (raw, scale, shift, _) = launches_by_family(
        lib, run_layer(dev, case, x, x_scale, x_shift, bound, weight, bias, gamma, beta))
    raw, scale, shift = raw.cpu(), scale.cpu().double(), shift.cpu().double()

    want_raw, want_normed, want_scale, want_shift = reference(xhat, weight, bias, gamma, beta, stride)
    e32 = fp32_floor(xhat, weight, bias, stride, want_raw)
    tol = max(TOL, 3.0 * e32)
    assert raw.shape == want_raw.shape
    finite = bool(torch.isfinite(raw).all())
    err = float((raw.double() - want_raw).abs().max()) if finite else float('nan')
    normed = raw.double() * scale.view(n, cout, 1, 1, 1) + shift.view(n, cout, 1, 1, 1)
    err_n = float((normed - want_normed).abs().max()) if finite else float('nan')
    err_scale = float(((scale - want_scale).abs() / want_scale.abs().clamp(min=1.0)).max())
    err_shift = float(((shift - want_shift).abs() / want_shift.abs().clamp(min=1.0)).max())
    print('conv3d layer %s (%s): launches %s  e32 %.2e  gate %.2e  raw err %.3g  normalised err %.3g  scale err %.3g  '
          'shift err %.3g' % (case_id(case), note, {k[7:]: v for k, v in counts.items() if v}, e32, tol, err, err_n,
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
    assert err_n <= 5 * tol, (err_n, 5 * tol)
    # 4. folded InstanceNorm coefficients
    assert err_scale <= 5 * tol, (err_scale, 5 * tol)
    assert err_shift <= 5 * tol, (err_shift, 5 * tol)
