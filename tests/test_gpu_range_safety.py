"""GPU (-m gpu): the fp16-split kernels on statistics they were not tuned on: conv2d_x3 (P = 2) and conv2d_t8 of Matching;
conv3d_nx, conv3d_t8x, conv3d_ks (split and fp32 forms) and deconv3d_cell of the Regularization hourglass.

Round 3 scaled the fp16 operands by compile-time constants (weights x 2^10, normalised activations x 2^4): |w| >= 64,
a large gamma or a large plain residual sum overflowed to inf without an error.  Since round 4 both scales are powers
of two derived from the data -- max|w| at packing time, the range certificate that travels with every source
(common.hpp Src::bound: |gamma| sqrt(count) + |beta| from in_finalize, the producer's own maxima for plain tensors) --
and a source WITHOUT a certificate takes the range-safe bf16 form.  These tests use trained-checkpoint-like statistics
(reference benchmark_on_flyingthings3d.py:55-60 loads one; none is available offline): gamma log-uniform in [0.05, 20],
beta in +-5, heavy-tailed weights with a few |w| in [2, 100], inputs with outliers.  Bound: 2e-5 of the output scale
(max |reference|), the same relative accuracy as the 2e-5 absolute gate of the O(1) cases in test_gpu_conv_block.py.

The 3-D layers keep ONE set of InstanceNorm statistics per volume, so the certificate in_finalize writes is
max_c |gamma_c| sqrt(d h w) + |beta_c| over the whole volume: hundreds of times looser than the data at full size.  The
single-layer 3-D cases hand the kernels exactly that bound (and name, through the launch probe, the kernel that took the
layer); the whole-Regularization cases run the hourglass with checkpoint-like parameters at a shape whose inner levels
all run on conv3d_ks and at the smallest shape that puts the 16-channel level on conv3d_nx, and show through a child
process with PDS_CONV3D_KSX=0 PDS_DECONV_CELL_X=0 that the default run took the split forms of conv3d_ks and
deconv3d_cell (their launch names do not tell the forms apart).  Where a 3-D gate is compared with the fp32 CPU
restatement of the same case it is max(relative bound, 3 x that restatement's own distance from fp64).
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import pds_oracle as oracle
from tests import helpers
from tests import test_gpu_conv3d_layers as layers3d
from tests import test_gpu_parity as parity
import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib

pytestmark = pytest.mark.gpu

REL_TOL = 2e-5        # max |error| / max |reference|
REL_TOL_MEAN = 6e-7   # mean |error| / max |reference|


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def heavy_tailed_weights(g, cout, cin, outliers, kernel=(3, 3)):
    """He-like bulk plus `outliers` entries of magnitude 2 .. 100 (log-uniform, random sign); `kernel` = (3, 3) for a 2-D
    layer, three extents for a 3-D one."""
    taps = 1
    for k in kernel:
        taps *= k
    w = torch.randn(cout, cin, *kernel, generator=g) / (cin * taps) ** 0.5
    idx = torch.randperm(w.numel(), generator=g)[:outliers]
    mag = torch.exp(torch.rand(outliers, generator=g) * (torch.log(torch.tensor(100.0)) - torch.log(torch.tensor(2.0)))
                    + torch.log(torch.tensor(2.0)))
    sign = torch.where(torch.rand(outliers, generator=g) < 0.5, -1.0, 1.0)
    w.view(-1)[idx] = mag * sign
    return w


def log_uniform(g, n, lo, hi):
    return torch.exp(torch.rand(n, generator=g) * (torch.log(torch.tensor(hi)) - torch.log(torch.tensor(lo)))
                     + torch.log(torch.tensor(lo)))


def run_chained(dev, x, x_scale, x_shift, xpp, bound, weight, bias, gamma, beta):
    lib = _lib.load()
    n, cin, d, h, w = x.shape
    cout = weight.shape[0]
    tensors = [t.to(dev).contiguous() if t is not None else None for t in (weight, bias, gamma, beta)]
    params = _lib.ConvBlockParams()
    params.weight, params.bias = tensors[0].data_ptr(), tensors[1].data_ptr()
    params.gamma = tensors[2].data_ptr() if gamma is not None else None
    params.beta = tensors[3].data_ptr() if beta is not None else None
    raw = torch.full((n, cout, d, h, w), float('nan'), device=dev)
    scale = torch.zeros(n * cout * d, device=dev)
    shift = torch.zeros(n * cout * d, device=dev)
    ws = torch.empty(int(lib.pds_conv_block_workspace_bytes(n, cin, cout, d, h, w, 1, 1, 1)), dtype=torch.uint8, device=dev)
    xg, sg, hg = x.to(dev), x_scale.reshape(-1).to(dev).contiguous(), x_shift.reshape(-1).to(dev).contiguous()
    bg = bound.reshape(1).to(dev) if bound is not None else None
    _lib.check(lib.pds_conv_block_chained_fwd(ctypes.byref(params), _lib.ptr(xg), _lib.ptr(sg), _lib.ptr(hg), xpp,
                                              _lib.ptr(bg) if bg is not None else None, _lib.ptr(raw), _lib.ptr(scale),
                                              _lib.ptr(shift), n, cin, cout, d, h, w, 1, 1, 1, _lib.ptr(ws), ws.numel(),
                                              _lib.stream_handle(dev)),
               'pds_conv_block_chained_fwd')
    torch.cuda.synchronize()
    return raw.cpu()


def instance_norm_coefficients(x, gamma, beta):
    """Folded coefficients (per (n, c, d) plane) of InstanceNorm2d(affine) over the raw producer output x, and the
    rigorous bound in_finalize attaches to them."""
    n, c, d, h, w = x.shape
    xd = x.double()
    mean = xd.mean(dim=(3, 4), keepdim=True)
    var = xd.var(dim=(3, 4), unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    scale = gamma.double().view(1, c, 1, 1, 1) * rstd
    shift = beta.double().view(1, c, 1, 1, 1) - mean * scale
    bound = (gamma.abs() * (h * w) ** 0.5 + beta.abs()).max()
    return scale.float(), shift.float(), bound.float()


def reference_block(xhat, weight, bias, activation=True):
    """fp64 conv (+ LeakyReLU when the block has an InstanceNorm behind it: network_blocks.py:47-58; the bare 64 -> 8
    convolution of matching.py:89-93 has neither)."""
    n, cin, d, h, w = xhat.shape
    planes = xhat.double().permute(0, 2, 1, 3, 4).reshape(n * d, cin, h, w)
    y = F.conv2d(planes, weight.double(), bias.double(), padding=1)
    if activation:
        y = F.leaky_relu(y, 0.1)
    return y.reshape(n, d, -1, h, w).permute(0, 2, 1, 3, 4)


CASES = [
    # n, cin, d, h, w, cout
    (1, 64, 6, 48, 80, 64),     # conv2d_x3
    (2, 64, 3, 17, 47, 64),     # ragged
    (1, 64, 3, 20, 240, 8),     # conv2d_t8w (full-width rows)
    (1, 64, 2, 21, 36, 8),      # conv2d_t8 (16 x 32 tiles)
]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'n%d_%dto%d_d%d_%dx%d' % (c[0], c[1], c[5], c[2], c[3], c[4]))
def test_chained_block_trained_like_statistics(dev, case):
    n, cin, d, h, w, cout = case
    g = torch.Generator().manual_seed(1234 + w + cout)
    # raw producer output: LeakyReLU-like, far from unit scale, a few outliers of 50 sigma
    x = F.leaky_relu(torch.randn(n, cin, d, h, w, generator=g) * 11.0 + 3.0, 0.1)
    flat = x.view(-1)
    flat[torch.randperm(flat.numel(), generator=g)[:64]] *= 50.0
    gamma_in = log_uniform(g, cin, 0.05, 20.0) * torch.where(torch.rand(cin, generator=g) < 0.2, -1.0, 1.0)
    beta_in = (torch.rand(cin, generator=g) * 2 - 1) * 5.0
    x_scale, x_shift, bound = instance_norm_coefficients(x, gamma_in, beta_in)
    weight = heavy_tailed_weights(g, cout, cin, outliers=24)
    bias = torch.randn(cout, generator=g) * 2.0
    affine = cout == 64
    gamma = torch.ones(cout) if affine else None
    beta = torch.zeros(cout) if affine else None
    raw = run_chained(dev, x, x_scale, x_shift, 1, bound, weight, bias, gamma, beta)
    xhat = torch.addcmul(x_shift.expand_as(x), x_scale.expand_as(x), x)   # the fp32 value the loader forms
    want = reference_block(xhat, weight, bias, activation=affine)
    out_scale = float(want.abs().max())
    err = (raw.double() - want).abs()
    print('trained-like %s: |out| max %.3g  max err %.3g (%.2e rel)  mean err %.3g (%.2e rel)  max|w| %.1f  bound %.0f  max|x^| %.0f'
          % (case, out_scale, float(err.max()), float(err.max()) / out_scale, float(err.mean()),
             float(err.mean()) / out_scale, float(weight.abs().max()), float(bound), float(xhat.abs().max())))
    assert torch.isfinite(raw).all(), 'fp16 operands out of range'
    assert float(err.max()) <= REL_TOL * out_scale
    assert float(err.mean()) <= REL_TOL_MEAN * out_scale


def test_huge_activations_with_and_without_a_bound(dev):
    """Normalised activations up to ~5e6 and weights up to 1e3: round 3's constants (x 16, x 1024) made fp16 infinities
    of both.  With a range certificate the fp16 form scales them into range; without one (x_bound = NULL) the launch
    must take the range-safe bf16 form -- both finite and as accurate as ever."""
    n, cin, d, h, w, cout = 1, 64, 2, 33, 64, 64
    g = torch.Generator().manual_seed(99)
    x = torch.randn(n, cin, d, h, w, generator=g)
    x_scale = torch.full((n, cin, d, 1, 1), 1.0e6)
    x_shift = torch.full((n, cin, d, 1, 1), 3.0e5)
    weight = torch.randn(cout, cin, 3, 3, generator=g) * 40.0
    weight[3, 5, 1, 1] = 1000.0
    bias = torch.randn(cout, generator=g)
    xhat = torch.addcmul(x_shift.expand_as(x), x_scale.expand_as(x), x)
    want = reference_block(xhat, weight, bias)
    out_scale = float(want.abs().max())
    for bound in (xhat.abs().max() * 3.0, None):
        raw = run_chained(dev, x, x_scale, x_shift, 1, bound, weight, bias, torch.ones(cout), torch.zeros(cout))
        assert torch.isfinite(raw).all(), 'bound=%s' % (bound,)
        err = float((raw.double() - want).abs().max())
        print('huge activations, bound %s: max err %.3g of %.3g (%.2e rel)' % (bound is not None, err, out_scale, err / out_scale))
        assert err <= REL_TOL * out_scale, (bound is not None, err, out_scale)


def randomise_like_a_checkpoint(op, g, outliers=12):
    """MatchingOperation / Regularization parameters: `.2.weight` / `.2.bias` are the InstanceNorm affine terms of a block
    (network_blocks.py:47-85), 4-D and 5-D tensors the (transposed) convolution kernels, the other vectors convolution
    biases."""
    with torch.no_grad():
        for name, p in op.named_parameters():
            c = p.shape[0]
            if p.dim() in (4, 5):   # (Conv2d / Conv3d / ConvTranspose3d kernels)
                p.copy_(heavy_tailed_weights(g, p.shape[0], p.shape[1], outliers, tuple(p.shape[2:])))
            elif name.endswith('.2.weight'):
                p.copy_(log_uniform(g, c, 0.05, 20.0) * torch.where(torch.rand(c, generator=g) < 0.2, -1.0, 1.0))
            elif name.endswith('.2.bias'):
                p.copy_((torch.rand(c, generator=g) * 2 - 1) * 5.0)
            else:
                p.copy_(torch.randn(c, generator=g))


@pytest.mark.parametrize('descriptor_scale', [1.0, 300.0, 0.004])
def test_matching_trained_like_statistics(dev, descriptor_scale):
    """The whole fused Matching path (factorised first layers, three conv2d_x3 launches, residual sums, conv2d_t8) with
    checkpoint-like parameters and descriptors with outliers, against the oracle in fp64."""
    g = torch.Generator().manual_seed(4321)
    op = helpers.seeded(pds.MatchingOperation, seed=11)
    randomise_like_a_checkpoint(op, g)
    p64 = {k: v.double() for k, v in helpers.prefixed(op.state_dict(), '_m._operation').items()}
    batch, h, w, maxd = 1, 40, 72, 23
    left = torch.randn(batch, 64, h, w, generator=g) * descriptor_scale
    right = torch.randn(batch, 64, h, w, generator=g) * descriptor_scale
    left.view(-1)[torch.randperm(left.numel(), generator=g)[:32]] *= 40.0
    right.view(-1)[torch.randperm(right.numel(), generator=g)[:32]] *= 40.0
    ref = oracle.matching_with_operation(p64, '_m', left.double(), right.double(), maxd)
    ref32 = oracle.matching_with_operation({k: v.float() for k, v in p64.items()}, '_m', left, right, maxd)
    net = pds.Matching(maxd, op).to(dev)
    with torch.no_grad():
        out = net(left.to(dev), right.to(dev))
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    out_scale = float(ref.abs().max())
    err = float((out.cpu().double() - ref).abs().max())
    err32 = float((ref32.double() - ref).abs().max())
    print('matching, descriptors x %g: |signature| max %.3g, HIP vs fp64 %.3g (%.2e rel), fp32 CPU oracle vs fp64 %.3g (%.2e rel)'
          % (descriptor_scale, out_scale, err, err / out_scale, err32, err32 / out_scale))
    # six chained layers with |gamma| up to 20 amplify rounding noise: the gate is the fp32 CPU restatement's own
    # distance from fp64 (x 3) or the single-layer bound, whichever is larger
    assert err <= max(REL_TOL * out_scale, 3.0 * err32), (err, err32, out_scale)


def test_nonfinite_statistics_are_counted(dev):
    """ABI v5: a NaN that reaches an InstanceNorm'ed layer is reported through host-mapped memory instead of
    travelling silently (the reference has no such check; network_blocks.py:47-58)."""
    lib = _lib.load()
    op = helpers.seeded(pds.MatchingOperation, seed=3)
    net = pds.Matching(7, op).to(dev)
    g = torch.Generator().manual_seed(5)
    left = torch.randn(1, 64, 16, 32, generator=g).to(dev)
    right = torch.randn(1, 64, 16, 32, generator=g).to(dev)
    with torch.no_grad():
        net(left, right)
    torch.cuda.synchronize()
    assert lib.pds_nonfinite_statistics(1) == 0
    left[0, 3, 4, 5] = float('nan')
    with torch.no_grad():
        out = net(left, right)
    torch.cuda.synchronize()
    assert torch.isnan(out).any()
    assert lib.pds_nonfinite_statistics(1) > 0
    assert lib.pds_nonfinite_statistics(0) == 0


# ------------------------------------------------------------------------------------- the 3-D kernels of the hourglass
def volume_norm_coefficients(x, gamma, beta):
    """Folded coefficients (per (n, c): ONE set of statistics per volume) of InstanceNorm3d(affine) over the raw producer
    output x, and the certificate in_finalize attaches: max_c |gamma_c| sqrt(d h w) + |beta_c| over the VOLUME."""
    n, c, d, h, w = x.shape
    xd = x.double()
    mean = xd.mean(dim=(2, 3, 4), keepdim=True)
    var = xd.var(dim=(2, 3, 4), unbiased=False, keepdim=True)
    scale = gamma.double().view(1, c, 1, 1, 1) / torch.sqrt(var + 1e-5)
    shift = beta.double().view(1, c, 1, 1, 1) - mean * scale
    bound = (gamma.abs() * float(d * h * w) ** 0.5 + beta.abs()).max()
    return scale.float(), shift.float(), bound.float()


def run_layer_3d(dev, case, x, x_scale, x_shift, bound, weight, bias):
    """One 3-D block through pds_conv_block_chained_fwd -> (launches per kernel family, raw output on the host)."""
    cout = weight.shape[0]
    run = layers3d.run_layer(dev, case, x, x_scale, x_shift, bound, weight, bias, torch.ones(cout), torch.zeros(cout))
    counts, result = layers3d.launches_by_family(_lib.load(), run)
    return counts, result[0].cpu()


def relative_gate_3d(raw, xhat, weight, bias, stride):
    """-> (max error, mean error, max gate, mean gate, output scale): 2e-5 / 6e-7 of max |reference|, or 3 x the distance
    of the CPU's own fp32 convolution from fp64 where that is larger."""
    want = F.leaky_relu(F.conv3d(xhat.double(), weight.double(), bias.double(), stride=stride, padding=1), 0.1)
    cpu32 = F.leaky_relu(F.conv3d(xhat, weight, bias, stride=stride, padding=1), 0.1)
    floor = (cpu32.double() - want).abs()
    out_scale = float(want.abs().max())
    err = (raw.double() - want).abs()
    return (float(err.max()), float(err.mean()), max(REL_TOL * out_scale, 3.0 * float(floor.max())),
            max(REL_TOL_MEAN * out_scale, 3.0 * float(floor.mean())), out_scale)


CASES_3D = [
    # kernel, n, cin, cout, d, h, w, stride, certified, note (the layout of tests/test_gpu_conv3d_layers.py)
    (layers3d.NX, 1, 16, 16, 10, 100, 100, 1, True, 'conv3d_nx'),
    (layers3d.T8X, 1, 8, 8, 5, 10, 80, 1, True, 'conv3d_t8x, guarded form'),
    (layers3d.KS, 1, 32, 32, 5, 9, 24, 1, True, 'conv3d_ks stride 1, split form'),
    (layers3d.KS, 1, 16, 32, 11, 17, 70, 2, True, 'conv3d_ks stride 2'),
]


@pytest.mark.parametrize('case', CASES_3D, ids=layers3d.case_id)
def test_chained_3d_block_trained_like_statistics(dev, case):
    kernel, n, cin, cout, d, h, w, stride, _, _ = case
    g = torch.Generator().manual_seed(4321 + w + cout)
    x = F.leaky_relu(torch.randn(n, cin, d, h, w, generator=g) * 11.0 + 3.0, 0.1)
    flat = x.view(-1)
    flat[torch.randperm(flat.numel(), generator=g)[:64]] *= 50.0
    gamma_in = log_uniform(g, cin, 0.05, 20.0) * torch.where(torch.rand(cin, generator=g) < 0.2, -1.0, 1.0)
    beta_in = (torch.rand(cin, generator=g) * 2 - 1) * 5.0
    x_scale, x_shift, bound = volume_norm_coefficients(x, gamma_in, beta_in)
    weight = heavy_tailed_weights(g, cout, cin, outliers=24, kernel=(3, 3, 3))
    bias = torch.randn(cout, generator=g) * 2.0
    counts, raw = run_layer_3d(dev, case, x, x_scale, x_shift, bound, weight, bias)
    xhat = torch.addcmul(x_shift.expand_as(x), x_scale.expand_as(x), x)   # the fp32 value the loader forms
    finite = bool(torch.isfinite(raw).all())
    err, mean_err, gate, mean_gate, out_scale = relative_gate_3d(raw, xhat, weight, bias, stride)
    print('trained-like 3-D %s: launches %s  |out| max %.3g  max err %.3g (%.2e rel, gate %.3g)  mean err %.3g (%.2e rel, '
          'gate %.3g)  max|w| %.1f  bound %.0f  max|x^| %.0f'
          % (layers3d.case_id(case), {k: v for k, v in counts.items() if v}, out_scale, err, err / out_scale, gate, mean_err,
             mean_err / out_scale, mean_gate, float(weight.abs().max()), float(bound), float(xhat.abs().max())))
    assert counts[kernel] > 0 and sum(counts.values()) == counts[kernel], counts
    assert finite, 'fp16 operands out of range'
    assert err <= gate, (err, gate)
    assert mean_err <= mean_gate, (mean_err, mean_gate)


@pytest.mark.parametrize('case', [CASES_3D[0], CASES_3D[2]], ids=layers3d.case_id)
def test_huge_activations_with_and_without_a_bound_3d(dev, case):
    """The 3-D restatement of test_huge_activations_with_and_without_a_bound: normalised activations up to ~5e6 and
    weights up to 1e3.  With a certificate the split kernel scales both into fp16 range; without one the launch must take
    an fp32 form (conv3d_mfma for the conv3d_nx layer, the fp32 form of conv3d_ks) -- both finite and as accurate as ever."""
    kernel, n, cin, cout, d, h, w, stride, _, _ = case
    g = torch.Generator().manual_seed(99 + cin)
    x = torch.randn(n, cin, d, h, w, generator=g)
    x_scale = torch.full((n, cin, 1, 1, 1), 1.0e6)
    x_shift = torch.full((n, cin, 1, 1, 1), 3.0e5)
    weight = torch.randn(cout, cin, 3, 3, 3, generator=g) * 40.0
    weight[3, 5, 1, 1, 1] = 1000.0
    bias = torch.randn(cout, generator=g)
    xhat = torch.addcmul(x_shift.expand_as(x), x_scale.expand_as(x), x)
    for bound in (xhat.abs().max() * 3.0, None):
        counts, raw = run_layer_3d(dev, case, x, x_scale, x_shift, bound, weight, bias)
        finite = bool(torch.isfinite(raw).all())
        err, mean_err, gate, mean_gate, out_scale = relative_gate_3d(raw, xhat, weight, bias, stride)
        print('huge 3-D activations %s, bound %s: launches %s  max err %.3g of %.3g (%.2e rel, gate %.3g)'
              % (layers3d.case_id(case), bound is not None, {k: v for k, v in counts.items() if v}, err, out_scale,
                 err / out_scale, gate))
        want_kernel = kernel if (bound is not None or kernel == layers3d.KS) else layers3d.MFMA
        assert counts[want_kernel] > 0 and sum(counts.values()) == counts[want_kernel], (bound is not None, counts)
        if kernel == layers3d.KS:   # the launch name carries the form
            form = 'conv3d_ks<fp16>' if bound is not None else 'conv3d_ks<fp32>'
            run = layers3d.run_layer(dev, case, x, x_scale, x_shift, bound, weight, bias, torch.ones(cout), torch.zeros(cout))
            assert layers3d.count_launches(_lib.load(), form, run)[0] > 0, form
        assert finite, 'bound=%s' % (bound,)
        assert err <= gate, (bound is not None, err, gate)


def probe_module(name, run, capacity=64):
    lib = _lib.load()
    _lib.check(lib.pds_probe_begin(name.encode(), capacity), 'pds_probe_begin')
    try:
        result = run()
        torch.cuda.synchronize()
    finally:
        count = lib.pds_probe_end(None, None, capacity)
    return count, result


def checkpoint_like_regularization(shape):
    """-> (module on the host, fp64 parameters under the prefix '_r', signatures, shortcut)."""
    g = torch.Generator().manual_seed(8765)
    reg = helpers.seeded(pds.Regularization, seed=11)
    randomise_like_a_checkpoint(reg, g)
    p64 = {k: v.double() for k, v in helpers.prefixed(reg.state_dict(), '_r').items()}
    n, c, d, h, w = shape
    ms = torch.randn(n, c, d, h, w, generator=g)
    ms.view(-1)[torch.randperm(ms.numel(), generator=g)[:64]] *= 40.0
    shortcut = torch.randn(n, c, h, w, generator=g)
    return reg, p64, ms, shortcut


REGULARIZATION_SHAPES = [
    ((1, 8, 16, 32, 48), False),      # every inner level on conv3d_ks
    ((1, 8, 32, 160, 160), True),     # 819 200 voxels: the smallest legal shape with the 16-channel level on conv3d_nx
]


@pytest.mark.parametrize('shape,expect_nx', REGULARIZATION_SHAPES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else None)
def test_regularization_trained_like_statistics(dev, shape, expect_nx):
    """The whole hourglass with checkpoint-like parameters against the oracle in fp64, the kernels that ran, and the fused
    estimator against the oracle's estimator on the GPU's own cost volume (arg-max flips cannot hide there)."""
    reg, p64, ms, shortcut = checkpoint_like_regularization(shape)
    with torch.no_grad():
        ref = oracle.regularization(p64, '_r', ms.double(), shortcut.double())
        ref32 = oracle.regularization({k: v.float() for k, v in p64.items()}, '_r', ms, shortcut)
    reg = reg.to(dev)
    msg, sg = ms.to(dev), shortcut.to(dev)

    def forward():
        with torch.no_grad():
            return reg(msg, sg)

    launches = {}
    for name in ('conv3d_nx', 'deconv3d_cell', 'deconv3d_cell<fp16>', 'conv3d_ks', 'conv3d_t8x'):
        launches[name], cost = probe_module(name, forward)
    cost = cost.cpu()
    assert torch.isfinite(cost).all()
    out_scale = float(ref.abs().max())
    err = float((cost.double() - ref).abs().max())
    err32 = float((ref32.double() - ref).abs().max())
    print('regularization %s: launches %s  |cost| max %.3g, HIP vs fp64 %.3g (%.2e rel), fp32 CPU oracle vs fp64 %.3g (%.2e rel)'
          % (shape, launches, out_scale, err, err / out_scale, err32, err32 / out_scale))
    assert (launches['conv3d_nx'] > 0) == expect_nx, launches
    assert launches['deconv3d_cell'] > 0 and launches['conv3d_ks'] > 0 and launches['conv3d_t8x'] > 0, launches
    assert launches['deconv3d_cell<fp16>'] > 0, launches
    assert err <= max(REL_TOL * out_scale, 3.0 * err32), (err, err32, out_scale)

    est = pds.SubpixelMap()
    with torch.no_grad():
        fused = reg.forward_with_estimator(msg, sg, est)
    torch.cuda.synchronize()
    want = oracle.subpixel_map(cost)
    est_max, est_mae = helpers.maxdiff(fused, want), helpers.meandiff(fused, want)
    print('regularization %s: fused estimator vs the oracle on the GPU cost volume: max %.3g  MAE %.3g' % (shape, est_max, est_mae))
    assert est_max <= parity.TOL_EST_MAX, est_max
    assert est_mae <= parity.TOL_EST_MAE, est_mae


SPLIT_FORMS_CHILD = (
    "import sys, torch\n"
    "from tests import test_gpu_range_safety as rs\n"
    "reg, p64, ms, shortcut = rs.checkpoint_like_regularization(rs.REGULARIZATION_SHAPES[0][0])\n"
    "dev = torch.device('cuda:0'); reg = reg.to(dev)\n"
    "with torch.no_grad(): cost = reg(ms.to(dev), shortcut.to(dev))\n"
    "torch.cuda.synchronize()\n"
    "torch.save(cost.cpu(), sys.argv[1])\n")


def test_regularization_default_run_takes_the_split_forms(dev, tmp_path):
    """The launch name of the chained conv3d_ks kernel does not tell the fp16-split form of a layer from its fp32 form (nor
    does the transposed K-split kernel inside it): the small whole-Regularization case once more in a child interpreter
    with PDS_CONV3D_KSX=0 PDS_DECONV_CELL_X=0 (the switches are read once per process).  Both cost volumes meet the gate;
    they differ in at least one bit, so the default run did not compute on the fp32 pipe."""
    shape = REGULARIZATION_SHAPES[0][0]
    reg, p64, ms, shortcut = checkpoint_like_regularization(shape)
    with torch.no_grad():
        ref = oracle.regularization(p64, '_r', ms.double(), shortcut.double())
        ref32 = oracle.regularization({k: v.float() for k, v in p64.items()}, '_r', ms, shortcut)
        cost = reg.to(dev)(ms.to(dev), shortcut.to(dev)).cpu()
    env = dict(os.environ)
    env.update({'PDS_DEBUG_SWITCHES': '1', 'PDS_CONV3D_KSX': '0', 'PDS_DECONV_CELL_X': '0'})
    path = str(tmp_path / 'cost_fp32_forms.pt')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, '-c', SPLIT_FORMS_CHILD, path], cwd=root, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0, out.stdout.decode(errors='replace')[-2000:]
    exact = torch.load(path)
    out_scale = float(ref.abs().max())
    gate = max(REL_TOL * out_scale, 3.0 * float((ref32.double() - ref).abs().max()))
    err, err_exact = float((cost.double() - ref).abs().max()), float((exact.double() - ref).abs().max())
    differing = int((cost != exact).sum())
    print('regularization %s: split forms %.3g, fp32 forms %.3g (gate %.3g); %d of %d values differ'
          % (shape, err, err_exact, gate, differing, cost.numel()))
    assert torch.isfinite(cost).all() and torch.isfinite(exact).all()
    assert err <= gate and err_exact <= gate, (err, err_exact, gate)
    assert differing > 0, 'the default run is bit-identical to the run without the fp16-split forms'
