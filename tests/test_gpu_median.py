"""GPU (-m gpu): the hole-aware median filter (median_filter, StereoRig.reconstruct(median_size=...);
pds_median_filter_fwd).

A median is a selection: everything is compared exactly (numpy array_equal, with equal_nan for the values, which also
treats -0.0 and +0.0 as equal, as the contract does); there is no tolerance in this feature and no case is left out.
The arbiter is oracle_median of tests/test_median_host.py (gather, sort, take rank (n - 1) // 2), which is itself held
to hand-written answers there.  The kernel works on tiles of TILE_W x TILE_H = 64 x 16 pixels (csrc/median.hip:
kMedianTileW, kMedianTileH) with a halo of k // 2, four pixels of a row per thread, so the shapes below sit around the
tile and the patterns are chosen to break a selection: ties everywhere, every window population from 0 to k * k, the
ends of the fp32 range, denormals and both zeros.
"""
import ctypes

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib
from tests.test_gpu_speckle import plane_scene, same, simple_rig
from tests.test_median_host import oracle_finish, oracle_median, oracle_parts

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 64, 16   # csrc/median.hip: kMedianTileW, kMedianTileH
NAN = float('nan')
FLT_MAX = float(np.finfo(np.float32).max)
KERNEL_SIZES = (3, 5, 7)
# fill_holes, min_valid: off; on with the default (a majority of the full window); on with one sample
FILLS = ((False, None), (True, None), (True, 1))


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ patterns
def constant(height, width, seed):
    return np.full((height, width), 7.25 + seed, dtype=np.float32)


def ramp(height, width, seed):
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float32)
    return (0.9 * xx - (0.31 + 0.1 * seed) * yy).astype(np.float32)


def step_edge(height, width, seed):
    d = np.full((height, width), 12.5, dtype=np.float32)
    yy, xx = np.mgrid[0:height, 0:width]
    d[xx + (yy + seed) // 3 >= width // 2] = 80.0   # a slanted edge: every split of a window between the two surfaces
    return d


def checkerboard(height, width, seed):
    yy, xx = np.mgrid[0:height, 0:width]
    return np.where((yy + xx + seed) % 2 == 0, 0.0, 50.0).astype(np.float32)


def noise(height, width, seed):
    return (np.random.RandomState(seed).rand(height, width) * 192).astype(np.float32)


def three_values(height, width, seed):
    return np.random.RandomState(10 + seed).choice(np.array([3.0, 3.5, 40.0], dtype=np.float32), (height, width))


def scene(height, width, seed):
    return plane_scene(height, width, seed=seed)   # outliers, blobs, NaN / +-inf holes (tests/test_gpu_speckle.py)


def all_nan(height, width, seed):
    return np.full((height, width), NAN, dtype=np.float32)


def single_pixel(height, width, seed):
    d = np.full((height, width), NAN, dtype=np.float32)
    rng = np.random.RandomState(20 + seed)
    d[rng.randint(height), rng.randint(width)] = 33.0
    return d


SPECIAL = np.array([1e-45, -1e-45, 1e-40, -1e-42, 1.1754942e-38, 1.1754944e-38, 0.0, -0.0, FLT_MAX, -FLT_MAX, -5.5, 3.25,
                    -191.0, 1e30, -1e-30, NAN, np.inf, -np.inf], dtype=np.float32)


def special_values(height, width, seed):
    """fp32 denormals, both zeros, the ends of the range, negative disparities and a few holes."""
    return np.random.RandomState(30 + seed).choice(SPECIAL, (height, width))


PATTERNS = {'constant': constant, 'ramp': ramp, 'step edge': step_edge, 'checkerboard': checkerboard, 'noise': noise,
            'three values': three_values, 'plane scene': scene, 'plane scene, speckle filtered': None,
            'all NaN': all_nan, 'single pixel': single_pixel, 'special values': special_values}
# (batch, height, width): degenerate images, one less / equal / one more than the tile in either direction, the
# benchmark sizes (1242: the scalar store form, w % 4 != 0), a large image, and batches of four
SHAPES = [(1, 1, 1), (1, 1, 300), (1, 300, 1), (1, 2, 2), (1, 7, 5), (1, TILE_H - 1, TILE_W - 1), (1, TILE_H, TILE_W),
          (1, TILE_H + 1, TILE_W + 1), (1, TILE_H - 1, TILE_W + 1), (1, TILE_H + 1, TILE_W - 1), (1, 540, 960),
          (1, 375, 1242), (1, 1080, 1920), (4, 540, 960), (4, 375, 1242)]


def images_of(name, shape, dev):
    batch, height, width = shape
    if PATTERNS[name] is None:   # real hole shapes: what the speckle filter leaves of the plane scene
        raw = torch.from_numpy(np.stack([scene(height, width, s) for s in range(batch)])).to(dev)
        return pds.speckle_filter(raw, 20).disparity.cpu().numpy()
    return np.stack([PATTERNS[name](height, width, s) for s in range(batch)])


def check_against_oracle(dev, name, shape):
    images = images_of(name, shape, dev)
    d = torch.from_numpy(images).to(dev)
    mask = np.random.RandomState(sum(shape)).rand(*images.shape) > 0.15
    weights = np.random.RandomState(1 + sum(shape)).choice(np.array([1, 2, 7, 255], dtype=np.uint8), images.shape)
    masks = ((None, None), (mask, torch.from_numpy(mask).to(dev)), (mask, torch.from_numpy(mask * weights).to(dev)))
    assert masks[1][1].dtype == torch.bool and masks[2][1].dtype == torch.uint8
    checked = 0
    for k in KERNEL_SIZES:
        parts = {}
        for host_mask, device_mask in masks:
            key = host_mask is None
            if key not in parts:
                parts[key] = [oracle_parts(images[b], k, None if host_mask is None else host_mask[b])
                              for b in range(shape[0])]
            for fill_holes, min_valid in FILLS:
                got = pds.median_filter(d, k, valid=device_mask, fill_holes=fill_holes, min_valid=min_valid)
                assert isinstance(got, pds.MedianFiltered) and got.valid.dtype == torch.bool
                assert got.disparity.dtype == torch.float32 and got.disparity.shape == d.shape == got.valid.shape
                values, ok = got.disparity.cpu().numpy(), got.valid.cpu().numpy()
                for b in range(shape[0]):
                    expected, expected_ok = oracle_finish(parts[key][b], k, fill_holes, min_valid)
                    case = (name, shape, k, None if device_mask is None else str(device_mask.dtype), fill_holes,
                            min_valid, b)
                    assert np.array_equal(ok[b], expected_ok), (case, np.argwhere(ok[b] != expected_ok)[:5].tolist())
                    assert np.array_equal(values[b], expected, equal_nan=True), case
                    # one of the window's inputs bit for bit (a zero may come back with either sign)
                    exact = expected_ok & (expected != 0)
                    assert np.array_equal(values[b].view(np.int32)[exact], expected.view(np.int32)[exact]), case
                    checked += 1
    return checked


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_median_filter_against_the_oracle(dev, shape):
    checked = 0
    for name in PATTERNS:
        checked += check_against_oracle(dev, name, shape)
    assert checked == len(PATTERNS) * len(KERNEL_SIZES) * 3 * len(FILLS) * shape[0]
    print('%s: %d images compared with the oracle, all equal' % (shape, checked))


def test_known_answers(dev):
    d = torch.tensor([[[1, 2, 3], [4, 100, 6], [7, 8, 9]]], dtype=torch.float32, device=dev)
    out = pds.median_filter(d)   # kernel_size 3
    assert out.disparity[0].tolist() == [[2, 3, 3], [4, 6, 6], [7, 7, 8]] and out.valid.all()
    holes = torch.tensor([[[1, NAN, 3], [NAN, NAN, NAN], [7, 8, NAN]]], device=dev)
    out = pds.median_filter(holes, 3, fill_holes=True, min_valid=4, fill_value=-1.0)
    assert out.disparity[0, 1, 1].item() == 3.0 and out.valid[0, 1, 1].item()
    out = pds.median_filter(holes, 3, fill_holes=True, fill_value=-1.0)   # the default asks for 5 of 9
    assert out.disparity[0, 1, 1].item() == -1.0 and not out.valid[0, 1, 1].item()
    out = pds.median_filter(holes, 3, fill_holes=True, min_valid=1)
    assert out.disparity[0].tolist() == [[1, 1, 3], [7, 3, 3], [7, 7, 8]] and out.valid.all()
    assert torch.isnan(pds.median_filter(holes).disparity[0, 1, 1]).item()   # the default fill is NaN
    small = torch.tensor([[[4.0, 1.0], [3.0, 2.0]]], device=dev)
    assert pds.median_filter(small, 7).disparity[0].tolist() == [[2, 2], [2, 2]]
    for fill in (NAN, 0.0, -1.0, float('inf')):
        out = pds.median_filter(holes, 5, fill_value=fill)
        expected, ok = oracle_median(holes[0].cpu().numpy(), 5, fill_value=fill)
        assert np.array_equal(out.disparity[0].cpu().numpy(), expected, equal_nan=True)
        assert np.array_equal(out.valid[0].cpu().numpy(), ok)


def test_denormals_zeros_and_the_ends_of_the_range_come_through_unchanged(dev):
    """The selection compares integer keys, so no floating-point mode can flush or reorder a value."""
    units = np.array([[1, 3, 2], [1, 4, 2], [7, 6, 5]], dtype=np.int32)   # multiples of the smallest denormal, 1.4e-45
    sign = np.array([[0, 0, 0], [1, 0, 1], [0, 0, 0]], dtype=np.int32)
    tiny = (units | (sign << 31)).view(np.float32)
    assert np.all(tiny != 0) and np.all(np.abs(tiny) < np.finfo(np.float32).tiny)   # denormal: below 2^-126
    for k in KERNEL_SIZES:
        got = pds.median_filter(torch.from_numpy(tiny).to(dev)[None], k).disparity[0].cpu().numpy()
        expected = oracle_median(tiny, k)[0]
        assert np.array_equal(got.view(np.int32), expected.view(np.int32)), k
    # -2 -1 1 2 [3] 4 5 6 7
    assert bits(pds.median_filter(torch.from_numpy(tiny).to(dev)[None], 3).disparity)[0, 1, 1].item() == 3
    ends = torch.tensor([[[FLT_MAX, -FLT_MAX, FLT_MAX], [-FLT_MAX, 1.0, FLT_MAX], [-FLT_MAX, FLT_MAX, -FLT_MAX]]],
                        device=dev)
    out = pds.median_filter(ends, 3)
    assert out.disparity[0, 1, 1].item() == 1.0 and out.disparity[0, 0, 0].item() == -FLT_MAX
    zeros = torch.tensor([[[0.0, -0.0, 0.0, -0.0]]], device=dev)
    assert torch.equal(pds.median_filter(zeros, 3).disparity, torch.zeros_like(zeros))   # (0.0 == -0.0)


def test_images_of_a_batch_are_independent_and_runs_repeat(dev):
    for shape in ((65, 129), (375, 1242), (270, 480)):
        images = [noise(*shape, seed=1), scene(*shape, seed=2), three_values(*shape, seed=3), special_values(*shape, 4)]
        stacked = torch.from_numpy(np.stack(images)).to(dev)
        valid = stacked != 3.5   # (NaN != 3.5 is True: the NaN holes stay holes by their value)
        for k in KERNEL_SIZES:
            whole = pds.median_filter(stacked, k, valid=valid, fill_holes=True, min_valid=3)
            again = pds.median_filter(stacked, k, valid=valid, fill_holes=True, min_valid=3)
            assert torch.equal(bits(whole.disparity), bits(again.disparity)) and torch.equal(whole.valid, again.valid)
            for b in range(4):
                alone = pds.median_filter(stacked[b:b + 1], k, valid=valid[b:b + 1], fill_holes=True, min_valid=3)
                assert torch.equal(bits(alone.disparity[0]), bits(whole.disparity[b])), (shape, k, b)
                assert torch.equal(alone.valid[0], whole.valid[b]), (shape, k, b)


def test_on_a_side_stream(dev):
    d = torch.from_numpy(scene(540, 960, 5)).to(dev)[None]
    for k in KERNEL_SIZES:
        first = pds.median_filter(d, k, fill_holes=True)
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            other = pds.median_filter(d, k, fill_holes=True)
            count = other.valid.sum()   # consumed on that stream
        stream.synchronize()
        assert torch.equal(bits(other.disparity), bits(first.disparity)) and torch.equal(other.valid, first.valid)
        assert int(count) == int(first.valid.sum())
        torch.cuda.current_stream(dev).wait_stream(stream)


def test_non_contiguous_and_wrong_inputs(dev):
    d = torch.from_numpy(noise(129, 65, seed=4)).to(dev)[None]
    d[0, 5:9, 7:30] = NAN
    view = d.transpose(1, 2)   # [1, 65, 129], not contiguous
    valid = (torch.from_numpy(noise(129, 65, seed=5)).to(dev)[None] > 30).transpose(1, 2)
    assert not view.is_contiguous() and not valid.is_contiguous()
    sliced = torch.from_numpy(noise(70, 140, seed=6)).to(dev)[None][:, 3:68, 5:134]   # rows with a stride
    for k in KERNEL_SIZES:
        out = pds.median_filter(view, k, valid=valid, fill_holes=True)
        expected, ok = oracle_median(view[0].cpu().numpy(), k, valid[0].cpu().numpy(), fill_holes=True)
        assert np.array_equal(out.disparity[0].cpu().numpy(), expected, equal_nan=True), k
        assert np.array_equal(out.valid[0].cpu().numpy(), ok), k
        assert np.array_equal(pds.median_filter(sliced, k).disparity[0].cpu().numpy(),
                              oracle_median(sliced[0].cpu().numpy(), k)[0], equal_nan=True), k
    with pytest.raises(TypeError, match='float32'):
        pds.median_filter(d.double())
    with pytest.raises(ValueError, match='empty input'):
        pds.median_filter(torch.zeros(0, 4, 5, device=dev))
    with pytest.raises(ValueError, match='empty input'):
        pds.median_filter(torch.zeros(1, 0, 5, device=dev))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pds.median_filter(d, valid=torch.ones(1, 129, 65, dtype=torch.bool))
    with pytest.raises(ValueError, match='kernel_size'):
        pds.median_filter(d, 4)


def test_unaligned_pointers_take_the_scalar_form_and_agree(dev):
    """Tensors sliced by one element, so that their pointers are not 16-byte aligned (the masks not even 4-byte): as
    inputs of the Python call, and as outputs of the entry point, where they decide the store form."""
    lib = _lib.load()
    for shape in ((1, 33, 64), (2, 135, 240)):   # w % 4 == 0: the vector form but for the pointers
        count = shape[0] * shape[1] * shape[2]
        image = torch.from_numpy(np.stack([scene(shape[1], shape[2], s) for s in range(shape[0])])).to(dev)
        mask = torch.from_numpy(np.random.RandomState(3).rand(*shape) > 0.2).to(dev)
        d = torch.empty(count + 1, device=dev)[1:].view(shape)
        v = torch.empty(count + 1, dtype=torch.bool, device=dev)[1:].view(shape)
        d.copy_(image)
        v.copy_(mask)
        assert d.data_ptr() % 16 == 4 and v.data_ptr() % 4 == 1 and d.is_contiguous()
        for k in KERNEL_SIZES:
            aligned = pds.median_filter(image, k, valid=mask, fill_holes=True, min_valid=2)
            out = pds.median_filter(d, k, valid=v, fill_holes=True, min_valid=2)
            assert torch.equal(bits(out.disparity), bits(aligned.disparity)) and torch.equal(out.valid, aligned.valid)
            # unaligned OUTPUTS: the entry point itself
            filtered = torch.full((count + 1,), -7.0, device=dev)
            ok = torch.full((count + 3,), 9, dtype=torch.uint8, device=dev)
            _lib.check(lib.pds_median_filter_fwd(_lib.ptr(d), _lib.ptr(v), _lib.ptr(filtered[1:]), _lib.ptr(ok[1:]),
                                                 *shape, k, 1, 2, NAN, _lib.stream_handle(dev)), 'pds_median_filter_fwd')
            torch.cuda.synchronize()
            assert torch.equal(bits(filtered[1:].view(shape)), bits(aligned.disparity)), (shape, k)
            assert torch.equal(ok[1:count + 1].view(shape), aligned.valid.to(torch.uint8)), (shape, k)
            # nothing beside the outputs is written
            assert filtered[0].item() == -7.0 and ok[0].item() == 9 and ok[count + 1:].tolist() == [9, 9]
            # ok is optional
            filtered.fill_(-7.0)
            _lib.check(lib.pds_median_filter_fwd(_lib.ptr(d), None, _lib.ptr(filtered[1:]), None, *shape, k, 0, 1,
                                                 NAN, _lib.stream_handle(dev)), 'pds_median_filter_fwd')
            torch.cuda.synchronize()
            assert torch.equal(bits(filtered[1:].view(shape)), bits(pds.median_filter(image, k).disparity)), (shape, k)


def test_overlapping_buffers_are_refused(dev):
    lib = _lib.load()
    shape = (1, 40, 64)
    d = torch.from_numpy(noise(40, 64, 0)).to(dev)[None]
    before = d.clone()
    valid = torch.ones(shape, dtype=torch.uint8, device=dev)
    filtered, ok = torch.empty_like(d), torch.empty_like(valid)
    stream = _lib.stream_handle(dev)

    def call(disparity, valid_, filtered_, ok_):
        return lib.pds_median_filter_fwd(disparity, valid_, filtered_, ok_, *shape, 3, 0, 5, NAN, stream)

    assert call(_lib.ptr(d), _lib.ptr(valid), _lib.ptr(d), _lib.ptr(ok)) != 0
    assert b'filtered overlaps disparity' in lib.pds_last_error()
    assert call(_lib.ptr(d), _lib.ptr(valid), ctypes.c_void_p(d.data_ptr() + 16), _lib.ptr(ok)) != 0
    assert b'filtered overlaps disparity' in lib.pds_last_error()
    assert call(_lib.ptr(d), _lib.ptr(valid), _lib.ptr(filtered), _lib.ptr(valid)) != 0
    assert b'ok overlaps valid' in lib.pds_last_error()
    assert call(_lib.ptr(d), _lib.ptr(valid), _lib.ptr(filtered), ctypes.c_void_p(valid.data_ptr() + 64)) != 0
    assert b'ok overlaps valid' in lib.pds_last_error()
    assert call(_lib.ptr(d), _lib.ptr(valid), _lib.ptr(filtered), _lib.ptr(d)) != 0 and b'aliases' in lib.pds_last_error()
    torch.cuda.synchronize()
    assert torch.equal(d, before) and bool((valid == 1).all())   # nothing was launched
    assert call(_lib.ptr(d), _lib.ptr(valid), _lib.ptr(filtered), _lib.ptr(ok)) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(filtered), bits(pds.median_filter(d, 3, valid=valid).disparity))


# ------------------------------------------------------------------------------------------------ integration
def identical(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.dtype == torch.float32:
        return a.shape == b.shape and torch.equal(bits(a), bits(b))
    return a.dtype == b.dtype and torch.equal(a, b)


def test_reconstruct_with_the_median_filter_equals_the_steps_by_hand(dev):
    torch.manual_seed(0)
    net = pds.PdsNetwork.default(63).eval().to(dev)
    rig = simple_rig(256, 128)
    g = torch.Generator().manual_seed(3)
    left = torch.randint(0, 256, (1, 128, 256, 3), generator=g, dtype=torch.uint8).to(dev)
    right = torch.randint(0, 256, (1, 128, 256, 3), generator=g, dtype=torch.uint8).to(dev)
    with torch.no_grad():
        l, r = rig.rectify(left, right)
        checked = net.forward_left_right(l, r, max_difference=1.0)
        plain = net(l, r)

    def by_hand(disparity, valid, size, fill_holes, min_valid):
        filtered = pds.median_filter(disparity, size, valid=valid, fill_holes=fill_holes, min_valid=min_valid)
        return filtered, rig.reproject(filtered.disparity, valid=filtered.valid)

    for size, fill_holes, min_valid in ((3, False, None), (5, True, None), (7, True, 4), (3, True, 1)):
        kwargs = dict(median_size=size, median_fill_holes=fill_holes, median_min_valid=min_valid)
        # directly behind the network
        out = rig.reconstruct(net, left, right, **kwargs)
        filtered, points = by_hand(plain, None, size, fill_holes, min_valid)
        assert identical(out.disparity, filtered.disparity) and identical(out.valid, filtered.valid)
        assert same(out.points, points) and identical(out.left_image, l) and identical(out.right_image, r)
        assert out.valid.dtype == torch.bool and torch.equal(out.valid, torch.isfinite(plain))
        # behind the check
        out = rig.reconstruct(net, left, right, max_difference=1.0, **kwargs)
        filtered, points = by_hand(checked.left, checked.left_valid, size, fill_holes, min_valid)
        assert identical(out.disparity, filtered.disparity) and identical(out.valid, filtered.valid)
        assert same(out.points, points) and torch.isnan(out.points[~out.valid]).all()
        assert not (checked.left_valid & ~out.valid).any()   # an eligible pixel stays one
        if not fill_holes:
            assert torch.equal(out.valid, checked.left_valid & torch.isfinite(checked.left))
        # behind the check and the speckle filter, and behind the speckle filter alone
        for max_difference, disparity, mask in ((1.0, checked.left, checked.left_valid), (None, plain, None)):
            out = rig.reconstruct(net, left, right, max_difference=max_difference, speckle_size=2,
                                  speckle_difference=8.0, **kwargs)
            keep = pds.speckle_filter(disparity, 2, max_difference=8.0, valid=mask).keep
            filtered, points = by_hand(disparity, keep, size, fill_holes, min_valid)
            assert identical(out.disparity, filtered.disparity) and identical(out.valid, filtered.valid)
            assert same(out.points, points) and torch.isnan(out.points[~out.valid]).all()
            print('reconstruct: median %d (fill_holes %s, min_valid %s) behind %s: %d eligible pixels, %d points' %
                  (size, fill_holes, min_valid, 'check + speckle' if mask is not None else 'speckle', int(keep.sum()),
                   int(out.valid.sum())))

    # median_size=None is the call without the argument, byte for byte
    for kwargs in ({}, {'max_difference': 1.0}, {'max_difference': 1.0, 'speckle_size': 5}, {'speckle_size': 5}):
        a = rig.reconstruct(net, left, right, **kwargs)
        b = rig.reconstruct(net, left, right, median_size=None, median_fill_holes=True, median_min_valid=3, **kwargs)
        for x, y in zip(a, b):
            assert identical(x, y), kwargs
    # with the speckle filter alone the disparity stays the network's map
    assert identical(rig.reconstruct(net, left, right, speckle_size=5).disparity, plain)
    with pytest.raises(ValueError, match='kernel_size'):
        rig.reconstruct(net, left, right, median_size=4)
