"""GPU (-m gpu): the packed, coloured point cloud (point_cloud, StereoRig.point_cloud; pds_point_cloud_fwd).

A compaction moves values, it computes none: everything is compared exactly (array_equal on the int32 bit views of the
points, on the colours, on the index and on the offsets); there is no tolerance in this feature and no case is left out.
The arbiter of the values is the dense output of the existing `reproject` on the same inputs, compacted on the host by
oracle_cloud of tests/test_point_cloud_host.py (which is itself held to hand-written answers there): the contract is
"bit-equal to reproject", and the depth window is applied to that dense depth.  The kernels work on tiles of T = 1024
flat pixels (csrc/common.hpp: kPointCloudTile), four pixels per thread, and one workgroup of 1024 threads scans the tile
counts, so the shapes sit around T and one case has more tiles than that workgroup has threads.
"""
import ctypes

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib
from tests.test_gpu_speckle import plane_scene, simple_rig
from tests.test_point_cloud_host import oracle_cloud

pytestmark = pytest.mark.gpu

T = 1024   # csrc/common.hpp: kPointCloudTile
SCAN_THREADS = 1024   # csrc/point_cloud.hip: kPcScanThreads
NAN, INF = float('nan'), float('inf')


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def matrix_of(height, width):
    """A Q of a rig with focal length 0.7 * 200 px and a 0.12 m baseline: W = d / 0.12, depth = 16.8 / d."""
    return np.array([[1.0, 0.0, 0.0, -0.5 * (width - 1)], [0.0, 1.0, 0.0, -0.5 * (height - 1)], [0.0, 0.0, 0.0, 140.0],
                     [0.0, 0.0, 1.0 / 0.12, 0.0]])


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check(dev, disparity, matrix=None, image=None, valid=None, confidence=None, min_confidence=0.0, min_depth=None,
          max_depth=None, with_index=True, note=''):
    """Runs point_cloud and reproject on the same inputs and compares the cloud with the compacted dense points, bit for
    bit.  -> (the cloud, the oracle's (points, colors, index, offsets))."""
    disparity = np.asarray(disparity, dtype=np.float32)
    batch, height, width = disparity.shape
    matrix = matrix_of(height, width) if matrix is None else matrix
    put = (lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    d, im, v, c = put(disparity), put(image), put(valid), put(confidence)
    dense = pds.reproject(d, matrix, valid=v, confidence=c, min_confidence=min_confidence).cpu().numpy()
    expected = oracle_cloud(dense, image, min_depth, max_depth)
    cloud = pds.point_cloud(d, matrix, image=im, valid=v, confidence=c, min_confidence=min_confidence,
                            min_depth=min_depth, max_depth=max_depth, with_index=with_index)
    compare(cloud, expected, (note, disparity.shape), with_index=with_index)
    return cloud, expected


def compare(cloud, expected, case, with_index=True, rows=None):
    points, colors, index, offsets = expected
    assert isinstance(cloud, pds.PointCloud)
    assert cloud.offsets.dtype == torch.int32 and np.array_equal(cloud.offsets.cpu().numpy(), offsets), case
    n = int(offsets[-1]) if rows is None else rows
    got = cloud.points.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (n, 3), (case, got.shape, n)
    assert np.array_equal(bits(got), bits(points[:n])), case
    if colors is None:
        assert cloud.colors is None, case
    else:
        got = cloud.colors.cpu().numpy()
        assert got.dtype == colors.dtype and got.shape == (n, 3), case
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(colors[:n]).view(np.uint8)), case
    if with_index:
        assert cloud.index.dtype == torch.int32 and np.array_equal(cloud.index.cpu().numpy(), index[:n]), case
    else:
        assert cloud.index is None, case


# ------------------------------------------------------------------------------------------------ keep patterns
def kept_value(shape, seed):
    return (5.0 + 60.0 * np.random.RandomState(seed).rand(*shape)).astype(np.float32)


def from_mask(shape, seed, mask):
    return np.where(mask.reshape(shape), kept_value(shape, seed), np.float32(NAN)).astype(np.float32)


def flat_mask(shape, positions):
    mask = np.zeros(int(np.prod(shape)), dtype=bool)
    mask[list(positions)] = True
    return mask


def all_kept(shape, seed):
    return kept_value(shape, seed)


def none_kept(shape, seed):
    return np.full(shape, NAN, dtype=np.float32)


def first_only(shape, seed):
    return from_mask(shape, seed, flat_mask(shape, [0]))


def last_only(shape, seed):
    return from_mask(shape, seed, flat_mask(shape, [-1]))


def middle_of_the_last_tile(shape, seed):
    total = int(np.prod(shape))
    start = (total - 1) // T * T
    return from_mask(shape, seed, flat_mask(shape, [start + (total - start) // 2]))


def alternating_pixels(shape, seed):
    return from_mask(shape, seed, np.arange(int(np.prod(shape))) % 2 == seed % 2)


def alternating_tiles(shape, seed):
    return from_mask(shape, seed, np.arange(int(np.prod(shape))) // T % 2 == seed % 2)


def half(shape, seed):
    return from_mask(shape, seed, np.random.RandomState(100 + seed).rand(*shape) < 0.5)


def sparse(shape, seed):
    return from_mask(shape, seed, np.random.RandomState(200 + seed).rand(*shape) < 0.01)


def scene(shape, seed):
    return np.stack([plane_scene(shape[1], shape[2], seed=seed + b) for b in range(shape[0])])


SPECIAL = np.array([0.0, -0.0, -1.0, -1e-45, 1e-45, 1e-40, 1.1754942e-38, 1.1754944e-38, 3.0, 64.5, NAN, INF, -INF],
                   dtype=np.float32)


def zeros_negatives_and_denormals(shape, seed):
    """d <= 0 is rejected; a denormal d > 0 is kept (W = d / 0.12 > 0) and its point is whatever reproject makes of it."""
    return np.random.RandomState(300 + seed).choice(SPECIAL, shape)


def empty_middle_entry(shape, seed):
    d = half(shape, seed)
    d[shape[0] // 2] = NAN
    return d


PATTERNS = [all_kept, none_kept, first_only, last_only, middle_of_the_last_tile, alternating_pixels, alternating_tiles,
            half, sparse, scene, zeros_negatives_and_denormals, empty_middle_entry]
# widths 1, 3, 5, 63, 64, 65, 157 x heights 1, 2 x batches 1, 2, 3 (all below one tile), then shapes whose totals are
# T - 1, T, T + 1, 2 T and 2 T + 3 and shapes of the same widths that cross one or two tile borders
SMALL = [(b, h, w) for w in (1, 3, 5, 63, 64, 65, 157) for h in (1, 2) for b in (1, 2, 3)]
AROUND_T = [(1, 1, T - 1), (1, 1, T), (1, 1, T + 1), (1, 1, 2 * T + 3), (1, T - 1, 1), (1, T, 1), (1, T + 1, 1),
            (1, 2 * T + 3, 1), (3, 683, 1), (1, 400, 3), (2, 205, 5), (3, 17, 63), (1, 16, 64), (2, 16, 64), (3, 11, 65),
            (2, 7, 157), (1, 2, T // 2), (1, 2, T // 2 + 1), (3, 2, 341), (3, 2, 342)]


def image_of(shape, layout, seed):
    rng = np.random.RandomState(400 + seed)
    if layout == 'uint8':
        return rng.randint(0, 256, shape + (3,)).astype(np.uint8)
    return (rng.rand(shape[0], 3, shape[1], shape[2]) * 255).astype(np.float32)


@pytest.mark.parametrize('shape', AROUND_T, ids=lambda s: '%dx%dx%d' % s)
def test_point_cloud_equals_the_compacted_reprojection(dev, shape):
    for seed, pattern in enumerate(PATTERNS):
        layout = ('uint8', 'float32', None)[seed % 3]
        image = None if layout is None else image_of(shape, layout, seed)
        check(dev, pattern(shape, seed), image=image, with_index=seed % 2 == 0, note=pattern.__name__)


def test_small_shapes_of_every_width_height_and_batch(dev):
    for number, shape in enumerate(SMALL):
        for seed, pattern in enumerate(PATTERNS):
            layout = ('uint8', 'float32', None)[(seed + number) % 3]
            image = None if layout is None else image_of(shape, layout, seed)
            check(dev, pattern(shape, seed), image=image, with_index=(seed + number) % 2 == 0, note=pattern.__name__)


def test_known_answer(dev):
    d = torch.tensor([[[NAN, 8.0, -1.0], [4.0, 0.0, 2.0]]], device=dev)
    image = torch.arange(18, dtype=torch.uint8, device=dev).reshape(1, 2, 3, 3)
    cloud = pds.point_cloud(d, matrix_of(2, 3), image=image, with_index=True)
    assert cloud.offsets.tolist() == [0, 3] and cloud.index.tolist() == [1, 3, 5]
    assert cloud.colors.tolist() == [[3, 4, 5], [9, 10, 11], [15, 16, 17]]
    # (x - 1, y - 0.5, 140) / (d / 0.12)
    expected = np.array([[0.0, -0.5, 140.0], [-1.0, 0.5, 140.0], [1.0, 0.5, 140.0]]) * 0.12 / np.array([[8.0], [4.0], [2.0]])
    assert np.allclose(cloud.points.cpu().numpy(), expected, rtol=1e-6, atol=0)
    planes = torch.arange(18, dtype=torch.float32, device=dev).reshape(1, 3, 2, 3)
    assert pds.point_cloud(d, matrix_of(2, 3), image=planes).colors.tolist() == [[1, 7, 13], [3, 9, 15], [5, 11, 17]]
    entry = cloud.entry(0)
    assert entry.points.shape == (3, 3) and entry.index.tolist() == [1, 3, 5]


# ------------------------------------------------------------------------------------------------ rejection sources
def test_valid_confidence_and_the_depth_window_alone_and_together(dev):
    for shape in ((2, 7, 157), (3, 17, 63), (1, 2, T // 2 + 1)):
        rng = np.random.RandomState(sum(shape))
        d = scene(shape, 3)
        valid = rng.rand(*shape) > 0.3
        confidence = rng.rand(*shape).astype(np.float32)
        confidence[rng.rand(*shape) < 0.05] = NAN
        confidence[0, 0, :3] = (0.25, np.nextafter(np.float32(0.25), np.float32(0)), NAN)   # at, just below, NaN
        image = image_of(shape, 'uint8', 1)
        # bounds that ARE the computed depths of two pixels: both are kept
        dense = pds.reproject(torch.from_numpy(d).to(dev), matrix_of(*shape[1:])).cpu().numpy()
        depths = np.unique(dense[..., 2][~np.isnan(dense[..., 0])])
        low, high = float(depths[len(depths) // 4]), float(depths[3 * len(depths) // 4])
        assert low < high
        for use_valid in (False, True):
            for use_confidence in (False, True):
                for window in ((None, None), (low, None), (None, high), (low, high), (low, low)):
                    cloud, expected = check(dev, d, image=image, valid=valid if use_valid else None,
                                            confidence=confidence if use_confidence else None, min_confidence=0.25,
                                            min_depth=window[0], max_depth=window[1],
                                            note=(use_valid, use_confidence, window))
                    if not use_valid and not use_confidence:
                        z = cloud.points[:, 2].cpu().numpy()
                        for bound in window:   # the pixel whose depth equals the bound is in the cloud
                            assert bound is None or (z == np.float32(bound)).any(), window
                        if window == (low, low):
                            assert len(z) > 0 and (z == np.float32(low)).all()
        # a confidence equal to the threshold passes, one just below and a NaN do not (d[0, 0, :3] made eligible)
        d[0, 0, :3] = 30.0
        cloud, _ = check(dev, d, confidence=confidence, min_confidence=0.25)
        first_row = cloud.index[:int(cloud.offsets[1])].cpu().numpy()
        assert 0 in first_row and 1 not in first_row and 2 not in first_row


def rotated_rig(width, height):
    """simple_rig with two degrees between the cameras, so that R1 is no identity and the two frames differ."""
    K = np.array([[0.7 * width, 0.0, 0.5 * width - 0.5], [0.0, 0.7 * width, 0.5 * height - 0.5], [0.0, 0.0, 1.0]])
    R = pds.rectification.rodrigues(np.array([0.3, -0.8, 0.5]) / np.linalg.norm([0.3, -0.8, 0.5]) * np.radians(2.0))
    return pds.StereoRig(K, np.array([-0.05, 0.01, 1e-3, -5e-4]), K, np.array([-0.04, 0.02, -4e-4, 6e-4]), R,
                         np.array([-0.12, 0.004, -0.002]), (width, height))


def test_the_rig_in_both_frames(dev):
    d = torch.from_numpy(scene((2, 64, 157), 5)).to(dev)
    image = torch.from_numpy(image_of((2, 64, 157), 'float32', 2)).to(dev)
    valid = torch.from_numpy(np.random.RandomState(5).rand(2, 64, 157) > 0.2).to(dev)
    for rig in (simple_rig(157, 64), rotated_rig(157, 64)):
        for frame in ('rectified', 'camera'):
            dense = rig.reproject(d, valid=valid, frame=frame).cpu().numpy()
            cloud = rig.point_cloud(d, image, valid, frame=frame, with_index=True)
            compare(cloud, oracle_cloud(dense, image.cpu().numpy()), frame)
            window = rig.point_cloud(d, image, valid, frame=frame, min_depth=0.3, max_depth=0.6)
            compare(window, oracle_cloud(dense, image.cpu().numpy(), 0.3, 0.6), frame, with_index=False)
            assert 0 < int(window.offsets[-1]) < int(cloud.offsets[-1])
    assert not np.array_equal(rig.reprojection_matrix('camera'), rig.reprojection_matrix('rectified'))   # (the rotated one)


# ------------------------------------------------------------------------------------------------ large shapes
def large_case(dev, shape, seed):
    """-> (the cloud, the oracle's answer, a function that runs the same call again)."""
    d = scene(shape, seed)
    image = image_of(shape, 'uint8', seed)
    valid = np.random.RandomState(seed).rand(*shape) > 0.1
    cloud, expected = check(dev, d, image=image, valid=valid, min_depth=0.1, note='large')
    tensors = [torch.from_numpy(a).to(dev) for a in (d, image, valid)]
    return cloud, expected, lambda: pds.point_cloud(tensors[0], matrix_of(*shape[1:]), image=tensors[1],
                                                     valid=tensors[2], min_depth=0.1, with_index=True)


def test_more_tiles_than_the_scan_workgroup_has_threads(dev):
    shape = (1, 1100, 2048)
    assert shape[1] * shape[2] // T > 2 * SCAN_THREADS   # 2200 tiles: three rounds of the scan
    cloud, expected, rerun = large_case(dev, shape, 7)
    assert int(expected[3][-1]) > 1000000
    # determinism: the same bits on a second run
    again = rerun()
    for a, b in ((cloud.points.view(torch.int32), again.points.view(torch.int32)), (cloud.colors, again.colors),
                 (cloud.index, again.index), (cloud.offsets, again.offsets)):
        assert torch.equal(a, b)
    # all kept, and float colours: every tile is full
    check(dev, all_kept(shape, 1), image=image_of(shape, 'float32', 1), note='large, all kept')


def test_the_benchmark_batch(dev):
    cloud, expected, _ = large_case(dev, (4, 375, 1242), 11)   # 375 * 1242 is not a multiple of 4, nor of the tile
    offsets = expected[3]
    for b in range(4):
        entry = cloud.entry(b)
        assert entry.points.shape[0] == offsets[b + 1] - offsets[b] > 0
        assert np.array_equal(entry.index.cpu().numpy(), expected[2][offsets[b]:offsets[b + 1]])


# ------------------------------------------------------------------------------------------------ alignment
def off_by_one(t):
    """A contiguous copy of t that begins one element behind a 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:]
    flat.copy_(t.reshape(-1))
    return flat.view(t.shape)


def test_unaligned_inputs_and_outputs_agree(dev):
    lib = _lib.load()
    for shape in ((1, 33, 64), (2, 135, 240), (3, 2, 342)):
        count = shape[0] * shape[1] * shape[2]
        matrix = matrix_of(*shape[1:])
        d = torch.from_numpy(scene(shape, 2)).to(dev)
        valid = torch.from_numpy(np.random.RandomState(3).rand(*shape) > 0.2).to(dev)
        confidence = torch.from_numpy(np.random.RandomState(4).rand(*shape).astype(np.float32)).to(dev)
        for layout in ('uint8', 'float32'):
            image = torch.from_numpy(image_of(shape, layout, 6)).to(dev)
            aligned = pds.point_cloud(d, matrix, image=image, valid=valid, confidence=confidence, min_confidence=0.1,
                                      with_index=True)
            dense = pds.reproject(d, matrix, valid=valid, confidence=confidence, min_confidence=0.1).cpu().numpy()
            expected = oracle_cloud(dense, image.cpu().numpy())
            compare(aligned, expected, (shape, layout))
            n = int(expected[3][-1])
            # unaligned INPUTS: the scalar load form
            d1, v1, c1, i1 = off_by_one(d), off_by_one(valid), off_by_one(confidence), off_by_one(image)
            assert d1.data_ptr() % 16 == 4 and v1.data_ptr() % 4 == 1 and i1.data_ptr() % 16 == image.element_size()
            compare(pds.point_cloud(d1, matrix, image=i1, valid=v1, confidence=c1, min_confidence=0.1, with_index=True),
                    expected, (shape, layout, 'inputs'))
            # unaligned OUTPUTS: the entry point itself, every misalignment of the first row
            c_matrix = (ctypes.c_float * 16)(*matrix.astype(np.float32).reshape(-1).tolist())
            workspace = torch.empty(lib.pds_point_cloud_workspace_bytes(*shape), dtype=torch.uint8, device=dev)
            for shift in (1, 2, 3):
                cshift = shift if layout == 'float32' else shift + 4   # (bytes: 5, 6, 7 behind a 16-byte boundary)
                points = torch.full((3 * count + 8,), -7.0, device=dev)
                colors = torch.full((3 * count + 16,), 99, dtype=image.dtype, device=dev)
                index = torch.full((count + 8,), -5, dtype=torch.int32, device=dev)
                offsets = torch.full((shape[0] + 3,), -5, dtype=torch.int32, device=dev)
                _lib.check(lib.pds_point_cloud_fwd(
                    _lib.ptr(d), _lib.ptr(valid), _lib.ptr(confidence), 0.1, c_matrix, -INF, INF, _lib.ptr(image),
                    1 if layout == 'uint8' else 0, _lib.ptr(points[shift:]), _lib.ptr(colors[cshift:]),
                    _lib.ptr(index[shift:]), _lib.ptr(offsets[1:]), count, *shape, _lib.ptr(workspace),
                    workspace.numel(), _lib.stream_handle(dev)), 'pds_point_cloud_fwd')
                torch.cuda.synchronize()
                case = (shape, layout, shift)
                assert points[shift:].data_ptr() % 16 == 4 * shift
                assert np.array_equal(bits(points[shift:shift + 3 * n].cpu().numpy()), bits(expected[0]).reshape(-1)), case
                assert np.array_equal(colors[cshift:cshift + 3 * n].cpu().numpy(), expected[1].reshape(-1)), case
                assert np.array_equal(index[shift:shift + n].cpu().numpy(), expected[2]), case
                assert np.array_equal(offsets[1:shape[0] + 2].cpu().numpy(), expected[3]), case
                # nothing beside the rows is written
                assert bool((points[:shift] == -7.0).all()) and bool((points[shift + 3 * n:] == -7.0).all()), case
                assert bool((colors[:cshift] == 99).all()) and bool((colors[cshift + 3 * n:] == 99).all()), case
                assert bool((index[:shift] == -5).all()) and bool((index[shift + n:] == -5).all()), case
                assert offsets[0].item() == -5 and offsets[shape[0] + 2].item() == -5, case


# ------------------------------------------------------------------------------------------------ capacity
def test_capacity_cuts_the_cloud_and_nothing_is_written_behind_it(dev):
    lib = _lib.load()
    shape = (3, 17, 63)
    count = shape[0] * shape[1] * shape[2]
    matrix = matrix_of(*shape[1:])
    d = torch.from_numpy(half(shape, 1)).to(dev)
    image = torch.from_numpy(image_of(shape, 'uint8', 1)).to(dev)
    expected = oracle_cloud(pds.reproject(d, matrix).cpu().numpy(), image.cpu().numpy())
    n = int(expected[3][-1])
    assert n > T + 100   # the cut can fall into the second tile
    for capacity in (0, 1, 2, T - 1, T, T + 1, n - 1, n, n + 1, count):
        held = min(capacity, n)
        cloud = pds.point_cloud(d, matrix, image=image, with_index=True, capacity=capacity, trim=False)
        assert cloud.points.shape == (capacity, 3) and cloud.colors.shape == (capacity, 3)
        assert cloud.index.shape == (capacity,) and cloud.offsets.is_cuda
        assert np.array_equal(cloud.offsets.cpu().numpy(), expected[3]), capacity   # offsets[B] is the TRUE count
        assert np.array_equal(bits(cloud.points[:held].cpu().numpy()), bits(expected[0][:held])), capacity
        assert np.array_equal(cloud.colors[:held].cpu().numpy(), expected[1][:held]), capacity
        assert np.array_equal(cloud.index[:held].cpu().numpy(), expected[2][:held]), capacity
        assert cloud.size() == held
        rows = sum(cloud.entry(b).points.shape[0] for b in range(shape[0]))
        assert rows == held, capacity
        if capacity < n:
            with pytest.raises(RuntimeError, match='do not fit capacity %d' % capacity):
                pds.point_cloud(d, matrix, image=image, capacity=capacity)
        else:
            compare(pds.point_cloud(d, matrix, image=image, with_index=True, capacity=capacity), expected, capacity)
        # the entry point itself, into buffers one row larger that are filled with a sentinel
        if capacity == 0:
            continue
        c_matrix = (ctypes.c_float * 16)(*matrix.astype(np.float32).reshape(-1).tolist())
        workspace = torch.empty(lib.pds_point_cloud_workspace_bytes(*shape), dtype=torch.uint8, device=dev)
        points = torch.full((capacity + 1, 3), -7.0, device=dev)
        colors = torch.full((capacity + 1, 3), 99, dtype=torch.uint8, device=dev)
        index = torch.full((capacity + 1,), -5, dtype=torch.int32, device=dev)
        offsets = torch.empty(shape[0] + 1, dtype=torch.int32, device=dev)
        _lib.check(lib.pds_point_cloud_fwd(
            _lib.ptr(d), None, None, 0.0, c_matrix, -INF, INF, _lib.ptr(image), 1, _lib.ptr(points), _lib.ptr(colors),
            _lib.ptr(index), _lib.ptr(offsets), capacity, *shape, _lib.ptr(workspace), workspace.numel(),
            _lib.stream_handle(dev)), 'pds_point_cloud_fwd')
        torch.cuda.synchronize()
        assert np.array_equal(bits(points[:held].cpu().numpy()), bits(expected[0][:held])), capacity
        assert np.array_equal(colors[:held].cpu().numpy(), expected[1][:held]), capacity
        assert np.array_equal(index[:held].cpu().numpy(), expected[2][:held]), capacity
        assert bool((points[held:] == -7.0).all()) and bool((colors[held:] == 99).all()), capacity
        assert bool((index[held:] == -5).all()) and offsets[-1].item() == n, capacity


def test_untrimmed_call_does_not_wait_and_a_side_stream_agrees(dev):
    shape = (1, 540, 960)
    d = torch.from_numpy(scene(shape, 5)).to(dev)
    image = torch.from_numpy(image_of(shape, 'uint8', 5)).to(dev)
    matrix = matrix_of(*shape[1:])
    first = pds.point_cloud(d, matrix, image=image, with_index=True, trim=False)
    assert first.offsets.is_cuda and first.offsets.device == d.device and first.points.shape == (540 * 960, 3)
    assert '_host_offsets' not in first.__dict__   # nothing was read back
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        other = pds.point_cloud(d, matrix, image=image, with_index=True, trim=False)
        total = other.offsets[-1].clone()   # consumed on that stream
    stream.synchronize()
    torch.cuda.current_stream(dev).wait_stream(stream)
    n = int(total)
    assert n == int(first.offsets[-1]) and 0 < n < 540 * 960
    assert torch.equal(other.offsets, first.offsets)
    assert torch.equal(other.points[:n].view(torch.int32), first.points[:n].view(torch.int32))
    assert torch.equal(other.colors[:n], first.colors[:n]) and torch.equal(other.index[:n], first.index[:n])
    trimmed = pds.point_cloud(d, matrix, image=image, with_index=True)
    assert trimmed.points.shape == (n, 3) and torch.equal(trimmed.points.view(torch.int32),
                                                          first.points[:n].view(torch.int32))
    assert first.entry(0).points.shape == (n, 3)   # (the read happens here)


def test_the_three_kernels_ran(dev):
    lib = _lib.load()
    shape = (2, 65, 129)
    d = torch.from_numpy(scene(shape, 1)).to(dev)
    tiles = (2 * 65 * 129 + T - 1) // T
    for name, expected in (('point_cloud', [tiles, 1, tiles]), ('point_cloud_count', [tiles]),
                           ('point_cloud_scan', [1]), ('point_cloud_scatter', [tiles])):
        _lib.check(lib.pds_probe_begin(name.encode(), 16), 'pds_probe_begin')
        try:
            pds.point_cloud(d, matrix_of(65, 129), trim=False)
            torch.cuda.synchronize()
        finally:
            workgroups, ms = (ctypes.c_int * 16)(), (ctypes.c_float * 16)()
            count = lib.pds_probe_end(ms, workgroups, 16)
        assert count == len(expected), (name, count, lib.pds_last_error())
        assert list(workgroups[:count]) == expected and all(t >= 0 for t in ms[:count]), name


# ------------------------------------------------------------------------------------------------ integration
def test_the_cloud_of_a_reconstruction_is_its_points_compacted(dev):
    torch.manual_seed(0)
    net = pds.PdsNetwork.default(63).eval().to(dev)
    rig = simple_rig(256, 128)
    g = torch.Generator().manual_seed(3)
    left = torch.randint(0, 256, (1, 128, 256, 3), generator=g, dtype=torch.uint8).to(dev)
    right = torch.randint(0, 256, (1, 128, 256, 3), generator=g, dtype=torch.uint8).to(dev)
    for kwargs in ({}, {'max_difference': 1.0}, {'max_difference': 1.0, 'speckle_size': 2, 'speckle_difference': 8.0,
                                                 'median_size': 3}):
        r = rig.reconstruct(net, left, right, **kwargs)
        cloud = rig.point_cloud(r.disparity, r.left_image, r.valid, with_index=True)
        expected = oracle_cloud(r.points.cpu().numpy(), r.left_image.cpu().numpy())
        compare(cloud, expected, kwargs)
        assert cloud.colors.dtype == torch.float32 and int(cloud.offsets[-1]) > 0
        if r.valid is not None:
            assert int(cloud.offsets[-1]) <= int(r.valid.sum())
        print('reconstruct %s: %d of %d pixels became points' % (kwargs, int(cloud.offsets[-1]), 128 * 256))
