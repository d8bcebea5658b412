"""GPU (-m gpu): the triangle mesh (triangle_mesh, StereoRig.triangle_mesh; pds_triangle_mesh_fwd).

Every output is an integer or a bit-copy, so everything is compared exactly (array_equal); there is no tolerance in this
feature and no case is left out.  The vertices are held to `point_cloud` on the same arguments (int32 views of the
points), the faces and face_offsets to oracle_mesh of tests/test_triangle_mesh_host.py (itself held to hand-written
answers there), fed with the kept mask derived from the dense output of `reproject` and the depth window, as
tests/test_gpu_point_cloud.py derives it.  The kernels work on tiles of T = 1024 flat pixels whose row below generally
lies in another tile, and one workgroup of 1024 threads scans the tile counts, so the shapes sit around T, end rows and
entries mid-tile, and one case has more tiles than that workgroup has threads.
"""
import ctypes

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib
from tests.test_gpu_point_cloud import image_of, matrix_of, off_by_one, rotated_rig, scene
from tests.test_gpu_speckle import simple_rig
from tests.test_triangle_mesh_host import check_invariants, oracle_mesh

pytestmark = pytest.mark.gpu

T = 1024   # csrc/common.hpp: kPointCloudTile
SCAN_THREADS = 1024   # csrc/point_cloud.hip: kPcScanThreads
NAN, INF = float('nan'), float('inf')


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.int32)


def kept_of(dev, d, matrix, valid=None, confidence=None, min_confidence=0.0, min_depth=None, max_depth=None):
    """The kept mask [B, H, W] (numpy) from the dense output of reproject and the depth window."""
    dense = pds.reproject(d, matrix, valid=valid, confidence=confidence, min_confidence=min_confidence).cpu().numpy()
    kept = ~np.isnan(dense[..., 0])
    if min_depth is not None:
        kept &= dense[..., 2] >= np.float32(min_depth)
    if max_depth is not None:
        kept &= dense[..., 2] <= np.float32(max_depth)
    return kept


def same_vertices(mesh, cloud, case):
    assert torch.equal(mesh.offsets, cloud.offsets) and mesh.offsets.dtype == torch.int32, case
    assert mesh.points.shape == cloud.points.shape and np.array_equal(bits(mesh.points), bits(cloud.points)), case
    for a, b in ((mesh.colors, cloud.colors), (mesh.index, cloud.index)):
        assert (a is None) == (b is None), case
        if a is not None:
            assert a.dtype == b.dtype and torch.equal(a, b), case


def check(dev, disparity, max_difference=1.0, flip=False, image=None, valid=None, confidence=None, min_confidence=0.0,
          min_depth=None, max_depth=None, with_index=True, note=''):
    """Runs triangle_mesh, point_cloud and reproject on the same inputs; vertices against the cloud, faces against the
    oracle, all bit for bit.  -> (the mesh, the oracle's (faces, face_offsets), the kept mask)."""
    disparity = np.asarray(disparity, dtype=np.float32)
    matrix = matrix_of(*disparity.shape[1:])
    put = (lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    d, im, v, c = put(disparity), put(image), put(valid), put(confidence)
    common = dict(image=im, valid=v, confidence=c, min_confidence=min_confidence, min_depth=min_depth,
                  max_depth=max_depth, with_index=with_index)
    kept = kept_of(dev, d, matrix, v, c, min_confidence, min_depth, max_depth)
    expected = oracle_mesh(disparity, kept, max_difference, flip)
    mesh = pds.triangle_mesh(d, matrix, max_difference=max_difference, flip=flip, **common)
    case = (note, disparity.shape, max_difference, flip)
    assert isinstance(mesh, pds.TriangleMesh), case
    same_vertices(mesh, pds.point_cloud(d, matrix, **common), case)
    assert mesh.face_offsets.dtype == torch.int32 and mesh.faces.dtype == torch.int32, case
    assert np.array_equal(mesh.face_offsets.cpu().numpy(), expected[1]), (case, mesh.face_offsets.tolist(), expected[1])
    assert mesh.faces.shape == expected[0].shape, (case, mesh.faces.shape, expected[0].shape)
    assert np.array_equal(mesh.faces.cpu().numpy(), expected[0]), case
    return mesh, expected, kept


# ------------------------------------------------------------------------------------------------ patterns
# each: (shape, seed) -> (disparity, max_difference)
def values(shape, seed):
    return (20.0 + np.random.RandomState(seed).rand(*shape)).astype(np.float32)   # differences below 1


def constant(shape, seed):
    return np.full(shape, 12.5, dtype=np.float32), 1.0   # all kept, ties everywhere


def random_half(shape, seed):
    return values(shape, seed), 0.5


def random_unbounded(shape, seed):
    return values(shape, seed) * np.float32(40.0), INF


def checkerboard(shape, seed):
    yy, xx = np.mgrid[0:shape[1], 0:shape[2]]
    return np.where(((xx + yy + seed) % 2 == 0)[None], values(shape, seed), np.float32(NAN)).astype(np.float32), INF


def every_third_missing(shape, seed):
    flat = np.arange(int(np.prod(shape))).reshape(shape)
    return np.where(flat % 3 == seed % 3, np.float32(NAN), values(shape, seed)).astype(np.float32), 1.0


def missing_rows(shape, seed):
    d = values(shape, seed)
    d[:, seed % 3::3] = NAN
    return d, 1.0


def vertical_step(shape, seed):
    d = values(shape, seed) * np.float32(0.25)
    d[:, :, shape[2] // 2:] += 30.0
    return d, 1.0


def diagonal_step(shape, seed):
    yy, xx = np.mgrid[0:shape[1], 0:shape[2]]
    d = values(shape, seed) * np.float32(0.25)
    return (d + np.where(xx + yy > (shape[1] + shape[2]) // 2, 30.0, 0.0)[None]).astype(np.float32), 1.0


SPECIAL = np.array([0.0, -0.0, -1.0, 1e-45, 3.0, 3.5, 4.0, 64.5, NAN, INF, -INF], dtype=np.float32)


def specials(shape, seed):
    return np.random.RandomState(300 + seed).choice(SPECIAL, shape), 1.0


def repeated_values_threshold_zero(shape, seed):
    return np.random.RandomState(500 + seed).randint(3, 6, shape).astype(np.float32), 0.0


def plane_scene(shape, seed):
    return scene(shape, seed), 1.0


def holes(shape, seed):
    d = values(shape, seed)
    d[np.random.RandomState(600 + seed).rand(*shape) < 0.3] = NAN
    return d, 0.75


PATTERNS = [constant, random_half, random_unbounded, checkerboard, every_third_missing, missing_rows, vertical_step,
            diagonal_step, specials, repeated_values_threshold_zero, plane_scene, holes]
# the row below lies in the next tile or straddles two; the last row of an entry and the end of a row lie mid-tile
SHAPES = [(1, 2, 2), (1, 1, 5), (1, 5, 1), (1, 2, 513), (1, 3, 1024), (1, 2, 1025), (2, 33, 31), (3, 17, 61), (4, 9, 257)]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_mesh_equals_the_cloud_and_the_oracle(dev, shape):
    faces = 0
    for seed, pattern in enumerate(PATTERNS):
        d, max_difference = pattern(shape, seed)
        layout = ('uint8', 'float32', None)[seed % 3]
        image = None if layout is None else image_of(shape, layout, seed)
        mesh, _, _ = check(dev, d, max_difference, flip=seed % 2 == 1, image=image, with_index=seed % 2 == 0,
                           note=pattern.__name__)
        if pattern is checkerboard or shape[1] == 1 or shape[2] == 1:
            assert mesh.faces.shape == (0, 3) and mesh.face_offsets.tolist() == [0] * (shape[0] + 1)
        if pattern is constant and shape[1] > 1 and shape[2] > 1:
            assert mesh.faces.shape[0] == 2 * shape[0] * (shape[1] - 1) * (shape[2] - 1)
        faces += mesh.faces.shape[0]
    assert faces > 0 or shape[1] == 1 or shape[2] == 1


def test_small_shapes_of_every_width_height_and_batch(dev):
    number = 0
    for width in range(1, 10):
        for height in range(1, 6):
            for batch in range(1, 4):
                shape = (batch, height, width)
                for seed in (number % len(PATTERNS), (number + 5) % len(PATTERNS)):
                    d, max_difference = PATTERNS[seed](shape, seed)
                    check(dev, d, max_difference, flip=number % 2 == 1, note=PATTERNS[seed].__name__)
                number += 1


def test_known_answer(dev):
    d = torch.tensor([[[10.0, 10.0, 40.0], [10.0, NAN, 40.0], [10.0, 10.0, 40.0]]], device=dev)
    mesh = pds.triangle_mesh(d, matrix_of(3, 3), with_index=True)
    assert mesh.index.tolist() == [0, 1, 2, 3, 5, 6, 7, 8] and mesh.offsets.tolist() == [0, 8]
    # cell (0, 0): e missing, (a, c, b); cell (0, 1): c missing, (a, e, b) crosses the step; cell (1, 0): b missing,
    # (a, c, e); cell (1, 1): a missing, (b, c, e) crosses the step
    assert mesh.faces.tolist() == [[0, 3, 1], [3, 5, 6]] and mesh.face_offsets.tolist() == [0, 2]
    unbounded = pds.triangle_mesh(d, matrix_of(3, 3), max_difference=INF, flip=True)
    assert unbounded.faces.tolist() == [[0, 1, 3], [1, 2, 4], [3, 6, 5], [4, 7, 6]]
    assert mesh.size() == 8 and mesh.face_count() == 2 and mesh.entry(0).faces.tolist() == [[0, 3, 1], [3, 5, 6]]


def test_more_tiles_than_the_scan_workgroup_has_threads(dev):
    shape = (1, 1026, 1023)
    assert (shape[1] * shape[2] + T - 1) // T == SCAN_THREADS + 1   # 1025 tiles: a second round of the scan
    for seed, pattern in ((3, plane_scene), (4, holes)):
        d, max_difference = pattern(shape, seed)
        mesh, expected, _ = check(dev, d, max_difference, image=image_of(shape, 'uint8', seed), note='large')
        assert len(expected[0]) > 500000


# ------------------------------------------------------------------------------------------------ rejection sources
def test_valid_confidence_and_the_depth_window_alone_and_together(dev):
    shape = (2, 33, 61)
    rng = np.random.RandomState(7)
    d = scene(shape, 3)
    valid = rng.rand(*shape) > 0.2
    confidence = rng.rand(*shape).astype(np.float32)
    confidence[rng.rand(*shape) < 0.05] = NAN
    dense = pds.reproject(torch.from_numpy(d).to(dev), matrix_of(*shape[1:])).cpu().numpy()
    depths = np.unique(dense[..., 2][~np.isnan(dense[..., 0])])
    low, high = float(depths[len(depths) // 8]), float(depths[7 * len(depths) // 8])
    counts = set()
    for use_valid in (False, True):
        for use_confidence in (False, True):
            for window in ((None, None), (low, None), (None, high), (low, high)):
                mesh, _, _ = check(dev, d, 1.0, valid=valid if use_valid else None,
                                   confidence=confidence if use_confidence else None, min_confidence=0.25,
                                   min_depth=window[0], max_depth=window[1], image=image_of(shape, 'float32', 1),
                                   note=(use_valid, use_confidence, window))
                counts.add(int(mesh.face_offsets[-1]))
    assert len(counts) >= 4   # the sources do decide


# ------------------------------------------------------------------------------------------------ alignment
def test_unaligned_inputs_and_outputs_agree(dev):
    lib = _lib.load()
    for shape in ((1, 33, 64), (3, 2, 342)):
        count = shape[0] * shape[1] * shape[2]
        matrix = matrix_of(*shape[1:])
        d = torch.from_numpy(scene(shape, 2)).to(dev)
        valid = torch.from_numpy(np.random.RandomState(3).rand(*shape) > 0.1).to(dev)
        image = torch.from_numpy(image_of(shape, 'uint8', 6)).to(dev)
        aligned = pds.triangle_mesh(d, matrix, image=image, valid=valid, with_index=True)
        expected = oracle_mesh(d.cpu().numpy(), kept_of(dev, d, matrix, valid), 1.0)
        assert np.array_equal(aligned.faces.cpu().numpy(), expected[0]) and len(expected[0]) > 100
        n, f = aligned.size(), aligned.face_count()
        # unaligned INPUTS: the scalar load form of the vertex kernels
        d1, v1, i1 = off_by_one(d), off_by_one(valid), off_by_one(image)
        assert d1.data_ptr() % 16 == 4
        other = pds.triangle_mesh(d1, matrix, image=i1, valid=v1, with_index=True)
        same_vertices(other, aligned, shape)
        assert torch.equal(other.faces, aligned.faces) and torch.equal(other.face_offsets, aligned.face_offsets)
        # unaligned OUTPUTS: the entry point itself, every misalignment of the first row
        c_matrix = (ctypes.c_float * 16)(*matrix.astype(np.float32).reshape(-1).tolist())
        workspace = torch.empty(lib.pds_triangle_mesh_workspace_bytes(*shape), dtype=torch.uint8, device=dev)
        assert workspace.data_ptr() % 16 == 0
        for shift in (1, 2, 3):
            points = torch.full((3 * count + 8,), -7.0, device=dev)
            colors = torch.full((3 * count + 16,), 99, dtype=torch.uint8, device=dev)
            index = torch.full((count + 8,), -5, dtype=torch.int32, device=dev)
            faces = torch.full((6 * count + 8,), -9, dtype=torch.int32, device=dev)
            offsets = torch.full((2 * shape[0] + 6,), -5, dtype=torch.int32, device=dev)
            face_offsets = offsets[shape[0] + 3:]
            _lib.check(lib.pds_triangle_mesh_fwd(
                _lib.ptr(d1), _lib.ptr(v1), None, 0.0, c_matrix, -INF, INF, 1.0, 0, _lib.ptr(i1), 1,
                _lib.ptr(points[shift:]), _lib.ptr(colors[shift + 4:]), _lib.ptr(index[shift:]), _lib.ptr(offsets[1:]),
                count, _lib.ptr(faces[shift:]), _lib.ptr(face_offsets[1:]), 2 * count, *shape, _lib.ptr(workspace),
                workspace.numel(), _lib.stream_handle(dev)), 'pds_triangle_mesh_fwd')
            torch.cuda.synchronize()
            case = (shape, shift)
            assert faces[shift:].data_ptr() % 16 == 4 * shift and points[shift:].data_ptr() % 16 == 4 * shift
            assert torch.equal(faces[shift:shift + 3 * f], aligned.faces.reshape(-1)), case
            assert torch.equal(points[shift:shift + 3 * n].view(torch.int32), aligned.points.reshape(-1).view(torch.int32))
            assert torch.equal(colors[shift + 4:shift + 4 + 3 * n], aligned.colors.reshape(-1)), case
            assert torch.equal(index[shift:shift + n], aligned.index), case
            assert torch.equal(offsets[1:shape[0] + 2], aligned.offsets), case
            assert torch.equal(face_offsets[1:shape[0] + 2], aligned.face_offsets), case
            # nothing beside the rows is written
            assert bool((faces[:shift] == -9).all()) and bool((faces[shift + 3 * f:] == -9).all()), case
            assert bool((points[:shift] == -7.0).all()) and bool((points[shift + 3 * n:] == -7.0).all()), case
            assert bool((index[:shift] == -5).all()) and bool((index[shift + n:] == -5).all()), case
            assert offsets[0].item() == -5 and offsets[shape[0] + 2].item() == -5, case
            assert face_offsets[0].item() == -5 and face_offsets[shape[0] + 2].item() == -5, case


# ------------------------------------------------------------------------------------------------ capacity
def test_capacities_cut_and_nothing_is_written_behind_them(dev):
    lib = _lib.load()
    shape = (3, 17, 63)
    count = shape[0] * shape[1] * shape[2]
    matrix = matrix_of(*shape[1:])
    d = torch.from_numpy(holes(shape, 1)[0]).to(dev)
    full = pds.triangle_mesh(d, matrix, max_difference=0.75, with_index=True)
    expected = oracle_mesh(d.cpu().numpy(), kept_of(dev, d, matrix), 0.75)
    assert np.array_equal(full.faces.cpu().numpy(), expected[0])
    n, f = full.size(), full.face_count()
    assert n > T + 100 and f > T + 100   # a cut can fall into the second tile
    c_matrix = (ctypes.c_float * 16)(*matrix.astype(np.float32).reshape(-1).tolist())
    workspace = torch.empty(lib.pds_triangle_mesh_workspace_bytes(*shape), dtype=torch.uint8, device=dev)
    for capacity, face_capacity in ((count, 0), (count, 1), (count, T - 1), (count, T + 1), (count, f - 1), (count, f),
                                    (n, f + 1), (n - 1, 2 * count), (T + 1, f), (1, T), (0, 0)):
        held, face_held = min(capacity, n), min(face_capacity, f)
        mesh = pds.triangle_mesh(d, matrix, max_difference=0.75, with_index=True, capacity=capacity,
                                 face_capacity=face_capacity, trim=False)
        case = (capacity, face_capacity)
        assert mesh.points.shape == (capacity, 3) and mesh.faces.shape == (face_capacity, 3), case
        assert mesh.offsets.is_cuda and mesh.face_offsets.is_cuda and '_host_both' not in mesh.__dict__
        assert torch.equal(mesh.offsets, full.offsets) and torch.equal(mesh.face_offsets, full.face_offsets), case   # TRUE
        assert torch.equal(mesh.faces[:face_held], full.faces[:face_held]), case   # the true rows, whatever the capacity
        assert torch.equal(mesh.points[:held].view(torch.int32), full.points[:held].view(torch.int32)), case
        assert torch.equal(mesh.index[:held], full.index[:held]), case
        assert mesh.size() == held and mesh.face_count() == face_held, case
        assert sum(mesh.entry(b).faces.shape[0] for b in range(shape[0])) == face_held, case
        if capacity < n:
            with pytest.raises(RuntimeError, match='points do not fit capacity %d' % capacity):
                pds.triangle_mesh(d, matrix, max_difference=0.75, capacity=capacity, face_capacity=face_capacity)
        elif face_capacity < f:
            with pytest.raises(RuntimeError, match='faces do not fit face_capacity %d' % face_capacity):
                pds.triangle_mesh(d, matrix, max_difference=0.75, capacity=capacity, face_capacity=face_capacity)
        else:
            trimmed = pds.triangle_mesh(d, matrix, max_difference=0.75, capacity=capacity, face_capacity=face_capacity)
            assert torch.equal(trimmed.faces, full.faces) and trimmed.points.shape == (n, 3), case
        # the entry point itself, into buffers one row larger that are filled with a sentinel
        points = torch.full((capacity + 1, 3), -7.0, device=dev)
        index = torch.full((capacity + 1,), -5, dtype=torch.int32, device=dev)
        faces = torch.full((face_capacity + 1, 3), -9, dtype=torch.int32, device=dev)
        both = torch.empty((2, shape[0] + 1), dtype=torch.int32, device=dev)
        _lib.check(lib.pds_triangle_mesh_fwd(
            _lib.ptr(d), None, None, 0.0, c_matrix, -INF, INF, 0.75, 0, None, 0, _lib.ptr(points), None, _lib.ptr(index),
            _lib.ptr(both[0]), capacity, _lib.ptr(faces), _lib.ptr(both[1]), face_capacity, *shape, _lib.ptr(workspace),
            workspace.numel(), _lib.stream_handle(dev)), 'pds_triangle_mesh_fwd')
        torch.cuda.synchronize()
        assert torch.equal(faces[:face_held], full.faces[:face_held]) and bool((faces[face_held:] == -9).all()), case
        assert torch.equal(points[:held].view(torch.int32), full.points[:held].view(torch.int32)), case
        assert bool((points[held:] == -7.0).all()) and bool((index[held:] == -5).all()), case
        assert both[0, -1].item() == n and both[1, -1].item() == f, case


def test_untrimmed_call_does_not_wait_and_a_side_stream_agrees(dev):
    shape = (1, 270, 480)
    d = torch.from_numpy(scene(shape, 5)).to(dev)
    image = torch.from_numpy(image_of(shape, 'uint8', 5)).to(dev)
    matrix = matrix_of(*shape[1:])
    first = pds.triangle_mesh(d, matrix, image=image, with_index=True, trim=False)
    assert first.offsets.is_cuda and first.face_offsets.is_cuda and first.faces.shape == (2 * 269 * 479, 3)
    assert '_host_both' not in first.__dict__   # nothing was read back
    assert first.offsets.data_ptr() + 8 == first.face_offsets.data_ptr()   # one [2, B + 1] tensor: one read serves both
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        other = pds.triangle_mesh(d, matrix, image=image, with_index=True, trim=False)
        totals = torch.stack([other.offsets[-1], other.face_offsets[-1]])   # consumed on that stream
    stream.synchronize()
    torch.cuda.current_stream(dev).wait_stream(stream)
    n, f = (int(v) for v in totals.tolist())
    assert 0 < n < 270 * 480 and 0 < f < 2 * 269 * 479
    assert torch.equal(other.offsets, first.offsets) and torch.equal(other.face_offsets, first.face_offsets)
    assert torch.equal(other.faces[:f], first.faces[:f])
    assert torch.equal(other.points[:n].view(torch.int32), first.points[:n].view(torch.int32))
    trimmed = pds.triangle_mesh(d, matrix, image=image, with_index=True)
    assert trimmed.faces.shape == (f, 3) and torch.equal(trimmed.faces, first.faces[:f])
    assert trimmed.points.shape == (n, 3) and '_host_both' in trimmed.__dict__
    assert first.entry(0).faces.shape == (f, 3)   # (the read happens here)


def test_three_calls_give_the_same_bits(dev):
    shape = (2, 135, 240)
    d = torch.from_numpy(scene(shape, 8)).to(dev)
    image = torch.from_numpy(image_of(shape, 'float32', 8)).to(dev)
    runs = [pds.triangle_mesh(d, matrix_of(*shape[1:]), image=image, with_index=True) for _ in range(3)]
    for again in runs[1:]:
        same_vertices(again, runs[0], 'repeat')
        assert torch.equal(again.faces, runs[0].faces) and torch.equal(again.face_offsets, runs[0].face_offsets)
    assert runs[0].face_count() > 10000


def test_the_face_kernels_ran(dev):
    lib = _lib.load()
    shape = (2, 65, 129)
    d = torch.from_numpy(scene(shape, 1)).to(dev)
    tiles = (2 * 65 * 129 + T - 1) // T
    for name, expected in (('triangle_mesh', [tiles, 1, tiles]), ('triangle_mesh_face_count', [tiles]),
                           ('triangle_mesh_face_scan', [1]), ('triangle_mesh_face_scatter', [tiles]),
                           ('point_cloud', [tiles, 1, tiles])):
        _lib.check(lib.pds_probe_begin(name.encode(), 16), 'pds_probe_begin')
        try:
            pds.triangle_mesh(d, matrix_of(65, 129), trim=False)
            torch.cuda.synchronize()
        finally:
            workgroups, ms = (ctypes.c_int * 16)(), (ctypes.c_float * 16)()
            count = lib.pds_probe_end(ms, workgroups, 16)
        assert count == len(expected), (name, count, lib.pds_last_error())
        assert list(workgroups[:count]) == expected and all(t >= 0 for t in ms[:count]), name


# ------------------------------------------------------------------------------------------------ integration
def test_the_rig_in_both_frames(dev):
    shape = (2, 64, 157)
    d = torch.from_numpy(scene(shape, 5)).to(dev)
    image = torch.from_numpy(image_of(shape, 'float32', 2)).to(dev)
    valid = torch.from_numpy(np.random.RandomState(5).rand(*shape) > 0.2).to(dev)
    for rig in (simple_rig(157, 64), rotated_rig(157, 64)):
        meshes = {}
        for frame in ('rectified', 'camera'):
            mesh = meshes[frame] = rig.triangle_mesh(d, image, valid, frame=frame, with_index=True, max_difference=2.0)
            same_vertices(mesh, rig.point_cloud(d, image, valid, frame=frame, with_index=True), frame)
            kept = ~np.isnan(rig.reproject(d, valid=valid, frame=frame).cpu().numpy()[..., 0])
            expected = oracle_mesh(d.cpu().numpy(), kept, 2.0)
            assert np.array_equal(mesh.faces.cpu().numpy(), expected[0]) and len(expected[0]) > 1000, frame
            assert np.array_equal(mesh.face_offsets.cpu().numpy(), expected[1]), frame
        assert torch.equal(meshes['rectified'].faces, meshes['camera'].faces)
    # the listed order faces the camera, on the GPU's own points
    mesh = meshes['camera']
    p = mesh.points.double()[mesh.faces.long()]
    facing = (torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]) * p[:, 0]).sum(dim=1)
    assert bool((facing < 0).all())


def test_normals_gathered_through_the_mesh_and_the_invariants_on_a_gpu_mesh(dev):
    shape = (2, 48, 77)
    d_host = scene(shape, 4)
    d = torch.from_numpy(d_host).to(dev)
    matrix = matrix_of(*shape[1:])
    mesh = pds.triangle_mesh(d, matrix, with_index=True, max_difference=1.5)
    normals = mesh.cloud().gather(pds.surface_normals(d, matrix).normals)
    assert normals.shape == (mesh.size(), 3) and mesh.size() == mesh.points.shape[0] > 1000
    kept = kept_of(dev, d, matrix)
    check_invariants(mesh.faces.cpu().numpy(), mesh.face_offsets.cpu().numpy(), d_host, kept, 1.5)
    for b in range(shape[0]):
        entry = mesh.entry(b)
        assert entry.faces.shape[0] > 0 and int(entry.faces.min()) >= 0 and int(entry.faces.max()) < entry.points.shape[0]
