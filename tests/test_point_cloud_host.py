"""CPU: the point cloud's entry points (pds_point_cloud_workspace_bytes, pds_point_cloud_fwd) are declared, exported and
bound and validate their arguments without a GPU, the Python surface (point_cloud, StereoRig.point_cloud, PointCloud)
refuses what it cannot run, and PointCloud.save_ply writes what a PLY reader expects.

The numpy oracle of tests/test_gpu_point_cloud.py lives here and is itself held to hand-written answers, so that a wrong
oracle cannot pass a wrong kernel.  Semantics (include/pds_hip.h): a pixel is kept iff the x of its dense point
(`reproject`) is not NaN and its depth lies in [min_depth, max_depth]; the kept pixels are packed in raster order, the
entries in batch order; offsets is the cumulative sum of the entries' counts."""
import ctypes
import importlib
import inspect
import math

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib

NAN, INF = float('nan'), float('inf')
module = importlib.import_module('practicaldeepstereo_nips2018_amd.point_cloud')   # (pds.point_cloud is the function)


# ------------------------------------------------------------------------------------------------ the oracle
def oracle_cloud(dense_points, image=None, min_depth=None, max_depth=None):
    """-> (points [N, 3], colors [N, 3] or None, index [N] int32, offsets [B + 1] int32) from the dense points
    [B, H, W, 3] of `reproject` (numpy float32) and the image (uint8 [B, H, W, 3] or float32 [B, 3, H, W])."""
    dense = np.asarray(dense_points, dtype=np.float32)
    assert dense.ndim == 4 and dense.shape[-1] == 3
    batch, height, width = dense.shape[:3]
    keep = ~np.isnan(dense[..., 0])
    if min_depth is not None:
        keep &= dense[..., 2] >= np.float32(min_depth)
    if max_depth is not None:
        keep &= dense[..., 2] <= np.float32(max_depth)
    points = dense[keep]   # a boolean mask gathers in C order: entries, then rows, then columns
    colors = None
    if image is not None:
        image = np.asarray(image)
        nhwc = image if image.dtype == np.uint8 else image.transpose(0, 2, 3, 1)
        assert nhwc.shape == dense.shape and image.dtype in (np.uint8, np.float32)
        colors = nhwc[keep]
    pixel = np.broadcast_to(np.arange(height * width, dtype=np.int32).reshape(1, height, width), keep.shape)
    index = pixel[keep]
    offsets = np.concatenate([[0], np.cumsum(keep.reshape(batch, -1).sum(axis=1))]).astype(np.int32)
    return points, colors, index, offsets


def dense_of(kept, batch, height, width):
    """Dense points with NaN everywhere but at {(b, y, x): (X, Y, Z)}."""
    dense = np.full((batch, height, width, 3), NAN, dtype=np.float32)
    for (b, y, x), point in kept.items():
        dense[b, y, x] = point
    return dense


def test_oracle_2x3_by_hand():
    dense = dense_of({(0, 0, 1): (1, 2, 3), (0, 1, 0): (4, 5, 6), (0, 1, 2): (7, 8, 9)}, 1, 2, 3)
    image = np.arange(18, dtype=np.uint8).reshape(1, 2, 3, 3)
    points, colors, index, offsets = oracle_cloud(dense, image)
    assert points.tolist() == [[1, 2, 3], [4, 5, 6], [7, 8, 9]] and points.dtype == np.float32
    assert colors.tolist() == [[3, 4, 5], [9, 10, 11], [15, 16, 17]] and colors.dtype == np.uint8
    assert index.tolist() == [1, 3, 5] and index.dtype == np.int32
    assert offsets.tolist() == [0, 3] and offsets.dtype == np.int32
    # a float image is [B, 3, H, W]: channel c of pixel i is 6 c + i
    planes = np.arange(18, dtype=np.float32).reshape(1, 3, 2, 3)
    assert oracle_cloud(dense, planes)[1].tolist() == [[1, 7, 13], [3, 9, 15], [5, 11, 17]]
    assert oracle_cloud(dense)[1] is None


def test_oracle_an_empty_entry_between_two_entries_with_points():
    dense = dense_of({(0, 0, 0): (1, 1, 1), (0, 1, 1): (2, 2, 2), (2, 0, 1): (3, 3, 3)}, 3, 2, 2)
    points, _, index, offsets = oracle_cloud(dense)
    assert offsets.tolist() == [0, 2, 2, 3]
    assert points[:, 0].tolist() == [1, 2, 3] and index.tolist() == [0, 3, 1]
    assert oracle_cloud(dense_of({}, 2, 1, 3))[3].tolist() == [0, 0, 0]
    assert oracle_cloud(dense_of({}, 2, 1, 3))[0].shape == (0, 3)


def test_oracle_depth_window_is_closed_and_only_x_decides_nan():
    dense = dense_of({(0, 0, 0): (0, 0, 1.0), (0, 0, 1): (0, 0, 2.0), (0, 0, 2): (0, 0, 3.0), (0, 0, 3): (0, 0, 4.0)},
                     1, 1, 5)
    assert oracle_cloud(dense, min_depth=2.0, max_depth=3.0)[2].tolist() == [1, 2]   # both bounds are kept
    assert oracle_cloud(dense, min_depth=2.0)[2].tolist() == [1, 2, 3]
    assert oracle_cloud(dense, max_depth=2.5)[2].tolist() == [0, 1]
    assert oracle_cloud(dense, min_depth=-INF, max_depth=INF)[2].tolist() == [0, 1, 2, 3]
    assert oracle_cloud(dense, min_depth=5.0)[3].tolist() == [0, 0]
    dense[0, 0, 4] = (7.0, NAN, 1.5)   # x decides
    assert oracle_cloud(dense)[2].tolist() == [0, 1, 2, 3, 4]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_point_cloud_symbols_declared_exported_and_bound(hip_library):
    header = open(_lib.HEADER_PATH).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pds_point_cloud_workspace_bytes', 'pds_point_cloud_fwd'):
        assert name + '(' in header and hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert hip_library.pds_abi_version() == 7
    for name in ('point_cloud', 'PointCloud', 'PointCloudEntry'):
        assert name in pds.__all__, name
    assert pds.PointCloud._fields == ('points', 'colors', 'index', 'offsets')
    assert callable(pds.point_cloud) and pds.point_cloud is module.point_cloud
    # the tile the GPU tests sit around is the kernel's
    common = open(_lib.HEADER_PATH.replace('include/pds_hip.h', 'practicaldeepstereo_nips2018_amd/csrc/common.hpp')).read()
    assert 'constexpr int kPointCloudTile = 1024;' in common
    # 4 bytes per tile of 1024 pixels, rounded to 256, + 256
    assert hip_library.pds_point_cloud_workspace_bytes(1, 1, 1) == 512
    assert hip_library.pds_point_cloud_workspace_bytes(1, 540, 960) == (507 * 4 + 255) // 256 * 256 + 256
    assert hip_library.pds_point_cloud_workspace_bytes(1, 1, 65 * 1024) == 512 + 256


def test_point_cloud_validation_needs_no_gpu(hip_library):
    lib = hip_library
    big = 1 << 24
    d, v, c, im, pts, col, idx, off, ws = [ctypes.c_void_p(big * n) for n in range(1, 10)]   # never dereferenced
    identity = (ctypes.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1).tolist())
    bad_matrix = (ctypes.c_float * 16)(*([1.0] * 15 + [NAN]))
    error = lib.pds_last_error

    def call(disparity=d, valid=v, confidence=c, min_confidence=0.0, matrix=identity, min_depth=-INF, max_depth=INF,
             image=im, layout=1, points=pts, colors=col, index=idx, offsets=off, capacity=6, shape=(1, 2, 3),
             workspace=ws, workspace_bytes=512):
        return lib.pds_point_cloud_fwd(disparity, valid, confidence, min_confidence, matrix, min_depth, max_depth, image,
                                       layout, points, colors, index, offsets, capacity, *shape, workspace,
                                       workspace_bytes, None)

    for name in ('disparity', 'matrix', 'points', 'offsets', 'workspace'):
        assert call(**{name: None}) != 0 and error() == b'point_cloud: null pointer', name
    for shape in [(0, 2, 3), (1, 0, 3), (1, 2, 0), (-1, 2, 3), (1, -2, 3), (1, 2, -3)]:
        assert call(shape=shape) != 0 and b'point_cloud: bad shape' in error(), shape
        assert lib.pds_point_cloud_workspace_bytes(*shape) == 0 and b'point_cloud: bad shape' in error(), shape
    for shape in [(1, 1 << 16, 1 << 16), (4, 1 << 15, 1 << 14)]:   # 2^32 and 2^31 pixels
        assert call(shape=shape, workspace_bytes=1 << 40) != 0 and b'32-bit indices' in error(), shape
        assert lib.pds_point_cloud_workspace_bytes(*shape) == 0 and b'32-bit indices' in error(), shape
    assert lib.pds_point_cloud_workspace_bytes(1, (1 << 15) - 1, 1 << 16) > 0   # 2^31 - 2^16 pixels are accepted
    for capacity in (-1, -(1 << 40)):
        assert call(capacity=capacity) != 0 and b'capacity must be >= 0' in error(), capacity
    assert call(image=None) != 0 and b'colors without an image' in error()
    for layout in (-1, 2, 7):
        assert call(layout=layout) != 0 and b'bad image_layout' in error(), layout
    assert call(workspace_bytes=511) != 0 and b'workspace too small (511 < 512)' in error()
    assert call(workspace_bytes=0) != 0 and b'workspace too small' in error()
    assert call(shape=(1, 540, 960), capacity=10, workspace_bytes=2303) != 0 and b'(2303 < 2304)' in error()
    assert call(min_confidence=NAN) != 0 and b'min_confidence is NaN' in error()
    assert call(min_depth=NAN) != 0 and b'a depth bound is NaN' in error()
    assert call(max_depth=NAN) != 0 and b'a depth bound is NaN' in error()
    assert call(min_depth=2.0, max_depth=1.0) != 0 and b'min_depth 2 > max_depth 1' in error()
    assert call(min_depth=INF, max_depth=-INF) != 0 and b'min_depth' in error()
    assert call(points=ctypes.c_void_p(pts.value + 2)) != 0 and b'not 4-byte aligned' in error()
    assert call(index=ctypes.c_void_p(idx.value + 1)) != 0 and b'not 4-byte aligned' in error()
    # the scatter pass reads the inputs again: nothing written may overlap anything read or written
    assert call(points=d) != 0 and b'an output aliases an input' in error()
    assert call(points=ctypes.c_void_p(d.value + 20)) != 0 and b'an output aliases an input' in error()
    assert call(colors=im) != 0 and b'an output aliases an input' in error()
    assert call(offsets=ctypes.c_void_p(v.value + 4)) != 0 and b'an output aliases an input' in error()
    assert call(workspace=c) != 0 and b'an output aliases an input' in error()
    assert call(index=ctypes.c_void_p(pts.value + 68)) != 0 and b'an output aliases another output' in error()
    assert call(offsets=ctypes.c_void_p(col.value + 16)) != 0 and b'an output aliases another output' in error()
    assert call(workspace=ctypes.c_void_p(off.value + 4)) != 0 and b'an output aliases another output' in error()
    assert call(matrix=bad_matrix) != 0 and b'non-finite matrix' in error()


# ------------------------------------------------------------------------------------------------ Python
def test_point_cloud_python_errors():
    ok, Q = torch.zeros(1, 4, 5), np.eye(4)
    with pytest.raises(TypeError, match='disparity must be a torch.Tensor'):
        pds.point_cloud(np.zeros((1, 4, 5), dtype=np.float32), Q)
    for bad in (ok.double(), ok.half(), ok.to(torch.int32)):
        with pytest.raises(TypeError, match='disparity must be float32'):
            pds.point_cloud(bad, Q)
    for bad in (torch.zeros(4, 5), torch.zeros(1, 1, 4, 5)):
        with pytest.raises(ValueError, match='disparity must have 3 dimensions'):
            pds.point_cloud(bad, Q)
    for bad in (np.eye(3), np.zeros((4, 3)), np.full((4, 4), NAN), np.diag([1.0, 1.0, 1.0, INF])):
        with pytest.raises(ValueError, match='matrix must be a finite 4x4'):   # reproject's message
            pds.point_cloud(ok, bad)
    with pytest.raises(ValueError, match='min_confidence is NaN'):           # reproject's message
        pds.point_cloud(ok, Q, min_confidence=NAN)
    with pytest.raises(ValueError, match='min_depth is NaN'):
        pds.point_cloud(ok, Q, min_depth=NAN)
    with pytest.raises(ValueError, match='max_depth is NaN'):
        pds.point_cloud(ok, Q, max_depth=NAN)
    with pytest.raises(ValueError, match=r'min_depth 2\.0 > max_depth 1\.0'):
        pds.point_cloud(ok, Q, min_depth=2.0, max_depth=1.0)
    for capacity in (2.0, '3', True, (4,)):
        with pytest.raises(TypeError, match='capacity must be an integer or None'):
            pds.point_cloud(ok, Q, capacity=capacity)
    with pytest.raises(ValueError, match='capacity must be >= 0'):
        pds.point_cloud(ok, Q, capacity=-1)
    # the image: remap's two layouts and remap's messages
    with pytest.raises(ValueError, match=r'a uint8 image must be \[B, H, W, 3\]'):
        pds.point_cloud(ok, Q, image=torch.zeros(1, 3, 4, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r'a float32 image must be \[B, 3, H, W\]'):
        pds.point_cloud(ok, Q, image=torch.zeros(1, 4, 5, 3))
    with pytest.raises(TypeError, match='image must be uint8'):
        pds.point_cloud(ok, Q, image=torch.zeros(1, 3, 4, 5, dtype=torch.float64))
    with pytest.raises(TypeError, match='image must be a torch.Tensor'):
        pds.point_cloud(ok, Q, image=np.zeros((1, 4, 5, 3), dtype=np.uint8))
    for image in (torch.zeros(1, 3, 4, 6), torch.zeros(2, 3, 4, 5), torch.zeros(1, 5, 5, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match='does not match disparity'):
            pds.point_cloud(ok, Q, image=image)
    for valid in (torch.ones(1, 4, 5), torch.ones(1, 4, 5, dtype=torch.uint8), torch.ones(1, 4, 6, dtype=torch.bool)):
        with pytest.raises(ValueError, match='valid must be torch.bool'):    # reproject's message
            pds.point_cloud(ok, Q, valid=valid)
    with pytest.raises(TypeError, match='confidence must be float32'):
        pds.point_cloud(ok, Q, confidence=ok.double())
    with pytest.raises(ValueError, match='confidence .* differ in shape'):
        pds.point_cloud(ok, Q, confidence=torch.zeros(1, 5, 4))
    # every argument in order, and still no CPU fallback
    for kwargs in ({}, {'image': torch.zeros(1, 3, 4, 5), 'valid': torch.ones(1, 4, 5, dtype=torch.bool),
                        'confidence': ok, 'min_confidence': 0.5, 'min_depth': 0.1, 'max_depth': 0.1,
                        'with_index': True, 'capacity': np.int64(7), 'trim': False}):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            pds.point_cloud(ok, Q, **kwargs)
    parameters = inspect.signature(pds.point_cloud).parameters
    assert [(n, p.default) for n, p in parameters.items()][2:] == [
        ('image', None), ('valid', None), ('confidence', None), ('min_confidence', 0.0), ('min_depth', None),
        ('max_depth', None), ('with_index', False), ('capacity', None), ('trim', True)]
    assert 'ONLY synchronisation' in pds.point_cloud.__doc__ and 'without any synchronisation' in pds.point_cloud.__doc__


def test_the_rig_has_the_counterpart_of_reproject():
    parameters = inspect.signature(pds.StereoRig.point_cloud).parameters
    assert list(parameters) == ['self', 'disparity', 'image', 'valid', 'confidence', 'min_confidence', 'frame', 'kw']
    assert parameters['frame'].default == 'rectified' and parameters['min_confidence'].default == 0.0
    assert parameters['kw'].kind is inspect.Parameter.VAR_KEYWORD
    assert 'rig.point_cloud(r.disparity, r.left_image, r.valid)' in pds.StereoRig.point_cloud.__doc__
    K = np.array([[180.0, 0.0, 127.5], [0.0, 180.0, 63.5], [0.0, 0.0, 1.0]])
    rig = pds.StereoRig(K, np.zeros(4), K, np.zeros(4), np.eye(3), np.array([-0.12, 0.0, 0.0]), (256, 128))
    with pytest.raises(ValueError, match="frame must be 'rectified' or 'camera'"):
        rig.point_cloud(torch.zeros(1, 128, 256), frame='world')
    with pytest.raises(ValueError, match='min_depth'):
        rig.point_cloud(torch.zeros(1, 128, 256), min_depth=3.0, max_depth=1.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rig.point_cloud(torch.zeros(1, 128, 256), frame='camera', with_index=True)
    # reconstruct and its result are what they were
    assert pds.rectification.Reconstruction._fields == ('left_image', 'right_image', 'disparity', 'valid', 'points')


# ------------------------------------------------------------------------------------------------ PointCloud on the host
def hand_made(colors):
    points = torch.tensor([[0.5, -1.25, 3.0], [1e-40, 2.0, -0.0], [7.0, 8.0, 9.0], [-3.5, 1e30, 0.125]])
    index = torch.tensor([4, 0, 1, 5], dtype=torch.int32)
    return pds.PointCloud(points, colors, index, torch.tensor([0, 1, 1, 4], dtype=torch.int32))


def read_ply(path):
    """-> (structured array of the vertices, header lines), parsed from the file's own header."""
    blob = open(path, 'rb').read()
    end = blob.index(b'end_header\n') + len(b'end_header\n')
    lines = blob[:end].decode('ascii').splitlines()
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0' and lines[-1] == 'end_header'
    count = int([l for l in lines if l.startswith('element vertex ')][0].split()[-1])
    assert sum(l.startswith('element ') for l in lines) == 1
    kinds = {'float': '<f4', 'uchar': 'u1'}
    fields = [(l.split()[2], kinds[l.split()[1]]) for l in lines if l.startswith('property ')]
    vertices = np.frombuffer(blob[end:], dtype=np.dtype(fields))
    assert vertices.shape == (count,) and len(blob) == end + count * np.dtype(fields).itemsize
    return vertices, lines


def test_ply_round_trip_without_and_with_colours(tmp_path):
    plain = hand_made(None)
    path = str(tmp_path / 'plain.ply')
    plain.save_ply(path)
    vertices, _ = read_ply(path)
    assert vertices.dtype.names == ('x', 'y', 'z') and vertices.dtype.itemsize == 12
    got = np.stack([vertices['x'], vertices['y'], vertices['z']], axis=1)
    assert np.array_equal(got.view(np.int32), plain.points.numpy().view(np.int32))   # the denormal and -0.0 included

    bytes_ = torch.tensor([[0, 128, 255], [1, 2, 3], [250, 251, 252], [9, 8, 7]], dtype=torch.uint8)
    coloured = hand_made(bytes_)
    path = str(tmp_path / 'coloured.ply')
    coloured.save_ply(path)
    vertices, _ = read_ply(path)
    assert vertices.dtype.names == ('x', 'y', 'z', 'red', 'green', 'blue') and vertices.dtype.itemsize == 15
    got = np.stack([vertices['x'], vertices['y'], vertices['z']], axis=1)
    assert np.array_equal(got.view(np.int32), coloured.points.numpy().view(np.int32))
    assert np.array_equal(np.stack([vertices['red'], vertices['green'], vertices['blue']], axis=1), bytes_.numpy())

    # one entry alone; the empty entry writes a valid file of no vertices
    coloured.save_ply(path, entry=2)
    vertices, _ = read_ply(path)
    assert vertices['x'].tolist() == [np.float32(1e-40), 7.0, -3.5] and vertices['blue'].tolist() == [3, 252, 7]
    coloured.save_ply(path, entry=1)
    assert read_ply(path)[0].shape == (0,)
    with pytest.raises(IndexError):
        coloured.save_ply(path, entry=3)


def test_ply_float_colours_are_clamped_and_rounded(tmp_path):
    floats = torch.tensor([[-3.0, 0.0, 0.49], [0.5, 1.5, 2.5], [254.5, 255.0, 300.0], [NAN, 127.6, 1e9]])
    cloud = hand_made(floats)
    path = str(tmp_path / 'floats.ply')
    cloud.save_ply(path)
    vertices, _ = read_ply(path)
    rgb = np.stack([vertices['red'], vertices['green'], vertices['blue']], axis=1)
    # ties go to even, as the doc string says; NaN becomes 0
    assert rgb.tolist() == [[0, 0, 0], [0, 2, 2], [254, 255, 255], [0, 128, 255]]
    assert 'clamped to 0 .. 255' in pds.PointCloud.save_ply.__doc__ and 'ties to even' in pds.PointCloud.save_ply.__doc__


def test_entries_are_views_and_a_cut_cloud_stops_at_its_rows():
    cloud = hand_made(torch.arange(12, dtype=torch.uint8).reshape(4, 3))
    assert cloud.host_offsets() == [0, 1, 1, 4] and cloud.size() == 4
    first, empty, last = cloud.entry(0), cloud.entry(1), cloud.entry(2)
    assert isinstance(first, pds.PointCloudEntry) and first._fields == ('points', 'colors', 'index')
    assert first.points.shape == (1, 3) and empty.points.shape == (0, 3) and last.points.shape == (3, 3)
    assert last.index.tolist() == [0, 1, 5] and last.colors[0].tolist() == [3, 4, 5]
    assert last.points.data_ptr() == cloud.points[1:].data_ptr()   # a view
    for b in (-1, 3):
        with pytest.raises(IndexError):
            cloud.entry(b)
    points, colors, index, offsets = cloud   # still a tuple of four
    assert points is cloud.points and colors is cloud.colors and index is cloud.index and offsets is cloud.offsets
    # offsets[B] = 6 points were found, the buffers hold 4: the views end with the buffers
    cut = pds.PointCloud(cloud.points, None, None, torch.tensor([0, 3, 6], dtype=torch.int32))
    assert cut.size() == 4 and cut.entry(0).points.shape == (3, 3) and cut.entry(1).points.shape == (1, 3)
    assert cut.entry(1).colors is None and cut.entry(1).index is None
