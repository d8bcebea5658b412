"""GPU (-m gpu): surface normals from disparity (surface_normals, StereoRig.surface_normals, PointCloud.gather, save_ply;
pds_surface_normals_fwd).

The arbiter is the numpy fp64 oracle of tests/test_surface_normals_host.py (itself held to hand-written answers and to a
second route there).  `valid` must match it exactly outside the pixels that module excludes (a grazing surface, H[3] next
to 0: at most 1 % of a scene, asserted there), and the angle between the normals stays within ANGLE_BOUND = 4 * EPS32,
EPS32 being the error of the float32 restatement measured there against the same oracle -- never against the kernel.
The kernel works on tiles of 64 x 16 pixels, so the shapes sit around them."""
import ctypes

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib
from tests.test_surface_normals_host import (ANGLE_BOUND, KINDS, SHAPES, angles, fit_normals, normal_scene, q_of, read_ply,
                                             settings)

pytestmark = pytest.mark.gpu

NAN, INF = float('nan'), float('inf')
TENSORS = ('disparity', 'valid', 'confidence')


@pytest.fixture(scope='module')
def dev(hip_library):
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def put(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run(dev, case, **kw):
    """surface_normals on a dictionary of numpy arguments (tests/test_surface_normals_host.py: normal_scene)."""
    arguments = {k: put(dev, case[k]) if k in TENSORS else case[k] for k in case}
    arguments.update(kw)
    result = pds.surface_normals(**arguments)
    assert isinstance(result, pds.SurfaceNormals)
    assert result.normals.dtype == torch.float32 and result.valid.dtype == torch.bool
    assert result.normals.is_contiguous() and result.valid.is_contiguous()
    assert tuple(result.normals.shape) == tuple(case['disparity'].shape) + (3,)
    return result.normals.cpu().numpy(), result.valid.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def check_against_oracle(normals, valid, oracle, fill_bits, where):
    """-> the largest angle.  Masks exact outside the excluded pixels, angles within the bound, unit vectors, the fill
    value bit for bit, every normal facing the viewpoint."""
    compared = ~oracle.fragile
    assert np.array_equal(valid[compared], oracle.valid[compared]), where
    assert (bits(normals[~valid]) == fill_bits).all(), where
    assert np.abs(np.linalg.norm(normals[valid].astype(np.float64), axis=-1) - 1.0).max(initial=0.0) <= 1e-6, where
    both = compared & oracle.valid
    worst = float(angles(normals[both], oracle.normals[both]).max(initial=0.0))
    print('%s: %d valid, %d excluded, largest angle %.3e rad (bound %.3e)' %
          (where, int(valid.sum()), int(oracle.fragile.sum()), worst, ANGLE_BOUND))
    assert worst <= ANGLE_BOUND, where
    return worst


# ------------------------------------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_against_the_fp64_oracle(dev, shape, kind):
    case = normal_scene(kind, shape)
    view = np.zeros(3) if case.get('viewpoint') is None else np.asarray(case['viewpoint'], dtype=np.float64)
    for k in (3, 5, 7):
        for max_difference, min_valid in settings(k):
            kw = dict(kernel_size=k, max_difference=max_difference, min_valid=min_valid)
            oracle = fit_normals(**kw, **case)
            fill = -7.5 if k == 5 else NAN
            normals, valid = run(dev, case, fill_value=fill, **kw)
            where = '%s %s k=%d md=%s mv=%s' % (kind, shape, k, max_difference, min_valid)
            check_against_oracle(normals, valid, oracle, bits(np.float32(fill)), where)
            # N . (X - viewpoint) <= 0 with the oracle's own point, wherever that is no coin toss
            sure = valid & oracle.valid & ~oracle.fragile
            facing = (normals[sure].astype(np.float64) * (oracle.points[sure] - view)).sum(-1)
            assert (facing <= 0).all(), where


# ------------------------------------------------------------------------------------------------ 2. known answers
@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 6, 9), (2, 17, 65), (1, 16, 132)], ids=lambda s: '%dx%dx%d' % s)
def test_a_constant_map_faces_the_camera_bit_for_bit(dev, shape):
    d = np.full(shape, 7.0, dtype=np.float32)
    Q = q_of(shape[1], shape[2])
    expected = bits(np.array([0.0, 0.0, -1.0], dtype=np.float32))
    for k in (3, 5, 7):
        normals, valid = run(dev, dict(disparity=d, matrix=Q), kernel_size=k, min_valid=3)
        oracle = fit_normals(d, Q, k, min_valid=3)
        assert np.array_equal(valid, oracle.valid) and valid.all() == (shape[1] > 1 and shape[2] > 1), (shape, k)
        assert (bits(normals[valid]) == expected).all(), (shape, k)          # +0, +0, -1: no -0 either
        assert np.isnan(normals[~valid]).all()
        behind, valid_behind = run(dev, dict(disparity=d, matrix=Q), kernel_size=k, min_valid=3, viewpoint=(0.0, 0.0, 100.0))
        assert np.array_equal(valid_behind, valid)
        assert (bits(behind[valid]) == bits(np.array([0.0, 0.0, 1.0], dtype=np.float32))).all(), (shape, k)


def test_the_hand_cases_of_the_host_file(dev):
    # three pixels of a 2 x 2 image
    d = np.array([[[2.0, 3.0], [4.0, NAN]]], dtype=np.float32)
    Q = q_of(2, 2)
    normals, valid = run(dev, dict(disparity=d, matrix=Q), kernel_size=3, max_difference=INF, min_valid=3)
    oracle = fit_normals(d, Q, 3, INF, min_valid=3)
    assert valid.tolist() == [[[True, True], [True, False]]] and angles(normals[valid], oracle.normals[valid]).max() <= ANGLE_BOUND
    assert not run(dev, dict(disparity=d, matrix=Q), kernel_size=3, max_difference=INF)[1].any()
    assert run(dev, dict(disparity=d, matrix=Q), kernel_size=3, max_difference=1.0, min_valid=3)[1].tolist() == [
        [[False, True], [False, False]]]
    # a row, a column and a diagonal: det == 0
    row = np.full((1, 1, 9), 5.0, dtype=np.float32)
    diagonal = np.where(np.eye(7, dtype=bool), 5.0, NAN).astype(np.float32)[None]
    for k in (3, 5, 7):
        assert not run(dev, dict(disparity=row, matrix=q_of(1, 9)), kernel_size=k, max_difference=INF, min_valid=3)[1].any()
        assert not run(dev, dict(disparity=row.reshape(1, 9, 1), matrix=q_of(9, 1)), kernel_size=k, max_difference=INF,
                       min_valid=3)[1].any()
    assert not run(dev, dict(disparity=diagonal, matrix=q_of(7, 7)), kernel_size=7, max_difference=INF, min_valid=3)[1].any()
    diagonal[0, 0, 1] = 5.0
    assert run(dev, dict(disparity=diagonal, matrix=q_of(7, 7)), kernel_size=7, max_difference=INF, min_valid=3)[1][0, 3, 3]
    # a centre with W <= 0 (W = 8 d - 48 vanishes at d = 6 exactly)
    Q = q_of(5, 5, baseline=0.125)
    Q[3, 3] = -48.0
    for centre in (5.0, 6.0):
        d = np.full((1, 5, 5), 12.0, dtype=np.float32)
        d[0, 2, 2] = centre
        valid = run(dev, dict(disparity=d, matrix=Q), kernel_size=3, max_difference=INF, min_valid=3)[1]
        assert not valid[0, 2, 2] and valid.sum() == 24, centre


def test_a_step_edge_keeps_each_side_on_its_plane(dev):
    """Two slanted planes that meet in a step of about 3 px of disparity between columns 69 and 70 (inside the second
    tile of a row, next to the border at 64): with the edge test every pixel, the edge columns
    included, has its own plane's normal; without it the columns next to the edge tilt."""
    height, width, edge = 20, 140, 70
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    left, right = 20.0 + xx / 64.0 - yy / 32.0, 26.0 - xx / 32.0 + yy / 64.0   # exact in float32
    d = np.where(xx < edge, left, right).astype(np.float32)[None]
    Q = q_of(height, width)
    for k in (3, 5, 7):
        normals, valid = run(dev, dict(disparity=d, matrix=Q), kernel_size=k, max_difference=1.5, min_valid=3)
        assert valid.all()
        for plane, columns in ((left, slice(0, edge)), (right, slice(edge, width))):
            whole = fit_normals(plane[None].astype(np.float32), Q, k, INF, min_valid=3)   # the plane without the edge
            assert angles(normals[0, :, columns], whole.normals[0, :, columns]).max() <= ANGLE_BOUND, k
        loose, _ = run(dev, dict(disparity=d, matrix=Q), kernel_size=k, max_difference=INF, min_valid=3)
        tilt = angles(loose[0], normals[0])
        r = k // 2
        assert (tilt[:, edge - r:edge + r] > 0.05).all() and tilt[:, :edge - r].max() == 0 and tilt[:, edge + r:].max() == 0


# ------------------------------------------------------------------------------------------------ 3. reproject
def test_consistent_with_reproject(dev):
    case = normal_scene('wall', (2, 35, 133))
    tensors = {k: put(dev, case[k]) for k in TENSORS}
    points = pds.reproject(tensors['disparity'], case['matrix'], valid=tensors['valid'], confidence=tensors['confidence'],
                           min_confidence=case['min_confidence'])
    for k in (3, 7):
        result = pds.surface_normals(tensors['disparity'], case['matrix'], kernel_size=k, min_valid=3, valid=tensors['valid'],
                                     confidence=tensors['confidence'], min_confidence=case['min_confidence'])
        assert bool((~torch.isnan(points).any(-1))[result.valid].all())       # valid implies a point
        assert bool(result.valid.any())
    # on an exact plane the normal is perpendicular to every chord between reprojected points
    height, width = 33, 70
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    d = put(dev, (30.0 + xx / 32.0 - yy / 64.0).astype(np.float32)[None])
    matrix = normal_scene('checker', (1, height, width))['matrix']
    P = pds.reproject(d, matrix).cpu().numpy().astype(np.float64)[0]
    for k in (3, 5, 7):
        result = pds.surface_normals(d, matrix, kernel_size=k, max_difference=INF, min_valid=3)
        assert bool(result.valid.all())
        N = result.normals.cpu().numpy().astype(np.float64)[0]
        for dy, dx in ((0, 1), (1, 0), (3, 5), (-7, 20)):
            p = P[max(0, -dy):height - max(0, dy), 0:width - dx]
            q = P[max(0, dy):height + min(0, dy), dx:width]
            n = N[max(0, -dy):height - max(0, dy), 0:width - dx]
            chord = q - p
            sine = np.abs((n * chord).sum(-1)) / np.linalg.norm(chord, axis=-1)
            # the bound on the angle, plus what float32 points (relative 2e-7 each) can put into a chord's direction
            slack = 4e-7 * np.linalg.norm(p, axis=-1) / np.linalg.norm(chord, axis=-1)
            assert (sine <= ANGLE_BOUND + slack).all(), (k, dy, dx, float((sine - slack).max()))


# ------------------------------------------------------------------------------------------------ 4. batch, repeatability
def test_batch_entries_are_independent_and_runs_repeat(dev):
    case = normal_scene('wall', (3, 33, 130))
    kw = dict(kernel_size=5, max_difference=0.5)
    normals, valid = run(dev, case, **kw)
    for b in (0, 2):
        single = {k: (v[b:b + 1] if k in TENSORS else v) for k, v in case.items()}
        n1, v1 = run(dev, single, **kw)
        assert np.array_equal(bits(n1[0]), bits(normals[b])) and np.array_equal(v1[0], valid[b]), b
    again, valid_again = run(dev, case, **kw)
    assert np.array_equal(bits(again), bits(normals)) and np.array_equal(valid_again, valid)
    stream = torch.cuda.Stream(device=dev)
    tensors = {k: put(dev, case[k]) if k in TENSORS else case[k] for k in case}
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream):
        side = pds.surface_normals(**tensors, **kw)
    stream.synchronize()
    assert np.array_equal(bits(side.normals.cpu().numpy()), bits(normals))
    assert np.array_equal(side.valid.cpu().numpy(), valid)


# ------------------------------------------------------------------------------------------------ 5. inputs and buffers
def test_non_contiguous_inputs(dev):
    case = normal_scene('wall', (2, 35, 133))
    expected, expected_valid = run(dev, case, kernel_size=5)
    wide = {k: put(dev, np.concatenate([case[k], case[k]], axis=2)) for k in TENSORS}
    views = {k: t[:, :, :133] for k, t in wide.items()}
    assert not views['disparity'].is_contiguous()
    result = pds.surface_normals(views['disparity'], case['matrix'], kernel_size=5, valid=views['valid'],
                                 confidence=views['confidence'], min_confidence=case['min_confidence'],
                                 viewpoint=case['viewpoint'])
    assert np.array_equal(bits(result.normals.cpu().numpy()), bits(expected))
    assert np.array_equal(result.valid.cpu().numpy(), expected_valid)


@pytest.mark.parametrize('shape', [(1, 17, 65), (2, 16, 64), (1, 5, 130)], ids=lambda s: '%dx%dx%d' % s)
def test_unaligned_pointers_agree_bit_for_bit(dev, hip_library, shape):
    """Pointers that are only 4-byte (the floats) or 1-byte (the flags) aligned: the records leave by the same staged
    rows with another shift, the flags one by one."""
    lib = hip_library
    case = normal_scene('wall', shape)
    batch, height, width = shape
    count = batch * height * width
    expected, expected_valid = run(dev, case, kernel_size=5, fill_value=-1.0)
    matrix = (ctypes.c_float * 16)(*np.asarray(case['matrix']).astype(np.float32).reshape(-1).tolist())
    view = (ctypes.c_float * 3)(*np.asarray(case['viewpoint']).astype(np.float32).tolist())
    for float_offset, flag_offset in ((1, 1), (2, 3), (3, 2)):
        d = torch.zeros(count + 4, dtype=torch.float32, device=dev)
        d[float_offset:float_offset + count] = put(dev, case['disparity']).reshape(-1)
        c = torch.zeros(count + 4, dtype=torch.float32, device=dev)
        c[float_offset:float_offset + count] = put(dev, case['confidence']).reshape(-1)
        v = torch.zeros(count + 4, dtype=torch.bool, device=dev)
        v[flag_offset:flag_offset + count] = put(dev, case['valid']).reshape(-1)
        out = torch.full((3 * count + 8,), 123.0, dtype=torch.float32, device=dev)
        good = torch.full((count + 8,), 7, dtype=torch.uint8, device=dev)
        _lib.check(lib.pds_surface_normals_fwd(
            ctypes.c_void_p(d.data_ptr() + 4 * float_offset), ctypes.c_void_p(v.data_ptr() + flag_offset),
            ctypes.c_void_p(c.data_ptr() + 4 * float_offset), case['min_confidence'], matrix, view, 5, 1.0, 13, -1.0,
            ctypes.c_void_p(out.data_ptr() + 4 * float_offset), ctypes.c_void_p(good.data_ptr() + flag_offset), batch,
            height, width, _lib.stream_handle(dev)), 'pds_surface_normals_fwd')
        got, flags = out.cpu().numpy(), good.cpu().numpy()
        where = (shape, float_offset, flag_offset)
        assert np.array_equal(bits(got[float_offset:float_offset + 3 * count]), bits(expected.reshape(-1))), where
        assert np.array_equal(flags[flag_offset:flag_offset + count], expected_valid.reshape(-1).astype(np.uint8)), where
        # and nothing outside the buffers was touched
        assert (got[:float_offset] == 123.0).all() and (got[float_offset + 3 * count:] == 123.0).all(), where
        assert (flags[:flag_offset] == 7).all() and (flags[flag_offset + count:] == 7).all(), where
    # valid_out may be absent
    out = torch.empty(3 * count, dtype=torch.float32, device=dev)
    d = put(dev, case['disparity'])
    _lib.check(lib.pds_surface_normals_fwd(_lib.ptr(d), None, None, 0.0, matrix, None, 3, INF, 3, NAN, _lib.ptr(out), None,
                                           batch, height, width, _lib.stream_handle(dev)), 'pds_surface_normals_fwd')
    expected = run(dev, dict(disparity=case['disparity'], matrix=case['matrix']), kernel_size=3, max_difference=INF,
                   min_valid=3)[0]
    assert np.array_equal(bits(out.cpu().numpy()), bits(expected.reshape(-1)))


def test_overlapping_buffers_are_refused(dev, hip_library):
    lib = hip_library
    buffer = torch.zeros(4 * 6 * 10, dtype=torch.float32, device=dev)
    flags = torch.zeros(64, dtype=torch.uint8, device=dev)
    matrix = (ctypes.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1).tolist())

    def call(disparity, normals, valid=None, valid_out=None):
        return lib.pds_surface_normals_fwd(disparity, valid, None, 0.0, matrix, None, 3, 1.0, 5, NAN, normals, valid_out,
                                           1, 6, 10, _lib.stream_handle(dev))

    base = buffer.data_ptr()
    assert call(ctypes.c_void_p(base), ctypes.c_void_p(base)) != 0
    assert b'surface_normals: an output aliases an input' in lib.pds_last_error()
    assert call(ctypes.c_void_p(base + 4 * 180 - 4), ctypes.c_void_p(base)) != 0           # the last record's last float
    assert call(ctypes.c_void_p(base + 4 * 180), ctypes.c_void_p(base)) == 0                # adjacent is fine
    assert call(ctypes.c_void_p(base + 4 * 180), ctypes.c_void_p(base), valid_out=ctypes.c_void_p(base + 4 * 100)) != 0
    assert b'surface_normals: an output aliases another output' in lib.pds_last_error()
    assert call(ctypes.c_void_p(base + 4 * 180), ctypes.c_void_p(base), valid=_lib.ptr(flags), valid_out=_lib.ptr(flags)) != 0
    assert b'surface_normals: an output aliases an input' in lib.pds_last_error()
    torch.cuda.synchronize(dev)


# ------------------------------------------------------------------------------------------------ 6. rig and cloud
def rotated_rig(width, height):
    K = np.array([[0.7 * width, 0.0, 0.5 * width - 0.5], [0.0, 0.7 * width, 0.5 * height - 0.5], [0.0, 0.0, 1.0]])
    R = pds.rectification.rodrigues(np.array([0.3, -0.8, 0.5]) / np.linalg.norm([0.3, -0.8, 0.5]) * np.radians(2.0))
    return pds.StereoRig(K, np.array([-0.05, 0.01, 1e-3, -5e-4]), K, np.array([-0.04, 0.02, -4e-4, 6e-4]), R,
                         np.array([-0.12, 0.004, -0.002]), (width, height))


def test_the_rig_and_the_cloud(dev, tmp_path):
    batch, height, width = 2, 35, 133
    rig = rotated_rig(width, height)
    assert np.abs(rig.R1 - np.eye(3)).max() > 1e-3
    rng = np.random.RandomState(5)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    d = np.stack([8.0 + 0.02 * xx - 0.01 * yy + 0.05 * rng.rand(height, width),
                  np.where(xx < 60, 12.0 + 0.01 * yy, 6.0 - 0.02 * xx + 0.3 * rng.rand(height, width))]).astype(np.float32)
    d[rng.rand(batch, height, width) < 0.05] = NAN
    mask = rng.rand(batch, height, width) > 0.1
    dt, vt = put(dev, d), put(dev, mask)
    by_rig = rig.surface_normals(dt, vt, kernel_size=3, max_difference=0.5)
    by_hand = pds.surface_normals(dt, rig.reprojection_matrix('rectified'), kernel_size=3, max_difference=0.5, valid=vt)
    assert torch.equal(by_rig.valid, by_hand.valid) and bool(by_rig.valid.any())
    assert np.array_equal(bits(by_rig.normals.cpu().numpy()), bits(by_hand.normals.cpu().numpy()))
    # the raw left camera's frame: R1^T applied to the rectified normals
    in_camera = rig.surface_normals(dt, vt, frame='left', kernel_size=3, max_difference=0.5)
    same = rig.surface_normals(dt, vt, frame='camera', kernel_size=3, max_difference=0.5)
    assert torch.equal(in_camera.valid, same.valid)
    assert np.array_equal(bits(in_camera.normals.cpu().numpy()), bits(same.normals.cpu().numpy()))
    oracle = fit_normals(d, rig.reprojection_matrix('rectified'), 3, 0.5, valid=mask)
    oracle_camera = fit_normals(d, rig.reprojection_matrix('camera'), 3, 0.5, valid=mask)
    compared = ~(oracle.fragile | oracle_camera.fragile)
    assert np.array_equal(in_camera.valid.cpu().numpy()[compared], by_rig.valid.cpu().numpy()[compared])
    both = compared & in_camera.valid.cpu().numpy() & by_rig.valid.cpu().numpy()
    turned = by_rig.normals.cpu().numpy().astype(np.float64) @ rig.R1      # rows: (R1^T n)^T = n^T R1
    worst = angles(in_camera.normals.cpu().numpy()[both], turned[both]).max()
    print('frame left vs R1^T applied to the rectified normals: largest angle %.3e rad' % worst)
    assert worst <= ANGLE_BOUND

    # the cloud: one normal per point, in the cloud's order
    cloud = rig.point_cloud(dt, valid=vt, with_index=True)
    points = rig.reproject(dt, vt)
    keep = ~torch.isnan(points).any(-1)
    gathered = cloud.gather(by_rig.normals)
    assert gathered.shape == (cloud.points.shape[0], 3) and gathered.shape[0] == int(keep.sum())
    assert np.array_equal(bits(gathered.cpu().numpy()), bits(by_rig.normals[keep].cpu().numpy()))
    assert torch.equal(cloud.gather(by_rig.valid), by_rig.valid[keep])
    assert np.array_equal(bits(cloud.gather(points).cpu().numpy()), bits(cloud.points.cpu().numpy()))
    loose = rig.point_cloud(dt, valid=vt, with_index=True, trim=False)          # no synchronisation, full capacity
    count = cloud.points.shape[0]
    assert np.array_equal(bits(loose.gather(by_rig.normals)[:count].cpu().numpy()), bits(gathered.cpu().numpy()))
    # and to a file
    path = str(tmp_path / 'cloud.ply')
    pds.save_ply(path, cloud, normals=gathered)
    lines, vertices = read_ply(path)
    assert 'element vertex %d' % count in lines and vertices.dtype.itemsize == 24
    assert np.array_equal(bits(np.stack([vertices['x'], vertices['y'], vertices['z']], -1)), bits(cloud.points.cpu().numpy()))
    assert np.array_equal(bits(np.stack([vertices['nx'], vertices['ny'], vertices['nz']], -1)), bits(gathered.cpu().numpy()))
    pds.save_ply(path, cloud, normals=gathered, entry=1)
    first = cloud.host_offsets()[1]
    _, vertices = read_ply(path)
    assert len(vertices) == count - first
    assert np.array_equal(bits(np.stack([vertices['nx'], vertices['ny'], vertices['nz']], -1)),
                          bits(gathered[first:].cpu().numpy()))
