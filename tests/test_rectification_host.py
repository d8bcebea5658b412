"""CPU: the host-side rectification math (stereo_rectify, StereoRig) against known answers and its own geometry, the
validation of a rig, and the C ABI of the rectification kernels (pds_rectify_maps_fwd, pds_remap_fwd, pds_reproject_fwd):
declared, exported, bound, and argument-checked without a GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib
from practicaldeepstereo_nips2018_amd import rectification

NEW_SYMBOLS = ['pds_rectify_maps_fwd', 'pds_remap_fwd', 'pds_reproject_fwd']

SIZE = (960, 540)   # (width, height)


def identity_rig():
    K = np.array([[500.0, 0.0, 479.5], [0.0, 500.0, 269.5], [0.0, 0.0, 1.0]])
    return K, np.zeros(5), K.copy(), np.zeros(5), np.eye(3), np.array([-0.12, 0.0, 0.0]), SIZE


def general_rig():
    """About 2 degrees about an oblique axis, a slightly off-axis baseline, unequal cameras, k1 < 0 with p1, p2, k3."""
    axis = np.array([0.3, -0.8, 0.5])
    R = rectification.rodrigues(axis / np.linalg.norm(axis) * math.radians(2.0))
    K1 = np.array([[702.0, 0.4, 478.0], [0.0, 698.0, 272.5], [0.0, 0.0, 1.0]])
    K2 = np.array([[695.0, 0.0, 484.5], [0.0, 691.0, 266.0], [0.0, 0.0, 1.0]])
    D1 = np.array([-0.12, 0.05, 1.2e-3, -8e-4, -0.01])
    D2 = np.array([-0.09, 0.03, -6e-4, 9e-4, 0.004])
    return K1, D1, K2, D2, R, np.array([-0.12, 0.004, -0.002]), SIZE


def project(P, X):
    h = X @ P[:, :3].T + P[:, 3]
    return h[:, :2] / h[:, 2:3]


def test_identity_rig_known_answer():
    R1, R2, P1, P2, Q = pds.stereo_rectify(*identity_rig())
    np.testing.assert_allclose(R1, np.eye(3), rtol=0, atol=1e-12)
    np.testing.assert_allclose(R2, np.eye(3), rtol=0, atol=1e-12)
    np.testing.assert_allclose(P1, [[500, 0, 479.5, 0], [0, 500, 269.5, 0], [0, 0, 1, 0]], rtol=0, atol=1e-9)
    np.testing.assert_allclose(P2[:, :3], P1[:, :3], rtol=0, atol=1e-9)
    assert P2[0, 3] == pytest.approx(-60.0, abs=1e-9) and P2[1, 3] == 0 and P2[2, 3] == 0
    assert Q[2, 3] == pytest.approx(500.0, abs=1e-9)
    assert Q[3, 2] == pytest.approx(1 / 0.12, rel=1e-12)
    assert Q[0, 3] == pytest.approx(-479.5, abs=1e-9) and Q[1, 3] == pytest.approx(-269.5, abs=1e-9)
    assert Q[3, 3] == 0


def test_general_rig_geometry():
    K1, D1, K2, D2, R, T, size = general_rig()
    R1, R2, P1, P2, Q = pds.stereo_rectify(K1, D1, K2, D2, R, T, size)
    for Rk in (R1, R2):
        np.testing.assert_allclose(Rk @ Rk.T, np.eye(3), rtol=0, atol=1e-12)
        assert np.linalg.det(Rk) == pytest.approx(1.0, abs=1e-12)
    f = P1[0, 0]
    assert P1[1, 1] == f and P2[0, 0] == f and P2[1, 1] == f and P1[1, 2] == P2[1, 2] and P1[0, 2] == P2[0, 2]
    # the k1 < 0 rule: f = min over cameras of fy (1 + k1 (W^2 + H^2) / (4 fy^2))
    w, h = size
    expected = min(K[1, 1] * (1 + D[0] * (w * w + h * h) / (4 * K[1, 1] ** 2)) for K, D in ((K1, D1), (K2, D2)))
    assert f == pytest.approx(expected, rel=1e-14)
    assert f < min(K1[1, 1], K2[1, 1])

    rng = np.random.default_rng(3)
    X = np.stack([rng.uniform(-3, 3, 200), rng.uniform(-2, 2, 200), rng.uniform(1.5, 40, 200)], axis=1)
    X2 = X @ R.T + T
    assert np.all(X2[:, 2] > 0)
    left = project(P1, X @ R1.T)
    right = project(P1, X2 @ R2.T)   # through the right camera: R2 X2 is the rectified right frame
    np.testing.assert_allclose(right, project(P2, X @ R1.T), rtol=0, atol=1e-9)   # P2 projects the rectified left frame
    np.testing.assert_allclose(left[:, 1], right[:, 1], rtol=0, atol=1e-9)   # rows align
    z_rect = (X @ R1.T)[:, 2]
    np.testing.assert_allclose(left[:, 0] - right[:, 0], -P2[0, 3] / z_rect, rtol=0, atol=1e-9)
    d = left[:, 0] - right[:, 0]
    hom = np.concatenate([left, d[:, None], np.ones((len(d), 1))], axis=1) @ Q.T
    np.testing.assert_allclose(hom[:, :3] / hom[:, 3:4], X @ R1.T, rtol=1e-9, atol=0)
    assert Q[3, 2] > 0 and P2[0, 3] < 0


def test_undistortion_inverts_the_distortion():
    K1, D1 = general_rig()[:2]
    n = rectification.undistort_points([[0.0, 0.0], [959.0, 539.0], [300.0, 100.0]], K1, D1)
    x, y = n[:, 0], n[:, 1]
    k1, k2, p1, p2, k3 = D1
    r2 = x * x + y * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    np.testing.assert_allclose(K1[0, 0] * xd + K1[0, 1] * yd + K1[0, 2], [0.0, 959.0, 300.0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(K1[1, 1] * yd + K1[1, 2], [0.0, 539.0, 100.0], rtol=0, atol=1e-9)


def test_rodrigues_round_trip():
    rng = np.random.default_rng(0)
    for angle in (0.0, 1e-9, 0.03, 1.0, 3.0, math.pi):
        axis = rng.normal(size=3)
        r = axis / np.linalg.norm(axis) * angle
        back = rectification.rodrigues_inverse(rectification.rodrigues(r))
        np.testing.assert_allclose(rectification.rodrigues(back), rectification.rodrigues(r), rtol=0, atol=1e-9)


def test_from_rectification_round_trips():
    K1, D1, K2, D2, R, T, size = general_rig()
    rig = pds.StereoRig(K1, D1, K2, D2, R, T, size)
    R1, R2, P1, P2, Q = pds.stereo_rectify(K1, D1, K2, D2, R, T, size)
    for name, a in (('R1', R1), ('R2', R2), ('P1', P1), ('P2', P2), ('Q', Q)):
        np.testing.assert_array_equal(getattr(rig, name), a, err_msg=name)
    again = pds.StereoRig.from_rectification(K1, D1, R1, P1, K2, D2, R2, P2, Q, size)
    for name in ('K1', 'D1', 'K2', 'D2', 'R1', 'R2', 'P1', 'P2', 'Q'):
        np.testing.assert_array_equal(getattr(again, name), getattr(rig, name), err_msg=name)
    assert again.image_size == rig.image_size == size
    # 4 coefficients are k1, k2, p1, p2 with k3 = 0
    four = pds.StereoRig.from_rectification(K1, D1[:4], R1, P1, K2, D2[:4], R2, P2, Q, size)
    np.testing.assert_array_equal(four.D1, np.concatenate([D1[:4], [0.0]]))
    # the map arguments: (P[:3, :3] R)^-1, (fx, fy, cx, cy, skew), D
    inverse, camera, distortion = rig.view_parameters(0)
    np.testing.assert_allclose(inverse @ (P1[:, :3] @ R1), np.eye(3), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(camera, [K1[0, 0], K1[1, 1], K1[0, 2], K1[1, 2], K1[0, 1]])
    np.testing.assert_array_equal(distortion, D1)
    # frame='camera' is diag(R1^T, 1) Q
    M = rig.reprojection_matrix('camera')
    np.testing.assert_allclose(M[:3], R1.T @ Q[:3], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(M[3], Q[3])
    with pytest.raises(ValueError, match='frame'):
        rig.reprojection_matrix('world')


def test_rig_validation():
    K1, D1, K2, D2, R, T, size = general_rig()
    with pytest.raises(ValueError, match='swap'):
        pds.stereo_rectify(K1, D1, K2, D2, R, -T, size)                         # right camera on the left
    with pytest.raises(ValueError, match='horizontal'):
        pds.stereo_rectify(K1, D1, K2, D2, R, np.array([-0.002, -0.12, 0.0]), size)   # vertical rig
    with pytest.raises(ValueError, match='rotation'):
        pds.stereo_rectify(K1, D1, K2, D2, R * 1.01, T, size)
    with pytest.raises(ValueError, match='rotation'):
        pds.stereo_rectify(K1, D1, K2, D2, np.diag([1.0, 1.0, -1.0]), T, size)
    with pytest.raises(ValueError, match='3x3'):
        pds.stereo_rectify(np.zeros((3, 4)), D1, K2, D2, R, T, size)
    with pytest.raises(ValueError, match='K2'):
        pds.stereo_rectify(K1, D1, np.eye(3) * 0, D2, R, T, size)
    for bad in (np.zeros(3), np.zeros(8), np.zeros(14), np.zeros(0)):
        with pytest.raises(ValueError, match='coefficients'):
            pds.stereo_rectify(K1, bad, K2, D2, R, T, size)
        with pytest.raises(ValueError, match='coefficients'):
            pds.StereoRig(K1, D1, K2, bad, R, T, size)
    with pytest.raises(ValueError, match='T must'):
        pds.stereo_rectify(K1, D1, K2, D2, R, [-0.12, 0.0], size)
    with pytest.raises(ValueError, match='image_size'):
        pds.stereo_rectify(K1, D1, K2, D2, R, T, (960,))

    R1, R2, P1, P2, Q = pds.stereo_rectify(K1, D1, K2, D2, R, T, size)
    ok = dict(K1=K1, D1=D1, R1=R1, P1=P1, K2=K2, D2=D2, R2=R2, P2=P2, Q=Q, image_size=size)

    def rig(**changes):
        return pds.StereoRig.from_rectification(**dict(ok, **changes))

    rig()
    with pytest.raises(ValueError, match='rotation'):
        rig(R1=R1 * 1.001)
    with pytest.raises(ValueError, match='3x3'):
        rig(R2=np.eye(4))
    with pytest.raises(ValueError, match='P2 must be 3x4'):
        rig(P2=P2[:, :3])
    with pytest.raises(ValueError, match='Q must be 4x4'):
        rig(Q=Q[:3])
    bad = P2.copy()
    bad[0, 0] *= 1.01
    with pytest.raises(ValueError, match='focal length'):
        rig(P2=bad)
    bad = P2.copy()
    bad[1, 2] += 1.0
    with pytest.raises(ValueError, match='cy'):
        rig(P2=bad)
    bad = P2.copy()
    bad[0, 3] = -bad[0, 3]
    with pytest.raises(ValueError, match='swap'):
        rig(P2=bad)
    bad = P2.copy()
    bad[1, 3] = bad[0, 3]
    with pytest.raises(ValueError, match='horizontal'):
        rig(P2=bad)
    with pytest.raises(ValueError, match='coefficients'):
        rig(D1=np.zeros(8))


def test_rectification_symbols_declared_exported_and_bound(hip_library):
    header = open(_lib.HEADER_PATH).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + '(' in header, name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert hip_library.pds_abi_version() == 7
    for name in ('StereoRig', 'stereo_rectify', 'remap', 'reproject'):
        assert name in pds.__all__ and hasattr(pds, name), name


def test_rectification_validation_needs_no_gpu(hip_library):
    lib = hip_library
    a, b, c, o, q = [ctypes.c_void_p(16 * k) for k in range(1, 6)]   # never dereferenced
    d9, d5 = (ctypes.c_double * 9)(*[0.0] * 9), (ctypes.c_double * 5)(*[0.0] * 5)

    def maps(*args, shape=(4, 8)):
        return lib.pds_rectify_maps_fwd(*args, *shape, None)

    for args in [(None, d5, d5, a, b), (d9, None, d5, a, b), (d9, d5, None, a, b), (d9, d5, d5, None, b),
                 (d9, d5, d5, a, None)]:
        assert maps(*args) != 0 and b'rectify_maps: null pointer' in lib.pds_last_error()
    for shape in [(0, 8), (4, 0), (-1, 8), (1 << 24, 1), (1 << 16, 1 << 16)]:
        assert maps(d9, d5, d5, a, b, shape=shape) != 0 and b'bad shape' in lib.pds_last_error(), shape
    nan9 = (ctypes.c_double * 9)(*([0.0] * 8 + [math.nan]))
    assert maps(nan9, d5, d5, a, b) != 0 and b'non-finite' in lib.pds_last_error()
    assert maps(d9, d5, d5, a, a) != 0 and b'alias' in lib.pds_last_error()

    def remap(image=a, layout=0, mx=b, my=c, out=o, shape=(2, 16, 24, 8, 12), border=0.0):
        return lib.pds_remap_fwd(image, layout, mx, my, out, *shape, border, 0, None)

    for kw in [dict(image=None), dict(mx=None), dict(my=None), dict(out=None)]:
        assert remap(**kw) != 0 and b'remap: null pointer' in lib.pds_last_error(), kw
    for layout in (-1, 2, 3):
        assert remap(layout=layout) != 0 and b'bad layout' in lib.pds_last_error()
    for shape in [(0, 16, 24, 8, 12), (2, 0, 24, 8, 12), (2, 16, 24, 8, -1), (2, 1 << 24, 1, 8, 12),
                  (1 << 10, 1 << 10, 1 << 10, 8, 12), (1 << 10, 8, 12, 1 << 10, 1 << 10)]:
        assert remap(shape=shape) != 0 and b'bad shape' in lib.pds_last_error(), shape
    for border in (math.nan, math.inf):
        assert remap(border=border) != 0 and b'border_value' in lib.pds_last_error()
    assert remap(out=b) != 0 and b'alias' in lib.pds_last_error()

    m16 = (ctypes.c_float * 16)(*[0.0] * 16)

    def reproject(disp=a, valid=None, conf=None, minc=0.0, matrix=m16, points=b, depth=c, shape=(1, 4, 8)):
        return lib.pds_reproject_fwd(disp, valid, conf, minc, matrix, points, depth, *shape, None)

    assert reproject(disp=None) != 0 and b'reproject: null pointer' in lib.pds_last_error()
    assert reproject(matrix=None) != 0 and b'reproject: null pointer' in lib.pds_last_error()
    assert reproject(points=None, depth=None) != 0 and b'both null' in lib.pds_last_error()
    for shape in [(0, 4, 8), (1, -4, 8), (1, 4, 0), (1 << 12, 1 << 12, 1 << 8)]:
        assert reproject(shape=shape) != 0 and b'bad shape' in lib.pds_last_error(), shape
    assert reproject(minc=math.nan) != 0 and b'min_confidence' in lib.pds_last_error()
    assert reproject(points=a) != 0 and b'alias' in lib.pds_last_error()
    assert reproject(points=b, depth=b) != 0 and b'alias' in lib.pds_last_error()
    inf16 = (ctypes.c_float * 16)(*([math.inf] + [0.0] * 15))
    assert reproject(matrix=inf16) != 0 and b'non-finite' in lib.pds_last_error()


def test_rectification_refuses_cpu_tensors():
    rig = pds.StereoRig(*identity_rig())
    images = torch.zeros(1, 540, 960, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rig.rectify(images, images)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rig.maps('cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rig.reproject(torch.ones(1, 540, 960))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pds.reproject(torch.ones(1, 4, 4), np.eye(4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pds.remap(torch.zeros(1, 3, 4, 4), torch.zeros(4, 4), torch.zeros(4, 4))
    net = pds.PdsNetwork.default(63).train()
    with pytest.raises(RuntimeError, match='inference only'):
        rig.reconstruct(net, images, images)
    net.eval()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rig.reconstruct(net, images, images)
