"""CPU: the rolling volume (TsdfVolume.shift / follow_delta / follow; pds_tsdf_shift_fwd, pds_tsdf_extract_leaving_fwd).

The numpy oracle of the shift, held to hand-written answers on a 3 x 2 x 2 volume (tests/test_gpu_tsdf_shift.py compares
the kernel with it bit for bit), the oracle of the leaving edges, follow_delta against hand values, the exactness of
``origin`` under many shifts, and every refusal that needs no GPU: from Python and through the C entries."""
import ctypes
import inspect
import re

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib, tsdf as tsdf_module, tsdf_color as tsdf_color_module
from tests.test_tsdf_host import IDENTITY, HostVolume

NAN = float('nan')
INF = float('inf')


# ------------------------------------------------------------------------------------------------ the oracles
def staying(n, d):
    """The half-open range of the indices i of an axis of n voxels with 0 <= i + d < n (empty: (0, 0))."""
    lo, hi = max(0, -d), min(n, n - d)
    return (lo, hi) if lo < hi else (0, 0)


def oracle_shift(tsdf, weight, color, delta):
    """out voxel (i, j, k) = in voxel (i + dx, j + dy, k + dz) where that lies inside, (1.0, 0.0, colour 0.0) elsewhere;
    tsdf, weight float32 [nz, ny, nx], color float32 [nz, ny, nx, 3] or None -> the three outputs.  The words are moved as
    int32, so every bit survives."""
    nz, ny, nx = tsdf.shape
    dx, dy, dz = delta
    (x0, x1), (y0, y1), (z0, z1) = staying(nx, dx), staying(ny, dy), staying(nz, dz)
    if x0 == x1 or y0 == y1 or z0 == z1:
        x0 = x1 = y0 = y1 = z0 = z1 = 0
    out = []
    for state, empty in ((tsdf, 1.0), (weight, 0.0), (color, 0.0)):
        if state is None:
            out.append(None)
            continue
        assert state.dtype == np.float32
        moved = np.full(state.shape, empty, dtype=np.float32)
        moved.view(np.int32)[z0:z1, y0:y1, x0:x1] = state.view(np.int32)[z0 + dz:z1 + dz, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        out.append(moved)
    return tuple(out)


def oracle_leaves(index, dims, delta):
    """index = 3 v + a of extracted rows -> bool per row: the edge from v to v + e_a does not survive the shift (v or its
    neighbour does not land inside the shifted volume: 0 <= (i, j, k) - delta < dims)."""
    nx, ny, nz = dims
    index = np.asarray(index, dtype=np.int64)
    v, a = index // 3, index % 3
    at = np.stack([v % nx, (v // nx) % ny, v // (nx * ny)], axis=1)
    nb = at + np.eye(3, dtype=np.int64)[a]
    n, d = np.array(dims), np.array(delta)
    lands = (lambda p: ((p - d >= 0) & (p - d < n)).all(axis=1))
    return ~(lands(at) & lands(nb))


def flat_offset(dims, delta):
    return (delta[2] * dims[1] + delta[1]) * dims[0] + delta[0]


def test_oracle_shift_3x2x2_by_hand():
    # nx = 3, ny = 2, nz = 2: voxel (i, j, k) holds 100 k + 10 j + i (+ 0.5 in the weight; + 0.25 m in the colour)
    t = np.array([[[0, 1, 2], [10, 11, 12]], [[100, 101, 102], [110, 111, 112]]], dtype=np.float32)
    w = t + 0.5
    c = t[..., None] + np.array([0.0, 0.25, 0.5], dtype=np.float32)
    E = 1.0   # the empty tsdf
    got = oracle_shift(t, w, c, (1, 0, 0))
    assert got[0].tolist() == [[[1, 2, E], [11, 12, E]], [[101, 102, E], [111, 112, E]]]
    assert got[1].tolist() == [[[1.5, 2.5, 0], [11.5, 12.5, 0]], [[101.5, 102.5, 0], [111.5, 112.5, 0]]]
    assert got[2][0, 0].tolist() == [[1, 1.25, 1.5], [2, 2.25, 2.5], [0, 0, 0]]
    assert got[2][1, 1].tolist() == [[111, 111.25, 111.5], [112, 112.25, 112.5], [0, 0, 0]]
    assert oracle_shift(t, w, None, (-2, 0, 0))[0].tolist() == [[[E, E, 0], [E, E, 10]], [[E, E, 100], [E, E, 110]]]
    assert oracle_shift(t, w, None, (0, 1, 0))[0].tolist() == [[[10, 11, 12], [E, E, E]], [[110, 111, 112], [E, E, E]]]
    assert oracle_shift(t, w, None, (0, 0, -1))[1].tolist() == [[[0, 0, 0], [0, 0, 0]], [[0.5, 1.5, 2.5], [10.5, 11.5, 12.5]]]
    assert oracle_shift(t, w, None, (1, -1, 1))[0].tolist() == [[[E, E, E], [101, 102, E]], [[E, E, E], [E, E, E]]]
    # nothing moves; everything goes: |d_a| = n_a and beyond, on one axis alone
    same = oracle_shift(t, w, c, (0, 0, 0))
    assert all(np.array_equal(a, b) for a, b in zip(same, (t, w, c)))
    for delta in ((3, 0, 0), (-3, 0, 0), (0, 2, 0), (0, 0, -2), (8, 0, 0), (1, 1, 7), (1 << 24, 0, 0)):
        gone = oracle_shift(t, w, c, delta)
        assert (gone[0] == 1.0).all() and (gone[1] == 0.0).all() and (gone[2] == 0.0).all(), delta
    # the bits: NaN payloads, -0.0 and inf travel
    odd = np.array([0x7fc00123, 0xffc00001, 0x80000000, 0x7f800000, 0xff800000, 0x00000001], dtype=np.uint32)
    t.reshape(-1)[:6] = odd.view(np.float32)
    moved = oracle_shift(t, w, None, (0, -1, 0))[0]
    assert moved.view(np.uint32)[0, 1].tolist() == odd[:3].tolist()
    assert moved.view(np.uint32)[0, 0].tolist() == [0x3f800000] * 3
    # the inputs are left alone
    assert t.view(np.uint32).reshape(-1)[:6].tolist() == odd.tolist() and w[0, 0, 0] == 0.5


def test_oracle_leaves_3x2x2_by_hand():
    dims = (3, 2, 2)
    # the three edges of voxel 0 = (0, 0, 0), and the +x and +z edges of voxel 4 = (1, 1, 0) (its +y neighbour does not
    # exist: such a row is never extracted)
    index = np.array([0, 1, 2, 12, 14])
    # one voxel to the right: old column 0 is lost, so every edge of voxel 0 leaves; voxel 4 and its neighbours
    # (2, 1, 0), (1, 1, 1) stay
    assert oracle_leaves(index, dims, (1, 0, 0)).tolist() == [True, True, True, False, False]
    # one to the left: old column 2 is lost, and with it the +x edge of voxel 4
    assert oracle_leaves(index, dims, (-1, 0, 0)).tolist() == [False, False, False, True, False]
    # one up in z: old layer 0 is lost: everything here
    assert oracle_leaves(index, dims, (0, 0, 1)).all()
    # one down in z: old layer 1 is lost: the +z edges
    assert oracle_leaves(index, dims, (0, 0, -1)).tolist() == [False, False, True, False, True]
    assert not oracle_leaves(index, dims, (0, 0, 0)).any() and oracle_leaves(index, dims, (0, 2, 0)).all()
    assert flat_offset(dims, (1, 0, 0)) == 1 and flat_offset(dims, (0, 1, 0)) == 3 and flat_offset(dims, (1, -1, 1)) == 4


# ------------------------------------------------------------------------------------------------ follow_delta, origin
def pose_at(centre, rotation=None):
    """[R | t] of a camera whose centre is `centre`: t = -R c."""
    R = np.eye(3) if rotation is None else pds.rectification.rodrigues(np.asarray(rotation, dtype=np.float64))
    return np.hstack([R, (-R @ np.asarray(centre, dtype=np.float64))[:, None]])


def test_follow_delta_by_hand():
    # every number a dyadic fraction: voxels of 1/8 m, 32 x 16 x 8 of them from (-2, -1, 0.5): the box is 4 x 2 x 1 m and
    # its middle lies at (0, 0, 1)
    volume = HostVolume((-2.0, -1.0, 0.5), 0.125, (32, 16, 8), 0.25)
    middle = np.array([0.0, 0.0, 1.0])
    voxel = 0.125
    assert volume.follow_delta(pose_at(middle)) == (0, 0, 0)
    assert all(isinstance(v, int) for v in volume.follow_delta(pose_at(middle)))
    # step - 1 voxels off: nothing; step voxels off: one step; and so in the negative direction (towards zero)
    for axis in range(3):
        e = np.eye(3)[axis]
        for sign in (1.0, -1.0):
            assert volume.follow_delta(pose_at(middle + sign * 7 * voxel * e)) == (0, 0, 0), (axis, sign)
            assert volume.follow_delta(pose_at(middle + sign * 7.9375 * voxel * e)) == (0, 0, 0), (axis, sign)
            assert volume.follow_delta(pose_at(middle + sign * 8 * voxel * e)) == tuple((sign * 8 * e).astype(int)), axis
            assert volume.follow_delta(pose_at(middle + sign * 15 * voxel * e)) == tuple((sign * 8 * e).astype(int)), axis
            assert volume.follow_delta(pose_at(middle + sign * 16 * voxel * e)) == tuple((sign * 16 * e).astype(int)), axis
    assert volume.follow_delta(pose_at(middle + voxel * np.array([9.0, -17.0, 3.0]))) == (8, -16, 0)
    # other steps
    assert volume.follow_delta(pose_at(middle + voxel * np.array([9.0, -17.0, 3.0])), step=1) == (9, -17, 3)
    assert volume.follow_delta(pose_at(middle + voxel * np.array([9.0, -17.0, 3.0])), step=4) == (8, -16, 0)
    assert volume.follow_delta(pose_at(middle + voxel * np.array([9.5, -17.5, 3.5])), step=1) == (9, -17, 3)
    # a rotated pose: the centre is -R^T t whatever R is (a quarter turn about y keeps the numbers dyadic)
    quarter = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    centre = middle + voxel * np.array([8.0, 0.0, -8.0])
    turned = np.hstack([quarter, (-quarter @ centre)[:, None]])
    assert volume.follow_delta(turned) == (8, 0, -8)
    assert volume.follow_delta(pose_at(centre, (0.3, -0.2, 0.1)), step=4) == (8, 0, -8)
    # anchor z = 0: the camera belongs on the near face of the box (z = 0.5), looking in
    near = dict(anchor=(0.5, 0.5, 0.0))
    assert volume.follow_delta(pose_at((0.0, 0.0, 0.5)), **near) == (0, 0, 0)
    assert volume.follow_delta(pose_at(middle), **near) == (0, 0, 0)          # 4 voxels behind the face: below a step
    assert volume.follow_delta(pose_at((0.0, 0.0, 1.5)), **near) == (0, 0, 8)
    assert volume.follow_delta(pose_at((0.0, 0.0, -0.5)), **near) == (0, 0, -8)
    assert volume.follow_delta(pose_at((0.0, 0.0, 1.0)), step=4, **near) == (0, 0, 4)
    # after a shift the target is measured from the new origin: the same camera now sits at the anchor
    volume.offset = (8, -16, 0)
    assert volume.origin.tolist() == [-1.0, -3.0, 0.5]
    assert volume.follow_delta(pose_at(middle + voxel * np.array([9.0, -17.0, 3.0]))) == (0, 0, 0)


def test_origin_is_exact_after_many_shifts():
    origin0 = (0.1, -0.7, 0.3)
    volume = HostVolume(origin0, 0.02, (8, 6, 4), 0.06)
    assert volume.offset == (0, 0, 0) and volume.origin0.tolist() == list(origin0)
    assert volume.origin.tolist() == list(origin0) and volume.origin.dtype == np.float64
    # (a shift of the state needs the GPU; what it does to the bookkeeping is this line of TsdfVolume._shift)
    for k in range(1000):
        delta = (3, -2, 1) if k % 2 == 0 else (-3, 2, -1)
        volume.offset = tuple(o + d for o, d in zip(volume.offset, delta))
        if k % 2 == 0:
            assert volume.origin.tolist() == [0.1 + 0.02 * 3, -0.7 + 0.02 * -2, 0.3 + 0.02 * 1]
    assert volume.offset == (0, 0, 0) and volume.origin.tolist() == list(origin0)
    # a long way in one direction: origin0 + voxel_size * offset, rounded once
    volume.offset = (1000 * 8, 0, -(1 << 24))
    assert volume.origin.tolist() == [0.1 + 0.02 * 8000, -0.7, 0.3 + 0.02 * -(1 << 24)]
    # an axis that never moved keeps its bits, the sign of a zero among them; reset() leaves the offset alone
    signed = HostVolume((-0.0, 0.0, 1.0), 0.5, (2, 2, 2), 1.0)
    assert np.signbit(signed.origin).tolist() == [True, False, False]
    signed.offset = (0, 4, 0)
    assert np.signbit(signed.origin).tolist() == [True, False, False] and signed.origin.tolist() == [-0.0, 2.0, 1.0]
    assert 'self.offset' not in inspect.getsource(pds.TsdfVolume.reset)
    assert 'self.offset' not in inspect.getsource(pds.ColorTsdfVolume.reset)
    # the folded transforms read the moved origin: b = R (origin + voxel_size / 2) + t
    assert signed.transforms(IDENTITY, 1)[0, 9:].tolist() == [0.25, 2.25, 1.25]
    # setting origin anchors the volume anew
    signed.origin = (1.0, 2.0, 3.0)
    assert signed.offset == (0, 0, 0) and signed.origin0.tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError, match='origin must hold 3 finite values'):
        signed.origin = (1.0, NAN, 3.0)


# ------------------------------------------------------------------------------------------------ Python refusals
def test_shift_and_follow_python_errors():
    volume = HostVolume((0.0, 0.0, 0.0), 0.1, (4, 3, 2), 0.3)
    for bad in ((1.5, 0, 0), (1, 0, None), 'abc', 7, None, (1.0, 2.0, 3.0)):
        with pytest.raises(TypeError, match='delta must be three integers'):
            volume.shift(bad)
    for bad in ((1, 0), (1, 0, 0, 0), ()):
        with pytest.raises(ValueError, match='delta must be three integers'):
            volume.shift(bad)
    for bad in (((1 << 24) + 1, 0, 0), (0, -(1 << 24) - 1, 0), (0, 0, 1 << 30)):
        with pytest.raises(ValueError, match=r'delta must be at most 2\^24 voxels'):
            volume.shift(bad)
    with pytest.raises(ValueError, match='min_weight is NaN'):
        volume.shift((1, 0, 0), leaving=True, min_weight=NAN)
    with pytest.raises(ValueError, match='capacity must be >= 0'):
        volume.shift((1, 0, 0), leaving=True, capacity=-1)
    with pytest.raises(TypeError, match='capacity must be an integer or None'):
        volume.shift((0, 0, 0), leaving=True, capacity=1.5)
    # follow_delta: the pose, the anchor, the step
    for bad in (np.eye(3), np.eye(4), np.zeros((1, 3, 4)), np.full((3, 4), NAN), np.hstack([np.eye(3), [[INF], [0], [0]]])):
        with pytest.raises(ValueError, match=r'pose must be a finite 3x4 \[R \| t\]'):
            volume.follow_delta(bad)
    with pytest.raises(TypeError, match='pose must be an array of numbers'):
        volume.follow_delta('here')
    for bad in ((0.5, NAN, 0.5), (0.5, 0.5, INF), (0.5, 0.5), (0.5,) * 4):
        with pytest.raises(ValueError, match='anchor must hold 3 finite values'):
            volume.follow_delta(IDENTITY, anchor=bad)
    with pytest.raises(TypeError, match='anchor must be three numbers'):
        volume.follow_delta(IDENTITY, anchor='middle')
    for bad in (0, -8):
        with pytest.raises(ValueError, match='step must be at least 1'):
            volume.follow_delta(IDENTITY, step=bad)
    for bad in (8.0, None, '8'):
        with pytest.raises(TypeError, match='step must be an integer'):
            volume.follow_delta(IDENTITY, step=bad)
    with pytest.raises(ValueError, match='step must be at least 1'):
        volume.follow(IDENTITY, step=0, leaving=True)
    # a camera 2^25 voxels away asks for more than a shift takes
    with pytest.raises(ValueError, match=r'delta must be at most 2\^24 voxels'):
        volume.follow_delta(pose_at((0.1 * (1 << 25), 0.0, 0.0)))
    # all of that comes before the state is touched; what is left is that there is no CPU fallback, and a refused
    # shift leaves the bookkeeping alone
    for kw in ({}, dict(leaving=True), dict(leaving=True, with_normals=False, capacity=5, trim=False)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            volume.shift((1, 0, 0), **kw)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        volume.follow(pose_at((2.0, 0.0, 0.0)), step=4)
    assert volume.offset == (0, 0, 0)
    # nothing to move: nothing is launched, and the host is not even asked where the state lives
    assert volume.shift((0, 0, 0)) is None and volume.follow(pose_at((0.2, 0.15, 0.1))) is None
    # the signatures
    parameters = inspect.signature(pds.TsdfVolume.shift).parameters
    assert [(n, p.default) for n, p in parameters.items()][1:] == [
        ('delta', inspect.Parameter.empty), ('leaving', False), ('min_weight', 1.0), ('with_normals', True),
        ('capacity', None), ('trim', True)]
    parameters = inspect.signature(pds.ColorTsdfVolume.shift).parameters
    assert [(n, p.default) for n, p in parameters.items()][-1] == ('with_colors', True) and len(parameters) == 8
    parameters = inspect.signature(pds.TsdfVolume.follow_delta).parameters
    assert [(n, p.default) for n, p in parameters.items()][1:] == [('pose', inspect.Parameter.empty),
                                                                   ('anchor', (0.5, 0.5, 0.5)), ('step', 8)]
    assert list(inspect.signature(pds.TsdfVolume.follow).parameters)[1:] == ['pose', 'anchor', 'step', 'shift_kw']
    for phrase in ('hashed or sparse volumes', 'in-place shifting', 'ring-buffer', 'a leaving *mesh*', 'Kintinuous',
                   'origin0 + voxel_size * offset', 'step * trunc(target_a)'):
        assert phrase in tsdf_module.__doc__, phrase
    assert 'sparse volumes' in tsdf_color_module.__doc__


# ------------------------------------------------------------------------------------------------ the C ABI
def test_rolling_symbols_declared_exported_and_bound(hip_library):
    header = open(_lib.ROLLING_HEADER_PATH).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = ('pds_tsdf_shift_fwd', 'pds_tsdf_extract_leaving_fwd')
    for name in names:
        assert name + '(' in header and hasattr(raw, name) and name in _lib.ROLLING_SIGNATURES, name
        assert getattr(hip_library, name).argtypes == _lib.ROLLING_SIGNATURES[name][1], name
        assert getattr(hip_library, name).restype == _lib.ROLLING_SIGNATURES[name][0], name
    declared = sorted(set(re.findall(r'\b(pds_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S))))
    assert declared == sorted(names) == sorted(_lib.ROLLING_SIGNATURES) and '#include "pds_hip.h"' in header
    assert header.count('Additive: ABI version unchanged') == 2
    assert not set(_lib.ROLLING_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.TRACKING_SIGNATURES) |
                                               set(_lib.PHOTOMETRIC_SIGNATURES))
    assert hip_library.pds_abi_version() == 7 and _lib.ABI_VERSION == 7
    assert '#define PDS_ABI_VERSION 7' in open(_lib.HEADER_PATH).read()
    # the leaving extraction takes what the extraction takes, and the delta behind the dims
    full, leaving = _lib.SIGNATURES['pds_tsdf_extract_fwd'][1], _lib.ROLLING_SIGNATURES['pds_tsdf_extract_leaving_fwd'][1]
    assert leaving[:13] == full[:13] and leaving[13:16] == [ctypes.c_int] * 3 and leaving[16:] == full[13:]
    for phrase in ('tsdf 1.0f, weight 0.0f, colour 0.0f', 'NaN', '-0.0', 'tsdf_extract_leaving_count', 'ONE launch',
                   'no byte outside', 'pds_tsdf_extract_workspace_bytes', 'not in the reference'):
        assert phrase in header, phrase


def test_rolling_validation_needs_no_gpu(hip_library):
    lib = hip_library
    big = 1 << 24
    t, w, c, to, wo, co, pts, nrm, idx, off, ws = [ctypes.c_void_p(big * n) for n in range(1, 12)]   # never dereferenced
    error = lib.pds_last_error
    at = (lambda p, nbytes: ctypes.c_void_p(p.value + nbytes))

    def shift(tsdf=t, weight=w, color=c, tsdf_out=to, weight_out=wo, color_out=co, delta=(1, 0, 0), dims=(4, 3, 2)):
        return lib.pds_tsdf_shift_fwd(tsdf, weight, color, tsdf_out, weight_out, color_out, *delta, *dims, None)

    for name in ('tsdf', 'weight', 'tsdf_out', 'weight_out'):
        assert shift(**{name: None}) != 0 and error() == b'tsdf_shift: null pointer', name
    for name in ('color', 'color_out'):
        assert shift(**{name: None}) != 0 and error() == b'tsdf_shift: color and color_out go together', name
    for dims in [(0, 3, 2), (4, 0, 2), (4, 3, 0), (-4, 3, 2)]:
        assert shift(dims=dims) != 0 and b'tsdf: bad volume' in error(), dims
    assert shift(dims=((1 << 24) + 1, 1, 1)) != 0 and b'tsdf: a dimension above 2^24' in error()
    for dims in [(895, 895, 895), (1 << 16, 1 << 16, 1)]:
        assert shift(dims=dims) != 0 and b'3 * nx * ny * nz does not fit' in error(), dims
    for name, p in (('tsdf', t), ('weight', w), ('color', c), ('tsdf_out', to), ('weight_out', wo), ('color_out', co)):
        for nbytes in (1, 2, 3):
            assert shift(**{name: at(p, nbytes)}) != 0 and b'tsdf_shift: a 32-bit buffer is not 4-byte aligned' in error()
    # out of place (4 x 3 x 2 voxels: 96 bytes, the colour 288): no output may touch an input or another output
    for kw in (dict(tsdf_out=t), dict(tsdf_out=at(t, 92)), dict(weight_out=at(t, -92)), dict(weight_out=w),
               dict(tsdf_out=at(c, 284)), dict(color_out=at(w, 92)), dict(color_out=at(c, -284)), dict(color_out=c)):
        assert shift(**kw) != 0 and error() == b'tsdf_shift: an output aliases an input', kw
    for kw in (dict(weight_out=to), dict(weight_out=at(to, 92)), dict(color_out=at(to, -284)), dict(color_out=at(wo, 92))):
        assert shift(**kw) != 0 and error() == b'tsdf_shift: an output aliases another output', kw
    # without a colour its addresses are nobody's
    assert shift(color=None, color_out=None, tsdf_out=at(t, 92)) != 0 and b'aliases an input' in error()

    origin = (ctypes.c_float * 3)(0.0, 0.0, 0.0)

    def leaving(tsdf=t, weight=w, origin=origin, voxel_size=0.1, min_weight=1.0, points=pts, normals=nrm, index=idx,
                offsets=off, capacity=10, dims=(4, 3, 2), delta=(1, 0, 0), workspace=ws, workspace_bytes=512):
        return lib.pds_tsdf_extract_leaving_fwd(tsdf, weight, origin, voxel_size, min_weight, points, normals, index,
                                                offsets, capacity, *dims, *delta, workspace, workspace_bytes, None)

    for name in ('tsdf', 'weight', 'origin', 'points', 'offsets', 'workspace'):
        assert leaving(**{name: None}) != 0 and error() == b'tsdf_extract_leaving: null pointer', name
    assert leaving(dims=(4, 0, 2)) != 0 and b'tsdf: bad volume' in error()
    assert leaving(dims=(895, 895, 895)) != 0 and b'does not fit' in error()
    assert leaving(capacity=-1) != 0 and b'tsdf_extract_leaving: capacity must be >= 0 (got -1)' in error()
    assert leaving(workspace_bytes=511) != 0 and b'tsdf_extract_leaving: workspace too small (511 < 512)' in error()
    for bad in (0.0, -1.0, NAN, INF):
        assert leaving(voxel_size=bad) != 0 and b'voxel_size must be positive and finite' in error(), bad
    assert leaving(min_weight=NAN) != 0 and b'tsdf_extract_leaving: min_weight is NaN' in error()
    assert leaving(origin=(ctypes.c_float * 3)(0.0, NAN, 0.0)) != 0 and b'tsdf_extract_leaving: non-finite origin' in error()
    assert leaving(points=at(pts, 2)) != 0 and b'not 4-byte aligned' in error()
    assert leaving(normals=at(nrm, 1)) != 0 and b'not 4-byte aligned' in error()
    assert leaving(points=t) != 0 and b'tsdf_extract_leaving: an output aliases an input' in error()
    assert leaving(index=at(w, 92)) != 0 and b'an output aliases an input' in error()
    assert leaving(normals=at(pts, 116)) != 0 and b'tsdf_extract_leaving: an output aliases another output' in error()
    assert leaving(offsets=at(idx, 36)) != 0 and b'an output aliases another output' in error()
    assert leaving(workspace=at(off, 4)) != 0 and b'an output aliases another output' in error()
    assert leaving(capacity=0, normals=pts, workspace_bytes=511) != 0 and b'workspace too small' in error()
