"""CPU: the triangle mesh's entry points (pds_triangle_mesh_workspace_bytes, pds_triangle_mesh_fwd) are declared, exported
and bound and validate their arguments without a GPU, the Python surface (triangle_mesh, StereoRig.triangle_mesh,
TriangleMesh) refuses what it cannot run, and save_ply writes the faces a PLY reader expects.

The numpy oracle of tests/test_gpu_triangle_mesh.py lives here (oracle_mesh, vectorised) and is held to hand-written
answers and to a second implementation that walks the table of include/pds_hip.h cell by cell (oracle_mesh_by_cells), so
that a wrong oracle cannot pass a wrong kernel.  Semantics: corners a = (x, y), b = (x + 1, y), c = (x, y + 1),
e = (x + 1, y + 1); two kept pixels are joined iff |D[p] - D[q]| <= max_difference in fp32; with four kept corners the
diagonal is a-e iff |D[a] - D[e]| < |D[b] - D[c]|, else b-c; b-c gives (a, c, b) then (b, c, e), a-e gives (a, c, e) then
(a, e, b); with three kept corners the one candidate that avoids the missing corner; a face needs its three edges."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib
from tests.test_point_cloud_host import read_ply as read_cloud_ply

NAN, INF = float('nan'), float('inf')


# ------------------------------------------------------------------------------------------------ the oracle
def ranks_of(kept):
    """-> (rank [B, H, W] int64: the packed row of a kept pixel over the whole batch, -1 elsewhere; offsets [B + 1])."""
    kept = np.asarray(kept, dtype=bool)
    rank = (np.cumsum(kept.reshape(-1)) - 1).reshape(kept.shape).astype(np.int64)
    rank[~kept] = -1
    offsets = np.concatenate([[0], np.cumsum(kept.reshape(kept.shape[0], -1).sum(axis=1))]).astype(np.int32)
    return rank, offsets


def oracle_mesh(disparity, kept, max_difference, flip=False):
    """-> (faces [F, 3] int32, face_offsets [B + 1] int32) of disparity [B, H, W] float32 and the kept mask [B, H, W]."""
    D = np.asarray(disparity, dtype=np.float32)
    K = np.asarray(kept, dtype=bool)
    assert D.ndim == 3 and K.shape == D.shape
    batch, height, width = D.shape
    if height < 2 or width < 2:
        return np.zeros((0, 3), dtype=np.int32), np.zeros(batch + 1, dtype=np.int32)
    rank, _ = ranks_of(K)
    t = np.float32(max_difference)
    corner = (lambda m: (m[:, :-1, :-1], m[:, :-1, 1:], m[:, 1:, :-1], m[:, 1:, 1:]))   # a, b, c, e
    (da, db, dc, de), (ka, kb, kc, ke), (ra, rb, rc, re) = corner(D), corner(K), corner(rank)
    with np.errstate(invalid='ignore', over='ignore'):
        difference = (lambda p, q: np.abs(p - q))   # float32 - float32: one fp32 subtraction
        assert difference(da, de).dtype == np.float32
        joined = (lambda kp, kq, p, q: kp & kq & (difference(p, q) <= t))
        count = ka.astype(int) + kb + kc + ke
        diagonal_ae = np.where(count == 4, difference(da, de) < difference(db, dc), ~(kb & kc))
        ab, ac, ae = joined(ka, kb, da, db), joined(ka, kc, da, dc), joined(ka, ke, da, de)
        bc, be, ce = joined(kb, kc, db, dc), joined(kb, ke, db, de), joined(kc, ke, dc, de)
    first = np.where(diagonal_ae, ae & ac & ce, bc & ac & ab)
    second = np.where(diagonal_ae, ae & be & ab, bc & ce & be)
    pick = diagonal_ae[..., None]
    first_vertices = np.where(pick, np.stack([ra, rc, re], axis=-1), np.stack([ra, rc, rb], axis=-1))
    second_vertices = np.where(pick, np.stack([ra, re, rb], axis=-1), np.stack([rb, rc, re], axis=-1))
    candidates = np.stack([first_vertices, second_vertices], axis=-2)   # [B, H - 1, W - 1, 2, 3]
    emitted = np.stack([first, second], axis=-1)
    faces = candidates[emitted].astype(np.int32)   # C order: entry, row, column, candidate
    if flip:
        faces = faces[:, [0, 2, 1]]
    face_offsets = np.concatenate([[0], np.cumsum(emitted.reshape(batch, -1).sum(axis=1))]).astype(np.int32)
    return np.ascontiguousarray(faces), face_offsets


def oracle_mesh_by_cells(disparity, kept, max_difference, flip=False):
    """The same answer, cell by cell from the table (slow: small shapes only)."""
    D = np.asarray(disparity, dtype=np.float32)
    K = np.asarray(kept, dtype=bool)
    batch, height, width = D.shape
    rank, _ = ranks_of(K)
    t = np.float32(max_difference)
    faces, face_offsets = [], [0]
    for n in range(batch):
        for y in range(height - 1):
            for x in range(width - 1):
                pixel = {'a': (n, y, x), 'b': (n, y, x + 1), 'c': (n, y + 1, x), 'e': (n, y + 1, x + 1)}
                have = ''.join(name for name in 'abce' if K[pixel[name]])
                gap = (lambda p, q: np.abs(D[pixel[p]] - D[pixel[q]]))   # np.float32 scalars: fp32 arithmetic
                if have == 'abce':
                    candidates = ['ace', 'aeb'] if gap('a', 'e') < gap('b', 'c') else ['acb', 'bce']
                else:
                    candidates = {'abc': ['acb'], 'bce': ['bce'], 'ace': ['ace'], 'abe': ['aeb']}.get(have, [])
                for p, q, r in candidates:
                    if gap(p, q) <= t and gap(q, r) <= t and gap(p, r) <= t:
                        face = [rank[pixel[p]], rank[pixel[q]], rank[pixel[r]]]
                        faces.append([face[0], face[2], face[1]] if flip else face)
        face_offsets.append(len(faces))
    return np.array(faces, dtype=np.int32).reshape(-1, 3), np.array(face_offsets, dtype=np.int32)


def faces_of(rows, kept=None, max_difference=1.0, flip=False):
    """The faces of one image given as nested lists (NaN: not kept, unless a mask is given), as a list of lists."""
    d = np.array([rows], dtype=np.float32)
    kept = ~np.isnan(d) if kept is None else np.array([kept], dtype=bool)
    answers = [f(np.nan_to_num(d, nan=7.0), kept, max_difference, flip) for f in (oracle_mesh, oracle_mesh_by_cells)]
    assert np.array_equal(answers[0][0], answers[1][0]) and np.array_equal(answers[0][1], answers[1][1])
    assert answers[0][0].dtype == np.int32 and answers[0][1].dtype == np.int32
    assert answers[0][1].tolist() == [0, len(answers[0][0])]
    return answers[0][0].tolist()


def test_oracle_every_keep_pattern_of_one_cell():
    # a constant cell: ties, so the diagonal is b-c wherever all four are kept.  Rows are a b / c e; ranks count the kept
    expected = {(1, 1, 1, 1): [[0, 2, 1], [1, 2, 3]],       # (a, c, b), (b, c, e)
                (1, 1, 1, 0): [[0, 2, 1]],                  # e missing: (a, c, b)
                (0, 1, 1, 1): [[0, 1, 2]],                  # a missing: (b, c, e) = rows 0, 1, 2
                (1, 0, 1, 1): [[0, 1, 2]],                  # b missing: (a, c, e)
                (1, 1, 0, 1): [[0, 2, 1]]}                  # c missing: (a, e, b): a = 0, b = 1, e = 2
    for pattern in range(16):
        keep = tuple((pattern >> bit) & 1 for bit in range(4))   # a, b, c, e
        mask = [[bool(keep[0]), bool(keep[1])], [bool(keep[2]), bool(keep[3])]]
        assert faces_of([[5.0, 5.0], [5.0, 5.0]], kept=mask) == expected.get(keep, []), keep


def test_oracle_the_diagonal_is_the_smaller_difference_and_a_tie_is_bc():
    # |a - e| = 0.25 < |b - c| = 0.5: a-e, (a, c, e) then (a, e, b)
    assert faces_of([[10.0, 10.5], [10.0, 10.25]]) == [[0, 2, 3], [0, 3, 1]]
    # |a - e| = 0.5 > |b - c| = 0.25: b-c, (a, c, b) then (b, c, e)
    assert faces_of([[10.0, 10.25], [10.0, 10.5]]) == [[0, 2, 1], [1, 2, 3]]
    # |a - e| = |b - c| = 0.5: the tie is b-c
    assert faces_of([[10.0, 10.5], [10.0, 10.5]]) == [[0, 2, 1], [1, 2, 3]]
    assert faces_of([[10.0, 10.5], [10.0, 10.5]], flip=True) == [[0, 1, 2], [1, 3, 2]]


def test_oracle_a_far_corner_leaves_the_one_triangle_that_avoids_it():
    near, far = 10.0, 50.0
    # the far corner makes its diagonal the longer one; the other diagonal's triangle without it survives
    assert faces_of([[near, near], [near, far]]) == [[0, 2, 1]]    # e far: b-c, (a, c, b)
    assert faces_of([[far, near], [near, near]]) == [[1, 2, 3]]    # a far: b-c, (b, c, e)
    assert faces_of([[near, far], [near, near]]) == [[0, 2, 3]]    # b far: a-e, (a, c, e)
    assert faces_of([[near, near], [far, near]]) == [[0, 3, 1]]    # c far: a-e, (a, e, b)
    # the shorter diagonal a-e (1.5) is too long, and there is no fallback to b-c (2.0), although a-b and a-c would do
    assert faces_of([[10.0, 11.0], [9.0, 11.5]], max_difference=1.0) == []


def test_oracle_threshold_zero_and_infinity():
    steps = [[1.0, 2.0, 2.0], [1.0, 2.0, 2.0]]
    assert faces_of(steps, max_difference=0.0) == [[1, 4, 2], [2, 4, 5]]   # only the cell of equal values; <= 0 holds
    assert faces_of(steps, max_difference=INF) == [[0, 3, 1], [1, 3, 4], [1, 4, 2], [2, 4, 5]]   # (|a - e| = |b - c|: b-c)
    assert faces_of([[1.0, 3e38], [2.0, 1e-3]], max_difference=INF) == [[0, 2, 3], [0, 3, 1]]
    assert faces_of([[1.0, 1.0], [1.0, np.nextafter(np.float32(1.0), np.float32(2.0))]], max_difference=0.0) == [[0, 2, 1]]


def test_oracle_3x3_with_a_step_edge_and_degenerate_shapes():
    # the right column is far: the cells of the left column pair survive, nothing crosses the step
    rows = [[10.0, 10.0, 40.0], [10.0, 10.0, 40.0], [10.0, 10.0, 40.0]]
    assert faces_of(rows) == [[0, 3, 1], [1, 3, 4], [3, 6, 4], [4, 6, 7]]
    # a diagonal step: the upper-left triangle of pixels is near
    rows = [[10.0, 10.0, 10.0], [10.0, 10.0, 40.0], [10.0, 40.0, 40.0]]
    assert faces_of(rows) == [[0, 3, 1], [1, 3, 4], [1, 4, 2], [3, 6, 4], [5, 7, 8]]
    for shape in ((1, 1, 5), (1, 5, 1), (1, 1, 1), (3, 1, 4)):
        faces, face_offsets = oracle_mesh(np.ones(shape, dtype=np.float32), np.ones(shape, dtype=bool), INF)
        assert faces.shape == (0, 3) and face_offsets.tolist() == [0] * (shape[0] + 1)
        assert oracle_mesh_by_cells(np.ones(shape, dtype=np.float32), np.ones(shape, dtype=bool), INF)[0].shape == (0, 3)


def test_oracle_batch_of_two_no_face_joins_entries_and_the_rows_are_global():
    d = np.full((2, 2, 2), 5.0, dtype=np.float32)
    kept = np.ones((2, 2, 2), dtype=bool)
    kept[0, 0, 0] = False
    faces, face_offsets = oracle_mesh(d, kept, 1.0)
    # entry 0 holds rows 0 .. 2 (b, c, e), entry 1 rows 3 .. 6
    assert faces.tolist() == [[0, 1, 2], [3, 5, 4], [4, 5, 6]] and face_offsets.tolist() == [0, 1, 3]
    # two entries of one row each would be a cell if they were one image
    assert oracle_mesh(np.ones((2, 1, 2), dtype=np.float32), np.ones((2, 1, 2), dtype=bool), 1.0)[0].shape == (0, 3)


# ------------------------------------------------------------------------------------------------ invariants
def check_invariants(faces, face_offsets, disparity, kept, max_difference):
    """What holds for every mesh of this kind, whoever computed it."""
    D = np.asarray(disparity, dtype=np.float32)
    batch, height, width = D.shape
    rank, offsets = ranks_of(kept)
    pixel_of_row = np.flatnonzero(np.asarray(kept).reshape(-1))   # flat pixel (over the batch) of every packed row
    assert face_offsets[0] == 0 and face_offsets[-1] == len(faces) and np.all(np.diff(face_offsets) >= 0)
    if len(faces) == 0:
        return
    assert faces.min() >= 0 and faces.max() < len(pixel_of_row)
    assert np.all(faces[:, 0] != faces[:, 1]) and np.all(faces[:, 1] != faces[:, 2]) and np.all(faces[:, 0] != faces[:, 2])
    entry = np.searchsorted(face_offsets[1:], np.arange(len(faces)), side='right')
    assert np.all(faces >= offsets[entry][:, None]) and np.all(faces < offsets[entry + 1][:, None])
    flat = pixel_of_row[faces]
    n, y, x = flat // (height * width), flat // width % height, flat % width
    assert np.all(n == entry[:, None])
    assert np.all(y.max(axis=1) - y.min(axis=1) <= 1) and np.all(x.max(axis=1) - x.min(axis=1) <= 1)   # one 2 x 2 cell
    d = D.reshape(-1)[flat]
    for i, j in ((0, 1), (1, 2), (0, 2)):
        assert np.all(np.abs(d[:, i] - d[:, j]) <= np.float32(max_difference))   # fp32
    edges = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [0, 2]]]), axis=1)
    _, uses = np.unique(edges, axis=0, return_counts=True)
    assert uses.max() <= 2   # a manifold with boundary
    anchors = flat.min(axis=1)
    assert np.all(np.diff(anchors) >= 0)   # ordered by corner a (the least pixel of a face is a, or b where a is absent)


def random_scene(shape, seed):
    rng = np.random.RandomState(seed)
    d = (20.0 + rng.rand(*shape) * 2.0).astype(np.float32)
    d[rng.rand(*shape) < 0.1] += 30.0
    d = np.round(d * 4) / 4   # repeated values: ties
    kept = rng.rand(*shape) > 0.2
    return d.astype(np.float32), kept


def test_invariants_on_random_scenes_and_the_two_oracles_agree():
    for seed, shape in enumerate([(1, 7, 9), (2, 5, 6), (3, 4, 4), (1, 2, 17), (2, 9, 2)]):
        d, kept = random_scene(shape, seed)
        for max_difference in (0.0, 0.5, 1.0, INF):
            for flip in (False, True):
                faces, face_offsets = oracle_mesh(d, kept, max_difference, flip)
                slow = oracle_mesh_by_cells(d, kept, max_difference, flip)
                assert np.array_equal(faces, slow[0]) and np.array_equal(face_offsets, slow[1]), (shape, max_difference)
                check_invariants(faces, face_offsets, d, kept, max_difference)
    d, kept = random_scene((2, 40, 50), 9)
    faces, face_offsets = oracle_mesh(d, kept, 1.0)
    assert 100 < len(faces) < 2 * 2 * 39 * 49
    check_invariants(faces, face_offsets, d, kept, 1.0)


def test_a_fully_kept_constant_map_is_a_disc():
    for height, width in ((2, 2), (3, 5), (6, 4)):
        d = np.full((1, height, width), 9.0, dtype=np.float32)
        faces, face_offsets = oracle_mesh(d, np.ones_like(d, dtype=bool), 0.0)
        F = 2 * (height - 1) * (width - 1)
        assert len(faces) == F == face_offsets[-1]
        edges = np.unique(np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [0, 2]]]), axis=1), axis=0)
        assert height * width - len(edges) + F == 1   # V - E + F of a disc


# ------------------------------------------------------------------------------------------------ winding
def test_the_listed_order_faces_a_camera_at_the_origin():
    """In fp64, on the reprojection matrix of the test rig (X right, Y down, Z forward) and on the Q the GPU tests use:
    ((p1 - p0) x (p2 - p0)) . p0 < 0 for every face of a slanted surface, and > 0 with flip."""
    K = np.array([[0.7 * 64, 0.0, 31.5], [0.0, 0.7 * 64, 15.5], [0.0, 0.0, 1.0]])
    rig = pds.StereoRig(K, np.zeros(4), K, np.zeros(4), np.eye(3), np.array([-0.12, 0.0, 0.0]), (64, 32))
    plain = np.array([[1.0, 0.0, 0.0, -31.5], [0.0, 1.0, 0.0, -15.5], [0.0, 0.0, 0.0, 140.0], [0.0, 0.0, 1.0 / 0.12, 0.0]])
    yy, xx = np.mgrid[0:32, 0:64].astype(np.float64)
    for matrix in (rig.reprojection_matrix('rectified'), plain):
        for d in (np.full((32, 64), 20.0), 20.0 + 0.05 * xx - 0.03 * yy, 30.0 + 4.0 * np.sin(xx / 5.0) * np.cos(yy / 4.0)):
            homogeneous = np.stack([xx, yy, d, np.ones_like(d)], axis=-1) @ np.asarray(matrix, dtype=np.float64).T
            assert np.all(homogeneous[..., 3] > 0)
            points = (homogeneous[..., :3] / homogeneous[..., 3:]).reshape(-1, 3)
            assert np.all(points[:, 2] > 0)
            kept = np.ones((1, 32, 64), dtype=bool)
            for flip, sign in ((False, -1.0), (True, 1.0)):
                faces, _ = oracle_mesh(d[None].astype(np.float32), kept, INF, flip)
                assert len(faces) == 2 * 31 * 63
                p0, p1, p2 = points[faces[:, 0]], points[faces[:, 1]], points[faces[:, 2]]
                facing = np.einsum('ij,ij->i', np.cross(p1 - p0, p2 - p0), p0)
                assert np.all(sign * facing > 0), (flip, facing.min(), facing.max())


# ------------------------------------------------------------------------------------------------ the C ABI
def test_triangle_mesh_symbols_declared_exported_and_bound(hip_library):
    header = open(_lib.HEADER_PATH).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pds_triangle_mesh_workspace_bytes', 'pds_triangle_mesh_fwd'):
        assert name + '(' in header and hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert hip_library.pds_abi_version() == 7
    for name in ('triangle_mesh', 'TriangleMesh', 'TriangleMeshEntry', 'save_ply'):
        assert name in pds.__all__, name
    assert pds.TriangleMesh._fields == ('points', 'colors', 'index', 'offsets', 'faces', 'face_offsets')
    assert pds.triangle_mesh is pds.mesh.triangle_mesh
    # the table is in the header and in the module text
    for text in (header, pds.mesh.__doc__):
        for phrase in ('(a, c, b) then (b, c, e)', '(a, c, e) then (a, e, b)', 'e missing: (a, c, b)',
                       'c missing: (a, e, b)', '<= max_difference'):
            assert phrase in text, phrase
    # twice the cloud's tile words + 4 bytes per pixel rounded up to 256
    words = hip_library.pds_point_cloud_workspace_bytes
    assert hip_library.pds_triangle_mesh_workspace_bytes(1, 1, 1) == 2 * 512 + 256
    assert hip_library.pds_triangle_mesh_workspace_bytes(1, 540, 960) == 2 * words(1, 540, 960) + 540 * 960 * 4
    assert hip_library.pds_triangle_mesh_workspace_bytes(2, 3, 11) == 2 * words(2, 3, 11) + 512


def test_triangle_mesh_validation_needs_no_gpu(hip_library):
    lib = hip_library
    big = 1 << 24
    d, v, c, im, pts, col, idx, off, fa, fo, ws = [ctypes.c_void_p(big * n) for n in range(1, 12)]   # never dereferenced
    identity = (ctypes.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1).tolist())
    bad_matrix = (ctypes.c_float * 16)(*([1.0] * 15 + [NAN]))
    error = lib.pds_last_error
    need = lib.pds_triangle_mesh_workspace_bytes(1, 2, 3)
    assert need == 2 * 512 + 256

    def call(disparity=d, valid=v, confidence=c, min_confidence=0.0, matrix=identity, min_depth=-INF, max_depth=INF,
             max_difference=1.0, flip=0, image=im, layout=1, points=pts, colors=col, index=idx, offsets=off, capacity=6,
             faces=fa, face_offsets=fo, face_capacity=4, shape=(1, 2, 3), workspace=ws, workspace_bytes=need):
        return lib.pds_triangle_mesh_fwd(disparity, valid, confidence, min_confidence, matrix, min_depth, max_depth,
                                         max_difference, flip, image, layout, points, colors, index, offsets, capacity,
                                         faces, face_offsets, face_capacity, *shape, workspace, workspace_bytes, None)

    for name in ('disparity', 'matrix', 'points', 'offsets', 'faces', 'face_offsets', 'workspace'):
        assert call(**{name: None}) != 0 and error() == b'triangle_mesh: null pointer', name
    for shape in [(0, 2, 3), (1, 0, 3), (1, 2, 0), (-1, 2, 3)]:
        assert call(shape=shape) != 0 and b'triangle_mesh: bad shape' in error(), shape
        assert lib.pds_triangle_mesh_workspace_bytes(*shape) == 0 and b'triangle_mesh: bad shape' in error(), shape
    for shape in [(1, 1 << 15, 1 << 15), (4, 1 << 14, 1 << 14), (1, 1 << 16, 1 << 16)]:   # 2 * B * H * W = 2^31, 2^33
        assert call(shape=shape, workspace_bytes=1 << 40) != 0 and b'32-bit indices' in error(), shape
        assert lib.pds_triangle_mesh_workspace_bytes(*shape) == 0 and b'32-bit indices' in error(), shape
    assert lib.pds_triangle_mesh_workspace_bytes(1, (1 << 15) - 1, 1 << 15) > 0   # 2 * B * H * W = 2^31 - 2^16
    assert lib.pds_triangle_mesh_workspace_bytes(1, 1, (1 << 30) - 1) > 0         # 2^31 - 2: the largest accepted
    for value in (-1, -(1 << 40)):
        assert call(capacity=value) != 0 and b'triangle_mesh: capacity must be >= 0' in error(), value
        assert call(face_capacity=value) != 0 and b'face_capacity must be >= 0' in error(), value
    for value in (NAN, -1.0, -1e-30, -INF):
        assert call(max_difference=value) != 0 and b'max_difference must be >= 0' in error(), value
    assert call(image=None) != 0 and b'colors without an image' in error()
    assert call(layout=2) != 0 and b'bad image_layout' in error()
    assert call(workspace_bytes=need - 1) != 0 and b'workspace too small (1279 < 1280)' in error()
    assert call(min_confidence=NAN) != 0 and b'min_confidence is NaN' in error()
    assert call(min_depth=NAN) != 0 and b'a depth bound is NaN' in error()
    assert call(min_depth=2.0, max_depth=1.0) != 0 and b'min_depth 2 > max_depth 1' in error()
    assert call(faces=ctypes.c_void_p(fa.value + 2)) != 0 and b'not 4-byte aligned' in error()
    assert call(face_offsets=ctypes.c_void_p(fo.value + 1)) != 0 and b'not 4-byte aligned' in error()
    assert call(workspace=ctypes.c_void_p(ws.value + 4)) != 0 and b'workspace is not 16-byte aligned' in error()
    assert call(faces=d) != 0 and b'an output aliases an input' in error()
    assert call(face_offsets=ctypes.c_void_p(v.value + 4)) != 0 and b'an output aliases an input' in error()
    assert call(workspace=c) != 0 and b'an output aliases an input' in error()
    assert call(faces=ctypes.c_void_p(pts.value + 24)) != 0 and b'an output aliases another output' in error()
    assert call(face_offsets=ctypes.c_void_p(off.value + 4)) != 0 and b'an output aliases another output' in error()
    assert call(workspace=ctypes.c_void_p(fa.value + 16)) != 0 and b'an output aliases another output' in error()
    assert call(matrix=bad_matrix) != 0 and b'non-finite matrix' in error()


# ------------------------------------------------------------------------------------------------ Python
def test_triangle_mesh_python_errors():
    ok, Q = torch.zeros(1, 4, 5), np.eye(4)
    with pytest.raises(TypeError, match='disparity must be a torch.Tensor'):
        pds.triangle_mesh(np.zeros((1, 4, 5), dtype=np.float32), Q)
    for bad in (ok.double(), ok.half(), ok.to(torch.int32)):
        with pytest.raises(TypeError, match='disparity must be float32'):
            pds.triangle_mesh(bad, Q)
    for bad in (torch.zeros(4, 5), torch.zeros(1, 1, 4, 5)):
        with pytest.raises(ValueError, match='disparity must have 3 dimensions'):
            pds.triangle_mesh(bad, Q)
    for bad in (np.eye(3), np.full((4, 4), NAN)):
        with pytest.raises(ValueError, match='matrix must be a finite 4x4'):
            pds.triangle_mesh(ok, bad)
    with pytest.raises(ValueError, match='min_confidence is NaN'):
        pds.triangle_mesh(ok, Q, min_confidence=NAN)
    with pytest.raises(ValueError, match=r'min_depth 2\.0 > max_depth 1\.0'):
        pds.triangle_mesh(ok, Q, min_depth=2.0, max_depth=1.0)
    for bad in (NAN, -1.0, -1e-300, -INF):
        with pytest.raises(ValueError, match='max_difference must be >= 0 and not NaN'):
            pds.triangle_mesh(ok, Q, max_difference=bad)
    with pytest.raises((TypeError, ValueError)):
        pds.triangle_mesh(ok, Q, max_difference='wide')
    for bad in (1, 'yes', None):
        with pytest.raises(TypeError, match='flip must be a bool'):
            pds.triangle_mesh(ok, Q, flip=bad)
    for name in ('capacity', 'face_capacity'):
        for bad in (2.0, '3', True):
            with pytest.raises(TypeError, match='%s must be an integer or None' % name):
                pds.triangle_mesh(ok, Q, **{name: bad})
        with pytest.raises(ValueError, match='%s must be >= 0' % name):
            pds.triangle_mesh(ok, Q, **{name: -1})
    with pytest.raises(ValueError, match=r'a uint8 image must be \[B, H, W, 3\]'):
        pds.triangle_mesh(ok, Q, image=torch.zeros(1, 3, 4, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match='does not match disparity'):
        pds.triangle_mesh(ok, Q, image=torch.zeros(1, 3, 4, 6))
    with pytest.raises(ValueError, match='valid must be torch.bool'):
        pds.triangle_mesh(ok, Q, valid=torch.ones(1, 4, 5))
    with pytest.raises(TypeError, match='confidence must be float32'):
        pds.triangle_mesh(ok, Q, confidence=ok.double())
    with pytest.raises(ValueError, match='32-bit indices'):
        pds.triangle_mesh(torch.zeros(1, 1 << 15, 1 << 15, device='meta'), Q)
    # every argument in order, and still no CPU fallback
    for kwargs in ({}, {'image': torch.zeros(1, 3, 4, 5), 'valid': torch.ones(1, 4, 5, dtype=torch.bool),
                        'confidence': ok, 'min_confidence': 0.5, 'min_depth': 0.1, 'max_depth': 0.1,
                        'max_difference': INF, 'flip': True, 'with_index': True, 'capacity': np.int64(7),
                        'face_capacity': 0, 'trim': False}):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            pds.triangle_mesh(ok, Q, **kwargs)
    parameters = inspect.signature(pds.triangle_mesh).parameters
    assert [(n, p.default) for n, p in parameters.items()][2:] == [
        ('image', None), ('valid', None), ('confidence', None), ('min_confidence', 0.0), ('min_depth', None),
        ('max_depth', None), ('max_difference', 1.0), ('flip', False), ('with_index', False), ('capacity', None),
        ('face_capacity', None), ('trim', True)]
    assert 'ONLY synchronisation' in pds.triangle_mesh.__doc__ and 'without any synchronisation' in pds.triangle_mesh.__doc__


def test_the_rig_has_the_counterpart_of_point_cloud():
    parameters = inspect.signature(pds.StereoRig.triangle_mesh).parameters
    assert list(parameters) == ['self', 'disparity', 'image', 'valid', 'confidence', 'min_confidence', 'frame', 'kw']
    assert list(parameters) == list(inspect.signature(pds.StereoRig.point_cloud).parameters)
    assert parameters['frame'].default == 'rectified' and parameters['kw'].kind is inspect.Parameter.VAR_KEYWORD
    K = np.array([[180.0, 0.0, 127.5], [0.0, 180.0, 63.5], [0.0, 0.0, 1.0]])
    rig = pds.StereoRig(K, np.zeros(4), K, np.zeros(4), np.eye(3), np.array([-0.12, 0.0, 0.0]), (256, 128))
    with pytest.raises(ValueError, match="frame must be 'rectified' or 'camera'"):
        rig.triangle_mesh(torch.zeros(1, 128, 256), frame='world')
    with pytest.raises(ValueError, match='max_difference'):
        rig.triangle_mesh(torch.zeros(1, 128, 256), max_difference=-1.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rig.triangle_mesh(torch.zeros(1, 128, 256), frame='camera', flip=True)
    assert pds.rectification.Reconstruction._fields == ('left_image', 'right_image', 'disparity', 'valid', 'points')


# ------------------------------------------------------------------------------------------------ TriangleMesh on the host
def hand_made(colors):
    points = torch.tensor([[0.5, -1.25, 3.0], [1e-40, 2.0, -0.0], [7.0, 8.0, 9.0], [-3.5, 1e30, 0.125], [1.0, 2.0, 3.0]])
    index = torch.tensor([4, 0, 1, 2, 3], dtype=torch.int32)
    faces = torch.tensor([[1, 3, 2], [2, 3, 4], [1, 4, 2]], dtype=torch.int32)
    return pds.TriangleMesh(points, colors, index, torch.tensor([0, 1, 1, 5], dtype=torch.int32), faces,
                            torch.tensor([0, 0, 0, 3], dtype=torch.int32))


def read_ply(path):
    """-> (structured array of the vertices, faces [F, 3] int32, header lines), parsed from the file's own header."""
    blob = open(path, 'rb').read()
    end = blob.index(b'end_header\n') + len(b'end_header\n')
    lines = blob[:end].decode('ascii').splitlines()
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0' and lines[-1] == 'end_header'
    elements = [l for l in lines if l.startswith('element ')]
    assert [l.split()[1] for l in elements] == ['vertex', 'face']
    count, face_count = int(elements[0].split()[-1]), int(elements[1].split()[-1])
    cut = lines.index(elements[1])
    assert lines[cut + 1:-1] == ['property list uchar int vertex_indices']
    kinds = {'float': '<f4', 'uchar': 'u1'}
    fields = np.dtype([(l.split()[2], kinds[l.split()[1]]) for l in lines[:cut] if l.startswith('property ')])
    vertices = np.frombuffer(blob[end:end + count * fields.itemsize], dtype=fields)
    records = np.frombuffer(blob[end + count * fields.itemsize:], dtype=np.dtype([('n', 'u1'), ('v', '<i4', (3,))]))
    assert records.dtype.itemsize == 13 and len(blob) == end + count * fields.itemsize + 13 * face_count
    assert records.shape == (face_count,) and np.all(records['n'] == 3)
    return vertices, records['v'].astype(np.int32).reshape(-1, 3), lines


def test_ply_round_trip_with_faces(tmp_path):
    colours = torch.tensor([[0, 128, 255], [1, 2, 3], [250, 251, 252], [9, 8, 7], [4, 5, 6]], dtype=torch.uint8)
    for colors in (None, colours):
        mesh = hand_made(colors)
        path = str(tmp_path / 'mesh.ply')
        mesh.save_ply(path)
        vertices, faces, _ = read_ply(path)
        assert vertices.dtype.itemsize == (12 if colors is None else 15) and vertices.shape == (5,)
        got = np.stack([vertices['x'], vertices['y'], vertices['z']], axis=1)
        assert np.array_equal(got.view(np.int32), mesh.points.numpy().view(np.int32))
        assert np.array_equal(faces, mesh.faces.numpy())
        if colors is not None:
            assert np.array_equal(np.stack([vertices['red'], vertices['green'], vertices['blue']], axis=1), colours.numpy())
        # the module function writes the same bytes
        other = str(tmp_path / 'other.ply')
        pds.save_ply(other, mesh)
        assert open(other, 'rb').read() == open(path, 'rb').read()
        # one entry alone: its vertices and its faces, rebased to it
        mesh.save_ply(path, entry=2)
        vertices, faces, _ = read_ply(path)
        assert vertices['x'].tolist() == [np.float32(1e-40), 7.0, -3.5, 1.0]
        assert faces.tolist() == [[0, 2, 1], [1, 2, 3], [0, 3, 1]]
        mesh.save_ply(path, entry=0)
        vertices, faces, _ = read_ply(path)
        assert vertices.shape == (1,) and faces.shape == (0, 3)
        with pytest.raises(IndexError):
            mesh.save_ply(path, entry=3)
    # with normals: x y z nx ny nz (then the colours), then the faces
    mesh = hand_made(colours)
    normals = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    pds.save_ply(path, mesh, normals=normals)
    vertices, faces, _ = read_ply(path)
    assert vertices.dtype.names == ('x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue')
    assert vertices['nz'].tolist() == [2.0, 5.0, 8.0, 11.0, 14.0] and np.array_equal(faces, mesh.faces.numpy())
    # a mesh whose vertices were cut cannot be written: its faces name rows the file would not hold
    cut = pds.TriangleMesh(mesh.points[:3], None, None, mesh.offsets, mesh.faces, mesh.face_offsets)
    with pytest.raises(ValueError, match='were cut at capacity 3'):
        cut.save_ply(path)
    with pytest.raises(TypeError, match='cloud must be a PointCloud or a TriangleMesh'):
        pds.save_ply(path, (mesh.points, None, None, mesh.offsets))


def test_the_ply_of_a_point_cloud_is_what_it_was(tmp_path):
    """save_ply(path, cloud) writes the bytes PointCloud.save_ply writes (the existing writer, which this feature does
    not touch), and the file of mesh.cloud() is the file of the mesh up to the face element."""
    colours = torch.tensor([[0, 128, 255], [1, 2, 3], [250, 251, 252], [9, 8, 7], [4, 5, 6]], dtype=torch.uint8)
    for colors in (None, colours, colours.to(torch.float32) * 1.01):
        mesh = hand_made(colors)
        cloud = mesh.cloud()
        assert isinstance(cloud, pds.PointCloud) and cloud.points is mesh.points and cloud.offsets is mesh.offsets
        for entry in (None, 0, 2):
            a, b, c = (str(tmp_path / name) for name in ('a.ply', 'b.ply', 'c.ply'))
            pds.save_ply(a, cloud, entry=entry)
            cloud.save_ply(b, entry=entry)
            assert open(a, 'rb').read() == open(b, 'rb').read()
            vertices, lines = read_cloud_ply(a)   # the reader of tests/test_point_cloud_host.py: one element only
            mesh.save_ply(c, entry=entry)
            assert read_ply(c)[0].tobytes() == vertices.tobytes()
            assert read_ply(c)[2][:len(lines) - 1] == lines[:-1]


def test_entries_counts_and_the_shared_host_offsets():
    mesh = hand_made(None)
    assert mesh.host_offsets() == [0, 1, 1, 5] and mesh.host_face_offsets() == [0, 0, 0, 3]
    assert mesh.size() == 5 and mesh.face_count() == 3
    assert mesh.cloud().__dict__['_host_offsets'] is mesh.host_offsets()   # read once, shared
    entry = mesh.entry(2)
    assert isinstance(entry, pds.TriangleMeshEntry) and entry._fields == ('points', 'colors', 'index', 'faces')
    assert entry.points.shape == (4, 3) and entry.points.data_ptr() == mesh.points[1:].data_ptr()
    assert entry.faces.tolist() == [[0, 2, 1], [1, 2, 3], [0, 3, 1]] and entry.index.tolist() == [0, 1, 2, 3]
    assert mesh.entry(0).faces.shape == (0, 3) and mesh.entry(1).points.shape == (0, 3)
    for b in (-1, 3):
        with pytest.raises(IndexError):
            mesh.entry(b)
    points, colors, index, offsets, faces, face_offsets = mesh   # still a tuple of six
    assert faces is mesh.faces and face_offsets is mesh.face_offsets
    # face_offsets[B] = 3 faces were found, the buffer holds 2
    cut = pds.TriangleMesh(mesh.points, None, None, mesh.offsets, mesh.faces[:2], mesh.face_offsets)
    assert cut.face_count() == 2 and cut.entry(2).faces.tolist() == [[0, 2, 1], [1, 2, 3]]
    gathered = mesh.cloud().gather(torch.arange(3 * 2 * 3, dtype=torch.float32).reshape(3, 2, 3))
    assert gathered.shape == (5,)
