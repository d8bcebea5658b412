"""CPU: the triangle mesh of a TSDF volume (pds_tsdf_mesh_workspace_bytes, pds_tsdf_mesh_fwd; TsdfVolume.extract_mesh,
SurfaceMesh).  The entry points are declared, exported and bound; every refusal of the C entry point and of the Python
method is reached without a GPU; and the contract itself is restated in numpy (oracle_mesh) and held to what it promises:
a closed, consistently wound manifold wherever the volume is observed.

The oracle decides on the float32 bits and computes positions in fp64.  Its winding does not come from a table: for every
(tetrahedron, sign pattern) it places the vertices at the midpoints of their edges in fp64 and compares the face normal
with the vector from the negative corners' centroid to the positive corners' (oracle_faces_of).  The kernel derives its
6 x 16 bits on its own, at compile time and in integers, so the two agree only if both follow the rule."""
import collections
import ctypes
import functools
import inspect
import itertools

import numpy as np
import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib

NAN, INF = float('nan'), float('inf')
TILE = 1024          # csrc/common.hpp: kPointCloudTile
MAX_GROUPS = 2048    # csrc/common.hpp: kTsdfMeshMaxGroups
PERMUTATIONS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))

# index int64 ascending = 7 v + (d - 1); points fp64 [N, 3]; normals fp64 [N, 3] with NaN rows; gradient_norm fp64 [N]: |g|
# before the normalisation, NaN where a stencil fails; faces int64 [F, 3] rows of points; keys int64 [F] = 6 c + t
Mesh = collections.namedtuple('Mesh', ['index', 'points', 'normals', 'gradient_norm', 'faces', 'keys'])


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def offset_of(d):
    return (d & 1, (d >> 1) & 1, (d >> 2) & 1)


def corners_of(t):
    a, b, _ = PERMUTATIONS[t]
    return (0, 1 << a, (1 << a) | (1 << b), 7)


def faces_per_pattern(signs):
    """How many faces the contract lists for the four signs of a tetrahedron."""
    negative = sum(bool(s) for s in signs)
    return {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[negative]


@functools.lru_cache(maxsize=None)
def oracle_faces_of(t, pattern):
    """The faces of tetrahedron t for the sign pattern (bit m: the corner at position m is negative), each a tuple of three
    edges (m, n), m < n, of positions; listed as the contract lists them and wound by fp64 geometry on the midpoints."""
    negative = [m for m in range(4) if pattern >> m & 1]
    positive = [m for m in range(4) if not pattern >> m & 1]
    if not negative or not positive:
        return ()
    if len(negative) == 1 or len(positive) == 1:
        (A,), (B, C, D) = (negative, positive) if len(negative) == 1 else (positive, negative)
        listed = [((A, B), (A, C), (A, D))]
    else:
        (A, B), (C, D) = negative, positive
        listed = [((A, C), (A, D), (B, D)), ((A, C), (B, D), (B, C))]
    at = np.array([offset_of(c) for c in corners_of(t)], dtype=np.float64)
    towards = at[positive].mean(axis=0) - at[negative].mean(axis=0)
    faces = []
    for face in listed:
        m0, m1, m2 = (0.5 * (at[p] + at[q]) for p, q in face)
        normal = np.cross(m1 - m0, m2 - m0)
        assert abs(normal @ towards) > 1e-3   # (never undecided: the midpoints' plane separates the two sides)
        if normal @ towards < 0:
            face = (face[0], face[2], face[1])
        faces.append(tuple(tuple(sorted(edge)) for edge in face))
    return tuple(faces)


def shifted(a, d, fill):
    """a[k + dz, j + dy, i + dx] for offset(d) = (dx, dy, dz), `fill` where that lies outside."""
    dx, dy, dz = offset_of(d)
    out = np.full_like(a, fill)
    nz, ny, nx = a.shape[:3]
    out[:nz - dz, :ny - dy, :nx - dx] = a[dz:, dy:, dx:]
    return out


def oracle_mesh(tsdf, weight, origin, voxel_size, min_weight=1.0):
    """tsdf, weight float32 [nz, ny, nx] -> Mesh: the contract of pds_tsdf_mesh_fwd in numpy."""
    tsdf, weight = np.asarray(tsdf), np.asarray(weight)
    assert tsdf.dtype == weight.dtype == np.float32 and tsdf.shape == weight.shape and tsdf.ndim == 3
    nz, ny, nx = tsdf.shape
    observed = weight >= np.float32(min_weight)
    negative = tsdf < 0
    value = tsdf.astype(np.float64)
    origin, voxel_size = f32(origin), float(f32(voxel_size))
    kk, jj, ii = np.mgrid[0:nz, 0:ny, 0:nx]
    flat = (kk * ny + jj) * nx + ii
    # g(c) and whether its six voxels are inside and observed
    gradient = np.zeros((nz, ny, nx, 3))
    whole = np.ones((nz, ny, nx), dtype=bool)
    for m, axis in enumerate((2, 1, 0)):
        plus, minus = np.roll(value, -1, axis), np.roll(value, 1, axis)
        position = np.arange(tsdf.shape[axis]).reshape([-1 if a == axis else 1 for a in range(3)])
        whole &= np.roll(observed, -1, axis) & np.roll(observed, 1, axis) & (position >= 1) & (position + 1 < tsdf.shape[axis])
        gradient[..., m] = plus - minus
    index, points, normals, norms = [], [], [], []
    for d in range(1, 8):
        crossing = observed & shifted(observed, d, False) & (negative != shifted(negative, d, False))
        where = np.nonzero(crossing)
        dx, dy, dz = offset_of(d)
        neighbour = (where[0] + dz, where[1] + dy, where[2] + dx)
        tv, tn = value[where], value[neighbour]
        r = tv / (tv - tn)
        at = np.stack([ii[where], jj[where], kk[where]], axis=1) + 0.5 + r[:, None] * np.array([dx, dy, dz])
        g = (1.0 - r)[:, None] * gradient[where] + r[:, None] * gradient[neighbour]
        length = np.sqrt((g * g).sum(axis=1))
        stencil = whole[where] & whole[neighbour]
        with np.errstate(invalid='ignore', divide='ignore'):
            unit = np.where((stencil & (length > 0))[:, None], g / length[:, None], NAN)
        index.append(7 * flat[where] + (d - 1))
        points.append(origin + voxel_size * at)
        normals.append(unit)
        norms.append(np.where(stencil, length, NAN))
    index = np.concatenate(index).astype(np.int64)
    order = np.argsort(index, kind='stable')
    index = index[order]
    # faces: per cell, tetrahedron and sign pattern
    keys, rows = [], []
    if min(nx, ny, nz) > 1:
        cell = flat[:-1, :-1, :-1].reshape(-1)
        stride = np.array([1, nx, nx * ny])
        corner = [cell + int(np.dot(offset_of(m), stride)) for m in range(8)]
        seen, sign = observed.reshape(-1), negative.reshape(-1)
        for t in range(6):
            p = corners_of(t)
            complete = seen[corner[p[0]]] & seen[corner[p[1]]] & seen[corner[p[2]]] & seen[corner[p[3]]]
            pattern = sum(sign[corner[p[m]]].astype(np.int64) << m for m in range(4))
            for s in range(1, 15):
                chosen = np.nonzero(complete & (pattern == s))[0]
                if len(chosen) == 0:
                    continue
                for f, face in enumerate(oracle_faces_of(t, s)):
                    wanted = np.stack([7 * corner[p[m]][chosen] + ((p[m] ^ p[n]) - 1) for m, n in face], axis=1)
                    row = np.searchsorted(index, wanted)
                    assert (index[np.minimum(row, len(index) - 1)] == wanted).all()   # faces name vertices that exist
                    keys.append(2 * (6 * cell[chosen] + t) + f)
                    rows.append(row)
    if keys:
        keys, rows = np.concatenate(keys), np.concatenate(rows)
        by_key = np.argsort(keys, kind='stable')
        keys, rows = keys[by_key] // 2, rows[by_key]
    else:
        keys, rows = np.zeros(0, dtype=np.int64), np.zeros((0, 3), dtype=np.int64)
    return Mesh(index, np.concatenate(points)[order], np.concatenate(normals)[order], np.concatenate(norms)[order],
                rows.astype(np.int64), keys.astype(np.int64))


def mesh_topology(faces):
    """-> (open_edges: the directed edges (u, w) whose reverse is in no face, repeated: directed edges in more than one
    face, edges: the number of undirected edges, referenced: the number of vertices some face names)."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    directed = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    span = int(faces.max(initial=0)) + 1
    code = directed[:, 0] * span + directed[:, 1]
    unique, counts = np.unique(code, return_counts=True)
    reverse = directed[:, 1] * span + directed[:, 0]
    open_edges = directed[~np.isin(reverse, unique)]
    undirected = np.unique(np.minimum(directed[:, 0], directed[:, 1]) * span + np.maximum(directed[:, 0], directed[:, 1]))
    return open_edges, int((counts > 1).sum()), len(undirected), len(np.unique(faces))


def sphere_volume(n=20, centre=(9.3, 10.1, 9.7), radius=6.4, truncation=2.5):
    """A sphere sampled at the voxel centres of an n^3 volume, negative inside, every voxel observed."""
    kk, jj, ii = np.mgrid[0:n, 0:n, 0:n].astype(np.float64)
    distance = np.sqrt((ii - centre[0]) ** 2 + (jj - centre[1]) ** 2 + (kk - centre[2]) ** 2)
    tsdf = np.clip((distance - radius) / truncation, -1.0, 1.0).astype(np.float32)
    assert not (tsdf == 0).any()
    return tsdf, np.ones_like(tsdf), np.array(centre) + 0.5   # (the centre in units of voxel_size from the origin)


def check_closed_sphere(index, points, faces, centre, origin, voxel_size):
    """The closed-manifold properties of the 20^3 sphere, on any implementation's output."""
    faces = np.asarray(faces, dtype=np.int64)
    points = np.asarray(points, dtype=np.float64)
    open_edges, repeated, edges, referenced = mesh_topology(faces)
    assert len(open_edges) == 0 and repeated == 0          # every undirected edge in two faces, once in each direction
    assert len(points) - edges + len(faces) == 2           # V - E + F = 2
    assert referenced == len(points) == len(index)         # every vertex referenced
    assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
    corner = points[faces]
    normal = np.cross(corner[:, 1] - corner[:, 0], corner[:, 2] - corner[:, 0])
    outward = corner.mean(axis=1) - (np.asarray(origin) + voxel_size * np.asarray(centre))
    assert ((normal * outward).sum(axis=1) > 0).all()      # negative inside: the faces look outward
    return len(points), edges, len(faces)


# ------------------------------------------------------------------------------------------------ declarations
def test_entry_points_are_declared_exported_and_bound(hip_library):
    header = open(_lib.HEADER_PATH).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pds_tsdf_mesh_workspace_bytes', 'pds_tsdf_mesh_fwd'):
        assert name + '(' in header and hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert hip_library.pds_abi_version() == 7 and '#define PDS_ABI_VERSION 7' in header
    assert pds.SurfaceMesh._fields == ('mesh', 'normals') and 'SurfaceMesh' in pds.__all__
    assert 'tsdf_mesh.hip' in [s.rsplit('/', 1)[-1] for s in _lib.sources()]
    common = open(_lib._CSRC + '/common.hpp').read()
    assert 'constexpr int kTsdfMeshMaxGroups = %d;' % MAX_GROUPS in common
    parameters = inspect.signature(pds.TsdfVolume.extract_mesh).parameters
    assert [(n, p.default) for n, p in parameters.items()][1:] == [
        ('min_weight', 1.0), ('with_normals', True), ('capacity', None), ('face_capacity', None), ('trim', True)]
    # the workspace: two lots of tile words (4 per tile rounded up to 256, plus 256), 4 bytes and 1 byte per voxel, each
    # rounded up to 256
    sizes = hip_library.pds_tsdf_mesh_workspace_bytes
    rounded = (lambda n: (n + 255) // 256 * 256)
    for dims in ((1, 1, 1), (2, 2, 2), (20, 20, 20), (33, 5, 7), (3, 3, 130), (256, 256, 256)):
        voxels = dims[0] * dims[1] * dims[2]
        words = rounded((voxels + TILE - 1) // TILE * 4) + 256
        assert sizes(*dims) == 2 * words + rounded(4 * voxels) + rounded(voxels), dims
        assert sizes(*dims) >= 2 * hip_library.pds_tsdf_extract_workspace_bytes(*dims) + 5 * voxels


# ------------------------------------------------------------------------------------------------ refusals
def test_mesh_validation_needs_no_gpu(hip_library):
    lib = hip_library
    big = 1 << 24
    t, w, ws, pts, nrm, idx, off, fcs, foff = [ctypes.c_void_p(big * n) for n in range(1, 10)]   # never dereferenced
    floats = (lambda values: (ctypes.c_float * len(values))(*values))
    origin = floats([0.0, 0.0, 0.0])
    error = lib.pds_last_error
    need = lib.pds_tsdf_mesh_workspace_bytes(4, 3, 2)
    assert need == 2 * 512 + 256 + 256

    def mesh(tsdf=t, weight=w, origin=origin, voxel_size=0.1, min_weight=1.0, points=pts, normals=nrm, index=idx,
             offsets=off, capacity=10, faces=fcs, face_offsets=foff, face_capacity=10, dims=(4, 3, 2), workspace=ws,
             workspace_bytes=need):
        return lib.pds_tsdf_mesh_fwd(tsdf, weight, origin, voxel_size, min_weight, points, normals, index, offsets,
                                     capacity, faces, face_offsets, face_capacity, *dims, workspace, workspace_bytes, None)

    for name in ('tsdf', 'weight', 'origin', 'points', 'offsets', 'faces', 'face_offsets', 'workspace'):
        assert mesh(**{name: None}) != 0 and error() == b'tsdf_mesh: null pointer', name
    for dims in [(0, 3, 2), (4, 0, 2), (4, 3, 0), (-4, 3, 2)]:
        assert mesh(dims=dims) != 0 and b'tsdf: bad volume' in error(), dims
        assert lib.pds_tsdf_mesh_workspace_bytes(*dims) == 0 and b'tsdf: bad volume' in error(), dims
    assert lib.pds_tsdf_mesh_workspace_bytes((1 << 24) + 1, 1, 1) == 0 and b'above 2^24' in error()
    # 12 * cells is the tighter limit of a volume of some thickness: 563^3 = 178 453 547 <= (2^31 - 1) / 12 = 178 956 970
    # < 564^3; 7 * voxels is the limit where there are few cells or none
    assert lib.pds_tsdf_mesh_workspace_bytes(564, 564, 564) > 0
    assert lib.pds_tsdf_mesh_workspace_bytes(565, 565, 565) == 0 and b'12 * cells does not fit' in error()
    assert mesh(dims=(565, 565, 565)) != 0 and b'12 * cells does not fit' in error()
    assert lib.pds_tsdf_mesh_workspace_bytes(675, 675, 675) == 0 and b'7 * nx * ny * nz does not fit' in error()
    assert lib.pds_tsdf_extract_workspace_bytes(675, 675, 675) > 0     # (extract_points still takes it)
    assert lib.pds_tsdf_mesh_workspace_bytes(1 << 24, 18, 1) > 0       # (no cell: only the vertices count)
    assert lib.pds_tsdf_mesh_workspace_bytes(1 << 24, 19, 1) == 0 and b'7 * nx * ny * nz does not fit' in error()
    assert mesh(dims=(1 << 24, 19, 1)) != 0 and b'7 * nx * ny * nz does not fit' in error()
    assert mesh(capacity=-1) != 0 and b'tsdf_mesh: capacity must be >= 0 (got -1)' in error()
    assert mesh(face_capacity=-2) != 0 and b'face_capacity must be >= 0 (got -2)' in error()
    assert mesh(workspace_bytes=need - 1) != 0 and b'workspace too small (%d < %d)' % (need - 1, need) in error()
    for bad in (0.0, -1.0, NAN, INF):
        assert mesh(voxel_size=bad) != 0 and b'voxel_size must be positive and finite' in error(), bad
    assert mesh(min_weight=NAN) != 0 and b'min_weight is NaN' in error()
    for bad in ([0.0, NAN, 0.0], [INF, 0.0, 0.0]):
        assert mesh(origin=floats(bad)) != 0 and b'non-finite origin' in error()
    for name, p in (('tsdf', t), ('weight', w), ('points', pts), ('normals', nrm), ('index', idx), ('offsets', off),
                    ('faces', fcs), ('face_offsets', foff)):
        assert mesh(**{name: ctypes.c_void_p(p.value + 2)}) != 0 and b'not 4-byte aligned' in error(), name
    assert mesh(workspace=ctypes.c_void_p(ws.value + 4)) != 0 and b'workspace is not 16-byte aligned' in error()
    # nothing written may overlap anything (4 x 3 x 2 voxels: 96 bytes; 10 rows: 120 / 40 bytes; the offsets: 8)
    assert mesh(points=t) != 0 and b'an output aliases an input' in error()
    assert mesh(faces=ctypes.c_void_p(w.value + 92)) != 0 and b'an output aliases an input' in error()
    assert mesh(face_offsets=ctypes.c_void_p(t.value + 4)) != 0 and b'an output aliases an input' in error()
    assert mesh(workspace=ctypes.c_void_p(w.value - need + 16)) != 0 and b'an output aliases an input' in error()
    assert mesh(normals=ctypes.c_void_p(pts.value + 116)) != 0 and b'an output aliases another output' in error()
    assert mesh(offsets=ctypes.c_void_p(idx.value + 36)) != 0 and b'an output aliases another output' in error()
    assert mesh(faces=ctypes.c_void_p(pts.value + 116)) != 0 and b'an output aliases another output' in error()
    assert mesh(face_offsets=ctypes.c_void_p(off.value + 4)) != 0 and b'an output aliases another output' in error()
    assert mesh(face_offsets=ctypes.c_void_p(fcs.value + 116)) != 0 and b'an output aliases another output' in error()
    assert mesh(workspace=ctypes.c_void_p(fcs.value + 112)) != 0 and b'an output aliases another output' in error()
    # a capacity of 0 holds no row, so nothing can overlap there
    assert mesh(capacity=0, normals=pts, workspace_bytes=need - 1) != 0 and b'workspace too small' in error()
    assert mesh(face_capacity=0, faces=pts, workspace_bytes=need - 1) != 0 and b'workspace too small' in error()


class HostVolume(pds.TsdfVolume):
    """A volume whose state stays on the host: the argument checks of extract_mesh run up to the point where they ask
    where the tensors live (the device of tests/test_tsdf_host.py, restated)."""

    def __init__(self, *args, **kw):
        try:
            super(HostVolume, self).__init__(*args, device='cpu', **kw)
        except RuntimeError as e:
            assert 'no CPU fallback' in str(e)
        # (expanded views: a volume at the limits of the index range costs no memory)
        self._tsdf, self._weight = torch.ones(1).expand(self.shape), torch.zeros(1).expand(self.shape)


def test_extract_mesh_python_errors():
    volume = HostVolume((0.0, 0.0, 0.0), 0.1, (4, 3, 2), 0.3)
    with pytest.raises(ValueError, match='min_weight is NaN'):
        volume.extract_mesh(min_weight=NAN)
    with pytest.raises(TypeError, match='min_weight|float'):
        volume.extract_mesh(min_weight=None)
    for name in ('capacity', 'face_capacity'):
        for bad in (2.5, 'many', True):
            with pytest.raises(TypeError, match='%s must be an integer or None' % name):
                volume.extract_mesh(**{name: bad})
        with pytest.raises(ValueError, match='%s must be >= 0' % name):
            volume.extract_mesh(**{name: -1})
    # 7 * voxels is refused where 3 * voxels, the constructor's limit, is not
    wide = HostVolume((0.0, 0.0, 0.0), 0.1, (675, 675, 675), 0.3)
    with pytest.raises(ValueError, match='7 \\* nx \\* ny \\* nz = %d does not fit 32-bit indices' % (7 * 675 ** 3)):
        wide.extract_mesh(capacity=10, face_capacity=10)
    thick = HostVolume((0.0, 0.0, 0.0), 0.1, (565, 565, 565), 0.3)
    with pytest.raises(ValueError, match='12 \\* cells = %d does not fit 32-bit indices' % (12 * 564 ** 3)):
        thick.extract_mesh(capacity=10, face_capacity=10)
    # every argument in order, and still no CPU fallback
    for kwargs in ({}, dict(min_weight=0.5, with_normals=False, capacity=0, face_capacity=7, trim=False)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            volume.extract_mesh(**kwargs)
    text = pds.TsdfVolume.extract_mesh.__doc__
    assert 'ONLY synchronisation' in text and 'without any synchronisation' in text and 'give both' in text
    text = inspect.getmodule(pds.TsdfVolume).__doc__
    for phrase in ('extract_mesh', 'pds_tsdf_mesh_fwd', 'marching tetrahedra', 'index = 7 v + (d - 1)',
                   'may be unreferenced', 'marching-cubes faces', 'colour'):
        assert phrase in text, phrase


# ------------------------------------------------------------------------------------------------ the rule itself
def test_winding_is_a_function_of_tetrahedron_and_signs():
    for t in range(6):
        p = corners_of(t)
        assert p[0] == 0 and p[3] == 7 and bin(p[1]).count('1') == 1 and bin(p[2]).count('1') == 2 and p[1] & p[2] == p[1]
        for s in range(16):
            faces = oracle_faces_of(t, s)
            assert len(faces) == faces_per_pattern([s >> m & 1 for m in range(4)])
            # the complement: the same faces the other way round
            turned = {tuple(reversed(f)) for f in oracle_faces_of(t, 15 - s)}
            rotations = (lambda f: {f, f[1:] + f[:1], f[2:] + f[:2]})
            assert all(rotations(f) & turned for f in faces) and len(turned) == len(faces)
    # the six tetrahedra tile the cell: each of the 19 edges of the triangulation from its lower corner, 7 directions
    edges = {(p[m], p[n]) for t in range(6) for p in [corners_of(t)] for m in range(4) for n in range(m + 1, 4)}
    assert len(edges) == 19 and all(a & b == a for a, b in edges)


def test_oracle_sphere_is_a_closed_manifold():
    tsdf, weight, centre = sphere_volume()
    origin, voxel_size = (-1.0, 0.5, 2.0), 0.05
    mesh = oracle_mesh(tsdf, weight, origin, voxel_size)
    vertices, edges, faces = check_closed_sphere(mesh.index, mesh.points, mesh.faces, centre, origin, voxel_size)
    assert vertices > 1500 and faces == 2 * vertices - 4 and (np.diff(mesh.index) > 0).all() and (np.diff(mesh.keys) >= 0).all()
    # the vertices lie on the sphere to within the sampling: a voxel's diagonal at most
    radius = np.linalg.norm(mesh.points - (np.asarray(origin) + voxel_size * centre), axis=1) / voxel_size
    assert np.abs(radius - 6.4).max() < 0.2
    # where every stencil is whole the normals look outward as well
    has = ~np.isnan(mesh.normals).any(axis=1)
    outward = mesh.points - (np.asarray(origin) + voxel_size * centre)
    assert has.all() and ((mesh.normals * outward).sum(axis=1) > 0).all()


def kuhn_tetrahedra_around(triangle, dims):
    """Every tetrahedron (its four voxels as (i, j, k)) of the triangulation, inside the volume, that contains the three
    voxels of `triangle`."""
    nx, ny, nz = dims
    low = np.min(triangle, axis=0)
    found = []
    for shift in itertools.product((0, -1), repeat=3):
        base = low + np.array(shift)
        if (base < 0).any() or (base + 1 >= np.array([nx, ny, nz])).any():
            continue
        for t in range(6):
            voxels = {tuple(base + np.array(offset_of(c))) for c in corners_of(t)}
            if all(tuple(v) in voxels for v in triangle):
                found.append(sorted(voxels))
    return found


def check_open_edges_border_the_unobserved(index, faces, observed):
    """Every mesh edge that lies in one face only lies in a face of the triangulation whose other tetrahedron has an
    unobserved corner (and therefore no faces).  observed bool [nz, ny, nx].  -> the number of such edges."""
    nz, ny, nx = observed.shape
    open_edges, repeated, _, _ = mesh_topology(faces)
    assert repeated == 0
    for u, w in open_edges:
        ends = set()
        for vertex in (u, w):
            v, d = int(index[vertex]) // 7, int(index[vertex]) % 7 + 1
            i, j, k = v % nx, v // nx % ny, v // (nx * ny)
            ends.add((i, j, k))
            ends.add(tuple(np.array([i, j, k]) + np.array(offset_of(d))))
        assert len(ends) == 3, (u, w)   # two edges of one triangle
        around = kuhn_tetrahedra_around(np.array(sorted(ends)), (nx, ny, nz))
        assert 1 <= len(around) <= 2
        blind = [tet for tet in around if not all(observed[k, j, i] for i, j, k in tet)]
        assert len(blind) >= 1, (u, w)
    return len(open_edges)


def test_oracle_sphere_with_an_unobserved_block():
    tsdf, weight, centre = sphere_volume()
    weight[2:6, 8:12, 8:12] = 0.0   # cuts the sphere's lower pole (k = 3.3)
    mesh = oracle_mesh(tsdf, weight, (0.0, 0.0, 0.0), 1.0)
    whole = oracle_mesh(tsdf, np.ones_like(weight), (0.0, 0.0, 0.0), 1.0)
    assert 0 < len(mesh.faces) < len(whole.faces) and len(mesh.index) < len(whole.index)
    assert check_open_edges_border_the_unobserved(mesh.index, mesh.faces, weight >= 1.0) >= 8
    # vertices on the rim may be unreferenced; none elsewhere
    assert len(np.unique(mesh.faces)) <= len(mesh.index)


def pattern_volume(pattern, seed=0):
    """A (2, 2, 2) volume, every voxel observed, whose corner m is negative iff bit m of `pattern` is set, with values of
    varied magnitude."""
    rng = np.random.RandomState(1000 * seed + pattern)
    magnitude = rng.choice(np.array([1.0, 0.75, 0.3, 1e-3, 0.0625, 2e-6], dtype=np.float32), 8)
    sign = np.array([-1.0 if pattern >> m & 1 else 1.0 for m in range(8)], dtype=np.float32)
    return (sign * magnitude).reshape(2, 2, 2), np.ones((2, 2, 2), dtype=np.float32)


def test_oracle_all_256_patterns_of_one_cell():
    canonical = (lambda faces: sorted(min(f[r:] + f[:r] for r in range(3)) for f in map(tuple, faces.tolist())))
    for pattern in range(256):
        tsdf, weight = pattern_volume(pattern)
        mesh = oracle_mesh(tsdf, weight, (0.0, 0.0, 0.0), 1.0)
        expected = sum(faces_per_pattern([pattern >> c & 1 for c in corners_of(t)]) for t in range(6))
        assert len(mesh.faces) == expected, pattern
        crossings = sum(1 for m in range(8) for d in range(1, 8) if m & d == 0 and (pattern >> m & 1) != (pattern >> (m | d) & 1))
        assert len(mesh.index) == crossings, pattern
        other = oracle_mesh(-tsdf, weight, (0.0, 0.0, 0.0), 1.0)
        assert np.array_equal(other.index, mesh.index)
        assert canonical(other.faces[:, ::-1]) == canonical(mesh.faces), pattern
        if 0 < pattern < 255:
            # every crossing is an edge of some tetrahedron of the cell: no vertex is left over, no edge used twice one way
            _, repeated, _, referenced = mesh_topology(mesh.faces)
            assert repeated == 0 and referenced == len(mesh.index), pattern
