"""TSDF fusion: disparity maps of a moving rig integrated into one volume, and the volume's surface (not in the reference).

Everything else behind the network works on one frame, and stereo depth noise grows with Z^2.  The remedy is to fuse the
frames into one model (KinectFusion, Open3D ``TSDFVolume.integrate`` / ``extract_point_cloud``): ``TsdfVolume`` is a
dense, bounded truncated-signed-distance volume on the GPU with two operations.

The volume: ``tsdf`` and ``weight``, float32 [nz, ny, nx], x fastest, 1.0 and 0.0 at the start.  Voxel (i, j, k) has its
centre at ``origin + voxel_size * (i + 0.5, j + 0.5, k + 0.5)`` in the world frame.

``integrate`` (``pds_tsdf_integrate_fwd``).  The host folds the pose ``[R | t]`` (world -> the frame ``matrix`` produces)
into ``A = voxel_size R`` and ``b = R (origin + voxel_size / 2) + t`` in fp64 and rounds them once to float32.  Per batch
entry, in order b = 0 .. B - 1, two launches: the first writes per source pixel the Z ``reproject`` gives (the same device
function, so the same pixels are kept: d finite and d > 0, W > 0, ``valid``, ``confidence >= min_confidence``), NaN where
the pixel is dropped or Z is not finite and positive; the second runs per voxel, in fp32:

    1. p_c = A (i, j, k) + b; skipped unless z_c > 0
    2. x = x_c / z_c, y = y_c / z_c, u = fx x + skew y + cx, v = fy y + cy; skipped unless both are finite
    3. px = floor(u + 0.5), py = floor(v + 0.5)                    (the rounding of ``register_depth``, ``splat=1``)
    4. skipped outside [0, W) x [0, H) or where the stored Z is NaN
    5. sdf = Z - z_c; skipped where sdf < -truncation
    6. t = min(1, sdf / truncation)
    7. w = 1, or with ``weight_by_confidence`` the pixel's confidence; skipped unless w > 0
    8. tsdf = (tsdf * W_old + t * w) / (W_old + w)
    9. weight = min(W_old + w, max_weight)

A skipped voxel is neither read nor written.  No atomics: the same bits on every run and stream.

``extract_points`` (``pds_tsdf_extract_fwd``).  A voxel is observed when its weight is at least ``min_weight``.  For voxel
v = (k * ny + j) * nx + i and axis a = 0, 1, 2 (+x, +y, +z) with n the neighbour along a: if n lies inside the volume, both
are observed and ``(tsdf[v] < 0) != (tsdf[n] < 0)``, there is a surface point at ``origin + voxel_size * ((i, j, k) + 0.5 +
r e_a)`` with ``r = tsdf[v] / (tsdf[v] - tsdf[n])`` and ``index = 3 v + a``; the points come in ascending index.  Its normal
is the normalised ``(1 - r) g(v) + r g(n)`` of the central differences ``g(c)_m = tsdf[c + e_m] - tsdf[c - e_m]``; the tsdf
is positive towards the camera, so the normal faces the viewer.  It is (NaN, NaN, NaN) where one of the twelve stencil
voxels is outside or unobserved or the gradient is zero; the point stays.  The decisions are exact on the stored bits.

``extract_mesh`` (``pds_tsdf_mesh_fwd``).  The same surface as a closed triangle mesh, by marching tetrahedra on the Kuhn
triangulation of each cell: sixteen sign cases per tetrahedron instead of a 256-case table, and closed by construction,
because neighbouring cells agree on the diagonal of every shared face.

    edges      a direction d = 1 .. 7 is a bit mask with ``offset(d) = (d & 1, (d >> 1) & 1, (d >> 2) & 1)``: 1, 2, 4 the
               axes, 3, 5, 6 the face diagonals, 7 the body diagonal.  The edge (v, d) joins voxel v to
               ``n = v + offset(d)`` where n lies inside the volume.
    vertices   an edge carries a vertex iff both ends are observed and ``(tsdf[v] < 0) != (tsdf[n] < 0)``:
               ``r = tsdf[v] / (tsdf[v] - tsdf[n])``, the point ``origin + voxel_size * ((i, j, k) + 0.5 + r offset(d))``,
               ``index = 7 v + (d - 1)``, in ascending index; the normal is the normalised ``(1 - r) g(v) + r g(n)`` with
               the same g and the same NaN rule as above.  For d = 1, 2, 4 point and normal are those of
               ``extract_points`` for a = 0, 1, 2, bit for bit.  A vertex is emitted whether or not a face uses it: on the
               rim of the observed region vertices may be unreferenced.
    cells      cell c has voxel c as its corner 0 (i < nx - 1, j < ny - 1, k < nz - 1), corner m = 0 .. 7 at
               ``offset(m)``.  Tetrahedron t = 0 .. 5 belongs to the axis permutation (a, b, e) in lexicographic order,
               (0,1,2) (0,2,1) (1,0,2) (1,2,0) (2,0,1) (2,1,0): corners ``p0 = 0``, ``p1 = 1 << a``, ``p2 = p1 | 1 << b``,
               ``p3 = 7``.  Its edge (pm, pn), m < n, is the edge (voxel of pm, d = pn ^ pm).
    faces      a tetrahedron emits faces iff its four corners are observed.  One corner A alone on its side of zero (the
               others B < C < D by position): the triangle (AB, AC, AD).  Two against two (the negative pair A < B, the
               others C < D): (AC, AD, BD) then (AC, BD, BC).  All alike: nothing.
    winding    by the right-hand rule the face normal points from the negative corners towards the positive ones, towards
               the viewer, like the normals; otherwise the second and third vertex are swapped.  Decided as if every
               vertex sat at its edge's midpoint: a function of (t, signs) alone, never a floating-point test.
    order      faces by 6 c + t, within a tetrahedron as listed; ``faces`` [F, 3] int32 rows of ``points``, the true rows
               even when the vertices were cut at ``capacity``.

A volume with a dimension of 1 has vertices and no faces.  Every decision is exact on the stored bits; no atomics: the
same bits on every run and stream.  Volumes with 7 * nx * ny * nz or 12 * cells above 2^31 - 1 are refused.

``raycast`` (``pds_tsdf_raycast_fwd``): raycasting the volume into a camera, as a depth map and a normal map, lives in
``tsdf_raycast.py`` with its contract; ``rays`` returns the fp64 rows it folds the pose into.

``track`` (``pds_icp_system_fwd``): pose estimation, the pose of a new frame by point-to-plane ICP against the raycast at
a predicted pose, lives in ``tracking.py`` with its contract.

``ColorTsdfVolume`` in ``tsdf_color.py`` fuses the image as well and colours the extracted surface and the raycast.

``shift`` / ``follow`` (``pds_tsdf_shift_fwd``, ``pds_tsdf_extract_leaving_fwd``): the rolling volume of Kintinuous.  The
box is fixed in size, not in place: ``shift((dx, dy, dz))`` moves it by whole voxels so that it can follow the rig.

    state      into fresh tensors, in one launch: new voxel (i, j, k) = old voxel (i + dx, j + dy, k + dz) where that lies
               inside the volume, and the empty state (tsdf 1.0, weight 0.0, colour 0.0) elsewhere.  Bit copies: a shift
               is exact, and shifts compose on the voxels that stay through all of them.  Any delta is legal; with
               ``|d_a| >= n_a`` on an axis the whole volume is empty afterwards.
    origin     the volume keeps ``origin0`` (what it was built with) and ``offset``, three Python ints that start at 0
               and to which every shift adds its delta; ``origin`` is ``origin0 + voxel_size * offset``, evaluated in
               fp64 from the integers, so a thousand shifts round once and a volume that never shifts has the ``origin``
               it was given, bit for bit.  Every other operation reads ``origin``, so it works on the shifted volume as
               on a fresh one built there.  ``reset()`` empties the state and leaves ``offset`` alone.
    leaving    with ``leaving=True`` the surface about to be lost is extracted first, against the old state: old voxel
               (i, j, k) lands inside the new volume iff ``0 <= (i, j, k) - delta < dims``; the edge from v to its
               neighbour n survives iff both land inside, otherwise it leaves.  The result holds exactly the rows of
               ``extract_points`` whose edge leaves, with the same bits, in world coordinates, ``index = 3 v + a`` in
               the old numbering, ascending.  ``extract_points`` after the shift gives the others, their index lower by
               ``3 ((dz ny + dy) nx + dx)`` (for ``min_weight > 0``: an entering voxel has weight 0).  Every edge of a
               surface that is integrated once is thus handed out exactly once: in a leaving cloud, or at the end.
    follow     ``follow_delta(pose)`` is host arithmetic: with the camera centre ``c = -R^T t`` the target is
               ``((c - origin) / voxel_size - anchor * dims) / step`` and ``delta_a = step * trunc(target_a)``, towards
               zero: ``anchor`` is where in the box the camera should sit, as a fraction per axis (a forward-looking rig
               wants z near 0), ``step`` the granularity and the hysteresis in voxels (a multiple of 4 keeps the aligned
               form of the kernel).  ``follow(pose)`` is ``shift(follow_delta(pose))``.

No host synchronisation except the one of ``trim=True``; no atomics: the same bits on every run and stream.

Out of scope: marching-cubes faces (the mesh is marching tetrahedra), colour, depth-dependent truncation or weights,
hashed or sparse volumes, mesh simplification, welding of vertices across exact zeros, in-place shifting, ring-buffer
addressing, a leaving *mesh*.
There is no CPU fallback.
"""
import collections
import ctypes
import math
import operator

import numpy as np
import torch

from practicaldeepstereo_nips2018_amd import _lib, tsdf_raycast as _raycast
from practicaldeepstereo_nips2018_amd.point_cloud import PointCloud, _rows

# cloud: PointCloud(points [N, 3], None, index [N] = 3 v + a, offsets [0, N]); normals [N, 3] float32 or None
SurfacePoints = collections.namedtuple('SurfacePoints', ['cloud', 'normals'])
# mesh: TriangleMesh(points [N, 3], None, index [N] = 7 v + (d - 1), offsets [0, N], faces [F, 3], face_offsets [0, F]);
# normals [N, 3] float32 or None
SurfaceMesh = collections.namedtuple('SurfaceMesh', ['mesh', 'normals'])

# what integrate hands to its entry point: the tensors on the GPU, the host arrays as ctypes, the shape
_Frames = collections.namedtuple('_Frames', ['disparity', 'valid', 'confidence', 'min_confidence', 'matrix', 'transforms',
                                             'camera', 'batch', 'height', 'width'])

_Float3 = ctypes.c_float * 3
_Float5 = ctypes.c_float * 5
_Float16 = ctypes.c_float * 16

_workspace = _lib.Workspace()


def _positive(value, name):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise TypeError('%s must be a number, got %r' % (name, value))
    if not value > 0.0:
        raise ValueError('%s must be positive, got %r' % (name, value))
    return value


def camera_of_matrix(matrix):
    """``(fx, fy, cx, cy, skew)`` of the frame a reprojection matrix of the canonical rectified form produces:
    ``[[1, 0, 0, -cx], [0, 1, 0, -cy], [0, 0, 0, f], [0, 0, a, b]]`` gives ``(f, f, cx, cy, 0)``."""
    m = np.asarray(matrix, dtype=np.float64)
    if m.shape != (4, 4) or not np.all(np.isfinite(m)):
        raise ValueError('matrix must be a finite 4x4, got shape %s' % (m.shape,))
    canonical = (m[0, 0] == 1 and m[1, 1] == 1 and m[0, 1] == 0 and m[0, 2] == 0 and m[1, 0] == 0 and m[1, 2] == 0 and
                 np.all(m[2, :3] == 0) and m[2, 3] > 0 and m[3, 0] == 0 and m[3, 1] == 0)
    if not canonical:
        raise ValueError('camera=None needs a matrix of the canonical rectified form [[1, 0, 0, -cx], [0, 1, 0, -cy], '
                         '[0, 0, 0, f], [0, 0, a, b]]: pass camera=(fx, fy, cx, cy, skew) of the frame this matrix produces')
    return (m[2, 3], m[2, 3], -m[0, 3], -m[1, 3], 0.0)


class TsdfVolume(object):
    """``TsdfVolume(origin, voxel_size, dims, truncation, max_weight=64.0, device='cuda')``: see the module text.
    ``dims = (nx, ny, nz)``.  ``tsdf`` and ``weight`` (float32 [nz, ny, nx]) are public and may be set to contiguous
    tensors of the same shape, dtype and device; ``reset()`` restores 1.0 and 0.0."""

    def __init__(self, origin, voxel_size, dims, truncation, max_weight=64.0, device='cuda'):
        try:
            origin = np.asarray(origin, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise TypeError('origin must be three numbers, got %r' % (origin,))
        if origin.size != 3 or not np.all(np.isfinite(origin)):
            raise ValueError('origin must hold 3 finite values, got %r' % (origin.tolist(),))
        self.origin0 = origin
        self.offset = (0, 0, 0)
        self.voxel_size = _positive(voxel_size, 'voxel_size')
        self.truncation = _positive(truncation, 'truncation')
        self.max_weight = _positive(max_weight, 'max_weight')
        if not (math.isfinite(self.voxel_size) and math.isfinite(self.truncation)):
            raise ValueError('voxel_size and truncation must be finite')
        try:
            nx, ny, nz = (operator.index(v) for v in dims)
        except (TypeError, ValueError):
            raise ValueError('dims must be three integers (nx, ny, nz), got %r' % (dims,))
        if nx < 1 or ny < 1 or nz < 1:
            raise ValueError('dims must be at least (1, 1, 1), got %r' % (dims,))
        if max(nx, ny, nz) > 2 ** 24:
            raise ValueError('dims must be at most 2^24 each (a voxel index is an exact float32), got %r' % (dims,))
        if 3 * nx * ny * nz > 2 ** 31 - 1:
            raise ValueError('3 * nx * ny * nz = %d does not fit 32-bit indices' % (3 * nx * ny * nz))
        self.dims = (nx, ny, nz)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('a TsdfVolume lives on an MI355X (cuda) device: the HIP path has no CPU fallback')
        self._tsdf = self._weight = None
        self.reset()

    @property
    def shape(self):
        nx, ny, nz = self.dims
        return (nz, ny, nx)

    @property
    def origin(self):
        """``origin0 + voxel_size * offset`` in fp64, from the integers: exact however many shifts led here, and
        ``origin0`` itself, bit for bit, on an axis that never moved.  Setting it anchors the volume anew: ``origin0``
        becomes the value and ``offset`` zero."""
        moved = self.origin0 + self.voxel_size * np.array(self.offset, dtype=np.float64)
        return np.where(np.array(self.offset) == 0, self.origin0, moved)   # (-0.0 + 0.0 would lose its sign)

    @origin.setter
    def origin(self, value):
        value = np.asarray(value, dtype=np.float64).reshape(-1)
        if value.size != 3 or not np.all(np.isfinite(value)):
            raise ValueError('origin must hold 3 finite values, got %r' % (value.tolist(),))
        self.origin0, self.offset = value, (0, 0, 0)

    def reset(self):
        """1.0 and 0.0 everywhere, in fresh tensors; ``offset`` stays: the box is emptied where it stands."""
        self._tsdf = torch.ones(self.shape, dtype=torch.float32, device=self.device)
        self._weight = torch.zeros(self.shape, dtype=torch.float32, device=self.device)
        self.device = self._tsdf.device
        return self

    def _state(self, t, name):
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s must be a torch.Tensor' % name)
        if t.dtype != torch.float32 or tuple(t.shape) != self.shape:
            raise ValueError('%s must be float32 %s, got %s %s' % (name, self.shape, t.dtype, tuple(t.shape)))
        if t.device != self.device:
            raise ValueError('%s must live on %s, got %s' % (name, self.device, t.device))
        if not t.is_contiguous():
            raise ValueError('%s must be contiguous' % name)
        return t.detach()

    tsdf = property(lambda self: self._tsdf, lambda self, t: setattr(self, '_tsdf', self._state(t, 'tsdf')))
    weight = property(lambda self: self._weight, lambda self, t: setattr(self, '_weight', self._state(t, 'weight')))

    def transforms(self, pose, batch):
        """The [batch, 12] fp64 rows ``A`` (9, row-major) and ``b`` (3) of ``integrate`` for ``pose``: 3x4 ``[R | t]`` for
        every entry, [batch, 3, 4], or None (the identity)."""
        if pose is None:
            pose = np.hstack([np.eye(3), np.zeros((3, 1))])
        try:
            pose = np.asarray(pose, dtype=np.float64)
        except (TypeError, ValueError):
            raise TypeError('pose must be an array of numbers')
        if pose.shape == (3, 4):
            pose = np.broadcast_to(pose, (batch, 3, 4))
        if pose.shape != (batch, 3, 4) or not np.all(np.isfinite(pose)):
            raise ValueError('pose must be a finite 3x4 [R | t] or [%d, 3, 4], got shape %s' % (batch, pose.shape))
        rows = np.empty((batch, 12))
        for b in range(batch):
            R, t = pose[b, :, :3], pose[b, :, 3]
            rows[b, :9] = (self.voxel_size * R).reshape(-1)
            rows[b, 9:] = R @ (self.origin + 0.5 * self.voxel_size) + t
        return rows

    def integrate(self, disparity, matrix, pose=None, camera=None, valid=None, confidence=None, min_confidence=0.0,
                  weight_by_confidence=False):
        """Integrates disparity float32 [B, H, W] into the volume, entry after entry (see the module text) -> self.

        ``matrix``: the 4x4 of ``reproject``.  ``pose``: 3x4 ``[R | t]`` or [B, 3, 4], from the world frame into the
        frame ``matrix`` produces (None: the identity).  ``camera``: ``(fx, fy, cx, cy, skew)``, the pinhole of that
        frame; None reads it off a matrix of the canonical rectified form (``camera_of_matrix``).  ``valid`` /
        ``confidence`` / ``min_confidence``: as ``reproject`` takes them.  ``weight_by_confidence``: a pixel counts with
        its confidence instead of 1.  Runs on the current stream, without autograd and without any synchronisation."""
        a = self._integrate_arguments(disparity, matrix, pose, camera, valid, confidence, min_confidence,
                                      weight_by_confidence)
        nx, ny, nz = self.dims
        lib = _lib.load()
        nbytes = int(lib.pds_tsdf_integrate_workspace_bytes(a.height, a.width))
        if nbytes == 0:
            raise ValueError('integrate: %s' % lib.pds_last_error().decode(errors='replace'))
        with torch.cuda.device(self.device):
            workspace = _workspace.get(nbytes, self.device)
            _lib.check(lib.pds_tsdf_integrate_fwd(
                _lib.ptr(a.disparity), None if a.valid is None else _lib.ptr(a.valid),
                None if a.confidence is None else _lib.ptr(a.confidence), a.min_confidence,
                int(bool(weight_by_confidence)), a.matrix, a.transforms, a.camera, self.truncation, self.max_weight,
                _lib.ptr(self._tsdf), _lib.ptr(self._weight), nx, ny, nz, a.batch, a.height, a.width,
                _lib.ptr(workspace), workspace.numel(), _lib.stream_handle(self.device)), 'pds_tsdf_integrate_fwd')
        return self

    def _integrate_arguments(self, disparity, matrix, pose, camera, valid, confidence, min_confidence,
                             weight_by_confidence, host_check=None):
        """The checks of ``integrate`` and what the entry point takes -> ``_Frames``.  ``host_check(shape)``: what a
        subclass judges of its own arguments without a GPU (``ColorTsdfVolume``: the image), before any tensor is asked
        where it lives."""
        # what can be judged without a GPU comes first: types, shapes, thresholds
        for name, t in (('disparity', disparity),) + ((('confidence', confidence),) if confidence is not None else ()):
            if not isinstance(t, torch.Tensor):
                raise TypeError('%s must be a torch.Tensor' % name)
            if t.dtype != torch.float32:
                raise TypeError('%s must be float32, got %s' % (name, t.dtype))
            if t.dim() != 3:
                raise ValueError('%s must have 3 dimensions, got %d' % (name, t.dim()))
        shape = tuple(disparity.shape)
        m = np.asarray(matrix, dtype=np.float64)
        if m.shape != (4, 4) or not np.all(np.isfinite(m)):
            raise ValueError('matrix must be a finite 4x4, got shape %s' % (m.shape,))
        if 0 in shape:
            raise ValueError('integrate: empty input %s' % (shape,))
        batch, height, width = shape
        rows = self.transforms(pose, batch)
        if camera is None:
            camera = camera_of_matrix(m)
        try:
            camera = np.asarray(camera, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise TypeError('camera must be a sequence of numbers, got %r' % (camera,))
        if camera.size != 5:
            raise ValueError('camera must hold 5 values (fx, fy, cx, cy, skew), got %d' % camera.size)
        if not np.all(np.isfinite(camera)):
            raise ValueError('camera has non-finite entries: %r' % camera.tolist())
        if not (camera[0] > 0 and camera[1] > 0):
            raise ValueError('camera must have positive focal lengths, got fx = %r, fy = %r' % (camera[0], camera[1]))
        min_confidence = float(min_confidence)
        if not math.isfinite(min_confidence):
            raise ValueError('min_confidence must be finite, got %r' % (min_confidence,))
        if valid is not None:
            if not isinstance(valid, torch.Tensor):
                raise TypeError('valid must be a torch.Tensor')
            if valid.dtype != torch.bool or tuple(valid.shape) != shape:
                raise ValueError('valid must be torch.bool %s, got %s %s' % (shape, valid.dtype, tuple(valid.shape)))
        if confidence is not None and tuple(confidence.shape) != shape:
            raise ValueError('confidence %s and disparity %s differ in shape' % (tuple(confidence.shape), shape))
        if weight_by_confidence and confidence is None:
            raise ValueError('weight_by_confidence needs a confidence')
        if host_check is not None:
            host_check(shape)
        # then where the tensors live
        d = _lib.require_gpu_tensor(disparity.detach(), 'disparity', 3)
        if valid is not None:
            if not valid.is_cuda:
                raise RuntimeError('valid must live on an MI355X (cuda) device: the HIP path has no CPU fallback')
            valid = valid.contiguous()
        if confidence is not None:
            confidence = _lib.require_gpu_tensor(confidence.detach(), 'confidence', 3)
        for name, t in (('disparity', d), ('valid', valid), ('confidence', confidence)):
            if t is not None and t.device != self.device:
                raise ValueError('%s and the volume live on different devices' % name)
        return _Frames(d, valid, confidence, min_confidence, _Float16(*m.astype(np.float32).reshape(-1).tolist()),
                       (ctypes.c_float * (12 * batch))(*rows.astype(np.float32).reshape(-1).tolist()),
                       _Float5(*camera.astype(np.float32).tolist()), batch, height, width)

    def rays(self, pose, batch):
        """The [batch, 21] fp64 rows ``M = R^T / voxel_size`` (9, row-major), ``o = (-R^T t - origin) / voxel_size - 0.5``
        (3) and ``R`` (9) of ``raycast`` for ``pose``: 3x4 ``[R | t]`` for every entry, [batch, 3, 4], or None (the
        identity).  A point p of the camera frame lies at the grid position M p + o, where voxel (i, j, k) is the point
        (i, j, k)."""
        return _raycast.rays(self, pose, batch)

    def raycast(self, camera, size, pose=None, min_weight=1.0, step=None, near=0.0, far=math.inf, with_normals=True):
        """The volume seen from a pinhole camera -> ``Raycast(depth, normals)`` (see ``tsdf_raycast``): ``depth`` float32
        [B, H, W], the camera-frame Z along the ray of each pixel centre, NaN where there is no surface; ``normals``
        float32 [B, H, W, 3], unit, in the camera frame, facing the camera, None without ``with_normals``.

        ``camera = (fx, fy, cx, cy, skew)``, ``size = (width, height)``.  ``pose``: 3x4 ``[R | t]`` or [B, 3, 4], world ->
        camera, as ``integrate`` takes it (None: the identity, B = 1).  ``min_weight``: a sample counts where the eight
        voxels around it have at least this weight.  ``step``: the distance between samples in units of Z (None:
        ``truncation / 2``).  ``near`` / ``far``: the range of Z searched.  Runs on the current stream, without autograd,
        workspace or any synchronisation; the volume is read only."""
        return _raycast.raycast(self, camera, size, pose=pose, min_weight=min_weight, step=step, near=near, far=far,
                                with_normals=with_normals)

    def track(self, disparity, matrix, pose, camera=None, size=None, iterations=10, max_distance=None, min_cosine=0.5,
              normals=None, valid=None, confidence=None, min_confidence=0.0, min_weight=1.0, min_count=100,
              min_eigenvalue=1e-4, tolerance=1e-6):
        """The pose of a new frame by point-to-plane ICP against the model -> ``Tracking(pose, rmse, inliers, iterations,
        status)`` (see ``tracking``): ``pose`` float64 [B, 3, 4], world -> frame, as ``integrate`` takes it.

        ``disparity`` / ``matrix`` / ``valid`` / ``confidence`` / ``min_confidence``: the frame, as ``integrate`` takes
        it.  ``pose``: the predicted pose, 3x4 or [B, 3, 4], world -> frame (e.g. the pose of the frame before); the
        volume is raycast once there, through ``camera`` (None: ``camera_of_matrix(matrix)``) at ``size = (width, height)``
        (None: the frame's), with ``min_weight``.  ``iterations``: at most so many rounds of ``icp_system`` -> one host
        read of 29 B doubles -> ``icp_solve`` -> T <- exp(xi) T; it stops early when |xi| falls below ``tolerance``.
        ``max_distance``: a pixel counts within this distance of its model point (None: 2 * truncation).  ``normals``:
        the frame's normals (``surface_normals``), compared with the model's through ``min_cosine``.  An entry with fewer
        than ``min_count`` rows, or whose smallest eigenvalue of A / count is below ``min_eigenvalue``, keeps its predicted
        pose and says so in ``status`` (``tracking.TOO_FEW_ROWS``, ``tracking.DEGENERATE``); nothing raises for it.

        ``track_pyramid`` is this loop coarse to fine and with Huber weights."""
        from practicaldeepstereo_nips2018_amd import tracking
        return tracking.track(self, disparity, matrix, pose, camera=camera, size=size, iterations=iterations,
                              max_distance=max_distance, min_cosine=min_cosine, normals=normals, valid=valid,
                              confidence=confidence, min_confidence=min_confidence, min_weight=min_weight,
                              min_count=min_count, min_eigenvalue=min_eigenvalue, tolerance=tolerance)

    def track_pyramid(self, disparity, matrix, pose, levels=3, huber=None, max_difference=None, **kw):
        """``track`` coarse to fine on a disparity pyramid and with Huber weights -> ``Tracking`` (see ``tracking``).
        ``kw``: the other keywords of ``track``.  ``levels=1, huber=None`` is ``track`` itself, byte for byte.

        ``levels`` > 1 tracks coarse to fine on ``disparity_pyramid(disparity, levels, max_difference, ...)`` against one
        raycast per level (``pyramid_camera``, ``size >> level``), levels ``levels - 1`` .. 0, the transform carried from
        level to level; ``iterations`` and ``max_distance`` may then hold one value per level, indexed by level.
        ``valid``, ``confidence`` and ``normals`` apply at level 0.  An entry refused above level 0 keeps its transform
        and goes on at the next level; ``status``, ``rmse`` and ``inliers`` are those of the last level-0 system and
        ``Tracking.iterations`` is the total.  ``max_difference`` (None: ``tracking.DEFAULT_MAX_DIFFERENCE``, one
        disparity step) is the pyramid's.  ``huber``: the threshold, in metres of point-to-plane distance, beyond which
        a residual's weight falls as huber / |r| (``icp_system_robust``); None: unweighted.  A frame that cannot be tracked
        says so in ``status``, as in ``track``."""
        from practicaldeepstereo_nips2018_amd import tracking
        return tracking.track(self, disparity, matrix, pose, levels=levels, huber=huber, max_difference=max_difference, **kw)

    def extract_points(self, min_weight=1.0, with_normals=True, capacity=None, trim=True):
        """The zero crossings of the volume -> ``SurfacePoints(cloud, normals)`` (see the module text): ``cloud`` is a
        ``PointCloud`` with ``colors=None``, ``index = 3 v + a`` and ``offsets = [0, N]``, so that ``save_ply(path, cloud,
        normals=normals)`` works as it is; ``normals`` float32 [N, 3], None without ``with_normals``.

        ``capacity``: rows of the output buffers; None means 3 * nx * ny * nz, which can never overflow (and is large:
        give one).  ``trim=True`` reads ``offsets`` once on the host -- the ONLY synchronisation of the call -- and returns
        tensors of exactly N rows; it raises if an explicit ``capacity`` was smaller than N.  ``trim=False`` returns the
        full-capacity buffers without any synchronisation; ``offsets[1]`` is the true count even beyond ``capacity``."""
        min_weight, rows = self._extract_arguments(min_weight, capacity)
        found = self._extract(min_weight, with_normals, rows, None)
        return _trimmed_points(found) if trim else found

    def _extract_arguments(self, min_weight, capacity):
        """What ``extract_points`` and ``shift(leaving=True)`` judge without a GPU -> (min_weight, rows)."""
        min_weight = float(min_weight)
        if math.isnan(min_weight):
            raise ValueError('min_weight is NaN')
        nx, ny, nz = self.dims
        return min_weight, _rows(capacity, 'capacity', 3 * nx * ny * nz)

    def _extract(self, min_weight, with_normals, rows, leaving):
        """The zero crossings (``leaving`` None: ``pds_tsdf_extract_fwd``), or of them those that a shift by ``leaving``
        loses (``pds_tsdf_extract_leaving_fwd``) -> untrimmed ``SurfacePoints`` of ``rows`` rows; no synchronisation."""
        nx, ny, nz = self.dims
        if not (self._tsdf.is_cuda and self._weight.is_cuda):
            raise RuntimeError('the volume must live on an MI355X (cuda) device: the HIP path has no CPU fallback')
        lib = _lib.load()
        nbytes = int(lib.pds_tsdf_extract_workspace_bytes(nx, ny, nz))
        if nbytes == 0:
            raise ValueError('extract_points: %s' % lib.pds_last_error().decode(errors='replace'))
        held = max(rows, 1)   # (a buffer of no rows has no address)
        points = torch.empty((held, 3), dtype=torch.float32, device=self.device)
        normals = torch.empty((held, 3), dtype=torch.float32, device=self.device) if with_normals else None
        index = torch.empty((held,), dtype=torch.int32, device=self.device)
        offsets = torch.empty((2,), dtype=torch.int32, device=self.device)
        c_origin = _Float3(*self.origin.astype(np.float32).tolist())
        with torch.cuda.device(self.device):
            workspace = _workspace.get(nbytes, self.device)
            if leaving is None:
                _lib.check(lib.pds_tsdf_extract_fwd(
                    _lib.ptr(self._tsdf), _lib.ptr(self._weight), c_origin, self.voxel_size, min_weight, _lib.ptr(points),
                    None if normals is None else _lib.ptr(normals), _lib.ptr(index), _lib.ptr(offsets), rows, nx, ny, nz,
                    _lib.ptr(workspace), workspace.numel(), _lib.stream_handle(self.device)), 'pds_tsdf_extract_fwd')
            else:
                _lib.check(lib.pds_tsdf_extract_leaving_fwd(
                    _lib.ptr(self._tsdf), _lib.ptr(self._weight), c_origin, self.voxel_size, min_weight, _lib.ptr(points),
                    None if normals is None else _lib.ptr(normals), _lib.ptr(index), _lib.ptr(offsets), rows, nx, ny, nz,
                    leaving[0], leaving[1], leaving[2], _lib.ptr(workspace), workspace.numel(),
                    _lib.stream_handle(self.device)), 'pds_tsdf_extract_leaving_fwd')
        cut = (lambda t: None if t is None else t[:rows])
        return SurfacePoints(PointCloud(cut(points), None, cut(index), offsets), cut(normals))

    # ------------------------------------------------------------------------------------------ the rolling volume
    def shift(self, delta, leaving=False, min_weight=1.0, with_normals=True, capacity=None, trim=True):
        """Moves the box by ``delta = (dx, dy, dz)`` whole voxels (see the module text) -> ``SurfacePoints`` with
        ``leaving``, else None.

        New voxel (i, j, k) holds what old voxel (i + dx, j + dy, k + dz) held, the empty state where there was none;
        the state goes into fresh tensors (one launch), ``offset`` advances by ``delta`` and ``origin`` with it.
        ``leaving=True`` first extracts, against the old state, the surface whose edges do not survive: a
        ``SurfacePoints`` as ``extract_points`` returns it, in world coordinates, ``index`` in the old numbering;
        ``min_weight``, ``with_normals``, ``capacity`` and ``trim`` are those of ``extract_points`` and are read only
        then; a ``capacity`` that ``trim=True`` finds too small raises before anything has moved.  ``delta == (0, 0, 0)``
        launches nothing and returns an empty result.  Runs on the current stream, without autograd; no synchronisation
        but the one host read of ``trim=True``."""
        return self._shift(delta, leaving, min_weight, with_normals, capacity, trim, False)

    def _shift(self, delta, leaving, min_weight, with_normals, capacity, trim, with_colors):
        delta = _delta(delta)
        if leaving:
            min_weight, rows = self._extract_arguments(min_weight, capacity)
        if delta == (0, 0, 0):
            return self._nothing_leaves(with_normals, with_colors) if leaving else None
        found = self._leaving_surface(delta, min_weight, with_normals, rows, with_colors) if leaving else None
        if leaving and trim:
            found = _trimmed_points(found)   # (the one host read; a capacity that is too small raises before anything moves)
        self._shift_state(delta)
        self.offset = tuple(o + d for o, d in zip(self.offset, delta))
        return found

    def _nothing_leaves(self, with_normals, with_colors):
        """The result of a shift by nothing: no rows, ``offsets = [0, 0]``, and no kernel of the library."""
        empty = (lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device))
        cloud = PointCloud(empty(0, 3), empty(0, 3) if with_colors else None,
                           torch.empty((0,), dtype=torch.int32, device=self.device),
                           torch.zeros((2,), dtype=torch.int32, device=self.device))
        cloud.__dict__['_host_offsets'] = [0, 0]
        return SurfacePoints(cloud, empty(0, 3) if with_normals else None)

    def _leaving_surface(self, delta, min_weight, with_normals, rows, with_colors):
        """The untrimmed leaving surface, against the state as it is (``ColorTsdfVolume`` colours it here)."""
        return self._extract(min_weight, with_normals, rows, delta)

    def _state_tensors(self):
        """The tensors a shift moves: tsdf, weight and the colour or None."""
        return self._tsdf, self._weight, None

    def _shift_state(self, delta):
        tsdf, weight, color = self._state_tensors()
        if not (tsdf.is_cuda and weight.is_cuda and (color is None or color.is_cuda)):
            raise RuntimeError('the volume must live on an MI355X (cuda) device: the HIP path has no CPU fallback')
        nx, ny, nz = self.dims
        out = [None if t is None else torch.empty_like(t) for t in (tsdf, weight, color)]
        lib = _lib.load()
        with torch.cuda.device(self.device):
            _lib.check(lib.pds_tsdf_shift_fwd(
                _lib.ptr(tsdf), _lib.ptr(weight), None if color is None else _lib.ptr(color), _lib.ptr(out[0]),
                _lib.ptr(out[1]), None if color is None else _lib.ptr(out[2]), delta[0], delta[1], delta[2], nx, ny, nz,
                _lib.stream_handle(self.device)), 'pds_tsdf_shift_fwd')
        self._tsdf, self._weight = out[0], out[1]
        return out[2]

    def follow_delta(self, pose, anchor=(0.5, 0.5, 0.5), step=8):
        """The shift that brings the camera of ``pose`` (3x4 ``[R | t]``, world -> camera) back to ``anchor`` -> three
        ints, multiples of ``step`` (see the module text); host arithmetic in fp64, no GPU."""
        try:
            pose = np.asarray(pose, dtype=np.float64)
        except (TypeError, ValueError):
            raise TypeError('pose must be an array of numbers')
        if pose.shape != (3, 4) or not np.all(np.isfinite(pose)):
            raise ValueError('pose must be a finite 3x4 [R | t], got shape %s' % (pose.shape,))
        try:
            anchor = np.asarray(anchor, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise TypeError('anchor must be three numbers, got %r' % (anchor,))
        if anchor.size != 3 or not np.all(np.isfinite(anchor)):
            raise ValueError('anchor must hold 3 finite values, got %r' % (anchor.tolist(),))
        try:
            step = operator.index(step)
        except TypeError:
            raise TypeError('step must be an integer, got %r' % (step,))
        if step < 1:
            raise ValueError('step must be at least 1, got %d' % step)
        centre = -pose[:, :3].T @ pose[:, 3]
        target = ((centre - self.origin) / self.voxel_size - anchor * np.array(self.dims, dtype=np.float64)) / step
        return _delta(tuple(step * int(v) for v in np.trunc(target)))

    def follow(self, pose, anchor=(0.5, 0.5, 0.5), step=8, **shift_kw):
        """``shift(follow_delta(pose, anchor, step), **shift_kw)``: the box follows the camera in steps of ``step``
        voxels and hands out what it leaves behind (``leaving=True``)."""
        return self.shift(self.follow_delta(pose, anchor=anchor, step=step), **shift_kw)

    def extract_mesh(self, min_weight=1.0, with_normals=True, capacity=None, face_capacity=None, trim=True):
        """The surface of the volume as a closed triangle mesh -> ``SurfaceMesh(mesh, normals)`` (see the module text):
        ``mesh`` is a ``TriangleMesh`` with ``colors=None``, ``index = 7 v + (d - 1)``, ``offsets = [0, N]`` and
        ``face_offsets = [0, F]``, so that ``mesh.save_ply(path, normals=normals)``, ``mesh.cloud()``, ``mesh.entry(0)``
        and ``mesh.face_count()`` work as they are; ``normals`` float32 [N, 3], None without ``with_normals``.

        ``capacity``: rows of the vertex buffers; None means 7 * nx * ny * nz.  ``face_capacity``: rows of ``faces``;
        None means 12 * (nx - 1) * (ny - 1) * (nz - 1).  Neither default can overflow, and both are large (28 and 12
        bytes per row: gigabytes for a 256^3 volume): give both.  ``trim=True`` reads both counts in one host read -- the
        ONLY synchronisation of the call -- and returns tensors of exactly N and F rows; it raises if an explicit capacity
        was too small.  ``trim=False`` returns the full-capacity buffers without any synchronisation; ``offsets[1]`` and
        ``face_offsets[1]`` are the true counts even beyond the capacities, and ``faces`` holds the true rows even when
        the vertices were cut.  Runs on the current stream, without autograd; the volume is read only."""
        from practicaldeepstereo_nips2018_amd.mesh import TriangleMesh   # (mesh.py imports point_cloud, as this module)
        min_weight = float(min_weight)
        if math.isnan(min_weight):
            raise ValueError('min_weight is NaN')
        nx, ny, nz = self.dims
        cells = (nx - 1) * (ny - 1) * (nz - 1)
        rows = _rows(capacity, 'capacity', 7 * nx * ny * nz)
        face_rows = _rows(face_capacity, 'face_capacity', 12 * cells)
        if 7 * nx * ny * nz > 2 ** 31 - 1:
            raise ValueError('extract_mesh: 7 * nx * ny * nz = %d does not fit 32-bit indices' % (7 * nx * ny * nz))
        if 12 * cells > 2 ** 31 - 1:
            raise ValueError('extract_mesh: 12 * cells = %d does not fit 32-bit indices' % (12 * cells))
        if not (self._tsdf.is_cuda and self._weight.is_cuda):
            raise RuntimeError('the volume must live on an MI355X (cuda) device: the HIP path has no CPU fallback')
        lib = _lib.load()
        nbytes = int(lib.pds_tsdf_mesh_workspace_bytes(nx, ny, nz))
        if nbytes == 0:
            raise ValueError('extract_mesh: %s' % lib.pds_last_error().decode(errors='replace'))
        held, face_held = max(rows, 1), max(face_rows, 1)   # (a buffer of no rows has no address)
        points = torch.empty((held, 3), dtype=torch.float32, device=self.device)
        normals = torch.empty((held, 3), dtype=torch.float32, device=self.device) if with_normals else None
        index = torch.empty((held,), dtype=torch.int32, device=self.device)
        faces = torch.empty((face_held, 3), dtype=torch.int32, device=self.device)
        both = torch.empty((2, 2), dtype=torch.int32, device=self.device)   # offsets, face_offsets: one host read
        c_origin = _Float3(*self.origin.astype(np.float32).tolist())
        with torch.cuda.device(self.device):
            workspace = _workspace.get(nbytes, self.device)
            _lib.check(lib.pds_tsdf_mesh_fwd(
                _lib.ptr(self._tsdf), _lib.ptr(self._weight), c_origin, self.voxel_size, min_weight, _lib.ptr(points),
                None if normals is None else _lib.ptr(normals), _lib.ptr(index), _lib.ptr(both[0]), rows,
                _lib.ptr(faces), _lib.ptr(both[1]), face_rows, nx, ny, nz, _lib.ptr(workspace), workspace.numel(),
                _lib.stream_handle(self.device)), 'pds_tsdf_mesh_fwd')
        cut = (lambda t, n: None if t is None else t[:n])
        mesh = TriangleMesh(cut(points, rows), None, cut(index, rows), both[0], cut(faces, face_rows), both[1])
        mesh.__dict__['_both'] = both
        found = SurfaceMesh(mesh, cut(normals, rows))
        return _trimmed_mesh(found) if trim else found


def _delta(delta):
    """``delta`` of ``shift`` -> three Python ints, each at most 2^24 in size."""
    try:
        delta = tuple(operator.index(v) for v in delta)
    except TypeError:
        raise TypeError('delta must be three integers (dx, dy, dz), got %r' % (delta,))
    if len(delta) != 3:
        raise ValueError('delta must be three integers (dx, dy, dz), got %r' % (delta,))
    if max(abs(v) for v in delta) > 2 ** 24:
        raise ValueError('delta must be at most 2^24 voxels on each axis, got %r' % (delta,))
    return delta


def _trimmed_points(found):
    """``SurfacePoints`` of full-capacity buffers -> the same with exactly N rows: the one host read of ``trim=True``."""
    cloud, rows = found.cloud, int(found.cloud.points.shape[0])
    count = cloud.host_offsets()[-1]   # the one synchronisation
    if count > rows:
        raise RuntimeError('extract_points: %d points do not fit capacity %d (trim=False returns the first %d and '
                           'the true count in offsets)' % (count, rows, rows))
    cut = (lambda t: None if t is None else t[:count])
    trimmed = PointCloud(cut(cloud.points), cut(cloud.colors), cut(cloud.index), cloud.offsets)
    trimmed.__dict__['_host_offsets'] = cloud.host_offsets()
    return SurfacePoints(trimmed, cut(found.normals))


def _trimmed_mesh(found):
    """``SurfaceMesh`` of full-capacity buffers -> the same with exactly N and F rows: the one host read of ``trim=True``."""
    mesh = found.mesh
    rows, face_rows = int(mesh.points.shape[0]), int(mesh.faces.shape[0])
    offsets, face_offsets = mesh._host()   # the one synchronisation
    count, face_count = offsets[-1], face_offsets[-1]
    if count > rows:
        raise RuntimeError('extract_mesh: %d vertices do not fit capacity %d (trim=False returns the first %d and '
                           'the true count in offsets)' % (count, rows, rows))
    if face_count > face_rows:
        raise RuntimeError('extract_mesh: %d faces do not fit face_capacity %d (trim=False returns the first %d and '
                           'the true count in face_offsets)' % (face_count, face_rows, face_rows))
    cut = (lambda t, n: None if t is None else t[:n])
    trimmed = type(mesh)(cut(mesh.points, count), cut(mesh.colors, count), cut(mesh.index, count), mesh.offsets,
                         cut(mesh.faces, face_count), mesh.face_offsets)
    trimmed.__dict__['_both'] = mesh.__dict__['_both']
    trimmed.__dict__['_host_both'] = mesh.__dict__['_host_both']
    return SurfaceMesh(trimmed, cut(found.normals, count))
