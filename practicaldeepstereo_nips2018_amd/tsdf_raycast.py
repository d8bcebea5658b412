"""TSDF raycast: a ``TsdfVolume`` seen from a pinhole camera, as a depth map and a normal map (not in the reference).

``extract_points`` returns the fused surface as an unordered cloud; everything else behind the network works on images.
Raycasting (the other half of KinectFusion) brings the denoised, hole-filled model back as an image: the model
prediction at a pose, what has been fused so far, or N noisy frames as one clean depth map.

``TsdfVolume.raycast(camera, size, pose=None, min_weight=1.0, step=None, near=0.0, far=inf, with_normals=True)`` ->
``Raycast(depth, normals)`` (``pds_tsdf_raycast_fwd``).  ``camera = (fx, fy, cx, cy, skew)``, ``size = (width, height)``,
``pose``: 3x4 ``[R | t]`` or [B, 3, 4], world -> camera, as ``integrate`` takes it (None: the identity, B = 1).
``depth``: float32 [B, H, W], the camera-frame Z of the surface along the ray of each pixel centre, NaN where there is
none (the convention of ``reproject(..., depth_only=True)``).  ``normals``: float32 [B, H, W, 3], unit, in the camera
frame, facing the camera, (NaN, NaN, NaN) where there is none; None without ``with_normals``.  ``step``: the distance
between samples in units of Z; None means ``truncation / 2``.

The host folds the pose in fp64 and rounds once to float32 (``TsdfVolume.rays`` returns the fp64 rows):
``M = R^T / voxel_size``, ``o = (-R^T t - origin) / voxel_size - 0.5``.  In these grid coordinates voxel (i, j, k) is the
point (i, j, k).  The kernel works per pixel (px, py) in fp32, every multiply-add an explicit fmaf:

    1. y = (py - cy) / fy, x = (px - cx - skew y) / fx, dir = (x, y, 1): the ray parameter s IS the camera Z.
       d = M dir, g(s) = o + s d
    2. [s0, s1]: s slab-clipped to 0 <= g_a <= n_a - 1 on the three axes, intersected with [near, far].  A miss if that is
       empty or not finite, or if any n_a < 2
    3. samples s_m = fmaf(m, step, s0), m = 0, 1, ... while s_m <= s1.  c_a = min(floor(g_a), n_a - 2), f_a = g_a - c_a;
       the sample is observed when all eight corners of cell c have weight >= min_weight; its value is then the trilinear
       interpolant of tsdf, in x, then y, then z, each lerp fmaf(t, b - a, a)
    4. the march stops at the first observed sample whose value is < 0.  A hit only if sample m - 1 exists, is observed
       and is not < 0; otherwise a miss (the ray met the surface from behind or came out of unobserved space).  Running
       past s1 is a miss
    5. depth = fmaf(step, v_prev / (v_prev - v_cur), s_prev)
    6. the normal is the analytic gradient of the trilinear interpolant in the cell that contains g(depth), rotated by R
       (the float32 row of the pose), scaled by its largest component and normalised; NaN where that cell has an
       unobserved corner or the gradient is zero or not finite -- the depth stays.  The tsdf is positive towards the
       camera, so the normal faces it; on noisy data the interpolant need not fall monotonically between two samples, and
       the few normals that would point along the ray (n . dir > 0) are negated

Current stream, no autograd, no synchronisation, no workspace, no atomics: the same bits on every run and stream.  A march
that could be long is refused: the box diagonal in metres / step may not exceed 65536 samples.

``depth_to_disparity(depth, matrix)`` (pure torch) turns such a depth map into the disparity a matrix of the canonical
rectified form reprojects to it, so that ``surface_normals``, ``triangle_mesh``, ``point_cloud`` and ``register_depth``
take the rendered model as they take a frame.

The consumer of the model prediction, pose estimation by point-to-plane ICP of a new frame against these two maps, is
``tracking.py`` (``TsdfVolume.track``).

``ColorTsdfVolume.raycast`` in ``tsdf_color.py`` adds the colour of the surface to the two maps.

Out of scope: empty-space skipping that changes the sample positions, refinement beyond the one linear step, colour, a
sparse volume.  There is no CPU fallback.
"""
import collections
import ctypes
import math
import operator

import numpy as np
import torch

from practicaldeepstereo_nips2018_amd import _lib

# depth float32 [B, H, W] (NaN: no surface); normals float32 [B, H, W, 3] or None
Raycast = collections.namedtuple('Raycast', ['depth', 'normals'])

_Float5 = ctypes.c_float * 5


def rays(volume, pose, batch):
    """The [batch, 21] fp64 rows ``M`` (9, row-major), ``o`` (3) and ``R`` (9) of ``raycast`` for ``pose``: 3x4 ``[R | t]``
    for every entry, [batch, 3, 4], or None (the identity)."""
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
    rows = np.empty((batch, 21))
    for b in range(batch):
        R, t = pose[b, :, :3], pose[b, :, 3]
        rows[b, :9] = (R.T / volume.voxel_size).reshape(-1)
        rows[b, 9:12] = (-R.T @ t - volume.origin) / volume.voxel_size - 0.5
        rows[b, 12:] = R.reshape(-1)
    return rows


def _number(value, name):
    try:
        return float(value)
    except (TypeError, ValueError):
        raise TypeError('%s must be a number, got %r' % (name, value))


def raycast(volume, camera, size, pose=None, min_weight=1.0, step=None, near=0.0, far=math.inf, with_normals=True):
    """``TsdfVolume.raycast``: see the module text."""
    # what can be judged without a GPU comes first
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
    try:
        width, height = (operator.index(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError('size must be two integers (width, height), got %r' % (size,))
    if width < 1 or height < 1:
        raise ValueError('size must be at least (1, 1), got %r' % (size,))
    batch = 1
    if pose is not None and np.ndim(pose) == 3:
        batch = int(np.shape(pose)[0])
        if batch < 1:
            raise ValueError('pose must hold at least one entry, got shape %s' % (np.shape(pose),))
    rows = rays(volume, pose, batch)
    if batch * height * width > 2 ** 31 - 1:
        raise ValueError('B * H * W = %d does not fit 32-bit indices' % (batch * height * width))
    min_weight = _number(min_weight, 'min_weight')
    if math.isnan(min_weight):
        raise ValueError('min_weight is NaN')
    step = 0.5 * volume.truncation if step is None else _number(step, 'step')
    if not (step > 0.0 and math.isfinite(step)):
        raise ValueError('step must be positive and finite, got %r' % (step,))
    near, far = _number(near, 'near'), _number(far, 'far')
    if not (near >= 0.0 and math.isfinite(near)):
        raise ValueError('near must be >= 0 and finite, got %r' % (near,))
    if not far > near:
        raise ValueError('far must be above near, got near = %r, far = %r' % (near, far))
    nx, ny, nz = volume.dims
    diagonal = volume.voxel_size * math.sqrt((nx - 1) ** 2 + (ny - 1) ** 2 + (nz - 1) ** 2)
    if diagonal / step > 65536:
        raise ValueError('step %r is too small: the box diagonal of %g m would hold %d samples (at most 65536)' %
                         (step, diagonal, int(diagonal / step)))
    # then where the tensors live
    if not (volume.tsdf.is_cuda and volume.weight.is_cuda):
        raise RuntimeError('the volume must live on an MI355X (cuda) device: the HIP path has no CPU fallback')
    depth = torch.empty((batch, height, width), dtype=torch.float32, device=volume.device)
    normals = torch.empty((batch, height, width, 3), dtype=torch.float32, device=volume.device) if with_normals else None
    rows = rows.astype(np.float32)
    c_rays = (ctypes.c_float * (12 * batch))(*rows[:, :12].reshape(-1).tolist())
    c_rotations = (ctypes.c_float * (9 * batch))(*rows[:, 12:].reshape(-1).tolist())
    c_camera = _Float5(*camera.astype(np.float32).tolist())
    lib = _lib.load()
    with torch.cuda.device(volume.device):
        _lib.check(lib.pds_tsdf_raycast_fwd(
            _lib.ptr(volume.tsdf), _lib.ptr(volume.weight), nx, ny, nz, volume.voxel_size, c_rays, c_rotations, c_camera,
            step, near, far, min_weight, _lib.ptr(depth), None if normals is None else _lib.ptr(normals), batch, height,
            width, _lib.stream_handle(volume.device)), 'pds_tsdf_raycast_fwd')
    return Raycast(depth, normals)


def depth_to_disparity(depth, matrix):
    """Depth (any float tensor, e.g. ``Raycast.depth``) -> the disparity that ``reproject`` with ``matrix`` turns back
    into it: for a matrix of the canonical rectified form ``[[1, 0, 0, -cx], [0, 1, 0, -cy], [0, 0, 0, f], [0, 0, a, b]]``
    (``camera_of_matrix`` recognises it) Z = f / (a d + b), so d = (f / Z - b) / a.  NaN stays NaN; a depth that is not
    positive, or whose disparity would not be, becomes NaN as well (``reproject`` drops d <= 0).  Pure torch, on the
    tensor's own device; the result feeds ``surface_normals``, ``triangle_mesh``, ``point_cloud`` and ``register_depth``."""
    from practicaldeepstereo_nips2018_amd.tsdf import camera_of_matrix
    if not isinstance(depth, torch.Tensor):
        raise TypeError('depth must be a torch.Tensor')
    if not depth.is_floating_point():
        raise TypeError('depth must be a floating-point tensor, got %s' % depth.dtype)
    focal = camera_of_matrix(matrix)[0]
    m = np.asarray(matrix, dtype=np.float64)
    a, b = float(m[3, 2]), float(m[3, 3])
    if a == 0.0:
        raise ValueError('matrix[3][2] is 0: this matrix gives every disparity the same depth')
    depth = depth.detach()
    disparity = (focal / depth - b) / a
    return torch.where((depth > 0) & (disparity > 0), disparity, torch.full_like(disparity, float('nan')))
