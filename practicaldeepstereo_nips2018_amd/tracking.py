"""Frame-to-model tracking: point-to-plane ICP of a disparity frame against the raycast model (not in the reference).

``TsdfVolume.integrate`` needs a pose per frame and ``TsdfVolume.raycast`` renders the model prediction of KinectFusion;
this module is the consumer of that prediction, so that the loop closes inside the package: track, integrate, raycast.

``icp_system(disparity, matrix, model, camera, transform=None, normals=None, valid=None, confidence=None,
min_confidence=0.0, max_distance=0.1, min_cosine=0.0, with_rows=False)`` -> ``IcpSystem(system, rows)``
(``pds_icp_system_fwd``; with Huber weights: ``icp_system_robust``, below).  ``disparity`` float32 [B, H, W] with
``matrix`` / ``valid`` / ``confidence`` / ``min_confidence`` as ``reproject`` takes them; ``normals`` float32
[B, H, W, 3], the frame's normals as ``surface_normals`` returns them (optional).  ``model``: a
``Raycast(depth [Bm, Hm, Wm], normals [Bm, Hm, Wm, 3])`` with Bm == B or 1; ``camera = (fx, fy, cx, cy, skew)`` its pinhole.  ``transform``: 3x4 ``[R | t]`` or [B, 3, 4] from the
frame's camera into the model's (None: the identity); the host rounds it once to float32.  Per source pixel, in fp32,
every multiply-add an explicit fmaf:

    1. P = the point ``reproject`` gives (the same device function); no row where it is NaN
    2. q_a = fmaf(R_a0, P_x, fmaf(R_a1, P_y, fmaf(R_a2, P_z, t_a))); no row unless q_z > 0 and q is finite
    3. x = q_x / q_z, y = q_y / q_z, u = fmaf(fx, x, fmaf(skew, y, cx)), v = fmaf(fy, y, cy);
       px = floor(u + 0.5), py = floor(v + 0.5) (the rounding of ``register_depth`` and ``integrate``); no row outside
       [0, Wm) x [0, Hm)
    4. Z = depth[py, px], n = normals[py, px]; no row where either holds a NaN.
       y_m = (py - cy) / fy, x_m = fmaf(-skew, y_m, px - cx) / fx (the ray of ``raycast``), m = (Z x_m, Z y_m, Z)
    5. e = m - q; no row unless fmaf(e_x, e_x, fmaf(e_y, e_y, e_z e_z)) <= max_distance * max_distance
    6. with frame normals n_f: s_a = fmaf(R_a0, n_fx, fmaf(R_a1, n_fy, R_a2 n_fz)); no row where n_f holds a NaN or not
       fmaf(s_x, n_x, fmaf(s_y, n_y, s_z n_z)) >= min_cosine
    7. r = fmaf(n_x, e_x, fmaf(n_y, e_y, n_z e_z)); J = (q x n, n), (q x n)_x = fmaf(q_y, n_z, -(q_z n_y)) and cyclic.
       The row is the seven float32 values (J_0 .. J_5, r)

``system`` is a float64 device tensor [B, 29]: the upper triangle of sum J J^T (21 values, row-major), sum J r (6),
sum r^2 and the row count.  Each product is formed exactly in fp64 from the float32 row values and added in fp64 in a
fixed order (thread t of a tile of 1024 pixels takes pixels k * 256 + t, k = 0 .. 3; a wave folds lane + 32, + 16, ...,
+ 1; waves 0 .. 3; the tiles of an entry in ascending order): no atomics, the same bits on every run and stream.
``rows`` float32 [B, H, W, 7] holds the row of every pixel, seven NaNs where there is none; None without ``with_rows``.
Current stream, no autograd, no host synchronisation.

``icp_system_robust(disparity, matrix, model, camera, huber, ...)`` (``pds_icp_system_robust_fwd``) takes the same
arguments and ``huber`` (positive, ``inf`` allowed; None: the unweighted entry point and its bits) and weights every row by
w = |r| <= huber ? 1.f : huber / |r| in fp32: each of the first 28 sums becomes fma((double) w, (double) a * (double) b,
sum) -- the inner product is exact in fp64, so the weight adds one rounding per term -- in the same order.  Slot 27 is
sum w r^2; slot 28 stays the unweighted row count.  The rows are unchanged.  ``huber=inf`` gives the bits of
``icp_system``.  ``icp_solve`` needs no change: A xi = g with weighted sums is one step of iteratively reweighted least
squares, and ``rmse`` is then sqrt(sum w r^2 / count).

``icp_solve(system, min_count=100, min_eigenvalue=1e-4)`` (host, numpy, fp64) -> ``IcpSolution(xi [B, 6], rmse [B],
count [B], status [B])``: minimising sum (r - J xi)^2 gives A xi = g with xi = (omega, v).  An entry with fewer than
``min_count`` rows is refused (``TOO_FEW_ROWS``), and so is one whose smallest eigenvalue of A / count is below
``min_eigenvalue`` (``DEGENERATE``: a single plane leaves three motions free); their xi is zero.  ``rmse`` is
sqrt(sum r^2 / count), NaN without rows.

``se3_exp(xi)`` -> the 3x4 ``[R | t]`` of the twist (omega, v): R = ``rodrigues(omega)``, t = V v with
V = I + (1 - cos th) / th^2 K + (th - sin th) / th^3 K^2, K the cross-product matrix of omega (the series below 1e-4 rad).

``TsdfVolume.track(disparity, matrix, pose, ...)`` -> ``Tracking(pose, rmse, inliers, iterations, status)``: raycasts the
volume ONCE at the predicted ``pose`` (world -> frame, as ``integrate`` takes it), starts from the identity transform
and iterates ``icp_system`` -> one host read of 29 B doubles -> ``icp_solve`` -> T <- exp(xi) T, until every entry is
refused, |xi| falls below ``tolerance`` or ``iterations`` are done.  The returned pose is T^-1 o pose, world -> frame,
ready for ``integrate``.  A refused entry keeps its predicted pose and says so in ``status``; nothing raises for a frame
that merely cannot be tracked.

``TsdfVolume.track_pyramid(disparity, matrix, pose, levels=3, huber=None, max_difference=None, ...)`` -> ``Tracking``
takes the keywords of ``track`` as well (``StereoRig.track`` goes there when it is given one of the three) and runs the
loop below (``track(volume, ..., levels=, huber=, max_difference=)`` of this module).  ``TsdfVolume.track`` and
``icp_system`` keep their argument lists.

Coarse to fine (``levels = L > 1``): what KinectFusion and its descendants do with image pyramids.  The frame becomes
``disparity_pyramid(disparity, L, max_difference, valid, confidence, min_confidence)`` (``pyramid.py``;
``max_difference=None``: ``DEFAULT_MAX_DIFFERENCE``, see there why), the model is raycast once per level at the predicted
pose with ``pyramid_camera(camera, l)`` at ``(W >> l, H >> l)``, and levels L - 1 .. 0 run the loop above with
``pyramid_matrix(matrix, l)``; the rigid transform carries from level to level.  Projective association pairs a pixel with
whatever lies within a pixel of its projection, and a pixel of level l is 2^l pixels wide: the coarse levels are there
to widen the basin (the corner scene of the tests does not show it: DESIGN.md 3.19), the fine ones keep the accuracy.  ``valid``, ``confidence`` and the frame's ``normals`` apply at level 0 only (the
pyramid has folded the first two in above it).  ``iterations`` is an int (the same count at every level) or a sequence of
length L indexed by level, and so is ``max_distance``.  An entry refused at a level above 0 keeps its transform and goes
on at the next finer level; a refusal at level 0 is what it is without levels.  ``status``, ``rmse`` and ``inliers`` are
those of the last level-0 system; ``Tracking.iterations`` is the total over the levels.  ``levels=1, huber=None`` is the
single-level loop, byte for byte.

For robust kernels or reweighting there is ``huber``: with it every system of the loop is ``icp_system_robust``'s, and
the loop is iteratively reweighted least squares with Huber weights.  The hard ``max_distance`` gate admits a mismatch blob whole or
rejects it whole; the weight lets the rows inside the gate count in proportion.

For colour terms there is ``track_color``.  Point-to-plane ICP cannot constrain motion along a surface: a wall leaves
three motions free and ``icp_solve`` refuses it as ``DEGENERATE``.  The image has the texture that fixes them, and the
model has it too since ``ColorTsdfVolume``; every descendant of KinectFusion that keeps colour adds a photometric term
(Steinbruecker / Kerl RGB-D odometry, Kintinuous / ElasticFusion, Open3D's coloured ICP).

``intensity_pyramid(image, levels=1, layout=None)`` (``pyramid.py``, ``pds_intensity_pyramid_fwd``) -> the luma
``fmaf(0.299f, c0, fmaf(0.587f, c1, 0.114f * c2))`` of an image and its halvings ``((a00 + a01) + (a10 + a11)) * 0.25f``.

``icp_color_system(disparity, intensity, matrix, model, model_intensity, camera, transform=None, normals=None,
valid=None, confidence=None, min_confidence=0.0, max_distance=0.1, min_cosine=0.0, huber=None, color_huber=None,
with_rows=False)`` -> ``IcpColorSystem(system, color_system, rows)`` (``pds_icp_color_system_fwd``).  ``intensity``
float32 [B, H, W]: the frame's level of the intensity pyramid; ``model``: a ``Raycast`` / ``ColorRaycast``, of which depth
and normals are read; ``model_intensity`` float32 [Bm, Hm, Wm]: ``intensity_pyramid(model.colors, 1, layout='nhwc')[0]``.
The geometric row is that of steps 1 - 7 by the same device code, and ``system`` has the bits of ``icp_system_robust`` on
the same arguments (of ``icp_system`` when ``huber`` is None).  The photometric row exists only where the geometric row
exists and where all of this holds, in fp32 with explicit fmaf:

    1. I_f = intensity[p] is not NaN
    2. with u, v of step 3, not rounded: x0 = floor(u), y0 = floor(v), a = u - x0, b = v - y0; no row unless 0 <= x0,
       x0 + 1 <= Wm - 1, 0 <= y0, y0 + 1 <= Hm - 1
    3. the taps L00, L10 (x0 + 1), L01 (y0 + 1), L11 of ``model_intensity`` and the model depths Z00 .. Z11 there; no row
       where one of the eight is NaN, or unless |Z_tap - q_z| <= max_distance for all four: the same surface, so colour
       is not mixed across an occlusion edge
    4. top = fmaf(a, L10 - L00, L00), bot = fmaf(a, L11 - L01, L01), I_m = fmaf(b, bot - top, top);
       I_u = fmaf(b, (L11 - L01) - (L10 - L00), L10 - L00), I_v = bot - top: the derivative of exactly what is sampled, so
       Gauss-Newton is consistent
    5. r_c = I_f - I_m; with x = q_x / q_z, y = q_y / q_z, iz = 1 / q_z: g_x = I_u fx iz, g_y = fmaf(I_u, skew, I_v fy) iz,
       g_z = -fmaf(g_x, x, g_y y); J_c = (q x g, g), the cross product formed as in step 7.  The row is
       (J_c0 .. J_c5, r_c), unscaled, in intensity units

The sign.  A step xi = (omega, v) moves the frame point as q <- q + omega x q + v.  Its projection (u, v) moves by
dpi/dq . dq with dpi/dq = [[fx, skew, -(fx x + skew y)], [0, fy, -fy y]] / q_z, and the sampled model intensity by
(I_u, I_v) . dpi/dq . dq = g . dq with g as in 5.  The residual after the step is
I_f - I_m(q + dq) = r_c - g . (omega x q) - g . v = r_c - (q x g) . omega - g . v = r_c - J_c xi, so the photometric rows
enter min sum (r - J xi)^2 as the geometric ones do (there r - n . dq, J = (q x n, n)).

``color_system`` holds the same 29 sums over the photometric rows, weighted by ``color_huber`` exactly as ``huber`` weights
the geometric ones (None or inf: exact products); slot 28 is the unweighted photometric row count.  Both systems come out
of one ``icp_color_rows`` launch per 16 entries and one reduce launch, in the order of additions of ``icp_system``; no
atomics.  ``rows`` float32 [B, H, W, 14]: the geometric row then the photometric row, seven NaNs each where absent.

``ColorTsdfVolume.track_color(disparity, image, matrix, pose, levels=1, huber=None, color_huber=None, color_weight=1e-3,
...)`` -> ``ColorTracking(pose, rmse, inliers, iterations, status, color_rmse, color_inliers)`` takes the keywords of
``track_pyramid`` too (``StereoRig.track_color`` sits beside it; ``track_color(volume, ...)`` of this module).  The frame
side is ``disparity_pyramid`` plus ``intensity_pyramid(image, levels)``; the model is one ``raycast(..., with_colors=True)``
per level plus its intensity; the iteration loop is that of ``track``, with one host read of 58 B doubles.  Per iteration
the host forms S = ``system`` and adds ``color_weight``^2 times the first 28 sums of ``color_system`` to those of S, in
fp64, and calls ``icp_solve(S, ...)`` unchanged: ``count``, ``min_count`` and the eigenvalue test act on the combined
normal matrix, which is what lets a textured wall pass.  ``rmse`` is the combined sqrt((sum r^2 + w^2 sum r_c^2) / count);
``color_rmse`` and ``color_inliers`` are those of the last level-0 photometric system, in intensity units.
``color_weight`` is in metres per intensity level: the default 1e-3 equates 5 levels of a 0 .. 255 image with 5 mm; an
image in 0 .. 1 wants 0.255.  ``color_weight=0`` with ``levels=1`` returns the pose, rmse, inliers and status of
``track_pyramid`` byte for byte.  ``levels <= 4`` (one launch of the intensity pyramid).  Refusals behave as in ``track``.

``track`` and ``track_pyramid`` stay purely geometric; for them it still holds:
Out of scope: colour terms, frame-to-frame tracking, loop closure.
Out of scope for the module: frame-to-frame tracking, loop closure.
There is no CPU fallback.
"""
import collections
import ctypes
import math
import operator

import numpy as np
import torch

from practicaldeepstereo_nips2018_amd import _lib

# system float64 [B, 29] on the device; rows float32 [B, H, W, 7] or None
IcpSystem = collections.namedtuple('IcpSystem', ['system', 'rows'])
# xi [B, 6] (omega, v), rmse [B], count [B] int64, status [B] int64: all numpy, on the host
IcpSolution = collections.namedtuple('IcpSolution', ['xi', 'rmse', 'count', 'status'])
# pose [B, 3, 4] float64 world -> frame; rmse [B]; inliers [B] int64; iterations int; status [B] int64: numpy
Tracking = collections.namedtuple('Tracking', ['pose', 'rmse', 'inliers', 'iterations', 'status'])
# system, color_system float64 [B, 29] on the device; rows float32 [B, H, W, 14] (geometric, then photometric) or None
IcpColorSystem = collections.namedtuple('IcpColorSystem', ['system', 'color_system', 'rows'])
# Tracking, and color_rmse [B] (intensity levels), color_inliers [B] int64: those of the last level-0 photometric system
ColorTracking = collections.namedtuple('ColorTracking', ['pose', 'rmse', 'inliers', 'iterations', 'status', 'color_rmse',
                                                         'color_inliers'])

TRACKED, TOO_FEW_ROWS, DEGENERATE = 0, 1, 2
SYSTEM = 29   # csrc/common.hpp: kIcpSystem

_Float5 = ctypes.c_float * 5
_Float16 = ctypes.c_float * 16
_IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))])

_workspace = _lib.Workspace()


def _number(value, name):
    try:
        return float(value)
    except (TypeError, ValueError):
        raise TypeError('%s must be a number, got %r' % (name, value))


def _poses(pose, batch, name):
    """-> [batch, 3, 4] fp64 from a 3x4, a [batch, 3, 4] or None (the identity)."""
    if pose is None:
        pose = _IDENTITY
    try:
        pose = np.asarray(pose, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError('%s must be an array of numbers' % name)
    if pose.shape == (3, 4):
        pose = np.broadcast_to(pose, (batch, 3, 4))
    if pose.shape != (batch, 3, 4) or not np.all(np.isfinite(pose)):
        raise ValueError('%s must be a finite 3x4 [R | t] or [%d, 3, 4], got shape %s' % (name, batch, pose.shape))
    return np.array(pose)


def _camera(camera):
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
    return camera


def _huber(huber, name='huber'):
    """None, or the positive Huber threshold as a float (+inf allowed)."""
    if huber is None:
        return None
    huber = _number(huber, name)
    if not huber > 0.0:
        raise ValueError('%s must be positive (inf allowed) or None, got %r' % (name, huber))
    return huber


def icp_system(disparity, matrix, model, camera, transform=None, normals=None, valid=None, confidence=None,
               min_confidence=0.0, max_distance=0.1, min_cosine=0.0, with_rows=False):
    """The point-to-plane system of a frame against a rendered model -> ``IcpSystem(system, rows)``: see the module text."""
    return _icp_system(disparity, matrix, model, camera, transform, normals, valid, confidence, min_confidence,
                       max_distance, min_cosine, with_rows, None)


def icp_system_robust(disparity, matrix, model, camera, huber, transform=None, normals=None, valid=None, confidence=None,
                      min_confidence=0.0, max_distance=0.1, min_cosine=0.0, with_rows=False):
    """``icp_system`` with Huber weights -> ``IcpSystem(system, rows)``: see the module text.  ``huber`` is positive
    (``inf`` allowed); None is ``icp_system`` itself, the unweighted entry point."""
    return _icp_system(disparity, matrix, model, camera, transform, normals, valid, confidence, min_confidence,
                       max_distance, min_cosine, with_rows, huber)


def icp_color_system(disparity, intensity, matrix, model, model_intensity, camera, transform=None, normals=None,
                     valid=None, confidence=None, min_confidence=0.0, max_distance=0.1, min_cosine=0.0, huber=None,
                     color_huber=None, with_rows=False):
    """The point-to-plane system and the photometric system of a frame with its intensity against a rendered, coloured
    model -> ``IcpColorSystem(system, color_system, rows)``: see the module text."""
    return _icp_system(disparity, matrix, model, camera, transform, normals, valid, confidence, min_confidence,
                       max_distance, min_cosine, with_rows, huber, color=(intensity, model_intensity, color_huber))


def _icp_system(disparity, matrix, model, camera, transform, normals, valid, confidence, min_confidence, max_distance,
                min_cosine, with_rows, huber, color=None):
    # what can be judged without a GPU comes first: types, shapes, thresholds
    floats = [('disparity', disparity, 3)]
    if color is not None:
        intensity, model_intensity, color_huber = color
        floats += [('intensity', intensity, 3), ('model_intensity', model_intensity, 3)]
    if confidence is not None:
        floats.append(('confidence', confidence, 3))
    if normals is not None:
        floats.append(('normals', normals, 4))
    try:
        model_depth, model_normals = model[0], model[1]
    except (TypeError, IndexError, KeyError):
        raise TypeError('model must be a Raycast(depth, normals), got %r' % (type(model).__name__,))
    if model_normals is None:
        raise ValueError('model has no normals: raycast with with_normals=True')
    floats += [('model.depth', model_depth, 3), ('model.normals', model_normals, 4)]
    for name, t, dims in floats:
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s must be a torch.Tensor' % name)
        if t.dtype != torch.float32:
            raise TypeError('%s must be float32, got %s' % (name, t.dtype))
        if t.dim() != dims:
            raise ValueError('%s must have %d dimensions, got %d' % (name, dims, t.dim()))
    shape = tuple(disparity.shape)
    m = np.asarray(matrix, dtype=np.float64)
    if m.shape != (4, 4) or not np.all(np.isfinite(m)):
        raise ValueError('matrix must be a finite 4x4, got shape %s' % (m.shape,))
    if 0 in shape:
        raise ValueError('icp_system: empty input %s' % (shape,))
    batch, height, width = shape
    if color is not None and tuple(intensity.shape) != shape:
        raise ValueError('intensity %s and disparity %s differ in shape' % (tuple(intensity.shape), shape))
    if batch * height * width > 2 ** 31 - 1:
        raise ValueError('B * H * W = %d does not fit 32-bit indices' % (batch * height * width))
    model_shape = tuple(model_depth.shape)
    if 0 in model_shape or model_shape[0] not in (1, batch):
        raise ValueError('model.depth must be [%d, Hm, Wm] or [1, Hm, Wm], got %s' % (batch, model_shape))
    if tuple(model_normals.shape) != model_shape + (3,):
        raise ValueError('model.normals must be %s, got %s' % (model_shape + (3,), tuple(model_normals.shape)))
    if color is not None and tuple(model_intensity.shape) != model_shape:
        raise ValueError('model_intensity must be %s, got %s' % (model_shape, tuple(model_intensity.shape)))
    if model_shape[0] * model_shape[1] * model_shape[2] > 2 ** 31 - 1:
        raise ValueError('Bm * Hm * Wm = %d does not fit 32-bit indices' % (model_shape[0] * model_shape[1] * model_shape[2]))
    camera = _camera(camera)
    transforms = _poses(transform, batch, 'transform')
    if normals is not None and tuple(normals.shape) != shape + (3,):
        raise ValueError('normals must be %s, got %s' % (shape + (3,), tuple(normals.shape)))
    if valid is not None:
        if not isinstance(valid, torch.Tensor):
            raise TypeError('valid must be a torch.Tensor')
        if valid.dtype != torch.bool or tuple(valid.shape) != shape:
            raise ValueError('valid must be torch.bool %s, got %s %s' % (shape, valid.dtype, tuple(valid.shape)))
    if confidence is not None and tuple(confidence.shape) != shape:
        raise ValueError('confidence %s and disparity %s differ in shape' % (tuple(confidence.shape), shape))
    min_confidence = _number(min_confidence, 'min_confidence')
    if math.isnan(min_confidence):
        raise ValueError('min_confidence is NaN')
    max_distance = _number(max_distance, 'max_distance')
    if not (max_distance > 0.0 and math.isfinite(max_distance)):
        raise ValueError('max_distance must be positive and finite, got %r' % (max_distance,))
    min_cosine = _number(min_cosine, 'min_cosine')
    if math.isnan(min_cosine):
        raise ValueError('min_cosine is NaN')
    huber = _huber(huber)
    if color is not None:
        color_huber = _huber(color_huber, 'color_huber')
    # then where the tensors live
    d = _lib.require_gpu_tensor(disparity.detach(), 'disparity', 3)
    device = d.device
    if color is not None:
        intensity = _lib.require_gpu_tensor(intensity.detach(), 'intensity', 3)
        model_intensity = _lib.require_gpu_tensor(model_intensity.detach(), 'model_intensity', 3)
    if valid is not None:
        if not valid.is_cuda:
            raise RuntimeError('valid must live on an MI355X (cuda) device: the HIP path has no CPU fallback')
        valid = valid.contiguous()
    if confidence is not None:
        confidence = _lib.require_gpu_tensor(confidence.detach(), 'confidence', 3)
    if normals is not None:
        normals = _lib.require_gpu_tensor(normals.detach(), 'normals', 4)
    model_depth = _lib.require_gpu_tensor(model_depth.detach(), 'model.depth', 3)
    model_normals = _lib.require_gpu_tensor(model_normals.detach(), 'model.normals', 4)
    for name, t in (('valid', valid), ('confidence', confidence), ('normals', normals), ('model.depth', model_depth),
                    ('model.normals', model_normals)) + (
                        (('intensity', intensity), ('model_intensity', model_intensity)) if color is not None else ()):
        if t is not None and t.device != device:
            raise ValueError('%s and disparity live on different devices' % name)
    system = torch.empty((batch, SYSTEM), dtype=torch.float64, device=device)
    rows = torch.empty(shape + (7,), dtype=torch.float32, device=device) if with_rows else None
    c_matrix = _Float16(*m.astype(np.float32).reshape(-1).tolist())
    c_camera = _Float5(*camera.astype(np.float32).tolist())
    c_transforms = (ctypes.c_float * (12 * batch))(*np.concatenate(
        [transforms[:, :, :3].reshape(batch, 9), transforms[:, :, 3]], axis=1).astype(np.float32).reshape(-1).tolist())
    lib = _lib.load()
    if color is not None:
        nbytes = int(lib.pds_icp_color_workspace_bytes(batch, height, width))
        if nbytes == 0:
            raise ValueError('icp_color_system: %s' % lib.pds_last_error().decode(errors='replace'))
        color_system = torch.empty((batch, SYSTEM), dtype=torch.float64, device=device)
        rows = torch.empty(shape + (14,), dtype=torch.float32, device=device) if with_rows else None
        inf = math.inf   # None: exact products
        with torch.cuda.device(device):
            workspace = _workspace.get(nbytes, device)
            _lib.check(lib.pds_icp_color_system_fwd(
                _lib.ptr(d), _lib.ptr(intensity), None if valid is None else _lib.ptr(valid),
                None if confidence is None else _lib.ptr(confidence), min_confidence, c_matrix,
                None if normals is None else _lib.ptr(normals), _lib.ptr(model_depth), _lib.ptr(model_normals),
                _lib.ptr(model_intensity), model_shape[0], model_shape[1], model_shape[2], c_camera, c_transforms,
                max_distance, min_cosine, inf if huber is None else huber, inf if color_huber is None else color_huber,
                _lib.ptr(system), _lib.ptr(color_system), None if rows is None else _lib.ptr(rows), batch, height, width,
                _lib.ptr(workspace), workspace.numel(), _lib.stream_handle(device)), 'pds_icp_color_system_fwd')
        return IcpColorSystem(system, color_system, rows)
    nbytes = int(lib.pds_icp_workspace_bytes(batch, height, width))
    if nbytes == 0:
        raise ValueError('icp_system: %s' % lib.pds_last_error().decode(errors='replace'))
    with torch.cuda.device(device):
        workspace = _workspace.get(nbytes, device)
        frame = (_lib.ptr(d), None if valid is None else _lib.ptr(valid),
                 None if confidence is None else _lib.ptr(confidence), min_confidence, c_matrix,
                 None if normals is None else _lib.ptr(normals), _lib.ptr(model_depth), _lib.ptr(model_normals),
                 model_shape[0], model_shape[1], model_shape[2], c_camera, c_transforms, max_distance, min_cosine)
        outputs = (_lib.ptr(system), None if rows is None else _lib.ptr(rows), batch, height, width, _lib.ptr(workspace),
                   workspace.numel(), _lib.stream_handle(device))
        if huber is None:
            _lib.check(lib.pds_icp_system_fwd(*(frame + outputs)), 'pds_icp_system_fwd')
        else:
            _lib.check(lib.pds_icp_system_robust_fwd(*(frame + (huber,) + outputs)), 'pds_icp_system_robust_fwd')
    return IcpSystem(system, rows)


_TRIANGLE = np.triu_indices(6)


def unpack_system(system):
    """[B, 29] (or [29]) -> (A [B, 6, 6] symmetric, g [B, 6], sum r^2 [B], count [B]) in fp64."""
    s = np.asarray(system, dtype=np.float64)
    if s.ndim == 1:
        s = s[None]
    if s.ndim != 2 or s.shape[1] != SYSTEM:
        raise ValueError('system must be [B, %d], got shape %s' % (SYSTEM, s.shape))
    A = np.zeros((s.shape[0], 6, 6))
    A[:, _TRIANGLE[0], _TRIANGLE[1]] = s[:, :21]
    A[:, _TRIANGLE[1], _TRIANGLE[0]] = s[:, :21]
    return A, s[:, 21:27].copy(), s[:, 27].copy(), s[:, 28].copy()


def icp_solve(system, min_count=100, min_eigenvalue=1e-4):
    """Host, numpy, fp64: [B, 29] -> ``IcpSolution(xi, rmse, count, status)``: see the module text."""
    if isinstance(system, torch.Tensor):
        system = system.detach().cpu().numpy()
    A, g, rr, count = unpack_system(system)
    min_count, min_eigenvalue = _number(min_count, 'min_count'), _number(min_eigenvalue, 'min_eigenvalue')
    batch = len(count)
    xi, rmse = np.zeros((batch, 6)), np.full(batch, np.nan)
    status = np.full(batch, TRACKED, dtype=np.int64)
    for b in range(batch):
        if count[b] > 0:
            rmse[b] = math.sqrt(max(rr[b], 0.0) / count[b])
        if not (count[b] >= min_count and count[b] > 0 and np.all(np.isfinite(A[b])) and np.all(np.isfinite(g[b]))):
            status[b] = TOO_FEW_ROWS
            continue
        if not np.linalg.eigvalsh(A[b] / count[b])[0] >= min_eigenvalue:
            status[b] = DEGENERATE
            continue
        xi[b] = np.linalg.solve(A[b], g[b])
    return IcpSolution(xi, rmse, count.astype(np.int64), status)


def se3_exp(xi):
    """Twist (omega, v), 6 values -> 3x4 ``[R | t]``: see the module text."""
    from practicaldeepstereo_nips2018_amd.rectification import rodrigues
    xi = np.asarray(xi, dtype=np.float64).reshape(-1)
    if xi.size != 6 or not np.all(np.isfinite(xi)):
        raise ValueError('xi must hold 6 finite values (omega, v), got %r' % (xi.tolist(),))
    w, v = xi[:3], xi[3:]
    theta2 = float(w @ w)
    theta = math.sqrt(theta2)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if theta < 1e-4:   # the series: the next terms are below 1e-18 relative
        b, c = 0.5 - theta2 / 24.0, 1.0 / 6.0 - theta2 / 120.0
    else:
        b, c = (1.0 - math.cos(theta)) / theta2, (theta - math.sin(theta)) / (theta2 * theta)
    V = np.eye(3) + b * K + c * (K @ K)
    return np.hstack([rodrigues(w), (V @ v)[:, None]])


def compose(a, b):
    """3x4 o 3x4: first b, then a."""
    return np.hstack([a[:, :3] @ b[:, :3], (a[:, :3] @ b[:, 3] + a[:, 3])[:, None]])


def invert(a):
    """The inverse of a rigid 3x4 ``[R | t]``: ``[R^T | -R^T t]``."""
    return np.hstack([a[:, :3].T, (-a[:, :3].T @ a[:, 3])[:, None]])


# ``max_difference`` of the frame's pyramid when ``track`` is given none: one disparity step, the threshold under which the
# package already calls two neighbouring pixels one surface (``speckle_filter`` / ``StereoRig.reconstruct``:
# ``speckle_difference = 1.0``).  The children of a level-l pixel lie 2^(l-1) pixels apart, so a surface whose disparity
# changes by less than 1 / 2^(l-1) per pixel along both axes together is still averaged whole at level l; a steeper one,
# and every depth edge, keeps its nearer children only -- a sample of the foreground, never a mixture.
DEFAULT_MAX_DIFFERENCE = 1.0


def _per_level(value, levels, name, convert):
    """A scalar (the same at every level) or a sequence of length ``levels`` indexed by level -> a list."""
    if isinstance(value, (list, tuple)) or (isinstance(value, np.ndarray) and value.ndim == 1):
        values = list(value)
        if len(values) != levels:
            raise ValueError('%s must be a single value or hold one per level (%d), got %d' % (name, levels, len(values)))
    else:
        values = [value] * levels
    return [convert(v) for v in values]


def track(volume, disparity, matrix, pose, camera=None, size=None, iterations=10, max_distance=None, min_cosine=0.5,
          normals=None, valid=None, confidence=None, min_confidence=0.0, min_weight=1.0, min_count=100,
          min_eigenvalue=1e-4, tolerance=1e-6, levels=1, huber=None, max_difference=None):
    """``TsdfVolume.track`` and ``TsdfVolume.track_pyramid``: see the module text."""
    return _track(volume, disparity, matrix, pose, camera, size, iterations, max_distance, min_cosine, normals, valid,
                  confidence, min_confidence, min_weight, min_count, min_eigenvalue, tolerance, levels, huber,
                  max_difference, None)


def track_color(volume, disparity, image, matrix, pose, levels=1, huber=None, color_huber=None, color_weight=1e-3,
                camera=None, size=None, iterations=10, max_distance=None, min_cosine=0.5, normals=None, valid=None,
                confidence=None, min_confidence=0.0, min_weight=1.0, min_count=100, min_eigenvalue=1e-4, tolerance=1e-6,
                max_difference=None):
    """``ColorTsdfVolume.track_color``: the loop of ``track`` on the sum of the point-to-plane and the photometric system
    -> ``ColorTracking``: see the module text."""
    if not hasattr(volume, 'color'):
        raise TypeError('track_color needs a ColorTsdfVolume: the model image is its coloured raycast')
    color_huber = _huber(color_huber, 'color_huber')
    color_weight = _number(color_weight, 'color_weight')
    if not (color_weight >= 0.0 and math.isfinite(color_weight)):
        raise ValueError('color_weight must be finite and >= 0 (metres per intensity level), got %r' % (color_weight,))
    return _track(volume, disparity, matrix, pose, camera, size, iterations, max_distance, min_cosine, normals, valid,
                  confidence, min_confidence, min_weight, min_count, min_eigenvalue, tolerance, levels, huber,
                  max_difference, (image, color_huber, color_weight))


def _track(volume, disparity, matrix, pose, camera, size, iterations, max_distance, min_cosine, normals, valid,
           confidence, min_confidence, min_weight, min_count, min_eigenvalue, tolerance, levels, huber, max_difference,
           color):
    """The loop of ``track``; with ``color = (image, color_huber, color_weight)`` that of ``track_color``."""
    from practicaldeepstereo_nips2018_amd import pyramid as _pyramid
    from practicaldeepstereo_nips2018_amd.tsdf import camera_of_matrix
    if not isinstance(disparity, torch.Tensor):
        raise TypeError('disparity must be a torch.Tensor')
    if disparity.dim() != 3:
        raise ValueError('disparity must have 3 dimensions, got %d' % disparity.dim())
    if 0 in tuple(disparity.shape):
        raise ValueError('track: empty input %s' % (tuple(disparity.shape),))
    batch, height, width = disparity.shape
    if pose is None:
        raise ValueError('track needs the predicted pose (world -> frame), e.g. the pose of the frame before')
    predicted = _poses(pose, batch, 'pose')
    m = np.asarray(matrix, dtype=np.float64)
    if m.shape != (4, 4) or not np.all(np.isfinite(m)):
        raise ValueError('matrix must be a finite 4x4, got shape %s' % (m.shape,))
    camera = _camera(camera_of_matrix(m) if camera is None else camera)
    if size is None:
        size = (width, height)
    levels = _pyramid.check_levels(levels, height, width)
    if color is not None:
        from practicaldeepstereo_nips2018_amd.tsdf_color import image_layout
        image, color_huber, color_weight = color
        layout = 'nchw' if image_layout(image, (batch, height, width)) == 0 else None
        if levels > _pyramid.INTENSITY_LEVELS:
            raise ValueError('track_color: levels must be in 1 .. %d, got %d' % (_pyramid.INTENSITY_LEVELS, levels))

    def count(value):
        try:
            value = operator.index(value)
        except TypeError:
            raise TypeError('iterations must be an integer, got %r' % (value,))
        if value < 1:
            raise ValueError('iterations must be at least 1, got %d' % value)
        return value

    def distance(value):
        value = 2.0 * volume.truncation if value is None else _number(value, 'max_distance')
        if not (value > 0.0 and math.isfinite(value)):
            raise ValueError('max_distance must be positive and finite, got %r' % (value,))
        return value

    iterations = _per_level(iterations, levels, 'iterations', count)
    max_distance = _per_level(max_distance, levels, 'max_distance', distance)
    tolerance = _number(tolerance, 'tolerance')
    if not tolerance >= 0.0:
        raise ValueError('tolerance must be >= 0, got %r' % (tolerance,))
    huber = _huber(huber)
    if levels > 1:
        max_difference = _pyramid.check_max_difference(DEFAULT_MAX_DIFFERENCE if max_difference is None else max_difference)
        try:
            size = (operator.index(size[0]), operator.index(size[1]))
        except (TypeError, IndexError):
            raise TypeError('size must be (width, height), got %r' % (size,))
        if (size[0] >> (levels - 1)) < 1 or (size[1] >> (levels - 1)) < 1:
            raise ValueError('levels = %d leaves no pixel of a %d x %d model at level %d' % ((levels,) + size + (levels - 1,)))
        frames = _pyramid.disparity_pyramid(disparity, levels, max_difference, valid=valid, confidence=confidence,
                                            min_confidence=min_confidence)
    else:
        frames = [disparity]
    # one model per level, each raycast once at the predicted pose
    models = [volume.raycast(_pyramid.pyramid_camera(camera, l) if l else camera,
                             (size[0] >> l, size[1] >> l) if l else size, pose=predicted, min_weight=min_weight)
              for l in range(levels)]
    if color is not None:
        # the frame's intensity pyramid in one launch, and the luma of every level's coloured raycast
        intensities = _pyramid.intensity_pyramid(image, levels, layout=layout)
        model_intensities = [_pyramid.intensity_pyramid(model.colors, 1, layout='nhwc')[0] for model in models]
        color_rmse, color_inliers = np.full(batch, np.nan), np.zeros(batch, dtype=np.int64)
    transform = np.broadcast_to(_IDENTITY, (batch, 3, 4)).copy()
    status = np.full(batch, TRACKED, dtype=np.int64)
    rmse, inliers = np.full(batch, np.nan), np.zeros(batch, dtype=np.int64)
    done = 0
    for l in range(levels - 1, -1, -1):
        # valid, confidence and the frame's normals belong to level 0: the pyramid has folded the first two in above it
        matrix_l = _pyramid.pyramid_matrix(m, l) if l else m
        camera_l = _camera(_pyramid.pyramid_camera(camera, l)) if l else camera
        fine = dict(normals=normals, valid=valid, confidence=confidence, min_confidence=min_confidence) if l == 0 else {}
        active = np.ones(batch, dtype=bool)   # an entry refused above level 0 keeps its transform and goes on here
        for _ in range(iterations[l]):
            if color is None:
                system = icp_system_robust(frames[l], matrix_l, models[l], camera_l, huber, transform=transform,
                                           max_distance=max_distance[l], min_cosine=min_cosine, **fine).system
                system = system.cpu().numpy()   # the one host read of 29 B doubles
            else:
                both = icp_color_system(frames[l], intensities[l], matrix_l, models[l], model_intensities[l], camera_l,
                                        transform=transform, max_distance=max_distance[l], min_cosine=min_cosine,
                                        huber=huber, color_huber=color_huber, **fine)
                both = torch.cat([both.system, both.color_system], dim=1).cpu().numpy()   # the one host read: 58 B doubles
                system, photometric = both[:, :SYSTEM].copy(), both[:, SYSTEM:]
                if color_weight > 0.0:   # (0: the geometric system as it is, and the bits of track_pyramid)
                    system[:, :SYSTEM - 1] += (color_weight * color_weight) * photometric[:, :SYSTEM - 1]
                if l == 0:
                    for b in np.nonzero(active)[0]:
                        color_inliers[b] = int(photometric[b, SYSTEM - 1])
                        color_rmse[b] = (math.sqrt(max(photometric[b, SYSTEM - 2], 0.0) / photometric[b, SYSTEM - 1])
                                         if photometric[b, SYSTEM - 1] > 0 else np.nan)
            solution = icp_solve(system, min_count, min_eigenvalue)
            done += 1
            moved = 0.0
            for b in np.nonzero(active)[0]:
                if l == 0:
                    rmse[b], inliers[b], status[b] = solution.rmse[b], solution.count[b], solution.status[b]
                if solution.status[b] != TRACKED:
                    active[b] = False
                    continue
                transform[b] = compose(se3_exp(solution.xi[b]), transform[b])
                moved = max(moved, float(np.linalg.norm(solution.xi[b])))
            if not active.any() or moved < tolerance:
                break
    result = predicted.copy()
    for b in range(batch):
        if status[b] == TRACKED:
            result[b] = compose(invert(transform[b]), predicted[b])
    if color is not None:
        return ColorTracking(result, rmse, inliers, done, status, color_rmse, color_inliers)
    return Tracking(result, rmse, inliers, done, status)
