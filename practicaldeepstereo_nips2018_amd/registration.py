"""Depth registration: the depth of the rectified left view seen from another camera (not in the reference).

Everything behind the network -- ``reproject``, ``point_cloud`` -- lives on the pixel grid of the rectified left view.
A detector runs on the raw (distorted) left frame, a rig with a colour camera wants depth per colour pixel, and the
occlusion mask of the right view is the left depth seen from the right camera.  ``register_depth`` is that step as one
entry point (``pds_register_depth_fwd``: a z-buffered forward warp, as OpenCV ``rgbd::registerDepth``, ROS
``depth_image_proc/register``, RealSense ``align``).  The host composes ``M' = [[R, t], [0, 0, 0, 1]] @ matrix`` in fp64
and rounds it once to float32; then, per source pixel ``p`` (raster index ``y * W + x`` within its batch entry), in fp32:

    1. (X, Y, Z) = reproject's point at p for M' (the same device function, so the same pixels are kept: d finite and
       d > 0, W > 0, ``valid``, ``confidence >= min_confidence``).  Dropped unless Z is finite and Z > 0.
    2. x = X / Z, y = Y / Z, r2 = x^2 + y^2.  Dropped when 1 + 3 k1 r2 + 5 k2 r2^2 + 7 k3 r2^3 <= 0: there the radial
       model has folded back, and a point far outside the field of view would otherwise land inside the image.  (OpenCV's
       projectPoints has no such guard.)
    3. kr = 1 + ((k3 r2 + k2) r2 + k1) r2;  xd = x kr + 2 p1 x y + p2 (r2 + 2 x^2);  yd = y kr + p1 (r2 + 2 y^2) + 2 p2 x y
       u = fx xd + skew yd + cx;  v = fy yd + cy.  Dropped if u or v is not finite.
    4. footprint: ``splat=1`` the one pixel (floor(u + 0.5), floor(v + 0.5)); ``splat=2`` the four pixels {floor(u),
       floor(u) + 1} x {floor(v), floor(v) + 1}, which closes the one-pixel cracks a forward warp leaves when the target
       samples the surface more densely than the source.  Footprint pixels outside the target are skipped one by one.
    5. every footprint pixel receives key = (uint64(bits of Z) << 32) | uint32(p) by a 64-bit unsigned atomic minimum.

    target pixel     depth [B, Ht, Wt] float32       index [B, Ht, Wt] int32     valid [B, Ht, Wt] bool
    never written    fill_value (default NaN)        -1                          False
    written          the winning Z, bit for bit      the winning p               True

The nearest point wins, among equal depths the smaller source index; the minimum of integers does not depend on arrival
order, so the output has the same bits on every run and on every stream (no floating-point atomic is involved).
Limit: with a target much denser than the source, background can show through foreground even with ``splat=2``.  There
is no hole filling; ``median_filter(depth, ..., valid=valid, fill_holes=True)`` on the registered depth is the tool for
that.  There is no CPU fallback.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from practicaldeepstereo_nips2018_amd import _lib

RegisteredDepth = collections.namedtuple('RegisteredDepth', ['depth', 'index', 'valid'])

_Float16 = ctypes.c_float * 16
_Float5 = ctypes.c_float * 5

_workspace = _lib.Workspace()


def compose(pose, matrix):
    """``M' = [[R, t], [0, 0, 0, 1]] @ matrix`` in fp64: ``matrix`` (4x4) takes a source pixel and its disparity to a
    point in some frame, ``pose = [R | t]`` (3x4) takes that frame to the target camera's."""
    pose = np.asarray(pose, dtype=np.float64)
    if pose.shape != (3, 4) or not np.all(np.isfinite(pose)):
        raise ValueError('pose must be a finite 3x4 [R | t], got shape %s' % (pose.shape,))
    m = np.asarray(matrix, dtype=np.float64)
    if m.shape != (4, 4) or not np.all(np.isfinite(m)):
        raise ValueError('matrix must be a finite 4x4, got shape %s' % (m.shape,))
    full = np.eye(4)
    full[:3] = pose
    return full @ m


def _five(values, name, pad_from=5):
    try:
        a = np.asarray([] if values is None else values, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise TypeError('%s must be a sequence of numbers, got %r' % (name, values))
    if not pad_from <= a.size <= 5:
        raise ValueError('%s must hold %s values, got %d' % (name, '5' if pad_from == 5 else '4 or 5', a.size))
    if not np.all(np.isfinite(a)):
        raise ValueError('%s has non-finite entries: %r' % (name, a.tolist()))
    return np.concatenate([a, np.zeros(5 - a.size)])


def _gpu_device(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor' % name)
    if not t.is_cuda:
        raise RuntimeError('%s must live on an MI355X (cuda) device: the HIP path has no CPU fallback' % name)
    return t.device


def register_depth(disparity, matrix, pose, camera, distortion, size, valid=None, confidence=None, min_confidence=0.0,
                   splat=1, fill_value=math.nan, with_index=True):
    """Disparity float32 [B, H, W] -> ``RegisteredDepth(depth, index, valid)`` on the pixel grid of another camera (see
    the module text).

    ``matrix``: the 4x4 of ``reproject``.  ``pose``: 3x4 ``[R | t]`` from that matrix's frame to the target camera's.
    ``camera``: ``(fx, fy, cx, cy, skew)`` of the target.  ``distortion``: ``(k1, k2, p1, p2[, k3])`` (None: none).
    ``size``: ``(Wt, Ht)``.  ``valid`` / ``confidence`` / ``min_confidence``: as ``reproject`` takes them.  ``splat``: 1 or 2.
    ``fill_value``: the depth of a target pixel nothing landed on.  ``with_index=False`` leaves ``index`` None.
    Runs on the current stream, without autograd and without any synchronisation."""
    # what can be judged without a GPU comes first: types, shapes, thresholds
    for name, t in (('disparity', disparity),) + ((('confidence', confidence),) if confidence is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s must be a torch.Tensor' % name)
        if t.dtype != torch.float32:
            raise TypeError('%s must be float32, got %s' % (name, t.dtype))
        if t.dim() != 3:
            raise ValueError('%s must have 3 dimensions, got %d' % (name, t.dim()))
    shape = tuple(disparity.shape)
    composed = compose(pose, matrix)
    camera = _five(camera, 'camera')
    if not (camera[0] > 0 and camera[1] > 0):
        raise ValueError('camera must have positive focal lengths, got fx = %r, fy = %r' % (camera[0], camera[1]))
    distortion = _five(distortion, 'distortion', pad_from=0 if distortion is None else 4)
    try:
        target_width, target_height = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError('size must be (width, height), got %r' % (size,))
    if target_width < 1 or target_height < 1:
        raise ValueError('size must be at least (1, 1), got %r' % (size,))
    min_confidence = float(min_confidence)
    if not math.isfinite(min_confidence):
        raise ValueError('min_confidence must be finite, got %r' % (min_confidence,))
    if isinstance(splat, bool) or splat not in (1, 2):
        raise ValueError('splat must be 1 or 2, got %r' % (splat,))
    fill_value = float(fill_value)
    if valid is not None:
        if not isinstance(valid, torch.Tensor):
            raise TypeError('valid must be a torch.Tensor')
        if valid.dtype != torch.bool or tuple(valid.shape) != shape:
            raise ValueError('valid must be torch.bool %s, got %s %s' % (shape, valid.dtype, tuple(valid.shape)))
    if confidence is not None and tuple(confidence.shape) != shape:
        raise ValueError('confidence %s and disparity %s differ in shape' % (tuple(confidence.shape), shape))
    # then where the tensors live
    d = _lib.require_gpu_tensor(disparity.detach(), 'disparity', 3)
    if d.numel() == 0:
        raise ValueError('register_depth: empty input %s' % (shape,))
    if valid is not None:
        _gpu_device(valid, 'valid')
        valid = valid.contiguous()
    if confidence is not None:
        confidence = _lib.require_gpu_tensor(confidence.detach(), 'confidence', 3)
    for name, t in (('valid', valid), ('confidence', confidence)):
        if t is not None and t.device != d.device:
            raise ValueError('%s and disparity live on different devices' % name)
    batch, height, width = shape
    c_matrix = _Float16(*composed.astype(np.float32).reshape(-1).tolist())
    c_camera = _Float5(*camera.astype(np.float32).tolist())
    c_distortion = _Float5(*distortion.astype(np.float32).tolist())
    lib = _lib.load()
    nbytes = int(lib.pds_register_depth_workspace_bytes(batch, target_height, target_width))
    if nbytes == 0:
        raise ValueError('register_depth: %s' % lib.pds_last_error().decode(errors='replace'))
    out_shape = (batch, target_height, target_width)
    depth = torch.empty(out_shape, dtype=torch.float32, device=d.device)
    index = torch.empty(out_shape, dtype=torch.int32, device=d.device) if with_index else None
    hit = torch.empty(out_shape, dtype=torch.bool, device=d.device)
    with torch.cuda.device(d.device):
        workspace = _workspace.get(nbytes, d.device)
        _lib.check(lib.pds_register_depth_fwd(
            _lib.ptr(d), None if valid is None else _lib.ptr(valid),
            None if confidence is None else _lib.ptr(confidence), min_confidence, c_matrix, c_camera, c_distortion,
            int(splat), fill_value, _lib.ptr(depth), None if index is None else _lib.ptr(index), _lib.ptr(hit), batch,
            height, width, target_height, target_width, _lib.ptr(workspace), workspace.numel(),
            _lib.stream_handle(d.device)), 'pds_register_depth_fwd')
    return RegisteredDepth(depth, index, hit)
