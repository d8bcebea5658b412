"""Edge- and hole-aware disparity pyramid (not in the reference): the frame side of coarse-to-fine tracking.

``disparity_pyramid(disparity, levels, max_difference, valid=None, confidence=None, min_confidence=0.0)`` -> a list of
``levels`` float32 tensors: ``[0]`` is ``disparity`` itself (not copied), ``[l]`` is [B, H >> l, W >> l].  Sizes floor, so a
last odd row or column is dropped; ``levels >= 1`` and ``H >> (levels - 1) >= 1``, ``W >> (levels - 1) >= 1``.  Disparity
values stay in level-0 units.  A pixel of level l is formed from its four children at level l - 1, taken in the order
(0,0), (0,1), (1,0), (1,1) (row, column); everything is fp32 without contraction:

    eligible   at level 0: isfinite(d) and d > 0, ``valid != 0`` where given, ``confidence >= min_confidence`` where given
               (a NaN fails): the mask of ``reproject`` less its matrix test.  Above level 0: the child is not NaN
    m          the largest eligible child: the foreground wins, and a block astride a depth edge is not averaged across
    members    the eligible children with m - c <= max_difference (one fp32 subtraction)
    value      the sum of the members in child order divided by their count; NaN without a member

One launch of ``pds_disparity_pyramid_fwd`` forms up to three levels (a workgroup owns a 32 x 32 block of its source and
needs no other); a deeper pyramid repeats it on its own last output: ceil((levels - 1) / 3) launches.  No atomics, no
workspace, the current stream, no autograd; the same bits on every run and stream.  There is no CPU fallback.

Pixel centres are integers, as in ``reproject`` and ``raycast``, so the mean position of a 2 x 2 block is 2 x' + 0.5 and

    S = [[2, 0, 0, .5], [0, 2, 0, .5], [0, 0, 1, 0], [0, 0, 0, 1]]

maps (x', y', d, 1) of level l to level l - 1.  ``pyramid_matrix(matrix, level)`` -> 4x4 fp64 ``matrix . S^level``: the
reprojection matrix of that level.  ``pyramid_camera(camera, level)`` -> ``(fx, fy, cx, cy, skew)`` after ``level`` times
(fx / 2, fy / 2, (cx - .5) / 2, (cy - .5) / 2, skew / 2): the pinhole that sees the same rays through the pixels of that
level, as ``raycast`` takes it.
"""
import ctypes
import math
import operator

import numpy as np
import torch

from practicaldeepstereo_nips2018_amd import _lib

LEVELS_PER_LAUNCH = 3   # csrc/common.hpp: kPyramidLevels
BLOCK = 32              # csrc/pyramid.hip: a workgroup per BLOCK x BLOCK pixels of the source

STEP = np.array([[2.0, 0.0, 0.0, 0.5], [0.0, 2.0, 0.0, 0.5], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])


def _level(level, name='level', least=0):
    if isinstance(level, bool):
        raise TypeError('%s must be an integer, got %r' % (name, level))
    try:
        level = operator.index(level)
    except TypeError:
        raise TypeError('%s must be an integer, got %r' % (name, level))
    if level < least:
        raise ValueError('%s must be at least %d, got %d' % (name, least, level))
    return level


def pyramid_matrix(matrix, level):
    """The reprojection matrix of pyramid level ``level``: 4x4 fp64 ``matrix . S^level`` (see the module text)."""
    level = _level(level)
    m = np.asarray(matrix, dtype=np.float64)
    if m.shape != (4, 4) or not np.all(np.isfinite(m)):
        raise ValueError('matrix must be a finite 4x4, got shape %s' % (m.shape,))
    # S^level in closed form (exact: powers of two): x = 2^l x' + (2^l - 1) / 2
    scale = float(2 ** level)
    step = np.array([[scale, 0.0, 0.0, 0.5 * (scale - 1.0)], [0.0, scale, 0.0, 0.5 * (scale - 1.0)],
                     [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    return m @ step


def pyramid_camera(camera, level):
    """The pinhole ``(fx, fy, cx, cy, skew)`` of pyramid level ``level`` (see the module text)."""
    level = _level(level)
    try:
        camera = np.asarray(camera, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise TypeError('camera must be a sequence of numbers, got %r' % (camera,))
    if camera.size != 5:
        raise ValueError('camera must hold 5 values (fx, fy, cx, cy, skew), got %d' % camera.size)
    fx, fy, cx, cy, skew = camera.tolist()
    for _ in range(level):
        fx, fy, cx, cy, skew = fx / 2, fy / 2, (cx - 0.5) / 2, (cy - 0.5) / 2, skew / 2
    return (fx, fy, cx, cy, skew)


def check_levels(levels, height, width):
    """``levels`` as an int, after the checks ``disparity_pyramid`` makes of it against the frame's size."""
    levels = _level(levels, 'levels', 1)
    if levels > 31 or (height >> (levels - 1)) < 1 or (width >> (levels - 1)) < 1:
        raise ValueError('levels = %d leaves no pixel of a %d x %d frame at level %d' % (levels, width, height, levels - 1))
    return levels


def check_max_difference(max_difference):
    try:
        max_difference = float(max_difference)
    except (TypeError, ValueError):
        raise TypeError('max_difference must be a number, got %r' % (max_difference,))
    if not (max_difference >= 0.0 and math.isfinite(max_difference)):
        raise ValueError('max_difference must be finite and >= 0, got %r' % (max_difference,))
    return max_difference


def launches(levels):
    """The launches a pyramid of ``levels`` levels takes."""
    return (levels - 1 + LEVELS_PER_LAUNCH - 1) // LEVELS_PER_LAUNCH


def disparity_pyramid(disparity, levels, max_difference, valid=None, confidence=None, min_confidence=0.0):
    """disparity [B, H, W] float32 on the GPU -> the list of its ``levels`` pyramid levels: see the module text."""
    # what can be judged without a GPU comes first
    if not isinstance(disparity, torch.Tensor):
        raise TypeError('disparity must be a torch.Tensor')
    if disparity.dtype != torch.float32:
        raise TypeError('disparity must be float32, got %s' % (disparity.dtype,))
    if disparity.dim() != 3:
        raise ValueError('disparity must have 3 dimensions, got %d' % disparity.dim())
    shape = tuple(disparity.shape)
    if 0 in shape:
        raise ValueError('disparity_pyramid: empty input %s' % (shape,))
    batch, height, width = shape
    if batch * height * width > 2 ** 31 - 1:
        raise ValueError('B * H * W = %d does not fit 32-bit indices' % (batch * height * width))
    levels = check_levels(levels, height, width)
    max_difference = check_max_difference(max_difference)
    if valid is not None:
        if not isinstance(valid, torch.Tensor):
            raise TypeError('valid must be a torch.Tensor')
        if valid.dtype not in (torch.bool, torch.uint8) or tuple(valid.shape) != shape:
            raise ValueError('valid must be torch.bool or torch.uint8 %s, got %s %s' % (shape, valid.dtype, tuple(valid.shape)))
    if confidence is not None:
        if not isinstance(confidence, torch.Tensor):
            raise TypeError('confidence must be a torch.Tensor')
        if confidence.dtype != torch.float32:
            raise TypeError('confidence must be float32, got %s' % (confidence.dtype,))
        if tuple(confidence.shape) != shape:
            raise ValueError('confidence %s and disparity %s differ in shape' % (tuple(confidence.shape), shape))
    try:
        min_confidence = float(min_confidence)
    except (TypeError, ValueError):
        raise TypeError('min_confidence must be a number, got %r' % (min_confidence,))
    if math.isnan(min_confidence):
        raise ValueError('min_confidence is NaN')
    # then where the tensors live
    d = _lib.require_gpu_tensor(disparity.detach(), 'disparity', 3)
    device = d.device
    if valid is not None:
        if not valid.is_cuda:
            raise RuntimeError('valid must live on an MI355X (cuda) device: the HIP path has no CPU fallback')
        valid = valid.contiguous()
    if confidence is not None:
        confidence = _lib.require_gpu_tensor(confidence.detach(), 'confidence', 3)
    for name, t in (('valid', valid), ('confidence', confidence)):
        if t is not None and t.device != device:
            raise ValueError('%s and disparity live on different devices' % name)
    pyramid = [disparity if d.data_ptr() == disparity.data_ptr() else d]
    if levels == 1:
        return pyramid
    lib = _lib.load()
    with torch.cuda.device(device):
        stream = _lib.stream_handle(device)
        source, source_level = d, 0
        while source_level < levels - 1:
            count = min(LEVELS_PER_LAUNCH, levels - 1 - source_level)
            h, w = source.shape[1:]
            outputs = [torch.empty((batch, h >> k, w >> k), dtype=torch.float32, device=device)
                       for k in range(1, count + 1)]
            pointers = (ctypes.c_void_p * count)(*[t.data_ptr() for t in outputs])
            first = source_level == 0
            _lib.check(lib.pds_disparity_pyramid_fwd(
                _lib.ptr(source), None if valid is None or not first else _lib.ptr(valid),
                None if confidence is None or not first else _lib.ptr(confidence), min_confidence, max_difference,
                pointers, count, source_level, batch, h, w, stream), 'pds_disparity_pyramid_fwd')
            pyramid += outputs
            source, source_level = outputs[-1], source_level + count
    return pyramid


INTENSITY_LEVELS = 4    # csrc/common.hpp: kIntensityLevels, level 0 included
INTENSITY_LAYOUTS = {'nchw': 0, 'nhwc': 2}   # float32 [B, 3, H, W] / float32 [B, H, W, 3]; uint8 is always [B, H, W, 3]


def intensity_layout(image, layout=None):
    """``image`` -> (the ``image_layout`` of ``pds_intensity_pyramid_fwd``, (B, H, W)); judged without a GPU.  uint8
    [B, H, W, 3] -> 1 and float32 [B, 3, H, W] -> 0, told apart as ``tsdf_color.image_layout`` does; float32 [B, H, W, 3],
    the layout of ``ColorRaycast.colors``, -> 2 with ``layout='nhwc'`` (``'nchw'`` names the other float layout; without
    ``layout`` a float32 image is [B, 3, H, W] where its shape allows and [B, H, W, 3] otherwise, so only a [B, 3, H, 3]
    image of colours needs the keyword)."""
    if not isinstance(image, torch.Tensor):
        raise TypeError('image must be a torch.Tensor')
    if layout is not None and layout not in INTENSITY_LAYOUTS:
        raise ValueError("layout must be None, 'nchw' or 'nhwc', got %r" % (layout,))
    if image.dtype == torch.uint8:
        if layout == 'nchw' or image.dim() != 4 or image.shape[-1] != 3:
            raise ValueError('a uint8 image must be [B, H, W, 3], got %s' % (tuple(image.shape),))
        return 1, tuple(image.shape[:3])
    if image.dtype != torch.float32:
        raise TypeError('image must be uint8 [B, H, W, 3], float32 [B, 3, H, W] or float32 [B, H, W, 3], got %s' % (image.dtype,))
    if image.dim() != 4:
        raise ValueError('a float32 image must be [B, 3, H, W] or [B, H, W, 3], got %s' % (tuple(image.shape),))
    first, last = image.shape[1] == 3, image.shape[-1] == 3
    if layout is None:   # (a shape that fits both is [B, 3, H, W], as ``tsdf_color.image_layout`` takes it)
        layout = 'nchw' if first else 'nhwc'
    if not (first if layout == 'nchw' else last):
        raise ValueError('a float32 image must be [B, 3, H, W] or [B, H, W, 3], got %s' % (tuple(image.shape),))
    if layout == 'nchw':
        return 0, (image.shape[0],) + tuple(image.shape[2:])
    return 2, tuple(image.shape[:3])


def intensity_pyramid(image, levels=1, layout=None):
    """The luma of ``image`` and its halvings -> a list of ``levels`` float32 tensors, ``[l]`` [B, H >> l, W >> l]
    (``pds_intensity_pyramid_fwd``, one launch): the images of photometric tracking.

    ``image``: uint8 [B, H, W, 3], float32 [B, 3, H, W] or float32 [B, H, W, 3] (see ``intensity_layout`` for ``layout``);
    values are not rescaled.  Level 0 is ``fmaf(0.299f, c0, fmaf(0.587f, c1, 0.114f * c2))``, level l + 1 is
    ``((a00 + a01) + (a10 + a11)) * 0.25f`` over the four children, in fp32 without contraction; NaN propagates.  Sizes
    floor and a last odd row or column is dropped; pixel centres follow ``disparity_pyramid`` (2 x' + 0.5), so
    ``pyramid_matrix`` / ``pyramid_camera`` apply unchanged.  ``1 <= levels <= 4`` and ``H >> (levels - 1) >= 1``,
    ``W >> (levels - 1) >= 1``.  No atomics, no workspace, the current stream, no autograd, no host synchronisation; the
    same bits on every run and stream.  There is no CPU fallback."""
    code, shape = intensity_layout(image, layout)
    if 0 in shape:
        raise ValueError('intensity_pyramid: empty input %s' % (tuple(image.shape),))
    batch, height, width = shape
    if batch * height * width > 2 ** 31 - 1:
        raise ValueError('B * H * W = %d does not fit 32-bit indices' % (batch * height * width))
    levels = check_levels(levels, height, width)
    if levels > INTENSITY_LEVELS:
        raise ValueError('levels must be in 1 .. %d, got %d' % (INTENSITY_LEVELS, levels))
    if not image.is_cuda:
        raise RuntimeError('image must live on an MI355X (cuda) device: the HIP path has no CPU fallback')
    image = image.detach().contiguous()
    device = image.device
    outputs = [torch.empty((batch, height >> l, width >> l), dtype=torch.float32, device=device) for l in range(levels)]
    pointers = (ctypes.c_void_p * levels)(*[t.data_ptr() for t in outputs])
    lib = _lib.load()
    with torch.cuda.device(device):
        _lib.check(lib.pds_intensity_pyramid_fwd(_lib.ptr(image), code, pointers, levels, batch, height, width,
                                                 _lib.stream_handle(device)), 'pds_intensity_pyramid_fwd')
    return outputs
