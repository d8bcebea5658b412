"""CPU: the entry points of the right view and the left-right consistency check (pds_embedding_mirrored_fwd,
pds_regularization_subpixel_map_mirrored_fwd, pds_left_right_check_fwd) are declared, exported and bound, validate their
arguments without a GPU, and the Python surface refuses what it cannot run."""
import ctypes
import math

import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib

NEW_SYMBOLS = ['pds_embedding_mirrored_fwd', 'pds_regularization_subpixel_map_mirrored_fwd',
               'pds_left_right_check_fwd']


def test_left_right_symbols_declared_exported_and_bound(hip_library):
    header = open(_lib.HEADER_PATH).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + '(' in header, name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert hip_library.pds_abi_version() == 7


def test_left_right_check_validation_needs_no_gpu(hip_library):
    lib = hip_library
    a, b, m, n, f, g = [ctypes.c_void_p(8 * k) for k in range(1, 7)]   # never dereferenced

    def call(*args, shape=(1, 2, 3), md=1.0):
        return lib.pds_left_right_check_fwd(*args, *shape, md, None)

    assert call(None, b, m, n, f, g) != 0 and b'null pointer' in lib.pds_last_error()
    assert call(a, None, m, n, f, g) != 0 and b'null pointer' in lib.pds_last_error()
    assert call(a, b, None, n, f, g) != 0 and b'null pointer' in lib.pds_last_error()
    assert call(a, b, m, None, f, g) != 0 and b'null pointer' in lib.pds_last_error()
    for shape in [(0, 2, 3), (1, 0, 3), (1, 2, 0), (-1, 2, 3), (1, 2, 1 << 24), (1 << 16, 1 << 16, 3)]:
        assert call(a, b, m, n, f, g, shape=shape) != 0 and b'bad shape' in lib.pds_last_error(), shape
    for md in [-1.0, -1e-30, math.nan, math.inf, -math.inf]:
        assert call(a, b, m, n, f, g, md=md) != 0 and b'max_difference' in lib.pds_last_error(), md
    assert call(a, b, m, n, a, g) != 0 and b'alias' in lib.pds_last_error()
    assert call(a, b, m, n, f, b) != 0 and b'alias' in lib.pds_last_error()
    assert call(a, b, m, n, f, f) != 0 and b'alias' in lib.pds_last_error()


def test_mirrored_embedding_validation_needs_no_gpu(hip_library):
    lib = hip_library
    params, keep = pds.Embedding().native_params()
    fake = ctypes.c_void_p(8)
    nbytes = lib.pds_embedding_workspace_bytes(ctypes.byref(params), 2, 32, 48, 0, 0)
    assert nbytes > 0

    def call(image=fake, h=32, ws_bytes=nbytes, top=0):
        return lib.pds_embedding_mirrored_fwd(ctypes.byref(params), image, fake, fake, 2, h, 48, top, 0, fake,
                                              ws_bytes, 0, None)

    assert call(image=None) != 0 and lib.pds_last_error() == b'embedding_mirrored: null pointer'
    assert call(h=0) != 0 and b'bad shape' in lib.pds_last_error()
    assert call(top=-1) != 0 and b'bad shape' in lib.pds_last_error()
    assert call(ws_bytes=16) != 0 and b'embedding_mirrored: workspace too small' in lib.pds_last_error()
    # the plain entry point keeps its own messages
    assert lib.pds_embedding_fwd(ctypes.byref(params), None, fake, fake, 2, 32, 48, 0, 0, fake, nbytes, 0, None) != 0
    assert lib.pds_last_error() == b'embedding: null pointer'
    del keep


def test_mirrored_fused_validation_needs_no_gpu(hip_library):
    lib = hip_library
    params = pds.Regularization().native_params()
    fake = ctypes.c_void_p(8)
    nbytes = lib.pds_regularization_workspace_bytes(ctypes.byref(params), 1, 16, 16, 32)
    assert nbytes > 0

    def call(disp, conf, hw, step, crop=(0, 0), ws_bytes=nbytes, d=16):
        return lib.pds_regularization_subpixel_map_mirrored_fwd(
            ctypes.byref(params), fake, fake, disp, conf, 1, d, 16, 32, hw, step, crop[0], crop[1], fake, ws_bytes, 0,
            None)

    assert call(None, fake, 4, 2) != 0 and b'null pointer' in lib.pds_last_error()
    assert call(fake, fake, 3, 2) != 0 and b'bad window/step' in lib.pds_last_error()
    assert call(fake, None, 4, 0) != 0 and b'bad window/step' in lib.pds_last_error()
    for crop in [(64, 0), (0, 128), (-1, 0), (0, -1)]:
        assert call(fake, None, 4, 2, crop=crop) != 0 and b'bad crop' in lib.pds_last_error(), crop
    assert call(fake, fake, 4, 2, ws_bytes=16) != 0 and b'workspace too small' in lib.pds_last_error()
    assert call(fake, None, 4, 2, d=12) != 0 and b'multiples of 16' in lib.pds_last_error()
    # a window of more than 4 taps per side takes the unfused path, which cannot fold the mirror (nor a crop)
    assert call(fake, None, 12, 2) != 0 and b'mirror is only folded into the fused kernel' in lib.pds_last_error()
    assert call(fake, None, 12, 2, crop=(1, 0)) != 0 and b'crop is only folded' in lib.pds_last_error()
    assert lib.pds_last_error().startswith(b'regularization_subpixel_map_mirrored:')


def test_left_right_check_python_errors():
    ok = torch.zeros(1, 4, 5)
    with pytest.raises(ValueError, match='differ in shape'):
        pds.left_right_check(ok, torch.zeros(1, 4, 6))
    with pytest.raises(ValueError, match='dimensions'):
        pds.left_right_check(torch.zeros(4, 5), torch.zeros(4, 5))
    with pytest.raises(ValueError, match='dimensions'):
        pds.left_right_check(torch.zeros(1, 1, 4, 5), torch.zeros(1, 1, 4, 5))
    for md in [-0.5, math.nan, math.inf]:
        with pytest.raises(ValueError, match='max_difference'):
            pds.left_right_check(ok, ok, max_difference=md)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pds.left_right_check(ok, ok)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pds.left_right_check(ok, ok, max_difference=0.0, fill=True)


def test_right_view_is_inference_only():
    net = pds.PdsNetwork.default(63).train()
    images = torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match='inference only'):
        net.forward_right(*images)
    with pytest.raises(RuntimeError, match='inference only'):
        net.forward_left_right(*images)
    net.eval()
    with pytest.raises(ValueError, match='max_difference'):
        net.forward_left_right(*images, max_difference=-1.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net.forward_right(*images)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net.forward_left_right(*images)


def test_mirrored_embedding_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pds.Embedding().forward_padded(torch.zeros(1, 3, 16, 16), 0, 0, mirror=True)
