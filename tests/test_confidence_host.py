"""CPU: the confidence entry points (pds_subpixel_map_confidence_fwd, pds_regularization_subpixel_map_confidence_fwd)
are declared, exported and bound, validate their arguments without a GPU, and the Python surface refuses what it
cannot run."""
import ctypes

import pytest
import torch

import practicaldeepstereo_nips2018_amd as pds
from practicaldeepstereo_nips2018_amd import _lib

NEW_SYMBOLS = ['pds_subpixel_map_confidence_fwd', 'pds_regularization_subpixel_map_confidence_fwd']


def test_confidence_symbols_declared_exported_and_bound(hip_library):
    header = open(_lib.HEADER_PATH).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + '(' in header, name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert hip_library.pds_abi_version() == 7


def test_standalone_confidence_validation_needs_no_gpu(hip_library):
    lib = hip_library
    assert lib.pds_subpixel_map_confidence_fwd(None, None, None, 1, 5, 1, 1, 2, 1, None) != 0
    assert b'null' in lib.pds_last_error()
    fake = ctypes.c_void_p(8)   # never dereferenced: every call below fails its checks first
    assert lib.pds_subpixel_map_confidence_fwd(fake, fake, None, 1, 5, 1, 1, 2, 1, None) != 0
    assert b'null' in lib.pds_last_error()
    assert lib.pds_subpixel_map_confidence_fwd(fake, fake, fake, 1, 5, 1, 1, 3, 2, None) != 0
    assert b'bad window/step' in lib.pds_last_error()
    assert lib.pds_subpixel_map_confidence_fwd(fake, fake, fake, 1, 5, 1, 1, 2, 0, None) != 0
    assert b'bad window/step' in lib.pds_last_error()
    assert lib.pds_subpixel_map_confidence_fwd(fake, fake, fake, 1, 0, 1, 1, 2, 1, None) != 0
    assert b'bad shape' in lib.pds_last_error()


def test_fused_confidence_validation_needs_no_gpu(hip_library):
    lib = hip_library
    params = pds.Regularization().native_params()
    fake = ctypes.c_void_p(8)
    nbytes = lib.pds_regularization_workspace_bytes(ctypes.byref(params), 1, 16, 16, 32)
    assert nbytes > 0

    def call(conf, hw, step, crop=(0, 0), ws_bytes=nbytes, d=16):
        return lib.pds_regularization_subpixel_map_confidence_fwd(
            ctypes.byref(params), fake, fake, fake, conf, 1, d, 16, 32, hw, step, crop[0], crop[1], fake, ws_bytes, 0,
            None)

    assert call(None, 4, 2) != 0 and b'null' in lib.pds_last_error()
    assert call(fake, 3, 2) != 0 and b'bad window/step' in lib.pds_last_error()
    assert call(fake, 4, 0) != 0 and b'bad window/step' in lib.pds_last_error()
    assert call(fake, 4, 2, crop=(64, 0)) != 0 and b'bad crop' in lib.pds_last_error()
    assert call(fake, 4, 2, ws_bytes=16) != 0 and b'workspace too small' in lib.pds_last_error()
    assert call(fake, 4, 2, d=12) != 0 and b'multiples of 16' in lib.pds_last_error()
    # the disparity entry point keeps its own messages
    assert lib.pds_regularization_subpixel_map_fwd(ctypes.byref(params), fake, fake, None, 1, 16, 16, 32, 4, 2, 0, 0,
                                                   fake, nbytes, 0, None) != 0
    assert lib.pds_last_error() == b'regularization_subpixel_map: null pointer'


def test_with_confidence_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pds.SubpixelMap().with_confidence(torch.zeros(1, 5, 2, 2))
    with pytest.raises(ValueError):
        pds.SubpixelMap(3, 2)


def test_forward_with_confidence_is_inference_only():
    net = pds.PdsNetwork.default(63).train()
    with pytest.raises(RuntimeError, match='inference only'):
        net.forward_with_confidence(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))
