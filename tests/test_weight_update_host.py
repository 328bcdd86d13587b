"""CPU: the C ABI of the in-place weight update (``e2v_update_tensor``, ``e2v_op_weight_forms``) as far as a host-only context
reaches: symbols, argument checks, call-order errors.  The arithmetic runs in tests/test_hip_weight_update.py (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

from eeg2video_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def host_ctx(lib):
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    ctx = C.c_void_p()
    assert lib.e2v_create(C.byref(cfg), -1, C.byref(ctx)) == 0
    yield ctx
    lib.e2v_destroy(ctx)


def _bias():
    x = np.zeros(4, np.float32)
    return x, x.ctypes.data_as(C.c_void_p), (C.c_int64 * 1)(4)


def test_new_symbols_are_exported_and_bound(lib):
    for name in ("e2v_update_tensor", "e2v_op_weight_forms"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert sorted(_lib.FORM_BITS.values()) == [1 << i for i in range(11)]


def test_host_only_context_refuses_updates(lib, host_ctx):
    x, p, shape = _bias()
    for on_device in (0, 1):
        assert lib.e2v_update_tensor(host_ctx, b"conv_in.bias", p, _lib.E2V_F32, on_device, shape, 1, None) == _lib.E2V_ESTATE
        assert b"host-only" in lib.e2v_last_error(host_ctx)
    mask = C.c_int(-1)
    assert lib.e2v_op_weight_forms(host_ctx, b"conv_in.bias", C.byref(mask)) == _lib.E2V_ESTATE
    assert mask.value == -1


def test_argument_checks_come_first(lib, host_ctx):
    x, p, shape = _bias()
    assert lib.e2v_update_tensor(None, b"conv_in.bias", p, _lib.E2V_F32, 0, shape, 1, None) == _lib.E2V_EINVAL
    assert lib.e2v_update_tensor(host_ctx, None, p, _lib.E2V_F32, 0, shape, 1, None) == _lib.E2V_EINVAL
    assert lib.e2v_update_tensor(host_ctx, b"conv_in.bias", None, _lib.E2V_F32, 0, shape, 1, None) == _lib.E2V_EINVAL
    assert lib.e2v_update_tensor(host_ctx, b"conv_in.bias", p, _lib.E2V_F32, 0, None, 1, None) == _lib.E2V_EINVAL
    assert lib.e2v_update_tensor(host_ctx, b"conv_in.bias", p, _lib.E2V_F32X3, 0, shape, 1, None) == _lib.E2V_EINVAL
    assert lib.e2v_update_tensor(host_ctx, b"conv_in.bias", p, 7, 0, shape, 1, None) == _lib.E2V_EINVAL
    mask = C.c_int(0)
    assert lib.e2v_op_weight_forms(None, b"conv_in.bias", C.byref(mask)) == _lib.E2V_EINVAL
    assert lib.e2v_op_weight_forms(host_ctx, None, C.byref(mask)) == _lib.E2V_EINVAL
    assert lib.e2v_op_weight_forms(host_ctx, b"conv_in.bias", None) == _lib.E2V_EINVAL


def test_load_tensor_bf16_gets_the_status_f32_gets(lib, host_ctx):
    """A host-only context accepts no load at all: bf16 must be turned away for THAT reason (as fp32 is), not as an unsupported type."""
    x, p, shape = _bias()
    st32 = lib.e2v_load_tensor(host_ctx, b"conv_in.bias", p, _lib.E2V_F32, shape, 1)
    h = np.zeros(4, np.uint16)
    st16 = lib.e2v_load_tensor(host_ctx, b"conv_in.bias", h.ctypes.data_as(C.c_void_p), _lib.E2V_BF16, shape, 1)
    assert st16 == st32 == _lib.E2V_ESTATE
