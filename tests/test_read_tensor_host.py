"""CPU: the C ABI of the weight read-back (``e2v_read_tensor``) as far as a host-only context reaches: the symbol, and every argument
error in its order of precedence -- each is answered before the host-only check, so a context without a GPU reports them.  The
UNet and VAE parts of the context are finalized by a dry run (``e2v_op_describe_dispatch``: bindings without device memory), which is
what lets the checks that depend on the kind of a tensor run here.  The arithmetic runs in tests/test_hip_read_tensor.py (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

from eeg2video_amd import _lib

F = _lib.FORM_BITS
CONV, NORM, LIN = b"conv_in.weight", b"conv_norm_out.weight", b"time_embedding.linear_1.weight"


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _host_ctx(lib):
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    ctx = C.c_void_p()
    assert lib.e2v_create(C.byref(cfg), -1, C.byref(ctx)) == 0
    return ctx


@pytest.fixture(scope="module")
def fresh_ctx(lib):
    ctx = _host_ctx(lib)
    yield ctx
    lib.e2v_destroy(ctx)


@pytest.fixture(scope="module")
def bound_ctx(lib):
    """host-only, UNet and VAE finalized by a dry run"""
    ctx = _host_ctx(lib)
    need = C.c_int64(0)
    assert lib.e2v_op_describe_dispatch(ctx, _lib.E2V_F32, 1, 2, 8, 8, 77, None, 0, C.byref(need)) == 0
    yield ctx
    lib.e2v_destroy(ctx)


def _shape_of(lib, ctx, key):
    shape, nd = (C.c_int64 * 4)(), C.c_int()
    for i in range(lib.e2v_num_expected_keys(ctx)):
        if lib.e2v_expected_key(ctx, i, shape, C.byref(nd)) == key:
            return [int(shape[d]) for d in range(nd.value)]
    raise KeyError(key)


def _call(lib, ctx, key, form=0, dtype=_lib.E2V_F32, shape=None, out=True, on_device=0, ndim=None):
    dims = _shape_of(lib, ctx, key) if shape is None else list(shape)
    buf = np.zeros(max(int(np.prod(dims)), 1), np.float32)
    st = lib.e2v_read_tensor(ctx, key, form, buf.ctypes.data_as(C.c_void_p) if out else None, dtype, on_device,
                             (C.c_int64 * max(len(dims), 1))(*dims), len(dims) if ndim is None else ndim, None)
    assert not buf.any()                 # nothing is ever written on a host-only context
    return st, lib.e2v_last_error(ctx) or b""


def test_symbol_is_exported_and_bound(lib):
    assert "e2v_read_tensor" in _lib.SIGNATURES
    assert lib.e2v_read_tensor.argtypes == _lib.SIGNATURES["e2v_read_tensor"][1]


def test_argument_errors_in_order_of_precedence(lib, bound_ctx):
    ctx = bound_ctx
    shape = (C.c_int64 * 4)(*_shape_of(lib, ctx, CONV))
    x = np.zeros(8, np.float32).ctypes.data_as(C.c_void_p)
    # null arguments, each with everything else wrong as well
    assert lib.e2v_read_tensor(None, CONV, 0, x, _lib.E2V_F32, 0, shape, 4, None) == _lib.E2V_EINVAL
    assert lib.e2v_read_tensor(ctx, None, 3, x, _lib.E2V_F32X3, 0, shape, 4, None) == _lib.E2V_EINVAL
    assert lib.e2v_read_tensor(ctx, b"no.such.key", 3, None, _lib.E2V_F32X3, 0, shape, 4, None) == _lib.E2V_EINVAL
    assert lib.e2v_read_tensor(ctx, b"no.such.key", 3, x, _lib.E2V_F32X3, 0, None, 4, None) == _lib.E2V_EINVAL
    # unknown key, before shape, dtype and form
    assert _call(lib, ctx, b"no.such.key", form=3, dtype=_lib.E2V_F32X3, shape=[5])[0] == _lib.E2V_ENOWEIGHT
    # wrong shape or ndim, before dtype and form
    good = _shape_of(lib, ctx, CONV)
    assert _call(lib, ctx, CONV, form=3, dtype=_lib.E2V_F32X3, shape=good[:3] + [1])[0] == _lib.E2V_ENOWEIGHT
    assert _call(lib, ctx, CONV, form=3, dtype=_lib.E2V_F32X3, shape=good[:3])[0] == _lib.E2V_ENOWEIGHT
    assert _call(lib, ctx, CONV, form=3, dtype=_lib.E2V_F32X3, shape=good, ndim=3)[0] == _lib.E2V_ENOWEIGHT
    # dtype, before form
    assert _call(lib, ctx, CONV, form=3, dtype=_lib.E2V_F32X3)[0] == _lib.E2V_EINVAL
    assert _call(lib, ctx, CONV, form=3, dtype=7)[0] == _lib.E2V_EINVAL
    # form: two bits, an unknown bit, a form with no index-map inverse
    assert _call(lib, ctx, LIN, form=F["fp32"] | F["bf16"])[0] == _lib.E2V_EINVAL
    assert _call(lib, ctx, LIN, form=1 << 11)[0] == _lib.E2V_EINVAL
    assert _call(lib, ctx, LIN, form=-1)[0] == _lib.E2V_EINVAL
    for name in ("conv_direct32", "wino2", "wino4", "bf16_up2", "f16_up2", "wino2_x3", "wino4_x3"):
        assert _call(lib, ctx, CONV, form=F[name])[0] == _lib.E2V_EINVAL, name
    # a 16-bit or X3 form of a RAW or CONV binding
    for key in (NORM, CONV, b"conv_in.bias"):
        for name in ("bf16", "fp16", "x3"):
            assert _call(lib, ctx, key, form=F[name])[0] == _lib.E2V_EINVAL, (key, name)


def test_well_formed_call_is_refused_as_host_only(lib, bound_ctx):
    for key in (CONV, NORM, LIN, b"vae.decoder.mid_block.attentions.0.query.weight"):
        for form in (0, F["fp32"]):
            for dtype in (_lib.E2V_F32, _lib.E2V_BF16, _lib.E2V_F16):
                for on_device in (0, 1):
                    st, err = _call(lib, bound_ctx, key, form=form, dtype=dtype, on_device=on_device)
                    assert st == _lib.E2V_ESTATE and b"host-only" in err, (key, form, dtype, err)
    st, err = _call(lib, bound_ctx, LIN, form=F["bf16"])        # the dry run's linears carry their bf16 copy
    assert st == _lib.E2V_ESTATE and b"host-only" in err


def test_form_not_built_and_part_not_finalized(lib, bound_ctx, fresh_ctx):
    st, err = _call(lib, bound_ctx, LIN, form=F["fp16"])        # the IEEE-half copy is built on first use, the x3 planes in that mode
    assert st == _lib.E2V_ESTATE and b"form not built" in err
    st, err = _call(lib, bound_ctx, LIN, form=F["x3"])
    assert st == _lib.E2V_ESTATE and b"form not built" in err
    st, err = _call(lib, bound_ctx, b"semantic.mlp.0.weight")   # (the dry run finalizes UNet and VAE only)
    assert st == _lib.E2V_ESTATE and b"not finalized" in err
    st, err = _call(lib, fresh_ctx, CONV)
    assert st == _lib.E2V_ESTATE and b"not finalized" in err
    assert _call(lib, fresh_ctx, CONV, form=F["wino4"])[0] == _lib.E2V_EINVAL      # the call's own errors still come first
