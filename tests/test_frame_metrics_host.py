"""CPU: the frame metrics (``e2v_frame_metrics``; the reference's ``ssim_metric`` / ``mse_metric``, 40_class_run_metrics.py:229-233) as
far as a machine without a GPU reaches:

* the float64 restatement of skimage's algorithm (tests/frame_metrics_restatement.py) is pinned by closed forms;
* the integer-moment fp32 arithmetic the C header documents, emulated in numpy, stays within 1e-6 absolute of the restatement --
  the bound the GPU test (tests/test_hip_frame_metrics.py) holds the kernel to.  The emulation's terms carry one fp32 rounding each
  (2^-24 relative) and S two more, on values of at most 1: about 3e-7 per position before averaging; 1e-6 leaves room for the
  worst position to be the only one (the 7x7 image);
* the argument checks of the entry point on a host-only context, in the documented order."""
import ctypes as C

import numpy as np
import pytest

from eeg2video_amd import _lib
from frame_metrics_restatement import C1, KINDS, image_pair, mse, mse_exact, quantise, ssim, ssim_emulated

SIZES = [(7, 7), (9, 11), (24, 40), (288, 512)]


# ---- anchors of the restatement ------------------------------------------------------------------------------------------------
def test_identical_images_score_one_and_zero():
    a, b = image_pair("identical", 24, 40, 3)
    assert ssim(a, b) == pytest.approx(1.0, abs=1e-12) and mse(a, b) == 0.0
    assert ssim_emulated(a, b) == np.float32(1.0) and mse_exact(a, b) == np.float32(0.0)


def test_constant_pair_has_a_closed_form():
    a, b = image_pair("constant", 9, 11, 3)
    want = (2 * 254 * 255 + C1) / (254 ** 2 + 255 ** 2 + C1)
    assert abs(want - 0.99999228) < 1e-8
    assert ssim(a, b) == pytest.approx(want, abs=1e-9)
    assert mse(a, b) == pytest.approx(1.0 / 65025, rel=1e-12)
    assert mse_exact(a, b) == np.float32(1.0 / 65025)


@pytest.mark.parametrize("d", [1, 37, 255])
def test_one_differing_pixel_gives_the_closed_form_mse(d):
    a = np.zeros((9, 11, 3), np.uint8)
    b = a.copy()
    b[4, 5, 1] = d
    assert mse(a, b) == pytest.approx(d * d / (65025 * 3 * 9 * 11), rel=1e-12)
    assert mse_exact(a, b) == np.float32(np.float64(d * d) / np.float64(65025 * 3 * 9 * 11))


def test_both_metrics_are_symmetric():
    a, b = image_pair("noise", 24, 40, 3)
    assert ssim(a, b) == ssim(b, a) and mse(a, b) == mse(b, a)
    assert ssim_emulated(a, b) == ssim_emulated(b, a)


def test_quantisation_is_the_truncation_of_frames_to_uint8():
    x = np.array([0.0, 1.0, 0.999999, 1.0 / 255.0, 0.5, -0.5, 1.5, np.nan, -np.inf, np.inf], np.float32)
    assert quantise(x).tolist() == [0, 255, 254, 1, 127, 0, 255, 0, 0, 255]
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal(quantise((u.astype(np.float32) + np.float32(0.5)) / np.float32(255.0)), u)


# ---- emulation against restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", KINDS)
def test_integer_moment_fp32_arithmetic_stays_within_1e6_of_float64(kind, size):
    a, b = image_pair(kind, size[0], size[1], 3)
    err = abs(float(ssim_emulated(a, b)) - ssim(a, b))
    print(f"{kind} {size}: |emulated - restatement| = {err:.3e}")
    assert err <= 1e-6
    assert float(mse_exact(a, b)) == pytest.approx(mse(a, b), rel=1e-6)


# ---- the C ABI on a host-only context --------------------------------------------------------------------------------------------
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


def test_symbol_and_constants_are_bound(lib):
    assert lib.e2v_frame_metrics.argtypes == _lib.SIGNATURES["e2v_frame_metrics"][1]
    assert (_lib.E2V_FRAMES_F32, _lib.E2V_FRAMES_U8, _lib.E2V_FRAMES_CHANNELS_LAST) == (0, 1, 2)


def test_argument_errors_in_order_of_precedence(lib, host_ctx):
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    U8, CL = _lib.E2V_FRAMES_U8, _lib.E2V_FRAMES_CHANNELS_LAST

    def call(ctx=host_ctx, a=p, ka=0, b=p, kb=U8 | CL, n=1, F=1, Cc=3, H=7, W=7, ssim=p, mse=p):
        st = lib.e2v_frame_metrics(ctx, a, ka, b, kb, n, F, Cc, H, W, ssim, mse, None)
        return st, (lib.e2v_last_error(ctx) or b"") if ctx else b""

    # E2V_EINVAL first, each with every later check failing as well
    assert call(ctx=None)[0] == _lib.E2V_EINVAL
    assert call(a=None, n=0, Cc=9, H=3)[0] == _lib.E2V_EINVAL
    assert call(b=None, n=0, Cc=9, H=3)[0] == _lib.E2V_EINVAL
    assert call(ssim=None, mse=None, n=0, Cc=9, H=3)[0] == _lib.E2V_EINVAL
    assert call(ka=4, n=0)[0] == _lib.E2V_EINVAL and call(kb=-1, F=0)[0] == _lib.E2V_EINVAL
    assert call(kb=8 | U8, Cc=0)[0] == _lib.E2V_EINVAL
    # shapes: counts, then channels, then the window
    assert call(n=0, Cc=9, H=3)[0] == _lib.E2V_ESHAPE and call(F=-1, Cc=9, H=3)[0] == _lib.E2V_ESHAPE
    st, msg = call(Cc=0, H=3)
    assert st == _lib.E2V_ESHAPE and b"channels" in msg
    st, msg = call(Cc=5, W=6)
    assert st == _lib.E2V_ESHAPE and b"channels" in msg
    for kw in ({"H": 6}, {"W": 6}, {"H": 0, "W": 512}):
        st, msg = call(**kw)
        assert st == _lib.E2V_ESHAPE and b"window exceeds the image" in msg, kw
    # well-formed calls reach the host-only check, whatever the kinds and whichever output is asked for
    for kw in ({}, {"ka": U8, "kb": 0}, {"ka": CL, "kb": CL | U8}, {"ssim": None}, {"mse": None}, {"n": 5, "F": 6, "Cc": 4, "H": 288, "W": 512},
               {"Cc": 1}):
        st, msg = call(**kw)
        assert st == _lib.E2V_ESTATE and b"host-only" in msg, kw
    assert not buf.any()                 # nothing is ever written on a host-only context
