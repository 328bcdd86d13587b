"""CPU: the DE / PSD features' host side -- the numpy restatement (``tests/eeg_features_restatement.py``) against the fixture the
reference's own ``DE_PSD`` wrote (``tests/golden/glmnet_ref.npz``), the band arithmetic, and the argument checks of ``e2v_eeg_de_psd``
that need no GPU.  No GPU work.

Bounds: the fixture stores, per row length, the distance of the fp32 index-order restatement from ``DE_PSD`` (``d32_psd_<m>`` relative
per element, ``d32_de_<m>`` absolute); an fp32 computation is held to ten times that.  The float64 restatement has to sit at float64
rounding distance: 1e-12, four orders of magnitude under the fp32 bound and three above what it measures.
"""
import ctypes as C
import os

import numpy as np
import pytest

from eeg2video_amd import _lib
from eeg_features_restatement import band_bins, de_psd, windows_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROW_LENGTHS = (100, 200, 400)


def load_fixture():
    return np.load(os.path.join(GOLDEN, "glmnet_ref.npz"))


def maker():
    """the fixture's maker, for the weights and inputs it builds from their names"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_glmnet_golden", os.path.join(GOLDEN, "make_glmnet_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("m", ROW_LENGTHS)
def test_restatement_matches_the_reference_fixture(fx, m):
    """m = 400: the row is truncated to its first 200 windowed samples; m = 100: zero-padded -- pinned without a GPU"""
    rows = maker().de_psd_rows(m)
    de, psd = de_psd(rows, 200, np.float64)
    e_psd, e_de = np.max(np.abs(psd - fx[f"psd_{m}"]) / np.abs(fx[f"psd_{m}"])), np.max(np.abs(de - fx[f"de_{m}"]))
    print(f"m = {m}: float64 restatement vs DE_PSD: psd {e_psd:.2e} relative, de {e_de:.2e} absolute")
    assert e_psd <= 1e-12 and e_de <= 1e-12
    assert fx[f"de_{m}"].shape == (62, 5) and fx[f"de_{m}"].min() > 10          # band energies far from zero
    de32, psd32 = de_psd(rows, 200, np.float32)
    d_psd, d_de = float(fx[f"d32_psd_{m}"]), float(fx[f"d32_de_{m}"])
    assert 0 < d_psd < 1e-5 and 0 < d_de < 1e-4
    assert np.max(np.abs(psd32 - fx[f"psd_{m}"]) / np.abs(fx[f"psd_{m}"])) <= 10 * d_psd and np.max(np.abs(de32 - fx[f"de_{m}"])) <= 10 * d_de


def test_the_transform_length_is_200_whatever_the_row_length(fx):
    rows = maker().de_psd_rows(400)
    bound = 10 * float(fx["d32_psd_400"])
    # samples past the first 200 do not enter ...
    other = rows.copy()
    other[:, 200:] = 7.0
    assert np.array_equal(de_psd(other)[1], de_psd(rows)[1])
    # ... but the Hann row is the one of 400 samples: the first 200 samples as a row of their own miss the fixture by far
    short = de_psd(rows[:, :200])[1]
    assert np.max(np.abs(short - fx["psd_400"]) / fx["psd_400"]) > 1000 * bound
    # a 100-sample row is the 200-sample row with zeros behind it under the SAME 100-sample Hann row: not the 200-sample result
    r100 = maker().de_psd_rows(100)
    padded = np.concatenate([r100, np.zeros_like(r100)], axis=1)
    assert np.max(np.abs(de_psd(padded)[1] - fx["psd_100"]) / fx["psd_100"]) > 1000 * bound


def test_band_bins_are_the_reference_ranges():
    assert band_bins(200) == [(0, 3), (3, 7), (7, 13), (13, 30), (30, 98)]      # range(fStartNum - 1, fEndNum); the bands overlap
    assert band_bins(100) is None          # int(99 / 100 * 200) = 198: past the half spectrum
    assert band_bins(256) is None          # int(1 / 256 * 200) = 0: the reference would index bin -1
    assert band_bins(198)[-1] == (30, 99) and band_bins(197)[-1] == (30, 99) and band_bins(196) is None      # int(101.02) = 101
    assert band_bins(250) is None and band_bins(199)[0] == (0, 3)


def test_zero_row_and_windows():
    x = np.zeros((3, 50), np.float32)
    x[1] = np.arange(50)
    de, psd = de_psd(x)
    assert np.all(psd[[0, 2]] == 0) and np.all(np.isneginf(de[[0, 2]])) and np.all(np.isfinite(de[1]))
    seg = np.arange(2 * 3 * 400, dtype=np.float32).reshape(2, 3, 400)
    win = windows_of(seg, 100, 50)
    assert win.shape == (2, 7, 3, 100) and np.array_equal(win[1, 6, 2], seg[1, 2, 300:400])


def test_entry_argument_checks_without_a_gpu(lib):
    """E2V_EINVAL for what is wrong with the call comes first and needs no device; a call that is right ends at the host-only context"""
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    ctx = C.c_void_p()
    assert lib.e2v_create(C.byref(cfg), -1, C.byref(ctx)) == 0
    try:
        ok = dict(eeg=0x1000, cs=24800, ws=50, es=400, B=2, W=7, C=62, m=100, fs=200, mean=None, scale=None, de=0x2000, psd=0x3000)

        def call(**over):
            a = dict(ok, **over)
            return lib.e2v_eeg_de_psd(ctx, a["eeg"], a["cs"], a["ws"], a["es"], a["B"], a["W"], a["C"], a["m"], a["fs"], a["mean"], a["scale"],
                                      a["de"], a["psd"], None)
        for over in (dict(eeg=None), dict(de=None, psd=None), dict(mean=0x4000), dict(scale=0x4000), dict(eeg=0x1002), dict(de=0x2001),
                     dict(psd=0x3002), dict(mean=0x4001, scale=0x5000), dict(cs=-1), dict(ws=-1), dict(es=-1), dict(B=0), dict(W=0), dict(C=0),
                     dict(m=0), dict(m=65537), dict(fs=100), dict(fs=256), dict(fs=0), dict(fs=-200)):
            assert call(**over) == _lib.E2V_EINVAL, over
            assert lib.e2v_last_error(ctx).decode().startswith("e2v_eeg_de_psd:"), over
        assert call(fs=100) == _lib.E2V_EINVAL and "sampling rate 100" in lib.e2v_last_error(ctx).decode()
        # the order: the NULL input is reported before the bad rate, the bad rate before the host-only context
        assert call(eeg=None, fs=100) == _lib.E2V_EINVAL and "eeg is NULL" in lib.e2v_last_error(ctx).decode()
        for over in ({}, dict(de=None), dict(psd=None), dict(m=400, W=1, ws=0), dict(fs=198)):
            assert call(**over) == _lib.E2V_ESTATE and "host-only" in lib.e2v_last_error(ctx).decode(), over
        assert lib.e2v_eeg_de_psd(None, 0x1000, 0, 0, 0, 1, 1, 1, 1, 200, None, None, 0x2000, None, None) == _lib.E2V_EINVAL
    finally:
        lib.e2v_destroy(ctx)
