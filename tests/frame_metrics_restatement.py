"""Restatement of the frame metrics the reference reports (``EEG2Video/40_class_run_metrics.py:229-233``), numpy + scipy, float64 -- the
yardstick of tests/test_frame_metrics_host.py (CPU) and tests/test_hip_frame_metrics.py (GPU).  skimage is not a dependency of this
build, so its algorithm is restated here and pinned by closed forms in the host test:

``structural_similarity(img1, img2, data_range=255, channel_axis=-1)`` with skimage's defaults -- per channel: 7x7 uniform filter of
x, y, xx, yy, xy; sample covariance (NP / (NP - 1)); K1 = 0.01, K2 = 0.03; S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)
(vx + vy + C2)); the map cropped by (7 - 1) // 2 = 3 on every side and averaged; then the mean over the channels -- and
``mse_loss(img1 / 255, img2 / 255)`` in float64.

``ssim_emulated`` restates the arithmetic ``e2v_frame_metrics`` documents (include/eeg2video_hip.h): exact integer window moments, the
four terms and S in fp32, the sum in float64."""
import numpy as np
from scipy.ndimage import uniform_filter

WIN, K1, K2, L = 7, 0.01, 0.03, 255.0
C1, C2 = (K1 * L) ** 2, (K2 * L) ** 2                      # 6.5025, 58.5225


def quantise(x):
    """fp32 frames -> the bytes e2v_frame_metrics scores: (uint8)(min(max(x, 0), 1) * 255.f), truncation, NaN -> 0"""
    x = np.asarray(x, np.float32)
    x = np.where(x > 0, x, np.float32(0))
    x = np.where(x < 1, x, np.float32(1))
    return (x * np.float32(255.0)).astype(np.uint8)


def ssim(img1, img2):
    """two uint8 ``[H,W,C]`` images -> SSIM (float64)"""
    assert img1.shape == img2.shape and img1.ndim == 3 and min(img1.shape[:2]) >= WIN
    npix = WIN * WIN
    cov_norm = npix / (npix - 1.0)
    pad = (WIN - 1) // 2
    out = []
    for c in range(img1.shape[2]):
        x, y = img1[:, :, c].astype(np.float64), img2[:, :, c].astype(np.float64)
        ux, uy = uniform_filter(x, size=WIN), uniform_filter(y, size=WIN)
        uxx, uyy, uxy = uniform_filter(x * x, size=WIN), uniform_filter(y * y, size=WIN), uniform_filter(x * y, size=WIN)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        out.append(s[pad:s.shape[0] - pad, pad:s.shape[1] - pad].mean(dtype=np.float64))
    return float(np.mean(out))


def mse(img1, img2):
    """two uint8 arrays of one shape -> mean((img1 / 255 - img2 / 255)^2) in float64"""
    d = img1.astype(np.float64) / 255.0 - img2.astype(np.float64) / 255.0
    return float(np.mean(d * d))


def mse_exact(img1, img2):
    """the exact integer sum divided once: what e2v_frame_metrics rounds to fp32"""
    d = img1.astype(np.int64) - img2.astype(np.int64)
    return np.float32(np.float64(int((d * d).sum())) / np.float64(65025 * img1.size))


def _window_sums(a):
    """``[H,W]`` int64 -> the 7x7 window sums ``[H-6,W-6]``, exact"""
    c = np.cumsum(np.cumsum(np.pad(a, ((1, 0), (1, 0))), 0), 1)
    return c[WIN:, WIN:] - c[:-WIN, WIN:] - c[WIN:, :-WIN] + c[:-WIN, :-WIN]


def ssim_emulated(img1, img2):
    """the integer-moment fp32 arithmetic of e2v_frame_metrics: two uint8 ``[H,W,C]`` images -> fp32 SSIM"""
    n = WIN * WIN
    f32 = np.float32
    total, count = 0.0, 0
    for c in range(img1.shape[2]):
        x, y = img1[:, :, c].astype(np.int64), img2[:, :, c].astype(np.int64)
        sx, sy, sxx, syy, sxy = _window_sums(x), _window_sums(y), _window_sums(x * x), _window_sums(y * y), _window_sums(x * y)
        assert max(np.abs(v).max() for v in (n * sxy, n * (sxx + syy), 2 * sx * sy)) < 2 ** 31
        a1 = (2 * sx * sy).astype(f32) / f32(n * n) + f32(C1)
        a2 = (2 * (n * sxy - sx * sy)).astype(f32) / f32(n * (n - 1)) + f32(C2)
        b1 = (sx * sx + sy * sy).astype(f32) / f32(n * n) + f32(C1)
        b2 = (n * (sxx + syy) - sx * sx - sy * sy).astype(f32) / f32(n * (n - 1)) + f32(C2)
        s = (a1 * a2) / (b1 * b2)
        assert s.dtype == np.float32
        total += float(s.astype(np.float64).sum())
        count += s.size
    return np.float32(total / count)


def clip_scores(a, b):
    """two uint8 clips ``[F,H,W,C]`` -> per-frame (ssim, mse) float64 arrays by the restatement"""
    return (np.array([ssim(x, y) for x, y in zip(a, b)]), np.array([mse(x, y) for x, y in zip(a, b)]))


# ---- the images both test files score ------------------------------------------------------------------------------------------
def image_pair(kind, h, w, c, seed=0):
    """two uint8 ``[h,w,c]`` images of one of the kinds the tests sweep"""
    rng = np.random.default_rng(1000 * seed + 7 * h + w + c)
    noise = lambda: rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == "noise":
        return noise(), noise()
    if kind == "gradient":                                   # a ramp plus small noise against the ramp plus other noise
        ramp = (np.add.outer(np.arange(h) * 3, np.arange(w) * 2)[:, :, None] + 40 * np.arange(c)) % 256
        mk = lambda: np.clip(ramp + rng.integers(-6, 7, (h, w, c)), 0, 255).astype(np.uint8)
        return mk(), mk()
    if kind == "constant":
        return np.full((h, w, c), 254, np.uint8), np.full((h, w, c), 255, np.uint8)
    if kind == "near_white":
        return (rng.integers(250, 256, (h, w, c), dtype=np.uint8), rng.integers(250, 256, (h, w, c), dtype=np.uint8))
    if kind == "inverted":
        a = noise()
        return a, (255 - a).astype(np.uint8)
    if kind == "identical":
        a = noise()
        return a, a.copy()
    raise ValueError(kind)


KINDS = ("noise", "gradient", "constant", "near_white", "inverted", "identical")
