"""Frame metrics of the reference's scoring script (``EEG2Video/40_class_run_metrics.py:190-233``) on the device: the same names and
signatures -- ``channel_last``, ``ssim_metric``, ``mse_metric``, ``ssim_score_only``, ``mse_score_only`` -- over ``Engine.frame_metrics``
(``e2v_frame_metrics``: skimage's ``structural_similarity(data_range=255, channel_axis=-1)`` and ``mse_loss(img1 / 255, img2 / 255)``,
one launch per clip instead of one host call per frame).  The classifier metrics of that script (``img_classify_metric``,
``video_classify_metric``, CLIP score) need hub models and are not here.

Every function takes an ``engine=`` keyword; by default one ``Engine()`` without weights is made on first use and kept.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

_engine = None


def _default_engine():
    global _engine
    if _engine is None:
        from .engine import Engine
        _engine = Engine()
    return _engine


def channel_last(img):
    """``[c,h,w]`` -> ``[h,w,c]``, ``[f,c,h,w]`` -> ``[f,h,w,c]``; an array whose last axis is 3 is returned as it is."""
    if img.shape[-1] == 3:
        return img
    if len(img.shape) == 3:
        return np.transpose(img, (1, 2, 0))
    if len(img.shape) == 4:
        return np.transpose(img, (0, 2, 3, 1))
    raise ValueError(f"img shape should be 3 or 4, but got {len(img.shape)}")


def _frames(x) -> torch.Tensor:
    """``[f,h,w,c]`` (or one image ``[h,w,c]``) pixel values 0..255 -> a uint8 tensor ``[f,h,w,c]``"""
    a = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)
    if a.ndim == 3:
        a = a[None]
    if a.ndim != 4:
        raise ValueError(f"expected [f,h,w,c] frames or one [h,w,c] image, got shape {a.shape}")
    if a.dtype != np.uint8:
        a = a.astype(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(a))


def _scores(pred, gt, engine) -> Tuple[np.ndarray, np.ndarray]:
    eng = engine if engine is not None else _default_engine()
    ssim, mse = eng.frame_metrics(_frames(pred), _frames(gt), a_channels_last=True, b_channels_last=True)
    return ssim[0].cpu().numpy().astype(np.float64), mse[0].cpu().numpy().astype(np.float64)


def ssim_metric(img1, img2, engine=None) -> float:
    """``structural_similarity(img1, img2, data_range=255, channel_axis=-1)`` of two ``[h,w,c]`` uint8 images"""
    return float(_scores(img1, img2, engine)[0][0])


def mse_metric(img1, img2, engine=None) -> float:
    """``mse_loss(img1 / 255, img2 / 255)`` of two uint8 images"""
    return float(_scores(channel_last(np.asarray(img1)), channel_last(np.asarray(img2)), engine)[1][0])


def ssim_score_only(pred_videos, gt_videos, engine=None, **kwargs) -> Tuple[float, float]:
    """``[f,h,w,3]`` or ``[f,c,h,w]`` uint8 clips -> (mean, std) of the per-frame SSIM"""
    s = _scores(channel_last(np.asarray(pred_videos)), channel_last(np.asarray(gt_videos)), engine)[0]
    return np.mean(s), np.std(s)


def mse_score_only(pred_videos, gt_videos, engine=None, **kwargs) -> Tuple[float, float]:
    """``[f,h,w,3]`` or ``[f,c,h,w]`` uint8 clips -> (mean, std) of the per-frame MSE of the pixel values / 255"""
    s = _scores(channel_last(np.asarray(pred_videos)), channel_last(np.asarray(gt_videos)), engine)[1]
    return np.mean(s), np.std(s)
