"""Frame metrics of the reference's scoring script (``EEG2Video/40_class_run_metrics.py:190-233``) on the device: the same names and
signatures -- ``channel_last``, ``ssim_metric``, ``mse_metric``, ``ssim_score_only``, ``mse_score_only`` -- over ``Engine.frame_metrics``
(``e2v_frame_metrics``: skimage's ``structural_similarity(data_range=255, channel_axis=-1)`` and ``mse_loss(img1 / 255, img2 / 255)``,
one launch per clip instead of one host call per frame) -- and its image N-way accuracy, ``n_way_top_k_acc`` and
``img_classify_metric`` (``:57-105``), over ``Engine.classify_frames`` (``e2v_image_classify``: the ViT classifier of every frame of a
clip in one call, fp32, instead of one fp16 forward per image), and its video N-way accuracy, ``video_classify_metric``
(``:108-142``), over ``Engine.classify_clips`` (``e2v_video_classify``: the VideoMAE classifier of all clips in one call), and its
CLIP score, ``clip_score`` / ``clip_score_only`` / ``n_way_scores`` (``:20-55,145-188``), over ``Engine.clip_embed`` and
``Engine.clip_similarity`` (``e2v_clip_embed``: the CLIP vision tower of every frame of a side in one call; ``e2v_clip_similarity``:
the cosine of every pair in one more -- instead of two fp16 forwards per comparison).

The frame metrics take an ``engine=`` keyword; by default one ``Engine()`` without weights is made on first use and kept.
``img_classify_metric``, ``video_classify_metric`` and the CLIP scores take a built model (``model=``) or a LOCAL checkpoint
directory (``cache_dir=``).
"""
from __future__ import annotations

from typing import List, Optional, Tuple, Union

import os

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


def n_way_top_k_acc(pred, class_id, n_way: int, num_trials: int = 40, top_k: int = 1) -> Tuple[float, float]:
    """``40_class_run_metrics.py:57-70``: ``num_trials`` times, ``n_way - 1`` distractor classes are drawn and the trial counts as
    correct when a ground-truth class is among the ``top_k`` of the picked ``pred`` values -> ``(accuracy, its binomial std)``.
    ``pred``: ``[classes]`` scores (tensor or array); ``class_id``: one id or several (the trial is correct if ANY of them is).
    The ``np.random.choice`` calls are the reference's, in its order, so a seeded run draws the same distractors; everything else is
    vectorised over the trials.  A ground truth is in the top ``top_k`` when fewer than ``top_k`` picked values are >= its own."""
    if isinstance(class_id, (int, np.integer)):
        class_id = [int(class_id)]
    p = np.asarray(pred.detach().cpu() if isinstance(pred, torch.Tensor) else pred).reshape(-1)
    ids = [int(i) for i in (class_id.detach().cpu().reshape(-1).tolist() if isinstance(class_id, torch.Tensor) else class_id)]
    pick_range = [i for i in np.arange(len(p)) if i not in ids]
    picked = np.stack([np.random.choice(pick_range, n_way - 1, replace=False) for _ in range(num_trials)])      # [trials, n_way - 1]
    beaten = (p[picked][:, None, :] >= p[ids][None, :, None]).sum(-1)                                           # [trials, ids]
    corrects = int((beaten < top_k).any(-1).sum())
    acc = corrects / num_trials
    return acc, np.sqrt(acc * (1 - acc) / num_trials)


_classifiers = {}


def _classifier(cache_dir: str, device):
    key = os.path.abspath(cache_dir)
    if key not in _classifiers:
        from .image_classifier import ViTForImageClassification
        index = torch.device(device).index if device is not None else None
        _classifiers[key] = ViTForImageClassification.from_pretrained(cache_dir, device=index or 0)
    return _classifiers[key]


def img_classify_metric(pred_videos, gt_videos, n_way: int = 50, num_trials: int = 100, top_k: int = 1, cache_dir: str = ".cache",
                        device: Optional[str] = "cuda", return_std: bool = False,
                        model=None) -> Union[List[float], Tuple[List[float], List[float]]]:
    """``40_class_run_metrics.py:72-105``: per frame, the N-way top-k accuracy of the generated frame's class probabilities against the
    three most likely classes of the ground-truth frame -> the list of accuracies (``return_std``: and the list of their stds).
    ``pred_videos`` / ``gt_videos``: ``[f,h,w,3]`` pixel values 0..255 (arrays or tensors, on the device or not).  ``model``: a built
    ``eeg2video_amd.image_classifier.ViTForImageClassification``; else ``cache_dir`` must be a LOCAL checkpoint directory of one (the
    reference names the hub model there; nothing is fetched here), loaded once per directory.  Each clip goes through the device in
    ONE ``classify_frames`` call -- not one forward per frame -- and only the probabilities and the top-3 indices come back."""
    assert n_way > top_k
    clf = model if model is not None else _classifier(cache_dir, device)
    pred = clf.classify(_frames(pred_videos), channels_last=True)[1].cpu().numpy()
    gt_ids = clf.classify(_frames(gt_videos), channels_last=True)[2].cpu().numpy()
    if len(pred) != len(gt_ids):
        raise ValueError(f"clips differ: {len(pred)} generated frames against {len(gt_ids)} ground-truth frames")
    acc_list, std_list = [], []
    for p, ids in zip(pred, gt_ids):
        acc, std = n_way_top_k_acc(p, [int(i) for i in ids], n_way, num_trials, top_k)
        acc_list.append(acc)
        std_list.append(std)
    if return_std:
        return acc_list, std_list
    return acc_list


_video_classifiers = {}


def _video_classifier(cache_dir: str, num_frames: int, device):
    key = (os.path.abspath(cache_dir), int(num_frames))
    if key not in _video_classifiers:
        from .video_classifier import VideoMAEForVideoClassification
        index = torch.device(device).index if device is not None else None
        _video_classifiers[key] = VideoMAEForVideoClassification.from_pretrained(cache_dir, num_frames=num_frames, device=index or 0)
    return _video_classifiers[key]


def _clips(x) -> torch.Tensor:
    """``[n,f,h,w,c]`` (or one clip ``[f,h,w,c]``) pixel values 0..255 -> a uint8 tensor ``[n,f,h,w,c]``"""
    a = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)
    if a.ndim == 4:
        a = a[None]
    if a.ndim != 5:
        raise ValueError(f"expected [n,f,h,w,c] clips or one [f,h,w,c] clip, got shape {a.shape}")
    if a.dtype != np.uint8:
        a = a.astype(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(a))


def video_classify_metric(pred_videos, gt_videos, n_way: int = 50, num_trials: int = 100, top_k: int = 1, num_frames: int = 6,
                          cache_dir: str = ".cache", device: Optional[str] = "cuda", return_std: bool = False,
                          model=None) -> Union[List[float], Tuple[List[float], List[float]]]:
    """``40_class_run_metrics.py:108-142``: per clip, the N-way top-k accuracy of the generated clip's class probabilities against the
    three most likely classes of the ground-truth clip -> the list of accuracies (``return_std``: and the list of their stds).
    ``pred_videos`` / ``gt_videos``: ``[n,f,h,w,3]`` pixel values 0..255 with ``f == num_frames`` (arrays or tensors, on the device or
    not).  ``model``: a built ``eeg2video_amd.video_classifier.VideoMAEForVideoClassification`` (its ``num_frames`` must be this call's);
    else ``cache_dir`` must be a LOCAL checkpoint directory of one (the reference names the hub model there; nothing is fetched here),
    loaded once per (directory, ``num_frames``).  All clips of a side go through the device in ONE ``classify_clips`` call; the trial
    loop then runs per clip in the reference's order -- ground truth's top 3, prediction's softmax, ``n_way_top_k_acc`` -- so a seeded
    run draws the reference's distractors."""
    assert n_way > top_k
    clf = model if model is not None else _video_classifier(cache_dir, num_frames, device)
    if clf.vcfg.num_frames != num_frames:
        raise ValueError(f"the classifier was built for num_frames={clf.vcfg.num_frames}, this call says {num_frames}")
    pred = clf.classify(_clips(pred_videos), channels_last=True)[1].cpu().numpy()
    gt_ids = clf.classify(_clips(gt_videos), channels_last=True)[2].cpu().numpy()
    if len(pred) != len(gt_ids):
        raise ValueError(f"{len(pred)} generated clips against {len(gt_ids)} ground-truth clips")
    acc_list, std_list = [], []
    for p, ids in zip(pred, gt_ids):
        acc, std = n_way_top_k_acc(p, [int(i) for i in ids], n_way, num_trials, top_k)
        acc_list.append(acc)
        std_list.append(std)
    if return_std:
        return acc_list, std_list
    return acc_list


_clip_models = {}


def _clip_model(cache_dir: str, device):
    key = os.path.abspath(cache_dir)
    if key not in _clip_models:
        from .clip_vision import CLIPVisionModelWithProjection
        index = torch.device(device).index if device is not None else None
        _clip_models[key] = CLIPVisionModelWithProjection.from_pretrained(cache_dir, device=index or 0)
    return _clip_models[key]


class clip_score:
    """``40_class_run_metrics.py:20-55``: ``clip_score(device, cache_dir)(img1, img2)`` -> the cosine similarity of the CLIP image
    embeddings of two ``[h,w,3]`` images of pixel values 0..255, a float.  ``model``: a built
    ``eeg2video_amd.clip_vision.CLIPVisionModelWithProjection``; else ``cache_dir`` must be a LOCAL checkpoint directory of one (the
    reference names the hub model there; nothing is fetched here), loaded once per directory.  fp32 where the reference runs fp16."""

    def __init__(self, device: Optional[str] = "cuda", cache_dir: str = ".cache", model=None):
        self.device = device
        self.clip_model = model if model is not None else _clip_model(cache_dir, device)

    def embed(self, images) -> torch.Tensor:
        """``[f,h,w,3]`` images (or one) -> ``image_embeds`` ``[f, D]`` on the device, one call"""
        return self.clip_model.embed(_frames(images), channels_last=True)

    def similarity(self, a: torch.Tensor, b: torch.Tensor, matrix: bool = False) -> torch.Tensor:
        return self.clip_model.engine.clip_similarity(a, b, matrix=matrix)

    @torch.no_grad()
    def __call__(self, img1, img2) -> float:
        return self.similarity(self.embed(img1), self.embed(img2)).item()


def clip_score_only(pred_videos, gt_videos, cache_dir: str = ".cache", device: Optional[str] = "cuda", model=None):
    """``40_class_run_metrics.py:176-188``: the mean over the frames of the CLIP score of a generated frame and its ground truth.
    ``pred_videos`` / ``gt_videos``: ``[f,h,w,3]`` pixel values 0..255.  Each side is embedded in ONE call, the ``f`` pair scores come
    from one more."""
    calc = clip_score(device, cache_dir, model)
    a, b = calc.embed(pred_videos), calc.embed(gt_videos)
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"{a.shape[0]} generated frames against {b.shape[0]} ground-truth frames")
    scores = [float(v) for v in calc.similarity(a, b).cpu().numpy()]
    return np.mean(scores)


def n_way_from_matrix(scores, n_way: int, top_k: int, num_trials: int) -> List[float]:
    """The trial loop of ``n_way_scores`` (``40_class_run_metrics.py:158-174``) over a matrix that already holds every score the
    loop could ask for: ``scores[i][j]`` is the score of generated image ``i`` against ground-truth image ``j`` (square).  Host
    arithmetic only.  The ``np.random.choice(len(rest), n_way - 1, replace=False)`` calls are the reference's, in its order, and index
    its ``rest`` (the ground truths without ``idx``: entry ``r`` is ground truth ``r`` below ``idx`` and ``r + 1`` from there on);
    ``0 in np.argsort(score_list)[-top_k:]`` is evaluated on the looked-up scores as Python floats, as ``.item()`` hands them to the
    reference -> ``correct / num_trials`` per generated image."""
    m = np.asarray(scores.detach().cpu() if isinstance(scores, torch.Tensor) else scores)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError(f"expected a square score matrix, got shape {m.shape}")
    n = m.shape[0]
    corrects = []
    for idx in range(n):
        row = [float(v) for v in m[idx]]
        gt_score = row[idx]
        correct_count = 0
        for _ in range(num_trials):
            n_imgs_idx = np.random.choice(n - 1, n_way - 1, replace=False)
            score_list = [gt_score] + [row[int(r) if r < idx else int(r) + 1] for r in n_imgs_idx]
            correct_count += 1 if 0 in np.argsort(score_list)[-top_k:] else 0
        corrects.append(correct_count / num_trials)
    return corrects


def n_way_scores(pred_videos, gt_videos, n_way: int = 50, top_k: int = 1, num_trials: int = 10, cache_dir: str = ".cache",
                 device: Optional[str] = "cuda", model=None) -> List[float]:
    """``40_class_run_metrics.py:145-174``: per generated image, the fraction of ``num_trials`` trials in which its CLIP score against
    its own ground truth is among the ``top_k`` of that score and the scores against ``n_way - 1`` other ground truths drawn at random.
    ``pred_videos`` / ``gt_videos``: ``[n,h,w,3]`` pixel values 0..255, ``n >= n_way``.  The reference runs the processor and the model
    again for both images of each of its ``n * (num_trials * (n_way - 1) + 1)`` comparisons; here each side is embedded ONCE, one
    matrix call gives every score, and ``n_way_from_matrix`` replays the reference's draws on it: under the same numpy seed the
    result is the reference's loop over the same scores."""
    assert n_way > top_k
    calc = clip_score(device, cache_dir, model)
    a, b = calc.embed(pred_videos), calc.embed(gt_videos)
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"{a.shape[0]} generated images against {b.shape[0]} ground-truth images")
    return n_way_from_matrix(calc.similarity(a, b, matrix=True), n_way, top_k, num_trials)
