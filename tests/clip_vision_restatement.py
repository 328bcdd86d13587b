"""Float64 / integer restatements of what ``e2v_clip_embed`` and ``e2v_clip_similarity`` compute, for the tests of the CLIP score
(imported by ``test_clip_vision_host.py`` and ``test_hip_clip_vision.py``; not a test module itself).

* ``crop_geometry`` / ``resize_crop_with_tables``: ``CLIPImageProcessor``'s resize of the shortest edge and centre crop from the
  per-axis tables of ``e2v_image_resize_table_filter``, in integer numpy (the whole resized image, then the crop);
* ``pillow_resize_crop``: the same through Pillow itself;
* ``clip_vision_forward``: ``CLIPVisionModelWithProjection`` in float64 numpy from a state dict in the checkpoint's spelling;
* ``cosine64``: ``torch.nn.functional.cosine_similarity(a, b, dim=-1, eps=1e-8)`` in float64, pairs or matrix;
* ``reference_n_way``: the loop of the reference's ``n_way_scores`` (``40_class_run_metrics.py:145-174``) over a score function.
"""
from __future__ import annotations

import math
import os

import numpy as np

from vit_restatement import _ln, apply_axis, patch_rows, pixel_table, rel_err  # noqa: F401  (shared with the image classifier's tests)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_vision_tiny.npz")
SHAPES = ((4, 36, 64), (2, 131, 90), (2, 112, 112))


def load_golden():
    z = np.load(GOLDEN)
    sd = {k[len("w."):]: z[k].astype(np.float32) for k in z.files if k.startswith("w.")}
    return z, sd


def golden_groups(z):
    """``[(images [n,H,W,3], cropped [n,S,S,3])]`` in the order of the stored embeddings (``z``: the npz file or a dict of it)"""
    return [(z[f"images_{h}x{w}"], z[f"cropped_{h}x{w}"] if f"cropped_{h}x{w}" in z else z[f"images_{h}x{w}"]) for _, h, w in SHAPES]


def crop_geometry(h: int, w: int, edge: int, size: int):
    """``(nh, nw, top, left)``: ``get_resize_output_image_size(default_to_square=False)`` and ``center_crop``"""
    nh, nw = (edge, int(edge * w / h)) if h <= w else (int(edge * h / w), edge)
    return nh, nw, (nh - size) // 2, (nw - size) // 2


def resize_crop_with_tables(img: np.ndarray, edge: int, size: int, table) -> np.ndarray:
    """``[H,W,3]`` uint8 -> ``[size,size,3]`` uint8; ``table(in_size, out_size) -> (first, count, coeff)``"""
    h, w, _ = img.shape
    nh, nw, top, left = crop_geometry(h, w, edge, size)
    if h > w * 100 and nh < h:                                        # PIL/Image.py: such an image is resized vertically first
        x = apply_axis(np.transpose(img, (2, 1, 0)), *table(h, nh))                   # [3,W,nh]
        x = apply_axis(np.transpose(x, (0, 2, 1)), *table(w, nw))                     # [3,nh,nw]
        full = np.transpose(x, (1, 2, 0))
    else:
        x = apply_axis(np.transpose(img, (2, 0, 1)), *table(w, nw))                   # [3,H,nw]
        x = apply_axis(np.transpose(x, (0, 2, 1)), *table(h, nh))                     # [3,nw,nh]
        full = np.transpose(x, (2, 1, 0))
    return np.ascontiguousarray(full[top:top + size, left:left + size])


def pillow_resize_crop(img: np.ndarray, edge: int, size: int, resample: int = 3) -> np.ndarray:
    from PIL import Image
    h, w, _ = img.shape
    nh, nw, top, left = crop_geometry(h, w, edge, size)
    full = np.asarray(Image.fromarray(img).resize((nw, nh), resample))
    return np.ascontiguousarray(full[top:top + size, left:left + size])


_erf = np.vectorize(math.erf)


def clip_vision_forward(sd, rows: np.ndarray, heads: int, eps: float, act: str = "quick_gelu") -> np.ndarray:
    """``rows`` ``[n, T-1, 3*P*P]`` patch rows -> ``image_embeds`` ``[n, projection_dim]``, float64 throughout"""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    m = "vision_model."
    pw = w[m + "embeddings.patch_embedding.weight"]
    c = pw.shape[0]
    x = rows.astype(np.float64) @ pw.reshape(c, -1).T
    n = x.shape[0]
    x = np.concatenate([np.broadcast_to(w[m + "embeddings.class_embedding"], (n, 1, c)), x], axis=1) + w[m + "embeddings.position_embedding.weight"]
    t = x.shape[1]
    x = _ln(x, w[m + "pre_layrnorm.weight"], w[m + "pre_layrnorm.bias"], eps)
    i = 0
    while f"{m}encoder.layers.{i}.layer_norm1.weight" in w:
        p = f"{m}encoder.layers.{i}."
        h = _ln(x, w[p + "layer_norm1.weight"], w[p + "layer_norm1.bias"], eps)
        q, k, v = (h @ w[p + f"self_attn.{nm}.weight"].T + w[p + f"self_attn.{nm}.bias"] for nm in ("q_proj", "k_proj", "v_proj"))
        split = lambda a: a.reshape(n, t, heads, 64).transpose(0, 2, 1, 3)
        s = split(q) @ split(k).transpose(0, 1, 3, 2) / 8.0
        s = np.exp(s - s.max(-1, keepdims=True))
        a = (s / s.sum(-1, keepdims=True)) @ split(v)
        a = a.transpose(0, 2, 1, 3).reshape(n, t, c)
        x = x + a @ w[p + "self_attn.out_proj.weight"].T + w[p + "self_attn.out_proj.bias"]
        h = _ln(x, w[p + "layer_norm2.weight"], w[p + "layer_norm2.bias"], eps)
        f = h @ w[p + "mlp.fc1.weight"].T + w[p + "mlp.fc1.bias"]
        f = f / (1.0 + np.exp(-1.702 * f)) if act == "quick_gelu" else 0.5 * f * (1.0 + _erf(f / math.sqrt(2.0)))
        x = x + f @ w[p + "mlp.fc2.weight"].T + w[p + "mlp.fc2.bias"]
        i += 1
    cls = _ln(x[:, 0], w[m + "post_layernorm.weight"], w[m + "post_layernorm.bias"], eps)
    return cls @ w["visual_projection.weight"].T


def cosine64(a, b, matrix: bool = False, eps: float = 1e-8) -> np.ndarray:
    """``x1 . x2 / (max(||x1||, eps) * max(||x2||, eps))`` over the last axis, float64"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na = np.maximum(np.sqrt((a * a).sum(-1)), eps)
    nb = np.maximum(np.sqrt((b * b).sum(-1)), eps)
    return (a @ b.T) / na[:, None] / nb[None, :] if matrix else (a * b).sum(-1) / na / nb


def reference_n_way(pred, gt, score, n_way: int, top_k: int, num_trials: int):
    """The reference's ``n_way_scores`` loop as it stands (``40_class_run_metrics.py:145-174``): ``pred``, ``gt`` sequences of equal
    length, ``score(p, g) -> float`` called once per comparison as there; draws from numpy's global generator in the reference's
    order -> the list of ``correct / num_trials`` per predicted image."""
    assert n_way > top_k
    corrects = []
    for idx in range(len(pred)):
        rest = [g for i, g in enumerate(gt) if i != idx]
        gt_score = score(pred[idx], gt[idx])
        correct = 0
        for _ in range(num_trials):
            n_idx = np.random.choice(len(rest), n_way - 1, replace=False)
            score_list = [gt_score] + [score(pred[idx], rest[int(j)]) for j in n_idx]
            correct += 1 if 0 in np.argsort(score_list)[-top_k:] else 0
        corrects.append(correct / num_trials)
    return corrects
