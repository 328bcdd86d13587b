"""Float64 / integer restatements of what ``e2v_video_classify`` computes, for the tests of the video classifier (imported by
``test_video_classifier_host.py`` and ``test_hip_video_classifier.py``; not a test module itself).

* ``crop_geometry`` / ``resize_crop_with_tables``: ``VideoMAEImageProcessor``'s shortest-edge resize (Pillow's two-pass antialiased
  BILINEAR from the per-axis tables of ``e2v_image_resize_table``) of which only the centre crop is computed, in integer numpy;
* ``tubelet_rows``: a clip's cropped bytes + the processor's pixel table -> the tubelet patch-row matrix the device builds;
* ``videomae_forward``: ``VideoMAEForVideoClassification`` in float64 numpy from a state dict in ``transformers``' spelling.

``apply_axis``, ``pixel_table``, ``softmax64``, ``top3`` and ``rel_err`` are the image classifier's (``vit_restatement.py``).
"""
from __future__ import annotations

import math
import os

import numpy as np

from vit_restatement import apply_axis, pixel_table, rel_err, softmax64, top3  # noqa: F401  (re-exported)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "videomae_tiny.npz")
GROUPS = ("36x64", "90x50", "56x56")


def load_golden():
    z = np.load(GOLDEN)
    sd = {k[len("w."):]: z[k].astype(np.float32) for k in z.files if k.startswith("w.")}
    return z, sd


def crop_geometry(h: int, w: int, edge: int, size: int):
    """``(nh, nw, top, left)``: the shortest edge to ``edge`` with the aspect ratio kept, then the centre crop of ``size``"""
    nh, nw = (edge, int(edge * w / h)) if h <= w else (int(edge * h / w), edge)
    return nh, nw, (nh - size) // 2, (nw - size) // 2


def _window(table, in_size, out_size, lo, size):
    first, count, coeff = table(in_size, out_size)
    return first[lo:lo + size], count[lo:lo + size], coeff[lo:lo + size]


def resize_crop_with_tables(img: np.ndarray, edge: int, size: int, table) -> np.ndarray:
    """``[H,W,3]`` uint8 -> the ``[size,size,3]`` centre crop of Pillow's resize to ``(nh, nw)``; only the window's rows and columns
    are computed.  ``table(in_size, out_size) -> (first, count, coeff)``"""
    h, w, _ = img.shape
    nh, nw, top, left = crop_geometry(h, w, edge, size)
    hor, ver = _window(table, w, nw, left, size), _window(table, h, nh, top, size)
    if h > w * 100 and nh < h:                                        # PIL/Image.py: such an image is resized vertically first
        x = apply_axis(np.transpose(img, (2, 1, 0)), *ver)            # [3,W,S]
        x = apply_axis(np.transpose(x, (0, 2, 1)), *hor)              # [3,S,S] (y, x)
        return np.ascontiguousarray(np.transpose(x, (1, 2, 0)))
    x = apply_axis(np.transpose(img, (2, 0, 1)), *hor)                # horizontal: [3,H,S]
    x = apply_axis(np.transpose(x, (0, 2, 1)), *ver)                  # vertical over [3,S,H] -> [3,S,S] (x, y)
    return np.ascontiguousarray(np.transpose(x, (2, 1, 0)))           # [y,x,c]


def pillow_resize_crop(img: np.ndarray, edge: int, size: int) -> np.ndarray:
    from PIL import Image
    nh, nw, top, left = crop_geometry(img.shape[0], img.shape[1], edge, size)
    return np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR))[top:top + size, left:left + size]


def tubelet_rows(cropped: np.ndarray, lut: np.ndarray, patch: int, tubelet: int) -> np.ndarray:
    """``[F,S,S,3]`` bytes of one clip -> ``[(F/ts)*(S/P)^2, 3*ts*P*P]`` fp32: token (t, py, px), column ``((c*ts + dt)*P + y)*P + x``
    (the flatten of the ``Conv3d`` weight)"""
    f, s = cropped.shape[0], cropped.shape[1]
    g, tt = s // patch, f // tubelet
    px = np.stack([lut[c][cropped[..., c]] for c in range(3)])        # [3,F,S,S]
    px = px.reshape(3, tt, tubelet, g, patch, g, patch).transpose(1, 3, 5, 0, 2, 4, 6)      # [t,py,px,c,dt,y,x]
    return np.ascontiguousarray(px.reshape(tt * g * g, 3 * tubelet * patch * patch))


def position_table64(n_position: int, d_hid: int) -> np.ndarray:
    """the fixed sinusoid in closed form, float64 (the mirror's table must be this rounded to fp32, up to libm's last bit)"""
    pos = np.arange(n_position, dtype=np.float64)[:, None]
    j = np.arange(d_hid)
    ang = pos / np.power(10000.0, 2 * (j // 2) / d_hid)
    return np.where(j % 2 == 0, np.sin(ang), np.cos(ang))


def _ln(x, g, b, eps):
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * g + b


_erf = np.vectorize(math.erf)


def videomae_forward(sd, rows: np.ndarray, pos: np.ndarray, heads: int, eps: float) -> np.ndarray:
    """``rows`` ``[n, T, 3*ts*P*P]`` tubelet rows, ``pos`` ``[T, C]`` -> logits ``[n, labels]``, float64 throughout.  No class token,
    no final LayerNorm; the mean over the tokens, ``fc_norm`` at ``nn.LayerNorm``'s default eps 1e-5, the classifier."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    pw = w["videomae.embeddings.patch_embeddings.projection.weight"]
    c = pw.shape[0]
    x = rows.astype(np.float64) @ pw.reshape(c, -1).T + w["videomae.embeddings.patch_embeddings.projection.bias"]
    x = x + np.asarray(pos, dtype=np.float64)
    n, t = x.shape[0], x.shape[1]
    i = 0
    while f"videomae.encoder.layer.{i}.layernorm_before.weight" in w:
        p = f"videomae.encoder.layer.{i}."
        h = _ln(x, w[p + "layernorm_before.weight"], w[p + "layernorm_before.bias"], eps)
        q, k, v = (h @ w[p + f"attention.attention.{nm}.weight"].T + w[p + f"attention.attention.{nm}.bias"] for nm in ("query", "key", "value"))
        split = lambda a: a.reshape(n, t, heads, 64).transpose(0, 2, 1, 3)
        s = split(q) @ split(k).transpose(0, 1, 3, 2) / 8.0
        s = np.exp(s - s.max(-1, keepdims=True))
        a = (s / s.sum(-1, keepdims=True)) @ split(v)
        a = a.transpose(0, 2, 1, 3).reshape(n, t, c)
        x = x + a @ w[p + "attention.output.dense.weight"].T + w[p + "attention.output.dense.bias"]
        h = _ln(x, w[p + "layernorm_after.weight"], w[p + "layernorm_after.bias"], eps)
        f = h @ w[p + "intermediate.dense.weight"].T + w[p + "intermediate.dense.bias"]
        f = 0.5 * f * (1.0 + _erf(f / math.sqrt(2.0)))
        x = x + f @ w[p + "output.dense.weight"].T + w[p + "output.dense.bias"]
        i += 1
    pooled = _ln(x.mean(1), w["fc_norm.weight"], w["fc_norm.bias"], 1e-5)
    return pooled @ w["classifier.weight"].T + w["classifier.bias"]
