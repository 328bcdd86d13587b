"""Float64 / integer restatements of what ``e2v_image_classify`` computes, for the tests of the image classifier (imported by
``test_image_classifier_host.py`` and ``test_hip_image_classifier.py``; not a test module itself).

* ``resize_with_tables``: Pillow's two-pass antialiased BILINEAR resize from the per-axis tables of ``e2v_image_resize_table``
  (horizontal pass first, the intermediate rounded to bytes), in integer numpy;
* ``patch_rows``: resized bytes + the processor's pixel table -> the patch-row matrix the device builds;
* ``vit_forward``: ``ViTForImageClassification`` in float64 numpy from a state dict in the checkpoint's spelling;
* ``softmax64`` / ``top3``: the head.
"""
from __future__ import annotations

import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vit_tiny.npz")


def load_golden():
    z = np.load(GOLDEN)
    sd = {k[len("w."):]: z[k].astype(np.float32) for k in z.files if k.startswith("w.")}
    return z, sd


def apply_axis(x: np.ndarray, first: np.ndarray, count: np.ndarray, coeff: np.ndarray) -> np.ndarray:
    """One pass over the LAST axis of a uint8 array: out[..., xx] = clip8((2^21 + sum_k coeff[xx, k] * x[..., first[xx] + k]) >> 22)"""
    out = np.empty(x.shape[:-1] + (len(first),), dtype=np.uint8)
    xi = x.astype(np.int64)
    for xx in range(len(first)):
        acc = (1 << 21) + (xi[..., first[xx]:first[xx] + count[xx]] * coeff[xx, :count[xx]].astype(np.int64)).sum(-1)
        out[..., xx] = np.clip(acc >> 22, 0, 255)
    return out


def resize_with_tables(img: np.ndarray, size: int, table) -> np.ndarray:
    """``[H,W,3]`` uint8 -> ``[size,size,3]`` uint8; ``table(in_size, out_size) -> (first, count, coeff)``"""
    h, w, _ = img.shape
    if h > w * 100 and size < h:                                      # PIL/Image.py: such an image is resized vertically first
        x = apply_axis(np.transpose(img, (2, 1, 0)), *table(h, size))                 # [3,W,S]
        x = apply_axis(np.transpose(x, (0, 2, 1)), *table(w, size))                   # [3,S,S] (y, x)
        return np.ascontiguousarray(np.transpose(x, (1, 2, 0)))
    x = np.transpose(img, (2, 0, 1))                                  # [3,H,W]
    x = apply_axis(x, *table(w, size))                                # horizontal: [3,H,S]
    x = apply_axis(np.transpose(x, (0, 2, 1)), *table(h, size))       # vertical over [3,S,H] -> [3,S,S] (x, y)
    return np.ascontiguousarray(np.transpose(x, (2, 1, 0)))           # [y,x,c]


def pillow_resize(img: np.ndarray, size: int) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((size, size), Image.BILINEAR))


def pixel_table(rescale: float, mean, std) -> np.ndarray:
    """``[3,256]`` fp32: the value ``ViTImageProcessor`` gives a byte -- rescaled in float64 and rounded to fp32, normalised in fp32"""
    b = (np.arange(256, dtype=np.float64) * rescale).astype(np.float32)
    return np.stack([(b - np.float32(mean[c])) / np.float32(std[c]) for c in range(3)]).astype(np.float32)


def patch_rows(resized: np.ndarray, lut: np.ndarray, patch: int) -> np.ndarray:
    """``[S,S,3]`` bytes -> ``[(S/P)^2, 3*P*P]`` fp32, column ``c*P*P + y*P + x`` (the flatten of the patch convolution's weight)"""
    s = resized.shape[0]
    g = s // patch
    px = np.stack([lut[c][resized[..., c]] for c in range(3)])        # [3,S,S]
    return np.ascontiguousarray(px.reshape(3, g, patch, g, patch).transpose(1, 3, 0, 2, 4).reshape(g * g, 3 * patch * patch))


def _ln(x, g, b, eps):
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * g + b


_erf = np.vectorize(math.erf)


def vit_forward(sd, rows: np.ndarray, heads: int, eps: float) -> np.ndarray:
    """``rows`` ``[n, T-1, 3*P*P]`` patch rows -> logits ``[n, labels]``, float64 throughout"""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    pw = w["vit.embeddings.patch_embeddings.projection.weight"]
    c = pw.shape[0]
    x = rows.astype(np.float64) @ pw.reshape(c, -1).T + w["vit.embeddings.patch_embeddings.projection.bias"]
    n = x.shape[0]
    x = np.concatenate([np.broadcast_to(w["vit.embeddings.cls_token"], (n, 1, c)), x], axis=1) + w["vit.embeddings.position_embeddings"]
    t = x.shape[1]
    i = 0
    while f"vit.encoder.layer.{i}.layernorm_before.weight" in w:
        p = f"vit.encoder.layer.{i}."
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
    cls = _ln(x[:, 0], w["vit.layernorm.weight"], w["vit.layernorm.bias"], eps)
    return cls @ w["classifier.weight"].T + w["classifier.bias"]


def softmax64(logits: np.ndarray) -> np.ndarray:
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def top3(logits: np.ndarray) -> np.ndarray:
    """``argsort(-1)[-3:]`` with the ties of a stable ascending sort"""
    return np.argsort(np.asarray(logits), axis=-1, kind="stable")[..., -3:].astype(np.int32)


def rel_err(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())
