"""Writes ``tests/golden/metric_towers_16bit.npz``: what torch on the CPU gives for the three tiny metric models run in 16-bit.

Run where ``transformers`` is installed (CPU is enough):  ``python tests/golden/make_metric_dtype_golden.py``

The three tiny models of ``vit_tiny.npz``, ``videomae_tiny.npz`` and ``clip_vision_tiny.npz`` are rebuilt from the weights those
fixtures store (``build_model`` of their generators), cast with ``.to(dtype)`` as the reference casts them
(``EEG2Video/40_class_run_metrics.py:41,89,125``: ``.to(device, torch.float16)``) and fed the fixtures' stored resized / cropped bytes
through the stored ``pixel_table``, the pixel values cast to the same dtype (``:50-51,97-98,134-135``).  For ``dtype`` in ``fp16``,
``bf16`` the file holds

* ``vit_logits_<dtype>``, ``vit_probs_<dtype>`` ``[8,50]``: the logits and ``logits.softmax(-1)`` IN that dtype (``:98``), widened;
* ``videomae_logits_<dtype>``, ``videomae_probs_<dtype>`` ``[8,50]``: the same for the video classifier (``:135``);
* ``clip_embeds_<dtype>`` ``[8,64]``: ``image_embeds.float()``; ``clip_pairs_<dtype>`` ``[8]`` and ``clip_matrix_<dtype>`` ``[8,8]``: fp32
  ``cosine_similarity`` of them (``:53-55``), pairs against the embeddings rolled by one as in ``clip_vision_tiny.npz``;
* ``dist_<name>``: max |16-bit result - fp32 fixture| of each array above -- the yardstick of the device tests
  (``tests/test_hip_metric_dtype.py`` recomputes it from the two fixtures and takes 4 x it as its bound);
* ``near_<name>``: the neighbourhood of the fp32 result a 16-bit run has to stay in, ``32 u max|fp32 result|`` with ``u`` the unit
  roundoff of the format (2^-11 / 2^-8): a two-layer pre-LN tower rounds its residual stream, the LayerNorm outputs, q / k / v, the
  probabilities, the attention output and the MLP's two tensors -- some twenty roundings of relative size ``u`` on the way to the head,
  none amplified by more than the O(1) gains of the fixture's weights -- so 32 leaves room and a wrong graph (a missing residual, a
  wrong eps or scale: errors of the size of the result itself) does not fit.  ``tests/test_metric_dtype_host.py`` holds ``dist`` to it.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_clip_vision_golden import build_model as build_clip  # noqa: E402
from make_video_golden import build_model as build_videomae  # noqa: E402
from make_vit_golden import build_model as build_vit  # noqa: E402

OUT = os.path.join(HERE, "metric_towers_16bit.npz")
DTYPES = (("fp16", torch.float16, 2.0 ** -11), ("bf16", torch.bfloat16, 2.0 ** -8))
NEAR_FACTOR = 32.0


def load(name):
    z = np.load(os.path.join(HERE, name))
    return z, {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")}


def stored(z, kind, prefix):
    """the fixture's stored processor output, in the fixture's order: resized / cropped bytes, a source already at the model's size as it is"""
    keys = [k for k in z.files if k.startswith(prefix + "_")]                       # images_HxW / clips_HxW, in file order
    return np.concatenate([z[kind + k[len(prefix):]] if kind + k[len(prefix):] in z.files else z[k] for k in keys])


def pixel_values(table, u8, channel_axis):
    """bytes [..., S, S, 3] -> the processor's fp32 pixel values with the channel at ``channel_axis``"""
    return np.stack([table[ch][u8[..., ch]] for ch in range(3)], axis=channel_axis).astype(np.float32)


def main():
    import transformers
    out = {}

    def put(name, got, want, u):
        got = np.asarray(got, dtype=np.float32)
        out[name] = got
        out["dist_" + name] = np.float32(np.abs(got - want).max())
        out["near_" + name] = np.float32(NEAR_FACTOR * u * np.abs(want).max())

    zv, sdv = load("vit_tiny.npz")
    zm, sdm = load("videomae_tiny.npz")
    zc, sdc = load("clip_vision_tiny.npz")
    pv_vit = torch.from_numpy(pixel_values(zv["pixel_table"], stored(zv, "resized", "images"), 1))           # [8,3,S,S]
    pv_vmae = torch.from_numpy(pixel_values(zm["pixel_table"], stored(zm, "cropped", "clips"), 2))           # [8,6,3,S,S]
    pv_clip = torch.from_numpy(pixel_values(zc["pixel_table"], stored(zc, "cropped", "images"), 1))          # [8,3,S,S]
    with torch.no_grad():
        # the stored inputs through the fp32 models give the stored fp32 results: the three rebuilds are the fixtures' models
        assert np.abs(build_vit(sdv)(pixel_values=pv_vit).logits.numpy() - zv["logits"]).max() < 1e-4
        assert np.abs(build_videomae(sdm)(pixel_values=pv_vmae).logits.numpy() - zm["logits"]).max() < 1e-4
        assert np.abs(build_clip(sdc)(pixel_values=pv_clip).image_embeds.numpy() - zc["image_embeds"]).max() < 1e-4
        for tag, dt, u in DTYPES:
            for name, build, sd, pv, z in (("vit", build_vit, sdv, pv_vit, zv), ("videomae", build_videomae, sdm, pv_vmae, zm)):
                logits = build(sd).to(dt)(pixel_values=pv.to(dt)).logits
                put(f"{name}_logits_{tag}", logits.float().numpy(), z["logits"], u)
                put(f"{name}_probs_{tag}", logits.softmax(-1).float().numpy(), z["probs"], u)
            emb = build_clip(sdc).to(dt)(pixel_values=pv_clip.to(dt)).image_embeds.float()
            put(f"clip_embeds_{tag}", emb.numpy(), zc["image_embeds"], u)
            put(f"clip_pairs_{tag}", F.cosine_similarity(emb, emb.roll(1, 0), dim=-1).numpy(), zc["pair_scores"], u)
            put(f"clip_matrix_{tag}", F.cosine_similarity(emb[:, None, :], emb[None, :, :], dim=-1).numpy(), zc["matrix"], u)
    out["transformers_version"] = np.array(transformers.__version__)
    out["torch_version"] = np.array(torch.__version__)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 1 << 20, f"{size} bytes: over the size limit for a committed file"
    print(f"{OUT}: {size} bytes, transformers {transformers.__version__}, torch {torch.__version__}")
    for k in sorted(out):
        if k.startswith("dist_"):
            print(f"  {k[5:]:24s} max |16-bit - fp32| {float(out[k]):.3e}   neighbourhood {float(out['near_' + k[5:]]):.3e}")


if __name__ == "__main__":
    main()
