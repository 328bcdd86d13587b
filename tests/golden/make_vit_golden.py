"""Writes ``tests/golden/vit_tiny.npz``: the ViT image classifier fixture, made by ``transformers`` and Pillow themselves.

Run where ``transformers`` and Pillow are installed (CPU is enough):  ``python tests/golden/make_vit_golden.py``

``transformers.ViTForImageClassification`` is built at ``TINY_IMAGE`` (hidden 128, 2 heads, 2 layers, intermediate 256, 112 x 112
images in 8 x 8 patches -- 197 tokens, the count of ViT-B/16 at 224 --, 50 labels) with weights from a seeded torch generator: projection
matrices scaled up so that scores, activations and logits have spread, LayerNorm weights around 1 and biases around 0 with real
variation.  Every tensor is rounded to fp16 and stored as fp16; the model runs on those values widened to fp32.  The file holds

* ``w.<name>``: the weights under the ``google/vit-base-patch16-224`` checkpoint's key names,
* ``images_36x64`` ``[4,36,64,3]``, ``images_130x90`` ``[2,130,90,3]``, ``images_112x112`` ``[2,112,112,3]``: random uint8 images,
* ``resized_36x64``, ``resized_130x90``: ``PIL.Image.resize((112, 112), BILINEAR)`` of them (a 112 x 112 image is its own resize),
* ``pixel_table`` ``[3,256]`` fp32: the value ``ViTImageProcessor`` gives each byte, per channel,
* ``logits`` and ``probs`` ``[8,50]`` fp32: the model's logits and their softmax, images in the order above,
* ``transformers_version``, ``pillow_version``.

Every stored image has a gap between its 3rd and 4th largest logit above ``1e-3 * max|logit|`` (asserted; the image seed is advanced
until all 8 qualify), so that the top-3 set of an implementation within the logits' tolerance is the fixture's.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from eeg2video_amd.weights import TINY_IMAGE, _VIT_V5_NAMES, image_param_spec  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vit_tiny.npz")
SHAPES = ((4, 36, 64), (2, 130, 90), (2, 112, 112))


def make_weights(seed: int = 2025):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in image_param_spec(TINY_IMAGE).items():
        if "layernorm" in name:
            v = torch.randn(shape, generator=g) * 0.25 + (1.0 if name.endswith(".weight") else 0.0)
        elif name.endswith(("cls_token", "position_embeddings")):
            v = torch.randn(shape, generator=g) * 0.5
        elif name.endswith(".bias"):
            v = torch.randn(shape, generator=g) * 0.1
        else:
            fan_in = int(np.prod(shape[1:]))
            gain = 1.5 if any(s in name for s in (".query.", ".key.", "intermediate.dense")) else 2.0 if name.startswith("classifier") else 1.0
            v = torch.randn(shape, generator=g) * gain / fan_in ** 0.5
        sd[name] = v.half()
    return sd


def to_installed_names(sd, own):
    """The checkpoint's names -> whatever this ``transformers`` calls the same tensors (5.x: ``vit.layers.{i}.attention.q_proj`` ...)"""
    if any(k.startswith("vit.encoder.layer.") for k in own):
        return dict(sd)
    out = {}
    for k, v in sd.items():
        if k.startswith("vit.encoder.layer."):
            rest = k[len("vit.encoder.layer."):]
            for new, old in _VIT_V5_NAMES:
                if old in rest:
                    rest = rest.replace(old, new)
                    break
            k = "vit.layers." + rest
        out[k] = v
    return out


def build_model(sd):
    from transformers import ViTConfig, ViTForImageClassification
    c = TINY_IMAGE
    model = ViTForImageClassification(ViTConfig(hidden_size=c.hidden, num_attention_heads=c.heads, num_hidden_layers=c.layers,
                                                intermediate_size=c.intermediate, image_size=c.image_size, patch_size=c.patch_size,
                                                num_labels=c.num_labels, layer_norm_eps=c.layer_norm_eps, hidden_act="gelu")).eval()
    load = {k: torch.as_tensor(v).float() for k, v in to_installed_names(sd, model.state_dict()).items()}
    missing, unexpected = model.load_state_dict(load, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return model


def main():
    import PIL
    import transformers
    from PIL import Image
    from transformers import ViTImageProcessor
    c = TINY_IMAGE
    sd = make_weights()
    model = build_model(sd)
    proc = ViTImageProcessor(size={"height": c.image_size, "width": c.image_size}, resample=Image.BILINEAR, rescale_factor=c.rescale_factor,
                             image_mean=list(c.image_mean), image_std=list(c.image_std))
    # the value of every byte, per channel: a 16 x 16 image of the 256 values through a processor that does not resize it
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    flat = ViTImageProcessor(size={"height": 16, "width": 16}, resample=Image.BILINEAR, rescale_factor=c.rescale_factor,
                             image_mean=list(c.image_mean), image_std=list(c.image_std))
    table = flat(images=ramp, return_tensors="np")["pixel_values"][0].reshape(3, 256).astype(np.float32)

    seed = 11
    while True:
        rng = np.random.default_rng(seed)
        groups = [rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8) for n, h, w in SHAPES]
        resized = [np.stack([np.asarray(Image.fromarray(im).resize((c.image_size, c.image_size), Image.BILINEAR)) for im in g]) for g in groups]
        pixels = []
        for g, r in zip(groups, resized):
            pv = proc(images=list(g), return_tensors="np")["pixel_values"].astype(np.float32)           # [n,3,S,S]
            want = np.stack([table[ch][r[..., ch]] for ch in range(3)], axis=1)
            assert np.array_equal(pv, want), "the processor is not Pillow's resize followed by the pixel table"
            pixels.append(pv)
        with torch.no_grad():
            logits = model(pixel_values=torch.from_numpy(np.concatenate(pixels))).logits.float()
        srt = np.sort(logits.numpy(), axis=-1)
        gap = srt[:, -3] - srt[:, -4]
        if (gap > 1e-3 * np.abs(logits.numpy()).max(-1)).all():
            break
        seed += 1
    out = {"w." + k: v.numpy() for k, v in sd.items()}
    for (n, h, w), g, r in zip(SHAPES, groups, resized):
        out[f"images_{h}x{w}"] = g
        if (h, w) != (c.image_size, c.image_size):
            out[f"resized_{h}x{w}"] = r
        else:
            assert np.array_equal(g, r)
    out["pixel_table"] = table
    out["logits"] = logits.numpy().astype(np.float32)
    out["probs"] = logits.softmax(-1).numpy().astype(np.float32)
    out["image_seed"] = np.int64(seed)
    out["transformers_version"] = np.array(transformers.__version__)
    out["pillow_version"] = np.array(PIL.__version__)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, image seed {seed}, transformers {transformers.__version__}, Pillow {PIL.__version__}")
    print("logit range", float(logits.min()), float(logits.max()), "smallest 3rd-4th gap", float(gap.min()), "max prob", float(logits.softmax(-1).max()))


if __name__ == "__main__":
    main()
