"""Writes ``tests/golden/clip_vision_tiny.npz``: the CLIP vision tower / CLIP score fixture, made by ``transformers``, Pillow and
torch themselves.

Run where ``transformers`` and Pillow are installed (CPU is enough):  ``python tests/golden/make_clip_vision_golden.py``

``transformers.CLIPVisionModelWithProjection`` is built at ``TINY_CLIP_VISION`` (hidden 128, 2 heads, 2 layers, intermediate 256,
112 x 112 images in 16 x 16 patches -- 50 tokens, the count of CLIP-B/32 at 224 --, projection 64, quick_gelu) with weights from a
seeded torch generator, scaled up so that the embeddings of random images have spread (with the default initialisation every pair
of random images scores about 0.99).  Every tensor is rounded to a multiple of 2^-10 (few distinct values: the compressed file stays
small), then to fp16, and stored as fp16; the model runs on those values widened to fp32.
The processor is ``CLIPImageProcessor`` with ``shortest_edge = 112``, a centre crop of 112, BICUBIC, CLIP's mean and std.  The file holds

* ``w.<name>``: the weights under the ``openai/clip-vit-base-patch32`` checkpoint's key names,
* ``images_36x64`` ``[4,36,64,3]`` (wide), ``images_131x90`` ``[2,131,90,3]`` (tall, an odd crop remainder), ``images_112x112``
  ``[2,112,112,3]`` (its own resize): random uint8 images,
* ``cropped_36x64``, ``cropped_131x90``: ``PIL.Image.resize((nw, nh), BICUBIC)`` of them, centre-cropped to 112 x 112,
* ``pixel_table`` ``[3,256]`` fp32: the value the processor gives each byte, per channel,
* ``image_embeds`` ``[8,64]`` fp32: the model's ``image_embeds``, images in the order above,
* ``pair_scores`` ``[8]``: ``F.cosine_similarity(e, roll(e, 1), dim=-1)``; ``matrix`` ``[8,8]``: of every pair of embeddings,
* ``transformers_version``, ``pillow_version``, ``torch_version``.

Asserted here: the processor's ``pixel_values`` equal resize + crop + table bit for bit.  The image seed is advanced until every row
of the matrix has gaps above ``1e-3`` between neighbouring sorted entries, so that an implementation within tolerance ranks every
row as the fixture does.  Printed: the distance of the fixture's fp32 values from the float64 restatement
(``tests/clip_vision_restatement.py``) -- what the GPU tests' tolerances are ten times of.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from eeg2video_amd.weights import TINY_CLIP_VISION, clip_vision_param_spec  # noqa: E402

OUT = os.path.join(HERE, "clip_vision_tiny.npz")
SHAPES = ((4, 36, 64), (2, 131, 90), (2, 112, 112))


def make_weights(seed: int = 2026):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in clip_vision_param_spec(TINY_CLIP_VISION).items():
        if "layer_norm" in name or "layrnorm" in name or "layernorm" in name:
            v = torch.randn(shape, generator=g) * 0.25 + (1.0 if name.endswith(".weight") else 0.0)
        elif name.endswith(("class_embedding", "position_embedding.weight")):
            v = torch.randn(shape, generator=g) * 0.5
        elif name.endswith(".bias"):
            v = torch.randn(shape, generator=g) * 0.1
        else:
            fan_in = int(np.prod(shape[1:]))
            gain = 3.0 if "patch_embedding" in name else 1.5 if any(s in name for s in (".q_proj.", ".k_proj.", ".fc1.")) else 1.0
            v = torch.randn(shape, generator=g) * gain / fan_in ** 0.5
        sd[name] = (torch.round(v * 1024) / 1024).half()
    return sd


def build_model(sd):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    c = TINY_CLIP_VISION
    model = CLIPVisionModelWithProjection(CLIPVisionConfig(
        hidden_size=c.hidden, num_attention_heads=c.heads, num_hidden_layers=c.layers, intermediate_size=c.intermediate,
        image_size=c.image_size, patch_size=c.patch_size, projection_dim=c.projection_dim, hidden_act=c.hidden_act,
        layer_norm_eps=c.layer_norm_eps)).eval()
    own = model.state_dict()
    load = {k: torch.as_tensor(v).float() for k, v in sd.items()}
    missing, unexpected = model.load_state_dict(load, strict=False)
    missing = [k for k in missing if not k.endswith("position_ids")]
    assert not missing and not unexpected, (missing, unexpected, sorted(own)[:8])
    return model


def main():
    import PIL
    import transformers
    import torch.nn.functional as F
    from PIL import Image
    from transformers import CLIPImageProcessor

    import clip_vision_restatement as R
    c = TINY_CLIP_VISION
    sd = make_weights()
    model = build_model(sd)
    kw = dict(do_resize=True, resample=Image.BICUBIC, do_center_crop=True, do_rescale=True, rescale_factor=c.rescale_factor,
              do_normalize=True, image_mean=list(c.image_mean), image_std=list(c.image_std), do_convert_rgb=True)
    proc = CLIPImageProcessor(size={"shortest_edge": c.resize_edge}, crop_size={"height": c.image_size, "width": c.image_size}, **kw)
    # the value of every byte, per channel: a 16 x 16 image of the 256 values through a processor that neither resizes nor crops it
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    flat = CLIPImageProcessor(size={"shortest_edge": 16}, crop_size={"height": 16, "width": 16}, **kw)
    table = flat(images=ramp, return_tensors="np")["pixel_values"][0].reshape(3, 256).astype(np.float32)
    assert np.array_equal(table, R.pixel_table(c.rescale_factor, c.image_mean, c.image_std)), "the pixel table is not rescale-then-normalise in fp32"

    seed = 21
    while True:
        rng = np.random.default_rng(seed)
        groups = [rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8) for n, h, w in SHAPES]
        cropped = [np.stack([R.pillow_resize_crop(im, c.resize_edge, c.image_size, Image.BICUBIC) for im in g]) for g in groups]
        pixels = []
        for g, r in zip(groups, cropped):
            pv = proc(images=list(g), return_tensors="np")["pixel_values"].astype(np.float32)           # [n,3,S,S]
            want = np.stack([table[ch][r[..., ch]] for ch in range(3)], axis=1)
            assert np.array_equal(pv, want), "the processor is not Pillow's resize, the centre crop and the pixel table"
            pixels.append(pv)
        with torch.no_grad():
            emb = model(pixel_values=torch.from_numpy(np.concatenate(pixels))).image_embeds.float()
        matrix = F.cosine_similarity(emb[:, None, :], emb[None, :, :], dim=-1)
        srt = np.sort(matrix.numpy(), axis=-1)
        if (np.diff(srt, axis=-1) > 1e-3).all():
            break
        seed += 1
    pairs = F.cosine_similarity(emb, emb.roll(1, 0), dim=-1)

    # how far the fixture's own fp32 arithmetic is from float64: the yardstick of the GPU tests' tolerances
    sd32 = {k: v.float().numpy() for k, v in sd.items()}
    rows = np.concatenate([np.stack([R.patch_rows(im, table, c.patch_size) for im in r]) for r in cropped])
    emb64 = R.clip_vision_forward(sd32, rows, c.heads, c.layer_norm_eps, c.hidden_act)
    e = emb.numpy()
    err_emb = R.rel_err(e, emb64)
    err_pair = float(np.abs(pairs.numpy() - R.cosine64(e, np.roll(e, 1, 0))).max())
    err_mat = float(np.abs(matrix.numpy() - R.cosine64(e, e, matrix=True)).max())
    err_mat_e2e = float(np.abs(matrix.numpy() - R.cosine64(emb64, emb64, matrix=True)).max())
    err_pair_e2e = float(np.abs(pairs.numpy() - R.cosine64(emb64, np.roll(emb64, 1, 0))).max())

    out = {"w." + k: v.numpy() for k, v in sd.items()}
    for (n, h, w), g, r in zip(SHAPES, groups, cropped):
        out[f"images_{h}x{w}"] = g
        if (h, w) != (c.image_size, c.image_size):
            out[f"cropped_{h}x{w}"] = r
        else:
            assert np.array_equal(g, r)
    out["pixel_table"] = table
    out["image_embeds"] = e.astype(np.float32)
    out["pair_scores"] = pairs.numpy().astype(np.float32)
    out["matrix"] = matrix.numpy().astype(np.float32)
    out["image_seed"] = np.int64(seed)
    out["transformers_version"] = np.array(transformers.__version__)
    out["pillow_version"] = np.array(PIL.__version__)
    out["torch_version"] = np.array(torch.__version__)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, image seed {seed}, transformers {transformers.__version__}, Pillow {PIL.__version__}")
    print("embedding range", float(e.min()), float(e.max()), "matrix range", float(matrix.min()), float(matrix.max()),
          "smallest gap in a sorted row", float(np.diff(srt, axis=-1).min()))
    print(f"fixture fp32 against the float64 restatement: image_embeds {err_emb:.3e} (max abs / max abs), pair scores {err_pair:.3e}, "
          f"matrix {err_mat:.3e} (cosine alone, from the fixture's embeddings); pair scores {err_pair_e2e:.3e}, matrix {err_mat_e2e:.3e} "
          f"(whole model, from float64 embeddings)")


if __name__ == "__main__":
    main()
