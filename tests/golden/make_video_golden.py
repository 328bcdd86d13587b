"""Writes ``tests/golden/videomae_tiny.npz``: the VideoMAE video classifier fixture, made by ``transformers`` and Pillow themselves.

Run where ``transformers`` and Pillow are installed (CPU is enough):  ``python tests/golden/make_video_golden.py``

``transformers.VideoMAEForVideoClassification`` is built at ``TINY_VIDEO`` (hidden 128, 2 heads, 2 layers, intermediate 256, 56 x 56
frames in 8 x 8 patches, tubelets of 2, 6 frames -- 147 tokens --, 50 labels) with weights from a seeded torch generator: projection
matrices scaled up so that scores, activations and logits have spread, LayerNorm weights around 1 and biases around 0 with real
variation.  Every tensor is rounded to fp16 and stored as fp16; the model runs on those values widened to fp32.  The file holds

* ``w.<name>``: the weights under the names of the installed ``transformers``' ``state_dict()`` (the ``Conv3d`` weight in five axes),
* ``clips_36x64`` ``[4,6,36,64,3]`` (wide), ``clips_90x50`` ``[2,6,90,50,3]`` (tall; the crop leaves an odd remainder),
  ``clips_56x56`` ``[2,6,56,56,3]`` (its own resize): uint8 clips -- blocks of 3 x 3 pixels of one random colour with a tenth of the
  pixels replaced by noise, so that the file compresses below the size limit for a committed file,
* ``cropped_36x64``, ``cropped_90x50``: the processor's bytes, i.e. ``PIL.Image.resize((nw, nh), BILINEAR)`` of every frame, centre-cropped,
* ``pixel_table`` ``[3,256]`` fp32: the value ``VideoMAEImageProcessor`` gives each byte, per channel,
* ``logits`` and ``probs`` ``[8,50]`` fp32: the model's logits and their softmax, clips in the order above,
* ``position_embeddings`` is NOT stored: it is a function of the config (``weights.video_position_table``; asserted equal here),
* ``transformers_version``, ``pillow_version``.

Asserted here: the processor's output equals Pillow's resize + the crop + the pixel table, bit for bit; every stored clip has a gap
between its 3rd and 4th largest logit above ``1e-3 * max|logit|`` (the clip seed is advanced until all 8 qualify), so that the top-3
set of an implementation within the logits' tolerance is the fixture's.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from eeg2video_amd.weights import TINY_VIDEO, video_checkpoint_spec, video_position_table  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "videomae_tiny.npz")
SHAPES = ((4, 36, 64), (2, 90, 50), (2, 56, 56))


def make_weights(seed: int = 2026):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in video_checkpoint_spec(TINY_VIDEO).items():
        if "layernorm" in name or name.startswith("fc_norm"):
            v = torch.randn(shape, generator=g) * 0.25 + (1.0 if name.endswith(".weight") else 0.0)
        elif name.endswith(".bias"):
            v = torch.randn(shape, generator=g) * 0.1
        else:
            fan_in = int(np.prod(shape[1:]))
            gain = 1.5 if any(s in name for s in (".query.", ".key.", "intermediate.dense")) else 2.0 if name.startswith("classifier") else 1.0
            v = torch.randn(shape, generator=g) * gain / fan_in ** 0.5
        sd[name] = v.half()
    return sd


def build_model(sd):
    from transformers import VideoMAEConfig, VideoMAEForVideoClassification
    c = TINY_VIDEO
    model = VideoMAEForVideoClassification(VideoMAEConfig(
        hidden_size=c.hidden, num_attention_heads=c.heads, num_hidden_layers=c.layers, intermediate_size=c.intermediate,
        image_size=c.image_size, patch_size=c.patch_size, tubelet_size=c.tubelet_size, num_frames=c.num_frames, num_labels=c.num_labels,
        layer_norm_eps=c.layer_norm_eps, hidden_act="gelu", qkv_bias=True, use_mean_pooling=True)).eval()
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == dict(video_checkpoint_spec(c))
    missing, unexpected = model.load_state_dict({k: torch.as_tensor(v).float() for k, v in sd.items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    own = model.videomae.embeddings.position_embeddings[0].numpy()
    assert np.array_equal(own, video_position_table(c.tokens, c.hidden)), "the mirror's position table is not transformers'"
    return model


def make_clip(rng, h, w):
    """6 frames of 3 x 3 blocks of one colour, a tenth of the pixels noise"""
    blocks = rng.integers(0, 256, (6, (h + 2) // 3, (w + 2) // 3, 3), dtype=np.uint8)
    clip = blocks.repeat(3, 1).repeat(3, 2)[:, :h, :w]
    noise = rng.integers(0, 256, clip.shape, dtype=np.uint8)
    return np.where(rng.random(clip.shape[:3])[..., None] < 0.1, noise, clip)


def main():
    import PIL
    import transformers
    from PIL import Image
    try:
        from transformers import VideoMAEImageProcessorPil as Processor        # the Pillow backend by name, where the default is torchvision's
    except ImportError:
        from transformers import VideoMAEImageProcessor as Processor
    c = TINY_VIDEO
    S = c.image_size
    sd = make_weights()
    model = build_model(sd)
    kw = dict(resample=Image.BILINEAR, rescale_factor=c.rescale_factor, image_mean=list(c.image_mean), image_std=list(c.image_std))
    proc = Processor(size={"shortest_edge": c.resize_edge}, crop_size={"height": S, "width": S}, **kw)
    # the value of every byte, per channel: a 16 x 16 frame of the 256 values through a processor that neither resizes nor crops it
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    flat = Processor(size={"shortest_edge": 16}, crop_size={"height": 16, "width": 16}, **kw)
    table = flat([ramp], return_tensors="np")["pixel_values"][0, 0].reshape(3, 256).astype(np.float32)

    seed = 21
    while True:
        rng = np.random.default_rng(seed)
        groups = [np.stack([make_clip(rng, h, w) for _ in range(n)]) for n, h, w in SHAPES]
        cropped, pixels = [], []
        for (n, h, w), g in zip(SHAPES, groups):
            nh, nw = (c.resize_edge, int(c.resize_edge * w / h)) if h <= w else (int(c.resize_edge * h / w), c.resize_edge)
            top, left = (nh - S) // 2, (nw - S) // 2
            r = np.stack([np.stack([np.asarray(Image.fromarray(f).resize((nw, nh), Image.BILINEAR))[top:top + S, left:left + S] for f in clip])
                          for clip in g])                                                                  # [n,6,S,S,3]
            pv = np.concatenate([proc(list(clip), return_tensors="np")["pixel_values"] for clip in g]).astype(np.float32)   # [n,6,3,S,S]
            want = np.stack([table[ch][r[..., ch]] for ch in range(3)], axis=2)
            assert np.array_equal(pv, want), "the processor is not Pillow's resize followed by the crop and the pixel table"
            cropped.append(r)
            pixels.append(pv)
        with torch.no_grad():
            logits = model(pixel_values=torch.from_numpy(np.concatenate(pixels))).logits.float()
        srt = np.sort(logits.numpy(), axis=-1)
        gap = srt[:, -3] - srt[:, -4]
        if (gap > 1e-3 * np.abs(logits.numpy()).max(-1)).all():
            break
        seed += 1
    out = {"w." + k: v.numpy() for k, v in sd.items()}
    for (n, h, w), g, r in zip(SHAPES, groups, cropped):
        out[f"clips_{h}x{w}"] = g
        if (h, w) != (S, S):
            out[f"cropped_{h}x{w}"] = r
        else:
            assert np.array_equal(g, r)
    out["pixel_table"] = table
    out["logits"] = logits.numpy().astype(np.float32)
    out["probs"] = logits.softmax(-1).numpy().astype(np.float32)
    out["clip_seed"] = np.int64(seed)
    out["transformers_version"] = np.array(transformers.__version__)
    out["pillow_version"] = np.array(PIL.__version__)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 1 << 20, f"{size} bytes: over the size limit for a committed file"
    print(f"{OUT}: {size} bytes, clip seed {seed}, transformers {transformers.__version__}, Pillow {PIL.__version__}")
    print("logit range", float(logits.min()), float(logits.max()), "smallest 3rd-4th gap", float(gap.min()), "max prob", float(logits.softmax(-1).max()))


if __name__ == "__main__":
    main()
