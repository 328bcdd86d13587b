#!/usr/bin/env python3
"""The CLIP score (``e2v_clip_embed`` + ``e2v_clip_similarity``) at the scoring script's size: CLIP-B/32's vision tower
(``openai/clip-vit-base-patch32``'s vision config, random weights), 32 generated + 32 ground-truth clips x 6 frames = 384 images of
288 x 512 uint8, channels-last, and the 192 x 192 matrix of their 512-dim embeddings.

    python tools/clip_score_bench.py [--out profiles/clip_score_<tag>.json] [--repeats 5] [--sweep]

call      wall clock from the call to the end of a stream synchronisation, each of ``--repeats`` after one warm-up (their spread is
          the session's run-to-run spread): ``e2v_clip_embed`` of the 384 images in one call, and the 192 x 192 matrix (also the
          1200 x 1200 one of a full 200-clip evaluation).
split     the library's own event profile of one call of each, IN A RUN OF ITS OWN (the events serialise the launches): kernel classes
          folded into preprocess / linears / attention / norms / other, ms and share.
torch     if ``transformers`` is importable: ``transformers.CLIPVisionModelWithProjection`` on torch-ROCm from the SAME weights, model
          forward only (pixel values already on the device; the processor's host time for one image is given beside it) -- fp32
          batched (the yardstick: 64 images per forward) and the reference's fp16 image-by-image loop, one forward per image of a pair
          (``40_class_run_metrics.py:50-54``; 2 x 192 forwards for the 192 frame pairs) -- and the agreement of its fp32 embeddings with
          ours on the first clip.  Not importable: only our side, and the record says so.
sweep     ``--sweep``: a scored sweep (``examples/run_sweep.py --score-against --classifier --video-classifier --clip-model``, bf16, one
          batch of 32 clips, all four metric groups on) and the ``score`` stage's share of ``generate``.
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

GROUPS = {"preprocess": ("video_preprocess",), "linears": ("igemm",), "attention": ("image_attn",), "norms": ("layernorm",)}


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def profiled(eng, fn, groups):
    torch.cuda.synchronize()
    eng.profile_begin()
    fn()
    prof = eng.profile_end()
    total = sum(v["ms"] for v in prof.values())
    split = {}
    for g, names in groups.items():
        ms = sum(v["ms"] for k, v in prof.items() if k.startswith(names))
        split[g] = {"ms": ms, "tflops": sum(v["flops"] for k, v in prof.items() if k.startswith(names)) / 1e9 / max(ms, 1e-9)}
    split["other"] = {"ms": total - sum(v["ms"] for v in split.values())}
    for v in split.values():
        v["share"] = v["ms"] / max(total, 1e-9)
    return {"profiled_run_total_ms": total, "split": split, "kernel_classes": prof}


def torch_side(sd, cfg, frames_u8, ours, repeats):
    import transformers
    from PIL import Image
    model = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(
        hidden_size=cfg.hidden, num_attention_heads=cfg.heads, num_hidden_layers=cfg.layers, intermediate_size=cfg.intermediate,
        image_size=cfg.image_size, patch_size=cfg.patch_size, projection_dim=cfg.projection_dim, hidden_act=cfg.hidden_act,
        layer_norm_eps=cfg.layer_norm_eps)).eval()
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not [k for k in missing if not k.endswith("position_ids")] and not unexpected, (missing, unexpected)
    proc = transformers.CLIPImageProcessor(size={"shortest_edge": cfg.resize_edge}, crop_size={"height": cfg.image_size, "width": cfg.image_size},
                                           resample=Image.BICUBIC)
    proc(images=frames_u8[0, 0], return_tensors="pt")
    t0 = time.perf_counter()
    for f in range(frames_u8.shape[1]):
        proc(images=frames_u8[0, f], return_tensors="pt")
    proc_ms = (time.perf_counter() - t0) * 1e3 / frames_u8.shape[1]
    n_img = frames_u8.shape[0] * frames_u8.shape[1]
    first = proc(images=list(frames_u8[0]), return_tensors="pt")["pixel_values"]          # the first clip, exactly as the processor makes it
    res = {"transformers": transformers.__version__, "processor_host_ms_per_image": proc_ms, "images": n_img}
    px = torch.randn(n_img, 3, cfg.image_size, cfg.image_size).clamp(-1.5, 1.5)
    px[:first.shape[0]] = first
    with torch.no_grad():
        m = model.to("cuda", torch.float32)
        x = px.to("cuda", torch.float32)
        res["fp32_batched64_ms_each"] = timed(lambda: [m(pixel_values=x[i:i + 64]).image_embeds for i in range(0, n_img, 64)], repeats)
        res["fp32_batched64_ms"] = statistics.median(res["fp32_batched64_ms_each"])
        ref = m(pixel_values=x[:first.shape[0]]).image_embeds.double().cpu()
        res["fp32_embeds_vs_ours_rel"] = float((ours[:first.shape[0]].double().cpu() - ref).abs().max() / ref.abs().max())
        m = model.to("cuda", torch.float16)
        x = px.to("cuda", torch.float16)
        half = n_img // 2

        def pair_loop():                    # clip_score.__call__ for every (generated, ground-truth) frame pair: two forwards and a cosine
            return [torch.nn.functional.cosine_similarity(m(x[i:i + 1]).image_embeds.float(), m(x[half + i:half + i + 1]).image_embeds.float(),
                                                          dim=-1).item() for i in range(half)]
        res["fp16_pair_loop_ms_each"] = timed(pair_loop, max(1, repeats // 2))
        res["fp16_pair_loop_ms"] = statistics.median(res["fp16_pair_loop_ms_each"])
    return res


def scored_sweep():
    import importlib.util
    import io
    from contextlib import redirect_stdout
    from eeg2video_amd.clip_vision import CLIPVisionModelWithProjection
    from eeg2video_amd.image_classifier import ViTForImageClassification
    from eeg2video_amd.video_classifier import VideoMAEForVideoClassification
    spec = importlib.util.spec_from_file_location("e2v_sweep_bench", os.path.join(ROOT, "examples", "run_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with tempfile.TemporaryDirectory() as d:
        dirs = {k: os.path.join(d, k) for k in ("vit", "vmae", "clip", "clips")}
        for cls, key in ((ViTForImageClassification, "vit"), (VideoMAEForVideoClassification, "vmae"), (CLIPVisionModelWithProjection, "clip")):
            m = cls().init_synthetic()
            m.save_pretrained(dirs[key])
            del m
            torch.cuda.empty_cache()
        common = ["--concepts", "8", "--per-concept", "4", "--batch", "32", "--steps", "50", "--dtype", "bf16"]
        buf = io.StringIO()
        with redirect_stdout(buf):
            mod.main(common + ["--out", dirs["clips"], "--npy"])
            mod.main(common + ["--score-against", dirs["clips"], "--classifier", dirs["vit"], "--video-classifier", dirs["vmae"],
                               "--clip-model", dirs["clip"]])
        rec = json.loads(buf.getvalue().strip().splitlines()[-1])
    st = rec["stage_seconds_rank0"]
    keep = ("ssim_mean", "image_2way_acc", "image_40way_acc", "video_2way_acc", "clip_score_mean", "clip_2way_acc", "clip_40way_acc")
    return {"workload": rec["workload"], "stage_seconds_rank0": st, "score_share_of_generate": st["score"] / st["generate"],
            **{k: rec[k] for k in keep if k in rec}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_score.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clips", type=int, default=32, help="per side")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--metric-dtype", default=None, choices=["fp32", "bf16", "fp16", "all"],
                    help="measure ONLY the arms of the call -- the tower in fp32 and in this 16-bit mode ('all': bf16 and fp16) -- in one "
                         "session, alternating (tools/metric_dtype_arms.py), and merge them into --out under 'metric_dtype_arms'")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/clip_score_bench.py measures on the GPU: none found")
    from eeg2video_amd.clip_vision import CLIPVisionModelWithProjection
    from eeg2video_amd.weights import ClipVisionConfig, clip_vision_param_spec, synth_state_dict
    cfg = ClipVisionConfig()
    sd = synth_state_dict(clip_vision_param_spec(cfg), seed=46, mode="perturbed")
    model = CLIPVisionModelWithProjection(cfg).load_state_dict(sd)
    eng = model.engine
    n, F, H, W = 2 * a.clips, 6, 288, 512
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (n, F, H, W, 3), dtype=np.uint8))
    d_frames = frames.cuda()
    embed = lambda: eng.clip_embed(d_frames, channels_last=True)
    if a.metric_dtype:
        from metric_dtype_arms import measure_arms, merge_into
        arms = measure_arms(model, embed, a.metric_dtype, a.repeats)
        arms["device"], arms["input"] = torch.cuda.get_device_name(0), f"{n * F} images of {H} x {W} uint8, channels-last, one e2v_clip_embed call"
        merge_into(a.out, "metric_dtype_arms", arms)
        print(json.dumps({"tool": os.path.basename(__file__), "metric_dtype_arms": {k: v for k, v in arms.items() if k != "kernel_classes"}}))
        return
    wall = timed(embed, a.repeats)
    emb = embed()
    half = emb.shape[0] // 2
    pa, pb = emb[:half].contiguous(), emb[half:].contiguous()
    sim = lambda: eng.clip_similarity(pa, pb, matrix=True)
    sim_wall = timed(sim, a.repeats)
    big_a, big_b = torch.randn(1200, cfg.projection_dim, device="cuda"), torch.randn(1200, cfg.projection_dim, device="cuda")
    big_wall = timed(lambda: eng.clip_similarity(big_a, big_b, matrix=True), a.repeats)
    res = {"tool": "tools/clip_score_bench.py", "device": torch.cuda.get_device_name(0),
           "model": "CLIP-B/32 vision tower at 224 (openai/clip-vit-base-patch32's vision config), random weights, fp32",
           "input": {"images": n * F, "clips_per_side": a.clips, "frames": F, "height": H, "width": W, "layout": "uint8 channels-last [n,F,H,W,3]"},
           "embed_wall_ms": statistics.median(wall), "embed_wall_ms_each": wall, "ms_per_image": statistics.median(wall) / (n * F),
           "matrix_192_wall_ms": statistics.median(sim_wall), "matrix_192_wall_ms_each": sim_wall,
           "matrix_1200_wall_ms": statistics.median(big_wall), "matrix_1200_wall_ms_each": big_wall,
           "embed_profile": profiled(eng, embed, GROUPS), "matrix_192_profile": profiled(eng, sim, {"similarity": ("clip_similarity",)}),
           "device_bytes": eng.device_bytes()}
    try:
        import transformers  # noqa: F401
        have = True
    except ImportError:
        have = False
        res["torch"] = "transformers is not importable here: only the library's side was measured"
    if have:
        res["torch"] = torch_side(sd, cfg, frames.numpy(), emb, a.repeats)
        res["ours_over_torch_fp32_batched"] = res["embed_wall_ms"] / res["torch"]["fp32_batched64_ms"]
        res["torch_fp16_pair_loop_over_ours"] = res["torch"]["fp16_pair_loop_ms"] / (res["embed_wall_ms"] + res["matrix_192_wall_ms"])
    if a.sweep:
        del model, eng
        torch.cuda.empty_cache()
        res["sweep_scored"] = scored_sweep()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
