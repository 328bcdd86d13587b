#!/usr/bin/env python3
"""The image classifier (``e2v_image_classify``) at the scoring script's size: ViT-B/16 (``google/vit-base-patch16-224``'s config,
random weights), 32 clips x 6 frames x 2 (generated and ground truth) = 384 images of 288 x 512 uint8, channels-last.

    python tools/image_classifier_bench.py [--out profiles/image_classifier_<tag>.json] [--repeats 5] [--sweep]

call      wall clock from the call to the end of a stream synchronisation, each of ``--repeats`` after one warm-up (their spread is
          the session's run-to-run spread), for the 384 images in one call.
split     the library's own event profile of one call, IN A RUN OF ITS OWN (the events serialise the launches): kernel classes folded
          into preprocess / linears / attention / head / other, ms and share.
torch     if ``transformers`` is importable: ``transformers.ViTForImageClassification`` on torch-ROCm from the SAME weights, model
          forward only (pixel values already on the device; the processor's host time for one frame is given beside it) -- fp32 and the
          reference's fp16, image by image as ``40_class_run_metrics.py:94-98`` runs it and batched (64 images per forward) -- and the
          agreement of its fp32 logits with ours on the first clip.  Not importable: only our side, and the record says so.
sweep     ``--sweep``: a scored sweep (``examples/run_sweep.py --score-against --classifier``, bf16, one batch of 32 clips) and the
          ``score`` stage's share of ``generate``.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

GROUPS = {"preprocess": ("image_preprocess",), "linears": ("igemm",), "attention": ("image_attn",), "head": ("image_head",)}


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


def torch_side(sd, cfg, frames_u8, ours_logits, repeats):
    import transformers
    from golden.make_vit_golden import to_installed_names
    from PIL import Image
    model = transformers.ViTForImageClassification(transformers.ViTConfig(
        hidden_size=cfg.hidden, num_attention_heads=cfg.heads, num_hidden_layers=cfg.layers, intermediate_size=cfg.intermediate,
        image_size=cfg.image_size, patch_size=cfg.patch_size, num_labels=cfg.num_labels, layer_norm_eps=cfg.layer_norm_eps)).eval()
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in to_installed_names(sd, model.state_dict()).items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    proc = transformers.ViTImageProcessor(size={"height": cfg.image_size, "width": cfg.image_size}, resample=Image.BILINEAR)
    t0 = time.perf_counter()
    proc(images=frames_u8[0, 0], return_tensors="pt")
    proc_ms = (time.perf_counter() - t0) * 1e3
    n_img = frames_u8.shape[0] * frames_u8.shape[1]
    first = proc(images=list(frames_u8[0]), return_tensors="pt")["pixel_values"]          # the first clip, exactly as the processor makes it
    res = {"transformers": transformers.__version__, "processor_host_ms_per_frame": proc_ms, "images": n_img}
    px = torch.randn(n_img, 3, cfg.image_size, cfg.image_size).clamp(-1, 1)
    px[:first.shape[0]] = first
    with torch.no_grad():
        for name, dt in (("fp32", torch.float32), ("fp16", torch.float16)):
            m = model.to("cuda", dt)
            x = px.to("cuda", dt)
            res[name + "_batched64_ms_each"] = timed(lambda: [m(pixel_values=x[i:i + 64]).logits for i in range(0, n_img, 64)], repeats)
            res[name + "_image_by_image_ms_each"] = timed(lambda: [m(pixel_values=x[i:i + 1]).logits for i in range(n_img)], max(1, repeats // 2))
            for k in ("batched64", "image_by_image"):
                res[f"{name}_{k}_ms"] = statistics.median(res[f"{name}_{k}_ms_each"])
            if dt == torch.float32:
                ref = m(pixel_values=x[:first.shape[0]]).logits.double().cpu()
                res["fp32_logits_vs_ours_rel"] = float((ours_logits[:first.shape[0]].double().cpu() - ref).abs().max() / ref.abs().max())
    return res


def scored_sweep(cfg, sd):
    import importlib.util
    import io
    from contextlib import redirect_stdout
    from eeg2video_amd.image_classifier import ViTForImageClassification
    spec = importlib.util.spec_from_file_location("e2v_sweep_bench", os.path.join(ROOT, "examples", "run_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with tempfile.TemporaryDirectory() as d:
        vit_dir, clips = os.path.join(d, "vit"), os.path.join(d, "clips")
        ViTForImageClassification(cfg).load_state_dict(sd).save_pretrained(vit_dir)
        common = ["--concepts", "8", "--per-concept", "4", "--batch", "32", "--steps", "50", "--dtype", "bf16"]
        buf = io.StringIO()
        with redirect_stdout(buf):
            mod.main(common + ["--out", clips, "--npy"])
            mod.main(common + ["--score-against", clips, "--classifier", vit_dir])
        rec = json.loads(buf.getvalue().strip().splitlines()[-1])
    st = rec["stage_seconds_rank0"]
    return {"workload": rec["workload"], "stage_seconds_rank0": st, "score_share_of_generate": st["score"] / st["generate"],
            "image_2way_acc": rec["image_2way_acc"], "image_40way_acc": rec["image_40way_acc"], "ssim_mean": rec["ssim_mean"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_classifier.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--metric-dtype", default=None, choices=["fp32", "bf16", "fp16", "all"],
                    help="measure ONLY the arms of the call -- the tower in fp32 and in this 16-bit mode ('all': bf16 and fp16) -- in one "
                         "session, alternating (tools/metric_dtype_arms.py), and merge them into --out under 'metric_dtype_arms'")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/image_classifier_bench.py measures on the GPU: none found")
    from eeg2video_amd.image_classifier import ViTForImageClassification
    from eeg2video_amd.weights import ImageConfig, image_param_spec, synth_state_dict
    cfg = ImageConfig()
    sd = synth_state_dict(image_param_spec(cfg), seed=45, mode="perturbed")
    clf = ViTForImageClassification(cfg).load_state_dict(sd)
    eng = clf.engine
    n, F, H, W = 2 * a.clips, 6, 288, 512
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (n, F, H, W, 3), dtype=np.uint8))
    d_frames = frames.cuda()
    if a.metric_dtype:
        from metric_dtype_arms import measure_arms, merge_into
        arms = measure_arms(clf, lambda: eng.classify_frames(d_frames, channels_last=True), a.metric_dtype, a.repeats)
        arms["device"], arms["input"] = torch.cuda.get_device_name(0), f"{n * F} images of {H} x {W} uint8, channels-last, one call"
        merge_into(a.out, "metric_dtype_arms", arms)
        print(json.dumps({"tool": os.path.basename(__file__), "metric_dtype_arms": {k: v for k, v in arms.items() if k != "kernel_classes"}}))
        return
    wall = timed(lambda: eng.classify_frames(d_frames, channels_last=True), a.repeats)
    logits = eng.classify_frames(d_frames, channels_last=True)[0]
    torch.cuda.synchronize()
    eng.profile_begin()
    eng.classify_frames(d_frames, channels_last=True)
    prof = eng.profile_end()
    total = sum(v["ms"] for v in prof.values())
    split = {g: {"ms": sum(v["ms"] for k, v in prof.items() if k.startswith(names)),
                 "tflops": sum(v["flops"] for k, v in prof.items() if k.startswith(names)) / 1e9 /
                 max(sum(v["ms"] for k, v in prof.items() if k.startswith(names)), 1e-9)} for g, names in GROUPS.items()}
    split["other"] = {"ms": total - sum(v["ms"] for v in split.values())}
    for v in split.values():
        v["share"] = v["ms"] / total
    res = {"tool": "tools/image_classifier_bench.py", "device": torch.cuda.get_device_name(0),
           "model": "ViT-B/16 at 224 (google/vit-base-patch16-224's config), random weights, fp32",
           "input": {"images": n * F, "clips": n, "frames": F, "height": H, "width": W, "layout": "uint8 channels-last [n,F,H,W,3]"},
           "call_wall_ms": statistics.median(wall), "call_wall_ms_each": wall, "ms_per_image": statistics.median(wall) / (n * F),
           "profiled_run_total_ms": total, "split": split, "kernel_classes": prof, "device_bytes": eng.device_bytes()}
    try:
        import transformers  # noqa: F401
        have = True
    except ImportError:
        have = False
        res["torch"] = "transformers is not importable here: only the library's side was measured"
    if have:
        res["torch"] = torch_side(sd, cfg, frames.numpy(), logits, a.repeats)
        res["ours_over_torch_fp32_batched"] = res["call_wall_ms"] / res["torch"]["fp32_batched64_ms"]
    if a.sweep:
        del clf, eng
        torch.cuda.empty_cache()
        res["sweep_scored"] = scored_sweep(cfg, sd)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
