#!/usr/bin/env python3
"""The video classifier (``e2v_video_classify``) at the scoring script's size: VideoMAE-B (``MCG-NJU/videomae-base-finetuned-kinetics``'s
config at ``num_frames=6``: 588 tokens; random weights), 64 clips (32 generated + 32 ground truth) x 6 frames of 288 x 512 uint8,
channels-last.

    python tools/video_classifier_bench.py [--out profiles/video_classifier_<tag>.json] [--repeats 5] [--sweep] [--no-torch]

call      wall clock from the call to the end of a stream synchronisation, each of ``--repeats`` after one warm-up (their spread is
          the session's run-to-run spread), for the 64 clips in one call.
split     the library's own event profile of one call, IN A RUN OF ITS OWN (the events serialise the launches): kernel classes folded
          into preprocess / linears / attention / head / other, ms and share.
attention the two routes to the token attention at the shape of one chunk of the call (16 clips x 12 heads x 588 tokens, and the stock
          16 frames' 1568): ``e2v_op_token_attention`` (what the call runs) against ``e2v_op_attention`` with mode 1, F = 1, n = B,
          Nq = Nk = T, D = 64 (``flash_attn_kernel<64>``, the UNet's kernel, which computes the same function), 20 launches per timed
          window between device events, the arms alternating, 5 windows each; and whether their bits agree.  (The yardstick of DESIGN 9:
          a dedicated kernel behind the first arm lost this comparison, so both arms now reach the same kernel and the ratio is the
          measurement's own noise; a future kernel behind ``e2v_op_token_attention`` is measured by the same lines.)
torch     if ``transformers`` is importable: ``transformers.VideoMAEForVideoClassification`` on torch-ROCm from the SAME weights, model
          forward only (pixel values already on the device) -- fp32 batched by 16 clips, and the reference's fp16 clip-by-clip loop
          (``40_class_run_metrics.py:131-135``) -- and the agreement of its fp32 logits with ours on the first two clips.
sweep     ``--sweep``: a scored sweep (``examples/run_sweep.py --score-against --classifier --video-classifier``, bf16, one batch of
          32 clips: all three metrics on) and the ``score`` stage's share of ``generate``.
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

GROUPS = {"preprocess": ("video_preprocess",), "linears": ("igemm",), "attention": ("token_attn", "flash_attn"),
          "head": ("image_head", "token_mean")}


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


def attention_ab(eng, B, T, heads, windows=5, launches=20):
    C = 64 * heads
    qkv = torch.randn(B * T, 3 * C, device="cuda", generator=torch.Generator("cuda").manual_seed(T))
    out_a, out_b = torch.empty(B * T, C, device="cuda"), torch.empty(B * T, C, device="cuda")
    arms = {"op_token_attention": lambda: eng.op_token_attention(qkv, B=B, T=T, heads=heads, out=out_a),
            "op_attention_mode1": lambda: eng.op_attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], n=B, F=1, heads=heads, D=64, Nq=T, Nk=T,
                                                           mode=1, scale=0.125, out=out_b)}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(windows):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / launches)
    flops = 4.0 * 64 * B * heads * T * T
    res = {"B": B, "T": T, "heads": heads, "launches_per_window": launches,
           "same_bits": bool(torch.equal(out_a.view(torch.int32), out_b.view(torch.int32))),
           "max_abs_diff": float((out_a - out_b).abs().max())}
    for name, v in ms.items():
        res[name] = {"ms_each": v, "ms": statistics.median(v), "spread": (max(v) - min(v)) / statistics.median(v),
                     "tflops": flops / 1e9 / statistics.median(v)}
    res["token_over_mode1"] = res["op_token_attention"]["ms"] / res["op_attention_mode1"]["ms"]
    return res


def torch_side(sd, cfg, frames_u8, ours_logits, repeats):
    import transformers
    from PIL import Image
    try:
        from transformers import VideoMAEImageProcessorPil as Processor
    except ImportError:
        from transformers import VideoMAEImageProcessor as Processor
    model = transformers.VideoMAEForVideoClassification(transformers.VideoMAEConfig(
        hidden_size=cfg.hidden, num_attention_heads=cfg.heads, num_hidden_layers=cfg.layers, intermediate_size=cfg.intermediate,
        image_size=cfg.image_size, patch_size=cfg.patch_size, tubelet_size=cfg.tubelet_size, num_frames=cfg.num_frames,
        num_labels=cfg.num_labels, layer_norm_eps=cfg.layer_norm_eps)).eval()
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    proc = Processor(size={"shortest_edge": cfg.resize_edge}, crop_size={"height": cfg.image_size, "width": cfg.image_size},
                     resample=Image.BILINEAR, rescale_factor=cfg.rescale_factor, image_mean=list(cfg.image_mean), image_std=list(cfg.image_std))
    t0 = time.perf_counter()
    first = torch.cat([proc(list(clip), return_tensors="pt")["pixel_values"] for clip in frames_u8[:2]])      # [2,F,3,S,S], as the processor makes them
    proc_ms = (time.perf_counter() - t0) * 1e3 / 2
    n = frames_u8.shape[0]
    res = {"transformers": transformers.__version__, "processor_host_ms_per_clip": proc_ms, "clips": n}
    px = torch.randn(n, cfg.num_frames, 3, cfg.image_size, cfg.image_size).clamp(-2, 2)
    px[:2] = first
    with torch.no_grad():
        m = model.to("cuda", torch.float32)
        x = px.cuda()
        res["fp32_batched16_ms_each"] = timed(lambda: [m(pixel_values=x[i:i + 16]).logits for i in range(0, n, 16)], repeats)
        ref = m(pixel_values=x[:2]).logits.double().cpu()
        res["fp32_logits_vs_ours_rel"] = float((ours_logits[:2].double().cpu() - ref).abs().max() / ref.abs().max())
        m = model.to("cuda", torch.float16)
        x = px.to("cuda", torch.float16)
        res["fp16_clip_by_clip_ms_each"] = timed(lambda: [m(pixel_values=x[i:i + 1]).logits for i in range(n)], max(1, repeats // 2))
    for k in ("fp32_batched16", "fp16_clip_by_clip"):
        res[k + "_ms"] = statistics.median(res[k + "_ms_each"])
    return res


def scored_sweep(vcfg, vsd):
    import importlib.util
    import io
    from contextlib import redirect_stdout
    from eeg2video_amd.image_classifier import ViTForImageClassification
    from eeg2video_amd.video_classifier import VideoMAEForVideoClassification
    from eeg2video_amd.weights import ImageConfig, image_param_spec, synth_state_dict
    spec = importlib.util.spec_from_file_location("e2v_sweep_bench", os.path.join(ROOT, "examples", "run_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with tempfile.TemporaryDirectory() as d:
        vit_dir, vmae_dir, clips = os.path.join(d, "vit"), os.path.join(d, "vmae"), os.path.join(d, "clips")
        icfg = ImageConfig()
        ViTForImageClassification(icfg).load_state_dict(synth_state_dict(image_param_spec(icfg), seed=45, mode="perturbed")).save_pretrained(vit_dir)
        VideoMAEForVideoClassification(vcfg).load_state_dict(vsd).save_pretrained(vmae_dir)
        torch.cuda.empty_cache()
        common = ["--concepts", "8", "--per-concept", "4", "--batch", "32", "--steps", "50", "--dtype", "bf16"]
        buf = io.StringIO()
        with redirect_stdout(buf):
            mod.main(common + ["--out", clips, "--npy"])
            mod.main(common + ["--score-against", clips, "--classifier", vit_dir, "--video-classifier", vmae_dir])
        rec = json.loads(buf.getvalue().strip().splitlines()[-1])
    st = rec["stage_seconds_rank0"]
    return {"workload": rec["workload"], "stage_seconds_rank0": st, "score_share_of_generate": st["score"] / st["generate"],
            **{k: rec[k] for k in ("image_2way_acc", "image_40way_acc", "video_2way_acc", "video_40way_acc", "ssim_mean")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_classifier.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--metric-dtype", default=None, choices=["fp32", "bf16", "fp16", "all"],
                    help="measure ONLY the arms of the call -- the tower in fp32 and in this 16-bit mode ('all': bf16 and fp16) -- in one "
                         "session, alternating (tools/metric_dtype_arms.py), and merge them into --out under 'metric_dtype_arms'")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/video_classifier_bench.py measures on the GPU: none found")
    from eeg2video_amd.video_classifier import VideoMAEForVideoClassification
    from eeg2video_amd.weights import VideoConfig, synth_state_dict, video_checkpoint_spec
    cfg = VideoConfig()
    sd = synth_state_dict(video_checkpoint_spec(cfg), seed=46, mode="perturbed")
    clf = VideoMAEForVideoClassification(cfg).load_state_dict(sd)
    eng = clf.engine
    n, F, H, W = 2 * a.clips, cfg.num_frames, 288, 512
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (n, F, H, W, 3), dtype=np.uint8))
    d_frames = frames.cuda()
    if a.metric_dtype:
        from metric_dtype_arms import measure_arms, merge_into
        arms = measure_arms(clf, lambda: eng.classify_clips(d_frames, channels_last=True), a.metric_dtype, a.repeats)
        arms["device"], arms["input"] = torch.cuda.get_device_name(0), f"{n} clips of {F} frames of {H} x {W} uint8, channels-last, one call"
        merge_into(a.out, "metric_dtype_arms", arms)
        print(json.dumps({"tool": os.path.basename(__file__), "metric_dtype_arms": {k: v for k, v in arms.items() if k != "kernel_classes"}}))
        return
    wall = timed(lambda: eng.classify_clips(d_frames, channels_last=True), a.repeats)
    logits = eng.classify_clips(d_frames, channels_last=True)[0]
    torch.cuda.synchronize()
    eng.profile_begin()
    eng.classify_clips(d_frames, channels_last=True)
    prof = eng.profile_end()
    total = sum(v["ms"] for v in prof.values())
    split = {g: {"ms": sum(v["ms"] for k, v in prof.items() if k.startswith(names)),
                 "tflops": sum(v["flops"] for k, v in prof.items() if k.startswith(names)) / 1e9 /
                 max(sum(v["ms"] for k, v in prof.items() if k.startswith(names)), 1e-9)} for g, names in GROUPS.items()}
    split["other"] = {"ms": total - sum(v["ms"] for v in split.values())}
    for v in split.values():
        v["share"] = v["ms"] / total
    res = {"tool": "tools/video_classifier_bench.py", "device": torch.cuda.get_device_name(0),
           "model": "VideoMAE-B/16 at 224, tubelets of 2, num_frames 6 (588 tokens), random weights, fp32",
           "input": {"clips": n, "frames": F, "height": H, "width": W, "layout": "uint8 channels-last [n,F,H,W,3]"},
           "call_wall_ms": statistics.median(wall), "call_wall_ms_each": wall, "ms_per_clip": statistics.median(wall) / n,
           "profiled_run_total_ms": total, "split": split, "kernel_classes": prof, "device_bytes": eng.device_bytes(),
           "attention_routes": [attention_ab(eng, 16, 588, cfg.heads), attention_ab(eng, 4, 1568, cfg.heads)]}
    have = not a.no_torch
    if have:
        try:
            import transformers  # noqa: F401
        except ImportError:
            have = False
            res["torch"] = "transformers is not importable here: only the library's side was measured"
    if have:
        res["torch"] = torch_side(sd, cfg, frames.numpy(), logits, a.repeats)
        res["ours_over_torch_fp32_batched"] = res["call_wall_ms"] / res["torch"]["fp32_batched16_ms"]
        res["torch_fp16_loop_over_ours"] = res["torch"]["fp16_clip_by_clip_ms"] / res["call_wall_ms"]
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
