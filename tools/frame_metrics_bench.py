#!/usr/bin/env python3
"""Frame metrics (``e2v_frame_metrics``) at the sweep's size: 32 clips x 6 frames x 3 channels at 288 x 512 = 576 single-channel
frames, the generated clips as the library leaves them (fp32, planar) against ground truth as ``imageio.mimread`` stacks it (uint8,
channels-last).

    python tools/frame_metrics_bench.py [--out profiles/frame_metrics_<tag>.json] [--repeats 20]

call      wall clock from the call to the end of a stream synchronisation, median of ``--repeats`` after one warm-up, and the kernel
          time of the ``frame_metrics`` class from the library's own event profile (both kernels of the call).  Algorithmic bytes =
          both inputs read once (5 bytes per sample); GB/s from the kernel time.
hbm       what ``tools/hbm_micro.py`` prints in the same session (a child process): the algorithmic GB/s of the project's other
          one-pass streaming kernels, for scale.
host      the float64 restatement of skimage's algorithm (tests/frame_metrics_restatement.py: scipy ``uniform_filter``, one thread)
          on one 288 x 512 x 3 frame of the same data, on this host -- what the reference's loop pays per frame -- and the agreement
          of the device scores with it over the first clip.
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_metrics.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--clips", type=int, default=32)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/frame_metrics_bench.py measures on the GPU: none found")
    from eeg2video_amd.engine import Engine
    from eeg2video_amd.weights import TINY_UNET, TINY_VAE
    from frame_metrics_restatement import clip_scores, quantise
    eng = Engine(TINY_UNET, TINY_VAE, 0)
    n, F, C, H, W = a.clips, 6, 3, 288, 512
    g = torch.Generator().manual_seed(0)
    # smooth frames with noise on top: scores away from both 0 and 1
    base = torch.nn.functional.interpolate(torch.rand((n * F, C, H // 16, W // 16), generator=g), size=(H, W), mode="bilinear")
    gen = (base + 0.08 * torch.randn(base.shape, generator=g)).clamp(0, 1).reshape(n, F, C, H, W).permute(0, 2, 1, 3, 4).contiguous()
    gt = ((base + 0.08 * torch.randn(base.shape, generator=g)).clamp(0, 1) * 255).to(torch.uint8).reshape(n, F, C, H, W)
    gt = gt.permute(0, 1, 3, 4, 2).contiguous()                                         # [n,F,H,W,C]
    d_gen, d_gt = gen.cuda(), gt.cuda()
    stream = torch.cuda.current_stream()
    ssim, mse = eng.frame_metrics(d_gen, d_gt, b_channels_last=True)                     # warm-up: the partials block is cached
    stream.synchronize()
    wall = []
    for _ in range(a.repeats):
        stream.synchronize()
        t0 = time.perf_counter()
        eng.frame_metrics(d_gen, d_gt, b_channels_last=True)
        stream.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    kern = []
    for _ in range(a.repeats):
        eng.profile_begin()
        eng.frame_metrics(d_gen, d_gt, b_channels_last=True)
        kern.append(eng.profile_end()["frame_metrics"])
    k_ms = statistics.median(k["ms"] for k in kern)
    res = {"tool": "tools/frame_metrics_bench.py", "device": torch.cuda.get_device_name(0),
           "shape": {"clips": n, "frames": F, "channels": C, "height": H, "width": W, "single_channel_frames": n * F * C},
           "inputs": "a: fp32 planar [n,C,F,H,W]; b: uint8 channels-last [n,F,H,W,C]",
           "call_wall_ms": statistics.median(wall), "call_wall_ms_each": wall, "kernel_ms": k_ms, "kernel_ms_each": [k["ms"] for k in kern],
           "algorithmic_bytes": kern[0]["bytes"], "algorithmic_gbps": kern[0]["bytes"] / k_ms / 1e6,
           "ssim_mean": float(ssim.double().mean()), "mse_mean": float(mse.double().mean())}

    micro = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hbm_micro.py")], capture_output=True, text=True, timeout=300)
    res["hbm_micro"] = {}
    for line in micro.stdout.splitlines():
        p = line.split()
        if len(p) >= 6 and p[2] == "ms" and p[4] == "GB/s":
            res["hbm_micro"][p[0]] = {"ms": float(p[1]), "algorithmic_gbps": float(p[3])}
    if micro.returncode != 0 or not res["hbm_micro"]:
        res["hbm_micro_error"] = (micro.stderr or micro.stdout)[-400:]

    pred = quantise(gen[0].permute(1, 2, 3, 0).numpy())                                  # clip 0 as [F,H,W,C] bytes
    t0 = time.perf_counter()
    clip_scores(pred[:1], gt[0].numpy()[:1])
    res["host_float64_ms_per_frame"] = (time.perf_counter() - t0) * 1e3
    want_s, want_m = clip_scores(pred, gt[0].numpy())
    res["max_abs_ssim_error_clip0"] = float(np.abs(ssim[0].cpu().double().numpy() - want_s).max())
    res["max_rel_mse_error_clip0"] = float((np.abs(mse[0].cpu().double().numpy() - want_m) / want_m).max())
    res["host_ms_for_these_frames"] = res["host_float64_ms_per_frame"] * n * F
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
