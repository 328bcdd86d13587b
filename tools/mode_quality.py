#!/usr/bin/env python3
"""What the 16-bit compute modes cost in the metrics the reference's users report: the same 8 clips (BASELINE configs[1] inputs:
bench.py's latents / conditioning, 50-step DDIM, CFG 12.5, synthetic SD-v1-4-size weights) generated in fp32, bf16 and fp16, and the
per-frame SSIM and MSE (``e2v_frame_metrics``: skimage's SSIM at data_range = 255, mse_loss of the bytes / 255) of each 16-bit mode's
frames against the fp32 frames, next to the max-abs figure the README states.

    python tools/mode_quality.py [--out profiles/mode_quality_<tag>.json] [--batch 8] [--steps 50]

Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mode_quality.json"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--guidance", type=float, default=12.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mode_quality.py measures on the GPU: none found")
    from eeg2video_amd.pipeline import build_pipeline
    from eeg2video_amd.weights import UNetConfig, VAEConfig, counter_normal, synth_state_dict, unet_param_spec, vae_param_spec
    ucfg, vcfg = UNetConfig(), VAEConfig()
    usd = synth_state_dict(unet_param_spec(ucfg), seed=42, mode="reference_init")
    vsd = synth_state_dict(vae_param_spec(vcfg), seed=43, mode="reference_init")
    eng = build_pipeline(ucfg, vcfg, device=0, unet_sd=usd, vae_sd=vsd).unet.engine
    dev, B = eng.device, a.batch
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    lat = torch.stack([t(counter_normal(1234 + k, "latent", (4, 6, 36, 64))) for k in range(B)]).to(dev)
    cond = torch.stack([t(counter_normal(1235 + 7919 * k, "cond", (77, 768))) for k in range(B)]).to(dev)
    unc = t(counter_normal(1236, "uncond", (1, 77, 768))).to(dev)
    frames, secs = {}, {}
    for mode in ("fp32", "bf16", "fp16"):
        eng.set_compute_dtype(mode)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames[mode] = eng.generate(lat, cond, unc, a.steps, a.guidance, 0.0, decode=True)
        torch.cuda.synchronize()
        secs[mode] = time.perf_counter() - t0                         # (first call of a mode: includes its warm-up)
    eng.set_compute_dtype("fp32")
    res = {"tool": "tools/mode_quality.py", "device": torch.cuda.get_device_name(0),
           "workload": f"{B} clips, {a.steps}-step DDIM, CFG {a.guidance}, 6x288x512, against the fp32 mode's frames",
           "first_call_seconds": secs, "modes": {}}
    for mode in ("bf16", "fp16"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ssim, mse = eng.frame_metrics(frames[mode], frames["fp32"])
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        s, m = ssim.double().cpu().numpy(), mse.double().cpu().numpy()
        res["modes"][mode] = {"ssim_mean": float(s.mean()), "ssim_std": float(s.std()), "ssim_min": float(s.min()),
                              "mse_mean": float(m.mean()), "mse_max": float(m.max()),
                              "psnr_db_of_mse_mean": float(-10 * np.log10(m.mean())) if m.mean() > 0 else None,
                              "max_abs": float((frames[mode] - frames["fp32"]).abs().max()), "frames_scored": int(s.size),
                              "score_call_ms": ms, "score_share_of_generate": ms / 1e3 / secs[mode]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
