#!/usr/bin/env python3
"""Long clips (video_length > 8): temporal_attn_long_kernel at the op level and the whole generate step at equal frame counts.

    python tools/long_clip_bench.py [--out profiles/long_clips_<tag>.json] [--ddim-steps 5] [--skip-op] [--skip-step]

op    the temporal attention op at the UNet's level-0/1/2 shapes (HW 2304 / 576 / 144, D 40 / 80 / 160, 8 heads), F in {6, 12, 16, 24,
      32}, bf16 rows with n = 16 samples and fp32 rows with n = 4: best of 5 event-timed launches, algorithmic GB/s as
      tools/tattn_micro.py counts it (q, k, v read once, o written once).  F = 6 is the wave kernel, F > 8 the long kernel.
step  e2v_generate (DDIM steps + CFG 12.5 + VAE decode) of SD-v1-4-sized random weights at equal frame counts: bf16 B = 32 x F = 6
      against B = 8 x F = 24 and B = 16 x F = 12 (and B = 2 x F = 24, a batch in the small-clip dispatch family), fp32 B = 8 x F = 6
      against B = 2 x F = 24.  One warm-up pass, the mean of >= 2 timed passes, and the temporal_attn share of the GPU time from
      profile_begin / profile_end in a separate untimed pass.
Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

LEVELS = [("L0", 2304, 40), ("L1", 576, 80), ("L2", 144, 160)]
FRAMES = [6, 12, 16, 24, 32]


def op_level(eng):
    rows = []
    for mode, n in (("bf16", 16), ("fp32", 4)):
        eng.set_compute_dtype(mode)
        for name, hw, d in LEVELS:
            for f in FRAMES:
                heads = 8
                c = heads * d
                qkv = torch.randn(n * f * hw, 3 * c, device="cuda")
                best = 1e9
                for _ in range(5):
                    eng.profile_begin()
                    eng.op_temporal_attention(qkv, n=n, F=f, HW=hw, heads=heads, D=d, scale=d ** -0.5)
                    best = min(best, eng.profile_end()["temporal_attn"]["ms"])
                byt = (4.0 if mode == "fp32" else 2.0) * 4 * n * f * hw * c
                row = {"mode": mode, "level": name, "n": n, "F": f, "HW": hw, "D": d, "heads": heads, "ms": best,
                       "gbps": byt / best / 1e6, "kernel": "temporal_attn_wave_kernel" if f == 6 else "temporal_attn_long_kernel"}
                print(f"op {mode} {name} n={n} F={f}: {best:.3f} ms {row['gbps']:.0f} GB/s", flush=True)
                rows.append(row)
                del qkv
    eng.set_compute_dtype("fp32")
    return rows


def step_level(pipe, ddim_steps, passes):
    from eeg2video_amd.weights import counter_normal
    eng = pipe.unet.engine
    legs = [("bf16", 32, 6), ("bf16", 8, 24), ("bf16", 16, 12), ("bf16", 2, 24), ("fp32", 8, 6), ("fp32", 2, 24)]
    out = []
    for mode, B, f in legs:
        eng.set_compute_dtype(mode)
        lat = torch.from_numpy(np.ascontiguousarray(counter_normal(1234, "latent", (B, 4, f, 36, 64)))).cuda()
        cond = torch.from_numpy(np.ascontiguousarray(counter_normal(1235, "cond", (B, 77, 768)))).cuda()
        unc = torch.from_numpy(np.ascontiguousarray(counter_normal(1236, "uncond", (1, 77, 768)))).cuda()
        run = lambda: eng.generate(lat, cond, unc, ddim_steps, 12.5, 0.0, decode=True)
        vid = run()                                           # warm-up
        torch.cuda.synchronize()
        finite = bool(torch.isfinite(vid).all().item())
        del vid
        times = []
        for _ in range(passes):
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        eng.profile_begin()                                   # untimed, event-instrumented pass
        run()
        table = eng.profile_end()
        tot = sum(v["ms"] for v in table.values())
        ta = table.get("temporal_attn", {"ms": 0.0, "launches": 0, "bytes": 0.0})
        s = float(np.mean(times))
        row = {"mode": mode, "B": B, "F": f, "ddim_steps": ddim_steps, "passes": passes, "s_per_pass": s, "s_each": times,
               "frames_per_s": B * f / s, "clips_per_s": B / s, "temporal_attn_share": ta["ms"] / tot if tot else 0.0,
               "temporal_attn_ms": ta["ms"], "temporal_attn_gbps": ta["bytes"] / (ta["ms"] * 1e6) if ta["ms"] else 0.0,
               "output_finite": finite}
        print(f"step {mode} B={B} F={f}: {s:.3f} s/pass {row['frames_per_s']:.1f} frames/s, temporal_attn {100 * row['temporal_attn_share']:.2f} % "
              f"({row['temporal_attn_gbps']:.0f} GB/s)", flush=True)
        out.append(row)
        del lat, cond, unc
        torch.cuda.empty_cache()
    eng.set_compute_dtype("fp32")
    by = {(r["mode"], r["B"], r["F"]): r for r in out}
    ratios = {
        "bf16_B8xF24_over_B32xF6_frames_per_s": by["bf16", 8, 24]["frames_per_s"] / by["bf16", 32, 6]["frames_per_s"],
        "bf16_B16xF12_over_B32xF6_frames_per_s": by["bf16", 16, 12]["frames_per_s"] / by["bf16", 32, 6]["frames_per_s"],
        "bf16_B2xF24_over_B8xF24_frames_per_s": by["bf16", 2, 24]["frames_per_s"] / by["bf16", 8, 24]["frames_per_s"],
        "fp32_B2xF24_over_B8xF6_frames_per_s": by["fp32", 2, 24]["frames_per_s"] / by["fp32", 8, 6]["frames_per_s"],
    }
    return out, ratios


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_clips.json"))
    ap.add_argument("--ddim-steps", type=int, default=5)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--skip-op", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    from eeg2video_amd.pipeline import build_pipeline
    from eeg2video_amd.weights import UNetConfig, VAEConfig, synth_state_dict, unet_param_spec, vae_param_spec
    res = {"tool": "tools/long_clip_bench.py", "device": torch.cuda.get_device_name(0)}
    ucfg, vcfg = UNetConfig(), VAEConfig()
    usd = synth_state_dict(unet_param_spec(ucfg), seed=42, mode="reference_init")
    vsd = synth_state_dict(vae_param_spec(vcfg), seed=43, mode="reference_init")
    pipe = build_pipeline(ucfg, vcfg, device=0, unet_sd=usd, vae_sd=vsd)
    del usd, vsd
    if not a.skip_op:
        res["op"] = op_level(pipe.unet.engine)
    if not a.skip_step:
        res["step"], res["ratios"] = step_level(pipe, a.ddim_steps, a.passes)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res.get("ratios", {})))


if __name__ == "__main__":
    main()
