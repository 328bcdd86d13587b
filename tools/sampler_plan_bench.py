#!/usr/bin/env python3
"""The plan loop (e2v_generate_plan) against the stepped loop, same process, same pipeline object, schedulers other than DDIM.

    python tools/sampler_plan_bench.py [--out profiles/sampler_plan_<tag>.json] [--passes 3] [--only pndm_b1_fp16,...]

Workload: SD-v1-4 shapes, synthetic weights, 6 x 288 x 512 clips (latents [B,4,6,36,64]), guidance 12.5.
  pndm_b1_fp16 / pndm_b1_bf16     the reference script's own call (inference_eeg2video.py:70,92-98 with the stock SD-v1-4 scheduler):
                                  PNDM, 100 steps, B = 1
  pndm_b8_bf16 / pndm_b8_fp32     PNDM, 50 steps, B = 8
  dpmpp_b8_bf16 / dpmpp_b8_fp32   DPM-Solver++ (2M), 50 steps, B = 8
Each configuration runs two arms of ``TuneAVideoPipeline.__call__``: "plan" (no callback: ``last_loop == "plan"``) and "stepped" (a
no-op ``callback``, which keeps the host-stepped loop -- the code path every scheduler but DDIM took before the plan loop existed).
One warm-up pass of each arm, then the arms alternate, ``--passes`` timed passes each.  The timer is the host clock around a call,
which ends in the D2H copy of the frames.  Per arm: median and spread (max - min) of the passes and the library's profiled launches
(HIP-event profile of a separate, untimed 5-step call, decode included; the difference of the arms per UNet evaluation is what the
plan loop saves per step -- its once-per-run work is spread over these few evaluations, and torch's own launches in the stepped arm,
cat / chunk / allocations, are not in it); per configuration ``e2v_device_bytes`` before its first call and after its last.  Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CONFIGS = {   # name -> (scheduler, steps, B, mode)
    "pndm_b1_fp16": ("PNDMScheduler", 100, 1, "fp16"),
    "pndm_b1_bf16": ("PNDMScheduler", 100, 1, "bf16"),
    "pndm_b8_bf16": ("PNDMScheduler", 50, 8, "bf16"),
    "dpmpp_b8_bf16": ("DPMSolverMultistepScheduler", 50, 8, "bf16"),
    "pndm_b8_fp32": ("PNDMScheduler", 50, 8, "fp32"),
    "dpmpp_b8_fp32": ("DPMSolverMultistepScheduler", 50, 8, "fp32"),
}
GUIDANCE = 12.5


def run_config(pipe, name, passes):
    from eeg2video_amd.scheduler import SCHEDULERS
    from eeg2video_amd.weights import counter_normal
    sched, steps, B, mode = CONFIGS[name]
    eng = pipe.unet.engine
    eng.set_compute_dtype(mode)
    pipe.scheduler = SCHEDULERS[sched](engine=eng)
    t = lambda seed, tag, shape: torch.from_numpy(np.ascontiguousarray(counter_normal(seed, tag, shape)))
    lat = t(1234, "latent", (B, 4, 6, 36, 64)).cuda()
    eeg = t(1235, "cond", (B, 77 * 768))
    neg = t(1236, "uncond", (1, 77, 768))
    noop = lambda i, ts, x: None

    def call(arm, n=steps):
        out = pipe(None, eeg, video_length=6, height=288, width=512, num_inference_steps=n, guidance_scale=GUIDANCE,
                   negative_prompt=neg, latents=lat, callback=noop if arm == "stepped" else None).videos
        assert pipe.last_loop == arm, (pipe.last_loop, arm)
        return out

    bytes_before = eng.device_bytes()
    arms = ("plan", "stepped")
    frames = {a: call(a) for a in arms}                              # warm-up of both
    diff = (frames["plan"] - frames["stepped"]).abs().max().item()
    finite = bool(torch.isfinite(frames["plan"]).all().item())
    times = {a: [] for a in arms}
    for _ in range(passes):
        for a in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(a)
            times[a].append(time.perf_counter() - t0)
    launches = {}
    for a in arms:                                                   # untimed, event-instrumented 5-step call
        call(a, 5)
        eng.profile_begin()
        call(a, 5)
        table = eng.profile_end()
        evals = 6 if sched == "PNDMScheduler" else 5
        launches[a] = {"profiled_launches_of_a_5_step_call": sum(v["launches"] for v in table.values()), "evaluations": evals,
                       "lincomb": table.get("lincomb", {}).get("launches", 0), "cfg_combine": table.get("cfg_combine", {}).get("launches", 0)}
    row = {"config": name, "scheduler": sched, "steps": steps, "B": B, "mode": mode, "guidance_scale": GUIDANCE, "passes": passes,
           "frames_max_abs_plan_vs_stepped": diff, "output_finite": finite,
           "device_bytes_before": bytes_before, "device_bytes_after": eng.device_bytes()}
    for a in arms:
        row[a] = {"s_median": statistics.median(times[a]), "s_spread": max(times[a]) - min(times[a]), "s_each": times[a],
                  "launches": launches[a]}
    row["stepped_over_plan"] = row["stepped"]["s_median"] / row["plan"]["s_median"]
    row["profiled_launches_saved_per_evaluation"] = (launches["stepped"]["profiled_launches_of_a_5_step_call"]
                                                     - launches["plan"]["profiled_launches_of_a_5_step_call"]) / launches["plan"]["evaluations"]
    print(f"{name}: plan {row['plan']['s_median']:.3f} s (spread {row['plan']['s_spread']:.3f}), stepped {row['stepped']['s_median']:.3f} s "
          f"(spread {row['stepped']['s_spread']:.3f}), stepped / plan {row['stepped_over_plan']:.4f}, frames differ by {diff:.2e}", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_plan.json"))
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated configuration names (default: all)")
    a = ap.parse_args()
    if a.passes < 3:
        ap.error("--passes: at least 3 timed passes per arm")
    names = [n for n in a.only.split(",") if n] or list(CONFIGS)
    from eeg2video_amd.pipeline import build_pipeline
    from eeg2video_amd.weights import UNetConfig, VAEConfig, synth_state_dict, unet_param_spec, vae_param_spec
    ucfg, vcfg = UNetConfig(), VAEConfig()
    usd = synth_state_dict(unet_param_spec(ucfg), seed=42, mode="reference_init")
    vsd = synth_state_dict(vae_param_spec(vcfg), seed=43, mode="reference_init")
    pipe = build_pipeline(ucfg, vcfg, device=0, unet_sd=usd, vae_sd=vsd)
    pipe.set_progress_bar_config(disable=True)
    del usd, vsd
    res = {"tool": "tools/sampler_plan_bench.py", "device": torch.cuda.get_device_name(0), "configs": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name in names:
        res["configs"].append(run_config(pipe, name, a.passes))
        with open(a.out, "w") as fh:                                 # (kept current: a run cut short leaves what it measured)
            json.dump(res, fh, indent=1)
    print(json.dumps({r["config"]: r["stepped_over_plan"] for r in res["configs"]}))


if __name__ == "__main__":
    main()
