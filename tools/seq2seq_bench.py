#!/usr/bin/env python3
"""The Seq2Seq latent model (``e2v_seq2seq_latents``) at the reference's size against the stage the sweep runs today.

    python tools/seq2seq_bench.py [--out profiles/seq2seq_<tag>.json] [--rounds 5] [--batches 1 8 32] [--sweep]

call      ``myTransformer`` at its default config (62 x 100 windows x 7, d_model 512, 2 + 4 layers, 4 x 36 x 64 latents), synthetic
          weights, ``first = 0, count = 6`` (the reference's ``[:, :-1]``: five decoder passes), against ``host_models.Seq2SeqLatents``
          on torch-ROCm on the same device -- the same architecture run as six full passes.  After warming both arms: ``--rounds``
          rounds of one call per arm IN TURN, wall clock from the call to the end of a stream synchronise; median (min .. max).
split     the library's own event profile of one call per batch, IN A RUN OF ITS OWN (the events serialise the launches): launches per
          call and ms per kernel class; and, by differencing timed calls, what the phases cost -- windows + encoder (a call for the
          text logits alone), each further decoder pass (``count`` = 1 .. 6), the predictor with the layout (``count`` = 1).
sweep     ``--sweep``: one bf16 B = 32 ``examples/run_sweep.py`` with ``--seq2seq host`` and one with ``native`` in this session: the
          ``seq2seq`` stage's seconds and share in each (written beside ``--out`` as ``..._sweep_...json`` when ``--sweep-out`` is given).
Prints one JSON line and writes it to --out."""
import argparse
import importlib.util
import io
import json
import os
import statistics
import sys
import time
from contextlib import redirect_stdout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "each_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-out", default="")
    args = ap.parse_args()

    from eeg2video_amd.engine import Engine
    from eeg2video_amd.host_models import Seq2SeqLatents
    from eeg2video_amd.seq2seq import myTransformer
    from eeg2video_amd.weights import TINY_UNET, TINY_VAE, Seq2SeqConfig, counter_normal

    cfg = Seq2SeqConfig()
    eng = Engine(TINY_UNET, TINY_VAE, 0, seq2seq_cfg=cfg)
    model = myTransformer(cfg, engine=eng).init_synthetic(47)
    torch.manual_seed(0)
    host = Seq2SeqLatents(d_model=cfg.d_model, latent_shape=tuple(cfg.latent), frames=cfg.steps).to(eng.device).eval()
    rec = {"config": "myTransformer defaults: 7 windows of 62 x 100, d_model 512, heads 4, ffn 2048, 2 + 4 layers, 6 steps, latent 4x36x64",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": args.rounds, "batches": {}}
    for B in args.batches:
        x = torch.from_numpy(np.stack([counter_normal(2000 + k, "win", (cfg.windows, cfg.electrodes, cfg.samples)) for k in range(B)])).to(eng.device)
        native = lambda: model.predict_latents(x, layout="bfchw")
        with torch.no_grad():
            torch_arm = lambda: host(x).float()
            for _ in range(3):                                       # warm both arms (workspaces, torch's kernel selection)
                native()
                torch_arm()
            ours, theirs = [], []
            for _ in range(args.rounds):                             # one call per arm in turn
                ours.append(once(native))
                theirs.append(once(torch_arm))
        entry = {"native": summary(ours), "host_torch": summary(theirs)}
        entry["speedup_median"] = entry["host_torch"]["median_ms"] / entry["native"]["median_ms"]
        spread = (entry["native"]["max_ms"] - entry["native"]["min_ms"]) + (entry["host_torch"]["max_ms"] - entry["host_torch"]["min_ms"])
        entry["faster_by_more_than_the_combined_spread"] = entry["host_torch"]["median_ms"] - entry["native"]["median_ms"] > spread
        # phases, by differencing timed calls (median of the rounds each)
        call = lambda **kw: statistics.median([once(lambda: eng.seq2seq_latents(x, **kw)) for _ in range(args.rounds)])
        eng.seq2seq_latents(x, latents=False, txt_logits=True)
        enc = call(latents=False, txt_logits=True)
        by_count = []
        for count in range(1, cfg.steps + 1):
            eng.seq2seq_latents(x, count=count)
            by_count.append(call(count=count))
        entry["phases_ms"] = {"windows_and_encoder_and_txt": enc, "count_1_minus_encoder__predictor_row_and_layout": by_count[0] - enc,
                              "calls_count_1_to_6": by_count, "per_further_decoder_pass": [by_count[i] - by_count[i - 1] for i in range(1, len(by_count))]}
        torch.cuda.synchronize()
        eng.profile_begin()                                          # a run of its own: the events serialise the launches
        native()
        prof = eng.profile_end()
        entry["profiled_call"] = {"launches": sum(v["launches"] for v in prof.values()), "total_ms": sum(v["ms"] for v in prof.values()),
                                  "kernel_classes": {k: {"launches": v["launches"], "ms": v["ms"]} for k, v in sorted(prof.items())}}
        rec["batches"][str(B)] = entry
        print(f"B={B}: native {entry['native']['median_ms']:.3f} ms ({entry['native']['min_ms']:.3f} .. {entry['native']['max_ms']:.3f}), "
              f"host torch {entry['host_torch']['median_ms']:.3f} ms ({entry['host_torch']['min_ms']:.3f} .. {entry['host_torch']['max_ms']:.3f}), "
              f"{entry['profiled_call']['launches']} launches", file=sys.stderr)
    if args.sweep:
        spec = importlib.util.spec_from_file_location("e2v_sweep", os.path.join(ROOT, "examples", "run_sweep.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        from eeg2video_amd.weights import SemanticConfig, UNetConfig, VAEConfig, synth_state_dict, unet_param_spec, vae_param_spec
        del model, eng
        torch.cuda.empty_cache()
        big = Engine(UNetConfig(), VAEConfig(), 0, sem_cfg=SemanticConfig(), seq2seq_cfg=cfg)      # one engine for both arms, built as the sweep builds its own
        big.load_state_dict(synth_state_dict(unet_param_spec(UNetConfig()), seed=42, mode="reference_init"))
        big.load_state_dict(synth_state_dict(vae_param_spec(VAEConfig()), seed=43, mode="reference_init"), prefix="vae.")
        big.finalize(Engine.UNET | Engine.VAE)
        sweep = {}
        for arm in ("host", "native"):
            buf = io.StringIO()
            with redirect_stdout(buf):
                mod.main(["--concepts", "1", "--per-concept", "32", "--batch", "32", "--steps", "50", "--dtype", "bf16", "--seq2seq", arm], engine=big)
            line = json.loads(buf.getvalue().strip().splitlines()[-1])
            sweep[arm] = {"seconds": line["seconds"], "seq2seq_s": line["stage_seconds_rank0"]["seq2seq"],
                          "seq2seq_share": line["stage_seconds_rank0"]["seq2seq"] / line["seconds"], "stage_seconds_rank0": line["stage_seconds_rank0"],
                          "workload": line["workload"]}
        rec["sweep_bf16_b32"] = sweep
        if args.sweep_out:
            with open(args.sweep_out, "w") as f:
                json.dump({"device": rec["device"], "torch": rec["torch"], **sweep}, f, indent=1)
                f.write("\n")
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
