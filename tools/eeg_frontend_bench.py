#!/usr/bin/env python3
"""The EEG front end (``e2v_eeg_de_psd``, ``e2v_glmnet_raw``, ``e2v_glmnet_mlp``) at the reference's sizes against what runs today.

    python tools/eeg_frontend_bench.py [--out profiles/eeg_frontend_<tag>.json] [--rounds 5] [--batches 1 8 32] [--sweep]

glfnet      ``glfnet(2, 64, 62, 200)`` on the library against ``host_models.GLMNet`` on torch-ROCm on the same device, loaded with the
            SAME state dict (its key names are the reference's); the two outputs' distance is recorded too.
glfnet_mlp  ``glfnet_mlp(40, 64, 310)`` against the same ``nn.Linear`` / ``nn.GELU`` stacks in torch, the same state dict.
de_psd      ``e2v_eeg_de_psd`` over ``[B, 62, 400]`` -- its one 2-s window, and its seven 500-ms windows read through strides -- against
            ``torch.fft.fft(n=200)`` on the device followed by the band arithmetic, and against the numpy restatement on the host
            (``tests/eeg_features_restatement.py``: the reference's own route is float64 numpy on the CPU).
After warming every arm: ``--rounds`` rounds of one call per arm IN TURN, wall clock from the call to the end of a stream synchronise;
median (min .. max).  ``profiled_call``: the library's own event profile of one call, in a run of its own.
sweep       ``--sweep``: one bf16 B = 32 ``examples/run_sweep.py`` with the flags off and one with ``--glmnet native --features native``:
            the ``glmnet`` and ``features`` stages' seconds and shares.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

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


def compare(arms, rounds):
    """arms: name -> callable; warmed, then one call per arm in turn per round"""
    for _ in range(3):
        for fn in arms.values():
            fn()
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(once(fn))
    out = {k: summary(v) for k, v in ms.items()}
    names = list(arms)
    for other in names[1:]:
        out[f"speedup_median_vs_{other}"] = out[other]["median_ms"] / out[names[0]]["median_ms"]
        spread = (out[names[0]]["max_ms"] - out[names[0]]["min_ms"]) + (out[other]["max_ms"] - out[other]["min_ms"])
        out[f"faster_than_{other}_by_more_than_the_combined_spread"] = out[other]["median_ms"] - out[names[0]]["median_ms"] > spread
    return out


def profiled(eng, fn):
    torch.cuda.synchronize()
    eng.profile_begin()                                              # a run of its own: the events serialise the launches
    fn()
    prof = eng.profile_end()
    return {"launches": sum(v["launches"] for v in prof.values()), "total_ms": sum(v["ms"] for v in prof.values()),
            "kernel_classes": {k: {"launches": v["launches"], "ms": v["ms"]} for k, v in sorted(prof.items())}}


def torch_de_psd(x, bins):
    """``x`` ``[..., m]`` on the device -> de ``[..., 5]``: torch.fft.fft(n=200) of the windowed row, then the band arithmetic"""
    m = x.shape[-1]
    hann = 0.5 - 0.5 * torch.cos(2 * torch.pi * torch.arange(1, m + 1, device=x.device, dtype=torch.float32) / (m + 1))
    power = torch.fft.fft(x * hann, n=200).abs()[..., :100] ** 2
    psd = torch.stack([power[..., a:b + 1].sum(-1) / (b - a + 1) for a, b in bins], dim=-1)
    return torch.log2(100 * psd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()

    from torch import nn

    from eeg2video_amd.engine import Engine
    from eeg2video_amd.glmnet import glfnet, glfnet_mlp
    from eeg2video_amd.host_models import GLMNet
    from eeg2video_amd.weights import TINY_UNET, TINY_VAE, GLMNetConfig, counter_normal, glmnet_synth_state_dict
    from eeg_features_restatement import band_bins, de_psd, windows_of

    cfg = GLMNetConfig()
    eng = Engine(TINY_UNET, TINY_VAE, 0, glmnet_cfg=cfg)
    raw_sd, mlp_sd = glmnet_synth_state_dict(cfg, "raw", 48), glmnet_synth_state_dict(cfg, "mlp", 49)
    raw = glfnet(2, 64, 62, 200, engine=eng).load_state_dict(raw_sd)
    mlp = glfnet_mlp(40, 64, 310, engine=eng).load_state_dict(mlp_sd)
    as_t = lambda sd: {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    host = GLMNet(2, 64, 62, 200).to(eng.device).eval()
    host.load_state_dict(as_t(raw_sd))

    class TorchMlp(nn.Module):                                       # glfnet_mlp as three nn.Linear stacks, the reference's names
        def __init__(self):
            super().__init__()
            net = lambda i: nn.Sequential(nn.Flatten(), nn.Linear(i, 512), nn.GELU(), nn.Linear(512, 256), nn.GELU(), nn.Linear(256, 64))
            self.globalnet, self.occipital_localnet, self.out = nn.ModuleDict({"net": net(310)}), nn.ModuleDict({"net": net(60)}), nn.Linear(128, 40)

        def forward(self, x):
            return self.out(torch.cat((self.globalnet["net"](x), self.occipital_localnet["net"](x[:, 50:62])), 1))
    host_mlp = TorchMlp().to(eng.device).eval()
    host_mlp.load_state_dict(as_t(mlp_sd))
    bins = band_bins(200)
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())
    rec = {"config": "glfnet(2, 64, 62, 200), glfnet_mlp(40, 64, 310), DE_PSD at 200 Hz over [B, 62, 400]", "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "rounds": args.rounds, "batches": {}}
    for B in args.batches:
        seg_np = np.stack([20.0 * counter_normal(1000 + k, "segment", (62, 400)) for k in range(B)]).astype(np.float32)
        seg = torch.from_numpy(seg_np).to(eng.device)
        x = seg[:, :, :200].contiguous()
        de = torch.from_numpy(np.stack([counter_normal(3000 + k, "de", (62, 5)) for k in range(B)])).to(eng.device)
        entry = {}
        with torch.no_grad():
            entry["glfnet"] = compare({"native": lambda: raw(x), "host_torch": lambda: host(x[:, None])}, args.rounds)
            entry["glfnet"]["outputs_rel_distance"] = rel(raw(x), host(x[:, None]))
            entry["glfnet"]["profiled_call"] = profiled(eng, lambda: raw(x))
            entry["glfnet_mlp"] = compare({"native": lambda: mlp(de), "host_torch": lambda: host_mlp(de)}, args.rounds)
            entry["glfnet_mlp"]["outputs_rel_distance"] = rel(mlp(de), host_mlp(de))
            entry["glfnet_mlp"]["profiled_call"] = profiled(eng, lambda: mlp(de))
            one = dict(samples=400, strides=(62 * 400, 0, 400), batch=B, windows=1, electrodes=62, psd=False)
            seven = dict(samples=100, strides=(62 * 400, 50, 400), batch=B, windows=7, electrodes=62, psd=False)
            win = seg.unfold(2, 100, 50).permute(0, 2, 1, 3)         # [B, 7, 62, 100], a view
            entry["de_psd_2s"] = compare({"native": lambda: eng.eeg_de_psd(seg, **one), "torch_fft": lambda: torch_de_psd(seg, bins),
                                          "numpy_host": lambda: de_psd(seg_np, 200)}, args.rounds)
            entry["de_psd_2s"]["outputs_rel_distance"] = rel(eng.eeg_de_psd(seg, **one)[0][:, 0], torch_de_psd(seg, bins))
            entry["de_psd_7x500ms"] = compare({"native": lambda: eng.eeg_de_psd(seg, **seven), "torch_fft": lambda: torch_de_psd(win, bins),
                                               "numpy_host": lambda: de_psd(windows_of(seg_np, 100, 50), 200)}, args.rounds)
            entry["de_psd_7x500ms"]["outputs_rel_distance"] = rel(eng.eeg_de_psd(seg, **seven)[0], torch_de_psd(win, bins))
            entry["de_psd_7x500ms"]["profiled_call"] = profiled(eng, lambda: eng.eeg_de_psd(seg, **seven))
        rec["batches"][str(B)] = entry
        for k, v in entry.items():
            others = ", ".join(f"{n} {v[n]['median_ms']:.3f}" for n in v if isinstance(v[n], dict) and "median_ms" in v[n] and n != "native")
            print(f"B={B} {k}: native {v['native']['median_ms']:.3f} ms ({v['native']['min_ms']:.3f} .. {v['native']['max_ms']:.3f}); {others}", file=sys.stderr)
    if args.sweep:
        spec = importlib.util.spec_from_file_location("e2v_sweep", os.path.join(ROOT, "examples", "run_sweep.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        from eeg2video_amd.weights import SemanticConfig, UNetConfig, VAEConfig, synth_state_dict, unet_param_spec, vae_param_spec
        del raw, mlp, eng
        torch.cuda.empty_cache()
        big = Engine(UNetConfig(), VAEConfig(), 0, sem_cfg=SemanticConfig(), glmnet_cfg=GLMNetConfig(mlp_out=0))      # one engine for both arms
        big.load_state_dict(synth_state_dict(unet_param_spec(UNetConfig()), seed=42, mode="reference_init"))
        big.load_state_dict(synth_state_dict(vae_param_spec(VAEConfig()), seed=43, mode="reference_init"), prefix="vae.")
        big.finalize(Engine.UNET | Engine.VAE)
        sweep = {}
        for arm, flags in (("off", []), ("on", ["--glmnet", "native", "--features", "native"])):
            buf = io.StringIO()
            with redirect_stdout(buf):
                mod.main(["--concepts", "1", "--per-concept", "32", "--batch", "32", "--steps", "50", "--dtype", "bf16"] + flags, engine=big)
            line = json.loads(buf.getvalue().strip().splitlines()[-1])
            st = line["stage_seconds_rank0"]
            sweep[arm] = {"seconds": line["seconds"], "glmnet_s": st["glmnet"], "glmnet_share": st["glmnet"] / line["seconds"],
                          "features_s": st.get("features"), "features_share": st["features"] / line["seconds"] if "features" in st else None,
                          "stage_seconds_rank0": st, "workload": line["workload"]}
        rec["sweep_bf16_b32"] = sweep
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
