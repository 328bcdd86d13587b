#!/usr/bin/env python3
"""In-place weight update against the full reload, at SD-v1-4 size with synthetic weights.

    python tools/weight_update_bench.py [--out profiles/weight_update_<tag>.json] [--reloads 2] [--repeats 10]

reload   ``UNet3DConditionModel.load_state_dict(full)`` on a built model: every tensor uploaded again and the part finalized again --
         the only way to move a weight before ``e2v_update_tensor``.  Wall clock around a device synchronisation, each pass reported.
update   ``sync_from`` of the tensors the fine-tuning script trains (``train_finetune_videodiffusion.py:47-51``: attn1.to_q, attn2.to_q,
         attn_temp.*) from device fp32 and from device fp16 sources: wall clock from the call to the end of a stream synchronisation,
         median of ``--repeats`` after one warm-up; ``enqueue_ms`` is the host time of the call alone.  Bytes moved = each source read
         once + every form written (fp32, bf16, and fp16 where it exists: ``e2v_op_weight_forms``); GB/s from the median.
Prints one JSON line and writes it to --out."""
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


def is_trainable(k):
    return ".attn1.to_q." in k or ".attn2.to_q." in k or ".attn_temp." in k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_update.json"))
    ap.add_argument("--reloads", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
    from eeg2video_amd import _lib
    from eeg2video_amd.pipeline import build_pipeline
    from eeg2video_amd.weights import UNetConfig, VAEConfig, synth_state_dict, unet_param_spec, vae_param_spec
    ucfg, vcfg = UNetConfig(), VAEConfig()
    usd = synth_state_dict(unet_param_spec(ucfg), seed=42, mode="reference_init")
    vsd = synth_state_dict(vae_param_spec(vcfg), seed=43, mode="reference_init")
    pipe = build_pipeline(ucfg, vcfg, device=0, unet_sd=usd, vae_sd=vsd)
    eng = pipe.unet.engine
    res = {"tool": "tools/weight_update_bench.py", "device": torch.cuda.get_device_name(0),
           "unet_parameters": int(sum(v.size for v in usd.values()))}

    reload_s = []
    for _ in range(a.reloads):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.unet.load_state_dict(usd)
        torch.cuda.synchronize()
        reload_s.append(time.perf_counter() - t0)
    res["reload_s_each"] = reload_s
    res["reload_s"] = min(reload_s)

    names = [k for k in usd if is_trainable(k)]
    res["update_tensors"] = len(names)
    res["update_parameters"] = int(sum(usd[k].size for k in names))
    bits = _lib.FORM_BITS
    for label, dt in (("device_fp32", torch.float32), ("device_fp16", torch.float16)):
        src = {k: torch.from_numpy(usd[k]).cuda().to(dt) for k in names}
        moved = 0
        for k, v in src.items():
            m = eng.weight_forms(k)
            per = v.element_size() + 4 * bool(m & bits["fp32"]) + 2 * bool(m & bits["bf16"]) + 2 * bool(m & bits["fp16"]) + 6 * bool(m & bits["x3"])
            moved += per * v.numel()
        stream = torch.cuda.current_stream()
        pipe.unet.sync_from(src)                             # warm-up
        stream.synchronize()
        total, enqueue = [], []
        for _ in range(a.repeats):
            stream.synchronize()
            t0 = time.perf_counter()
            pipe.unet.sync_from(src)
            t1 = time.perf_counter()
            stream.synchronize()
            total.append((time.perf_counter() - t0) * 1e3)
            enqueue.append((t1 - t0) * 1e3)
        ms = statistics.median(total)
        res[label] = {"ms_each": total, "ms": ms, "enqueue_ms": statistics.median(enqueue), "bytes_moved": moved,
                      "gbps": moved / ms / 1e6, "reload_over_update": res["reload_s"] * 1e3 / ms}
        del src
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
