#!/usr/bin/env python3
"""Weight read-back at SD-v1-4 size with synthetic weights, bf16 mode.

    python tools/weight_readback_bench.py [--out profiles/weight_readback_<tag>.json] [--repeats 5]

device   ``UNet3DConditionModel.state_dict()``: every tensor gathered into a fresh device tensor (``e2v_read_tensor``, on_device = 1:
         one launch per tensor).  Wall clock from the call to the end of a stream synchronisation, median of ``--repeats`` after one
         warm-up; ``enqueue_ms`` is the host time of the call alone.  Bytes moved = each fp32 source read once + each fp32 result
         written once; GB/s from the median, and its share of the measured HBM copy rate (6.29 TB/s, MI355X_MICROARCH.md).  It is a
         whole-call rate over many small launches, not a kernel's share of peak.
host     ``state_dict(device="cpu")``: each tensor gathered into a pool block and copied into pageable host memory, one stream
         synchronisation per tensor.
save     ``save_pretrained`` into a temporary directory: the host leg plus the safetensors file.
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

import torch  # noqa: E402

HBM_MEASURED_GBPS = 6290.0


def timed(fn, repeats, stream):
    fn()                                                    # warm-up
    stream.synchronize()
    total, enqueue = [], []
    for _ in range(repeats):
        stream.synchronize()
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        stream.synchronize()
        total.append((time.perf_counter() - t0) * 1e3)
        enqueue.append((t1 - t0) * 1e3)
        del out
    return {"ms_each": total, "ms": statistics.median(total), "enqueue_ms": statistics.median(enqueue)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_readback.json"))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/weight_readback_bench.py measures on the GPU: none found")
    from eeg2video_amd.pipeline import build_pipeline
    from eeg2video_amd.weights import UNetConfig, VAEConfig, synth_state_dict, unet_param_spec, vae_param_spec
    ucfg, vcfg = UNetConfig(), VAEConfig()
    usd = synth_state_dict(unet_param_spec(ucfg), seed=42, mode="reference_init")
    vsd = synth_state_dict(vae_param_spec(vcfg), seed=43, mode="reference_init")
    pipe = build_pipeline(ucfg, vcfg, device=0, unet_sd=usd, vae_sd=vsd)
    pipe.unet.engine.set_compute_dtype("bf16")
    stream = torch.cuda.current_stream()
    params = int(sum(v.size for v in usd.values()))
    res = {"tool": "tools/weight_readback_bench.py", "device": torch.cuda.get_device_name(0), "compute_dtype": "bf16",
           "unet_tensors": len(usd), "unet_parameters": params}

    dev = timed(lambda: pipe.unet.state_dict(), a.repeats, stream)
    dev["bytes_moved"] = 8 * params
    dev["gbps"] = dev["bytes_moved"] / dev["ms"] / 1e6
    dev["share_of_measured_hbm"] = dev["gbps"] / HBM_MEASURED_GBPS
    res["state_dict_device"] = dev
    res["state_dict_host"] = timed(lambda: pipe.unet.state_dict(device="cpu"), max(1, a.repeats // 2), stream)
    with tempfile.TemporaryDirectory() as tmp:
        res["save_pretrained"] = timed(lambda: pipe.unet.save_pretrained(tmp), max(1, a.repeats // 2), stream)
        res["save_pretrained"]["file_bytes"] = os.path.getsize(os.path.join(tmp, "diffusion_pytorch_model.safetensors"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
