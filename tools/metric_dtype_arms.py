"""What ``--metric-dtype`` of the three metric benchmarks (``tools/image_classifier_bench.py``, ``tools/video_classifier_bench.py``,
``tools/clip_score_bench.py``) shares: the arms of one call -- the tower in fp32 and in the 16-bit mode(s) named -- measured in ONE
session, alternating, so that a difference between arms is not a difference between sessions.

wall      host clock from the call to the end of a stream synchronisation; every arm is warmed first (the first 16-bit call derives the
          16-bit weight copies), then ``repeats`` rounds, each round one call per arm in turn.  ``ms`` is the median, ``ms_each`` the
          calls, ``spread`` (max - min) / median of the arm.
split     the library's event profile of one call per arm, in a run of its own after the timed rounds (the events serialise the
          launches): linears (``igemm*``), attention (``image_attn`` / ``flash_attn*``), rest (preprocess, embedding, LayerNorm,
          activation, pooling, head), ms and share of the profiled total.
"""
import json
import os
import statistics
import time

import torch

ATTENTION = ("image_attn", "flash_attn", "token_attn")


def measure_arms(model, call, dtype: str, repeats: int):
    """``model``: a mirror with ``set_compute_dtype``; ``call``: the timed call; ``dtype``: 'bf16', 'fp16', 'fp32' or 'all'"""
    arms = ["fp32"] + {"all": ["bf16", "fp16"], "fp32": []}.get(dtype, [dtype])
    eng = model.engine
    try:
        for d in arms:
            model.set_compute_dtype(d)
            call()
            call()
            torch.cuda.synchronize()
        wall = {d: [] for d in arms}
        for _ in range(repeats):
            for d in arms:
                model.set_compute_dtype(d)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                wall[d].append((time.perf_counter() - t0) * 1e3)
        out = {"arms": arms, "repeats": repeats, "order": "rounds of one call per arm, in the order of `arms`"}
        for d in arms:
            model.set_compute_dtype(d)
            torch.cuda.synchronize()
            eng.profile_begin()
            call()
            prof = eng.profile_end()
            total = sum(v["ms"] for v in prof.values())
            lin = sum(v["ms"] for k, v in prof.items() if k.startswith("igemm"))
            lin_flops = sum(v["flops"] for k, v in prof.items() if k.startswith("igemm"))
            att = sum(v["ms"] for k, v in prof.items() if k.startswith(ATTENTION))
            att_flops = sum(v["flops"] for k, v in prof.items() if k.startswith(ATTENTION))
            med = statistics.median(wall[d])
            out[d] = {"ms": med, "ms_each": wall[d], "spread": (max(wall[d]) - min(wall[d])) / med, "profiled_run_total_ms": total,
                      "split": {"linears": {"ms": lin, "share": lin / total, "tflops": lin_flops / 1e9 / max(lin, 1e-9)},
                                "attention": {"ms": att, "share": att / total, "tflops": att_flops / 1e9 / max(att, 1e-9)},
                                "rest": {"ms": total - lin - att, "share": (total - lin - att) / total}},
                      "kernel_classes": prof}
        for d in arms[1:]:
            out[d]["fp32_over_this"] = out["fp32"]["ms"] / out[d]["ms"]
        return out
    finally:
        model.set_compute_dtype("fp32")


def merge_into(path: str, key: str, value):
    """keep what ``path`` already records (the fp32 call, the torch side) and put ``value`` under ``key``"""
    rec = {}
    if os.path.isfile(path):
        with open(path) as fh:
            rec = json.load(fh)
    rec[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
