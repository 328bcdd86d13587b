#!/usr/bin/env python3
"""The CLIP text encoder at the full SD-v1-4 shape (12 layers, 768 / 12 heads / 3072, vocab 49408) with synthetic weights.

    python tools/text_encoder_bench.py [--out profiles/text_encoder_mi355x.json] [--calls 50] [--batches 1,8,32]

Per batch size (T = 77): ms per ``e2v_text_encode`` call -- a host clock around ``--calls`` back-to-back calls that end in a device
synchronise, after a warm-up call, best and median of 5 such windows -- then, in a separate event-instrumented pass
(``e2v_profile_begin`` / ``_end``), the split of the GPU time per kernel class, the share of the new attention and activation kernels,
and the sum of the kernel times: where that sum is far below the ms per call, the call is bound by its launches (8 per layer, 98
in all at 12 layers), not by its kernels.  Where ``transformers`` is importable the torch-ROCm fp32 ``CLIPTextModel`` is timed on the same ids and weights, and
the two outputs are compared (max |a-b| / max |b|).  Prints one JSON object and writes it to --out."""
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


def timed(run, calls, windows=5):
    run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(calls):
            run()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / calls)
    return {"ms_per_call_best": min(ms), "ms_per_call_median": statistics.median(ms), "windows": ms}


def torch_model(cfg, sd):
    try:
        from transformers import CLIPTextConfig, CLIPTextModel
    except Exception:
        return None
    tc = CLIPTextConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, intermediate_size=cfg.intermediate,
                        num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads, max_position_embeddings=cfg.max_positions,
                        hidden_act=cfg.hidden_act, layer_norm_eps=cfg.layer_norm_eps)
    model = CLIPTextModel(tc).eval()
    prefixed = any(k.startswith("text_model.") for k in model.state_dict())
    model.load_state_dict({(k if prefixed else k[len("text_model."):]): torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()},
                          strict=False)
    return model.cuda().float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_encoder_mi355x.json"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--batches", default="1,8,32")
    a = ap.parse_args()
    from eeg2video_amd.text_encoder import CLIPTextModel
    from eeg2video_amd.weights import TextConfig, synth_state_dict, text_param_spec
    cfg = TextConfig()
    sd = synth_state_dict(text_param_spec(cfg), seed=44, mode="perturbed")
    for k in sd:                                              # scores with spread, as in the tests
        if k.endswith("q_proj.weight") or k.endswith("k_proj.weight"):
            sd[k] = sd[k] * 4.0
    enc = CLIPTextModel(cfg).load_state_dict(sd)
    eng = enc.engine
    ref = torch_model(cfg, sd)
    c, i, t = cfg.hidden, cfg.intermediate, cfg.max_positions
    res = {"tool": "tools/text_encoder_bench.py", "device": torch.cuda.get_device_name(0), "config": cfg.__dict__, "T": t,
           "calls_per_window": a.calls, "torch_reference": ref is not None, "rows": []}
    g = torch.Generator().manual_seed(3)
    for b in [int(x) for x in a.batches.split(",")]:
        ids = torch.randint(0, cfg.vocab_size, (b, t), generator=g)
        out = torch.empty(b, t, c, device="cuda")
        row = {"B": b, "gflop": cfg.layers * (2.0 * b * t * (4 * c * c + 2 * c * i) + 4.0 * 64 * b * cfg.heads * t * (t + 1) / 2) / 1e9}
        row.update(timed(lambda: eng.text_encode(ids, out=out), a.calls))
        eng.profile_begin()
        eng.text_encode(ids, out=out)
        table = eng.profile_end()
        tot = sum(v["ms"] for v in table.values())
        new = sum(v["ms"] for k, v in table.items() if k.startswith("text_causal_attn") or k in ("text_quick_gelu", "text_gelu"))
        row.update({"classes": table, "kernel_ms_sum": tot, "launches": sum(v["launches"] for v in table.values()),
                    "attention_share": sum(v["ms"] for k, v in table.items() if k.startswith("text_causal_attn")) / tot,
                    "activation_share": sum(v["ms"] for k, v in table.items() if k in ("text_quick_gelu", "text_gelu")) / tot,
                    "new_kernels_share": new / tot, "kernel_ms_over_call_ms": tot / row["ms_per_call_best"],
                    "tflops_per_call": row["gflop"] / row["ms_per_call_best"]})
        if ref is not None:
            dev_ids = ids.cuda()
            with torch.no_grad():
                tr = timed(lambda: ref(input_ids=dev_ids)[0], a.calls)
                row["torch_fp32"] = tr
                y = ref(input_ids=dev_ids)[0].double()
            row["rel_err_vs_torch_fp32"] = ((out.double() - y).abs().max() / y.abs().max()).item()
            row["speedup_over_torch_fp32"] = tr["ms_per_call_best"] / row["ms_per_call_best"]
        print(f"B={b}: {row['ms_per_call_best']:.3f} ms/call (median {row['ms_per_call_median']:.3f}), kernels {tot:.3f} ms in "
              f"{row['launches']} launches, attention {100 * row['attention_share']:.1f} %, activation {100 * row['activation_share']:.1f} %"
              + (f", torch fp32 {row['torch_fp32']['ms_per_call_best']:.3f} ms" if ref is not None else ""), flush=True)
        res["rows"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({r["B"]: r["ms_per_call_best"] for r in res["rows"]}))


if __name__ == "__main__":
    main()
