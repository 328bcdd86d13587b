"""Bit comparison of the norm kernels (and of temporal attention, which shares their lane reduction) between two builds of the library:
every GroupNorm / LayerNorm case of tests/h16_budget.py under every kernel form, in bf16 and fp16 (``GN_FORMS_AB`` and ``E2V_GN_GROUP_MB = 1`` too where the
library is a ``make ab`` build), the fp32 cases of tests/test_hip_ops.py (test_groupnorm_5d, test_groupnorm_concat_group_straddles_seam,
test_layernorm with E2V_LN_ROWS 1 and 0 and its ragged row counts) and every ``TEMPORAL_CASES`` form, one SHA-256 of the output bytes
per case.

    E2V_LIB_PATH=/path/to/other/libeeg2video_hip.so python tools/norm_bits.py a.json     # one build per process
    python tools/norm_bits.py b.json                                                      # the shipped build
    python tools/norm_bits.py --compare a.json b.json                                     # exit 1 on any difference
"""
import contextlib, hashlib, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sha(y):
    import torch
    return hashlib.sha256(y.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def digests():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import h16_budget as hb
    from eeg2video_amd.engine import Engine
    from eeg2video_amd.weights import TINY_UNET, TINY_VAE
    eng = Engine(TINY_UNET, TINY_VAE, 0)
    out = {}
    types = ["bf16", "fp16"]
    try:                                                 # a `make ab` build has the switches of the arms that were not adopted
        eng.set_knob("E2V_GN_ROWS", 1)
        ab = True
    except ValueError:
        ab = False

    @contextlib.contextmanager
    def form_of(ty, form, defaults):
        try:
            eng.set_compute_dtype(ty)
            for k, v in form.items():
                eng.set_knob(k, v)
            yield eng
        finally:
            for k in form:
                eng.set_knob(k, defaults[k])
            eng.set_compute_dtype("fp32")
    rnd = hb.rnd
    # fp32: the shapes of tests/test_hip_ops.py
    for c, groups, n, f, hw in [(320, 32, 2, 6, 40), (64, 32, 3, 3, 300), (960, 32, 1, 6, 100), (128, 8, 2, 1, 600)]:
        x = (rnd(n * f * hw, c, seed=30) * 2.0 + 0.7).cuda()
        ga, be = (rnd(c, seed=31) * 0.2 + 1.0).cuda(), (rnd(c, seed=32) * 0.2).cuda()
        for silu in (False, True):
            out[f"fp32 groupnorm C{c} g{groups} n{n} P{f * hw} silu{int(silu)}"] = _sha(
                eng.op_groupnorm(x, ga, be, samples=n, P=f * hw, groups=groups, eps=1e-5, silu=silu))
    a, s = rnd(2 * 500, 64, seed=33).cuda(), (rnd(2 * 500, 32, seed=34) * 3 - 1).cuda()
    ga, be = (rnd(96, seed=35) * 0.2 + 1.0).cuda(), (rnd(96, seed=36) * 0.2).cuda()
    out["fp32 groupnorm seam 64+32 g32"] = _sha(eng.op_groupnorm(a, ga, be, samples=2, P=500, groups=32, eps=1e-5, silu=True, x1=s))
    for c in (64, 320, 640, 1280, 768, 1032):
        x, g, b = (rnd(777, c, seed=40) * 3 + 1).cuda(), (rnd(c, seed=41) * 0.2 + 1).cuda(), (rnd(c, seed=42) * 0.2).cuda()
        for ln_rows in (1, 0):
            eng.set_knob("E2V_LN_ROWS", ln_rows)
            try:
                for rows in (777, 1, 3, 9):
                    out[f"fp32 layernorm C{c} rows{rows} LN_ROWS={ln_rows}"] = _sha(eng.op_layernorm(x[:rows].contiguous(), g, b))
            finally:
                eng.set_knob("E2V_LN_ROWS", 1)
    # 16-bit: the tables, under every form the library has
    gn_defaults = dict(hb.GN_DEFAULTS, E2V_GN_GROUP_MB=0)
    gn_forms = hb.GN_FORMS + [{"E2V_GN_FUSED_SMALL": 0}, {"E2V_GN_FUSED_SMALL": 3}] + (hb.GN_FORMS_AB + [{"E2V_GN_GROUP_MB": 1}] if ab else [])
    for ty in types:
        # (+ the 4-channels-per-lane case of tests/test_hip_ops.py, which the table's mutants cannot express)
        for case in hb.GN_CASES + [dict(id="quads_both_sources", samples=2, P=70, c0=60, c1=36, groups=8, silu=True)]:
            a, s, gamma, beta = (t.cuda() if t is not None else None for t in hb.gn_inputs(case))
            for form in gn_forms:
                with form_of(ty, form, gn_defaults) as e:
                    out[f"{ty} groupnorm {case['id']} [{hb.form_id(form)}]"] = _sha(
                        e.op_groupnorm(a, gamma, beta, samples=case["samples"], P=case["P"], groups=case["groups"], eps=1e-5, silu=case["silu"], x1=s))
        for case in hb.LN_CASES:
            if case["C"] > hb.LN_MAX_WIDTH:
                continue
            x, gamma, beta = (t.cuda() for t in hb.ln_inputs(case))
            for form in hb.LN_FORMS:
                with form_of(ty, form, hb.LN_DEFAULTS) as e:
                    out[f"{ty} layernorm {case['id']} [{hb.form_id(form)}]"] = _sha(e.op_layernorm(x, gamma, beta))
        for case in hb.TEMPORAL_CASES:
            qkv = hb.temporal_inputs(case).cuda()
            for form in case["forms"]:
                with form_of(ty, form, hb.TEMPORAL_DEFAULTS) as e:
                    out[f"{ty} temporal {case['id']} [{hb.form_id(form)}]"] = _sha(
                        e.op_temporal_attention(qkv, n=case["n"], F=case["f"], HW=case["hw"], heads=case["heads"], D=case["d"], scale=case["d"] ** -0.5))
    for case in hb.TEMPORAL_CASES:                       # fp32 rows through the same wave kernel
        qkv = hb.temporal_inputs(case).cuda()
        out[f"fp32 temporal {case['id']}"] = _sha(
            eng.op_temporal_attention(qkv, n=case["n"], F=case["f"], HW=case["hw"], heads=case["heads"], D=case["d"], scale=case["d"] ** -0.5))
    torch.cuda.synchronize()
    return out


def main(argv):
    if argv and argv[0] == "--compare":
        a, b = (json.load(open(p)) for p in argv[1:3])
        diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
        print(json.dumps({"cases": len(set(a) | set(b)), "byte_equal": len(set(a) | set(b)) - len(diff), "different": diff}))
        return 1 if diff else 0
    d = digests()
    json.dump(d, open(argv[0], "w"), indent=1)
    print(f"{len(d)} cases -> {argv[0]} (library: {os.environ.get('E2V_LIB_PATH', 'shipped')})")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
