"""Bit comparison of the fp32 GEMM epilogue between two builds of the library: every case of tests/test_hip_igemm_epilogue.py
(fenced operands, ragged M / N / K, bias / residual / time-embedding / GEGLU epilogues) and of tests/test_hip_igemm_schedule.py (the
mixed and wide tile schedules of the production graph), and every case of the 16-bit GEMM table (``GEMM_CASES`` of tests/h16_budget.py:
each in bf16 and in fp16, under the switches of its form, stored in 16 bits as the graph stores it), one SHA-256 of the output bytes per case.

    E2V_LIB_PATH=/path/to/other/libeeg2video_hip.so python tools/igemm_epilogue_bits.py a.json     # one build per process
    python tools/igemm_epilogue_bits.py b.json                                                      # the shipped build
    python tools/igemm_epilogue_bits.py --compare a.json b.json                                     # exit 1 on any difference
"""
import hashlib, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digests():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import test_hip_igemm_epilogue as t
    import test_hip_igemm_schedule as ts
    eng = t.make_engine()
    out = {}
    for module in (t, ts):
        for name, run in module.cases():
            y, _ = run(eng)
            out[name] = _sha(y)
    import h16_budget as hb
    import test_hip_h16_gemm_store as tg
    eng.set_knob("E2V_OP_IO16", 1)
    try:
        for ty in tg.TYPES:
            for case in sorted(hb.GEMM_CASES, key=lambda c: c["pid"]):           # (forms of one problem back to back: its operands are cached)
                with tg.form_of(eng, ty, case["form"]) as e:
                    out[f"h16 {case['id']} [{ty}]"] = _sha(tg.run(e, tg._problem(case["pid"], ty)))
    finally:
        eng.set_knob("E2V_OP_IO16", 0)
    return out


def _sha(y):
    import torch
    return hashlib.sha256(y.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


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
