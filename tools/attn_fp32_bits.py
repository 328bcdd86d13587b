"""Bit comparison of the fp32 attention kernel between two builds of the library: every op-level case of
tests/test_hip_attn_fp32_tiles.py (``cases()``: the tile walks at D = 40 / 8 / 80 / 160, cross attention, the leftover-column pattern,
both rescale paths, large scores), one SHA-256 of the output bytes per case.

    E2V_LIB_PATH=/path/to/other/libeeg2video_hip.so python tools/attn_fp32_bits.py a.json     # one build per process
    python tools/attn_fp32_bits.py b.json                                                      # the shipped build
    python tools/attn_fp32_bits.py --compare a.json b.json                                     # exit 1 on any difference
"""
import hashlib, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digests():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import test_hip_attn_fp32_tiles as t
    eng = t.make_engine()
    out = {}
    for name, run in t.cases():
        y, _ = run(eng)
        out[name] = hashlib.sha256(y.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
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
