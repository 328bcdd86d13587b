"""CPU: the restated fp32 tile schedule (tests/igemm_schedule.py) against the build, and the coverage of its case table.

tests/test_dispatch_golden.py ties tests/golden/dispatch_sd_v1_4.json to ``igemm()`` of this build; (a) ties ``schedule()`` to every
``igemm_f32`` line of that table, so the restatement is the library's rule.  (b)-(d) are about ``CASES``, the launches
tests/test_hip_igemm_schedule.py runs on the GPU: each reaches the class it was chosen for, together they reach every class the
production graph runs -- a rule change that makes a new class fails (c) instead of silently losing coverage --, and the sliced re-runs
they are compared with bit for bit stay on the narrow schedule the rest of the suite covers.
"""
import json
import os

import pytest

from igemm_schedule import (CASES, ROWS, chunk_tiles, kind_of, klass, launch_of, owner, parse_golden, region, sched_args, schedule,
                            schedule_of, slice_launches)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dispatch_sd_v1_4.json")
TABLES = ("fp32_b1", "fp32_b8", "fp32_b32")


def golden_launches():
    table = json.load(open(GOLDEN))
    return [(key, line) + parse_golden(line) for key in TABLES for line in table[key] if " igemm_f32 " in line]


def test_restatement_gives_every_golden_schedule():
    """(a) rb1, w and s of all igemm_f32 lines, the t9 ones included"""
    lines = golden_launches()
    assert len(lines) >= 228
    wrong = []
    for key, line, launch, recorded in lines:
        s = schedule(**sched_args(launch))
        if (s["rb1"], s["w1"], s["s1"]) != recorded:
            wrong.append(f"{key}: {line}\n    restated: rb1={s['rb1']} w{s['w1']} s{s['s1']}")
    assert not wrong, "\n".join(wrong)
    kinds = [kind_of(schedule(**sched_args(l[2]))) for l in lines if l[0] == "fp32_b1"]
    print({k: kinds.count(k) for k in ("mixed", "wide", "narrow")})
    assert kinds.count("mixed") + kinds.count("wide") > kinds.count("narrow")      # why the wide tiles need tests of their own


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_case_reaches_its_class(case):
    """(b)"""
    s, k = schedule_of(case), klass(**launch_of(case))
    assert (k[0], k[5], k[6]) == case["claim"], (k, s)
    assert {key: s[key] for key in case["more"]} == case["more"], s
    if k[0] == "mixed":                          # the seam lies inside every chunk: each runs wide row blocks, then tail ones
        assert all(n > s["tail_rb"] > 0 for n in s["chunks"]), s


def test_case_names_are_unique():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)


def test_cases_reach_every_class_of_the_production_table():
    """(c)"""
    golden = {}
    for key, line, launch, _ in golden_launches():
        golden.setdefault(klass(**launch), f"{key}: {line}")
    reached = {klass(**launch_of(c)) for c in CASES}
    print(f"{len(golden)} classes in the table, {len(reached)} reached by CASES")
    assert len(golden) >= 25
    missing = [f"{k}: e.g. {line}" for k, line in sorted(golden.items()) if k not in reached]
    assert not missing, "classes (schedule, taps, batched, geglu, cat, s1, masked, stride 2) without a case:\n" + "\n".join(missing)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_slices_are_narrow(case):
    """(d)"""
    for launch in slice_launches(case):
        s = schedule(**sched_args(launch))
        if case["kind"] == "geglu":              # never narrow; one row block per chunk at the most, as in the other GEGLU tests
            assert s["nbm"] <= 8, s
        else:
            assert kind_of(s) == "narrow", (launch, s)


def test_a_launch_below_one_round_is_narrow():
    for n in (64, 128, 200, 320, 1224, 1280):
        for nbm in range(1, 60):
            s = schedule(nbm * ROWS, n)
            if (s["w1"] + s["s1"]) * s["nbm"] < 512 - 8 * (s["w1"] + s["s1"]):        # (the rule sizes by the longest chunk)
                assert kind_of(s) == "narrow", (n, nbm, s)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_every_tile_is_owned_once(case):
    """owner() is a bijection between the (row block, column tile) pairs of the schedule and the workgroups that do not return early"""
    s = schedule_of(case)
    n = launch_of(case)["N"]
    seen = {}
    for rb in range(s["nbm"]):
        for col in range(0, n, 64):
            o = owner(s, rb, col)
            assert o["col0"] <= col < o["col0"] + int(o["shape"].split("x")[1])
            seen.setdefault(o["block"], set()).add((rb, o["col0"]))
    assert all(len(v) == 1 for v in seen.values())
    tiles = chunk_tiles(s)
    assert len(seen) == sum(tiles) and max(seen) < 8 * max(tiles)
    assert {"wide": {"wide", "s1"}, "narrow": {"tail"}}.get(kind_of(s), {"wide", "s1", "tail"}) >= \
        {owner(s, rb, col)["region"] for rb in range(s["nbm"]) for col in range(0, n, 64)}


def test_region_names_the_tile():
    by = {c["name"]: c for c in CASES}
    text = region(by["linear 6500x40x1160 bias_residual"], 700, 1155)      # chunk 0 owns row blocks 0..5, the last one is its tail
    assert "row block 5 (no. 5 of XCD chunk 0), tail region, column tile 18 (128x64 at column 1152)" in text
    text = region(by["linear 6500x40x1160 bias_residual"], 0, 1155)
    assert "row block 0 (no. 0 of XCD chunk 0), s1 region, column tile 9 (128x64 at column 1152), workgroup 72" in text
    text = region(by["geglu 1300x32"], 700, 100)                            # output column 100: h and gate in GEMM columns 196 and 228
    assert "wide region, column tile 1 (128x128 at column 128)" in text
    assert "Winograd tile 470 (row block 3 of each of the 36 batch entries" in region(by["winograd4 conv 6x35x46 32->320 rowbias resid"], 7000, 300)
