"""No GPU: the per-element budget of the GEMM-shaped ops stored in 16 bits (``tests/h16_budget.py``, GEMM section) is neither too tight
for correct arithmetic nor too loose to see a wrong epilogue.  For every case of the table and both 16-bit types: (a) a torch emulation
of the kernels' arithmetic (fp32 accumulation in 64-channel chunks; bias, time-embedding row and residual added in fp32; ONE rounding)
stays within the budget of the float64 reference; (b) its error before the rounding stays below the fp32 term e32 alone; (c) every
mutant reference that applies -- a neighbour row's residual, the other sample's time-embedding row under a 32-row chunk, bias and
residual of the piece to the left at a tile seam, the sum rounded before the residual is added, GEGLU halves exchanged or the last block
dropped, two sub-pixel parities exchanged, the last split-K run left out, the second source read with the first one's stride or from a
seam one chunk early -- exceeds the budget at least ``MUTANT_FACTOR`` times somewhere in every row, chunk, piece or block it touches.
(c) is a condition on the case's inputs (cancellation rows, offset bias pieces, time-embedding rows 6 apart), never on the budget.
``tests/test_hip_h16_gemm_store.py`` runs the same table on the kernels.  Run with ``-s`` for the figures per case."""
import pytest
import torch

import h16_budget as hb

TYPES = ["bf16", "fp16"]


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("case", hb.GEMM_CASES, ids=[c["id"] for c in hb.GEMM_CASES])
def test_gemm_store_budget(case, ty):
    p = hb.gemm_problem(case, ty)
    ref, budget = p["ref"], p["budget"]
    assert ref.shape == (p["M"], p["No"]) and bool(torch.isfinite(ref).all()) and bool((budget > 0).all())
    y, y32 = hb.gemm_emulation(p)
    emu = float(((y - ref).abs() / budget).max())
    e32 = hb.DELTA * p["S"] + p["extra"]
    sum_err = float(((y32 - ref).abs() / e32).max())
    weakest, weakest_name, n = float("inf"), None, 0
    for name, groups in hb.gemm_mutants(p, case["form"]):
        assert groups, f"{case['id']} {ty}: mutant {name} touches nothing"
        for label, rows, cols, mref in groups:
            n += 1
            ratio = float(((mref - ref[rows][:, cols]).abs() / budget[rows][:, cols]).max())
            if ratio < weakest:
                weakest, weakest_name = ratio, (name, label)
    print(f"\n{case['id']} [{ty}]: emulation {emu:.3f} of the budget, its fp32 part {sum_err:.3f} of e32; " +
          (f"weakest mutant {weakest:.1f} x budget ({weakest_name[0]} in {weakest_name[1]}; {n} groups)" if n else "no mutant applies"))
    assert emu <= 1.0, f"{case['id']} {ty}: the emulation of correct arithmetic is at {emu:.3f} of the budget"
    assert sum_err < 1.0, f"{case['id']} {ty}: the emulation's error before the rounding is {sum_err:.3f} of e32"
    assert weakest >= hb.MUTANT_FACTOR, f"{case['id']} {ty}: mutant {weakest_name[0]} reaches only {weakest:.2f} x budget in {weakest_name[1]}"


def test_every_form_of_the_table_has_its_cases():
    """The forms the issue names, each with a bounds case; a case's sentinels exist where its mutants need them."""
    forms = {c["form_name"] for c in hb.GEMM_CASES}
    assert forms == {"default", "tile", "pers", "256s3", "t256", "t256p_blds1", "t256p_blds0", "splitk2", "splitk5", "up2x", "cat", "cat_pers"}
    for f in forms:
        assert sum(c["guard"] for c in hb.GEMM_CASES if c["form_name"] == f) == 1
    for c in hb.GEMM_CASES:
        M, N, No = hb.gemm_shape(c)
        assert M > 0 and No > 0 and not (c.get("geglu") and (c.get("resid") or c.get("rps")))
    assert hb.gemm_shape(hb.GEMM_PROBLEM_BY_ID["conv128to256_2x8x12_s2_rps24r"])[0] == 48 and hb.gemm_shape(hb.GEMM_PROBLEM_BY_ID["conv64to128_3x8x23_rps184r"])[0] == 2 * 256 + 40


def test_256_row_cases_beyond_the_narrow_schedule():
    """The two `256s3` cases chosen for the mixed and the wide schedule of 256-row tiles are of that class: the restated rule, generalised
    to 256-row blocks and 256 slots, says so; the form's other cases are narrow (three row blocks)."""
    import igemm_schedule as sc
    kinds = {}
    for c in hb.GEMM_CASES:
        if c["form_name"] != "256s3":
            continue
        M, N, _ = hb.gemm_shape(c)
        s = sc.schedule(M, N, rows=256, slots=256)
        kinds[c["pid"]] = sc.kind_of(s)
        for k, v in c.get("sched256", {}).items():
            assert (sc.kind_of(s) if k == "kind" else s[k]) == v, f"{c['id']}: {k} is {s.get(k, sc.kind_of(s))}, the table claims {v}"
    assert kinds == {"lin552x320x192r": "narrow", "conv64to128_3x8x23_rps184r": "narrow", "lin45500x64x192r": "mixed", "lin65000x64x192r": "wide"}


def test_gate_restates_the_kernels_formula():
    """bf16: the logistic form within 2.8e-4 of erf-GELU (the bound the kernel's comment states); fp16: the erf form itself."""
    x = torch.linspace(-8, 8, 4001, dtype=torch.float64)
    exact = torch.nn.functional.gelu(x)
    assert float((hb.gate(x, "bf16") - exact).abs().max()) < 2.8e-4
    assert float((hb.gate(x, "fp16") - exact).abs().max()) < 1e-12
    d = (hb.gate(x + 1e-6, "bf16") - hb.gate(x - 1e-6, "bf16")) / 2e-6
    assert float(d.abs().max()) < hb.GATE_SLOPE
