"""No GPU: the per-element budgets of ``tests/h16_budget.py`` are neither too tight for correct arithmetic nor too loose to see a wrong
kernel.  For every case of the table and both 16-bit types: (a) a torch emulation of the kernels' arithmetic (fp32 statistics / scores,
P rounded to the type, the output rounded to the type) stays within the budget of the float64 reference; (b) every mutant reference
that applies to the case -- one row, key or piece lost, a neighbour's counted in, a wrong count, a wrong source -- exceeds the budget at
least ``MUTANT_FACTOR`` times in every slab / row / frame it touches.  (b) is a condition on the case's inputs: a case that misses it is
reshaped (sentinels, a smaller slab), the budget is not touched.  ``tests/test_hip_h16_budget.py`` runs the same table on the kernels;
this file is what keeps that one from going blind.  Run with ``-s`` for the figures per case."""
import pytest
import torch

import h16_budget as hb

TYPES = ["bf16", "fp16"]
_ids = lambda cases: [c["id"] for c in cases]


def _check(case_id, ty, out, budget, emulated, mutant_refs, group_rows):
    """``mutant_refs``: (mutant, its reference dict) pairs.  Prints and asserts (a) and (b)."""
    emu = float(hb.ratios(emulated, out["ref"], budget).max())
    weakest, weakest_name = float("inf"), None
    for mutant, m in mutant_refs:
        per_group = hb.group_max(hb.ratios(m["ref"], out["ref"], budget), group_rows, m.get("row_mask"))[m["touched"]]
        assert len(per_group), f"{case_id} {ty}: mutant {mutant} touches nothing"
        if float(per_group.min()) < weakest:
            weakest, weakest_name = float(per_group.min()), (mutant, m["touched"][int(per_group.argmin())])
    print(f"\n{case_id} [{ty}]: emulation {emu:.3f} of the budget; weakest mutant {weakest:.1f} x budget "
          f"({weakest_name[0]} in group {weakest_name[1]}; {len(mutant_refs)} mutants)")
    assert emu <= 1.0, f"{case_id} {ty}: the emulation of correct arithmetic is at {emu:.3f} of the budget"
    assert weakest >= hb.MUTANT_FACTOR, f"{case_id} {ty}: mutant {weakest_name[0]} reaches only {weakest:.2f} x budget in group {weakest_name[1]}"


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("case", hb.GN_CASES, ids=_ids(hb.GN_CASES))
def test_groupnorm_budget(case, ty):
    x, gamma, beta = hb.gn_rounded(case, ty)
    kw = hb.gn_kwargs(case)
    out = hb.groupnorm_reference(x, gamma, beta, c0=case["c0"], **kw)
    budget = hb.norm_budget(out, gamma, ty)
    muts = [(m, hb.groupnorm_reference(x, gamma, beta, c0=case["c0"], mutant=m, **kw)) for m in hb.gn_mutants(case)]
    _check(case["id"], ty, out, budget, hb.groupnorm_emulation(x, gamma, beta, ty, **kw), muts, case["P"])
    if "constant_group" in case:                          # the constant group's reference is beta (SiLU of it), exactly
        P, cpg, g, slab = case["P"], x.shape[1] // case["groups"], case["constant_group"], (case["samples"] - 1) // 2
        want = beta.double()[g * cpg:(g + 1) * cpg]
        want = want * torch.sigmoid(want) if case["silu"] else want
        assert torch.equal(out["ref"][slab * P:(slab + 1) * P, g * cpg:(g + 1) * cpg], want.expand(P, cpg))


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("case", hb.LN_CASES, ids=_ids(hb.LN_CASES))
def test_layernorm_budget(case, ty):
    x, gamma, beta = hb.ln_inputs(case)
    x = hb.rt(x, ty)
    out = hb.layernorm_reference(x, gamma, beta)
    budget = hb.norm_budget(out, gamma, ty)
    muts = [(m, hb.layernorm_reference(x, gamma, beta, mutant=m)) for m in hb.ln_mutants(case)]
    _check(case["id"], ty, out, budget, hb.layernorm_emulation(x, gamma, beta, ty), muts, 1)


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("case", hb.SC_CASES, ids=_ids(hb.SC_CASES))
def test_sparse_causal_budget(case, ty):
    qkv = hb.sc_inputs(case)
    c = qkv.shape[1] // 3
    run = lambda **kw: hb.sparse_causal_reference(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], ty=ty, **hb.sc_kwargs(case), **kw)
    out = run()
    muts = [(m, run(mutant=m)) for m in hb.sc_mutants(case)]
    _check(case["id"], ty, out, hb.attention_budget(out, ty), run(emulate=True)["ref"], muts, case["nq"])


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("case", hb.CROSS_CASES, ids=_ids(hb.CROSS_CASES))
def test_cross_budget(case, ty):
    q, kv = hb.cross_inputs(case)
    c = q.shape[1]
    run = lambda **kw: hb.cross_reference(q, kv[:, :c], kv[:, c:], ty=ty, **hb.cross_kwargs(case), **kw)
    out = run()
    muts = [(m, run(mutant=m)) for m in hb.cross_mutants(case)]
    _check(case["id"], ty, out, hb.attention_budget(out, ty), run(emulate=True)["ref"], muts, case["nq"])


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("case", hb.TEMPORAL_CASES, ids=_ids(hb.TEMPORAL_CASES))
def test_temporal_budget(case, ty):
    qkv = hb.temporal_inputs(case)
    run = lambda **kw: hb.temporal_reference(qkv, ty=ty, **hb.temporal_kwargs(case), **kw)
    out = run()
    muts = [(m, run(mutant=m)) for m in hb.temporal_mutants(case)]
    _check(case["id"], ty, out, hb.attention_budget(out, ty), run(emulate=True)["ref"], muts, case["hw"])


def test_assert_within_budget_names_the_place():
    """The message of a failure carries what a reader needs to find the kernel path: here a GroupNorm that lost row 63 of sample 1."""
    case = hb.GN_CASES[2]
    x, gamma, beta = hb.gn_rounded(case, "bf16")
    kw = hb.gn_kwargs(case)
    out = hb.groupnorm_reference(x, gamma, beta, c0=case["c0"], **kw)
    budget = hb.norm_budget(out, gamma, "bf16")
    assert hb.assert_within_budget(out["ref"], out["ref"], budget, "self") == 0.0
    wrong = hb.groupnorm_reference(x, gamma, beta, c0=case["c0"], mutant=("drop_row", 63), **kw)["ref"]
    with pytest.raises(AssertionError, match=r"sample 0, row \d+ of 130 \(64-row chunk \d\), channel \d+ = group 1"):
        hb.assert_within_budget(wrong, out["ref"], budget, "groupnorm", hb.where_groupnorm(case))
    bad = out["ref"].clone()
    bad[7, 3] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        hb.assert_within_budget(bad, out["ref"], budget, "groupnorm", hb.where_groupnorm(case))
