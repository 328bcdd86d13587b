"""No GPU: the budgets of ``tests/vae_attn_budget.py`` are neither too tight for correct arithmetic nor too loose to see a wrong kernel.
For every case of its tables and every mode the case runs in: (a) a float32 torch emulation of the kernels' arithmetic stays within the
budget of the float64 reference at every element -- scores, probabilities and output; (b) every mutant that applies to the case exceeds a
budget at least ``MUTANT_FACTOR`` times in every image (block) or row (softmax) it touches, in one of the quantities
``tests/test_hip_vae_attention.py`` checks there.  Both are conditions on the INPUTS of a case: a case that misses (b) gets other
sentinels, the budget is not touched.  Run with ``-s`` for the figures per case."""
import pytest
import torch

import vae_attn_budget as vb

_ids = lambda cases: [c["id"] for c in cases]
BLOCK_PARAMS = [pytest.param(c, m, id=f"{c['id']}-{m}") for c in vb.BLOCK_CASES for m in c["modes"]]


def _per_group(r, group_rows):
    return r.reshape(-1, group_rows, r.shape[-1]).amax((1, 2))


@pytest.mark.parametrize("case,mode", BLOCK_PARAMS)
def test_block_budget(case, mode):
    kw = dict(nimg=case["nimg"], HW=case["HW"], C=case["C"], mode=mode)
    qkv = vb.block_inputs(case)
    ref = vb.block_reference(qkv, **kw)
    budgets = dict(zip("spo", vb.block_budgets(ref, **kw)))
    emu = vb.block_reference(qkv, emulate=True, **kw)
    emu_ratio = {k: float(vb.ratio(emu[k], ref[k], budgets[k]).max()) for k in "spo"}
    weakest, weakest_name, count = float("inf"), None, 0
    for kind in vb.BLOCK_MUTANTS:
        if not vb.applicable((kind,), ref=ref, **{k: kw[k] for k in ("nimg", "HW", "C")}):
            continue
        m = vb.block_reference(qkv, mutant=(kind,), **kw)
        seen = torch.stack([_per_group(vb.ratio(m[k], ref[k], budgets[k]), case["HW"]) for k in "spo"]).amax(0)[m["touched"]]
        assert len(seen), f"{case['id']} {mode}: mutant {kind} touches nothing"
        count += 1
        if float(seen.min()) < weakest:
            weakest, weakest_name = float(seen.min()), (kind, m["touched"][int(seen.argmin())])
    print(f"\n{case['id']} [{mode}]: emulation at {emu_ratio['s']:.3f} / {emu_ratio['p']:.3f} / {emu_ratio['o']:.3f} of the score / probability / "
          f"output budget; weakest mutant {weakest:.1f} x budget ({weakest_name[0]} in image {weakest_name[1]}; {count} mutants)")
    for k, name in zip("spo", ("scores", "probabilities", "output")):
        assert emu_ratio[k] <= 1.0, f"{case['id']} {mode}: the emulation of correct arithmetic is at {emu_ratio[k]:.3f} of the {name} budget"
    assert weakest >= vb.MUTANT_FACTOR, f"{case['id']} {mode}: mutant {weakest_name[0]} reaches only {weakest:.2f} x budget in image {weakest_name[1]}"


def test_every_block_mutant_applies_somewhere():
    """the table reaches every mutant in every mode"""
    for mode in vb.MODES:
        hit = set()
        for case in vb.BLOCK_CASES:
            if mode not in case["modes"]:
                continue
            kw = dict(nimg=case["nimg"], HW=case["HW"], C=case["C"])
            ref = vb.block_reference(vb.block_inputs(case), mode=mode, **kw)
            hit |= {k for k in vb.BLOCK_MUTANTS if vb.applicable((k,), ref=ref, **kw)}
        assert hit == set(vb.BLOCK_MUTANTS), (mode, set(vb.BLOCK_MUTANTS) - hit)


SOFTMAX_MUTANT_ROWS = {"no_row_max": (1, 3, 4), "sum_first_256": (3, 6)}      # the rows of softmax_inputs built to show each


@pytest.mark.parametrize("out_mode", vb.SOFTMAX_OUT)
@pytest.mark.parametrize("cols", vb.SOFTMAX_COLS)
def test_softmax_budget(cols, out_mode):
    x = vb.softmax_inputs(cols)
    ref = vb.softmax_reference(x)
    budget = vb.softmax_budget(ref, out_mode)
    emu = float(vb.ratio(vb.softmax_emulation(x, out_mode), ref["p"], budget).max())
    weakest = float("inf")
    for kind, rows in SOFTMAX_MUTANT_ROWS.items():
        if kind == "sum_first_256" and cols <= 256:
            continue
        if kind == "no_row_max":
            assert bool((x[list(rows)].amax(-1) > vb.EXP_OVERFLOW).all())
        m = vb.softmax_reference(x, (kind,))
        weakest = min(weakest, float(vb.ratio(m["p"], ref["p"], budget).amax(-1)[list(rows)].min()))
    print(f"\nsoftmax {cols} columns [{out_mode}]: emulation at {emu:.3f} of the budget; weakest mutant {weakest:.1f} x budget")
    assert emu <= 1.0, f"softmax {cols} [{out_mode}]: the emulation of correct arithmetic is at {emu:.3f} of the budget"
    assert weakest >= vb.MUTANT_FACTOR, f"softmax {cols} [{out_mode}]: a mutant reaches only {weakest:.2f} x budget"
    # what the GPU test asserts about the special rows holds for the reference itself
    assert float((ref["p"][vb.CONSTANT_ROW] - 1.0 / cols).abs().max()) <= 1e-15
    others = torch.ones(cols, dtype=torch.bool)
    others[max(cols - 2, 0)] = False
    assert float(ref["p"][vb.DOMINANT_ROW][others].max()) < 2.0 ** -150          # below every fp32 number: exactly 0 on the device


@pytest.mark.parametrize("two_byte", [False, True])
@pytest.mark.parametrize("rows,cols", vb.TRANSPOSE_SHAPES)
def test_transpose_reference_and_mutant(rows, cols, two_byte):
    x = vb.transpose_inputs(rows, cols, two_byte)
    ref = vb.transpose_reference(x)
    assert ref.shape == (vb.TRANSPOSE_BATCH, cols, rows)
    for b, r, c in [(0, 0, 0), (1, rows - 1, 0), (2, 0, cols - 1), (2, rows - 1, cols - 1), (1, rows // 2, cols // 3)]:
        assert ref[b, c, r] == x[b, r, c]
    if vb.swap_extent(rows, cols) < 2:                   # (33 x 33: a corner tile of one element)
        return
    wrong = vb.transpose_reference(x, ("transpose_swap",))
    differs = (wrong != ref).reshape(vb.TRANSPOSE_BATCH, -1).sum(1)
    r0, c0 = vb.corner_tile(rows, cols)
    assert bool((differs > 0).all()), "the swap inside the ragged corner tile changes nothing: bit equality could not see it"
    assert torch.equal(wrong[:, :c0, :], ref[:, :c0, :]) and torch.equal(wrong[:, :, :r0], ref[:, :, :r0]), "the mutant reaches outside the corner tile"


def test_expf_ulps_counts_ulps():
    """the measuring helper: an exponential that is exact to fp32 rounding is within half an ulp, one that is 3 ulps off reads 3"""
    x = vb.softmax_inputs(260)
    d = x.float() - x.float().amax(-1, keepdim=True)
    good = torch.exp(d.double()).float()
    worst, _ = vb.expf_ulps(good, x)
    assert worst <= 0.5
    off = good.clone()
    off[0, 5] = torch.nextafter(torch.nextafter(torch.nextafter(off[0, 5], torch.tensor(9.0)), torch.tensor(9.0)), torch.tensor(9.0))
    worst, _ = vb.expf_ulps(off, x)
    assert 2.4 <= worst <= 3.6
