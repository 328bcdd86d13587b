"""GPU: the GEMM-shaped ops of the 16-bit modes -- linear, GEGLU, 3x3 conv, the sub-pixel form of resize + conv, split-K, the two-source
linear -- run the way the GRAPH launches them (switch ``E2V_OP_IO16``: 16-bit output tensor of exactly M x N, 16-bit residual), every
element against the float64 reference of ``tests/h16_budget.py`` within its own budget: one rounding of the stored value plus the fp32
summation-order term.  The cases, their sentinels (cancellation rows at the tile edges, offset bias pieces at the tile seams,
time-embedding rows 6 apart) and the mutants they are proven sensitive to are the table of that module; ``tests/
test_h16_gemm_budget_host.py`` holds the table to its conditions without a GPU.  Every case names the kernel that has to serve it and
FAILS if ``e2v_op_last_dispatch`` (switch ``E2V_OP_RECORD``) names another.  Each test prints its largest error / budget and where it
lies, and how many elements differ from the fp32-output form of the same call rounded once (``-s``): DESIGN section 5 quotes them."""
import contextlib
import functools

import pytest
import torch

import h16_budget as hb

pytestmark = pytest.mark.gpu

TYPES = ["bf16", "fp16"]
RTOL, ATOL = 2e-5, 2e-5            # fp32 vs float64: the tolerance of tests/test_hip_ops.py::test_linear
GUARD_KIB = 64


@pytest.fixture(scope="module")
def eng():
    from eeg2video_amd.engine import Engine
    from eeg2video_amd.weights import TINY_UNET, TINY_VAE
    e = Engine(TINY_UNET, TINY_VAE, 0)
    try:
        e.set_knob("E2V_OP_IO16", 1)
        e.set_knob("E2V_OP_RECORD", 1)
        yield e
    finally:
        e.set_knob("E2V_OP_IO16", 0)
        e.set_knob("E2V_OP_RECORD", 0)


@contextlib.contextmanager
def form_of(eng, ty, form):
    """16-bit mode ``ty`` and the switches of ``form``; everything back to its default afterwards."""
    try:
        eng.set_compute_dtype(ty)
        for k, v in form.items():
            eng.set_knob(k, v)
        yield eng
        torch.cuda.synchronize()
    finally:
        try:
            for k in form:
                eng.set_knob(k, hb.GEMM_DEFAULTS[k])
            eng.set_knob("E2V_OP_IO16", 1)
            eng.set_knob("E2V_POOL_GUARD", 0)
        finally:
            eng.set_compute_dtype("fp32")


@functools.lru_cache(maxsize=6)
def _problem(pid, ty):
    return hb.gemm_problem(hb.GEMM_PROBLEM_BY_ID[pid], ty)


def _dev(p):
    """The case's operands on the device (kept with the problem: every form of a problem reuses them)."""
    if "dev" not in p:
        p["dev"] = {k: (p[k].cuda().contiguous() if p[k] is not None else None) for k in ("x0", "x1", "w", "bias", "rowbias", "resid")}
    return p["dev"]


def run(eng, p, resid_rounded=False):
    """``resid_rounded``: hand the op the residual already rounded to the type (for the fp32-output form, which would add it unrounded)."""
    case, d = p["case"], _dev(p)
    if resid_rounded and d["resid"] is not None:
        d = dict(d, resid=hb.rt(p["resid"], p["ty"]).cuda())
    if case["op"] == "linear":
        return eng.op_linear(d["x0"], d["w"], d["bias"], d["resid"], geglu=bool(case.get("geglu")), x1=d["x1"])
    up = 2 if case.get("up2x") else 1
    return eng.op_conv3x3(d["x0"], d["w"], d["bias"], x1=d["x1"], n_img=case["n_img"], Hs=case["Hs"], Ws=case["Ws"], Hi=up * case["Hs"],
                          Wi=up * case["Ws"], stride=case.get("stride", 1), pad_lo=case.get("pad_lo", 1), rowbias=d["rowbias"],
                          rows_per_sample=case.get("rps") or 1, resid=d["resid"])


def _served_by(eng, case, what):
    tags = eng.last_dispatch()
    assert case["expect"] in tags, f"{what}: expected `{case['expect']}`, the launch was served by `{tags}`"
    assert not case["refuse"] or case["refuse"] not in tags, f"{what}: `{case['refuse']}` must not serve this launch, it was `{tags}`"
    return tags


_PARAMS = [pytest.param(c, id=c["id"]) for c in hb.GEMM_CASES]


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("case", _PARAMS)
def test_gemm_store(eng, case, ty):
    """One case of the table: the dispatch, a finite result, every element within its budget.  Reported, not asserted: the elements that
    differ from round16(fp32-output form of the same call on the same rounded residual) -- zero where the two epilogues add in the same
    order."""
    p = _problem(case["pid"], ty)
    what = f"{case['id']} [{ty}]"
    if "sched256" in case:                     # a case chosen for a tile schedule of 256-row blocks: the restated rule names its class
        import igemm_schedule as sc
        s = sc.schedule(p["M"], p["N"], rows=256, slots=256)
        assert sc.kind_of(s) == case["sched256"]["kind"], f"{what}: the launch is {sc.kind_of(s)}, chosen as {case['sched256']['kind']}"
        what += f" ({sc.kind_of(s)} schedule: rb1={s['rb1']} w{s['w1']} s{s['s1']} s2={s['s2']} tail_rb={s['tail_rb']})"
    with form_of(eng, ty, case["form"]) as e:
        y = run(e, p).cpu()
        tags = _served_by(e, case, what)
        e.set_knob("E2V_OP_IO16", 0)
        y32 = run(e, p, resid_rounded=True).cpu()
    worst = hb.assert_within_budget(y, p["ref"], p["budget"], what, hb.where_gemm(p))
    ratio = (y.double() - p["ref"]).abs() / p["budget"]
    r, c = divmod(int(ratio.argmax()), ratio.shape[1])
    differ = int((hb.rt(y32, ty) != y).sum())
    print(f"\n{what}:{tags}: largest error / budget = {worst:.3f} at {hb.where_gemm(p)(r, c)}; "
          f"{differ} of {y.numel()} elements differ from round16(fp32-output form)")


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in hb.GEMM_CASES if c["guard"]])
def test_gemm_store_under_pool_guard(eng, case, ty):
    """The bounds test of the 16-bit store: each form's first case once more with E2V_POOL_GUARD -- the 16-bit output tensor is an
    exactly sized pool block between two poisoned guard zones.  No zone altered, at least as many blocks checked as the unguarded call
    took from the pool, the same bits as unguarded (so no NaN of the poison either: the unguarded run met its budget above)."""
    p = _problem(case["pid"], ty)
    what = f"{case['id']} [{ty}] guarded"
    with form_of(eng, ty, case["form"]) as e:
        before = e.pool_gets()
        y0 = run(e, p).cpu()
        taken = e.pool_gets() - before
        e.set_knob("E2V_POOL_GUARD", GUARD_KIB)
        e.pool_guard_report()                              # (the totals start here)
        standing = e.pool_guard_report()[0]                # no work since the last report: the blocks that are compared every time
        y1 = run(e, p).cpu()
        _served_by(e, case, what)
        checked, violations, text = e.pool_guard_report()
    print(f"\n{what}: {checked} blocks checked, {standing} of them standing ({taken} pool tensors per unguarded call), {violations} violations")
    assert violations == 0, f"{what}: {text}"
    assert taken >= 3 and checked - standing >= taken, (checked, standing, taken)
    assert bool(torch.isfinite(y1).all()), f"{what}: non-finite outputs under guard"
    assert torch.equal(y1.view(torch.int32), y0.view(torch.int32)), f"{what}: the guarded run differs from the unguarded one"


@pytest.mark.parametrize("ty", TYPES)
def test_geglu_gate_term_of_the_fp32_output_form(eng, ty):
    """DELTA_G, the one measured number of the GEGLU budget: the fp32-OUTPUT form (switch off -- not the code the cases above test;
    tests/test_hip_ops.py holds it to 1e-4 of this formula) against the float64 formula, per element, over the GEGLU problems of the
    table.  What the fp32 sums may cost is e32 = DELTA S; what an element is off BEYOND that is the gate's (hardware exp2 / rcp), as a
    multiple of |v| (|g| + 1): the largest max(|y - ref| - DELTA S, 0) / (|v| (|g| + 1)).  h16_budget.DELTA_G is twice the value observed
    when the table was written (two gate instruction sequences and two tile families share it); a run that observes more than the
    constant fails.  Also printed: the largest |y - ref| / (DELTA S), i.e. how much of e32 the fp32-output form uses."""
    worst, used = 0.0, 0.0
    for case in hb.GEGLU_PROBLEMS:
        p = _problem(case["pid"], ty)
        with form_of(eng, ty, {}) as e:
            e.set_knob("E2V_OP_IO16", 0)
            y = run(e, p).cpu().double()
        h = p["N"] // 2
        v, g = p["acc"][:, :h] + p["b"][:h], p["acc"][:, h:] + p["b"][h:]
        err = (y - p["ref"]).abs()
        obs = float((torch.clamp(err - hb.DELTA * p["S"], min=0.0) / (v.abs() * (g.abs() + 1.0))).max())
        frac = float((err / (hb.DELTA * p["S"])).max())
        print(f"\n{case['pid']} [{ty}] fp32-output GEGLU: largest excess over DELTA S / (|v| (|g| + 1)) = {obs:.3e}; largest |y - ref| / (DELTA S) = {frac:.3f}")
        worst, used = max(worst, obs), max(used, frac)
    print(f"\nGEGLU gate term [{ty}]: observed {worst:.3e} (constant {hb.DELTA_G[ty]:.3e}); the fp32-output form uses {used:.3f} of DELTA S")
    assert worst <= hb.DELTA_G[ty], f"{ty}: observed {worst:.3e} exceeds DELTA_G = {hb.DELTA_G[ty]:.3e}"


@pytest.fixture(params=["fp32", "f32x3"])
def eng32(request, eng):
    if request.param == "fp32":
        yield eng
        return
    from eeg2video_amd.engine import Engine
    from eeg2video_amd.weights import TINY_UNET, TINY_VAE
    e = Engine(TINY_UNET, TINY_VAE, 0)
    e.set_compute_dtype("f32x3")
    yield e


@pytest.mark.parametrize("case", [pytest.param(c, id=c["pid"]) for c in hb.CAT_PROBLEMS])
def test_two_source_linear_fp32_modes(eng32, case):
    """The 1x1 shortcut over [h ; skip] in the fp32 and f32x3 modes (both switches are ignored there): against float64 on the unrounded
    operands at the tolerance of test_linear.  The two sources are views with DIFFERENT row strides into wider buffers, so a second
    source read with the first one's stride cannot pass."""
    M, c0, c1, N = case["M"], case["c0"], case["c1"], case["N"]
    x, w, b = hb.rnd(M, c0 + c1, seed=700), hb.rnd(N, c0 + c1, seed=701) * (c0 + c1) ** -0.5, hb.rnd(N, seed=702)
    buf0 = torch.full((M, c0 + 8), float("nan"), device="cuda")
    buf1 = torch.full((M, c1 + 20), float("nan"), device="cuda")
    buf0[:, :c0], buf1[:, 4:4 + c1] = x[:, :c0].cuda(), x[:, c0:].cuda()
    y = eng32.op_linear(buf0[:, :c0], w.cuda(), b.cuda(), x1=buf1[:, 4:4 + c1]).cpu().double()
    ref = x.double() @ w.double().T + b.double()
    scale = float(ref.abs().max())
    err = float((y - ref).abs().max())
    print(f"\n{case['pid']} [{eng32.compute_dtype}]:{eng32.last_dispatch()}: max abs err {err:.3e} (ref scale {scale:.3e})")
    assert err <= ATOL * max(1.0, scale) + RTOL * scale, f"max abs err {err:.3e} (ref scale {scale:.3e})"
    one = eng32.op_linear(x.cuda(), w.cuda(), b.cuda()).cpu().double()          # the same K columns from one tensor
    assert float((one - ref).abs().max()) <= ATOL * max(1.0, scale) + RTOL * scale
