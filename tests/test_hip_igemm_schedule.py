"""GPU: the fp32 GEMM and convs at the tile schedules the graph really runs (csrc/igemm.hip: igemm(), "tile schedule").

A launch below one round of 512 tiles runs 128x64 tiles only (*narrow*), and that is all the other op-level tests reach; the production
graph mostly runs *mixed* and *wide* launches -- 128x128 tiles, the 128x64 ``s1`` tile behind them, the masked wide tile, the seam
between wide and tail tiles inside an XCD chunk, batched Winograd GEMMs on wide tiles.  tests/igemm_schedule.py restates the rule and
lists ``CASES`` that reach every class of the production dispatch table (tests/test_igemm_schedule_host.py).  Each case here:

* operands and output in poisoned, fenced buffers (tests/test_hip_bounds.py), ``x`` with a padded row stride;
* the schedule is the claimed one: ``e2v_op_last_dispatch`` of a ``taps = 1`` launch carries ``rb1 / w / s``, which must be the
  restatement's (the record of ``igemm_kernel`` carries none: the host test ties the restatement to the build for the ``t9`` lines);
* a per-element budget against float64 -- linears and direct convs:
  ``|y - ref| <= (K + 4) 2^-24 (sum_k |x_ik| |w_jk| + |bias_j| + |rowbias| + |resid_ij|)``, the forward bound of a length-K
  multiply-add chain in any order plus at most three epilogue additions, computed from the operands; Winograd convs and GEGLU keep the
  bound of their own tests;
* bit identity with the narrow schedule: the same operands re-run in slices that are narrow launches (linears: 1000 rows at a time,
  convs: one image at a time) must give the same bits in every row -- a 128x64 and a 128x128 tile give an output the same k order.

A failure names the row block, column tile, region (wide / s1 / tail) and XCD chunk of the worst element (igemm_schedule.region).
``cases()`` lists (name, run) for tools/igemm_epilogue_bits.py.
"""
import os

import pytest
import torch
import torch.nn.functional as F

from igemm_schedule import CASES, SLICE_ROWS, case_named, conv_out_hw, kind_of, region, schedule_of, wino_m
from test_hip_bounds import BOUNDS, fenced, fenced_out, make_engine, rnd, run_fenced, to_cl

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                     # unit roundoff of fp32
RTOL, ATOL = 2e-5, 2e-5            # tests/test_hip_ops.py: test_linear_geglu
X3_BOUND = 4e-5                    # tests/test_hip_model.py: test_f32x3_mode_unet_vae_and_ops_vs_oracle, of the output scale
X3_ROWS = ("linear 6500x16x1280 none", "linear 9500x16x1224 bias_residual", "winograd4 conv 6x35x46 32->320 rowbias resid")
SCHEDULE_SWITCHES = ("E2V_IGEMM_SCHED", "E2V_IGEMM_K16", "E2V_IGEMM_ABLATE")


def default_schedule_or_fail():
    """the restatement is the rule at its defaults: with one of the switches set this module fails, it does not skip"""
    found = [k for k in SCHEDULE_SWITCHES if k in os.environ]
    if found:
        pytest.fail(f"{', '.join(found)} set in the environment: the tile schedule under test is the default one")


def recording_engine():
    e = make_engine()
    e.set_knob("E2V_OP_RECORD", 1)
    return e


@pytest.fixture(scope="module")
def eng():
    default_schedule_or_fail()
    e = recording_engine()
    try:
        yield e
    finally:
        e.set_knob("E2V_OP_RECORD", 0)


@pytest.fixture(scope="module")
def eng_x3():
    default_schedule_or_fail()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("E2V_F32X3", "1")                       # read when the context is created
        e = recording_engine()
    try:
        yield e
    finally:
        e.set_knob("E2V_OP_RECORD", 0)


# ------------------------------------------------------------------ operands and float64 references ---------------------------------
_shared = {}                       # operands and references of the cases the f32x3 arm runs again: computed once, never written


def problem(case):
    if case["name"] in _shared:
        return _shared[case["name"]]
    p = {"linear": linear_problem, "geglu": geglu_problem, "conv": conv_problem}[case["kind"]](case)
    if case["name"] in X3_ROWS:
        _shared[case["name"]] = p
    return p


def linear_problem(case):
    m, k, n = case["M"], case["K"], case["N"]
    x, w = rnd(m, k, seed=20), rnd(n, k, seed=21, scale=0.05)
    b = rnd(n, seed=22) if case["epilogue"] != "none" else None
    r = rnd(m, n, seed=23) if case["epilogue"] == "bias_residual" else None
    ref = x.double() @ w.double().T
    mag = x.double().abs() @ w.double().abs().T
    if b is not None:
        ref, mag = ref + b.double(), mag + b.double().abs()
    if r is not None:
        ref, mag = ref + r.double(), mag + r.double().abs()
    return dict(x=x, w=w, b=b, r=r, ref=ref, budget=(k + 4) * U * mag)


def geglu_problem(case):
    m, c = case["M"], case["c"]
    x, w, b = rnd(m, c, seed=24), rnd(8 * c, c, seed=25, scale=0.1), rnd(8 * c, seed=26)
    h, g = F.linear(x.double(), w.double(), b.double()).chunk(2, dim=-1)
    return dict(x=x, w=w, b=b, r=None, ref=h * F.gelu(g))


def conv_problem(case):
    n, h, w, cin, cout = case["n"], case["h"], case["w"], case["cin"], case["cout"]
    ho, wo = conv_out_hw(case)
    x, wt, b = rnd(n, cin, h, w, seed=1), rnd(cout, cin, 3, 3, seed=2, scale=0.1), rnd(cout, seed=3)
    temb = rnd(n, cout, seed=4) if case["rowbias"] else None
    res = to_cl(rnd(n, cout, ho, wo, seed=5)) if case["resid"] else None
    src = x.double()
    if case["up"] > 1:                                     # the nearest resize by a whole factor
        src = src.repeat_interleave(case["up"], 2).repeat_interleave(case["up"], 3)
    cols = F.unfold(src, 3, padding=1, stride=case["stride"]).permute(0, 2, 1).reshape(n * ho * wo, cin * 9)      # [rows, cin x 9 taps]
    w2 = wt.double().reshape(cout, cin * 9)
    ref = cols @ w2.T + b.double()
    mag = cols.abs() @ w2.abs().T + b.double().abs()       # (Winograd cases: unused, their bound is the global one of their own tests)
    if temb is not None:
        t = temb.double().repeat_interleave(ho * wo, 0)
        ref, mag = ref + t, mag + t.abs()
    if res is not None:
        ref, mag = ref + res.double(), mag + res.double().abs()
    return dict(x=to_cl(x), wt=wt, b=b, temb=temb, res=res, ref=ref, budget=(9 * cin + 4) * U * mag)


# ------------------------------------------------------------------ the launches ----------------------------------------------------
def by_region(case, flat_idx, ncols):
    """the 128 x 64 blocks that hold the elements ``flat_idx``, counted by the region of the schedule that owns them"""
    flat_idx = flat_idx.cpu()
    regions = {}
    for blk in torch.unique((flat_idx // ncols // 128) * 100000 + (flat_idx % ncols) // 64).tolist():
        rb, ct = divmod(blk, 100000)
        text = region(case, rb * 128, ct * 64)
        name = text.split("; regions ")[1].split(")")[0] if "; regions " in text else next(r for r in ("wide", "s1", "tail") if f", {r} region" in text)
        regions[name] = regions.get(name, 0) + 1
    return regions


def where(case, flat, ncols):
    row, col = divmod(int(flat), ncols)
    return f"element ({row}, {col}): {region(case, row, col)}"


def run_fenced_named(case, call, ins, out):
    """run_fenced; an element that was left unwritten (or read poison) is reported with the tile that owns it"""
    try:
        return run_fenced(call, ins, out)
    except AssertionError as e:
        if "NaN in the result" not in str(e):
            raise
        nan = torch.isnan(out.view).flatten().nonzero().flatten()
        raise AssertionError(f"{case['name']}: {str(e).splitlines()[0]}; in 128x64 blocks of: {by_region(case, nan, out.cols)}; first at "
                             f"{where(case, int(nan[0]), out.cols)}") from None


def run_linear(eng, case, p):
    """-> (result of the one big launch, its dispatch record, the same rows from launches of SLICE_ROWS rows)"""
    geglu = case["kind"] == "geglu"
    c1 = case.get("c1", 0)
    c0 = p["x"].shape[1] - c1
    m = p["x"].shape[0]
    fx = fenced(p["x"][:, :c0], ld=c0 + 4, name="x")
    f1 = fenced(p["x"][:, c0:], ld=c1 + 4, name="x1") if c1 else None
    fw = fenced(p["w"], name="w")
    fb = fenced(p["b"], name="bias") if p["b"] is not None else None
    fr = fenced(p["r"], name="resid") if p["r"] is not None else None
    out = fenced_out((m, p["ref"].shape[1]))
    call = lambda lo, hi, o: eng.op_linear(fx.t[lo:hi], fw.t, fb.t if fb else None, fr.t[lo:hi] if fr else None, geglu=geglu, out=o,
                                           x1=f1.t[lo:hi] if f1 else None)
    y = run_fenced_named(case, lambda: call(0, m, out.t), [fx, f1, fw, fb, fr], out)
    tag = eng.last_dispatch()
    parts = [call(lo, min(lo + SLICE_ROWS, m), None) for lo in range(0, m, SLICE_ROWS)]
    return y, tag, torch.cat(parts)


def run_conv(eng, case, p):
    """-> (result of the one big launch, its dispatch record, the same rows from one launch per image)"""
    n, hs, ws, up, stride = case["n"], case["h"], case["w"], case["up"], case["stride"]
    ho, wo = conv_out_hw(case)
    c1 = case["c1"]
    c0 = case["cin"] - c1
    fx = fenced(p["x"][:, :c0], name="x0")
    f1 = fenced(p["x"][:, c0:], name="x1") if c1 else None
    fw, fb = fenced(p["wt"], name="w"), fenced(p["b"], name="bias")
    ft = fenced(p["temb"], name="rowbias") if p["temb"] is not None else None
    fr = fenced(p["res"], name="resid") if p["res"] is not None else None
    out = fenced_out((n * ho * wo, case["cout"]))
    ri, ro = hs * ws, ho * wo

    def call(i0, i1, o):
        return eng.op_conv3x3(fx.t[i0 * ri:i1 * ri], fw.t, fb.t, f1.t[i0 * ri:i1 * ri] if f1 else None, n_img=i1 - i0, Hs=hs, Ws=ws,
                              Hi=hs * up, Wi=ws * up, stride=stride, rowbias=ft.t[i0:i1] if ft else None, rows_per_sample=ro,
                              resid=fr.t[i0 * ro:i1 * ro] if fr else None, out=o)
    eng.set_conv_algo(case["algo"])
    try:
        y = run_fenced_named(case, lambda: call(0, n, out.t), [fx, f1, fw, fb, ft, fr], out)
        tag = eng.last_dispatch()
        parts = [call(i, i + 1, None) for i in range(n)]
    finally:
        eng.set_conv_algo("auto")
    return y, tag, torch.cat(parts)


def run_case(eng, case):
    p = problem(case)
    y, tag, sliced = (run_conv if case["kind"] == "conv" else run_linear)(eng, case, p)
    return p, y, tag, sliced


def cases():
    for case in CASES:
        yield "schedule: " + case["name"], (lambda e, c=case: (run_case(e, c)[1], None))


# ------------------------------------------------------------------ the checks ------------------------------------------------------
def expected_record(case):
    s = schedule_of(case)
    if case["kind"] == "conv" and not wino_m(case):
        return " -> igemm_kernel 128x128x32"
    return f" rb1={s['rb1']} w{s['w1']} s{s['s1']} -> igemm_k16_kernel 128x128x16"


def accuracy(case, y, p, x3=False):
    """-> (passes, report): the worst element's error against its bound, with the tile that owns it"""
    err = (y.cpu().double() - p["ref"]).abs()
    ncols = err.shape[1]
    if x3:
        bound = X3_BOUND * p["ref"].abs().max().item()
        what = f"{X3_BOUND:g} of the output scale"
    elif "budget" in p and not wino_m(case):
        bound, what = p["budget"], "per-element budget (K + 4) 2^-24 sum |terms|"
    else:
        tol = BOUNDS[case["algo"]] if case["kind"] == "conv" else dict(rtol=RTOL, atol=ATOL)
        scale = p["ref"].abs().max().item()
        bound = tol["atol"] * max(1.0, scale) + tol["rtol"] * scale
        what = f"atol {tol['atol']:g} max(1, scale) + rtol {tol['rtol']:g} scale"
    ratio = err / bound
    worst = int(ratio.argmax())
    b = bound.flatten()[worst].item() if isinstance(bound, torch.Tensor) else bound
    ok = bool((err <= bound).all())
    return ok, f"worst error / bound {ratio.flatten()[worst].item():.3f} (|err| {err.flatten()[worst].item():.3e}, bound {b:.3e}: {what}) at " + \
        where(case, worst, ncols)


def bit_identity(case, y, sliced):
    """-> (identical, report): where the big launch and the narrow slices differ, by region"""
    diff = (y.view(torch.int32) != sliced.view(torch.int32))
    count = int(diff.sum())
    if not count:
        return True, f"bit-identical to the narrow slices in all {y.shape[0]} rows"
    idx = diff.flatten().nonzero().flatten().cpu()
    ncols = y.shape[1]
    delta = (y.double() - sliced.double()).abs().flatten().cpu()
    worst = int(delta.argmax())
    regions = by_region(case, idx, ncols)
    return False, (f"{count} of {y.numel()} elements differ from the narrow slices, in 128x64 blocks of: {regions}; first at "
                   f"{where(case, int(idx[0]), ncols)}; largest |difference| {delta[worst].item():.3e} at {where(case, worst, ncols)}")


def check(eng, case, x3=False):
    p, y, tag, sliced = run_case(eng, case)
    s = schedule_of(case)
    ok_acc, acc = accuracy(case, y, p, x3)
    ok_bits, bits = bit_identity(case, y, sliced)
    print(f"\n{case['name']}{' [f32x3]' if x3 else ''}: {kind_of(s)}, nbm {s['nbm']}, chunks {'/'.join(map(str, s['chunks']))}, tail_rb "
          f"{s['tail_rb']}; record '{tag}'\n  {acc}\n  {bits}")
    if not x3:
        assert tag.count("->") == 1 and expected_record(case) in tag, f"dispatch record '{tag}', restated '{expected_record(case)}'"
    assert ok_acc, acc
    assert ok_bits, bits


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_schedule_case(eng, case):
    check(eng, case)


@pytest.mark.parametrize("name", X3_ROWS)
def test_schedule_case_f32x3(eng_x3, name):
    """launch_igemm_x3 takes the same schedule with another kernel (it leaves no dispatch record: the profile names it)"""
    eng_x3.profile_begin()
    try:
        check(eng_x3, case_named(name), x3=True)
    finally:
        prof = eng_x3.profile_end()
    assert "igemm_f32x3" in prof, "the split-bf16 kernel did not run"
