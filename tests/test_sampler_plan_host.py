"""CPU: sampler plans.  ``trace_plan`` records the updates of every scheduler mirror from the mirror's own ``step`` /
``scale_model_input``; the recorded plan, interpreted in numpy float32, reproduces the oracle's step sequence; its structure fits the
device loop (UNet evaluations, work slots, noise order); the library validates plans on a host-only context before anything else.
No GPU work."""
import ctypes as C

import numpy as np
import pytest
import torch

from eeg2video_amd import _lib, scheduler as S
from eeg2video_amd.sampler_plan import LINCOMB, MAX_SLOTS, UNET, PlanOp, SamplerPlan, trace_plan
from eeg2video_amd.weights import counter_normal

SHAPE = (2, 4, 3, 5, 6)
STEPS = [1, 2, 3, 4, 7, 20]


def cases():
    import oracle as O
    #        mirror, oracle, eta, bound (tests/test_hip_schedulers.py: 3e-6; LMS 3e-4 -- the mirror integrates numerically, the oracle exactly)
    return {"pndm": (S.PNDMScheduler, O.PNDMOracle, 0.0, 3e-6),
            "euler": (S.EulerDiscreteScheduler, O.EulerOracle, 0.0, 3e-6),
            "euler_a": (S.EulerAncestralDiscreteScheduler, O.EulerAncestralOracle, 0.0, 3e-6),
            "lms": (S.LMSDiscreteScheduler, O.LMSOracle, 0.0, 3e-4),
            "dpmpp": (S.DPMSolverMultistepScheduler, O.DPMSolverPPOracle, 0.0, 3e-6),
            "ddim_eta": (S.DDIMScheduler, O.DDIMOracle, 0.7, 3e-6)}


NAMES = ["pndm", "euler", "euler_a", "lms", "dpmpp", "ddim_eta"]
_plans = {}


def plan_of(name, n):
    if (name, n) not in _plans:
        mirror_cls, _, eta, _ = cases()[name]
        _plans[name, n] = trace_plan(mirror_cls(), n, eta=eta)
    return _plans[name, n]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def host_ctx(lib):
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    ctx = C.c_void_p()
    assert lib.e2v_create(C.byref(cfg), -1, C.byref(ctx)) == 0
    yield ctx
    lib.e2v_destroy(ctx)


# ------------------------------------------------------------------ traced plans against the oracles
@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("name", NAMES)
def test_traced_plan_vs_oracle(name, n):
    """the oracle's loop on fixed eps / noise sequences against the plan interpreted in float32 with the same sequences"""
    _, oracle_cls, eta, bound = cases()[name]
    plan = plan_of(name, n)
    so = oracle_cls()
    ts = so.set_timesteps(n)
    x0 = counter_normal(41, "x", SHAPE).astype(np.float32) * np.float32(float(so.init_noise_sigma))
    eps = [counter_normal(42 + i, "e", SHAPE).astype(np.float32) for i in range(len(ts))]
    noise = [counter_normal(900 + i, "z", SHAPE).astype(np.float32) for i in range(len(ts))]
    x = _t(x0)
    for i, t in enumerate(ts):
        t = int(t) if float(t).is_integer() else float(t)
        so.scale_model_input(x, t)
        x = so.step(_t(eps[i]), t, x, eta=eta, noise=_t(noise[i]))
    assert plan.n_unet == len(ts)
    assert [float(t) for t in ts] == plan.timesteps
    got = plan.run_numpy(x0, eps, noise)
    assert got.dtype == np.float32
    ref = x.double().numpy()
    err = np.abs(got.astype(np.float64) - ref).max() / (np.abs(ref).max() + 1e-30)
    print(f"{name} n={n}: max abs / output scale {err:.3e} (bound {bound:.0e})")
    assert err < bound, err


def test_scale_model_input_feeds_the_unet():
    """sigma-space plans: the UNet reads x / sqrt(sigma^2 + 1), the update reads x"""
    plan = plan_of("euler", 3)
    sm = S.EulerDiscreteScheduler()
    sm.set_timesteps(3)
    seen = []
    plan.run_numpy(np.ones(4, np.float32), lambda x, t, k: seen.append((float(x[0]), t)) or np.zeros(4, np.float32))
    assert [t for _, t in seen] == [float(t) for t in sm.timesteps]
    for (v, _), sigma in zip(seen, sm.sigmas[:-1]):          # eps = 0: the Euler update leaves x = 1
        assert abs(v - 1.0 / (float(sigma) ** 2 + 1) ** 0.5) < 1e-6


# ------------------------------------------------------------------ structure
@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("name", NAMES)
def test_plan_structure(name, n, lib, host_ctx):
    mirror_cls, _, eta, _ = cases()[name]
    plan = plan_of(name, n)
    sm = mirror_cls()
    sm.set_timesteps(n)
    assert plan.n_unet == len(sm.timesteps) == (n + 1 if name == "pndm" and n >= 2 else n)
    assert 1 <= plan.n_slots <= MAX_SLOTS and 0 <= plan.final_slot < plan.n_slots
    assert plan.n_noise == (len(sm.timesteps) if name in ("euler_a", "ddim_eta") else 0)
    reads = [-1 - s for op in plan.ops for s in op.src if s < 0]
    assert reads == list(range(plan.n_noise))                # each noise tensor once, in step order
    written = {0}
    per_eval = 0
    for op in plan.ops:
        assert op.dst not in op.src                          # no op writes a slot it reads
        assert all(s in written for s in op.src if s >= 0)
        assert (len(op.src) == 1 and not op.coef) if op.kind == UNET else 1 <= len(op.src) == len(op.coef) <= 5
        written.add(op.dst)
        per_eval = 0 if op.kind == UNET else per_eval + 1
        assert per_eval <= 2                                 # at most two recorded lincombs per evaluation
    for op in plan.ops:                                      # a timestep is fractional only when it differs from its rounding
        if op.kind == UNET:
            assert op.fractional == (op.timestep != round(op.timestep))
    # the library's own validation, then the host-only answer
    ops = plan.c_ops()
    st = lib.e2v_generate_plan(host_ctx, None, None, None, 0, 1, 3, 4, 6, 77, ops, len(ops), plan.n_slots, plan.final_slot,
                               None if plan.n_noise == 0 else 1, plan.n_noise, 7.5, None, None, None)
    assert st == _lib.E2V_ESTATE, lib.e2v_last_error(host_ctx)
    assert b"host-only" in lib.e2v_last_error(host_ctx)
    st = lib.e2v_op_run_plan(host_ctx, ops, len(ops), plan.n_slots, plan.final_slot, None, None, None, plan.n_unet,
                             None if plan.n_noise == 0 else 1, plan.n_noise, 7.5, None, 10, None)
    assert st == _lib.E2V_ESTATE, lib.e2v_last_error(host_ctx)


def test_mixed_timestep_kinds_are_traced():
    """linspace(0, 999, 7)[::-1]: 999, 832.5, 666, 499.5, 333, 166.5, 0"""
    plan = plan_of("euler", 7)
    assert plan.timesteps == [999.0, 832.5, 666.0, 499.5, 333.0, 166.5, 0.0]
    assert [op.fractional for op in plan.ops if op.kind == UNET] == [False, True, False, True, False, True, False]


def test_peak_slots_and_pndm_reuse():
    assert max(plan_of(name, 20).n_slots for name in NAMES) <= 6      # PNDM and LMS: the sample, four model outputs and the new one
    assert plan_of("euler", 20).n_slots <= 4


def test_deterministic_ddim_and_foreign_schedulers_are_not_traced():
    with pytest.raises(ValueError, match="eta = 0"):
        trace_plan(S.DDIMScheduler(), 4, eta=0.0)

    class Other(S.PNDMScheduler):
        pass
    with pytest.raises(TypeError):
        trace_plan(Other(), 4)


# ------------------------------------------------------------------ the scheduler afterwards
class _Engine:
    """records the lincomb calls of a mirror stepped by hand (tensors: small numpy arrays)"""

    def __init__(self):
        self.calls = []

    def lincomb(self, terms):
        self.calls.append([float(c) for c, _ in terms])
        return sum(float(c) * t for c, t in terms)


@pytest.mark.parametrize("name", NAMES)
def test_scheduler_state_after_tracing(name):
    """a traced scheduler steps exactly as a fresh one: same timesteps, same coefficients, same results"""
    mirror_cls, _, eta, _ = cases()[name]
    n = 7

    def run(sm):
        eng = _Engine()
        sm.engine = eng
        x = np.full(3, 0.5)
        for i, t in enumerate(sm.timesteps):
            sm.scale_model_input(x, t)
            kw = {"eta": eta, "variance_noise": np.full(3, 0.1 * i)} if name == "ddim_eta" else \
                 {"noise": np.full(3, 0.1 * i)} if name == "euler_a" else {}
            x = sm.step(np.full(3, 0.25 + 0.01 * i), t, x, **kw).prev_sample
        return eng.calls, x

    fresh = mirror_cls()
    fresh.set_timesteps(n)
    traced = mirror_cls()
    marker = object()
    traced.engine = marker
    trace_plan(traced, n, eta=eta)
    assert traced.engine is marker and traced.num_inference_steps == n
    assert torch.equal(traced.timesteps, fresh.timesteps)
    calls_t, x_t = run(traced)
    calls_f, x_f = run(fresh)
    assert calls_t == calls_f and np.array_equal(x_t, x_f)
    # and the recorded coefficients are the stepped ones, in order
    plan = plan_of(name, n)
    assert [list(op.coef) for op in plan.ops if op.kind == LINCOMB] == calls_f


# ------------------------------------------------------------------ validation failures
def _good():
    return [PlanOp(UNET, 1, (0,), (), 500.0, False), PlanOp(LINCOMB, 2, (0, 1), (1.0, -0.5))]


def _call(lib, ctx, ops, n_slots=3, final_slot=2, n_noise=0):
    plan = SamplerPlan(list(ops), n_slots, final_slot, n_noise)
    arr = plan.c_ops()
    st = lib.e2v_generate_plan(ctx, None, None, None, 0, 1, 3, 4, 6, 77, arr, len(arr), n_slots, final_slot,
                               1 if n_noise else None, n_noise, 7.5, None, None, None)
    msg = lib.e2v_last_error(ctx).decode()
    st2 = lib.e2v_op_run_plan(ctx, arr, len(arr), n_slots, final_slot, None, None, None, plan.n_unet, 1 if n_noise else None, n_noise,
                              7.5, None, 10, None)
    assert st2 == st and lib.e2v_last_error(ctx).decode() == msg
    return st, msg


BAD = {   # name -> (ops, keyword overrides, op index the message names or None for a plan-level message)
    "source slot out of range": ([_good()[0], PlanOp(LINCOMB, 2, (0, 3), (1.0, 1.0))], {}, 1),
    "destination slot out of range": ([PlanOp(UNET, 3, (0,), (), 500.0)], {}, 0),
    "negative destination": ([PlanOp(UNET, -1, (0,), (), 500.0)], {}, 0),
    "noise index out of range": ([_good()[0], PlanOp(LINCOMB, 2, (0, 1, -3), (1.0, 1.0, 1.0))], {"n_noise": 2}, 1),
    "noise without a noise array": ([_good()[0], PlanOp(LINCOMB, 2, (0, -1), (1.0, 1.0))], {"n_noise": 0}, 1),
    "a UNET op reading noise": ([PlanOp(UNET, 1, (-1,), (), 500.0), _good()[1]], {"n_noise": 1}, 0),
    "no terms": ([_good()[0], PlanOp(LINCOMB, 2, (), ())], {}, 1),
    "a UNET op with two sources": ([PlanOp(UNET, 1, (0, 0), (), 500.0), _good()[1]], {}, 0),
    "slot read before it is written": ([_good()[0], PlanOp(LINCOMB, 1, (0, 2), (1.0, 1.0)), _good()[1]], {}, 1),
    "an op writing a slot it reads": ([_good()[0], PlanOp(LINCOMB, 1, (0, 1), (1.0, 1.0))], {"final_slot": 1}, 1),
    "final slot never written": (_good(), {"n_slots": 4, "final_slot": 3}, None),
    "final slot out of range": (_good(), {"final_slot": 3}, None),
    "too many slots": (_good(), {"n_slots": 9}, None),
    "no slots": (_good(), {"n_slots": 0}, None),
    "nan coefficient": ([_good()[0], PlanOp(LINCOMB, 2, (0, 1), (1.0, float("nan")))], {}, 1),
    "inf coefficient": ([_good()[0], PlanOp(LINCOMB, 2, (0, 1), (float("inf"), 1.0))], {}, 1),
    "coefficient beyond float": ([_good()[0], PlanOp(LINCOMB, 2, (0, 1), (1e300, 1.0))], {}, 1),
    "nan timestep": ([PlanOp(UNET, 1, (0,), (), float("nan"), True), _good()[1]], {}, 0),
    "integral timestep too large": ([PlanOp(UNET, 1, (0,), (), 1000.0), _good()[1]], {}, 0),
    "integral timestep negative": ([PlanOp(UNET, 1, (0,), (), -1.0), _good()[1]], {}, 0),
    "integral timestep with a fraction": ([PlanOp(UNET, 1, (0,), (), 500.5, False), _good()[1]], {}, 0),
    "no UNET op": ([PlanOp(LINCOMB, 1, (0,), (2.0,)), PlanOp(LINCOMB, 2, (0, 1), (1.0, 1.0))], {}, None),
    "unknown kind": ([_good()[0], PlanOp(7, 2, (0,), (1.0,))], {}, 1),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_malformed_plan_is_einval(what, lib, host_ctx):
    ops, kw, index = BAD[what]
    st, msg = _call(lib, host_ctx, ops, **kw)
    assert st == _lib.E2V_EINVAL, (what, st, msg)
    assert (f"plan op {index}:" in msg) if index is not None else msg.startswith("plan:"), msg


def test_six_terms_is_einval(lib, host_ctx):
    """(a term count above the array: written into the struct by hand)"""
    arr = SamplerPlan(_good(), 3, 2, 0).c_ops()
    arr[1].n_src = 6
    st = lib.e2v_generate_plan(host_ctx, None, None, None, 0, 1, 3, 4, 6, 77, arr, 2, 3, 2, None, 0, 7.5, None, None, None)
    assert st == _lib.E2V_EINVAL and b"plan op 1:" in lib.e2v_last_error(host_ctx)


def test_well_formed_plan_passes_validation(lib, host_ctx):
    st, msg = _call(lib, host_ctx, _good())
    assert st == _lib.E2V_ESTATE and "host-only" in msg
    # a fractional timestep may lie anywhere; a wrong eps count is the test entry's own check
    st, msg = _call(lib, host_ctx, [PlanOp(UNET, 1, (0,), (), 832.5, True), _good()[1]])
    assert st == _lib.E2V_ESTATE
    arr = SamplerPlan(_good(), 3, 2, 0).c_ops()
    assert lib.e2v_op_run_plan(host_ctx, arr, 2, 3, 2, None, None, None, 2, None, 0, 7.5, None, 10, None) == _lib.E2V_EINVAL


def test_plan_op_layout(lib):
    assert lib.e2v_plan_op_size() == C.sizeof(_lib.E2VPlanOp) == 88
