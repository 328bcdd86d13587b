"""GPU: sampler plans on the device.  The update arithmetic of a traced plan (``e2v_op_run_plan``) against the scheduler mirror stepped
by hand, bit for bit; the plan loop of the pipeline (``e2v_generate_plan``) against the stepped loop and the oracle for every scheduler
the constructor accepts; mixed integral / fractional timesteps through the per-run cache, the generator's draw order, the bf16 mode,
steady-state allocation, the guarded pool and what a refused call leaves behind."""
import numpy as np
import pytest
import torch

from eeg2video_amd import scheduler as S
from eeg2video_amd.sampler_plan import LINCOMB, UNET, PlanOp, SamplerPlan, trace_plan
from eeg2video_amd.weights import (TINY_UNET, TINY_VAE, counter_normal, synth_state_dict, unet_param_spec,
                                   vae_param_spec)
from test_hip_bounds import GUARD_KIB, engines, fenced, fenced_out, guarded_run, pipes, run_fenced

pytestmark = pytest.mark.gpu

TOK, D = 77, TINY_UNET.cross_attention_dim


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


@pytest.fixture(scope="module")
def tiny():
    from eeg2video_amd.pipeline import build_pipeline
    usd = synth_state_dict(unet_param_spec(TINY_UNET), seed=42, mode="perturbed")
    vsd = synth_state_dict(vae_param_spec(TINY_VAE), seed=43, mode="perturbed")
    pipe = build_pipeline(TINY_UNET, TINY_VAE, device=0, unet_sd=usd, vae_sd=vsd)
    pipe.set_progress_bar_config(disable=True)
    return pipe, {k: _t(v) for k, v in usd.items()}, {k: _t(v) for k, v in vsd.items()}


def pairs():
    import oracle as O
    #        mirror, oracle, eta of the pipeline runs, frame bound against the oracle (tests/test_hip_schedulers.py)
    return {"pndm": (S.PNDMScheduler, O.PNDMOracle, 0.0, 1e-3),
            "euler": (S.EulerDiscreteScheduler, O.EulerOracle, 0.0, 1e-3),
            "euler_a": (S.EulerAncestralDiscreteScheduler, O.EulerAncestralOracle, 0.0, 1e-3),
            "lms": (S.LMSDiscreteScheduler, O.LMSOracle, 0.0, 2e-3),
            "dpmpp": (S.DPMSolverMultistepScheduler, O.DPMSolverPPOracle, 0.0, 1e-3),
            "ddim_eta": (S.DDIMScheduler, O.DDIMOracle, 0.6, 1e-3)}


STOCHASTIC = ("euler_a", "ddim_eta")


# ------------------------------------------------------------------ plan updates against the mirrors, bit for bit
def stepped_updates(eng, sm, x0, eu, ec, guidance, noise, name, eta):
    """the mirror stepped by hand as the pipeline's stepped loop does: scale_model_input, cfg_combine, step"""
    x = x0
    for i, t in enumerate(sm.timesteps):
        sm.scale_model_input(x, t)
        eps = eng.cfg_combine(eu[i], ec[i], guidance) if guidance > 1.0 else eu[i]
        kw = {"eta": eta, "variance_noise": noise[i]} if name == "ddim_eta" else {"noise": noise[i]} if name == "euler_a" else {}
        x = sm.step(eps, t, x, **kw).prev_sample
    return x


def update_inputs(name, n, shape, eng, eta=0.7):
    sm = pairs()[name][0](engine=eng)
    plan = trace_plan(sm, n, eta=eta)
    k = plan.n_unet
    x0 = (_t(counter_normal(41, "x", shape)) * float(sm.init_noise_sigma)).float().cuda()
    eu = _t(counter_normal(42, "eu", (k,) + shape)).cuda()
    ec = _t(counter_normal(43, "ec", (k,) + shape)).cuda()
    noise = _t(counter_normal(44, "z", (k,) + shape)).cuda() if plan.n_noise else None
    return sm, plan, x0, eu, ec, noise


UPDATE_CASES = [("pndm", 7), ("lms", 7), ("dpmpp", 20), ("dpmpp", 4), ("euler", 7), ("euler_a", 7), ("ddim_eta", 7)]


@pytest.mark.parametrize("guidance", [7.5, 1.0])
@pytest.mark.parametrize("shape", [(2, 4, 3, 5, 6), (1, 4, 3, 5, 7)])
@pytest.mark.parametrize("name,n", UPDATE_CASES)
def test_plan_updates_equal_the_mirror_bit_for_bit(tiny, name, n, shape, guidance):
    eng = tiny[0].unet.engine
    sm, plan, x0, eu, ec, noise = update_inputs(name, n, shape, eng)
    assert plan.n_noise == (plan.n_unet if name in STOCHASTIC else 0)
    got = eng.run_plan_updates(plan, x0, eu, ec if guidance > 1.0 else None, guidance, noise)
    want = stepped_updates(eng, sm, x0, eu, ec, guidance, noise, name, 0.7)
    assert got.shape == want.shape and torch.isfinite(got).all()
    assert torch.equal(got, want), (got - want).abs().max().item()


def test_pndm_plan_updates_fenced(tiny):
    """every operand and the result between poisoned fences: no word outside the tensors changes, the inputs keep their bits"""
    eng = tiny[0].unet.engine
    shape = (1, 4, 3, 5, 7)
    sm, plan, x0, eu, ec, _ = update_inputs("pndm", 7, shape, eng)
    fx, fu, fc, out = fenced(x0, name="x0"), fenced(eu, name="eps_u"), fenced(ec, name="eps_c"), fenced_out(shape)
    y = run_fenced(lambda: eng.run_plan_updates(plan, fx.t, fu.t, fc.t, 7.5, out=out.t), [fx, fu, fc], out)
    want = stepped_updates(eng, sm, x0, eu, ec, 7.5, None, "pndm", 0.0)
    assert torch.equal(y.reshape(shape), want)


# ------------------------------------------------------------------ the plan loop against the stepped loop and the oracle
_ref = {}


def inputs(b, seed=70):
    shape = (b, 4, 3, 4, 6)
    return (shape, _t(counter_normal(seed, "lat", shape)), _t(counter_normal(seed + 1, "eeg", (b, TOK * D))),
            _t(counter_normal(seed + 2, "neg", (1, TOK, D))))


def run_pipe(pipe, mirror, eeg, lat, neg, n, guidance, eta, seed=None, stepped=False):
    """one pipeline call with `mirror` swapped in; the stepped loop is forced with a callback that keeps the latest latents"""
    kept = []
    old = pipe.scheduler
    try:
        pipe.scheduler = mirror
        out = pipe(None, eeg, video_length=3, height=32, width=48, num_inference_steps=n, guidance_scale=guidance,
                   negative_prompt=neg, latents=lat.cuda(), eta=eta,
                   generator=torch.Generator().manual_seed(seed) if seed is not None else None,
                   callback=(lambda i, t, x: kept.append(x)) if stepped else None).videos
    finally:
        pipe.scheduler = old
    assert pipe.last_loop == ("stepped" if stepped else "plan")
    return out, (kept[-1] if kept else None)


@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("name", ["pndm", "euler", "euler_a", "lms", "dpmpp", "ddim_eta"])
def test_plan_loop_vs_stepped_loop_and_oracle(tiny, name, b):
    from oracle import generate
    pipe, usd, vsd = tiny
    eng = pipe.unet.engine
    mirror_cls, oracle_cls, eta, bound = pairs()[name]
    n, g = 4, 7.5
    shape, lat, eeg, neg = inputs(b)
    seed = 11 if name in STOCHASTIC else None
    noises = None
    if seed is not None:
        g2 = torch.Generator().manual_seed(seed)
        noises = [torch.randn(shape, generator=g2) for _ in range(n)]
    if (name, b) not in _ref:
        _ref[name, b] = generate(usd, TINY_UNET, vsd, TINY_VAE, lat, eeg.reshape(b, TOK, D), neg, n, g, eta=eta,
                                 scheduler=oracle_cls(), noises=noises)
    ref = _ref[name, b]
    out, _ = run_pipe(pipe, mirror_cls(engine=eng), eeg, lat, neg, n, g, eta, seed)
    stepped, lat_stepped = run_pipe(pipe, mirror_cls(engine=eng), eeg, lat, neg, n, g, eta, seed, stepped=True)
    assert out.shape == ref.shape and torch.isfinite(out).all()
    e_ref, e_step = (out - ref).abs().max().item(), (out - stepped).abs().max().item()
    # the engine call the pipeline made, for the latents
    sm = mirror_cls(engine=eng)
    plan = trace_plan(sm, n, eta=eta)
    x0 = lat.cuda() * sm.init_noise_sigma                   # (prepare_latents' own expression)
    vid, lat_plan = eng.generate_plan(x0, eeg.reshape(b, TOK, D).cuda(), neg.cuda(), plan, g,
                                      noise=torch.stack(noises) if noises else None, return_latents=True)
    e_lat = rel_err(lat_plan, lat_stepped)
    print(f"{name} B={b}: frames vs oracle {e_ref:.3e} (bound {bound:.0e}), vs stepped loop {e_step:.3e} (bound 1e-5, "
          f"bit-equal: {torch.equal(out, stepped)}), latents vs stepped / scale {e_lat:.3e} (bound 2e-5, "
          f"bit-equal: {torch.equal(lat_plan, lat_stepped)})")
    assert torch.equal(vid.cpu(), out)
    assert e_ref < bound, e_ref
    assert e_step < 1e-5, e_step
    assert e_lat < 2e-5, e_lat


def test_mixed_integral_and_fractional_timesteps(tiny):
    """Euler, n = 7: 999, 832.5, 666, 499.5, 333, 166.5, 0 -- the per-run cache serves the integral ones from the int64 sinusoid path
    and the fractional ones from the fp32 path, as the stepped loop's uncached calls do"""
    pipe = tiny[0]
    eng = pipe.unet.engine
    _, lat, eeg, neg = inputs(1, seed=80)
    plan = trace_plan(S.EulerDiscreteScheduler(engine=eng), 7)
    kinds = [op.fractional for op in plan.ops if op.kind == UNET]
    assert True in kinds and False in kinds
    out, _ = run_pipe(pipe, S.EulerDiscreteScheduler(engine=eng), eeg, lat, neg, 7, 7.5, 0.0)
    stepped, _ = run_pipe(pipe, S.EulerDiscreteScheduler(engine=eng), eeg, lat, neg, 7, 7.5, 0.0, stepped=True)
    e = (out - stepped).abs().max().item()
    print(f"euler n=7: frames vs stepped loop {e:.3e}, bit-equal: {torch.equal(out, stepped)}")
    assert torch.isfinite(out).all() and e < 1e-5, e


def test_pndm_without_guidance(tiny):
    from oracle import PNDMOracle, generate
    pipe, usd, vsd = tiny
    eng = pipe.unet.engine
    _, lat, eeg, _ = inputs(1, seed=90)
    ref = generate(usd, TINY_UNET, vsd, TINY_VAE, lat, eeg.reshape(1, TOK, D), None, 4, 1.0, scheduler=PNDMOracle())
    out, _ = run_pipe(pipe, S.PNDMScheduler(engine=eng), eeg, lat, None, 4, 1.0, 0.0)
    stepped, _ = run_pipe(pipe, S.PNDMScheduler(engine=eng), eeg, lat, None, 4, 1.0, 0.0, stepped=True)
    assert (out - ref).abs().max().item() < 1e-3
    assert (out - stepped).abs().max().item() < 1e-5


@pytest.mark.parametrize("name", STOCHASTIC)
def test_generator_draw_order(tiny, name):
    """the plan loop draws its noise from the caller's generator in step order -- the stepped loop's draws; reversed, it differs"""
    pipe = tiny[0]
    eng = pipe.unet.engine
    mirror_cls, _, eta, _ = pairs()[name]
    shape, lat, eeg, neg = inputs(1, seed=100)
    n = 4
    out, _ = run_pipe(pipe, mirror_cls(engine=eng), eeg, lat, neg, n, 7.5, eta, seed=11)
    stepped, _ = run_pipe(pipe, mirror_cls(engine=eng), eeg, lat, neg, n, 7.5, eta, seed=11, stepped=True)
    assert (out - stepped).abs().max().item() < 1e-5
    g = torch.Generator().manual_seed(11)
    draws = [torch.randn(shape, generator=g) for _ in range(n)]
    sm = mirror_cls(engine=eng)
    plan = trace_plan(sm, n, eta=eta)
    x0 = lat.cuda() * sm.init_noise_sigma                   # (prepare_latents' own expression)
    cond = eeg.reshape(1, TOK, D).cuda()
    same = eng.generate_plan(x0, cond, neg.cuda(), plan, 7.5, noise=torch.stack(draws)).cpu()
    assert torch.equal(same, out)
    rev = eng.generate_plan(x0, cond, neg.cuda(), plan, 7.5, noise=torch.stack(draws[::-1])).cpu()
    assert not (rev - stepped).abs().max().item() < 1e-5


def test_bf16_context(tiny):
    """the PNDM plan loop in the bf16 mode: finite frames, latents within 5e-2 of the fp32 run's scale (tests/test_hip_model.py)"""
    pipe = tiny[0]
    eng = pipe.unet.engine
    _, lat, eeg, neg = inputs(1, seed=110)
    plan = trace_plan(S.PNDMScheduler(engine=eng), 4)
    args = (lat.cuda(), eeg.reshape(1, TOK, D).cuda(), neg.cuda(), plan, 7.5)
    _, lat32 = eng.generate_plan(*args, return_latents=True)
    try:
        eng.set_compute_dtype("bf16")
        vid16, lat16 = eng.generate_plan(*args, return_latents=True)
    finally:
        eng.set_compute_dtype("fp32")
    e = rel_err(lat16, lat32)
    print(f"PNDM plan loop, bf16 vs fp32 latents / scale: {e:.3e}")
    assert torch.isfinite(vid16).all() and torch.isfinite(lat16).all()
    assert 0 < e < 5e-2, e


def test_no_steady_state_allocation(tiny):
    pipe = tiny[0]
    eng = pipe.unet.engine
    _, lat, eeg, neg = inputs(2, seed=120)
    cond = eeg.reshape(2, TOK, D).cuda()
    for name in ("pndm", "euler_a"):
        sm = pairs()[name][0](engine=eng)
        plan = trace_plan(sm, 4)
        noise = torch.randn((plan.n_noise, 2, 4, 3, 4, 6), generator=torch.Generator().manual_seed(3)).cuda() if plan.n_noise else None
        sizes = []
        for _ in range(3):
            eng.generate_plan(lat.cuda(), cond, neg.cuda(), plan, 7.5, noise=noise)
            torch.cuda.synchronize()
            sizes.append(eng.device_bytes())
        assert sizes[1] == sizes[2], (name, sizes)


def test_pndm_plan_loop_guarded():
    """E2V_POOL_GUARD: the slots, the noise-free PNDM loop and the per-run caches between guard zones -- the same bits, no zone altered"""
    pp = pipes()
    _, lat, eeg, neg = inputs(1, seed=130)
    gl, gc, gu = lat.cuda(), eeg.reshape(1, TOK, D).cuda(), neg.cuda()
    plan = trace_plan(S.PNDMScheduler(), 4)
    assert GUARD_KIB == 64
    vid, lat_out = guarded_run(engines(pp), lambda e: e.generate_plan(gl, gc, gu, plan, 7.5, return_latents=True), what="PNDM plan loop")
    assert torch.isfinite(vid).all() and torch.isfinite(lat_out).all()


def test_euler_ancestral_plan_loop_guarded():
    """the same with a noise array and mixed timestep kinds (n = 3: 999, 499.5, 0)"""
    pp = pipes()
    _, lat, eeg, neg = inputs(1, seed=140)
    gl, gc, gu = lat.cuda(), eeg.reshape(1, TOK, D).cuda(), neg.cuda()
    plan = trace_plan(S.EulerAncestralDiscreteScheduler(), 3)
    noise = _t(counter_normal(141, "z", (3,) + tuple(lat.shape))).cuda()
    guarded_run(engines(pp), lambda e: e.generate_plan(gl * 14.6, gc, gu, plan, 7.5, noise=noise, return_latents=True),
                what="Euler-ancestral plan loop")


# ------------------------------------------------------------------ refused calls
def test_refused_calls_raise_and_write_nothing(tiny):
    pipe = tiny[0]
    eng = pipe.unet.engine
    shape = (1, 4, 3, 4, 6)
    good = trace_plan(S.EulerAncestralDiscreteScheduler(engine=eng), 3)
    x0 = _t(counter_normal(150, "x", shape)).cuda()
    eu = _t(counter_normal(151, "e", (3,) + shape)).cuda()
    noise = _t(counter_normal(152, "z", (3,) + shape)).cuda()
    sentinel = 12345.0
    out = torch.full(shape, sentinel, device="cuda")
    bad = SamplerPlan([PlanOp(UNET, 1, (0,), (), 500.0), PlanOp(LINCOMB, 2, (0, 5), (1.0, 1.0))], 3, 2, 0)
    with pytest.raises(ValueError, match="plan op 1"):
        eng.run_plan_updates(bad, x0, eu[:1], out=out)
    with pytest.raises(ValueError, match="noise"):
        eng.run_plan_updates(good, x0, eu, noise=noise[:2], out=out)
    with pytest.raises(ValueError, match="noise"):
        eng.run_plan_updates(good, x0, eu, noise=noise[:, :, :2], out=out)
    with pytest.raises(ValueError, match="noise"):
        eng.run_plan_updates(good, x0, eu, out=out)
    with pytest.raises(ValueError, match="eps_u"):
        eng.run_plan_updates(good, x0, eu[:2], noise=noise, out=out)
    torch.cuda.synchronize()
    assert (out == sentinel).all()
    _, lat, eeg, neg = inputs(1, seed=160)
    cond = eeg.reshape(1, TOK, D).cuda()
    with pytest.raises(ValueError, match="plan op 1"):
        eng.generate_plan(lat.cuda(), cond, neg.cuda(), bad, 7.5)
    with pytest.raises(ValueError, match="noise"):
        eng.generate_plan(lat.cuda(), cond, neg.cuda(), good, 7.5, noise=noise[:2])
    with pytest.raises(ValueError, match="uncond"):
        eng.generate_plan(lat.cuda(), cond, None, good, 7.5, noise=noise)
    # the engine still works, and a generator list keeps the stepped loop
    ok = eng.run_plan_updates(good, x0, eu, noise=noise, out=out)
    assert ok is out and torch.isfinite(out).all() and not (out == sentinel).any()
    old = pipe.scheduler
    try:
        pipe.scheduler = S.EulerDiscreteScheduler(engine=eng)
        pipe(None, eeg, video_length=3, height=32, width=48, num_inference_steps=2, guidance_scale=7.5, negative_prompt=neg,
             latents=lat.cuda(), generator=[torch.Generator().manual_seed(1)])
        assert pipe.last_loop == "stepped"
    finally:
        pipe.scheduler = old
    pipe(None, eeg, video_length=3, height=32, width=48, num_inference_steps=2, guidance_scale=7.5, negative_prompt=neg,
         latents=lat.cuda())
    assert pipe.last_loop == "ddim"


def test_stock_sd_directory_takes_the_plan_loop(tiny, tmp_path):
    """inference_eeg2video.py:70,92-98 against a directory whose model_index.json names PNDMScheduler, as the stock SD-v1-4 one does"""
    import os
    from eeg2video_amd.pipeline import TuneAVideoPipeline
    from eeg2video_amd.unet import UNet3DConditionModel
    from eeg2video_amd.vae import AutoencoderKL
    from test_hip_model import _save_sd_dir
    _, usd, vsd = tiny
    scfg = {"_class_name": "PNDMScheduler", "_diffusers_version": "0.11.1", "beta_start": 0.00085, "beta_end": 0.012,
            "beta_schedule": "scaled_linear", "num_train_timesteps": 1000, "set_alpha_to_one": False, "trained_betas": None,
            "steps_offset": 0, "skip_prk_steps": True}
    root = str(tmp_path / "sd")
    _save_sd_dir(root, usd, vsd, scfg)
    unet = UNet3DConditionModel.from_pretrained(root, subfolder="unet", torch_dtype=torch.float16,
                                                vae_config=AutoencoderKL.config_from_dir(os.path.join(root, "vae"))).to("cuda")
    pipe = TuneAVideoPipeline.from_pretrained(root, unet=unet, torch_dtype=torch.float16).to("cuda")
    pipe.set_progress_bar_config(disable=True)
    assert pipe.last_loop is None
    _, lat, eeg, neg = inputs(1)
    pipe.negative_embeddings = neg
    video = pipe(None, eeg[0:1], video_length=3, height=32, width=48, num_inference_steps=5, guidance_scale=12.5,
                 latents=lat.cuda()).videos
    assert pipe.last_loop == "plan" and tuple(video.shape) == (1, 3, 3, 32, 48) and torch.isfinite(video).all()
