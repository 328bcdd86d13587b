"""GPU: the model-level C ABI (UNet forward, DDIM/CFG step, VAE, the fused generate loop) and the Python
mirrors of the reference interfaces, against the CPU oracle and the reference-generated goldens.

Tolerance: BASELINE.json asks for <= 1e-3 relative fp32 on the end-to-end frames; single modules are held to
1e-4 of the tensor's scale (fp32 both sides; only the summation order differs)."""
import os

import numpy as np
import pytest
import torch

from eeg2video_amd.weights import (TINY_UNET, TINY_VAE, counter_normal, synth_state_dict, unet_param_spec,
                                   vae_param_spec)

pytestmark = pytest.mark.gpu


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


@pytest.fixture(scope="module")
def tiny():
    """One engine with tiny UNet + VAE ('perturbed' weights: no neutral gamma/beta, non-zero temporal to_out)."""
    from eeg2video_amd.pipeline import build_pipeline
    usd = synth_state_dict(unet_param_spec(TINY_UNET), seed=42, mode="perturbed")
    vsd = synth_state_dict(vae_param_spec(TINY_VAE), seed=43, mode="perturbed")
    pipe = build_pipeline(TINY_UNET, TINY_VAE, device=0, unet_sd=usd, vae_sd=vsd)
    pipe.set_progress_bar_config(disable=True)
    return pipe, {k: _t(v) for k, v in usd.items()}, {k: _t(v) for k, v in vsd.items()}


def test_key_scheme_matches_library(tiny):
    pipe = tiny[0]
    exp = pipe.unet.engine.expected_keys()
    spec = dict(unet_param_spec(TINY_UNET))
    spec.update({"vae." + k: v for k, v in vae_param_spec(TINY_VAE).items()})
    from eeg2video_amd.weights import SemanticConfig, semantic_param_spec
    spec.update({"semantic." + k: v for k, v in semantic_param_spec(SemanticConfig(), TINY_UNET.cross_attention_dim).items()})
    assert exp == spec


def test_unet_forward_vs_reference_golden(tiny, golden_dir):
    """The reference's own UNet3DConditionModel.forward output (tests/golden/make_golden.py, tier 2)."""
    pipe = tiny[0]
    g = np.load(os.path.join(golden_dir, "reference_t2_unet_tiny.npz"))
    x, cond = _t(g["t2.unet.x"]), _t(g["t2.unet.cond"])
    y = pipe.unet(x.cuda(), 501, encoder_hidden_states=cond.cuda()).sample
    assert rel_err(y, _t(g["t2.unet.out_t501"])) < 1e-4
    y2 = pipe.unet(x.cuda(), torch.tensor([751, 1]), encoder_hidden_states=cond.cuda())["sample"]
    assert rel_err(y2, _t(g["t2.unet.out_t751_1"])) < 1e-4


@pytest.mark.parametrize("shape,tokens", [((2, 4, 3, 9, 12), 11), ((1, 4, 6, 8, 8), 77), ((3, 4, 2, 5, 7), 5)])
def test_unet_forward_vs_oracle(tiny, shape, tokens):
    from oracle import unet3d_forward
    pipe, usd, _ = tiny
    x = _t(counter_normal(5, "x", shape))
    cond = _t(counter_normal(6, "c", (shape[0], tokens, TINY_UNET.cross_attention_dim)))
    ref = unet3d_forward(usd, TINY_UNET, x, 301, cond)
    y = pipe.unet(x.cuda(), 301, cond.cuda(), return_dict=False)[0]
    assert y.shape == ref.shape and rel_err(y, ref) < 1e-4


def test_unet_batch_entries_are_independent(tiny):
    """No op of the UNet mixes samples (the property the multi-GPU sharding rests on)."""
    pipe = tiny[0]
    x = _t(counter_normal(7, "x", (3, 4, 3, 9, 12))).cuda()
    cond = _t(counter_normal(8, "c", (3, 11, TINY_UNET.cross_attention_dim))).cuda()
    full = pipe.unet(x, 41, cond).sample
    for i in range(3):
        one = pipe.unet(x[i:i + 1], 41, cond[i:i + 1]).sample
        assert torch.equal(one, full[i:i + 1])          # bit-exact: same kernels, same summation order


def test_ddim_cfg_step_vs_oracle(tiny):
    from oracle import DDIMOracle
    pipe = tiny[0]
    eng = pipe.unet.engine
    s = DDIMOracle()
    s.set_timesteps(50)
    x, eu, ec = (_t(counter_normal(9, k, (2, 4, 3, 9, 12))) for k in ("x", "eu", "ec"))
    for t in (981, 501, 1):
        eps = eu + 12.5 * (ec - eu)
        ref = s.step(eps, t, x)
        y = eng.ddim_cfg_step(eu.cuda(), ec.cuda(), x.cuda(), 12.5, t, t - 20)
        assert rel_err(y, ref) < 2e-6
        y1 = eng.ddim_cfg_step(eps.cuda(), None, x.cuda(), 1.0, t, t - 20)
        assert rel_err(y1, ref) < 2e-6


def test_ddim_schedule_bit_exact(tiny):
    from oracle import DDIMOracle
    eng = tiny[0].unet.engine
    for n in (1, 4, 7, 50, 100, 250, 1000):
        assert np.array_equal(eng.ddim_timesteps(n), DDIMOracle().set_timesteps(n))
    assert np.array_equal(eng.alphas_cumprod(), tiny[0].scheduler.alphas_cumprod.numpy())      # handed over by bind()


@pytest.mark.parametrize("n,h,w", [(2, 4, 6), (3, 6, 4), (2, 11, 12)])      # (h w = 132: the attention of the mid block on more than one tile)
def test_vae_decode_vs_oracle(tiny, n, h, w):
    from oracle import vae_decode
    pipe, _, vsd = tiny
    z = _t(counter_normal(10, "z", (n, 4, h, w)))
    ref = vae_decode(vsd, TINY_VAE, z)
    y = pipe.vae.decode(z.cuda()).sample
    assert y.shape == ref.shape and rel_err(y, ref) < 1e-4


def test_vae_encode_vs_oracle(tiny):
    from oracle import vae_encode
    pipe, _, vsd = tiny
    img = _t(counter_normal(11, "img", (2, 3, 32, 48)))
    mean, logvar = vae_encode(vsd, TINY_VAE, img)
    dist = pipe.vae.encode(img.cuda()).latent_dist
    assert rel_err(dist.mean, mean) < 1e-4 and rel_err(dist.logvar, logvar) < 1e-4
    assert torch.equal(dist.mode(), dist.mean)


def test_vae_decode_latents_roundtrip_shapes_and_range(tiny):
    pipe = tiny[0]
    lat = _t(counter_normal(12, "lat", (2, 4, 3, 4, 6)))
    vid = pipe.decode_latents(lat.cuda())
    assert isinstance(vid, np.ndarray) and vid.shape == (2, 3, 3, 32, 48) and vid.dtype == np.float32
    assert vid.min() >= 0.0 and vid.max() <= 1.0


@pytest.mark.parametrize("guidance", [12.5, 1.0])
def test_generate_vs_oracle_end_to_end(tiny, guidance):
    """BASELINE config-1 shape of test at tiny size: 4-step DDIM, CFG, decode; frames within 1e-3 relative."""
    from oracle import generate
    pipe, usd, vsd = tiny
    b, f, h, w, tok = 2, 3, 8, 12, 9
    lat = _t(counter_normal(13, "lat", (b, 4, f, h, w)))
    cond = _t(counter_normal(14, "cond", (b, tok, TINY_UNET.cross_attention_dim)))
    unc = _t(counter_normal(15, "unc", (1, tok, TINY_UNET.cross_attention_dim)))
    trace = {}
    ref = generate(usd, TINY_UNET, vsd, TINY_VAE, lat, cond, unc, num_inference_steps=4, guidance_scale=guidance, trace=trace)
    eng = pipe.unet.engine
    vid, lat_out = eng.generate(lat.cuda(), cond.cuda(), unc.cuda(), 4, guidance, 0.0, decode=True, return_latents=True)
    assert rel_err(lat_out, trace["latents"][-1]) < 1e-3
    assert vid.shape == ref.shape
    assert (vid.cpu() - ref).abs().max().item() < 1e-3          # frames live in [0, 1]

    # teacher-forced per-step check (SURVEY §8(d) parity procedure ii): feed the oracle's latents of step k
    ts = eng.ddim_timesteps(4)
    x = lat
    for k, t in enumerate(ts):
        if guidance > 1.0:
            emb = torch.cat([unc.expand(b, -1, -1), cond])
            eps = pipe.unet(torch.cat([x, x]).cuda(), int(t), emb.cuda()).sample
            x_new = eng.ddim_cfg_step(eps[:b], eps[b:], x.cuda(), guidance, int(t), int(t) - 250)
        else:
            eps = pipe.unet(x.cuda(), int(t), cond.cuda()).sample
            x_new = eng.ddim_cfg_step(eps, None, x.cuda(), guidance, int(t), int(t) - 250)
        assert rel_err(x_new, trace["latents"][k]) < 2e-4, k
        x = trace["latents"][k]


def test_pipeline_call_matches_reference_semantics(tiny):
    """TuneAVideoPipeline.__call__ drop-in: same kwargs, output object, fused and stepped loops agree."""
    from oracle import generate
    pipe, usd, vsd = tiny
    b, f, tok = 1, 3, 77
    d = TINY_UNET.cross_attention_dim
    lat = _t(counter_normal(16, "lat", (b, 4, f, 4, 6)))
    eeg = _t(counter_normal(17, "eeg", (b, tok * d)))               # New variant: precomputed embeddings, model=None
    neg = _t(counter_normal(18, "neg", (1, tok, d)))
    out = pipe(None, eeg, video_length=f, height=32, width=48, num_inference_steps=3, guidance_scale=12.5,
               negative_prompt=neg, latents=lat.cuda())
    assert out.videos.shape == (b, 3, f, 32, 48) and out.videos.dtype == torch.float32 and out.videos.device.type == "cpu"
    assert out["videos"] is out.videos
    ref = generate(usd, TINY_UNET, vsd, TINY_VAE, lat, eeg.reshape(b, tok, d), neg, 3, 12.5)
    assert (out.videos - ref).abs().max().item() < 1e-3
    seen = []
    stepped = pipe(None, eeg, video_length=f, height=32, width=48, num_inference_steps=3, guidance_scale=12.5,
                   negative_prompt=neg, latents=lat.cuda(), callback=lambda i, t, x: seen.append((i, int(t))),
                   return_dict=False)
    assert seen == [(0, 667), (1, 334), (2, 1)]
    assert (stepped - out.videos).abs().max().item() < 1e-5
    # a `model` callable is applied to the EEG first (pipeline_tuneeeg2video.py:149)
    via_model = pipe(lambda e: e * 1.0, eeg, f, 32, 48, 3, 12.5, neg, latents=lat.cuda()).videos
    assert torch.equal(via_model, out.videos)


def test_pipeline_error_behaviour(tiny):
    pipe = tiny[0]
    d = TINY_UNET.cross_attention_dim
    eeg = torch.zeros(1, 77 * d)
    with pytest.raises(ValueError, match="has to be of type"):
        pipe(None, [1, 2], 3, 32, 48)
    with pytest.raises(ValueError, match="divisible by 8"):
        pipe(None, eeg, 3, 30, 48)
    with pytest.raises(ValueError, match="callback_steps"):
        pipe(None, eeg, 3, 32, 48, callback_steps=0)
    with pytest.raises(ValueError, match="Unexpected latents shape"):
        pipe(None, eeg, 3, 32, 48, guidance_scale=1.0, latents=torch.zeros(1, 4, 3, 5, 6))
    with pytest.raises(ValueError, match="generators"):
        pipe(None, eeg, 3, 32, 48, guidance_scale=1.0, generator=[torch.Generator(), torch.Generator()])
    with pytest.raises(ValueError, match="unconditional embedding"):
        pipe(None, eeg, 3, 32, 48, guidance_scale=7.5)
    with pytest.raises(RuntimeError):
        pipe.unet.load_state_dict({"conv_in.weight": torch.zeros(1)})


def test_cfg_guidance_one_is_identity(tiny):
    """g = 1: eps_u + 1 * (eps_c - eps_u) == eps_c (SURVEY §4 invariant v)."""
    eng = tiny[0].unet.engine
    x, eu, ec = (_t(counter_normal(19, k, (1, 4, 3, 4, 6))).cuda() for k in ("x", "eu", "ec"))
    a = eng.ddim_cfg_step(eu, ec, x, 1.0, 501, 481)
    b = eng.ddim_cfg_step(ec, None, x, 1.0, 501, 481)
    assert (a - b).abs().max().item() < 1e-6


def test_bf16_compute_mode_unet_and_generate(tiny):
    """BASELINE configs[2]: bf16 MFMA (fp32 accumulate) for convs / linears, everything else fp32.  bf16 keeps 8 mantissa
    bits, so the tolerance is 5e-2 of the tensor scale (the fp32 mode's is 1e-4)."""
    from oracle import generate, unet3d_forward
    pipe, usd, vsd = tiny
    eng = pipe.unet.engine
    x = _t(counter_normal(5, "x", (2, 4, 3, 9, 12)))
    cond = _t(counter_normal(6, "c", (2, 11, TINY_UNET.cross_attention_dim)))
    ref = unet3d_forward(usd, TINY_UNET, x, 301, cond)
    y32 = pipe.unet(x.cuda(), 301, cond.cuda()).sample
    try:
        eng.set_compute_dtype("bf16")
        y16 = pipe.unet(x.cuda(), 301, cond.cuda()).sample
        e = rel_err(y16, ref)
        assert 1e-5 < e < 5e-2, e                                   # really ran in bf16, and is still close
        lat = _t(counter_normal(13, "lat", (1, 4, 3, 8, 12)))
        c1 = _t(counter_normal(14, "cond", (1, 9, TINY_UNET.cross_attention_dim)))
        u1 = _t(counter_normal(15, "unc", (1, 9, TINY_UNET.cross_attention_dim)))
        vid = eng.generate(lat.cuda(), c1.cuda(), u1.cuda(), 4, 7.5, 0.0)
        refv = generate(usd, TINY_UNET, vsd, TINY_VAE, lat, c1, u1, 4, 7.5)
        assert (vid.cpu() - refv).abs().max().item() < 0.1 and torch.isfinite(vid).all()
    finally:
        eng.set_compute_dtype("fp32")
    assert torch.equal(pipe.unet(x.cuda(), 301, cond.cuda()).sample, y32)     # back to the parity configuration


@pytest.mark.parametrize("algo", ["1", "2", "3"])
def test_conv_algorithms_forced_unet_and_vae_vs_oracle(algo, monkeypatch):
    """E2V_CONV_ALGO=1: every 3x3 conv through the direct implicit GEMM; =2: every stride-1 3x3 conv in Winograd
    F(2x2,3x3) form with the resnets' GroupNorm + SiLU fused into its input transform; =3: the same in F(4x4,3x3) form.
    (The default, auto, picks per layer by channel count and map size and is what every other test of this file runs.)
    Same oracle, same tolerance."""
    from eeg2video_amd.pipeline import build_pipeline
    from oracle import unet3d_forward, vae_decode
    monkeypatch.setenv("E2V_CONV_ALGO", algo)
    usd = synth_state_dict(unet_param_spec(TINY_UNET), seed=42, mode="perturbed")
    vsd = synth_state_dict(vae_param_spec(TINY_VAE), seed=43, mode="perturbed")
    pipe = build_pipeline(TINY_UNET, TINY_VAE, device=0, unet_sd=usd, vae_sd=vsd)
    shape = (2, 4, 3, 9, 12)
    x = _t(counter_normal(5, "x", shape))
    cond = _t(counter_normal(6, "c", (shape[0], 11, TINY_UNET.cross_attention_dim)))
    ref = unet3d_forward({k: _t(v) for k, v in usd.items()}, TINY_UNET, x, 301, cond)
    y = pipe.unet(x.cuda(), 301, cond.cuda(), return_dict=False)[0]
    assert rel_err(y, ref) < 1e-4
    z = _t(counter_normal(11, "z", (2, 4, 4, 6)))
    refv = vae_decode({k: _t(v) for k, v in vsd.items()}, TINY_VAE, z)
    yv = pipe.vae.decode(z.cuda()).sample
    assert rel_err(yv, refv) < 1e-4


def test_ddim_next_step_vs_reference_golden(tiny, golden_dir):
    """e2v_ddim_next_step against the reference's own next_step outputs (tuneavideo/util.py:56-66)."""
    eng = tiny[0].unet.engine
    g = np.load(os.path.join(golden_dir, "reference_t1_inversion.npz"))
    eng.set_alphas_cumprod(g["inv.alphas_cumprod"])
    eps, x = _t(g["inv.eps"]).cuda(), _t(g["inv.x"]).cuda()
    for n, t in g["inv.next_step.cases"]:
        y = eng.ddim_next_step(eps, int(t), x, int(n))
        assert rel_err(y, _t(g[f"inv.next_step.n{n}.t{t}"])) < 2e-6, (n, t)


def test_ddim_inversion_vs_oracle_and_mirror(tiny):
    """The fused device loop (e2v_ddim_invert) and the tuneavideo/util.py mirror against the oracle's ddim_loop driving the
    oracle UNet; the inverted latent then round-trips through the generate loop's first steps without blowing up."""
    from eeg2video_amd.scheduler import DDIMScheduler
    from eeg2video_amd.util import ddim_inversion, next_step
    from oracle import DDIMOracle, ddim_loop, unet3d_forward
    pipe, usd, _ = tiny
    eng = pipe.unet.engine
    n = 3
    x = _t(counter_normal(31, "x", (2, 4, 3, 9, 12)))
    cond = _t(counter_normal(32, "c", (1, 11, TINY_UNET.cross_attention_dim)))
    so = DDIMOracle()
    so.set_timesteps(n)
    ref = ddim_loop(lambda l, t, c: unet3d_forward(usd, TINY_UNET, l, t, c), so, x, n, cond)
    sch = DDIMScheduler(engine=eng)
    sch.set_timesteps(n)
    got = ddim_inversion(pipe.unet, sch, x.cuda(), n, prompt=cond)
    assert len(got) == n + 1 and torch.equal(got[0].cpu(), x)
    for a, b in zip(got, ref):
        assert rel_err(a, b) < 1e-4
    last = eng.ddim_invert(x.cuda(), cond.repeat(2, 1, 1).cuda(), n, return_all=False)
    assert torch.equal(last, got[-1])
    # the stepwise mirror gives the same numbers as the fused loop
    lat = x.cuda()
    for i in range(n):
        t = int(sch.timesteps[len(sch.timesteps) - i - 1])
        eps = pipe.unet(lat, t, encoder_hidden_states=cond.repeat(2, 1, 1).cuda())["sample"]
        lat = next_step(eps, t, lat, sch)
    assert torch.equal(lat, got[-1])
    with pytest.raises(ValueError):
        ddim_inversion(pipe.unet, sch, x.cuda(), n + 1, prompt=cond)


def test_f32x3_mode_unet_vae_and_ops_vs_oracle(monkeypatch):
    """Opt-in E2V_F32X3: every linear / Winograd-domain GEMM runs as six bf16-piece MFMAs over exactly split operands
    (igemm_tile_x3).  It must meet the SAME tolerances as the fp32-MFMA path: per-op 2e-5 of the output scale, tiny UNet /
    VAE 1e-4 against the oracle."""
    from eeg2video_amd.pipeline import build_pipeline
    from oracle import unet3d_forward, vae_decode
    monkeypatch.setenv("E2V_F32X3", "1")
    usd = synth_state_dict(unet_param_spec(TINY_UNET), seed=42, mode="perturbed")
    vsd = synth_state_dict(vae_param_spec(TINY_VAE), seed=43, mode="perturbed")
    pipe = build_pipeline(TINY_UNET, TINY_VAE, device=0, unet_sd=usd, vae_sd=vsd)
    eng = pipe.unet.engine
    g = torch.Generator().manual_seed(3)
    for m, k, n in [(240, 1280, 1280), (1000, 320, 960), (77, 64, 128), (130, 40, 72)]:
        x, w, b, r = (torch.randn(*s, generator=g) for s in ((m, k), (n, k), (n,), (m, n)))
        w = w * 0.05
        eng.profile_begin()
        y = eng.op_linear(x.cuda(), w.cuda(), b.cuda(), r.cuda())
        assert "igemm_f32x3" in eng.profile_end(), "the split-bf16 kernel did not run"
        ref = torch.nn.functional.linear(x.double(), w.double(), b.double()) + r.double()
        assert (y.cpu().double() - ref).abs().max().item() <= 4e-5 * ref.abs().max().item()
    shape = (2, 4, 3, 9, 12)
    x = _t(counter_normal(5, "x", shape))
    cond = _t(counter_normal(6, "c", (shape[0], 11, TINY_UNET.cross_attention_dim)))
    ref = unet3d_forward({k: _t(v) for k, v in usd.items()}, TINY_UNET, x, 301, cond)
    y = pipe.unet(x.cuda(), 301, cond.cuda(), return_dict=False)[0]
    assert rel_err(y, ref) < 1e-4
    z = _t(counter_normal(11, "z", (2, 4, 4, 6)))
    refv = vae_decode({k: _t(v) for k, v in vsd.items()}, TINY_VAE, z)
    assert rel_err(pipe.vae.decode(z.cuda()).sample, refv) < 1e-4
    with pytest.raises(RuntimeError):                   # selecting it after the weights are finalized is a call-order error
        eng.set_compute_dtype("f32x3")


def test_pndm_scheduler_vs_oracle_and_pipeline(tiny):
    """PNDMScheduler mirror (host schedule + e2v_lincomb on the device) against oracle/pndm.py on a random trajectory, and
    the pipeline's stepped loop with it (guidance through e2v_cfg_combine) against the oracle loop."""
    from eeg2video_amd.scheduler import PNDMScheduler
    from oracle import PNDMOracle, generate
    pipe, usd, vsd = tiny
    eng = pipe.unet.engine
    so, sm = PNDMOracle(), PNDMScheduler(engine=eng)
    so.set_timesteps(7)
    sm.set_timesteps(7)
    assert sm.timesteps.tolist() == so.timesteps.tolist()
    xo = _t(counter_normal(41, "x", (2, 4, 3, 5, 6)))
    xm = xo.cuda()
    for i, t in enumerate(so.timesteps):
        eps = _t(counter_normal(42 + i, "e", (2, 4, 3, 5, 6)))
        xo = so.step(eps, int(t), xo)
        xm = sm.step(eps.cuda(), int(t), xm).prev_sample
        assert rel_err(xm, xo) < 2e-6, i
    eu, ec = _t(counter_normal(60, "u", (3, 7))), _t(counter_normal(61, "c", (3, 7)))
    assert rel_err(eng.cfg_combine(eu.cuda(), ec.cuda(), 12.5), eu + 12.5 * (ec - eu)) < 1e-6      # fused vs unfused multiply-add
    # whole pipeline, 3 inference steps (4 UNet evaluations), guidance on
    b, f, tok, d = 1, 3, 77, TINY_UNET.cross_attention_dim
    lat = _t(counter_normal(70, "lat", (b, 4, f, 4, 6)))
    eeg = _t(counter_normal(71, "eeg", (b, tok * d)))
    neg = _t(counter_normal(72, "neg", (1, tok, d)))
    ref = generate(usd, TINY_UNET, vsd, TINY_VAE, lat, eeg.reshape(b, tok, d), neg, 3, 7.5, scheduler=PNDMOracle())
    old = pipe.scheduler
    try:
        pipe.scheduler = PNDMScheduler(engine=eng)
        out = pipe(None, eeg, video_length=f, height=32, width=48, num_inference_steps=3, guidance_scale=7.5,
                   negative_prompt=neg, latents=lat.cuda()).videos
    finally:
        pipe.scheduler = old
    assert out.shape == ref.shape and (out - ref).abs().max().item() < 1e-3


def _save_sd_dir(root, usd, vsd, scheduler_cfg, half=True):
    """A local Stable-Diffusion directory as diffusers lays it out (model_index.json, unet/, vae/, scheduler/), tiny configs,
    weights saved as fp16 like the reference's checkpoints."""
    import json
    import dataclasses
    cast = (lambda v: v.half()) if half else (lambda v: v)
    os.makedirs(os.path.join(root, "unet")); os.makedirs(os.path.join(root, "vae")); os.makedirs(os.path.join(root, "scheduler"))
    ucfg = {"_class_name": "UNet3DConditionModel", "_diffusers_version": "0.11.1", "sample_size": TINY_UNET.sample_size,
            "in_channels": 4, "out_channels": 4, "block_out_channels": list(TINY_UNET.block_out_channels), "layers_per_block": 2,
            "cross_attention_dim": TINY_UNET.cross_attention_dim, "attention_head_dim": TINY_UNET.attention_head_dim,
            "norm_num_groups": 32, "norm_eps": 1e-5, "act_fn": "silu", "flip_sin_to_cos": True, "freq_shift": 0,
            "down_block_types": ["CrossAttnDownBlock2D"] * 3 + ["DownBlock2D"], "up_block_types": ["UpBlock2D"] + ["CrossAttnUpBlock2D"] * 3}
    json.dump(ucfg, open(os.path.join(root, "unet", "config.json"), "w"))
    torch.save({k: cast(v) for k, v in usd.items()}, os.path.join(root, "unet", "diffusion_pytorch_model.bin"))
    vcfg = {"_class_name": "AutoencoderKL", "_diffusers_version": "0.11.1", "in_channels": 3, "out_channels": 3, "latent_channels": 4,
            "block_out_channels": list(TINY_VAE.block_out_channels), "layers_per_block": TINY_VAE.layers_per_block,
            "norm_num_groups": TINY_VAE.norm_num_groups, "act_fn": "silu", "sample_size": 64,
            "down_block_types": ["DownEncoderBlock2D"] * 4, "up_block_types": ["UpDecoderBlock2D"] * 4}
    json.dump(vcfg, open(os.path.join(root, "vae", "config.json"), "w"))
    torch.save({k: cast(v) for k, v in vsd.items()}, os.path.join(root, "vae", "diffusion_pytorch_model.bin"))
    json.dump(scheduler_cfg, open(os.path.join(root, "scheduler", "scheduler_config.json"), "w"))
    json.dump({"_class_name": "StableDiffusionPipeline", "_diffusers_version": "0.11.1", "scheduler": ["diffusers", scheduler_cfg["_class_name"]],
               "unet": ["diffusers", "UNet2DConditionModel"], "vae": ["diffusers", "AutoencoderKL"]}, open(os.path.join(root, "model_index.json"), "w"))


@pytest.mark.parametrize("sched", ["DDIMScheduler", "PNDMScheduler"])
def test_from_pretrained_local_dir_fp16_as_the_reference_script_does(tiny, tmp_path, sched):
    """inference_eeg2video.py:69-72,90-98 with only the imports changed: UNet3DConditionModel.from_pretrained(dir,
    subfolder='unet', torch_dtype=float16).to('cuda'), TuneAVideoPipeline.from_pretrained(dir, unet=unet, torch_dtype=float16)
    .to('cuda'), enable_xformers / enable_vae_slicing, half latents.  `torch_dtype=torch.float16` selects the fp16 ARITHMETIC, as it
    does for the reference modules (round 5; it used to mean fp32 arithmetic on widened weights): the result sits within an fp16-grade
    distance of the fp32 oracle on the fp16-rounded weights; `.to(torch.float32)` -- and a pipeline loaded without a dtype -- give the
    fp32 result.  The stock SD-v1-4 directory carries a PNDM scheduler config with the outdated steps_offset the constructor patches
    (pipeline_tuneeeg2video.py:59-71)."""
    from eeg2video_amd.pipeline import TuneAVideoPipeline
    from eeg2video_amd.unet import UNet3DConditionModel
    from eeg2video_amd.vae import AutoencoderKL
    from oracle import DDIMOracle, PNDMOracle, generate
    _, usd, vsd = tiny
    scfg = {"_class_name": sched, "_diffusers_version": "0.11.1", "beta_start": 0.00085, "beta_end": 0.012,
            "beta_schedule": "scaled_linear", "num_train_timesteps": 1000, "set_alpha_to_one": False, "trained_betas": None,
            "steps_offset": 0 if sched == "PNDMScheduler" else 1}
    scfg.update({"clip_sample": False} if sched == "DDIMScheduler" else {"skip_prk_steps": True})
    root = str(tmp_path / "sd")
    _save_sd_dir(root, usd, vsd, scfg)
    unet = UNet3DConditionModel.from_pretrained(root, subfolder="unet", torch_dtype=torch.float16,
                                                vae_config=AutoencoderKL.config_from_dir(os.path.join(root, "vae"))).to("cuda")
    assert unet.engine.compute_dtype == "fp16"
    pipe = TuneAVideoPipeline.from_pretrained(root, unet=unet, torch_dtype=torch.float16).to("cuda")
    pipe.enable_xformers_memory_efficient_attention()
    pipe.enable_vae_slicing()
    pipe.set_progress_bar_config(disable=True)
    assert type(pipe.scheduler).__name__ == sched and pipe.scheduler.config.steps_offset == 1 and pipe.vae.engine is unet.engine
    assert unet.engine.compute_dtype == "fp16"
    b, f, tok, d = 1, 3, 77, TINY_UNET.cross_attention_dim
    lat = _t(counter_normal(70, "lat", (b, 4, f, 4, 6))).half()
    eeg = _t(counter_normal(71, "eeg", (b, tok * d))).half()
    neg = _t(counter_normal(72, "neg", (1, tok, d)))
    run = lambda p_: p_(None, eeg.cuda(), latents=lat, video_length=f, height=32, width=48, num_inference_steps=3, guidance_scale=12.5,
                        negative_prompt=neg).videos
    out = run(pipe)
    h = lambda sd: {k: v.half().float() for k, v in sd.items()}
    ref = generate(h(usd), TINY_UNET, h(vsd), TINY_VAE, lat.float(), eeg.float().reshape(b, tok, d), neg, 3, 12.5,
                   scheduler=DDIMOracle() if sched == "DDIMScheduler" else PNDMOracle())
    e16 = (out - ref).abs().max().item()
    assert out.dtype == torch.float32 and e16 < 1.5e-2, e16             # fp16 arithmetic under CFG 12.5 (bf16 on this clip: ~8x that)
    pipe.to(torch.float32)                                               # the same objects in the fp32 mode: the parity tolerance
    assert unet.engine.compute_dtype == "fp32"
    out32 = run(pipe)
    assert (out32 - ref).abs().max().item() < 1e-3
    # a whole pipeline from the directory alone (no unet=, no dtype given): fp32 mode, same result as the fp32 run above
    pipe2 = TuneAVideoPipeline.from_pretrained(root)
    pipe2.set_progress_bar_config(disable=True)
    assert pipe2.unet.engine.compute_dtype == "fp32"
    assert torch.equal(run(pipe2), out32)


def test_from_pretrained_2d_inflates_a_2d_checkpoint(tiny, tmp_path):
    """UNet3DConditionModel.from_pretrained_2d (unet.py:415-449; caller train_finetune_videodiffusion.py:110): a 2-D Stable-Diffusion
    UNet directory -- no `attn_temp` / `norm_temp` keys, 2-D block names in config.json -- loads into the 3-D model; the `_temp.` keys
    keep the FRESH model's init (unet.py:445-447: `if '_temp.' in k: state_dict.update({k: v})`), everything else comes from the
    checkpoint.  A missing config / weight file raises RuntimeError as the reference does (:421-422, :442-443)."""
    from eeg2video_amd.unet import UNet3DConditionModel
    from eeg2video_amd.vae import AutoencoderKL
    from oracle import unet3d_forward
    _, usd, vsd = tiny
    sd2d = {k: v for k, v in usd.items() if "_temp." not in k}
    assert 0 < len(sd2d) < len(usd)
    root = str(tmp_path / "sd2d")
    _save_sd_dir(root, sd2d, vsd, {"_class_name": "DDIMScheduler", "steps_offset": 1}, half=False)
    vcfg = AutoencoderKL.config_from_dir(os.path.join(root, "vae"))
    unet = UNet3DConditionModel.from_pretrained_2d(root, subfolder="unet", vae_config=vcfg)
    # the state dict the reference would end up with: checkpoint values + fresh `_temp.` parameters of this architecture
    fresh = synth_state_dict({k: s for k, s in unet.state_dict_spec().items() if "_temp." in k}, mode="reference_init")
    full = dict(sd2d)
    full.update({k: _t(v) for k, v in fresh.items()})
    assert set(full) == set(usd)
    assert float(full["down_blocks.0.attentions.0.transformer_blocks.0.attn_temp.to_out.0.weight"].abs().max()) == 0.0   # attention.py:201
    x = _t(counter_normal(5, "x", (2, 4, 3, 9, 12)))
    cond = _t(counter_normal(6, "c", (2, 11, TINY_UNET.cross_attention_dim)))
    y = unet(x.cuda(), 333, cond.cuda())["sample"]
    ref = unet3d_forward(full, TINY_UNET, x, 333, cond)
    assert rel_err(y, ref) < 1e-4
    with pytest.raises(RuntimeError, match="does not exist"):
        UNet3DConditionModel.from_pretrained_2d(str(tmp_path / "nowhere"), subfolder="unet")
    os.remove(os.path.join(root, "unet", "diffusion_pytorch_model.bin"))
    with pytest.raises(RuntimeError, match="does not exist"):
        UNet3DConditionModel.from_pretrained_2d(root, subfolder="unet", vae_config=vcfg)


def test_use_linear_projection_checkpoint_loads_and_matches(tiny):
    """UNet3DConditionModel(use_linear_projection=True) (unet.py:59, attention.py:60-63,83-86: Linear-shaped proj_in / proj_out weights as SD-2.x checkpoints carry them, proj_in /
    proj_out stored as [C, C] nn.Linear weights): the mirror reshapes the two weights to the 1x1-conv layout -- the same GEMM on
    channel-last rows (pinned against the reference itself in tests/test_oracle_golden.py) -- so the model must load such a state dict
    and give bit for bit what the conv-shaped one gives."""
    from eeg2video_amd.unet import UNet3DConditionModel
    pipe, usd, _ = tiny
    kw = dict(sample_size=TINY_UNET.sample_size, in_channels=4, out_channels=4, block_out_channels=TINY_UNET.block_out_channels,
              layers_per_block=TINY_UNET.layers_per_block, cross_attention_dim=TINY_UNET.cross_attention_dim,
              attention_head_dim=TINY_UNET.attention_head_dim, norm_num_groups=TINY_UNET.norm_num_groups, norm_eps=TINY_UNET.norm_eps)
    lin_sd = {k: (v.reshape(v.shape[0], v.shape[1]) if k.endswith(("proj_in.weight", "proj_out.weight")) else v) for k, v in usd.items()}
    assert any(v.ndim == 2 and k.endswith("proj_in.weight") for k, v in lin_sd.items())
    m = UNet3DConditionModel(use_linear_projection=True, upcast_attention=True, device=0, **kw)   # (fp32 scores / softmax: always the case here)
    m.load_state_dict(lin_sd)
    x = _t(counter_normal(5, "x", (2, 4, 3, 9, 12))).cuda()
    cond = _t(counter_normal(6, "c", (2, 11, TINY_UNET.cross_attention_dim))).cuda()
    assert torch.equal(m(x, 301, cond).sample, pipe.unet(x, 301, cond).sample)
    with pytest.raises(RuntimeError):                      # the conv-shaped mirror still refuses the Linear-shaped weights
        UNet3DConditionModel(device=0, **kw).load_state_dict(lin_sd)
    with pytest.raises(RuntimeError, match="size mismatch"):   # and the Linear-shaped mirror the conv-shaped ones, as the reference's strict load does
        UNet3DConditionModel(use_linear_projection=True, device=0, **kw).load_state_dict(usd)


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_per_block_attention_head_dim_vs_oracle(tiny, mode):
    """`attention_head_dim` as a tuple (unet.py:71,110-111): down block i takes entry i (:131), the mid block the last one (:151), the up
    blocks the reversed list (:165,194) -- the SD-2.x UNet's 5 / 10 / 20 / 20.  Tiny config with 4 / 4 / 8 / 16 heads (head dims 16 / 32 /
    32 / 16): against the oracle (which walks the same three index rules), and a uniform tuple is the int."""
    import dataclasses
    from eeg2video_amd.unet import UNet3DConditionModel
    from oracle import unet3d_forward
    _, usd, _ = tiny
    heads = (4, 4, 8, 16)
    cfg = dataclasses.replace(TINY_UNET, attention_head_dim=heads)
    kw = dict(sample_size=cfg.sample_size, in_channels=4, out_channels=4, block_out_channels=cfg.block_out_channels, layers_per_block=cfg.layers_per_block,
              cross_attention_dim=cfg.cross_attention_dim, norm_num_groups=cfg.norm_num_groups, norm_eps=cfg.norm_eps)
    m = UNet3DConditionModel(attention_head_dim=heads, device=0, **kw)
    m.load_state_dict(usd)                                  # (the weights do not depend on the head count)
    x = _t(counter_normal(15, "x", (2, 4, 3, 9, 12)))
    cond = _t(counter_normal(16, "c", (2, 11, cfg.cross_attention_dim)))
    ref = unet3d_forward(usd, cfg, x, 301, cond)
    ref8 = unet3d_forward(usd, TINY_UNET, x, 301, cond)
    assert rel_err(ref, ref8) > 1e-3                       # (another model: the head split changes the attention)
    try:
        m.engine.set_compute_dtype(mode)
        y = m(x.cuda(), 301, cond.cuda()).sample
    finally:
        m.engine.set_compute_dtype("fp32")
    assert rel_err(y, ref) < (1e-4 if mode == "fp32" else 5e-3), rel_err(y, ref)
    if mode == "fp32":
        u = UNet3DConditionModel(attention_head_dim=(8, 8, 8, 8), device=0, **kw)
        u.load_state_dict(usd)
        assert u.ucfg.attention_head_dim == 8
        with pytest.raises(ValueError, match="entries"):
            UNet3DConditionModel(attention_head_dim=(8, 8), device=0, **kw)
        m.set_attention_slice("auto")                       # per-block head counts reach the slice check (unet.py:209-272): 16 blocks x 3
        assert m._attention_slice[:3] == [2, 2, 2] and m._attention_slice[-3:] == [2, 2, 2] and max(m._attention_slice) == 8
        assert len(m._attention_slice) == 48


def test_memory_knobs_of_the_reference_objects_are_accepted(tiny):
    """set_attention_slice (unet.py:209-272), enable_gradient_checkpointing (:274-276), enable_sequential_cpu_offload
    (pipeline_tuneeeg2video.py:121-131): a caller that sets them keeps working; the argument checks and messages of
    set_attention_slice are the reference's; the output does not change."""
    pipe, _, _ = tiny
    unet = pipe.unet
    x = _t(counter_normal(5, "x", (1, 4, 3, 8, 8))).cuda()
    cond = _t(counter_normal(6, "c", (1, 7, TINY_UNET.cross_attention_dim))).cuda()
    before = unet(x, 10, cond).sample
    unet.set_attention_slice("auto")
    unet.set_attention_slice("max")
    unet.set_attention_slice(2)
    n_layers = 3 * 16                                      # attn1, attn2, attn_temp of the 16 transformer blocks
    unet.set_attention_slice([1] * n_layers)
    with pytest.raises(ValueError, match="different attention layers"):
        unet.set_attention_slice([1] * (n_layers - 1))
    with pytest.raises(ValueError, match="has to be smaller or equal to"):
        unet.set_attention_slice(TINY_UNET.attention_head_dim + 1)
    unet.enable_gradient_checkpointing()
    pipe.enable_sequential_cpu_offload()
    pipe.enable_sequential_cpu_offload(gpu_id=0)
    with pytest.raises(ValueError):
        pipe.enable_sequential_cpu_offload(gpu_id=7)
    pipe.enable_attention_slicing()
    assert torch.equal(unet(x, 10, cond).sample, before)


def test_text_prompt_twin_with_precomputed_embeddings(tiny):
    """pipeline_tuneavideo.py:315-412 (caller train_finetune_videodiffusion.py:331-335): same kwargs -- prompt, negative_prompt,
    num_videos_per_prompt -- with the prompt given as precomputed [B,77,768]-style embeddings (the CLIP text encoder is outside the
    path): identical frames to the EEG pipeline fed the same embeddings; the reference's errors for a bad prompt type / mismatched
    negative prompt; a str prompt without tokenizer / text_encoder says what is missing; with a (stub) tokenizer + text encoder
    the str path runs, the empty prompt giving the unconditional embedding (:189-190)."""
    from eeg2video_amd.pipeline_tuneavideo import TuneAVideoPipeline as TextPipeline
    pipe, _, _ = tiny
    tp = TextPipeline(vae=pipe.vae, text_encoder=None, tokenizer=None, unet=pipe.unet, scheduler=pipe.scheduler)
    tp.set_progress_bar_config(disable=True)
    d, tok, f = TINY_UNET.cross_attention_dim, 77, 3
    emb = _t(counter_normal(80, "emb", (2, tok, d)))
    neg = _t(counter_normal(81, "neg", (1, tok, d)))
    lat = _t(counter_normal(82, "lat", (2, 4, f, 4, 6)))
    a = tp(emb, video_length=f, height=32, width=48, num_inference_steps=3, guidance_scale=7.5, negative_prompt=neg, latents=lat).videos
    b = pipe(None, emb.reshape(2, -1).cuda(), latents=lat, video_length=f, height=32, width=48, num_inference_steps=3, guidance_scale=7.5,
             negative_prompt=neg).videos
    assert a.shape == (2, 3, f, 32, 48) and torch.equal(a, b)
    # num_videos_per_prompt repeats each prompt's embedding (:182-184); latents are per generated video
    lat4 = _t(counter_normal(83, "lat4", (4, 4, f, 4, 6)))
    c = tp(emb, video_length=f, height=32, width=48, num_inference_steps=2, guidance_scale=7.5, negative_prompt=neg, latents=lat4,
           num_videos_per_prompt=2).videos
    e = pipe(None, emb.repeat_interleave(2, 0).reshape(4, -1).cuda(), latents=lat4, video_length=f, height=32, width=48,
             num_inference_steps=2, guidance_scale=7.5, negative_prompt=neg).videos
    assert torch.equal(c, e)
    with pytest.raises(ValueError, match="`prompt` has to be of type"):
        tp(3.0, video_length=f, height=32, width=48)
    with pytest.raises(TypeError, match="`negative_prompt` should be the same type"):
        tp(emb, video_length=f, height=32, width=48, negative_prompt="a photo", latents=lat)
    with pytest.raises(ValueError, match="tokenizer"):
        tp("a panda", video_length=f, height=32, width=48, latents=lat[:1])

    class Tok:                      # minimal stand-ins with the transformers CLIP call interface
        model_max_length = tok

        def __call__(self, prompts, padding=None, max_length=None, truncation=None, return_tensors=None):
            ids = torch.zeros((len(prompts), max_length), dtype=torch.long)
            for i, p in enumerate(prompts):
                ids[i, :len(p)] = torch.tensor([ord(ch) % 50 + 1 for ch in p][:max_length], dtype=torch.long)
            return type("Enc", (), {"input_ids": ids, "attention_mask": (ids > 0).long()})()

    class Enc(torch.nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(0)
            self.table = torch.nn.Embedding(64, d)

        def forward(self, ids, attention_mask=None):
            return (self.table(ids),)

    enc = Enc().cuda()
    tp2 = TextPipeline(vae=pipe.vae, text_encoder=enc, tokenizer=Tok(), unet=pipe.unet, scheduler=pipe.scheduler)
    tp2.set_progress_bar_config(disable=True)
    v = tp2(["a panda", "a bear"], video_length=f, height=32, width=48, num_inference_steps=2, guidance_scale=7.5, latents=lat).videos
    with torch.no_grad():
        pe = enc(Tok()(["a panda", "a bear"], max_length=tok).input_ids.cuda())[0]
        ne = enc(Tok()(["", ""], max_length=tok).input_ids.cuda())[0]
    w = tp(pe, video_length=f, height=32, width=48, num_inference_steps=2, guidance_scale=7.5, negative_prompt=ne, latents=lat).videos
    assert torch.equal(v, w)
