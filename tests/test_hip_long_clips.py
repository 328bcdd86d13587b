"""GPU: long clips (video_length > 8) -- temporal_attn_long_kernel against the torch reference of the op, the sparse-causal attention at a
frame count the other tests never reach, and the tiny / full UNet, generate, pipeline and DDIM inversion against the oracle at F > 8.

Tolerances are the ones the F <= 8 tests use (tests/test_hip_ops.py, test_hip_model.py, test_hip_full.py)."""
import numpy as np
import pytest
import torch

from eeg2video_amd.weights import (TINY_UNET, TINY_VAE, UNetConfig, VAEConfig, counter_normal, synth_state_dict, unet_param_spec,
                                   vae_param_spec)

pytestmark = pytest.mark.gpu

H16_TYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
TOL = {"bf16": 8e-3, "fp16": 1e-3, "fp32": 1e-4}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def close(a, b, rtol, atol):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = b.abs().max().item() + 1e-30
    err = (a - b).abs().max().item()
    assert err <= atol * max(1.0, scale) + rtol * scale, f"max abs err {err:.3e} (ref scale {scale:.3e})"


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _ref_attn(q, k, v, scale):
    s = torch.baddbmm(torch.empty(q.shape[0], q.shape[1], k.shape[1]), q, k.transpose(1, 2), beta=0, alpha=scale)
    return torch.bmm(s.softmax(-1), v)


def _heads(x, h):
    b, s, c = x.shape
    return x.reshape(b, s, h, c // h).permute(0, 2, 1, 3).reshape(b * h, s, c // h)


def _unheads(x, h):
    bh, s, d = x.shape
    return x.reshape(bh // h, h, s, d).permute(0, 2, 1, 3).reshape(bh // h, s, h * d)


def _temporal_ref(qkv, n, f, hw, heads, d):
    """attention.py:261-267: '(b f) d c -> (b d) f c', attention over the frames of each pixel, and back."""
    c = heads * d
    t = qkv.reshape(n, f, hw, 3 * c).permute(0, 2, 1, 3).reshape(n * hw, f, 3 * c)
    q, k, v = t[..., :c], t[..., c:2 * c], t[..., 2 * c:]
    ref = _unheads(_ref_attn(_heads(q, heads), _heads(k, heads), _heads(v, heads), d ** -0.5), heads)
    return ref.reshape(n, hw, f, c).permute(0, 2, 1, 3).reshape(n * f * hw, c)


@pytest.fixture(scope="module")
def eng():
    from eeg2video_amd.engine import Engine
    return Engine(TINY_UNET, TINY_VAE, 0)


def _run_mode(eng, mode, fn):
    try:
        eng.set_compute_dtype(mode)
        return fn()
    finally:
        eng.set_compute_dtype("fp32")


# ------------------------------------------------------------------ the op ---------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("d", [8, 40, 80, 160])
@pytest.mark.parametrize("f", [9, 12, 16, 17, 24, 32, 33, 64])
def test_long_temporal_attention_vs_torch(eng, mode, d, f):
    heads, n, hw = 8, 2, 33
    qkv = rnd(n * f * hw, 3 * heads * d, seed=300 + f)
    src = qkv.to(H16_TYPES[mode]).float() if mode != "fp32" else qkv
    ref = _temporal_ref(src, n, f, hw, heads, d)
    g = qkv.cuda()
    y = _run_mode(eng, mode, lambda: eng.op_temporal_attention(g, n=n, F=f, HW=hw, heads=heads, D=d, scale=d ** -0.5))
    close(y, ref, rtol=TOL[mode], atol=TOL[mode])


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("f", [16, 40])
def test_long_temporal_attention_large_scores(eng, mode, f):
    """q.k of about +-80 after the scale: the softmax must subtract its running maximum (exp(80) overflows fp32's exp2 range only
    without it) and rescale across key tiles."""
    heads, n, hw, d = 8, 1, 20, 40
    qkv = rnd(n * f * hw, 3 * heads * d, seed=401)
    c = heads * d
    qkv[:, :2 * c] *= 4.5            # q.k * d^-0.5 has a standard deviation of ~20: extremes of +-60 ... 90
    src = qkv.to(H16_TYPES[mode]).float() if mode != "fp32" else qkv
    ref = _temporal_ref(src, n, f, hw, heads, d)
    s = torch.einsum("nfpc,ngpc->nfgp", *(src.reshape(n, f, hw, 3 * c)[..., i * c:i * c + d] for i in (0, 1))) * d ** -0.5
    assert s.abs().max() > 50
    g = qkv.cuda()
    y = _run_mode(eng, mode, lambda: eng.op_temporal_attention(g, n=n, F=f, HW=hw, heads=heads, D=d, scale=d ** -0.5))
    assert torch.isfinite(y).all()
    close(y, ref, rtol=TOL[mode], atol=TOL[mode])


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("d,f", [(40, 24), (160, 33)])
def test_long_temporal_attention_is_deterministic_and_per_sample(eng, mode, d, f):
    """Two runs are bit-identical, and n = 3 equals its three n = 1 slices bit for bit."""
    heads, n, hw = 8, 3, 37
    c = heads * d
    qkv = rnd(n * f * hw, 3 * c, seed=402).cuda()
    run = lambda x, m: eng.op_temporal_attention(x, n=m, F=f, HW=hw, heads=heads, D=d, scale=d ** -0.5)

    def go():
        a, b = run(qkv, n), run(qkv, n)
        ones = [run(qkv[i * f * hw:(i + 1) * f * hw].contiguous(), 1) for i in range(n)]
        return a, b, ones
    a, b, ones = _run_mode(eng, mode, go)
    assert torch.equal(a, b)
    for i in range(n):
        assert torch.equal(a[i * f * hw:(i + 1) * f * hw], ones[i]), i


def test_sparse_causal_attention_at_sixteen_frames(eng):
    """attention.py:292-321 at F = 16: keys / values of frame i = [frame 0 ; frame max(i-1, 0)]."""
    d, nq, f, n, heads = 40, 50, 16, 2, 8
    c = heads * d
    qkv = rnd(n * f * nq, 3 * c, seed=403)
    q, k, v = (qkv[:, i * c:(i + 1) * c].reshape(n * f, nq, c) for i in range(3))
    former = torch.arange(f) - 1
    former[0] = 0
    gather = lambda t: torch.cat([t.reshape(n, f, nq, c)[:, [0] * f], t.reshape(n, f, nq, c)[:, former]], dim=2).reshape(n * f, 2 * nq, c)
    ref = _unheads(_ref_attn(_heads(q, heads), _heads(gather(k), heads), _heads(gather(v), heads), d ** -0.5), heads)
    g = qkv.cuda()
    y = eng.op_attention(g[:, :c], g[:, c:2 * c], g[:, 2 * c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nq, mode=0, scale=d ** -0.5)
    close(y.reshape(n * f, nq, c), ref, rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------ tiny model -----------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from eeg2video_amd.pipeline import build_pipeline
    usd = synth_state_dict(unet_param_spec(TINY_UNET), seed=42, mode="perturbed")
    vsd = synth_state_dict(vae_param_spec(TINY_VAE), seed=43, mode="perturbed")
    pipe = build_pipeline(TINY_UNET, TINY_VAE, device=0, unet_sd=usd, vae_sd=vsd)
    pipe.set_progress_bar_config(disable=True)
    return pipe, {k: _t(v) for k, v in usd.items()}, {k: _t(v) for k, v in vsd.items()}


@pytest.mark.parametrize("shape,tokens", [((2, 4, 9, 9, 12), 11), ((1, 4, 16, 8, 8), 77), ((1, 4, 24, 5, 7), 5)])
def test_tiny_unet_forward_long_clip_vs_oracle(tiny, shape, tokens):
    from oracle import unet3d_forward
    pipe, usd, _ = tiny
    x = _t(counter_normal(405, "x", shape))
    cond = _t(counter_normal(406, "c", (shape[0], tokens, TINY_UNET.cross_attention_dim)))
    ref = unet3d_forward(usd, TINY_UNET, x, 301, cond)
    y = pipe.unet(x.cuda(), 301, cond.cuda(), return_dict=False)[0]
    assert y.shape == ref.shape and rel_err(y, ref) < 1e-4


def test_tiny_generate_pipeline_and_inversion_long_clip(tiny):
    from eeg2video_amd.scheduler import DDIMScheduler
    from eeg2video_amd.util import ddim_inversion
    from oracle import DDIMOracle, ddim_loop, generate, unet3d_forward
    pipe, usd, vsd = tiny
    eng = pipe.unet.engine
    d = TINY_UNET.cross_attention_dim
    # generate end to end: 3 steps, CFG 12.5, F = 16
    b, f, h, w, tok = 1, 16, 4, 6, 9
    lat = _t(counter_normal(407, "lat", (b, 4, f, h, w)))
    cond = _t(counter_normal(408, "cond", (b, tok, d)))
    unc = _t(counter_normal(409, "unc", (1, tok, d)))
    ref = generate(usd, TINY_UNET, vsd, TINY_VAE, lat, cond, unc, num_inference_steps=3, guidance_scale=12.5)
    vid = eng.generate(lat.cuda(), cond.cuda(), unc.cuda(), 3, 12.5, 0.0)
    assert vid.shape == ref.shape == (b, 3, f, 32, 48)
    assert (vid.cpu() - ref).abs().max().item() < 1e-3
    # the pipeline's __call__ with video_length = 16
    eeg = _t(counter_normal(410, "eeg", (b, 77 * d)))
    neg = _t(counter_normal(411, "neg", (1, 77, d)))
    out = pipe(None, eeg, video_length=f, height=32, width=48, num_inference_steps=3, guidance_scale=12.5, negative_prompt=neg,
               latents=lat.cuda())
    assert out.videos.shape == (b, 3, f, 32, 48) and torch.isfinite(out.videos).all()
    ref2 = generate(usd, TINY_UNET, vsd, TINY_VAE, lat, eeg.reshape(b, 77, d), neg, 3, 12.5)
    assert (out.videos - ref2).abs().max().item() < 1e-3
    # DDIM inversion at F = 12 against the oracle loop
    n = 3
    x = _t(counter_normal(412, "x", (1, 4, 12, 5, 6)))
    c = _t(counter_normal(413, "c", (1, 11, d)))
    so = DDIMOracle()
    so.set_timesteps(n)
    want = ddim_loop(lambda l, t, cc: unet3d_forward(usd, TINY_UNET, l, t, cc), so, x, n, c)
    sch = DDIMScheduler(engine=eng)
    sch.set_timesteps(n)
    got = ddim_inversion(pipe.unet, sch, x.cuda(), n, prompt=c)
    assert len(got) == n + 1
    for a, r in zip(got, want):
        assert rel_err(a, r) < 1e-4


def test_tiny_long_clip_batch_entries_are_bit_identical_to_single_calls(tiny):
    """fp32, F = 16: a B = 3 generate equals the three single-clip calls bit for bit (test_hip_full.py holds this at F = 6)."""
    pipe = tiny[0]
    eng = pipe.unet.engine
    d = TINY_UNET.cross_attention_dim
    lat = torch.stack([_t(counter_normal(420 + k, "lat", (4, 16, 4, 6))) for k in range(3)]).cuda()
    cond = torch.stack([_t(counter_normal(430 + k, "cond", (9, d))) for k in range(3)]).cuda()
    unc = _t(counter_normal(440, "unc", (1, 9, d))).cuda()
    vid, lat_out = eng.generate(lat, cond, unc, 2, 12.5, 0.0, decode=True, return_latents=True)
    for k in range(3):
        v1, l1 = eng.generate(lat[k:k + 1], cond[k:k + 1], unc, 2, 12.5, 0.0, decode=True, return_latents=True)
        assert torch.equal(l1[0], lat_out[k]), k
        assert torch.equal(v1[0], vid[k]), k


# ------------------------------------------------------------------ full size ------------------------------------------------------
@pytest.fixture(scope="module")
def full():
    from eeg2video_amd.pipeline import build_pipeline
    ucfg, vcfg = UNetConfig(), VAEConfig()
    usd = synth_state_dict(unet_param_spec(ucfg), seed=42, mode="reference_init")
    vsd = synth_state_dict(vae_param_spec(vcfg), seed=43, mode="reference_init")
    pipe = build_pipeline(ucfg, vcfg, device=0, unet_sd=usd, vae_sd=vsd)
    pipe.set_progress_bar_config(disable=True)
    return pipe, usd


def test_full_unet_sample_sixteen_frames_vs_oracle(full):
    """[1,4,16,36,64], t = 501 (the oracle takes about 2.7x the F = 6 sample's time).  fp32 within 1e-3 of the reference scale; bf16 and
    fp16 no worse than 1.5x their own distance at F = 6 on the same seeds (computed here)."""
    from oracle import unet3d_forward
    pipe, usd = full
    eng = pipe.unet.engine
    sd = {k: _t(v) for k, v in usd.items()}
    cond = _t(counter_normal(1235, "cond", (1, 77, 768)))
    errs = {}
    for f in (6, 16):
        x = _t(counter_normal(1234, "latent", (1, 4, f, 36, 64)))
        with torch.no_grad():
            ref = unet3d_forward(sd, UNetConfig(), x, 501, cond)
        for mode in ("fp32", "bf16", "fp16"):
            y = _run_mode(eng, mode, lambda: pipe.unet(x.cuda(), 501, cond.cuda()).sample.float())
            assert y.shape == (1, 4, f, 36, 64)
            errs[mode, f] = rel_err(y, ref)
    print("full UNet sample max-abs / max-ref: " + ", ".join(f"{m} F{f} {e:.3e}" for (m, f), e in errs.items()))
    assert errs["fp32", 16] < 1e-3
    for mode in ("bf16", "fp16"):
        assert errs[mode, 16] <= 1.5 * errs[mode, 6], mode
