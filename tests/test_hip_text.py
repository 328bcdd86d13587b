"""GPU: the CLIP text encoder (``e2v_text_encode``, ``csrc/text.hip``) against ``transformers``.

References: the committed fixture (``tests/golden/clip_text_tiny.npz``: ``transformers.CLIPTextModel`` outputs) where it applies, the
float64 run of the plain-torch restatement (``tests/clip_text_restatement.py``, pinned to the fixture on the CPU) for every other shape.
Metric and bound: max |a-b| / max |b| < 1e-5 -- fp32 arithmetic on the GEMM kernels the Semantic Predictor meets the same bound with;
torch-fp32 itself sits 6.3e-7 (tiny) .. 1.3e-6 (full SD-v1-4 size) from float64 on the fixture's kind of weights (measured when the
fixture was written: ``tests/clip_text_restatement.py``).
"""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from clip_text_restatement import causal_attention, clip_text_forward, rel_err
from eeg2video_amd.weights import (TINY_TEXT, TINY_UNET, TINY_VAE, TextConfig, counter_normal, synth_state_dict, text_param_spec,
                                   unet_param_spec, vae_param_spec)
from test_hip_bounds import GUARD_KIB, PADS, environment, fenced, fenced_out, run_fenced

pytestmark = pytest.mark.gpu

BOUND = 1e-5
T_CASES = (1, 13, 64, 77)          # one token; a partial wave of queries; exactly one wave; one wave and the 13-row tail


def make_engine(text_cfg):
    from eeg2video_amd.engine import Engine
    return Engine(TINY_UNET, TINY_VAE, 0, text_cfg=text_cfg)


def make_encoder(text_cfg, sd, engine=None):
    from eeg2video_amd.text_encoder import CLIPTextModel
    return CLIPTextModel(text_cfg, engine=engine or make_engine(text_cfg)).load_state_dict(sd)


def synth_text(cfg, seed=5):
    """counter-RNG weights; q / k projections scaled up so that the softmax rows are far from uniform (scores of std ~2 instead of 0.1)"""
    sd = synth_state_dict(text_param_spec(cfg), seed=seed, mode="perturbed")
    for k in sd:
        if k.endswith("q_proj.weight") or k.endswith("k_proj.weight"):
            sd[k] = sd[k] * 4.0
    return sd


def draw_ids(cfg, b, t, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, cfg.vocab_size, (b, t), generator=g)


def check(out, ref, what):
    err = rel_err(out, ref)
    print(f"{what}: max|a-b|/max|b| = {err:.3e} (bound {BOUND:.0e})")
    assert tuple(out.shape) == tuple(ref.shape) and not torch.isnan(out).any() and err < BOUND, (what, err)


@pytest.fixture(scope="module")
def fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "clip_text_tiny.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def tiny():
    """(encoder at TINY_TEXT with synthetic weights, the weights)"""
    sd = synth_text(TINY_TEXT)
    return make_encoder(TINY_TEXT, sd), sd


@pytest.fixture(scope="module")
def tiny_ref(tiny):
    """float64 restatement outputs of the tiny model, computed once per (B, T)"""
    _, sd = tiny
    cache = {}

    def get(b, t):
        if (b, t) not in cache:
            ids = draw_ids(TINY_TEXT, b, t, seed=100 * b + t)
            cache[(b, t)] = (ids, clip_text_forward(sd, ids, TINY_TEXT, torch.float64))
        return cache[(b, t)]
    return get


# ------------------------------------------------------------------ 1. the fixture ---------------------------------------------------
@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_fixture_parity_with_transformers(fixture, act):
    cfg = dataclasses.replace(TINY_TEXT, hidden_act=act)
    sd = {k: v for k, v in fixture.items() if k.startswith("text_model.")}
    enc = make_encoder(cfg, sd)
    out = enc(torch.from_numpy(fixture["input_ids"]))
    assert out[0] is out.last_hidden_state and out[0].dtype == torch.float32 and out[0].is_cuda
    check(out[0], torch.from_numpy(fixture["out_" + act]), f"HIP vs transformers {fixture['transformers_version']} ({act})")
    assert enc.engine.weight_forms("text.text_model.encoder.layers.0.self_attn.q_proj.weight") == 1        # fp32 only
    assert enc.engine.weight_forms("text.text_model.encoder.layers.1.mlp.fc2.weight") == 1
    assert enc.engine.weight_forms("text.text_model.embeddings.token_embedding.weight") == 1


def test_checkpoint_keys_without_the_prefix_and_with_position_ids(fixture, tiny):
    """``transformers`` 5 keys the state dict without ``text_model.``; older checkpoints carry an ``embeddings.position_ids`` buffer"""
    sd = {k[len("text_model."):]: v for k, v in fixture.items() if k.startswith("text_model.")}
    sd["embeddings.position_ids"] = np.arange(77)[None]
    enc = make_encoder(TINY_TEXT, sd)
    check(enc(fixture["input_ids"])[0], torch.from_numpy(fixture["out_quick_gelu"]), "prefix-less keys")
    del sd["final_layer_norm.bias"]
    with pytest.raises(RuntimeError, match="missing"):
        tiny[0].load_state_dict(sd)


# ------------------------------------------------------------------ 2. shapes -------------------------------------------------------
@pytest.mark.parametrize("t", T_CASES)
@pytest.mark.parametrize("b", [1, 5])
def test_shapes_vs_restatement(tiny, tiny_ref, b, t):
    ids, ref = tiny_ref(b, t)
    check(tiny[0](ids)[0], ref, f"tiny B={b} T={t}")


@pytest.mark.parametrize("t", T_CASES + (65, 127))          # and the second key block with one and with 63 live lanes
@pytest.mark.parametrize("heads", [1, 2, 3])
def test_op_causal_attention(tiny, heads, t):
    b = 2
    qkv = torch.from_numpy(counter_normal(7 * heads + t, "qkv", (b * t, 3 * heads * 64)))
    out = tiny[0].engine.op_causal_attention(qkv.cuda(), B=b, T=t, heads=heads)
    check(out, causal_attention(qkv, b, t, heads), f"op heads={heads} T={t}")


def test_op_causal_attention_at_the_lds_limit(tiny):
    """T = 128, the largest prompt the kernel takes (two full passes of keys per lane); 129 is refused"""
    eng, b, heads = tiny[0].engine, 1, 2
    qkv = torch.from_numpy(counter_normal(3, "qkv128", (b * 128, 3 * heads * 64)))
    check(eng.op_causal_attention(qkv.cuda(), B=b, T=128, heads=heads), causal_attention(qkv, b, 128, heads), "op T=128")
    with pytest.raises(ValueError, match="128"):
        eng.op_causal_attention(torch.zeros(129, 3 * 64, device="cuda"), B=1, T=129, heads=1)


# ------------------------------------------------------------------ 3. real widths --------------------------------------------------
def test_one_layer_at_sd_v1_4_widths():
    """768 / 12 heads / 3072: the LayerNorm-768 and K = 3072 instances (one layer, vocab 64: no 12-layer model in the suite)"""
    cfg = TextConfig(vocab_size=64, hidden=768, heads=12, layers=1, intermediate=3072, max_positions=77)
    sd = synth_text(cfg, seed=9)
    ids = draw_ids(cfg, 2, 77, seed=11)
    check(make_encoder(cfg, sd)(ids)[0], clip_text_forward(sd, ids, cfg, torch.float64), "one layer at 768/12/3072")


# ------------------------------------------------------------------ 4. causality ----------------------------------------------------
def test_causality_bit_for_bit(tiny):
    enc = tiny[0]
    ids = draw_ids(TINY_TEXT, 3, 77, seed=21)
    a = enc(ids)[0].clone()
    ids2 = ids.clone()
    ids2[:, 40:] = (ids2[:, 40:] + 1 + draw_ids(TINY_TEXT, 3, 37, seed=22) % (TINY_TEXT.vocab_size - 1)) % TINY_TEXT.vocab_size
    assert (ids2[:, 40:] != ids[:, 40:]).all()
    b = enc(ids2)[0]
    assert torch.equal(a[:, :40], b[:, :40])
    assert (a[:, 40:] != b[:, 40:]).any(dim=-1).all()


# ------------------------------------------------------------------ 5. compute modes ------------------------------------------------
def test_same_bits_in_every_compute_mode(tiny):
    enc = tiny[0]
    ids = draw_ids(TINY_TEXT, 2, 77, seed=31)
    ref = enc(ids)[0].clone()
    try:
        for mode in ("bf16", "fp16"):
            enc.engine.set_compute_dtype(mode)
            assert torch.equal(enc(ids)[0], ref), mode
    finally:
        enc.engine.set_compute_dtype("fp32")
    assert torch.equal(enc(ids)[0], ref)


def test_same_bits_in_an_f32x3_context():
    """E2V_F32X3 is chosen before the weights are finalized: the text part still keeps fp32 matrices only and runs fp32"""
    sd = synth_text(TINY_TEXT)
    ids = draw_ids(TINY_TEXT, 2, 13, seed=32)
    ref = make_encoder(TINY_TEXT, sd)(ids)[0]
    eng = make_engine(TINY_TEXT)
    eng.set_compute_dtype("f32x3")
    enc = make_encoder(TINY_TEXT, sd, engine=eng)
    assert torch.equal(enc(ids)[0], ref)
    assert eng.weight_forms("text.text_model.encoder.layers.0.mlp.fc1.weight") == 1


# ------------------------------------------------------------------ 6. errors -------------------------------------------------------
def test_errors(tiny):
    from eeg2video_amd import _lib
    enc = tiny[0]
    ok = draw_ids(TINY_TEXT, 2, 5, seed=41)
    before = enc(ok)[0].clone()
    for bad in (TINY_TEXT.vocab_size, -1):
        ids = ok.clone()
        ids[1, 3] = bad
        with pytest.raises(ValueError, match="text_vocab_size"):
            enc(ids)
    with pytest.raises(ValueError, match="text_max_positions"):
        enc(torch.zeros((1, TINY_TEXT.max_positions + 1), dtype=torch.long))
    with pytest.raises(NotImplementedError, match="attention_mask"):
        enc(ok, attention_mask=torch.ones_like(ok))
    res = enc(ok)
    (only,) = res                                              # one element, as a tuple: out[1] is an IndexError
    assert only is res.last_hidden_state and res["last_hidden_state"] is only
    with pytest.raises(IndexError):
        res[1]
    with pytest.raises(KeyError):
        res["pooler_output"]
    odd = torch.empty(2 * 5 * TINY_TEXT.hidden + 1, device="cuda")[1:]          # 4 bytes off a 16-byte boundary
    ids_np = np.ascontiguousarray(ok.numpy())
    assert enc.engine.lib.e2v_text_encode(enc.engine.ctx, ids_np.ctypes.data_as(_lib.c_int64_p), 2, 5, odd.data_ptr(), None) == _lib.E2V_EINVAL
    with pytest.raises(ValueError, match="frozen"):
        enc.engine.update_state_dict({"text_model.final_layer_norm.weight": torch.ones(TINY_TEXT.hidden)}, prefix="text.")
    assert torch.equal(enc(ok)[0], before)                     # nothing of the refused calls was enqueued
    fresh = make_engine(TINY_TEXT)                             # text config, nothing loaded
    with pytest.raises(RuntimeError, match="not finalized"):
        fresh.text_encode(ok)
    with pytest.raises(RuntimeError, match="not loaded"):
        fresh.finalize(fresh.TEXT)
    plain = make_engine(None)                                  # no text config
    with pytest.raises(RuntimeError, match="without a text encoder"):
        plain.text_encode(ok)
    ids = np.ascontiguousarray(ok.numpy())
    out = torch.empty(2, 5, TINY_TEXT.hidden, device="cuda")
    assert plain.lib.e2v_text_encode(plain.ctx, ids.ctypes.data_as(_lib.c_int64_p), 2, 5, out.data_ptr(), None) == _lib.E2V_ESTATE
    with pytest.raises(RuntimeError, match="no text encoder"):
        plain.finalize(plain.TEXT)


# ------------------------------------------------------------------ 7. bounds -------------------------------------------------------
@pytest.mark.parametrize("b,t", [(3, 77), (3, 13)])
def test_output_fenced(tiny, b, t):
    enc = tiny[0]
    ids = draw_ids(TINY_TEXT, b, t, seed=51)
    plain = enc(ids)[0].clone()
    out = fenced_out((b, t, TINY_TEXT.hidden))
    y = run_fenced(lambda: enc.engine.text_encode(ids, out=out.t), [], out)
    assert torch.equal(y.view(b, t, -1), plain)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("b,t", [(3, 77), (3, 13)])
def test_op_causal_attention_fenced(tiny, b, t, pad):
    heads = 2
    c = heads * 64
    qkv = torch.from_numpy(counter_normal(61 + t, "qkvf", (b * t, 3 * c)))
    fi, fo = fenced(qkv, ld=3 * c + pad, name="qkv"), fenced_out((b * t, c), ld=c + pad)
    y = run_fenced(lambda: tiny[0].engine.op_causal_attention(fi.t, B=b, T=t, heads=heads, out=fo.t), [fi], fo)
    check(y, causal_attention(qkv, b, t, heads), f"fenced op T={t} pad={pad}")


def test_guarded_pool_and_steady_state(tiny):
    """E2V_POOL_GUARD on: every workspace block of a tiny encode (and the text weights) sits between guard zones; none is altered, and
    the result equals the unguarded one.  A repeated call takes the same number of pool blocks and no new device memory."""
    enc, sd = tiny
    ids = draw_ids(TINY_TEXT, 2, 13, seed=71)
    plain = enc(ids)[0].clone()
    torch.cuda.synchronize()
    eng = enc.engine
    g0, bytes0 = eng.pool_gets(), eng.device_bytes()
    enc(ids)
    g1 = eng.pool_gets()
    enc(ids)
    torch.cuda.synchronize()
    assert eng.pool_gets() - g1 == g1 - g0 > 0 and eng.device_bytes() == bytes0
    with environment({}, GUARD_KIB):
        genc = make_encoder(TINY_TEXT, sd)
        genc.engine.pool_guard_report()
        y = genc(ids)[0]
        checked, violations, text = genc.engine.pool_guard_report()
        assert violations == 0, text
        assert checked >= g1 - g0, (checked, g1 - g0)
        assert not torch.isnan(y).any() and torch.equal(y, plain)


# ------------------------------------------------------------------ 8. the pipeline -------------------------------------------------
PIPE_TEXT = TextConfig(vocab_size=64, hidden=TINY_UNET.cross_attention_dim, heads=1, layers=2, intermediate=128, max_positions=77)


class Tok:
    """a stand-in with the ``transformers`` CLIP tokenizer's call interface: bos, one id per character, eos-padded"""
    model_max_length = 77

    def __call__(self, prompts, padding=None, max_length=None, truncation=None, return_tensors=None):
        ids = torch.full((len(prompts), max_length), 63, dtype=torch.long)
        for i, p in enumerate(prompts):
            body = [62] + [ord(ch) % 60 + 1 for ch in p][:max_length - 2]
            ids[i, :len(body)] = torch.tensor(body, dtype=torch.long)
        return type("Enc", (), {"input_ids": ids, "attention_mask": (ids != 63).long()})()


@pytest.fixture(scope="module")
def sd_dir(tmp_path_factory):
    """a local Stable-Diffusion directory (tiny configs) with unet/, vae/, scheduler/ and text_encoder/"""
    from safetensors.torch import save_file
    root = str(tmp_path_factory.mktemp("sd"))
    t = lambda sd: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}
    usd = t(synth_state_dict(unet_param_spec(TINY_UNET), seed=42, mode="perturbed"))
    vsd = t(synth_state_dict(vae_param_spec(TINY_VAE), seed=43, mode="perturbed"))
    tsd = t(synth_text(PIPE_TEXT, seed=44))
    for sub in ("unet", "vae", "scheduler", "text_encoder"):
        os.makedirs(os.path.join(root, sub))
    dump = lambda obj, *path: json.dump(obj, open(os.path.join(root, *path), "w"))
    dump({"_class_name": "UNet3DConditionModel", "sample_size": TINY_UNET.sample_size, "in_channels": 4, "out_channels": 4,
          "block_out_channels": list(TINY_UNET.block_out_channels), "layers_per_block": 2, "cross_attention_dim": TINY_UNET.cross_attention_dim,
          "attention_head_dim": TINY_UNET.attention_head_dim, "norm_num_groups": 32, "norm_eps": 1e-5}, "unet", "config.json")
    torch.save(usd, os.path.join(root, "unet", "diffusion_pytorch_model.bin"))
    dump({"_class_name": "AutoencoderKL", "in_channels": 3, "out_channels": 3, "latent_channels": 4,
          "block_out_channels": list(TINY_VAE.block_out_channels), "layers_per_block": TINY_VAE.layers_per_block,
          "norm_num_groups": TINY_VAE.norm_num_groups}, "vae", "config.json")
    torch.save(vsd, os.path.join(root, "vae", "diffusion_pytorch_model.bin"))
    dump({"_class_name": "DDIMScheduler", "beta_start": 0.00085, "beta_end": 0.012, "beta_schedule": "scaled_linear",
          "num_train_timesteps": 1000, "set_alpha_to_one": False, "steps_offset": 1, "clip_sample": False}, "scheduler", "scheduler_config.json")
    dump({"architectures": ["CLIPTextModel"], "vocab_size": PIPE_TEXT.vocab_size, "hidden_size": PIPE_TEXT.hidden,
          "num_attention_heads": PIPE_TEXT.heads, "num_hidden_layers": PIPE_TEXT.layers, "intermediate_size": PIPE_TEXT.intermediate,
          "max_position_embeddings": 77, "hidden_act": "quick_gelu", "layer_norm_eps": 1e-5}, "text_encoder", "config.json")
    tsd["text_model.embeddings.position_ids"] = torch.arange(77)[None]
    save_file(tsd, os.path.join(root, "text_encoder", "model.safetensors"))
    return root


def test_text_twin_with_the_native_encoder(sd_dir):
    """``from_pretrained`` on a directory with ``text_encoder/`` builds the library's CLIPTextModel on the pipeline's engine; a ``str``
    list prompt then gives the frames of the twin fed ``engine.text_encode`` of the same ids, the empty prompt being the negative."""
    from eeg2video_amd.pipeline_tuneavideo import TuneAVideoPipeline as TextPipeline
    from eeg2video_amd.text_encoder import CLIPTextModel
    pipe = TextPipeline.from_pretrained(sd_dir, tokenizer=Tok())
    pipe.set_progress_bar_config(disable=True)
    eng = pipe.unet.engine
    assert isinstance(pipe.text_encoder, CLIPTextModel) and pipe.text_encoder.engine is eng and pipe.vae.engine is eng
    assert pipe.text_encoder.tcfg == PIPE_TEXT and not getattr(pipe.text_encoder.config, "use_attention_mask", False)
    f, prompts = 2, ["a panda", "a bear eating"]
    lat = torch.from_numpy(counter_normal(82, "lat", (2, 4, f, 4, 6)))
    kw = dict(video_length=f, height=32, width=48, num_inference_steps=2, guidance_scale=7.5, latents=lat)
    v = pipe(prompts, **kw).videos
    emb = eng.text_encode(Tok()(prompts, max_length=77).input_ids)
    neg = eng.text_encode(Tok()(["", ""], max_length=77).input_ids)
    w = pipe(emb, negative_prompt=neg, **kw).videos
    assert v.shape == (2, 3, f, 32, 48) and torch.equal(v, w)
    assert not torch.equal(v[0], pipe(prompts[::-1], **kw).videos[0])          # the prompt does reach the frames
    # text_encoder=False: no encoder is built, and a str prompt raises what the constructor called with None always raised
    none = TextPipeline.from_pretrained(sd_dir, tokenizer=Tok(), text_encoder=False)
    assert none.text_encoder is None and none.unet.engine.text_cfg is None
    with pytest.raises(ValueError, match="tokenizer"):
        none(prompts, **kw)
    built = TextPipeline(vae=pipe.vae, text_encoder=None, tokenizer=Tok(), unet=pipe.unet, scheduler=pipe.scheduler)
    with pytest.raises(ValueError, match="tokenizer"):
        built(prompts, **kw)


def test_text_twin_around_a_prebuilt_unet(sd_dir):
    """``from_pretrained(dir, unet=hip_unet)`` with ``text_encoder/`` present (every real SD directory has one): a UNet whose engine was
    created without a text config gives the embeddings-only pipeline it always gave -- nothing raises, frames from embeddings as
    before --, and so does one created for ANOTHER text encoder; a UNet created with the directory's text config gets the native
    encoder on its engine."""
    from eeg2video_amd.pipeline import TuneAVideoPipeline as EEGPipeline
    from eeg2video_amd.pipeline_tuneavideo import TuneAVideoPipeline as TextPipeline
    from eeg2video_amd.text_encoder import CLIPTextModel
    from eeg2video_amd.unet import UNet3DConditionModel
    from eeg2video_amd.vae import AutoencoderKL
    vcfg = AutoencoderKL.config_from_dir(os.path.join(sd_dir, "vae"))
    f, prompts = 2, ["a panda", "a bear eating"]
    lat = torch.from_numpy(counter_normal(82, "lat", (2, 4, f, 4, 6)))
    kw = dict(video_length=f, height=32, width=48, num_inference_steps=2, guidance_scale=7.5, latents=lat)
    emb = torch.from_numpy(counter_normal(83, "emb", (2, 77, TINY_UNET.cross_attention_dim)))
    neg = torch.from_numpy(counter_normal(84, "neg", (1, 77, TINY_UNET.cross_attention_dim)))
    for other in (None, dataclasses.replace(PIPE_TEXT, layers=1)):
        unet = UNet3DConditionModel.from_pretrained(sd_dir, subfolder="unet", vae_config=vcfg, text_config=other)
        pipe = TextPipeline.from_pretrained(sd_dir, unet=unet, tokenizer=Tok())
        pipe.set_progress_bar_config(disable=True)
        assert pipe.text_encoder is None and pipe.unet is unet and pipe.vae.engine is unet.engine
        v = pipe(emb, negative_prompt=neg, **kw).videos
        assert v.shape == (2, 3, f, 32, 48) and torch.isfinite(v).all()
        with pytest.raises(ValueError, match="tokenizer"):
            pipe(prompts, **kw)
    unet = UNet3DConditionModel.from_pretrained(sd_dir, subfolder="unet", vae_config=vcfg, text_config=PIPE_TEXT)
    pipe = TextPipeline.from_pretrained(sd_dir, unet=unet, tokenizer=Tok())
    pipe.set_progress_bar_config(disable=True)
    assert isinstance(pipe.text_encoder, CLIPTextModel) and pipe.text_encoder.engine is unet.engine
    assert torch.equal(pipe(emb, negative_prompt=neg, **kw).videos, v)          # the text part changes nothing of the rest
    assert pipe(prompts, **kw).videos.shape == v.shape
    with pytest.raises(ValueError, match="text_config"):
        EEGPipeline.from_pretrained(sd_dir, unet=unet, text_config=PIPE_TEXT)
