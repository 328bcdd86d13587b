"""GPU: weights of a finalized model read back (``e2v_read_tensor``, ``Engine.read_tensor`` / ``state_dict``, the models'
``state_dict`` and ``save_pretrained``) are the tensors that were loaded, or the ones an update wrote.

Every comparison is ``torch.equal``: a read is a copy of stored fp32 bits through the inverse of finalize's row map, an exact widening
of a stored 16-bit copy, the exact sum of the three f32x3 planes, or one round-to-nearest-even cast of those -- which is what
``tensor.to(torch.bfloat16)`` / ``.to(torch.float16)`` compute.  No tolerance anywhere.

One engine holds all four parts (UNet, VAE, Semantic Predictor with its 22-input K-padded first layer, text encoder) in the tiny
configurations of ``eeg2video_amd.weights``, built from ``synth_state_dict(mode="perturbed")``; replacement tensors are drawn as
tests/test_hip_weight_update.py draws them."""
import json
import math
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from eeg2video_amd import _lib
from eeg2video_amd.weights import (TINY_SEMANTIC, TINY_TEXT, TINY_UNET, TINY_VAE, counter_normal, semantic_param_spec,
                                   synth_state_dict, text_param_spec, unet_param_spec, vae_param_spec)

pytestmark = pytest.mark.gpu

BITS = _lib.FORM_BITS
MODES = ["fp32", "bf16", "fp16", "f32x3"]
BLK = "transformer_blocks.0"
D0, M0 = f"down_blocks.0.attentions.0.{BLK}", f"mid_block.attentions.0.{BLK}"
VATT = "vae.decoder.mid_block.attentions.0"
TL0 = "text.text_model.encoder.layers.0.self_attn"

#: one linear weight of each binding flavour
LIN_PLAIN, LIN_SLICE, LIN_GEGLU, LIN_KPAD = "time_embedding.linear_1.weight", f"{M0}.attn1.to_k.weight", f"{M0}.ff.net.0.proj.weight", "semantic.mlp.0.weight"
LIN_KEYS = [LIN_PLAIN, LIN_SLICE, LIN_GEGLU, LIN_KPAD]
CONV_3X3, CONV_4CH, NORM = "down_blocks.2.resnets.1.conv1.weight", "vae.decoder.conv_in.weight", "down_blocks.0.resnets.0.norm1.weight"
#: one key per binding kind: norm affine, plain bias, slice of a fused bias, interleaved bias, the four linear flavours, 3x3 convs
KIND_KEYS = [NORM, "time_embedding.linear_1.bias", f"{VATT}.key.bias", f"{M0}.ff.net.0.proj.bias", f"{VATT}.value.weight",
             f"{D0}.attn2.to_v.weight", f"{D0}.attn_temp.to_q.weight", "semantic.mlp.2.weight", CONV_3X3, CONV_4CH, "conv_out.weight"] + LIN_KEYS


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def draw(key, shape, seed=1042):
    z = counter_normal(seed, key, shape).astype(np.float64)
    if len(shape) > 1:
        return _t((z / math.sqrt(int(np.prod(shape[1:])))).astype(np.float32))
    return _t(((1.0 if key.endswith(".weight") else 0.0) + 0.2 * z).astype(np.float32))


def is_trainable(k):         # train_finetune_videodiffusion.py:47-51
    return ".attn1.to_q." in k or ".attn2.to_q." in k or ".attn_temp." in k


SPECS = OrderedDict([("", unet_param_spec(TINY_UNET)), ("vae.", vae_param_spec(TINY_VAE)),
                     ("semantic.", semantic_param_spec(TINY_SEMANTIC, TINY_UNET.cross_attention_dim)), ("text.", text_param_spec(TINY_TEXT))])
SDS = {p: synth_state_dict(spec, seed=42 + i, mode="perturbed") for i, (p, spec) in enumerate(SPECS.items())}
#: every tensor the engine was given, under the engine's key (the reference: computed once, never written)
LOADED = OrderedDict((p + k, _t(v)) for p, sd in SDS.items() for k, v in sd.items())


class Models:
    def __init__(self, unet_sd=None):
        from eeg2video_amd.engine import Engine
        from eeg2video_amd.semantic import CLIP
        from eeg2video_amd.text_encoder import CLIPTextModel
        from eeg2video_amd.unet import UNet3DConditionModel
        from eeg2video_amd.vae import AutoencoderKL
        c = TINY_UNET
        self.eng = eng = Engine(TINY_UNET, TINY_VAE, 0, sem_cfg=TINY_SEMANTIC, text_cfg=TINY_TEXT)
        self.unet = UNet3DConditionModel(sample_size=c.sample_size, in_channels=c.in_channels, out_channels=c.out_channels,
                                         block_out_channels=c.block_out_channels, layers_per_block=c.layers_per_block,
                                         cross_attention_dim=c.cross_attention_dim, attention_head_dim=c.attention_head_dim,
                                         norm_num_groups=c.norm_num_groups, norm_eps=c.norm_eps, engine=eng)
        self.vae = AutoencoderKL(TINY_VAE, engine=eng)
        self.sem = CLIP(TINY_SEMANTIC, engine=eng)
        self.text = CLIPTextModel(TINY_TEXT, engine=eng)
        self.unet.load_state_dict(unet_sd if unet_sd is not None else SDS[""])
        self.vae.load_state_dict(SDS["vae."])
        self.sem.load_state_dict(SDS["semantic."])
        self.text.load_state_dict(SDS["text."])

    def by_prefix(self):
        return {"": self.unet, "vae.": self.vae, "semantic.": self.sem, "text.": self.text}


_inputs = {}


def inputs():
    if not _inputs:
        d = TINY_UNET.cross_attention_dim
        _inputs.update(x=_t(counter_normal(5, "x", (2, 4, 3, 8, 8))).cuda(), cond=_t(counter_normal(6, "c", (2, 11, d))).cuda(),
                       z=_t(counter_normal(11, "z", (1, 4, 2, 4, 6))).cuda(), img=_t(counter_normal(12, "img", (2, 3, 32, 48))).cuda(),
                       eeg=_t(counter_normal(3, "eeg", (8, TINY_SEMANTIC.in_features))).cuda(),
                       ids=torch.tensor([[1, 5, 9, 100, 127, 3, 0, 2, 2], [127, 64, 8, 8, 1, 0, 31, 77, 2]]),
                       emb=_t(counter_normal(8, "emb", (1, 77, d))).cuda(), neg=_t(counter_normal(9, "neg", (1, 77, d))).cuda(),
                       lat=_t(counter_normal(7, "lat", (1, 4, 2, 8, 8))).cuda())
    return _inputs


def unet_out(unet):
    i = inputs()
    return unet(i["x"], 301, i["cond"], return_dict=False)[0]


def vae_out(vae):
    i = inputs()
    dist = vae.encode(i["img"]).latent_dist
    return torch.cat([vae.decode(i["z"]).sample.flatten(), dist.mean.flatten(), dist.logvar.flatten()])


def build(mode, monkeypatch, warm=False):
    """An engine in `mode`; warm: every part has run once, so the forms a mode builds on first use (the IEEE-half copies) exist."""
    if mode == "f32x3":
        monkeypatch.setenv("E2V_F32X3", "1")
    m = Models()
    if mode in ("bf16", "fp16"):
        m.eng.set_compute_dtype(mode)
    if warm:
        assert all(bool(torch.isfinite(o).all()) for o in (unet_out(m.unet), vae_out(m.vae), m.sem(inputs()["eeg"])))
    return m


def live_forms(eng, key):
    """the readable forms next to fp32: the 16-bit copies and planes of a LINEAR's weight (a 3x3 conv reports its 16-bit kernel
    layouts under the same bits; they have no index-map inverse)"""
    if LOADED[key].dim() == 4 and LOADED[key].shape[2:] == (3, 3):
        return []
    have = eng.weight_forms(key)
    return [n for n in ("bf16", "fp16", "x3") if have & BITS[n]]


def expect_form(w, name):
    return {"fp32": w, "x3": w, "bf16": w.to(torch.bfloat16).float(), "fp16": w.to(torch.float16).float()}[name]


# ---- 1. round trip of every key ------------------------------------------------------------------------------------------------------
def test_the_key_set_covers_every_re_layout():
    keys = list(LOADED)
    for a in ("attn1", "attn2", "attn_temp"):
        for p in ("to_q", "to_k", "to_v"):
            assert f"{D0}.{a}.{p}.weight" in keys
    assert f"{D0}.ff.net.0.proj.weight" in keys and f"{D0}.ff.net.0.proj.bias" in keys
    for p in ("query", "key", "value"):
        assert f"{VATT}.{p}.weight" in keys and f"{VATT}.{p}.bias" in keys
    for p in ("q_proj", "k_proj", "v_proj"):
        assert f"{TL0}.{p}.weight" in keys and f"{TL0}.{p}.bias" in keys
    assert LOADED[CONV_4CH].shape[1:] == (4, 3, 3) and LOADED[CONV_3X3].shape[2:] == (3, 3) and LOADED[NORM].dim() == 1
    assert LOADED[LIN_KPAD].shape[1] == 22 and LOADED[LIN_KPAD].shape[1] % 8 != 0
    assert set(KIND_KEYS) <= set(keys)


@pytest.mark.parametrize("mode", MODES)
def test_every_key_reads_back_as_loaded(mode, monkeypatch):
    m = build(mode, monkeypatch)
    assert list(m.eng.expected_keys()) and set(m.eng.expected_keys()) == set(LOADED)
    if mode == "f32x3":
        assert m.eng.weight_forms(LIN_SLICE) & BITS["x3"]
    for k, w in LOADED.items():
        got = m.eng.read_tensor(k)
        assert got.dtype == torch.float32 and got.shape == w.shape and got.is_cuda, k
        assert torch.equal(got.cpu(), w), k
    for prefix, model in m.by_prefix().items():
        sd = model.state_dict()
        assert list(sd) == list(SPECS[prefix]) == list(model.state_dict_spec()), prefix
        for k, v in sd.items():
            assert tuple(v.shape) == tuple(SPECS[prefix][k]) and v.dtype == torch.float32 and v.is_cuda, k
            assert torch.equal(v.cpu(), LOADED[prefix + k]), k
    host = m.sem.state_dict(device="cpu")
    assert all(not v.is_cuda and torch.equal(v, LOADED["semantic." + k]) for k, v in host.items()) and list(host) == list(SPECS["semantic."])


def test_a_torch_module_loads_the_state_dict():
    """``torch_module.load_state_dict(hip_model.state_dict())`` for a module with the reference's key names
    (train_semantic_predictor.py:11-32: ``self.mlp = nn.Sequential(Linear, ReLU, ...)``)"""
    from torch import nn
    c, d = TINY_SEMANTIC, TINY_UNET.cross_attention_dim

    class Predictor(nn.Module):
        def __init__(self):
            super().__init__()
            widths = [c.in_features, c.hidden, c.hidden, c.hidden, c.hidden, c.tokens * d]
            layers = []
            for i in range(5):
                layers += [nn.Linear(widths[i], widths[i + 1]), nn.ReLU()]
            self.mlp = nn.Sequential(*layers[:-1])
    m = Models()
    mod = Predictor()
    mod.load_state_dict(m.sem.state_dict())                       # strict
    assert all(torch.equal(v, LOADED["semantic." + k]) for k, v in mod.state_dict().items())


# ---- 2. forms ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_every_live_form_of_a_linear(mode, monkeypatch):
    m = build(mode, monkeypatch, warm=True)
    eng = m.eng
    assert "bf16" in live_forms(eng, LIN_SLICE) or mode == "f32x3"
    if mode == "fp16":
        assert "fp16" in live_forms(eng, LIN_SLICE)
    if mode == "f32x3":
        assert all("x3" in live_forms(eng, k) for k in LIN_KEYS)
    for k in LIN_KEYS:
        w = LOADED[k]
        assert torch.equal(eng.read_tensor(k, form="fp32").cpu(), w), k
        live = live_forms(eng, k)
        for name in live:
            assert torch.equal(eng.read_tensor(k, form=name).cpu(), expect_form(w, name)), (k, name)
        for name in ("bf16", "fp16", "x3"):
            if name not in live:
                with pytest.raises(RuntimeError, match="form not built"):
                    eng.read_tensor(k, form=name)
    # the text tower keeps fp32 matrices only, in every mode
    assert live_forms(eng, f"{TL0}.k_proj.weight") == []
    with pytest.raises(RuntimeError, match="form not built"):
        eng.read_tensor(f"{TL0}.k_proj.weight", form="bf16")
    with pytest.raises(ValueError):
        eng.read_tensor(CONV_3X3, form="bf16")
    with pytest.raises(ValueError):
        eng.read_tensor(NORM, form="x3")


# ---- 3. output types -----------------------------------------------------------------------------------------------------------------
def test_output_types_are_one_rounding_of_the_fp32_read():
    m = Models()
    for k, w in LOADED.items():
        for dt in (torch.bfloat16, torch.float16):
            got = m.eng.read_tensor(k, dtype=dt)
            assert got.dtype == dt and got.shape == w.shape, k
            assert torch.equal(got, m.eng.read_tensor(k).to(dt)), (k, dt)
            assert torch.equal(got.cpu(), w.to(dt)), (k, dt)
    m.eng.set_compute_dtype("bf16")
    for k in LIN_KEYS:             # a stored bf16 copy into an fp16 result: widened exactly, then rounded once
        assert torch.equal(m.eng.read_tensor(k, form="bf16", dtype=torch.float16).cpu(), LOADED[k].to(torch.bfloat16).float().to(torch.float16)), k


# ---- 4. after an update --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp16", "f32x3"])
def test_reads_follow_updates(mode, monkeypatch):
    m = build(mode, monkeypatch, warm=True)
    eng = m.eng
    # neighbours of the updated tensors inside the same fused matrices and biases, and tensors of their own
    untouched = [f"{M0}.attn1.to_q.weight", f"{M0}.attn1.to_v.weight", f"{VATT}.query.weight", f"{VATT}.query.bias", f"{VATT}.value.bias",
                 f"{D0}.attn2.to_k.weight", "semantic.mlp.4.bias", "conv_in.weight", f"{M0}.ff.net.2.weight"]
    assert not set(untouched) & set(KIND_KEYS)
    forms = {k: live_forms(eng, k) for k in KIND_KEYS}
    assert any(forms[k] for k in LIN_KEYS)
    for seed, on_device in ((1042, False), (2042, True)):
        new = {k: draw(k, LOADED[k].shape, seed) for k in KIND_KEYS}
        assert all(not torch.equal(new[k], LOADED[k]) for k in KIND_KEYS)
        eng.update_state_dict({k: (v.cuda() if on_device else v) for k, v in new.items()})
        for k in KIND_KEYS:
            assert live_forms(eng, k) == forms[k], k
            assert torch.equal(eng.read_tensor(k).cpu(), new[k]), (k, on_device)
            for name in forms[k]:
                assert torch.equal(eng.read_tensor(k, form=name).cpu(), expect_form(new[k], name)), (k, name, on_device)
        for k in untouched:
            assert torch.equal(eng.read_tensor(k).cpu(), LOADED[k]), k
            for name in live_forms(eng, k):
                assert torch.equal(eng.read_tensor(k, form=name).cpu(), expect_form(LOADED[k], name)), (k, name)


# ---- 5. stream order, device destinations ------------------------------------------------------------------------------------------
def test_reads_are_stream_ordered_and_allocate_nothing():
    m = Models()
    eng = m.eng
    keys = [LIN_SLICE, LIN_GEGLU, LIN_KPAD, CONV_3X3, NORM, f"{M0}.ff.net.0.proj.bias"]
    new = {k: draw(k, LOADED[k].shape).cuda() for k in keys}
    first = {k: torch.empty_like(new[k]) for k in keys}
    second = {k: torch.empty_like(new[k]) for k in keys}
    eng.update_state_dict({k: LOADED[k].cuda() for k in keys})        # warm-up: nothing of the sequence below is a first call
    eng.read_tensor(keys[0], out=first[keys[0]])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        before = eng.device_bytes()
        for k in keys:                       # read -> update -> read, nothing in between
            eng.read_tensor(k, out=first[k])
            eng.update_state_dict({k: new[k]})
            eng.read_tensor(k, out=second[k])
        for _ in range(20):
            eng.read_tensor(LIN_GEGLU, out=second[LIN_GEGLU])
            eng.read_tensor(LIN_KPAD, dtype=torch.bfloat16)
        after = eng.device_bytes()
    side.synchronize()
    assert before == after
    for k in keys:
        assert torch.equal(first[k].cpu(), LOADED[k]), k
        assert torch.equal(second[k], new[k]), k
    # host destinations: the staging block is cached by the first read of a size
    host = torch.empty(LOADED[CONV_3X3].shape)
    eng.read_tensor(CONV_3X3, out=host)
    assert torch.equal(host, new[CONV_3X3].cpu())
    cached = eng.device_bytes()
    for _ in range(5):
        host.zero_()
        eng.read_tensor(CONV_3X3, out=host)
        assert torch.equal(host, new[CONV_3X3].cpu())
    assert eng.device_bytes() == cached
    h16 = torch.empty(LOADED[LIN_KPAD].shape, dtype=torch.float16)
    assert torch.equal(eng.read_tensor(LIN_KPAD, dtype=torch.float16, out=h16), new[LIN_KPAD].cpu().to(torch.float16))


# ---- 6. nothing outside the tensor -----------------------------------------------------------------------------------------------
_fenced = {}          # one engine for the cases below: they only read


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("key", [LIN_KPAD, CONV_4CH, LIN_SLICE, LIN_GEGLU, f"{M0}.ff.net.0.proj.bias"])
def test_nothing_is_written_outside_the_tensor(key, dtype):
    if "m" not in _fenced:
        _fenced["m"] = Models()
    m = _fenced["m"]
    w = LOADED[key]
    n, per16 = w.numel(), 16 // torch.empty(0, dtype=dtype).element_size()
    for off in (0, 1, 3):
        big = torch.full((n + 4 * per16 + 64,), -7.0, dtype=dtype, device="cuda")
        assert big.data_ptr() % 16 == 0
        start = 2 * per16 + off
        assert (big.data_ptr() + start * big.element_size()) % 16 == off * big.element_size()
        out = big[start:start + n].view(w.shape)
        got = m.eng.read_tensor(key, dtype=dtype, out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        assert torch.equal(big[start:start + n].cpu().view(w.shape), w.to(dtype)), (key, off)
        assert bool((big[:start] == -7.0).all()) and bool((big[start + n:] == -7.0).all()), (key, off)


# ---- 7. save_pretrained --------------------------------------------------------------------------------------------------------------
def _file_state_dict(path, safe, st_name="diffusion_pytorch_model.safetensors", bin_name="diffusion_pytorch_model.bin"):
    assert os.path.isfile(os.path.join(path, st_name)) == safe and os.path.isfile(os.path.join(path, bin_name)) == (not safe)
    if safe:
        from safetensors.torch import load_file
        return load_file(os.path.join(path, st_name))
    return torch.load(os.path.join(path, bin_name), map_location="cpu", weights_only=True)


def _check_file(path, prefix, safe, **names):
    sd = _file_state_dict(path, safe, **names)
    assert set(sd) == set(SPECS[prefix])
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(SPECS[prefix][k]) and v.dtype == torch.float32 and torch.equal(v, LOADED[prefix + k]), k
    with open(os.path.join(path, "config.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("safe", [True, False])
def test_models_save_and_load_again(safe, tmp_path):
    from eeg2video_amd.semantic import CLIP
    from eeg2video_amd.text_encoder import CLIPTextModel
    from eeg2video_amd.unet import UNet3DConditionModel
    from eeg2video_amd.vae import AutoencoderKL
    m = Models()
    i = inputs()
    d = {n: str(tmp_path / n) for n in ("unet", "vae", "text", "sem")}
    m.unet.save_pretrained(d["unet"], safe_serialization=safe)
    assert _check_file(d["unet"], "", safe)["_class_name"] == "UNet3DConditionModel"
    again = UNet3DConditionModel.from_pretrained(d["unet"], vae_config=TINY_VAE)
    assert again.engine is not m.eng and torch.equal(unet_out(again), unet_out(m.unet))

    m.vae.save_pretrained(d["vae"], safe_serialization=safe)
    assert _check_file(d["vae"], "vae.", safe)["_class_name"] == "AutoencoderKL"
    again = AutoencoderKL.from_pretrained(d["vae"], unet_config=TINY_UNET)
    assert again.engine is not m.eng and torch.equal(vae_out(again), vae_out(m.vae))

    m.text.save_pretrained(d["text"], safe_serialization=safe)
    cj = _check_file(d["text"], "text.", safe, st_name="model.safetensors", bin_name="pytorch_model.bin")
    assert cj["_class_name"] == "CLIPTextModel"
    again = CLIPTextModel.from_pretrained(d["text"], subfolder=None)
    assert again.engine is not m.eng and torch.equal(again(i["ids"])[0], m.text(i["ids"])[0])

    m.sem.save_pretrained(d["sem"], safe_serialization=safe)
    _check_file(d["sem"], "semantic.", safe)
    again = CLIP.from_pretrained(d["sem"], engine=Models().eng)
    assert torch.equal(again(i["eeg"]), m.sem(i["eeg"]))


def test_pipeline_saves_what_the_device_holds(tmp_path):
    """The validation pipeline of train_finetune_videodiffusion.py:343-362 after training moved the trainable subset: what
    ``save_pretrained`` writes is what the device holds, so the pipeline loaded from the directory renders the same frames."""
    from eeg2video_amd.pipeline_tuneavideo import TuneAVideoPipeline
    from eeg2video_amd.scheduler import DDIMScheduler
    m = Models()
    i = inputs()
    pipe = TuneAVideoPipeline(vae=m.vae, text_encoder=m.text, tokenizer=None, unet=m.unet, scheduler=DDIMScheduler(engine=m.eng))
    pipe.set_progress_bar_config(disable=True)

    def frames(p):
        out = p(i["emb"], video_length=2, height=64, width=64, num_inference_steps=2, guidance_scale=7.5, negative_prompt=i["neg"],
                latents=i["lat"]).videos
        assert p.last_loop == "ddim" and bool(torch.isfinite(out).all())
        return out
    before = frames(pipe)
    trained = {k: draw(k, v.shape).cuda() for k, v in LOADED.items() if is_trainable(k) and k in SPECS[""]}
    assert len(trained) == 16 * 7          # per transformer block: attn1.to_q, attn2.to_q, attn_temp.{to_q, to_k, to_v, to_out.0.{weight, bias}}
    pipe.unet.sync_from(trained)
    after = frames(pipe)
    assert not torch.equal(after, before)
    root = str(tmp_path / "pipe")
    pipe.save_pretrained(root)
    with open(os.path.join(root, "model_index.json")) as f:
        index = json.load(f)
    assert index["_class_name"] == "TuneAVideoPipeline" and index["scheduler"][1] == "DDIMScheduler"
    assert index["unet"][1] == "UNet3DConditionModel" and index["vae"][1] == "AutoencoderKL" and index["text_encoder"][1] == "CLIPTextModel"
    for sub, name in (("unet", "diffusion_pytorch_model.safetensors"), ("vae", "diffusion_pytorch_model.safetensors"),
                      ("text_encoder", "model.safetensors"), ("scheduler", "scheduler_config.json")):
        assert os.path.isfile(os.path.join(root, sub, name)), sub
    assert not os.path.exists(os.path.join(root, "tokenizer"))
    with open(os.path.join(root, "scheduler", "scheduler_config.json")) as f:
        sched = json.load(f)
    assert sched["_class_name"] == "DDIMScheduler" and {k: sched[k] for k in pipe.scheduler.config} == dict(pipe.scheduler.config)
    loaded = TuneAVideoPipeline.from_pretrained(root)
    loaded.set_progress_bar_config(disable=True)
    assert loaded.unet.engine is not m.eng and loaded.text_encoder is not None and loaded.text_encoder.engine is loaded.unet.engine
    assert torch.equal(frames(loaded), after)
    assert torch.equal(loaded.text_encoder(i["ids"])[0], m.text(i["ids"])[0])
    sd = loaded.unet.state_dict()
    assert all(torch.equal(sd[k], trained[k]) for k in trained)
