"""CPU: the CLIP text encoder's host side -- config fields and key scheme of a host-only context, the argument checks that need no
GPU -- and the reference chain of the GPU tests: ``transformers`` -> ``tests/golden/clip_text_tiny.npz`` -> the plain-torch
restatement (``tests/clip_text_restatement.py``) that covers the shapes the fixture does not."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import torch

from clip_text_restatement import clip_text_forward, rel_err
from eeg2video_amd import _lib
from eeg2video_amd.weights import (TINY_TEXT, SemanticConfig, TextConfig, UNetConfig, VAEConfig, semantic_param_spec, text_param_spec,
                                   unet_param_spec, vae_param_spec)

BOUND = 1e-5        # max |a-b| / max |b|, as test_semantic_predictor_vs_oracle


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "clip_text_tiny.npz"))
    return {k: z[k] for k in z.files}


def host_ctx(lib, text_cfg=None, **fields):
    from eeg2video_amd.engine import fill_text_config
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    if text_cfg is not None:
        fill_text_config(cfg, text_cfg)
    for k, v in fields.items():
        setattr(cfg, k, v)
    ctx = C.c_void_p()
    return lib.e2v_create(C.byref(cfg), -1, C.byref(ctx)), ctx


def key_scheme(lib, ctx):
    shape, nd, got = (C.c_int64 * 4)(), C.c_int(), {}
    for i in range(lib.e2v_num_expected_keys(ctx)):
        k = lib.e2v_expected_key(ctx, i, shape, C.byref(nd)).decode()
        got[k] = tuple(shape[d] for d in range(nd.value))
    return got


def old_scheme():
    want = dict(unet_param_spec(UNetConfig()))
    want.update({"vae." + k: v for k, v in vae_param_spec(VAEConfig()).items()})
    want.update({"semantic." + k: v for k, v in semantic_param_spec(SemanticConfig(), 768).items()})
    return want


def test_default_config_has_no_text_encoder_and_the_old_key_scheme(lib):
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    assert [getattr(cfg, f) for f in ("text_vocab_size", "text_hidden", "text_heads", "text_layers", "text_intermediate",
                                      "text_max_positions", "text_act")] == [0] * 7 and cfg.text_norm_eps == 0.0
    st, ctx = host_ctx(lib)
    assert st == 0
    got = key_scheme(lib, ctx)
    lib.e2v_destroy(ctx)
    assert got == old_scheme() and len(got) == 798 + 248 + 10 and not any(k.startswith("text.") for k in got)


def test_key_scheme_with_a_text_config_is_the_old_one_plus_the_text_spec(lib):
    st, ctx = host_ctx(lib, TINY_TEXT)
    assert st == 0
    got = key_scheme(lib, ctx)
    lib.e2v_destroy(ctx)
    want = old_scheme()
    want.update({"text." + k: v for k, v in text_param_spec(TINY_TEXT).items()})
    assert got == want and len(got) == 798 + 248 + 10 + len(text_param_spec(TINY_TEXT))


def test_sd_v1_4_text_spec_is_the_checkpoints():
    """196 tensors: 2 tables, 12 layers of 16, the final LayerNorm -- the ``text_encoder`` state dict without ``position_ids``."""
    spec = text_param_spec(TextConfig())
    assert len(spec) == 2 + 12 * 16 + 2
    assert spec["text_model.embeddings.token_embedding.weight"] == (49408, 768)
    assert spec["text_model.embeddings.position_embedding.weight"] == (77, 768)
    assert spec["text_model.encoder.layers.11.mlp.fc1.weight"] == (3072, 768) and spec["text_model.encoder.layers.0.mlp.fc2.bias"] == (768,)
    assert spec["text_model.final_layer_norm.weight"] == (768,)


def test_text_encode_on_a_host_only_context_is_a_state_error(lib):
    for text_cfg in (TINY_TEXT, None):
        st, ctx = host_ctx(lib, text_cfg)
        assert st == 0
        ids = np.zeros((1, 4), np.int64)
        out = np.zeros((1, 4, 128), np.float32)
        assert lib.e2v_text_encode(ctx, ids.ctypes.data_as(_lib.c_int64_p), 1, 4, out.ctypes.data_as(C.c_void_p), None) == _lib.E2V_ESTATE
        assert b"host-only" in lib.e2v_last_error(ctx)
        assert lib.e2v_finalize_weights(ctx, 8) == _lib.E2V_ESTATE
        lib.e2v_destroy(ctx)
    assert lib.e2v_text_encode(None, None, 1, 4, None, None) == _lib.E2V_EINVAL


def test_create_validates_the_text_fields(lib):
    st, ctx = host_ctx(lib, TINY_TEXT, text_heads=3)
    assert st == _lib.E2V_EINVAL and b"64 * text_heads" in lib.e2v_last_error(None)
    st, ctx = host_ctx(lib, dataclasses.replace(TINY_TEXT, hidden=1344, heads=21))          # 64 * 21: past the LayerNorm limit
    assert st == _lib.E2V_EINVAL and b"1280" in lib.e2v_last_error(None)
    st, ctx = host_ctx(lib, TINY_TEXT, text_max_positions=129)
    assert st == _lib.E2V_EINVAL and b"128" in lib.e2v_last_error(None)
    st, ctx = host_ctx(lib, TINY_TEXT, text_act=2)
    assert st == _lib.E2V_EINVAL
    for ok in (TINY_TEXT, TextConfig(), dataclasses.replace(TINY_TEXT, max_positions=128, hidden_act="gelu")):
        st, ctx = host_ctx(lib, ok)
        assert st == 0
        lib.e2v_destroy(ctx)


def test_text_weights_are_frozen_for_update_tensor(lib):
    st, ctx = host_ctx(lib, TINY_TEXT)
    w = np.zeros((128,), np.float32)
    shape = (C.c_int64 * 1)(128)
    key = b"text.text_model.final_layer_norm.weight"
    assert lib.e2v_update_tensor(ctx, key, w.ctypes.data_as(C.c_void_p), _lib.E2V_F32, 0, shape, 1, None) == _lib.E2V_EINVAL
    assert b"frozen" in lib.e2v_last_error(ctx)
    lib.e2v_destroy(ctx)


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_restatement_vs_transformers_fixture(fixture, act):
    sd = {k: v for k, v in fixture.items() if k.startswith("text_model.")}
    assert set(sd) == set(text_param_spec(TINY_TEXT)) and all(v.dtype == np.float16 for v in sd.values())
    ids = fixture["input_ids"]
    assert ids.shape == (3, 77) and ids.dtype == np.int64 and (ids[0, 12:] == ids[0, -1]).all()
    out = clip_text_forward(sd, ids, dataclasses.replace(TINY_TEXT, hidden_act=act))
    ref = fixture["out_" + act]
    err = rel_err(out, ref)
    print(f"restatement vs transformers {fixture['transformers_version']} ({act}): {err:.3e}")
    assert ref.shape == (3, 77, 128) and ref.dtype == np.float32 and err < BOUND, err


def test_restatement_is_causal_and_sees_the_activation(fixture):
    """the restatement's own sanity: rows in front of a changed token do not move, and the two activations give different outputs"""
    sd = {k: v for k, v in fixture.items() if k.startswith("text_model.")}
    ids = fixture["input_ids"].copy()
    a = clip_text_forward(sd, ids, TINY_TEXT)
    ids[:, 40:] = (ids[:, 40:] + 1) % TINY_TEXT.vocab_size
    b = clip_text_forward(sd, ids, TINY_TEXT)
    assert torch.equal(a[:, :40], b[:, :40]) and not torch.equal(a[:, 40:], b[:, 40:])
    assert rel_err(fixture["out_gelu"], fixture["out_quick_gelu"]) > 1e-2


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_transformers_regenerates_the_fixture(fixture, act):
    pytest.importorskip("transformers")
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    try:
        from make_text_golden import run_transformers
    finally:
        sys.path.pop(0)
    sd = {k: v for k, v in fixture.items() if k.startswith("text_model.")}
    err = rel_err(run_transformers(sd, fixture["input_ids"], act), fixture["out_" + act])
    print(f"transformers here vs the committed outputs ({act}): {err:.3e}")
    assert err < BOUND, err
