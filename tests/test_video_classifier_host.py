"""CPU: the video classifier's host side -- the crop-window tables against Pillow, the float64 restatement against the
``transformers`` fixture (``tests/golden/videomae_tiny.npz``), config fields / key scheme / argument checks of a host-only context, the
two spellings of the checkpoint, and ``video_classify_metric``'s trial bookkeeping against the reference's loop.

Tolerances, measured on the CPU without the code under test (``test_restatement_vs_transformers_fixture`` and
``test_fp32_attention_distance_from_float64`` print them again):
  * the fixture's fp32 ``transformers`` logits sit 4.6e-7 (max |a-b| / max |b|) from the float64 restatement, its softmax 4.9e-7
    (absolute); the device bounds are ten times that: LOGIT_BOUND 4.6e-6, PROB_BOUND 4.9e-6;
  * an fp32 torch-CPU ``softmax(q k^T / 8) v`` sits 9.8e-7 from float64 at T = 1568; ATTN_BOUND 9.8e-6.
Here the restatement itself must be within the bound of the fixture, so that the device, held to the same bound of the fixture, is
never asked for more than the reference's own error allows.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from eeg2video_amd import _lib
from eeg2video_amd.engine import fill_video_config, image_resize_table
from eeg2video_amd.weights import (TINY_IMAGE, TINY_VIDEO, VIDEO_POSITION_KEY, SemanticConfig, UNetConfig, VAEConfig, VideoConfig,
                                   counter_normal, semantic_param_spec, unet_param_spec, vae_param_spec, video_checkpoint_key,
                                   video_checkpoint_rename, video_checkpoint_spec, video_engine_shape, video_param_spec,
                                   video_position_table)
from test_image_classifier_host import reference_n_way_top_k_acc
from videomae_restatement import (GROUPS, crop_geometry, load_golden, pillow_resize_crop, pixel_table, position_table64, rel_err,
                                  resize_crop_with_tables, softmax64, top3, tubelet_rows, videomae_forward)

LOGIT_BOUND = 4.6e-6       # 10 x 4.6e-7, the fixture's distance from the float64 restatement
PROB_BOUND = 4.9e-6        # 10 x 4.9e-7, likewise for the softmax (absolute)
ATTN_BOUND = 9.8e-6        # 10 x 9.8e-7, fp32 torch-CPU attention against float64 at T = 1568


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def host_ctx(lib, video_cfg=None, **fields):
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    if video_cfg is not None:
        fill_video_config(cfg, video_cfg)
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


# ---- crop-window tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,edge", [(288, 512, 224), (36, 64, 32), (90, 50, 32), (45, 77, 32), (32, 32, 32), (36, 64, 56), (90, 50, 56)])
def test_crop_window_tables_equal_pillow_bit_for_bit(h, w, edge):
    """the window of the two-pass resize from ``e2v_image_resize_table`` against ``PIL.Image.resize((nw, nh), BILINEAR)`` + the crop:
    the production shape, a wide and a tall source (odd crop remainder), one whose long side rounds down, and a frame that is its own
    resize -- at the sizes of the issue and of the fixture"""
    pytest.importorskip("PIL")
    img = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    got, want = resize_crop_with_tables(img, edge, edge, image_resize_table), pillow_resize_crop(img, edge, edge)
    assert got.shape == want.shape == (edge, edge, 3) and np.array_equal(got, want), int((got != want).sum())


def test_crop_geometry_is_the_processors():
    assert crop_geometry(288, 512, 224, 224) == (224, 398, 0, 87)                 # columns 87 .. 310
    assert crop_geometry(36, 64, 56, 56) == (56, 99, 0, 21)
    assert crop_geometry(90, 50, 56, 56) == (100, 56, 22, 0)
    assert crop_geometry(90, 50, 32, 32) == (57, 32, 12, 0)                       # 25 rows left over: 12 above, 13 below
    assert crop_geometry(56, 56, 56, 56) == (56, 56, 0, 0)


def test_fixture_cropped_bytes_are_reproduced(golden):
    z, _ = golden
    c = TINY_VIDEO
    assert str(z["pillow_version"]) and str(z["transformers_version"])
    for g in GROUPS[:2]:
        for clip, want in zip(z["clips_" + g], z["cropped_" + g]):
            for f in (0, 5):
                assert np.array_equal(resize_crop_with_tables(clip[f], c.resize_edge, c.image_size, image_resize_table), want[f])
    assert z["clips_36x64"].shape == (4, 6, 36, 64, 3) and z["clips_90x50"].shape == (2, 6, 90, 50, 3) and z["clips_56x56"].shape == (2, 6, 56, 56, 3)
    assert np.array_equal(pixel_table(c.rescale_factor, c.image_mean, c.image_std), z["pixel_table"])     # the processor's own table


# ---- restatement -----------------------------------------------------------------------------------------------------------------
def fixture_rows(z):
    rows = []
    for g in GROUPS:
        for i, clip in enumerate(z["clips_" + g]):
            cropped = z["cropped_" + g][i] if "cropped_" + g in z.files else clip
            rows.append(tubelet_rows(cropped, z["pixel_table"], TINY_VIDEO.patch_size, TINY_VIDEO.tubelet_size))
    return np.stack(rows)


def test_restatement_vs_transformers_fixture(golden):
    z, sd = golden
    c = TINY_VIDEO
    assert {k: v.shape for k, v in sd.items()} == dict(video_checkpoint_spec(c)) and all(z["w." + k].dtype == np.float16 for k in sd)
    logits = videomae_forward(sd, fixture_rows(z), video_position_table(c.tokens, c.hidden), c.heads, c.layer_norm_eps)
    err = rel_err(logits, z["logits"])
    perr = float(np.abs(softmax64(logits) - z["probs"]).max())
    print(f"float64 restatement vs transformers {z['transformers_version']} fp32: logits {err:.3e} (device bound {LOGIT_BOUND:.1e}), "
          f"softmax {perr:.3e} (device bound {PROB_BOUND:.1e})")
    assert z["logits"].shape == (8, 50) and z["logits"].dtype == np.float32 and err < LOGIT_BOUND and perr < PROB_BOUND, (err, perr)
    assert LOGIT_BOUND <= 10.5 * err and PROB_BOUND <= 10.5 * perr          # the bounds are ten times this distance, not more
    srt = np.sort(z["logits"], -1)
    assert ((srt[:, -3] - srt[:, -4]) > 1e-3 * np.abs(z["logits"]).max(-1)).all()        # the fixture's own promise
    assert np.array_equal(top3(logits), top3(z["logits"]))


def test_fixture_has_no_class_token_position_table_or_final_layernorm(golden):
    z, sd = golden
    assert "videomae.layernorm.weight" not in sd and "fc_norm.weight" in sd
    assert not any("cls_token" in k or "position" in k for k in sd)


def test_fp32_attention_distance_from_float64():
    b, heads, t = 2, 2, 1568
    qkv = torch.from_numpy(counter_normal(70 + t, "vmae_qkv", (b * t, 3 * 64 * heads))) * torch.tensor([1.5, 1.5, 1.0]).repeat_interleave(64 * heads)

    def ref(x):
        q, k, v = (y.view(b, t, heads, 64).transpose(1, 2) for y in x.chunk(3, dim=-1))
        return (torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v).transpose(1, 2).reshape(b * t, heads * 64)
    err = rel_err(ref(qkv), ref(qkv.double()))
    print(f"fp32 torch-CPU attention vs float64 at T = {t}: {err:.3e} (device bound {ATTN_BOUND:.1e})")
    assert err < ATTN_BOUND


def test_position_table_is_the_sinusoid():
    c = TINY_VIDEO
    tab = video_position_table(c.tokens, c.hidden)
    assert tab.shape == (147, 128) and tab.dtype == np.float32
    assert np.abs(tab - position_table64(c.tokens, c.hidden)).max() < 1e-7
    assert (tab[0, 0::2] == 0).all() and (tab[0, 1::2] == 1).all()
    assert video_position_table(588, 768).shape == (588, 768) and VideoConfig().tokens == 588 and VideoConfig(num_frames=16).tokens == 1568
    transformers = pytest.importorskip("transformers")
    from transformers.models.videomae.modeling_videomae import get_sinusoid_encoding_table
    assert np.array_equal(get_sinusoid_encoding_table(c.tokens, c.hidden)[0].numpy(), tab)      # transformers' own bits


# ---- keys and ABI ----------------------------------------------------------------------------------------------------------------
VMAE_INTS = ("vmae_hidden", "vmae_heads", "vmae_layers", "vmae_intermediate", "vmae_image_size", "vmae_patch_size", "vmae_tubelet_size",
             "vmae_num_frames", "vmae_num_labels", "vmae_resize_edge")


def test_default_config_has_no_video_classifier(lib):
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    assert [getattr(cfg, f) for f in VMAE_INTS] == [0] * len(VMAE_INTS)
    assert cfg.vmae_norm_eps == 0.0 and cfg.vmae_rescale == 0.0 and list(cfg.vmae_mean) == [0.0] * 3 and list(cfg.vmae_std) == [0.0] * 3
    names = [f[0] for f in _lib.E2VConfig._fields_]
    assert names[-14:] == ["vmae_hidden", "vmae_heads", "vmae_layers", "vmae_intermediate", "vmae_image_size", "vmae_patch_size",
                           "vmae_tubelet_size", "vmae_num_frames", "vmae_num_labels", "vmae_norm_eps", "vmae_resize_edge", "vmae_rescale",
                           "vmae_mean", "vmae_std"] and names[-15] == "vit_std"                  # appended after the vit_* fields
    st, ctx = host_ctx(lib)
    assert st == 0
    got = key_scheme(lib, ctx)
    frames = np.zeros((1, 6, 8, 8, 3), np.uint8)
    out = np.zeros((1, 50), np.float32)
    st = lib.e2v_video_classify(ctx, frames.ctypes.data_as(C.c_void_p), 3, 1, 6, 8, 8, out.ctypes.data_as(C.c_void_p), None, None, None)
    assert st == _lib.E2V_ESTATE and b"no video classifier" in lib.e2v_last_error(ctx)
    assert lib.e2v_finalize_weights(ctx, 32) == _lib.E2V_ESTATE
    lib.e2v_destroy(ctx)
    assert got == old_scheme() and not any(k.startswith("video.") for k in got)


def test_key_scheme_with_a_video_config_is_the_old_one_plus_the_video_spec(lib):
    st, ctx = host_ctx(lib, TINY_VIDEO)
    assert st == 0
    got = key_scheme(lib, ctx)
    lib.e2v_destroy(ctx)
    want = old_scheme()
    want.update({"video." + k: v for k, v in video_param_spec(TINY_VIDEO).items()})
    assert got == want and len(got) == 798 + 248 + 10 + len(video_param_spec(TINY_VIDEO))
    assert [k for k in got if k.startswith("video.")] == ["video." + k for k in video_param_spec(TINY_VIDEO)]      # and in its order
    assert got["video." + VIDEO_POSITION_KEY] == (147, 128)


def test_videomae_base_spec_is_transformers():
    """196 tensors of the state dict: 2 of the embedding, 12 layers of 16, fc_norm, the classifier; plus the position table"""
    spec, ck = video_param_spec(VideoConfig()), video_checkpoint_spec(VideoConfig())
    assert len(ck) == 2 + 12 * 16 + 2 + 2 and len(spec) == len(ck) + 1 and list(spec)[0] == VIDEO_POSITION_KEY
    assert ck["videomae.embeddings.patch_embeddings.projection.weight"] == (768, 3, 2, 16, 16)
    assert spec["videomae.embeddings.patch_embeddings.projection.weight"] == (768, 6, 16, 16) == video_engine_shape((768, 3, 2, 16, 16))
    assert spec[VIDEO_POSITION_KEY] == (588, 768) and spec["classifier.weight"] == (400, 768)
    assert all(video_engine_shape(v) == spec[k] for k, v in ck.items())


def test_transformers_here_uses_the_installed_spelling():
    transformers = pytest.importorskip("transformers")
    c = TINY_VIDEO
    model = transformers.VideoMAEForVideoClassification(transformers.VideoMAEConfig(
        hidden_size=c.hidden, num_attention_heads=c.heads, num_hidden_layers=c.layers, intermediate_size=c.intermediate,
        image_size=c.image_size, patch_size=c.patch_size, tubelet_size=c.tubelet_size, num_frames=c.num_frames, num_labels=c.num_labels))
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == dict(video_checkpoint_spec(c))
    assert model.fc_norm.eps == 1e-5 and model.videomae.layernorm is None


def to_original_spelling(sd):
    """the installed spelling -> the hub file's: ``q_bias`` / ``v_bias`` beside bias-free projections (the key bias, zeros, is dropped)"""
    out = {}
    for k, v in sd.items():
        if k.endswith(".attention.attention.query.bias"):
            out[k[:-len("query.bias")] + "q_bias"] = v
        elif k.endswith(".attention.attention.value.bias"):
            out[k[:-len("value.bias")] + "v_bias"] = v
        elif not k.endswith(".attention.attention.key.bias"):
            out[k] = v
    return out


def test_both_spellings_name_the_same_tensors():
    spec = video_checkpoint_spec(TINY_VIDEO)
    sd = {k: np.full(v, i, np.float32) for i, (k, v) in enumerate(spec.items())}
    orig = to_original_spelling(sd)
    assert len(orig) == len(sd) - TINY_VIDEO.layers and any(k.endswith("q_bias") for k in orig) and not any(k.endswith("key.bias") for k in orig)
    back = video_checkpoint_rename(orig)
    assert sorted(back) == sorted(spec)
    for k, v in back.items():
        if k.endswith(".attention.attention.key.bias"):
            assert v.shape == spec[k] and not v.any()                          # an absent key bias is zeros
        else:
            assert np.array_equal(v, sd[k]), k
    assert all(video_checkpoint_key(k) == k for k in spec)
    same = video_checkpoint_rename(sd)
    assert list(same) == list(sd) and all(same[k] is sd[k] for k in sd)        # the installed spelling passes through
    t = video_checkpoint_rename({k: torch.from_numpy(v) for k, v in orig.items()})
    assert isinstance(t["videomae.encoder.layer.0.attention.attention.key.bias"], torch.Tensor)


def test_create_validates_each_video_field(lib):
    def refused(text, cfg=TINY_VIDEO, **fields):
        st, _ = host_ctx(lib, cfg, **fields)
        assert st == _lib.E2V_EINVAL and text in lib.e2v_last_error(None), (fields, lib.e2v_last_error(None))
    refused(b"64 * vmae_heads", vmae_heads=3)
    refused(b"1280", dataclasses.replace(TINY_VIDEO, hidden=1344, heads=21))
    refused(b"multiple of vmae_tubelet_size", vmae_num_frames=5)
    refused(b"multiple of vmae_patch_size", vmae_image_size=52, vmae_resize_edge=52)
    refused(b"vmae_resize_edge", vmae_resize_edge=48)
    refused(b"at least 3", vmae_num_labels=2)
    refused(b"vmae_intermediate", vmae_intermediate=254)
    refused(b"positive", vmae_tubelet_size=0)
    refused(b"positive", vmae_norm_eps=0.0)
    st, _ = host_ctx(lib, TINY_VIDEO, vmae_std=(C.c_float * 3)(0.2, 0.0, 0.2))
    assert st == _lib.E2V_EINVAL and b"vmae_std" in lib.e2v_last_error(None)
    for ok in (TINY_VIDEO, VideoConfig(), VideoConfig(num_frames=16), dataclasses.replace(TINY_VIDEO, resize_edge=64),
               dataclasses.replace(TINY_VIDEO, tubelet_size=3, num_frames=3)):
        st, ctx = host_ctx(lib, ok)
        assert st == 0, lib.e2v_last_error(None)
        lib.e2v_destroy(ctx)


def test_call_order_and_argument_errors_on_a_host_only_context(lib):
    st, ctx = host_ctx(lib, TINY_VIDEO)
    assert st == 0
    frames = np.zeros((1, 6, 8, 8, 3), np.uint8)
    out = np.zeros((2, 64), np.float32)
    fp, op = frames.ctypes.data_as(C.c_void_p), out.ctypes.data
    U8CL = _lib.E2V_FRAMES_U8 | _lib.E2V_FRAMES_CHANNELS_LAST
    call = lambda *a: lib.e2v_video_classify(ctx, *a, None)
    assert call(fp, U8CL, 1, 6, 8, 8, op, None, None) == _lib.E2V_ESTATE and b"not finalized" in lib.e2v_last_error(ctx)
    assert call(fp, U8CL, 1, 6, 8, 8, None, op, None) == _lib.E2V_ESTATE                      # any two outputs may be null ...
    assert call(fp, U8CL, 1, 6, 8, 8, None, None, None) == _lib.E2V_EINVAL                    # ... not all three
    assert call(None, U8CL, 1, 6, 8, 8, op, None, None) == _lib.E2V_EINVAL
    assert call(fp, U8CL, 0, 6, 8, 8, op, None, None) == _lib.E2V_EINVAL                      # n < 1
    assert call(fp, 4, 1, 6, 8, 8, op, None, None) == _lib.E2V_EINVAL                         # unknown kind bit
    assert call(fp, U8CL, 1, 6, 8, 8, C.c_void_p(op + 2), None, None) == _lib.E2V_EINVAL      # misaligned output
    assert call(C.c_void_p(frames.ctypes.data + 1), _lib.E2V_FRAMES_F32, 1, 6, 8, 8, op, None, None) == _lib.E2V_EINVAL      # fp32 frames at an odd byte
    assert call(C.c_void_p(frames.ctypes.data + 1), U8CL, 1, 6, 8, 8, op, None, None) == _lib.E2V_ESTATE                     # bytes may start anywhere
    for f in (4, 5, 7, 16):                                                                   # F != vmae_num_frames, odd ones among them
        assert call(fp, U8CL, 1, f, 8, 8, op, None, None) == _lib.E2V_ESHAPE and b"vmae_num_frames" in lib.e2v_last_error(ctx)
    for f, h, w in ((0, 8, 8), (6, 0, 8), (6, 8, 0)):
        assert call(fp, U8CL, 1, f, h, w, op, None, None) == _lib.E2V_ESHAPE
    assert call(fp, U8CL, 1, 6, 30000, 30000, op, None, None) == _lib.E2V_ESHAPE and b"LDS band" in lib.e2v_last_error(ctx)     # 1073 rows of 56 bytes per output row
    assert call(fp, 4, 1, 5, 8, 8, op, None, None) == _lib.E2V_EINVAL                         # the argument errors come first
    assert lib.e2v_video_classify(None, fp, U8CL, 1, 6, 8, 8, op, None, None, None) == _lib.E2V_EINVAL
    assert lib.e2v_finalize_weights(ctx, 32) == _lib.E2V_ESTATE and b"host-only" in lib.e2v_last_error(ctx)
    # the op entries: argument checks first, then the host-only refusal
    att = lambda *a: lib.e2v_op_token_attention(ctx, *a, None)
    assert att(C.c_void_p(64), 384, C.c_void_p(64), 128, 1, 0, 2) == _lib.E2V_ESHAPE
    assert att(C.c_void_p(64), 380, C.c_void_p(64), 128, 1, 5, 2) == _lib.E2V_EINVAL          # ldqkv below 3 * heads * 64
    assert att(C.c_void_p(68), 384, C.c_void_p(64), 128, 1, 5, 2) == _lib.E2V_EINVAL          # 16-byte alignment
    assert att(None, 384, C.c_void_p(64), 128, 1, 5, 2) == _lib.E2V_EINVAL
    assert att(C.c_void_p(64), 384, C.c_void_p(64), 128, 1, 1568, 2) == _lib.E2V_ESTATE       # no limit on T
    pre = lambda *a: lib.e2v_op_video_preprocess(ctx, fp, U8CL, *a, None)
    assert pre(1, 6, 8, 8, 56, 9, 2, 56, None, C.c_void_p(64)) == _lib.E2V_ESHAPE             # S no multiple of P
    assert pre(1, 6, 8, 8, 56, 8, 2, 48, None, C.c_void_p(64)) == _lib.E2V_ESHAPE             # edge below S
    assert pre(1, 5, 8, 8, 56, 8, 2, 56, None, C.c_void_p(64)) == _lib.E2V_ESHAPE             # F no multiple of ts
    assert pre(1, 6, 8, 8, 56, 8, 2, 56, None, None) == _lib.E2V_EINVAL
    assert pre(1, 6, 8, 8, 56, 8, 2, 56, None, C.c_void_p(64)) == _lib.E2V_ESTATE
    lib.e2v_destroy(ctx)
    st, ctx = host_ctx(lib)                                                                   # no video config: no pixel table either
    assert lib.e2v_op_video_preprocess(ctx, fp, U8CL, 1, 6, 8, 8, 56, 8, 2, 56, None, C.c_void_p(64), None) == _lib.E2V_ESTATE
    assert b"no pixel table" in lib.e2v_last_error(ctx)
    lib.e2v_destroy(ctx)


def test_video_weights_are_frozen_for_update_tensor(lib):
    st, ctx = host_ctx(lib, TINY_VIDEO)
    w = np.zeros((128,), np.float32)
    shape = (C.c_int64 * 1)(128)
    assert lib.e2v_update_tensor(ctx, b"video.fc_norm.weight", w.ctypes.data_as(C.c_void_p), _lib.E2V_F32, 0, shape, 1, None) == _lib.E2V_EINVAL
    assert b"frozen" in lib.e2v_last_error(ctx) and b"video" in lib.e2v_last_error(ctx)
    lib.e2v_destroy(ctx)


def test_signatures_hold_the_new_entries(lib):
    for name in ("e2v_video_classify", "e2v_op_video_preprocess", "e2v_op_token_attention"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["e2v_video_classify"][1]) == 11 and len(_lib.SIGNATURES["e2v_op_video_preprocess"][1]) == 14
    assert lib.e2v_op_set_knob(b"E2V_VMAE_CHUNK", 16) == 0 and lib.e2v_op_set_knob(b"E2V_VMAE_CHUNKS", 16) != 0


def test_image_and_video_configs_live_side_by_side(lib):
    from eeg2video_amd.engine import fill_image_config
    from eeg2video_amd.weights import image_param_spec
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    fill_image_config(cfg, TINY_IMAGE)
    fill_video_config(cfg, TINY_VIDEO)
    ctx = C.c_void_p()
    assert lib.e2v_create(C.byref(cfg), -1, C.byref(ctx)) == 0
    got = list(key_scheme(lib, ctx))
    lib.e2v_destroy(ctx)
    assert got[-len(video_param_spec(TINY_VIDEO)):] == ["video." + k for k in video_param_spec(TINY_VIDEO)]
    assert sum(k.startswith("image.") for k in got) == len(image_param_spec(TINY_IMAGE))


# ---- video_classify_metric -------------------------------------------------------------------------------------------------------
class SeededClassifier:
    """stands in for the device: clip i of either side is its first byte's row of seeded probabilities"""

    def __init__(self, probs, num_frames=6):
        self.vcfg = dataclasses.replace(TINY_VIDEO, num_frames=num_frames)
        self.probs, self.calls = probs, 0

    def classify(self, frames, channels_last=None):
        assert frames.dtype == torch.uint8 and frames.dim() == 5 and frames.shape[-1] == 3 and channels_last
        self.calls += 1
        p = torch.from_numpy(self.probs[frames[:, 0, 0, 0, 0].numpy()])
        return torch.log(p), p, torch.from_numpy(top3(p.numpy()))


def reference_video_loop(pred_probs, gt_probs, n_way, num_trials, top_k):
    """EEG2Video/40_class_run_metrics.py:128-139 with the two forwards replaced by the seeded probabilities"""
    acc_list, std_list = [], []
    for pred, gt in zip(pred_probs, gt_probs):
        gt_class_id = torch.from_numpy(gt).argsort(-1, descending=False).flatten()[-3:]
        pred_out = torch.from_numpy(pred).flatten()
        acc, std = reference_n_way_top_k_acc(pred_out, [int(i) for i in gt_class_id], n_way, num_trials, top_k)
        acc_list.append(acc)
        std_list.append(std)
    return acc_list, std_list


@pytest.mark.parametrize("n_way,top_k", [(2, 1), (40, 1), (50, 1), (40, 3)])
def test_video_classify_metric_bookkeeping_equals_the_reference_loop(n_way, top_k):
    from eeg2video_amd.metrics import video_classify_metric
    g = torch.Generator().manual_seed(n_way + top_k)
    probs = torch.rand(9, 60, generator=g, dtype=torch.float64).softmax(-1).float().numpy()
    pred_idx, gt_idx = [0, 1, 2, 3, 4], [5, 6, 7, 8, 2]
    clips = lambda idx: np.stack([np.full((6, 4, 4, 3), i, np.uint8) for i in idx])
    fake = SeededClassifier(probs)
    np.random.seed(3)
    got = video_classify_metric(clips(pred_idx), clips(gt_idx), n_way=n_way, num_trials=25, top_k=top_k, return_std=True, model=fake)
    np.random.seed(3)
    want = reference_video_loop(probs[pred_idx], probs[gt_idx], n_way, 25, top_k)
    assert got == want and fake.calls == 2                                       # one device call per side, not per clip
    np.random.seed(3)
    assert video_classify_metric(torch.from_numpy(clips(pred_idx)), clips(gt_idx), n_way=n_way, num_trials=25, top_k=top_k, model=fake) == want[0]
    with pytest.raises(ValueError, match="num_frames"):
        video_classify_metric(clips(pred_idx), clips(gt_idx), num_frames=16, model=fake)
    with pytest.raises(ValueError, match="5 generated clips against 4"):
        video_classify_metric(clips(pred_idx), clips(gt_idx[:4]), model=fake)
    with pytest.raises(AssertionError):
        video_classify_metric(clips(pred_idx), clips(gt_idx), n_way=3, top_k=3, model=fake)
