"""CPU: the CLIP score's host side -- the bicubic resize table against Pillow, the crop-window geometry against the processor's bytes,
the float64 restatement against the ``transformers`` fixture (``tests/golden/clip_vision_tiny.npz``), config fields / key scheme /
argument checks of a host-only context, ``n_way_from_matrix`` against a restatement of the reference's loop, and what
``from_pretrained`` refuses."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest

from eeg2video_amd import _lib
from eeg2video_amd.engine import clip_vision_config, image_resize_table
from eeg2video_amd.metrics import n_way_from_matrix
from eeg2video_amd.weights import (TINY_CLIP_VISION, ClipVisionConfig, SemanticConfig, UNetConfig, VAEConfig, clip_vision_param_spec,
                                   semantic_param_spec, unet_param_spec, vae_param_spec)
from clip_vision_restatement import (SHAPES, clip_vision_forward, cosine64, crop_geometry, golden_groups, load_golden, patch_rows,
                                     pillow_resize_crop, pixel_table, reference_n_way, rel_err, resize_crop_with_tables)
from vit_restatement import apply_axis

BOUND = 1e-5        # max |a-b| / max |b|: the project's bound for fp32 arithmetic (tests/test_hip_text.py)
bicubic = lambda i, o: image_resize_table(i, o, 3)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def host_ctx(lib, clip_cfg=None, **fields):
    """a host-only context; ``clip_cfg``: made by ``e2v_create_clip_vision`` with that tower (``fields``: overrides of its struct)"""
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    ctx = C.c_void_p()
    if clip_cfg is None:
        return lib.e2v_create(C.byref(cfg), -1, C.byref(ctx)), ctx
    vcfg = clip_vision_config(clip_cfg)
    for k, v in fields.items():
        setattr(vcfg, k, v)
    return lib.e2v_create_clip_vision(C.byref(cfg), C.byref(vcfg), -1, C.byref(ctx)), ctx


def key_scheme(lib, ctx):
    shape, nd, got = (C.c_int64 * 4)(), C.c_int(), {}
    for i in range(lib.e2v_num_expected_keys(ctx)):
        k = lib.e2v_expected_key(ctx, i, shape, C.byref(nd)).decode()
        got[k] = tuple(shape[d] for d in range(nd.value))
    return got


# ---- resize table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", [(288, 224), (512, 398), (37, 112), (36, 112), (64, 199), (131, 163), (90, 112), (112, 112),
                                        (500, 33), (7, 64), (1, 5), (300, 299)])
def test_bicubic_table_equals_pillow_bit_for_bit(n_in, n_out):
    """one axis of ``e2v_image_resize_table_filter(..., 3)`` applied in integer numpy against ``Image.resize(BICUBIC)`` of an image
    that only that axis resizes: the production pair (288 -> 224, 512 -> 398), upscales, downscales (a strong one), 1:1, ``in = 1``"""
    Image = pytest.importorskip("PIL.Image")
    img = np.random.default_rng(n_in * 1000 + n_out).integers(0, 256, (5, n_in), dtype=np.uint8)
    got = apply_axis(img, *bicubic(n_in, n_out))
    want = np.asarray(Image.fromarray(img).resize((n_out, 5), Image.BICUBIC))
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    got_v = apply_axis(np.ascontiguousarray(img.T[None]).transpose(0, 2, 1), *bicubic(n_in, n_out))[0].T       # the same as a vertical pass
    assert np.array_equal(got_v, np.asarray(Image.fromarray(np.ascontiguousarray(img.T)).resize((5, n_out), Image.BICUBIC)))


def test_bicubic_clips_as_pillow_does():
    """black / white stripes overshoot on both sides: sums below 0 and above 255 are clipped to bytes after the shift"""
    Image = pytest.importorskip("PIL.Image")
    img = np.zeros((4, 90), np.uint8)
    img[:, (np.arange(90) // 3) % 2 == 1] = 255
    for n_out in (131, 61, 90):
        first, count, coeff = bicubic(90, n_out)
        acc = np.stack([(1 << 21) + (img[0, first[x]:first[x] + count[x]].astype(np.int64) * coeff[x, :count[x]]).sum() for x in range(n_out)]) >> 22
        want = np.asarray(Image.fromarray(img).resize((n_out, 4), Image.BICUBIC))
        assert np.array_equal(np.clip(acc, 0, 255), want[0])
        if n_out != 90:
            assert acc.min() < 0 and acc.max() > 255                     # the case really clips, and
            assert (want == 0).any() and (want == 255).any()
    assert (bicubic(90, 131)[2] < 0).any()                               # coefficients are negative in places


def test_filter_2_is_the_bilinear_table_and_other_filters_are_refused(lib):
    for n_in, n_out in ((288, 224), (512, 398), (37, 112), (112, 112), (500, 33)):
        for a, b in zip(image_resize_table(n_in, n_out), image_resize_table(n_in, n_out, 2)):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    ksize = C.c_int(0)
    for bad in (0, 1, 4, 5, -1):
        assert lib.e2v_image_resize_table_filter(8, 8, bad, None, None, None, C.byref(ksize)) == _lib.E2V_EINVAL
    assert lib.e2v_image_resize_table_filter(0, 8, 3, None, None, None, C.byref(ksize)) == _lib.E2V_EINVAL
    assert lib.e2v_image_resize_table_filter(8, 8, 3, None, None, None, None) == _lib.E2V_EINVAL
    assert lib.e2v_image_resize_table_filter(512, 398, 3, None, None, None, C.byref(ksize)) == 0 and ksize.value == 7
    assert lib.e2v_image_resize_table_filter(288, 224, 3, None, None, None, C.byref(ksize)) == 0 and ksize.value == 7


def test_accumulator_headroom():
    """22 bits leave the 32-bit accumulator room: 2^21 + 255 * (the positive or the negative coefficients of an output) stays inside"""
    for n_in, n_out in ((288, 224), (512, 398), (37, 112), (4096, 224), (3, 4096), (500, 33)):
        coeff = bicubic(n_in, n_out)[2].astype(np.int64)
        assert (1 << 21) + 255 * np.where(coeff > 0, coeff, 0).sum(-1).max() < 2 ** 31
        assert (1 << 21) + 255 * np.where(coeff < 0, coeff, 0).sum(-1).min() >= -2 ** 31


# ---- crop-window plan ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,edge,size", [(288, 512, 224, 224), (512, 288, 224, 224), (100, 37, 112, 112), (37, 100, 112, 112),
                                           (300, 225, 224, 224), (1300, 12, 16, 16)])
def test_resize_and_crop_from_tables_equals_pillow(h, w, edge, size):
    pytest.importorskip("PIL")
    img = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    assert np.array_equal(resize_crop_with_tables(img, edge, size, bicubic), pillow_resize_crop(img, edge, size, 3))


def test_crop_geometry():
    assert crop_geometry(288, 512, 224, 224) == (224, 398, 0, 87)
    assert crop_geometry(131, 90, 112, 112) == (163, 112, 25, 0)         # an odd remainder: 51 rows dropped, 25 on top
    assert crop_geometry(36, 64, 112, 112) == (112, 199, 0, 43)


def test_fixture_cropped_bytes_are_reproduced(golden):
    z, _ = golden
    c = TINY_CLIP_VISION
    assert str(z["pillow_version"]) and str(z["transformers_version"])
    assert [z[f"images_{h}x{w}"].shape for _, h, w in SHAPES] == [(n, h, w, 3) for n, h, w in SHAPES]
    for images, cropped in golden_groups(z):
        for img, want in zip(images, cropped):
            assert np.array_equal(resize_crop_with_tables(img, c.resize_edge, c.image_size, bicubic), want)
    assert np.array_equal(pixel_table(c.rescale_factor, c.image_mean, c.image_std), z["pixel_table"])     # the processor's own table
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "clip_vision_tiny.npz")) < 1 << 20


# ---- restatement -----------------------------------------------------------------------------------------------------------------
def fixture_rows(z):
    return np.stack([patch_rows(img, z["pixel_table"], TINY_CLIP_VISION.patch_size) for _, cropped in golden_groups(z) for img in cropped])


def test_restatement_vs_transformers_fixture(golden):
    z, sd = golden
    c = TINY_CLIP_VISION
    assert set(sd) == set(clip_vision_param_spec(c)) and all(z["w." + k].dtype == np.float16 for k in sd)
    emb = clip_vision_forward(sd, fixture_rows(z), c.heads, c.layer_norm_eps, c.hidden_act)
    err = rel_err(z["image_embeds"], emb)
    print(f"transformers {z['transformers_version']} fp32 image_embeds vs the float64 restatement: {err:.3e}")
    assert z["image_embeds"].shape == (8, 64) and z["image_embeds"].dtype == np.float32 and err < BOUND, err
    e = z["image_embeds"]
    perr = float(np.abs(z["pair_scores"] - cosine64(e, np.roll(e, 1, 0))).max())
    merr = float(np.abs(z["matrix"] - cosine64(e, e, matrix=True)).max())
    e2e = float(np.abs(z["matrix"] - cosine64(emb, emb, matrix=True)).max())
    print(f"cosine alone: pairs {perr:.3e}, matrix {merr:.3e}; whole model: matrix {e2e:.3e}")
    assert perr < 1e-6 and merr < 1e-6 and e2e < BOUND
    srt = np.sort(z["matrix"], -1)
    assert (np.diff(srt, axis=-1) > 1e-3).all()                                           # the fixture's own promise
    assert np.array_equal(np.argsort(cosine64(emb, emb, matrix=True), -1), np.argsort(z["matrix"], -1))


def test_cosine_restatement_is_torchs():
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((6, 20)), rng.standard_normal((6, 20))
    a[2] = 0.0
    b[4] = 1e-10                                                             # a norm below eps: each norm is clamped on its own
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    assert np.allclose(cosine64(a, b), F.cosine_similarity(ta, tb, dim=-1).numpy(), rtol=1e-12, atol=1e-15)
    assert np.allclose(cosine64(a, b, matrix=True), F.cosine_similarity(ta[:, None], tb[None], dim=-1).numpy(), rtol=1e-12, atol=1e-15)
    assert cosine64(a, b)[2] == 0.0


# ---- keys and ABI ----------------------------------------------------------------------------------------------------------------
CLIPV_INT_FIELDS = ("clipv_hidden", "clipv_heads", "clipv_layers", "clipv_intermediate", "clipv_image_size", "clipv_patch_size",
                    "clipv_projection_dim", "clipv_act", "clipv_resize_edge", "clipv_resample")


def test_a_plain_context_has_no_vision_tower(lib):
    """``e2v_config`` keeps its layout (the tower's config is a struct of its own); ``e2v_create``, and ``e2v_create_clip_vision`` with
    a NULL or all-zero tower, make a context without one"""
    assert lib.e2v_config_size() == C.sizeof(_lib.E2VConfig) and lib.e2v_clipv_config_size() == C.sizeof(_lib.E2VClipVConfig)
    assert not any(f[0].startswith("clipv_") for f in _lib.E2VConfig._fields_)
    assert [f[0] for f in _lib.E2VClipVConfig._fields_][:10] == list(CLIPV_INT_FIELDS[:8]) + ["clipv_norm_eps", "clipv_resize_edge"]
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    for vcfg in (None, C.byref(_lib.E2VClipVConfig())):
        ctx = C.c_void_p()
        assert lib.e2v_create_clip_vision(C.byref(cfg), vcfg, -1, C.byref(ctx)) == 0
        assert not any(k.startswith("clipv.") for k in key_scheme(lib, ctx))
        lib.e2v_destroy(ctx)
    st, ctx = host_ctx(lib)
    assert st == 0
    got = key_scheme(lib, ctx)
    frames = np.zeros((1, 1, 8, 8, 3), np.uint8)
    out = np.zeros((1, 64), np.float32)
    st = lib.e2v_clip_embed(ctx, frames.ctypes.data_as(C.c_void_p), 3, 1, 1, 8, 8, out.ctypes.data_as(C.c_void_p), None)
    assert st == _lib.E2V_ESTATE and b"no CLIP vision tower" in lib.e2v_last_error(ctx)
    assert lib.e2v_finalize_weights(ctx, 64) == _lib.E2V_ESTATE
    lib.e2v_destroy(ctx)
    want = dict(unet_param_spec(UNetConfig()))
    want.update({"vae." + k: v for k, v in vae_param_spec(VAEConfig()).items()})
    want.update({"semantic." + k: v for k, v in semantic_param_spec(SemanticConfig(), 768).items()})
    assert got == want and not any(k.startswith("clipv.") for k in got)


def test_key_scheme_with_a_vision_config_is_the_old_one_plus_the_spec(lib):
    st, ctx = host_ctx(lib, TINY_CLIP_VISION)
    assert st == 0
    got = key_scheme(lib, ctx)
    spec = clip_vision_param_spec(TINY_CLIP_VISION)
    assert [k for k in got if k.startswith("clipv.")] == ["clipv." + k for k in spec]                 # in the spec's order
    assert all(got["clipv." + k] == v for k, v in spec.items()) and len(got) == 798 + 248 + 10 + len(spec)
    # keys accepted or refused
    # (a host-only context cannot load; tests/test_hip_clip_vision.py loads and is refused on the device)
    assert "clipv.vision_model.embeddings.position_ids" not in got                                    # a buffer, not a weight
    assert "clipv.visual_projection.bias" not in got and "clipv.vision_model.embeddings.patch_embedding.bias" not in got
    assert "clipv.vision_model.pre_layernorm.weight" not in got and got["clipv.vision_model.pre_layrnorm.weight"] == (128,)
    # both entry points answer a host-only context with E2V_ESTATE
    frames = np.zeros((1, 1, 8, 8, 3), np.uint8)
    out = np.zeros((4, 64), np.float32)
    st = lib.e2v_clip_embed(ctx, frames.ctypes.data_as(C.c_void_p), 3, 1, 1, 8, 8, out.ctypes.data_as(C.c_void_p), None)
    assert st == _lib.E2V_ESTATE, lib.e2v_last_error(ctx)
    a = np.zeros((4, 64), np.float32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    assert lib.e2v_clip_similarity(ctx, p(a), 4, p(a), 4, 64, 0, p(out), None) == _lib.E2V_ESTATE
    # and what is wrong with the call itself comes first
    assert lib.e2v_clip_similarity(ctx, p(a), 4, p(a), 4, 62, 0, p(out), None) == _lib.E2V_ESHAPE
    assert lib.e2v_clip_similarity(ctx, p(a), 4, p(a), 3, 64, 0, p(out), None) == _lib.E2V_ESHAPE
    assert lib.e2v_clip_similarity(ctx, p(a), 0, p(a), 4, 64, 1, p(out), None) == _lib.E2V_ESHAPE
    assert lib.e2v_clip_similarity(ctx, p(a), 4, p(a), 4, 64, 2, p(out), None) == _lib.E2V_EINVAL
    assert lib.e2v_clip_similarity(ctx, None, 4, p(a), 4, 64, 0, p(out), None) == _lib.E2V_EINVAL
    assert lib.e2v_clip_similarity(ctx, C.c_void_p(a.ctypes.data + 4), 1, p(a), 1, 4, 0, p(out), None) == _lib.E2V_EINVAL       # 16-byte rows
    assert lib.e2v_clip_embed(ctx, None, 3, 1, 1, 8, 8, p(out), None) == _lib.E2V_EINVAL
    assert lib.e2v_clip_embed(ctx, p(frames), 3, 1, 1, 8, 8, None, None) == _lib.E2V_EINVAL
    assert lib.e2v_clip_embed(ctx, p(frames), 3, 1, 1, 0, 8, p(out), None) == _lib.E2V_ESHAPE
    lib.e2v_destroy(ctx)


def test_clip_b32_spec_is_the_checkpoints():
    """199 tensors: 3 of the embeddings, pre_layrnorm, 12 layers of 16, post_layernorm, the projection"""
    spec = clip_vision_param_spec(ClipVisionConfig())
    assert len(spec) == 3 + 2 + 12 * 16 + 2 + 1 and ClipVisionConfig().tokens == 50 and TINY_CLIP_VISION.tokens == 50
    assert spec["vision_model.embeddings.class_embedding"] == (768,) and spec["vision_model.embeddings.position_embedding.weight"] == (50, 768)
    assert spec["vision_model.embeddings.patch_embedding.weight"] == (768, 3, 32, 32) and spec["visual_projection.weight"] == (512, 768)
    assert "vision_model.pre_layrnorm.weight" in spec and "visual_projection.bias" not in spec


def test_transformers_here_names_the_same_tensors():
    transformers = pytest.importorskip("transformers")
    c = TINY_CLIP_VISION
    model = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(
        hidden_size=c.hidden, num_attention_heads=c.heads, num_hidden_layers=c.layers, intermediate_size=c.intermediate,
        image_size=c.image_size, patch_size=c.patch_size, projection_dim=c.projection_dim))
    own = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith("position_ids")}
    assert own == dict(clip_vision_param_spec(c))


def test_create_validates_the_vision_fields(lib):
    st, _ = host_ctx(lib, TINY_CLIP_VISION, clipv_heads=3)
    assert st == _lib.E2V_EINVAL and b"64 * clipv_heads" in lib.e2v_last_error(None)
    st, _ = host_ctx(lib, dataclasses.replace(TINY_CLIP_VISION, hidden=1344, heads=21))
    assert st == _lib.E2V_EINVAL and b"1280" in lib.e2v_last_error(None)
    st, _ = host_ctx(lib, TINY_CLIP_VISION, clipv_image_size=110)
    assert st == _lib.E2V_EINVAL and b"multiple of clipv_patch_size" in lib.e2v_last_error(None)
    st, _ = host_ctx(lib, dataclasses.replace(TINY_CLIP_VISION, image_size=272, resize_edge=272))      # 17^2 + 1 = 290 tokens
    assert st == _lib.E2V_EINVAL and b"288" in lib.e2v_last_error(None)
    st, _ = host_ctx(lib, TINY_CLIP_VISION, clipv_projection_dim=62)
    assert st == _lib.E2V_EINVAL
    st, _ = host_ctx(lib, TINY_CLIP_VISION, clipv_resample=1)
    assert st == _lib.E2V_EINVAL and b"clipv_resample" in lib.e2v_last_error(None)
    st, _ = host_ctx(lib, TINY_CLIP_VISION, clipv_resize_edge=100)
    assert st == _lib.E2V_EINVAL and b"clipv_resize_edge" in lib.e2v_last_error(None)
    st, _ = host_ctx(lib, TINY_CLIP_VISION, clipv_act=2)
    assert st == _lib.E2V_EINVAL
    st, _ = host_ctx(lib, dataclasses.replace(TINY_CLIP_VISION, image_std=(0.5, 0.0, 0.5)))
    assert st == _lib.E2V_EINVAL and b"clipv_std" in lib.e2v_last_error(None)
    for ok in (TINY_CLIP_VISION, ClipVisionConfig(),                                                                    # B/32: 50 tokens
               ClipVisionConfig(patch_size=16),                                                                         # B/16: 197
               ClipVisionConfig(hidden=1024, heads=16, layers=24, intermediate=4096, patch_size=14, projection_dim=768),  # L/14: 257
               dataclasses.replace(TINY_CLIP_VISION, resample=2, hidden_act="gelu")):
        st, ctx = host_ctx(lib, ok)
        assert st == 0, lib.e2v_last_error(None)
        lib.e2v_destroy(ctx)


# ---- the trial loop ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_way,top_k,num_trials", [(12, 5, 1, 7), (12, 12, 3, 4), (9, 2, 1, 10), (20, 10, 2, 3)])
def test_n_way_from_matrix_is_the_reference_loop(n, n_way, top_k, num_trials):
    """the vectorised look-up against the reference's loop, image by image through a score function, under the same numpy seed: the
    same draws in the same order, ``rest`` indexed as there (the ground truths without ``idx``), ties included"""
    rng = np.random.default_rng(n * 100 + n_way)
    m = rng.random((n, n)).astype(np.float32)
    m[3, :] = np.round(m[3, :], 1)                                           # ties, the diagonal's among them
    m[5, :] = m[5, 5]
    pred, gt = list(range(n)), list(range(n))
    calls = []
    score = lambda p, g: calls.append((p, g)) or float(m[p, g])
    np.random.seed(1234)
    want = reference_n_way(pred, gt, score, n_way, top_k, num_trials)
    after = np.random.random()
    np.random.seed(1234)
    got = n_way_from_matrix(m, n_way, top_k, num_trials)
    assert got == want and np.random.random() == after                       # and the generator stands where the reference leaves it
    assert len(calls) == n * (num_trials * (n_way - 1) + 1)                  # the pairs the reference embeds again and again
    assert 0.0 < np.mean(want) < 1.0 or n_way == 2
    with pytest.raises(ValueError):
        n_way_from_matrix(m[:, :-1], n_way, top_k, num_trials)


# ---- from_pretrained refusals (no GPU: config_from_dir reads two JSON files) ------------------------------------------------------
def write_dir(tmp_path, config=None, proc=None):
    c = TINY_CLIP_VISION
    cj = {"hidden_size": c.hidden, "num_attention_heads": c.heads, "num_hidden_layers": c.layers, "intermediate_size": c.intermediate,
          "image_size": c.image_size, "patch_size": c.patch_size, "projection_dim": c.projection_dim, "hidden_act": c.hidden_act,
          "layer_norm_eps": c.layer_norm_eps}
    pj = {"size": {"shortest_edge": c.resize_edge}, "crop_size": {"height": c.image_size, "width": c.image_size}, "resample": 3,
          "rescale_factor": c.rescale_factor, "image_mean": list(c.image_mean), "image_std": list(c.image_std)}
    cj.update(config or {})
    pj.update(proc or {})
    d = tmp_path / f"m{len(list(tmp_path.iterdir()))}"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(cj))
    (d / "preprocessor_config.json").write_text(json.dumps(pj))
    return str(d)


def test_config_from_dir_reads_both_config_kinds_and_refuses_what_the_kernels_cannot_do(tmp_path):
    from eeg2video_amd.clip_vision import CLIPVisionModelWithProjection as M
    assert M.config_from_dir(write_dir(tmp_path)) == TINY_CLIP_VISION
    c = TINY_CLIP_VISION
    full = {"model_type": "clip", "projection_dim": c.projection_dim, "text_config": {"hidden_size": 32},
            "vision_config": {"hidden_size": c.hidden, "num_attention_heads": c.heads, "num_hidden_layers": c.layers,
                              "intermediate_size": c.intermediate, "image_size": c.image_size, "patch_size": c.patch_size}}
    d = write_dir(tmp_path)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(full, f)
    assert M.config_from_dir(d) == TINY_CLIP_VISION                                            # a full CLIPConfig
    assert M.config_from_dir(write_dir(tmp_path, proc={"resample": 2})).resample == 2
    for config, proc, word in (({"num_attention_heads": 4}, None, "head dim"),                   # 128 / 4 = 32
                               ({"image_size": 272}, {"crop_size": {"height": 272, "width": 272}, "size": {"shortest_edge": 272}}, "tokens"),
                               (None, {"crop_size": {"height": 96, "width": 96}}, "crops"),
                               (None, {"crop_size": {"height": 112, "width": 96}}, "square"),
                               (None, {"resample": 1}, "resample"),                              # LANCZOS
                               (None, {"resample": 0}, "resample"),
                               (None, {"size": {"height": 112, "width": 112}}, "shortest"),
                               (None, {"do_center_crop": False}, "do_center_crop"),
                               ({"hidden_act": "silu"}, None, "hidden_act")):
        with pytest.raises(NotImplementedError, match=word):
            M.config_from_dir(write_dir(tmp_path, config, proc))
    with pytest.raises(RuntimeError, match="not a directory"):
        M.from_pretrained(str(tmp_path / "openai" / "clip-vit-base-patch32"))
    with pytest.raises(RuntimeError, match="does not exist"):
        M.from_pretrained(write_dir(tmp_path))                                                 # no weights file: before any engine is made
