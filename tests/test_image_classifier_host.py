"""CPU: the image classifier's host side -- the resize table against Pillow, the float64 restatement against the ``transformers``
fixture (``tests/golden/vit_tiny.npz``), config fields / key scheme / argument checks of a host-only context, and ``n_way_top_k_acc``
against a line-by-line restatement of the reference's loop."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from eeg2video_amd import _lib
from eeg2video_amd.engine import fill_image_config, image_resize_table
from eeg2video_amd.weights import (TINY_IMAGE, ImageConfig, SemanticConfig, UNetConfig, VAEConfig, image_checkpoint_key, image_param_spec,
                                   semantic_param_spec, unet_param_spec, vae_param_spec)
from vit_restatement import (load_golden, patch_rows, pillow_resize, pixel_table, rel_err, resize_with_tables, softmax64, top3,
                             vit_forward)

BOUND = 1e-5        # max |a-b| / max |b|: the project's bound for fp32 arithmetic (tests/test_hip_text.py)
GROUPS = ("36x64", "130x90", "112x112")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def host_ctx(lib, image_cfg=None, **fields):
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    if image_cfg is not None:
        fill_image_config(cfg, image_cfg)
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


# ---- resize table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,size", [(288, 512, 224), (36, 64, 112), (130, 90, 112), (112, 112, 112), (30, 20, 32), (37, 61, 32),
                                      (224, 224, 224), (1, 1, 16), (1, 50, 8), (50, 1, 8), (260, 2, 16), (200, 2, 16)])
def test_resize_table_equals_pillow_bit_for_bit(h, w, size):
    """the two-pass resize from ``e2v_image_resize_table`` against ``PIL.Image.resize(BILINEAR)``: the production shape, the fixture's
    three, upscales, ``in == out``, ``in = 1``, and either side of the 100:1 aspect beyond which Pillow runs the vertical pass first"""
    pytest.importorskip("PIL")
    img = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    got, want = resize_with_tables(img, size, image_resize_table), pillow_resize(img, size)
    assert got.shape == want.shape == (size, size, 3) and np.array_equal(got, want), int((got != want).sum())


def test_resize_table_shape_and_taps(lib):
    first, count, coeff = image_resize_table(512, 224)
    assert coeff.shape == (224, 7) and count.max() <= 7 and first.min() == 0 and (first + count).max() == 512      # 7 taps across
    assert image_resize_table(288, 224)[2].shape == (224, 5)                                                       # 5 down
    assert (coeff.sum(-1) - (1 << 22)).__abs__().max() <= 4                     # each row is a partition of 1 in 22-bit fixed point
    f1, c1, k1 = image_resize_table(64, 64)                                     # in == out: the identity
    assert np.array_equal(f1, np.arange(64)) and (k1[:, 0] == 1 << 22).all() and (k1[:, 1:] == 0).all()
    ksize = C.c_int(0)
    assert lib.e2v_image_resize_table(0, 8, None, None, None, C.byref(ksize)) == _lib.E2V_EINVAL
    assert lib.e2v_image_resize_table(8, 8, None, None, None, None) == _lib.E2V_EINVAL


def test_fixture_resized_bytes_are_reproduced(golden):
    z, _ = golden
    assert str(z["pillow_version"]) and str(z["transformers_version"])
    for g in GROUPS[:2]:
        for img, want in zip(z["images_" + g], z["resized_" + g]):
            assert np.array_equal(resize_with_tables(img, TINY_IMAGE.image_size, image_resize_table), want)
    assert z["images_36x64"].shape == (4, 36, 64, 3) and z["images_130x90"].shape == (2, 130, 90, 3) and z["images_112x112"].shape == (2, 112, 112, 3)
    c = TINY_IMAGE
    assert np.array_equal(pixel_table(c.rescale_factor, c.image_mean, c.image_std), z["pixel_table"])     # the processor's own table


# ---- restatement -----------------------------------------------------------------------------------------------------------------
def fixture_rows(z):
    rows = []
    for g in GROUPS:
        for i, img in enumerate(z["images_" + g]):
            resized = z["resized_" + g][i] if "resized_" + g in z.files else img
            rows.append(patch_rows(resized, z["pixel_table"], TINY_IMAGE.patch_size))
    return np.stack(rows)


def test_restatement_vs_transformers_fixture(golden):
    z, sd = golden
    assert set(sd) == set(image_param_spec(TINY_IMAGE)) and all(z["w." + k].dtype == np.float16 for k in sd)
    logits = vit_forward(sd, fixture_rows(z), TINY_IMAGE.heads, TINY_IMAGE.layer_norm_eps)
    err = rel_err(logits, z["logits"])
    print(f"float64 restatement vs transformers {z['transformers_version']} fp32 logits: {err:.3e}")
    assert z["logits"].shape == (8, 50) and z["logits"].dtype == np.float32 and err < BOUND, err
    perr = float(np.abs(softmax64(logits) - z["probs"]).max())
    print(f"softmax: {perr:.3e}")
    assert perr < 1e-6
    srt = np.sort(z["logits"], -1)
    assert ((srt[:, -3] - srt[:, -4]) > 1e-3 * np.abs(z["logits"]).max(-1)).all()        # the fixture's own promise
    assert np.array_equal(top3(logits), top3(z["logits"]))


def test_top3_ties_rank_as_a_stable_ascending_sort():
    x = np.array([[1.0, 3.0, 3.0, 2.0, 3.0], [0.0, 0.0, 0.0, 0.0, 0.0]])
    assert top3(x).tolist() == [[1, 2, 4], [2, 3, 4]]


# ---- keys and ABI ----------------------------------------------------------------------------------------------------------------
def test_default_config_has_no_image_classifier(lib):
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    assert [getattr(cfg, f) for f in ("vit_hidden", "vit_heads", "vit_layers", "vit_intermediate", "vit_image_size", "vit_patch_size",
                                      "vit_num_labels")] == [0] * 7
    assert cfg.vit_norm_eps == 0.0 and cfg.vit_rescale == 0.0 and list(cfg.vit_mean) == [0.0] * 3 and list(cfg.vit_std) == [0.0] * 3
    st, ctx = host_ctx(lib)
    assert st == 0
    got = key_scheme(lib, ctx)
    frames = np.zeros((1, 1, 8, 8, 3), np.uint8)
    out = np.zeros((1, 50), np.float32)
    st = lib.e2v_image_classify(ctx, frames.ctypes.data_as(C.c_void_p), 3, 1, 1, 8, 8, out.ctypes.data_as(C.c_void_p), None, None, None)
    assert st == _lib.E2V_ESTATE and b"no image classifier" in lib.e2v_last_error(ctx)
    assert lib.e2v_finalize_weights(ctx, 16) == _lib.E2V_ESTATE
    lib.e2v_destroy(ctx)
    assert got == old_scheme() and not any(k.startswith("image.") for k in got)


def test_key_scheme_with_an_image_config_is_the_old_one_plus_the_image_spec(lib):
    st, ctx = host_ctx(lib, TINY_IMAGE)
    assert st == 0
    got = key_scheme(lib, ctx)
    lib.e2v_destroy(ctx)
    want = old_scheme()
    want.update({"image." + k: v for k, v in image_param_spec(TINY_IMAGE).items()})
    assert got == want and len(got) == 798 + 248 + 10 + len(image_param_spec(TINY_IMAGE))
    assert [k for k in got if k.startswith("image.")] == ["image." + k for k in image_param_spec(TINY_IMAGE)]      # and in its order


def test_vit_base_spec_is_the_checkpoints():
    """200 tensors: 4 of the embeddings, 12 layers of 16, the final LayerNorm, the classifier"""
    spec = image_param_spec(ImageConfig())
    assert len(spec) == 4 + 12 * 16 + 2 + 2 and ImageConfig().tokens == 197 and TINY_IMAGE.tokens == 197
    assert spec["vit.embeddings.position_embeddings"] == (1, 197, 768) and spec["vit.embeddings.cls_token"] == (1, 1, 768)
    assert spec["vit.embeddings.patch_embeddings.projection.weight"] == (768, 3, 16, 16)
    assert spec["vit.encoder.layer.11.intermediate.dense.weight"] == (3072, 768) and spec["classifier.weight"] == (1000, 768)


def test_both_spellings_name_the_same_tensors():
    spec = image_param_spec(TINY_IMAGE)
    v5 = ["vit.embeddings.cls_token", "vit.embeddings.position_embeddings", "vit.embeddings.patch_embeddings.projection.weight",
          "vit.embeddings.patch_embeddings.projection.bias", "vit.layernorm.weight", "vit.layernorm.bias", "classifier.weight", "classifier.bias"]
    for i in range(TINY_IMAGE.layers):
        for n in ("attention.q_proj", "attention.k_proj", "attention.v_proj", "attention.o_proj", "layernorm_before", "layernorm_after",
                  "mlp.fc1", "mlp.fc2"):
            v5 += [f"vit.layers.{i}.{n}.weight", f"vit.layers.{i}.{n}.bias"]
    assert sorted(image_checkpoint_key(k) for k in v5) == sorted(spec)
    assert all(image_checkpoint_key(k) == k for k in spec)


def test_transformers_here_uses_one_of_the_two_spellings():
    transformers = pytest.importorskip("transformers")
    c = TINY_IMAGE
    model = transformers.ViTForImageClassification(transformers.ViTConfig(
        hidden_size=c.hidden, num_attention_heads=c.heads, num_hidden_layers=c.layers, intermediate_size=c.intermediate,
        image_size=c.image_size, patch_size=c.patch_size, num_labels=c.num_labels))
    own = {image_checkpoint_key(k): tuple(v.shape) for k, v in model.state_dict().items()}
    assert own == dict(image_param_spec(c))


def test_create_validates_the_image_fields(lib):
    st, _ = host_ctx(lib, TINY_IMAGE, vit_heads=3)
    assert st == _lib.E2V_EINVAL and b"64 * vit_heads" in lib.e2v_last_error(None)
    st, _ = host_ctx(lib, dataclasses.replace(TINY_IMAGE, hidden=1344, heads=21))
    assert st == _lib.E2V_EINVAL and b"1280" in lib.e2v_last_error(None)
    st, _ = host_ctx(lib, TINY_IMAGE, vit_image_size=110)
    assert st == _lib.E2V_EINVAL and b"multiple of vit_patch_size" in lib.e2v_last_error(None)
    st, _ = host_ctx(lib, dataclasses.replace(TINY_IMAGE, image_size=136))                     # 17^2 + 1 = 290 tokens
    assert st == _lib.E2V_EINVAL and b"288" in lib.e2v_last_error(None)
    st, _ = host_ctx(lib, TINY_IMAGE, vit_num_labels=2)
    assert st == _lib.E2V_EINVAL
    for ok in (TINY_IMAGE, ImageConfig(), ImageConfig(hidden=1024, heads=16, layers=24, intermediate=4096, patch_size=14),     # ViT-L/14: 257
               dataclasses.replace(TINY_IMAGE, image_size=128)):                                                                # 257 tokens
        st, ctx = host_ctx(lib, ok)
        assert st == 0, lib.e2v_last_error(None)
        lib.e2v_destroy(ctx)


def test_call_order_and_argument_errors_on_a_host_only_context(lib):
    st, ctx = host_ctx(lib, TINY_IMAGE)
    assert st == 0
    frames = np.zeros((1, 2, 8, 8, 3), np.uint8)
    out = np.zeros((2, 64), np.float32)
    fp, op = frames.ctypes.data_as(C.c_void_p), out.ctypes.data
    U8CL = _lib.E2V_FRAMES_U8 | _lib.E2V_FRAMES_CHANNELS_LAST
    call = lambda *a: lib.e2v_image_classify(ctx, *a, None)
    assert call(fp, U8CL, 1, 2, 8, 8, op, None, None) == _lib.E2V_ESTATE and b"not finalized" in lib.e2v_last_error(ctx)
    assert call(fp, U8CL, 1, 2, 8, 8, None, op, None) == _lib.E2V_ESTATE                      # any two outputs may be null ...
    assert call(fp, U8CL, 1, 2, 8, 8, None, None, None) == _lib.E2V_EINVAL                    # ... not all three
    assert call(None, U8CL, 1, 2, 8, 8, op, None, None) == _lib.E2V_EINVAL
    assert call(fp, U8CL, 0, 2, 8, 8, op, None, None) == _lib.E2V_EINVAL                      # n < 1
    assert call(fp, 4, 1, 2, 8, 8, op, None, None) == _lib.E2V_EINVAL                         # unknown kind bit
    assert call(fp, U8CL, 1, 2, 8, 8, C.c_void_p(op + 2), None, None) == _lib.E2V_EINVAL      # misaligned output
    assert call(C.c_void_p(frames.ctypes.data + 1), _lib.E2V_FRAMES_F32, 1, 2, 8, 8, op, None, None) == _lib.E2V_EINVAL      # fp32 frames at an odd byte
    assert call(C.c_void_p(frames.ctypes.data + 1), U8CL, 1, 2, 8, 8, op, None, None) == _lib.E2V_ESTATE                     # bytes may start anywhere
    for f, h, w in ((0, 8, 8), (2, 0, 8), (2, 8, 0)):
        assert call(fp, U8CL, 1, f, h, w, op, None, None) == _lib.E2V_ESHAPE
    assert call(fp, U8CL, 1, 2, 100000, 2000, op, None, None) == _lib.E2V_ESHAPE and b"LDS band" in lib.e2v_last_error(ctx)
    assert lib.e2v_image_classify(None, fp, U8CL, 1, 2, 8, 8, op, None, None, None) == _lib.E2V_EINVAL
    assert lib.e2v_finalize_weights(ctx, 16) == _lib.E2V_ESTATE and b"host-only" in lib.e2v_last_error(ctx)
    # the op entries: argument checks first, then the host-only refusal
    assert lib.e2v_op_image_attention(ctx, C.c_void_p(64), 384, C.c_void_p(64), 128, 1, 289, 2, None) == _lib.E2V_ESHAPE
    assert lib.e2v_op_image_attention(ctx, C.c_void_p(64), 384, C.c_void_p(64), 128, 1, 288, 2, None) == _lib.E2V_ESTATE
    assert lib.e2v_op_image_preprocess(ctx, fp, U8CL, 1, 2, 8, 8, 112, 9, None, C.c_void_p(64), None) == _lib.E2V_ESHAPE
    assert lib.e2v_op_image_preprocess(ctx, fp, U8CL, 1, 2, 8, 8, 112, 8, None, C.c_void_p(64), None) == _lib.E2V_ESTATE
    lib.e2v_destroy(ctx)


def test_image_weights_are_frozen_for_update_tensor(lib):
    st, ctx = host_ctx(lib, TINY_IMAGE)
    w = np.zeros((128,), np.float32)
    shape = (C.c_int64 * 1)(128)
    assert lib.e2v_update_tensor(ctx, b"image.vit.layernorm.weight", w.ctypes.data_as(C.c_void_p), _lib.E2V_F32, 0, shape, 1, None) == _lib.E2V_EINVAL
    assert b"frozen" in lib.e2v_last_error(ctx)
    lib.e2v_destroy(ctx)


def test_signatures_hold_the_new_entries(lib):
    for name in ("e2v_image_classify", "e2v_image_resize_table", "e2v_op_image_preprocess", "e2v_op_image_attention"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["e2v_image_classify"][1]) == 11 and len(_lib.SIGNATURES["e2v_image_resize_table"][1]) == 6


# ---- n_way_top_k_acc -------------------------------------------------------------------------------------------------------------
def reference_n_way_top_k_acc(pred, class_id, n_way, num_trials=40, top_k=1):
    """EEG2Video/40_class_run_metrics.py:57-70, line by line"""
    if isinstance(class_id, int):
        class_id = [class_id]
    pick_range = [i for i in np.arange(len(pred)) if i not in class_id]
    corrects = 0
    for t in range(num_trials):
        idxs_picked = np.random.choice(pick_range, n_way - 1, replace=False)
        for gt_id in class_id:
            pred_picked = torch.cat([pred[gt_id].unsqueeze(0), pred[idxs_picked]])
            pred_picked = pred_picked.argsort(descending=False)[-top_k:]
            if 0 in pred_picked:
                corrects += 1
                break
    return corrects / num_trials, np.sqrt(corrects / num_trials * (1 - corrects / num_trials) / num_trials)


@pytest.mark.parametrize("n_way,top_k", [(2, 1), (40, 1), (50, 1), (40, 3), (50, 3)])       # (2, 3) is no case: the metric asserts n_way > top_k
def test_n_way_top_k_acc_equals_the_reference_loop(n_way, top_k):
    from eeg2video_amd.metrics import n_way_top_k_acc
    g = torch.Generator().manual_seed(n_way * 10 + top_k)
    for trial in range(4):
        pred = torch.rand(60, generator=g, dtype=torch.float64).softmax(-1)       # distinct values: no ties for the reference's unstable argsort
        ids = [int(i) for i in torch.randperm(60, generator=g)[:3]]
        for class_id in (ids[0], ids):
            np.random.seed(trial)
            want = reference_n_way_top_k_acc(pred, class_id, n_way, 25, top_k)
            np.random.seed(trial)
            got = n_way_top_k_acc(pred, class_id, n_way, 25, top_k)
            assert got == want, (got, want)
            np.random.seed(trial)
            assert n_way_top_k_acc(pred.numpy(), torch.tensor(ids) if class_id is ids else class_id, n_way, 25, top_k) == want


def test_n_way_top_k_acc_closed_forms():
    from eeg2video_amd.metrics import n_way_top_k_acc
    pred = torch.linspace(0.0, 1.0, 50)
    np.random.seed(0)
    assert n_way_top_k_acc(pred, 49, 40, 30, 1) == (1.0, 0.0)                 # gt is the arg-max
    assert n_way_top_k_acc(pred, 0, 2, 30, 1) == (0.0, 0.0)                   # gt is the arg-min
    assert n_way_top_k_acc(pred, [0, 49, 7], 10, 30, 1)[0] == 1.0             # three ids: any of them counts
    assert n_way_top_k_acc(pred, [0, 1, 2], 10, 30, 1)[0] == 0.0
    assert n_way_top_k_acc(pred, 0, 2, 30, 2)[0] == 1.0                       # top 2 of 2
    acc, std = n_way_top_k_acc(pred, 25, 2, 400, 1)                           # the median against one distractor: about a half
    assert 0.35 < acc < 0.65 and std == pytest.approx(np.sqrt(acc * (1 - acc) / 400))
