"""CPU: the 16-bit mode of the metric towers without a GPU -- the new symbols, ``e2v_set_tower_dtype``'s argument validation on a
host-only context, the fixture of the torch-CPU 16-bit runs (``tests/golden/metric_towers_16bit.npz``) against the fp32 fixtures, and
the ranking rules of ``tests/metric_dtype_rules.py`` applied to those CPU runs themselves.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from eeg2video_amd import _lib
from eeg2video_amd.engine import clip_vision_config, fill_image_config, fill_video_config
from eeg2video_amd.weights import TINY_CLIP_VISION, TINY_IMAGE, TINY_VIDEO
from metric_dtype_rules import DTYPES, TOWERS, bound, check_row_ranking, check_top3, cpu_distance, load16, load32, top3_ascending

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("e2v_set_tower_dtype", "e2v_tower_dtype", "e2v_op_tower_preprocess", "e2v_op_tower_attention", "e2v_op_tower_token_mean",
       "e2v_op_tower_layernorm", "e2v_op_tower_activation", "e2v_op_tower_embed")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def z16():
    return load16()


def host_ctx(lib, image=False, video=False, clip=False):
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    if image:
        fill_image_config(cfg, TINY_IMAGE)
    if video:
        fill_video_config(cfg, TINY_VIDEO)
    ctx = C.c_void_p()
    if clip:
        vc = clip_vision_config(TINY_CLIP_VISION)
        assert lib.e2v_create_clip_vision(C.byref(cfg), C.byref(vc), -1, C.byref(ctx)) == 0, lib.e2v_last_error(None)
    else:
        assert lib.e2v_create(C.byref(cfg), -1, C.byref(ctx)) == 0, lib.e2v_last_error(None)
    return ctx


def test_new_symbols_are_declared_exported_and_bound(lib):
    text = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("eeg2video_hip.h", "eeg2video_hip_ops.h"))
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name + " is not declared"
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None, name


def test_set_tower_dtype_validates_on_a_host_only_context(lib):
    """no HIP call is made: what is wrong with the arguments, and a tower the context does not have, are answered without a GPU"""
    full = host_ctx(lib, image=True, video=True, clip=True)
    try:
        for part in (16, 32, 64):
            assert lib.e2v_tower_dtype(full, part) == _lib.E2V_F32                           # the default
            for dt in (_lib.E2V_BF16, _lib.E2V_F16, _lib.E2V_BF16, _lib.E2V_F32):            # repeatedly, and back
                assert lib.e2v_set_tower_dtype(full, part, dt) == _lib.E2V_OK
                assert lib.e2v_tower_dtype(full, part) == dt
            assert lib.e2v_set_tower_dtype(full, part, _lib.E2V_F32X3) == _lib.E2V_EINVAL
            assert lib.e2v_set_tower_dtype(full, part, 99) == _lib.E2V_EINVAL
            assert lib.e2v_tower_dtype(full, part) == _lib.E2V_F32                           # a refused call changes nothing
        lib.e2v_set_tower_dtype(full, 16, _lib.E2V_F16)                                      # one tower's mode is its own
        assert [lib.e2v_tower_dtype(full, p) for p in (16, 32, 64)] == [_lib.E2V_F16, _lib.E2V_F32, _lib.E2V_F32]
        for part in (8, 1, 2, 4, 0, 48, 128, -16):                                           # the text encoder stays fp32
            assert lib.e2v_set_tower_dtype(full, part, _lib.E2V_F16) == _lib.E2V_EINVAL, part
            assert lib.e2v_tower_dtype(full, part) == -1
        assert b"16" in lib.e2v_last_error(full) and b"64" in lib.e2v_last_error(full)
        assert lib.e2v_set_tower_dtype(None, 16, _lib.E2V_F16) == _lib.E2V_EINVAL and lib.e2v_tower_dtype(None, 16) == -1
    finally:
        lib.e2v_destroy(full)
    bare = host_ctx(lib)
    only_image = host_ctx(lib, image=True)
    try:
        for part in (16, 32, 64):
            assert lib.e2v_set_tower_dtype(bare, part, _lib.E2V_F16) == _lib.E2V_ESTATE, part
            assert b"no such tower" in lib.e2v_last_error(bare)
        assert lib.e2v_set_tower_dtype(only_image, 16, _lib.E2V_BF16) == _lib.E2V_OK
        assert lib.e2v_set_tower_dtype(only_image, 32, _lib.E2V_BF16) == _lib.E2V_ESTATE
        assert lib.e2v_set_tower_dtype(only_image, 64, _lib.E2V_BF16) == _lib.E2V_ESTATE
        assert lib.e2v_set_tower_dtype(only_image, 8, _lib.E2V_BF16) == _lib.E2V_EINVAL       # the argument check comes first
    finally:
        lib.e2v_destroy(bare)
        lib.e2v_destroy(only_image)


def test_the_engines_compute_dtype_does_not_reach_a_tower(lib):
    ctx = host_ctx(lib, image=True)
    try:
        assert lib.e2v_set_compute_dtype(ctx, _lib.E2V_F16) == _lib.E2V_OK
        assert lib.e2v_tower_dtype(ctx, 16) == _lib.E2V_F32
        assert lib.e2v_set_tower_dtype(ctx, 16, _lib.E2V_BF16) == _lib.E2V_OK
        assert lib.e2v_set_compute_dtype(ctx, _lib.E2V_F32) == _lib.E2V_OK
        assert lib.e2v_tower_dtype(ctx, 16) == _lib.E2V_BF16
    finally:
        lib.e2v_destroy(ctx)


def test_mirrors_have_the_setter_and_from_pretrained_takes_the_keyword():
    import inspect

    from eeg2video_amd.clip_vision import CLIPVisionModelWithProjection
    from eeg2video_amd.engine import Engine
    from eeg2video_amd.image_classifier import ViTForImageClassification
    from eeg2video_amd.video_classifier import VideoMAEForVideoClassification
    for cls in (ViTForImageClassification, VideoMAEForVideoClassification, CLIPVisionModelWithProjection):
        assert callable(cls.set_compute_dtype) and isinstance(cls.compute_dtype, property)
        assert "compute_dtype" in inspect.signature(cls.from_pretrained).parameters
    assert callable(Engine.set_tower_dtype) and callable(Engine.tower_dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tower", sorted(TOWERS))
def test_fixture_16bit_runs_stay_in_the_stated_neighbourhood(z16, tower, dtype):
    """each stored 16-bit result: its distance from the fp32 fixture is the one the file states, and inside the neighbourhood it states"""
    z32 = load32(tower)
    for q in TOWERS[tower][1]:
        name = f"{tower}_{q}_{dtype}"
        dist = cpu_distance(z16, z32, tower, q, dtype)
        print(f"{name}: max |16-bit - fp32| = {dist:.3e}, stated neighbourhood {float(z16['near_' + name]):.3e}, device bound {bound(z16, z32, tower, q, dtype):.3e}")
        assert z16[name].dtype == np.float32 and z16[name].shape == z32[TOWERS[tower][1][q]].shape
        assert np.float32(dist) == z16["dist_" + name]
        assert 0.0 < dist <= float(z16["near_" + name])
    if tower != "clip":                                                         # probabilities of a row still sum to 1 within the format
        u = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}[dtype]
        assert np.abs(z16[f"{tower}_probs_{dtype}"].sum(-1) - 1.0).max() <= 50 * u


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tower", ["vit", "videomae"])
def test_top3_rule_passes_on_the_cpu_16bit_runs(z16, tower, dtype):
    """the torch-CPU 16-bit logits are within 1 x their own distance of fp32, so they have to pass the rule the device is held to at
    4 x; in fp16 they give the fixture's ORDERED top 3 on all 8 rows and the rule determines the top-3 set of every row"""
    z32 = load32(tower)
    b = bound(z16, z32, tower, "logits", dtype)
    got = top3_ascending(z16[f"{tower}_logits_{dtype}"])
    determined = check_top3(got, z32["logits"], b, f"{tower} {dtype}")
    srt = np.sort(z32["logits"], -1)
    print(f"{tower} {dtype}: 2 x bound = {2 * b:.3e}, smallest 3rd-4th gap {float((srt[:, -3] - srt[:, -4]).min()):.3e}, top-3 set determined in {determined} of 8 rows")
    if dtype == "fp16":                                                         # (bf16 logits tie: 8 bits of mantissa at a scale of 4)
        assert np.array_equal(got, top3_ascending(z32["logits"]))
        assert determined == 8
    with pytest.raises(AssertionError):                                         # the rule is not vacuous: a foreign label fails it
        worst = np.argsort(z32["logits"], -1)[:, :1]
        check_top3(np.concatenate([worst, got[:, 1:]], -1), z32["logits"], b)
    with pytest.raises(AssertionError):                                         # nor is the order: the largest listed below the third
        check_top3(got[:, ::-1], z32["logits"], bound(z16, z32, tower, "logits", "fp16"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_clip_ranking_rule_passes_on_the_cpu_16bit_runs(z16, dtype):
    z32 = load32("clip")
    b = bound(z16, z32, "clip", "matrix", dtype)
    fixed, total = check_row_ranking(z16[f"clip_matrix_{dtype}"], z32["matrix"], b, f"clip {dtype}")
    gaps = np.diff(np.sort(z32["matrix"], -1), axis=-1)
    print(f"clip {dtype}: 2 x bound = {2 * b:.3e}, smallest sorted gap {float(gaps.min()):.3e}, {fixed} of {total} column pairs determined")
    assert fixed > 0
    if dtype == "fp16":
        assert fixed >= 0.9 * total                                             # nearly all pairs are determined
    with pytest.raises(AssertionError):
        check_row_ranking(-z16[f"clip_matrix_{dtype}"], z32["matrix"], b)
