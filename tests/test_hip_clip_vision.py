"""GPU: the CLIP vision tower and the CLIP score (``e2v_clip_embed``, ``e2v_clip_similarity``, ``csrc/clip.hip``) against
``transformers``, Pillow and torch.

References: the committed fixture (``tests/golden/clip_vision_tiny.npz``: ``transformers.CLIPVisionModelWithProjection`` embeddings of
8 images, Pillow's bicubic bytes after the centre crop, the processor's pixel table, ``F.cosine_similarity`` of the embeddings) for
the whole model; the integer restatement of Pillow's resize (``tests/clip_vision_restatement.py``, pinned to Pillow bit for bit on the
CPU) for the preprocess; the float64 cosine, computed on the spot, for the similarity op.

Whole-model tolerances are TEN TIMES what the CPU measures without the code under test -- the fixture's own fp32 values against the
float64 restatement, printed by ``tests/golden/make_clip_vision_golden.py`` (transformers 5.15, torch on the CPU):

* ``image_embeds``  1.023e-6 (max |a-b| / max |b|)  -> bound 1.03e-5
* pair scores       2.583e-7 (max |a-b|)            -> bound 2.6e-6
* matrix            4.682e-7 (max |a-b|)            -> bound 4.7e-6

The similarity op alone is held to the rounding of its own arithmetic: a dot of D products in four partial sums is off by at most
(D / 4 + 3) u times sum |a_d b_d| <= |a| |b| (u = 2^-24), each norm by half of that relatively, plus a square root and two divisions:
(D / 2 + 10) u in all -- 1.6e-5 at D = 512, 7.2e-7 at D = 4.
"""
import json
import os

import numpy as np
import pytest
import torch

from eeg2video_amd import _lib
from eeg2video_amd.engine import image_resize_table
from eeg2video_amd.weights import TINY_CLIP_VISION, TINY_UNET, TINY_VAE, clip_vision_param_spec, counter_normal
from clip_vision_restatement import (cosine64, golden_groups, load_golden, patch_rows, pixel_table, reference_n_way, rel_err,
                                     resize_crop_with_tables)
from test_hip_bounds import GUARD_KIB, environment, fenced, fenced_out, run_fenced

pytestmark = pytest.mark.gpu

EMB_BOUND, PAIR_BOUND, MATRIX_BOUND = 1.03e-5, 2.6e-6, 4.7e-6
C = TINY_CLIP_VISION
S, P, E, D = C.image_size, C.patch_size, C.resize_edge, C.projection_dim
bicubic = lambda i, o: image_resize_table(i, o, 3)


def make_engine():
    from eeg2video_amd.engine import Engine
    return Engine(TINY_UNET, TINY_VAE, 0, clip_vision_cfg=C)


def make_model(sd, engine=None):
    from eeg2video_amd.clip_vision import CLIPVisionModelWithProjection
    return CLIPVisionModelWithProjection(C, engine=engine or make_engine()).load_state_dict(sd)


@pytest.fixture(scope="module")
def golden():
    z, sd = load_golden()
    return {k: z[k] for k in z.files}, sd


@pytest.fixture(scope="module")
def model(golden):
    return make_model(golden[1])


@pytest.fixture(scope="module")
def cropped8(golden):
    """the 8 fixture images as Pillow resized and cropped them, ``[8,112,112,3]`` uint8, in the fixture's order (at 112 x 112 an
    image is its own resize and crop, so these go through the device's processor unchanged)"""
    return np.concatenate([cropped for _, cropped in golden_groups(golden[0])])


@pytest.fixture(scope="module")
def batch8(model, cropped8):
    """``image_embeds`` of the 8 cropped images in one call, on the host -- the result the other tests compare bits with"""
    return model.engine.clip_embed(torch.from_numpy(cropped8)[None], channels_last=True).cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


def as_kind(img_u8, f32, channels_last):
    """``[n,F,H,W,3]`` uint8 -> the same frames as uint8 / float32 in either layout; the float is the middle of the byte's bucket"""
    t = torch.from_numpy(np.ascontiguousarray(img_u8))
    if f32:
        t = (t.float() + 0.5) / 255.0
    return t if channels_last else t.permute(0, 4, 1, 2, 3).contiguous()


# ------------------------------------------------------------------ 1. preprocess ----------------------------------------------------
@pytest.mark.parametrize("group", range(3))
def test_preprocess_fixture_images_bit_for_bit(model, golden, group):
    z = golden[0]
    imgs, cropped = golden_groups(z)[group]
    want = np.concatenate([patch_rows(r, z["pixel_table"], P) for r in cropped])            # Pillow's bytes + the processor's table
    got = None
    for f32 in (False, True):
        for cl in (True, False):
            rows = model.engine.op_clip_preprocess(as_kind(imgs[:, None], f32, cl), size=S, patch=P, edge=E, channels_last=cl).cpu()
            assert rows.shape == (len(imgs) * (S // P) ** 2, 3 * P * P)
            if got is None:
                got = rows
                assert np.array_equal(rows.numpy().view(np.int32), want.view(np.int32)), int((rows.numpy() != want).sum())
            assert torch.equal(bits(rows), bits(got)), (f32, cl)                           # the four type / layout combinations agree


@pytest.mark.parametrize("h,w,edge,size,patch", [(288, 512, 224, 224, 32),    # the reference's frames at CLIP-B/32: 7 taps both ways
                                                 (512, 288, 224, 224, 32),    # the same on its side
                                                 (30, 20, 32, 32, 8),         # an upscale
                                                 (1300, 12, 16, 16, 8)])      # more than 100 times as tall as wide: vertical first
def test_preprocess_shapes_bit_for_bit(model, h, w, edge, size, patch):
    rng = np.random.default_rng(h + w)
    imgs = rng.integers(0, 256, (2, 3, h, w, 3), dtype=np.uint8)                           # 2 clips of 3 frames
    lut = pixel_table(1 / 255, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))               # per-channel values: a channel mix-up shows
    want = np.concatenate([patch_rows(resize_crop_with_tables(im, edge, size, bicubic), lut, patch) for im in imgs.reshape(6, h, w, 3)])
    for cl in (True, False):
        rows = model.engine.op_clip_preprocess(as_kind(imgs, False, cl), size=size, patch=patch, edge=edge, lut=lut, channels_last=cl).cpu().numpy()
        assert np.array_equal(rows.view(np.int32), want.view(np.int32)), (cl, int((rows != want).sum()))


def test_preprocess_filter_2_is_the_video_preprocess_and_bytes_at_odd_alignment(model):
    eng = model.engine
    rng = np.random.default_rng(3)
    flat = torch.from_numpy(rng.integers(0, 256, (1 + 2 * 19 * 31 * 3,), dtype=np.uint8)).cuda()
    view = flat[1:].view(1, 2, 19, 31, 3)                                                   # starts at an odd byte
    lut = pixel_table(1 / 255, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    a = eng.op_clip_preprocess(view, size=16, patch=8, edge=16, lut=lut, channels_last=True)
    b = eng.op_clip_preprocess(view.cpu().clone(), size=16, patch=8, edge=16, lut=lut, channels_last=True)
    assert torch.equal(bits(a), bits(b))
    want = np.concatenate([patch_rows(resize_crop_with_tables(im, 16, 16, bicubic), lut, 8) for im in view.cpu().numpy()[0]])
    assert np.array_equal(a.cpu().numpy().view(np.int32), want.view(np.int32))
    bil = eng.op_clip_preprocess(view, size=16, patch=8, edge=16, filter=2, lut=lut, channels_last=True)
    vid = eng.op_video_preprocess(view, size=16, patch=8, tubelet=1, edge=16, lut=lut, channels_last=True)
    assert torch.equal(bits(bil), bits(vid)) and not torch.equal(bits(bil), bits(a))
    with pytest.raises(ValueError):                                                         # E2V_EINVAL: LANCZOS
        eng.op_clip_preprocess(view, size=16, patch=8, edge=16, filter=1, lut=lut, channels_last=True)


# ------------------------------------------------------------------ 2. the similarity op ---------------------------------------------
def sim_bound(d):
    return (d / 2 + 10) * 2.0 ** -24


@pytest.mark.parametrize("d", [4, 64, 260, 512])
def test_op_clip_similarity(model, d):
    eng = model.engine
    for na in (1, 3, 65):
        for nb in (1, 3, 65):
            a = torch.from_numpy(counter_normal(7 * na + d, "sim_a", (na, d)))
            b = torch.from_numpy(counter_normal(11 * nb + d, "sim_b", (nb, d))) * 3.0 + 0.25 * a[0]
            if na == 3:
                a[1] = 0.0                                                                  # a zero row: 0, not NaN
            m = eng.clip_similarity(a, b, matrix=True).cpu()
            err = float(np.abs(m.double().numpy() - cosine64(a.numpy(), b.numpy(), matrix=True)).max())
            assert m.shape == (na, nb) and not torch.isnan(m).any() and err <= sim_bound(d), (na, nb, err)
            if na == 3:
                assert (m[1] == 0).all()
            # pairs of every (i, j) carry the bits of the matrix
            ii, jj = np.divmod(np.arange(na * nb), nb)
            p = eng.clip_similarity(a[ii], b[jj]).cpu()
            assert p.shape == (na * nb,) and torch.equal(bits(p), bits(m.reshape(-1))), (na, nb)
    print(f"D={d}: bound {sim_bound(d):.2e}")


def test_op_clip_similarity_at_the_reference_size_and_a_tiny_norm(model):
    """1200 x 1200 x 512 is the frame-level use (200 clips x 6 frames a side); a row whose norm is below eps is divided by eps"""
    eng = model.engine
    a = torch.from_numpy(counter_normal(1, "sim_big_a", (1200, 512)))
    b = torch.from_numpy(counter_normal(2, "sim_big_b", (1200, 512))) + 0.5 * a
    m = eng.clip_similarity(a, b, matrix=True).cpu()
    err = float(np.abs(m.double().numpy() - cosine64(a.numpy(), b.numpy(), matrix=True)).max())
    print(f"1200 x 1200 x 512: max |a-b| = {err:.3e} (bound {sim_bound(512):.2e})")
    assert err <= sim_bound(512)
    assert torch.equal(bits(eng.clip_similarity(a, b).cpu()), bits(torch.diagonal(m)))
    tiny = torch.full((1, 4), 1e-10)
    got = eng.clip_similarity(tiny, torch.full((1, 4), 1e-3)).item()
    want = torch.nn.functional.cosine_similarity(tiny.double(), torch.full((1, 4), 1e-3).double(), dim=-1).item()
    assert abs(got - want) <= 1e-6 * want and got < 0.1                                      # 2e-10 / 1e-8: not 1
    with pytest.raises(ValueError):
        eng.clip_similarity(a[:, :510], b[:, :510])                                         # D not a multiple of 4
    with pytest.raises(ValueError):
        eng.clip_similarity(a[:5], b[:4])


@pytest.mark.parametrize("matrix", [False, True])
def test_op_clip_similarity_fenced(model, matrix):
    eng = model.engine
    na, nb, d = (17, 17, 260) if not matrix else (17, 33, 260)
    a, b = torch.from_numpy(counter_normal(3, "sim_fa", (na, d))), torch.from_numpy(counter_normal(4, "sim_fb", (nb, d)))
    fa, fb, fo = fenced(a, name="a"), fenced(b, name="b"), fenced_out((na, nb) if matrix else (1, na))

    def call():
        st = eng.lib.e2v_clip_similarity(eng.ctx, fa.t.data_ptr(), na, fb.t.data_ptr(), nb, d, int(matrix), fo.t.data_ptr(), None)
        assert st == 0, eng.lib.e2v_last_error(eng.ctx)
    y = run_fenced(call, [fa, fb], fo).cpu()
    want = cosine64(a.numpy(), b.numpy(), matrix=matrix)
    assert float(np.abs(y.double().numpy().reshape(want.shape) - want).max()) <= sim_bound(d)


# ------------------------------------------------------------------ 3. the whole model ----------------------------------------------
def test_whole_model_vs_the_transformers_fixture(model, golden, batch8):
    z = golden[0]
    eng = model.engine
    err = rel_err(batch8, z["image_embeds"])
    pairs = eng.clip_similarity(batch8, batch8.roll(1, 0)).cpu().numpy()
    matrix = eng.clip_similarity(batch8, batch8, matrix=True).cpu().numpy()
    perr = float(np.abs(pairs.astype(np.float64) - z["pair_scores"]).max())
    merr = float(np.abs(matrix.astype(np.float64) - z["matrix"]).max())
    print(f"HIP vs transformers {z['transformers_version']}: image_embeds max|a-b|/max|b| = {err:.3e} (bound {EMB_BOUND:.2e}), "
          f"pair scores {perr:.3e} (bound {PAIR_BOUND:.1e}), matrix {merr:.3e} (bound {MATRIX_BOUND:.1e})")
    assert batch8.shape == (8, D) and batch8.dtype == torch.float32 and not torch.isnan(batch8).any() and err < EMB_BOUND, err
    assert perr < PAIR_BOUND and merr < MATRIX_BOUND, (perr, merr)
    assert np.array_equal(np.argsort(matrix, -1), np.argsort(z["matrix"], -1))              # every row ranks as the fixture ranks it


def test_original_shapes_give_the_bits_of_pillows_bytes(model, golden, batch8):
    """each group at its own size: the preprocess is Pillow's bit for bit, so the model sees the same patch rows as for the cropped bytes"""
    i0 = 0
    for imgs, _ in golden_groups(golden[0]):
        out = model.engine.clip_embed(torch.from_numpy(imgs)[:, None], channels_last=True)  # n clips of one frame
        assert torch.equal(bits(out.cpu()), bits(batch8[i0:i0 + len(imgs)]))
        i0 += len(imgs)


# ------------------------------------------------------------------ 4. determinism ---------------------------------------------------
def test_an_image_does_not_depend_on_batch_chunk_or_mode(model, cropped8, batch8):
    eng = model.engine
    frames = torch.from_numpy(cropped8)

    def same(out, rows, what):
        assert torch.equal(bits(out.cpu()), bits(batch8[rows])), what

    same(eng.clip_embed(frames[None], channels_last=True), slice(0, 8), "a second run")
    for i in (0, 5, 7):
        same(eng.clip_embed(frames[i][None, None], channels_last=True), slice(i, i + 1), f"image {i} alone")
    same(eng.clip_embed(frames.view(2, 4, S, S, 3), channels_last=True), slice(0, 8), "2 clips of 4 frames")
    planar = frames.view(2, 4, S, S, 3).permute(0, 4, 1, 2, 3).contiguous()
    try:
        eng.set_knob("E2V_CLIPV_CHUNK", 3)                                                  # chunks of 3, 3 and 2 images: across the clips
        same(eng.clip_embed(frames[None], channels_last=True), slice(0, 8), "chunks of 3")
        same(eng.clip_embed(planar), slice(0, 8), "chunks of 3, planar clips of 4")
    finally:
        eng.set_knob("E2V_CLIPV_CHUNK", 256)
    for mode in ("bf16", "fp16"):
        try:
            eng.set_compute_dtype(mode)
            same(eng.clip_embed(frames[None], channels_last=True), slice(0, 8), mode)
        finally:
            eng.set_compute_dtype("fp32")
    videos = as_kind(cropped8[None], True, False).cuda()                                    # [n,3,F,H,W] floats in [0,1]: what e2v_generate leaves
    same(eng.clip_embed(videos), slice(0, 8), "planar floats")


# ------------------------------------------------------------------ 5. the Python layer ----------------------------------------------
def write_checkpoint(path, sd, safe, full=False):
    os.makedirs(path, exist_ok=True)
    vision = {"hidden_size": C.hidden, "num_attention_heads": C.heads, "num_hidden_layers": C.layers, "intermediate_size": C.intermediate,
              "image_size": C.image_size, "patch_size": C.patch_size, "hidden_act": C.hidden_act, "layer_norm_eps": C.layer_norm_eps,
              "num_channels": 3}
    if full:
        config = {"architectures": ["CLIPModel"], "model_type": "clip", "projection_dim": C.projection_dim, "vision_config": vision,
                  "text_config": {"hidden_size": 64, "num_attention_heads": 1}}
    else:
        config = dict(vision, architectures=["CLIPVisionModelWithProjection"], model_type="clip_vision_model", projection_dim=C.projection_dim)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(config, f)
    with open(os.path.join(path, "preprocessor_config.json"), "w") as f:
        json.dump({"crop_size": {"height": C.image_size, "width": C.image_size}, "do_center_crop": True, "do_convert_rgb": True,
                   "do_normalize": True, "do_rescale": True, "do_resize": True, "image_mean": list(C.image_mean), "image_std": list(C.image_std),
                   "image_processor_type": "CLIPImageProcessor", "resample": 3, "rescale_factor": 1 / 255,
                   "size": {"shortest_edge": C.resize_edge}}, f)
    tensors = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}
    tensors["vision_model.embeddings.position_ids"] = torch.arange(C.tokens)[None]          # older checkpoints carry the buffer
    if full:                                                                                # and a full CLIP checkpoint its text side
        tensors["text_model.embeddings.position_ids"] = torch.arange(4)[None]
        tensors["text_projection.weight"] = torch.zeros(C.projection_dim, 64)
        tensors["logit_scale"] = torch.tensor(2.6592)
    if safe:
        from safetensors.torch import save_file
        save_file(tensors, os.path.join(path, "model.safetensors"))
    else:
        torch.save(tensors, os.path.join(path, "pytorch_model.bin"))


@pytest.mark.parametrize("full,safe", [(False, True), (False, False), (True, True), (True, False)])
def test_from_pretrained_round_trips(model, golden, cropped8, batch8, tmp_path, full, safe):
    from eeg2video_amd.clip_vision import CLIPVisionModelWithProjection
    sd = golden[1]
    d = str(tmp_path / "clip")
    write_checkpoint(d, sd, safe, full)
    m = CLIPVisionModelWithProjection.from_pretrained(d, engine=model.engine)              # (the same config: the engine is reused)
    assert m.ccfg == C and m.config.projection_dim == D
    out = m(torch.from_numpy(cropped8))                                                     # [8,112,112,3]: 8 frames of one clip
    assert out[0] is out.image_embeds and torch.equal(bits(out.image_embeds.cpu()), bits(batch8))
    assert torch.equal(bits(m(cropped8[3]).image_embeds.cpu()), bits(batch8[3:4]))          # one [h,w,3] image, as clip_score hands it over
    back = m.state_dict(device="cpu")
    assert list(back) == list(clip_vision_param_spec(C))
    for k, v in back.items():
        assert v.dtype == torch.float32 and np.array_equal(v.numpy(), sd[k]), k            # the loaded bits, fused tensors included
    d2 = str(tmp_path / "again")
    m.save_pretrained(d2, safe_serialization=safe)
    assert CLIPVisionModelWithProjection.config_from_dir(d2) == C
    assert os.path.isfile(os.path.join(d2, "model.safetensors" if safe else "pytorch_model.bin"))
    again = CLIPVisionModelWithProjection.from_pretrained(d2, engine=model.engine)
    assert torch.equal(bits(again(cropped8[:2]).image_embeds.cpu()), bits(batch8[:2]))


def test_keys_update_read_and_absence(golden, cropped8, batch8):
    from eeg2video_amd.engine import Engine
    sd = golden[1]
    m = make_model(sd)
    eng = m.engine
    with pytest.raises(RuntimeError, match="unexpected"):                                   # E2V_ENOWEIGHT: a buffer is not a weight
        eng.load_state_dict({"vision_model.embeddings.position_ids": torch.zeros(1, C.tokens)}, prefix="clipv.")
    with pytest.raises(RuntimeError, match="unexpected"):
        eng.load_state_dict({"visual_projection.bias": torch.zeros(D)}, prefix="clipv.")
    assert eng.weight_forms("clipv.vision_model.encoder.layers.0.self_attn.q_proj.weight") == 1          # fp32 only
    assert eng.weight_forms("clipv.visual_projection.weight") == 1
    frames = torch.from_numpy(cropped8[:2])[None]
    # update_tensor then read_tensor on clipv. keys: a fused projection, a norm affine, the bias-free patch matrix
    for key in ("vision_model.encoder.layers.1.self_attn.k_proj.weight", "vision_model.pre_layrnorm.bias",
                "vision_model.embeddings.patch_embedding.weight", "visual_projection.weight"):
        new = torch.from_numpy(sd[key]) * 0.5 + 0.125
        m.sync_from({key: new, "text_model.final_layer_norm.weight": torch.ones(3)})        # (names the tower does not have are ignored)
        assert torch.equal(bits(m.state_dict(device="cpu")[key]), bits(new)), key
        moved = eng.clip_embed(frames, channels_last=True).cpu()
        assert not torch.equal(bits(moved), bits(batch8[:2])), key
        m.sync_from({key: torch.from_numpy(sd[key])})
        assert torch.equal(bits(eng.clip_embed(frames, channels_last=True).cpu()), bits(batch8[:2])), key
    plain = Engine(TINY_UNET, TINY_VAE, 0)
    with pytest.raises(RuntimeError, match="without a CLIP vision tower"):
        plain.clip_embed(torch.zeros(1, 1, 8, 8, 3, dtype=torch.uint8), channels_last=True)
    with pytest.raises(RuntimeError, match="no CLIP vision tower"):
        plain.finalize(plain.CLIP_VISION)
    with pytest.raises(ValueError):
        plain.finalize(128)
    assert plain.clip_similarity(batch8, batch8).shape == (8,)                              # the score needs no tower


def test_clip_scores_equal_the_cpu_route(model, golden, cropped8, batch8):
    """``clip_score``, ``clip_score_only`` and ``n_way_scores`` against the seeded CPU route through the fixture's embeddings: the
    reference's loop over the device's own pair scores gives the same list, and over the fixture's scores too (the fixture's rows have
    gaps of 1e-3, the scores agree to 4.7e-6, so every comparison falls the same way)"""
    from eeg2video_amd.metrics import clip_score, clip_score_only, n_way_scores
    z = golden[0]
    eng = model.engine
    calc = clip_score(model=model)
    s03 = calc(cropped8[0], cropped8[3])
    assert isinstance(s03, float) and abs(s03 - float(z["matrix"][0, 3])) < MATRIX_BOUND
    assert s03 == eng.clip_similarity(batch8[0:1], batch8[3:4]).item()
    pred, gt = cropped8, np.roll(cropped8, 1, 0)
    got = clip_score_only(pred, gt, model=model)
    assert abs(got - float(np.mean(z["pair_scores"].astype(np.float64)))) < PAIR_BOUND
    assert got == np.mean([float(v) for v in eng.clip_similarity(batch8, batch8.roll(1, 0)).cpu().numpy()])
    fixture = z["matrix"][:, np.roll(np.arange(8), 1)]                                      # [i][j]: pred i against gt j = image j - 1
    device = eng.clip_similarity(batch8, batch8.roll(1, 0), matrix=True).cpu().numpy()
    for n_way, top_k, trials in ((2, 1, 10), (5, 1, 6), (8, 3, 4)):
        np.random.seed(9)
        got = n_way_scores(pred, gt, n_way=n_way, top_k=top_k, num_trials=trials, model=model)
        for m in (device, fixture):
            np.random.seed(9)
            want = reference_n_way(list(range(8)), list(range(8)), lambda p, g: float(m[p, g]), n_way, top_k, trials)
            assert got == want, (n_way, top_k)
    np.random.seed(6)
    assert n_way_scores(pred, pred, n_way=4, num_trials=5, model=model) == [1.0] * 8        # an image against itself scores 1: the largest
    with pytest.raises(RuntimeError, match="never\\s+reads the network"):
        clip_score_only(pred, gt, cache_dir="openai/clip-vit-base-patch32")


def test_sweep_scored_with_a_clip_model(golden, tmp_path, capsys):
    """``examples/run_sweep.py --score-against DIR --clip-model DIR``: a sweep scored against its own frames"""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "run_sweep.py")
    spec = importlib.util.spec_from_file_location("e2v_sweep_clip", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    clip_dir, out = str(tmp_path / "clip"), str(tmp_path / "clips")
    write_checkpoint(clip_dir, golden[1], True)
    common = ["--tiny", "--concepts", "2", "--per-concept", "1", "--batch", "2", "--steps", "2"]
    mod.main(common + ["--out", out, "--npy"])
    capsys.readouterr()
    mod.main(common + ["--score-against", out, "--clip-model", clip_dir])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert abs(rec["clip_score_mean"] - 1.0) < 1e-6 and 0.0 <= rec["clip_2way_acc"] <= 1.0 and "clip_40way_acc" not in rec      # 6 frames
    assert rec["ssim_mean"] == 1 and rec["stage_seconds_rank0"]["score"] > 0
    with pytest.raises(SystemExit):
        mod.main(common + ["--clip-model", clip_dir])


# ------------------------------------------------------------------ 6. bounds --------------------------------------------------------
def test_outputs_fenced_and_pool_guarded(golden, cropped8, batch8):
    """one call with E2V_POOL_GUARD on and a fenced output: no store outside a tensor, inside the library or out of it"""
    frames = torch.from_numpy(cropped8[:5]).cuda()
    with environment({}, GUARD_KIB):
        m = make_model(golden[1])
        eng = m.engine
        eng.pool_guard_report()
        emb, sim = fenced_out((5, D)), fenced_out((5, 5))
        gets = eng.pool_gets()

        def call():
            st = eng.lib.e2v_clip_embed(eng.ctx, frames.data_ptr(), _lib.E2V_FRAMES_U8 | _lib.E2V_FRAMES_CHANNELS_LAST, 1, 5, S, S,
                                        emb.t.data_ptr(), None)
            assert st == 0, eng.lib.e2v_last_error(eng.ctx)
        y = run_fenced(call, [], emb)
        taken = eng.pool_gets() - gets
        checked, violations, text = eng.pool_guard_report()
        assert violations == 0, text
        assert taken > 0 and checked >= taken, (checked, taken)
        assert torch.equal(bits(y.cpu()), bits(batch8[:5]))
        src = y.contiguous()

        def call2():
            st = eng.lib.e2v_clip_similarity(eng.ctx, src.data_ptr(), 5, src.data_ptr(), 5, D, 1, sim.t.data_ptr(), None)
            assert st == 0, eng.lib.e2v_last_error(eng.ctx)
        run_fenced(call2, [], sim)
        assert eng.pool_guard_report()[1] == 0


def test_steady_state_takes_no_new_memory(model, cropped8):
    eng, frames = model.engine, torch.from_numpy(cropped8[None]).cuda()
    a = eng.clip_embed(frames, channels_last=True)
    torch.cuda.synchronize()
    g0, bytes0 = eng.pool_gets(), eng.device_bytes()
    eng.clip_embed(frames, channels_last=True)
    g1 = eng.pool_gets()
    eng.clip_embed(frames, channels_last=True)
    eng.clip_similarity(a, a, matrix=True)
    torch.cuda.synchronize()
    assert eng.pool_gets() - g1 == g1 - g0 > 0 and eng.device_bytes() == bytes0
