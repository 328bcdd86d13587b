"""GPU: the ViT image classifier (``e2v_image_classify``, ``csrc/vit.hip``) against ``transformers`` and Pillow.

References: the committed fixture (``tests/golden/vit_tiny.npz``: ``transformers.ViTForImageClassification`` logits of 8 images,
Pillow's resized bytes, the processor's pixel table) for the whole model; the integer restatement of Pillow's resize
(``tests/vit_restatement.py``, pinned to Pillow bit for bit on the CPU) for the preprocess; ``torch.softmax(q k^T / 8) v`` in float64,
computed on the spot, for the attention op.  Metric and bound for fp32 arithmetic: max |a-b| / max |b| < 1e-5, as ``tests/test_hip_text.py``;
the float64 restatement itself sits 5.4e-7 from the fixture's fp32 logits (``tests/test_image_classifier_host.py`` prints it).
"""
import json
import os

import numpy as np
import pytest
import torch

from eeg2video_amd import _lib
from eeg2video_amd.engine import image_resize_table
from eeg2video_amd.weights import TINY_IMAGE, TINY_UNET, TINY_VAE, _VIT_V5_NAMES, counter_normal, image_param_spec
from test_hip_bounds import GUARD_KIB, PADS, environment, fenced, fenced_out, run_fenced
from test_image_classifier_host import reference_n_way_top_k_acc
from vit_restatement import load_golden, patch_rows, pixel_table, rel_err, resize_with_tables, softmax64, top3

pytestmark = pytest.mark.gpu

BOUND = 1e-5
GROUPS = ("36x64", "130x90", "112x112")
S, P = TINY_IMAGE.image_size, TINY_IMAGE.patch_size


def make_engine():
    from eeg2video_amd.engine import Engine
    return Engine(TINY_UNET, TINY_VAE, 0, image_cfg=TINY_IMAGE)


def make_classifier(sd, engine=None):
    from eeg2video_amd.image_classifier import ViTForImageClassification
    return ViTForImageClassification(TINY_IMAGE, engine=engine or make_engine()).load_state_dict(sd)


@pytest.fixture(scope="module")
def golden():
    z, sd = load_golden()
    return {k: z[k] for k in z.files}, sd


@pytest.fixture(scope="module")
def clf(golden):
    return make_classifier(golden[1])


@pytest.fixture(scope="module")
def resized8(golden):
    """the 8 fixture images as Pillow resized them, ``[8,112,112,3]`` uint8, in the fixture's order"""
    z = golden[0]
    return np.concatenate([z["resized_36x64"], z["resized_130x90"], z["images_112x112"]])


@pytest.fixture(scope="module")
def batch8(clf, resized8):
    """(logits, probs, top3) of the 8 resized images in one call, on the host -- the reference result the other tests compare bits with"""
    out = clf.engine.classify_frames(torch.from_numpy(resized8)[None], channels_last=True)
    return tuple(t.cpu() for t in out)


def bits(t):
    return t.contiguous().view(torch.int32)


def as_kind(img_u8, f32, channels_last):
    """``[n,F,H,W,3]`` uint8 -> the same frames as uint8 / float32 in either layout; the float is the middle of the byte's bucket"""
    t = torch.from_numpy(np.ascontiguousarray(img_u8))
    if f32:
        t = (t.float() + 0.5) / 255.0
    return t if channels_last else t.permute(0, 4, 1, 2, 3).contiguous()


# ------------------------------------------------------------------ 1. preprocess ----------------------------------------------------
def expected_rows(imgs, size, patch, lut):
    return np.concatenate([patch_rows(resize_with_tables(im, size, image_resize_table), lut, patch) for im in imgs])


@pytest.mark.parametrize("group", GROUPS)
def test_preprocess_fixture_images_bit_for_bit(clf, golden, group):
    z = golden[0]
    imgs = z["images_" + group]
    resized = z["resized_" + group] if "resized_" + group in z else imgs
    want = np.concatenate([patch_rows(r, z["pixel_table"], P) for r in resized])            # Pillow's bytes + the processor's table
    got = None
    for f32 in (False, True):
        for cl in (True, False):
            rows = clf.engine.op_image_preprocess(as_kind(imgs[:, None], f32, cl), size=S, patch=P, channels_last=cl).cpu()
            assert rows.shape == (len(imgs) * (S // P) ** 2, 3 * P * P)
            if got is None:
                got = rows
                assert np.array_equal(rows.numpy().view(np.int32), want.view(np.int32)), int((rows.numpy() != want).sum())
            assert torch.equal(bits(rows), bits(got)), (f32, cl)                           # the four type / layout combinations agree


@pytest.mark.parametrize("h,w,size,patch", [(288, 512, 224, 16),       # the reference's frames at ViT-B/16: 7 taps across, 5 down
                                            (30, 20, 32, 8),           # an upscale
                                            (260, 2, 16, 8),           # more than 100 times as tall as wide: Pillow's vertical-first order
                                            (6000, 60, 112, 8)])       # a band of 8 output rows does not fit LDS: narrower bands
def test_preprocess_shapes_bit_for_bit(clf, h, w, size, patch):
    rng = np.random.default_rng(h + w)
    imgs = rng.integers(0, 256, (2, 3, h, w, 3), dtype=np.uint8)                           # 2 clips of 3 frames
    lut = pixel_table(1 / 255, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))               # per-channel values: a channel mix-up shows
    want = expected_rows(imgs.reshape(6, h, w, 3), size, patch, lut)
    try:
        from vit_restatement import pillow_resize
        assert np.array_equal(pillow_resize(imgs[0, 0], size), resize_with_tables(imgs[0, 0], size, image_resize_table))
    except ImportError:
        pass
    for cl in (True, False):
        rows = clf.engine.op_image_preprocess(as_kind(imgs, False, cl), size=size, patch=patch, lut=lut, channels_last=cl).cpu().numpy()
        assert np.array_equal(rows.view(np.int32), want.view(np.int32)), (cl, int((rows != want).sum()))


def test_preprocess_reads_bytes_at_any_alignment_and_quantises_floats(clf):
    rng = np.random.default_rng(3)
    flat = torch.from_numpy(rng.integers(0, 256, (1 + 2 * 9 * 11 * 3,), dtype=np.uint8)).cuda()
    view = flat[1:].view(1, 2, 9, 11, 3)                                                   # starts at an odd byte
    a = clf.engine.op_image_preprocess(view, size=16, patch=8, channels_last=True)
    b = clf.engine.op_image_preprocess(view.cpu().clone(), size=16, patch=8, channels_last=True)
    assert torch.equal(bits(a), bits(b))
    x = torch.tensor([-1.0, 0.0, 0.5, 1.0, 2.0, float("nan")]).view(1, 1, 1, 6, 1).repeat(1, 1, 1, 1, 3)       # one row of 6 pixels
    q = torch.tensor([0, 0, 127, 255, 255, 0], dtype=torch.uint8).view(1, 1, 1, 6, 1).repeat(1, 1, 1, 1, 3)    # clamp, truncate, NaN -> 0
    assert torch.equal(bits(clf.engine.op_image_preprocess(x, size=8, patch=8, channels_last=True)),
                       bits(clf.engine.op_image_preprocess(q, size=8, patch=8, channels_last=True)))


# ------------------------------------------------------------------ 2. attention -----------------------------------------------------
def attention_ref(qkv, b, t, heads):
    q, k, v = (x.double().view(b, t, heads, 64).transpose(1, 2) for x in qkv.chunk(3, dim=-1))
    return (torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v).transpose(1, 2).reshape(b * t, heads * 64)


@pytest.mark.parametrize("t", [1, 17, 50, 64, 65, 128, 129, 197, 257])
def test_op_image_attention(clf, t):
    b, heads = 3, 2
    qkv = torch.from_numpy(counter_normal(70 + t, "vit_qkv", (b * t, 3 * 64 * heads))) * torch.tensor([1.5, 1.5, 1.0]).repeat_interleave(64 * heads)
    out = clf.engine.op_image_attention(qkv, B=b, T=t, heads=heads)
    err = rel_err(out.cpu(), attention_ref(qkv, b, t, heads))
    print(f"image attention T={t}: max|a-b|/max|b| = {err:.3e} (bound {BOUND:.0e})")
    assert not torch.isnan(out).any() and err < BOUND, err


def test_op_image_attention_limit(clf):
    qkv = torch.zeros(289, 3 * 64)
    assert clf.engine.op_image_attention(qkv[:288], B=1, T=288, heads=1).shape == (288, 64)
    with pytest.raises(ValueError, match="288"):                                           # E2V_ESHAPE
        clf.engine.op_image_attention(qkv, B=1, T=289, heads=1)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("t", [65, 197])
def test_op_image_attention_fenced(clf, t, pad):
    b, heads = 2, 2
    c = heads * 64
    qkv = torch.from_numpy(counter_normal(90 + t, "vit_qkvf", (b * t, 3 * c)))
    fi, fo = fenced(qkv, ld=3 * c + pad, name="qkv"), fenced_out((b * t, c), ld=c + pad)
    y = run_fenced(lambda: clf.engine.op_image_attention(fi.t, B=b, T=t, heads=heads, out=fo.t), [fi], fo)
    assert rel_err(y.cpu(), attention_ref(qkv, b, t, heads)) < BOUND


# ------------------------------------------------------------------ 3. the whole model ----------------------------------------------
def test_whole_model_vs_the_transformers_fixture(clf, golden, batch8):
    z = golden[0]
    logits, probs, t3 = batch8
    err = rel_err(logits, z["logits"])
    perr = float(np.abs(probs.double().numpy() - softmax64(logits.numpy())).max())
    print(f"HIP vs transformers {z['transformers_version']} logits: max|a-b|/max|b| = {err:.3e} (bound {BOUND:.0e}); "
          f"probs vs the float64 softmax of the device's logits: {perr:.3e} (bound 1e-6)")
    assert logits.shape == (8, 50) and logits.dtype == torch.float32 and not torch.isnan(logits).any() and err < BOUND, err
    assert perr < 1e-6, perr
    assert t3.dtype == torch.int32 and np.array_equal(t3.numpy(), top3(z["logits"]))        # all 8 images
    assert np.array_equal(t3.numpy(), top3(logits.numpy()))                                 # and the device's own logits say the same


def test_original_shapes_give_the_bits_of_pillows_bytes(clf, golden, batch8):
    """each group at its own size: the preprocess is Pillow's bit for bit, so the model sees the same patch rows as for the resized bytes"""
    z, i0 = golden[0], 0
    for g in GROUPS:
        imgs = torch.from_numpy(z["images_" + g])
        out = clf.engine.classify_frames(imgs[:, None], channels_last=True)                 # n clips of one frame
        for got, want in zip(out, batch8):
            assert torch.equal(bits(got.cpu()), bits(want[i0:i0 + len(imgs)])), g
        i0 += len(imgs)


# ------------------------------------------------------------------ 4. determinism ---------------------------------------------------
def test_an_image_does_not_depend_on_batch_chunk_or_mode(clf, resized8, batch8):
    eng = clf.engine
    frames = torch.from_numpy(resized8)

    def same(out, rows, what):
        for got, want in zip(out, batch8):
            assert torch.equal(bits(got.cpu()), bits(want[rows])), what

    same(eng.classify_frames(frames[None], channels_last=True), slice(0, 8), "a second run")
    for i in (0, 5, 7):
        same(eng.classify_frames(frames[i][None, None], channels_last=True), slice(i, i + 1), f"image {i} alone")
    same(eng.classify_frames(frames.view(2, 4, S, S, 3), channels_last=True), slice(0, 8), "2 clips of 4 frames")
    try:
        eng.set_knob("E2V_VIT_CHUNK", 3)                                                    # chunks of 3, 3 and 2 images
        same(eng.classify_frames(frames[None], channels_last=True), slice(0, 8), "chunks of 3")
    finally:
        eng.set_knob("E2V_VIT_CHUNK", 64)
    for mode in ("bf16", "fp16"):
        try:
            eng.set_compute_dtype(mode)
            same(eng.classify_frames(frames[None], channels_last=True), slice(0, 8), mode)
        finally:
            eng.set_compute_dtype("fp32")


def test_planar_float_frames_are_the_same_images(clf, resized8, batch8):
    """``[n,3,F,H,W]`` floats in [0,1] -- what ``e2v_generate`` leaves on the device -- go in as they are"""
    videos = as_kind(resized8[None], True, False).cuda()
    for got, want in zip(clf.engine.classify_frames(videos), batch8):
        assert torch.equal(bits(got.cpu()), bits(want))


# ------------------------------------------------------------------ 5. the Python layer ----------------------------------------------
def to_v5(sd):
    out = {}
    for k, v in sd.items():
        if k.startswith("vit.encoder.layer."):
            rest = k[len("vit.encoder.layer."):]
            for new, old in _VIT_V5_NAMES:
                if old in rest:
                    rest = rest.replace(old, new)
                    break
            k = "vit.layers." + rest
        out[k] = v
    return out


def write_checkpoint(path, sd, safe, resample=2):
    c = TINY_IMAGE
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump({"architectures": ["ViTForImageClassification"], "model_type": "vit", "hidden_size": c.hidden, "num_attention_heads": c.heads,
                   "num_hidden_layers": c.layers, "intermediate_size": c.intermediate, "image_size": c.image_size, "patch_size": c.patch_size,
                   "hidden_act": "gelu", "layer_norm_eps": c.layer_norm_eps, "qkv_bias": True, "num_channels": 3,
                   "id2label": {str(i): f"LABEL_{i}" for i in range(c.num_labels)}}, f)
    with open(os.path.join(path, "preprocessor_config.json"), "w") as f:
        json.dump({"do_normalize": True, "do_rescale": True, "do_resize": True, "image_mean": [0.5, 0.5, 0.5], "image_std": [0.5, 0.5, 0.5],
                   "image_processor_type": "ViTImageProcessor", "resample": resample, "rescale_factor": 1 / 255,
                   "size": {"height": c.image_size, "width": c.image_size}}, f)
    tensors = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}
    if safe:
        from safetensors.torch import save_file
        save_file(tensors, os.path.join(path, "model.safetensors"))
    else:
        torch.save(tensors, os.path.join(path, "pytorch_model.bin"))


@pytest.mark.parametrize("spelling,safe", [("checkpoint", True), ("checkpoint", False), ("v5", True), ("v5", False)])
def test_from_pretrained_round_trips(clf, golden, resized8, batch8, tmp_path, spelling, safe):
    from eeg2video_amd.image_classifier import ViTForImageClassification
    sd = golden[1]
    d = str(tmp_path / "vit")
    write_checkpoint(d, sd if spelling == "checkpoint" else to_v5(sd), safe)
    model = ViTForImageClassification.from_pretrained(d, engine=clf.engine)                # (the same config: the engine is reused)
    assert model.icfg == TINY_IMAGE and model.config.num_labels == 50
    out = model(torch.from_numpy(resized8))                                                 # [8,112,112,3]: 8 frames of one clip
    assert out[0] is out.logits and torch.equal(bits(out.logits.cpu()), bits(batch8[0]))
    back = model.state_dict(device="cpu")
    assert list(back) == list(image_param_spec(TINY_IMAGE))
    for k, v in back.items():
        assert v.dtype == torch.float32 and np.array_equal(v.numpy(), sd[k]), k            # the loaded bits, fused and padded tensors included
    d2 = str(tmp_path / "again")
    model.save_pretrained(d2, safe_serialization=safe)
    assert ViTForImageClassification.config_from_dir(d2) == TINY_IMAGE
    assert os.path.isfile(os.path.join(d2, "model.safetensors" if safe else "pytorch_model.bin"))


def test_from_pretrained_refusals(tmp_path, golden):
    from eeg2video_amd.image_classifier import ViTForImageClassification
    with pytest.raises(RuntimeError, match="never\\s+reads the network"):
        ViTForImageClassification.from_pretrained("google/vit-base-patch16-224")
    d = str(tmp_path / "bicubic")
    write_checkpoint(d, golden[1], True, resample=3)
    with pytest.raises(NotImplementedError, match="BILINEAR"):
        ViTForImageClassification.from_pretrained(d)


def test_frozen_and_absent(clf):
    with pytest.raises(ValueError, match="frozen"):
        clf.engine.update_state_dict({"vit.layernorm.weight": torch.ones(TINY_IMAGE.hidden)}, prefix="image.")
    assert clf.engine.weight_forms("image.vit.encoder.layer.0.attention.attention.query.weight") == 1          # fp32 only
    assert clf.engine.weight_forms("image.classifier.weight") == 1
    from eeg2video_amd.engine import Engine
    plain = Engine(TINY_UNET, TINY_VAE, 0)
    with pytest.raises(RuntimeError, match="without an image classifier"):
        plain.classify_frames(torch.zeros(1, 1, 8, 8, 3, dtype=torch.uint8), channels_last=True)
    with pytest.raises(RuntimeError, match="no image classifier"):
        plain.finalize(plain.IMAGE)


def test_img_classify_metric_equals_the_cpu_route(clf, golden, resized8):
    from eeg2video_amd.metrics import img_classify_metric
    z = golden[0]
    pred_idx, gt_idx = list(range(0, 6)), list(range(2, 8))                                 # two 6-frame clips out of the 8 images
    pred, gt = resized8[pred_idx], resized8[gt_idx]
    for n_way, top_k in ((2, 1), (40, 1), (40, 3)):
        np.random.seed(5)
        got_acc, got_std = img_classify_metric(pred, gt, n_way=n_way, num_trials=20, top_k=top_k, return_std=True, model=clf)
        np.random.seed(5)
        want = [reference_n_way_top_k_acc(torch.from_numpy(z["probs"][p]), [int(i) for i in top3(z["logits"][g])], n_way, 20, top_k)
                for p, g in zip(pred_idx, gt_idx)]
        assert isinstance(got_acc, list) and isinstance(got_std, list) and len(got_acc) == len(got_std) == 6
        assert got_acc == [a for a, _ in want] and got_std == [s for _, s in want], (n_way, top_k)
    np.random.seed(6)
    assert img_classify_metric(gt, gt, n_way=2, num_trials=10, model=clf) == [1.0] * 6      # pred = gt: the arg-max is one of its top 3
    np.random.seed(6)
    assert img_classify_metric(torch.from_numpy(gt), gt, n_way=2, num_trials=10, model=clf, return_std=True) == ([1.0] * 6, [0.0] * 6)
    with pytest.raises(RuntimeError, match="never\\s+reads the network"):
        img_classify_metric(pred, gt, cache_dir="google/vit-base-patch16-224")


def test_sweep_scored_with_a_classifier(golden, tmp_path, capsys):
    """``examples/run_sweep.py --score-against DIR --classifier DIR``: a sweep scored against its own frames wins every trial"""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "run_sweep.py")
    spec = importlib.util.spec_from_file_location("e2v_sweep_classified", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    vit_dir, out = str(tmp_path / "vit"), str(tmp_path / "clips")
    write_checkpoint(vit_dir, golden[1], True)
    common = ["--tiny", "--concepts", "2", "--per-concept", "1", "--batch", "2", "--steps", "2"]
    mod.main(common + ["--out", out, "--npy"])
    capsys.readouterr()
    mod.main(common + ["--score-against", out, "--classifier", vit_dir])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["image_2way_acc"] == 1.0 and rec["image_40way_acc"] == 1.0 and rec["ssim_mean"] == 1 and rec["stage_seconds_rank0"]["score"] > 0
    with pytest.raises(SystemExit):
        mod.main(common + ["--classifier", vit_dir])


# ------------------------------------------------------------------ 6. bounds --------------------------------------------------------
def test_outputs_fenced_and_pool_guarded(golden, resized8, batch8):
    """one call with E2V_POOL_GUARD on and fenced outputs: no store outside a tensor, inside the library or out of it"""
    frames = torch.from_numpy(resized8[:5]).cuda()
    with environment({}, GUARD_KIB):
        g = make_classifier(golden[1])
        eng = g.engine
        eng.pool_guard_report()
        lo, pr, t3 = fenced_out((5, 50)), fenced_out((5, 50)), fenced_out((5, 3))
        gets = eng.pool_gets()

        def call():
            st = eng.lib.e2v_image_classify(eng.ctx, frames.data_ptr(), _lib.E2V_FRAMES_U8 | _lib.E2V_FRAMES_CHANNELS_LAST, 1, 5, S, S,
                                            lo.t.data_ptr(), pr.t.data_ptr(), t3.t.data_ptr(), None)
            assert st == 0, eng.lib.e2v_last_error(eng.ctx)
        y = run_fenced(call, [lo, pr], t3)
        taken = eng.pool_gets() - gets
        checked, violations, text = eng.pool_guard_report()
        assert violations == 0, text
        assert taken > 0 and checked >= taken, (checked, taken)
        assert torch.equal(bits(lo.view.cpu()), bits(batch8[0][:5])) and torch.equal(bits(pr.view.cpu()), bits(batch8[1][:5]))
        assert torch.equal(y.cpu().view(torch.int32), batch8[2][:5])
        # only the outputs asked for are written
        only = fenced_out((5, 3))
        st = eng.lib.e2v_image_classify(eng.ctx, frames.data_ptr(), 3, 1, 5, S, S, None, None, only.t.data_ptr(), None)
        torch.cuda.synchronize()
        only.check()
        assert st == 0 and torch.equal(only.view.cpu().view(torch.int32), batch8[2][:5])
        assert eng.pool_guard_report()[1] == 0


def test_steady_state_takes_no_new_memory(clf, resized8):
    eng, frames = clf.engine, torch.from_numpy(resized8[None]).cuda()
    eng.classify_frames(frames, channels_last=True)
    torch.cuda.synchronize()
    g0, bytes0 = eng.pool_gets(), eng.device_bytes()
    eng.classify_frames(frames, channels_last=True)
    g1 = eng.pool_gets()
    eng.classify_frames(frames, channels_last=True)
    torch.cuda.synchronize()
    assert eng.pool_gets() - g1 == g1 - g0 > 0 and eng.device_bytes() == bytes0
