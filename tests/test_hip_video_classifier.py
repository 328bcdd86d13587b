"""GPU: the VideoMAE video classifier (``e2v_video_classify``, ``csrc/video.hip``) against ``transformers`` and Pillow.

References: the committed fixture (``tests/golden/videomae_tiny.npz``: ``transformers.VideoMAEForVideoClassification`` logits of 8
clips, the processor's cropped bytes, its pixel table) for the whole model; the integer restatement of the processor
(``tests/videomae_restatement.py``, pinned to Pillow bit for bit on the CPU) for the preprocess; ``torch.softmax(q k^T / 8) v`` in
float64, computed on the spot, for the attention op.

Tolerances, measured on the CPU without the code under test (``tests/test_video_classifier_host.py`` prints and pins them): the
fixture's fp32 logits sit 4.6e-7 (max |a-b| / max |b|) from the float64 restatement and its softmax 4.9e-7 (absolute); an fp32
torch-CPU attention sits 9.8e-7 from float64 at T = 1568.  The device bounds are ten times those distances -- fp32 summation order
differs by kernel --: logits 4.6e-6, softmax 4.9e-6, attention 9.8e-6.
"""
import json
import os

import numpy as np
import pytest
import torch

from eeg2video_amd import _lib
from eeg2video_amd.engine import image_resize_table
from eeg2video_amd.weights import (TINY_UNET, TINY_VAE, TINY_VIDEO, counter_normal, synth_state_dict, video_checkpoint_spec,
                                   video_position_table)
from test_hip_bounds import GUARD_KIB, PADS, environment, fenced, fenced_out, run_fenced
from test_image_classifier_host import reference_n_way_top_k_acc
from test_video_classifier_host import ATTN_BOUND, LOGIT_BOUND, PROB_BOUND, to_original_spelling
from videomae_restatement import (GROUPS, load_golden, pillow_resize_crop, pixel_table, rel_err, resize_crop_with_tables, softmax64, top3,
                                  tubelet_rows)

pytestmark = pytest.mark.gpu

S, P, TS, E, F = TINY_VIDEO.image_size, TINY_VIDEO.patch_size, TINY_VIDEO.tubelet_size, TINY_VIDEO.resize_edge, TINY_VIDEO.num_frames


def make_engine(cfg=TINY_VIDEO):
    from eeg2video_amd.engine import Engine
    return Engine(TINY_UNET, TINY_VAE, 0, video_cfg=cfg)


def make_classifier(sd, engine=None):
    from eeg2video_amd.video_classifier import VideoMAEForVideoClassification
    return VideoMAEForVideoClassification(TINY_VIDEO, engine=engine or make_engine()).load_state_dict(sd)


@pytest.fixture(scope="module")
def golden():
    z, sd = load_golden()
    return {k: z[k] for k in z.files}, sd


@pytest.fixture(scope="module")
def clf(golden):
    return make_classifier(golden[1])


@pytest.fixture(scope="module")
def cropped8(golden):
    """the 8 fixture clips as the processor cropped them, ``[8,6,56,56,3]`` uint8, in the fixture's order"""
    z = golden[0]
    return np.concatenate([z["cropped_36x64"], z["cropped_90x50"], z["clips_56x56"]])


@pytest.fixture(scope="module")
def batch8(clf, cropped8):
    """(logits, probs, top3) of the 8 cropped clips in one call, on the host -- the result the other tests compare bits with"""
    out = clf.engine.classify_clips(torch.from_numpy(cropped8), channels_last=True)
    return tuple(t.cpu() for t in out)


def bits(t):
    return t.contiguous().view(torch.int32)


def as_kind(clips_u8, f32, channels_last):
    """``[n,F,H,W,3]`` uint8 -> the same clips as uint8 / float32 in either layout; the float is the middle of the byte's bucket"""
    t = torch.from_numpy(np.ascontiguousarray(clips_u8))
    if f32:
        t = (t.float() + 0.5) / 255.0
    return t if channels_last else t.permute(0, 4, 1, 2, 3).contiguous()


# ------------------------------------------------------------------ 1. preprocess ----------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_preprocess_fixture_clips_bit_for_bit_in_all_four_kinds(clf, golden, group):
    z = golden[0]
    clips = z["clips_" + group]
    cropped = z["cropped_" + group] if "cropped_" + group in z else clips
    want = np.concatenate([tubelet_rows(c, z["pixel_table"], P, TS) for c in cropped])       # the processor's bytes + its table
    got = None
    for f32 in (False, True):
        for cl in (True, False):
            rows = clf.engine.op_video_preprocess(as_kind(clips, f32, cl), size=S, patch=P, tubelet=TS, edge=E, channels_last=cl).cpu()
            assert rows.shape == (len(clips) * (F // TS) * (S // P) ** 2, 3 * TS * P * P)
            if got is None:
                got = rows
                assert np.array_equal(rows.numpy().view(np.int32), want.view(np.int32)), int((rows.numpy() != want).sum())
            assert torch.equal(bits(rows), bits(got)), (f32, cl)                           # the four type / layout combinations agree


@pytest.mark.parametrize("h,w,size,patch,ts,edge", [(288, 512, 224, 16, 2, 224),   # the reference's frames at VideoMAE-B: columns 87..310 of 398
                                                     (45, 77, 32, 8, 2, 40),        # edge above the crop: both axes cropped, odd remainders
                                                     (30, 20, 32, 8, 3, 32),        # an upscale of a tall frame, tubelets of 3
                                                     (420, 4, 2, 2, 1, 3)])         # more than 100 times as tall as wide and shrunk: vertical pass first
def test_preprocess_shapes_bit_for_bit(clf, h, w, size, patch, ts, edge):
    rng = np.random.default_rng(h + w)
    clips = rng.integers(0, 256, (2, 6, h, w, 3), dtype=np.uint8)
    lut = pixel_table(1 / 255, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    want = np.concatenate([tubelet_rows(np.stack([resize_crop_with_tables(f, edge, size, image_resize_table) for f in c]), lut, patch, ts)
                           for c in clips])
    try:
        assert np.array_equal(pillow_resize_crop(clips[1, 3], edge, size), resize_crop_with_tables(clips[1, 3], edge, size, image_resize_table))
    except ImportError:
        pass
    for cl in (True, False):
        rows = clf.engine.op_video_preprocess(as_kind(clips, False, cl), size=size, patch=patch, tubelet=ts, edge=edge, lut=lut,
                                              channels_last=cl).cpu().numpy()
        assert np.array_equal(rows.view(np.int32), want.view(np.int32)), (cl, int((rows != want).sum()))


def test_preprocess_output_is_fenced(clf, golden):
    clips = torch.from_numpy(golden[0]["clips_90x50"]).cuda()
    fo = fenced_out((2 * 3 * 49, 3 * TS * P * P))
    y = run_fenced(lambda: clf.engine.op_video_preprocess(clips, size=S, patch=P, tubelet=TS, edge=E, channels_last=True, out=fo.t), [], fo)
    assert torch.equal(bits(y.cpu()), bits(clf.engine.op_video_preprocess(clips, size=S, patch=P, tubelet=TS, edge=E, channels_last=True).cpu()))


# ------------------------------------------------------------------ 2. attention -----------------------------------------------------
def attention_ref(qkv, b, t, heads):
    q, k, v = (x.double().view(b, t, heads, 64).transpose(1, 2) for x in qkv.chunk(3, dim=-1))
    return (torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v).transpose(1, 2).reshape(b * t, heads * 64)


@pytest.mark.parametrize("t", [1, 31, 32, 33, 64, 65, 147, 257, 588, 1568])
def test_op_token_attention(clf, t):
    """accuracy against float64, fenced on both sides (strided rows), and the bits of a sequence alone = in the batch"""
    b, heads = 2, 2
    c = heads * 64
    qkv = torch.from_numpy(counter_normal(70 + t, "vmae_qkv", (b * t, 3 * c))) * torch.tensor([1.5, 1.5, 1.0]).repeat_interleave(c)
    want = attention_ref(qkv, b, t, heads)
    pad = PADS[t % 2]
    fi, fo = fenced(qkv, ld=3 * c + pad, name="qkv"), fenced_out((b * t, c), ld=c + pad)
    y = run_fenced(lambda: clf.engine.op_token_attention(fi.t, B=b, T=t, heads=heads, out=fo.t), [fi], fo).cpu()
    err = rel_err(y, want)
    print(f"token attention T={t}: max|a-b|/max|b| = {err:.3e} (bound {ATTN_BOUND:.1e})")
    assert err < ATTN_BOUND, err
    both = clf.engine.op_token_attention(qkv, B=b, T=t, heads=heads).cpu()
    assert torch.equal(bits(both), bits(y))                                                # contiguous rows: the same bits
    for i in range(b):
        alone = clf.engine.op_token_attention(qkv[i * t:(i + 1) * t], B=1, T=t, heads=heads).cpu()
        assert torch.equal(bits(alone), bits(both[i * t:(i + 1) * t])), i


def test_op_token_attention_in_a_batch_of_eight_and_other_head_counts(clf):
    """8 sequences (whole samples per XCD) and 3 heads: the bits of a sequence's head do not depend on how the grid is dealt"""
    t = 147
    qkv = torch.from_numpy(counter_normal(5, "vmae_qkv8", (8 * t, 3 * 192)))
    out = clf.engine.op_token_attention(qkv, B=8, T=t, heads=3).cpu()
    assert rel_err(out, attention_ref(qkv, 8, t, 3)) < ATTN_BOUND
    for i in (0, 3, 7):
        assert torch.equal(bits(clf.engine.op_token_attention(qkv[i * t:(i + 1) * t], B=1, T=t, heads=3).cpu()), bits(out[i * t:(i + 1) * t]))


# ------------------------------------------------------------------ 3. the whole model ----------------------------------------------
def test_whole_model_vs_the_transformers_fixture(clf, golden, batch8):
    z = golden[0]
    logits, probs, t3 = batch8
    err = rel_err(logits, z["logits"])
    perr = float(np.abs(probs.double().numpy() - z["probs"].astype(np.float64)).max())
    serr = float(np.abs(probs.double().numpy() - softmax64(logits.numpy())).max())
    print(f"HIP vs transformers {z['transformers_version']}: logits max|a-b|/max|b| = {err:.3e} (bound {LOGIT_BOUND:.1e}), "
          f"softmax {perr:.3e} (bound {PROB_BOUND:.1e}); softmax vs the float64 softmax of the device's logits {serr:.3e}")
    assert logits.shape == (8, 50) and logits.dtype == torch.float32 and not torch.isnan(logits).any() and err < LOGIT_BOUND, err
    assert perr < PROB_BOUND and serr < PROB_BOUND, (perr, serr)
    assert t3.dtype == torch.int32 and np.array_equal(t3.numpy(), top3(z["logits"]))        # all 8 clips
    assert np.array_equal(t3.numpy(), top3(logits.numpy()))


def test_original_shapes_give_the_bits_of_the_processors_bytes(clf, golden, batch8):
    """each group at its own size: the preprocess is the processor's bit for bit, so the model sees the same rows as for the cropped bytes"""
    z, i0 = golden[0], 0
    for g in GROUPS:
        clips = torch.from_numpy(z["clips_" + g])
        out = clf.engine.classify_clips(clips, channels_last=True)
        for got, want in zip(out, batch8):
            assert torch.equal(bits(got.cpu()), bits(want[i0:i0 + len(clips)])), g
        i0 += len(clips)


# ------------------------------------------------------------------ 4. determinism ---------------------------------------------------
def test_a_clip_does_not_depend_on_batch_chunk_mode_or_run(clf, cropped8, batch8):
    eng = clf.engine
    clips = torch.from_numpy(cropped8)

    def same(out, rows, what):
        for got, want in zip(out, batch8):
            assert torch.equal(bits(got.cpu()), bits(want[rows])), what

    same(eng.classify_clips(clips, channels_last=True), slice(0, 8), "a second run")
    for i in (0, 5, 7):
        same(eng.classify_clips(clips[i], channels_last=True), slice(i, i + 1), f"clip {i} alone")
    same(eng.classify_clips(clips[3:6], channels_last=True), slice(3, 6), "clips 3..5 at positions 0..2")
    try:
        eng.set_knob("E2V_VMAE_CHUNK", 3)                                                   # chunks of 3, 3 and 2 clips
        same(eng.classify_clips(clips, channels_last=True), slice(0, 8), "chunks of 3")
    finally:
        eng.set_knob("E2V_VMAE_CHUNK", 16)
    for mode in ("bf16", "fp16"):
        try:
            eng.set_compute_dtype(mode)
            same(eng.classify_clips(clips, channels_last=True), slice(0, 8), mode)
        finally:
            eng.set_compute_dtype("fp32")


def test_planar_float_clips_are_the_same_clips(clf, cropped8, batch8):
    """``[n,3,F,H,W]`` floats in [0,1] -- what ``e2v_generate`` leaves on the device -- go in as they are"""
    videos = as_kind(cropped8, True, False).cuda()
    for got, want in zip(clf.engine.classify_clips(videos), batch8):
        assert torch.equal(bits(got.cpu()), bits(want))


# ------------------------------------------------------------------ 5. the Python layer ----------------------------------------------
def write_checkpoint(path, sd, safe, cfg=TINY_VIDEO, num_frames=None, resample=2):
    c = cfg
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump({"architectures": ["VideoMAEForVideoClassification"], "model_type": "videomae", "hidden_size": c.hidden,
                   "num_attention_heads": c.heads, "num_hidden_layers": c.layers, "intermediate_size": c.intermediate, "image_size": c.image_size,
                   "patch_size": c.patch_size, "tubelet_size": c.tubelet_size, "num_frames": num_frames or c.num_frames, "hidden_act": "gelu",
                   "layer_norm_eps": c.layer_norm_eps, "qkv_bias": True, "use_mean_pooling": True, "num_channels": 3,
                   "id2label": {str(i): f"LABEL_{i}" for i in range(c.num_labels)}}, f)
    with open(os.path.join(path, "preprocessor_config.json"), "w") as f:
        json.dump({"do_normalize": True, "do_rescale": True, "do_resize": True, "do_center_crop": True, "image_mean": list(c.image_mean),
                   "image_std": list(c.image_std), "image_processor_type": "VideoMAEImageProcessor", "resample": resample,
                   "rescale_factor": 1 / 255, "size": {"shortest_edge": c.resize_edge},
                   "crop_size": {"height": c.image_size, "width": c.image_size}}, f)
    tensors = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}
    if safe:
        from safetensors.torch import save_file
        save_file(tensors, os.path.join(path, "model.safetensors"))
    else:
        torch.save(tensors, os.path.join(path, "pytorch_model.bin"))


def with_zero_key_bias(sd):
    return {k: (np.zeros_like(v) if k.endswith(".attention.attention.key.bias") else v) for k, v in sd.items()}


@pytest.mark.parametrize("spelling,safe", [("installed", True), ("installed", False), ("original", True), ("original", False)])
def test_from_pretrained_round_trips(clf, golden, cropped8, batch8, tmp_path, spelling, safe):
    from eeg2video_amd.video_classifier import VideoMAEForVideoClassification
    sd = golden[1] if spelling == "installed" else with_zero_key_bias(golden[1])           # the original spelling has no key bias
    d = str(tmp_path / "vmae")
    write_checkpoint(d, sd if spelling == "installed" else to_original_spelling(sd), safe, num_frames=16)      # the hub config says 16 ...
    model = VideoMAEForVideoClassification.from_pretrained(d, num_frames=6, engine=clf.engine)                 # ... the reference passes 6
    try:
        assert model.vcfg == TINY_VIDEO and model.config.num_labels == 50 and model.config.num_frames == 6
        out = model(torch.from_numpy(cropped8))
        if spelling == "installed":
            assert out[0] is out.logits and torch.equal(bits(out.logits.cpu()), bits(batch8[0]))
        else:               # a key bias moves every score of a query by one constant, which the softmax removes: the same classes
            assert out.logits.shape == (8, 50) and np.array_equal(top3(out.logits.cpu().numpy()), batch8[2].numpy())
        back = model.state_dict(device="cpu")
        assert list(back) == list(video_checkpoint_spec(TINY_VIDEO))
        for k, v in back.items():
            assert v.dtype == torch.float32 and tuple(v.shape) == video_checkpoint_spec(TINY_VIDEO)[k] and np.array_equal(v.numpy(), sd[k]), k
        assert np.array_equal(model.position_embeddings.cpu().numpy()[0], video_position_table(147, 128))
        d2 = str(tmp_path / "again")
        model.save_pretrained(d2, safe_serialization=safe)
        assert VideoMAEForVideoClassification.config_from_dir(d2) == TINY_VIDEO
        assert VideoMAEForVideoClassification.config_from_dir(d2, num_frames=16).tokens == 8 * 49
        assert os.path.isfile(os.path.join(d2, "model.safetensors" if safe else "pytorch_model.bin"))
    finally:
        clf.load_state_dict(golden[1])                                                      # the shared engine gets the fixture's weights back


def test_num_frames_override_sizes_the_position_table(golden, cropped8, tmp_path):
    """the same weights at num_frames = 4: 98 tokens, another table, and clips of 4 frames"""
    from eeg2video_amd.video_classifier import VideoMAEForVideoClassification
    d = str(tmp_path / "vmae")
    write_checkpoint(d, golden[1], True)
    model = VideoMAEForVideoClassification.from_pretrained(d, num_frames=4)
    assert model.vcfg.num_frames == 4 and model.vcfg.tokens == 98
    assert np.array_equal(model.position_embeddings.cpu().numpy()[0], video_position_table(98, 128))
    logits, probs, t3 = model.classify(torch.from_numpy(cropped8[:2, :4]))
    assert logits.shape == (2, 50) and not torch.isnan(logits).any() and np.array_equal(t3.cpu().numpy(), top3(logits.cpu().numpy()))
    with pytest.raises(ValueError, match="num_frames=4"):
        model.classify(torch.from_numpy(cropped8[:2]))                                      # 6 frames
    with pytest.raises(ValueError, match="vmae_num_frames"):                                # and below the mirror: E2V_ESHAPE
        model.engine.classify_clips(torch.from_numpy(cropped8[:1, :5]), channels_last=True)


def test_from_pretrained_refusals(tmp_path, golden):
    from eeg2video_amd.video_classifier import VideoMAEForVideoClassification
    with pytest.raises(RuntimeError, match="never\\s+reads the network"):
        VideoMAEForVideoClassification.from_pretrained("MCG-NJU/videomae-base-finetuned-kinetics", num_frames=6)
    d = str(tmp_path / "vmae")
    write_checkpoint(d, golden[1], True)
    with pytest.raises(ValueError, match="multiple of tubelet_size"):
        VideoMAEForVideoClassification.from_pretrained(d, num_frames=5)                     # odd F
    d = str(tmp_path / "bicubic")
    write_checkpoint(d, golden[1], True, resample=3)
    with pytest.raises(NotImplementedError, match="BILINEAR"):
        VideoMAEForVideoClassification.from_pretrained(d)


def test_frozen_and_absent(clf, cropped8):
    with pytest.raises(ValueError, match="frozen"):
        clf.engine.update_state_dict({"fc_norm.weight": torch.ones(TINY_VIDEO.hidden)}, prefix="video.")
    assert clf.engine.weight_forms("video.videomae.encoder.layer.0.attention.attention.query.weight") == 1          # fp32 only
    assert clf.engine.weight_forms("video.classifier.weight") == 1
    with pytest.raises(ValueError, match="vmae_num_frames"):
        clf.engine.classify_clips(torch.from_numpy(cropped8[:1, :4]), channels_last=True)   # F != num_frames
    from eeg2video_amd.engine import Engine
    plain = Engine(TINY_UNET, TINY_VAE, 0)
    with pytest.raises(RuntimeError, match="without a video classifier"):
        plain.classify_clips(torch.zeros(1, 6, 8, 8, 3, dtype=torch.uint8), channels_last=True)
    with pytest.raises(RuntimeError, match="no video classifier"):
        plain.finalize(plain.VIDEO)


def test_video_classify_metric_equals_the_cpu_route(clf, golden, cropped8):
    from eeg2video_amd.metrics import video_classify_metric
    z = golden[0]
    pred_idx, gt_idx = [0, 1, 2, 3, 4], [3, 4, 5, 6, 7]
    pred, gt = cropped8[pred_idx], cropped8[gt_idx]
    for n_way, top_k in ((2, 1), (40, 1), (40, 3)):
        np.random.seed(5)
        got_acc, got_std = video_classify_metric(pred, gt, n_way=n_way, num_trials=20, top_k=top_k, return_std=True, model=clf)
        np.random.seed(5)
        want = [reference_n_way_top_k_acc(torch.from_numpy(z["probs"][p]), [int(i) for i in top3(z["logits"][g])], n_way, 20, top_k)
                for p, g in zip(pred_idx, gt_idx)]
        assert isinstance(got_acc, list) and isinstance(got_std, list) and len(got_acc) == len(got_std) == 5
        assert got_acc == [a for a, _ in want] and got_std == [s for _, s in want], (n_way, top_k)
    np.random.seed(6)
    assert video_classify_metric(gt, gt, n_way=2, num_trials=10, model=clf) == [1.0] * 5    # pred = gt: the arg-max is one of its top 3
    with pytest.raises(RuntimeError, match="never\\s+reads the network"):
        video_classify_metric(pred, gt, cache_dir="MCG-NJU/videomae-base-finetuned-kinetics")


def test_sweep_scored_with_a_video_classifier(tmp_path, capsys):
    """``examples/run_sweep.py --score-against DIR --video-classifier DIR``: a sweep scored against its own clips wins every trial.  The
    tiny sweep makes clips of 3 frames, so the checkpoint is one of tubelets of 3 (49 tokens), with synthetic weights."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "run_sweep.py")
    spec = importlib.util.spec_from_file_location("e2v_sweep_video_classified", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import dataclasses
    cfg = dataclasses.replace(TINY_VIDEO, image_size=32, resize_edge=32, tubelet_size=3, num_frames=3)
    vmae_dir, out = str(tmp_path / "vmae"), str(tmp_path / "clips")
    write_checkpoint(vmae_dir, synth_state_dict(video_checkpoint_spec(cfg), seed=46, mode="perturbed"), True, cfg=cfg)
    common = ["--tiny", "--concepts", "2", "--per-concept", "1", "--batch", "2", "--steps", "2"]
    mod.main(common + ["--out", out, "--npy"])
    capsys.readouterr()
    mod.main(common + ["--score-against", out, "--video-classifier", vmae_dir])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["video_2way_acc"] == 1.0 and rec["video_40way_acc"] == 1.0 and rec["ssim_mean"] == 1 and rec["stage_seconds_rank0"]["score"] > 0
    assert "image_2way_acc" not in rec
    with pytest.raises(SystemExit):
        mod.main(common + ["--video-classifier", vmae_dir])


# ------------------------------------------------------------------ 6. bounds --------------------------------------------------------
def test_outputs_fenced_and_pool_guarded(golden, batch8):
    """one call with E2V_POOL_GUARD on and fenced outputs, at the tall shape (both tables sliced): no store outside a tensor"""
    clips = torch.from_numpy(golden[0]["clips_90x50"]).cuda()                               # clips 4 and 5 of the fixture
    with environment({}, GUARD_KIB):
        g = make_classifier(golden[1])
        eng = g.engine
        eng.pool_guard_report()
        lo, pr, t3 = fenced_out((2, 50)), fenced_out((2, 50)), fenced_out((2, 3))
        gets = eng.pool_gets()

        def call():
            st = eng.lib.e2v_video_classify(eng.ctx, clips.data_ptr(), _lib.E2V_FRAMES_U8 | _lib.E2V_FRAMES_CHANNELS_LAST, 2, 6, 90, 50,
                                            lo.t.data_ptr(), pr.t.data_ptr(), t3.t.data_ptr(), None)
            assert st == 0, eng.lib.e2v_last_error(eng.ctx)
        y = run_fenced(call, [lo, pr], t3)
        taken = eng.pool_gets() - gets
        checked, violations, text = eng.pool_guard_report()
        assert violations == 0, text
        assert taken > 0 and checked >= taken, (checked, taken)
        assert torch.equal(bits(lo.view.cpu()), bits(batch8[0][4:6])) and torch.equal(bits(pr.view.cpu()), bits(batch8[1][4:6]))
        assert torch.equal(y.cpu().view(torch.int32), batch8[2][4:6])
        # only the outputs asked for are written
        only = fenced_out((2, 3))
        st = eng.lib.e2v_video_classify(eng.ctx, clips.data_ptr(), 3, 2, 6, 90, 50, None, None, only.t.data_ptr(), None)
        torch.cuda.synchronize()
        only.check()
        assert st == 0 and torch.equal(only.view.cpu().view(torch.int32), batch8[2][4:6])
        assert eng.pool_guard_report()[1] == 0


def test_steady_state_takes_no_new_memory(clf, cropped8):
    eng, clips = clf.engine, torch.from_numpy(cropped8).cuda()
    eng.classify_clips(clips, channels_last=True)
    torch.cuda.synchronize()
    g0, bytes0 = eng.pool_gets(), eng.device_bytes()
    eng.classify_clips(clips, channels_last=True)
    g1 = eng.pool_gets()
    eng.classify_clips(clips, channels_last=True)
    torch.cuda.synchronize()
    assert eng.pool_gets() - g1 == g1 - g0 > 0 and eng.device_bytes() == bytes0
