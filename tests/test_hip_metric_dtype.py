"""GPU: the metric towers (ViT classifier, VideoMAE classifier, CLIP vision tower) in their opt-in 16-bit modes
(``e2v_set_tower_dtype``, ``set_compute_dtype`` on the mirrors).

Whole calls.  The reference for a tower in fp16 / bf16 is the tower's fp32 fixture (``vit_tiny.npz``, ``videomae_tiny.npz``,
``clip_vision_tiny.npz``); the bound is 4 x the distance of the torch-CPU run in the same dtype from that fixture
(``tests/golden/metric_towers_16bit.npz``, ``tests/metric_dtype_rules.py``: two independent draws of the same class of rounding noise),
computed from the two fixtures when the test runs.  Max-abs distances from the fp32 fixture, torch CPU / this library on an MI355X:

    tower     quantity     fp16 CPU   fp16 device   bf16 CPU   bf16 device
    ViT       logits       6.4e-3     4.1e-3        5.8e-2     4.6e-2
    ViT       probs        1.7e-3     1.1e-3        1.1e-2     3.4e-3
    VideoMAE  logits       2.5e-3     1.1e-3        3.0e-2     1.8e-2
    VideoMAE  probs        4.4e-4     6.2e-5        2.9e-3     6.4e-4
    CLIP      embeddings   3.4e-3     3.3e-3        3.0e-2     2.4e-2
    CLIP      8 x 8 matrix 2.6e-4     4.4e-4        2.4e-3     3.1e-3

Ops.  The new ``e2v_op_tower_*`` entries against references computed on the spot: the fp32 preprocess rounded once (bit for bit),
``tests/h16_budget.py``'s ``cross_reference`` / ``attention_budget`` for the attention, float64 on the rounded rows for the mean and the
LayerNorm (``norm_budget``).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from eeg2video_amd import _lib
from eeg2video_amd.weights import TINY_CLIP_VISION, TINY_IMAGE, TINY_UNET, TINY_VAE, TINY_VIDEO, counter_normal
from h16_budget import TYPES, assert_within_budget, attention_budget, cross_reference, layernorm_reference, norm_budget, rt
from metric_dtype_rules import DTYPES, TOWERS, bound, check_row_ranking, check_top3, cpu_distance, load16, load32
from test_hip_bounds import GUARD_KIB, environment, fenced, fenced_out, run_fenced
from test_image_classifier_host import reference_n_way_top_k_acc

pytestmark = pytest.mark.gpu

FORM_BIT = {"bf16": _lib.FORM_BITS["bf16"], "fp16": _lib.FORM_BITS["fp16"]}
CODE = {"bf16": _lib.E2V_BF16, "fp16": _lib.E2V_F16}


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b, what=""):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(bits(x.cpu()), bits(y.cpu())), f"{what}: output {i} differs"


def as_kind(u8, f32, channels_last):
    """``[n,F,H,W,3]`` uint8 -> the same frames as uint8 / float32 in either layout; the float is the middle of the byte's bucket"""
    t = torch.from_numpy(np.ascontiguousarray(u8))
    if f32:
        t = (t.float() + 0.5) / 255.0
    return t if channels_last else t.permute(0, 4, 1, 2, 3).contiguous()


# ------------------------------------------------------------------ the three towers, one description each ---------------------------
class Tower:
    """``stored``: the 8 fixture images / clips as the processor left them, ``[8,(F,)S,S,3]`` uint8; ``groups``: the same 8 at their three
    source shapes.  ``run`` takes ``[n,F,H,W,3]``-shaped frames (any kind) and returns a tuple of device tensors, 8 rows for ``stored``."""

    def __init__(self, name):
        self.name = name
        self.z32 = load32(name)
        z = self.z32
        if name == "vit":
            import vit_restatement as R
            from eeg2video_amd.image_classifier import ViTForImageClassification as M
            self.cfg, self.kw, self.part, self.prefix, self.chunk = TINY_IMAGE, "image_cfg", 16, "image.", ("E2V_VIT_CHUNK", 64)
            self.groups = [z["images_36x64"], z["images_130x90"], z["images_112x112"]]
            self.stored = np.concatenate([z["resized_36x64"], z["resized_130x90"], z["images_112x112"]])
        elif name == "videomae":
            import videomae_restatement as R
            from eeg2video_amd.video_classifier import VideoMAEForVideoClassification as M
            self.cfg, self.kw, self.part, self.prefix, self.chunk = TINY_VIDEO, "video_cfg", 32, "video.", ("E2V_VMAE_CHUNK", 16)
            self.groups = [z["clips_36x64"], z["clips_90x50"], z["clips_56x56"]]
            self.stored = np.concatenate([z["cropped_36x64"], z["cropped_90x50"], z["clips_56x56"]])
        else:
            import clip_vision_restatement as R
            from eeg2video_amd.clip_vision import CLIPVisionModelWithProjection as M
            self.cfg, self.kw, self.part, self.prefix, self.chunk = TINY_CLIP_VISION, "clip_vision_cfg", 64, "clipv.", ("E2V_CLIPV_CHUNK", 256)
            pairs = R.golden_groups(z)
            self.groups = [g for g, _ in pairs]
            self.stored = np.concatenate([c for _, c in pairs])
        self.sd = R.load_golden()[1]
        self.M = M
        self.model = self.make()
        self.cache = {}

    def make(self, sd=None):
        from eeg2video_amd.engine import Engine
        return self.M(self.cfg, engine=Engine(TINY_UNET, TINY_VAE, 0, **{self.kw: self.cfg})).load_state_dict(sd or self.sd)

    def clips(self, u8):
        """fixture arrays -> ``[n,F,H,W,3]``: the classifier's images are n clips of one frame, the video's clips are clips"""
        return u8 if self.name == "videomae" else u8[:, None]

    def run(self, frames, channels_last=True, model=None):
        eng = (model or self.model).engine
        if self.name == "vit":
            return tuple(eng.classify_frames(frames, channels_last=channels_last))
        if self.name == "videomae":
            return tuple(eng.classify_clips(frames, channels_last=channels_last))
        return (eng.clip_embed(frames, channels_last=channels_last),)

    def batch8(self, dtype):
        """the 8 stored images / clips in one call in ``dtype`` (the model is left in fp32), on the host: computed once per dtype"""
        if dtype not in self.cache:
            self.model.set_compute_dtype(dtype)
            try:
                self.cache[dtype] = tuple(t.cpu() for t in self.run(torch.from_numpy(self.clips(self.stored))))
            finally:
                self.model.set_compute_dtype("fp32")
        return self.cache[dtype]


@pytest.fixture(scope="module")
def towers():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Tower(name)
        return made[name]
    return get


@pytest.fixture(scope="module")
def z16():
    return load16()


@pytest.fixture
def tw(towers, request):
    return towers(request.param)


ALL = pytest.mark.parametrize("tw", sorted(TOWERS), indirect=True)
BOTH = pytest.mark.parametrize("dtype", DTYPES)


# ------------------------------------------------------------------ 1. whole calls ---------------------------------------------------
@BOTH
@ALL
def test_whole_call_within_4x_the_cpu_16bit_distance(tw, z16, dtype):
    out = tw.batch8(dtype)
    eng = tw.model.engine
    if tw.name == "clip":
        emb = out[0]
        got = {"embeds": emb.numpy(), "pairs": eng.clip_similarity(emb, emb.roll(1, 0)).cpu().numpy(),
               "matrix": eng.clip_similarity(emb, emb, matrix=True).cpu().numpy()}
    else:
        got = {"logits": out[0].numpy(), "probs": out[1].numpy()}
    for q, key in TOWERS[tw.name][1].items():
        ref = tw.z32[key].astype(np.float64)
        err, b = float(np.abs(got[q].astype(np.float64) - ref).max()), bound(z16, tw.z32, tw.name, q, dtype)
        print(f"{tw.name} {dtype} {q}: device max |a - fp32| = {err:.3e}, torch CPU {cpu_distance(z16, tw.z32, tw.name, q, dtype):.3e}, bound {b:.3e}")
        assert got[q].dtype == np.float32 and got[q].shape == ref.shape and np.isfinite(got[q]).all()
        assert err <= b, (q, err, b)
    assert not torch.equal(bits(out[0]), bits(tw.batch8("fp32")[0]))                        # the mode is really another arithmetic
    if tw.name == "clip":
        fixed, total = check_row_ranking(got["matrix"], tw.z32["matrix"], bound(z16, tw.z32, "clip", "matrix", dtype), f"clip {dtype}")
        print(f"clip {dtype}: {fixed} of {total} column pairs determined")
        assert fixed > 0
    else:
        determined = check_top3(out[2].numpy(), tw.z32["logits"], bound(z16, tw.z32, tw.name, "logits", dtype), f"{tw.name} {dtype}")
        print(f"{tw.name} {dtype}: top-3 set determined in {determined} of 8 rows")
        assert out[2].dtype == torch.int32 and (determined == 8 or dtype == "bf16")
        # the head is fp32 and unchanged: probs and top 3 are those of the device's own logits
        assert np.abs(out[1].numpy() - torch.softmax(out[0].double(), -1).numpy()).max() < 1e-6
        assert np.array_equal(np.sort(out[2].numpy(), -1), np.sort(np.argsort(out[0].numpy(), -1, kind="stable")[:, -3:], -1))


@BOTH
@ALL
def test_source_shapes_and_frame_kinds_give_the_same_bits(tw, dtype):
    """all 8 at their three source shapes, uint8 and fp32, planar and channels-last: the 16-bit preprocess stores Pillow's bytes through the
    table rounded once, so every kind gives the bits of the stored bytes"""
    want = tw.batch8(dtype)
    tw.model.set_compute_dtype(dtype)
    try:
        i0 = 0
        for g in tw.groups:
            n = len(g)
            for f32 in (False, True):
                for cl in (True, False):
                    got = tw.run(as_kind(tw.clips(g), f32, cl), channels_last=cl)
                    same(got, tuple(t[i0:i0 + n] for t in want), f"{tw.name} {dtype} {g.shape} f32={f32} channels_last={cl}")
            i0 += n
    finally:
        tw.model.set_compute_dtype("fp32")


# ------------------------------------------------------------------ 2. determinism, and the way back to fp32 -------------------------
@BOTH
@ALL
def test_an_item_does_not_depend_on_batch_chunk_engine_mode_or_run(tw, dtype):
    want = tw.batch8(dtype)
    eng = tw.model.engine
    frames = torch.from_numpy(tw.clips(tw.stored))
    rows = lambda sl: tuple(t[sl] for t in want)
    tw.model.set_compute_dtype(dtype)
    try:
        assert tw.model.compute_dtype == dtype == eng.tower_dtype(tw.part)
        same(tw.run(frames), want, "a second run")
        for i in (0, 5, 7):
            same(tw.run(frames[i:i + 1]), rows(slice(i, i + 1)), f"item {i} alone")
        same(tw.run(frames[2:7]), rows(slice(2, 7)), "a batch of 5 from position 2")
        try:
            eng.set_knob(tw.chunk[0], 3)                                                    # chunks of 3, 3 and 2
            same(tw.run(frames), want, "chunks of 3")
            same(tw.run(as_kind(tw.clips(tw.stored), True, False), channels_last=False), want, "chunks of 3, planar floats")
        finally:
            eng.set_knob(*tw.chunk)
        for mode in ("bf16", "fp16", "fp32"):                                               # the engine's own compute dtype does not reach a tower
            try:
                eng.set_compute_dtype(mode)
                same(tw.run(frames), want, f"engine in {mode}")
            finally:
                eng.set_compute_dtype("fp32")
    finally:
        tw.model.set_compute_dtype("fp32")


@ALL
def test_back_to_fp32_restores_the_fp32_bits(tw, z16):
    """a call before any switch, then 16-bit calls, then fp32 again: the fixture-tested fp32 bits come back, whatever happened in between"""
    m = tw.make()
    frames = torch.from_numpy(tw.clips(tw.stored))
    assert m.compute_dtype == "fp32"
    before = tuple(t.cpu() for t in tw.run(frames, model=m))
    same(before, tw.batch8("fp32"), "a fresh model in its default mode")
    key = {"vit": "logits", "videomae": "logits", "clip": "image_embeds"}[tw.name]
    assert float(np.abs(before[0].numpy() - tw.z32[key]).max()) <= 1e-5 * float(np.abs(tw.z32[key]).max())     # the fp32 tests' bound
    for dtype in ("fp16", "bf16", "fp16"):
        assert m.set_compute_dtype(dtype) is m and m.compute_dtype == dtype
        same(tw.run(frames, model=m), tw.batch8(dtype), f"{dtype} on a second model")
        m.set_compute_dtype(torch.float32)
        same(tw.run(frames, model=m), before, f"fp32 after {dtype}")
    for bad in ("f32x3", "int8"):
        with pytest.raises(ValueError):
            m.set_compute_dtype(bad)
    assert m.to(torch.float16) is m and m.compute_dtype == "fp32"                           # .to() selects nothing, as before
    from eeg2video_amd.engine import Engine
    with pytest.raises(ValueError):
        m.engine.set_tower_dtype(Engine.TEXT, "fp16")
    others = [p for p in (16, 32, 64) if p != tw.part]
    with pytest.raises(RuntimeError, match="no such tower"):
        m.engine.set_tower_dtype(others[0], "fp16")


@BOTH
@ALL
def test_steady_state_takes_no_new_memory(tw, dtype):
    eng, frames = tw.model.engine, torch.from_numpy(tw.clips(tw.stored)).cuda()
    tw.model.set_compute_dtype(dtype)
    try:
        tw.run(frames)                                                                      # (builds the 16-bit copies on first use)
        torch.cuda.synchronize()
        g0, bytes0 = eng.pool_gets(), eng.device_bytes()
        tw.run(frames)
        g1 = eng.pool_gets()
        tw.run(frames)
        torch.cuda.synchronize()
        assert eng.pool_gets() - g1 == g1 - g0 > 0 and eng.device_bytes() == bytes0
    finally:
        tw.model.set_compute_dtype("fp32")


# ------------------------------------------------------------------ 3. bounds --------------------------------------------------------
@BOTH
@ALL
def test_outputs_fenced_and_pool_guarded(tw, dtype):
    """one call with E2V_POOL_GUARD on and fenced outputs: no store outside a tensor, inside the library (the 16-bit rows and the 16-bit
    weight copies built on first use included) or out of it; the guarded run gives the unguarded bits"""
    want = tw.batch8(dtype)
    n = 5
    frames = torch.from_numpy(tw.clips(tw.stored[:n])).cuda()
    nc, F, S = frames.shape[0], frames.shape[1], frames.shape[2]
    kind = _lib.E2V_FRAMES_U8 | _lib.E2V_FRAMES_CHANNELS_LAST
    with environment({}, GUARD_KIB):
        m = tw.make()
        eng = m.engine
        m.set_compute_dtype(dtype)
        eng.pool_guard_report()
        gets = eng.pool_gets()
        if tw.name == "clip":
            outs = [fenced_out((n, tw.cfg.projection_dim))]
            call = lambda: eng.lib.e2v_clip_embed(eng.ctx, frames.data_ptr(), kind, nc, F, S, S, outs[0].t.data_ptr(), None)
        else:
            L = tw.cfg.num_labels
            outs = [fenced_out((n, L)), fenced_out((n, L)), fenced_out((n, 3))]
            fn = eng.lib.e2v_image_classify if tw.name == "vit" else eng.lib.e2v_video_classify
            call = lambda: fn(eng.ctx, frames.data_ptr(), kind, nc, F, S, S, outs[0].t.data_ptr(), outs[1].t.data_ptr(), outs[2].t.data_ptr(), None)

        def checked_call():
            st = call()
            assert st == 0, eng.lib.e2v_last_error(eng.ctx)
        y = run_fenced(checked_call, outs[1:], outs[0])
        taken = eng.pool_gets() - gets
        checked, violations, text = eng.pool_guard_report()
        assert violations == 0, text
        assert taken > 0 and checked >= taken, (checked, taken)
        assert torch.equal(bits(y.cpu()), bits(want[0][:n]))
        if tw.name != "clip":
            assert torch.equal(bits(outs[1].view.cpu()), bits(want[1][:n]))
            assert torch.equal(outs[2].view.cpu().view(torch.int32), want[2][:n])


# ------------------------------------------------------------------ 4. weights: forms, update, read-back ------------------------------
@BOTH
def test_clipv_update_refreshes_the_16bit_form_and_read_tensor_reads_it(towers, dtype):
    tw = towers("clip")
    ty = TYPES[dtype]
    frames = torch.from_numpy(tw.clips(tw.stored[:3]))
    m = tw.make()
    eng = m.engine
    keys = ("vision_model.encoder.layers.1.self_attn.k_proj.weight", "vision_model.encoder.layers.0.mlp.fc2.weight",
            "vision_model.embeddings.patch_embedding.weight")
    for k in keys:
        assert eng.weight_forms("clipv." + k) == _lib.FORM_BITS["fp32"]                     # after finalize: fp32 only
        with pytest.raises(RuntimeError, match="not built"):
            eng.read_tensor("clipv." + k, form=dtype)
    m.set_compute_dtype(dtype)
    same(tw.run(frames, model=m), tuple(t[:3] for t in tw.batch8(dtype)), "before any update")
    for k in keys:                                                                          # built lazily, on the first call in the mode
        assert eng.weight_forms("clipv." + k) == _lib.FORM_BITS["fp32"] | FORM_BIT[dtype], k
        stored = eng.read_tensor("clipv." + k, form=dtype).cpu()
        assert torch.equal(bits(stored), bits(torch.from_numpy(np.asarray(tw.sd[k], dtype=np.float32)).to(ty).float())), k
    assert eng.weight_forms("clipv.visual_projection.weight") == _lib.FORM_BITS["fp32"]    # the head stays fp32
    for k in keys:
        new = torch.from_numpy(np.asarray(tw.sd[k], dtype=np.float32)) * 0.5 + 0.0123      # (not representable: the rounding shows)
        m.sync_from({k: new})
        moved = tuple(t.cpu() for t in tw.run(frames, model=m))
        assert not torch.equal(bits(moved[0]), bits(tw.batch8(dtype)[0][:3])), k
        assert torch.equal(bits(eng.read_tensor("clipv." + k, form=dtype).cpu()), bits(new.to(ty).float())), k      # the rounded bits
        assert torch.equal(bits(eng.read_tensor("clipv." + k).cpu()), bits(new)), k
        fresh_sd = dict(tw.sd)
        fresh_sd[k] = new.numpy()
        fresh = tw.make(fresh_sd)
        fresh.set_compute_dtype(dtype)
        same(moved, tw.run(frames, model=fresh), f"update of {k} against a fresh build")
        m.sync_from({k: torch.from_numpy(np.asarray(tw.sd[k], dtype=np.float32))})
        same(tw.run(frames, model=m), tuple(t[:3] for t in tw.batch8(dtype)), f"{k} put back")
    m.set_compute_dtype("fp32")                                                             # the unused form is kept, and the fp32 path ignores it
    same(tw.run(frames, model=m), tuple(t[:3] for t in tw.batch8("fp32")), "fp32 after the updates")
    assert eng.weight_forms("clipv." + keys[0]) == _lib.FORM_BITS["fp32"] | FORM_BIT[dtype]


# ------------------------------------------------------------------ 5. ops -----------------------------------------------------------
def lut3():
    from vit_restatement import pixel_table
    return pixel_table(1 / 255, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


PREP_CASES = [("vit", 288, 512, 224, 16, 1, 0), ("vit", 30, 20, 32, 8, 1, 0), ("vit", 260, 2, 16, 8, 1, 0),
              ("videomae", 36, 64, 32, 8, 2, 32), ("videomae", 131, 50, 24, 8, 2, 29),      # tall, (nh - S) odd: an odd crop remainder
              ("clip", 288, 512, 224, 32, 1, 224), ("clip", 131, 90, 48, 16, 1, 51)]


@BOTH
@pytest.mark.parametrize("name,h,w,size,patch,ts,edge", PREP_CASES)
def test_op_preprocess_is_the_fp32_preprocess_rounded_once(towers, dtype, name, h, w, size, patch, ts, edge):
    tw = towers(name)
    eng = tw.model.engine
    rng = np.random.default_rng(h * 7 + w)
    F = 2 * ts
    clips = rng.integers(0, 256, (2, F, h, w, 3), dtype=np.uint8)
    lut = lut3()
    want = None
    for f32 in (False, True):
        for cl in (True, False):
            x = as_kind(clips, f32, cl)
            if name == "vit":
                ref = eng.op_image_preprocess(x, size=size, patch=patch, lut=lut, channels_last=cl)
            elif name == "videomae":
                ref = eng.op_video_preprocess(x, size=size, patch=patch, tubelet=ts, edge=edge, lut=lut, channels_last=cl)
            else:
                ref = eng.op_clip_preprocess(x, size=size, patch=patch, edge=edge, filter=3, lut=lut, channels_last=cl)
            got = eng.op_tower_preprocess(x, tower=tw.part, dtype=dtype, size=size, patch=patch, lut=lut, tubelet=ts, edge=edge, filter=3,
                                          channels_last=cl)
            assert got.shape == ref.shape
            assert torch.equal(bits(got), bits(ref.to(TYPES[dtype]).float())), (f32, cl, int((got != ref.to(TYPES[dtype]).float()).sum()))
            if want is None:
                want = got
                assert not torch.equal(bits(got), bits(ref))                                # (the table's values are not 16-bit numbers)
            assert torch.equal(bits(got), bits(want)), (f32, cl)


@BOTH
def test_op_preprocess_reads_bytes_at_odd_alignment_and_is_fenced(towers, dtype):
    tw = towers("vit")
    eng = tw.model.engine
    rng = np.random.default_rng(3)
    flat = torch.from_numpy(rng.integers(0, 256, (1 + 2 * 9 * 11 * 3,), dtype=np.uint8)).cuda()
    view = flat[1:].view(1, 2, 9, 11, 3)                                                    # starts at an odd byte
    lut = np.ascontiguousarray(lut3())
    a = eng.op_tower_preprocess(view, tower=16, dtype=dtype, size=16, patch=8, lut=lut, channels_last=True)
    b = eng.op_image_preprocess(view.cpu().clone(), size=16, patch=8, lut=lut, channels_last=True)
    assert torch.equal(bits(a), bits(b.to(TYPES[dtype]).float()))
    out = fenced_out((2 * 4, 3 * 64))
    kind = _lib.E2V_FRAMES_U8 | _lib.E2V_FRAMES_CHANNELS_LAST

    def call():
        st = eng.lib.e2v_op_tower_preprocess(eng.ctx, 16, CODE[dtype], view.data_ptr(), kind, 1, 2, 9, 11, 16, 8, 1, 0, 3,
                                             lut.ctypes.data_as(C.POINTER(C.c_float)), out.t.data_ptr(), None)
        assert st == 0, eng.lib.e2v_last_error(eng.ctx)
    assert torch.equal(bits(run_fenced(call, [], out)), bits(a))


@BOTH
@pytest.mark.parametrize("t", [1, 31, 32, 33, 50, 64, 65, 147, 197, 257, 588])
def test_op_attention_within_the_rounding_budget(towers, dtype, t):
    """non-causal attention at D = 64, 2 heads, as a 16-bit tower runs it; T up to 96 takes the resident-keys kernel, longer ones the
    staged one (32- and 64-key stages, ragged last tiles and query blocks)"""
    eng = towers("vit").model.engine
    b, heads = 3, 2
    c = 64 * heads
    qkv = torch.from_numpy(counter_normal(170 + t, "tower_qkv", (b * t, 3 * c))) * torch.tensor([1.5, 1.5, 1.0]).repeat_interleave(c)
    fi, fo = fenced(qkv, ld=3 * c + 8, name="qkv"), fenced_out((b * t, c), ld=c + 4)

    def call():
        st = eng.lib.e2v_op_tower_attention(eng.ctx, CODE[dtype], fi.t.data_ptr(), fi.ld, fo.t.data_ptr(), fo.ld, b, t, heads, None)
        assert st == 0, eng.lib.e2v_last_error(eng.ctx)
    y = run_fenced(call, [fi], fo).cpu()
    q, k, v = qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:]
    ref = cross_reference(q, k, v, n=b, F=1, heads=heads, Nq=t, Nk=t, scale=0.125, ty=dtype)
    worst = assert_within_budget(y, ref["ref"], attention_budget(ref, dtype), f"tower attention {dtype} T={t}")
    print(f"T={t} {dtype}: worst error / budget {worst:.3f}")
    assert torch.equal(bits(y), bits(y.to(TYPES[dtype]).float()))                           # the output was stored in 16 bits
    assert torch.equal(bits(eng.op_tower_attention(qkv, dtype=dtype, B=b, T=t, heads=heads).cpu()), bits(y))
    if t in (50, 147):                                                                      # a sequence's rows do not depend on the batch
        assert torch.equal(bits(eng.op_tower_attention(qkv[t:2 * t], dtype=dtype, B=1, T=t, heads=heads).cpu()), bits(y[t:2 * t]))


@BOTH
@pytest.mark.parametrize("B,T,C", [(3, 147, 128), (2, 7, 132), (1, 588, 768), (5, 8, 4)])
def test_op_token_mean_against_float64(towers, dtype, B, T, C):
    """fp32 sum over the rounded rows in index order, one division: |error| <= T 2^-24 mean|x| (the chain of T fp32 additions and the
    division, each relative 2^-24 of a partial sum bounded by sum|x|)"""
    eng = towers("videomae").model.engine
    x = torch.from_numpy(counter_normal(300 + T, "tower_mean", (B * T, C))) * 3.0 + 0.5
    xr = rt(x, dtype).double().view(B, T, C)
    fo = fenced_out((B, C))
    xd = x.cuda()

    def call():
        st = eng.lib.e2v_op_tower_token_mean(eng.ctx, CODE[dtype], xd.data_ptr(), B, T, C, fo.t.data_ptr(), None)
        assert st == 0, eng.lib.e2v_last_error(eng.ctx)
    y = run_fenced(call, [], fo).cpu().double()
    budget = T * 2.0 ** -24 * xr.abs().mean(1) + 2.0 ** -149
    err = (y - xr.mean(1)).abs()
    print(f"token mean {dtype} {B}x{T}x{C}: worst error / budget {float((err / budget).max()):.3f}")
    assert (err <= budget).all()
    seq = xr.float()[:, 0]
    for i in range(1, T):
        seq = seq + xr.float()[:, i]
    assert torch.equal(bits(y.float()), bits(seq / T))                                      # index order, bit for bit


@BOTH
@pytest.mark.parametrize("rows,stride,C,eps", [(5, 50, 128, 1e-5), (3, 197, 768, 1e-12), (4, 1, 132, 1e-6), (2, 3, 1024, 1e-5), (9, 2, 1280, 1e-5)])
def test_op_layernorm_16bit_rows_to_fp32_against_float64(towers, dtype, rows, stride, C, eps):
    """the strided class-row form (stride = T) and the dense form (stride 1), at the towers' eps values; the result is not rounded"""
    eng = towers("vit").model.engine
    total = (rows - 1) * stride + 1
    x = torch.from_numpy(counter_normal(400 + C + stride, "tower_ln", (total, C))) * 2.0 + 0.25
    gamma = torch.from_numpy(counter_normal(401 + C, "tower_ln_g", (C,))) * 0.25 + 1.0
    beta = torch.from_numpy(counter_normal(402 + C, "tower_ln_b", (C,))) * 0.1
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    fo = fenced_out((rows, C))

    def call():
        st = eng.lib.e2v_op_tower_layernorm(eng.ctx, CODE[dtype], xd.data_ptr(), rows, stride, C, gd.data_ptr(), bd.data_ptr(), float(eps),
                                            fo.t.data_ptr(), None)
        assert st == 0, eng.lib.e2v_last_error(eng.ctx)
    y = run_fenced(call, [], fo).cpu()
    ref = layernorm_reference(rt(x, dtype)[::stride][:rows], gamma, beta, eps=eps)
    worst = assert_within_budget(y, ref["ref"], norm_budget(ref, gamma, dtype), f"tower layernorm {dtype} C={C} stride={stride}")
    # the output is not rounded, so the budget's rounding term (2 u |ref|) is idle here: the statistics term alone has to hold it
    from h16_budget import DELTA
    stats_only = DELTA * gamma.double().abs() * (ref["xhat"].abs() + ref["mu"].abs() * ref["rstd"] + 1.0)
    tight = assert_within_budget(y, ref["ref"], stats_only, f"tower layernorm {dtype} C={C} stride={stride}, statistics term alone")
    print(f"layernorm {dtype} rows={rows} stride={stride} C={C}: worst error / budget {worst:.3f}, / its statistics term {tight:.3f}")
    assert not torch.equal(bits(y), bits(y.to(TYPES[dtype]).float()))                       # fp32 out: NOT rounded to the storage type
    same(eng.op_tower_layernorm(x, gamma, beta, dtype=dtype, rows=rows, stride=stride, eps=eps), y, "the wrapper")
    wrong = layernorm_reference(rt(x, dtype)[::stride][:rows], gamma, beta, eps=1e-2)["ref"]      # the eps reaches the kernel
    if eps <= 1e-5:
        assert float((y.double() - wrong).abs().max()) > 10 * float((y.double() - ref["ref"]).abs().max())


@BOTH
@pytest.mark.parametrize("act", [0, 1])
def test_op_activation_and_embed_round_once(towers, dtype, act):
    eng = towers("vit").model.engine
    ty = TYPES[dtype]
    u = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}[dtype]
    x = torch.from_numpy(counter_normal(500 + act, "tower_act", (37, 136))) * 3.0
    y = eng.op_tower_activation(x, dtype=dtype, act=act).cpu()
    xr = rt(x, dtype).double()
    ref = xr * torch.sigmoid(1.702 * xr) if act == 0 else 0.5 * xr * (1.0 + torch.erf(xr / 2 ** 0.5))
    assert torch.equal(bits(y), bits(y.to(ty).float()))
    # one rounding of the stored value (u |ref|, the subnormal step for fp16) + the fp32 evaluation of exp / erf (1e-6 absolute)
    assert ((y.double() - ref).abs() <= u * ref.abs() + 2.0 ** -24 + 1e-6).all()
    nimg, T, C = 3, 5, 132
    pos = torch.from_numpy(counter_normal(510, "tower_pos", (T, C)))
    cls = torch.from_numpy(counter_normal(511, "tower_cls", (C,)))
    for with_cls in (True, False):
        p = torch.from_numpy(counter_normal(512 + with_cls, "tower_patches", (nimg * (T - 1 if with_cls else T), C))) * 2.0
        got = eng.op_tower_embed(p, pos, dtype=dtype, nimg=nimg, cls=cls if with_cls else None).cpu()
        pr = rt(p, dtype)
        if with_cls:
            tok = torch.cat([cls.expand(nimg, 1, C), pr.view(nimg, T - 1, C)], 1)
        else:
            tok = pr.view(nimg, T, C)
        want = (tok + pos[None]).to(ty).float().view(nimg * T, C)                           # one fp32 addition, one rounding: exact
        assert torch.equal(bits(got), bits(want)), with_cls


# ------------------------------------------------------------------ 6. the metrics use whatever the model is set to -------------------
@BOTH
def test_metrics_with_a_16bit_model_equal_the_cpu_route_on_the_devices_own_outputs(towers, dtype):
    """``img_classify_metric``, ``video_classify_metric`` and ``n_way_scores`` take the model as it is set: the seeded CPU route fed the
    DEVICE's own 16-bit-mode probs / top 3 / matrix gives the same lists"""
    from clip_vision_restatement import reference_n_way
    from eeg2video_amd.metrics import img_classify_metric, n_way_scores, video_classify_metric
    for name, metric, pred_idx, gt_idx in (("vit", img_classify_metric, list(range(0, 6)), list(range(2, 8))),
                                           ("videomae", video_classify_metric, [0, 1, 2, 3, 4], [3, 4, 5, 6, 7])):
        tw = towers(name)
        logits, probs, top3 = tw.batch8(dtype)
        tw.model.set_compute_dtype(dtype)
        try:
            for n_way, top_k in ((2, 1), (40, 1), (40, 3)):
                np.random.seed(5)
                got_acc, got_std = metric(tw.stored[pred_idx], tw.stored[gt_idx], n_way=n_way, num_trials=20, top_k=top_k, return_std=True,
                                          model=tw.model)
                np.random.seed(5)
                want = [reference_n_way_top_k_acc(probs[p], [int(i) for i in top3[g]], n_way, 20, top_k) for p, g in zip(pred_idx, gt_idx)]
                assert got_acc == [a for a, _ in want] and got_std == [s for _, s in want], (name, n_way, top_k)
        finally:
            tw.model.set_compute_dtype("fp32")
    tw = towers("clip")
    emb = tw.batch8(dtype)[0]
    device = tw.model.engine.clip_similarity(emb, emb.roll(1, 0), matrix=True).cpu().numpy()
    pred, gt = tw.stored, np.roll(tw.stored, 1, 0)
    tw.model.set_compute_dtype(dtype)
    try:
        for n_way, top_k, trials in ((2, 1, 10), (5, 1, 6), (8, 3, 4)):
            np.random.seed(9)
            got = n_way_scores(pred, gt, n_way=n_way, top_k=top_k, num_trials=trials, model=tw.model)
            np.random.seed(9)
            assert got == reference_n_way(list(range(8)), list(range(8)), lambda p, g: float(device[p, g]), n_way, top_k, trials), (n_way, top_k)
    finally:
        tw.model.set_compute_dtype("fp32")
