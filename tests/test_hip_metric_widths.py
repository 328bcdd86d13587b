"""GPU: the three metric towers (``e2v_image_classify``, ``e2v_video_classify``, ``e2v_clip_embed``) at the widths the metrics run
them at, and the classifier head (``image_head_kernel``, ``csrc/vit.hip``) beyond 64 labels.

The towers' own modules run ``hidden=128, heads=2, intermediate=256`` with 50 labels: a lane of the embed kernels takes no second
step there, a lane of the head holds at most one logit, the class-row LayerNorm runs at C = 128 only and the tile planner
(``csrc/gemm_sched.h``) has one choice.  Here:

1. one layer at ViT-B/16, VideoMAE-B (2 frames), CLIP-B/32 and CLIP-L/14 widths against the float64 restatements
   (``vit_restatement.py``, ``videomae_restatement.py``, ``clip_vision_restatement.py``), synthetic weights with the q / k projections
   scaled by 4 as ``test_hip_text.synth_text`` does.  Metric and bound: max |a-b| / max |b| < 1e-5, the project's fp32 bound;
2. an image's bits do not depend on the batch, the chunk or the compute mode at these widths -- and, for ViT-B/16 and CLIP-B/32, in a
   batch large enough for the planner to cut 128 x 128 tiles, which the three-image calls never reach (the test prints and checks the
   recorded dispatch of ``op_linear`` on the same shapes);
3. the head on chosen logits: with a zero classifier weight the logits are the bias, so the top-3 insertion chain, the pop, ties and
   the strided softmax are driven through the public call for L in {3, 64, 65, 130, 400, 1000};
4. one run per tower with ``E2V_POOL_GUARD`` on and fenced outputs.

Inputs are random bytes already at S x S: every resize is the identity (the preprocess tests are in the towers' modules).
"""
import dataclasses

import numpy as np
import pytest
import torch

from clip_vision_restatement import clip_vision_forward
from eeg2video_amd import _lib
from eeg2video_amd.weights import (TINY_IMAGE, TINY_UNET, TINY_VAE, TINY_VIDEO, ClipVisionConfig, ImageConfig, VideoConfig,
                                   clip_vision_param_spec, counter_normal, image_param_spec, synth_state_dict, video_checkpoint_spec,
                                   video_position_table)
from test_hip_bounds import GUARD_KIB, environment, fenced_out, run_fenced
from videomae_restatement import tubelet_rows, videomae_forward
from vit_restatement import patch_rows, pixel_table, rel_err, softmax64, top3, vit_forward

pytestmark = pytest.mark.gpu

BOUND = 1e-5
PROB_BOUND = 1e-6                  # probs against the float64 softmax of the device's own logits, absolute (test_hip_image_classifier.py)
U8CL = _lib.E2V_FRAMES_U8 | _lib.E2V_FRAMES_CHANNELS_LAST


# ------------------------------------------------------------------ the four configurations -----------------------------------------
@dataclasses.dataclass(frozen=True)
class Tower:
    kind: str                      # "image" | "video" | "clip"
    cfg: object
    n: int                         # images (clips) of the base call
    seed: int                      # of the weights and the frames; checked on the CPU: the reference's top 4 logits are apart
    knob: str
    knob_default: int
    wide_batch: int = 0            # images at which the fc1 GEMM gets 128 x 128 tiles (0: not run)

    @property
    def out_dim(self):
        return self.cfg.projection_dim if self.kind == "clip" else self.cfg.num_labels


TOWERS = {
    # 197 tokens, K = 768 patch rows, 1000 labels: 16 logits per lane of the head
    "vit_b16": Tower("image", ImageConfig(layers=1), 3, 11, "E2V_VIT_CHUNK", 64, wide_batch=12),
    # 196 tokens (3 key tiles + 4 keys, a 4-row tail in token_mean), K = 1536, 400 labels
    "videomae_b": Tower("video", VideoConfig(layers=1, num_frames=2), 2, 12, "E2V_VMAE_CHUNK", 16),
    # 50 tokens, K = 3072, projection 512
    "clip_b32": Tower("clip", ClipVisionConfig(layers=1), 3, 13, "E2V_CLIPV_CHUNK", 256, wide_batch=48),
    # 257 tokens (4 keys per lane + 1), K = 588 (9 whole 64-deep steps + 12), LayerNorm-1024, projection 768
    "clip_l14": Tower("clip", ClipVisionConfig(hidden=1024, heads=16, layers=1, intermediate=4096, patch_size=14, projection_dim=768), 3, 14,
                      "E2V_CLIPV_CHUNK", 256),
}
NAMES = list(TOWERS)


def make_engine(t):
    from eeg2video_amd.engine import Engine
    return Engine(TINY_UNET, TINY_VAE, 0, **{{"image": "image_cfg", "video": "video_cfg", "clip": "clip_vision_cfg"}[t.kind]: t.cfg})


def make_model(t, sd, engine=None):
    if t.kind == "image":
        from eeg2video_amd.image_classifier import ViTForImageClassification as cls
    elif t.kind == "video":
        from eeg2video_amd.video_classifier import VideoMAEForVideoClassification as cls
    else:
        from eeg2video_amd.clip_vision import CLIPVisionModelWithProjection as cls
    return cls(t.cfg, engine=engine or make_engine(t)).load_state_dict(sd)


def synth(t):
    """counter-RNG weights under the checkpoint's names; q / k projections scaled up so that the softmax rows are far from uniform"""
    spec = {"image": image_param_spec, "video": video_checkpoint_spec, "clip": clip_vision_param_spec}[t.kind](t.cfg)
    sd = synth_state_dict(spec, seed=t.seed, mode="perturbed")
    for k in sd:
        if k.endswith(("query.weight", "key.weight", "q_proj.weight", "k_proj.weight")):
            sd[k] = sd[k] * 4.0
    return sd


def draw_frames(t, n, seed):
    """``n`` random images (clips) of S x S bytes as the entry point takes them, channels last: image / clip ``[1,n,S,S,3]`` (one clip
    of n frames), video ``[n,F,S,S,3]``"""
    s = t.cfg.image_size
    shape = (n, t.cfg.num_frames, s, s, 3) if t.kind == "video" else (1, n, s, s, 3)
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8))


def pick(t, frames, rows):
    return frames[rows] if t.kind == "video" else frames[:, rows]


def run(t, eng, frames):
    """the entry point's outputs on the host: ``(logits, probs, top3)`` or ``(image_embeds,)``"""
    if t.kind == "image":
        out = eng.classify_frames(frames, channels_last=True)
    elif t.kind == "video":
        out = eng.classify_clips(frames, channels_last=True)
    else:
        out = (eng.clip_embed(frames, channels_last=True),)
    return tuple(o.cpu() for o in out)


def reference(t, sd, frames):
    """the float64 restatement on the patch rows of the bytes (the config's pixel table) -> ``[n, out_dim]``"""
    c = t.cfg
    lut = pixel_table(c.rescale_factor, c.image_mean, c.image_std)
    f = frames.numpy()
    if t.kind == "video":
        rows = np.stack([tubelet_rows(clip, lut, c.patch_size, c.tubelet_size) for clip in f])
        return videomae_forward(sd, rows, video_position_table(c.tokens, c.hidden), c.heads, c.layer_norm_eps)
    rows = np.stack([patch_rows(img, lut, c.patch_size) for img in f[0]])
    if t.kind == "image":
        return vit_forward(sd, rows, c.heads, c.layer_norm_eps)
    return clip_vision_forward(sd, rows, c.heads, c.layer_norm_eps, c.hidden_act)


def bits(x):
    return x.contiguous().view(torch.int32)


def same(got, want, rows, what):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w[rows].shape and torch.equal(bits(g), bits(w[rows])), what


@pytest.fixture(scope="module")
def tower():
    """name -> the configuration with its weights, model, frames, float64 reference and the base result (all of the frames in one
    call), built once for sections 1, 2 and 4"""
    cache = {}

    def get(name):
        if name not in cache:
            t = TOWERS[name]
            sd = synth(t)
            frames = draw_frames(t, t.n, t.seed)
            ref = reference(t, sd, frames)
            if t.kind != "clip":                                                            # on the reference, before any device result exists
                gap = top4_gap(ref)
                assert gap >= 1e-4, f"{name}: seed {t.seed} leaves two of the reference's top 4 logits {gap:.2e} of the largest apart: pick another"
            model = make_model(t, sd)
            cache[name] = dict(t=t, sd=sd, frames=frames, ref=ref, model=model, eng=model.engine, base=run(t, model.engine, frames))
        return cache[name]
    return get


# ------------------------------------------------------------------ 1. one layer at the real widths ---------------------------------
def top4_gap(ref):
    """the smallest distance between two of an image's four largest logits, over max |logits|"""
    four = np.sort(ref, axis=-1)[:, -4:]
    return float(np.diff(four, axis=-1).min() / np.abs(ref).max())


@pytest.mark.parametrize("name", NAMES)
def test_one_layer_at_real_widths_vs_float64(tower, name):
    """logits / embeddings of 3 images (2 clips) against the float64 restatement, and for the classifiers the head's two other
    outputs: the softmax of the device's own logits and their top 3 -- which are the reference's top 3 too, the reference's four
    largest logits being further apart (at least 1e-4 of the largest: the fixture asserts it before the device runs; 2.3e-3 and
    7.3e-3 for the seeds here) than the bound moves one.

    Measured on an MI355X: vit_b16 1.56e-6, videomae_b 7.9e-7, clip_b32 1.19e-6, clip_l14 1.31e-6; the same restatements run in
    fp32 numpy on the CPU sit 4.8e-7, 3.2e-7, 6.6e-7 and 9.8e-7 from float64."""
    c = tower(name)
    t, ref, out = c["t"], c["ref"], c["base"]
    classifier = t.kind != "clip"
    y = out[0]
    err = rel_err(y, ref)
    print(f"\n{name} ({t.n} x {t.cfg.tokens} tokens, hidden {t.cfg.hidden}): max|a-b|/max|b| = {err:.3e} (bound {BOUND:.0e})")
    assert y.shape == (t.n, t.out_dim) and y.dtype == torch.float32 and not torch.isnan(y).any()
    assert err < BOUND, err
    if classifier:
        logits, probs, t3 = out
        perr = float(np.abs(probs.double().numpy() - softmax64(logits.numpy())).max())
        print(f"{name}: probs vs the float64 softmax of the device's logits {perr:.3e} (bound {PROB_BOUND:.0e})")
        assert probs.shape == logits.shape and probs.dtype == torch.float32 and perr < PROB_BOUND, perr
        assert t3.shape == (t.n, 3) and t3.dtype == torch.int32
        assert np.array_equal(t3.numpy(), top3(logits.numpy()))                             # whatever the arithmetic error
        assert np.array_equal(t3.numpy(), top3(ref))


# ------------------------------------------------------------------ 2. batch, chunk and mode ----------------------------------------
def linear_dispatch(eng, m, k, n):
    """which kernel and tile schedule serve an fp32 linear of this shape: the entry points hand ``Runner::linear`` the same launch
    description ``e2v_op_linear`` builds, and only the kernel-level calls are recorded"""
    x, w, b = (torch.zeros(s, device="cuda") for s in ((m, k), (n, k), (n,)))
    eng.op_linear(x, w, b)
    return eng.last_dispatch().strip()


def tower_dispatch(t, eng, images):
    """the recorded dispatch of the patch projection, the fc1 linear and the head at ``images`` images"""
    c = t.cfg
    k = 3 * c.patch_size ** 2 * (c.tubelet_size if t.kind == "video" else 1)
    per = c.tokens if t.kind == "video" else c.tokens - 1
    eng.set_knob("E2V_OP_RECORD", 1)
    try:
        return {"patch": linear_dispatch(eng, images * per, k, c.hidden),
                "fc1": linear_dispatch(eng, images * c.tokens, c.hidden, c.intermediate),
                "head": linear_dispatch(eng, images, c.hidden, t.out_dim)}
    finally:
        eng.set_knob("E2V_OP_RECORD", 0)


@pytest.mark.parametrize("name", NAMES)
def test_batch_chunk_and_mode_do_not_show(tower, name):
    """each image (clip) alone, chunks of 1 and 2, and the 16-bit compute modes give the bits of the one call over all of them.  The
    recorded dispatch of the patch projection, fc1 and the head is printed at both row counts: on an MI355X all of them answer
    ``rb1=0`` (128 x 64 tiles only, less than one round of the chip) at M = the batch and at M = one image, so this test compares
    launches that differ in their row-block count alone; the next test supplies a second schedule."""
    c = tower(name)
    t, eng, frames, base = c["t"], c["eng"], c["frames"], c["base"]
    for what, images in (("the batch", t.n), ("one image", 1)):
        for layer, tag in tower_dispatch(t, eng, images).items():
            print(f"\n{name} {layer} at {what}: {tag}", end="")
    same(run(t, eng, frames), base, slice(0, t.n), "a second run")
    for i in range(t.n):
        same(run(t, eng, pick(t, frames, slice(i, i + 1))), base, slice(i, i + 1), f"{i} alone")
    for chunk in (1, 2):
        try:
            eng.set_knob(t.knob, chunk)
            same(run(t, eng, frames), base, slice(0, t.n), f"chunks of {chunk}")
        finally:
            eng.set_knob(t.knob, t.knob_default)
    for mode in ("bf16", "fp16"):
        try:
            eng.set_compute_dtype(mode)
            same(run(t, eng, frames), base, slice(0, t.n), mode)
        finally:
            eng.set_compute_dtype("fp32")


@pytest.mark.parametrize("name", [n for n in NAMES if TOWERS[n].wide_batch])
def test_an_image_in_a_batch_that_gets_wide_tiles(tower, name):
    """three images never fill one round of the chip, so every GEMM of the tests above runs as 128 x 64 tiles whatever M is.  Here the
    base images lead a batch whose fc1 GEMM the planner cuts into 128 x 128 tiles followed by a half-size tail (``rb1`` > 0 in the
    recorded dispatch; checked, so that the test says so if a planner change takes its subject away): the same bits again."""
    c = tower(name)
    t, eng, frames, base = c["t"], c["eng"], c["frames"], c["base"]
    small, wide = tower_dispatch(t, eng, t.n), tower_dispatch(t, eng, t.wide_batch)
    print(f"\n{name} fc1 at {t.n} images: {small['fc1']}\n{name} fc1 at {t.wide_batch} images: {wide['fc1']}")
    assert "rb1=0 " in small["fc1"] and "rb1=" in wide["fc1"] and "rb1=0 " not in wide["fc1"], (small, wide)
    more = draw_frames(t, t.wide_batch - t.n, t.seed + 100)
    batch = torch.cat([frames, more], dim=1)
    out = run(t, eng, batch)
    assert not torch.isnan(out[0]).any()
    same([o[:t.n] for o in out], base, slice(0, t.n), f"the base images in a batch of {t.wide_batch}")


# ------------------------------------------------------------------ 3. the head on chosen logits ------------------------------------
HEAD_CASES = [("image", 3), ("image", 64), ("image", 65), ("image", 130), ("image", 400), ("image", 1000), ("video", 400), ("video", 1000)]


def head_vectors(L):
    """name -> fp32 ``[L]``: the logits the head is driven with.  Lane ``j % 64`` of the kernel holds logits j, j + 64, ...; cases that
    need more logits than L are left out."""
    base = counter_normal(L, "head_logits", (L,)).astype(np.float32)                        # distinct values, |.| < 8
    assert len(np.unique(base)) == L and np.abs(base).max() < 8 and (base > 0).any() and (base < 0).any()
    out = {}

    def plant(name, idx, vals, onto=base):
        if max(idx) < L and min(idx) >= 0 and len(set(idx)) == len(idx):
            v = onto.copy()
            v[list(idx)] = vals
            out[name] = v

    # the three largest on ONE lane (the pop runs twice); descending, ascending and mixed index order: the three branches of the chain
    for name, vals in (("descending", (30, 20, 10)), ("ascending", (10, 20, 30)), ("mixed, largest in the middle", (20, 30, 10)),
                       ("mixed, smallest in the middle", (30, 10, 20))):
        plant(f"one lane, {name}", (1, 65, 129), vals)
        plant(f"one lane's last three, {name}", (L - 129, L - 65, L - 1), vals)
    # three lanes; two on one lane and one on another, the lone one first, second and third
    plant("three lanes, first step", (0, 1, 2), (10, 30, 20))
    plant("three lanes, one wave", (5, 17, 40), (20, 10, 30))
    plant("three lanes, later steps", (5, 64 + 17, 128 + 40), (30, 20, 10))
    for name, vals in (("lone third", (30, 20, 10)), ("lone second", (30, 10, 20)), ("lone first", (20, 10, 30)), ("lone first, pair ascending", (10, 20, 30))):
        plant(f"two on a lane and one, {name}", (0, 64, 10), vals)
    # exact ties: argsort's stable order, the larger index last
    out["all equal"] = np.full(L, 0.5, dtype=np.float32)
    five = [i for i in (0, 64, 128, 10, 20, 33, 47) if i < L][:5]
    if len(five) == 5:
        plant("the top value five times", five, 30)
    tied = [i for i in (2, 66, 30, 130) if i < L]
    if len(tied) >= 2:
        plant("a tie for third place", [5, 6] + tied, [30, 20] + [10] * len(tied))
        plant("a tie for second and third place", [5] + tied, [30] + [10] * len(tied))
    # sign and range
    out["all negative"] = base - np.float32(10)
    out["around zero"] = base
    plant("one logit 80 above the rest", (L // 2,), np.float32(base.max() + 80))
    out["magnitude 1e4"] = base * np.float32(1e4)
    assert all(v.dtype == np.float32 and v.shape == (L,) and not np.signbit(v[v == 0]).any() for v in out.values())
    return out


def test_head_vectors_pin_the_expectation():
    """``top3()`` is ``torch.argsort(..., stable=True)[-3:]`` on every vector the head is driven with (ties included), and the case
    list reaches what it is for: at L >= 130 three logits on one lane, at L = 3 one logit a lane (host arithmetic only)"""
    for L in sorted({L for _, L in HEAD_CASES}):
        vs = head_vectors(L)
        for name, v in vs.items():
            assert np.array_equal(top3(v), torch.argsort(torch.from_numpy(v), dim=-1, stable=True)[-3:].numpy().astype(np.int32)), (L, name)
        assert ("one lane, descending" in vs) == (L >= 130) and ("two on a lane and one, lone third" in vs) == (L >= 65)
        assert "three lanes, first step" in vs and "all equal" in vs and ("a tie for third place" in vs) == (L >= 31)
    assert np.array_equal(top3(head_vectors(400)["all equal"]), [397, 398, 399])
    assert np.array_equal(top3(head_vectors(400)["the top value five times"]), [20, 64, 128])


def head_tower(kind, L):
    if kind == "image":
        return Tower("image", dataclasses.replace(TINY_IMAGE, layers=1, num_labels=L), 2, 21, "E2V_VIT_CHUNK", 64)
    return Tower("video", dataclasses.replace(TINY_VIDEO, layers=1, num_labels=L), 2, 22, "E2V_VMAE_CHUNK", 16)


@pytest.mark.parametrize("kind,L", HEAD_CASES)
def test_head_on_chosen_logits(kind, L):
    """a zero classifier weight makes every image's logits the bias exactly (0 * x sums to +0): logits bit for bit, ``top3`` as the
    stable argsort has it, ``probs`` within 1e-6 of the float64 softmax -- then each output alone, the other two pointers null"""
    t = head_tower(kind, L)
    sd = synth(t)
    sd["classifier.weight"] = np.zeros_like(sd["classifier.weight"])
    frames = draw_frames(t, t.n, t.seed)
    eng = make_engine(t)
    for name, bias in head_vectors(L).items():
        sd["classifier.bias"] = bias
        make_model(t, sd, engine=eng)                                                       # (the towers are frozen: a fresh load)
        logits, probs, t3 = run(t, eng, frames)
        want = torch.from_numpy(bias)
        for i in range(t.n):
            assert torch.equal(bits(logits[i]), bits(want)), (name, i)
            assert np.array_equal(t3[i].numpy(), top3(bias)), (name, i, t3[i].tolist(), top3(bias).tolist())
        perr = float(np.abs(probs.double().numpy() - softmax64(bias)[None]).max())
        assert not torch.isnan(probs).any() and perr < PROB_BOUND, (name, perr)
    # the last vector again, one output at a time: only what is asked for is written, and it carries the same bits
    dev = frames.cuda()
    n, f, s = (t.n, t.cfg.num_frames, t.cfg.image_size) if kind == "video" else (1, t.n, t.cfg.image_size)
    entry = eng.lib.e2v_video_classify if kind == "video" else eng.lib.e2v_image_classify
    for which, (shape, want) in enumerate((((t.n, L), logits), ((t.n, L), probs), ((t.n, 3), t3))):
        only = fenced_out(shape)
        ptrs = [None, None, None]
        ptrs[which] = only.t.data_ptr()

        def call():
            st = entry(eng.ctx, dev.data_ptr(), U8CL, n, f, s, s, *ptrs, None)
            assert st == 0, eng.lib.e2v_last_error(eng.ctx)
        y = run_fenced(call, [], only).cpu()
        assert torch.equal(bits(y), bits(want)), which                                      # (words: the fence is float-typed, top3 int32)


# ------------------------------------------------------------------ 4. guarded and fenced at the real widths ------------------------
@pytest.mark.parametrize("name", ["vit_b16", "videomae_b", "clip_l14"])
def test_outputs_fenced_and_pool_guarded_at_real_widths(tower, name):
    """one call with E2V_POOL_GUARD on (a NaN-filled pool with guard bands) and fenced outputs: no store outside a block or a tensor,
    and the unguarded base's bits -- a read of pool memory nobody wrote (a K = 588 tail, the class-row LayerNorm past its row) would
    show"""
    c = tower(name)
    t, base = c["t"], c["base"]
    dev = c["frames"].cuda()
    n, f, s = (t.n, t.cfg.num_frames, t.cfg.image_size) if t.kind == "video" else (1, t.n, t.cfg.image_size)
    with environment({}, GUARD_KIB):
        eng = make_model(t, c["sd"]).engine
        eng.pool_guard_report()
        shapes = [(t.n, t.out_dim)] if t.kind == "clip" else [(t.n, t.out_dim), (t.n, t.out_dim), (t.n, 3)]
        outs = [fenced_out(sh) for sh in shapes]
        entry = {"image": eng.lib.e2v_image_classify, "video": eng.lib.e2v_video_classify, "clip": eng.lib.e2v_clip_embed}[t.kind]
        gets = eng.pool_gets()

        def call():
            st = entry(eng.ctx, dev.data_ptr(), U8CL, n, f, s, s, *[o.t.data_ptr() for o in outs], None)
            assert st == 0, eng.lib.e2v_last_error(eng.ctx)
        run_fenced(call, outs[:-1], outs[-1])
        taken = eng.pool_gets() - gets
        checked, violations, text = eng.pool_guard_report()
        assert violations == 0, text
        assert taken > 0 and checked >= taken, (checked, taken)
        for o, want in zip(outs, base):
            assert not torch.isnan(o.view).any()
            assert torch.equal(bits(o.view.cpu()), bits(want)), name
