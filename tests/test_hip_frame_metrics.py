"""GPU: per-frame SSIM and MSE on the device (``e2v_frame_metrics``, ``Engine.frame_metrics``, ``eeg2video_amd.metrics``,
``examples/run_sweep.py --score-against``) against the float64 restatement of skimage's algorithm
(tests/frame_metrics_restatement.py, pinned by closed forms in tests/test_frame_metrics_host.py).

Bounds: SSIM 1e-6 absolute -- the one tests/test_frame_metrics_host.py derives for the documented fp32 arithmetic -- and MSE 1e-6
relative (one fp32 rounding of an exact quotient is 6e-8).  The kernel scores tiles of 256 window columns x 32 window rows
(kernels.h: FrameMetricsTile), so the shape list holds one image whose (H - 6, W - 6) = (70, 293) spans three strips and two
column tiles and is a multiple of neither."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from eeg2video_amd import _lib
from eeg2video_amd.weights import TINY_UNET, TINY_VAE
from frame_metrics_restatement import C1, KINDS, clip_scores, image_pair, mse_exact, quantise, ssim

pytestmark = pytest.mark.gpu

TILE_COLS, TILE_ROWS = 256, 32
SHAPES = [(1, 1, 1, 7, 7), (2, 3, 3, 9, 11), (1, 2, 3, 32, 48), (1, 1, 3, 288, 512), (1, 1, 2, 2 * TILE_ROWS + 6 + 6, TILE_COLS + 37 + 6)]
U8, CL = _lib.E2V_FRAMES_U8, _lib.E2V_FRAMES_CHANNELS_LAST


@pytest.fixture(scope="module")
def eng():
    from eeg2video_amd.engine import Engine
    return Engine(TINY_UNET, TINY_VAE, 0)


@functools.lru_cache(maxsize=None)
def clips(kind, shape):
    """two planar uint8 batches ``[n,C,F,H,W]`` of `kind` and the restatement's per-image (ssim, exact mse) ``[n,F]``"""
    n, F, Cc, H, W = shape
    a, b = np.empty((n, Cc, F, H, W), np.uint8), np.empty((n, Cc, F, H, W), np.uint8)
    s, m = np.empty((n, F)), np.empty((n, F), np.float32)
    for i in range(n):
        for f in range(F):
            x, y = image_pair(kind, H, W, Cc, seed=i * F + f)
            a[i, :, f], b[i, :, f] = x.transpose(2, 0, 1), y.transpose(2, 0, 1)
            s[i, f], m[i, f] = ssim(x, y), mse_exact(x, y)
    for v in (a, b, s, m):
        v.setflags(write=False)
    return a, b, s, m


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def run(eng, a, b, **kw):
    s, m = eng.frame_metrics(a, b, **kw)
    torch.cuda.synchronize()
    return s.cpu().numpy(), m.cpu().numpy()


def check(got, want_ssim, want_mse, what=""):
    s, m = got
    assert s.dtype == np.float32 and m.dtype == np.float32 and s.shape == want_ssim.shape == m.shape
    err = np.abs(s.astype(np.float64) - want_ssim).max()
    print(f"{what}: max |ssim - restatement| = {err:.3e}")
    assert err <= 1e-6, what
    assert np.all(np.abs(m.astype(np.float64) - want_mse.astype(np.float64)) <= 1e-6 * want_mse.astype(np.float64)), what


# ---- parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_restatement(eng, kind, shape):
    a, b, s, m = clips(kind, shape)
    got = run(eng, dev(a), dev(b))
    check(got, s, m, f"{kind} {shape}")
    assert np.array_equal(got[1], m)                                   # the MSE is the exact integer sum, divided and rounded once
    if kind == "identical":
        assert np.all(got[0] == np.float32(1.0)) and np.all(got[1] == 0.0)
    if kind == "constant":
        want = (2 * 254 * 255 + C1) / (254 ** 2 + 255 ** 2 + C1)
        assert np.abs(got[0].astype(np.float64) - want).max() <= 1e-6 and np.all(got[1] == np.float32(1.0 / 65025))
    back = run(eng, dev(b), dev(a))                                     # symmetric, bit for bit
    assert np.array_equal(back[0], got[0]) and np.array_equal(back[1], got[1])


# ---- every pixel belongs to exactly one tile -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 3, 9, 11), (1, 1, 2, 2 * TILE_ROWS + 12, TILE_COLS + 43)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("where", ["last_rows", "last_cols", "corners"])
def test_mse_counts_the_border_once(eng, where, shape):
    n, F, Cc, H, W = shape
    a = np.array(clips("noise", shape)[0])
    b = a.copy()
    if where == "last_rows":
        b[..., H - 3:, :] ^= 0x55
    elif where == "last_cols":
        b[..., :, W - 3:] ^= 0x0F
    else:
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            b[..., y, x] = 255 - b[..., y, x]
    d = a.astype(np.int64) - b.astype(np.int64)
    want_mse = np.float32(np.float64(int((d * d).sum())) / np.float64(65025 * Cc * H * W))
    want_ssim = ssim(a[0, :, 0].transpose(1, 2, 0), b[0, :, 0].transpose(1, 2, 0))
    s, m = run(eng, dev(a), dev(b))
    assert m[0, 0] == want_mse and want_mse > 0
    assert abs(float(s[0, 0]) - want_ssim) <= 1e-6


# ---- input kinds ---------------------------------------------------------------------------------------------------------------------
def as_kind(u8_planar, f32, channels_last):
    t = dev(u8_planar)
    if f32:
        t = (t.float() + 0.5) / 255.0
    return t.permute(0, 2, 3, 4, 1).contiguous() if channels_last else t


@pytest.mark.parametrize("shape", [(2, 3, 3, 9, 11), (1, 2, 4, 40, 300)], ids=lambda s: "x".join(map(str, s)))
def test_type_and_layout_of_each_input_are_independent(eng, shape):
    a, b, s, m = clips("gradient", shape)
    base = run(eng, dev(a), dev(b))
    check(base, s, m, f"u8 planar {shape}")
    for af in (0, 1):
        for acl in (0, 1):
            for bf in (0, 1):
                for bcl in (0, 1):
                    got = run(eng, as_kind(a, af, acl), as_kind(b, bf, bcl), a_channels_last=bool(acl), b_channels_last=bool(bcl))
                    assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), (af, acl, bf, bcl)


def test_floats_score_as_their_frames_to_uint8_bytes(eng):
    g = torch.Generator().manual_seed(3)
    x, y = torch.rand((2, 3, 2, 17, 23), generator=g).cuda(), torch.rand((2, 3, 2, 17, 23), generator=g).cuda()
    xb, yb = eng.frames_to_uint8(x), eng.frames_to_uint8(y)
    assert np.array_equal(xb.cpu().numpy(), quantise(x.cpu().numpy()))
    got, want = run(eng, x, y), run(eng, xb, yb)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    mixed = run(eng, x, yb)
    assert np.array_equal(mixed[0], want[0]) and np.array_equal(mixed[1], want[1])


def test_out_of_range_floats_and_nan_are_clamped(eng):
    x = torch.rand((1, 1, 1, 8, 9), generator=torch.Generator().manual_seed(4))
    y = x.clone()
    x[0, 0, 0, 0, 0], x[0, 0, 0, 3, 4], x[0, 0, 0, 7, 8] = -0.5, 1.5, float("nan")
    y[0, 0, 0, 0, 0], y[0, 0, 0, 3, 4], y[0, 0, 0, 7, 8] = 0.0, 1.0, 0.0
    xq = torch.from_numpy(quantise(x.numpy()))
    assert (xq[0, 0, 0, 0, 0], xq[0, 0, 0, 3, 4], xq[0, 0, 0, 7, 8]) == (0, 255, 0)
    other = torch.rand((1, 1, 1, 8, 9), generator=torch.Generator().manual_seed(5))
    got, want, byt = run(eng, x, other), run(eng, y, other), run(eng, xq, other)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], byt[0]) and np.array_equal(got[1], byt[1])
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()


# ---- alignment -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [(1, 3), (3, 1)])
def test_uint8_inputs_at_odd_byte_offsets(eng, offsets):
    """slices of a larger buffer at byte offsets 1 and 3, channels-last with W * C = 13 * 3 = 39 bytes per row"""
    shape = (2, 2, 3, 9, 13)
    a, b, s, m = clips("noise", shape)
    n, F, Cc, H, W = shape
    outs = []
    for src, off in ((a, offsets[0]), (b, offsets[1])):
        cl = np.ascontiguousarray(src.transpose(0, 2, 3, 4, 1))
        buf = torch.full((cl.size + 8,), 0xEE, dtype=torch.uint8, device="cuda")
        buf[off:off + cl.size] = dev(cl).flatten()
        outs.append(buf)
    ss = torch.empty((n, F), device="cuda", dtype=torch.float32)
    mm = torch.empty((n, F), device="cuda", dtype=torch.float32)
    st = eng.lib.e2v_frame_metrics(eng.ctx, outs[0].data_ptr() + offsets[0], U8 | CL, outs[1].data_ptr() + offsets[1], U8 | CL, n, F, Cc, H,
                                   W, ss.data_ptr(), mm.data_ptr(), None)
    torch.cuda.synchronize()
    assert st == _lib.E2V_OK, eng.lib.e2v_last_error(eng.ctx)
    check((ss.cpu().numpy(), mm.cpu().numpy()), s, m, f"offsets {offsets}")
    assert np.array_equal(mm.cpu().numpy(), m)


# ---- batch independence, determinism ---------------------------------------------------------------------------------------------------
def test_an_image_scores_the_same_alone_and_in_a_batch(eng):
    shape = (5, 2, 3, 45, 270)
    a, b, s, m = clips("gradient", shape)
    full = run(eng, dev(a), dev(b))
    again = run(eng, dev(a), dev(b))
    assert np.array_equal(full[0], again[0]) and np.array_equal(full[1], again[1])
    check(full, s, m, "n = 5")
    for i in range(5):
        one = run(eng, dev(a[i:i + 1]), dev(b[i:i + 1]))
        assert np.array_equal(one[0][0], full[0][i]) and np.array_equal(one[1][0], full[1][i]), i


# ---- outputs -----------------------------------------------------------------------------------------------------------------------
def test_outputs_stay_inside_their_slots_and_either_may_be_null(eng):
    shape = (2, 3, 3, 9, 11)
    a, b, s, m = clips("noise", shape)
    n, F, Cc, H, W = shape
    da, db = dev(a), dev(b)
    cnt, pad = n * F, 16
    for want_ssim, want_mse in ((True, True), (True, False), (False, True)):
        buf = torch.full((2 * cnt + 3 * pad,), -7.0, device="cuda")
        ps = buf.data_ptr() + 4 * pad if want_ssim else None
        pm = buf.data_ptr() + 4 * (2 * pad + cnt) if want_mse else None
        before = eng.device_bytes()
        st = eng.lib.e2v_frame_metrics(eng.ctx, da.data_ptr(), U8, db.data_ptr(), U8, n, F, Cc, H, W, ps, pm, None)
        torch.cuda.synchronize()
        assert st == _lib.E2V_OK, eng.lib.e2v_last_error(eng.ctx)
        if (want_ssim, want_mse) != (True, True):
            assert eng.device_bytes() == before                        # the partials block of this shape is cached by now
        h = buf.cpu().numpy()
        gs, gm = h[pad:pad + cnt].reshape(n, F), h[2 * pad + cnt:2 * pad + 2 * cnt].reshape(n, F)
        assert np.all(h[:pad] == -7.0) and np.all(h[pad + cnt:2 * pad + cnt] == -7.0) and np.all(h[2 * pad + 2 * cnt:] == -7.0)
        if want_ssim:
            assert np.abs(gs.astype(np.float64) - s).max() <= 1e-6
        else:
            assert np.all(gs == -7.0)
        if want_mse:
            assert np.array_equal(gm, m)
        else:
            assert np.all(gm == -7.0)
    assert eng.lib.e2v_frame_metrics(eng.ctx, da.data_ptr(), U8, db.data_ptr(), U8, n, F, Cc, H, W, None, None, None) == _lib.E2V_EINVAL


def test_engine_checks_shapes_after_the_layout(eng):
    a = torch.zeros((2, 3, 2, 9, 11), dtype=torch.uint8)
    s, m = eng.frame_metrics(a, a.permute(0, 2, 3, 4, 1), b_channels_last=True)          # a non-contiguous view, from the host
    assert tuple(s.shape) == (2, 2) and tuple(m.shape) == (2, 2) and s.is_cuda
    s1, _ = eng.frame_metrics(a[0], a[0])                                                  # 4-D: one clip
    assert tuple(s1.shape) == (1, 2)
    with pytest.raises(ValueError, match="clips differ"):
        eng.frame_metrics(a, a.permute(0, 2, 3, 4, 1))
    with pytest.raises(ValueError, match="uint8 or float32"):
        eng.frame_metrics(a.double(), a)
    with pytest.raises(ValueError, match="window exceeds"):
        eng.frame_metrics(a[..., :6], a[..., :6])


# ---- the reference's names ---------------------------------------------------------------------------------------------------------
def test_mirror_of_the_scoring_script(eng):
    from eeg2video_amd import metrics
    a, b, _, _ = clips("gradient", (1, 4, 3, 12, 20))
    pred, gt = a[0].transpose(1, 2, 3, 0), b[0].transpose(1, 2, 3, 0)                     # [f,h,w,3]
    want_s, want_m = clip_scores(pred, gt)
    for p, g in ((pred, gt), (pred.transpose(0, 3, 1, 2), gt.transpose(0, 3, 1, 2))):     # and [f,c,h,w]
        mean, std = metrics.ssim_score_only(p, g, engine=eng)
        assert abs(mean - want_s.mean()) <= 1e-6 and abs(std - want_s.std()) <= 1e-6
        mean, std = metrics.mse_score_only(p, g, engine=eng)
        assert abs(mean - want_m.mean()) <= 1e-6 * want_m.mean() and abs(std - want_m.std()) <= 1e-6 * want_m.mean()
    assert abs(metrics.ssim_metric(pred[1], gt[1], engine=eng) - want_s[1]) <= 1e-6
    assert abs(metrics.mse_metric(pred[1], gt[1], engine=eng) - want_m[1]) <= 1e-6 * want_m[1]
    assert metrics.channel_last(pred) is pred and metrics.channel_last(pred.transpose(0, 3, 1, 2)).shape == pred.shape


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------
def test_sweep_scores_against_a_directory_of_clips(tmp_path, capsys):
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "run_sweep.py")
    spec = importlib.util.spec_from_file_location("e2v_sweep_scored", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    common = ["--tiny", "--concepts", "2", "--per-concept", "2", "--batch", "3", "--steps", "2"]
    d16, d32 = str(tmp_path / "bf16"), str(tmp_path / "fp32")
    lo = mod.main(common + ["--dtype", "bf16", "--out", d16, "--npy"])
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "ssim_mean" not in plain and "score" not in plain["stage_seconds_rank0"]
    hi = mod.main(common + ["--out", d32, "--npy", "--score-against", d16])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    cl = lambda u8: u8.permute(0, 2, 3, 4, 1).numpy()                                     # [n,F,H,W,3]
    scores = [clip_scores(x, y) for x, y in zip(cl(hi), cl(lo))]
    s, m = np.stack([p[0] for p in scores]), np.stack([p[1] for p in scores])
    assert abs(rec["ssim_mean"] - s.mean()) <= 1e-6 and abs(rec["ssim_std"] - s.std()) <= 1e-6
    assert abs(rec["mse_mean"] - m.mean()) <= 1e-6 * m.mean() and rec["mse_mean"] > 0
    assert rec["stage_seconds_rank0"]["score"] > 0 and set(rec) - set(plain) == {"ssim_mean", "ssim_std", "mse_mean"}
    mod.main(common + ["--score-against", d32])
    same = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert same["ssim_mean"] == 1 and same["ssim_std"] == 0 and same["mse_mean"] == 0
