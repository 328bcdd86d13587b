"""GPU: every hand-written kernel, called through the C ABI, against a plain PyTorch fp32 reference of the
same op on the CPU (floating-point kernels: tolerance stated per test; fp32 MFMA is an exact-product fmaf
chain, so differences are summation order only)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2e-5      # fp32 vs fp32, different summation order


@pytest.fixture(scope="module")
def eng():
    from eeg2video_amd.engine import Engine
    from eeg2video_amd.weights import TINY_UNET, TINY_VAE
    return Engine(TINY_UNET, TINY_VAE, 0)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def to_cl(x):      # [n, C, H, W] -> [n*H*W, C]
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


def from_cl(y, n, h, w):
    return y.reshape(n, h, w, -1).permute(0, 3, 1, 2).contiguous()


def close(a, b, rtol=RTOL, atol=ATOL):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = b.abs().max().item() + 1e-30
    err = (a - b).abs().max().item()
    assert err <= atol * max(1.0, scale) + rtol * scale, f"max abs err {err:.3e} (ref scale {scale:.3e})"


# ------------------------------------------------------------------ conv / linear -------------------
@pytest.mark.parametrize("cin,cout,n,h,w", [(32, 64, 2, 5, 8), (4, 64, 3, 9, 12), (64, 4, 2, 7, 5), (96, 320, 1, 18, 32),
                                            (320, 320, 2, 36, 64)])
def test_conv3x3_plain(eng, cin, cout, n, h, w):
    x, wt, b = rnd(n, cin, h, w, seed=1), rnd(cout, cin, 3, 3, seed=2, scale=0.1), rnd(cout, seed=3)
    ref = F.conv2d(x, wt, b, padding=1)
    y = eng.op_conv3x3(to_cl(x).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=h, Ws=w)
    close(from_cl(y, n, h, w), ref)


def test_conv3x3_stride2_both_paddings(eng):
    n, c, h, w = 2, 32, 9, 12
    x, wt, b = rnd(n, c, h, w, seed=4), rnd(64, c, 3, 3, seed=5, scale=0.1), rnd(64, seed=6)
    ref = F.conv2d(x, wt, b, stride=2, padding=1)                               # Downsample3D (resnet.py:87)
    y = eng.op_conv3x3(to_cl(x).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=h, Ws=w, stride=2)
    close(from_cl(y, n, ref.shape[2], ref.shape[3]), ref)
    x2 = rnd(n, c, 8, 12, seed=7)                                               # VAE encoder: F.pad (0,1,0,1), no padding
    ref2 = F.conv2d(F.pad(x2, (0, 1, 0, 1)), wt, b, stride=2)
    y2 = eng.op_conv3x3(to_cl(x2).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=8, Ws=12, stride=2, pad_lo=0, pad_hi=1)
    close(from_cl(y2, n, ref2.shape[2], ref2.shape[3]), ref2)


@pytest.mark.parametrize("hs,ws,hi,wi", [(5, 8, 9, 16), (5, 8, 10, 16), (3, 3, 5, 6), (2, 2, 3, 3), (5, 6, 12, 7)])
def test_conv3x3_fused_nearest_resize(eng, hs, ws, hi, wi):
    """Upsample3D: F.interpolate(size=...) nearest, then conv (resnet.py:58-69); 5 -> 9 is the L3->L2 case."""
    n, c = 3, 32
    x, wt, b = rnd(n, c, hs, ws, seed=8), rnd(64, c, 3, 3, seed=9, scale=0.1), rnd(64, seed=10)
    ref = F.conv2d(F.interpolate(x, size=(hi, wi), mode="nearest"), wt, b, padding=1)
    y = eng.op_conv3x3(to_cl(x).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=hs, Ws=ws, Hi=hi, Wi=wi)
    close(from_cl(y, n, hi, wi), ref)


def test_conv3x3_concat_rowbias_residual(eng):
    """torch.cat([h, skip], 1) read in place + time-embedding row bias + residual epilogue."""
    n_s, f, c0, c1, cout, h, w = 2, 3, 64, 32, 64, 5, 6
    n = n_s * f
    a, s = rnd(n, c0, h, w, seed=11), rnd(n, c1, h, w, seed=12)
    wt, b = rnd(cout, c0 + c1, 3, 3, seed=13, scale=0.1), rnd(cout, seed=14)
    temb, res = rnd(n_s, cout, seed=15), rnd(n, cout, h, w, seed=16)
    ref = F.conv2d(torch.cat([a, s], 1), wt, b, padding=1) + temb.repeat_interleave(f, 0)[:, :, None, None] + res
    y = eng.op_conv3x3(to_cl(a).cuda(), wt.cuda(), b.cuda(), x1=to_cl(s).cuda(), n_img=n, Hs=h, Ws=w,
                       rowbias=temb.cuda().contiguous(), rows_per_sample=f * h * w, resid=to_cl(res).cuda())
    close(from_cl(y, n, h, w), ref)


@pytest.fixture
def wino(eng):
    """Force the Winograd F(2x2,3x3) form for every stride-1 3x3 conv of the test, then restore the default."""
    eng.set_conv_algo("winograd")
    yield eng
    eng.set_conv_algo("auto")


@pytest.mark.parametrize("cin,cout,n,h,w", [(32, 64, 2, 5, 8), (4, 64, 3, 9, 12), (64, 4, 2, 7, 5), (256, 256, 2, 18, 32),
                                            (1280, 640, 1, 9, 16), (64, 32, 2, 1, 1), (32, 32, 1, 2, 3)])
def test_conv3x3_winograd(wino, cin, cout, n, h, w):
    """Winograd F(2x2,3x3) (wino.hip): same fp32 result as F.conv2d to the tolerance of the direct kernel; odd maps
    exercise the ragged last tile row / column."""
    x, wt, b = rnd(n, cin, h, w, seed=1), rnd(cout, cin, 3, 3, seed=2, scale=0.1), rnd(cout, seed=3)
    ref = F.conv2d(x, wt, b, padding=1)
    y = wino.op_conv3x3(to_cl(x).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=h, Ws=w)
    close(from_cl(y, n, h, w), ref)


@pytest.mark.parametrize("hs,ws,hi,wi", [(5, 8, 9, 16), (5, 8, 10, 16), (3, 3, 5, 6), (2, 2, 3, 3), (5, 6, 12, 7)])
def test_conv3x3_winograd_fused_nearest_resize(wino, hs, ws, hi, wi):
    n, c = 3, 32
    x, wt, b = rnd(n, c, hs, ws, seed=8), rnd(64, c, 3, 3, seed=9, scale=0.1), rnd(64, seed=10)
    ref = F.conv2d(F.interpolate(x, size=(hi, wi), mode="nearest"), wt, b, padding=1)
    y = wino.op_conv3x3(to_cl(x).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=hs, Ws=ws, Hi=hi, Wi=wi)
    close(from_cl(y, n, hi, wi), ref)


def test_conv3x3_winograd_concat_rowbias_residual_and_chunking(wino, monkeypatch):
    n_s, f, c0, c1, cout, h, w = 2, 3, 64, 32, 64, 5, 6
    n = n_s * f
    a, s = rnd(n, c0, h, w, seed=11), rnd(n, c1, h, w, seed=12)
    wt, b = rnd(cout, c0 + c1, 3, 3, seed=13, scale=0.1), rnd(cout, seed=14)
    temb, res = rnd(n_s, cout, seed=15), rnd(n, cout, h, w, seed=16)
    ref = F.conv2d(torch.cat([a, s], 1), wt, b, padding=1) + temb.repeat_interleave(f, 0)[:, :, None, None] + res
    y = wino.op_conv3x3(to_cl(a).cuda(), wt.cuda(), b.cuda(), x1=to_cl(s).cuda(), n_img=n, Hs=h, Ws=w,
                        rowbias=temb.cuda().contiguous(), rows_per_sample=f * h * w, resid=to_cl(res).cuda())
    close(from_cl(y, n, h, w), ref)


@pytest.mark.parametrize("cin,cout,n,h,w", [(32, 64, 2, 5, 8), (64, 4, 2, 7, 5), (256, 256, 2, 18, 32), (640, 320, 1, 36, 64),
                                            (64, 32, 2, 1, 1), (32, 32, 1, 4, 4)])
def test_conv3x3_winograd_f4(eng, cin, cout, n, h, w):
    """Opt-in F(4x4,3x3): transform constants up to 8 cost ~17x the direct sum's rounding error -- 1e-4 of the output
    scale here (measured 5e-6 on a 640-channel conv), which is why it is not the default."""
    eng.set_conv_algo("winograd4")
    try:
        x, wt, b = rnd(n, cin, h, w, seed=1), rnd(cout, cin, 3, 3, seed=2, scale=0.1), rnd(cout, seed=3)
        res = rnd(n, cout, h, w, seed=4)
        ref = F.conv2d(x, wt, b, padding=1) + res
        y = eng.op_conv3x3(to_cl(x).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=h, Ws=w, resid=to_cl(res).cuda())
        close(from_cl(y, n, h, w), ref, rtol=1e-4, atol=1e-4)
    finally:
        eng.set_conv_algo("auto")


def test_conv3x3_stride2_ignores_winograd(wino):
    """stride 2 has no F(2x2,3x3) form: the forced setting falls back to the direct kernel."""
    n, c, h, w = 2, 32, 9, 12
    x, wt, b = rnd(n, c, h, w, seed=4), rnd(64, c, 3, 3, seed=5, scale=0.1), rnd(64, seed=6)
    ref = F.conv2d(x, wt, b, stride=2, padding=1)
    y = wino.op_conv3x3(to_cl(x).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=h, Ws=w, stride=2)
    close(from_cl(y, n, ref.shape[2], ref.shape[3]), ref)


@pytest.mark.parametrize("m,k,n", [(240, 1280, 1280), (77, 64, 128), (1000, 320, 960), (130, 40, 72), (5, 320, 1280)])
def test_linear(eng, m, k, n):
    x, w, b, r = rnd(m, k, seed=20), rnd(n, k, seed=21, scale=0.05), rnd(n, seed=22), rnd(m, n, seed=23)
    close(eng.op_linear(x.cuda(), w.cuda(), b.cuda(), r.cuda()), F.linear(x, w, b) + r)
    close(eng.op_linear(x.cuda(), w.cuda()), F.linear(x, w))


@pytest.mark.parametrize("m,c", [(300, 64), (864, 320)])
def test_linear_geglu(eng, m, c):
    """FeedForward GEGLU (dep): h, gate = proj(x).chunk(2); h * gelu_erf(gate)."""
    x, w, b = rnd(m, c, seed=24), rnd(8 * c, c, seed=25, scale=0.1), rnd(8 * c, seed=26)
    h, g = F.linear(x, w, b).chunk(2, dim=-1)
    close(eng.op_linear(x.cuda(), w.cuda(), b.cuda(), geglu=True), h * F.gelu(g))


# ------------------------------------------------------------------ norms ---------------------------
@pytest.mark.parametrize("c,groups,n,f,hw", [(320, 32, 2, 6, 40), (64, 32, 3, 3, 300), (960, 32, 1, 6, 100), (128, 8, 2, 1, 600)])
@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_5d(eng, c, groups, n, f, hw, silu):
    """5-D GroupNorm: statistics over (C/G) x F x H x W jointly (resnet.py:177)."""
    x = rnd(n, c, f, hw, 1, seed=30) * 2.0 + 0.7
    ga, be = rnd(c, seed=31) * 0.2 + 1.0, rnd(c, seed=32) * 0.2
    ref = F.group_norm(x, groups, ga, be, 1e-5)
    ref = F.silu(ref) if silu else ref
    xcl = x.permute(0, 2, 3, 4, 1).reshape(n * f * hw, c).contiguous()
    y = eng.op_groupnorm(xcl.cuda(), ga.cuda(), be.cuda(), samples=n, P=f * hw, groups=groups, eps=1e-5, silu=silu)
    close(y.reshape(n, f, hw, 1, c).permute(0, 4, 1, 2, 3), ref)


def test_groupnorm_concat_group_straddles_seam(eng):
    """up-block concat 1280 + 640 -> 1920 channels, 60 per group: group 21 straddles the seam."""
    n, c0, c1, p = 2, 64, 32, 500            # 96 / 32 = 3 channels per group; 64 / 3 is not an integer
    a, s = rnd(n, c0, p, 1, seed=33), rnd(n, c1, p, 1, seed=34) * 3 - 1
    ga, be = rnd(c0 + c1, seed=35) * 0.2 + 1.0, rnd(c0 + c1, seed=36) * 0.2
    ref = F.silu(F.group_norm(torch.cat([a, s], 1), 32, ga, be, 1e-5))
    cl = lambda t: t.permute(0, 2, 3, 1).reshape(n * p, -1).contiguous()
    y = eng.op_groupnorm(cl(a).cuda(), ga.cuda(), be.cuda(), samples=n, P=p, groups=32, eps=1e-5, silu=True, x1=cl(s).cuda())
    close(y.reshape(n, p, 1, c0 + c1).permute(0, 3, 1, 2), ref)


@pytest.mark.parametrize("c", [64, 320, 640, 1280, 768, 1032])       # (768 / 1032: the wave-per-row kernel at 3 / 5 quads per lane)
def test_layernorm(eng, c):
    x, g, b = rnd(777, c, seed=40) * 3 + 1, rnd(c, seed=41) * 0.2 + 1, rnd(c, seed=42) * 0.2
    close(eng.op_layernorm(x.cuda(), g.cuda(), b.cuda()), F.layer_norm(x, (c,), g, b, 1e-5))
    try:                                                     # the wave-per-row kernel (C = 320 / 640 / 1280 take the shared-wave rows by default)
        eng.set_knob("E2V_LN_ROWS", 0)
        close(eng.op_layernorm(x.cuda(), g.cuda(), b.cuda()), F.layer_norm(x, (c,), g, b, 1e-5))
    finally:
        eng.set_knob("E2V_LN_ROWS", 1)
    for rows in (1, 3, 9):                                   # ragged row groups
        close(eng.op_layernorm(x[:rows].cuda().contiguous(), g.cuda(), b.cuda()), F.layer_norm(x[:rows], (c,), g, b, 1e-5))


# ------------------------------------------------------------------ attention -----------------------
def _ref_attn(q, k, v, scale):
    s = torch.baddbmm(torch.empty(q.shape[0], q.shape[1], k.shape[1]), q, k.transpose(1, 2), beta=0, alpha=scale)
    return torch.bmm(s.softmax(-1), v)


def _heads(x, h):     # [b, s, h*d] -> [b*h, s, d]
    b, s, c = x.shape
    return x.reshape(b, s, h, c // h).permute(0, 2, 1, 3).reshape(b * h, s, c // h)


def _unheads(x, h):
    bh, s, d = x.shape
    return x.reshape(bh // h, h, s, d).permute(0, 2, 1, 3).reshape(bh // h, s, h * d)


@pytest.mark.parametrize("d,nq,f,n", [(8, 108, 3, 2), (16, 30, 4, 1), (32, 9, 3, 2), (40, 200, 6, 1), (80, 144, 3, 1),
                                      (160, 40, 6, 2), (64, 70, 2, 1)])
def test_sparse_causal_attention(eng, d, nq, f, n):
    """attention.py:292-321: keys/values of frame i = [frame 0 ; frame max(i-1,0)], heads folded into batch."""
    heads = 8 if d != 160 else 4
    c = heads * d
    qkv = rnd(n * f * nq, 3 * c, seed=50)
    q, k, v = (qkv[:, i * c:(i + 1) * c].reshape(n * f, nq, c) for i in range(3))
    former = torch.arange(f) - 1
    former[0] = 0
    gather = lambda t: torch.cat([t.reshape(n, f, nq, c)[:, [0] * f], t.reshape(n, f, nq, c)[:, former]], dim=2).reshape(n * f, 2 * nq, c)
    ref = _unheads(_ref_attn(_heads(q, heads), _heads(gather(k), heads), _heads(gather(v), heads), d ** -0.5), heads)
    g = qkv.cuda()
    y = eng.op_attention(g[:, :c], g[:, c:2 * c], g[:, 2 * c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nq, mode=0, scale=d ** -0.5)
    close(y.reshape(n * f, nq, c), ref, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("d,nq,nk", [(8, 108, 11), (40, 300, 77), (80, 144, 77), (160, 40, 77)])
def test_cross_attention(eng, d, nq, nk):
    heads, n, f = 8, 2, 3
    c = heads * d
    q, kv = rnd(n * f * nq, c, seed=51), rnd(n * nk, 2 * c, seed=52)
    k, v = kv[:, :c].reshape(n, nk, c), kv[:, c:].reshape(n, nk, c)
    rep = lambda t: t.repeat_interleave(f, 0)
    ref = _unheads(_ref_attn(_heads(q.reshape(n * f, nq, c), heads), _heads(rep(k), heads), _heads(rep(v), heads), d ** -0.5), heads)
    gq, gkv = q.cuda(), kv.cuda()
    y = eng.op_attention(gq, gkv[:, :c], gkv[:, c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nk, mode=1, scale=d ** -0.5)
    close(y.reshape(n * f, nq, c), ref, rtol=1e-4, atol=1e-5)


def test_attention_online_softmax_rescale_branch(eng):
    """Force the running max to jump at a late key tile (one key spiked against every query)."""
    heads, d, n, f, nq = 8, 40, 1, 3, 100
    c = heads * d
    qkv = rnd(n * f * nq, 3 * c, seed=53)
    qkv[2 * nq + 90, c:2 * c] *= 25.0          # a key of frame 2, in the 3rd tile of the 2nd segment for f = 3... and of frame>=?
    qkv[70, c:2 * c] *= 25.0                   # a key of frame 0 (seen by every frame), 3rd tile
    q, k, v = (qkv[:, i * c:(i + 1) * c].reshape(n * f, nq, c) for i in range(3))
    former = torch.arange(f) - 1
    former[0] = 0
    gather = lambda t: torch.cat([t.reshape(n, f, nq, c)[:, [0] * f], t.reshape(n, f, nq, c)[:, former]], dim=2).reshape(n * f, 2 * nq, c)
    ref = _unheads(_ref_attn(_heads(q, heads), _heads(gather(k), heads), _heads(gather(v), heads), d ** -0.5), heads)
    g = qkv.cuda()
    y = eng.op_attention(g[:, :c], g[:, c:2 * c], g[:, 2 * c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nq, mode=0, scale=d ** -0.5)
    close(y.reshape(n * f, nq, c), ref, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("d,f,hw", [(8, 3, 50), (40, 6, 33), (160, 6, 7)])
def test_temporal_attention(eng, d, f, hw):
    """attention.py:261-267: '(b f) d c -> (b d) f c', attention over frames, and back."""
    heads, n = 8, 2
    c = heads * d
    qkv = rnd(n * f * hw, 3 * c, seed=54)
    t = qkv.reshape(n, f, hw, 3 * c).permute(0, 2, 1, 3).reshape(n * hw, f, 3 * c)
    q, k, v = t[..., :c], t[..., c:2 * c], t[..., 2 * c:]
    ref = _unheads(_ref_attn(_heads(q, heads), _heads(k, heads), _heads(v, heads), d ** -0.5), heads)
    ref = ref.reshape(n, hw, f, c).permute(0, 2, 1, 3).reshape(n * f * hw, c)
    y = eng.op_temporal_attention(qkv.cuda(), n=n, F=f, HW=hw, heads=heads, D=d, scale=d ** -0.5)
    close(y, ref, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("d,f,hw", [(40, 6, 50), (80, 6, 33), (160, 6, 7)])
def test_temporal_attention_wave_kernel_vs_staged_kernel(eng, mode, d, f, hw):
    """attn_temp (attention.py:261-267) has two kernels: temporal_attn_wave_kernel (registers only, the default) and the LDS-staged
    one behind E2V_TATTN_WAVE = 0.  Same-process A/B through the knob table: both against the reference, and against each other to
    summation order (fp32) / one output rounding (bf16)."""
    heads, n = 8, 2
    c = heads * d
    qkv = rnd(n * f * hw, 3 * c, seed=254)
    src = qkv.to(H16_TYPES[mode]).float() if mode != "fp32" else qkv
    t = src.reshape(n, f, hw, 3 * c).permute(0, 2, 1, 3).reshape(n * hw, f, 3 * c)
    q, k, v = t[..., :c], t[..., c:2 * c], t[..., 2 * c:]
    ref = _unheads(_ref_attn(_heads(q, heads), _heads(k, heads), _heads(v, heads), d ** -0.5), heads)
    ref = ref.reshape(n, hw, f, c).permute(0, 2, 1, 3).reshape(n * f * hw, c)
    try:
        eng.set_compute_dtype(mode)
        g = qkv.cuda()
        run = lambda: eng.op_temporal_attention(g, n=n, F=f, HW=hw, heads=heads, D=d, scale=d ** -0.5)
        wave = run()
        eng.set_knob("E2V_TATTN_WAVE", 0)
        staged = run()
    finally:
        eng.set_knob("E2V_TATTN_WAVE", 1)
        eng.set_compute_dtype("fp32")
    tol = {"bf16": 8e-3, "fp16": 1e-3, "fp32": 1e-4}[mode]
    close(wave, ref, rtol=tol, atol=tol)
    close(staged, ref, rtol=tol, atol=tol)
    close(wave, staged, rtol=tol, atol=tol)


# ------------------------------------------------------------------ bf16-activation mode (BASELINE configs[2]) -------
# e2v_set_compute_dtype(E2V_BF16): the op entry points round their fp32 operands to bf16 once and run the kernels the graph
# runs in that mode (bgemm.hip LDS-DMA tiles, flash_attn_b16io, the bf16-I/O norm kernels).  GEMM-shaped ops return fp32, so
# they are compared TIGHTLY with the same op on bf16-rounded operands in fp32 (summation order only), and loosely with
# the fp32 op (bf16 has 8 mantissa bits).
# The same tests run in BOTH 16-bit modes -- "bf16" (configs[2]) and "fp16" (IEEE half: the reference's own inference dtype,
# inference_eeg2video.py:69-70) -- the kernels are one template over the element type (csrc/h16.h).  H16 holds the type the running
# test was parametrised with; rb() rounds a reference operand the way that mode's kernels do.
H16 = {"name": "bf16", "dtype": torch.bfloat16}
H16_TYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(params=["bf16", "fp16"])
def h16(request):
    """Name of the 16-bit mode of this test instance (for `eng.set_compute_dtype(h16)`); rb() follows it."""
    H16.update(name=request.param, dtype=H16_TYPES[request.param])
    yield request.param
    H16.update(name="bf16", dtype=torch.bfloat16)


@pytest.fixture
def bf(eng, h16):
    eng.set_compute_dtype(h16)
    yield eng
    eng.set_compute_dtype("fp32")


def rb(t):
    return t.to(H16["dtype"]).float()


def tol16(bf16_tol, fp16_tol=None):
    """Tolerance of "one rounding of the output" checks: the bf16 figure, or 1/4 of it in fp16 mode (three more mantissa bits: the errors
    are 1/8, the bound keeps a factor of two of slack)."""
    return bf16_tol if H16["name"] == "bf16" else (fp16_tol if fp16_tol is not None else bf16_tol / 4)


def ab_build(eng):
    """True when the library was built with `make AB=1` (-DE2V_AB): the variants that were measured and not adopted and the other arms of
    same-process A/Bs exist together with their switches.  The shipped build refuses those switch names; the tests below then check
    the shipped arm only."""
    try:
        eng.set_knob("E2V_ATTN_FOLD", 1)
        return True
    except ValueError:
        return False


def gelu_bf16_grade(x):
    """The GEGLU gate as the kernels of the running 16-bit mode evaluate it (igemm_epi.h: gelu_gate16).  bf16 mode:
    x / (1 + exp(-(a x + b x^3))), |error| <= 2.8e-4 against the exact erf form (bounded in tests/test_oracle_anchors.py) -- 1/14 of a
    bf16 rounding; fp16 mode rounds 8x finer and keeps the erf form (A&S 7.1.26, 1.5e-7) like fp32."""
    from h16_budget import gate          # the formula lives with the per-element budgets (tests/h16_budget.py)
    return gate(x, H16["name"])


def test_bf16_conv_and_linear(bf):
    n, c, h, w = 2, 64, 9, 12
    x, wt, b = rnd(n, c, h, w, seed=60), rnd(128, c, 3, 3, seed=61, scale=0.1), rnd(128, seed=62)
    y = from_cl(bf.op_conv3x3(to_cl(x).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=h, Ws=w), n, h, w)
    close(y, F.conv2d(rb(x), rb(wt), b, padding=1), rtol=1e-4, atol=1e-4)
    close(y, F.conv2d(x, wt, b, padding=1), rtol=tol16(2e-2), atol=tol16(2e-2))
    xl, wl, bl, r = rnd(300, 320, seed=63), rnd(960, 320, seed=64, scale=0.05), rnd(960, seed=65), rnd(300, 960, seed=66)
    close(bf.op_linear(xl.cuda(), wl.cuda(), bl.cuda(), r.cuda()), F.linear(rb(xl), rb(wl), bl) + r, rtol=1e-4, atol=1e-4)
    xg, wg, bg = rnd(200, 64, seed=67), rnd(512, 64, seed=68, scale=0.1), rnd(512, seed=69)
    hh, gg = F.linear(rb(xg), rb(wg), bg).chunk(2, dim=-1)
    yg = bf.op_linear(xg.cuda(), wg.cuda(), bg.cuda(), geglu=True)
    close(yg, hh * gelu_bf16_grade(gg), rtol=1e-4, atol=1e-4)           # the kernel's own gate formula: summation order only
    close(yg, hh * F.gelu(gg), rtol=tol16(4e-4, 1e-4), atol=tol16(4e-4, 1e-4))                    # the exact erf form: + |value| x 2.8e-4 of the gate approximation
    # input channels not a multiple of 8 (conv_in: 4 latent channels): zero-padded to the 16-byte granule, still bf16
    x4, w4 = rnd(1, 4, 5, 6, seed=70), rnd(64, 4, 3, 3, seed=71)
    close(from_cl(bf.op_conv3x3(to_cl(x4).cuda(), w4.cuda(), n_img=1, Hs=5, Ws=6), 1, 5, 6), F.conv2d(rb(x4), rb(w4), padding=1),
          rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("cin,cout,n,h,w", [(32, 64, 2, 5, 8), (64, 4, 2, 7, 5), (96, 320, 1, 18, 32), (320, 320, 2, 36, 64),
                                            (640, 136, 1, 9, 16), (128, 3, 1, 16, 24)])
def test_bf16_conv3x3_shapes(bf, cin, cout, n, h, w):
    """ragged row blocks, ragged last channel chunk (cin % 64 != 0), N = 320 (two 128 tiles + one 64), N not a multiple of 8
    (the VAE's 3-channel conv_out: scalar epilogue)."""
    x, wt, b = rnd(n, cin, h, w, seed=1), rnd(cout, cin, 3, 3, seed=2, scale=0.1), rnd(cout, seed=3)
    y = bf.op_conv3x3(to_cl(x).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=h, Ws=w)
    close(from_cl(y, n, h, w), F.conv2d(rb(x), rb(wt), b, padding=1), rtol=1e-4, atol=1e-4)


def test_bf16_conv3x3_geometries(bf):
    """stride 2 with both paddings, the fused nearest resize, the channel concat with row bias and residual -- the gather
    table and the two-source k-loop of the LDS-DMA kernel."""
    n, c, h, w = 2, 32, 9, 12
    x, wt, b = rnd(n, c, h, w, seed=4), rnd(64, c, 3, 3, seed=5, scale=0.1), rnd(64, seed=6)
    ref = F.conv2d(rb(x), rb(wt), b, stride=2, padding=1)
    y = bf.op_conv3x3(to_cl(x).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=h, Ws=w, stride=2)
    close(from_cl(y, n, ref.shape[2], ref.shape[3]), ref, rtol=1e-4, atol=1e-4)
    x2 = rnd(n, c, 8, 12, seed=7)
    ref2 = F.conv2d(F.pad(rb(x2), (0, 1, 0, 1)), rb(wt), b, stride=2)
    y2 = bf.op_conv3x3(to_cl(x2).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=8, Ws=12, stride=2, pad_lo=0, pad_hi=1)
    close(from_cl(y2, n, ref2.shape[2], ref2.shape[3]), ref2, rtol=1e-4, atol=1e-4)
    for hs, ws, hi, wi in [(5, 8, 9, 16), (3, 3, 5, 6), (5, 6, 12, 7)]:
        xu = rnd(3, c, hs, ws, seed=8)
        refu = F.conv2d(F.interpolate(rb(xu), size=(hi, wi), mode="nearest"), rb(wt), b, padding=1)
        yu = bf.op_conv3x3(to_cl(xu).cuda(), wt.cuda(), b.cuda(), n_img=3, Hs=hs, Ws=ws, Hi=hi, Wi=wi)
        close(from_cl(yu, 3, hi, wi), refu, rtol=1e-4, atol=1e-4)
    n_s, f, c0, c1, cout, h, w = 2, 3, 64, 32, 64, 5, 6
    n = n_s * f
    a, s = rnd(n, c0, h, w, seed=11), rnd(n, c1, h, w, seed=12)
    wc, bc = rnd(cout, c0 + c1, 3, 3, seed=13, scale=0.1), rnd(cout, seed=14)
    temb, res = rnd(n_s, cout, seed=15), rnd(n, cout, h, w, seed=16)
    refc = F.conv2d(torch.cat([rb(a), rb(s)], 1), rb(wc), bc, padding=1) + temb.repeat_interleave(f, 0)[:, :, None, None] + res
    yc = bf.op_conv3x3(to_cl(a).cuda(), wc.cuda(), bc.cuda(), x1=to_cl(s).cuda(), n_img=n, Hs=h, Ws=w,
                       rowbias=temb.cuda().contiguous(), rows_per_sample=f * h * w, resid=to_cl(res).cuda())
    close(from_cl(yc, n, h, w), refc, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("m,k,n", [(240, 1280, 1280), (77, 64, 128), (1000, 320, 960), (130, 40, 72), (5, 320, 1280), (257, 768, 136),
                                   (300, 310, 96)])
def test_bf16_linear_shapes(bf, m, k, n):
    """K = 40 / 310 (ragged 64-chunk, K padded to 8), N = 72 / 136 (ragged column tile), M = 5 (one partial row block)."""
    x, w, b, r = rnd(m, k, seed=20), rnd(n, k, seed=21, scale=0.05), rnd(n, seed=22), rnd(m, n, seed=23)
    close(bf.op_linear(x.cuda(), w.cuda(), b.cuda(), r.cuda()), F.linear(rb(x), rb(w), b) + r, rtol=1e-4, atol=1e-4)
    close(bf.op_linear(x.cuda(), w.cuda()), F.linear(rb(x), rb(w)), rtol=1e-4, atol=1e-4)


def test_bf16_norms_and_temporal_attention(bf):
    """bf16 rows in and out, fp32 statistics / softmax: against the fp32 op on bf16-rounded inputs, to one bf16 rounding of
    the output (2^-8 relative)."""
    samples, P, c0, c1, groups = 3, 50, 64, 32, 8
    a, s = rnd(samples * P, c0, seed=30), rnd(samples * P, c1, seed=31)
    g, be = rnd(c0 + c1, seed=32), rnd(c0 + c1, seed=33)
    xin = torch.cat([rb(a), rb(s)], 1).reshape(samples, P, c0 + c1).permute(0, 2, 1)
    ref = F.silu(F.group_norm(xin, groups, g, be, 1e-5)).permute(0, 2, 1).reshape(samples * P, c0 + c1)
    y = bf.op_groupnorm(a.cuda(), g.cuda(), be.cuda(), samples=samples, P=P, groups=groups, eps=1e-5, silu=True, x1=s.cuda())
    close(y, ref, rtol=tol16(8e-3), atol=tol16(8e-3))
    x = rnd(77, 320, seed=34)
    gl, bl = rnd(320, seed=35), rnd(320, seed=36)
    close(bf.op_layernorm(x.cuda(), gl.cuda(), bl.cuda()), F.layer_norm(rb(x), (320,), gl, bl), rtol=tol16(8e-3), atol=tol16(8e-3))
    d, f, hw, n, heads = 40, 6, 33, 2, 8
    c = heads * d
    qkv = rnd(n * f * hw, 3 * c, seed=37)
    t = rb(qkv).reshape(n, f, hw, 3 * c).permute(0, 2, 1, 3).reshape(n * hw, f, 3 * c)
    q, k, v = t[..., :c], t[..., c:2 * c], t[..., 2 * c:]
    ref = _unheads(_ref_attn(_heads(q, heads), _heads(k, heads), _heads(v, heads), d ** -0.5), heads)
    ref = ref.reshape(n, hw, f, c).permute(0, 2, 1, 3).reshape(n * f * hw, c)
    y = bf.op_temporal_attention(qkv.cuda(), n=n, F=f, HW=hw, heads=heads, D=d, scale=d ** -0.5)
    close(y, ref, rtol=tol16(8e-3), atol=tol16(8e-3))


def test_bf16_groupnorm_four_channels_per_lane(bf):
    """Widths that are no multiple of 8 (c0 = 60, c1 = 36): gn_partial_kernel and gn_apply_kernel at 4 channels per lane on 16-bit rows,
    both sources, two row chunks (P = 70): against torch on rounded inputs, to one rounding of the output."""
    samples, P, c0, c1, groups = 2, 70, 60, 36, 8
    a, s = rnd(samples * P, c0, seed=150), rnd(samples * P, c1, seed=151)
    g, be = rnd(c0 + c1, seed=152), rnd(c0 + c1, seed=153)
    xin = torch.cat([rb(a), rb(s)], 1).reshape(samples, P, c0 + c1).permute(0, 2, 1)
    ref = F.silu(F.group_norm(xin, groups, g, be, 1e-5)).permute(0, 2, 1).reshape(samples * P, c0 + c1)
    y = bf.op_groupnorm(a.cuda(), g.cuda(), be.cuda(), samples=samples, P=P, groups=groups, eps=1e-5, silu=True, x1=s.cuda())
    close(y, ref, rtol=tol16(8e-3), atol=tol16(8e-3))


@pytest.mark.parametrize("c,rows", [(320, 128), (640, 192), (1280, 64), (256, 320), (512, 64), (64, 128)])
def test_rowblock_sums_against_fp64(eng, c, rows):
    """The row-block sums a conv of the bf16 mode leaves for the GroupNorm behind it (IgemmArgs::rbsum; here from the stand-alone kernel
    that reproduces the epilogue's summation order): (sum, sum of squares) per 64-row block and channel of the bf16-ROUNDED tensor,
    against fp64 to fp32 summation accuracy."""
    x = rnd(rows, c, seed=300) * 3.0 + 0.5
    y = eng.op_rowblock_sums(x.cuda()).cpu().double()
    xb = rb(x).double().reshape(rows // 64, 64, c)
    ref = torch.stack([xb.sum(1), (xb * xb).sum(1)], dim=-1)
    assert y.shape == ref.shape
    assert (y - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()


@pytest.mark.parametrize("c,rows", [(320, 77), (320, 16), (640, 45), (1280, 13), (1280, 4)])
def test_bf16_layernorm_sub_wave_rows(bf, c, rows):
    """The LayerNorm whose rows share a wave (8 / 16 / 32 lanes per row at C = 320 / 640 / 1280, E2V_LN_ROWS), ragged last row group:
    against torch on bf16-rounded input, and against the wave-per-row-group kernel (same arithmetic, other summation order)."""
    x = rnd(rows, c, seed=140)
    gl, bl = rnd(c, seed=141), rnd(c, seed=142)
    ref = F.layer_norm(rb(x), (c,), gl, bl)
    try:
        bf.set_knob("E2V_LN_ROWS", 1)
        y = bf.op_layernorm(x.cuda(), gl.cuda(), bl.cuda())
        bf.set_knob("E2V_LN_ROWS", 0)
        y0 = bf.op_layernorm(x.cuda(), gl.cuda(), bl.cuda())
    finally:
        bf.set_knob("E2V_LN_ROWS", 1)
    close(y, ref, rtol=tol16(8e-3), atol=tol16(8e-3))
    close(y, y0, rtol=tol16(8e-3), atol=tol16(8e-3))


@pytest.mark.parametrize("c0,c1,groups,silu", [(320, 0, 32, True), (320, 320, 32, True), (640, 320, 32, True), (1280, 640, 32, False), (128, 0, 32, True)])
def test_bf16_groupnorm_row_tiled_and_sample_runs(bf, c0, c1, groups, silu):
    """The row-tiled apply pass (E2V_GN_ROWS) and the statistics -> apply runs of samples sized for the Infinity Cache (E2V_GN_GROUP_MB):
    5 samples x 700 rows (a ragged last row chunk), one or two sources.  Runs of samples change the launch order only: bit-identical
    to the whole-tensor launch; the row-tiled pass against the flat one: the same affine, SiLU through exp2 / rcp instead of
    expf / division -> one bf16 rounding; both against torch on bf16-rounded inputs."""
    samples, P = 5, 700
    a = rnd(samples * P, c0, seed=130)
    s = rnd(samples * P, c1, seed=131) if c1 else None
    g, be = rnd(c0 + c1, seed=132), rnd(c0 + c1, seed=133)
    xin = (torch.cat([rb(a), rb(s)], 1) if c1 else rb(a)).reshape(samples, P, c0 + c1).permute(0, 2, 1)
    ref = F.group_norm(xin, groups, g, be, 1e-5)
    ref = (F.silu(ref) if silu else ref).permute(0, 2, 1).reshape(samples * P, c0 + c1)
    run = lambda: bf.op_groupnorm(a.cuda(), g.cuda(), be.cuda(), samples=samples, P=P, groups=groups, eps=1e-5, silu=silu,
                                  x1=s.cuda() if c1 else None)
    whole = run()
    close(whole, ref, rtol=tol16(8e-3), atol=tol16(8e-3))
    if not ab_build(bf):
        return                                                # (the two other arms exist in `make AB=1` builds only)
    try:
        bf.set_knob("E2V_GN_GROUP_MB", 1)                     # 0.45 .. 2.7 MB per sample -> runs of one or two samples
        runs = run()
        bf.set_knob("E2V_GN_ROWS", 0)
        flat = run()
    finally:
        bf.set_knob("E2V_GN_ROWS", 1); bf.set_knob("E2V_GN_GROUP_MB", 0)
    assert torch.equal(whole, runs)
    close(whole, flat, rtol=tol16(8e-3), atol=tol16(8e-3))


@pytest.mark.parametrize("d,nq,f,n,mode", [(8, 108, 3, 2, 0), (16, 30, 4, 1, 0), (32, 9, 3, 2, 0), (40, 200, 6, 1, 0), (80, 144, 3, 1, 0),
                                           (160, 40, 6, 2, 0), (64, 70, 2, 1, 0), (40, 300, 3, 2, 1), (160, 40, 3, 2, 1)])
def test_bf16_attention(eng, d, nq, f, n, mode, h16):
    """bf16 MFMA attention (configs[2]): Q, K, V, P rounded to bf16, fp32 softmax / accumulate; tolerance 2e-2 of the
    output scale against the fp32 reference."""
    heads = 8 if d != 160 else 4
    c = heads * d
    try:
        eng.set_compute_dtype(h16)
        if mode == 0:
            qkv = rnd(n * f * nq, 3 * c, seed=80)
            q, k, v = (qkv[:, i * c:(i + 1) * c].reshape(n * f, nq, c) for i in range(3))
            former = torch.arange(f) - 1
            former[0] = 0
            gather = lambda t: torch.cat([t.reshape(n, f, nq, c)[:, [0] * f], t.reshape(n, f, nq, c)[:, former]], dim=2).reshape(n * f, 2 * nq, c)
            ref = _unheads(_ref_attn(_heads(q, heads), _heads(gather(k), heads), _heads(gather(v), heads), d ** -0.5), heads)
            g = qkv.cuda()
            y = eng.op_attention(g[:, :c], g[:, c:2 * c], g[:, 2 * c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nq, mode=0, scale=d ** -0.5)
        else:
            nk = 77
            q, kv = rnd(n * f * nq, c, seed=81), rnd(n * nk, 2 * c, seed=82)
            k, v = kv[:, :c].reshape(n, nk, c), kv[:, c:].reshape(n, nk, c)
            rep = lambda t: t.repeat_interleave(f, 0)
            ref = _unheads(_ref_attn(_heads(q.reshape(n * f, nq, c), heads), _heads(rep(k), heads), _heads(rep(v), heads), d ** -0.5), heads)
            gq, gkv = q.cuda(), kv.cuda()
            y = eng.op_attention(gq, gkv[:, :c], gkv[:, c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nk, mode=1, scale=d ** -0.5)
        close(y.reshape(n * f, nq, c), ref, rtol=tol16(2e-2), atol=tol16(2e-2))
    finally:
        eng.set_compute_dtype("fp32")


@pytest.mark.parametrize("d,nq,f,n,nk,qboost", [(40, 333, 6, 9, 77, 1.0), (80, 100, 3, 2, 77, 1.0), (160, 40, 3, 10, 77, 1.0), (40, 50, 2, 1, 96, 1.0),
                                                 (40, 70, 2, 3, 33, 1.0), (40, 200, 2, 2, 77, 30.0), (8, 45, 2, 1, 5, 1.0)])
def test_bf16_cross_attention_resident_keys(eng, d, nq, f, n, nk, qboost, h16):
    """Cross-attention with the conditioning's K / V resident in LDS (cross_attn_resident_kernel: one-pass softmax over <= 96 keys, no
    barrier in the query loop): 77 keys and other counts (96 = all three key tiles full, 33, 5), >= 8 samples (whole samples per XCD)
    and fewer, a last query tile that is ragged, several tiles per wave, and queries scaled 30x so that |max score| > 8 takes the
    subtract-the-maximum branch.  Against the fp32 reference on bf16-rounded operands, and against the staged kernel."""
    heads = 8 if d != 160 else 4
    c = heads * d
    q, kv = rnd(n * f * nq, c, seed=181) * qboost, rnd(n * nk, 2 * c, seed=182)
    k, v = rb(kv[:, :c]).reshape(n, nk, c), rb(kv[:, c:]).reshape(n, nk, c)
    rep = lambda t: t.repeat_interleave(f, 0)
    qs = d ** -0.5 * 1.4426950408889634                   # the kernels fold scale * log2(e) into Q and round it to bf16 once: so does the reference
    q_eff = rb(rb(q) * qs) / qs
    ref = _unheads(_ref_attn(_heads(q_eff.reshape(n * f, nq, c), heads), _heads(rep(k), heads), _heads(rep(v), heads), d ** -0.5), heads)
    gq, gkv = q.cuda(), kv.cuda()
    run = lambda: eng.op_attention(gq, gkv[:, :c], gkv[:, c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nk, mode=1, scale=d ** -0.5)
    try:
        eng.set_compute_dtype(h16)
        eng.set_knob("E2V_ATTN_CROSS_RESIDENT", 1)
        y = run()
        eng.set_knob("E2V_ATTN_CROSS_RESIDENT", 0)
        y0 = run()
    finally:
        eng.set_knob("E2V_ATTN_CROSS_RESIDENT", 1)
        eng.set_compute_dtype("fp32")
    close(y.reshape(n * f, nq, c), ref, rtol=tol16(2e-2), atol=tol16(2e-2))
    close(y, y0, rtol=tol16(2e-2), atol=tol16(2e-2))
    assert torch.isfinite(y).all()


def test_linear_16k_and_32k_tiles_are_bit_identical(monkeypatch):
    """The taps == 1 layers run on the 16-k-stage tile (three workgroups per CU) by default; the 32-k tile (E2V_IGEMM_K16=0) walks
    k in the same order, so the two must agree bit for bit -- on plain, residual and GEGLU epilogues, ragged M / N included."""
    import subprocess, sys, os
    code = r'''
import sys, torch
sys.path.insert(0, %r)
from eeg2video_amd.engine import Engine
from eeg2video_amd.weights import TINY_UNET, TINY_VAE
eng = Engine(TINY_UNET, TINY_VAE, 0)
g = torch.Generator().manual_seed(5)
outs = []
for m, k, n, geglu in [(1000, 320, 960, False), (130, 40, 72, False), (864, 320, 2560, True), (4097, 1280, 320, False)]:
    x, w, b = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) * 0.05, torch.randn(n, generator=g)
    r = None if geglu else torch.randn(m, n, generator=g).cuda()
    outs.append(eng.op_linear(x.cuda(), w.cuda(), b.cuda(), r, geglu=geglu).cpu())
torch.save(outs, sys.argv[1])
''' % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import tempfile
    res = []
    for flag in ("1", "0"):
        with tempfile.NamedTemporaryFile(suffix=".pt") as f:
            env = dict(os.environ, E2V_IGEMM_K16=flag)
            subprocess.run([sys.executable, "-c", code, f.name], check=True, env=env, timeout=300)
            res.append(torch.load(f.name))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("m,k,n", [(133, 64, 70), (40, 320, 3), (257, 128, 129)])
def test_linear_width_not_multiple_of_four(eng, m, k, n):
    """N % 4 != 0 takes the scalar epilogue (no 16-byte accesses) of the tiles."""
    x, w, b = rnd(m, k, seed=70), rnd(n, k, seed=71, scale=0.05), rnd(n, seed=72)
    close(eng.op_linear(x.cuda(), w.cuda(), b.cuda()), F.linear(x, w, b))


# ------------------------------------------------------------------ bf16 mode: the 256-row deep-pipelined tiles (bgemm256.hip) -------
# Layers with whole 64-deep K steps, K >= 640 and N a multiple of 320 (256 x 320 tiles) or 256 (GEGLU, the VAE's widths) take
# bgemm_t256_kernel: v_mfma_f32_16x16x32_bf16, two K-step buffers restaged piecewise, staggered wave rows.  Same contract as the
# tiles of bgemm.hip, so: the same tight comparison with the op on bf16-rounded operands (summation order only), on shapes that
# cover ragged row blocks, several images under one tile, the concat seam, stride 2 with both paddings, odd / even K-step
# counts, one K step less than the pipeline depth... and, with E2V_BGEMM_T256 = 0, closeness to the other kernels.
@pytest.fixture
def bf256(bf):
    """bf16 mode with the 256-row tiles FORCED wherever the layer shape allows them (E2V_BGEMM_T256 = 2: the launch-size and
    residual rules of the dispatcher, which would send these small test launches to bgemm.hip, are off)."""
    bf.set_knob("E2V_BGEMM_T256", 2)
    yield bf
    bf.set_knob("E2V_BGEMM_T256", 1)


@pytest.mark.parametrize("m,k,n,resid", [(240, 1280, 1280, True), (300, 320, 960, False), (1000, 320, 320, True), (70001, 320, 960, True), (1000, 640, 320, True), (4097, 704, 640, False), (256, 640, 512, True),
                                         (777, 1920, 256, False), (513, 2560, 320, True), (64, 640, 960, False)])
def test_bf16_t256_linear(bf256, m, k, n, resid):
    bf = bf256
    x, w, b = rnd(m, k, seed=120), rnd(n, k, seed=121, scale=0.05), rnd(n, seed=122)
    r = rnd(m, n, seed=123) if resid else None
    y = bf.op_linear(x.cuda(), w.cuda(), b.cuda(), r.cuda() if resid else None)
    ref = F.linear(rb(x), rb(w), b) + (r if resid else 0)
    close(y, ref, rtol=1e-4, atol=1e-4)
    bf.set_knob("E2V_BGEMM_T256", 0)
    try:
        y0 = bf.op_linear(x.cuda(), w.cuda(), b.cuda(), r.cuda() if resid else None)
    finally:
        bf.set_knob("E2V_BGEMM_T256", 2)
    assert torch.equal(y, y0)           # same k order, and the two MFMA shapes round alike: the dispatcher's choice never changes a result
    # the persistent form (workgroups walk a tile list, the DMA stream runs on across tile boundaries, register epilogue) against the
    # one-tile-per-workgroup form: P = 2 forces it on every linear, P = 0 switches it off
    outs = []
    for pers in (2, 0):
        bf.set_knob("E2V_BGEMM_T256P", pers)
        try:
            outs.append(bf.op_linear(x.cuda(), w.cuda(), b.cuda(), r.cuda() if resid else None))
        finally:
            bf.set_knob("E2V_BGEMM_T256P", 1)
    close(outs[0], ref, rtol=1e-4, atol=1e-4)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], y0)
    print(f"T256 vs bgemm.hip tiles (m={m}, k={k}, n={n}): bit-identical = {torch.equal(y, y0)}, max |diff| = {(y - y0).abs().max().item():.3e}")


@pytest.mark.parametrize("m,k,n", [(300, 640, 512), (1000, 1280, 2560), (130, 704, 5120), (70000, 320, 512)])
def test_bf16_t256_geglu(bf256, m, k, n):
    bf = bf256
    """GEGLU projection (attention.py:189): packed width n = 2 x out, value / gate interleaved per 64 columns -> 256 x 256 tiles."""
    x, w, b = rnd(m, k, seed=130), rnd(n, k, seed=131, scale=0.05), rnd(n, seed=132)
    hh, gg = F.linear(rb(x), rb(w), b).chunk(2, dim=-1)
    outs = []
    for pers in (2, 0):
        bf.set_knob("E2V_BGEMM_T256P", pers)
        try:
            outs.append(bf.op_linear(x.cuda(), w.cuda(), b.cuda(), geglu=True))
        finally:
            bf.set_knob("E2V_BGEMM_T256P", 1)
    close(outs[0], hh * gelu_bf16_grade(gg), rtol=1e-4, atol=1e-4)
    close(outs[0], hh * F.gelu(gg), rtol=tol16(4e-4, 1e-4), atol=tol16(4e-4, 1e-4))
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("cin,cout,n,h,w,stride", [(128, 320, 3, 9, 16, 1), (64, 640, 2, 18, 32, 1), (192, 320, 7, 5, 8, 1), (128, 256, 1, 36, 64, 1),
                                                   (128, 320, 2, 17, 12, 2), (320, 320, 2, 36, 64, 1), (64, 512, 1, 9, 16, 1)])
def test_bf16_t256_conv3x3(bf256, cin, cout, n, h, w, stride):
    bf = bf256
    """3x3 convs on the 256-row tiles: images of 144 / 576 / 40 / 2304 pixels (a tile spans several images or a fraction of one, the
    last tile is ragged), 9 x (cin / 64) K steps, stride 2 (Downsample3D)."""
    x, wt, b = rnd(n, cin, h, w, seed=140), rnd(cout, cin, 3, 3, seed=141, scale=0.05), rnd(cout, seed=142)
    ref = F.conv2d(rb(x), rb(wt), b, padding=1, stride=stride)
    y = bf.op_conv3x3(to_cl(x).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=h, Ws=w, stride=stride)
    close(from_cl(y, n, ref.shape[2], ref.shape[3]), ref, rtol=1e-4, atol=1e-4)
    bf.set_knob("E2V_BGEMM_T256", 0)
    try:
        y0 = bf.op_conv3x3(to_cl(x).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=h, Ws=w, stride=stride)
    finally:
        bf.set_knob("E2V_BGEMM_T256", 2)
    assert torch.equal(y, y0)


def test_bf16_t256_conv3x3_geometries(bf256):
    bf = bf256
    """The VAE encoder's stride-2 conv with (0, 1) padding, and the resnet's second conv at the up-blocks: channel concat with the
    time-embedding row and the residual (two X sources with different row strides, the K loop crossing the seam)."""
    n, c, cout = 2, 128, 256
    wt, b = rnd(cout, c, 3, 3, seed=150, scale=0.05), rnd(cout, seed=151)
    x2 = rnd(n, c, 8, 12, seed=152)
    ref2 = F.conv2d(F.pad(rb(x2), (0, 1, 0, 1)), rb(wt), b, stride=2)
    y2 = bf.op_conv3x3(to_cl(x2).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=8, Ws=12, stride=2, pad_lo=0, pad_hi=1)
    close(from_cl(y2, n, ref2.shape[2], ref2.shape[3]), ref2, rtol=1e-4, atol=1e-4)
    n_s, f, c0, c1, cout, h, w = 2, 3, 128, 64, 320, 9, 16
    nn = n_s * f
    a, s = rnd(nn, c0, h, w, seed=153), rnd(nn, c1, h, w, seed=154)
    wc, bc = rnd(cout, c0 + c1, 3, 3, seed=155, scale=0.05), rnd(cout, seed=156)
    temb, res = rnd(n_s, cout, seed=157), rnd(nn, cout, h, w, seed=158)
    refc = F.conv2d(torch.cat([rb(a), rb(s)], 1), rb(wc), bc, padding=1) + temb.repeat_interleave(f, 0)[:, :, None, None] + res
    yc = bf.op_conv3x3(to_cl(a).cuda(), wc.cuda(), bc.cuda(), x1=to_cl(s).cuda(), n_img=nn, Hs=h, Ws=w,
                       rowbias=temb.cuda().contiguous(), rows_per_sample=f * h * w, resid=to_cl(res).cuda())
    close(from_cl(yc, nn, h, w), refc, rtol=1e-4, atol=1e-4)


def test_bf16_t256_tail_split(bf256):
    """A launch whose last round of 256 workgroups would be at most half full sends the row blocks of that round through a second
    launch of 256 x 192 and 256 x 128 tiles (bgemm_t256_tail_kernel).  Same k order per output: bit-identical to the unsplit launch.
    Linear (persistent main part, residual) and 3x3 conv (time-embedding rows, residual, a ragged last row block)."""
    bf = bf256
    if not ab_build(bf):
        pytest.skip("the tail split was measured and not adopted: its kernel exists in `make AB=1` builds only")
    m, k, n = 256 * 66 + 40, 320, 1280                     # 67 row blocks x 4 column tiles = 268 tiles: one full round + 12
    x, w, b, r = rnd(m, k, seed=190), rnd(n, k, seed=191, scale=0.05), rnd(n, seed=192), rnd(m, n, seed=193)
    nimg, c, cout, h, wd = 118, 64, 1280, 9, 16             # M = 16 992 = 66.4 row blocks
    xc, wc, bc = rnd(nimg, c, h, wd, seed=194), rnd(cout, c, 3, 3, seed=195, scale=0.05), rnd(cout, seed=196)
    temb, res = rnd(2, cout, seed=197), rnd(nimg, cout, h, wd, seed=198)
    outs = {}
    try:
        for tail in (1, 0):
            bf.set_knob("E2V_BGEMM_T256_TAIL", tail)
            y = bf.op_linear(x.cuda(), w.cuda(), b.cuda(), r.cuda())
            yc = bf.op_conv3x3(to_cl(xc).cuda(), wc.cuda(), bc.cuda(), n_img=nimg, Hs=h, Ws=wd, rowbias=temb.cuda().contiguous(),
                               rows_per_sample=59 * h * wd, resid=to_cl(res).cuda())
            outs[tail] = (y, yc)
    finally:
        bf.set_knob("E2V_BGEMM_T256_TAIL", 0)                 # (the default: measured +-0 over a UNet step)
    assert torch.equal(outs[1][0], outs[0][0]) and torch.equal(outs[1][1], outs[0][1])
    close(outs[1][0], F.linear(rb(x), rb(w), b) + r, rtol=1e-4, atol=1e-4)
    refc = F.conv2d(rb(xc), rb(wc), bc, padding=1) + temb.repeat_interleave(59, 0)[:, :, None, None] + res
    close(from_cl(outs[1][1], nimg, h, wd), refc, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("n,c,cout,hs,ws", [(12, 320, 320, 18, 32), (5, 256, 256, 9, 16), (3, 640, 640, 5, 8), (2, 128, 512, 7, 6)])
def test_bf16_upsample_conv_sub_pixel_form(bf256, n, c, cout, hs, ws):
    """`Upsample3D` (resnet.py:30-62: nearest 2x + 3x3 conv) as four 2x2 convs on the source map, one per output parity, weights summed
    over the taps that read the same source pixel (bgemm_up2x: 4 / 9 of the multiplies).  (1) the identity itself, pure torch in
    fp64; (2) the HIP result against that parity form with the kernel's operand rounding (x and the SUMMED weights rounded to
    bf16): summation order only, 1e-4; (3) against the resize-then-conv on the old gather path (E2V_BGEMM_UP2X = 0), which rounds the
    nine weights separately: one bf16 rounding of a weight apart."""
    bf = bf256
    x, wt, b = rnd(n, c, hs, ws, seed=170), rnd(cout, c, 3, 3, seed=171, scale=0.05), rnd(cout, seed=172)
    sets = {0: ([0], [1, 2]), 1: ([0, 1], [2])}          # parity -> taps of the 3-wide kernel that fall on source offset 0 / 1

    def parity_form(xx, ww, bb, round_w):
        out = torch.zeros(n, cout, 2 * hs, 2 * ws, dtype=xx.dtype)
        for a in (0, 1):
            for bq in (0, 1):
                w2 = torch.stack([torch.stack([ww[:, :, sets[a][ty]][:, :, :, sets[bq][tx]].sum((2, 3)) for tx in (0, 1)], -1) for ty in (0, 1)], -2)
                if round_w:
                    w2 = rb(w2)
                out[:, :, a::2, bq::2] = F.conv2d(F.pad(xx, (1 - bq, bq, 1 - a, a)), w2, bb)
        return out

    direct = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), wt.double(), b.double(), padding=1)
    assert (parity_form(x.double(), wt.double(), b.double(), False) - direct).abs().max() < 1e-10
    ref = parity_form(rb(x), wt, b, True)
    try:
        bf.set_knob("E2V_BGEMM_UP2X", 1)
        y = bf.op_conv3x3(to_cl(x).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=hs, Ws=ws, Hi=2 * hs, Wi=2 * ws)
        bf.set_knob("E2V_BGEMM_UP2X", 0)
        y0 = bf.op_conv3x3(to_cl(x).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=hs, Ws=ws, Hi=2 * hs, Wi=2 * ws)
    finally:
        bf.set_knob("E2V_BGEMM_UP2X", 1)
    close(from_cl(y, n, 2 * hs, 2 * ws), ref, rtol=1e-4, atol=1e-4)
    close(from_cl(y0, n, 2 * hs, 2 * ws), F.conv2d(F.interpolate(rb(x), scale_factor=2, mode="nearest"), rb(wt), b, padding=1), rtol=1e-4, atol=1e-4)
    assert not torch.equal(y, y0)                          # (the sub-pixel form did run: its weight rounding differs)
    close(y, y0, rtol=tol16(4e-3), atol=tol16(4e-3))


@pytest.mark.parametrize("d,nq,f,n", [(40, 256, 3, 1), (40, 333, 4, 9), (40, 192, 2, 2), (40, 130, 3, 1), (40, 2304, 2, 1)])
def test_bf16_attention_64_queries_per_wave(eng, d, nq, f, n, h16):
    """flash_attn_b16q64_kernel (attn_q64.hip; SparseCausalAttention, attention.py:272-328): a wave owns two 32-query blocks.  Whole
    workgroups of 4 / 3 / 2 waves (256 / 192 / 128 queries), a ragged last query block (333, 130: a wave whose second block is empty, a
    wave with no query at all), a ragged last key tile, >= 8 samples (whole samples per XCD) and fewer, frames 0 / 1 (one key segment) and
    later ones (two), and the UNet's level-0 size.  Against the fp32 reference on the operands as the kernel rounds them (Q pre-multiplied
    by scale * log2 e and rounded to bf16 once), and bit for bit against the 32-query kernel (the integer test for "some score tops its
    row's maximum by 2^8" decides as the float maximum does)."""
    heads = 8
    c = heads * d
    qkv = rnd(n * f * nq, 3 * c, seed=280)
    qs = d ** -0.5 * 1.4426950408889634
    q = (rb(rb(qkv[:, :c]) * qs) / qs).reshape(n * f, nq, c)
    k, v = (rb(qkv[:, i * c:(i + 1) * c]).reshape(n * f, nq, c) for i in (1, 2))
    former = torch.arange(f) - 1
    former[0] = 0
    gather = lambda t: torch.cat([t.reshape(n, f, nq, c)[:, [0] * f], t.reshape(n, f, nq, c)[:, former]], dim=2).reshape(n * f, 2 * nq, c)
    ref = _unheads(_ref_attn(_heads(q, heads), _heads(gather(k), heads), _heads(gather(v), heads), d ** -0.5), heads)
    try:
        eng.set_compute_dtype(h16)
        g = qkv.cuda()
        run = lambda: eng.op_attention(g[:, :c], g[:, c:2 * c], g[:, 2 * c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nq, mode=0, scale=d ** -0.5)
        ab = ab_build(eng)
        y = run()                                         # the software-pipelined form (the default at d = 40)
        if ab:
            eng.set_knob("E2V_ATTN_Q64P", 0)
            yp = run()                                    # the phase-by-phase form (`make AB=1` builds only)
        eng.set_knob("E2V_ATTN_Q64", 0)
        y32 = run()
    finally:
        eng.set_knob("E2V_ATTN_Q64", 1)
        if ab:
            eng.set_knob("E2V_ATTN_Q64P", 1)
        eng.set_compute_dtype("fp32")
    # pipelined form: the reference maximum is a bf16 number carried in Q, so P rounds differently: same softmax, other roundings
    assert not torch.equal(y, y32)
    close(y.reshape(n * f, nq, c), ref, rtol=tol16(1e-2), atol=tol16(1e-2))            # bf16 rounding of P and of the output
    close(y32.reshape(n * f, nq, c), ref, rtol=tol16(1e-2), atol=tol16(1e-2))
    close(y, y32, rtol=tol16(1e-2), atol=tol16(1e-2))
    if ab:      # phase form: same MFMA sequence per (query, key tile) and the same maximum decisions per 32-query block as the 32-query kernel
        assert torch.equal(yp, y32)


def test_bf16_attention_64_queries_per_wave_random_shapes(eng, h16):
    """A sweep of ragged shapes through the 64-query kernel -- query counts that leave the last workgroup one, two, three or four waves,
    waves with one query block or none, key counts that end a 64-key stage after 1 .. 63 keys (marker-column masking) or exactly on
    it, 1 .. 6 frames (one or two key segments), fewer and more than 8 samples (the two XCD mappings) -- each against the 32-query
    kernel, which the tests above hold against torch: same softmax, other roundings."""
    import random
    rng = random.Random(20240)
    heads, d = 8, 40
    c = heads * d
    try:
        eng.set_compute_dtype(h16)
        for case in range(14):
            nq = rng.choice([128, 129, 191, 192, 193, 255, 256, 257, 320, 383, 448, 511, 577, 640])
            f = rng.randint(1, 6)
            n = rng.choice([1, 2, 3, 8, 9, 11])
            qkv = rnd(n * f * nq, 3 * c, seed=400 + case)
            g = qkv.cuda()
            run = lambda: eng.op_attention(g[:, :c], g[:, c:2 * c], g[:, 2 * c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nq, mode=0, scale=d ** -0.5)
            eng.set_knob("E2V_ATTN_Q64", 1)
            y = run()
            eng.set_knob("E2V_ATTN_Q64", 0)
            y32 = run()
            assert torch.isfinite(y).all(), (nq, f, n)
            err = (y - y32).abs().max().item() / (y32.abs().max().item() + 1e-30)
            assert err < tol16(1e-2), (nq, f, n, err)
    finally:
        eng.set_knob("E2V_ATTN_Q64", 1)
        eng.set_compute_dtype("fp32")


def test_bf16_attention_64_queries_per_wave_huge_scores(eng, h16):
    """The pipelined 64-query kernel carries a row's reference maximum in Q as the sum of two bf16 numbers.  Queries scaled 400x put
    the scores in the thousands (one bf16 number would be off by up to 16 there and a far larger factor beyond): the softmax is then
    nearly one-hot, must stay finite, and must pick the same keys as the fp32 reference on the bf16-rounded operands."""
    heads, d, n, f, nq = 8, 40, 1, 3, 256
    c = heads * d
    qkv = rnd(n * f * nq, 3 * c, seed=281)
    qkv[:, :c] *= 400.0
    qs = d ** -0.5 * 1.4426950408889634
    q = (rb(rb(qkv[:, :c]) * qs) / qs).reshape(n * f, nq, c)
    k, v = (rb(qkv[:, i * c:(i + 1) * c]).reshape(n * f, nq, c) for i in (1, 2))
    former = torch.arange(f) - 1
    former[0] = 0
    gather = lambda t: torch.cat([t.reshape(n, f, nq, c)[:, [0] * f], t.reshape(n, f, nq, c)[:, former]], dim=2).reshape(n * f, 2 * nq, c)
    ref = _unheads(_ref_attn(_heads(q, heads), _heads(gather(k), heads), _heads(gather(v), heads), d ** -0.5), heads)
    try:
        eng.set_compute_dtype(h16)
        g = qkv.cuda()
        y = eng.op_attention(g[:, :c], g[:, c:2 * c], g[:, 2 * c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nq, mode=0, scale=d ** -0.5)
    finally:
        eng.set_compute_dtype("fp32")
    assert torch.isfinite(y).all()
    close(y.reshape(n * f, nq, c), ref, rtol=tol16(2e-2), atol=tol16(2e-2))


@pytest.mark.parametrize("boost", [3.0, 25.0])
def test_bf16_attention_deferred_maximum_branches(eng, boost, h16):
    """bf16 attention keeps a row's reference maximum until a score exceeds it by more than 2^8 (the rescale of the accumulators is
    a wave-level branch that would otherwise run on most key tiles).  Both sides of that threshold against a FULL fp32 reference on
    the bf16-rounded inputs: late keys (3rd and 5th 32-key tile, second key segment too) boosted 3x -- their scores top the running
    maximum by LESS than the threshold: the deferred path, probabilities above 1 -- and 25x: far above it, the rescale branch.  Rows
    come out wrong by O(0.1) if either path scales the accumulator, the pending probabilities or the normaliser inconsistently."""
    heads, d, n, f, nq = 8, 40, 1, 3, 200
    c = heads * d
    qkv = rnd(n * f * nq, 3 * c, seed=153)
    for key in (70, 150, 2 * nq + 130, nq + 190):
        qkv[key, c:2 * c] *= boost
    qb = rb(qkv)
    q, k, v = (qb[:, i * c:(i + 1) * c].reshape(n * f, nq, c) for i in range(3))
    former = torch.arange(f) - 1
    former[0] = 0
    gather = lambda t: torch.cat([t.reshape(n, f, nq, c)[:, [0] * f], t.reshape(n, f, nq, c)[:, former]], dim=2).reshape(n * f, 2 * nq, c)
    ref = _unheads(_ref_attn(_heads(q, heads), _heads(gather(k), heads), _heads(gather(v), heads), d ** -0.5), heads)
    try:
        eng.set_compute_dtype(h16)
        g = qkv.cuda()
        outs = []
        ab = ab_build(eng)
        # 64 queries per wave (attn_q64.hip, pipelined), the 32-query kernel; `make AB=1` builds: + the phase form and the plain (no fold) form
        arms = ((1, 1, 1), (0, 1, 1)) + (((1, 0, 1), (0, 0, 0)) if ab else ())
        for q64, q64p, fold in arms:
            eng.set_knob("E2V_ATTN_Q64", q64)
            if ab:
                eng.set_knob("E2V_ATTN_Q64P", q64p)
                eng.set_knob("E2V_ATTN_FOLD", fold)
            outs.append(eng.op_attention(g[:, :c], g[:, c:2 * c], g[:, 2 * c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nq, mode=0, scale=d ** -0.5))
    finally:
        eng.set_knob("E2V_ATTN_Q64", 1)
        if ab:
            eng.set_knob("E2V_ATTN_FOLD", 1); eng.set_knob("E2V_ATTN_Q64P", 1)
        eng.set_compute_dtype("fp32")
    if ab:
        assert torch.equal(outs[2], outs[1])                 # both sides of the threshold: the phase form and the 32-query kernel decide and round alike
    for y in outs:
        close(y.reshape(n * f, nq, c), ref, rtol=tol16(2e-2), atol=tol16(2e-2))


def _sparse_causal_ref(q, k, v, n, f, nq, c, heads, d):
    former = torch.arange(f) - 1
    former[0] = 0
    gather = lambda t: torch.cat([t.reshape(n, f, nq, c)[:, [0] * f], t.reshape(n, f, nq, c)[:, former]], dim=2).reshape(n * f, 2 * nq, c)
    return _unheads(_ref_attn(_heads(q, heads), _heads(gather(k), heads), _heads(gather(v), heads), d ** -0.5), heads)


@pytest.mark.parametrize("q64", [1, 0])
def test_h16_attention_hugely_negative_scores_with_a_ragged_key_stage(eng, h16, q64):
    """Keys past the end of a segment (Nk % 64 != 0) are masked on the matrix pipe in the 64-query kernel: a marker column of their K rows
    times a mask slot of Q.  The masked score is (-reference maximum) - marker^2, so the marker product must drown ANY reference: every
    real score here sits near -46 000 (log2 units), where a mask of -2^15 (what the kernel used before round 5) would have turned the
    padded keys into +13 000 -> exp2 overflow.  Both kernels (64- and 32-query), both 16-bit types, against fp32 on the rounded operands."""
    heads, d, n, f, nq = 8, 40, 1, 3, 200                  # 200 keys: the last 64-key stage holds 8
    c = heads * d
    qkv = rnd(n * f * nq, 3 * c, seed=501)
    for hh in range(heads):                                # 32 of a head's 40 dims carry +80 (q) / -80 (k): q . k ~ -204 800 per (query, key)
        qkv[:, hh * d:hh * d + 32] = 80.0
        qkv[:, c + hh * d:c + hh * d + 32] = -80.0
    qs = d ** -0.5 * 1.4426950408889634
    q = (rb(rb(qkv[:, :c]) * qs) / qs).reshape(n * f, nq, c)
    k, v = (rb(qkv[:, i * c:(i + 1) * c]).reshape(n * f, nq, c) for i in (1, 2))
    ref = _sparse_causal_ref(q, k, v, n, f, nq, c, heads, d)
    assert (q[0, 0, :d] * k[0, 0, :d]).sum().item() * qs < -40000
    try:
        eng.set_compute_dtype(h16)
        eng.set_knob("E2V_ATTN_Q64", q64)
        g = qkv.cuda()
        y = eng.op_attention(g[:, :c], g[:, c:2 * c], g[:, 2 * c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nq, mode=0, scale=d ** -0.5)
    finally:
        eng.set_knob("E2V_ATTN_Q64", 1)
        eng.set_compute_dtype("fp32")
    assert torch.isfinite(y).all()
    close(y.reshape(n * f, nq, c), ref, rtol=tol16(2e-2), atol=tol16(2e-2))


@pytest.mark.parametrize("q64", [1, 0])
def test_fp16_attention_scores_near_the_top_of_the_fp16_range(eng, q64):
    """Range of the fp16 mode: the reference's .half() run stores q . k * scale as fp16, so scores up to 65 504 stay finite THERE.  The
    kernels keep scores in log2 units (x 1.4427: up to 94 500) in fp32 accumulators; the one fp16 number that scales with them is the
    reference maximum riding in Q in the 64-query kernel -- held as -m / 2 against marker columns of 2.0 (H16Traits<_Float16>).  Scores
    near 5.2e4 (7.6e4 in log2 units, past fp16's 65 504): finite, and the softmax over the small differences is still right."""
    H16.update(name="fp16", dtype=torch.float16)
    try:
        heads, d, n, f, nq = 8, 40, 1, 3, 256
        c = heads * d
        qkv = rnd(n * f * nq, 3 * c, seed=502)
        for hh in range(heads):                            # 36 dims at 96 in q and k: q . k * scale ~ 52 460; 4 dims of noise: a real softmax
            qkv[:, hh * d:hh * d + 36] = 96.0
            qkv[:, c + hh * d:c + hh * d + 36] = 96.0
        qs = d ** -0.5 * 1.4426950408889634
        q = (rb(rb(qkv[:, :c]) * qs) / qs).reshape(n * f, nq, c)
        k, v = (rb(qkv[:, i * c:(i + 1) * c]).reshape(n * f, nq, c) for i in (1, 2))
        s00 = (q[0, 0, :d] * k[0, 0, :d]).sum().item() * d ** -0.5
        assert 5.0e4 < s00 < 6.5504e4 and s00 * 1.4427 > 6.5504e4
        ref = _sparse_causal_ref(q, k, v, n, f, nq, c, heads, d)
        try:
            eng.set_compute_dtype("fp16")
            eng.set_knob("E2V_ATTN_Q64", q64)
            g = qkv.cuda()
            y = eng.op_attention(g[:, :c], g[:, c:2 * c], g[:, 2 * c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nq, mode=0, scale=d ** -0.5)
        finally:
            eng.set_knob("E2V_ATTN_Q64", 1)
            eng.set_compute_dtype("fp32")
        assert torch.isfinite(y).all()
        close(y.reshape(n * f, nq, c), ref, rtol=1e-2, atol=1e-2)
    finally:
        H16.update(name="bf16", dtype=torch.bfloat16)


def test_fp16_activations_near_the_top_of_the_fp16_range(eng):
    """fp16 mode, values a .half() run of the reference can hold: a linear whose accumulators reach 5.8e4 -- and 7.7e4, past 65 504:
    the accumulator is fp32 and the op entry returns it unrounded -- comes back exact; a stored fp16 tensor of +-6e4 goes through
    GroupNorm (fp32 statistics: a sum of squares of 7e12) and comes out +-1."""
    H16.update(name="fp16", dtype=torch.float16)
    try:
        eng.set_compute_dtype("fp16")
        x = torch.full((256, 64), 30.0)
        w = torch.zeros(320, 64)
        w[:, :] = 30.0                                       # 64 * 900 = 57 600
        w[7] = 40.0                                          # 64 * 1200 = 76 800 > 65 504
        y = eng.op_linear(x.cuda(), w.cuda())                # the op entry returns fp32: the accumulator before the fp16 rounding
        assert torch.isfinite(y).all() and y[0, 0].item() == 57600.0 and y[0, 7].item() == 76800.0
        # through a stored fp16 tensor: GroupNorm in -> out rounds to fp16 storage
        big = torch.full((64, 32), 6.0e4)
        big[::2] = -6.0e4
        out = eng.op_groupnorm(big.cuda(), torch.ones(32).cuda(), torch.zeros(32).cuda(), samples=1, P=64, groups=4, eps=1e-5, silu=False)
        assert torch.isfinite(out).all() and (out.abs() - 1.0).abs().max().item() < 2e-3      # +-6e4 is representable: normalised to +-1
    finally:
        eng.set_compute_dtype("fp32")
        H16.update(name="bf16", dtype=torch.bfloat16)


# ------------------------------------------------------------------ split-K (the small-batch dispatch family, bgemm.hip) -------
@pytest.mark.parametrize("runs", [2, 3, 5, 16])
def test_h16_splitk_conv_and_linear_equal_the_unsplit_kernels_to_summation_order(bf, runs):
    """bgemm_splitk_kernel + splitk_reduce_kernel (the reference's clip-by-clip loop, inference_eeg2video.py:90-100, leaves the deep
    levels 40-140 tiles for 256 CUs): K cut into `runs` runs of whole 64-channel chunks, fp32 partial planes, an ordered reduce with the
    epilogue.  E2V_SPLITK_FORCE puts the op entry points on it.  Against the same op on the unsplit kernels: fp32 summation order only
    (1e-5 of the output scale) -- 3x3 convs with a concat (runs inside each source), time-embedding rows + residual, stride 2, a
    ragged last row block, N = 320 (two 128 tiles + one 64) and N = 72; linears with K = 1280 / 2560 + bias + residual."""
    def both(fn):
        try:
            bf.set_knob("E2V_SPLITK_FORCE", runs)
            y = fn()
        finally:
            bf.set_knob("E2V_SPLITK_FORCE", 0)
        return y, fn()
    n_s, f, c0, c1, cout, h, w = 2, 3, 128, 64, 320, 5, 8
    n = n_s * f
    a, s = rnd(n, c0, h, w, seed=601), rnd(n, c1, h, w, seed=602)
    wc, bc = rnd(cout, c0 + c1, 3, 3, seed=603, scale=0.1), rnd(cout, seed=604)
    temb, res = rnd(n_s, cout, seed=605), rnd(n, cout, h, w, seed=606)
    ga, gs, gw, gb, gt, gr = to_cl(a).cuda(), to_cl(s).cuda(), wc.cuda(), bc.cuda(), temb.cuda().contiguous(), to_cl(res).cuda()
    y, y0 = both(lambda: bf.op_conv3x3(ga, gw, gb, x1=gs, n_img=n, Hs=h, Ws=w, rowbias=gt, rows_per_sample=f * h * w, resid=gr))
    ref = F.conv2d(torch.cat([rb(a), rb(s)], 1), rb(wc), bc, padding=1) + temb.repeat_interleave(f, 0)[:, :, None, None] + res
    assert not torch.equal(y, y0)                              # (the split form did run: another summation order)
    close(y, y0, rtol=1e-5, atol=1e-5)
    close(from_cl(y, n, h, w), ref, rtol=1e-4, atol=1e-4)
    x2, w2, b2 = rnd(3, 256, 9, 12, seed=607), rnd(72, 256, 3, 3, seed=608, scale=0.1), rnd(72, seed=609)
    g2, gw2, gb2 = to_cl(x2).cuda(), w2.cuda(), b2.cuda()
    y, y0 = both(lambda: bf.op_conv3x3(g2, gw2, gb2, n_img=3, Hs=9, Ws=12, stride=2))
    close(y, y0, rtol=1e-5, atol=1e-5)
    close(from_cl(y, 3, 5, 6), F.conv2d(rb(x2), rb(w2), b2, stride=2, padding=1), rtol=1e-4, atol=1e-4)
    for m, k, nn in [(480, 1280, 1280), (154, 2560, 320), (1000, 640, 72)]:
        xl, wl, bl, r = rnd(m, k, seed=610), rnd(nn, k, seed=611, scale=0.05), rnd(nn, seed=612), rnd(m, nn, seed=613)
        gx, gwl, gbl, grr = xl.cuda(), wl.cuda(), bl.cuda(), r.cuda()
        y, y0 = both(lambda: bf.op_linear(gx, gwl, gbl, grr))
        close(y, y0, rtol=1e-5, atol=1e-5)
        close(y, F.linear(rb(xl), rb(wl), bl) + r, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("samples,P,c0,c1,groups,silu", [(2, 240, 1280, 0, 32, True), (2, 240, 1280, 1280, 32, True), (3, 864, 1280, 640, 32, True),
                                                         (12, 144, 1280, 0, 32, False), (2, 50, 64, 32, 8, True), (1, 2304, 320, 0, 32, False),
                                                         (3, 45, 80, 0, 8, True)])        # (45 rows x 5 channel pairs: an odd piece count)
def test_h16_groupnorm_one_kernel_form_of_the_small_batch_family(bf, samples, P, c0, c1, groups, silu):
    """gn_fused_small_kernel (norm.hip): one workgroup per (sample, group) reads its P x cpg slice once (both sources of a concat, groups
    that straddle the seam: 1920 / 32 = 60 does not divide 1280), folds in fp64 and applies from LDS -- the small-batch family's
    GroupNorm where the slice fits 144 KB.  Against torch on the rounded inputs to one output rounding, and against the three-launch
    path (same statistics to fp32 rounding: the outputs agree to one rounding of the 16-bit type)."""
    a = rnd(samples * P, c0, seed=700) * 2.0 + 0.3
    s = rnd(samples * P, c1, seed=701) if c1 else None
    g, be = rnd(c0 + c1, seed=702), rnd(c0 + c1, seed=703)
    xin = (torch.cat([rb(a), rb(s)], 1) if c1 else rb(a)).reshape(samples, P, c0 + c1).permute(0, 2, 1)
    ref = F.group_norm(xin, groups, g, be, 1e-5)
    ref = (F.silu(ref) if silu else ref).permute(0, 2, 1).reshape(samples * P, c0 + c1)
    ga, gs, gg, gb = a.cuda(), (s.cuda() if c1 else None), g.cuda(), be.cuda()
    run = lambda: bf.op_groupnorm(ga, gg, gb, samples=samples, P=P, groups=groups, eps=1e-5, silu=silu, x1=gs)
    try:
        bf.set_knob("E2V_GN_FUSED_SMALL", 2)
        y = run()
    finally:
        bf.set_knob("E2V_GN_FUSED_SMALL", 1)
    y0 = run()
    close(y, ref, rtol=tol16(8e-3), atol=tol16(8e-3))
    close(y, y0, rtol=tol16(8e-3), atol=tol16(8e-3))


@pytest.mark.parametrize("samples,P,c0,c1,groups,silu", [(2, 13824, 320, 0, 32, True), (2, 13824, 320, 320, 32, True), (2, 3456, 640, 0, 32, True),
                                                         (2, 3456, 1280, 640, 32, True), (12, 2304, 320, 0, 32, False), (3, 1000, 64, 32, 8, True),
                                                         (1, 77, 96, 0, 4, False)])
def test_h16_groupnorm_cooperative_single_launch(bf, samples, P, c0, c1, groups, silu):
    """gn_coop_kernel (norm.hip): the small-batch family's GroupNorm where the tensor fits the LDS of the chip -- read ONCE by <= 256
    co-resident workgroups (cooperative launch), statistics from LDS, grid barrier, the fp64 fold per (sample, group), grid barrier,
    apply from LDS.  The UNet's level-0 / level-1 shapes of one clip (two samples; per-frame norm: 12), a concat whose groups straddle the
    seam, ragged rows per workgroup.  Against torch on the rounded inputs and against the three-launch path: one output rounding.
    MEASURED AND NOT ADOPTED (the cooperative launch costs more than the two launches it saves: profiles/r05_shape_ab_b1_gn_cooperative.log):
    the kernel exists in `make ab` builds only, where this test runs."""
    try:
        bf.set_knob("E2V_GN_COOP", 0)
    except ValueError:
        pytest.skip("the cooperative one-launch GroupNorm was measured and not adopted: `make ab` builds only (DESIGN 3.9)")
    a = rnd(samples * P, c0, seed=710) * 1.5 + 0.2
    s = rnd(samples * P, c1, seed=711) if c1 else None
    g, be = rnd(c0 + c1, seed=712), rnd(c0 + c1, seed=713)
    xin = (torch.cat([rb(a), rb(s)], 1) if c1 else rb(a)).reshape(samples, P, c0 + c1).permute(0, 2, 1)
    ref = F.group_norm(xin, groups, g, be, 1e-5)
    ref = (F.silu(ref) if silu else ref).permute(0, 2, 1).reshape(samples * P, c0 + c1)
    ga, gs, gg, gb = a.cuda(), (s.cuda() if c1 else None), g.cuda(), be.cuda()
    run = lambda: bf.op_groupnorm(ga, gg, gb, samples=samples, P=P, groups=groups, eps=1e-5, silu=silu, x1=gs)
    try:
        bf.set_knob("E2V_GN_COOP", 2)
        y = run()
    finally:
        bf.set_knob("E2V_GN_COOP", 0)
    y0 = run()
    assert torch.isfinite(y).all()
    close(y, ref, rtol=tol16(8e-3), atol=tol16(8e-3))
    close(y, y0, rtol=tol16(8e-3), atol=tol16(8e-3))
