"""The Winograd transform kernels with what the fp32 resnets fold into them (wino.hip through ``e2v_op_conv3x3_gn``): GroupNorm affine
+ SiLU inside the input transform, time-embedding row and residual in the output transform.

GPU: GroupNorm + SiLU + conv against (a) the unfused chain ``op_groupnorm(silu=True)`` -> ``op_conv3x3`` in the same Winograd form and
(b) torch, at the bounds ``tests/test_hip_ops.py`` applies to these forms -- ``close(rtol=1e-4, atol=1e-4)`` for F(4x4)
(``test_conv3x3_winograd_f4``), the default ``close`` (2e-5) for F(2x2) (``test_conv3x3_winograd``).  Every map has ragged last tiles and
``beta`` is centred at 3: a padding position that contributed SiLU(shift) instead of 0 would move the border outputs by O(1).
CPU: the entry refuses, on a host-only context, a shape for which the library picks no Winograd form."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 2e-5, 2e-5                      # tests/test_hip_ops.py: fp32 vs fp32, different summation order
BOUNDS = {"winograd": dict(rtol=RTOL, atol=ATOL), "winograd4": dict(rtol=1e-4, atol=1e-4)}
GROUPS, EPS, BETA = 32, 1e-5, 3.0

# n_s samples x f frames of hs x ws (-> hi x wi through the nearest resize); c0 (+ c1 concatenated) -> cout channels
CASES = {
    "5x8": dict(n_s=2, f=3, c0=64, c1=0, cout=64, hs=5, ws=8),                              # Ho % 4 == 1
    "9x16_concat_temb_resid": dict(n_s=2, f=3, c0=64, c1=32, cout=64, hs=9, ws=16, epilogue=True),   # seam 64 inside a 3-channel group
    "18x32": dict(n_s=1, f=2, c0=64, c1=0, cout=32, hs=18, ws=32),
    "7x5": dict(n_s=3, f=1, c0=32, c1=0, cout=64, hs=7, ws=5, epilogue=True),
    "5x8_to_9x16": dict(n_s=2, f=2, c0=64, c1=0, cout=64, hs=5, ws=8, hi=9, wi=16),
    "concat_resize_temb_resid": dict(n_s=2, f=2, c0=64, c1=32, cout=32, hs=5, ws=8, hi=9, wi=16, epilogue=True),
}


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def to_cl(x):      # [n, C, H, W] -> [n*H*W, C]
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


def from_cl(y, n, h, w):
    return y.reshape(n, h, w, -1).permute(0, 3, 1, 2).contiguous()


def close(a, b, rtol=RTOL, atol=ATOL, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = b.abs().max().item() + 1e-30
    err = (a - b).abs().max().item()
    bound = atol * max(1.0, scale) + rtol * scale
    print(f"{what}: max abs err {err:.3e} (ref scale {scale:.3e}, bound {bound:.3e})")
    assert err <= bound, f"{what}: max abs err {err:.3e} (ref scale {scale:.3e}, bound {bound:.3e})"


def check_case(eng, algo, n_s, f, c0, c1, cout, hs, ws, hi=None, wi=None, epilogue=False):
    """fused GroupNorm + SiLU + conv == the unfused chain in the same Winograd form == torch"""
    hi, wi = hi or hs, wi or ws
    n, c = n_s * f, c0 + c1
    x = rnd(n, c, hs, ws, seed=1) * 1.5 + 0.3
    ga, be = rnd(c, seed=2) * 0.2 + 1.0, rnd(c, seed=3) * 0.2 + BETA
    wt, b = rnd(cout, c, 3, 3, seed=4, scale=0.1), rnd(cout, seed=5)
    temb, res = (rnd(n_s, cout, seed=6), rnd(n, cout, hi, wi, seed=7)) if epilogue else (None, None)
    # torch: the 5-D GroupNorm of ResnetBlock3D (statistics over the frames of a sample), SiLU, nearest resize, conv
    x5 = x.reshape(n_s, f, c, hs, ws).permute(0, 2, 1, 3, 4)
    act = F.silu(F.group_norm(x5, GROUPS, ga, be, EPS)).permute(0, 2, 1, 3, 4).reshape(n, c, hs, ws)
    if (hi, wi) != (hs, ws):
        act = F.interpolate(act, size=(hi, wi), mode="nearest")
    ref = F.conv2d(act, wt, b, padding=1)
    if epilogue:
        ref = ref + temb.repeat_interleave(f, 0)[:, :, None, None] + res
    x0 = to_cl(x[:, :c0]).cuda()
    x1 = to_cl(x[:, c0:]).cuda() if c1 else None
    epi = dict(rowbias=temb.cuda().contiguous(), rows_per_sample=f * hi * wi, resid=to_cl(res).cuda()) if epilogue else {}
    eng.set_conv_algo(algo)
    try:
        fused = eng.op_conv3x3_gn(x0, ga.cuda(), be.cuda(), wt.cuda(), b.cuda(), x1=x1, n_img=n, Hs=hs, Ws=ws, Hi=hi, Wi=wi,
                                  gn_P=f * hs * ws, groups=GROUPS, eps=EPS, **epi)
        hn = eng.op_groupnorm(x0, ga.cuda(), be.cuda(), samples=n_s, P=f * hs * ws, groups=GROUPS, eps=EPS, silu=True, x1=x1)
        chain = eng.op_conv3x3(hn, wt.cuda(), b.cuda(), n_img=n, Hs=hs, Ws=ws, Hi=hi, Wi=wi, **epi)
        torch.cuda.synchronize()
    finally:
        eng.set_conv_algo("auto")
    assert torch.isfinite(fused).all()
    close(fused, chain, what=f"{algo} fused vs unfused chain", **BOUNDS[algo])
    close(from_cl(fused, n, hi, wi), ref, what=f"{algo} fused vs torch", **BOUNDS[algo])


def conv_launches(eng, algo):
    """wino_in_gn_silu launches of one fused call = the number of image chunks it was split into"""
    eng.profile_begin()
    check_case(eng, algo, **CASES["9x16_concat_temb_resid"])
    return eng.profile_end()["wino_in_gn_silu"]["launches"]


def make_engine():
    from eeg2video_amd.engine import Engine
    from eeg2video_amd.weights import TINY_UNET, TINY_VAE
    return Engine(TINY_UNET, TINY_VAE, 0)


@pytest.fixture(scope="module")
def eng():
    return make_engine()


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["winograd4", "winograd"])
@pytest.mark.parametrize("case", list(CASES))
def test_groupnorm_silu_conv_fused_in_the_transforms(eng, algo, case):
    check_case(eng, algo, **CASES[case])


@pytest.mark.gpu
def test_image_chunks_reach_the_groupnorm_slab_index():
    """A 1 MB workspace (E2V_WINO_WS_MB, read when the context is created: hence the child process) splits the 6 images of two samples
    into passes of 3 + 3 (F(4x4)) and 2 + 2 + 2 (F(2x2)): the later passes start at img_lo > 0, the last one inside the second GroupNorm
    slab."""
    env = dict(os.environ, E2V_WINO_WS_MB="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "chunked"], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0 and "chunked ok: passes winograd4=2 winograd=3" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["winograd4", "winograd"])
def test_rowbias_rows_that_cut_through_images(eng, algo):
    """rows_per_sample = 20 on 5x6 maps: a rowbias row ends inside an image and inside a tile (the per-pixel form of the output
    transform; the graph only ever passes whole images per sample)."""
    n, c, cout, h, w, rps = 2, 32, 64, 5, 6, 20
    x, wt, b = rnd(n, c, h, w, seed=1), rnd(cout, c, 3, 3, seed=2, scale=0.1), rnd(cout, seed=3)
    temb, res = rnd(n * h * w // rps, cout, seed=4), rnd(n, cout, h, w, seed=5)
    ref = to_cl(F.conv2d(x, wt, b, padding=1) + res) + temb.repeat_interleave(rps, 0)
    eng.set_conv_algo(algo)
    try:
        y = eng.op_conv3x3(to_cl(x).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=h, Ws=w, rowbias=temb.cuda().contiguous(),
                           rows_per_sample=rps, resid=to_cl(res).cuda())
    finally:
        eng.set_conv_algo("auto")
    close(y, ref, what=f"{algo} per-pixel rowbias", **BOUNDS[algo])


def test_refuses_a_shape_without_a_winograd_form():
    """Host-only context, no GPU: stride 2 has no Winograd form -> E2V_ESHAPE before any device work; the same call at stride 1 passes
    the shape check and stops at "no GPU" (E2V_ESTATE)."""
    from eeg2video_amd import _lib
    lib = _lib.load()
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    ctx = C.c_void_p()
    assert lib.e2v_create(C.byref(cfg), -1, C.byref(ctx)) == _lib.E2V_OK
    try:
        p = 0x1000                            # never dereferenced on these paths

        def call(stride, ho, wo, c0=32):
            return lib.e2v_op_conv3x3_gn(ctx, p, c0, None, 0, 2, 9, 12, 9, 12, ho, wo, stride, 1, 9 * 12, 32, 1e-5, p, p, p, p, 64, None, 1,
                                         None, p, None)

        for algo in (3, 2):                   # winograd4, winograd
            assert lib.e2v_set_conv_algo(ctx, algo) == _lib.E2V_OK
            assert call(2, 5, 6) == _lib.E2V_ESHAPE
            assert b"Winograd" in lib.e2v_last_error(ctx)
            assert call(1, 9, 12) == _lib.E2V_ESTATE
        assert lib.e2v_set_conv_algo(ctx, 1) == _lib.E2V_OK          # direct: no Winograd form anywhere
        assert call(1, 9, 12) == _lib.E2V_ESHAPE
        assert call(1, 9, 12, c0=30) == _lib.E2V_EINVAL              # channels not a multiple of 4
    finally:
        lib.e2v_destroy(ctx)


if __name__ == "__main__" and sys.argv[1:] == ["chunked"]:
    sys.path.insert(0, ROOT)
    assert os.environ.get("E2V_WINO_WS_MB") == "1"
    engine = make_engine()
    passes = {algorithm: conv_launches(engine, algorithm) for algorithm in ("winograd4", "winograd")}
    print("chunked ok: passes " + " ".join(f"{k}={v}" for k, v in passes.items()))
