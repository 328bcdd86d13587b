"""GPU: bounds tests.  The parity tests look only at the ``rows x C`` floats a kernel was supposed to produce; these look at everything else.

Part A (fp32 mode, ``e2v_op_*``): every operand and the result of an op lies in the middle of a device buffer filled with the poison
``0x7FC07FC0`` (a quiet NaN as fp32; each half, ``0x7FC0``, a NaN as bf16 and as IEEE half), with at least 16 Ki floats of fence on each side
and, where the C ABI takes a row stride, poisoned gap columns between the rows.  After the call: no fence word and no gap column changed
(inputs included), the result holds no NaN (nothing it depends on lay outside the operands, and every element was written), and it meets
the bound of the op's parity test against a float64 reference.

Part B (``E2V_POOL_GUARD``): the same idea inside the library, where the caller cannot look -- workspace-pool blocks, weight layouts and
the GroupNorm workspaces get poisoned guard zones and poisoned payloads; ``e2v_op_pool_guard_report`` says whether a guard changed.  Each
guarded run is repeated unguarded in the same process and must give the same bits.
"""
import contextlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eeg2video_amd.weights import TINY_SEMANTIC, TINY_UNET, TINY_VAE, counter_normal, semantic_param_spec, synth_state_dict
from test_hip_weight_update import BITS, CONV_256, KIND_KEYS, LIN_Q, U0, UPS, V0, draw
from test_hip_wino_transforms import BETA, BOUNDS, CASES, EPS, GROUPS

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2e-5      # tests/test_hip_ops.py: fp32 vs fp32, different summation order
ATTN = dict(rtol=1e-4, atol=1e-5)          # tests/test_hip_ops.py: the attention tests
POISON = 0x7FC07FC0
FENCE = 16 * 1024            # floats on each side of a fenced tensor
PADS = (4, 36)               # row stride = width + pad wherever the ABI takes a stride (multiples of 4 floats)


def make_engine():
    from eeg2video_amd.engine import Engine
    from eeg2video_amd.weights import TINY_UNET, TINY_VAE
    return Engine(TINY_UNET, TINY_VAE, 0)


@pytest.fixture(scope="module")
def eng():
    return make_engine()


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


# ------------------------------------------------------------------ the fence -------------------------------------------------------
class Fenced:
    """A tensor laid out in the middle of one flat, poisoned device buffer.  ``t``: the view to hand to the op -- ``shape`` where the rows
    are contiguous, else the 2-D ``[rows, cols]`` view with row stride ``ld``."""

    def __init__(self, shape, ld=None, values=None, name=""):
        shape = tuple(shape)
        rows = shape[0]
        cols = 1
        for d in shape[1:]:
            cols *= d
        ld = ld or cols
        assert ld >= cols and (ld == cols or len(shape) == 2)
        self.name, self.rows, self.cols, self.ld = name, rows, cols, ld
        self.buf = torch.full((2 * FENCE + rows * ld,), POISON, dtype=torch.int32, device="cuda")
        body = self.buf.view(torch.float32)[FENCE:FENCE + rows * ld].view(rows, ld)
        self.view = body[:, :cols]
        self.values = None
        if values is not None:
            self.values = values.detach().reshape(rows, cols).to(device="cuda", dtype=torch.float32)
            self.view.copy_(self.values)
        self.t = self.view if ld != cols else body.view(shape)
        assert self.t.data_ptr() == self.buf.data_ptr() + 4 * FENCE
        outside = torch.ones(2 * FENCE + rows * ld, dtype=torch.bool, device="cuda")
        outside[FENCE:FENCE + rows * ld].view(rows, ld)[:, :cols] = False
        self.outside = outside

    def check(self):
        """every word outside the tensor's own elements still holds the pattern, bit for bit; an input's own elements are unchanged"""
        bad = (self.outside & (self.buf != POISON)).nonzero().flatten()
        if bad.numel():
            first, last = int(bad[0]) - FENCE, int(bad[-1]) - FENCE
            raise AssertionError(f"{self.name}: {bad.numel()} words outside the tensor changed ([{self.rows}][{self.cols}], row stride "
                                 f"{self.ld}); first at float offset {first} (row {first // self.ld}, column {first % self.ld}) from the "
                                 f"tensor's start, last at {last}")
        if self.values is not None:
            assert torch.equal(self.view.view(torch.int32), self.values.view(torch.int32)), f"{self.name}: the input itself changed"


def fenced(t, ld=None, name="in"):
    return Fenced(t.shape, ld, t, name)


def fenced_out(shape, ld=None):
    return Fenced(shape, ld, None, "out")


def run_fenced(call, ins, out):
    """``call(*views of ins, out=view of out)``; returns the result after the fence and NaN checks"""
    ins = [i for i in ins if i is not None]
    call()
    torch.cuda.synchronize()
    for f in ins + [out]:
        f.check()
    y = out.view.clone()
    assert not torch.isnan(y).any(), f"{int(torch.isnan(y).sum())} NaN in the result: an element was not written, or depends on memory outside the operands"
    return y


def test_fence_detects_a_store_outside_the_tensor():
    """the checker itself: a word of the trailing fence, a gap column and the last word of the leading fence"""
    for where in ("tail", "gap", "head"):
        f = fenced_out((5, 8), ld=12)
        off = {"tail": FENCE + 5 * 12, "gap": FENCE + 12 + 8, "head": FENCE - 1}[where]
        f.buf[off] = 0
        with pytest.raises(AssertionError, match="outside the tensor changed"):
            f.check()
    f = fenced_out((5, 8), ld=12)
    f.view.fill_(1.0)
    f.check()


# ------------------------------------------------------------------ linear ----------------------------------------------------------
LINEAR = [(5, 320, 1280), (77, 64, 128), (130, 40, 72), (133, 64, 70), (257, 128, 129), (40, 320, 3)]


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("m,k,n", LINEAR)
def test_linear_fenced(eng, m, k, n, epilogue, pad):
    x, w = rnd(m, k, seed=20), rnd(n, k, seed=21, scale=0.05)
    b, r = (rnd(n, seed=22), rnd(m, n, seed=23)) if epilogue else (None, None)
    ref = F.linear(x.double(), w.double(), b.double() if epilogue else None) + (r.double() if epilogue else 0)
    fx, fw, out = fenced(x, ld=k + pad, name="x"), fenced(w, name="w"), fenced_out((m, n))
    fb, fr = (fenced(b, name="bias"), fenced(r, name="resid")) if epilogue else (None, None)
    y = run_fenced(lambda: eng.op_linear(fx.t, fw.t, fb.t if fb else None, fr.t if fr else None, out=out.t), [fx, fw, fb, fr], out)
    close(y, ref, what=f"linear {m}x{k}x{n}")


@pytest.mark.parametrize("pad", PADS)
def test_linear_geglu_fenced(eng, pad):
    m, c = 300, 64
    x, w, b = rnd(m, c, seed=24), rnd(8 * c, c, seed=25, scale=0.1), rnd(8 * c, seed=26)
    h, g = F.linear(x.double(), w.double(), b.double()).chunk(2, dim=-1)
    fx, fw, fb, out = fenced(x, ld=c + pad, name="x"), fenced(w, name="w"), fenced(b, name="bias"), fenced_out((m, 4 * c))
    y = run_fenced(lambda: eng.op_linear(fx.t, fw.t, fb.t, geglu=True, out=out.t), [fx, fw, fb], out)
    close(y, h * F.gelu(g), what="geglu")


# ------------------------------------------------------------------ conv3x3 ---------------------------------------------------------
def conv_fenced(eng, x, wt, b, *, x1=None, stride=1, pad_lo=1, pad_hi=1, hi=None, wi=None, temb=None, f=1, res=None, what="", **tol):
    """x (and x1, concatenated on channels): [n, c, hs, ws]; temb: [n / f, cout] rows of the time embedding; res: [n, cout, ho, wo]"""
    n, _, hs, ws = x.shape
    hi, wi = hi or hs, wi or ws
    src = (torch.cat([x, x1], 1) if x1 is not None else x).double()
    if (hi, wi) != (hs, ws):
        src = F.interpolate(src, size=(hi, wi), mode="nearest")
    ref = F.conv2d(F.pad(src, (pad_lo, pad_hi, pad_lo, pad_hi)), wt.double(), b.double(), stride=stride)
    ho, wo = ref.shape[2], ref.shape[3]
    if temb is not None:
        ref = ref + temb.double().repeat_interleave(f, 0)[:, :, None, None]
    if res is not None:
        ref = ref + res.double()
    fx, fw, fb = fenced(to_cl(x), name="x0"), fenced(wt, name="w"), fenced(b, name="bias")
    f1 = fenced(to_cl(x1), name="x1") if x1 is not None else None
    ft = fenced(temb, name="rowbias") if temb is not None else None
    fr = fenced(to_cl(res), name="resid") if res is not None else None
    out = fenced_out((n * ho * wo, wt.shape[0]))
    y = run_fenced(lambda: eng.op_conv3x3(fx.t, fw.t, fb.t, f1.t if f1 else None, n_img=n, Hs=hs, Ws=ws, Hi=hi, Wi=wi, stride=stride,
                                          pad_lo=pad_lo, pad_hi=pad_hi, rowbias=ft.t if ft else None, rows_per_sample=f * ho * wo,
                                          resid=fr.t if fr else None, out=out.t), [fx, fw, fb, f1, ft, fr], out)
    close(from_cl(y, n, ho, wo), ref, what=what, **tol)


def concat_case():
    n_s, f, c0, c1, cout, h, w = 2, 3, 64, 32, 64, 5, 6
    n = n_s * f
    return dict(x=rnd(n, c0, h, w, seed=11), x1=rnd(n, c1, h, w, seed=12), wt=rnd(cout, c0 + c1, 3, 3, seed=13, scale=0.1),
                b=rnd(cout, seed=14), temb=rnd(n_s, cout, seed=15), res=rnd(n, cout, h, w, seed=16), f=f)


PLAIN = [(4, 64, 3, 9, 12), (64, 4, 2, 7, 5), (32, 64, 2, 5, 8)]
RESIZE = [(2, 2, 3, 3), (5, 6, 12, 7), (5, 8, 9, 16)]


@pytest.mark.parametrize("cin,cout,n,h,w", PLAIN)
def test_conv3x3_direct_plain_fenced(eng, cin, cout, n, h, w):
    conv_fenced(eng, rnd(n, cin, h, w, seed=1), rnd(cout, cin, 3, 3, seed=2, scale=0.1), rnd(cout, seed=3), what="direct")


@pytest.mark.parametrize("h,pad_lo,pad_hi", [(9, 1, 1), (8, 0, 1)])
def test_conv3x3_direct_stride2_fenced(eng, h, pad_lo, pad_hi):
    conv_fenced(eng, rnd(2, 32, h, 12, seed=4), rnd(64, 32, 3, 3, seed=5, scale=0.1), rnd(64, seed=6), stride=2, pad_lo=pad_lo,
                pad_hi=pad_hi, what="stride 2")


@pytest.mark.parametrize("hs,ws,hi,wi", RESIZE)
def test_conv3x3_direct_resize_fenced(eng, hs, ws, hi, wi):
    conv_fenced(eng, rnd(3, 32, hs, ws, seed=8), rnd(64, 32, 3, 3, seed=9, scale=0.1), rnd(64, seed=10), hi=hi, wi=wi, what="resize")


def test_conv3x3_direct_concat_rowbias_residual_fenced(eng):
    conv_fenced(eng, what="concat", **concat_case())


@pytest.fixture(params=["winograd", "winograd4"])
def wino(eng, request):
    eng.set_conv_algo(request.param)
    yield eng, request.param
    eng.set_conv_algo("auto")


@pytest.mark.parametrize("cin,cout,n,h,w", PLAIN + [(64, 32, 2, 1, 1), (32, 32, 1, 2, 3), (32, 32, 1, 4, 4)])
def test_conv3x3_winograd_fenced(wino, cin, cout, n, h, w):
    e, algo = wino
    conv_fenced(e, rnd(n, cin, h, w, seed=1), rnd(cout, cin, 3, 3, seed=2, scale=0.1), rnd(cout, seed=3), what=algo, **BOUNDS[algo])


def test_conv3x3_winograd_resize_and_concat_fenced(wino):
    e, algo = wino
    conv_fenced(e, rnd(3, 32, 5, 6, seed=8), rnd(64, 32, 3, 3, seed=9, scale=0.1), rnd(64, seed=10), hi=12, wi=7, what=algo + " resize",
                **BOUNDS[algo])
    conv_fenced(e, what=algo + " concat", **BOUNDS[algo], **concat_case())


def conv_gn_fenced(eng, algo, n_s, f, c0, c1, cout, hs, ws, hi=None, wi=None, epilogue=False):
    """GroupNorm + SiLU + conv in the transforms (tests/test_hip_wino_transforms.py: check_case), operands fenced, torch in float64"""
    hi, wi = hi or hs, wi or ws
    n, c = n_s * f, c0 + c1
    x = rnd(n, c, hs, ws, seed=1) * 1.5 + 0.3
    ga, be = rnd(c, seed=2) * 0.2 + 1.0, rnd(c, seed=3) * 0.2 + BETA
    wt, b = rnd(cout, c, 3, 3, seed=4, scale=0.1), rnd(cout, seed=5)
    temb, res = (rnd(n_s, cout, seed=6), rnd(n, cout, hi, wi, seed=7)) if epilogue else (None, None)
    x5 = x.double().reshape(n_s, f, c, hs, ws).permute(0, 2, 1, 3, 4)
    act = F.silu(F.group_norm(x5, GROUPS, ga.double(), be.double(), EPS)).permute(0, 2, 1, 3, 4).reshape(n, c, hs, ws)
    if (hi, wi) != (hs, ws):
        act = F.interpolate(act, size=(hi, wi), mode="nearest")
    ref = F.conv2d(act, wt.double(), b.double(), padding=1)
    if epilogue:
        ref = ref + temb.double().repeat_interleave(f, 0)[:, :, None, None] + res.double()
    fx, fg, fbe, fw, fb = (fenced(to_cl(x[:, :c0]), name="x0"), fenced(ga, name="gamma"), fenced(be, name="beta"), fenced(wt, name="w"),
                           fenced(b, name="bias"))
    f1 = fenced(to_cl(x[:, c0:]), name="x1") if c1 else None
    ft, fr = (fenced(temb, name="rowbias"), fenced(to_cl(res), name="resid")) if epilogue else (None, None)
    out = fenced_out((n * hi * wi, cout))
    epi = dict(rowbias=ft.t, rows_per_sample=f * hi * wi, resid=fr.t) if epilogue else {}
    eng.set_conv_algo(algo)
    try:
        y = run_fenced(lambda: eng.op_conv3x3_gn(fx.t, fg.t, fbe.t, fw.t, fb.t, x1=f1.t if f1 else None, n_img=n, Hs=hs, Ws=ws, Hi=hi,
                                                 Wi=wi, gn_P=f * hs * ws, groups=GROUPS, eps=EPS, out=out.t, **epi),
                       [fx, fg, fbe, fw, fb, f1, ft, fr], out)
    finally:
        eng.set_conv_algo("auto")
    close(from_cl(y, n, hi, wi), ref, what=f"{algo} GroupNorm + SiLU + conv", **BOUNDS[algo])


@pytest.mark.parametrize("algo", ["winograd4", "winograd"])
@pytest.mark.parametrize("case", list(CASES))
def test_conv3x3_gn_fenced(eng, algo, case):
    conv_gn_fenced(eng, algo, **CASES[case])


@pytest.mark.parametrize("algo", ["winograd4", "winograd"])
def test_conv3x3_winograd_chunked_fenced(monkeypatch, algo):
    """A 1 MB workspace cap (E2V_WINO_WS_MB, read when the context is created) splits the images of a call into several passes
    (tests/test_hip_wino_transforms.py: test_image_chunks_reach_the_groupnorm_slab_index): the later passes start inside the tensors."""
    monkeypatch.setenv("E2V_WINO_WS_MB", "1")
    e = make_engine()
    e.profile_begin()
    conv_gn_fenced(e, algo, **CASES["9x16_concat_temb_resid"])
    assert e.profile_end()["wino_in_gn_silu"]["launches"] == {"winograd4": 2, "winograd": 3}[algo]
    e.set_conv_algo(algo)
    conv_fenced(e, what=algo + " concat, chunked", **BOUNDS[algo], **concat_case())
    conv_fenced(e, rnd(6, 64, 9, 16, seed=1), rnd(64, 64, 3, 3, seed=2, scale=0.1), rnd(64, seed=3), what=algo + " 9x16, chunked",
                **BOUNDS[algo])


# ------------------------------------------------------------------ norms -----------------------------------------------------------
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("c,groups,n,f,hw", [(64, 32, 3, 3, 300), (128, 8, 2, 1, 600)])
def test_groupnorm_fenced(eng, c, groups, n, f, hw, silu):
    x = rnd(n, c, f, hw, 1, seed=30) * 2.0 + 0.7
    ga, be = rnd(c, seed=31) * 0.2 + 1.0, rnd(c, seed=32) * 0.2
    ref = F.group_norm(x.double(), groups, ga.double(), be.double(), 1e-5)
    ref = F.silu(ref) if silu else ref
    xcl = x.permute(0, 2, 3, 4, 1).reshape(n * f * hw, c).contiguous()
    fx, fg, fb, out = fenced(xcl, name="x"), fenced(ga, name="gamma"), fenced(be, name="beta"), fenced_out((n * f * hw, c))
    y = run_fenced(lambda: eng.op_groupnorm(fx.t, fg.t, fb.t, samples=n, P=f * hw, groups=groups, eps=1e-5, silu=silu, out=out.t),
                   [fx, fg, fb], out)
    close(y.reshape(n, f, hw, 1, c).permute(0, 4, 1, 2, 3), ref, what="groupnorm")


@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_seam_fenced(eng, silu):
    n, c0, c1, p = 2, 64, 32, 500
    a, s = rnd(n, c0, p, 1, seed=33), rnd(n, c1, p, 1, seed=34) * 3 - 1
    ga, be = rnd(c0 + c1, seed=35) * 0.2 + 1.0, rnd(c0 + c1, seed=36) * 0.2
    ref = F.group_norm(torch.cat([a, s], 1).double(), 32, ga.double(), be.double(), 1e-5)
    ref = F.silu(ref) if silu else ref
    cl = lambda t: t.permute(0, 2, 3, 1).reshape(n * p, -1).contiguous()
    f0, f1, fg, fb, out = fenced(cl(a), name="x0"), fenced(cl(s), name="x1"), fenced(ga, name="gamma"), fenced(be, name="beta"), fenced_out((n * p, c0 + c1))
    y = run_fenced(lambda: eng.op_groupnorm(f0.t, fg.t, fb.t, samples=n, P=p, groups=32, eps=1e-5, silu=silu, x1=f1.t, out=out.t),
                   [f0, f1, fg, fb], out)
    close(y.reshape(n, p, 1, c0 + c1).permute(0, 3, 1, 2), ref, what="groupnorm over the seam")


@pytest.mark.parametrize("ln_rows", [1, 0])
@pytest.mark.parametrize("c", [64, 320, 1280])
def test_layernorm_fenced(eng, c, ln_rows):
    x, g, b = rnd(777, c, seed=40) * 3 + 1, rnd(c, seed=41) * 0.2 + 1, rnd(c, seed=42) * 0.2
    ref = F.layer_norm(x.double(), (c,), g.double(), b.double(), 1e-5)
    fg, fb = fenced(g, name="gamma"), fenced(b, name="beta")
    try:
        eng.set_knob("E2V_LN_ROWS", ln_rows)
        for rows in (1, 3, 9, 777):
            fx, out = fenced(x[:rows].contiguous(), name="x"), fenced_out((rows, c))
            y = run_fenced(lambda: eng.op_layernorm(fx.t, fg.t, fb.t, out=out.t), [fx, fg, fb], out)
            close(y, ref[:rows], what=f"layernorm {rows} x {c}")
    finally:
        eng.set_knob("E2V_LN_ROWS", 1)


# ------------------------------------------------------------------ attention -------------------------------------------------------
def attn64(q, k, v, scale):        # [b, s, d] each, float64
    return torch.bmm((torch.bmm(q, k.transpose(1, 2)) * scale).softmax(-1), v)


def heads_of(x, h):                # [b, s, h*d] -> [b*h, s, d]
    b, s, c = x.shape
    return x.reshape(b, s, h, c // h).permute(0, 2, 1, 3).reshape(b * h, s, c // h)


def unheads(x, h):
    bh, s, d = x.shape
    return x.reshape(bh // h, h, s, d).permute(0, 2, 1, 3).reshape(bh // h, s, h * d)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("d,nq,f,n", [(8, 108, 3, 2), (32, 9, 3, 2), (40, 200, 6, 1), (64, 70, 2, 1), (80, 144, 3, 1), (160, 40, 6, 2)])
def test_sparse_causal_attention_fenced(eng, d, nq, f, n, pad):
    heads = 8 if d != 160 else 4
    c = heads * d
    qkv = rnd(n * f * nq, 3 * c, seed=50)
    q, k, v = (qkv[:, i * c:(i + 1) * c].double().reshape(n * f, nq, c) for i in range(3))
    former = torch.arange(f) - 1
    former[0] = 0
    gather = lambda t: torch.cat([t.reshape(n, f, nq, c)[:, [0] * f], t.reshape(n, f, nq, c)[:, former]], dim=2).reshape(n * f, 2 * nq, c)
    ref = unheads(attn64(heads_of(q, heads), heads_of(gather(k), heads), heads_of(gather(v), heads), d ** -0.5), heads)
    fq, out = fenced(qkv, ld=3 * c + pad, name="qkv"), fenced_out((n * f * nq, c), ld=c + pad)
    g = fq.t
    y = run_fenced(lambda: eng.op_attention(g[:, :c], g[:, c:2 * c], g[:, 2 * c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nq, mode=0,
                                            scale=d ** -0.5, out=out.t), [fq], out)
    close(y.reshape(n * f, nq, c), ref, what="sparse-causal attention", **ATTN)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("d,nq,nk", [(8, 108, 11), (40, 300, 77), (160, 40, 77)])
def test_cross_attention_fenced(eng, d, nq, nk, pad):
    heads, n, f = 8, 2, 3
    c = heads * d
    q, kv = rnd(n * f * nq, c, seed=51), rnd(n * nk, 2 * c, seed=52)
    k, v = kv[:, :c].double().reshape(n, nk, c), kv[:, c:].double().reshape(n, nk, c)
    rep = lambda t: t.repeat_interleave(f, 0)
    ref = unheads(attn64(heads_of(q.double().reshape(n * f, nq, c), heads), heads_of(rep(k), heads), heads_of(rep(v), heads), d ** -0.5), heads)
    fq, fkv, out = fenced(q, ld=c + pad, name="q"), fenced(kv, ld=2 * c + pad, name="kv"), fenced_out((n * f * nq, c), ld=c + pad)
    y = run_fenced(lambda: eng.op_attention(fq.t, fkv.t[:, :c], fkv.t[:, c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nk, mode=1,
                                            scale=d ** -0.5, out=out.t), [fq, fkv], out)
    close(y.reshape(n * f, nq, c), ref, what="cross-attention", **ATTN)


def temporal64(qkv, n, f, hw, heads, d):
    c = heads * d
    t = qkv.double().reshape(n, f, hw, 3 * c).permute(0, 2, 1, 3).reshape(n * hw, f, 3 * c)
    ref = unheads(attn64(heads_of(t[..., :c], heads), heads_of(t[..., c:2 * c], heads), heads_of(t[..., 2 * c:], heads), d ** -0.5), heads)
    return ref.reshape(n, hw, f, c).permute(0, 2, 1, 3).reshape(n * f * hw, c)


def temporal_fenced(eng, d, f, hw, seed, **tol):
    heads, n = 8, 2
    qkv = rnd(n * f * hw, 3 * heads * d, seed=seed)
    fq, out = fenced(qkv, name="qkv"), fenced_out((n * f * hw, heads * d))
    y = run_fenced(lambda: eng.op_temporal_attention(fq.t, n=n, F=f, HW=hw, heads=heads, D=d, scale=d ** -0.5, out=out.t), [fq], out)
    close(y, temporal64(qkv, n, f, hw, heads, d), what=f"temporal attention d={d} f={f}", **tol)


@pytest.mark.parametrize("wave", [1, 0])
@pytest.mark.parametrize("d,f,hw", [(8, 3, 50), (40, 6, 33), (160, 6, 7)])
def test_temporal_attention_fenced(eng, d, f, hw, wave):
    try:
        eng.set_knob("E2V_TATTN_WAVE", wave)
        temporal_fenced(eng, d, f, hw, 54, **ATTN)
    finally:
        eng.set_knob("E2V_TATTN_WAVE", 1)


@pytest.mark.parametrize("d", [8, 40, 160])
@pytest.mark.parametrize("f", [9, 17, 33])
def test_long_temporal_attention_fenced(eng, d, f):
    temporal_fenced(eng, d, f, 7, 300 + f, rtol=1e-4, atol=1e-4)          # tests/test_hip_long_clips.py: TOL["fp32"]


# ------------------------------------------------------------------ layout conversion, row-block sums --------------------------------
@pytest.mark.parametrize("c,cpad", [(4, 4), (4, 32), (5, 8)])
def test_to_channels_last_fenced(eng, c, cpad):
    n, fhw = 2, 3 * 5 * 7
    x = rnd(n, c, fhw, seed=90)
    ref = torch.zeros(n, fhw, cpad)
    ref[:, :, :c] = x.permute(0, 2, 1)
    fx, out = fenced(x, name="x"), fenced_out((n * fhw, cpad))
    y = run_fenced(lambda: eng.op_to_channels_last(fx.t, Cpad=cpad, out=out.t), [fx], out)
    assert torch.equal(y.cpu(), ref.reshape(n * fhw, cpad))


@pytest.mark.parametrize("c,ld", [(4, 4), (4, 32), (5, 5), (5, 33), (5, 8)])
def test_from_channels_last_fenced(eng, c, ld):
    """ld in {C, C + 28}, and the padded row of to_channels_last (5 channels in rows of 8); the kernel reads single floats"""
    n, fhw = 2, 3 * 5 * 7
    x = rnd(n * fhw, c, seed=91)
    fx, out = fenced(x, ld=ld, name="x"), fenced_out((n, c, fhw))
    y = run_fenced(lambda: eng.op_from_channels_last(fx.t, n=n, C=c, out=out.t), [fx], out)
    assert torch.equal(y.cpu().reshape(n, c, fhw), x.reshape(n, fhw, c).permute(0, 2, 1))


def test_rowblock_sums_fenced(eng):
    c, rows = 64, 128
    x = rnd(rows, c, seed=300) * 3.0 + 0.5
    xb = x.to(torch.bfloat16).double().reshape(rows // 64, 64, c)
    ref = torch.stack([xb.sum(1), (xb * xb).sum(1)], dim=-1)
    fx, out = fenced(x, name="x"), fenced_out((rows // 64, c, 2))
    y = run_fenced(lambda: eng.op_rowblock_sums(fx.t, out=out.t), [fx], out).cpu().double().reshape(ref.shape)
    assert (y - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()


# =====================================================================================================================================
# Part B: the guarded workspace pool (E2V_POOL_GUARD)
# =====================================================================================================================================
GUARD_KIB = 64
H16_TYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
UNET_BOUND = {"fp32": 1e-4, "f32x3": 1e-4, "bf16": 5e-2, "fp16": 5e-3}      # tests/test_hip_model.py: max abs / max |oracle|, tiny UNet
# the tiny VAE has no 16-bit test of its own: the bound of the tiny UNet in the same mode (no more layers, the same roundings per layer)
VAE_BOUND = UNET_BOUND
KNOB_DEFAULTS = {"E2V_BGEMM_T256": 1, "E2V_BGEMM_UP2X": 1, "E2V_SPLITK_FORCE": 0, "E2V_ATTN_Q64": 1, "E2V_ATTN_CROSS_RESIDENT": 1,
                 "E2V_GN_FUSED_SMALL": 1, "E2V_LN_ROWS": 1, "E2V_SMALL_FAMILY_CLIPS": 4, "E2V_GN_COOP": 0}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def set_guard(kib):
    from eeg2video_amd import _lib
    assert _lib.load().e2v_op_set_knob(b"E2V_POOL_GUARD", int(kib)) == 0


@contextlib.contextmanager
def settings(eng, mode="fp32", knobs=None, guard=0):
    """arithmetic mode, run-time switches and the guard switch for one run; everything back to its default afterwards"""
    knobs = knobs or {}
    try:
        set_guard(guard)
        if mode in ("fp32", "bf16", "fp16"):                  # (f32x3 is chosen when the engine is built)
            eng.set_compute_dtype(mode)
        for k, v in knobs.items():
            eng.set_knob(k, v)
        yield
        torch.cuda.synchronize()
    finally:
        set_guard(0)
        for k in knobs:
            eng.set_knob(k, KNOB_DEFAULTS[k])
        if mode in ("fp32", "bf16", "fp16"):
            eng.set_compute_dtype("fp32")


@contextlib.contextmanager
def environment(env, guard):
    """what an engine reads when it is created"""
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        set_guard(guard)
        yield
    finally:
        set_guard(0)
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def tensors(y):
    return list(y) if isinstance(y, (tuple, list)) else [y]


def same_bits(a, b):
    return all(x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
               for x, y in zip(tensors(a), tensors(b)))


def guarded_run(pair, run, mode="fp32", knobs=None, what=""):
    """``pair``: (engine built with the switch off, engine built with it on).  The call runs twice unguarded (deterministic?), once
    guarded; the guarded run reports no violation, checked at least as many blocks as the unguarded call took from the pool -- over and
    above the blocks every report compares anyway (weight layouts, GroupNorm workspaces, pool blocks the engine keeps): the count of a
    report with no work before it --, holds no NaN and equals the unguarded run bit for bit.  Returns the guarded result for the caller's comparison with the oracle."""
    off, on = pair
    with settings(off, mode, knobs, 0):
        before = off.pool_gets()
        y0 = run(off)
        taken = off.pool_gets() - before
        y0b = run(off)
    assert same_bits(y0, y0b), f"{what}: two unguarded runs differ"
    with settings(on, mode, knobs, GUARD_KIB):
        on.pool_guard_report()                              # (the totals start here; what building the engine did was reported there)
        standing = on.pool_guard_report()[0]                # no work since the last report: the blocks that are compared every time
        y1 = run(on)
        checked, violations, text = on.pool_guard_report()
    print(f"{what}: {checked} blocks checked, {standing} of them standing ({taken} pool tensors per unguarded call), {violations} violations")
    assert violations == 0, f"{what}: {text}"
    assert checked > 0 and checked - standing >= taken, (checked, standing, taken)
    for t in tensors(y1):
        assert not torch.isnan(t).any(), f"{what}: {int(torch.isnan(t).sum())} NaN under guard"
    assert same_bits(y1, y0), f"{what}: the guarded run differs from the unguarded one, max |diff| " \
                              f"{max((a.double() - b.double()).abs().max().item() for a, b in zip(tensors(y1), tensors(y0))):.3e}"
    return y1


# ------------------------------------------------------------------ the detector's own test -----------------------------------------
def test_pool_guard_detector_selftest():
    """One word of a block's trailing guard zone is set from the host (an address inside the pool's own allocation): the report shows
    exactly that zone, at that offset, and the next report is clean.  The only place a guard is touched on purpose."""
    with environment({}, GUARD_KIB):
        e = make_engine()
        assert e.pool_guard_report()[1] == 0
        e.pool_guard_selftest(1000 * 4, 4 * 37)
        checked, violations, text = e.pool_guard_report()
        assert violations == 1 and checked >= 1, text
        assert "pool block, payload 4000 bytes: trailing guard altered, first at byte offset 148" in text, text
        assert e.pool_guard_report()[1:] == (0, "")
        x = rnd(77, 64, seed=1).cuda()                      # 16-bit payloads: the zones are compared in 16-bit units
        e.set_compute_dtype("bf16")
        e.op_layernorm(x, torch.ones(64).cuda(), torch.zeros(64).cuda())
        checked, violations, text = e.pool_guard_report()
        assert checked >= 2 and violations == 0, text
    with pytest.raises(RuntimeError):                       # switch off: E2V_ESTATE
        e.pool_guard_selftest(4000, 0)


def test_pool_guard_report_on_a_host_only_context():
    import ctypes as C
    from eeg2video_amd import _lib
    lib = _lib.load()
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    ctx = C.c_void_p()
    assert lib.e2v_create(C.byref(cfg), -1, C.byref(ctx)) == _lib.E2V_OK
    try:
        a, b = C.c_int64(0), C.c_int64(0)
        assert lib.e2v_op_pool_guard_report(ctx, C.byref(a), C.byref(b), None, 0) == _lib.E2V_ESTATE
    finally:
        lib.e2v_destroy(ctx)


# ------------------------------------------------------------------ tiny models ------------------------------------------------------
_pipes, _oracle = {}, {}                                   # (U0 / V0: the 'perturbed' tiny state dicts of seeds 42 / 43, as everywhere)


def build_pipe(usd=U0, vsd=V0):
    from eeg2video_amd.pipeline import build_pipeline
    pipe = build_pipeline(TINY_UNET, TINY_VAE, device=0, unet_sd=usd, vae_sd=vsd)
    pipe.set_progress_bar_config(disable=True)
    return pipe


def fresh_pipes(env=None, usd=U0, vsd=V0):
    """(pipeline built with the switch off, pipeline built with it on -- weight layouts guarded, their builders reported clean)"""
    with environment(env or {}, 0):
        off = build_pipe(usd, vsd)
    with environment(env or {}, GUARD_KIB):
        on = build_pipe(usd, vsd)
        checked, violations, text = on.unet.engine.pool_guard_report()
    assert violations == 0 and checked > 0, text
    return off, on


def pipes(**env):
    key = tuple(sorted(env.items()))
    if key not in _pipes:
        _pipes[key] = fresh_pipes(env)
    return _pipes[key]


def engines(pp):
    return pp[0].unet.engine, pp[1].unet.engine


def by_engine(pp):
    return {id(p.unet.engine): p for p in pp}


def oracle(key, fn):
    if key not in _oracle:
        _oracle[key] = fn()
    return _oracle[key]


def sd_t(sd):
    return {k: _t(v) for k, v in sd.items()}


UNET_SHAPES = [((2, 4, 3, 9, 12), 11), ((3, 4, 2, 5, 7), 5), ((1, 4, 9, 5, 7), 5)]
UNET_CONFIGS = [("fp32", {}, {}), ("bf16", {}, {}), ("fp16", {}, {}), ("f32x3", {"E2V_F32X3": "1"}, {}),
                ("fp32", {"E2V_CONV_ALGO": "1"}, {}), ("fp32", {"E2V_CONV_ALGO": "2"}, {}), ("fp32", {"E2V_CONV_ALGO": "3"}, {}),
                ("bf16", {}, {"E2V_SMALL_FAMILY_CLIPS": 0}), ("fp16", {}, {"E2V_SMALL_FAMILY_CLIPS": 0})]


@pytest.mark.parametrize("mode,env,knobs", UNET_CONFIGS, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else v)
@pytest.mark.parametrize("shape,tokens", UNET_SHAPES)
def test_tiny_unet_forward_guarded(shape, tokens, mode, env, knobs):
    from oracle import unet3d_forward
    pp = pipes(**env)
    who = by_engine(pp)
    x = _t(counter_normal(5, "x", shape))
    cond = _t(counter_normal(6, "c", (shape[0], tokens, TINY_UNET.cross_attention_dim)))
    ref = oracle(("unet", shape, tokens), lambda: unet3d_forward(sd_t(U0), TINY_UNET, x, 301, cond))
    gx, gc = x.cuda(), cond.cuda()
    y = guarded_run(engines(pp), lambda e: who[id(e)].unet(gx, 301, gc, return_dict=False)[0].float(), mode, knobs, f"UNet {shape} {mode}")
    e = rel_err(y, ref)
    print(f"UNet {shape} {mode} {env} {knobs}: max abs / max ref {e:.3e}")
    assert y.shape == ref.shape and e < UNET_BOUND[mode]


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_tiny_vae_guarded(mode):
    """decode and encode, whole graphs (the batched strided GEMMs, softmax_rows and transpose2d of the VAE's attention on their own:
    tests/test_hip_vae_attention.py)"""
    from oracle import vae_decode, vae_encode
    pp = pipes()
    who = by_engine(pp)
    for n, h, w in [(3, 6, 4), (2, 4, 6)]:
        z = _t(counter_normal(10, "z", (n, 4, h, w)))
        ref = oracle(("dec", n, h, w), lambda: vae_decode(sd_t(V0), TINY_VAE, z))
        gz = z.cuda()
        y = guarded_run(engines(pp), lambda e: who[id(e)].vae.decode(gz).sample.float(), mode, None, f"VAE decode {n}x{h}x{w} {mode}")
        print(f"VAE decode {mode}: {rel_err(y, ref):.3e}")
        assert y.shape == ref.shape and rel_err(y, ref) < VAE_BOUND[mode]
    img = _t(counter_normal(11, "img", (2, 3, 32, 48)))
    mean, logvar = oracle("enc", lambda: vae_encode(sd_t(V0), TINY_VAE, img))
    gi = img.cuda()
    m, lv = guarded_run(engines(pp), lambda e: e.vae_encode(gi), mode, None, f"VAE encode {mode}")
    print(f"VAE encode {mode}: {rel_err(m, mean):.3e} {rel_err(lv, logvar):.3e}")
    assert rel_err(m, mean) < VAE_BOUND[mode] and rel_err(lv, logvar) < VAE_BOUND[mode]


def test_tiny_generate_and_inversion_guarded():
    """two guided steps + decode (the kv / temb step caches, the scheduler kernels), and one step of DDIM inversion"""
    from oracle import DDIMOracle, ddim_loop, generate, unet3d_forward
    pp = pipes()
    d = TINY_UNET.cross_attention_dim
    lat = _t(counter_normal(1, "lat", (1, 4, 3, 8, 12)))
    cond, unc = _t(counter_normal(2, "cond", (1, 7, d))), _t(counter_normal(3, "unc", (1, 7, d)))
    gl, gc, gu = lat.cuda(), cond.cuda(), unc.cuda()
    vid, lat_out = guarded_run(engines(pp), lambda e: e.generate(gl, gc, gu, 2, 12.5, 0.0, decode=True, return_latents=True), what="generate")
    trace = {}
    ref = generate(sd_t(U0), TINY_UNET, sd_t(V0), TINY_VAE, lat, cond, unc, 2, 12.5, trace=trace)
    assert rel_err(lat_out, trace["latents"][-1]) < 1e-3                                   # tests/test_hip_model.py: test_generate_vs_oracle_end_to_end
    assert vid.shape == ref.shape and (vid.cpu() - ref).abs().max().item() < 1e-3          # __graft_entry__.smoke, tests/test_hip_model.py
    x = _t(counter_normal(31, "x", (2, 4, 3, 9, 12)))
    c = _t(counter_normal(32, "c", (1, 11, d)))
    so = DDIMOracle()
    so.set_timesteps(1)
    want = ddim_loop(lambda l, t, cc: unet3d_forward(sd_t(U0), TINY_UNET, l, t, cc), so, x, 1, c)
    gx, gcc = x.cuda(), c.repeat(2, 1, 1).cuda()
    got = guarded_run(engines(pp), lambda e: e.ddim_invert(gx, gcc, 1, return_all=True), what="DDIM inversion")
    assert len(got) == 2
    for a, r in zip(got, want):
        assert rel_err(a, r) < 1e-4


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_semantic_predictor_guarded(mode):
    """B = 1, 16 (the last batch gemv_rows takes), 17 (the first the GEMM takes) and 130"""
    from eeg2video_amd.engine import Engine
    from eeg2video_amd.semantic import CLIP
    from oracle import semantic_predictor
    sd = synth_state_dict(semantic_param_spec(TINY_SEMANTIC, TINY_UNET.cross_attention_dim), seed=44, mode="perturbed")
    models = {}
    for kib in (0, GUARD_KIB):
        with environment({}, kib):
            e = Engine(TINY_UNET, TINY_VAE, 0, sem_cfg=TINY_SEMANTIC)
            models[id(e)] = CLIP(TINY_SEMANTIC, engine=e).load_state_dict({"state_dict": sd})
            if kib:
                assert e.pool_guard_report()[1] == 0
    pair = tuple(m.engine for m in models.values())
    for batch in (1, 16, 17, 130):
        eeg = _t(counter_normal(3, "eeg", (batch, TINY_SEMANTIC.in_features)))
        ref = semantic_predictor(sd_t(sd), eeg)
        g = eeg.cuda()
        out = guarded_run(pair, lambda e: models[id(e)](g), mode, None, f"semantic predictor B={batch} {mode}")
        err = rel_err(out, ref)
        print(f"semantic predictor B={batch} {mode}: {err:.3e}")
        assert err < (1e-5 if mode == "fp32" else 5e-2)      # tests/test_hip_extras.py


# ------------------------------------------------------------------ weight updates --------------------------------------------------
X_UPD = dict(x=(2, 4, 3, 9, 12), tokens=11, lat=(2, 4, 3, 8, 8))


def upd_inputs():
    d = TINY_UNET.cross_attention_dim
    return oracle("upd", lambda: dict(
        x=_t(counter_normal(5, "x", X_UPD["x"])).cuda(), cond=_t(counter_normal(6, "c", (2, X_UPD["tokens"], d))).cuda(),
        lat=_t(counter_normal(7, "lat", X_UPD["lat"])).cuda(), gcond=_t(counter_normal(8, "gc", (2, X_UPD["tokens"], d))).cuda(),
        z=_t(counter_normal(11, "z", (1, 4, 2, 4, 6))).cuda(), img=_t(counter_normal(12, "img", (2, 3, 32, 48))).cuda()))


def unet_fwd(pipe, small=False):
    i = upd_inputs()
    return pipe.unet(i["lat"] if small else i["x"], 301, i["gcond"] if small else i["cond"], return_dict=False)[0].float()


def vae_fwd(pipe):
    i = upd_inputs()
    mean, logvar = pipe.vae.engine.vae_encode(i["img"])
    return torch.cat([pipe.vae.engine.vae_decode(i["z"]).flatten(), mean.flatten(), logvar.flatten()])


@pytest.mark.parametrize("group", list(KIND_KEYS))
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_weight_update_guarded(mode, group):
    """e2v_update_tensor scatters into dev_alloc blocks that sit next to other weights: forward (the forms of the mode exist), update
    every key of the group, forward again -- unguarded and guarded, bit-identical, no guard of any weight layout altered, and the
    result is the one a fresh build of the updated state dict gives (tests/test_hip_weight_update.py: test_every_binding_kind)."""
    is_vae = group == "vae"
    fwd = vae_fwd if is_vae else unet_fwd
    new = {k: draw(k, (V0 if is_vae else U0)[k].shape) for k in KIND_KEYS[group]}
    pp = fresh_pipes()
    who = by_engine(pp)

    def run(e):
        p = who[id(e)]
        if not getattr(p, "_updated", False):
            before = fwd(p)
            (p.vae if is_vae else p.unet).sync_from({k: _t(v).cuda() for k, v in new.items()})
            p._updated = True
            assert not torch.equal(fwd(p), before)
        return fwd(p)

    y = guarded_run(engines(pp), run, mode, None, f"update {group} {mode}")
    fresh = build_pipe(U0, dict(V0, **new)) if is_vae else build_pipe(dict(U0, **new), V0)
    with settings(fresh.unet.engine, mode):
        ref = fwd(fresh)
    assert torch.isfinite(y).all() and torch.equal(y, ref)


@pytest.mark.parametrize("mode,algo", [("fp32", "direct"), ("fp32", "winograd"), ("fp32", "winograd4"), ("f32x3", "winograd"),
                                       ("f32x3", "winograd4"), ("bf16", None), ("fp16", None)])
def test_conv_form_update_guarded(mode, algo):
    """tests/test_hip_weight_update.py: test_conv_update_refreshes_every_live_form under guard -- each lazily built conv layout is
    brought to life, then rewritten by the update"""
    small = mode in ("bf16", "fp16")
    keys = [CONV_256, UPS, "conv_in.weight", LIN_Q]
    expect = {("fp32", "direct"): {CONV_256: ["fp32", "conv_direct32"], LIN_Q: ["fp32", "bf16"]},
              ("fp32", "winograd"): {CONV_256: ["fp32", "wino2"]}, ("fp32", "winograd4"): {CONV_256: ["fp32", "wino4"]},
              ("f32x3", "winograd"): {CONV_256: ["wino2", "wino2_x3"], LIN_Q: ["x3"]},
              ("f32x3", "winograd4"): {CONV_256: ["wino4", "wino4_x3"], LIN_Q: ["x3"]},
              ("bf16", None): {CONV_256: ["bf16"], UPS: ["bf16_up2"], LIN_Q: ["bf16"]},
              ("fp16", None): {CONV_256: ["fp16"], UPS: ["f16_up2"], LIN_Q: ["fp16"]}}[mode, algo]
    new = {k: draw(k, U0[k].shape) for k in keys}
    pp = fresh_pipes({"E2V_F32X3": "1"} if mode == "f32x3" else None)
    who = by_engine(pp)
    knobs = {"E2V_BGEMM_UP2X": 2, "E2V_SMALL_FAMILY_CLIPS": 0} if small else None

    def run(e):
        p = who[id(e)]
        if not getattr(p, "_updated", False):
            if algo:
                e.set_conv_algo(algo)
            before = unet_fwd(p, small)
            for k, names in expect.items():
                for n in names:
                    assert e.weight_forms(k) & BITS[n], (k, n, e.weight_forms(k))
            forms = {k: e.weight_forms(k) for k in keys}
            p.unet.sync_from({k: _t(v).cuda() for k, v in new.items()})
            p._updated = True
            assert {k: e.weight_forms(k) for k in keys} == forms           # nothing is built by an update
            assert not torch.equal(unet_fwd(p, small), before)
        return unet_fwd(p, small)

    y = guarded_run(engines(pp), run, mode, knobs, f"conv forms {mode} {algo}")
    with environment({"E2V_F32X3": "1"} if mode == "f32x3" else {}, 0):
        fresh = build_pipe(dict(U0, **new), V0)                           # the state a fresh build of the updated state dict has
    if algo:
        fresh.unet.engine.set_conv_algo(algo)
    with settings(fresh.unet.engine, mode, knobs):
        ref = unet_fwd(fresh, small)
    assert torch.isfinite(y).all() and torch.equal(y, ref)


# ------------------------------------------------------------------ 16-bit op entry points: the operands live in the pool ------------
@pytest.fixture(scope="module")
def op_pair():
    with environment({}, 0):
        off = make_engine()
    with environment({}, GUARD_KIB):
        on = make_engine()
    return off, on


@pytest.fixture(params=["bf16", "fp16"])
def h16(request):
    return request.param


def rb(t, mode):
    return t.to(H16_TYPES[mode]).float()


def tol16(mode, bf16_tol, fp16_tol=None):                  # tests/test_hip_ops.py
    return bf16_tol if mode == "bf16" else (fp16_tol if fp16_tol is not None else bf16_tol / 4)


def gelu16(x, mode):                                       # tests/test_hip_ops.py: gelu_bf16_grade
    return F.gelu(x) if mode == "fp16" else x / (1.0 + torch.exp(-(1.60031415 * x + 0.06940179 * x ** 3)))


@pytest.mark.parametrize("m,k,n,t256,geglu", [(130, 40, 72, 1, False), (257, 768, 136, 1, False), (5, 320, 1280, 1, False),
                                              (4097, 704, 640, 2, False), (513, 2560, 320, 2, False), (130, 704, 5120, 2, True)])
def test_h16_linear_guarded(op_pair, h16, m, k, n, t256, geglu):
    x, w, b = rnd(m, k, seed=20), rnd(n, k, seed=21, scale=0.05), rnd(n, seed=22)
    r = None if geglu or (m, k, n) == (4097, 704, 640) else rnd(m, n, seed=23)
    gx, gw, gb, gr = x.cuda(), w.cuda(), b.cuda(), (r.cuda() if r is not None else None)
    y = guarded_run(op_pair, lambda e: e.op_linear(gx, gw, gb, gr, geglu=geglu), h16, {"E2V_BGEMM_T256": t256}, f"linear {m}x{k}x{n}")
    ref = F.linear(rb(x, h16), rb(w, h16), b)
    if geglu:
        hh, gg = ref.chunk(2, dim=-1)
        ref = hh * gelu16(gg, h16)
    close(y, ref + (r if r is not None else 0), rtol=1e-4, atol=1e-4, what="linear")


def conv16(op_pair, mode, x, wt, b, knobs=None, x1=None, stride=1, pad_lo=1, pad_hi=1, hi=None, wi=None, temb=None, f=1, res=None, what="conv",
           ref=None):
    n, _, hs, ws = x.shape
    hi, wi = hi or hs, wi or ws
    if ref is None:
        src = rb(torch.cat([x, x1], 1) if x1 is not None else x, mode)
        if (hi, wi) != (hs, ws):
            src = F.interpolate(src, size=(hi, wi), mode="nearest")
        ref = F.conv2d(F.pad(src, (pad_lo, pad_hi, pad_lo, pad_hi)), rb(wt, mode), b, stride=stride)
        if temb is not None:
            ref = ref + temb.repeat_interleave(f, 0)[:, :, None, None]
        if res is not None:
            ref = ref + res
    ho, wo = ref.shape[2], ref.shape[3]
    g = dict(x=to_cl(x).cuda(), w=wt.cuda(), b=b.cuda(), x1=to_cl(x1).cuda() if x1 is not None else None,
             t=temb.cuda().contiguous() if temb is not None else None, r=to_cl(res).cuda() if res is not None else None)
    y = guarded_run(op_pair, lambda e: e.op_conv3x3(g["x"], g["w"], g["b"], g["x1"], n_img=n, Hs=hs, Ws=ws, Hi=hi, Wi=wi, stride=stride, pad_lo=pad_lo,
                                                    pad_hi=pad_hi, rowbias=g["t"], rows_per_sample=f * ho * wo, resid=g["r"]), mode, knobs, what)
    close(from_cl(y, n, ho, wo), ref, rtol=1e-4, atol=1e-4, what=what)
    return y


def test_h16_conv_geometries_guarded(op_pair, h16):
    """the lists of test_bf16_conv3x3_geometries and test_bf16_t256_conv3x3_geometries (tests/test_hip_ops.py)"""
    wt, b = rnd(64, 32, 3, 3, seed=5, scale=0.1), rnd(64, seed=6)
    conv16(op_pair, h16, rnd(2, 32, 9, 12, seed=4), wt, b, stride=2, what="stride 2")
    conv16(op_pair, h16, rnd(2, 32, 8, 12, seed=7), wt, b, stride=2, pad_lo=0, pad_hi=1, what="stride 2, pad (0, 1)")
    for hs, ws, hi, wi in [(5, 8, 9, 16), (3, 3, 5, 6), (5, 6, 12, 7)]:
        conv16(op_pair, h16, rnd(3, 32, hs, ws, seed=8), wt, b, hi=hi, wi=wi, what="resize")
    conv16(op_pair, h16, what="concat", **concat_case())
    t256 = {"E2V_BGEMM_T256": 2}
    wt, b = rnd(256, 128, 3, 3, seed=150, scale=0.05), rnd(256, seed=151)
    conv16(op_pair, h16, rnd(2, 128, 8, 12, seed=152), wt, b, t256, stride=2, pad_lo=0, pad_hi=1, what="256-row tiles, stride 2")
    n_s, f, c0, c1, cout, h, w = 2, 3, 128, 64, 320, 9, 16
    conv16(op_pair, h16, rnd(n_s * f, c0, h, w, seed=153), rnd(cout, c0 + c1, 3, 3, seed=155, scale=0.05), rnd(cout, seed=156), t256,
           x1=rnd(n_s * f, c1, h, w, seed=154), temb=rnd(n_s, cout, seed=157), f=f, res=rnd(n_s * f, cout, h, w, seed=158), what="256-row tiles, concat")


def test_h16_upsample_conv_sub_pixel_form_guarded(op_pair, h16):
    """tests/test_hip_ops.py: test_bf16_upsample_conv_sub_pixel_form at (2, 128, 512, 7, 6)"""
    n, c, cout, hs, ws = 2, 128, 512, 7, 6
    x, wt, b = rnd(n, c, hs, ws, seed=170), rnd(cout, c, 3, 3, seed=171, scale=0.05), rnd(cout, seed=172)
    sets = {0: ([0], [1, 2]), 1: ([0, 1], [2])}
    ref = torch.zeros(n, cout, 2 * hs, 2 * ws)
    for a in (0, 1):
        for bq in (0, 1):
            w2 = torch.stack([torch.stack([wt[:, :, sets[a][ty]][:, :, :, sets[bq][tx]].sum((2, 3)) for tx in (0, 1)], -1) for ty in (0, 1)], -2)
            ref[:, :, a::2, bq::2] = F.conv2d(F.pad(rb(x, h16), (1 - bq, bq, 1 - a, a)), rb(w2, h16), b)
    conv16(op_pair, h16, x, wt, b, {"E2V_BGEMM_T256": 2, "E2V_BGEMM_UP2X": 1}, hi=2 * hs, wi=2 * ws, ref=ref, what="sub-pixel upsample")


@pytest.mark.parametrize("runs", [2, 3, 5, 16])
def test_h16_splitk_guarded(op_pair, h16, runs):
    """tests/test_hip_ops.py: test_h16_splitk_conv_and_linear_equal_the_unsplit_kernels_to_summation_order -- the partial planes are a
    pool block that every run must fill before the reduce reads it"""
    force = {"E2V_SPLITK_FORCE": runs}
    n_s, f, c0, c1, cout, h, w = 2, 3, 128, 64, 320, 5, 8
    n = n_s * f
    conv16(op_pair, h16, rnd(n, c0, h, w, seed=601), rnd(cout, c0 + c1, 3, 3, seed=603, scale=0.1), rnd(cout, seed=604), force,
           x1=rnd(n, c1, h, w, seed=602), temb=rnd(n_s, cout, seed=605), f=f, res=rnd(n, cout, h, w, seed=606), what="split-K conv")
    conv16(op_pair, h16, rnd(3, 256, 9, 12, seed=607), rnd(72, 256, 3, 3, seed=608, scale=0.1), rnd(72, seed=609), force, stride=2,
           what="split-K conv, stride 2")
    m, k, nn = 154, 2560, 320
    xl, wl, bl, r = rnd(m, k, seed=610), rnd(nn, k, seed=611, scale=0.05), rnd(nn, seed=612), rnd(m, nn, seed=613)
    gx, gw, gb, gr = xl.cuda(), wl.cuda(), bl.cuda(), r.cuda()
    y = guarded_run(op_pair, lambda e: e.op_linear(gx, gw, gb, gr), h16, force, "split-K linear")
    close(y, F.linear(rb(xl, h16), rb(wl, h16), bl) + r, rtol=1e-4, atol=1e-4, what="split-K linear")


def attn32(q, k, v, scale):        # tests/test_hip_ops.py: _ref_attn
    s = torch.baddbmm(torch.empty(q.shape[0], q.shape[1], k.shape[1]), q, k.transpose(1, 2), beta=0, alpha=scale)
    return torch.bmm(s.softmax(-1), v)


@pytest.mark.parametrize("q64", [1, 0])
@pytest.mark.parametrize("d,nq,f,n", [(40, 130, 3, 1), (40, 333, 4, 9), (32, 9, 3, 2)])
def test_h16_sparse_causal_attention_guarded(op_pair, h16, d, nq, f, n, q64):
    """d = 40: test_bf16_attention_64_queries_per_wave (operands as the kernel rounds them, 1e-2); d = 32: test_bf16_attention (2e-2)"""
    heads = 8
    c = heads * d
    qkv = rnd(n * f * nq, 3 * c, seed=280)
    if d == 40:
        qs = d ** -0.5 * 1.4426950408889634
        q = (rb(rb(qkv[:, :c], h16) * qs, h16) / qs).reshape(n * f, nq, c)
        k, v = (rb(qkv[:, i * c:(i + 1) * c], h16).reshape(n * f, nq, c) for i in (1, 2))
        tol = tol16(h16, 1e-2)
    else:
        q, k, v = (qkv[:, i * c:(i + 1) * c].reshape(n * f, nq, c) for i in range(3))
        tol = tol16(h16, 2e-2)
    former = torch.arange(f) - 1
    former[0] = 0
    gather = lambda t: torch.cat([t.reshape(n, f, nq, c)[:, [0] * f], t.reshape(n, f, nq, c)[:, former]], dim=2).reshape(n * f, 2 * nq, c)
    ref = unheads(attn32(heads_of(q, heads), heads_of(gather(k), heads), heads_of(gather(v), heads), d ** -0.5), heads)
    g = qkv.cuda()
    y = guarded_run(op_pair, lambda e: e.op_attention(g[:, :c], g[:, c:2 * c], g[:, 2 * c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nq, mode=0,
                                                      scale=d ** -0.5), h16, {"E2V_ATTN_Q64": q64}, f"attention d={d} nq={nq}")
    close(y.reshape(n * f, nq, c), ref, rtol=tol, atol=tol, what="attention")


def test_h16_cross_attention_resident_keys_guarded(op_pair, h16):
    d, nq, f, n, nk, heads = 40, 50, 2, 1, 96, 8
    c = heads * d
    q, kv = rnd(n * f * nq, c, seed=181), rnd(n * nk, 2 * c, seed=182)
    k, v = rb(kv[:, :c], h16).reshape(n, nk, c), rb(kv[:, c:], h16).reshape(n, nk, c)
    rep = lambda t: t.repeat_interleave(f, 0)
    qs = d ** -0.5 * 1.4426950408889634
    q_eff = rb(rb(q, h16) * qs, h16) / qs
    ref = unheads(attn32(heads_of(q_eff.reshape(n * f, nq, c), heads), heads_of(rep(k), heads), heads_of(rep(v), heads), d ** -0.5), heads)
    gq, gkv = q.cuda(), kv.cuda()
    y = guarded_run(op_pair, lambda e: e.op_attention(gq, gkv[:, :c], gkv[:, c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nk, mode=1, scale=d ** -0.5),
                    h16, {"E2V_ATTN_CROSS_RESIDENT": 1}, "cross-attention, resident keys")
    close(y.reshape(n * f, nq, c), ref, rtol=tol16(h16, 2e-2), atol=tol16(h16, 2e-2), what="cross-attention")


def coop_build(eng):
    try:
        eng.set_knob("E2V_GN_COOP", 0)
        return True
    except ValueError:
        return False


@pytest.mark.parametrize("form", ["row_tiled", "fused_small", "cooperative"])
def test_h16_groupnorm_forms_guarded(op_pair, h16, form):
    """one case per form: the row-tiled apply pass with sample runs (two sources, 5 x 700 rows), the one-kernel form of the small-batch
    family, and -- in builds that carry it (`make ab`) -- the smallest cooperative case.  tests/test_hip_ops.py, 8e-3 / 2e-3."""
    samples, P, c0, c1, groups, silu, knobs = {"row_tiled": (5, 700, 320, 320, 32, True, None),
                                               "fused_small": (2, 50, 64, 32, 8, True, {"E2V_GN_FUSED_SMALL": 2}),
                                               "cooperative": (1, 77, 96, 0, 4, False, {"E2V_GN_COOP": 2})}[form]
    if form == "cooperative" and not coop_build(op_pair[0]):
        pytest.skip("the cooperative one-launch GroupNorm was measured and not adopted: `make ab` builds only (DESIGN 3.9)")
    a = rnd(samples * P, c0, seed=130)
    s = rnd(samples * P, c1, seed=131) if c1 else None
    g, be = rnd(c0 + c1, seed=132), rnd(c0 + c1, seed=133)
    xin = (torch.cat([rb(a, h16), rb(s, h16)], 1) if c1 else rb(a, h16)).reshape(samples, P, c0 + c1).permute(0, 2, 1)
    ref = F.group_norm(xin, groups, g, be, 1e-5)
    ref = (F.silu(ref) if silu else ref).permute(0, 2, 1).reshape(samples * P, c0 + c1)
    ga, gs, gg, gb = a.cuda(), (s.cuda() if c1 else None), g.cuda(), be.cuda()
    y = guarded_run(op_pair, lambda e: e.op_groupnorm(ga, gg, gb, samples=samples, P=P, groups=groups, eps=1e-5, silu=silu, x1=gs), h16, knobs,
                    f"groupnorm {form}")
    close(y, ref, rtol=tol16(h16, 8e-3), atol=tol16(h16, 8e-3), what="groupnorm")


@pytest.mark.parametrize("c,rows", [(320, 77), (1280, 13), (1280, 4)])
def test_h16_layernorm_guarded(op_pair, h16, c, rows):
    x, gl, bl = rnd(rows, c, seed=140), rnd(c, seed=141), rnd(c, seed=142)
    gx, gg, gb = x.cuda(), gl.cuda(), bl.cuda()
    y = guarded_run(op_pair, lambda e: e.op_layernorm(gx, gg, gb), h16, None, f"layernorm {rows} x {c}")
    close(y, F.layer_norm(rb(x, h16), (c,), gl, bl), rtol=tol16(h16, 8e-3), atol=tol16(h16, 8e-3), what="layernorm")
