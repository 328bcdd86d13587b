"""The 16-k fp32 GEMM tile with its operands moved by LDS-DMA (igemm_k16_kernel: unpadded, XOR-swizzled 64-byte LDS rows, two stage
buffers, four workgroups per CU).

* Bit identity against the untouched register-staged 32-k tile (``E2V_IGEMM_K16=0``, read once per process: one child per arm, every case
  in one child).  Both walk k in the same order through the same MFMA sequence, so every output word must be equal.
* The default arm in this process, operands and result in the poisoned, fenced buffers of ``tests/test_hip_bounds.py`` (x and x1 with a
  padded row stride): nothing outside the result is written, nothing outside the operands is read, and every element stays inside the
  bound ``tests/test_hip_igemm_schedule.py`` puts on its kind of launch -- linears: ``(K + 4) 2^-24 (sum |x||w| + |bias| + |resid|)`` per
  element against float64; GEGLU (a product of two such sums through an erf) and the Winograd convs (whose transforms amplify): that
  file's global bounds, ``RTOL / ATOL`` and ``BOUNDS[algo]``.

The shapes are the smallest that reach each path of the loader and the ring: one ragged stage (K = 8, K = 4 in the Winograd GEMMs), an
even and an odd stage count, a last stage that holds one 16-byte chunk (K = 20), rows and columns that end inside a DMA piece, wide and
narrow tiles in one launch, the concat seam with both segments ragged (24 + 40), the residual, GEGLU and scalar epilogues, and batched
launches (the 16 / 36 GEMMs of a Winograd conv).
"""
import os
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.nn.functional as F

from test_hip_bounds import BOUNDS, conv_fenced, fenced, fenced_out, make_engine, rnd, run_fenced, to_cl

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                     # unit roundoff of fp32
RTOL, ATOL = 2e-5, 2e-5            # tests/test_hip_igemm_schedule.py: the GEGLU launches
PAD = 4                            # floats between the rows of x and x1
RECORD = "igemm_k16_kernel 128x128x16"

# (name, M, K of x, K of x1, N = rows of w, epilogue)
LINEARS = [
    ("1x16x4", 1, 16, 0, 4, "bias"),
    ("130x8x72 one ragged stage, 2-row last block, ragged narrow tile", 130, 8, 0, 72, "bias"),
    ("128x32x64 exact tile, even stage count", 128, 32, 0, 64, "bias"),
    ("129x48x200 odd stage count, wide + narrow tiles", 129, 48, 0, 200, "bias"),
    ("300x20x132 last stage of one chunk", 300, 20, 0, 132, "bias"),
    ("257x320x320 residual", 257, 320, 0, 320, "bias_residual"),
    ("260x320x256 geglu", 260, 320, 0, 256, "geglu"),
    ("40x320x3 scalar epilogue", 40, 320, 0, 3, "bias"),
    ("200x(24+40)x96 concat, both segments ragged", 200, 24, 40, 96, "bias"),
]
CONVS = [("winograd4", 2, 4, 4, 8, 12), ("winograd", 2, 4, 4, 8, 12)]      # (form, images, cin, cout, h, w): the smallest widths the forms take


def linear_operands(i):
    _, m, k0, k1, n, epi = LINEARS[i]
    x, w, b = rnd(m, k0 + k1, seed=300 + 4 * i), rnd(n, k0 + k1, seed=301 + 4 * i, scale=0.05), rnd(n, seed=302 + 4 * i)
    r = rnd(m, n, seed=303 + 4 * i) if epi == "bias_residual" else None
    return x, w, b, r


def conv_operands(i):
    _, n, cin, cout, h, w = CONVS[i]
    return rnd(n, cin, h, w, seed=400 + 3 * i), rnd(cout, cin, 3, 3, seed=401 + 3 * i, scale=0.1), rnd(cout, seed=402 + 3 * i)


def run_all(eng):
    """every case on plain device tensors -> list of results (the child processes of the bit-identity test)"""
    outs = []
    for i, (_, m, k0, k1, n, epi) in enumerate(LINEARS):
        x, w, b, r = linear_operands(i)
        gx = x.cuda()
        outs.append(eng.op_linear(gx[:, :k0], w.cuda(), b.cuda(), r.cuda() if r is not None else None, geglu=epi == "geglu",
                                  x1=gx[:, k0:] if k1 else None).cpu())
    for i, (algo, n, cin, cout, h, w_) in enumerate(CONVS):
        x, wt, b = conv_operands(i)
        eng.set_conv_algo(algo)
        try:
            outs.append(eng.op_conv3x3(to_cl(x).cuda(), wt.cuda(), b.cuda(), n_img=n, Hs=h, Ws=w_).cpu())
        finally:
            eng.set_conv_algo("auto")
    return outs


def test_dma_tile_and_32k_tile_are_bit_identical():
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, torch\n"
            f"sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r})\n"
            "import test_hip_igemm_dma as t\n"
            "torch.save(t.run_all(t.make_engine()), sys.argv[1])\n")
    res = []
    for flag in ("1", "0"):
        with tempfile.NamedTemporaryFile(suffix=".pt") as f:
            subprocess.run([sys.executable, "-c", code, f.name], check=True, env=dict(os.environ, E2V_IGEMM_K16=flag), timeout=300)
            res.append(torch.load(f.name))
    names = [c[0] for c in LINEARS] + [f"{c[0]} conv" for c in CONVS]
    assert len(res[0]) == len(res[1]) == len(names)
    for name, a, b in zip(names, *res):
        diff = int((a.view(torch.int32) != b.view(torch.int32)).sum())
        print(f"{name}: {diff} of {a.numel()} words differ")
        assert torch.equal(a, b), f"{name}: {diff} of {a.numel()} words differ between the 16-k DMA tile and the 32-k tile"


@pytest.fixture(scope="module")
def eng():
    if "E2V_IGEMM_K16" in os.environ:
        pytest.fail("E2V_IGEMM_K16 set in the environment: the arm under test is the default one")
    e = make_engine()
    e.set_knob("E2V_OP_RECORD", 1)
    try:
        yield e
    finally:
        e.set_knob("E2V_OP_RECORD", 0)


@pytest.mark.parametrize("i", range(len(LINEARS)), ids=[c[0].split()[0] for c in LINEARS])
def test_dma_tile_linear_fenced(eng, i):
    name, m, k0, k1, n, epi = LINEARS[i]
    x, w, b, r = linear_operands(i)
    geglu = epi == "geglu"
    fx = fenced(x[:, :k0], ld=k0 + PAD, name="x")
    f1 = fenced(x[:, k0:], ld=k1 + PAD, name="x1") if k1 else None
    fw, fb = fenced(w, name="w"), fenced(b, name="bias")
    fr = fenced(r, name="resid") if r is not None else None
    out = fenced_out((m, n // 2 if geglu else n))
    y = run_fenced(lambda: eng.op_linear(fx.t, fw.t, fb.t, fr.t if fr else None, geglu=geglu, out=out.t, x1=f1.t if f1 else None),
                   [fx, f1, fw, fb, fr], out)
    tag = eng.last_dispatch()
    assert RECORD in tag, f"dispatch record '{tag}'"
    if geglu:
        h, g = F.linear(x.double(), w.double(), b.double()).chunk(2, dim=-1)
        ref = h * F.gelu(g)
        scale = ref.abs().max().item()
        bound = torch.full_like(ref, ATOL * max(1.0, scale) + RTOL * scale)
    else:
        ref = x.double() @ w.double().T + b.double()
        mag = x.double().abs() @ w.double().abs().T + b.double().abs()
        if r is not None:
            ref, mag = ref + r.double(), mag + r.double().abs()
        bound = (k0 + k1 + 4) * U * mag
    err = (y.cpu().double() - ref).abs()
    ratio = err / bound
    worst = int(ratio.argmax())
    print(f"{name}: worst error / bound {ratio.flatten()[worst].item():.3f} (|err| {err.flatten()[worst].item():.3e}) at element "
          f"{divmod(worst, ref.shape[1])}")
    assert bool((err <= bound).all()), f"{name}: |err| {err.flatten()[worst].item():.3e} > bound {bound.flatten()[worst].item():.3e} at {divmod(worst, ref.shape[1])}"


@pytest.mark.parametrize("i", range(len(CONVS)), ids=[c[0] for c in CONVS])
def test_dma_tile_winograd_batched_fenced(eng, i):
    algo = CONVS[i][0]
    x, wt, b = conv_operands(i)
    eng.set_conv_algo(algo)
    try:
        conv_fenced(eng, x, wt, b, what=algo, **BOUNDS[algo])
        tag = eng.last_dispatch()
    finally:
        eng.set_conv_algo("auto")
    assert RECORD in tag, f"dispatch record '{tag}'"
