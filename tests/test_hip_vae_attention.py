"""GPU: the attention of the VAE mid block kernel by kernel -- ``e2v_op_vae_attention_core`` (``Runner::vae_attention_core``, the member
both VAE graphs call: the batched strided scores GEMM with ``alpha``, ``softmax_rows``, ``transpose2d``, the batched PV GEMM),
``e2v_op_softmax_rows`` and ``e2v_op_transpose2d`` -- against the float64 references and per-element budgets of
``tests/vae_attn_budget.py``.  The case tables, sentinels and the mutants they are proven sensitive to are that module's;
``tests/test_vae_attn_budget_host.py`` holds them to their conditions without a GPU.

* the block: scaled scores, probabilities (as the PV GEMM reads them) and output each within its budget, in fp32, bf16 and fp16; in fp32
  both GEMMs must have run on the 16-k LDS-DMA tile; the same calls with every operand and result in the fenced, poisoned buffers of
  ``tests/test_hip_bounds.py``, and once under the guarded pool; an f32x3 context gives the bits of fp32 (the block never sets ``x3``);
* the softmax alone, rows padded: budget, row sums, a constant row, a dominant key, 16-bit copies, the padding untouched;
* the transpose alone, padded row and batch strides, 4- and 2-byte payloads: bit-exact, nothing else written;
* bit identity: image z of a three-image call against the one-image call (the tile plan differs with the batch), and the 16-k DMA tile
  against the 32-k tile (``E2V_IGEMM_K16=0``, one child process per arm);
* the one measured constant of the budgets, the ulp error of the device's ``expf``, measured again.

Each test prints its largest error / budget and where it lies (``-s``)."""
import functools
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import vae_attn_budget as vb
from test_hip_bounds import FENCE, GUARD_KIB, POISON, environment, fenced, fenced_out, guarded_run, make_engine

pytestmark = pytest.mark.gpu

RECORD = "igemm_k16_kernel 128x128x16"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
BLOCK_PARAMS = [pytest.param(c, m, id=f"{c['id']}-{m}") for c in vb.BLOCK_CASES for m in c["modes"]]
NAMES = ("scores", "probabilities", "output")


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


@pytest.fixture(scope="module")
def op_pair():
    with environment({}, 0):
        off = make_engine()
    with environment({}, GUARD_KIB):
        on = make_engine()
    return off, on


class mode_of:
    def __init__(self, eng, mode):
        self.eng, self.mode = eng, mode

    def __enter__(self):
        self.eng.set_compute_dtype(self.mode)
        return self.eng

    def __exit__(self, *exc):
        self.eng.set_compute_dtype("fp32")


def kw_of(case):
    return dict(nimg=case["nimg"], HW=case["HW"], C=case["C"])


@functools.lru_cache(maxsize=None)
def block_ref(case_id, mode):
    case = next(c for c in vb.BLOCK_CASES if c["id"] == case_id)
    ref = vb.block_reference(vb.block_inputs(case), mode=mode, **kw_of(case))
    return (ref["s"], ref["p"], ref["o"]), vb.block_budgets(ref, mode=mode, **kw_of(case))


@functools.lru_cache(maxsize=None)
def block_plain(eng, case_id, mode):
    """the case on plain device tensors: (o, s, p) and the dispatch record, computed once and left unchanged"""
    case = next(c for c in vb.BLOCK_CASES if c["id"] == case_id)
    with mode_of(eng, mode) as e:
        out = e.op_vae_attention_core(vb.block_inputs(case).cuda(), intermediates=True, **kw_of(case))
        tag = e.last_dispatch()
    return tuple(t.cpu() for t in out), tag


def bits(t):
    return t.contiguous().view(torch.int32)


def check_budget(what, y, ref, budget, group_rows=None):
    """every element of y within its budget; prints the largest ratio and its place; returns the ratio"""
    y = y.detach().cpu()
    assert y.shape == ref.shape == budget.shape, f"{what}: shapes {tuple(y.shape)}, {tuple(ref.shape)}"
    r = vb.ratio(y, ref, budget)
    i = int(r.argmax())
    row, col = divmod(i, r.shape[1])
    worst = float(r.flatten()[i])
    place = f"[{row}, {col}]" + (f" (image {row // group_rows}, row {row % group_rows})" if group_rows else "")
    print(f"{what}: worst error / budget {worst:.3f} (|err| {float((y.double() - ref).abs().flatten()[i]):.3e}) at {place}")
    assert worst <= 1.0, (f"{what}: {int((r > 1).sum())} of {r.numel()} elements over budget; worst {place}: got {float(y.flatten()[i]):.9g}, reference "
                          f"{float(ref.flatten()[i]):.9g} = {worst:.2f} x budget {float(budget.flatten()[i]):.3e}")
    return worst


# ------------------------------------------------------------------ the block
@pytest.mark.parametrize("case,mode", BLOCK_PARAMS)
def test_core_block_vs_float64(eng, case, mode):
    """scores, probabilities and output of every case against the float64 reference, each element within its budget; fp32: both GEMMs on
    the 16-k DMA tile."""
    (o, s, p), tag = block_plain(eng, case["id"], mode)
    refs, budgets = block_ref(case["id"], mode)
    print()
    for name, y, ref, b in zip(NAMES, (s, p, o), refs, budgets):
        check_budget(f"{case['id']} [{mode}] {name}", y, ref, b, case["HW"])
    if mode == "fp32":
        assert tag.count(RECORD) == 2, f"dispatch record '{tag}'"


@pytest.mark.parametrize("case,mode", BLOCK_PARAMS)
def test_core_block_fenced(eng, case, mode):
    """the same call with qkv, the result and the two intermediates inside poisoned, fenced buffers: no word outside them changes, qkv is
    unchanged, no NaN comes out (nothing was read that is not an operand, every element was written), and the bits are those of the
    plain call (which the test above holds to the budgets)."""
    rows, HW, C = case["nimg"] * case["HW"], case["HW"], case["C"]
    fq = fenced(vb.block_inputs(case), name="qkv")
    fo, fs, fp = fenced_out((rows, C)), fenced_out((rows, HW)), fenced_out((rows, HW))
    fs.name, fp.name = "scores", "probs"
    with mode_of(eng, mode) as e:
        e.op_vae_attention_core(fq.t, out=fo.t, scores=fs.t, probs=fp.t, **kw_of(case))
    torch.cuda.synchronize()
    for f in (fq, fo, fs, fp):
        f.check()
    plain, _ = block_plain(eng, case["id"], mode)
    for name, f, want in zip(("output", "scores", "probabilities"), (fo, fs, fp), plain):
        y = f.view.cpu()
        assert not torch.isnan(y).any(), f"{case['id']} [{mode}] {name}: {int(torch.isnan(y).sum())} NaN: an element was not written, or depends on memory outside the operands"
        assert torch.equal(bits(y), bits(want)), f"{case['id']} [{mode}] {name}: the fenced call and the plain call differ"


@pytest.mark.parametrize("case,mode", BLOCK_PARAMS)
def test_core_block_guarded(op_pair, case, mode):
    """once under the guarded workspace pool: the scores, the 16-bit copies, V^T and the 16-bit operands live there"""
    g = vb.block_inputs(case).cuda()
    o, s, p = guarded_run(op_pair, lambda e: e.op_vae_attention_core(g, intermediates=True, **kw_of(case)), mode, None, f"{case['id']} [{mode}]")
    refs, budgets = block_ref(case["id"], mode)
    for name, y, ref, b in zip(NAMES, (s, p, o), refs, budgets):
        check_budget(f"{case['id']} [{mode}, guarded] {name}", y, ref, b, case["HW"])


def test_f32x3_context_gives_the_bits_of_fp32(eng):
    """the block never sets ``x3``: its GEMMs are the fp32 ones whatever the context splits elsewhere"""
    e3 = make_engine()
    e3.set_compute_dtype("f32x3")                        # (before any weights: the mode is chosen ahead of e2v_finalize_weights)
    assert e3.compute_dtype == "f32x3"
    for case in vb.BLOCK_CASES:
        if "fp32" not in case["modes"]:
            continue
        got = e3.op_vae_attention_core(vb.block_inputs(case).cuda(), intermediates=True, **kw_of(case))
        want, _ = block_plain(eng, case["id"], "fp32")
        for name, a, b in zip(("output", "scores", "probabilities"), got, want):
            assert torch.equal(bits(a.cpu()), bits(b)), f"{case['id']} {name}: an f32x3 context differs from fp32"


@pytest.mark.parametrize("mode", vb.MODES)
def test_core_block_refuses_what_the_graph_refuses(eng, mode):
    """H*W has to be a multiple of 4 (16-bit modes: 8): refused, and the output left alone"""
    for HW, C in (vb.REFUSED_FP32 if mode == "fp32" else vb.REFUSED_16BIT):
        out = torch.full((HW, C), 7.0, device="cuda")
        with mode_of(eng, mode) as e, pytest.raises((ValueError, RuntimeError)):
            e.op_vae_attention_core(vb.rnd(HW, 3 * C, seed=1).cuda(), nimg=1, HW=HW, C=C, out=out)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), f"HW = {HW} [{mode}]: a refused call wrote to its output"


BATCH_OF_3 = [c for c in vb.BLOCK_CASES if c["HW"] in (24, 260, 264) and c["C"] == 64 and c["nimg"] == 3 and not c["offset"]]


@pytest.mark.parametrize("case,mode", [pytest.param(c, m, id=f"{c['id']}-{m}") for c in BATCH_OF_3 for m in c["modes"]])
def test_image_z_of_a_batch_equals_the_single_image_call(eng, case, mode):
    """word for word, scores, probabilities and output, in fp32 and in each 16-bit mode: at HW = 260 (fp32; the 16-bit modes take 264)
    the tile plan of the batched launch differs from the single one"""
    HW = case["HW"]
    batch, _ = block_plain(eng, case["id"], mode)
    qkv = vb.block_inputs(case).reshape(3, HW, -1)
    with mode_of(eng, mode) as e:
        for z in range(3):
            one = e.op_vae_attention_core(qkv[z].contiguous().cuda(), nimg=1, HW=HW, C=64, intermediates=True)
            for name, a, b in zip(("output", "scores", "probabilities"), one, batch):
                diff = int((bits(a.cpu()) != bits(b[z * HW:(z + 1) * HW])).sum())
                assert diff == 0, f"HW = {HW} [{mode}] image {z}, {name}: {diff} of {a.numel()} words differ from the batched call"


def run_all(eng):
    """every fp32 case on plain device tensors -> [(o, s, p)] (the child processes of the tile test)"""
    return [tuple(t.cpu() for t in eng.op_vae_attention_core(vb.block_inputs(c).cuda(), intermediates=True, **kw_of(c)))
            for c in vb.BLOCK_CASES if "fp32" in c["modes"]]


def test_dma_tile_and_32k_tile_are_bit_identical():
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, torch\n"
            f"sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r})\n"
            "import test_hip_vae_attention as t\n"
            "torch.save(t.run_all(t.make_engine()), sys.argv[1])\n")
    res = []
    for flag in ("1", "0"):
        with tempfile.NamedTemporaryFile(suffix=".pt") as f:
            subprocess.run([sys.executable, "-c", code, f.name], check=True, env=dict(os.environ, E2V_IGEMM_K16=flag), timeout=300)
            res.append(torch.load(f.name))
    names = [c["id"] for c in vb.BLOCK_CASES if "fp32" in c["modes"]]
    assert len(res[0]) == len(res[1]) == len(names)
    for name, a3, b3 in zip(names, *res):
        for part, a, b in zip(("output", "scores", "probabilities"), a3, b3):
            diff = int((bits(a) != bits(b)).sum())
            assert diff == 0, f"{name} {part}: {diff} of {a.numel()} words differ between the 16-k DMA tile and the 32-k tile"


# ------------------------------------------------------------------ fenced buffers of any element size
class RawFence:
    """``count`` elements of ``dtype`` (int16 / int32 / a 16-bit float type) in the middle of a poisoned flat device buffer"""

    def __init__(self, count, dtype, name):
        self.name, self.count = name, count
        size = torch.empty(0, dtype=dtype).element_size()
        self.per = 4 // size
        self.words = torch.full((2 * FENCE + (count + self.per - 1) // self.per,), POISON, dtype=torch.int32, device="cuda")
        self.flat = self.words.view(dtype)[FENCE * self.per:FENCE * self.per + count]
        self.inside = torch.zeros(self.words.numel() * self.per, dtype=torch.bool, device="cuda")

    def own(self, index):
        """mark flat element indices (a tensor) as the tensor's own"""
        self.inside[FENCE * self.per + index.to("cuda")] = True

    def check(self):
        raw = self.words.view(torch.int16) if self.per == 2 else self.words
        poison = 0x7FC0 if self.per == 2 else POISON
        bad = (~self.inside & (raw != poison)).nonzero().flatten()
        assert bad.numel() == 0, (f"{self.name}: {bad.numel()} elements outside the tensor changed; first at element {int(bad[0]) - FENCE * self.per} "
                                  f"from the tensor's start, last at {int(bad[-1]) - FENCE * self.per}")


def strided(rows, cols, ld, batch=1, sb=0):
    """flat indices of ``batch`` matrices [rows][cols] of row stride ld, sb apart"""
    i = torch.arange(batch)[:, None, None] * sb + torch.arange(rows)[None, :, None] * ld + torch.arange(cols)[None, None, :]
    return i.reshape(-1)


# ------------------------------------------------------------------ the softmax alone
@functools.lru_cache(maxsize=None)
def softmax_ref(cols, out_mode):
    ref = vb.softmax_reference(vb.softmax_inputs(cols))
    return ref, vb.softmax_budget(ref, out_mode)


def softmax_run(eng, cols, out_mode, pad=4):
    """x (and the 16-bit copy) with ``pad`` poisoned columns between the rows -> (x afterwards, the copy widened or None), on the host"""
    x = vb.softmax_inputs(cols)
    rows, ld = x.shape[0], cols + pad
    idx = strided(rows, cols, ld)
    fx = RawFence(rows * ld, torch.int32, "x")
    fx.own(idx)
    xv = fx.flat.view(torch.float32).view(rows, ld)[:, :cols]
    xv.copy_(x)
    f16 = pv = None
    if out_mode != "fp32":
        f16 = RawFence(rows * ld, DTYPES[out_mode], "out16")
        f16.own(idx)
        pv = f16.flat.view(rows, ld)[:, :cols]
    eng.op_softmax_rows(xv, out16=pv)
    torch.cuda.synchronize()
    fx.check()
    if f16 is not None:
        f16.check()
    return xv.cpu(), (pv.float().cpu() if pv is not None else None)


@pytest.mark.parametrize("out_mode", vb.SOFTMAX_OUT)
@pytest.mark.parametrize("cols", vb.SOFTMAX_COLS)
def test_softmax_rows(eng, cols, out_mode):
    """fewer columns than a wave, one short of / exactly / one piece more than the 256 threads, two and nine passes; rows spanning +-3e4, a
    constant row, one dominant key, values that overflow without the maximum, every magnitude of the exponential."""
    ref, budget = softmax_ref(cols, out_mode)
    x_after, copy = softmax_run(eng, cols, out_mode)
    p = x_after if out_mode == "fp32" else copy
    assert not torch.isnan(p).any(), f"{int(torch.isnan(p).sum())} NaN in the probabilities"
    print()
    check_budget(f"softmax {cols} columns [{out_mode}]", p, ref["p"], budget)
    others = torch.ones(cols, dtype=torch.bool)
    others[max(cols - 2, 0)] = False
    if cols > 1:
        stray = float(p[vb.DOMINANT_ROW][others].abs().max())
        assert stray <= (vb.SPACING["fp16"] / 2 if out_mode == "fp16" else 0.0), f"a key 200 below the dominant one has probability {stray:.3e}"
    if out_mode == "fp32":
        sums = p.double().sum(-1)
        worst = float((sums - 1.0).abs().max())
        print(f"softmax {cols} columns: row sums within {worst:.3e} of 1 (allowed {cols * vb.U:.3e})")
        assert worst <= cols * vb.U, f"a row sums to 1 {worst:+.3e}, allowed {cols * vb.U:.3e}"
    else:                                                # x keeps the exponentials: none above 1, the maximum's exactly 1
        assert float(x_after.max()) == 1.0 and bool((x_after.amax(-1) == 1.0).all()) and float(x_after.min()) >= 0.0


def test_expf_ulp_is_within_the_constant(eng):
    """the measurement behind ``vae_attn_budget.EXPF_ULP``, repeated: the exponentials softmax_rows leaves next to a 16-bit copy against
    float64 exp of the same fp32 argument, over every softmax case.  Twice the observation must not exceed the constant."""
    worst, at = 0.0, None
    for cols in vb.SOFTMAX_COLS:
        e_dev, _ = softmax_run(eng, cols, "bf16")
        w, arg = vb.expf_ulps(e_dev, vb.softmax_inputs(cols))
        if w > worst:
            worst, at = w, (cols, arg)
    print(f"\nexpf: largest error {worst:.4f} ulp (at argument {at[1]:.6g}, {at[0]} columns); the budgets allow {vb.EXPF_ULP} ulp")
    assert vb.EXPF_ULP == max(2.0 * vb.EXPF_ULP_MEASURED, 2.0)
    assert 2.0 * worst <= vb.EXPF_ULP, f"expf is {worst:.3f} ulp off at {at}: EXPF_ULP = {vb.EXPF_ULP} is less than twice that"


# ------------------------------------------------------------------ the transpose alone
@pytest.mark.parametrize("two_byte", [False, True], ids=["4byte", "2byte"])
@pytest.mark.parametrize("rows,cols", vb.TRANSPOSE_SHAPES)
def test_transpose2d(eng, rows, cols, two_byte):
    """one ragged tile, a ragged second tile in each direction, nine row tiles, one element past a tile both ways; three matrices whose
    batch strides are larger than the matrices, padded row strides; every element bit for bit and nothing else written."""
    x = vb.transpose_inputs(rows, cols, two_byte)
    dtype, batch = x.dtype, vb.TRANSPOSE_BATCH
    ld_in, ld_out = cols + 4, rows + 6
    sb_in, sb_out = rows * ld_in + 24, cols * ld_out + 40
    fi = RawFence((batch - 1) * sb_in + rows * ld_in, dtype, "in")
    fo = RawFence((batch - 1) * sb_out + cols * ld_out, dtype, "out")
    src, dst = strided(rows, cols, ld_in, batch, sb_in), strided(cols, rows, ld_out, batch, sb_out)
    fi.own(src)
    fo.own(dst)
    fi.flat[src.cuda()] = x.reshape(-1).cuda()
    before = fi.words.clone()
    eng.op_transpose2d(fi.flat, fo.flat, rows=rows, cols=cols, batch=batch, ld_in=ld_in, ld_out=ld_out, sb_in=sb_in, sb_out=sb_out)
    torch.cuda.synchronize()
    fo.check()
    assert torch.equal(fi.words, before), "the input buffer changed"
    got = fo.flat[dst.cuda()].cpu().reshape(batch, cols, rows)
    want = vb.transpose_reference(x)
    diff = int((got != want).sum())
    assert diff == 0, f"transpose {rows} x {cols} ({'2' if two_byte else '4'}-byte): {diff} of {want.numel()} elements differ; first at {tuple(int(i) for i in (got != want).nonzero()[0])}"
