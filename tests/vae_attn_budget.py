"""Per-element budgets for the attention of the VAE mid block as ``Runner::vae_attention_core`` runs it -- a batched GEMM whose A and W are
column slices of the fused qkv rows (scores, scaled by ``alpha = C^-0.5``), ``softmax_rows``, ``transpose2d`` and a second batched GEMM
(``K = HW``, ``W = V^T``) -- and for the softmax and the transpose on their own.  Pure torch on the CPU, float64; no kernel is called from
here.  The sibling of ``tests/h16_budget.py`` (whose rounding helpers, ``MUTANT_FACTOR`` and 16-bit attention budget it uses), in the same
three parts: references, budgets, mutants, and the case table that ``tests/test_vae_attn_budget_host.py`` (no GPU: the budgets are
neither too tight for correct arithmetic nor too loose to see a wrong kernel) and ``tests/test_hip_vae_attention.py`` (the kernels)
both iterate over.

References.  ``mode`` is ``fp32``, ``bf16`` or ``fp16``.  The operands are rounded the way ``e2v_op_vae_attention_core`` rounds them (16-bit
modes: qkv to the type, once); ``alpha`` is the fp32 number the graph computes, ``1.0f / sqrtf((float)C)``; everything after that is
float64.  A reference returns its by-products: ``sum |q||k|`` per score, ``|s - m|`` per score (its largest per row is the
span of the row), ``sum p |v|`` per output.

Budgets.  ``U = 2^-24`` is the unit roundoff of fp32, ``u`` / ``h`` the unit roundoff and the smallest spacing of the 16-bit type
(``h16_budget.UNIT`` / ``SPACING``).  Every element has a bound, none is left out.

* scores (fp32 in every mode)::

      |s' - s| <= B_s = (C + 4) U alpha sum_k |q_k||k_k|  +  U |s|

  the project's linear bound (``tests/test_hip_igemm_dma.py``) at K = C, carried through the scale, plus one rounding of the
  multiplication by alpha.  In the 16-bit modes the products of the rounded operands are exact in fp32 and the sums are fp32: the same
  bound.

* softmax of a row x of ``cols`` columns, m its maximum, p = e / l, e_j = exp(x_j - m), l = sum_j e_j.  Relative error of p_i::

      r_i = U |x_i - m| + X            the rounding of x_i - m (an absolute error in the exponent is a relative one of e_i) and expf,
          + sum_j p_j (U |x_j - m| + X)    the same two per term of l, weighted as l weights them (never more than U max|x - m| + X),
          + cols U                     l itself: an fp32 sum of cols positive terms, in any order,
          + 3 U                        the reciprocal (one ulp = 2 U allowed) and the product.
      |p' - p| <= B_p = r p + 2^-126

  ``X = EXPF_ULP * 2 U`` (one ulp is at most 2 U relative).  2^-126: a result below the smallest normal fp32 number may be flushed or
  lose bits.  With a 16-bit copy the stored value is rounded once more, as ``h16_budget.gemm_budget`` writes it:
  ``B_p16 = B_p + max(u (p + B_p), h / 2)``.

  ``EXPF_ULP`` is the one number here that is not derived.  HIP's math-accuracy table is not among the files of a ROCm installation, so it
  was measured on an MI355X: the exponentials ``softmax_rows`` leaves in x when it writes a 16-bit copy, against ``exp`` in float64 of the
  SAME fp32 argument ``fl(x - m)``, in ulps of the float64 value, over every softmax case of the table below (arguments from 0 down to
  -6e4, results down to the smallest normal).  Measured: 0.7901 ulp, at the argument -3.20649 (256 columns).  The budget takes twice that
  and never less than 2 ulp, so 2 ulp;
  ``test_hip_vae_attention.py::test_expf_ulp_is_within_the_constant`` repeats the measurement and fails if twice the observation exceeds
  the constant.  It is never calibrated against the block's output.

* inside the block the softmax runs on the kernel's scores s' = s + d, |d| <= B_s: softmax(s + d)_i = p_i e^(d_i) / sum_j p_j e^(d_j), a
  relative change of at most ``expm1(B_s_i + sum_j p_j B_s_j)``; with r as above (evaluated with |s - m| + 2 max_j B_s_j for |x - m|)::

      B_p(block) = p ((1 + expm1(B_s_i + sum_j p_j B_s_j)) (1 + r_i) - 1) + 2^-126        (16-bit copy: + max(u (p + B_p), h / 2))

* block output, o = sum_j p_j v_j::

      fp32    B_o = (HW + 4) U (sum_j p_j |v_j| + sum_j B_p_j |v_j|)  +  sum_j B_p_j |v_j|
      16-bit  B_o = the same with the fp32 B_p (before the rounding of the copy)  +  4 max(u (sum_j p_j |v_j| + |o|), h / 2)

  the linear bound of the PV GEMM at K = HW on the probabilities it really reads, the error of those probabilities carried through the
  product, and in the 16-bit modes ``h16_budget.attention_budget`` for a 16-bit P and a 16-bit store.

* transpose: bit equality.

Mutants: the reference with one deliberate error -- ``drop_last_key`` (out of the sum and of the product), ``drop_last_stage`` (the last 16
keys out of the PV product only), ``next_image_k`` / ``next_image_v`` (image z + 1's K in the scores / V in the product), ``no_alpha``,
``alpha_1_over_C``, ``no_row_max`` (fp32 exponentials of the raw scores: overflow where a score exceeds 88.7), ``sum_first_256`` (the
normaliser over the first 256 columns only), ``transpose_swap`` (row and column swapped inside the ragged corner tile of the transpose).
A mutant is "seen" in an image or row when one of the quantities the GPU test checks there -- scores, probabilities, output -- is at least
``MUTANT_FACTOR`` times over its budget.  Sentinels make that hold: the V rows of the keys at the stage and tile edges are 16 x, the K rows
of the last eight keys 3 x (so the columns past 256 carry weight), and the ``offset`` case adds a common component to q and k that lifts
every score by about 112 -- softmax does not change, a kernel that forgot the maximum overflows.
"""
import math

import torch

from h16_budget import MUTANT_FACTOR, SPACING, TYPES, UNIT, attention_budget, rnd, rt      # noqa: F401  (re-exported to the two test files)

U = 2.0 ** -24
TINY = 2.0 ** -126
EXPF_ULP_MEASURED = 0.7901        # ulp, measured on an MI355X (see above)
EXPF_ULP = max(2.0 * EXPF_ULP_MEASURED, 2.0)
MODES = ["fp32", "bf16", "fp16"]
EXP_OVERFLOW = 88.72              # expf overflows above log(FLT_MAX) = 88.7228


def rounded(t, mode):
    return t.float() if mode == "fp32" else rt(t, mode)


def alpha_of(C):
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(torch.tensor(float(C), dtype=torch.float32)))


# ---------------------------------------------------------------------------------------------------------------- softmax
def softmax_reference(x, mutant=None):
    """``x``: ``[..., cols]``.  Returns p, e (the exponentials), ``dist`` = |x - m| per element, all float64.  ``mutant``: None,
    ("no_row_max",) or ("sum_first_256",)."""
    x = x.double()
    m = x.amax(-1, keepdim=True)
    kind = mutant[0] if mutant else None
    if kind == "no_row_max":                             # fp32 exponentials of the raw values, as a kernel without the maximum would
        e = torch.exp(x.float()).double()
        l = e.sum(-1, keepdim=True).float().double()
        return {"p": e / l, "e": e, "dist": (x - m).abs()}
    e = torch.exp(x - m)
    if kind == "sum_first_256":
        l = e[..., :256].sum(-1, keepdim=True)
    elif kind is None:
        l = e.sum(-1, keepdim=True)
    else:
        raise ValueError(mutant)
    return {"p": e / l, "e": e, "dist": (x - m).abs()}


def softmax_rel(p, dist, cols, extra_dist=0.0):
    """r of the module docstring, per element"""
    x_term = U * (dist + extra_dist) + EXPF_ULP * 2.0 * U
    return x_term + (p * x_term).sum(-1, keepdim=True) + (cols + 3.0) * U


def store16(value, budget, mode):
    """one more rounding, to the 16-bit type of ``mode``, of a value that is itself ``budget`` off"""
    if mode == "fp32":
        return budget
    return budget + torch.clamp(UNIT[mode] * (value.abs() + budget), min=SPACING[mode] / 2)


def softmax_budget(ref, out_mode):
    """``ref``: softmax_reference(x); ``out_mode``: "fp32" (in place) or the type of the 16-bit copy"""
    p = ref["p"]
    b32 = softmax_rel(p, ref["dist"], p.shape[-1]) * p + TINY
    return store16(p, b32, out_mode)


def softmax_emulation(x, out_mode):
    """the kernel's arithmetic in fp32 torch: maximum, exp(x - m), the sum, one reciprocal, the product, the rounding of the copy"""
    x = x.float()
    e = torch.exp(x - x.amax(-1, keepdim=True))
    p = e * (1.0 / e.sum(-1, keepdim=True))
    return (p if out_mode == "fp32" else rt(p, out_mode)).double()


def expf_ulps(e_dev, x):
    """Error of the device's exponentials ``e_dev`` (what softmax_rows leaves in x next to a 16-bit copy) in ulps of the float64 value of
    exp at the SAME fp32 argument fl(x - m), over the results that are normal fp32 numbers.  Returns (largest ulp error, its argument)."""
    x = x.float()
    d = (x - x.amax(-1, keepdim=True))                   # the fp32 subtraction the kernel makes
    want = torch.exp(d.double())
    ok = want >= TINY
    ulp = torch.exp2(torch.floor(torch.log2(want.clamp(min=TINY))) - 23.0)
    err = ((e_dev.double() - want).abs() / ulp) * ok
    i = int(err.argmax())
    return float(err.flatten()[i]), float(d.flatten()[i])


# ---------------------------------------------------------------------------------------------------------------- transpose
def corner_tile(rows, cols):
    """(r0, c0) of the last 32 x 32 tile in both directions, or None when it is not ragged"""
    r0, c0 = (rows - 1) // 32 * 32, (cols - 1) // 32 * 32
    return (r0, c0) if (rows % 32 or cols % 32) else None


def swap_extent(rows, cols):
    """side of the square inside the ragged corner tile whose elements can change places (0: no ragged corner tile)"""
    return min(rows - (rows - 1) // 32 * 32, cols - (cols - 1) // 32 * 32) if corner_tile(rows, cols) else 0


def transpose_reference(x, mutant=None):
    """``x``: ``[batch, rows, cols]`` of any dtype -> ``[batch, cols, rows]``.  ``mutant``: ("transpose_swap",): inside the ragged corner tile
    element (r0 + i, c0 + j) is read from (r0 + j, c0 + i) wherever that lies inside the matrix."""
    if mutant is None:
        return x.transpose(1, 2).contiguous()
    assert mutant[0] == "transpose_swap"
    _, rows, cols = x.shape
    r0, c0 = corner_tile(rows, cols)
    src = x.clone()
    n = swap_extent(rows, cols)                          # (r0 + j < rows and c0 + i < cols for i, j < n)
    src[:, r0:r0 + n, c0:c0 + n] = x[:, r0:r0 + n, c0:c0 + n].transpose(1, 2)
    return src.transpose(1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------- the block
BLOCK_MUTANTS = ["drop_last_key", "drop_last_stage", "next_image_k", "next_image_v", "no_alpha", "alpha_1_over_C", "no_row_max",
                 "sum_first_256", "transpose_swap"]


def block_reference(qkv, *, nimg, HW, C, mode, mutant=None, emulate=False):
    """``qkv``: ``[nimg * HW, 3 C]`` fp32 as the entry takes it.  Returns s (scaled scores), p, o and the by-products sqk = alpha sum |q||k|,
    dist = |s - m|, pv = sum p |v| (float64; ``[nimg * HW, HW]`` and ``[nimg * HW, C]``), and ``touched``: the images a mutant changes.
    ``emulate``: the kernels' arithmetic in fp32 torch instead (fp32 GEMMs and softmax, P and o rounded to the type in 16-bit modes)."""
    t = rounded(qkv, mode).reshape(nimg, HW, 3 * C)
    dt = torch.float32 if emulate else torch.float64
    q, k, v = (t[..., i * C:(i + 1) * C].to(dt) for i in range(3))
    alpha = alpha_of(C)
    kind = mutant[0] if mutant else None
    assert kind is None or kind in BLOCK_MUTANTS, mutant
    touched = list(range(nimg))
    ks, vs = k, v
    if kind in ("next_image_k", "next_image_v"):
        touched = list(range(nimg - 1))
        nxt = list(range(1, nimg)) + [nimg - 1]          # (the last image has no neighbour: it keeps its own)
        ks, vs = (k[nxt] if kind == "next_image_k" else k), (v[nxt] if kind == "next_image_v" else v)
    if kind == "transpose_swap":                        # V^T built by the wrong transpose: [nimg, C, HW] back to [nimg, HW, C]
        vs = transpose_reference(v, mutant).transpose(1, 2)
    a = {"no_alpha": 1.0, "alpha_1_over_C": 1.0 / C}.get(kind, alpha)
    raw = q @ ks.transpose(1, 2)
    s = raw * a
    sqk = (q.abs() @ ks.abs().transpose(1, 2)) * a
    if emulate:
        p = softmax_emulation(s, mode).float()
        o = p @ vs
        return {"s": s.double().reshape(nimg * HW, HW), "p": p.double().reshape(nimg * HW, HW),
                "o": (o if mode == "fp32" else rt(o, mode)).double().reshape(nimg * HW, C)}
    sm_mut = mutant if kind in ("no_row_max", "sum_first_256") else None
    if kind == "drop_last_key":
        sm = softmax_reference(s[..., :-1])
        p = torch.cat([sm["p"], torch.zeros(nimg, HW, 1, dtype=dt)], -1)
        dist = torch.cat([sm["dist"], torch.zeros(nimg, HW, 1, dtype=dt)], -1)
    else:
        sm = softmax_reference(s, sm_mut)
        p, dist = sm["p"], sm["dist"]
    if kind == "no_row_max":                            # only the rows whose exponentials overflow differ
        over = (s.amax(-1) > EXP_OVERFLOW).any(-1)
        touched = [z for z in range(nimg) if bool(over[z])]
    pp = p
    if kind == "drop_last_stage":
        pp = p.clone()
        pp[..., -16:] = 0.0
    o = pp @ vs
    flat = lambda x: x.reshape(nimg * HW, x.shape[-1])
    return {"s": flat(s), "p": flat(p), "o": flat(o), "sqk": flat(sqk), "dist": flat(dist), "pv": flat(pp @ vs.abs()), "touched": touched,
            "v_abs": vs.abs()}


def block_budgets(ref, *, nimg, HW, C, mode):
    """(B_s, B_p, B_o) of the module docstring for ``ref`` = block_reference(...)"""
    s, p, o = ref["s"], ref["p"], ref["o"]
    b_s = (C + 4) * U * ref["sqk"] + U * s.abs()
    carried = torch.expm1(b_s + (p * b_s).sum(-1, keepdim=True))
    r = softmax_rel(p, ref["dist"], HW, extra_dist=2.0 * b_s.amax(-1, keepdim=True))
    b_p32 = p * ((1.0 + carried) * (1.0 + r) - 1.0) + TINY
    b_p = store16(p, b_p32, mode)
    through = (b_p32.reshape(nimg, HW, HW) @ ref["v_abs"]).reshape(nimg * HW, C)
    b_o = (HW + 4) * U * (ref["pv"] + through) + through
    if mode != "fp32":
        b_o = b_o + attention_budget({"pv": ref["pv"], "ref": o}, mode)
    return b_s, b_p, b_o


def applicable(mutant, *, nimg, HW, C, ref):
    kind = mutant[0]
    if kind in ("next_image_k", "next_image_v"):
        return nimg > 1
    if kind == "drop_last_stage":
        return HW > 16
    if kind == "drop_last_key":
        return HW > 1
    if kind == "sum_first_256":
        return HW > 256
    if kind == "no_row_max":
        return bool((ref["s"].amax(-1) > EXP_OVERFLOW).any())
    if kind == "transpose_swap":
        return swap_extent(HW, C) > 1
    return True


def ratio(y, ref, budget):
    """|y - ref| / budget with every non-finite value counted as infinitely wrong"""
    return torch.nan_to_num((y.double() - ref).abs() / budget, nan=math.inf, posinf=math.inf)


# ---------------------------------------------------------------------------------------------------------------- cases
SENTINEL_KEYS = (0, 15, 16, 127, 128, 255, 256, -16, -1)       # stage (16 k) and tile (128, 256) edges, the first key of the last stage


def _case(HW, C, nimg, modes=MODES, offset=False):
    return dict(id=f"hw{HW}_c{C}_n{nimg}" + ("_offset" if offset else ""), HW=HW, C=C, nimg=nimg, modes=list(modes), offset=offset)


# HW: 4 fewer columns than a wave; 24 the tiny VAE's; 132 a second row block of 4 rows, a wide + a ragged narrow column tile, K ending in
# a one-chunk stage; 260 (fp32) a third, 4-row row block and two wide + a ragged narrow column tile; 264 (16-bit: K = 4 * 64 + 8).
# C: 40 (2.5 stages, a ragged transpose tile), 64 (the tiny VAE), 512 (the real width).  16-bit modes take HW % 8 == 0 only.
BLOCK_CASES = [
    _case(4, 64, 3, ["fp32"]),
    _case(24, 40, 3), _case(24, 64, 1), _case(24, 64, 3), _case(24, 512, 1), _case(24, 512, 3),
    _case(24, 64, 3, offset=True),
    _case(132, 64, 1, ["fp32"]), _case(132, 64, 3, ["fp32"]),
    _case(260, 64, 1, ["fp32"]), _case(260, 64, 3, ["fp32"]),
    _case(264, 64, 1), _case(264, 64, 3),
]
REFUSED_16BIT = [(4, 64), (132, 64), (260, 64)]                 # HW % 8 != 0: the entry refuses what the graph refuses
REFUSED_FP32 = [(6, 64), (130, 64)]                             # HW % 4 != 0


def block_inputs(case):
    """qkv ``[nimg * HW, 3 C]``.  q and k are scaled so that a score is about N(0, 1.5^2) at every width; sentinels: V rows of SENTINEL_KEYS
    16 x, K rows of the last eight keys 3 x; ``offset``: 30 added to column 0 of q and of k (every score + 900 alpha)."""
    HW, C, nimg = case["HW"], case["C"], case["nimg"]
    seed = 7000 + 13 * HW + C + 1000 * nimg + (5 if case["offset"] else 0)
    qkv = rnd(nimg, HW, 3 * C, seed=seed)
    qkv[..., :2 * C] *= 1.5 ** 0.5                       # (alpha q . k of N(0, a^2) entries has deviation a^2)
    keys = sorted({j % HW for j in SENTINEL_KEYS if -HW <= j < HW})
    qkv[:, keys, 2 * C:] *= 16.0
    qkv[:, max(HW - 8, 0):, C:2 * C] *= 3.0
    if case["offset"]:
        qkv[..., 0] += 30.0
        qkv[..., C] += 30.0
    return qkv.reshape(nimg * HW, 3 * C).contiguous()


SOFTMAX_COLS = [4, 252, 256, 260, 516, 2304]
SOFTMAX_OUT = ["fp32", "bf16", "fp16"]


def softmax_inputs(cols):
    """``[7, cols]``: 0 N(0, 2^2); 1 spanning +-3e4; 2 constant; 3 one dominant key (column cols - 2 is 200 above the rest); 4 N(0, 1) + 100
    (nothing survives without the maximum); 5 a ramp 0 .. -100 (every magnitude of the exponential, down to the subnormals); 6 large
    values at the far end (the columns past 256 carry the weight)."""
    x = torch.empty(7, cols)
    x[0] = rnd(cols, seed=900 + cols) * 2.0
    x[1] = torch.linspace(-3.0e4, 3.0e4, cols)[torch.randperm(cols, generator=torch.Generator().manual_seed(cols))]
    x[2] = 1.25
    x[3] = rnd(cols, seed=901 + cols)
    x[3, max(cols - 2, 0)] += 200.0
    x[4] = rnd(cols, seed=902 + cols) + 100.0
    x[5] = torch.linspace(0.0, -100.0, cols)
    x[6] = rnd(cols, seed=903 + cols)
    x[6, -min(4, cols):] += 3.0
    return x


DOMINANT_ROW, CONSTANT_ROW = 3, 2
TRANSPOSE_SHAPES = [(4, 40), (36, 64), (260, 40), (33, 33)]     # (rows, cols)
TRANSPOSE_BATCH = 3


def transpose_inputs(rows, cols, two_byte):
    """``[3, rows, cols]`` of distinct bit patterns: int32 counting from 1, or int16"""
    n = TRANSPOSE_BATCH * rows * cols
    base = torch.arange(1, n + 1, dtype=torch.int64)
    return (base % 65521 - 32760).to(torch.int16).reshape(TRANSPOSE_BATCH, rows, cols) if two_byte else \
        (base * 2654435761 % 2147483629).to(torch.int32).reshape(TRANSPOSE_BATCH, rows, cols)
