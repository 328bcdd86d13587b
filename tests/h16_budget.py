"""Per-element rounding budgets for the ops of the 16-bit modes whose output is stored in 16 bits: GroupNorm, LayerNorm, sparse-causal,
cross and temporal attention and -- in a section of its own at the end, with its own references, budget, mutants and case table -- the
GEMM-shaped ops (linear, GEGLU, 3x3 conv, split-K, sub-pixel conv, two-source linear) as the graph launches them.  Pure torch on the
CPU, float64; no kernel is called from here.

What is here, and who uses it:

* references -- every operand rounded the way the kernels round it (rows to the stored type once; for sparse-causal and cross
  attention Q times ``scale * log2(e)`` rounded once more, as the kernels fold it; the temporal kernels scale the fp32 score instead),
  everything after that in float64.  A reference returns the result and the by-products its budget needs;
* budgets -- ``u`` is the unit roundoff of the stored type (2^-8 bf16, 2^-11 fp16), ``h`` its smallest spacing (the subnormal step:
  a rounding never costs less than h / 2, which matters for fp16 outputs below 6.1e-5 and is nothing otherwise):

    norms      |y - ref| <= 2 max(u |ref|, h/2) + DELTA |gamma| (|xhat| + |mu| / sqrt(var + eps) + 1)
               two roundings of the output (the store, and one more: the row-tiled apply evaluates SiLU through exp2 / rcp) plus the
               effect of fp32 statistics: DELTA = 2e-5 is the suite's fp32 summation-order tolerance (RTOL of test_hip_ops.py), a
               relative error of that size in 1/sqrt(var + eps) moves y by |gamma xhat|, in mu by |gamma| |mu| / sqrt(var + eps), and the
               affine itself (two fp32 roundings of scale and shift) by the 1.
    attention  |o - ref| <= 4 max(u (sum_j p_j |v_j| + |ref|), h/2)
               P rounded in the numerator (u sum p|v|), the same rounded P in the normaliser (u |ref|... bounded by u sum p|v|), the
               output rounded (u |ref|), and one more u (sum p|v| + |ref|) for fp32 accumulation and the hardware exp2;

* ``assert_within_budget`` -- every element, none left out, and a failure says where the worst one lies;
* mutants -- the same references with one deliberate error (a row or key lost, a neighbour's counted, a wrong count, a wrong
  source).  ``tests/test_h16_budget_host.py`` holds every case to: a torch emulation of the kernels' arithmetic stays within the
  budget, and every mutant that applies exceeds it at least ``MUTANT_FACTOR`` times in every slab / row / frame it touches.  That is a
  condition on the INPUTS of a case (sentinel rows and keys make it hold), checked without a GPU; ``tests/test_hip_h16_budget.py``
  then runs the same cases through the kernels;
* the case table both files iterate over.
"""
import math

import torch

LOG2E = 1.4426950408889634
DELTA = 2e-5                      # fp32 statistics: the suite's summation-order tolerance (tests/test_hip_ops.py RTOL)
MUTANT_FACTOR = 4.0               # a mutant has to exceed the budget this many times where it acts
TYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
UNIT = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
SPACING = {"bf16": 2.0 ** -133, "fp16": 2.0 ** -24}


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def rt(t, ty):
    """Round an fp32 tensor to the stored type of mode ``ty`` (round to nearest even, as the entry points convert), back as fp32."""
    return t.float().to(TYPES[ty]).float()


def _silu(z):
    return z * torch.sigmoid(z)


# ---------------------------------------------------------------------------------------------------------------- norms
def norm_budget(out, gamma, ty):
    u, h = UNIT[ty], SPACING[ty]
    ref = out["ref"]
    return 2.0 * torch.clamp(u * ref.abs(), min=h / 2) + DELTA * gamma.double().abs() * (out["xhat"].abs() + out["mu"].abs() * out["rstd"] + 1.0)


def groupnorm_reference(x, gamma, beta, *, samples, P, groups, c0, eps=1e-5, silu=False, mutant=None):
    """``x``: ``[samples * P, C]`` rows (both sources side by side, already rounded), statistics per (sample, group) over P rows x C / groups
    channels.  ``mutant``: None, ("drop_row", r), ("next_sample_row",), ("var_n_minus_1",) or ("seam_one_source",) -- a lost or foreign
    row changes the sums and leaves the count alone, as a kernel with a wrong loop bound would.  Returns ref, xhat, mu, rstd (each
    ``[samples * P, C]``) and ``touched``: the samples whose statistics the mutant changes."""
    x, ga, be = x.double(), gamma.double(), beta.double()
    C = x.shape[1]
    cpg = C // groups
    N = cpg * P
    xg = x.reshape(samples, P, groups, cpg)
    s1, s2, cnt = xg.sum((1, 3)), (xg * xg).sum((1, 3)), torch.full((samples, groups), float(N), dtype=torch.float64)
    touched = list(range(samples))
    kind = mutant[0] if mutant else None
    if kind == "drop_row":
        r = mutant[1]
        s1, s2 = s1 - xg[:, r].sum(-1), s2 - (xg[:, r] ** 2).sum(-1)
    elif kind == "next_sample_row":
        s1, s2 = s1.clone(), s2.clone()
        s1[:-1] += xg[1:, 0].sum(-1)
        s2[:-1] += (xg[1:, 0] ** 2).sum(-1)
        touched = list(range(samples - 1))
    elif kind == "seam_one_source":
        gs = c0 // cpg
        assert 0 < c0 - gs * cpg < cpg, "no group straddles the seam"
        part = xg[:, :, gs, :c0 - gs * cpg]
        s1, s2, cnt = s1.clone(), s2.clone(), cnt.clone()
        s1[:, gs], s2[:, gs], cnt[:, gs] = part.sum((1, 2)), (part * part).sum((1, 2)), float((c0 - gs * cpg) * P)
    mean = s1 / cnt
    var = torch.clamp(s2 / cnt - mean * mean, min=0.0)
    if kind == "var_n_minus_1":
        var = var * (N / (N - 1.0))
    elif kind not in (None, "drop_row", "next_sample_row", "seam_one_source"):
        raise ValueError(mutant)
    rstd = 1.0 / torch.sqrt(var + eps)
    full = lambda t: t[:, None, :, None].expand(samples, P, groups, cpg).reshape(samples * P, C)
    mu, rs = full(mean), full(rstd)
    xhat = (x - mu) * rs
    z = xhat * ga + be
    return {"ref": _silu(z) if silu else z, "xhat": xhat, "mu": mu, "rstd": rs, "touched": touched}


def groupnorm_emulation(x, gamma, beta, ty, *, samples, P, groups, eps=1e-5, silu=False):
    """The kernels' arithmetic in torch: fp32 sums of x and x^2, the fold (mean, E[x^2] - mean^2, 1 / sqrt) in fp64, scale and shift rounded
    to fp32, the affine and SiLU in fp32, the output rounded to the type."""
    x = x.float()
    C = x.shape[1]
    cpg = C // groups
    xg = x.reshape(samples, P, groups, cpg)
    s1, s2 = xg.sum((1, 3)).double(), (xg * xg).sum((1, 3)).double()
    mean = s1 / (cpg * P)
    rstd = 1.0 / torch.sqrt(torch.clamp(s2 / (cpg * P) - mean * mean, min=0.0) + eps)
    full = lambda t: t[:, None, :, None].expand(samples, P, groups, cpg).reshape(samples * P, C)
    scale = (full(rstd) * gamma.double()).float()
    shift = (beta.double() - full(mean * rstd) * gamma.double()).float()
    z = x * scale + shift
    return rt(_silu(z) if silu else z, ty).double()


def layernorm_reference(x, gamma, beta, eps=1e-5, mutant=None):
    """``x``: ``[rows, C]`` rounded rows.  ``mutant``: None or ("drop_piece", k): columns 8k .. 8k + 7 (what one lane loads at a time) are
    left out of every row's sums, the count stays C."""
    x, ga, be = x.double(), gamma.double(), beta.double()
    rows, C = x.shape
    xs = x
    if mutant:
        assert mutant[0] == "drop_piece"
        xs = x.clone()
        xs[:, 8 * mutant[1]:8 * mutant[1] + 8] = 0.0
    mean = xs.sum(-1, keepdim=True) / C
    var = torch.clamp((xs * xs).sum(-1, keepdim=True) / C - mean * mean, min=0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    return {"ref": xhat * ga + be, "xhat": xhat, "mu": mean.expand(rows, C), "rstd": rstd.expand(rows, C), "touched": list(range(rows))}


def layernorm_emulation(x, gamma, beta, ty, eps=1e-5):
    """Two passes in fp32 (mean, then the squares of x - mean), rsqrt, affine, one rounding."""
    x = x.float()
    mean = x.sum(-1, keepdim=True) / x.shape[1]
    d = x - mean
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) / x.shape[1] + eps)
    return rt(d * rstd * gamma.float() + beta.float(), ty).double()


# ---------------------------------------------------------------------------------------------------------------- attention
def attention_budget(out, ty):
    return 4.0 * torch.clamp(UNIT[ty] * (out["pv"] + out["ref"].abs()), min=SPACING[ty] / 2)


def _split_heads(t, heads):       # [..., rows, heads * d] -> [..., heads, rows, d]
    *lead, rows, c = t.shape
    return t.reshape(*lead, rows, heads, c // heads).transpose(-2, -3)


def _merge_heads(t):              # [..., heads, rows, d] -> [..., rows, heads * d]
    t = t.transpose(-2, -3)
    return t.reshape(*t.shape[:-2], t.shape[-2] * t.shape[-1])


def _attend(q2, k, v, mask=None, emulate=None):
    """softmax in the exp2 domain: ``q2`` carries scale * log2(e).  ``mask``: True where a (query, key) pair is left out.  ``emulate``: a
    type name -- fp32 scores and exp2, P rounded to the type for the numerator AND the normaliser, fp32 accumulation, output rounded."""
    dt = torch.float32 if emulate else torch.float64
    q2, k, v = q2.to(dt), k.to(dt), v.to(dt)
    s = q2 @ k.transpose(-1, -2)
    if mask is not None:
        s = s.masked_fill(mask, -math.inf)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    if emulate:
        p = rt(p, emulate)
        return rt((p @ v) / p.sum(-1, keepdim=True), emulate).double(), None
    p = p / p.sum(-1, keepdim=True)
    return p @ v, p @ v.abs()


def _fold_q(q, scale, ty):
    """Q as the MFMA kernels hold it: the rounded row times scale * log2(e) in fp32, rounded to the type once more."""
    return rt(rt(q, ty) * (scale * LOG2E), ty)


def sparse_causal_reference(q, k, v, *, n, F, heads, Nq, scale, ty, mutant=None, emulate=False):
    """``q, k, v``: ``[n * F * Nq, heads * d]`` fp32 as the op takes them; keys of frame f = [frame 0 ; frame max(f - 1, 0)].  ``mutant``:
    ("drop_key", j) -- key j of the 2 Nq is lost for every query; ("drop_key_last_block", j, qb) -- only for the queries of the last
    (ragged) block of qb; ("second_segment_own_frame",) -- the second segment comes from frame f; ("next_frame_key",) -- the row after
    the second segment (key 0 of frame max(f - 1, 0) + 1) is counted in."""
    c = q.shape[1]
    q2 = _split_heads(_fold_q(q, scale, ty).reshape(n, F, Nq, c), heads)
    kk, vv = rt(k, ty).reshape(n, F, Nq, c), rt(v, ty).reshape(n, F, Nq, c)
    former = (torch.arange(F) - 1).clamp(min=0)
    kind = mutant[0] if mutant else None
    frames = list(range(F))
    if kind == "second_segment_own_frame":             # (frame 0 is its own predecessor: nothing changes there)
        former = torch.arange(F)
        frames = list(range(1, F))
    parts = lambda t: [t[:, [0] * F], t[:, former]]
    kp, vp = parts(kk), parts(vv)
    if kind == "next_frame_key":
        nxt = (torch.arange(F) - 1).clamp(min=0) + 1
        kp.append(kk[:, nxt, :1])
        vp.append(vv[:, nxt, :1])
    kg, vg = _split_heads(torch.cat(kp, 2), heads), _split_heads(torch.cat(vp, 2), heads)
    mask, row_mask = None, None
    if kind in ("drop_key", "drop_key_last_block"):
        mask = torch.zeros(Nq, kg.shape[-2], dtype=torch.bool)
        q0 = 0 if kind == "drop_key" else (Nq - 1) // mutant[2] * mutant[2]
        mask[q0:, mutant[1]] = True
        row_mask = (torch.arange(Nq) >= q0).repeat(n * F)
    elif kind not in (None, "second_segment_own_frame", "next_frame_key"):
        raise ValueError(mutant)
    o, pv = _attend(q2, kg, vg, mask, ty if emulate else None)
    flat = lambda t: _merge_heads(t).reshape(n * F * Nq, c)
    return {"ref": flat(o), "pv": flat(pv) if pv is not None else None, "touched": [s * F + f for s in range(n) for f in frames],
            "row_mask": row_mask}


def cross_reference(q, k, v, *, n, F, heads, Nq, Nk, scale, ty, mutant=None, emulate=False):
    """``q``: ``[n * F * Nq, c]``, ``k, v``: ``[n * Nk, c]`` (one conditioning per sample, shared by its frames).  ``mutant``: ("drop_key", j);
    ("drop_key_last_block", j, qb): only for the last (ragged) block of qb of a sample's F * Nq query rows; ("next_sample_key",): key 0
    of the next sample is counted in (samples before the last)."""
    c = q.shape[1]
    q2 = _split_heads(_fold_q(q, scale, ty).reshape(n, F * Nq, c), heads)
    kk, vv = rt(k, ty).reshape(n, Nk, c), rt(v, ty).reshape(n, Nk, c)
    kind = mutant[0] if mutant else None
    touched, row_mask = list(range(n * F)), None
    if kind == "next_sample_key":
        kk = torch.cat([kk, torch.cat([kk[1:, :1], torch.zeros(1, 1, c)])], 1)
        vv = torch.cat([vv, torch.cat([vv[1:, :1], torch.zeros(1, 1, c)])], 1)
        touched = list(range((n - 1) * F))
    mask = None
    if kind in ("drop_key", "drop_key_last_block"):
        mask = torch.zeros(F * Nq, kk.shape[1], dtype=torch.bool)
        q0 = 0 if kind == "drop_key" else (F * Nq - 1) // mutant[2] * mutant[2]
        mask[q0:, mutant[1]] = True
        row_mask = (torch.arange(F * Nq) >= q0).repeat(n)
        touched = sorted({s * F + r // Nq for s in range(n) for r in range(q0, F * Nq)})
    elif kind not in (None, "next_sample_key"):
        raise ValueError(mutant)
    if kind == "next_sample_key":              # the last sample has no neighbour: its appended key is masked out
        mask = torch.zeros(n, 1, F * Nq, Nk + 1, dtype=torch.bool)
        mask[-1, :, :, Nk] = True
    o, pv = _attend(q2, _split_heads(kk, heads), _split_heads(vv, heads), mask, ty if emulate else None)
    flat = lambda t: _merge_heads(t).reshape(n * F * Nq, c)
    return {"ref": flat(o), "pv": flat(pv) if pv is not None else None, "touched": touched, "row_mask": row_mask}


def temporal_reference(qkv, *, n, F, HW, heads, scale, ty, mutant=None, emulate=False):
    """``qkv``: ``[n * F * HW, 3 c]``; every pixel attends over its F frames ('(b f) d c -> (b d) f c').  The temporal kernels keep Q as
    stored and scale the fp32 score.  ``mutant``: ("drop_key", j): frame j is lost as a key for every query."""
    c = qkv.shape[1] // 3
    t = rt(qkv, ty).double().reshape(n, F, HW, 3 * c).transpose(1, 2)                 # [n, HW, F, 3c]
    q, k, v = (_split_heads(t[..., i * c:(i + 1) * c], heads) for i in range(3))
    mask = None
    if mutant:
        assert mutant[0] == "drop_key"
        mask = torch.zeros(F, F, dtype=torch.bool)
        mask[:, mutant[1]] = True
    q2 = (q.float() * (scale * LOG2E)) if emulate else q * (scale * LOG2E)
    o, pv = _attend(q2, k, v, mask, ty if emulate else None)
    flat = lambda t_: _merge_heads(t_).transpose(1, 2).reshape(n * F * HW, c)
    return {"ref": flat(o), "pv": flat(pv) if pv is not None else None, "touched": list(range(n * F)), "row_mask": None}


# ---------------------------------------------------------------------------------------------------------------- the check
def ratios(y, ref, budget):
    return (y.detach().cpu().double() - ref).abs() / budget


def group_max(ratio, group_rows, row_mask=None):
    """Largest ratio per group of ``group_rows`` consecutive rows (a slab, a row, a frame), over the rows of ``row_mask`` if given."""
    if row_mask is not None:
        ratio = ratio * row_mask[:, None]
    return ratio.reshape(-1, group_rows, ratio.shape[-1]).amax((1, 2))


def assert_within_budget(y, ref, budget, what, where=None):
    """Every element of ``y`` within ``budget`` of ``ref``; returns the largest ratio error / budget.  ``where(row, col)`` names the
    slab / frame / head / block of an element for the failure message."""
    y = y.detach().cpu().double()
    assert y.shape == ref.shape == budget.shape, f"{what}: shapes {tuple(y.shape)}, {tuple(ref.shape)}, {tuple(budget.shape)}"
    bad = ~torch.isfinite(y)
    if bad.any():
        r, c = (int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} non-finite outputs, the first at [{r}, {c}]" + (f" ({where(r, c)})" if where else ""))
    ratio = (y - ref).abs() / budget
    worst = float(ratio.max())
    if worst > 1.0:
        r, c = divmod(int(ratio.argmax()), ratio.shape[1])
        over = ratio > 1.0
        rows_over = over.any(1).nonzero().flatten()
        raise AssertionError(
            f"{what}: {int(over.sum())} of {ratio.numel()} elements over budget; worst [{r}, {c}]" + (f" ({where(r, c)})" if where else "") +
            f": got {float(y[r, c]):.6g}, reference {float(ref[r, c]):.6g}, |error| {float((y - ref)[r, c].abs()):.3e} = {worst:.1f} x budget "
            f"{float(budget[r, c]):.3e}; rows over budget: {int(rows_over[0])} .. {int(rows_over[-1])} ({len(rows_over)} rows)")
    return worst


def where_groupnorm(case):
    P, cpg = case["P"], (case["c0"] + case["c1"]) // case["groups"]
    return lambda r, c: (f"sample {r // P}, row {r % P} of {P} (64-row chunk {r % P // 64}), channel {c} = group {c // cpg}"
                         + (", source 1" if c >= case["c0"] else ""))


def where_layernorm(case):
    return lambda r, c: f"row {r} of {case['rows']}, column {c} (piece {c // 8})"


def where_attention(case):
    d, nq, f = case["d"], case["nq"], case["f"]
    return lambda r, c: (f"sample {r // (f * nq)}, frame {r // nq % f}, query {r % nq} of {nq} (32-query block {r % nq // 32}, "
                         f"64-query block {r % nq // 64}), head {c // d}, column {c % d}")


def where_temporal(case):
    d, hw, f = case["d"], case["hw"], case["f"]
    return lambda r, c: f"sample {r // (f * hw)}, frame {r // hw % f}, pixel {r % hw} of {hw}, head {c // d}, column {c % d}"


# ---------------------------------------------------------------------------------------------------------------- cases
SENTINEL_ROWS = (0, 63, 64, -1)                      # of a slab: the edges of the 64-row chunks
SENTINEL_KEYS = (0, 31, 32, 63, 64, -1)              # of a frame's keys: the edges of the 32- and 64-key stages
GN_FORMS = [{}, {"E2V_GN_FUSED_SMALL": 2}]
GN_FORMS_AB = [{"E2V_GN_ROWS": 0}, {"E2V_GN_COOP": 2}]
GN_DEFAULTS = {"E2V_GN_FUSED_SMALL": 1, "E2V_GN_ROWS": 1, "E2V_GN_COOP": 0}

GN_CASES = [
    dict(id="seam_cpg12", samples=3, P=50, c0=64, c1=32, groups=8, silu=True),          # group 5 straddles the seam
    dict(id="odd_pieces", samples=3, P=45, c0=80, c1=0, groups=8, silu=True),
    dict(id="two_chunks_plus_2", samples=2, P=130, c0=320, c1=0, groups=32, silu=False),
    dict(id="one_chunk", samples=2, P=64, c0=128, c1=0, groups=32, silu=True),
    dict(id="real_seam_cpg60", samples=2, P=240, c0=1280, c1=640, groups=32, silu=True),
    dict(id="constant_group", samples=3, P=50, c0=64, c1=32, groups=8, silu=True, constant_group=2),
    # one source of each kind: 8-channel statistics for 64, 4-channel for 36 and for the 100-wide apply pass; group 6 straddles the seam
    # (c0 = 60, c1 = 36, groups = 8 -- 4 channels per lane on both sources -- is in tests/test_hip_ops.py: with no seam group and
    # 12 x 70 values per group its variance-over-N-1 mutant reaches 3.9 x this budget in bf16, short of MUTANT_FACTOR)
    dict(id="mixed_alignment", samples=2, P=70, c0=64, c1=36, groups=10, silu=True),
]


def gn_sentinel_group(case):
    cpg = (case["c0"] + case["c1"]) // case["groups"]
    return case["c0"] // cpg if case["c1"] and case["c0"] % cpg else 1


def gn_inputs(case):
    """fp32 rows of the two sources, gamma, beta.  Sentinels: rows 0, 63, 64 and P - 1 of the middle sample (sample 0 of two) are scaled
    32x in one group's channels (the seam group where there is one)."""
    samples, P, c0, c1, groups = (case[k] for k in ("samples", "P", "c0", "c1", "groups"))
    C = c0 + c1
    cpg = C // groups
    x = rnd(samples * P, C, seed=400) * 1.5 + 0.25
    slab, gs = (samples - 1) // 2, gn_sentinel_group(case)
    for r in sorted({r % P for r in SENTINEL_ROWS if r < P}):
        x[slab * P + r, gs * cpg:(gs + 1) * cpg] *= 32.0
    if "constant_group" in case:                      # constant after rounding: E[x^2] - mean^2 cancels, the reference is beta
        g = case["constant_group"]
        x[slab * P:(slab + 1) * P, g * cpg:(g + 1) * cpg] = 3.0
    gamma, beta = rnd(C, seed=401) * 0.2 + 1.0, rnd(C, seed=402) * 0.2
    return x[:, :c0].contiguous(), (x[:, c0:].contiguous() if c1 else None), gamma, beta


def gn_rounded(case, ty):
    a, s, gamma, beta = gn_inputs(case)
    return (torch.cat([rt(a, ty), rt(s, ty)], 1) if s is not None else rt(a, ty)), gamma, beta


def gn_kwargs(case):
    return dict(samples=case["samples"], P=case["P"], groups=case["groups"], silu=case["silu"])


def gn_mutants(case):
    """The mutants that apply.  Variance over N - 1 moves y by |gamma xhat| / (2 N): the budget allows DELTA (|xhat| + ...) at an element
    whose reference is near zero, so the mutant can reach MUTANT_FACTOR only where 1 / (2 N) > MUTANT_FACTOR x DELTA, N < 6250 -- at
    cpg x P = 14 400 the wrong count is an error of the size the fp32 statistics are allowed."""
    P, cpg = case["P"], (case["c0"] + case["c1"]) // case["groups"]
    m = [("drop_row", r) for r in sorted({r % P for r in SENTINEL_ROWS if r < P})] + [("next_sample_row",)]
    if cpg * P < 1.0 / (2 * MUTANT_FACTOR * DELTA):
        m.append(("var_n_minus_1",))
    if case["c1"] and case["c0"] % cpg:
        m.append(("seam_one_source",))
    return m


LN_FORMS = [{"E2V_LN_ROWS": 1}, {"E2V_LN_ROWS": 0}]
LN_DEFAULTS = {"E2V_LN_ROWS": 1}
LN_MAX_WIDTH = 1280                # e2v_op_layernorm takes no wider row (the kernels behind it hold 1280 / 1536 columns in registers)
LN_CASES = [dict(id=f"C{c}_rows{rows}", C=c, rows=rows) for c in (320, 640, 1280, 64, 1544) for rows in (1, 17)]
# the wave-per-row kernel's other instances: C = 324 is no multiple of 8 (4 channels per lane on 16-bit rows; its last piece of 8 for
# the mutants and sentinels is columns 312 .. 319, and 316 / 323 carry the sentinels), C = 768 / 1032 are two / three octets per lane
LN_CASES += [dict(id=f"C{c}_rows{rows}", C=c, rows=rows) for c, rows in ((324, 9), (768, 17), (1032, 5))]


def ln_inputs(case):
    """Sentinels: columns 0, 7, 8, C - 8 and C - 1 of one row (the ends of the first, second and last 8-column piece) are scaled 32x."""
    C, rows = case["C"], case["rows"]
    x = rnd(rows, C, seed=410) * 1.5 + 0.25
    for col in (0, 7, 8, C - 8, C - 1):
        x[min(5, rows - 1), col] *= 32.0
    return x, rnd(C, seed=411) * 0.2 + 1.0, rnd(C, seed=412) * 0.2


def ln_mutants(case):
    pieces = case["C"] // 8
    return [("drop_piece", k) for k in sorted({0, 1, pieces // 2, pieces - 1})]


# attention: `forms` are the switch settings a case runs under (each names the kernel it selects), `kboost`: two late K rows x 3
SC_DEFAULTS = {"E2V_ATTN_Q64": 1, "E2V_ATTN_KT64": 1}
_Q64_FORMS = [{}, {"E2V_ATTN_Q64": 0}, {"E2V_ATTN_Q64": 0, "E2V_ATTN_KT64": 0}]
SC_CASES = [
    dict(id="d40_q130_f3", d=40, nq=130, f=3, n=1, heads=8, forms=_Q64_FORMS),          # q64 pipelined / 32-query kt64 / 32-query kt32
    dict(id="d40_q130_f3_kboost", d=40, nq=130, f=3, n=1, heads=8, forms=_Q64_FORMS, kboost=True),
    dict(id="d40_q130_f2_n9", d=40, nq=130, f=2, n=9, heads=8, forms=[{}]),              # n % 8 != 0: the other XCD mapping
    dict(id="d80_q70_f3", d=80, nq=70, f=3, n=1, heads=8, forms=[{}]),
    dict(id="d80_q70_f3_kboost", d=80, nq=70, f=3, n=1, heads=8, forms=[{}], kboost=True),
    dict(id="d160_q40_f3", d=160, nq=40, f=3, n=1, heads=4, forms=[{}]),                 # 32-key stages, by LDS size
    dict(id="d8_q33_f3", d=8, nq=33, f=3, n=1, heads=8, forms=[{}]),
]
CROSS_DEFAULTS = {"E2V_ATTN_CROSS_RESIDENT": 1}
_CROSS_FORMS = [{"E2V_ATTN_CROSS_RESIDENT": 1}, {"E2V_ATTN_CROSS_RESIDENT": 0}]
CROSS_CASES = ([dict(id=f"d40_k{nk}", d=40, nq=45, f=3, n=2, heads=8, nk=nk, forms=_CROSS_FORMS) for nk in (77, 96, 33, 5)] +
               [dict(id="d160_k77", d=160, nq=45, f=3, n=2, heads=8, nk=77, forms=_CROSS_FORMS),
                dict(id="d40_k77_kboost", d=40, nq=45, f=3, n=2, heads=8, nk=77, forms=_CROSS_FORMS, kboost=True)])
TEMPORAL_DEFAULTS = {"E2V_TATTN_WAVE": 1}
_WAVE_FORMS = [{"E2V_TATTN_WAVE": 1}, {"E2V_TATTN_WAVE": 0}]
TEMPORAL_CASES = [
    dict(id="d40_f6_hw33", d=40, f=6, hw=33, n=2, heads=8, forms=_WAVE_FORMS),
    dict(id="d40_f6_hw33_kboost", d=40, f=6, hw=33, n=2, heads=8, forms=_WAVE_FORMS, kboost=True),
    dict(id="d160_f6_hw7", d=160, f=6, hw=7, n=2, heads=8, forms=[{}]),
    dict(id="d40_f16_hw9", d=40, f=16, hw=9, n=2, heads=8, forms=[{}]),                   # more than 8 frames: the long-clip kernel
    dict(id="d40_f16_hw9_kboost", d=40, f=16, hw=9, n=2, heads=8, forms=[{}], kboost=True),
]


def _keys_of(nk, which=SENTINEL_KEYS):
    return sorted({j % nk for j in which if j < nk})


def sc_inputs(case):
    """q | k | v rows ``[n * F * Nq, 3 c]``.  Sentinels: in every frame the V rows of keys 0, 31, 32, 63, 64 and Nq - 1 are scaled 16x (a lost
    edge key then moves the output grossly whatever its weight); ``kboost``: K rows Nq - 9 and Nq - 2 of every frame x 3, so that the
    running maximum moves in the last key stage of either segment."""
    d, nq, f, n, heads = (case[k] for k in ("d", "nq", "f", "n", "heads"))
    c = heads * d
    qkv = rnd(n * f * nq, 3 * c, seed=420).reshape(n * f, nq, 3 * c)
    qkv[:, _keys_of(nq), 2 * c:] *= 16.0
    if case.get("kboost"):
        qkv[:, [nq - 9, nq - 2], c:2 * c] *= 3.0
    return qkv.reshape(n * f * nq, 3 * c).contiguous()


def sc_kwargs(case):
    return dict(n=case["n"], F=case["f"], heads=case["heads"], Nq=case["nq"], scale=case["d"] ** -0.5)


def sc_mutants(case):
    nq = case["nq"]
    keys = _keys_of(nq) + [nq + j for j in _keys_of(nq)]
    m = [("drop_key", j) for j in keys]
    for qb in (32, 64):
        if nq % qb:
            m += [("drop_key_last_block", j, qb) for j in (0, nq - 1, nq, 2 * nq - 1)]
    return m + [("second_segment_own_frame",), ("next_frame_key",)]


def cross_inputs(case):
    d, nq, f, n, heads, nk = (case[k] for k in ("d", "nq", "f", "n", "heads", "nk"))
    c = heads * d
    q, kv = rnd(n * f * nq, c, seed=421), rnd(n * nk, 2 * c, seed=422).reshape(n, nk, 2 * c)
    kv[:, _keys_of(nk), c:] *= 16.0
    if case.get("kboost"):
        kv[:, [nk - 9, nk - 2], :c] *= 3.0
    return q, kv.reshape(n * nk, 2 * c).contiguous()


def cross_kwargs(case):
    return dict(n=case["n"], F=case["f"], heads=case["heads"], Nq=case["nq"], Nk=case["nk"], scale=case["d"] ** -0.5)


def cross_mutants(case):
    nk, rows = case["nk"], case["f"] * case["nq"]
    m = [("drop_key", j) for j in _keys_of(nk)]
    if rows % 32:
        m += [("drop_key_last_block", j, 32) for j in (0, nk - 1)]
    return m + [("next_sample_key",)]


def temporal_inputs(case):
    """``[n * F * HW, 3 c]``; sentinels: the V rows of frames 0 and F - 1 x 16; ``kboost``: the K rows of frames F - 2 and F - 1 x 3."""
    d, f, hw, n, heads = (case[k] for k in ("d", "f", "hw", "n", "heads"))
    c = heads * d
    qkv = rnd(n * f * hw, 3 * c, seed=423).reshape(n, f, hw, 3 * c)
    qkv[:, [0, f - 1], :, 2 * c:] *= 16.0
    if case.get("kboost"):
        qkv[:, [f - 2, f - 1], :, c:2 * c] *= 3.0
    return qkv.reshape(n * f * hw, 3 * c).contiguous()


def temporal_kwargs(case):
    return dict(n=case["n"], F=case["f"], HW=case["hw"], heads=case["heads"], scale=case["d"] ** -0.5)


def temporal_mutants(case):
    return [("drop_key", j) for j in sorted({0, 15 % case["f"], case["f"] - 1})]


def form_id(form):
    return ",".join(f"{k[4:]}={v}" for k, v in form.items()) or "default"


# ================================================================================================================
# GEMM-shaped ops (linear, GEGLU, 3x3 conv, two-source linear) stored in 16 bits: the launch the graph makes (switch E2V_OP_IO16)
# ================================================================================================================
# Reference: float64 on operands rounded as the kernels round them -- x, w and the residual to the type (the sub-pixel form of resize +
# conv: the tap SUMS of w, taken in fp32, rounded once), bias and the time-embedding rows ("rowbias") as the fp32 values they are.
# Budget, per element, with S = sum_k |x_k w_k| + |bias| + |rowbias| + |resid| and e32 = DELTA S:
#
#     |y - ref| <= max(u (|ref| + e32), h/2) + e32
#
# -- ONE rounding of the stored value (of a sum that is itself e32 off) plus the suite's fp32 summation-order allowance.  GEGLU,
# ref = v gate(g): S = S_v |gate(g)| + GATE_SLOPE |v| S_g (|gate'| <= 1.13) and e32 gets DELTA_G |v| (|g| + 1) for the gate's hardware
# exp2 / rcp -- DELTA_G is measured (see below), everything else is derived.
# DELTA_G: measured on an MI355X from the fp32-OUTPUT GEGLU form (switch off; tests/test_hip_h16_gemm_store.py::
# test_geglu_gate_term_of_the_fp32_output_form repeats the measurement): what an element is off beyond DELTA S, over |v| (|g| + 1),
# largest over the GEGLU problems of the table.  Observed 0 in both types -- that form stays within 0.003 of DELTA S, gate included
# (the logistic / erf sequences cost a few 1e-7 |v gate(g)|, 1/100 of DELTA S_v |gate(g)|) -- so twice the observation is 0 as well
# and the term is carried for the day a gate sequence changes: the measuring test fails when it observes more than the constant.
DELTA_G_OBSERVED = {"bf16": 0.0, "fp16": 0.0}
DELTA_G = {ty: 2.0 * v for ty, v in DELTA_G_OBSERVED.items()}
GATE_SLOPE = 1.2
EDGE_ROWS = (127, 128, 255, 256, -1)                # the first / last rows of 128- and 256-row tiles, and the last row
SEAM_COLS = (64, 128, 192, 256, 320)                # the first columns of 64-, 128-, 256- and 320-column tiles
GEMM_DEFAULTS = {"E2V_BGEMM_S3_SMALL": 1, "E2V_BGEMM_PERS": 1, "E2V_BGEMM_256": 1, "E2V_BGEMM_T256": 1, "E2V_BGEMM_T256P": 1,
                 "E2V_BGEMM_T256P_BIAS_LDS": 1, "E2V_SPLITK_FORCE": 0, "E2V_BGEMM_UP2X": 1}


def gate(g, ty):
    """The GEGLU gate as the kernels of mode ``ty`` evaluate it (igemm_epi.h: gelu_gate16), in the precision of ``g``: bf16 mode the
    logistic form x / (1 + exp(-(a x + b x^3))), fp16 mode (like fp32) the erf form."""
    if ty == "fp16":
        return 0.5 * g * (1.0 + torch.erf(g * 0.7071067811865476))
    return g / (1.0 + torch.exp(-(1.60031415 * g + 0.06940179 * g ** 3)))


def _edge_rows(M):
    return sorted({r % M for r in EDGE_ROWS if r < M})


def _seam_cols(N):
    return sorted({c for c in SEAM_COLS if c + 8 <= N} | ({N - 8} if N >= 16 else set()))


def _sentinel_cols(N):
    """Eight columns spread over the width: their weights carry one sign per input channel, so that a cancellation row (whose source
    pixels carry the same signs) has |acc| = sum |x w| there -- the rounding of the accumulator is then as large as it can be next to S."""
    return sorted({int(c) for c in torch.linspace(1, N - 2, 8).round().long()})


def _splitk_runs(c0, c1, want):
    """bgemm.hip's splitk_layout: (runs in source 0, chunks per run in source 0, runs in source 1, chunks per run in source 1)."""
    Q0, Q1 = (c0 + 63) // 64, (c1 + 63) // 64
    want = min(want, Q0 + Q1)
    if Q1:
        s0 = min(max(int(want * Q0 / (Q0 + Q1) + 0.5), 1), want - 1)
        s1 = want - s0
    else:
        s0, s1 = want, 0
    q0 = (Q0 + s0 - 1) // s0
    s0 = (Q0 + q0 - 1) // q0
    q1 = 0
    if Q1:
        q1 = (Q1 + s1 - 1) // s1
        s1 = (Q1 + q1 - 1) // q1
    return s0, q0, s1, q1


def _unfold(img, kh, kw, stride, pad):
    """``img`` [n, C, H, W] float64, ``pad`` = (left, right, top, bottom) zeros -> [n * Ho * Wo, kh * kw, C] and (Ho, Wo)."""
    import torch.nn.functional as F
    n, C = img.shape[:2]
    p = F.pad(img, pad)
    Ho, Wo = (p.shape[2] - kh) // stride + 1, (p.shape[3] - kw) // stride + 1
    cols = F.unfold(p, (kh, kw), stride=stride)                                        # [n, C * kh * kw, Ho * Wo], channel-major
    return cols.reshape(n, C, kh * kw, Ho * Wo).permute(0, 3, 2, 1).reshape(n * Ho * Wo, kh * kw, C), (Ho, Wo)


def _to_nchw(x_cl, n, H, W):
    return x_cl.reshape(n, H, W, -1).permute(0, 3, 1, 2)


_UP2_TAPS = {0: ([0], [1, 2]), 1: ([0, 1], [2])}      # output parity -> taps of the 3-wide kernel that fall on source offset 0 / 1


def _gemm_parts(case, ty, x0, x1, w):
    """The launch as GEMMs: a list of (output rows, A [rows, taps, C], W [N, taps, C]) in float64 on ROUNDED operands, and for every
    output row the source rows (pixels; -1: padding) its A row was gathered from.  One part, except for the sub-pixel form (four)."""
    if case["op"] == "linear":
        A = rt(torch.cat([x0, x1], 1) if x1 is not None else x0, ty).double()
        M = A.shape[0]
        return [(torch.arange(M), A[:, None, :], rt(w, ty).double()[:, None, :])], torch.arange(M)[:, None]
    n, Hs, Ws = case["n_img"], case["Hs"], case["Ws"]
    xs = rt(torch.cat([x0, x1], 1) if x1 is not None else x0, ty).double()
    img = _to_nchw(xs, n, Hs, Ws)
    ids = torch.arange(1, n * Hs * Ws + 1, dtype=torch.float64).reshape(n, 1, Hs, Ws)     # 0 = padding
    N, C = w.shape[:2]
    if case.get("up2x"):
        Ho, Wo = 2 * Hs, 2 * Ws
        rows = torch.arange(n * Ho * Wo).reshape(n, Ho, Wo)
        parts, src = [], torch.full((n * Ho * Wo, 4), -1, dtype=torch.long)
        for a in (0, 1):
            for b in (0, 1):
                w2 = torch.stack([torch.stack([w[:, :, _UP2_TAPS[a][ty_]][:, :, :, _UP2_TAPS[b][tx]].sum((2, 3)) for tx in (0, 1)], -1)
                                  for ty_ in (0, 1)], -2)                                  # [N, C, 2, 2], summed in fp32
                pad = (1 - b, b, 1 - a, a)
                A, _ = _unfold(img, 2, 2, 1, pad)
                r = rows[:, a::2, b::2].reshape(-1)
                parts.append((r, A, rt(w2, ty).double().reshape(N, C, 4).permute(0, 2, 1)))
                src[r] = _unfold(ids, 2, 2, 1, pad)[0][:, :, 0].long() - 1
        return parts, src
    lo, st = case.get("pad_lo", 1), case.get("stride", 1)
    A, (Ho, Wo) = _unfold(img, 3, 3, st, (lo, 1, lo, 1))
    assert (Ho, Wo) == conv_out_map(case), (Ho, Wo)
    src = _unfold(ids, 3, 3, st, (lo, 1, lo, 1))[0][:, :, 0].long() - 1
    return [(torch.arange(A.shape[0]), A, rt(w, ty).double().reshape(N, C, 9).permute(0, 2, 1))], src


def conv_out_map(case):
    lo, st = case.get("pad_lo", 1), case.get("stride", 1)
    Hi, Wi = (2 * case["Hs"], 2 * case["Ws"]) if case.get("up2x") else (case["Hs"], case["Ws"])
    return (Hi + lo + 1 - 3) // st + 1, (Wi + lo + 1 - 3) // st + 1


def _acc(parts, M, N, chan=None, absolute=False, emulate=False):
    """sum_k x_k w_k per output element over the channels ``chan`` (a slice; None: all).  ``absolute``: of |x_k w_k|.  ``emulate``: fp32
    accumulation in 64-channel chunks, as the kernels walk K."""
    out = torch.zeros(M, N, dtype=torch.float32 if emulate else torch.float64)
    for rows, A, W in parts:
        if chan is not None:
            A, W = A[:, :, chan], W[:, :, chan]
        if absolute:
            A, W = A.abs(), W.abs()
        if emulate:
            acc = torch.zeros(A.shape[0], N, dtype=torch.float32)
            for q in range(0, A.shape[2], 64):
                acc += A[:, :, q:q + 64].float().reshape(A.shape[0], -1) @ W[:, :, q:q + 64].float().reshape(N, -1).T
            out[rows] = acc
        else:
            out[rows] = A.reshape(A.shape[0], -1) @ W.reshape(N, -1).T
    return out


def gemm_shape(case):
    """(M, N of the launch, columns of the output)."""
    if case["op"] == "linear":
        M, N = case["M"], case["N"]
    else:
        Ho, Wo = conv_out_map(case)
        M, N = case["n_img"] * Ho * Wo, case["N"]
    return M, N, (N // 2 if case.get("geglu") else N)


def gemm_problem(case, ty):
    """Inputs of the case as the op takes them (fp32 tensors; the residual's cancellation rows depend on the type) and the float64
    terms of its reference.  Sentinels: at every edge row (127, 128, 255, 256, M - 1) the residual is -(acc + bias + rowbias) rounded to
    the type plus a unit normal / 16 ("cancellation rows": |ref| << |acc|), the source pixels of those rows carry one sign per channel
    and so do the weights of eight columns (there |acc| = sum |x w|); the residual rows next to them are 8 x; the time-embedding rows of
    neighbouring samples differ by at least 4 in every column; the bias pieces on the two sides of a tile seam are offset by +- 4."""
    M, N, No = gemm_shape(case)
    lin = case["op"] == "linear"
    c0, c1 = case["c0"], case.get("c1", 0)
    K = c0 + c1
    seed = 500 + 7 * sum(map(ord, case["pid"]))
    rows_in = M if lin else case["n_img"] * case["Hs"] * case["Ws"]
    x = rnd(rows_in, K, seed=seed)
    w = rnd(N, K, seed=seed + 1) * K ** -0.5 if lin else rnd(N, K, 3, 3, seed=seed + 1) * (9 * K) ** -0.5
    bias = rnd(N, seed=seed + 2)
    has_resid, geglu = bool(case.get("resid")), bool(case.get("geglu"))
    edges = _edge_rows(M)
    if has_resid:                                      # one sign per channel: the sentinel columns' weights, the cancellation rows' pixels
        sign = torch.where(rnd(K, seed=seed + 3) >= 0, 1.0, -1.0)
        cols = _sentinel_cols(N)
        w[cols] = w[cols].abs() * (sign[None, :] if lin else sign[None, :, None, None])
    if not geglu:
        for c in _seam_cols(N):
            bias[c:c + 8] += 4.0
            bias[c - 8:c] -= 4.0
    x0 = x[:, :c0].contiguous()
    x1 = x[:, c0:].contiguous() if c1 else None
    if has_resid:
        _, src = _gemm_parts(case, ty, x0, x1, w)
        pix = src[edges].reshape(-1)
        pix = pix[pix >= 0].unique()
        x[pix] = x[pix].abs() * sign[None, :]
        x0 = x[:, :c0].contiguous()
        x1 = x[:, c0:].contiguous() if c1 else None
    parts, _ = _gemm_parts(case, ty, x0, x1, w)
    acc, sabs = _acc(parts, M, N), _acc(parts, M, N, absolute=True)
    b = bias.double()
    rowbias, rowb = None, torch.zeros(M, N, dtype=torch.float64)
    if case.get("rps"):
        rps = case["rps"]
        samples = (M + rps - 1) // rps
        rowbias = rnd(samples, N, seed=seed + 4) * 0.2 + 6.0 * (torch.arange(samples) % 2)[:, None]
        rowb = rowbias.double()[torch.arange(M) // rps]
    resid, r = None, torch.zeros(M, N, dtype=torch.float64)
    if has_resid:
        resid = rnd(M, N, seed=seed + 5)
        for m in edges:
            for nb in (m - 1, m + 1):
                if 0 <= nb < M and nb not in edges:
                    resid[nb] *= 8.0
        noise = rnd(len(edges), N, seed=seed + 6) / 16.0
        resid[edges] = rt(-(acc + b + rowb)[edges], ty) + noise
        r = rt(resid, ty).double()
    p = dict(case=case, ty=ty, M=M, N=N, No=No, x0=x0, x1=x1, w=w, bias=bias, rowbias=rowbias, resid=resid, parts=parts, acc=acc, sabs=sabs,
             b=b, rowb=rowb, r=r, edges=edges)
    p["ref"], p["S"], p["extra"] = _gemm_ref(p, acc, sabs, b, rowb, r)
    p["budget"] = gemm_budget(p["ref"], p["S"], ty, p["extra"])
    return p


def _gemm_ref(p, acc, sabs, b, rowb, r, swap_blocks=()):
    """Reference, S and the gate term from the terms.  ``swap_blocks``: GEGLU mutant -- output blocks of 32 columns whose value and gate
    are exchanged."""
    ty = p["ty"]
    if not p["case"].get("geglu"):
        return acc + b + rowb + r, sabs + b.abs() + rowb.abs() + r.abs(), 0.0
    h = p["N"] // 2
    v, g = acc[:, :h] + b[:h], acc[:, h:] + b[h:]
    sv, sg = sabs[:, :h] + b[:h].abs(), sabs[:, h:] + b[h:].abs()
    for j in swap_blocks:
        c = slice(32 * j, 32 * j + 32)
        v, g = v.clone(), g.clone()
        v[:, c], g[:, c] = g[:, c].clone(), v[:, c].clone()
    return v * gate(g, ty), sv * gate(g, ty).abs() + GATE_SLOPE * v.abs() * sg, DELTA_G[ty] * v.abs() * (g.abs() + 1.0)


def gemm_budget(ref, S, ty, extra=0.0):
    e32 = DELTA * S + extra
    return torch.clamp(UNIT[ty] * (ref.abs() + e32), min=SPACING[ty] / 2) + e32


def gemm_emulation(p):
    """The kernels' arithmetic in torch: fp32 accumulation in 64-channel chunks, bias, time-embedding row and residual added in fp32,
    one rounding.  Returns the rounded result and the unrounded fp32 one (both as float64)."""
    ty = p["ty"]
    acc = _acc(p["parts"], p["M"], p["N"], emulate=True)
    if p["case"].get("geglu"):
        h = p["N"] // 2
        y = (acc[:, :h] + p["bias"][:h]) * gate(acc[:, h:] + p["bias"][h:], ty)
    else:
        y = acc + p["bias"]
        if p["rowbias"] is not None:
            y = y + p["rowb"].float()
        if p["resid"] is not None:
            y = y + p["r"].float()
    return rt(y, ty).double(), y.double()


def gemm_mutants(p, form):
    """The mutants that apply to problem ``p`` under the switches ``form``: (name, groups) with groups = [(label, rows, cols, mutated
    reference on [rows, cols])] -- the mutant has to exceed the budget MUTANT_FACTOR times somewhere in EVERY group.  rows: an index
    tensor, cols: a slice."""
    case, ty, M, N, No = p["case"], p["ty"], p["M"], p["N"], p["No"]
    acc, sabs, b, rowb, r, ref = p["acc"], p["sabs"], p["b"], p["rowb"], p["r"], p["ref"]
    allc, allr = slice(0, No), torch.arange(M)
    out = []
    row = lambda m: torch.tensor([m])
    if case.get("geglu"):
        nblk = No // 32
        for j in sorted({0, nblk // 2, nblk - 1}):
            c = slice(32 * j, 32 * j + 32)
            out.append((("geglu_swap_block", j), [(f"block {j}", allr, c, _gemm_ref(p, acc, sabs, b, rowb, r, swap_blocks=(j,))[0][:, c])]))
        c = slice(No - 32, No)
        out.append((("geglu_last_block_dropped",), [("last block", allr, c, torch.zeros(M, 32, dtype=torch.float64))]))
        return out
    if p["resid"] is not None:
        for m in p["edges"]:
            if m >= 1:
                out.append((("resid_of_row_above", m), [(f"row {m}", row(m), allc, ref[m:m + 1] - r[m:m + 1] + r[m - 1:m])]))
            if m + 1 < M:
                out.append((("resid_of_row_below", m), [(f"row {m}", row(m), allc, ref[m:m + 1] - r[m:m + 1] + r[m + 1:m + 2])]))
        out.append((("rounded_before_resid",), [(f"row {m}", row(m), allc, (rt(acc + b + rowb, ty).double() + r)[m:m + 1]) for m in p["edges"]]))
    if p["rowbias"] is not None:
        rps = case["rps"]
        chunks = [c for c in range(0, M, 32) if c // rps != (min(c + 32, M) - 1) // rps]
        assert chunks, "no 32-row chunk straddles two samples"
        for which in ("first", "last"):
            groups = []
            for c in chunks:
                rr = torch.arange(c, min(c + 32, M))
                s = (c if which == "first" else int(rr[-1])) // rps
                groups.append((f"rows {c}..{int(rr[-1])}", rr, allc, ref[rr] - rowb[rr] + p["rowbias"].double()[s]))
            out.append((("chunk_rowbias_of_" + which + "_sample",), groups))
    for c in _seam_cols(N):
        cs, left = slice(c, c + 8), slice(c - 8, c)
        out.append((("seam_piece_from_the_left", c), [(f"columns {c}..{c + 7}", allr, cs, ref[:, cs] - b[cs] - r[:, cs] + b[left] + r[:, left])]))
    if case.get("up2x"):
        Ho, Wo = conv_out_map(case)
        img = ref.reshape(case["n_img"], Ho, Wo, N)
        rows = torch.arange(M).reshape(case["n_img"], Ho, Wo)
        a, bq = rows[:, 0::2, 1::2].reshape(-1), rows[:, 1::2, 0::2].reshape(-1)
        out.append((("parities_exchanged", "01<->10"), [("parity (0, 1)", a, allc, img[:, 1::2, 0::2].reshape(-1, N)),
                                                        ("parity (1, 0)", bq, allc, img[:, 0::2, 1::2].reshape(-1, N))]))
    want = form.get("E2V_SPLITK_FORCE", 0)
    if want >= 2:
        c0, c1 = case["c0"], case.get("c1", 0)
        s0, q0, s1, q1 = _splitk_runs(c0, c1, want)
        assert s0 + s1 >= 2
        chan = slice(c0 + (s1 - 1) * q1 * 64, c0 + c1) if s1 else slice((s0 - 1) * q0 * 64, c0)
        last = _acc(p["parts"], M, N, chan=chan)
        out.append((("last_run_left_out", want), [(f"row {m}", row(m), allc, (ref - last)[m:m + 1]) for m in range(M)]))
    if case["op"] == "linear" and case.get("c1"):
        c0, c1 = case["c0"], case["c1"]
        A, W = p["parts"][0][1][:, 0], p["parts"][0][2][:, 0]
        mut = []
        if c0 != c1:                                   # source 1 read with source 0's row stride (past the end: wrapped)
            flat = A[:, c0:].reshape(-1)
            idx = (torch.arange(M)[:, None] * c0 + torch.arange(c1)[None, :]) % flat.numel()
            mut.append((("source1_with_stride_of_source0",), torch.cat([A[:, :c0], flat[idx]], 1), 1))
        if c0 >= 64:                                   # the seam one 64-channel chunk early: source 1 from there on, zeros behind its end
            mut.append((("seam_one_chunk_early",), torch.cat([A[:, :c0 - 64], A[:, c0:], torch.zeros(M, 64, dtype=torch.float64)], 1), 0))
        for name, Am, first in mut:
            full = Am @ W.T + b
            out.append((name, [(f"row {m}", row(m), allc, full[m:m + 1]) for m in range(first, M)]))
    return out


def where_gemm(p):
    rps = p["case"].get("rps")
    return lambda r, c: (f"row {r} of {p['M']} (row {r % 128} of 128-row tile {r // 128}, row {r % 256} of 256-row tile {r // 256}, "
                         f"32-row chunk {r // 32}" + (f", sample {r // rps}" if rps else "") + f"), column {c} of {p['No']} "
                         f"(column {c % 64} of 64-column tile {c // 64}, piece {c // 8})" + (", cancellation row" if r in p["edges"] and p["resid"] is not None else ""))


# ---- the case table ------------------------------------------------------------------------------------------------------------
# pid: the problem (shape + operands; forms that run the same problem share it), expect / refuse: the kernel the launch must / must
# not be served by (e2v_op_last_dispatch).  Shapes: the smallest at which the form can still go wrong -- a ragged last row block, more
# than one tile in both directions, every width at which the store takes another path (N % 8 != 0: element-wise).
def _lin(pid, M, K, N, resid=False, geglu=False, c1=0):
    return dict(pid=pid, op="linear", M=M, c0=K - c1, c1=c1, N=2 * N if geglu else N, resid=resid, geglu=geglu)


def _conv(pid, n_img, Hs, Ws, cin, N, resid=False, rps=0, c1=0, **kw):
    return dict(pid=pid, op="conv", n_img=n_img, Hs=Hs, Ws=Ws, c0=cin - c1, c1=c1, N=N, resid=resid, rps=rps, **kw)


_P = {
    "lin130x40x72": _lin("lin130x40x72", 130, 40, 72),
    "lin300x320x192r": _lin("lin300x320x192r", 300, 320, 192, resid=True),
    "lin77x256x70r": _lin("lin77x256x70r", 77, 256, 70, resid=True),
    "lin77x64x70r": _lin("lin77x64x70r", 77, 64, 70, resid=True),
    "lin257x128x64": _lin("lin257x128x64", 257, 128, 64),
    "lin8300x64x1024r": _lin("lin8300x64x1024r", 8300, 64, 1024, resid=True),
    "geglu300x64x96": _lin("geglu300x64x96", 300, 64, 96, geglu=True),
    "geglu300x320x128": _lin("geglu300x320x128", 300, 320, 128, geglu=True),
    "geglu300x640x256": _lin("geglu300x640x256", 300, 640, 256, geglu=True),
    "lin552x320x192r": _lin("lin552x320x192r", 552, 320, 192, resid=True),
    # 256-row tiles beyond the narrow schedule (sched256: what igemm_schedule.schedule(rows=256, slots=256) has to say of the launch):
    # 178 row blocks in unequal chunks, the last two of each chunk as 128x64 tiles only; 254 row blocks, 128x128 + 128x64 everywhere
    "lin45500x64x192r": dict(_lin("lin45500x64x192r", 45500, 64, 192, resid=True),
                             sched256=dict(kind="mixed", nbm=178, rb1=162, w1=1, s1=1, s2=3, tail_rb=2, chunks=(22, 22, 22, 23, 22, 22, 22, 23))),
    "lin65000x64x192r": dict(_lin("lin65000x64x192r", 65000, 64, 192, resid=True), sched256=dict(kind="wide", nbm=254, rb1=254, w1=1, s1=1, s2=3, tail_rb=0)),
    "lin513x640x320r": _lin("lin513x640x320r", 513, 640, 320, resid=True),
    "lin513x640x320": _lin("lin513x640x320", 513, 640, 320),
    "lin300x640x512r": _lin("lin300x640x512r", 300, 640, 512, resid=True),
    "lin300x640x512": _lin("lin300x640x512", 300, 640, 512),
    "lin130x640x72r": _lin("lin130x640x72r", 130, 640, 72, resid=True),
    "cat300x64+64x192": _lin("cat300x64+64x192", 300, 128, 192, c1=64),
    "cat130x128+64x72": _lin("cat130x128+64x72", 130, 192, 72, c1=64),
    "cat513x320+320x320": _lin("cat513x320+320x320", 513, 640, 320, c1=320),
    "conv64to136_2x7x5_rps35r": _conv("conv64to136_2x7x5_rps35r", 2, 7, 5, 64, 136, resid=True, rps=35),
    "conv64to128_3x9x16_rps144r": _conv("conv64to128_3x9x16_rps144r", 3, 9, 16, 64, 128, resid=True, rps=144),
    "conv64to128_2x7x5_rps35r": _conv("conv64to128_2x7x5_rps35r", 2, 7, 5, 64, 128, resid=True, rps=35),
    "conv64to128_3x8x23_rps184r": _conv("conv64to128_3x8x23_rps184r", 3, 8, 23, 64, 128, resid=True, rps=184),
    "conv128to320_3x9x16_rps144r": _conv("conv128to320_3x9x16_rps144r", 3, 9, 16, 128, 320, resid=True, rps=144),
    "conv128to256_2x8x12_s2_rps24r": _conv("conv128to256_2x8x12_s2_rps24r", 2, 8, 12, 128, 256, resid=True, rps=24, stride=2, pad_lo=0),
    "conv128+64to320_2x7x5r": _conv("conv128+64to320_2x7x5r", 2, 7, 5, 192, 320, resid=True, c1=64),
    "conv128to64_2x5x8_rps40r": _conv("conv128to64_2x5x8_rps40r", 2, 5, 8, 128, 64, resid=True, rps=40),
    "conv64+64to64_2x5x8r": _conv("conv64+64to64_2x5x8r", 2, 5, 8, 128, 64, resid=True, c1=64),
    "up2x_2x128to256_7x6": _conv("up2x_2x128to256_7x6", 2, 7, 6, 128, 256, up2x=True),
    "up2x_3x256to320_5x8": _conv("up2x_3x256to320_5x8", 3, 5, 8, 256, 320, up2x=True),
}


def _form(name, knobs, rows, ab=False):
    """rows: (pid, expect[, refuse]).  The first row is the form's bounds case (run once more under E2V_POOL_GUARD)."""
    out = []
    for i, r in enumerate(rows):
        case = dict(_P[r[0]], id=f"{name}-{r[0]}", form=dict(knobs), form_name=name, expect=r[1], refuse=r[2] if len(r) > 2 else None,
                    guard=i == 0, ab=ab)
        out.append(case)
    return out


_S3, _PERS, _N64, _BG = "bgemm_s3_kernel", "bgemm_pers_kernel", "bgemm_n64_kernel", "bgemm_kernel 128x128"
_TILE = {"E2V_BGEMM_S3_SMALL": 0, "E2V_BGEMM_PERS": 0}
_T256 = {"E2V_BGEMM_T256": 2, "E2V_BGEMM_T256P": 0}
_T256P = {"E2V_BGEMM_T256": 2, "E2V_BGEMM_T256P": 2}
GEMM_CASES = (
    # the default rules at small sizes: the three-stage ring where K is at least four 64-deep stages; a linear of fewer stages
    # without a residual and K <= 320 takes the persistent kernel (E2V_BGEMM_PERS = 1)
    _form("default", {}, [("lin300x320x192r", _S3), ("lin130x40x72", _PERS), ("lin77x256x70r", _S3), ("conv64to136_2x7x5_rps35r", _S3)]) +
    # the two-stage tile kernels: launches of less than one round are cut into 128 x 64 tiles (bgemm_n64_kernel) -- GEGLU excepted;
    # 128 x 128 tiles with a 128 x 64 tail need more than a round: 8300 x 1024
    _form("tile", _TILE, [("lin300x320x192r", _N64), ("lin130x40x72", _N64), ("lin77x64x70r", _N64), ("lin257x128x64", _N64),
                          ("geglu300x64x96", _BG), ("lin8300x64x1024r", _BG + "+128x64")]) +
    _form("pers", {"E2V_BGEMM_S3_SMALL": 0, "E2V_BGEMM_PERS": 2},
          [("lin300x320x192r", _PERS), ("lin8300x64x1024r", _PERS), ("geglu300x320x128", _PERS), ("conv64to128_3x9x16_rps144r", _PERS),
           ("conv64to128_2x7x5_rps35r", _N64, _PERS)]) +          # time-embedding rows of more than two samples under one tile: refused
    _form("256s3", {"E2V_BGEMM_256": 2, "E2V_BGEMM_T256": 0}, [("lin552x320x192r", "bgemm256s3_kernel"), ("conv64to128_3x8x23_rps184r", "bgemm256s3_kernel"),
                                                                ("lin45500x64x192r", "bgemm256s3_kernel"), ("lin65000x64x192r", "bgemm256s3_kernel")]) +
    _form("t256", _T256, [("lin513x640x320r", "bgemm_t256_kernel 256x320"), ("lin300x640x512r", "bgemm_t256_kernel 256x256"),
                          ("geglu300x640x256", "bgemm_t256_kernel 256x256"), ("conv128to320_3x9x16_rps144r", "bgemm_t256_kernel 256x320"),
                          ("conv128to256_2x8x12_s2_rps24r", "bgemm_t256_kernel 256x256"), ("conv128+64to320_2x7x5r", "bgemm_t256_kernel 256x320")]) +
    _form("t256p_blds1", dict(_T256P, E2V_BGEMM_T256P_BIAS_LDS=1),
          [("lin513x640x320r", "bgemm_t256p_kernel 256x320", "bias-lds"), ("lin513x640x320", "bgemm_t256p_kernel 256x320 bias-lds"),
           ("lin300x640x512r", "bgemm_t256p_kernel 256x256", "bias-lds"), ("lin300x640x512", "bgemm_t256p_kernel 256x256 bias-lds"),
           ("geglu300x640x256", "bgemm_t256p_kernel 256x256 bias-lds")]) +
    _form("t256p_blds0", dict(_T256P, E2V_BGEMM_T256P_BIAS_LDS=0),
          [("lin513x640x320", "bgemm_t256p_kernel 256x320", "bias-lds"), ("lin300x640x512", "bgemm_t256p_kernel 256x256", "bias-lds"),
           ("geglu300x640x256", "bgemm_t256p_kernel 256x256", "bias-lds")]) +
    sum((_form(f"splitk{s}", {"E2V_SPLITK_FORCE": s},
               [("lin130x640x72r", f"bgemm_splitk_kernel 128x128 x{s}"), ("conv128to64_2x5x8_rps40r", "bgemm_splitk_kernel 128x128 x2"),
                ("conv64+64to64_2x5x8r", "bgemm_splitk_kernel 128x128 x2")]) for s in (2, 5)), []) +
    _form("up2x", {"E2V_BGEMM_UP2X": 1}, [("up2x_2x128to256_7x6", "bgemm_t256_kernel 256x256"), ("up2x_3x256to320_5x8", "bgemm_t256_kernel 256x320")]) +
    _form("cat", {}, [("cat300x64+64x192", _PERS), ("cat130x128+64x72", _PERS), ("cat513x320+320x320", _S3)]) +
    _form("cat_pers", {"E2V_BGEMM_S3_SMALL": 0, "E2V_BGEMM_PERS": 2},
          [("cat300x64+64x192", _PERS), ("cat130x128+64x72", _PERS), ("cat513x320+320x320", _PERS)])
)
GEMM_PROBLEM_BY_ID = _P
GEMM_PROBLEMS = list(_P.values())
GEGLU_PROBLEMS = [c for c in GEMM_PROBLEMS if c.get("geglu")]
CAT_PROBLEMS = [c for c in GEMM_PROBLEMS if c["op"] == "linear" and c.get("c1")]
