"""Per-element rounding budgets for the ops of the 16-bit modes whose output is stored in 16 bits: GroupNorm, LayerNorm, sparse-causal,
cross and temporal attention.  Pure torch on the CPU, float64; no kernel is called from here.

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
