"""GPU: the key-tile loop of the fp32 attention kernel (csrc/attn.hip, flash_attn_kernel<D>) through e2v_op_attention, against float64
on the CPU, at ``rtol=1e-4, atol=1e-5`` (the tolerance tests/test_hip_ops.py holds this op to).

The loop walks whole 32-key tiles in pairs (the LDS buffer of a tile body is a compile-time constant), takes a leading odd tile, a
trailing whole tile and each segment's ragged last tile through a general body, rescales its accumulators under a wave-uniform branch
only when a row maximum moved, and, where the head dimension leaves 8 value columns over (D = 40, D = 8), accumulates those on
v_mfma_f32_4x4x1_16b_f32.  The shapes below reach each of those paths:

  Nq = Nk = 32    one whole tile per segment: frames 0 / 1 run the general body once, frame 2 starts its second segment on an odd tile
  Nq = Nk = 40    a whole tile and a ragged 8 per segment (an odd number of tiles per segment)
  Nq = Nk = 144   four whole tiles and a ragged 16: two pairs, the ragged tile, then the second segment from an odd tile
  Nq = Nk = 160   five whole tiles: two pairs and a trailing whole tile
  Nk = 77 (cross) one pair and a ragged 13; Nq = 40 leaves three of the workgroup's four waves without queries

with n = 1, 2, 8 (workgroups dealt to the XCDs by (frame, head), by frame and by sample) and F = 3, heads = 2 (frames 0 and 1 attend
to one key segment, frame 2 to two).  ``cases()`` lists every op-level case for tools/attn_fp32_bits.py.
"""
import functools

import pytest
import torch

from test_hip_bounds import close, make_engine, rnd

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5
DS = (40, 8, 80, 160)             # 40 and 8 leave 8 value columns over; 80 runs a third 32-row tile; 160 is five whole tiles
NS = (32, 40, 144, 160)
SAMPLES = (1, 2, 8)
F, HEADS = 3, 2


@pytest.fixture(scope="module")
def eng():
    return make_engine()


def _heads(x, h):     # [b, s, h*d] -> [b*h, s, d]
    b, s, c = x.shape
    return x.reshape(b, s, h, c // h).permute(0, 2, 1, 3).reshape(b * h, s, c // h)


def _unheads(x, h):
    bh, s, d = x.shape
    return x.reshape(bh // h, h, s, d).permute(0, 2, 1, 3).reshape(bh // h, s, h * d)


def _ref(q, k, v, scale):      # float64
    return torch.bmm((torch.bmm(q, k.transpose(1, 2)) * scale).softmax(-1), v)


def ref_sparse_causal(q, k, v, n, f, nq, heads, d):
    """q, k, v: [n*f*nq, heads*d]; keys / values of frame i = [frame 0 ; frame max(i - 1, 0)]"""
    c = heads * d
    q, k, v = (t.double().reshape(n * f, nq, c) for t in (q, k, v))
    former = torch.arange(f) - 1
    former[0] = 0
    gather = lambda t: torch.cat([t.reshape(n, f, nq, c)[:, [0] * f], t.reshape(n, f, nq, c)[:, former]], dim=2).reshape(n * f, 2 * nq, c)
    return _unheads(_ref(_heads(q, heads), _heads(gather(k), heads), _heads(gather(v), heads), d ** -0.5), heads).reshape(n * f * nq, c)


def ref_cross(q, k, v, n, f, nq, nk, heads, d):
    """q: [n*f*nq, heads*d]; k, v: [n*nk, heads*d], the same rows for every frame of a sample"""
    c = heads * d
    rep = lambda t: t.double().reshape(n, nk, c).repeat_interleave(f, 0)
    return _unheads(_ref(_heads(q.double().reshape(n * f, nq, c), heads), _heads(rep(k), heads), _heads(rep(v), heads), d ** -0.5),
                    heads).reshape(n * f * nq, c)


def run_sparse_causal(eng, qkv, n, f, nq, heads, d):
    c = heads * d
    g = qkv.cuda()
    return eng.op_attention(g[:, :c], g[:, c:2 * c], g[:, 2 * c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nq, mode=0, scale=d ** -0.5).cpu()


def run_cross(eng, q, kv, n, f, nq, nk, heads, d):
    c = heads * d
    gq, gkv = q.cuda(), kv.cuda()
    return eng.op_attention(gq, gkv[:, :c], gkv[:, c:], n=n, F=f, heads=heads, D=d, Nq=nq, Nk=nk, mode=1, scale=d ** -0.5).cpu()


# ---------------------------------------------------------------- inputs (built once per shape; the references are cached and never written)
@functools.lru_cache(maxsize=None)
def shape_problem(d, nq, n):
    qkv = rnd(n * F * nq, 3 * HEADS * d, seed=1000 + d + nq + n)
    c = HEADS * d
    return qkv, ref_sparse_causal(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], n, F, nq, HEADS, d)


@functools.lru_cache(maxsize=None)
def cross_problem(d, nq, nk=77, n=2):
    c = HEADS * d
    q, kv = rnd(n * F * nq, c, seed=2000 + d + nq), rnd(n * nk, 2 * c, seed=2001 + d + nq)
    return q, kv, ref_cross(q, kv[:, :c], kv[:, c:], n, F, nq, nk, HEADS, d)


@functools.lru_cache(maxsize=None)
def pattern_problem(d, nq):
    """Q = 0: every attended key has the same probability.  The 8 leftover value columns hold ``key + column / 64`` (key: the row's index
    in its frame), so a swapped column, a key counted twice or dropped, or a mixed-up half-wave each move the result by at least 1/64
    per column or 1/(2 nq) per key; their expected value is ``(nq - 1) / 2 + column / 64`` for every frame (both segments of frame 2
    hold the same pattern).  The other columns are random and go against float64."""
    n, c, lo = 2, HEADS * d, d - 8
    qkv = rnd(n * F * nq, 3 * c, seed=3000 + d + nq)
    qkv[:, :c] = 0.0
    v = qkv[:, 2 * c:].reshape(n * F, nq, HEADS, d)
    key = torch.arange(nq, dtype=torch.float32).reshape(1, nq, 1, 1)
    col = torch.arange(lo, d, dtype=torch.float32).reshape(1, 1, 1, 8)
    v[..., lo:] = key + col / 64.0
    ref = ref_sparse_causal(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], n, F, nq, HEADS, d)
    closed = ((nq - 1) / 2.0 + torch.arange(lo, d, dtype=torch.float64) / 64.0).expand(n * F * nq, HEADS, 8)
    assert torch.allclose(ref.reshape(-1, HEADS, d)[..., lo:], closed, rtol=1e-12, atol=0)
    return qkv, ref, closed, n


@functools.lru_cache(maxsize=None)
def moved_problem(d, kind):
    """Scores along one direction u: ``rising`` -- key i of a frame scores about 0.3 i against every query, and frame 1 continues where
    frame 0 ends, so every row's maximum moves in every tile of both segments; ``first`` -- key 0 of frame 0 scores 40 above the rest
    (all within +-3), so after the first tile no maximum moves again."""
    n, nq, c = 1, 144, HEADS * d
    qkv = rnd(n * F * nq, 3 * c, seed=4000 + d, scale=0.1)
    u = torch.nn.functional.normalize(rnd(HEADS, d, seed=4001 + d), dim=-1)
    s = d ** 0.5                                                            # undoes the op's d ** -0.5
    q = qkv[:, :c].reshape(n * F, nq, HEADS, d)
    k = qkv[:, c:2 * c].reshape(n * F, nq, HEADS, d)
    q += u * (1.0 + 0.05 * rnd(n * F, nq, HEADS, 1, seed=4002 + d))
    if kind == "rising":
        k += u * s * 0.3 * (torch.arange(nq).reshape(1, nq, 1, 1) + nq * torch.arange(F).reshape(F, 1, 1, 1).clamp(max=1)).float()
    else:
        k[0, 0] += u * s * 40.0
    return qkv, ref_sparse_causal(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], n, F, nq, HEADS, d), n, nq


@functools.lru_cache(maxsize=None)
def large_problem(d):
    """scores of about +-80 (exp2 domain: +-115): unit-norm rows, q . k in [-1, 1], times 80 after the op's own scale"""
    n, nq, c = 1, 40, HEADS * d
    qkv = rnd(n * F * nq, 3 * c, seed=5000 + d)
    for i in range(2):
        t = qkv[:, i * c:(i + 1) * c].reshape(-1, HEADS, d)
        t[:] = torch.nn.functional.normalize(t, dim=-1) * (80.0 * d ** 0.5) ** 0.5
    t = qkv[:, c:2 * c].reshape(n * F, nq, HEADS, d)
    qh = qkv[:, :c].reshape(n * F, nq, HEADS, d)
    t[:, 5] = qh[:, 7]                                                      # key 5 = query 7: a score of exactly +80 ...
    t[:, 33] = -qh[:, 9]                                                    # ... and, in the ragged tile, one of -80
    return qkv, ref_sparse_causal(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], n, F, nq, HEADS, d), n, nq


def cases():
    """(name, run(eng) -> (y, ref)) of every op-level case"""
    for d in DS:
        for nq in NS:
            for n in SAMPLES:
                yield f"shape D{d} N{nq} n{n}", (lambda e, d=d, nq=nq, n=n: (run_sparse_causal(e, shape_problem(d, nq, n)[0], n, F, nq, HEADS, d),
                                                                                  shape_problem(d, nq, n)[1]))
        for nq in (40, 144):
            yield f"cross D{d} Nq{nq} Nk77", (lambda e, d=d, nq=nq: (run_cross(e, *cross_problem(d, nq)[:2], 2, F, nq, 77, HEADS, d),
                                                                         cross_problem(d, nq)[2]))
    for d in (40, 8):
        for nq in (40, 144):
            yield f"pattern D{d} N{nq}", (lambda e, d=d, nq=nq: (run_sparse_causal(e, pattern_problem(d, nq)[0], pattern_problem(d, nq)[3], F, nq, HEADS, d),
                                                                    pattern_problem(d, nq)[1]))
    for d in DS:
        for kind in ("rising", "first"):
            yield f"moved {kind} D{d}", (lambda e, d=d, kind=kind: (run_sparse_causal(e, moved_problem(d, kind)[0], moved_problem(d, kind)[2], F,
                                                                                       moved_problem(d, kind)[3], HEADS, d), moved_problem(d, kind)[1]))
        yield f"large D{d}", (lambda e, d=d: (run_sparse_causal(e, large_problem(d)[0], large_problem(d)[2], F, large_problem(d)[3], HEADS, d),
                                               large_problem(d)[1]))


# ---------------------------------------------------------------- tests
@pytest.mark.parametrize("nq", NS)
@pytest.mark.parametrize("d", DS)
def test_sparse_causal_tile_walk(eng, d, nq):
    for n in SAMPLES:
        qkv, ref = shape_problem(d, nq, n)
        close(run_sparse_causal(eng, qkv, n, F, nq, HEADS, d), ref, rtol=RTOL, atol=ATOL, what=f"D{d} N{nq} n{n}")


@pytest.mark.parametrize("d", DS)
def test_cross_tile_walk(eng, d):
    for nq in (40, 144):
        q, kv, ref = cross_problem(d, nq)
        close(run_cross(eng, q, kv, 2, F, nq, 77, HEADS, d), ref, rtol=RTOL, atol=ATOL, what=f"cross D{d} Nq{nq}")


@pytest.mark.parametrize("nq", (40, 144))
@pytest.mark.parametrize("d", (40, 8))
def test_leftover_columns_keys_and_halves(eng, d, nq):
    qkv, ref, closed, n = pattern_problem(d, nq)
    y = run_sparse_causal(eng, qkv, n, F, nq, HEADS, d)
    close(y, ref, rtol=RTOL, atol=ATOL, what=f"pattern D{d} N{nq}")
    # the closed form, element by element: a column off by one is 1/64 = 1.6e-2 away, the bound at most 1e-4 * 72 + 1e-5
    got = y.double().reshape(-1, HEADS, d)[..., d - 8:]
    err = (got - closed).abs()
    print(f"pattern D{d} N{nq}: leftover columns max abs err {err.max().item():.3e}")
    assert (err <= ATOL + RTOL * closed.abs()).all()


@pytest.mark.parametrize("kind", ("rising", "first"))
@pytest.mark.parametrize("d", DS)
def test_row_maximum_moves_in_every_tile_or_never(eng, d, kind):
    qkv, ref, n, nq = moved_problem(d, kind)
    close(run_sparse_causal(eng, qkv, n, F, nq, HEADS, d), ref, rtol=RTOL, atol=ATOL, what=f"moved {kind} D{d}")


@pytest.mark.parametrize("d", DS)
def test_large_scores_stay_finite(eng, d):
    qkv, ref, n, nq = large_problem(d)
    y = run_sparse_causal(eng, qkv, n, F, nq, HEADS, d)
    assert torch.isfinite(y).all()
    close(y, ref, rtol=RTOL, atol=ATOL, what=f"large D{d}")


@pytest.mark.parametrize("d", DS)
def test_deterministic_and_independent_of_the_batch(eng, d):
    nq, c = 144, HEADS * d
    qkv, _ = shape_problem(d, nq, 2)
    a = run_sparse_causal(eng, qkv, 2, F, nq, HEADS, d)
    b = run_sparse_causal(eng, qkv, 2, F, nq, HEADS, d)
    assert torch.equal(a, b), "two runs of one launch differ"
    rows = F * nq
    alone = torch.cat([run_sparse_causal(eng, qkv[i * rows:(i + 1) * rows].contiguous(), 1, F, nq, HEADS, d) for i in range(2)])
    assert torch.equal(a, alone), "n = 2 differs from its two samples run alone"
