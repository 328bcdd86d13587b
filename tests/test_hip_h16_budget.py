"""GPU: the ops of the 16-bit modes whose output is stored in 16 bits -- every GroupNorm and LayerNorm form, sparse-causal, cross and
temporal attention -- through the C ABI, each element against the float64 reference of ``tests/h16_budget.py`` within its own rounding
budget (norms: two roundings of that element plus the fp32 statistics term; attention: 4 u (sum p |v| + |o|)).  The cases, their
sentinel rows / keys and the mutants they are proven sensitive to are the table of that module; ``tests/test_h16_budget_host.py`` holds
the table to its conditions without a GPU.  Every case runs once per kernel form (``set_knob``, restored afterwards); the forms of
``make AB=1`` builds run where the library has them.  Each test prints its largest error / budget (``-s``): DESIGN section 5 quotes
them."""
import contextlib
import functools

import pytest
import torch

import h16_budget as hb

pytestmark = pytest.mark.gpu

TYPES = ["bf16", "fp16"]


@pytest.fixture(scope="module")
def eng():
    from eeg2video_amd.engine import Engine
    from eeg2video_amd.weights import TINY_UNET, TINY_VAE
    return Engine(TINY_UNET, TINY_VAE, 0)


def ab_build(eng):
    """True when the library was built with ``make AB=1``: the variants that were measured and not adopted exist with their switches."""
    try:
        eng.set_knob("E2V_ATTN_FOLD", 1)
        return True
    except ValueError:
        return False


@contextlib.contextmanager
def form_of(eng, ty, form, defaults):
    """Run under a kernel form: 16-bit mode ``ty`` and the switches of ``form``; everything back to ``defaults`` afterwards."""
    try:
        eng.set_compute_dtype(ty)
        for k, v in form.items():
            eng.set_knob(k, v)
        yield eng
    finally:
        try:
            for k in form:
                eng.set_knob(k, defaults[k])
        finally:
            eng.set_compute_dtype("fp32")


def _params(cases, with_forms=None):
    """(case, form) pairs with readable ids; ``with_forms``: one list of forms for every case, else the case's own."""
    out = []
    for c in cases:
        for f in (with_forms if with_forms is not None else c["forms"]):
            out.append(pytest.param(c, f, id=f"{c['id']}-{hb.form_id(f)}"))
    return out


def _report(what, worst):
    print(f"\n{what}: largest error / budget = {worst:.3f}")


# ------------------------------------------------------------------ GroupNorm
@functools.lru_cache(maxsize=None)
def _gn_ref(case_id, ty):
    case = next(c for c in hb.GN_CASES if c["id"] == case_id)
    x, gamma, beta = hb.gn_rounded(case, ty)
    out = hb.groupnorm_reference(x, gamma, beta, c0=case["c0"], **hb.gn_kwargs(case))
    return out["ref"], hb.norm_budget(out, gamma, ty)


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("case,form", _params(hb.GN_CASES, hb.GN_FORMS + hb.GN_FORMS_AB))
def test_groupnorm(eng, case, form, ty):
    """Default: gn_partial_kernel at 8 channels per lane + gn_finalize_kernel + gn_apply8_rows_kernel (widths that are no multiple of 8:
    gn_partial_kernel and gn_apply_kernel at 4); FUSED_SMALL = 2: gn_fused_small_kernel; in AB builds
    GN_ROWS = 0: the flat apply pass, GN_COOP = 2: gn_coop_kernel.  One lost, doubled or foreign row, a wrong count or a seam group read
    from one source is at least 4 x over this budget in every sample it touches (host test)."""
    if form in hb.GN_FORMS_AB and not ab_build(eng):
        pytest.skip("this arm was measured and not adopted: `make AB=1` builds only")
    a, s, gamma, beta = hb.gn_inputs(case)
    ref, budget = _gn_ref(case["id"], ty)
    with form_of(eng, ty, form, hb.GN_DEFAULTS) as e:
        y = e.op_groupnorm(a.cuda(), gamma.cuda(), beta.cuda(), samples=case["samples"], P=case["P"], groups=case["groups"], eps=1e-5,
                           silu=case["silu"], x1=s.cuda() if s is not None else None)
    what = f"groupnorm {case['id']} [{ty}, {hb.form_id(form)}]"
    _report(what, hb.assert_within_budget(y, ref, budget, what, hb.where_groupnorm(case)))


@pytest.mark.parametrize("ty", TYPES)
def test_groupnorm_mixed_alignment_dispatch(eng, ty):
    """c0 = 64 takes the 8-channel statistics kernel, c1 = 36 the 4-channel one, the 100-wide output the 4-channel apply pass: every
    element within its budget AND the recorded dispatch (``e2v_op_last_dispatch``) names, source by source, the kernels that ran."""
    case = next(c for c in hb.GN_CASES if c["id"] == "mixed_alignment")
    a, s, gamma, beta = hb.gn_inputs(case)
    ref, budget = _gn_ref(case["id"], ty)
    eng.set_knob("E2V_OP_RECORD", 1)
    try:
        with form_of(eng, ty, {}, hb.GN_DEFAULTS) as e:
            y = e.op_groupnorm(a.cuda(), gamma.cuda(), beta.cuda(), samples=case["samples"], P=case["P"], groups=case["groups"], eps=1e-5,
                               silu=case["silu"], x1=s.cuda())
            tags = e.last_dispatch()
    finally:
        eng.set_knob("E2V_OP_RECORD", 0)
    what = f"groupnorm {case['id']} [{ty}, recorded]"
    _report(what, hb.assert_within_budget(y, ref, budget, what, hb.where_groupnorm(case)))
    for needle in ("gn_partial8_kernel rows64[0]", "gn_partial_kernel rows64[1]", "gn_finalize_kernel", "gn_apply_kernel"):
        assert needle in tags, f"{what}: `{needle}` is not in the recorded dispatch `{tags}`"
    assert "gn_apply8" not in tags and "gn_fused_small" not in tags, f"{what}: the recorded dispatch is `{tags}`"


# ------------------------------------------------------------------ LayerNorm
@functools.lru_cache(maxsize=None)
def _ln_ref(case_id, ty):
    case = next(c for c in hb.LN_CASES if c["id"] == case_id)
    x, gamma, beta = hb.ln_inputs(case)
    out = hb.layernorm_reference(hb.rt(x, ty), gamma, beta)
    return out["ref"], hb.norm_budget(out, gamma, ty)


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("case,form", _params(hb.LN_CASES, hb.LN_FORMS))
def test_layernorm(eng, case, form, ty):
    """C = 320 / 640 / 1280 at 8 / 16 / 32 lanes per row (layernorm_rows_kernel) and, with LN_ROWS = 0, one wave per four rows
    (layernorm_wave_kernel at 8 channels per lane, which C = 64, 768 and 1032 take either way -- one, two and three octets per lane --
    and C = 324 at 4 channels per lane); one row and ragged 5, 9, 17.  No kernel holds a row wider than 1536 columns, and
    the entry point takes none wider than 1280: C = 1544 has to be REFUSED -- the wave-per-row kernels would leave the columns past
    their registers unread and unwritten -- and the output buffer left alone."""
    x, gamma, beta = hb.ln_inputs(case)
    what = f"layernorm {case['id']} [{ty}, {hb.form_id(form)}]"
    with form_of(eng, ty, form, hb.LN_DEFAULTS) as e:
        if case["C"] > hb.LN_MAX_WIDTH:
            out = torch.full(tuple(x.shape), 7.0, device="cuda")
            with pytest.raises((ValueError, RuntimeError)):
                e.op_layernorm(x.cuda(), gamma.cuda(), beta.cuda(), out=out)
            assert bool((out == 7.0).all()), f"{what}: a refused call wrote to its output"
            return
        y = e.op_layernorm(x.cuda(), gamma.cuda(), beta.cuda())
    ref, budget = _ln_ref(case["id"], ty)
    _report(what, hb.assert_within_budget(y, ref, budget, what, hb.where_layernorm(case)))


# ------------------------------------------------------------------ attention
@functools.lru_cache(maxsize=None)
def _sc_ref(case_id, ty):
    case = next(c for c in hb.SC_CASES if c["id"] == case_id)
    qkv = hb.sc_inputs(case)
    c = qkv.shape[1] // 3
    out = hb.sparse_causal_reference(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], ty=ty, **hb.sc_kwargs(case))
    return out["ref"], hb.attention_budget(out, ty)


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("case,form", _params(hb.SC_CASES))
def test_sparse_causal_attention(eng, case, form, ty):
    """d = 40, Nq = 130: flash_attn_b16q64p_kernel (two ragged queries; key stages of 64, 64, 2 per segment), with ATTN_Q64 = 0 the
    32-query flash_attn_b16io_kernel on 64-key stages, with ATTN_KT64 = 0 on 32-key stages; n = 9: the XCD mapping of a sample count
    that is no multiple of 8; d = 80 / 160 / 8: the 32-query kernel at the other head sizes (d = 160: 32-key stages by LDS size).  The V
    rows of the keys at the stage edges are 16 x: a key lost there, for every query or for the ragged query block only, a second segment
    from the wrong frame or a key of the next frame counted in is at least 4 x over the budget in every frame (host test); `kboost`
    cases move the running maximum in the last key stage."""
    qkv = hb.sc_inputs(case).cuda()
    c = qkv.shape[1] // 3
    ref, budget = _sc_ref(case["id"], ty)
    with form_of(eng, ty, form, hb.SC_DEFAULTS) as e:
        y = e.op_attention(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], n=case["n"], F=case["f"], heads=case["heads"], D=case["d"],
                           Nq=case["nq"], Nk=case["nq"], mode=0, scale=case["d"] ** -0.5)
    what = f"sparse-causal attention {case['id']} [{ty}, {hb.form_id(form)}]"
    _report(what, hb.assert_within_budget(y, ref, budget, what, hb.where_attention(case)))


@functools.lru_cache(maxsize=None)
def _cross_ref(case_id, ty):
    case = next(c for c in hb.CROSS_CASES if c["id"] == case_id)
    q, kv = hb.cross_inputs(case)
    c = q.shape[1]
    out = hb.cross_reference(q, kv[:, :c], kv[:, c:], ty=ty, **hb.cross_kwargs(case))
    return out["ref"], hb.attention_budget(out, ty)


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("case,form", _params(hb.CROSS_CASES))
def test_cross_attention(eng, case, form, ty):
    """77 keys and 96 (all three key tiles full), 33, 5; the resident kernel (cross_attn_resident_kernel) and, with
    ATTN_CROSS_RESIDENT = 0, the staged one; 135 query rows per sample: a ragged last 32-row tile."""
    q, kv = hb.cross_inputs(case)
    q, kv = q.cuda(), kv.cuda()
    c = q.shape[1]
    ref, budget = _cross_ref(case["id"], ty)
    with form_of(eng, ty, form, hb.CROSS_DEFAULTS) as e:
        y = e.op_attention(q, kv[:, :c], kv[:, c:], n=case["n"], F=case["f"], heads=case["heads"], D=case["d"], Nq=case["nq"],
                           Nk=case["nk"], mode=1, scale=case["d"] ** -0.5)
    what = f"cross attention {case['id']} [{ty}, {hb.form_id(form)}]"
    _report(what, hb.assert_within_budget(y, ref, budget, what, hb.where_attention(case)))


@functools.lru_cache(maxsize=None)
def _temporal_ref(case_id, ty):
    case = next(c for c in hb.TEMPORAL_CASES if c["id"] == case_id)
    out = hb.temporal_reference(hb.temporal_inputs(case), ty=ty, **hb.temporal_kwargs(case))
    return out["ref"], hb.attention_budget(out, ty)


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("case,form", _params(hb.TEMPORAL_CASES))
def test_temporal_attention(eng, case, form, ty):
    """temporal_attn_wave_kernel and, with TATTN_WAVE = 0, the LDS-staged kernel; 16 frames: the long-clip kernel.  The V rows of the
    first and last frame are 16 x."""
    qkv = hb.temporal_inputs(case).cuda()
    ref, budget = _temporal_ref(case["id"], ty)
    with form_of(eng, ty, form, hb.TEMPORAL_DEFAULTS) as e:
        y = e.op_temporal_attention(qkv, n=case["n"], F=case["f"], HW=case["hw"], heads=case["heads"], D=case["d"], scale=case["d"] ** -0.5)
    what = f"temporal attention {case['id']} [{ty}, {hb.form_id(form)}]"
    _report(what, hb.assert_within_budget(y, ref, budget, what, hb.where_temporal(case)))
