"""CPU: GLMNet's host side -- the float64 restatement (``tests/glmnet_restatement.py``) against the fixture the reference's own modules
wrote (``tests/golden/glmnet_ref.npz``), the BatchNorm fold, the key scheme of a host-only ``e2v_create_ex2`` context, the config struct
and what it refuses, and the argument checks of ``e2v_glmnet_raw`` / ``e2v_glmnet_mlp`` that need no GPU.  No GPU work.

Bound: the fixture stores, per quantity, the distance ``d`` of the reference's fp32 run from the same module in float64
(``max|a - b| / max|b|``); whatever is compared with the fixture is held to ``10 d``.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from eeg2video_amd import _lib
from eeg2video_amd.weights import TINY_GLMNET, GLMNetConfig, glmnet_param_spec, glmnet_synth_state_dict
from glmnet_restatement import glfnet, glfnet_mlp, rel_err, shallownet_fold, shallownet_maps, shallownet_maps_folded, sub
from test_eeg_features_host import load_fixture, maker


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def glm_struct(lib, **over):
    g = _lib.E2VGlmConfig()
    lib.e2v_default_glm_config(C.byref(g))
    for k, v in over.items():
        setattr(g, "glm_" + k, v)
    return g


def create(lib, glm, s2s=None):
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    ctx = C.c_void_p()
    st = lib.e2v_create_ex2(C.byref(cfg), None, C.byref(s2s) if s2s is not None else None, C.byref(glm) if glm is not None else None, -1,
                            C.byref(ctx))
    return st, ctx


def keys_of(lib, ctx):
    shape, nd = (C.c_int64 * 4)(), C.c_int()
    out = {}
    for i in range(lib.e2v_num_expected_keys(ctx)):
        k = lib.e2v_expected_key(ctx, i, shape, C.byref(nd)).decode()
        out[k] = tuple(shape[d] for d in range(nd.value))
    return out


def test_restatement_matches_the_reference_fixture(fx):
    cfg, mk = GLMNetConfig(), maker()
    r = glfnet(glmnet_synth_state_dict(cfg, "raw"), mk.raw_inputs())
    m = glfnet_mlp(glmnet_synth_state_dict(cfg, "mlp"), mk.mlp_inputs())
    pairs = [("raw_logits", r["logits"]), ("raw_global", r["features"][:, :64]), ("raw_occipital", r["features"][:, 64:]),
             ("raw_maps_global", r["maps_global"]), ("raw_maps_occipital", r["maps_occipital"]),
             ("mlp_logits", m["logits"]), ("mlp_global", m["features"][:, :64]), ("mlp_occipital", m["features"][:, 64:])]
    for name, got in pairs:
        d = float(fx["d64_" + name])
        err = rel_err(got, fx[name])
        print(f"{name}: restatement vs fixture {err:.3e}, fixture vs float64 {d:.3e}, bound {10 * d:.3e}")
        assert 0 < d < 1e-5 and err <= 10 * d, (name, err, d)
    assert fx["raw_maps_global"].shape == (3, 40, 26) and fx["raw_logits"].shape == (3, 2) and fx["mlp_logits"].shape == (3, 40)
    # the clips differ by far more than the bound, and the occipital net sees electrodes 50 .. 61 and no others
    assert rel_err(r["logits"][0], r["logits"][1]) > 1000 * float(fx["d64_raw_logits"])
    x = mk.raw_inputs().copy()
    x[:, :50] += 1.0
    assert torch.equal(glfnet(glmnet_synth_state_dict(cfg, "raw"), x)["maps_occipital"], r["maps_occipital"])
    x[:, 61] += 1.0
    assert not torch.equal(glfnet(glmnet_synth_state_dict(cfg, "raw"), x)["maps_occipital"], r["maps_occipital"])


def test_param_spec_is_the_reference_state_dict(fx):
    for tag, count in (("raw", 24), ("mlp", 14)):
        spec = glmnet_param_spec(GLMNetConfig(), tag)
        assert list(spec) == [str(k) for k in fx[tag + "_keys"]] and len(spec) == count
        shapes = [tuple(int(v) for v in str(s).split(";") if v) for s in fx[tag + "_shapes"]]
        assert [tuple(v) for v in spec.values()] == shapes
    sd = glmnet_synth_state_dict(GLMNetConfig(), "raw")
    assert all((v >= 0.5).all() and (v <= 1.5).all() for k, v in sd.items() if k.endswith("running_var"))
    assert all(np.abs(v).max() > 0.05 for k, v in sd.items() if k.endswith("running_mean"))
    assert sd["globalnet.net.2.num_batches_tracked"].dtype == np.int64
    assert GLMNetConfig().pooled_columns == 26 and GLMNetConfig().raw_features == 1040 and TINY_GLMNET.pooled_columns == 10


@pytest.mark.parametrize("cfg,net,C_", [(GLMNetConfig(), "globalnet.", 62), (GLMNetConfig(), "occipital_localnet.", 12), (TINY_GLMNET, "globalnet.", 5)],
                         ids=["global", "occipital", "tiny"])
def test_batchnorm_fold_against_the_unfolded_order(cfg, net, C_):
    """one filter [F][C][taps] + a constant, folded in double, against conv -> conv -> BatchNorm in the reference's order, in double"""
    sd = sub(glmnet_synth_state_dict(cfg, "raw", seed=5), net)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, C_, cfg.samples, generator=g, dtype=torch.float64)
    w, c = shallownet_fold(sd, cfg.bn_eps)
    assert tuple(w.shape) == (cfg.filters, C_, cfg.taps) and tuple(c.shape) == (cfg.filters,)
    want = shallownet_maps(sd, x, torch.float64, cfg.bn_eps, cfg.pool, cfg.pool_stride)
    got = shallownet_maps_folded(w, c, x, cfg.pool, cfg.pool_stride)
    assert tuple(got.shape) == (2, cfg.filters, cfg.pooled_columns)
    assert rel_err(got, want) < 1e-13
    # rounded once to fp32 (what the device holds) the fold stays within a few fp32 roundings of the unfolded double result
    got32 = shallownet_maps_folded(w.float().double(), c.float().double(), x, cfg.pool, cfg.pool_stride)
    assert rel_err(got32, want) < 1e-6


def test_config_struct_size_and_defaults(lib):
    assert lib.e2v_glm_config_size() == C.sizeof(_lib.E2VGlmConfig) == 60
    g = glm_struct(lib)
    c = GLMNetConfig()
    got = (g.glm_electrodes, g.glm_samples, g.glm_occ_first, g.glm_occ_count, g.glm_filters, g.glm_taps, g.glm_pool, g.glm_pool_stride, g.glm_bands,
           g.glm_hidden1, g.glm_hidden2, g.glm_emb, g.glm_raw_out, g.glm_mlp_out)
    assert got == (c.electrodes, c.samples, c.occ_first, c.occ_count, c.filters, c.taps, c.pool, c.pool_stride, c.bands) + tuple(c.hidden) + (
        c.emb, c.raw_out, c.mlp_out)
    assert g.glm_bn_eps == np.float32(1e-5)
    # the older structs keep their size
    assert lib.e2v_s2s_config_size() == 72 and lib.e2v_config_size() == C.sizeof(_lib.E2VConfig)


@pytest.mark.parametrize("cfg", [GLMNetConfig(), TINY_GLMNET], ids=["reference", "tiny"])
@pytest.mark.parametrize("which", ["raw", "mlp", "both"])
def test_host_only_context_lists_the_keys(lib, cfg, which):
    from dataclasses import replace
    from eeg2video_amd.engine import glmnet_config
    if which == "raw":
        cfg = replace(cfg, mlp_out=0)
    if which == "mlp":
        cfg = replace(cfg, raw_out=0)
    st, ctx = create(lib, glmnet_config(cfg))
    assert st == 0, lib.e2v_last_error(None)
    try:
        got = {k: v for k, v in keys_of(lib, ctx).items() if k.startswith("glm.")}
        want = {}
        for tag in ("raw", "mlp"):
            if which in (tag, "both"):
                want.update({f"glm.{tag}.{k}": v for k, v in glmnet_param_spec(cfg, tag).items() if not k.endswith("num_batches_tracked")})
        assert got == want and list(got) == list(want)
        assert len(want) == {"raw": 22, "mlp": 14, "both": 36}[which]
        assert len(keys_of(lib, ctx)) == 798 + 248 + 10 + len(want)
        # (a host-only context refuses every finalize as such; the mask itself is tested on the GPU: tests/test_hip_glmnet.py)
        assert lib.e2v_finalize_weights(ctx, 256) == _lib.E2V_ESTATE and "host-only" in lib.e2v_last_error(ctx).decode()
    finally:
        lib.e2v_destroy(ctx)


def test_contexts_without_the_part_have_no_keys_of_it(lib):
    from test_seq2seq_host import s2s_struct
    for s2s in (None, s2s_struct(lib)):
        for glm in (None, _lib.E2VGlmConfig()):                   # NULL, and all zero: no GLMNet
            st, ctx = create(lib, glm, s2s)
            assert st == 0
            assert not any(k.startswith("glm.") for k in keys_of(lib, ctx))
            assert lib.e2v_finalize_weights(ctx, 256) != _lib.E2V_OK                 # (E2V_EINVAL on a device: tests/test_hip_glmnet.py)
            assert len(keys_of(lib, ctx)) == 798 + 248 + 10 + (119 if s2s is not None else 0)
            lib.e2v_destroy(ctx)
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    ctx = C.c_void_p()
    assert lib.e2v_create_ex(C.byref(cfg), None, None, -1, C.byref(ctx)) == 0      # the older creator forwards with no GLMNet
    assert lib.e2v_num_expected_keys(ctx) == 798 + 248 + 10 and lib.e2v_finalize_weights(ctx, 256) != _lib.E2V_OK
    lib.e2v_destroy(ctx)


@pytest.mark.parametrize("over,words", [
    (dict(raw_out=0, mlp_out=0, emb=8), "not both 0"),
    (dict(raw_out=-1), "not both 0"),
    (dict(taps=0), "positive"),
    (dict(bn_eps=0.0), "positive"),
    (dict(electrodes=5000), "bounded"),
    (dict(occ_first=51), "inside glm_electrodes"),
    (dict(occ_first=0, occ_count=63), "inside glm_electrodes"),
    (dict(emb=66), "multiples of 4"),
    (dict(hidden1=510), "multiples of 4"),
    (dict(samples=74), "at least glm_taps + glm_pool - 1"),
    (dict(samples=205), "1040 * (glm_samples / 200)"),           # 27 columns: 1080 against the reference's 1040
    (dict(samples=400), "1040 * (glm_samples / 200)"),           # 66 columns: 2640 against 2080
    (dict(samples=199), "1040 * (glm_samples / 200)"),           # 25 columns against a linear of width 0
    (dict(filters=7, samples=80), "multiple of 4"),              # 7 * 2 = 14
    (dict(electrodes=4096, occ_first=0, samples=204), "LDS"),
])
def test_bad_configs_are_refused(lib, over, words):
    st, ctx = create(lib, glm_struct(lib, **over))
    msg = lib.e2v_last_error(None).decode()
    assert st == _lib.E2V_EINVAL and not ctx.value, (over, st)
    assert words in msg, (over, msg)


def test_accepted_sample_counts(lib):
    for samples in (200, 202, 204):                              # the reference's own range: 26 columns each
        st, ctx = create(lib, glm_struct(lib, samples=samples))
        assert st == 0, (samples, lib.e2v_last_error(None))
        lib.e2v_destroy(ctx)
    st, ctx = create(lib, glm_struct(lib, samples=400, raw_out=0))      # without a raw model the sample count binds nothing
    assert st == 0
    lib.e2v_destroy(ctx)


def test_entry_argument_checks_without_a_gpu(lib):
    """E2V_EINVAL for what is wrong with the call comes first and needs no device; then the state of the context (E2V_ESTATE)"""
    st, ctx = create(lib, glm_struct(lib))
    st0, plain = create(lib, None)
    st1, mlp_only = create(lib, glm_struct(lib, raw_out=0))
    assert st == 0 and st0 == 0 and st1 == 0
    try:
        ok = dict(eeg=0x1000, cs=12400, es=200, B=1, mean=None, scale=None, lg=0x2000, ft=None, lb=None)

        def raw(c, **over):
            a = dict(ok, **over)
            return lib.e2v_glmnet_raw(c, a["eeg"], a["cs"], a["es"], a["B"], a["mean"], a["scale"], a["lg"], a["ft"], a["lb"], None)
        for over in (dict(eeg=None), dict(lg=None), dict(mean=0x3000), dict(scale=0x3000), dict(eeg=0x1002), dict(lg=0x2001), dict(ft=0x2002),
                     dict(lb=0x2003), dict(cs=-1), dict(es=-1), dict(B=0)):
            assert raw(ctx, **over) == _lib.E2V_EINVAL, over
            assert lib.e2v_last_error(ctx).decode().startswith("e2v_glmnet_raw:"), over
        assert raw(plain, B=0) == _lib.E2V_EINVAL                 # a bad argument before the missing part
        assert raw(plain) == _lib.E2V_ESTATE and "no GLMNet" in lib.e2v_last_error(plain).decode()
        assert raw(mlp_only) == _lib.E2V_ESTATE and "no raw model" in lib.e2v_last_error(mlp_only).decode()
        assert raw(ctx) == _lib.E2V_ESTATE and "not finalized" in lib.e2v_last_error(ctx).decode()
        assert raw(ctx, lg=None, lb=0x2004) == _lib.E2V_ESTATE

        def mlp(c, de=0x1000, B=1, lg=0x2000, ft=None, lb=None):
            return lib.e2v_glmnet_mlp(c, de, B, lg, ft, lb, None)
        for kw in (dict(de=None), dict(lg=None), dict(de=0x1001), dict(lg=0x2002), dict(B=0)):
            assert mlp(ctx, **kw) == _lib.E2V_EINVAL, kw
            assert lib.e2v_last_error(ctx).decode().startswith("e2v_glmnet_mlp:"), kw
        assert mlp(plain) == _lib.E2V_ESTATE and "no GLMNet" in lib.e2v_last_error(plain).decode()
        assert mlp(ctx) == _lib.E2V_ESTATE and "not finalized" in lib.e2v_last_error(ctx).decode()
        assert mlp(mlp_only) == _lib.E2V_ESTATE and "not finalized" in lib.e2v_last_error(mlp_only).decode()
        assert lib.e2v_glmnet_raw(None, 0x1000, 0, 0, 1, None, None, 0x2000, None, None, None) == _lib.E2V_EINVAL
        # update is refused for a glm. key whatever the state
        shape = (C.c_int64 * 1)(2)
        buf = (C.c_float * 2)()
        assert lib.e2v_update_tensor(ctx, b"glm.raw.out.bias", buf, _lib.E2V_F32, 0, shape, 1, None) == _lib.E2V_EINVAL
        assert "e2v_finalize_weights(ctx, 256)" in lib.e2v_last_error(ctx).decode()
    finally:
        for c in (ctx, plain, mlp_only):
            lib.e2v_destroy(c)
