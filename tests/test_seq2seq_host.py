"""CPU: the Seq2Seq latent model's host side -- the float64 restatement against the fixture the reference's own module wrote
(``tests/golden/seq2seq_ref.npz``), the key scheme of a host-only ``e2v_create_ex`` context, the config struct and what it refuses, the
argument checks of ``e2v_seq2seq_latents`` that need no GPU, and the scaler reordering.  No GPU work.

Bound (the video tower's rule): the fixture stores, per quantity, the distance ``d`` of the reference's fp32 run from the same module in
float64 (``max|a - b| / max|b|``); whatever is compared with the fixture is held to ``10 d``.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from eeg2video_amd import _lib
from eeg2video_amd.weights import (SEQ2SEQ_PE_KEY, TINY_SEQ2SEQ, Seq2SeqConfig, seq2seq_engine_spec, seq2seq_param_spec,
                                   seq2seq_position_table, seq2seq_unused_key, synth_state_dict)
from seq2seq_restatement import rel_err, seq2seq_forward

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture():
    return np.load(os.path.join(GOLDEN, "seq2seq_ref.npz"))


def fixture_case():
    """the fixture's weights and inputs, rebuilt from their names as the maker builds them"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_seq2seq_golden", os.path.join(GOLDEN, "make_seq2seq_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.fixture_state_dict(), mod.fixture_inputs()


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def s2s_struct(lib, **over):
    s = _lib.E2VS2sConfig()
    lib.e2v_default_s2s_config(C.byref(s))
    for k, v in over.items():
        setattr(s, "s2s_" + k, v)
    return s


def create(lib, s2s, clipv=None):
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    ctx = C.c_void_p()
    st = lib.e2v_create_ex(C.byref(cfg), clipv, C.byref(s2s) if s2s is not None else None, -1, C.byref(ctx))
    return st, ctx


def keys_of(lib, ctx):
    shape, nd = (C.c_int64 * 4)(), C.c_int()
    out = {}
    for i in range(lib.e2v_num_expected_keys(ctx)):
        k = lib.e2v_expected_key(ctx, i, shape, C.byref(nd)).decode()
        out[k] = tuple(shape[d] for d in range(nd.value))
    return out


def test_restatement_matches_the_reference_fixture(fx):
    sd, src = fixture_case()
    cfg = Seq2SeqConfig()
    r = seq2seq_forward(sd, cfg, src, pe=fx["pe"])
    idx = torch.from_numpy(fx["latent_idx"])
    lat = r["latents"].reshape(2, cfg.steps + 1, -1)
    for name, got, want in (("enc_out", r["enc_out"], fx["enc_out"]), ("tokens", r["tokens"], fx["tokens"]), ("txt", r["txt"], fx["txt"]),
                            ("latents", lat[:, :, idx], fx["latents_at"]), ("latents", lat[:, 0], fx["latents_tok0"])):
        d = float(fx["d64_" + name])
        err = rel_err(got, want)
        print(f"{name}: restatement vs fixture {err:.3e}, fixture vs float64 {d:.3e}, bound {10 * d:.3e}")
        assert 0 < d < 1e-5 and err <= 10 * d, (name, err, d)
    # token 0 is the zero row: its latent is predictor.bias, for every clip
    assert np.array_equal(fx["latents_tok0"][0], fx["latents_tok0"][1]) and np.array_equal(fx["latents_tok0"][0], sd["predictor.bias"])
    # the two clips' first predicted frames differ by at least two orders of magnitude more than the bound: what reaches the decoder
    # from the EEG (through the cross-attention alone) is resolved by the comparison, not lost in it
    assert rel_err(lat[0, 1], lat[1, 1]) > 100 * 10 * float(fx["d64_latents"])


def test_positions_matter_to_the_fixture(fx):
    """without the position rows, or with the windows reversed, the restatement leaves the bound by orders of magnitude"""
    sd, src = fixture_case()
    cfg = Seq2SeqConfig()
    bound = 10 * float(fx["d64_tokens"])
    assert rel_err(seq2seq_forward(sd, cfg, src, pe=np.zeros_like(fx["pe"]))["tokens"], fx["tokens"]) > 100 * bound
    assert rel_err(seq2seq_forward(sd, cfg, src[:, ::-1].copy(), pe=fx["pe"])["tokens"], fx["tokens"]) > 100 * bound


def test_param_spec_is_the_reference_state_dict(fx):
    spec = seq2seq_param_spec(Seq2SeqConfig())
    assert list(spec) == [str(k) for k in fx["keys"]] and len(spec) == 125
    shapes = [tuple(int(v) for v in str(s).split(";") if v) for s in fx["shapes"]]
    assert [tuple(v) for v in spec.values()] == shapes
    assert sum(int(np.prod(v)) for v in spec.values()) == 35172112
    assert np.array_equal(seq2seq_position_table(7, 512).numpy(), fx["pe"])             # the mirror's expression gives the buffer's bits
    sd = synth_state_dict(spec, mode="perturbed")
    assert all((v > 0).all() for k, v in sd.items() if k.endswith("running_var"))


def test_config_struct_size_and_defaults(lib):
    assert lib.e2v_s2s_config_size() == C.sizeof(_lib.E2VS2sConfig) == 72
    s = s2s_struct(lib)
    c = Seq2SeqConfig()
    got = (s.s2s_electrodes, s.s2s_samples, s.s2s_windows, s.s2s_f1, s.s2s_d, s.s2s_f2, s.s2s_d_model, s.s2s_heads, s.s2s_ffn,
           s.s2s_encoder_layers, s.s2s_decoder_layers, s.s2s_steps, s.s2s_latent_channels, s.s2s_latent_h, s.s2s_latent_w, s.s2s_txt_classes)
    assert got == (c.electrodes, c.samples, c.windows, c.F1, c.D, c.F2, c.d_model, c.heads, c.ffn, c.encoder_layers, c.decoder_layers,
                   c.steps) + tuple(c.latent) + (c.txt_classes,)
    assert s.s2s_norm_eps == np.float32(1e-5) and s.s2s_bn_eps == np.float32(1e-5)


@pytest.mark.parametrize("cfg", [Seq2SeqConfig(), TINY_SEQ2SEQ], ids=["reference", "tiny"])
def test_host_only_context_lists_the_keys(lib, cfg):
    from eeg2video_amd.engine import seq2seq_config
    st, ctx = create(lib, seq2seq_config(cfg))
    assert st == 0
    try:
        got = {k[4:]: v for k, v in keys_of(lib, ctx).items() if k.startswith("s2s.")}
        want = seq2seq_engine_spec(cfg)
        assert got == dict(want) and list(got) == list(want)
        spec = seq2seq_param_spec(cfg)
        assert set(spec) - set(got) == {k for k in spec if seq2seq_unused_key(k)} and got[SEQ2SEQ_PE_KEY] == (cfg.windows, cfg.d_model)
        assert len(keys_of(lib, ctx)) == 798 + 248 + 10 + len(want)
    finally:
        lib.e2v_destroy(ctx)


def test_create_ex_without_parts_is_create(lib):
    st, ctx = create(lib, None)
    assert st == 0 and lib.e2v_num_expected_keys(ctx) == 798 + 248 + 10
    lib.e2v_destroy(ctx)
    zero = _lib.E2VS2sConfig()
    st, ctx = create(lib, zero)                                  # all zero: no model
    assert st == 0 and lib.e2v_num_expected_keys(ctx) == 798 + 248 + 10
    lib.e2v_destroy(ctx)


@pytest.mark.parametrize("over,words", [
    (dict(heads=3), "multiple of s2s_heads"),
    (dict(d_model=8, heads=4, ffn=8), "multiple of 4, at most 128"),      # head dim 2
    (dict(d_model=1024, heads=4), "at most 128"),                # head dim 256
    (dict(d_model=1284, heads=321), "1280"),
    (dict(windows=33), "at most 32"),
    (dict(steps=32), "at most 32"),
    (dict(ffn=2050), "s2s_ffn"),
    (dict(samples=31), "at least 32"),
    (dict(f2=3), "multiple of 4"),                               # 3 * 3 = 9 features
    (dict(latent_h=3, latent_w=5), "multiple of 4"),
    (dict(electrodes=400), "LDS"),
    (dict(norm_eps=0.0), "positive"),
    (dict(decoder_layers=0), "positive"),
])
def test_bad_configs_are_refused(lib, over, words):
    st, ctx = create(lib, s2s_struct(lib, **over))
    msg = lib.e2v_last_error(None).decode()
    assert st == _lib.E2V_EINVAL and not ctx.value, (over, st)
    assert words in msg, (over, msg)


def test_entry_argument_checks_without_a_gpu(lib):
    """E2V_EINVAL for what is wrong with the call comes first and needs no device; then the state of the context (E2V_ESTATE)"""
    st, ctx = create(lib, s2s_struct(lib))
    st0, plain = create(lib, None)
    assert st == 0 and st0 == 0
    try:
        ok = dict(eeg=0x1000, cs=43400, ws=6200, es=100, mean=None, scale=None, B=1, first=0, count=6, layout=0, lat=0x2000, txt=None, tok=None)

        def call(c, **over):
            a = dict(ok, **over)
            return lib.e2v_seq2seq_latents(c, a["eeg"], a["cs"], a["ws"], a["es"], a["mean"], a["scale"], a["B"], a["first"], a["count"],
                                           a["layout"], a["lat"], a["txt"], a["tok"], None)
        for over in (dict(eeg=None), dict(lat=None), dict(mean=0x3000), dict(scale=0x3000), dict(eeg=0x1002), dict(lat=0x2004), dict(tok=0x2008),
                     dict(txt=0x2001), dict(cs=-1), dict(layout=2), dict(first=-1), dict(count=0), dict(first=2, count=6), dict(count=8), dict(B=0)):
            assert call(ctx, **over) == _lib.E2V_EINVAL, over
            assert lib.e2v_last_error(ctx).decode().startswith("e2v_seq2seq_latents:"), over
        # the order: a bad argument is reported before the missing config / the unfinalized part / the host-only context
        assert call(plain, layout=5) == _lib.E2V_EINVAL
        assert call(plain) == _lib.E2V_ESTATE and "no Seq2Seq" in lib.e2v_last_error(plain).decode()
        assert call(ctx) == _lib.E2V_ESTATE and "not finalized" in lib.e2v_last_error(ctx).decode()
        assert call(ctx, lat=None, txt=0x2004, first=-7, count=99, layout=9) == _lib.E2V_ESTATE      # txt alone: the range is not looked at
        # update is refused for an s2s. key whatever the state
        shape = (C.c_int64 * 1)(512)
        buf = (C.c_float * 512)()
        assert lib.e2v_update_tensor(ctx, b"s2s.predictor.bias", buf, _lib.E2V_F32, 0, shape, 1, None) == _lib.E2V_EINVAL
        assert "e2v_finalize_weights(ctx, 128)" in lib.e2v_last_error(ctx).decode()
    finally:
        lib.e2v_destroy(ctx)
        lib.e2v_destroy(plain)


def test_scaler_reordering_is_standard_scaler():
    """the mirror's [windows, electrodes, samples] view of sklearn's per-feature vectors: transform, un-flatten and move the window axis
    as the reference does (:320-330), against (x - mean) / scale on the stacked windows"""
    from eeg2video_amd.seq2seq import scaler_to_windows
    from sklearn.preprocessing import StandardScaler
    cfg = TINY_SEQ2SEQ
    rng = np.random.default_rng(0)
    c, l, f = cfg.electrodes, cfg.samples, cfg.windows
    eeg = rng.normal(size=(11, c, l, f)) * rng.uniform(0.5, 3.0, size=(1, c, l, f)) + rng.normal(size=(1, c, l, f))      # [b, c, l, f]: windows stacked last
    sc = StandardScaler().fit(eeg.reshape(11, -1))
    ref = sc.transform(eeg.reshape(11, -1)).reshape(11, c, l, f).transpose(0, 3, 1, 2)                                  # 'b c l f -> b f c l'
    mean, scale = scaler_to_windows(sc.mean_, cfg).double().numpy(), scaler_to_windows(sc.scale_, cfg).double().numpy()
    assert mean.shape == (f, c, l)
    got = (eeg.transpose(0, 3, 1, 2) - mean[None]) / scale[None]
    assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()                # (the mirror's vectors are fp32)
    with pytest.raises(ValueError):
        scaler_to_windows(sc.mean_[:-1], cfg)
