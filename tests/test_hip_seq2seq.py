"""GPU: the Seq2Seq latent model on the device (``e2v_seq2seq_latents``, ``eeg2video_amd.seq2seq.myTransformer``) against the fixture the
reference's own module wrote and against the float64 full-recompute restatement (``tests/seq2seq_restatement.py``).

Bounds, all as ``max|a - b| / max|b|`` and none fixed here:
* against the fixture: ``10 d``, ``d`` the fixture's own stored distance of the reference's fp32 run from the same module in float64;
* where no reference run exists (the op tests, the tiny configs): ``10 x`` the distance of fp32 torch on the CPU from the float64
  restatement on the same inputs, measured in the test itself.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eeg2video_amd.weights import (SEQ2SEQ_PE_KEY, TINY_SEQ2SEQ, TINY_UNET, TINY_VAE, Seq2SeqConfig, counter_normal, seq2seq_param_spec,
                                   seq2seq_position_table, synth_state_dict)
from seq2seq_restatement import attention, eegnet_features, rel_err, seq2seq_forward
from test_hip_bounds import GUARD_KIB, environment, fenced, fenced_out, guarded_run, run_fenced, same_bits
from test_seq2seq_host import fixture_case, load_fixture

pytestmark = pytest.mark.gpu


def rnd(*shape, seed=0, scale=1.0):
    """float64 holding fp32 values: the device and both references see the same numbers"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).float().double()


def bits(t):
    return t.contiguous().view(torch.int32)


def held(got, want64, want32, what):
    """the device within 10 x the distance of fp32 torch-CPU from float64 (a case torch computes exactly -- one key: the softmax is 1 --
    the device has to compute exactly too)"""
    d = rel_err(want32, want64)
    err = rel_err(got.detach().cpu(), want64)
    print(f"{what}: device vs float64 {err:.3e}, fp32 torch-CPU vs float64 {d:.3e}, bound {10 * d:.3e}")
    assert err <= 10 * d, (what, err, d)


# ------------------------------------------------------------------ engines ---------------------------------------------------------
def tiny_state_dict(cfg, seed=47):
    """synthetic weights with the fixture's treatment: q and k rows of every in_proj x 4, so that softmax rows are far from uniform"""
    sd = synth_state_dict(seq2seq_param_spec(cfg), seed=seed, mode="perturbed")
    del sd[SEQ2SEQ_PE_KEY]
    for k in sd:
        if k.endswith("in_proj_weight"):
            sd[k] = sd[k].copy()
            sd[k][:2 * cfg.d_model] *= 4.0
        if k.endswith("num_batches_tracked"):
            sd[k] = np.zeros((), np.int64)
    return sd


def tiny_inputs(cfg, clips, seed=300):
    return np.stack([counter_normal(seed + b, "eeg", (cfg.windows, cfg.electrodes, cfg.samples)) for b in range(clips)])


_MODELS = {}


def model_of(cfg):
    """one mirror (and engine) per config for the whole module"""
    if cfg not in _MODELS:
        from eeg2video_amd.engine import Engine
        from eeg2video_amd.seq2seq import myTransformer
        eng = Engine(TINY_UNET, TINY_VAE, 0, seq2seq_cfg=cfg)
        sd = fixture_case()[0] if cfg == Seq2SeqConfig() else tiny_state_dict(cfg)
        _MODELS[cfg] = (myTransformer(cfg, engine=eng).load_state_dict(sd), sd)
    return _MODELS[cfg]


@pytest.fixture(scope="module")
def tiny():
    return model_of(TINY_SEQ2SEQ)


@pytest.fixture(scope="module")
def eng(tiny):
    return tiny[0].engine


@pytest.fixture(scope="module")
def tiny_ref(tiny):
    """the float64 restatement of the tiny model over 5 clips, computed once"""
    cfg, src = TINY_SEQ2SEQ, tiny_inputs(TINY_SEQ2SEQ, 5)
    return src, seq2seq_forward(tiny[1], cfg, src, pe=seq2seq_position_table(cfg.windows, cfg.d_model))


def run_all(model, src, **kw):
    x = torch.from_numpy(np.ascontiguousarray(src)).float().cuda()
    c = model.cfg
    kw.setdefault("count", c.steps + 1)
    return model.engine.seq2seq_latents(x, txt_logits=True, tokens=True, **kw)


# ------------------------------------------------------------------ 1. the reference's fixture --------------------------------------
def test_fixture_parity_at_full_size():
    fx = load_fixture()
    cfg = Seq2SeqConfig()
    model, sd = model_of(cfg)
    src = fixture_case()[1]
    out = run_all(model, src)
    torch.cuda.synchronize()
    lat = out["latents"].reshape(2, cfg.steps + 1, -1).cpu()
    idx = torch.from_numpy(fx["latent_idx"])
    for name, got, want in (("tokens", out["tokens"].cpu(), fx["tokens"]), ("txt", out["txt_logits"].cpu(), fx["txt"]),
                            ("latents", lat[:, :, idx], fx["latents_at"])):
        d = float(fx["d64_" + name])
        err = rel_err(got, want)
        print(f"{name}: device vs fixture {err:.3e}, fixture vs float64 {d:.3e}, bound {10 * d:.3e}")
        assert err <= 10 * d, (name, err, d)
    # a zero row through the GEMM adds exact zeros: token 0 of every clip is predictor.bias, bit for bit
    bias = torch.from_numpy(sd["predictor.bias"])
    assert torch.equal(bits(lat[0, 0]), bits(bias)) and torch.equal(bits(lat[1, 0]), bits(bias))
    assert torch.equal(bits(lat[:, 0]), bits(torch.from_numpy(fx["latents_tok0"])))
    # the form inference keeps, without the pass it throws away
    keep = model.predict_latents(src, layout="bfchw")
    assert torch.equal(bits(keep.cpu()), bits(out["latents"][:, :-1].cpu()))


# ------------------------------------------------------------------ 2. the EEGNet embedding kernel ----------------------------------
def eegnet_case(C, T, F1, D, F2, B=2, W=3, step=50, seed=11):
    fd = F1 * D
    w = dict(w1=rnd(F1, 1, 1, 64, seed=seed, scale=0.25), w2=rnd(fd, 1, C, 1, seed=seed + 1, scale=0.5), w3=rnd(fd, 1, 1, 16, seed=seed + 2, scale=0.4),
             w4=rnd(F2, fd, 1, 1, seed=seed + 3, scale=0.3))
    for i, (name, n) in enumerate((("bn1", F1), ("bn2", fd), ("bn3", F2))):
        w[name] = torch.stack([1 + 0.3 * rnd(n, seed=seed + 10 + i), 0.3 * rnd(n, seed=seed + 20 + i), 0.5 * rnd(n, seed=seed + 30 + i),
                               0.5 + torch.rand(n, generator=torch.Generator().manual_seed(seed + 40 + i), dtype=torch.float64)]).float().double()
    seg = rnd(B, C, T + (W - 1) * step, seed=seed + 50)                      # raw segments; window w starts step * w samples in
    win = seg.unfold(2, T, step).permute(0, 2, 1, 3).contiguous()            # [B, W, C, T], the stacked windows
    return w, seg, win


def eegnet_ref(w, win, dtype):
    t = lambda v: v.to(dtype)
    b, nw, c, tt = win.shape
    return eegnet_features(t(win).reshape(b * nw, c, tt), t(w["w1"]), tuple(t(w["bn1"])), t(w["w2"]), tuple(t(w["bn2"])), t(w["w3"]), t(w["w4"]),
                           tuple(t(w["bn3"])))


@pytest.mark.parametrize("F1,D,F2", [(16, 4, 16), (4, 2, 8)])
@pytest.mark.parametrize("C,T", [(5, 32), (5, 39), (62, 100), (3, 127)])
def test_op_eegnet_embed(eng, C, T, F1, D, F2):
    """(5,32): both pools exact, a window shorter than the 64-tap kernel; (5,39): pool-4 remainder 3, then 9 -> 1; (62,100): the
    reference's, one column dropped; (3,127)"""
    B, W = 2, 3
    w, seg, win = eegnet_case(C, T, F1, D, F2, B, W)
    # block 2 before its ELU has both signs (the negative branch of the ELU is exercised)
    f = lambda p: (p[0] / torch.sqrt(p[3] + 1e-5), p[1] - p[2] * p[0] / torch.sqrt(p[3] + 1e-5))
    y = F.conv2d(F.pad(win.reshape(B * W, 1, C, T), (31, 32, 0, 0)), w["w1"])
    y = F.conv2d(y * f(w["bn1"])[0][None, :, None, None] + f(w["bn1"])[1][None, :, None, None], w["w2"], groups=F1)
    y = y * f(w["bn2"])[0][None, :, None, None] + f(w["bn2"])[1][None, :, None, None]
    assert (y < -0.5).any() and (y > 0.5).any()
    want64, want32 = eegnet_ref(w, win, torch.float64), eegnet_ref(w, win, torch.float32)
    kw = dict(B=B, W=W, C=C, T=T, F1=F1, D=D, F2=F2)
    feat = F2 * ((T // 4) // 8)
    fin, out = fenced(win.float(), name="eeg"), fenced_out((B * W, feat))
    got = run_fenced(lambda: eng.op_eegnet_embed(fin.t, w, out=out.t, **kw), [fin], out)
    held(got, want64, want32, f"eegnet C{C} T{T} F{F1}/{D}/{F2}")
    # the raw segment read through strides, windows 200 bytes apart: the same bits as the stacked windows
    L = seg.shape[2]
    fseg, out2 = fenced(seg.float(), name="segment"), fenced_out((B * W, feat))
    got2 = run_fenced(lambda: eng.op_eegnet_embed(fseg.t, w, strides=(C * L, 50, L), out=out2.t, **kw), [fseg], out2)
    assert torch.equal(bits(got2), bits(got))
    # the scaler, applied as a value is staged, against the same ops on (x - mean) / scale
    mean, scale = rnd(W, C, T, seed=91, scale=0.5), 0.5 + torch.rand(W, C, T, generator=torch.Generator().manual_seed(92), dtype=torch.float64)
    mean, scale = mean.float().double(), scale.float().double()              # the values the device sees
    xs = (win.float().double() - mean[None]) / scale[None]
    got3 = eng.op_eegnet_embed(win.float().cuda(), w, scaler=(mean.float(), scale.float()), **kw)
    held(got3, eegnet_ref(w, xs, torch.float64), eegnet_ref(w, xs, torch.float32), "eegnet + scaler")
    assert not torch.equal(bits(got3), bits(got))


# ------------------------------------------------------------------ 3. the attention kernel -----------------------------------------
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("Nq,Nk,pos,causal", [(1, 1, 0, True), (1, 4, 3, True), (1, 7, 6, True), (7, 7, 0, False), (3, 7, 0, True), (7, 7, 0, True)])
@pytest.mark.parametrize("D", [16, 64, 128])
def test_op_seq_attention(eng, D, Nq, Nk, pos, causal, heads, B):
    c = heads * D
    q, k, v = (rnd(B, n, c, seed=s, scale=sc) for n, s, sc in ((Nq, 1, 1.5), (Nk, 2, 1.0), (Nk, 3, 1.0)))
    mask = None
    if causal:                                                       # query i at position pos + i sees keys 0 .. pos + i
        mask = torch.full((Nq, Nk), float("-inf"), dtype=torch.float64).triu(pos + 1)
    want64 = attention(q, k, v, heads, mask)
    want32 = attention(q.float(), k.float(), v.float(), heads, None if mask is None else mask.float())
    pad = 4                                                          # rows 4 floats apart from dense: a slice of a wider buffer
    fq, fk, fv = (fenced(t.reshape(-1, c).float(), ld=c + pad, name=n) for t, n in ((q, "q"), (k, "k"), (v, "v")))
    out = fenced_out((B * Nq, c), ld=c + pad)
    got = run_fenced(lambda: eng.op_seq_attention(fq.t, fk.t, fv.t, B=B, heads=heads, D=D, Nq=Nq, Nk=Nk, q_pos0=pos, causal=causal, out=out.t),
                     [fq, fk, fv], out)
    held(got.reshape(B, Nq, c), want64, want32, f"seq_attn D{D} Nq{Nq} Nk{Nk} pos{pos} causal{int(causal)} h{heads} B{B}")


# ------------------------------------------------------------------ 4. the whole model, tiny configs --------------------------------
@pytest.mark.parametrize("windows,steps,heads,B", [(3, 3, 4, 5), (1, 1, 1, 1), (7, 6, 4, 2), (3, 6, 1, 2), (7, 1, 4, 1), (1, 3, 1, 5)])
def test_tiny_model_against_the_full_recompute_restatement(windows, steps, heads, B):
    """one cached row per pass on the device, every row recomputed in every pass in the restatement: the same model"""
    import dataclasses
    cfg = dataclasses.replace(TINY_SEQ2SEQ, windows=windows, steps=steps, heads=heads)
    model, sd = model_of(cfg)
    src = tiny_inputs(cfg, B)
    pe = seq2seq_position_table(cfg.windows, cfg.d_model)
    r64 = seq2seq_forward(sd, cfg, src, pe=pe)
    r32 = seq2seq_forward(sd, cfg, src, pe=pe, dtype=torch.float32)
    out = run_all(model, src)
    for name, key in (("tokens", "tokens"), ("txt", "txt_logits"), ("latents", "latents")):
        held(out[key], r64[name], r32[name], f"tiny W{windows} S{steps} h{heads} B{B} {name}")


# ------------------------------------------------------------------ 5. slices and layouts -------------------------------------------
def test_slices_layouts_and_single_outputs(tiny, tiny_ref):
    model, _ = tiny
    cfg, src = model.cfg, tiny_ref[0][:2]
    full = run_all(model, src)
    x = torch.from_numpy(src).float().cuda()
    T1 = cfg.steps + 1
    for first in range(T1):
        for count in range(1, T1 - first + 1):
            part = model.engine.seq2seq_latents(x, first=first, count=count, tokens=True)
            assert torch.equal(bits(part["latents"]), bits(full["latents"][:, first:first + count])), (first, count)
            n = first + count                                        # token rows the call computed; the rest stay as they were (zeros)
            assert torch.equal(bits(part["tokens"][:, :n]), bits(full["tokens"][:, :n])) and not part["tokens"][:, n:].any(), (first, count)
            alt = model.engine.seq2seq_latents(x, first=first, count=count, layout="bcfhw")["latents"]
            assert alt.shape == (2, cfg.latent[0], count) + tuple(cfg.latent[1:])
            assert torch.equal(bits(alt), bits(part["latents"].permute(0, 2, 1, 3, 4)))
    only_txt = model.engine.seq2seq_latents(x, latents=False, txt_logits=True)
    only_tok = model.engine.seq2seq_latents(x, count=T1, latents=False, tokens=True)
    only_lat = model.engine.seq2seq_latents(x, count=T1)
    assert set(only_txt) == {"txt_logits"} and torch.equal(bits(only_txt["txt_logits"]), bits(full["txt_logits"]))
    assert set(only_tok) == {"tokens"} and torch.equal(bits(only_tok["tokens"]), bits(full["tokens"]))
    assert set(only_lat) == {"latents"} and torch.equal(bits(only_lat["latents"]), bits(full["latents"]))
    held(full["latents"], tiny_ref[1]["latents"][:2], seq2seq_forward(tiny[1], cfg, src, pe=seq2seq_position_table(cfg.windows, cfg.d_model),
                                                                      dtype=torch.float32)["latents"], "tiny latents")


# ------------------------------------------------------------------ 6. the same bits everywhere -------------------------------------
def test_same_bits_alone_in_a_batch_run_to_run_and_in_every_mode(tiny, tiny_ref):
    model, _ = tiny
    src = tiny_ref[0]
    e = model.engine
    ref = run_all(model, src)
    assert same_bits(list(run_all(model, src).values()), list(ref.values()))                     # run to run
    for b in range(5):                                                                       # a clip alone = the clip at place b of 5
        one = run_all(model, src[b:b + 1])
        for k in ref:
            assert torch.equal(bits(one[k][0]), bits(ref[k][b])), (k, b)
    shuffled = run_all(model, src[[3, 0, 4, 1, 2]])
    for k in ref:
        assert torch.equal(bits(shuffled[k]), bits(ref[k][[3, 0, 4, 1, 2]])), k
    try:
        for mode in ("bf16", "fp16"):
            e.set_compute_dtype(mode)
            assert same_bits(list(run_all(model, src).values()), list(ref.values())), mode
    finally:
        e.set_compute_dtype("fp32")
    before = e.device_bytes()                                        # the workspace of a shape is cached after its first call
    run_all(model, src)
    run_all(model, src[:1])
    torch.cuda.synchronize()
    assert e.device_bytes() == before


def test_outputs_fenced_and_pool_guarded(tiny, tiny_ref):
    from eeg2video_amd.engine import Engine
    from eeg2video_amd.seq2seq import myTransformer
    model, sd = tiny
    cfg, src = model.cfg, tiny_ref[0][:3]
    x = torch.from_numpy(src).float()
    ref = run_all(model, src)
    fin = fenced(x, name="eeg")
    lat, tok, txt = fenced_out((3, cfg.steps + 1) + tuple(cfg.latent)), fenced_out((3, cfg.steps + 1, cfg.d_model)), fenced_out((3, cfg.txt_classes))
    model.engine.seq2seq_latents(fin.t, count=cfg.steps + 1, txt_logits=True, tokens=True, out=dict(latents=lat.t, tokens=tok.t, txt_logits=txt.t))
    torch.cuda.synchronize()
    for f, key in ((fin, None), (lat, "latents"), (tok, "tokens"), (txt, "txt_logits")):
        f.check()
        if key:
            assert torch.equal(bits(f.view.reshape(ref[key].shape)), bits(ref[key])), key
    with environment({}, GUARD_KIB):                                 # an engine whose weight layouts are guarded too
        on = myTransformer(cfg, engine=Engine(TINY_UNET, TINY_VAE, 0, seq2seq_cfg=cfg)).load_state_dict(sd)
    run = lambda e: list(e.seq2seq_latents(x.cuda(), count=cfg.steps + 1, txt_logits=True, tokens=True).values())
    y = guarded_run((model.engine, on.engine), run, what="seq2seq_latents")
    assert same_bits(y, list(ref.values()))


# ------------------------------------------------------------------ 7. errors -------------------------------------------------------
def test_errors_in_order_and_nothing_enqueued(tiny):
    from eeg2video_amd.engine import Engine
    model, _ = tiny
    cfg, e = model.cfg, model.engine
    x = torch.zeros(1, cfg.windows, cfg.electrodes, cfg.samples, device="cuda")
    gets = e.pool_gets()
    for kw in (dict(layout="bchw"), dict(first=-1), dict(count=0), dict(first=2, count=cfg.steps), dict(count=cfg.steps + 2)):
        with pytest.raises(ValueError):
            e.seq2seq_latents(x, **kw)
    with pytest.raises(ValueError):                                  # a scaler of the wrong shape never reaches the library
        e.seq2seq_latents(x, scaler=(torch.zeros(3), torch.ones(3)))
    with pytest.raises(ValueError):
        e.seq2seq_latents(x[0, 0], strides=(0, 1, cfg.samples), batch=1)      # strides past the end of the buffer
    assert e.pool_gets() == gets                                     # nothing was taken from the pool: nothing was enqueued
    fresh = Engine(TINY_UNET, TINY_VAE, 0, seq2seq_cfg=cfg)          # a bad argument first (ValueError), then the state (RuntimeError)
    with pytest.raises(ValueError):
        fresh.seq2seq_latents(x, count=0)
    with pytest.raises(RuntimeError, match="not finalized"):
        fresh.seq2seq_latents(x)
    with pytest.raises(RuntimeError, match="without a Seq2Seq"):
        Engine(TINY_UNET, TINY_VAE, 0).seq2seq_latents(x)
    assert fresh.pool_gets() == 0


# ------------------------------------------------------------------ 8. the mirror ---------------------------------------------------
def test_mirror_checkpoint_round_trip(tiny, tmp_path):
    from eeg2video_amd.seq2seq import Seq2Seq, myTransformer
    model, sd = tiny
    cfg = model.cfg
    assert Seq2Seq is myTransformer
    got = model.state_dict()
    spec = seq2seq_param_spec(cfg)
    assert list(got) == list(spec) and len(got) == 125 - 12 * (2 - cfg.encoder_layers) - 18 * (4 - cfg.decoder_layers)
    for k, v in got.items():
        if k == SEQ2SEQ_PE_KEY:                                      # not in the loaded dict: the reference's expression, all rows
            assert tuple(v.shape) == spec[k] and torch.equal(v[0, :cfg.windows], seq2seq_position_table(cfg.windows, cfg.d_model))
        else:
            want = torch.from_numpy(np.asarray(sd[k]))
            assert v.dtype == want.dtype and torch.equal(v, want), k
    path = str(tmp_path / "seq2seqmodel.pt")
    model.save_checkpoint(path)
    assert set(torch.load(path, weights_only=True)) == {"state_dict"}
    again = myTransformer.from_checkpoint(path, cfg)                 # {'state_dict': ...} as the reference saves it; the full pe buffer inside
    back = again.state_dict()
    assert all(torch.equal(back[k], got[k]) for k in got)
    torch.save(got, path)                                            # a bare state dict loads too
    assert myTransformer.from_checkpoint(path, cfg, engine=again.engine) is not None
    src = tiny_inputs(cfg, 2)
    txt, lat = model(src, torch.zeros((2, cfg.steps + 1) + tuple(cfg.latent)))
    txt2, lat2 = again(src)
    assert txt.shape == (2, cfg.txt_classes) and lat.shape == (2, cfg.steps + 1) + tuple(cfg.latent)
    assert torch.equal(bits(txt), bits(txt2)) and torch.equal(bits(lat), bits(lat2))
    keep = model.predict_latents(src, layout="bfchw")
    assert torch.equal(bits(keep), bits(lat[:, :-1]))
    assert torch.equal(bits(model.predict_latents(src)), bits(lat[:, :-1].permute(0, 2, 1, 3, 4)))
    with pytest.raises(ValueError):
        model(src, torch.zeros(2, 1, 1))
    # a raw segment under the sliding windows = the windows stacked on the host
    seg = counter_normal(5, "segment", (2, cfg.electrodes, cfg.samples + (cfg.windows - 1) * (cfg.samples // 2)))
    stacked = torch.from_numpy(seg).unfold(2, cfg.samples, cfg.samples // 2).permute(0, 2, 1, 3).contiguous()
    assert torch.equal(bits(model.predict_latents(seg)), bits(model.predict_latents(stacked)))
    # read back / update
    e = model.engine
    for k in ("eeg_embedding.block_2.1.running_var", "transformer_decoder.layers.1.multihead_attn.in_proj_weight", "txtpredictor.weight",
              "positional_encoding.pe"):
        want = seq2seq_position_table(cfg.windows, cfg.d_model) if k == SEQ2SEQ_PE_KEY else torch.from_numpy(sd[k])
        assert torch.equal(e.read_tensor("s2s." + k).cpu(), want), k
    with pytest.raises(ValueError, match="finalize_weights"):
        e.update_state_dict({"predictor.bias": torch.zeros(cfg.latent_size)}, prefix="s2s.")


def test_mirror_input_scaler(tiny):
    model, sd = tiny
    cfg = model.cfg
    src = tiny_inputs(cfg, 2, seed=77)
    g = torch.Generator().manual_seed(5)
    n = cfg.electrodes * cfg.samples * cfg.windows
    mean, scale = torch.randn(n, generator=g) * 0.3, torch.rand(n, generator=g) + 0.5          # sklearn's (c l f) feature order
    try:
        model.set_input_scaler(mean.numpy(), scale.numpy())
        got = model.predict_latents(src, layout="bfchw")
    finally:
        model.set_input_scaler(None, None)
    m = mean.double().reshape(cfg.electrodes, cfg.samples, cfg.windows).permute(2, 0, 1)
    s = scale.double().reshape(cfg.electrodes, cfg.samples, cfg.windows).permute(2, 0, 1)
    xs = (torch.from_numpy(src).double() - m[None]) / s[None]
    pe = seq2seq_position_table(cfg.windows, cfg.d_model)
    held(got, seq2seq_forward(sd, cfg, xs, pe=pe)["latents"][:, :-1], seq2seq_forward(sd, cfg, xs, pe=pe, dtype=torch.float32)["latents"][:, :-1],
         "tiny latents under the scaler")


# ------------------------------------------------------------------ 9. the sweep ----------------------------------------------------
def test_sweep_with_the_native_seq2seq_stage(capsys):
    """``examples/run_sweep.py --tiny --seq2seq native``: every stage of a clip is the library's, so a clip's frames are the same bits
    whatever the batching"""
    import json
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "run_sweep.py")
    spec = importlib.util.spec_from_file_location("e2v_sweep_s2s", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.main(["--tiny", "--concepts", "2", "--per-concept", "2", "--batch", "3", "--steps", "2", "--seq2seq", "native"])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["clips"] == 4 and rec["stage_seconds_rank0"]["seq2seq"] > 0
    assert tuple(a.shape) == (4, 3, 3, 32, 48) and a.dtype == torch.uint8
    b = mod.main(["--tiny", "--concepts", "2", "--per-concept", "2", "--batch", "4", "--steps", "2", "--seq2seq", "native"])
    c = mod.main(["--tiny", "--concepts", "2", "--per-concept", "2", "--batch", "1", "--steps", "2", "--seq2seq", "native"])
    assert torch.equal(a, b) and torch.equal(a, c)
