"""GPU: the GLMNet pair on the device (``e2v_glmnet_raw``, ``e2v_glmnet_mlp``, ``eeg2video_amd.glmnet``) against the fixture the
reference's own modules wrote and against the float64 restatement (``tests/glmnet_restatement.py``).

Bounds, all as ``max|a - b| / max|b|`` and none fixed here:
* against the fixture: ``10 d``, ``d`` the fixture's own stored distance of the reference's fp32 run from the same module in float64;
* where no reference run exists (the op tests, the tiny config): ``10 x`` the distance of fp32 torch on the CPU from the float64
  restatement on the same inputs, measured in the test itself.
"""
from dataclasses import replace

import numpy as np
import pytest
import torch

from eeg2video_amd.weights import TINY_GLMNET, TINY_UNET, TINY_VAE, GLMNetConfig, counter_normal, glmnet_param_spec, glmnet_synth_state_dict
import glmnet_restatement as R
from test_eeg_features_host import load_fixture, maker
from test_hip_bounds import GUARD_KIB, environment, fenced, fenced_out, guarded_run, run_fenced, same_bits

pytestmark = pytest.mark.gpu


def rnd(*shape, seed=0, scale=1.0):
    """float64 holding fp32 values: the device and both references see the same numbers"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).float().double()


def bits(t):
    return t.contiguous().view(torch.int32)


def held(got, want64, want32, what):
    d = R.rel_err(want32, want64)
    err = R.rel_err(got.detach().cpu(), want64)
    print(f"{what}: device vs float64 {err:.3e}, fp32 torch-CPU vs float64 {d:.3e}, bound {10 * d:.3e}")
    assert err <= 10 * d, (what, err, d)


# ------------------------------------------------------------------ engines ---------------------------------------------------------
_MODELS = {}


def models_of(cfg):
    """both mirrors on ONE engine per config for the whole module: (glfnet, glfnet_mlp, raw state dict, mlp state dict)"""
    if cfg not in _MODELS:
        from eeg2video_amd.engine import Engine
        from eeg2video_amd.glmnet import glfnet, glfnet_mlp
        eng = Engine(TINY_UNET, TINY_VAE, 0, glmnet_cfg=cfg)
        raw_sd, mlp_sd = glmnet_synth_state_dict(cfg, "raw"), glmnet_synth_state_dict(cfg, "mlp")
        raw = glfnet(cfg.raw_out, cfg.emb, cfg.electrodes, cfg.samples, engine=eng).load_state_dict(raw_sd)
        with pytest.raises(RuntimeError, match="not finalized"):              # the part waits for its second model
            raw(np.zeros((1, 1, cfg.electrodes, cfg.samples), np.float32))
        mlp = glfnet_mlp(cfg.mlp_out, cfg.emb, cfg.electrodes * cfg.bands, engine=eng).load_state_dict(mlp_sd)
        _MODELS[cfg] = (raw, mlp, raw_sd, mlp_sd)
    return _MODELS[cfg]


@pytest.fixture(scope="module")
def tiny():
    return models_of(TINY_GLMNET)


@pytest.fixture(scope="module")
def eng(tiny):
    return tiny[0].engine


def tiny_inputs(clips, seed=400):
    c = TINY_GLMNET
    return (np.stack([counter_normal(seed + b, "eeg", (c.electrodes, c.samples)) for b in range(clips)]),
            np.stack([counter_normal(seed + 50 + b, "de", (c.electrodes, c.bands)) for b in range(clips)]))


@pytest.fixture(scope="module")
def tiny_ref(tiny):
    """the float64 restatement of both tiny models over 5 clips, computed once"""
    c = TINY_GLMNET
    x, de = tiny_inputs(5)
    kw = dict(first=c.occ_first, count=c.occ_count)
    return x, de, R.glfnet(tiny[2], x, eps=c.bn_eps, pool=c.pool, stride=c.pool_stride, **kw), R.glfnet_mlp(tiny[3], de, **kw)


# ------------------------------------------------------------------ 1. the reference's fixture --------------------------------------
def test_fixture_parity_at_full_size():
    fx, mk = load_fixture(), maker()
    raw, mlp, _, _ = models_of(GLMNetConfig())
    x, de = torch.from_numpy(mk.raw_inputs()), torch.from_numpy(mk.mlp_inputs())
    e = raw.engine
    r = e.glmnet_raw(x.cuda(), features=True, labels=True)
    m = e.glmnet_mlp(de.cuda(), features=True, labels=True)
    torch.cuda.synchronize()
    pairs = [("raw_logits", r["logits"]), ("raw_global", r["features"][:, :64]), ("raw_occipital", r["features"][:, 64:]),
             ("mlp_logits", m["logits"]), ("mlp_global", m["features"][:, :64]), ("mlp_occipital", m["features"][:, 64:])]
    # the pooled maps: the kernel of each net on its own, from the same tensors
    for name, first, count in (("globalnet", 0, 62), ("occipital_localnet", 50, 12)):
        sd = R.sub(glmnet_synth_state_dict(GLMNetConfig(), "raw"), name + ".")
        w = dict(w1=torch.from_numpy(sd["net.0.weight"]), b1=torch.from_numpy(sd["net.0.bias"]), w2=torch.from_numpy(sd["net.1.weight"]),
                 b2=torch.from_numpy(sd["net.1.bias"]),
                 bn=torch.stack([torch.from_numpy(sd["net.2." + f]) for f in ("weight", "bias", "running_mean", "running_var")]))
        maps = e.op_shallownet(x.cuda().flatten()[first * 200:], w, B=3, C=count, T=200, F=40, K=25, P=51, S=5, strides=(62 * 200, 200))
        pairs.append(("raw_maps_" + name.split("_")[0].replace("net", ""), maps.reshape(3, 40, 26)))
    for name, got in pairs:
        d = float(fx["d64_" + name])
        err = R.rel_err(got.cpu(), fx[name])
        print(f"{name}: device vs fixture {err:.3e}, fixture vs float64 {d:.3e}, bound {10 * d:.3e}")
        assert err <= 10 * d, (name, err, d)
    assert r["labels"].dtype == torch.int32 and np.array_equal(r["labels"].cpu().numpy(), fx["raw_logits"].argmax(1))
    assert np.array_equal(m["labels"].cpu().numpy(), fx["mlp_logits"].argmax(1))
    # the mirrors on the reference's input shapes
    assert torch.equal(bits(raw(x[:, None])), bits(r["logits"])) and torch.equal(bits(raw.embed(x[:, None])), bits(r["features"]))
    assert torch.equal(raw.predict(x.numpy()[:, None]), r["labels"])
    assert torch.equal(bits(mlp(de)), bits(m["logits"])) and torch.equal(mlp.predict(de.reshape(3, 310)), m["labels"])
    # a raw 2-s segment: its first 200 samples, read where they lie
    seg = torch.cat([x, torch.from_numpy(counter_normal(9, "tail", (3, 62, 200)))], dim=2)
    assert torch.equal(bits(raw(seg)), bits(r["logits"]))


# ------------------------------------------------------------------ 2. the ShallowNet kernel ----------------------------------------
def shallow_case(C, T, F, K, seed=11):
    w = dict(w1=rnd(F, 1, 1, K, seed=seed, scale=0.3), b1=rnd(F, seed=seed + 1, scale=0.2), w2=rnd(F, F, C, 1, seed=seed + 2, scale=0.25),
             b2=rnd(F, seed=seed + 3, scale=0.2))
    w["bn"] = torch.stack([1 + 0.3 * rnd(F, seed=seed + 10), 0.3 * rnd(F, seed=seed + 20), 0.5 * rnd(F, seed=seed + 30),
                           0.5 + torch.rand(F, generator=torch.Generator().manual_seed(seed + 40), dtype=torch.float64)]).float().double()
    sd = {"net.0.weight": w["w1"], "net.0.bias": w["b1"], "net.1.weight": w["w2"], "net.1.bias": w["b2"], "net.2.weight": w["bn"][0],
          "net.2.bias": w["bn"][1], "net.2.running_mean": w["bn"][2], "net.2.running_var": w["bn"][3]}
    return w, sd


@pytest.mark.parametrize("C,first,count,T,F,K,P,S", [
    (5, 0, 5, 40, 8, 5, 7, 3), (5, 2, 3, 40, 8, 5, 7, 3), (5, 0, 5, 41, 8, 5, 7, 3), (5, 2, 3, 41, 8, 5, 7, 3),      # 10 / 11 pooled columns
    (5, 0, 5, 40, 6, 5, 7, 3),                                                                                        # a filter group that runs past F
    (62, 0, 62, 200, 40, 25, 51, 5), (62, 50, 12, 204, 40, 25, 51, 5)])                                               # the reference's
def test_op_shallownet(eng, C, first, count, T, F, K, P, S):
    B = 3
    w, sd = shallow_case(count, T, F, K)
    x = rnd(B, C, T, seed=60 + T)
    sub_x = x[:, first:first + count]
    cols = (T - K + 1 - P) // S + 1
    # before its ELU the map has both signs (the negative branch is exercised)
    pre = R.shallownet_maps_folded(*R.shallownet_fold(sd), sub_x, pool=1, stride=1)
    assert (pre < -0.3).any() and (pre > 0.5).any()
    want64, want32 = (R.shallownet_maps(sd, sub_x, dt, 1e-5, P, S).flatten(1) for dt in (torch.float64, torch.float32))
    kw = dict(B=B, C=count, T=T, F=F, K=K, P=P, S=S)
    fin, out = fenced(x.float(), name="eeg"), fenced_out((B, F * cols))
    src = fin.t.flatten()[first * T:]                                # the occipital rows of the SAME clip, through the electrode stride
    got = run_fenced(lambda: eng.op_shallownet(src, w, strides=(C * T, T), out=out.t, **kw), [fin], out)
    held(got, want64, want32, f"shallownet C{C} [{first}:{first + count}] T{T} F{F}")
    # the input scaler, applied as a value is staged
    mean, scale = rnd(count, T, seed=91, scale=0.5), (0.5 + torch.rand(count, T, generator=torch.Generator().manual_seed(92), dtype=torch.float64)).float().double()
    xs = (sub_x - mean[None]) / scale[None]
    fm, fs = fenced(mean.float(), name="mean"), fenced(scale.float(), name="scale")
    out2 = fenced_out((B, F * cols))
    got2 = run_fenced(lambda: eng.op_shallownet(src, w, strides=(C * T, T), scaler=(fm.t, fs.t), out=out2.t, **kw), [fin, fm, fs], out2)
    held(got2, R.shallownet_maps(sd, xs, torch.float64, 1e-5, P, S).flatten(1), R.shallownet_maps(sd, xs, torch.float32, 1e-5, P, S).flatten(1),
         "shallownet + scaler")
    assert not torch.equal(bits(got2), bits(got))


def test_op_shallownet_refuses_what_does_not_fit(eng):
    w, _ = shallow_case(5, 10, 8, 5)
    x = torch.zeros(1, 5, 10, device="cuda")
    with pytest.raises(ValueError, match="taps \\+ pool - 1"):      # 10 samples: no pooled column
        eng.op_shallownet(x, w, B=1, C=5, T=10, F=8, K=5, P=7, S=3)


# ------------------------------------------------------------------ 3. the tiny models ----------------------------------------------
def test_tiny_models_against_the_restatement(tiny, tiny_ref):
    raw, mlp, raw_sd, mlp_sd = tiny
    c = TINY_GLMNET
    x, de, r64, m64 = tiny_ref
    kw = dict(first=c.occ_first, count=c.occ_count)
    r32 = R.glfnet(raw_sd, x, torch.float32, eps=c.bn_eps, pool=c.pool, stride=c.pool_stride, **kw)
    m32 = R.glfnet_mlp(mlp_sd, de, torch.float32, **kw)
    r = raw.engine.glmnet_raw(torch.from_numpy(x).cuda(), features=True, labels=True)
    m = raw.engine.glmnet_mlp(torch.from_numpy(de).cuda(), features=True, labels=True)
    for name in ("logits", "features"):
        held(r[name], r64[name], r32[name], "tiny glfnet " + name)
        held(m[name], m64[name], m32[name], "tiny glfnet_mlp " + name)
    assert torch.equal(r["labels"].cpu().long(), r64["logits"].argmax(1)) and torch.equal(m["labels"].cpu().long(), m64["logits"].argmax(1))


def test_tied_logits_give_the_lower_index():
    from eeg2video_amd.engine import Engine
    from eeg2video_amd.glmnet import glfnet_mlp
    cfg = replace(TINY_GLMNET, raw_out=0, mlp_out=5)
    sd = glmnet_synth_state_dict(cfg, "mlp")
    sd["out.weight"] = np.zeros_like(sd["out.weight"])
    sd["out.bias"] = np.array([0.5, 2.0, -1.0, 2.0, 2.0], np.float32)       # the maximum three times: index 1 is the label
    model = glfnet_mlp(5, cfg.emb, cfg.electrodes * cfg.bands, config=cfg).load_state_dict(sd)
    de = torch.from_numpy(tiny_inputs(4)[1])
    assert model.predict(de).tolist() == [1, 1, 1, 1]
    assert torch.equal(model(de).cpu(), torch.from_numpy(sd["out.bias"]).expand(4, 5))
    sd["out.bias"] = np.array([3.0, 2.0, -1.0, 3.0, 2.0], np.float32)
    assert glfnet_mlp(5, cfg.emb, cfg.electrodes * cfg.bands, config=cfg, engine=model.engine).load_state_dict(sd).predict(de).tolist() == [0] * 4
    assert isinstance(model.engine, Engine) and model.engine.glmnet_cfg.raw_out == 0


# ------------------------------------------------------------------ 4. same bits ----------------------------------------------------
def run_both(e, x, de):
    r = e.glmnet_raw(x, features=True, labels=True)
    m = e.glmnet_mlp(de, features=True, labels=True)
    return [r["logits"], r["features"], r["labels"].float(), m["logits"], m["features"], m["labels"].float()]


def test_same_bits_alone_in_a_batch_and_in_every_compute_dtype(tiny, tiny_ref):
    e = tiny[0].engine
    x, de = torch.from_numpy(tiny_ref[0]).cuda(), torch.from_numpy(tiny_ref[1]).cuda()
    whole = run_both(e, x, de)
    assert same_bits(run_both(e, x, de), whole)                      # run to run
    for b in range(5):
        alone = run_both(e, x[b:b + 1].contiguous(), de[b:b + 1].contiguous())
        assert same_bits([t[0] for t in alone], [t[b] for t in whole]), b
    for mode in ("bf16", "fp16"):
        try:
            e.set_compute_dtype(mode)
            assert same_bits(run_both(e, x, de), whole), mode
        finally:
            e.set_compute_dtype("fp32")


# ------------------------------------------------------------------ 5. bounds and memory --------------------------------------------
def test_outputs_fenced_pool_guarded_and_steady_state(tiny, tiny_ref):
    from eeg2video_amd.engine import Engine
    from eeg2video_amd.glmnet import glfnet, glfnet_mlp
    raw, mlp, raw_sd, mlp_sd = tiny
    c, e = TINY_GLMNET, raw.engine
    x, de = torch.from_numpy(tiny_ref[0][:3]), torch.from_numpy(tiny_ref[1][:3])
    ref = run_both(e, x.cuda(), de.cuda())
    torch.cuda.synchronize()
    before = e.device_bytes()                                        # the workspace of a batch size is cached after its first call
    run_both(e, x.cuda(), de.cuda())
    torch.cuda.synchronize()
    assert e.device_bytes() == before
    fx_, fde = fenced(x, name="eeg"), fenced(de, name="de")
    lab = torch.full((3 + 2,), -7, dtype=torch.int32, device="cuda")
    for call, fin, width in ((e.glmnet_raw, fx_, c.raw_out), (e.glmnet_mlp, fde, c.mlp_out)):
        lg, ft = fenced_out((3, width)), fenced_out((3, 2 * c.emb))
        call(fin.t, features=True, labels=True, out=dict(logits=lg.t, features=ft.t, labels=lab[1:4]))
        torch.cuda.synchronize()
        for f in (fin, lg, ft):
            f.check()
        assert lab[0] == -7 and lab[4] == -7
        k = 0 if call == e.glmnet_raw else 3
        assert torch.equal(bits(lg.view.reshape(3, width)), bits(ref[k])) and torch.equal(bits(ft.view.reshape(3, 2 * c.emb)), bits(ref[k + 1]))
        assert torch.equal(lab[1:4].float(), ref[k + 2])
    with environment({}, GUARD_KIB):                                 # an engine whose weight layouts are guarded too
        on = Engine(TINY_UNET, TINY_VAE, 0, glmnet_cfg=c)
        glfnet(c.raw_out, c.emb, c.electrodes, c.samples, engine=on).load_state_dict(raw_sd)
        glfnet_mlp(c.mlp_out, c.emb, c.electrodes * c.bands, engine=on).load_state_dict(mlp_sd)
    y = guarded_run((e, on), lambda g: run_both(g, x.cuda(), de.cuda()), what="glmnet_raw + glmnet_mlp")
    assert same_bits(y, ref)


# ------------------------------------------------------------------ 6. errors -------------------------------------------------------
def test_errors_in_order_and_nothing_enqueued(tiny):
    from eeg2video_amd.engine import Engine
    c, e = TINY_GLMNET, tiny[0].engine
    x = torch.zeros(1, c.electrodes, c.samples, device="cuda")
    de = torch.zeros(1, c.electrodes, c.bands, device="cuda")
    gets = e.pool_gets()
    for kw in (dict(scaler=(torch.zeros(3), torch.ones(3))), dict(strides=(0, c.samples)), dict(strides=(c.electrodes * c.samples, c.samples), batch=2),
               dict(strides=(-1, c.samples), batch=1), dict(out=dict(logits=torch.empty(2, c.raw_out, device="cuda"))),
               dict(labels=True, out=dict(labels=torch.empty(1, device="cuda")))):
        with pytest.raises(ValueError):
            e.glmnet_raw(x, **kw)
    for bad in (x[0], x.cpu(), x.double(), torch.zeros(1, c.electrodes, c.samples + 1, device="cuda")):
        with pytest.raises(ValueError):
            e.glmnet_raw(bad)
    with pytest.raises(ValueError, match="no output"):
        e.glmnet_raw(x, logits=False)
    with pytest.raises(ValueError, match="no output"):
        e.glmnet_mlp(de, logits=False)
    with pytest.raises(ValueError):
        e.glmnet_mlp(de[:, :-1].contiguous())
    assert e.pool_gets() == gets                                     # nothing was taken from the pool: nothing was enqueued
    fresh = Engine(TINY_UNET, TINY_VAE, 0, glmnet_cfg=c)             # a bad argument first (ValueError), then the state (RuntimeError)
    with pytest.raises(ValueError, match="no output"):
        fresh.glmnet_raw(x, logits=False)
    with pytest.raises(RuntimeError, match="not finalized"):
        fresh.glmnet_raw(x)
    with pytest.raises(RuntimeError, match="not finalized"):
        fresh.glmnet_mlp(de)
    with pytest.raises(RuntimeError):                                # finalize before the keys are loaded
        fresh.finalize(Engine.GLM)
    assert fresh.pool_gets() == 0
    plain = Engine(TINY_UNET, TINY_VAE, 0)
    with pytest.raises(RuntimeError, match="without a GLMNet"):
        plain.glmnet_raw(x)
    with pytest.raises(ValueError, match="bit mask"):                # bit 256 on a context without the part: outside the mask, as always
        plain.finalize(256)
    with pytest.raises(ValueError, match="bit mask"):
        plain.finalize(128)
    with pytest.raises(ValueError, match="bit mask"):                # a GLMNet context has no bit 128 either
        fresh.finalize(128)
    only = Engine(TINY_UNET, TINY_VAE, 0, glmnet_cfg=replace(c, raw_out=0))
    with pytest.raises(RuntimeError, match="no raw model"):
        only.glmnet_raw(x)


# ------------------------------------------------------------------ 7. the mirrors --------------------------------------------------
def test_mirror_checkpoint_round_trip(tiny, tmp_path):
    from eeg2video_amd.glmnet import glfnet, glfnet_mlp
    raw, mlp, raw_sd, mlp_sd = tiny
    c = TINY_GLMNET
    x, de = tiny_inputs(2, seed=77)
    for model, sd, cls, tag, args, inp in ((raw, raw_sd, glfnet, "raw", (c.raw_out, c.emb, c.electrodes, c.samples), x[:, None]),
                                           (mlp, mlp_sd, glfnet_mlp, "mlp", (c.mlp_out, c.emb, c.electrodes * c.bands), de)):
        got = model.state_dict()
        spec = glmnet_param_spec(c, tag)
        assert list(got) == list(spec) and len(got) == (24 if tag == "raw" else 14)
        for k, v in got.items():
            want = torch.from_numpy(np.asarray(sd[k]))
            assert v.dtype == want.dtype and tuple(v.shape) == spec[k] and torch.equal(v, want), k
        path = str(tmp_path / f"glmnet_{tag}.pt")
        model.save_checkpoint(path)
        again = cls.from_checkpoint(path, *args, config=c)           # an engine of its own, this model alone
        assert (again.cfg.mlp_out if tag == "raw" else again.cfg.raw_out) == 0
        back = again.state_dict()
        assert all(torch.equal(back[k], got[k]) for k in got)
        torch.save({"state_dict": got}, path)                        # the wrapped form loads too
        assert cls.from_checkpoint(path, *args, config=c, engine=again.engine) is not None
        y, y2 = model(inp), again(inp)
        assert tuple(y.shape) == (2, args[0]) and torch.equal(bits(y), bits(y2))
        assert torch.equal(model.predict(inp).cpu().long(), y.cpu().argmax(1))
        with pytest.raises(RuntimeError, match="missing"):
            cls(*args, config=c, engine=again.engine).load_state_dict({k: v for k, v in sd.items() if k != "out.bias"})
    # read back / update
    e = raw.engine
    for k in ("raw.globalnet.net.2.running_var", "raw.occipital_localnet.net.1.weight", "raw.out.weight", "mlp.globalnet.net.1.weight", "mlp.out.bias"):
        tag, name = k.split(".", 1)
        assert torch.equal(e.read_tensor("glm." + k).cpu(), torch.from_numpy((raw_sd if tag == "raw" else mlp_sd)[name])), k
    with pytest.raises(ValueError, match="finalize_weights"):
        e.update_state_dict({"out.bias": torch.zeros(c.raw_out)}, prefix="glm.raw.")
    assert set(e.state_dict(e.GLM, prefix="glm.")) == {"raw." + k for k in raw_sd if not k.endswith("tracked")} | {"mlp." + k for k in mlp_sd}


def test_mirror_input_scaler(tiny):
    raw, _, raw_sd, _ = tiny
    c = TINY_GLMNET
    x = tiny_inputs(2, seed=88)[0]
    g = torch.Generator().manual_seed(5)
    mean, scale = torch.randn(c.electrodes, c.samples, generator=g) * 0.3, torch.rand(c.electrodes, c.samples, generator=g) + 0.5
    try:
        raw.set_input_scaler(mean.numpy().reshape(-1), scale.numpy())
        got = raw(x[:, None])
    finally:
        raw.set_input_scaler(None, None)
    xs = (torch.from_numpy(x).double() - mean.double()[None]) / scale.double()[None]
    kw = dict(eps=c.bn_eps, pool=c.pool, stride=c.pool_stride, first=c.occ_first, count=c.occ_count)
    held(got, R.glfnet(raw_sd, xs, **kw)["logits"], R.glfnet(raw_sd, xs, torch.float32, **kw)["logits"], "tiny glfnet under the scaler")
    assert not torch.equal(bits(got), bits(raw(x[:, None])))


def test_features_feed_the_feature_model(tiny):
    """DE of a window on the device goes into glfnet_mlp as it comes out of the extractor"""
    _, mlp, _, mlp_sd = tiny
    c = TINY_GLMNET
    seg = (20.0 * torch.from_numpy(counter_normal(3, "seg", (2, c.electrodes, 200)))).float()
    de, _ = mlp.engine.eeg_de_psd(seg.cuda().reshape(2, 1, c.electrodes, 200))
    got = mlp(de[:, 0])
    kw = dict(first=c.occ_first, count=c.occ_count)
    held(got, R.glfnet_mlp(mlp_sd, de[:, 0].cpu(), **kw)["logits"], R.glfnet_mlp(mlp_sd, de[:, 0].cpu(), torch.float32, **kw)["logits"], "DE -> glfnet_mlp")


# ------------------------------------------------------------------ 8. the sweep ----------------------------------------------------
def test_sweep_with_the_native_front_end(capsys):
    """``examples/run_sweep.py --tiny --glmnet native --features native`` (with ``--seq2seq native``: the host look-alike of that stage
    is torch and not batch-invariant): the label and the Semantic Predictor's input come from the clip's own raw segment and every model
    stage is the library's, so a clip's frames are the same bits whatever the batching"""
    import importlib.util
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "run_sweep.py")
    spec = importlib.util.spec_from_file_location("e2v_sweep_glm", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    flags = ["--tiny", "--concepts", "2", "--per-concept", "2", "--steps", "2", "--glmnet", "native", "--features", "native", "--seq2seq", "native"]
    a = mod.main(flags + ["--batch", "3"])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["clips"] == 4 and rec["stage_seconds_rank0"]["features"] > 0 and rec["stage_seconds_rank0"]["glmnet"] > 0
    assert tuple(a.shape) == (4, 3, 3, 32, 48) and a.dtype == torch.uint8
    b = mod.main(flags + ["--batch", "4"])
    c = mod.main(flags + ["--batch", "1"])
    assert torch.equal(a, b) and torch.equal(a, c)
    mod.main(["--tiny", "--concepts", "1", "--per-concept", "2", "--steps", "2", "--batch", "2"])      # the default: no such stage
    assert "features" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])["stage_seconds_rank0"]
