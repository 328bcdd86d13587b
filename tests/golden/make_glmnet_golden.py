"""Writes ``tests/golden/glmnet_ref.npz``: the EEG front end's fixture -- ``DE_PSD``, ``glfnet`` and ``glfnet_mlp`` -- made by the
reference's own code.

Run where a checkout of the reference and torch + scipy + einops are (CPU is enough, it takes a second):
``python tests/golden/make_glmnet_golden.py [REFERENCE_ROOT]`` (default: the ``E2V_REFERENCE`` environment variable).

``EEG_preprocessing/DE_PSD.py`` and ``EEG2Video/models/models.py`` are imported by path and run unmodified, the modules in ``eval()``
under ``no_grad``.

* Weights: ``glmnet_synth_state_dict(GLMNetConfig(), model)`` -- a function of the key names, not stored.  BatchNorm running
  statistics are non-trivial (mean within +-0.16, var 0.5 .. 1.5, gamma 0.75 .. 1.25).
* Inputs, counter-RNG and not stored: 3 clips ``[3, 62, 200]`` (``counter_normal(3026 + clip, "eeg", ...)``) for ``glfnet(2, 64, 62,
  200)``; 3 feature blocks ``[3, 62, 5]`` (``counter_normal(3126 + i, "de", ...)``) for ``glfnet_mlp(40, 64, 310)``; rows ``[62, m]`` of
  N(0, 20^2) (``20 * counter_normal(3226 + m, "rows", ...)``) for ``DE_PSD`` at ``m`` = 100, 200, 400.
* Stored: ``raw_keys`` / ``raw_shapes`` and ``mlp_keys`` / ``mlp_shapes`` (the modules' ``state_dict()`` names in order);
  ``raw_logits`` ``[3, 2]``, ``raw_global`` / ``raw_occipital`` ``[3, 64]`` (the two embeddings), ``raw_maps_global`` /
  ``raw_maps_occipital`` ``[3, 40, 26]`` (the pooled maps, captured by a forward hook on the AvgPool2d); ``mlp_logits`` ``[3, 40]``,
  ``mlp_global`` / ``mlp_occipital`` ``[3, 64]``; ``de_<m>`` / ``psd_<m>`` ``[62, 5]`` as float64, what ``DE_PSD`` returned.
* ``d64_<name>`` for the models: ``max|a - b| / max|b|`` of the fp32 module from the same module in float64 -- the reference's own
  rounding error.  ``DE_PSD`` is float64 already, so its distances are made differently: ``d32_psd_<m>`` (``max |a - b| / |b|``, relative
  per element) and ``d32_de_<m>`` (``max |a - b|``, absolute) of the fp32 index-order restatement
  (``tests/eeg_features_restatement.py``) from ``DE_PSD``; ``r64_psd_<m>`` / ``r64_de_<m>`` the same for the float64 restatement.
The tests take ten times a stored distance as their bound.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from eeg2video_amd.weights import GLMNetConfig, counter_normal, glmnet_param_spec, glmnet_synth_state_dict  # noqa: E402
from eeg_features_restatement import de_psd  # noqa: E402

OUT = os.path.join(HERE, "glmnet_ref.npz")
CLIPS = 3
ROW_LENGTHS = (100, 200, 400)


def raw_inputs(cfg=GLMNetConfig(), clips=CLIPS):
    return np.stack([counter_normal(3026 + b, "eeg", (cfg.electrodes, cfg.samples)) for b in range(clips)])


def mlp_inputs(cfg=GLMNetConfig(), clips=CLIPS):
    return np.stack([counter_normal(3126 + b, "de", (cfg.electrodes, cfg.bands)) for b in range(clips)])


def de_psd_rows(m, electrodes=62):
    return (20.0 * counter_normal(3226 + m, "rows", (electrodes, m))).astype(np.float32)


def load_by_path(ref_root, name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_root, *parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_model(model, sd, x, dtype):
    model = model.eval()
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.to(dtype)
    grabbed, hooks = {}, []
    for name in ("globalnet", "occipital_localnet"):
        net = getattr(model, name)
        hooks.append(net.register_forward_hook(lambda m, i, o, name=name: grabbed.__setitem__(name, o.detach())))
        if isinstance(net.net[4], torch.nn.AvgPool2d):                      # shallownet: the pooled maps in front of the flatten
            hooks.append(net.net[4].register_forward_hook(lambda m, i, o, name=name: grabbed.__setitem__("maps_" + name, o.detach()[:, :, 0])))
    with torch.no_grad():
        logits = model(torch.from_numpy(x).to(dtype))
    for h in hooks:
        h.remove()
    out = {"logits": logits, "global": grabbed["globalnet"], "occipital": grabbed["occipital_localnet"]}
    if "maps_globalnet" in grabbed:
        out["maps_global"], out["maps_occipital"] = grabbed["maps_globalnet"], grabbed["maps_occipital_localnet"]
    keys = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    return out, keys


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("E2V_REFERENCE")
    if not ref_root:
        raise SystemExit("usage: make_glmnet_golden.py REFERENCE_ROOT (or E2V_REFERENCE in the environment)")
    cfg = GLMNetConfig()
    models = load_by_path(ref_root, "ref_glmnet_models", "EEG2Video", "models", "models.py")
    ref_de_psd = load_by_path(ref_root, "ref_de_psd", "EEG_preprocessing", "DE_PSD.py").DE_PSD
    dist = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())
    out = {"torch_version": np.array(torch.__version__)}

    for tag, make, x in (("raw", lambda: models.glfnet(cfg.raw_out, cfg.emb, cfg.electrodes, cfg.samples), raw_inputs(cfg)[:, None]),
                         ("mlp", lambda: models.glfnet_mlp(cfg.mlp_out, cfg.emb, cfg.electrodes * cfg.bands), mlp_inputs(cfg))):
        sd = glmnet_synth_state_dict(cfg, tag)
        r32, keys = run_model(make(), sd, x, torch.float32)
        r64, _ = run_model(make(), sd, x, torch.float64)
        assert [k for k, _ in keys] == list(glmnet_param_spec(cfg, tag)) and dict(keys) == dict(glmnet_param_spec(cfg, tag))
        out[tag + "_keys"] = np.array([k for k, _ in keys])
        out[tag + "_shapes"] = np.array([";".join(str(d) for d in s) for _, s in keys])
        for name in r32:
            out[f"{tag}_{name}"] = r32[name].numpy()
            out[f"d64_{tag}_{name}"] = np.float64(dist(r32[name], r64[name]))
            print(f"{tag}_{name} {tuple(r32[name].shape)}: fp32 module vs float64 module {out[f'd64_{tag}_{name}']:.3e}   "
                  f"max|x| {float(r64[name].abs().max()):.3e}")
        if tag == "raw":
            bn = sd["globalnet.net.2.running_mean"], sd["globalnet.net.2.running_var"]
            print(f"BatchNorm statistics: mean {bn[0].min():.3f} .. {bn[0].max():.3f}, var {bn[1].min():.3f} .. {bn[1].max():.3f}")
            assert np.abs(bn[0]).max() > 0.05 and bn[1].min() >= 0.5 and bn[1].max() <= 2.0

    for m in ROW_LENGTHS:
        rows = de_psd_rows(m, cfg.electrodes)
        de, psd = ref_de_psd(rows.astype(np.float64), 200, m / 200)
        out[f"de_{m}"], out[f"psd_{m}"] = de, psd
        for tag, dtype in (("r64", np.float64), ("d32", np.float32)):
            de_r, psd_r = de_psd(rows, 200, dtype)
            out[f"{tag}_psd_{m}"] = np.float64(np.max(np.abs(psd_r.astype(np.float64) - psd) / np.abs(psd)))
            out[f"{tag}_de_{m}"] = np.float64(np.max(np.abs(de_r.astype(np.float64) - de)))
        print(f"DE_PSD m = {m}: de {de.min():.2f} .. {de.max():.2f}; float64 restatement psd {out[f'r64_psd_{m}']:.2e} rel, de "
              f"{out[f'r64_de_{m}']:.2e} abs; fp32 restatement psd {out[f'd32_psd_{m}']:.2e} rel, de {out[f'd32_de_{m}']:.2e} abs")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
