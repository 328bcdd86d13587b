"""``glfnet`` and ``glfnet_mlp`` -- the reference's GLMNet pair (``EEG2Video/models/models.py:352-413``) on the engine, under the
reference's class names and constructor arguments.  ``glfnet(out_dim, emb_dim, C, T)`` reads raw EEG ``[B, 1, C, T]``; its fast / slow
label selects DANA's ``dynamic_beta``.  ``glfnet_mlp(out_dim, emb_dim, input_dim)`` reads DE features ``[B, C, 5]``
(``eeg2video_amd.features``).

Each loads the reference's checkpoint (a bare ``state_dict()`` or ``{'state_dict': ...}``) with its 24 / 14 names.  The device holds what
inference reads (``Engine.GLM``, keys under ``glm.raw.`` / ``glm.mlp.``); ``num_batches_tracked`` stays on the host, so that
``state_dict()`` gives every entry back bit for bit.  A model makes an engine of its own for its half of the pair; to run both on one
context build ``Engine(..., glmnet_cfg=GLMNetConfig(...))`` with both widths and hand it to both as ``engine=`` -- the part is
finalized when the second one has loaded.

``host_models.GLMNet`` is NOT this model: it is a torch module written from the shapes and left as the sweep's default stage.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import replace
from typing import Optional

import numpy as np
import torch

from .engine import Engine
from .weights import GLMNetConfig, UNetConfig, VAEConfig, glmnet_param_spec, glmnet_synth_state_dict

PREFIX = {"raw": "glm.raw.", "mlp": "glm.mlp."}


class _GLMModel:
    MODEL = ""          # "raw" / "mlp"

    def __init__(self, config: GLMNetConfig, engine: Optional[Engine], device: int):
        other = "mlp_out" if self.MODEL == "raw" else "raw_out"
        if engine is None:
            config = replace(config, **{other: 0})
            engine = Engine(UNetConfig(), VAEConfig(), device, glmnet_cfg=config)
        elif engine.glmnet_cfg is None or replace(engine.glmnet_cfg, **{other: 0}) != replace(config, **{other: 0}):
            raise RuntimeError("the engine was not built with this GLMNet config: create it with Engine(..., glmnet_cfg=config)")
        self.cfg, self.engine = engine.glmnet_cfg, engine
        self._host = OrderedDict()           # what the device does not hold, as loaded
        self._scaler = None

    @property
    def device(self) -> torch.device:
        return self.engine.device

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def requires_grad_(self, flag: bool = False):
        return self

    # -- weights -----------------------------------------------------------------------------
    def state_dict_spec(self):
        return glmnet_param_spec(self.cfg, self.MODEL)

    def load_state_dict(self, state_dict, strict: bool = True):
        """The reference's names, all of them; with ``strict=False`` unknown names are ignored."""
        spec = self.state_dict_spec()
        missing = [k for k in spec if k not in state_dict]
        unexpected = [k for k in state_dict if k not in spec]
        if missing or (strict and unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for {type(self).__name__}: missing {missing[:4]}... unexpected {unexpected[:4]}...")
        as_tensor = lambda v: v.detach().cpu() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))
        host, dev = OrderedDict(), OrderedDict()
        for k, shape in spec.items():
            v = as_tensor(state_dict[k])
            if tuple(v.shape) != tuple(shape):
                raise RuntimeError(f"size mismatch for {k}: {tuple(v.shape)}, expected {tuple(shape)}")
            if k.endswith("num_batches_tracked"):
                host[k] = v.clone()
            else:
                dev[k] = v
        self.engine.load_state_dict(dev, prefix=PREFIX[self.MODEL])
        loaded = getattr(self.engine, "_glm_loaded", set()) | {self.MODEL}
        self.engine._glm_loaded = loaded
        if {m for m, width in (("raw", self.cfg.raw_out), ("mlp", self.cfg.mlp_out)) if width > 0} <= loaded:
            self.engine.finalize(Engine.GLM)
        self._host = host
        return self

    def state_dict(self, device="cpu"):
        """Every entry under the reference's names and in its order: the device's tensors read back (``Engine.read_tensor``),
        ``num_batches_tracked`` as it was loaded."""
        out = OrderedDict()
        for k in self.state_dict_spec():
            out[k] = self._host[k].clone().to(device) if k in self._host else self.engine.read_tensor(PREFIX[self.MODEL] + k).to(device)
        return out

    def save_checkpoint(self, path: str) -> None:
        """``torch.save(model.state_dict(), path)``, as the reference's training scripts save it."""
        torch.save(self.state_dict(device="cpu"), path)

    def init_synthetic(self, seed: int = 47):
        return self.load_state_dict(glmnet_synth_state_dict(self.cfg, self.MODEL, seed=seed))

    @staticmethod
    def _checkpoint(path):
        obj = torch.load(path, map_location="cpu", weights_only=True)
        return obj["state_dict"] if isinstance(obj, dict) and "state_dict" in obj and not isinstance(obj["state_dict"], torch.Tensor) else obj

    # -- forward -----------------------------------------------------------------------------
    def _run(self, x, **want):
        raise NotImplementedError

    def forward(self, x) -> torch.Tensor:
        """The logits ``[B, out_dim]``, the reference's return value."""
        return self._run(x, logits=True)["logits"]

    __call__ = forward

    def embed(self, x) -> torch.Tensor:
        """``[B, 2 emb_dim]``: the global and the occipital embedding side by side, what the head reads."""
        return self._run(x, logits=False, features=True)["features"]

    def predict(self, x) -> torch.Tensor:
        """``[B]`` int32: argmax of the logits, the lowest index among equal maxima."""
        return self._run(x, logits=False, labels=True)["labels"]


class glfnet(_GLMModel):  # noqa: N801  (the reference's name)
    """``glfnet(out_dim, emb_dim, C, T, engine=None, device=0)``.  Only ``T`` = 200 .. 204 give the reference's own linear its width."""
    MODEL = "raw"

    def __init__(self, out_dim: int = 2, emb_dim: int = 64, C: int = 62, T: int = 200, *, config: Optional[GLMNetConfig] = None,
                 engine: Optional[Engine] = None, device: int = 0):
        base = config if config is not None else (engine.glmnet_cfg if engine is not None and engine.glmnet_cfg is not None else GLMNetConfig())
        super().__init__(replace(base, raw_out=out_dim, emb=emb_dim, electrodes=C, samples=T), engine, device)

    @classmethod
    def from_checkpoint(cls, path: str, out_dim: int = 2, emb_dim: int = 64, C: int = 62, T: int = 200, **kw):
        return cls(out_dim, emb_dim, C, T, **kw).load_state_dict(cls._checkpoint(path))

    def set_input_scaler(self, mean=None, scale=None):
        """A per-value scaler ``[C, T]`` (or flat, electrode-major) applied on the device as a value is read, ``(x - mean) / scale``.
        ``None``: no scaler."""
        if (mean is None) != (scale is None):
            raise ValueError("the scaler is a mean AND a scale, or neither")
        if mean is None:
            self._scaler = None
            return self
        shape = (self.cfg.electrodes, self.cfg.samples)
        conv = lambda v: torch.as_tensor(np.asarray(v), dtype=torch.float32).reshape(shape).to(self.device).contiguous()
        self._scaler = (conv(mean), conv(scale))
        return self

    def _run(self, x, **want):
        """``x``: the reference's ``[B, 1, C, T]`` (or ``[B, C, T]``); a raw segment ``[B, C, L]`` with ``L > T`` is read through the
        electrode stride where it lies, its first ``T`` samples."""
        c = self.cfg
        x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if x.dim() == 4 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 3 or x.shape[1] != c.electrodes or x.shape[2] < c.samples:
            raise ValueError(f"expected x [B,1,{c.electrodes},{c.samples}] (or a segment [B,{c.electrodes},L >= {c.samples}]), got {tuple(x.shape)}")
        length = x.shape[2]
        return self.engine.glmnet_raw(x, strides=(c.electrodes * length, length), batch=x.shape[0], scaler=self._scaler, **want)


class glfnet_mlp(_GLMModel):  # noqa: N801  (the reference's name)
    """``glfnet_mlp(out_dim, emb_dim, input_dim, engine=None, device=0)``; ``input_dim`` = electrodes * 5."""
    MODEL = "mlp"

    def __init__(self, out_dim: int = 40, emb_dim: int = 64, input_dim: int = 310, *, config: Optional[GLMNetConfig] = None,
                 engine: Optional[Engine] = None, device: int = 0):
        base = config if config is not None else (engine.glmnet_cfg if engine is not None and engine.glmnet_cfg is not None else GLMNetConfig())
        if input_dim % base.bands:
            raise ValueError(f"input_dim {input_dim} is not electrodes * {base.bands}")
        super().__init__(replace(base, mlp_out=out_dim, emb=emb_dim, electrodes=input_dim // base.bands), engine, device)

    @classmethod
    def from_checkpoint(cls, path: str, out_dim: int = 40, emb_dim: int = 64, input_dim: int = 310, **kw):
        return cls(out_dim, emb_dim, input_dim, **kw).load_state_dict(cls._checkpoint(path))

    def _run(self, x, **want):
        c = self.cfg
        x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if x.dim() == 2 and x.shape[1] == c.electrodes * c.bands:
            x = x.reshape(-1, c.electrodes, c.bands)
        return self.engine.glmnet_mlp(x, **want)
