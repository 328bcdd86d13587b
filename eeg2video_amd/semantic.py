"""Semantic Predictor ``CLIP`` (the EEG -> CLIP-text-embedding MLP) with the reference's interface, on device.

Mirror of ``EEG2Video/models/train_semantic_predictor.py:11-32`` (same class name, ``forward(eeg)`` returning
``[B, 77*768]``, state-dict keys ``mlp.{0,2,4,6,8}.{weight,bias}``).  This is the step immediately before the hot
path (``pipeline_tuneeeg2video.py:149``); it is a callable, so it drops into ``pipe(model, eeg, ...)`` as ``model``.
"""
from __future__ import annotations

from typing import Optional

import torch

from .engine import Engine, named_tensors
from .weights import SemanticConfig, synth_state_dict, semantic_param_spec


class CLIP:
    def __init__(self, config: SemanticConfig = SemanticConfig(), *, engine: Optional[Engine] = None, device: int = 0):
        self.scfg = config
        self.engine = engine if engine is not None else Engine(device=device, sem_cfg=config)
        if self.engine.sem_cfg != config:
            raise ValueError("the engine was created for a different semantic-predictor config")

    def state_dict_spec(self):
        return semantic_param_spec(self.scfg, self.engine.unet_cfg.cross_attention_dim)

    def load_state_dict(self, state_dict, strict: bool = True):
        sd = state_dict.get("state_dict", state_dict) if isinstance(state_dict, dict) else state_dict   # :146-147 saves {'state_dict': ...}
        spec = self.state_dict_spec()
        missing = [k for k in spec if k not in sd]
        if strict and missing:
            raise RuntimeError(f"Error(s) in loading state_dict for CLIP: missing {missing[:4]}...")
        given = {k: v for k, v in sd.items() if k in spec}
        if missing and self.engine.ready & Engine.SEMANTIC:  # strict=False, some keys of a built model: those tensors move, in place
            self.engine.update_state_dict(given, prefix="semantic.")
            return self
        self.engine.load_state_dict(given, prefix="semantic.")
        self.engine.finalize(Engine.SEMANTIC)
        return self

    def sync_from(self, source, only_trainable: bool = False):
        """Follow the predictor while ``train_semantic_predictor.py`` trains it: the built model takes the tensors of ``source`` (the
        ``nn.Module``, a mapping, or ``(name, tensor)`` pairs) in place, on the current stream (``Engine.update_state_dict``)."""
        spec = self.state_dict_spec()
        self.engine.update_state_dict({k: v for k, v in named_tensors(source, only_trainable) if k in spec}, prefix="semantic.")
        return self

    def state_dict(self, dtype: torch.dtype = torch.float32, device="cuda"):
        """What the built predictor holds now, read back from the device (``Engine.state_dict``): the keys and shapes
        ``train_semantic_predictor.py:146-147`` saves -- the first layer without the K padding the kernels run it with."""
        from .unet import _model_state_dict
        return _model_state_dict(self.engine, Engine.SEMANTIC, "semantic.", self.state_dict_spec(), dtype, device)

    def save_pretrained(self, save_directory: str, safe_serialization: bool = True):
        """``config.json`` (the ``SemanticConfig`` fields and the embedding width) + ``diffusion_pytorch_model.safetensors``
        (``safe_serialization=False``: the ``.bin``), the directory ``from_pretrained`` below reads."""
        from .unet import _save_checkpoint
        config = {"_class_name": type(self).__name__, "in_features": self.scfg.in_features, "hidden": self.scfg.hidden,
                  "tokens": self.scfg.tokens, "cross_attention_dim": self.engine.unet_cfg.cross_attention_dim}
        _save_checkpoint(save_directory, config, self.state_dict(device="cpu"), safe_serialization)

    @classmethod
    def from_pretrained(cls, pretrained_model_path: str, *, engine: Optional[Engine] = None, device: int = 0):
        """A directory written by ``save_pretrained`` (local only)."""
        import json
        import os
        from .unet import _load_checkpoint
        with open(os.path.join(pretrained_model_path, "config.json")) as f:
            cj = json.load(f)
        config = SemanticConfig(in_features=cj["in_features"], hidden=cj["hidden"], tokens=cj["tokens"])
        if engine is None:
            from .weights import UNetConfig
            engine = Engine(UNetConfig(cross_attention_dim=cj.get("cross_attention_dim", UNetConfig.cross_attention_dim)),
                            device=device, sem_cfg=config)
        return cls(config, engine=engine).load_state_dict(_load_checkpoint(pretrained_model_path))

    def init_synthetic(self, seed: int = 44, mode: str = "reference_init"):
        return self.load_state_dict(synth_state_dict(self.state_dict_spec(), seed=seed, mode=mode))

    def cuda(self):
        return self

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def forward(self, eeg: torch.Tensor) -> torch.Tensor:
        return self.engine.semantic_predict(eeg)

    __call__ = forward
