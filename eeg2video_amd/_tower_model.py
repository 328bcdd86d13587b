"""What the three metric-tower wrappers (``image_classifier``, ``video_classifier``, ``clip_vision``) share: a model whose weights
live on an ``Engine`` part, with its own compute dtype, loaded from and saved to a LOCAL ``transformers`` directory."""
from __future__ import annotations

import json
import os

import torch

from .unet import FrozenDict

SAFETENSORS_NAME = "model.safetensors"        # transformers.utils.SAFE_WEIGHTS_NAME
WEIGHTS_NAME = "pytorch_model.bin"            # transformers.utils.WEIGHTS_NAME
PROCESSOR_NAME = "preprocessor_config.json"   # transformers.utils.IMAGE_PROCESSOR_NAME


class _TowerModel:
    _PART: int                      # the engine part of the subclass: Engine.IMAGE / VIDEO / CLIP_VISION

    @property
    def config(self) -> FrozenDict:
        return self._internal_dict

    @property
    def dtype(self) -> torch.dtype:
        return torch.float32

    @property
    def device(self) -> torch.device:
        return self.engine.device

    def to(self, *a, **k):          # the weights live on the engine's GPU; the arithmetic is chosen by set_compute_dtype alone
        return self

    @property
    def compute_dtype(self) -> str:
        """``'fp32'`` (the default), ``'bf16'`` or ``'fp16'``: the arithmetic of this model on its engine (``Engine.tower_dtype``)."""
        return self.engine.tower_dtype(self._PART)

    def set_compute_dtype(self, dtype):
        """Opt into 16-bit arithmetic for this model alone: ``'fp16'`` (what the reference runs it in,
        ``40_class_run_metrics.py``: ``.to(device, torch.float16)``), ``'bf16'``, or back to ``'fp32'`` -- a name or a ``torch.dtype``
        (``Engine.set_tower_dtype``).  The outputs stay fp32; ``torch_dtype=`` and ``.to()`` do not select it."""
        self.engine.set_tower_dtype(self._PART, dtype)
        return self

    def eval(self):
        return self

    def requires_grad_(self, flag: bool = False):
        return self

    # -- a local ``transformers`` directory ---------------------------------------------------
    @staticmethod
    def _require_dir(path: str, what: str, hub: str) -> None:
        if not os.path.isdir(path):
            raise RuntimeError(f"{path!r} is not a directory: this {what} loads from a local checkpoint directory only and never "
                               f"reads the network (download {hub!r} elsewhere and pass its directory)")

    @staticmethod
    def _require_weights(path: str) -> None:
        if not os.path.isfile(os.path.join(path, WEIGHTS_NAME)) and not os.path.isfile(os.path.join(path, SAFETENSORS_NAME)):
            raise RuntimeError(f"{os.path.join(path, SAFETENSORS_NAME)} does not exist")

    @staticmethod
    def _read_configs(path: str):
        """``(config.json, preprocessor_config.json)`` of the directory, parsed"""
        files = os.path.join(path, "config.json"), os.path.join(path, PROCESSOR_NAME)
        for f in files:
            if not os.path.isfile(f):
                raise RuntimeError(f"{f} does not exist")
        out = []
        for name in files:
            with open(name) as f:
                out.append(json.load(f))
        return out

    @staticmethod
    def _write_processor(save_directory: str, proc: dict) -> None:
        with open(os.path.join(save_directory, PROCESSOR_NAME), "w") as f:
            json.dump(proc, f, indent=2, sort_keys=True)
            f.write("\n")
