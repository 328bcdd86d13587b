"""``CLIPTextModel`` with the ``transformers`` interface the pipelines use, executed by the HIP library.

Mirror of ``transformers.CLIPTextModel`` as ``EEG2Video/pipelines/pipeline_tuneavideo.py:174-177,220-223`` and
``train_finetune_videodiffusion.py:109,281`` call it: ``from_pretrained(path, subfolder="text_encoder")`` from a LOCAL directory,
``text_encoder(input_ids, attention_mask=None)[0]`` / ``.last_hidden_state``, ``config``, ``dtype``, ``device``, ``to()``,
``requires_grad_()``.  The model lives on an ``Engine`` created with a ``TextConfig`` -- shared with the UNet and the VAE in a pipeline --
and runs in fp32 whatever the engine's compute dtype (``e2v_text_encode``).  No pooled output, no padding mask (the SD text encoder
config has no ``use_attention_mask``), and the weights are frozen once loaded, as they are in the reference's training script (:115).
"""
from __future__ import annotations

import json
import os
from typing import Optional

import torch

from .engine import Engine
from .unet import FrozenDict, _load_checkpoint
from .weights import TEXT_ACTS, TextConfig, UNetConfig, VAEConfig, synth_state_dict, text_param_spec

SAFETENSORS_NAME = "model.safetensors"        # transformers.utils.SAFE_WEIGHTS_NAME
WEIGHTS_NAME = "pytorch_model.bin"            # transformers.utils.WEIGHTS_NAME


class CLIPTextModelOutput:
    """``BaseModelOutputWithPooling`` look-alike without the pooled output: ``out[0]`` and ``out.last_hidden_state``."""

    def __init__(self, last_hidden_state: torch.Tensor):
        self.last_hidden_state = last_hidden_state

    def __getitem__(self, k):
        if k in ("last_hidden_state", 0):
            return self.last_hidden_state
        if isinstance(k, int):
            raise IndexError(k)              # (one element: tuple unpacking stops here)
        raise KeyError(k)

    def to_tuple(self):
        return (self.last_hidden_state,)


class CLIPTextModel:
    #: marks the encoder whose input ids stay on the host (``pipeline_tuneavideo._encode_text``)
    native = True

    def __init__(self, config: TextConfig = TextConfig(), *, engine: Optional[Engine] = None, device: int = 0):
        if config.hidden_act not in TEXT_ACTS:
            raise NotImplementedError(f"hidden_act={config.hidden_act!r}: the text encoder implements {sorted(TEXT_ACTS)}")
        self.tcfg = config
        self._internal_dict = FrozenDict(vocab_size=config.vocab_size, hidden_size=config.hidden, num_attention_heads=config.heads,
                                         num_hidden_layers=config.layers, intermediate_size=config.intermediate,
                                         max_position_embeddings=config.max_positions, hidden_act=config.hidden_act,
                                         layer_norm_eps=config.layer_norm_eps)
        if engine is not None and engine.text_cfg != config:
            raise RuntimeError(f"the engine was created for a text encoder of {engine.text_cfg}, this one is {config}: create the "
                               "engine (or the UNet) with text_config=CLIPTextModel.config_from_dir(<dir>/text_encoder)")
        self.engine = engine if engine is not None else Engine(UNetConfig(), VAEConfig(), device, text_cfg=config)

    @property
    def config(self) -> FrozenDict:
        return self._internal_dict

    @property
    def dtype(self) -> torch.dtype:
        return torch.float32

    @property
    def device(self) -> torch.device:
        return self.engine.device

    def to(self, *a, **k):          # the weights live on the engine's GPU and the arithmetic is fp32 in every mode
        return self

    def eval(self):
        return self

    def requires_grad_(self, flag: bool = False):
        return self

    # -- weights -----------------------------------------------------------------------------
    def state_dict_spec(self):
        return text_param_spec(self.tcfg)

    def load_state_dict(self, state_dict, strict: bool = True):
        """Keys as the checkpoint has them, with or without the ``text_model.`` prefix (``transformers`` 5 dropped it); the
        ``embeddings.position_ids`` buffer of older checkpoints is ignored."""
        spec = self.state_dict_spec()
        sd = {}
        for k, v in state_dict.items():
            if k.endswith("embeddings.position_ids"):
                continue
            sd[k if k.startswith("text_model.") else "text_model." + k] = v
        missing = [k for k in spec if k not in sd]
        unexpected = [k for k in sd if k not in spec]
        if missing or (strict and unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for CLIPTextModel: missing {missing[:4]}... unexpected {unexpected[:4]}...")
        self.engine.load_state_dict({k: sd[k] for k in spec}, prefix="text.")
        self.engine.finalize(Engine.TEXT)
        return self

    def state_dict(self, dtype: torch.dtype = torch.float32, device="cuda"):
        """What the built text encoder holds, read back from the device (``Engine.state_dict``) under the checkpoint's names
        (``text_model.``...); q / k / v projections come out of the fused matrix and bias."""
        from .unet import _model_state_dict
        return _model_state_dict(self.engine, Engine.TEXT, "text.", self.state_dict_spec(), dtype, device)

    def save_pretrained(self, save_directory: str, safe_serialization: bool = True):
        """``config.json`` as ``config_from_dir`` reads it + ``model.safetensors`` (``safe_serialization=False``:
        ``pytorch_model.bin``)."""
        from .unet import _save_checkpoint
        config = {"_class_name": type(self).__name__, "architectures": [type(self).__name__], "model_type": "clip_text_model"}
        config.update(self.config)
        _save_checkpoint(save_directory, config, self.state_dict(device="cpu"), safe_serialization, SAFETENSORS_NAME, WEIGHTS_NAME)

    def init_synthetic(self, seed: int = 44, mode: str = "perturbed"):
        return self.load_state_dict(synth_state_dict(self.state_dict_spec(), seed=seed, mode=mode))

    @staticmethod
    def config_from_dir(path: str) -> TextConfig:
        """``config.json`` of a ``transformers`` ``CLIPTextModel`` directory -> ``TextConfig``."""
        cfg_file = os.path.join(path, "config.json")
        if not os.path.isfile(cfg_file):
            raise RuntimeError(f"{cfg_file} does not exist")
        with open(cfg_file) as f:
            cj = json.load(f)
        cj = cj.get("text_config", cj) if "hidden_size" not in cj else cj       # (a CLIPConfig nests the text tower's)
        d = TextConfig()
        return TextConfig(vocab_size=cj.get("vocab_size", d.vocab_size), hidden=cj.get("hidden_size", d.hidden),
                          heads=cj.get("num_attention_heads", d.heads), layers=cj.get("num_hidden_layers", d.layers),
                          intermediate=cj.get("intermediate_size", d.intermediate),
                          max_positions=cj.get("max_position_embeddings", d.max_positions),
                          hidden_act=cj.get("hidden_act", d.hidden_act), layer_norm_eps=cj.get("layer_norm_eps", d.layer_norm_eps))

    @classmethod
    def from_pretrained(cls, pretrained_model_path: str, subfolder: Optional[str] = "text_encoder", torch_dtype=None, *,
                        engine: Optional[Engine] = None, device: int = 0):
        """Local directory only (``train_finetune_videodiffusion.py:109``): ``config.json`` + ``model.safetensors`` (or
        ``pytorch_model.bin``).  ``torch_dtype`` is accepted for drop-in use: checkpoints of any float type are widened to fp32."""
        path = os.path.join(pretrained_model_path, subfolder) if subfolder else pretrained_model_path
        model = cls(cls.config_from_dir(path), engine=engine, device=device)
        if not os.path.isfile(os.path.join(path, WEIGHTS_NAME)) and not os.path.isfile(os.path.join(path, SAFETENSORS_NAME)):
            raise RuntimeError(f"{os.path.join(path, SAFETENSORS_NAME)} does not exist")
        return model.load_state_dict(_load_checkpoint(path, SAFETENSORS_NAME, WEIGHTS_NAME), strict=False)

    # -- forward -----------------------------------------------------------------------------
    def forward(self, input_ids, attention_mask=None, position_ids=None, return_dict: bool = True, **kwargs):
        if attention_mask is not None:
            raise NotImplementedError("attention_mask: padding masks are not implemented (the SD text encoder runs without one: its "
                                      "config has no use_attention_mask)")
        if position_ids is not None:
            raise NotImplementedError("position_ids other than 0 .. T-1 are not implemented")
        out = self.engine.text_encode(input_ids)
        return CLIPTextModelOutput(out) if return_dict else (out,)

    __call__ = forward
