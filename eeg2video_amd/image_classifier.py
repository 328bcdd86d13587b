"""``ViTForImageClassification`` with its ``ViTImageProcessor``, executed by the HIP library.

Mirror of the pair ``EEG2Video/40_class_run_metrics.py:86-98`` builds for ``img_classify_metric``
(``ViTImageProcessor.from_pretrained('google/vit-base-patch16-224')`` + ``ViTForImageClassification.from_pretrained(...)``), as one
object: ``from_pretrained(local_dir)`` reads the model AND the processor config, ``model(frames)`` takes the frames themselves -- uint8
(or float ``[0,1]``) clips, on the device or not -- and returns the logits; ``classify(frames)`` also returns the softmax and the
indices of the three largest logits, which is what the metric uses.  The model lives on an ``Engine`` created with an ``ImageConfig``
and runs in its OWN arithmetic (``set_compute_dtype``: fp32 by default, opt-in bf16 / fp16) whatever the engine's compute dtype
(``e2v_image_classify``).  The weights are frozen once loaded.

Nothing here reads the network: a checkpoint is a LOCAL directory (``config.json``, ``preprocessor_config.json``,
``model.safetensors`` or ``pytorch_model.bin``), e.g. a ``snapshot_download`` of the hub model made elsewhere.
"""
from __future__ import annotations

from typing import Optional

import torch

from ._tower_model import PROCESSOR_NAME, SAFETENSORS_NAME, WEIGHTS_NAME, _TowerModel
from .engine import Engine
from .unet import FrozenDict, _load_checkpoint
from .weights import ImageConfig, UNetConfig, VAEConfig, image_checkpoint_key, image_param_spec, synth_state_dict

_BILINEAR = 2                                 # PIL.Image.Resampling.BILINEAR, the only resample implemented


class ImageClassifierOutput:
    """``transformers.modeling_outputs.ImageClassifierOutput`` look-alike: ``out.logits``, ``out[0]``, ``out["logits"]``."""

    def __init__(self, logits: torch.Tensor):
        self.logits = logits

    def __getitem__(self, k):
        if k in ("logits", 0):
            return self.logits
        if isinstance(k, int):
            raise IndexError(k)
        raise KeyError(k)

    def to_tuple(self):
        return (self.logits,)


class ViTForImageClassification(_TowerModel):
    _PART = Engine.IMAGE

    def __init__(self, config: ImageConfig = ImageConfig(), *, engine: Optional[Engine] = None, device: int = 0):
        self.icfg = config
        self._internal_dict = FrozenDict(hidden_size=config.hidden, num_attention_heads=config.heads, num_hidden_layers=config.layers,
                                         intermediate_size=config.intermediate, image_size=config.image_size,
                                         patch_size=config.patch_size, num_labels=config.num_labels, num_channels=3,
                                         hidden_act="gelu", qkv_bias=True, layer_norm_eps=config.layer_norm_eps)
        if engine is not None and engine.image_cfg != config:
            raise RuntimeError(f"the engine was created for an image classifier of {engine.image_cfg}, this one is {config}: create "
                               "the engine with image_cfg=ViTForImageClassification.config_from_dir(<dir>)")
        self.engine = engine if engine is not None else Engine(UNetConfig(), VAEConfig(), device, image_cfg=config)

    # -- weights -----------------------------------------------------------------------------
    def state_dict_spec(self):
        return image_param_spec(self.icfg)

    def load_state_dict(self, state_dict, strict: bool = True):
        """Keys as the ``google/vit-base-patch16-224`` checkpoint has them (``vit.encoder.layer.{i}.attention.attention.query`` ...)
        or as ``transformers`` 5 spells the same tensors (``vit.layers.{i}.attention.q_proj``, ``mlp.fc1`` ...)."""
        spec = self.state_dict_spec()
        sd = {image_checkpoint_key(k): v for k, v in state_dict.items()}
        missing = [k for k in spec if k not in sd]
        unexpected = [k for k in sd if k not in spec]
        if missing or (strict and unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for ViTForImageClassification: missing {missing[:4]}... unexpected {unexpected[:4]}...")
        self.engine.load_state_dict({k: sd[k] for k in spec}, prefix="image.")
        self.engine.finalize(Engine.IMAGE)
        return self

    def state_dict(self, dtype: torch.dtype = torch.float32, device="cuda"):
        """What the built classifier holds, read back from the device (``Engine.state_dict``) under the checkpoint's names; query /
        key / value come out of the fused matrix and bias."""
        from .unet import _model_state_dict
        return _model_state_dict(self.engine, Engine.IMAGE, "image.", self.state_dict_spec(), dtype, device)

    def save_pretrained(self, save_directory: str, safe_serialization: bool = True):
        """``config.json`` and ``preprocessor_config.json`` as ``config_from_dir`` reads them + ``model.safetensors``
        (``safe_serialization=False``: ``pytorch_model.bin``), in the checkpoint's spelling."""
        from .unet import _save_checkpoint
        c = self.icfg
        config = {"architectures": [type(self).__name__], "model_type": "vit",
                  "id2label": {str(i): f"LABEL_{i}" for i in range(c.num_labels)}}
        config.update({k: v for k, v in self.config.items() if k != "num_labels"})
        _save_checkpoint(save_directory, config, self.state_dict(device="cpu"), safe_serialization, SAFETENSORS_NAME, WEIGHTS_NAME)
        proc = {"image_processor_type": "ViTImageProcessor", "do_resize": True, "do_rescale": True, "do_normalize": True,
                "size": {"height": c.image_size, "width": c.image_size}, "resample": _BILINEAR, "rescale_factor": c.rescale_factor,
                "image_mean": list(c.image_mean), "image_std": list(c.image_std)}
        self._write_processor(save_directory, proc)

    def init_synthetic(self, seed: int = 45, mode: str = "perturbed"):
        return self.load_state_dict(synth_state_dict(self.state_dict_spec(), seed=seed, mode=mode))

    @staticmethod
    def config_from_dir(path: str) -> ImageConfig:
        """``config.json`` + ``preprocessor_config.json`` of a ``transformers`` ViT directory -> ``ImageConfig``."""
        cj, pj = _TowerModel._read_configs(path)
        d = ImageConfig()
        if cj.get("hidden_act", "gelu") != "gelu":
            raise NotImplementedError(f"hidden_act={cj['hidden_act']!r}: the image classifier implements the erf 'gelu'")
        if not cj.get("qkv_bias", True) or cj.get("num_channels", 3) != 3:
            raise NotImplementedError("the image classifier implements biased q / k / v projections over 3-channel images")
        if pj.get("resample", _BILINEAR) != _BILINEAR:
            raise NotImplementedError(f"resample={pj['resample']!r}: the preprocess implements Pillow's BILINEAR (2)")
        for flag in ("do_resize", "do_rescale", "do_normalize"):
            if not pj.get(flag, True):
                raise NotImplementedError(f"{flag}=false: the preprocess resizes, rescales and normalises")
        size = pj.get("size", cj.get("image_size", d.image_size))
        if isinstance(size, dict):
            if size.get("height") != size.get("width") or size.get("height") is None:
                raise NotImplementedError(f"size={size!r}: the preprocess resizes to a square {{'height': S, 'width': S}}")
            size = size["height"]
        image_size = cj.get("image_size", d.image_size)
        if size != image_size:
            raise NotImplementedError(f"the processor resizes to {size}, the model takes {image_size}: interpolate_pos_encoding is not implemented")
        if "num_labels" in cj:
            labels = cj["num_labels"]
        elif "id2label" in cj:
            labels = len(cj["id2label"])
        else:
            labels = d.num_labels
        return ImageConfig(hidden=cj.get("hidden_size", d.hidden), heads=cj.get("num_attention_heads", d.heads),
                           layers=cj.get("num_hidden_layers", d.layers), intermediate=cj.get("intermediate_size", d.intermediate),
                           image_size=image_size, patch_size=cj.get("patch_size", d.patch_size), num_labels=labels,
                           layer_norm_eps=cj.get("layer_norm_eps", d.layer_norm_eps),
                           rescale_factor=pj.get("rescale_factor", d.rescale_factor),
                           image_mean=tuple(pj.get("image_mean", d.image_mean)), image_std=tuple(pj.get("image_std", d.image_std)))

    @classmethod
    def from_pretrained(cls, pretrained_model_path: str, torch_dtype=None, *, engine: Optional[Engine] = None, device: int = 0,
                        compute_dtype=None, **kwargs):
        """LOCAL directory only.  ``torch_dtype`` and ``cache_dir`` are accepted for drop-in use: checkpoints of any float type are
        widened to fp32, and nothing is ever fetched.  ``compute_dtype``: ``set_compute_dtype`` on the built model (``None``: fp32)."""
        path = str(pretrained_model_path)
        cls._require_dir(path, "classifier", "google/vit-base-patch16-224")
        model = cls(cls.config_from_dir(path), engine=engine, device=device)
        cls._require_weights(path)
        if compute_dtype is not None:
            model.set_compute_dtype(compute_dtype)
        return model.load_state_dict(_load_checkpoint(path, SAFETENSORS_NAME, WEIGHTS_NAME), strict=False)

    # -- forward -----------------------------------------------------------------------------
    def classify(self, frames: torch.Tensor, channels_last: Optional[bool] = None):
        """``(logits, probs, top3)`` of every frame (``Engine.classify_frames``).  ``channels_last=None``: decided by the shape -- a
        last axis of 3 is ``[n,F,H,W,3]`` / ``[F,H,W,3]``, as the reference stacks its frames."""
        if not isinstance(frames, torch.Tensor):
            import numpy as np
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if channels_last is None:
            channels_last = frames.shape[-1] == 3
        return self.engine.classify_frames(frames, channels_last=channels_last)

    def forward(self, frames, channels_last: Optional[bool] = None, return_dict: bool = True, **kwargs):
        logits = self.classify(frames, channels_last)[0]
        return ImageClassifierOutput(logits) if return_dict else (logits,)

    __call__ = forward
