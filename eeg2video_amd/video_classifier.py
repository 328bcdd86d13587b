"""``VideoMAEForVideoClassification`` with its ``VideoMAEImageProcessor``, executed by the HIP library.

Mirror of the pair ``EEG2Video/40_class_run_metrics.py:113-118`` builds for ``video_classify_metric``
(``VideoMAEImageProcessor.from_pretrained('MCG-NJU/videomae-base-finetuned-kinetics')`` +
``VideoMAEForVideoClassification.from_pretrained(..., num_frames=6)``), as one object, on the pattern of
``image_classifier.ViTForImageClassification``: ``from_pretrained(local_dir, num_frames=...)`` reads the model AND the processor
config, ``model(frames)`` takes the clips themselves -- uint8 (or float ``[0,1]``), on the device or not -- and returns the logits per
clip; ``classify(frames)`` also returns the softmax and the indices of the three largest logits, which is what the metric uses.  The
model lives on an ``Engine`` created with a ``VideoConfig`` and runs in its OWN arithmetic (``set_compute_dtype``: fp32 by default, opt-in bf16 / fp16) whatever the engine's compute dtype
(``e2v_video_classify``).  The weights are frozen once loaded.

The position table is no checkpoint tensor: ``transformers`` computes the fixed sinusoid at construction, sized by ``num_frames``.
So does this mirror (``weights.video_position_table``, the same numpy formula), which is how ``num_frames=6`` re-sizes it.

Nothing here reads the network: a checkpoint is a LOCAL directory (``config.json``, ``preprocessor_config.json``,
``model.safetensors`` or ``pytorch_model.bin``).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import numpy as np
import torch

from ._tower_model import PROCESSOR_NAME, SAFETENSORS_NAME, WEIGHTS_NAME, _TowerModel
from .engine import Engine
from .image_classifier import ImageClassifierOutput, _BILINEAR
from .unet import FrozenDict, _load_checkpoint
from .weights import (VIDEO_POSITION_KEY, UNetConfig, VAEConfig, VideoConfig, synth_state_dict, video_checkpoint_rename,
                      video_checkpoint_spec, video_engine_shape, video_param_spec, video_position_table)

HUB_NAME = "MCG-NJU/videomae-base-finetuned-kinetics"


class VideoMAEForVideoClassification(_TowerModel):
    _PART = Engine.VIDEO

    def __init__(self, config: VideoConfig = VideoConfig(), *, engine: Optional[Engine] = None, device: int = 0):
        self.vcfg = config
        self._internal_dict = FrozenDict(hidden_size=config.hidden, num_attention_heads=config.heads, num_hidden_layers=config.layers,
                                         intermediate_size=config.intermediate, image_size=config.image_size,
                                         patch_size=config.patch_size, tubelet_size=config.tubelet_size, num_frames=config.num_frames,
                                         num_labels=config.num_labels, num_channels=3, hidden_act="gelu", qkv_bias=True,
                                         use_mean_pooling=True, layer_norm_eps=config.layer_norm_eps)
        if engine is not None and engine.video_cfg != config:
            raise RuntimeError(f"the engine was created for a video classifier of {engine.video_cfg}, this one is {config}: create "
                               "the engine with video_cfg=VideoMAEForVideoClassification.config_from_dir(<dir>)")
        self.engine = engine if engine is not None else Engine(UNetConfig(), VAEConfig(), device, video_cfg=config)

    # -- weights -----------------------------------------------------------------------------
    def state_dict_spec(self):
        """``transformers``' own ``state_dict()`` of this model: no position table, the ``Conv3d`` weight in five axes."""
        return video_checkpoint_spec(self.vcfg)

    def load_state_dict(self, state_dict, strict: bool = True):
        """Keys as the installed ``transformers`` has them, or as the original checkpoint file spells the attention biases
        (``q_bias`` / ``v_bias``, no key bias: ``weights.video_checkpoint_rename``)."""
        spec = self.state_dict_spec()
        sd = video_checkpoint_rename(state_dict)
        missing = [k for k in spec if k not in sd]
        unexpected = [k for k in sd if k not in spec]
        if missing or (strict and unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for VideoMAEForVideoClassification: missing {missing[:4]}... unexpected {unexpected[:4]}...")
        load = OrderedDict()
        for k, shape in video_param_spec(self.vcfg).items():
            if k == VIDEO_POSITION_KEY:
                load[k] = video_position_table(self.vcfg.tokens, self.vcfg.hidden)
                continue
            v = sd[k]
            if tuple(v.shape) != spec[k]:
                raise RuntimeError(f"size mismatch for {k}: the checkpoint has {tuple(v.shape)}, the model {spec[k]}")
            load[k] = v.reshape(video_engine_shape(v.shape))
        self.engine.load_state_dict(load, prefix="video.")
        self.engine.finalize(Engine.VIDEO)
        return self

    def state_dict(self, dtype: torch.dtype = torch.float32, device="cuda"):
        """What the built classifier holds, read back from the device (``Engine.state_dict``) under ``transformers``' names and
        shapes; query / key / value come out of the fused matrix and bias.  The position table is not part of it, as in
        ``transformers`` (``position_embeddings``: the attribute)."""
        from .unet import _model_state_dict
        sd = _model_state_dict(self.engine, Engine.VIDEO, "video.", video_param_spec(self.vcfg), dtype, device)
        return OrderedDict((k, sd[k].reshape(shape)) for k, shape in self.state_dict_spec().items())

    @property
    def position_embeddings(self) -> torch.Tensor:
        """``[1, T, hidden]`` as ``VideoMAEEmbeddings.position_embeddings``, read back from the device"""
        return self.engine.state_dict(Engine.VIDEO, prefix="video.")[VIDEO_POSITION_KEY][None]

    def save_pretrained(self, save_directory: str, safe_serialization: bool = True):
        """``config.json`` and ``preprocessor_config.json`` as ``config_from_dir`` reads them + ``model.safetensors``
        (``safe_serialization=False``: ``pytorch_model.bin``), in the installed ``transformers``' spelling."""
        from .unet import _save_checkpoint
        c = self.vcfg
        config = {"architectures": [type(self).__name__], "model_type": "videomae",
                  "id2label": {str(i): f"LABEL_{i}" for i in range(c.num_labels)}}
        config.update({k: v for k, v in self.config.items() if k != "num_labels"})
        _save_checkpoint(save_directory, config, self.state_dict(device="cpu"), safe_serialization, SAFETENSORS_NAME, WEIGHTS_NAME)
        proc = {"image_processor_type": "VideoMAEImageProcessor", "do_resize": True, "do_center_crop": True, "do_rescale": True,
                "do_normalize": True, "size": {"shortest_edge": c.resize_edge}, "crop_size": {"height": c.image_size, "width": c.image_size},
                "resample": _BILINEAR, "rescale_factor": c.rescale_factor, "image_mean": list(c.image_mean), "image_std": list(c.image_std)}
        self._write_processor(save_directory, proc)

    def init_synthetic(self, seed: int = 46, mode: str = "perturbed"):
        return self.load_state_dict(synth_state_dict(self.state_dict_spec(), seed=seed, mode=mode))

    @staticmethod
    def config_from_dir(path: str, num_frames: Optional[int] = None) -> VideoConfig:
        """``config.json`` + ``preprocessor_config.json`` of a ``transformers`` VideoMAE directory -> ``VideoConfig``;
        ``num_frames`` overrides the config's, as the keyword of ``from_pretrained`` does in ``transformers``."""
        cj, pj = _TowerModel._read_configs(path)
        d = VideoConfig()
        if cj.get("hidden_act", "gelu") != "gelu":
            raise NotImplementedError(f"hidden_act={cj['hidden_act']!r}: the video classifier implements the erf 'gelu'")
        if not cj.get("qkv_bias", True) or cj.get("num_channels", 3) != 3:
            raise NotImplementedError("the video classifier implements biased q / v projections over 3-channel frames")
        if not cj.get("use_mean_pooling", True):
            raise NotImplementedError("use_mean_pooling=false (a final LayerNorm and the first token): the video classifier implements the mean-pooled head")
        if pj.get("resample", _BILINEAR) != _BILINEAR:
            raise NotImplementedError(f"resample={pj['resample']!r}: the preprocess implements Pillow's BILINEAR (2)")
        for flag in ("do_resize", "do_center_crop", "do_rescale", "do_normalize"):
            if not pj.get(flag, True):
                raise NotImplementedError(f"{flag}=false: the preprocess resizes, crops, rescales and normalises")
        image_size = cj.get("image_size", d.image_size)
        size = pj.get("size", {"shortest_edge": d.resize_edge})
        if not isinstance(size, dict) or set(size) != {"shortest_edge"}:
            raise NotImplementedError(f"size={size!r}: the preprocess resizes the shortest edge ({{'shortest_edge': E}})")
        crop = pj.get("crop_size", {"height": image_size, "width": image_size})
        if isinstance(crop, int):
            crop = {"height": crop, "width": crop}
        if crop.get("height") != image_size or crop.get("width") != image_size:
            raise NotImplementedError(f"the processor crops to {crop!r}, the model takes {image_size} x {image_size}")
        if "num_labels" in cj:
            labels = cj["num_labels"]
        elif "id2label" in cj:
            labels = len(cj["id2label"])
        else:
            labels = d.num_labels
        frames = cj.get("num_frames", 16) if num_frames is None else int(num_frames)
        return VideoConfig(hidden=cj.get("hidden_size", d.hidden), heads=cj.get("num_attention_heads", d.heads),
                           layers=cj.get("num_hidden_layers", d.layers), intermediate=cj.get("intermediate_size", d.intermediate),
                           image_size=image_size, patch_size=cj.get("patch_size", d.patch_size),
                           tubelet_size=cj.get("tubelet_size", d.tubelet_size), num_frames=frames, num_labels=labels,
                           layer_norm_eps=cj.get("layer_norm_eps", d.layer_norm_eps), resize_edge=size["shortest_edge"],
                           rescale_factor=pj.get("rescale_factor", d.rescale_factor),
                           image_mean=tuple(pj.get("image_mean", d.image_mean)), image_std=tuple(pj.get("image_std", d.image_std)))

    @classmethod
    def from_pretrained(cls, pretrained_model_path: str, torch_dtype=None, *, num_frames: Optional[int] = None,
                        engine: Optional[Engine] = None, device: int = 0, compute_dtype=None, **kwargs):
        """LOCAL directory only.  ``num_frames`` overrides the checkpoint's (the reference passes 6 where the checkpoint says 16): the
        token count and the position table follow it; the weights do not depend on it.  ``torch_dtype`` and ``cache_dir`` are accepted
        for drop-in use: checkpoints of any float type are widened to fp32, and nothing is ever fetched.  ``compute_dtype``: ``set_compute_dtype`` on the built model (``None``: fp32)."""
        path = str(pretrained_model_path)
        cls._require_dir(path, "classifier", HUB_NAME)
        config = cls.config_from_dir(path, num_frames)
        if config.num_frames < 1 or config.num_frames % config.tubelet_size:
            raise ValueError(f"num_frames={config.num_frames} is not a positive multiple of tubelet_size={config.tubelet_size}")
        model = cls(config, engine=engine, device=device)
        cls._require_weights(path)
        if compute_dtype is not None:
            model.set_compute_dtype(compute_dtype)
        return model.load_state_dict(_load_checkpoint(path, SAFETENSORS_NAME, WEIGHTS_NAME), strict=False)

    # -- forward -----------------------------------------------------------------------------
    def classify(self, frames: torch.Tensor, channels_last: Optional[bool] = None):
        """``(logits, probs, top3)`` of every clip (``Engine.classify_clips``).  ``channels_last=None``: decided by the shape -- a
        last axis of 3 is ``[n,F,H,W,3]`` / ``[F,H,W,3]``, as the reference stacks its frames."""
        if not isinstance(frames, torch.Tensor):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if channels_last is None:
            channels_last = frames.shape[-1] == 3
        f = frames.shape[-4] if channels_last else frames.shape[-3]
        if frames.dim() in (4, 5) and f != self.vcfg.num_frames:
            raise ValueError(f"a clip has {f} frames, the model was built for num_frames={self.vcfg.num_frames} "
                             "(from_pretrained(dir, num_frames=...) sizes the position table)")
        return self.engine.classify_clips(frames, channels_last=channels_last)

    def forward(self, frames, channels_last: Optional[bool] = None, return_dict: bool = True, **kwargs):
        logits = self.classify(frames, channels_last)[0]
        return ImageClassifierOutput(logits) if return_dict else (logits,)

    __call__ = forward
