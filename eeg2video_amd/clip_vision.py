"""``CLIPVisionModelWithProjection`` with its ``CLIPImageProcessor``, executed by the HIP library.

Mirror of the pair the reference's ``clip_score`` builds (``EEG2Video/40_class_run_metrics.py:40-42``:
``CLIPVisionModelWithProjection.from_pretrained("openai/clip-vit-base-patch32")`` + ``AutoProcessor.from_pretrained(...)``), as one
object: ``from_pretrained(local_dir)`` reads the model AND the processor config, ``model(frames)`` takes the frames themselves -- uint8
(or float ``[0,1]``) clips, on the device or not -- and ``.image_embeds`` of the result are the projected class embeddings, not
normalised.  The model lives on an ``Engine`` created with a ``ClipVisionConfig`` and runs in its OWN arithmetic (``set_compute_dtype``: fp32 by default, opt-in bf16 / fp16) whatever the engine's compute dtype
(``e2v_clip_embed``).

Nothing here reads the network: a checkpoint is a LOCAL directory (``config.json`` -- a ``CLIPVisionConfig`` or a full ``CLIPConfig``
with ``vision_config`` --, ``preprocessor_config.json``, ``model.safetensors`` or ``pytorch_model.bin``), e.g. a ``snapshot_download``
of the hub model made elsewhere.  A full CLIP checkpoint's text tower, ``logit_scale`` and ``position_ids`` buffers are ignored.
"""
from __future__ import annotations

from typing import Optional

import torch

from ._tower_model import PROCESSOR_NAME, SAFETENSORS_NAME, WEIGHTS_NAME, _TowerModel
from .engine import Engine, named_tensors
from .unet import FrozenDict, _load_checkpoint
from .weights import TEXT_ACTS, ClipVisionConfig, UNetConfig, VAEConfig, clip_vision_param_spec, synth_state_dict

_RESAMPLES = (2, 3)                           # PIL.Image.Resampling.BILINEAR / BICUBIC: the filters the resize tables have
_MAX_TOKENS = 288                             # kImageAttnMaxT: the attention kernel keeps K and V of an image's head in LDS


class CLIPVisionModelOutput:
    """``transformers.models.clip.modeling_clip.CLIPVisionModelOutput`` look-alike: ``out.image_embeds``, ``out[0]``,
    ``out["image_embeds"]``."""

    def __init__(self, image_embeds: torch.Tensor):
        self.image_embeds = image_embeds

    def __getitem__(self, k):
        if k in ("image_embeds", 0):
            return self.image_embeds
        if isinstance(k, int):
            raise IndexError(k)
        raise KeyError(k)

    def to_tuple(self):
        return (self.image_embeds,)


class CLIPVisionModelWithProjection(_TowerModel):
    _PART = Engine.CLIP_VISION

    def __init__(self, config: ClipVisionConfig = ClipVisionConfig(), *, engine: Optional[Engine] = None, device: int = 0):
        self.ccfg = config
        self._internal_dict = FrozenDict(hidden_size=config.hidden, num_attention_heads=config.heads, num_hidden_layers=config.layers,
                                         intermediate_size=config.intermediate, image_size=config.image_size,
                                         patch_size=config.patch_size, projection_dim=config.projection_dim, num_channels=3,
                                         hidden_act=config.hidden_act, layer_norm_eps=config.layer_norm_eps)
        if engine is not None and engine.clip_vision_cfg != config:
            raise RuntimeError(f"the engine was created for a CLIP vision tower of {engine.clip_vision_cfg}, this one is {config}: "
                               "create the engine with clip_vision_cfg=CLIPVisionModelWithProjection.config_from_dir(<dir>)")
        self.engine = engine if engine is not None else Engine(UNetConfig(), VAEConfig(), device, clip_vision_cfg=config)

    # -- weights -----------------------------------------------------------------------------
    def state_dict_spec(self):
        return clip_vision_param_spec(self.ccfg)

    def load_state_dict(self, state_dict, strict: bool = True):
        """Keys as the ``openai/clip-vit-base-patch32`` checkpoint has them (``vision_model.encoder.layers.{i}.self_attn.q_proj`` ...).
        ``position_ids`` buffers are not weights and are skipped; with ``strict=False`` so is everything else the tower does not
        have (a full CLIP checkpoint's ``text_model.*``, ``text_projection.weight``, ``logit_scale``)."""
        spec = self.state_dict_spec()
        sd = {k: v for k, v in state_dict.items() if not k.endswith("position_ids")}
        missing = [k for k in spec if k not in sd]
        unexpected = [k for k in sd if k not in spec]
        if missing or (strict and unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for CLIPVisionModelWithProjection: missing {missing[:4]}... unexpected {unexpected[:4]}...")
        self.engine.load_state_dict({k: sd[k] for k in spec}, prefix="clipv.")
        self.engine.finalize(Engine.CLIP_VISION)
        return self

    def sync_from(self, source, only_trainable: bool = False):
        """Bring the built tower to the tensors of ``source`` (an ``nn.Module``, a mapping, or ``(name, tensor)`` pairs) in place, on the
        current stream (``Engine.update_state_dict``); names this model does not have are ignored."""
        spec = self.state_dict_spec()
        self.engine.update_state_dict({k: v for k, v in named_tensors(source, only_trainable) if k in spec}, prefix="clipv.")
        return self

    def state_dict(self, dtype: torch.dtype = torch.float32, device="cuda"):
        """What the built tower holds NOW, read back from the device (``Engine.state_dict``) under the checkpoint's names; q / k / v come
        out of the fused matrix and bias."""
        from .unet import _model_state_dict
        return _model_state_dict(self.engine, Engine.CLIP_VISION, "clipv.", self.state_dict_spec(), dtype, device)

    def save_pretrained(self, save_directory: str, safe_serialization: bool = True):
        """``config.json`` (a ``CLIPVisionConfig``) and ``preprocessor_config.json`` as ``config_from_dir`` reads them +
        ``model.safetensors`` (``safe_serialization=False``: ``pytorch_model.bin``), in the checkpoint's spelling."""
        from .unet import _save_checkpoint
        c = self.ccfg
        config = {"architectures": [type(self).__name__], "model_type": "clip_vision_model"}
        config.update(self.config)
        _save_checkpoint(save_directory, config, self.state_dict(device="cpu"), safe_serialization, SAFETENSORS_NAME, WEIGHTS_NAME)
        proc = {"image_processor_type": "CLIPImageProcessor", "do_resize": True, "do_center_crop": True, "do_rescale": True,
                "do_normalize": True, "do_convert_rgb": True, "size": {"shortest_edge": c.resize_edge},
                "crop_size": {"height": c.image_size, "width": c.image_size}, "resample": c.resample, "rescale_factor": c.rescale_factor,
                "image_mean": list(c.image_mean), "image_std": list(c.image_std)}
        self._write_processor(save_directory, proc)

    def init_synthetic(self, seed: int = 46, mode: str = "perturbed"):
        return self.load_state_dict(synth_state_dict(self.state_dict_spec(), seed=seed, mode=mode))

    @staticmethod
    def config_from_dir(path: str) -> ClipVisionConfig:
        """``config.json`` (``CLIPVisionConfig``, or ``CLIPConfig`` with its ``vision_config``) + ``preprocessor_config.json`` of a
        ``transformers`` CLIP directory -> ``ClipVisionConfig``.  Refuses what the kernels cannot do."""
        cj, pj = _TowerModel._read_configs(path)
        d = ClipVisionConfig()
        top = cj
        if "vision_config" in cj:                                # a full CLIPConfig: projection_dim sits at the top as well
            cj = dict(cj["vision_config"] or {})
            cj.setdefault("projection_dim", top.get("projection_dim", d.projection_dim))
        hidden, heads = cj.get("hidden_size", d.hidden), cj.get("num_attention_heads", d.heads)
        if hidden != 64 * heads:
            raise NotImplementedError(f"hidden_size={hidden} over {heads} heads is a head dim of {hidden / heads:g}: the attention kernel has 64 only")
        act = cj.get("hidden_act", d.hidden_act)
        if act not in TEXT_ACTS:
            raise NotImplementedError(f"hidden_act={act!r}: the vision tower implements {sorted(TEXT_ACTS)}")
        if cj.get("num_channels", 3) != 3:
            raise NotImplementedError("the vision tower takes 3-channel images")
        image_size, patch = cj.get("image_size", d.image_size), cj.get("patch_size", d.patch_size)
        tokens = (image_size // patch) ** 2 + 1
        if tokens > _MAX_TOKENS:
            raise NotImplementedError(f"{tokens} tokens an image: the attention kernel holds at most {_MAX_TOKENS}")
        resample = pj.get("resample", d.resample)
        if resample not in _RESAMPLES:
            raise NotImplementedError(f"resample={resample!r}: the preprocess implements Pillow's BILINEAR (2) and BICUBIC (3)")
        for flag in ("do_resize", "do_center_crop", "do_rescale", "do_normalize"):
            if not pj.get(flag, True):
                raise NotImplementedError(f"{flag}=false: the preprocess resizes, crops, rescales and normalises")
        size = pj.get("size", d.resize_edge)
        if isinstance(size, dict):
            if set(size) != {"shortest_edge"}:
                raise NotImplementedError(f"size={size!r}: the preprocess resizes the shortest edge ({{'shortest_edge': E}})")
            size = size["shortest_edge"]
        crop = pj.get("crop_size", image_size)
        if isinstance(crop, dict):
            if crop.get("height") != crop.get("width") or crop.get("height") is None:
                raise NotImplementedError(f"crop_size={crop!r}: the preprocess crops a square")
            crop = crop["height"]
        if crop != image_size:
            raise NotImplementedError(f"the processor crops {crop}, the model takes {image_size}: interpolate_pos_encoding is not implemented")
        if size < image_size:
            raise NotImplementedError(f"shortest_edge={size} below the crop of {image_size}: the crop would pad")
        return ClipVisionConfig(hidden=hidden, heads=heads, layers=cj.get("num_hidden_layers", d.layers),
                                intermediate=cj.get("intermediate_size", d.intermediate), image_size=image_size, patch_size=patch,
                                projection_dim=cj.get("projection_dim", d.projection_dim), hidden_act=act,
                                layer_norm_eps=cj.get("layer_norm_eps", d.layer_norm_eps), resize_edge=size, resample=resample,
                                rescale_factor=pj.get("rescale_factor", d.rescale_factor),
                                image_mean=tuple(pj.get("image_mean", d.image_mean)), image_std=tuple(pj.get("image_std", d.image_std)))

    @classmethod
    def from_pretrained(cls, pretrained_model_path: str, torch_dtype=None, *, engine: Optional[Engine] = None, device: int = 0,
                        compute_dtype=None, **kwargs):
        """LOCAL directory only.  ``torch_dtype`` and ``cache_dir`` are accepted for drop-in use: checkpoints of any float type are
        widened to fp32, and nothing is ever fetched.  ``compute_dtype``: ``set_compute_dtype`` on the built model (``None``: fp32)."""
        path = str(pretrained_model_path)
        cls._require_dir(path, "model", "openai/clip-vit-base-patch32")
        config = cls.config_from_dir(path)
        cls._require_weights(path)
        model = cls(config, engine=engine, device=device)
        if compute_dtype is not None:
            model.set_compute_dtype(compute_dtype)
        return model.load_state_dict(_load_checkpoint(path, SAFETENSORS_NAME, WEIGHTS_NAME), strict=False)

    # -- forward -----------------------------------------------------------------------------
    def embed(self, frames, channels_last: Optional[bool] = None) -> torch.Tensor:
        """``image_embeds`` ``[n*F, projection_dim]`` of every frame (``Engine.clip_embed``).  ``frames``: clips ``[n,3,F,H,W]`` /
        ``[n,F,H,W,3]``, one clip, or ONE image ``[H,W,3]`` as the reference's ``clip_score`` takes it.  ``channels_last=None``:
        decided by the shape -- a last axis of 3 is channels-last, as the reference stacks its frames."""
        if not isinstance(frames, torch.Tensor):
            import numpy as np
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if channels_last is None:
            channels_last = frames.shape[-1] == 3
        if frames.dim() == 3:
            frames = frames[None] if channels_last else frames[:, None]
        return self.engine.clip_embed(frames, channels_last=channels_last)

    def forward(self, frames, channels_last: Optional[bool] = None, return_dict: bool = True, **kwargs):
        embeds = self.embed(frames, channels_last)
        return CLIPVisionModelOutput(embeds) if return_dict else (embeds,)

    __call__ = forward
