"""``Engine``: one ``e2v_ctx`` (weights + workspace on one GPU) behind a small Python object.

torch is used for what the boundary needs and nothing else: device buffers (``torch.empty``),
the current HIP stream, and D2H copies.  Every computation is a call into ``libeeg2video_hip.so``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .weights import (TEXT_ACTS, ClipVisionConfig, GLMNetConfig, ImageConfig, SemanticConfig, Seq2SeqConfig, TextConfig, UNetConfig,
                      VAEConfig, VideoConfig)

_ERRORS = {
    _lib.E2V_EINVAL: ValueError,
    _lib.E2V_ESHAPE: ValueError,
    _lib.E2V_ENOWEIGHT: RuntimeError,
    _lib.E2V_EHIP: RuntimeError,
    _lib.E2V_ESTATE: RuntimeError,
}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class Engine:
    """Owns one ``e2v_ctx``.  ``unet_cfg`` / ``vae_cfg`` mirror the reference configs; ``text_cfg`` (``None``: no text encoder)
    the ``CLIPTextModel`` one, ``image_cfg`` (``None``: no image classifier) the ``ViTForImageClassification`` one, ``video_cfg``
    (``None``: no video classifier) the ``VideoMAEForVideoClassification`` one, ``clip_vision_cfg`` (``None``: no CLIP vision tower)
    the ``CLIPVisionModelWithProjection`` one, ``seq2seq_cfg`` (``None``: no Seq2Seq latent model) the reference's ``myTransformer``,
    ``glmnet_cfg`` (``None``: no GLMNet) its ``glfnet`` / ``glfnet_mlp`` pair."""

    UNET, VAE, SEMANTIC, TEXT, IMAGE, VIDEO, CLIP_VISION = 1, 2, 4, 8, 16, 32, 64
    SEQ2SEQ = 128
    GLM = 256

    def __init__(self, unet_cfg: UNetConfig = UNetConfig(), vae_cfg: VAEConfig = VAEConfig(), device: int = 0,
                 sem_cfg: SemanticConfig = SemanticConfig(), text_cfg: Optional[TextConfig] = None,
                 image_cfg: Optional[ImageConfig] = None, video_cfg: Optional[VideoConfig] = None,
                 clip_vision_cfg: Optional[ClipVisionConfig] = None, seq2seq_cfg: Optional[Seq2SeqConfig] = None,
                 glmnet_cfg: Optional[GLMNetConfig] = None):
        if not torch.cuda.is_available():
            raise RuntimeError("eeg2video_amd needs an AMD GPU (torch.cuda.is_available() is False); "
                               "there is no CPU path")
        self.lib = _lib.load()
        self.unet_cfg, self.vae_cfg, self.sem_cfg, self.text_cfg = unet_cfg, vae_cfg, sem_cfg, text_cfg
        self.image_cfg, self.video_cfg, self.clip_vision_cfg = image_cfg, video_cfg, clip_vision_cfg
        self.seq2seq_cfg = seq2seq_cfg
        self.glmnet_cfg = glmnet_cfg
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        torch.zeros(1, device=self.device)          # make sure torch has initialised the device's context
        cfg = _lib.E2VConfig()
        self.lib.e2v_default_config(C.byref(cfg))
        cfg.in_channels, cfg.out_channels = unet_cfg.in_channels, unet_cfg.out_channels
        cfg.block_out_channels = (C.c_int * 4)(*unet_cfg.block_out_channels)
        cfg.layers_per_block = unet_cfg.layers_per_block
        cfg.cross_attention_dim = unet_cfg.cross_attention_dim
        hd = unet_cfg.attention_head_dim                      # an int, or one head count per down block (unet.py:71,110-111)
        if isinstance(hd, int):
            cfg.attention_heads = hd
        else:
            if len(hd) != 4:
                raise ValueError("attention_head_dim as a tuple needs one entry per down block (4)")
            cfg.attention_heads = int(hd[0])
            cfg.attention_heads_per_block = (C.c_int * 4)(*[int(h) for h in hd])
        cfg.norm_num_groups, cfg.norm_eps = unet_cfg.norm_num_groups, unet_cfg.norm_eps
        cfg.flip_sin_to_cos, cfg.freq_shift = int(unet_cfg.flip_sin_to_cos), float(unet_cfg.freq_shift)
        cfg.vae_in_channels, cfg.vae_latent_channels = vae_cfg.in_channels, vae_cfg.latent_channels
        cfg.vae_block_out_channels = (C.c_int * 4)(*vae_cfg.block_out_channels)
        cfg.vae_layers_per_block = vae_cfg.layers_per_block
        cfg.vae_norm_num_groups, cfg.vae_norm_eps = vae_cfg.norm_num_groups, vae_cfg.norm_eps
        cfg.vae_scaling_factor = vae_cfg.scaling_factor
        cfg.sem_in_features, cfg.sem_hidden, cfg.sem_tokens = sem_cfg.in_features, sem_cfg.hidden, sem_cfg.tokens
        if text_cfg is not None:
            fill_text_config(cfg, text_cfg)
        if image_cfg is not None:
            fill_image_config(cfg, image_cfg)
        if video_cfg is not None:
            fill_video_config(cfg, video_cfg)
        self._cfg = cfg
        ctx = C.c_void_p()
        if glmnet_cfg is not None:                            # any optional part: structs of their own beside the e2v_config
            self._clipv_cfg = clip_vision_config(clip_vision_cfg) if clip_vision_cfg is not None else None
            self._s2s_cfg = seq2seq_config(seq2seq_cfg) if seq2seq_cfg is not None else None
            self._glm_cfg = glmnet_config(glmnet_cfg)
            st = self.lib.e2v_create_ex2(C.byref(cfg), C.byref(self._clipv_cfg) if self._clipv_cfg is not None else None,
                                         C.byref(self._s2s_cfg) if self._s2s_cfg is not None else None, C.byref(self._glm_cfg), device,
                                         C.byref(ctx))
        elif seq2seq_cfg is not None:
            self._clipv_cfg = clip_vision_config(clip_vision_cfg) if clip_vision_cfg is not None else None
            self._s2s_cfg = seq2seq_config(seq2seq_cfg)
            st = self.lib.e2v_create_ex(C.byref(cfg), C.byref(self._clipv_cfg) if self._clipv_cfg is not None else None,
                                        C.byref(self._s2s_cfg), device, C.byref(ctx))
        elif clip_vision_cfg is not None:                     # the tower's config is a struct of its own beside the e2v_config
            self._clipv_cfg = clip_vision_config(clip_vision_cfg)
            st = self.lib.e2v_create_clip_vision(C.byref(cfg), C.byref(self._clipv_cfg), device, C.byref(ctx))
        else:
            st = self.lib.e2v_create(C.byref(cfg), device, C.byref(ctx))
        if st != _lib.E2V_OK:
            raise _ERRORS.get(st, RuntimeError)(self.lib.e2v_last_error(None).decode())
        self.ctx = ctx
        self.ready = 0
        self.compute_dtype = "fp32"

    def __del__(self):
        ctx, self.ctx = getattr(self, "ctx", None), None
        if ctx:
            self.lib.e2v_destroy(ctx)

    # ------------------------------------------------------------------ helpers
    def _check(self, st: int) -> None:
        if st != _lib.E2V_OK:
            raise _ERRORS.get(st, RuntimeError)(self.lib.e2v_last_error(self.ctx).decode())

    def _dev(self, t: torch.Tensor, name: str) -> torch.Tensor:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"`{name}` has to be of type `torch.Tensor` but is {type(t)}")
        return t.to(device=self.device, dtype=torch.float32).contiguous()

    def expected_keys(self) -> Dict[str, Tuple[int, ...]]:
        out = {}
        shape = (C.c_int64 * 4)()
        nd = C.c_int()
        for i in range(self.lib.e2v_num_expected_keys(self.ctx)):
            k = self.lib.e2v_expected_key(self.ctx, i, shape, C.byref(nd)).decode()
            out[k] = tuple(int(shape[d]) for d in range(nd.value))
        return out

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd: Mapping[str, object], prefix: str = "") -> None:
        """Upload tensors keyed by the reference's state-dict names (``prefix='vae.'`` for the VAE)."""
        for k, v in sd.items():
            if isinstance(v, torch.Tensor):
                v = v.detach().cpu()
                if v.dtype not in (torch.float32, torch.float16):      # bf16 / fp64 checkpoints: widened (or narrowed) to fp32 here
                    v = v.float()
                v = v.numpy()
            a = np.ascontiguousarray(v)
            if a.dtype == np.float16:
                dt = _lib.E2V_F16
            else:
                a = np.ascontiguousarray(a, dtype=np.float32)
                dt = _lib.E2V_F32
            shape = (C.c_int64 * a.ndim)(*a.shape)
            self._check(self.lib.e2v_load_tensor(self.ctx, (prefix + k).encode(), a.ctypes.data_as(C.c_void_p), dt,
                                                 shape, a.ndim))

    def finalize(self, which: int) -> None:
        self._check(self.lib.e2v_finalize_weights(self.ctx, which))
        self.ready |= which

    _UPDATE_DTYPES = {torch.float32: _lib.E2V_F32, torch.float16: _lib.E2V_F16, torch.bfloat16: _lib.E2V_BF16}

    def update_state_dict(self, sd, prefix: str = "") -> None:
        """Overwrite tensors of a FINALIZED part in place (``e2v_update_tensor``): every form the engine holds of each tensor
        (fused / interleaved fp32 matrices, 16-bit copies, f32x3 planes, conv layouts already built) is rewritten on the current
        stream, with no device synchronisation and no reload -- what ``optimizer.step()`` looks like to the validation pipeline of
        ``train_finetune_videodiffusion.py:196-200,320-335``.  ``sd``: a mapping or an iterable of ``(name, tensor)``.  Tensors
        already on the engine's device in fp32 / fp16 / bf16 are read where they are (device pointer); anything else goes by host
        pointer in its own 16-bit type or as fp32 (fp64 is narrowed as ``load_state_dict`` does)."""
        stream = torch.cuda.current_stream(self.device)
        self._pending = [(ev, src) for ev, src in getattr(self, "_pending", []) if not ev.query()]
        host_sources = []
        for k, v in (sd.items() if isinstance(sd, Mapping) else sd):
            on_device = 0
            if isinstance(v, torch.Tensor):
                v = v.detach()
                if v.device == self.device and v.dtype in self._UPDATE_DTYPES:
                    v = v.contiguous()
                    v.record_stream(stream)              # the allocator must not hand the block out before the queued read
                    on_device = 1
                else:
                    v = v.cpu()
                    v = (v if v.dtype in self._UPDATE_DTYPES else v.float()).contiguous()
                    host_sources.append(v)
                dt, ptr, shape = self._UPDATE_DTYPES[v.dtype], v.data_ptr(), tuple(v.shape)
            else:
                a = np.ascontiguousarray(v)
                if a.dtype != np.float16:
                    a = np.ascontiguousarray(a, dtype=np.float32)
                host_sources.append(a)
                dt, ptr, shape = (_lib.E2V_F16 if a.dtype == np.float16 else _lib.E2V_F32), a.ctypes.data, a.shape
            if not shape or 0 in shape:
                raise ValueError(f"{prefix + k}: an empty or 0-dim tensor is no weight")
            cshape = (C.c_int64 * len(shape))(*shape)
            self._check(self.lib.e2v_update_tensor(self.ctx, (prefix + k).encode(), C.c_void_p(ptr), dt, on_device, cshape, len(shape),
                                                   stream.cuda_stream))
        if host_sources:                                 # host memory stays referenced until the stream has passed its copies
            ev = torch.cuda.Event()
            ev.record(stream)
            self._pending.append((ev, host_sources))

    def _key_shapes(self) -> Dict[str, Tuple[int, ...]]:
        if getattr(self, "_shapes", None) is None:
            self._shapes = self.expected_keys()
        return self._shapes

    def read_tensor(self, key: str, form: Optional[str] = None, dtype: torch.dtype = torch.float32,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One tensor of a FINALIZED part, read back in the torch layout of the reference state dict (``e2v_read_tensor``): the inverse
        of every re-layout finalize makes, on the current stream, with no synchronisation and no allocation inside the library.
        ``form``: which stored form is read, a name of ``_lib.FORM_BITS`` -- ``None`` / ``'fp32'``: the fp32 values; for the weight of
        a linear also ``'bf16'`` / ``'fp16'`` (that stored copy, widened exactly) and ``'x3'`` (the three planes summed: the fp32
        weight exactly).  ``dtype``: float32, bfloat16 or float16 (round to nearest even).  Returns a device tensor; ``out``: a
        contiguous tensor of that dtype and the key's shape to write instead -- any view of a device buffer, whatever its alignment,
        or a CPU tensor (then the call returns when the copy has landed; it waits for the current stream only)."""
        shapes = self._key_shapes()
        if key not in shapes:
            raise RuntimeError(f"unexpected state-dict key: {key}")
        shape = shapes[key]
        if dtype not in self._UPDATE_DTYPES:
            raise ValueError(f"read_tensor writes float32, bfloat16 or float16, not {dtype}")
        if form is not None and form not in _lib.FORM_BITS:
            raise ValueError(f"form {form!r}: one of {sorted(_lib.FORM_BITS)}")
        if out is None:
            out = torch.empty(shape, device=self.device, dtype=dtype)
        elif not isinstance(out, torch.Tensor) or out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous() \
                or out.device not in (self.device, torch.device("cpu")):
            raise ValueError(f"`out` has to be a contiguous {dtype} tensor of shape {shape} on {self.device} or on the host")
        stream = torch.cuda.current_stream(self.device)
        on_device = int(out.device == self.device)
        if on_device:
            out.record_stream(stream)
        cshape = (C.c_int64 * len(shape))(*shape)
        self._check(self.lib.e2v_read_tensor(self.ctx, key.encode(), _lib.FORM_BITS[form] if form else 0, C.c_void_p(out.data_ptr()),
                                             self._UPDATE_DTYPES[dtype], on_device, cshape, len(shape), stream.cuda_stream))
        return out

    _PART_PREFIX = {4: "semantic.", 2: "vae.", 8: "text.", 16: "image.", 32: "video.", 64: "clipv.", 128: "s2s.", 256: "glm."}

    def state_dict(self, part: int, prefix: str = "", dtype: torch.dtype = torch.float32, device="cuda"):
        """Every tensor of one finalized part (``Engine.UNET`` / ``VAE`` / ``SEMANTIC`` / ``TEXT`` / ``IMAGE`` / ``VIDEO`` / ``CLIP_VISION``) as the device holds it NOW -- after any
        ``update_state_dict`` --, an ``OrderedDict`` in ``expected_keys()`` order with ``prefix`` (the one ``load_state_dict`` adds:
        ``'vae.'``, ``'semantic.'``, ``'text.'``) stripped from the names.  ``device``: ``'cuda'`` (tensors on the engine's device) or
        ``'cpu'``."""
        from collections import OrderedDict
        dev = torch.device(device)
        if dev.type == "cuda":
            dev = self.device
        elif dev.type != "cpu":
            raise ValueError(f"state_dict(device={device!r}): 'cuda' or 'cpu'")
        own = self._PART_PREFIX.get(part, "")
        if part not in (self.UNET, self.VAE, self.SEMANTIC, self.TEXT, self.IMAGE, self.VIDEO, self.CLIP_VISION, self.SEQ2SEQ, self.GLM) or prefix not in ("", own):
            raise ValueError(f"state_dict(part={part!r}, prefix={prefix!r}): one part, and the prefix load_state_dict adds for it ({own!r})")
        foreign = tuple(self._PART_PREFIX.values())
        out = OrderedDict()
        for k, shape in self._key_shapes().items():
            if not (k.startswith(own) if own else not k.startswith(foreign)):
                continue
            t = torch.empty(shape, device=dev, dtype=dtype)
            out[k[len(prefix):]] = self.read_tensor(k, dtype=dtype, out=t)
        return out

    def weight_forms(self, key: str) -> int:
        """Test aid (``e2v_op_weight_forms``): bit mask of the forms of ``key`` that exist on the device (``_lib.FORM_BITS``)."""
        mask = C.c_int(0)
        self._check(self.lib.e2v_op_weight_forms(self.ctx, key.encode(), C.byref(mask)))
        return mask.value

    def set_compute_dtype(self, dtype) -> None:
        """'fp32' (default, parity configuration), 'bf16' (BASELINE configs[2]: bf16 MFMA, bf16 activations in HBM, fp32 accumulate /
        statistics / softmax) or 'fp16' (the same kernels on IEEE half: the reference's own inference dtype,
        ``inference_eeg2video.py:69-70`` ``torch_dtype=torch.float16``).  A ``torch.dtype`` is accepted too."""
        code = compute_dtype_code(dtype)
        self._check(self.lib.e2v_set_compute_dtype(self.ctx, code))
        self.compute_dtype = {_lib.E2V_F32: "fp32", _lib.E2V_F16: "fp16", _lib.E2V_BF16: "bf16", _lib.E2V_F32X3: "f32x3"}[code]

    _DTYPE_NAMES = {_lib.E2V_F32: "fp32", _lib.E2V_F16: "fp16", _lib.E2V_BF16: "bf16", _lib.E2V_F32X3: "f32x3"}

    def set_tower_dtype(self, part: int, dtype) -> None:
        """The arithmetic of ONE metric tower (``e2v_set_tower_dtype``): ``part`` is ``Engine.IMAGE``, ``VIDEO`` or ``CLIP_VISION``,
        ``dtype`` ``'fp32'`` (the default, bit for bit the fp32 path), ``'bf16'`` or ``'fp16'`` (the reference's own dtype for these
        models, ``40_class_run_metrics.py:41,89,125``) or the ``torch.dtype``.  Independent of ``set_compute_dtype``; the outputs stay
        fp32.  May be called at any time; the 16-bit copies of the tower's matrices are built on the first call in that mode."""
        self._check(self.lib.e2v_set_tower_dtype(self.ctx, int(part), compute_dtype_code(dtype)))

    def tower_dtype(self, part: int) -> str:
        """``'fp32'``, ``'bf16'`` or ``'fp16'``: what ``set_tower_dtype`` left ``part`` at (``e2v_tower_dtype``)."""
        code = self.lib.e2v_tower_dtype(self.ctx, int(part))
        if code not in self._DTYPE_NAMES:
            raise ValueError(f"tower_dtype(part={part!r}): Engine.IMAGE, Engine.VIDEO or Engine.CLIP_VISION")
        return self._DTYPE_NAMES[code]

    def set_conv_algo(self, algo: str) -> None:
        """'auto' (default: Winograd F(2x2,3x3) for the wide stride-1 3x3 convs, direct implicit GEMM elsewhere),
        'direct' or 'winograd'.  For the graph entry points call it before the weights are finalized."""
        code = {"auto": 0, "direct": 1, "winograd": 2, "winograd4": 3}[algo]
        self._check(self.lib.e2v_set_conv_algo(self.ctx, code))

    def set_knob(self, name: str, value: int) -> None:
        """Run-time switch of DESIGN section 10 (tests / profiling: same-process A/B of kernel variants)."""
        if self.lib.e2v_op_set_knob(name.encode(), int(value)) != 0:
            raise ValueError(f"unknown switch {name!r}")

    def device_bytes(self) -> int:
        return int(self.lib.e2v_device_bytes(self.ctx))

    def profile_begin(self) -> None:
        self._check(self.lib.e2v_profile_begin(self.ctx))

    def profile_end(self) -> dict:
        import json
        buf = C.create_string_buffer(1 << 20)
        n = self.lib.e2v_profile_end(self.ctx, buf, len(buf))
        if n < 0:
            raise RuntimeError("e2v_profile_end failed")
        return json.loads(buf.value.decode())

    # ------------------------------------------------------------------ schedule
    def ddim_timesteps(self, n: int) -> np.ndarray:
        out = np.empty(n, dtype=np.int64)
        self._check(self.lib.e2v_ddim_timesteps(self.ctx, n, out.ctypes.data_as(_lib.c_int64_p)))
        return out

    def alphas_cumprod(self) -> np.ndarray:
        out = np.empty(self._cfg.num_train_timesteps, dtype=np.float32)
        self._check(self.lib.e2v_ddim_alphas_cumprod(self.ctx, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def set_alphas_cumprod(self, table: np.ndarray) -> None:
        t = np.ascontiguousarray(table, dtype=np.float32)
        self._check(self.lib.e2v_set_alphas_cumprod(self.ctx, t.ctypes.data_as(C.POINTER(C.c_float)), t.size))

    def set_ddim_schedule(self, alphas_cumprod: np.ndarray, steps_offset: int) -> None:
        """Hand the ctx the schedule of the scheduler object the caller holds (table + ``steps_offset``), so that the
        fused loop and a stepped loop driven by that scheduler agree."""
        t = np.ascontiguousarray(alphas_cumprod, dtype=np.float32)
        self._check(self.lib.e2v_set_ddim_schedule(self.ctx, t.ctypes.data_as(C.POINTER(C.c_float)), t.size, int(steps_offset)))
        self._cfg.num_train_timesteps, self._cfg.steps_offset = int(t.size), int(steps_offset)

    def _check_loop_inputs(self, x: torch.Tensor, cond: torch.Tensor, un: Optional[torch.Tensor]) -> None:
        """Shapes the fused loops index device memory by: everything is checked here, on the host, because the library
        copies ``B*T*D`` floats from ``cond`` / ``uncond`` whatever their real size."""
        if x.dim() != 5 or cond.dim() != 3:
            raise ValueError(f"expected latents [B,C,F,h,w] and cond [B,T,D], got {tuple(x.shape)} / {tuple(cond.shape)}")
        b, c = x.shape[0], x.shape[1]
        if c != self.unet_cfg.in_channels:
            raise ValueError(f"latents have {c} channels, the UNet takes {self.unet_cfg.in_channels}")
        if cond.shape[0] != b:
            raise ValueError(f"cond batch {cond.shape[0]} != latent batch {b}")
        if cond.shape[2] != self.unet_cfg.cross_attention_dim:
            raise ValueError(f"cond feature dim {cond.shape[2]} != cross_attention_dim {self.unet_cfg.cross_attention_dim}")
        if un is not None:
            if un.dim() != 3 or un.shape[0] not in (1, b) or tuple(un.shape[1:]) != tuple(cond.shape[1:]):
                raise ValueError(f"uncond must be [1 or {b},{cond.shape[1]},{cond.shape[2]}], got {tuple(un.shape)}")

    # ------------------------------------------------------------------ hot path
    def unet_forward(self, sample: torch.Tensor, timesteps: Sequence[int], cond: torch.Tensor) -> torch.Tensor:
        sample, cond = self._dev(sample, "sample"), self._dev(cond, "encoder_hidden_states")
        if sample.dim() != 5 or cond.dim() != 3 or cond.shape[0] != sample.shape[0]:
            raise ValueError(f"expected sample [N,C,F,H,W] and cond [N,T,D], got {tuple(sample.shape)} / {tuple(cond.shape)}")
        n, c, f, h, w = sample.shape
        if c != self.unet_cfg.in_channels or cond.shape[2] != self.unet_cfg.cross_attention_dim:
            raise ValueError("channel count of `sample` or feature dim of `encoder_hidden_states` does not match the config")
        out = torch.empty((n, self.unet_cfg.out_channels, f, h, w), device=self.device, dtype=torch.float32)
        tarr = np.asarray(timesteps).reshape(-1)
        if np.issubdtype(tarr.dtype, np.floating) and not np.all(tarr == np.round(tarr)):
            tf = np.ascontiguousarray(tarr, dtype=np.float32)        # fractional timesteps (Euler / LMS schedules)
            self._check(self.lib.e2v_unet_forward_ft(self.ctx, sample.data_ptr(), tf.ctypes.data_as(C.POINTER(C.c_float)), tf.size,
                                                     cond.data_ptr(), n, f, h, w, cond.shape[1], out.data_ptr(), _stream()))
            return out
        ts = np.ascontiguousarray(tarr.astype(np.int64))
        self._check(self.lib.e2v_unet_forward(self.ctx, sample.data_ptr(), ts.ctypes.data_as(_lib.c_int64_p), ts.size,
                                              cond.data_ptr(), n, f, h, w, cond.shape[1], out.data_ptr(), _stream()))
        return out

    TAP_NAMES = ("emb", "down0", "down1", "down2", "down3", "mid", "up0", "up1", "up2", "up3")

    def unet_forward_taps(self, sample: torch.Tensor, timesteps: Sequence[int], cond: torch.Tensor):
        """Test aid (``e2v_op_unet_forward_taps``): the forward plus the block outputs ``oracle/unet3d.py`` exposes as ``taps``
        (fp32 NCFHW; ``emb`` as [N, 1280]).  Returns ``(sample_out, {name: tensor})``."""
        sample, cond = self._dev(sample, "sample"), self._dev(cond, "encoder_hidden_states")
        n, c, f, h, w = sample.shape
        out = torch.empty((n, self.unet_cfg.out_channels, f, h, w), device=self.device, dtype=torch.float32)
        boc = list(self.unet_cfg.block_out_channels)
        down = lambda v: (v - 1) // 2 + 1                              # 3x3, stride 2, padding 1
        hs, ws = [h], [w]
        for _ in range(3):
            hs.append(down(hs[-1])); ws.append(down(ws[-1]))
        lv = lambda ch, l: n * ch * f * hs[l] * ws[l]
        cap = (n * 4 * boc[0] + sum(lv(boc[i], min(i + 1, 3)) for i in range(4)) + lv(boc[3], 3)
               + sum(lv(boc[3 - i], max(3 - i - 1, 0)) for i in range(4)))
        buf = torch.empty(int(cap), device=self.device, dtype=torch.float32)
        shapes = np.zeros(80, dtype=np.int64)
        count = C.c_int(0)
        ts = np.ascontiguousarray(np.asarray(timesteps).reshape(-1).astype(np.int64))
        self._check(self.lib.e2v_op_unet_forward_taps(self.ctx, sample.data_ptr(), ts.ctypes.data_as(_lib.c_int64_p), ts.size,
                                                      cond.data_ptr(), n, f, h, w, cond.shape[1], out.data_ptr(), buf.data_ptr(),
                                                      buf.numel(), shapes.ctypes.data_as(_lib.c_int64_p), C.byref(count), _stream()))
        taps, off = {}, 0
        for i in range(count.value):
            shp = [int(v) for v in shapes[5 * i:5 * i + 5]]
            cnt = int(np.prod(shp))
            t = buf[off:off + cnt].reshape(shp)
            taps[self.TAP_NAMES[i]] = t.reshape(shp[0], shp[1]) if self.TAP_NAMES[i] == "emb" else t
            off += cnt
        return out, taps

    def ddim_cfg_step(self, eps_uncond: torch.Tensor, eps_cond: Optional[torch.Tensor], x: torch.Tensor,
                      guidance_scale: float, t: int, t_prev: int) -> torch.Tensor:
        eu, x = self._dev(eps_uncond, "eps"), self._dev(x, "sample")
        ec = self._dev(eps_cond, "eps_cond") if eps_cond is not None else None
        out = torch.empty_like(x)
        self._check(self.lib.e2v_ddim_cfg_step(self.ctx, eu.data_ptr(), ec.data_ptr() if ec is not None else None,
                                               x.data_ptr(), out.data_ptr(), x.numel(), float(guidance_scale), int(t),
                                               int(t_prev), _stream()))
        return out

    def cfg_combine(self, eps_uncond: torch.Tensor, eps_cond: torch.Tensor, guidance_scale: float) -> torch.Tensor:
        eu, ec = self._dev(eps_uncond, "eps_uncond"), self._dev(eps_cond, "eps_cond")
        out = torch.empty_like(eu)
        self._check(self.lib.e2v_cfg_combine(self.ctx, eu.data_ptr(), ec.data_ptr(), float(guidance_scale), out.data_ptr(),
                                             eu.numel(), _stream()))
        return out

    def lincomb(self, terms) -> torch.Tensor:
        """sum of coef * tensor over 1..5 (coef, tensor) pairs of equal shape."""
        xs = [self._dev(t, "term") for _, t in terms]
        n = len(xs)
        if not 1 <= n <= 5 or any(x.shape != xs[0].shape for x in xs):
            raise ValueError("lincomb takes 1..5 tensors of one shape")
        out = torch.empty_like(xs[0])
        ptrs = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
        coefs = (C.c_float * n)(*[float(c) for c, _ in terms])
        self._check(self.lib.e2v_lincomb(self.ctx, n, ptrs, coefs, out.data_ptr(), out.numel(), _stream()))
        return out

    def ddim_next_step(self, eps: torch.Tensor, t: int, x: torch.Tensor, num_inference_steps: int) -> torch.Tensor:
        e, x = self._dev(eps, "eps"), self._dev(x, "sample")
        out = torch.empty_like(x)
        self._check(self.lib.e2v_ddim_next_step(self.ctx, e.data_ptr(), x.data_ptr(), out.data_ptr(), x.numel(), int(t),
                                                int(num_inference_steps), _stream()))
        return out

    def ddim_invert(self, latents: torch.Tensor, cond: torch.Tensor, num_inv_steps: int, return_all: bool = True):
        """DDIM inversion loop on the device (reference: tuneavideo/util.py ddim_loop); returns the list of n+1 latents
        (return_all) or only the last one."""
        x, cond = self._dev(latents, "latents"), self._dev(cond, "cond")
        self._check_loop_inputs(x, cond, None)
        b, c, f, h, w = x.shape
        allb = torch.empty((num_inv_steps + 1,) + tuple(x.shape), device=self.device, dtype=torch.float32) if return_all else None
        last = torch.empty_like(x) if not return_all else None
        self._check(self.lib.e2v_ddim_invert(self.ctx, x.data_ptr(), cond.data_ptr(), b, f, h, w, cond.shape[1],
                                             int(num_inv_steps), allb.data_ptr() if return_all else None,
                                             last.data_ptr() if last is not None else None, _stream()))
        return list(allb.unbind(0)) if return_all else last

    def vae_decode(self, latents: torch.Tensor, postprocess: bool = True) -> torch.Tensor:
        z = self._dev(latents, "latents")
        if z.dim() == 4:
            z = z[:, :, None]
            squeeze = True
        else:
            squeeze = False
        b, c, f, h, w = z.shape
        out = torch.empty((b, self.vae_cfg.out_channels, f, 8 * h, 8 * w), device=self.device, dtype=torch.float32)
        self._check(self.lib.e2v_vae_decode(self.ctx, z.contiguous().data_ptr(), b, f, h, w, int(postprocess),
                                            out.data_ptr(), _stream()))
        return out[:, :, 0] if squeeze else out

    def vae_encode(self, images: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        x = self._dev(images, "images")
        n, c, h, w = x.shape
        lat = self.vae_cfg.latent_channels
        mean = torch.empty((n, lat, h // 8, w // 8), device=self.device, dtype=torch.float32)
        logvar = torch.empty_like(mean)
        self._check(self.lib.e2v_vae_encode(self.ctx, x.data_ptr(), n, h, w, mean.data_ptr(), logvar.data_ptr(), _stream()))
        return mean, logvar

    def generate(self, latents: torch.Tensor, cond: torch.Tensor, uncond: Optional[torch.Tensor],
                 num_inference_steps: int = 50, guidance_scale: float = 7.5, eta: float = 0.0, decode: bool = True,
                 return_latents: bool = False):
        x, cond = self._dev(latents, "latents"), self._dev(cond, "cond")
        un = self._dev(uncond, "uncond") if uncond is not None else None
        self._check_loop_inputs(x, cond, un)
        if guidance_scale > 1.0 and un is None:
            raise ValueError("classifier-free guidance (guidance_scale > 1) needs `uncond`")
        b, c, f, h, w = x.shape
        videos = torch.empty((b, self.vae_cfg.out_channels, f, 8 * h, 8 * w), device=self.device,
                             dtype=torch.float32) if decode else None
        lat_out = torch.empty_like(x) if return_latents else None
        self._check(self.lib.e2v_generate(
            self.ctx, x.data_ptr(), cond.data_ptr(), un.data_ptr() if un is not None else None,
            un.shape[0] if un is not None else 0, b, f, h, w, cond.shape[1], int(num_inference_steps),
            float(guidance_scale), float(eta), videos.data_ptr() if decode else None,
            lat_out.data_ptr() if return_latents else None, _stream()))
        return (videos, lat_out) if return_latents else videos

    def _plan_noise(self, plan, noise, shape) -> Optional[torch.Tensor]:
        """The ``[n_noise, *shape]`` fp32 device tensor a plan reads (a tensor or a sequence of ``n_noise`` tensors), checked here on
        the host because the library reads ``n_noise * prod(shape)`` floats whatever the real size."""
        if plan.n_noise == 0:
            if noise is not None and len(noise) != 0:
                raise ValueError("this plan reads no noise tensor")
            return None
        if noise is None:
            raise ValueError(f"this plan reads {plan.n_noise} noise tensors of shape {tuple(shape)}: pass `noise`")
        if not isinstance(noise, torch.Tensor):
            noise = torch.stack([self._dev(z, "noise") for z in noise])
        noise = self._dev(noise, "noise")
        if tuple(noise.shape) != (plan.n_noise,) + tuple(shape):
            raise ValueError(f"`noise` must be {(plan.n_noise,) + tuple(shape)}, got {tuple(noise.shape)}")
        return noise

    def generate_plan(self, latents: torch.Tensor, cond: torch.Tensor, uncond: Optional[torch.Tensor], plan,
                      guidance_scale: float = 7.5, noise=None, decode: bool = True, return_latents: bool = False):
        """``generate`` with the per-step update of a ``sampler_plan.SamplerPlan`` (``e2v_generate_plan``): the whole loop of any
        scheduler mirror on the device.  ``noise``: the ``[plan.n_noise, B, 4, F, h, w]`` N(0, 1) tensors of a stochastic plan, in
        step order.  Results are written only when every check has passed."""
        x, cond = self._dev(latents, "latents"), self._dev(cond, "cond")
        un = self._dev(uncond, "uncond") if uncond is not None else None
        self._check_loop_inputs(x, cond, un)
        if guidance_scale > 1.0 and un is None:
            raise ValueError("classifier-free guidance (guidance_scale > 1) needs `uncond`")
        z = self._plan_noise(plan, noise, x.shape)
        b, c, f, h, w = x.shape
        videos = torch.empty((b, self.vae_cfg.out_channels, f, 8 * h, 8 * w), device=self.device,
                             dtype=torch.float32) if decode else None
        lat_out = torch.empty_like(x) if return_latents else None
        ops = plan.c_ops()
        self._check(self.lib.e2v_generate_plan(
            self.ctx, x.data_ptr(), cond.data_ptr(), un.data_ptr() if un is not None else None,
            un.shape[0] if un is not None else 0, b, f, h, w, cond.shape[1], ops, len(ops), int(plan.n_slots), int(plan.final_slot),
            z.data_ptr() if z is not None else None, int(plan.n_noise), float(guidance_scale),
            videos.data_ptr() if decode else None, lat_out.data_ptr() if return_latents else None, _stream()))
        return (videos, lat_out) if return_latents else videos

    def run_plan_updates(self, plan, x0: torch.Tensor, eps_u, eps_c=None, guidance_scale: float = 1.0, noise=None,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Test aid (``e2v_op_run_plan``): the plan's updates with the UNet's results handed in -- ``eps_u`` (and, with guidance on,
        ``eps_c``) ``[plan.n_unet, *x0.shape]``, UNET op ``k`` taking entry ``k``.  Returns the final slot (``out=``: written there)."""
        x0 = self._dev(x0, "x0")                             # (a float32 tensor already on the device is used where it is)
        want = (plan.n_unet,) + tuple(x0.shape)

        def stacked(e, name):
            e = self._dev(e if isinstance(e, torch.Tensor) else torch.stack([self._dev(t, name) for t in e]), name)
            if tuple(e.shape) != want:
                raise ValueError(f"`{name}` must be {want}, got {tuple(e.shape)}")
            return e
        eu = stacked(eps_u, "eps_u")
        cfg = guidance_scale > 1.0
        if cfg and eps_c is None:
            raise ValueError("classifier-free guidance (guidance_scale > 1) needs `eps_c`")
        ec = stacked(eps_c, "eps_c") if cfg else None
        z = self._plan_noise(plan, noise, x0.shape)
        out = self._op_out(out, tuple(x0.shape))
        ops = plan.c_ops()
        self._check(self.lib.e2v_op_run_plan(self.ctx, ops, len(ops), int(plan.n_slots), int(plan.final_slot), x0.data_ptr(),
                                             eu.data_ptr(), ec.data_ptr() if ec is not None else None, int(plan.n_unet),
                                             z.data_ptr() if z is not None else None, int(plan.n_noise), float(guidance_scale),
                                             out.data_ptr(), x0.numel(), _stream()))
        return out

    # ------------------------------------------------------------------ the steps either side of the path
    def semantic_predict(self, eeg: torch.Tensor) -> torch.Tensor:
        x = self._dev(eeg, "eeg")
        if x.dim() != 2 or x.shape[1] != self.sem_cfg.in_features:
            raise ValueError(f"expected eeg [B,{self.sem_cfg.in_features}], got {tuple(x.shape)}")
        out = torch.empty((x.shape[0], self.sem_cfg.tokens * self.unet_cfg.cross_attention_dim), device=self.device,
                          dtype=torch.float32)
        self._check(self.lib.e2v_semantic_predict(self.ctx, x.data_ptr(), x.shape[0], out.data_ptr(), _stream()))
        return out

    def text_encode(self, input_ids, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``CLIPTextModel.forward(input_ids)[0]`` (``e2v_text_encode``): ``[B,T]`` token ids (a tensor on any device, an array or
        nested lists -- they travel as a HOST int64 array) -> the last hidden state ``[B,T,hidden]`` fp32 on the engine's device.
        fp32 arithmetic whatever the engine's compute dtype.  ``out``: a contiguous fp32 ``[B,T,hidden]`` tensor to write instead."""
        if self.text_cfg is None:
            raise RuntimeError("this engine was built without a text encoder (Engine(..., text_cfg=TextConfig()))")
        if isinstance(input_ids, torch.Tensor):
            input_ids = input_ids.detach().cpu().numpy()
        ids = np.ascontiguousarray(np.asarray(input_ids), dtype=np.int64)
        if ids.ndim == 1:
            ids = ids[None]
        if ids.ndim != 2 or ids.size == 0:
            raise ValueError(f"expected input_ids [B,T], got shape {ids.shape}")
        b, t = ids.shape
        out = self._op_out(out, (b, t, self.text_cfg.hidden))
        self._check(self.lib.e2v_text_encode(self.ctx, ids.ctypes.data_as(_lib.c_int64_p), b, t, out.data_ptr(), _stream()))
        return out

    def seq2seq_latents(self, eeg: torch.Tensor, *, strides: Optional[Tuple[int, int, int]] = None, batch: Optional[int] = None,
                        scaler: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, first: int = 0, count: Optional[int] = None,
                        layout: str = "bfchw", latents: bool = True, txt_logits: bool = False, tokens: bool = False,
                        out: Optional[Dict[str, torch.Tensor]] = None):
        """``myTransformer.forward`` in eval mode with the slice its inference keeps (``e2v_seq2seq_latents``).  ``eeg``: a contiguous fp32
        tensor on the engine's device, by default stacked windows ``[B, windows, electrodes, samples]``; with ``strides`` = (clip, window,
        channel) element strides and ``batch`` any buffer the strides describe -- a raw segment ``[B, electrodes, L]`` under sliding
        windows of step ``s`` is ``(electrodes * L, s, L)``.  ``scaler``: ``(mean, scale)`` ``[windows, electrodes, samples]`` applied as
        ``(x - mean) / scale``.  Tokens ``[first, first + count)`` of the ``steps + 1`` (``count=None``: ``steps - first``, i.e. the
        reference's ``[:, :-1]`` from ``first = 0``); ``layout`` ``'bfchw'`` ``[B,count,C,h,w]`` or ``'bcfhw'`` ``[B,C,count,h,w]``.
        Returns a dict with the outputs asked for: ``latents``, ``txt_logits`` ``[B,classes]``, ``tokens`` ``[B,steps+1,d_model]``
        (rows past ``first + count - 1`` are zeros).  ``out``: contiguous fp32 tensors of those shapes to write instead, by name (a
        ``tokens`` tensor given this way keeps its rows past ``first + count - 1``).  fp32 arithmetic whatever the compute dtype."""
        sc = self.seq2seq_cfg
        if sc is None:
            raise RuntimeError("this engine was built without a Seq2Seq latent model (Engine(..., seq2seq_cfg=Seq2SeqConfig()))")
        if layout not in ("bfchw", "bcfhw"):
            raise ValueError(f"layout {layout!r}: 'bfchw' or 'bcfhw'")
        if not isinstance(eeg, torch.Tensor) or eeg.device != self.device or eeg.dtype != torch.float32 or not eeg.is_contiguous():
            raise ValueError(f"`eeg` has to be a contiguous float32 tensor on {self.device}")
        if strides is None:
            if tuple(eeg.shape[1:]) != (sc.windows, sc.electrodes, sc.samples):
                raise ValueError(f"expected eeg [B,{sc.windows},{sc.electrodes},{sc.samples}], got {tuple(eeg.shape)}")
            b = eeg.shape[0]
            strides = (sc.windows * sc.electrodes * sc.samples, sc.electrodes * sc.samples, sc.samples)
        else:
            if batch is None:
                raise ValueError("`strides` needs `batch`")
            b = int(batch)
            cs, ws, es = (int(v) for v in strides)
            if min(cs, ws, es) < 0 or b < 1:
                raise ValueError("strides are non-negative element counts, batch at least 1")
            if (b - 1) * cs + (sc.windows - 1) * ws + (sc.electrodes - 1) * es + sc.samples > eeg.numel():
                raise ValueError("the strides reach past the end of `eeg`")
            strides = (cs, ws, es)
        mean_p = scale_p = None
        if scaler is not None:
            mean, scale = (self._dev(t, "scaler") for t in scaler)
            if tuple(mean.shape) != (sc.windows, sc.electrodes, sc.samples) or mean.shape != scale.shape:
                raise ValueError(f"the scaler is (mean, scale), each [{sc.windows},{sc.electrodes},{sc.samples}]")
            mean_p, scale_p = mean.data_ptr(), scale.data_ptr()
        if count is None:
            count = sc.steps - first
        given, out = out or {}, {}
        if latents:
            shape = (b, count) + tuple(sc.latent) if layout == "bfchw" else (b, sc.latent[0], count) + tuple(sc.latent[1:])
            shape = tuple(max(int(v), 0) for v in shape)
            out["latents"] = self._op_out(given["latents"], shape) if "latents" in given else torch.empty(shape, device=self.device, dtype=torch.float32)
        if txt_logits:
            out["txt_logits"] = self._op_out(given.get("txt_logits"), (b, sc.txt_classes))
        if tokens:
            shape = (b, sc.steps + 1, sc.d_model)
            out["tokens"] = self._op_out(given["tokens"], shape) if "tokens" in given else torch.zeros(shape, device=self.device, dtype=torch.float32)
        ptr = lambda k: out[k].data_ptr() if k in out else None
        self._check(self.lib.e2v_seq2seq_latents(self.ctx, eeg.data_ptr(), strides[0], strides[1], strides[2], mean_p, scale_p, b, int(first),
                                                 int(count), 0 if layout == "bfchw" else 1, ptr("latents"), ptr("txt_logits"), ptr("tokens"),
                                                 _stream()))
        return out

    def eeg_de_psd(self, eeg: torch.Tensor, *, samples: Optional[int] = None, strides: Optional[Tuple[int, int, int]] = None,
                   batch: Optional[int] = None, windows: Optional[int] = None, electrodes: Optional[int] = None, fs: int = 200,
                   scaler: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, de: bool = True, psd: bool = True,
                   out: Optional[Dict[str, torch.Tensor]] = None):
        """The reference's ``DE_PSD`` of every row (``e2v_eeg_de_psd``).  ``eeg``: a contiguous fp32 tensor on the engine's device, by
        default stacked windows ``[B, windows, electrodes, samples]``; with ``strides`` = (clip, window, electrode) element strides,
        ``batch``, ``windows``, ``electrodes`` and ``samples`` any buffer the strides describe -- the ``step``-spaced windows of a raw
        segment ``[B, electrodes, L]`` are ``(electrodes * L, step, L)``.  The transform length is 200 whatever ``samples`` is (longer
        rows are truncated after the Hann window, as the reference does).  ``scaler``: ``(mean, scale)``, ``electrodes * 5`` values each,
        applied to DE as ``(de - mean) / scale``.  Returns ``(de, psd)``, each ``[B, windows, electrodes, 5]`` or ``None`` where not asked
        for; ``out``: contiguous fp32 tensors of that shape to write instead, by name.  An all-zero row gives ``psd`` 0 and ``de``
        ``-inf``.  fp32 arithmetic whatever the compute dtype."""
        if not isinstance(eeg, torch.Tensor) or eeg.device != self.device or eeg.dtype != torch.float32 or not eeg.is_contiguous():
            raise ValueError(f"`eeg` has to be a contiguous float32 tensor on {self.device}")
        if strides is None:
            if eeg.dim() != 4 or min(eeg.shape) < 1:
                raise ValueError(f"expected eeg [B,windows,electrodes,samples], got {tuple(eeg.shape)}")
            b, w, c, m = (int(v) for v in eeg.shape)
            if any(given is not None and int(given) != have for given, have in ((batch, b), (windows, w), (electrodes, c), (samples, m))):
                raise ValueError("without `strides` the sizes are the shape of `eeg`")
            strides = (w * c * m, c * m, m)
        else:
            if None in (samples, batch, windows, electrodes):
                raise ValueError("`strides` needs `batch`, `windows`, `electrodes` and `samples`")
            b, w, c, m = int(batch), int(windows), int(electrodes), int(samples)
            cs, ws, es = (int(v) for v in strides)
            if min(cs, ws, es) < 0 or min(b, w, c, m) < 1:
                raise ValueError("strides are non-negative element counts, sizes at least 1")
            if (b - 1) * cs + (w - 1) * ws + (c - 1) * es + m > eeg.numel():
                raise ValueError("the strides reach past the end of `eeg`")
            strides = (cs, ws, es)
        mean_p = scale_p = None
        if scaler is not None:
            mean, scale = (self._dev(t, "scaler") for t in scaler)
            if mean.numel() != c * 5 or scale.numel() != c * 5:
                raise ValueError(f"the scaler is (mean, scale), each electrodes * 5 = {c * 5} values")
            mean_p, scale_p = mean.data_ptr(), scale.data_ptr()
        given = out or {}
        de_t = self._op_out(given.get("de"), (b, w, c, 5)) if de else None
        psd_t = self._op_out(given.get("psd"), (b, w, c, 5)) if psd else None
        self._check(self.lib.e2v_eeg_de_psd(self.ctx, eeg.data_ptr(), strides[0], strides[1], strides[2], b, w, c, m, int(fs), mean_p, scale_p,
                                            de_t.data_ptr() if de else None, psd_t.data_ptr() if psd else None, _stream()))
        return de_t, psd_t

    def _glm_outputs(self, b, width, logits, features, labels, out):
        given, res = out or {}, {}
        if logits:
            res["logits"] = self._op_out(given.get("logits"), (b, width))
        if features:
            res["features"] = self._op_out(given.get("features"), (b, 2 * self.glmnet_cfg.emb))
        if labels:
            lab = given.get("labels")
            if lab is None:
                lab = torch.empty(b, device=self.device, dtype=torch.int32)
            elif not isinstance(lab, torch.Tensor) or lab.device != self.device or lab.dtype != torch.int32 or tuple(lab.shape) != (b,) or not lab.is_contiguous():
                raise ValueError(f"`labels` has to be a contiguous int32 tensor [{b}] on {self.device}")
            res["labels"] = lab
        return res

    def glmnet_raw(self, eeg: torch.Tensor, *, strides: Optional[Tuple[int, int]] = None, batch: Optional[int] = None,
                   scaler: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, logits: bool = True, features: bool = False,
                   labels: bool = False, out: Optional[Dict[str, torch.Tensor]] = None):
        """``glfnet.forward`` in eval mode (``e2v_glmnet_raw``).  ``eeg``: a contiguous fp32 tensor on the engine's device, by default
        ``[B, electrodes, samples]`` (or the reference's ``[B, 1, electrodes, samples]``); with ``strides`` = (clip, electrode) element
        strides and ``batch`` any buffer the strides describe -- the first ``samples`` of raw segments ``[B, electrodes, L]`` are
        ``(electrodes * L, L)``.  ``scaler``: ``(mean, scale)`` ``[electrodes, samples]`` applied as ``(x - mean) / scale``.  Returns a
        dict with the outputs asked for: ``logits`` ``[B, raw_out]``, ``features`` ``[B, 2 emb]`` (the concatenated embeddings),
        ``labels`` ``[B]`` int32 (argmax, the lowest index among equal maxima).  ``out``: tensors of those shapes to write instead, by
        name.  fp32 arithmetic whatever the compute dtype."""
        gc = self.glmnet_cfg
        if gc is None:
            raise RuntimeError("this engine was built without a GLMNet (Engine(..., glmnet_cfg=GLMNetConfig()))")
        if gc.raw_out <= 0:
            raise RuntimeError("this engine's GLMNet config has no raw model (raw_out = 0)")
        if not isinstance(eeg, torch.Tensor) or eeg.device != self.device or eeg.dtype != torch.float32 or not eeg.is_contiguous():
            raise ValueError(f"`eeg` has to be a contiguous float32 tensor on {self.device}")
        if strides is None:
            if eeg.dim() == 4 and eeg.shape[1] == 1:
                eeg = eeg[:, 0]
            if eeg.dim() != 3 or tuple(eeg.shape[1:]) != (gc.electrodes, gc.samples) or eeg.shape[0] < 1:
                raise ValueError(f"expected eeg [B,{gc.electrodes},{gc.samples}] or [B,1,{gc.electrodes},{gc.samples}], got {tuple(eeg.shape)}")
            b = int(eeg.shape[0])
            strides = (gc.electrodes * gc.samples, gc.samples)
        else:
            if batch is None:
                raise ValueError("`strides` needs `batch`")
            b = int(batch)
            cs, es = (int(v) for v in strides)
            if min(cs, es) < 0 or b < 1:
                raise ValueError("strides are non-negative element counts, batch at least 1")
            if (b - 1) * cs + (gc.electrodes - 1) * es + gc.samples > eeg.numel():
                raise ValueError("the strides reach past the end of `eeg`")
            strides = (cs, es)
        mean_p = scale_p = None
        if scaler is not None:
            mean, scale = (self._dev(t, "scaler") for t in scaler)
            if tuple(mean.shape) != (gc.electrodes, gc.samples) or mean.shape != scale.shape:
                raise ValueError(f"the scaler is (mean, scale), each [{gc.electrodes},{gc.samples}]")
            mean_p, scale_p = mean.data_ptr(), scale.data_ptr()
        res = self._glm_outputs(b, gc.raw_out, logits, features, labels, out)
        ptr = lambda k: res[k].data_ptr() if k in res else None
        self._check(self.lib.e2v_glmnet_raw(self.ctx, eeg.data_ptr(), strides[0], strides[1], b, mean_p, scale_p, ptr("logits"), ptr("features"),
                                            ptr("labels"), _stream()))
        return res

    def glmnet_mlp(self, de: torch.Tensor, *, logits: bool = True, features: bool = False, labels: bool = False,
                   out: Optional[Dict[str, torch.Tensor]] = None):
        """``glfnet_mlp.forward`` (``e2v_glmnet_mlp``).  ``de``: a contiguous fp32 tensor ``[B, electrodes, bands]`` on the engine's
        device, for instance one window of ``eeg_de_psd``.  Outputs as ``glmnet_raw``, ``logits`` ``[B, mlp_out]``."""
        gc = self.glmnet_cfg
        if gc is None:
            raise RuntimeError("this engine was built without a GLMNet (Engine(..., glmnet_cfg=GLMNetConfig()))")
        if gc.mlp_out <= 0:
            raise RuntimeError("this engine's GLMNet config has no feature model (mlp_out = 0)")
        if not isinstance(de, torch.Tensor) or de.device != self.device or de.dtype != torch.float32 or not de.is_contiguous():
            raise ValueError(f"`de` has to be a contiguous float32 tensor on {self.device}")
        if de.dim() != 3 or tuple(de.shape[1:]) != (gc.electrodes, gc.bands) or de.shape[0] < 1:
            raise ValueError(f"expected de [B,{gc.electrodes},{gc.bands}], got {tuple(de.shape)}")
        b = int(de.shape[0])
        res = self._glm_outputs(b, gc.mlp_out, logits, features, labels, out)
        ptr = lambda k: res[k].data_ptr() if k in res else None
        self._check(self.lib.e2v_glmnet_mlp(self.ctx, de.data_ptr(), b, ptr("logits"), ptr("features"), ptr("labels"), _stream()))
        return res

    def dana_noise(self, x0: torch.Tensor, eps_div: torch.Tensor, eps_same: torch.Tensor, t: Sequence[int],
                   dynamic_beta: float, time_steps: int = 500) -> torch.Tensor:
        """``[B,F,C,H,W]`` Seq2Seq latents + the two noise draws -> noised latents in the pipeline layout ``[B,C,F,H,W]``."""
        x0, ed, es = self._dev(x0, "x_0"), self._dev(eps_div, "eps_div"), self._dev(eps_same, "eps_same")
        b, f, c, h, w = x0.shape
        if tuple(ed.shape) != (b, f, c, h, w) or tuple(es.shape) != (b, 1, c, h, w):
            raise ValueError("noise shapes do not match x_0")
        ts = np.ascontiguousarray(np.asarray(t, dtype=np.int64).reshape(-1))
        if ts.size != b:
            raise ValueError("one timestep per clip is required")
        out = torch.empty((b, c, f, h, w), device=self.device, dtype=torch.float32)
        self._check(self.lib.e2v_dana_noise(self.ctx, x0.data_ptr(), ed.data_ptr(), es.data_ptr(),
                                            ts.ctypes.data_as(_lib.c_int64_p), int(time_steps), float(dynamic_beta), b, f, c,
                                            h, w, out.data_ptr(), _stream()))
        return out

    def frames_to_uint8(self, videos: torch.Tensor) -> torch.Tensor:
        v = self._dev(videos, "videos")
        out = torch.empty(v.shape, device=self.device, dtype=torch.uint8)
        self._check(self.lib.e2v_frames_to_uint8(self.ctx, v.data_ptr(), out.data_ptr(), v.numel(), _stream()))
        return out

    def frame_metrics(self, a: torch.Tensor, b: torch.Tensor, a_channels_last: bool = False,
                      b_channels_last: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """Per-frame SSIM and MSE of two clips (``e2v_frame_metrics``; the reference's ``ssim_metric`` / ``mse_metric``,
        ``40_class_run_metrics.py:229-233``) -> ``(ssim, mse)``, fp32 ``[n,F]`` each on the engine's device.  ``a`` / ``b``: uint8, or
        float32 in ``[0,1]`` (quantised as ``frames_to_uint8`` does), planar ``[n,C,F,H,W]`` (``[C,F,H,W]``: one clip) or, with the
        input's ``*_channels_last`` flag, ``[n,F,H,W,C]`` (``[F,H,W,C]``); host tensors are copied over.  The two inputs choose type
        and layout independently; a non-contiguous view is made contiguous, a contiguous slice at any offset is read in place."""
        views = []
        for t, cl, name in ((a, a_channels_last, "a"), (b, b_channels_last, "b")):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"`{name}` has to be of type `torch.Tensor` but is {type(t)}")
            if t.dtype not in (torch.uint8, torch.float32):
                raise ValueError(f"`{name}` has to be uint8 or float32, not {t.dtype}")
            if t.dim() == 4:
                t = t[None]
            if t.dim() != 5:
                raise ValueError(f"`{name}`: expected a 4-D clip or a 5-D batch of clips, got shape {tuple(t.shape)}")
            t = t.to(self.device).contiguous()
            n, c, f, h, w = (t.shape[0], t.shape[4], t.shape[1], t.shape[2], t.shape[3]) if cl else tuple(t.shape)
            kind = (_lib.E2V_FRAMES_U8 if t.dtype == torch.uint8 else _lib.E2V_FRAMES_F32) | (_lib.E2V_FRAMES_CHANNELS_LAST if cl else 0)
            views.append((t, kind, (n, f, c, h, w)))
        (ta, ka, dims), (tb, kb, dims_b) = views
        if dims != dims_b:
            raise ValueError(f"clips differ: (n, F, C, H, W) = {dims} against {dims_b}")
        n, f, c, h, w = dims
        ssim = torch.empty((n, f), device=self.device, dtype=torch.float32)
        mse = torch.empty((n, f), device=self.device, dtype=torch.float32)
        self._check(self.lib.e2v_frame_metrics(self.ctx, ta.data_ptr(), ka, tb.data_ptr(), kb, n, f, c, h, w, ssim.data_ptr(),
                                               mse.data_ptr(), _stream()))
        return ssim, mse

    def _frames_arg(self, frames: torch.Tensor, channels_last: bool, name: str = "frames"):
        """A batch of RGB clips as the C ABI takes it: ``(tensor on the device, kind, (n, F, H, W))``"""
        t = frames
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"`{name}` has to be of type `torch.Tensor` but is {type(t)}")
        if t.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"`{name}` has to be uint8 or float32, not {t.dtype}")
        if t.dim() == 4:
            t = t[None]
        if t.dim() != 5 or t.shape[4 if channels_last else 1] != 3:
            raise ValueError(f"`{name}`: expected RGB clips [n,3,F,H,W] (channels_last: [n,F,H,W,3]) or one clip, got shape {tuple(frames.shape)}")
        t = t.to(self.device).contiguous()
        n, f, h, w = (t.shape[0], t.shape[1], t.shape[2], t.shape[3]) if channels_last else (t.shape[0], t.shape[2], t.shape[3], t.shape[4])
        kind = (_lib.E2V_FRAMES_U8 if t.dtype == torch.uint8 else _lib.E2V_FRAMES_F32) | (_lib.E2V_FRAMES_CHANNELS_LAST if channels_last else 0)
        return t, kind, (n, f, h, w)

    def classify_frames(self, frames: torch.Tensor, channels_last: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``ViTImageProcessor`` + ``ViTForImageClassification`` over every frame (``e2v_image_classify``; the classifier half of the
        reference's ``img_classify_metric``, ``40_class_run_metrics.py:86-98``) -> ``(logits, probs, top3)``: fp32 ``[n*F, labels]``
        twice and int32 ``[n*F, 3]``, the indices of the three largest logits in ascending order (``argsort(-1)[-3:]``), on the engine's
        device, frame ``f`` of clip ``i`` at row ``i*F + f``.  ``frames``: uint8, or float32 in ``[0,1]`` (quantised as
        ``frames_to_uint8`` does), planar ``[n,3,F,H,W]`` (``[3,F,H,W]``: one clip) or, with ``channels_last``, ``[n,F,H,W,3]``; host
        tensors are copied over.  The tower's own arithmetic (``set_tower_dtype``; fp32 by default) whatever the engine's compute dtype."""
        if self.image_cfg is None:
            raise RuntimeError("this engine was built without an image classifier (Engine(..., image_cfg=ImageConfig()))")
        t, kind, (n, f, h, w) = self._frames_arg(frames, channels_last)
        labels = self.image_cfg.num_labels
        logits = torch.empty((n * f, labels), device=self.device, dtype=torch.float32)
        probs = torch.empty((n * f, labels), device=self.device, dtype=torch.float32)
        top3 = torch.empty((n * f, 3), device=self.device, dtype=torch.int32)
        self._check(self.lib.e2v_image_classify(self.ctx, t.data_ptr(), kind, n, f, h, w, logits.data_ptr(), probs.data_ptr(),
                                                top3.data_ptr(), _stream()))
        return logits, probs, top3

    def classify_clips(self, frames: torch.Tensor, channels_last: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``VideoMAEImageProcessor`` + ``VideoMAEForVideoClassification`` over every clip (``e2v_video_classify``; the classifier half
        of the reference's ``video_classify_metric``, ``40_class_run_metrics.py:108-142``) -> ``(logits, probs, top3)``: fp32
        ``[n, labels]`` twice and int32 ``[n, 3]``, the indices of the three largest logits in ascending order, on the engine's device.
        ``frames``: as ``classify_frames`` takes them, with exactly ``video_cfg.num_frames`` frames per clip.  fp32 arithmetic whatever
        the engine's compute dtype."""
        if self.video_cfg is None:
            raise RuntimeError("this engine was built without a video classifier (Engine(..., video_cfg=VideoConfig()))")
        t, kind, (n, f, h, w) = self._frames_arg(frames, channels_last)
        labels = self.video_cfg.num_labels
        logits = torch.empty((n, labels), device=self.device, dtype=torch.float32)
        probs = torch.empty((n, labels), device=self.device, dtype=torch.float32)
        top3 = torch.empty((n, 3), device=self.device, dtype=torch.int32)
        self._check(self.lib.e2v_video_classify(self.ctx, t.data_ptr(), kind, n, f, h, w, logits.data_ptr(), probs.data_ptr(),
                                                top3.data_ptr(), _stream()))
        return logits, probs, top3

    def clip_embed(self, frames: torch.Tensor, channels_last: bool = False) -> torch.Tensor:
        """``CLIPImageProcessor`` + ``CLIPVisionModelWithProjection`` over every frame (``e2v_clip_embed``; the model half of the
        reference's ``clip_score``, ``40_class_run_metrics.py:20-55``) -> ``image_embeds`` fp32 ``[n*F, projection_dim]`` on the
        engine's device, NOT normalised, frame ``f`` of clip ``i`` at row ``i*F + f``.  ``frames``: as ``classify_frames`` takes them.
        The tower's own arithmetic (``set_tower_dtype``; fp32 by default) whatever the engine's compute dtype."""
        if self.clip_vision_cfg is None:
            raise RuntimeError("this engine was built without a CLIP vision tower (Engine(..., clip_vision_cfg=ClipVisionConfig()))")
        t, kind, (n, f, h, w) = self._frames_arg(frames, channels_last)
        out = torch.empty((n * f, self.clip_vision_cfg.projection_dim), device=self.device, dtype=torch.float32)
        self._check(self.lib.e2v_clip_embed(self.ctx, t.data_ptr(), kind, n, f, h, w, out.data_ptr(), _stream()))
        return out

    def clip_similarity(self, a: torch.Tensor, b: torch.Tensor, matrix: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``torch.nn.functional.cosine_similarity(a, b, dim=-1)`` (eps 1e-8) of fp32 rows on the device (``e2v_clip_similarity``):
        ``a`` ``[na, D]``, ``b`` ``[nb, D]`` -> ``[na]`` (pairs, ``na == nb``) or, with ``matrix``, ``[na, nb]`` over every pair of
        rows.  Element ``(i, j)`` of the matrix carries the bits of the pair form on ``(a[i], b[j])``.  Needs no vision tower."""
        a, b = self._dev(a, "a"), self._dev(b, "b")
        if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
            raise ValueError(f"clip_similarity: expected a [na, D] and b [nb, D], got {tuple(a.shape)} and {tuple(b.shape)}")
        shape = (a.shape[0], b.shape[0]) if matrix else (a.shape[0],)
        if out is None:
            out = torch.empty(shape, device=self.device, dtype=torch.float32)
        self._check(self.lib.e2v_clip_similarity(self.ctx, a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], a.shape[1], int(bool(matrix)),
                                                 out.data_ptr(), _stream()))
        return out

    # ------------------------------------------------------------------ the one exchange of the path
    def comm_init(self, group=None) -> int:
        """Open the library's own RCCL communicator over the ranks of the (already initialised) ``torch.distributed`` group:
        rank 0 draws the id, ``torch.distributed`` only ships its 128 bytes.  Returns the world size."""
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        # one communicator per GROUP: a different group of the same size must not reuse it (its ranks are other processes)
        key = tuple(dist.get_process_group_ranks(group if group is not None else dist.group.WORLD))
        if self.lib.e2v_comm_world(self.ctx) == world and getattr(self, "_comm_key", None) == key:
            return world
        if self.lib.e2v_comm_world(self.ctx) > 0:
            self.comm_destroy()
        buf = (C.c_ubyte * 128)()
        if rank == 0:
            if self.lib.e2v_comm_unique_id(buf) != _lib.E2V_OK:
                raise RuntimeError("e2v_comm_unique_id failed (is librccl.so loadable?)")
        ids = [bytes(buf)]
        dist.broadcast_object_list(ids, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        raw = (C.c_ubyte * 128).from_buffer_copy(ids[0])
        self._check(self.lib.e2v_comm_init(self.ctx, raw, rank, world))
        self._comm_key = key
        return world

    def comm_destroy(self) -> None:
        self._check(self.lib.e2v_comm_destroy(self.ctx))
        self._comm_key = None

    def allgather_frames(self, frames: torch.Tensor, as_uint8: bool = False) -> torch.Tensor:
        """``[b,3,F,H,W]`` fp32 frames of this rank -> ``[world*b,3,F,H,W]`` of all ranks (fp32 or uint8), one ``ncclAllGather``
        issued by the library on the current stream; every rank must hold the same ``b``."""
        world = self.lib.e2v_comm_world(self.ctx)
        if world <= 0:
            raise RuntimeError("allgather_frames: no communicator (Engine.comm_init first)")
        v = self._dev(frames, "frames")
        out = torch.empty((world * v.shape[0],) + tuple(v.shape[1:]), device=self.device, dtype=torch.uint8 if as_uint8 else torch.float32)
        self._check(self.lib.e2v_allgather_frames(self.ctx, v.data_ptr(), v.numel(), int(as_uint8), out.data_ptr(), _stream()))
        return out

    # ------------------------------------------------------------------ kernel-level ops (channel-last tensors)
    def _op_out(self, out, shape, strided=False):
        """The result tensor of an op wrapper: a fresh one, or the caller's ``out=`` used where it is (never copied).  ``strided``: the
        C ABI takes an output row stride, so a 2-D view with unit column stride will do; everywhere else ``out`` must be contiguous."""
        if out is None:
            return torch.empty(shape, device=self.device, dtype=torch.float32)
        if not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float32:
            raise ValueError("`out` has to be a float32 tensor on the engine's device")
        if tuple(out.shape) != tuple(shape):
            raise ValueError(f"`out` has shape {tuple(out.shape)}, the op writes {tuple(shape)}")
        if strided:
            if out.dim() != 2 or (out.shape[1] > 1 and out.stride(1) != 1) or out.stride(0) < out.shape[1]:
                raise ValueError("`out` has to be a 2-D view with unit column stride")
        elif not out.is_contiguous():
            raise ValueError("`out` has to be contiguous: this op takes no output row stride")
        return out

    def op_conv3x3(self, x0, w, bias=None, x1=None, *, n_img, Hs, Ws, Hi=None, Wi=None, stride=1, pad_lo=1, pad_hi=1,
                   rowbias=None, rows_per_sample=1, resid=None, out=None):
        Hi, Wi = Hi or Hs, Wi or Ws
        Ho = (Hi + pad_lo + pad_hi - 3) // stride + 1
        Wo = (Wi + pad_lo + pad_hi - 3) // stride + 1
        cout = w.shape[0]
        out = self._op_out(out, (n_img * Ho * Wo, cout))
        p = lambda t: t.data_ptr() if t is not None else None
        self._check(self.lib.e2v_op_conv3x3(self.ctx, x0.data_ptr(), x0.shape[1], p(x1), x1.shape[1] if x1 is not None else 0,
                                            n_img, Hs, Ws, Hi, Wi, Ho, Wo, stride, pad_lo, w.data_ptr(), p(bias), cout,
                                            p(rowbias), rows_per_sample, p(resid), out.data_ptr(), _stream()))
        return out

    def op_conv3x3_gn(self, x0, gamma, beta, w, bias=None, x1=None, *, n_img, Hs, Ws, gn_P, groups, eps, Hi=None, Wi=None, stride=1,
                      pad_lo=1, pad_hi=1, rowbias=None, rows_per_sample=1, resid=None, out=None):
        """GroupNorm + SiLU + 3x3 conv as the fp32 resnets run them (``e2v_op_conv3x3_gn``): statistics over slabs of ``gn_P`` source
        rows, affine + SiLU inside the Winograd input transform.  Raises ``ValueError`` where the conv takes no Winograd form."""
        Hi, Wi = Hi or Hs, Wi or Ws
        Ho = (Hi + pad_lo + pad_hi - 3) // stride + 1
        Wo = (Wi + pad_lo + pad_hi - 3) // stride + 1
        cout = w.shape[0]
        out = self._op_out(out, (n_img * Ho * Wo, cout))
        p = lambda t: t.data_ptr() if t is not None else None
        self._check(self.lib.e2v_op_conv3x3_gn(self.ctx, x0.data_ptr(), x0.shape[1], p(x1), x1.shape[1] if x1 is not None else 0,
                                               n_img, Hs, Ws, Hi, Wi, Ho, Wo, stride, pad_lo, gn_P, groups, float(eps),
                                               gamma.data_ptr(), beta.data_ptr(), w.data_ptr(), p(bias), cout, p(rowbias),
                                               rows_per_sample, p(resid), out.data_ptr(), _stream()))
        return out

    def op_linear(self, x, w, bias=None, resid=None, geglu=False, out=None, x1=None):
        """``x`` (and ``x1``): 2-D views with unit column stride, row stride = ``.stride(0)``.  ``x1``: second source, the K columns of
        a row are ``[x ; x1]`` (``e2v_op_linear_cat``)."""
        m, k = x.shape
        n = w.shape[0] // 2 if geglu else w.shape[0]
        out = self._op_out(out, (m, n))
        p = lambda t: t.data_ptr() if t is not None else None
        if x1 is None:
            self._check(self.lib.e2v_op_linear(self.ctx, x.data_ptr(), x.stride(0), m, k, w.data_ptr(), p(bias), n, p(resid),
                                               int(geglu), out.data_ptr(), _stream()))
        else:
            if x1.shape[0] != m or w.shape[1] != k + x1.shape[1]:
                raise ValueError(f"two-source linear: x {tuple(x.shape)}, x1 {tuple(x1.shape)}, w {tuple(w.shape)}")
            self._check(self.lib.e2v_op_linear_cat(self.ctx, x.data_ptr(), k, x.stride(0), x1.data_ptr(), x1.shape[1], x1.stride(0), m,
                                                   w.data_ptr(), p(bias), n, p(resid), int(geglu), out.data_ptr(), _stream()))
        return out

    def last_dispatch(self) -> str:
        """Test aid (``e2v_op_last_dispatch``, switch ``E2V_OP_RECORD``): the kernels that served this thread's latest op call."""
        buf = C.create_string_buffer(4096)
        self._check(self.lib.e2v_op_last_dispatch(buf, len(buf)))
        return buf.value.decode()

    def op_rowblock_sums(self, x, out=None):
        """Canonical (sum, sum of squares) per 64-row block and column of ``x`` rounded to bf16: ``[rows / 64, C, 2]``."""
        rows, c = x.shape
        out = self._op_out(out, (rows // 64, c, 2))
        self._check(self.lib.e2v_op_rowblock_sums(self.ctx, x.data_ptr(), rows, c, out.data_ptr(), _stream()))
        return out

    def op_groupnorm(self, x0, gamma, beta, *, samples, P, groups, eps, silu=False, x1=None, out=None):
        c = x0.shape[1] + (x1.shape[1] if x1 is not None else 0)
        out = self._op_out(out, (samples * P, c))
        self._check(self.lib.e2v_op_groupnorm(self.ctx, x0.data_ptr(), x0.shape[1], x1.data_ptr() if x1 is not None else None,
                                              x1.shape[1] if x1 is not None else 0, samples, P, groups, float(eps),
                                              gamma.data_ptr(), beta.data_ptr(), int(silu), out.data_ptr(), _stream()))
        return out

    def op_layernorm(self, x, gamma, beta, eps=1e-5, out=None):
        out = self._op_out(out, tuple(x.shape))
        self._check(self.lib.e2v_op_layernorm(self.ctx, x.data_ptr(), x.shape[0], x.shape[1], gamma.data_ptr(),
                                              beta.data_ptr(), float(eps), out.data_ptr(), _stream()))
        return out

    def op_attention(self, q, k, v, *, n, F, heads, D, Nq, Nk, mode, scale, out=None):
        """q/k/v: 2-D views (row stride = ``.stride(0)``) of channel-last buffers; returns [n*F*Nq, heads*D].  ``out``: a 2-D view
        whose ``.stride(0)`` is the output row stride ``ldo``."""
        out = self._op_out(out, (n * F * Nq, heads * D), strided=True)
        assert k.stride(0) == v.stride(0)
        self._check(self.lib.e2v_op_attention(self.ctx, q.data_ptr(), q.stride(0), k.data_ptr(), v.data_ptr(), k.stride(0),
                                              out.data_ptr(), out.stride(0), n, F, heads, D, Nq, Nk, mode, float(scale),
                                              _stream()))
        return out

    def op_temporal_attention(self, qkv, *, n, F, HW, heads, D, scale, out=None):
        out = self._op_out(out, (n * F * HW, heads * D))
        self._check(self.lib.e2v_op_temporal_attention(self.ctx, qkv.data_ptr(), out.data_ptr(), n, F, HW, heads, D,
                                                       float(scale), _stream()))
        return out

    def op_vae_attention_core(self, qkv, *, nimg, HW, C, out=None, scores=None, probs=None, intermediates=False):
        """``e2v_op_vae_attention_core``: the VAE mid-block attention between its qkv linear and its projection, the graph's own code.
        ``qkv``: contiguous ``[nimg*HW, 3C]``; returns ``[nimg*HW, C]``.  ``intermediates`` (or a ``scores=`` / ``probs=`` tensor
        ``[nimg*HW, HW]``): returns ``(out, scores, probs)`` -- the scaled fp32 scores and the probabilities as the kernels left them."""
        if (not isinstance(qkv, torch.Tensor) or qkv.device != self.device or qkv.dtype != torch.float32 or not qkv.is_contiguous()
                or tuple(qkv.shape) != (nimg * HW, 3 * C)):
            raise ValueError(f"`qkv` has to be a contiguous float32 tensor [{nimg * HW}, {3 * C}] on {self.device}")
        out = self._op_out(out, (nimg * HW, C))
        want = intermediates or scores is not None or probs is not None
        if want:
            scores, probs = self._op_out(scores, (nimg * HW, HW)), self._op_out(probs, (nimg * HW, HW))
        self._check(self.lib.e2v_op_vae_attention_core(self.ctx, qkv.data_ptr(), out.data_ptr(), nimg, HW, C,
                                                       scores.data_ptr() if want else None, probs.data_ptr() if want else None, _stream()))
        return (out, scores, probs) if want else out

    def _reach(self, t, name, itemsize):
        """elements of ``itemsize`` bytes from ``t``'s first element to the end of its storage (what a strided op may address)"""
        if not isinstance(t, torch.Tensor) or t.device != self.device or t.element_size() != itemsize:
            raise ValueError(f"`{name}` has to be a tensor of {itemsize}-byte elements on {self.device}")
        st = t.untyped_storage()
        return (st.nbytes() - (t.data_ptr() - st.data_ptr())) // itemsize

    def op_softmax_rows(self, x, *, out16=None):
        """``e2v_op_softmax_rows``, IN PLACE: ``x`` a 2-D float32 view ``[rows, cols]`` with unit column stride, row stride =
        ``.stride(0)``.  ``out16``: a bfloat16 / float16 view of the same shape and row stride that receives the rounded probabilities
        (``x`` then keeps the exponentials, not normalised).  Returns ``x``."""
        if x.dim() != 2 or x.dtype != torch.float32 or (x.shape[1] > 1 and x.stride(1) != 1) or x.stride(0) < x.shape[1]:
            raise ValueError("`x` has to be a 2-D float32 view with unit column stride")
        rows, cols = x.shape
        ld = x.stride(0)
        if (rows - 1) * ld + cols > self._reach(x, "x", 4):
            raise ValueError("`x` reaches past the end of its storage")
        mode = 0
        if out16 is not None:
            mode = {torch.bfloat16: 1, torch.float16: 2}.get(out16.dtype, 0)
            if (mode == 0 or tuple(out16.shape) != (rows, cols) or out16.stride(0) != ld or (cols > 1 and out16.stride(1) != 1)
                    or (rows - 1) * ld + cols > self._reach(out16, "out16", 2)):
                raise ValueError("`out16` has to be a bfloat16 / float16 view of x's shape and row stride")
        self._check(self.lib.e2v_op_softmax_rows(self.ctx, x.data_ptr(), ld, rows, cols, out16.data_ptr() if mode else None, mode, _stream()))
        return x

    def op_transpose2d(self, x, out, *, rows, cols, batch=1, ld_in=None, ld_out=None, sb_in=None, sb_out=None):
        """``e2v_op_transpose2d``: ``out[b][c][r] = x[b][r][c]`` for ``batch`` matrices of ``rows x cols`` read from ``x``'s first element
        on (row stride ``ld_in``, matrices ``sb_in`` elements apart) and written from ``out``'s first element on (``ld_out``, ``sb_out``).
        ``x`` and ``out`` share an element size of 2 or 4 bytes; the payload moves as bits.  Returns ``out``."""
        size = x.element_size()
        if size not in (2, 4):
            raise ValueError("the transpose moves 2- or 4-byte elements")
        ld_in, ld_out = ld_in or cols, ld_out or rows
        sb_in, sb_out = (rows * ld_in if sb_in is None else sb_in), (cols * ld_out if sb_out is None else sb_out)
        if min(rows, cols, batch) < 1 or ld_in < cols or ld_out < rows or min(sb_in, sb_out) < 0:
            raise ValueError("bad transpose sizes or strides")
        if (batch - 1) * sb_in + (rows - 1) * ld_in + cols > self._reach(x, "x", size):
            raise ValueError("the strides reach past the end of `x`")
        if (batch - 1) * sb_out + (cols - 1) * ld_out + rows > self._reach(out, "out", size):
            raise ValueError("the strides reach past the end of `out`")
        self._check(self.lib.e2v_op_transpose2d(self.ctx, x.data_ptr(), ld_in, out.data_ptr(), ld_out, rows, cols, batch, sb_in, sb_out,
                                                int(size == 2), _stream()))
        return out

    def op_causal_attention(self, qkv, *, B, T, heads, out=None):
        """``qkv``: a 2-D view ``[B*T, 3 * heads * 64]`` (row stride = ``.stride(0)``) holding q | k | v; returns ``[B*T, heads * 64]``
        (``e2v_op_causal_attention``: query i of a prompt attends to its keys 0 .. i).  ``out``: a 2-D view with its own row stride."""
        out = self._op_out(out, (B * T, heads * 64), strided=True)
        if tuple(qkv.shape) != (B * T, 3 * heads * 64) or qkv.stride(1) != 1:
            raise ValueError(f"`qkv` has shape {tuple(qkv.shape)}, expected {(B * T, 3 * heads * 64)} with unit column stride")
        self._check(self.lib.e2v_op_causal_attention(self.ctx, qkv.data_ptr(), qkv.stride(0), out.data_ptr(), out.stride(0), B, T,
                                                     heads, _stream()))
        return out

    def op_eegnet_embed(self, eeg, weights, *, B, W, C, T, F1, D, F2, strides=None, scaler=None, bn_eps=1e-5, out=None):
        """``e2v_op_eegnet_embed``: the EEGNet embedding kernel on its own.  ``eeg``: a contiguous fp32 device tensor read through
        ``strides`` = (clip, window, channel) element strides (``None``: stacked windows ``[B,W,C,T]``); ``weights``: the torch-layout
        tensors ``dict(w1 [F1,1,1,64], bn1, w2 [F1 D,1,C,1], bn2, w3 [F1 D,1,1,16], w4 [F2,F1 D,1,1], bn3)``, each ``bn*`` a
        ``[4, n]`` stack of weight, bias, running_mean, running_var; ``scaler``: ``(mean, scale)`` ``[W,C,T]``.
        Returns ``[B * W, F2 * ((T // 4) // 8)]``."""
        if not isinstance(eeg, torch.Tensor) or eeg.device != self.device or eeg.dtype != torch.float32 or not eeg.is_contiguous():
            raise ValueError(f"`eeg` has to be a contiguous float32 tensor on {self.device}")
        if strides is None:
            strides = (W * C * T, C * T, T)
        cs, ws, es = (int(v) for v in strides)
        if min(cs, ws, es) < 0 or (B - 1) * cs + (W - 1) * ws + (C - 1) * es + T > eeg.numel():
            raise ValueError("the strides are negative or reach past the end of `eeg`")
        fd = F1 * D
        want = {"w1": F1 * 64, "bn1": 4 * F1, "w2": fd * C, "bn2": 4 * fd, "w3": fd * 16, "w4": F2 * fd, "bn3": 4 * F2}
        w = {}
        for k, n in want.items():
            w[k] = self._dev(weights[k], k)
            if w[k].numel() != n:
                raise ValueError(f"weights[{k!r}] has {w[k].numel()} elements, expected {n}")
        mean_p = scale_p = None
        if scaler is not None:
            mean, scale = (self._dev(t, "scaler") for t in scaler)
            if mean.numel() != W * C * T or scale.numel() != W * C * T:
                raise ValueError("the scaler is (mean, scale), each [W,C,T]")
            mean_p, scale_p = mean.data_ptr(), scale.data_ptr()
        out = self._op_out(out, (B * W, F2 * ((T // 4) // 8)))
        self._check(self.lib.e2v_op_eegnet_embed(self.ctx, eeg.data_ptr(), cs, ws, es, mean_p, scale_p, B, W, C, T, F1, D, F2,
                                                 w["w1"].data_ptr(), w["bn1"].data_ptr(), w["w2"].data_ptr(), w["bn2"].data_ptr(),
                                                 w["w3"].data_ptr(), w["w4"].data_ptr(), w["bn3"].data_ptr(), float(bn_eps), out.data_ptr(),
                                                 _stream()))
        return out

    def op_shallownet(self, eeg, weights, *, B, C, T, F, K, P, S, strides=None, scaler=None, bn_eps=1e-5, out=None):
        """``e2v_op_shallownet``: the ShallowNet kernel on its own.  ``eeg``: a contiguous fp32 device tensor read through ``strides`` =
        (clip, electrode) element strides (``None``: ``[B,C,T]``); ``weights``: the torch-layout tensors ``dict(w1 [F,1,1,K], b1 [F],
        w2 [F,F,C,1], b2 [F], bn [4,F])``, ``bn`` the stack of weight, bias, running_mean, running_var; ``scaler``: ``(mean, scale)``
        ``[C,T]``.  Returns the pooled maps ``[B, F * columns]``, filter-major."""
        if not isinstance(eeg, torch.Tensor) or eeg.device != self.device or eeg.dtype != torch.float32 or not eeg.is_contiguous():
            raise ValueError(f"`eeg` has to be a contiguous float32 tensor on {self.device}")
        if strides is None:
            strides = (C * T, T)
        cs, es = (int(v) for v in strides)
        if min(cs, es) < 0 or (B - 1) * cs + (C - 1) * es + T > eeg.numel():
            raise ValueError("the strides are negative or reach past the end of `eeg`")
        want = {"w1": F * K, "b1": F, "w2": F * F * C, "b2": F, "bn": 4 * F}
        w = {}
        for k, n in want.items():
            w[k] = self._dev(weights[k], k)
            if w[k].numel() != n:
                raise ValueError(f"weights[{k!r}] has {w[k].numel()} elements, expected {n}")
        mean_p = scale_p = None
        if scaler is not None:
            mean, scale = (self._dev(t, "scaler") for t in scaler)
            if mean.numel() != C * T or scale.numel() != C * T:
                raise ValueError("the scaler is (mean, scale), each [C,T]")
            mean_p, scale_p = mean.data_ptr(), scale.data_ptr()
        tc = T - K + 1
        cols = (tc - P) // S + 1 if tc >= P else 0
        out = self._op_out(out, (B, F * cols))
        self._check(self.lib.e2v_op_shallownet(self.ctx, eeg.data_ptr(), cs, es, mean_p, scale_p, B, C, T, F, K, P, S, w["w1"].data_ptr(),
                                               w["b1"].data_ptr(), w["w2"].data_ptr(), w["b2"].data_ptr(), w["bn"].data_ptr(), float(bn_eps),
                                               out.data_ptr(), _stream()))
        return out

    def op_seq_attention(self, q, k, v, *, B, heads, D, Nq, Nk, q_pos0=0, causal=False, out=None):
        """``e2v_op_seq_attention``: ``q`` a 2-D view ``[B*Nq, heads*D]``, ``k``, ``v`` 2-D views ``[B*Nk, heads*D]`` of one row stride
        (``.stride(0)``; unit column stride) -> ``[B*Nq, heads*D]``; ``causal``: query i sits at position ``q_pos0 + i``.
        ``out``: a 2-D view with its own row stride."""
        out = self._op_out(out, (B * Nq, heads * D), strided=True)
        for name, t, rows in (("q", q, B * Nq), ("k", k, B * Nk), ("v", v, B * Nk)):
            if tuple(t.shape) != (rows, heads * D) or t.stride(1) != 1 or t.dtype != torch.float32 or t.device != self.device:
                raise ValueError(f"`{name}` has to be a float32 view [{rows}, {heads * D}] with unit column stride on {self.device}")
        if k.stride(0) != v.stride(0):
            raise ValueError("`k` and `v` share one row stride")
        self._check(self.lib.e2v_op_seq_attention(self.ctx, q.data_ptr(), q.stride(0), k.data_ptr(), v.data_ptr(), k.stride(0), out.data_ptr(),
                                                  out.stride(0), B, heads, D, Nq, Nk, int(q_pos0), int(bool(causal)), _stream()))
        return out

    def op_image_preprocess(self, frames, *, size, patch, lut=None, channels_last=False, out=None):
        """``e2v_op_image_preprocess``: clips -> the patch rows ``[n*F*(size/patch)^2, 3*patch^2]`` of the classifier's preprocess.
        ``lut``: ``[3,256]`` fp32 pixel values of a byte per channel (``None``: the engine's image config)."""
        t, kind, (n, f, h, w) = self._frames_arg(frames, channels_last)
        lut_p = None
        if lut is not None:
            lut = np.ascontiguousarray(np.asarray(lut, dtype=np.float32).reshape(3, 256))
            lut_p = lut.ctypes.data_as(C.POINTER(C.c_float))
        out = self._op_out(out, (n * f * (size // patch) ** 2, 3 * patch * patch))
        self._check(self.lib.e2v_op_image_preprocess(self.ctx, t.data_ptr(), kind, n, f, h, w, size, patch, lut_p, out.data_ptr(), _stream()))
        return out

    def op_image_attention(self, qkv, *, B, T, heads, out=None):
        """``e2v_op_image_attention``: ``qkv`` ``[B*T, 3*64*heads]`` -> ``[B*T, 64*heads]``, non-causal, fp32 in every mode."""
        qkv = self._dev(qkv, "qkv")
        if qkv.dim() != 2 or qkv.shape[0] != B * T or qkv.shape[1] != 3 * 64 * heads:
            raise ValueError(f"expected qkv [B*T, 3*64*heads] = [{B * T}, {3 * 64 * heads}], got {tuple(qkv.shape)}")
        out = self._op_out(out, (B * T, 64 * heads), strided=True)
        self._check(self.lib.e2v_op_image_attention(self.ctx, qkv.data_ptr(), qkv.stride(0), out.data_ptr(), out.stride(0), B, T, heads,
                                                    _stream()))
        return out

    def op_video_preprocess(self, frames, *, size, patch, tubelet, edge, lut=None, channels_last=False, out=None):
        """``e2v_op_video_preprocess``: clips -> the tubelet patch rows ``[n*(F/tubelet)*(size/patch)^2, 3*tubelet*patch^2]`` of the video
        classifier's preprocess (shortest edge resized to ``edge``, centre crop of ``size``).  ``lut``: ``[3,256]`` fp32 pixel values
        of a byte per channel (``None``: the engine's video config)."""
        t, kind, (n, f, h, w) = self._frames_arg(frames, channels_last)
        lut_p = None
        if lut is not None:
            lut = np.ascontiguousarray(np.asarray(lut, dtype=np.float32).reshape(3, 256))
            lut_p = lut.ctypes.data_as(C.POINTER(C.c_float))
        out = self._op_out(out, (n * (f // max(tubelet, 1)) * (size // patch) ** 2, 3 * tubelet * patch * patch))
        self._check(self.lib.e2v_op_video_preprocess(self.ctx, t.data_ptr(), kind, n, f, h, w, size, patch, tubelet, edge, lut_p,
                                                     out.data_ptr(), _stream()))
        return out

    def op_clip_preprocess(self, frames, *, size, patch, edge, filter=3, lut=None, channels_last=False, out=None):
        """``e2v_op_clip_preprocess``: frames -> the patch rows ``[n*F*(size/patch)^2, 3*patch^2]`` of the CLIP processor (shortest edge
        resized to ``edge`` with Pillow's ``filter`` -- 2 BILINEAR, 3 BICUBIC --, centre crop of ``size``).  ``lut``: ``[3,256]`` fp32
        pixel values of a byte per channel (``None``: the engine's CLIP vision config)."""
        t, kind, (n, f, h, w) = self._frames_arg(frames, channels_last)
        lut_p = None
        if lut is not None:
            lut = np.ascontiguousarray(np.asarray(lut, dtype=np.float32).reshape(3, 256))
            lut_p = lut.ctypes.data_as(C.POINTER(C.c_float))
        out = self._op_out(out, (n * f * (size // patch) ** 2, 3 * patch * patch))
        self._check(self.lib.e2v_op_clip_preprocess(self.ctx, t.data_ptr(), kind, n, f, h, w, size, patch, edge, filter, lut_p,
                                                    out.data_ptr(), _stream()))
        return out

    def op_token_attention(self, qkv, *, B, T, heads, out=None):
        """``e2v_op_token_attention``: ``qkv`` ``[B*T, 3*64*heads]`` (a 2-D view with unit column stride is read where it is) ->
        ``[B*T, 64*heads]``, non-causal, any ``T``, fp32 in every mode."""
        if not (isinstance(qkv, torch.Tensor) and qkv.device == self.device and qkv.dtype == torch.float32 and qkv.dim() == 2
                and qkv.stride(1) == 1):
            qkv = self._dev(qkv, "qkv")
        if qkv.dim() != 2 or qkv.shape[0] != B * T or qkv.shape[1] != 3 * 64 * heads:
            raise ValueError(f"expected qkv [B*T, 3*64*heads] = [{B * T}, {3 * 64 * heads}], got {tuple(qkv.shape)}")
        out = self._op_out(out, (B * T, 64 * heads), strided=True)
        self._check(self.lib.e2v_op_token_attention(self.ctx, qkv.data_ptr(), qkv.stride(0), out.data_ptr(), out.stride(0), B, T, heads,
                                                    _stream()))
        return out

    # ---- the pieces of a metric tower in a 16-bit mode (fp32 at the boundary: inputs rounded once, 16-bit results widened exactly)
    def op_tower_preprocess(self, frames, *, tower, dtype, size, patch, lut, tubelet=1, edge=0, filter=3, channels_last=False, out=None):
        """``e2v_op_tower_preprocess``: the preprocess of tower ``Engine.IMAGE`` / ``VIDEO`` / ``CLIP_VISION`` storing ``dtype`` patch
        rows (returned widened): ``op_image_preprocess`` / ``op_video_preprocess`` / ``op_clip_preprocess`` rounded once."""
        t, kind, (n, f, h, w) = self._frames_arg(frames, channels_last)
        lut = np.ascontiguousarray(np.asarray(lut, dtype=np.float32).reshape(3, 256))
        ts = tubelet if tower == self.VIDEO else 1
        out = self._op_out(out, (n * (f // max(ts, 1)) * (size // patch) ** 2, 3 * ts * patch * patch))
        self._check(self.lib.e2v_op_tower_preprocess(self.ctx, int(tower), compute_dtype_code(dtype), t.data_ptr(), kind, n, f, h, w, size,
                                                     patch, tubelet, edge, filter, lut.ctypes.data_as(C.POINTER(C.c_float)), out.data_ptr(),
                                                     _stream()))
        return out

    def op_tower_attention(self, qkv, *, dtype, B, T, heads, out=None):
        """``e2v_op_tower_attention``: ``qkv`` ``[B*T, 3*64*heads]`` rounded to ``dtype`` -> ``[B*T, 64*heads]``, the attention of a
        16-bit tower (non-causal, any ``T``; fp32 scores and softmax, 16-bit probabilities and output, widened)."""
        if not (isinstance(qkv, torch.Tensor) and qkv.device == self.device and qkv.dtype == torch.float32 and qkv.dim() == 2
                and qkv.stride(1) == 1):
            qkv = self._dev(qkv, "qkv")
        if qkv.dim() != 2 or qkv.shape[0] != B * T or qkv.shape[1] != 3 * 64 * heads:
            raise ValueError(f"expected qkv [B*T, 3*64*heads] = [{B * T}, {3 * 64 * heads}], got {tuple(qkv.shape)}")
        out = self._op_out(out, (B * T, 64 * heads), strided=True)
        self._check(self.lib.e2v_op_tower_attention(self.ctx, compute_dtype_code(dtype), qkv.data_ptr(), qkv.stride(0), out.data_ptr(),
                                                    out.stride(0), B, T, heads, _stream()))
        return out

    def op_tower_token_mean(self, x, *, dtype, B, T, out=None):
        """``e2v_op_tower_token_mean``: ``x`` ``[B*T, C]`` rounded to ``dtype`` -> the fp32 mean over each clip's ``T`` rows ``[B, C]``."""
        x = self._dev(x, "x")
        out = self._op_out(out, (B, x.shape[1]))
        self._check(self.lib.e2v_op_tower_token_mean(self.ctx, compute_dtype_code(dtype), x.data_ptr(), B, T, x.shape[1], out.data_ptr(), _stream()))
        return out

    def op_tower_layernorm(self, x, gamma, beta, *, dtype, rows, stride=1, eps=1e-5, out=None):
        """``e2v_op_tower_layernorm``: rows ``0, stride, 2 stride, ...`` (``rows`` of them) of ``x`` ``[>= (rows-1)*stride+1, C]`` rounded
        to ``dtype``, normalised into fp32 ``[rows, C]`` (not rounded): the LayerNorm in front of a 16-bit tower's head."""
        x, gamma, beta = self._dev(x, "x"), self._dev(gamma, "gamma"), self._dev(beta, "beta")
        if x.dim() != 2 or x.shape[0] < (rows - 1) * stride + 1:
            raise ValueError(f"`x` has shape {tuple(x.shape)}: at least {(rows - 1) * stride + 1} rows are read")
        out = self._op_out(out, (rows, x.shape[1]))
        self._check(self.lib.e2v_op_tower_layernorm(self.ctx, compute_dtype_code(dtype), x.data_ptr(), rows, stride, x.shape[1],
                                                    gamma.data_ptr(), beta.data_ptr(), float(eps), out.data_ptr(), _stream()))
        return out

    def op_tower_activation(self, x, *, dtype, act, out=None):
        """``e2v_op_tower_activation``: ``act`` 0 quick-GELU / 1 erf GELU in fp32 on ``x`` rounded to ``dtype``, the result rounded once
        (returned widened).  ``x.numel()`` a multiple of 8."""
        x = self._dev(x, "x")
        out = self._op_out(out, tuple(x.shape))
        self._check(self.lib.e2v_op_tower_activation(self.ctx, compute_dtype_code(dtype), x.data_ptr(), x.numel(), int(act), out.data_ptr(), _stream()))
        return out

    def op_tower_embed(self, patches, pos, *, dtype, nimg, cls=None, out=None):
        """``e2v_op_tower_embed``: the token rows of a 16-bit tower from ``patches`` rounded to ``dtype`` -- with a class row ``cls``
        ``[C]`` in front (ViT, CLIP: ``patches`` ``[nimg*(T-1), C]``) or without (VideoMAE: ``[nimg*T, C]``) -- plus ``pos`` ``[T, C]``
        in fp32, rounded once (returned widened)."""
        patches, pos = self._dev(patches, "patches"), self._dev(pos, "pos")
        cls = self._dev(cls, "cls") if cls is not None else None
        T, Cw = pos.shape
        out = self._op_out(out, (nimg * T, Cw))
        self._check(self.lib.e2v_op_tower_embed(self.ctx, compute_dtype_code(dtype), patches.data_ptr(), cls.data_ptr() if cls is not None else None,
                                                pos.data_ptr(), nimg, T, Cw, out.data_ptr(), _stream()))
        return out

    def op_to_channels_last(self, x, *, Cpad=None, out=None):
        """``[n, C, FHW]`` -> channel-last rows ``[n * FHW, Cpad]`` (``e2v_op_to_channels_last``; columns C.. are written as zeros)."""
        n, c, fhw = x.shape
        cpad = Cpad or c
        out = self._op_out(out, (n * fhw, cpad))
        self._check(self.lib.e2v_op_to_channels_last(self.ctx, x.data_ptr(), out.data_ptr(), n, c, cpad, fhw, _stream()))
        return out

    def op_from_channels_last(self, x, *, n, C, out=None):
        """Channel-last rows ``[n * FHW, >= C]`` (a 2-D view, row stride = ``.stride(0)``) -> ``[n, C, FHW]``
        (``e2v_op_from_channels_last``)."""
        fhw = x.shape[0] // n
        out = self._op_out(out, (n, C, fhw))
        self._check(self.lib.e2v_op_from_channels_last(self.ctx, x.data_ptr(), x.stride(0), out.data_ptr(), n, C, fhw, _stream()))
        return out

    def pool_guard_report(self):
        """Test aid (``e2v_op_pool_guard_report``, switch ``E2V_POOL_GUARD``): ``(blocks_checked, violations, text)`` since the previous
        report, one line of ``text`` per violated guard zone."""
        checked, bad = C.c_int64(0), C.c_int64(0)
        buf = C.create_string_buffer(1 << 16)
        self._check(self.lib.e2v_op_pool_guard_report(self.ctx, C.byref(checked), C.byref(bad), buf, len(buf)))
        return checked.value, bad.value, buf.value.decode()

    def pool_gets(self) -> int:
        """Test aid (``e2v_op_pool_gets``): blocks the workspace pool has handed out so far."""
        return int(self.lib.e2v_op_pool_gets(self.ctx))

    def pool_guard_selftest(self, payload_bytes: int, offset: int) -> None:
        """Test aid (``e2v_op_pool_guard_selftest``): take one guarded block, alter the word ``offset`` bytes into its trailing guard
        zone from the host, release it -- the next report must name it."""
        self._check(self.lib.e2v_op_pool_guard_selftest(self.ctx, int(payload_bytes), int(offset), _stream()))


def fill_text_config(cfg: "_lib.E2VConfig", text_cfg: TextConfig) -> None:
    """The ``text_*`` fields of an ``e2v_config`` from a ``TextConfig``."""
    if text_cfg.hidden_act not in TEXT_ACTS:
        raise NotImplementedError(f"hidden_act={text_cfg.hidden_act!r}: the text encoder implements {sorted(TEXT_ACTS)}")
    cfg.text_vocab_size, cfg.text_hidden, cfg.text_heads = text_cfg.vocab_size, text_cfg.hidden, text_cfg.heads
    cfg.text_layers, cfg.text_intermediate, cfg.text_max_positions = text_cfg.layers, text_cfg.intermediate, text_cfg.max_positions
    cfg.text_act, cfg.text_norm_eps = TEXT_ACTS[text_cfg.hidden_act], text_cfg.layer_norm_eps


def fill_image_config(cfg: "_lib.E2VConfig", image_cfg: ImageConfig) -> None:
    """The ``vit_*`` fields of an ``e2v_config`` from an ``ImageConfig``."""
    cfg.vit_hidden, cfg.vit_heads, cfg.vit_layers = image_cfg.hidden, image_cfg.heads, image_cfg.layers
    cfg.vit_intermediate, cfg.vit_image_size, cfg.vit_patch_size = image_cfg.intermediate, image_cfg.image_size, image_cfg.patch_size
    cfg.vit_num_labels, cfg.vit_norm_eps, cfg.vit_rescale = image_cfg.num_labels, image_cfg.layer_norm_eps, float(image_cfg.rescale_factor)
    cfg.vit_mean = (C.c_float * 3)(*[float(v) for v in image_cfg.image_mean])
    cfg.vit_std = (C.c_float * 3)(*[float(v) for v in image_cfg.image_std])


def fill_video_config(cfg: "_lib.E2VConfig", video_cfg: VideoConfig) -> None:
    """The ``vmae_*`` fields of an ``e2v_config`` from a ``VideoConfig``."""
    cfg.vmae_hidden, cfg.vmae_heads, cfg.vmae_layers = video_cfg.hidden, video_cfg.heads, video_cfg.layers
    cfg.vmae_intermediate, cfg.vmae_image_size, cfg.vmae_patch_size = video_cfg.intermediate, video_cfg.image_size, video_cfg.patch_size
    cfg.vmae_tubelet_size, cfg.vmae_num_frames, cfg.vmae_num_labels = video_cfg.tubelet_size, video_cfg.num_frames, video_cfg.num_labels
    cfg.vmae_norm_eps, cfg.vmae_resize_edge, cfg.vmae_rescale = video_cfg.layer_norm_eps, video_cfg.resize_edge, float(video_cfg.rescale_factor)
    cfg.vmae_mean = (C.c_float * 3)(*[float(v) for v in video_cfg.image_mean])
    cfg.vmae_std = (C.c_float * 3)(*[float(v) for v in video_cfg.image_std])


def clip_vision_config(cv: ClipVisionConfig) -> "_lib.E2VClipVConfig":
    """The ``e2v_clipv_config`` of a ``ClipVisionConfig`` (``e2v_create_clip_vision``)."""
    cfg = _lib.E2VClipVConfig()
    if cv.hidden_act not in TEXT_ACTS:
        raise ValueError(f"clip vision hidden_act {cv.hidden_act!r}: the library has {sorted(TEXT_ACTS)}")
    cfg.clipv_hidden, cfg.clipv_heads, cfg.clipv_layers, cfg.clipv_intermediate = cv.hidden, cv.heads, cv.layers, cv.intermediate
    cfg.clipv_image_size, cfg.clipv_patch_size, cfg.clipv_projection_dim = cv.image_size, cv.patch_size, cv.projection_dim
    cfg.clipv_act, cfg.clipv_norm_eps = TEXT_ACTS[cv.hidden_act], cv.layer_norm_eps
    cfg.clipv_resize_edge, cfg.clipv_resample, cfg.clipv_rescale = cv.resize_edge, cv.resample, float(cv.rescale_factor)
    cfg.clipv_mean = (C.c_float * 3)(*[float(v) for v in cv.image_mean])
    cfg.clipv_std = (C.c_float * 3)(*[float(v) for v in cv.image_std])
    return cfg


def seq2seq_config(sc: Seq2SeqConfig) -> "_lib.E2VS2sConfig":
    """The ``e2v_s2s_config`` of a ``Seq2SeqConfig`` (``e2v_create_ex``)."""
    cfg = _lib.E2VS2sConfig()
    cfg.s2s_electrodes, cfg.s2s_samples, cfg.s2s_windows = sc.electrodes, sc.samples, sc.windows
    cfg.s2s_f1, cfg.s2s_d, cfg.s2s_f2 = sc.F1, sc.D, sc.F2
    cfg.s2s_d_model, cfg.s2s_heads, cfg.s2s_ffn = sc.d_model, sc.heads, sc.ffn
    cfg.s2s_encoder_layers, cfg.s2s_decoder_layers, cfg.s2s_steps = sc.encoder_layers, sc.decoder_layers, sc.steps
    cfg.s2s_latent_channels, cfg.s2s_latent_h, cfg.s2s_latent_w = sc.latent
    cfg.s2s_txt_classes, cfg.s2s_norm_eps, cfg.s2s_bn_eps = sc.txt_classes, sc.norm_eps, sc.bn_eps
    return cfg


def glmnet_config(gc: GLMNetConfig) -> "_lib.E2VGlmConfig":
    """The ``e2v_glm_config`` of a ``GLMNetConfig`` (``e2v_create_ex2``)."""
    cfg = _lib.E2VGlmConfig()
    cfg.glm_electrodes, cfg.glm_samples, cfg.glm_occ_first, cfg.glm_occ_count = gc.electrodes, gc.samples, gc.occ_first, gc.occ_count
    cfg.glm_filters, cfg.glm_taps, cfg.glm_pool, cfg.glm_pool_stride = gc.filters, gc.taps, gc.pool, gc.pool_stride
    cfg.glm_bands, (cfg.glm_hidden1, cfg.glm_hidden2), cfg.glm_emb = gc.bands, gc.hidden, gc.emb
    cfg.glm_raw_out, cfg.glm_mlp_out, cfg.glm_bn_eps = gc.raw_out, gc.mlp_out, gc.bn_eps
    return cfg


def image_resize_table(in_size: int, out_size: int, filter: Optional[int] = None):
    """One axis of Pillow's antialiased resize (host arithmetic, no GPU): ``(first, count, coeff)`` -- ``first``, ``count`` int32
    ``[out_size]``, ``coeff`` int32 ``[out_size, ksize]`` in 22-bit fixed point.  ``filter``: ``None`` -- BILINEAR through
    ``e2v_image_resize_table`` --, or Pillow's code through ``e2v_image_resize_table_filter``: 2 BILINEAR, 3 BICUBIC."""
    lib = _lib.load()
    ksize = C.c_int(0)
    if filter is None:
        call = lambda *a: lib.e2v_image_resize_table(in_size, out_size, *a)
    else:
        call = lambda *a: lib.e2v_image_resize_table_filter(in_size, out_size, int(filter), *a)
    if call(None, None, None, C.byref(ksize)) != _lib.E2V_OK:
        raise ValueError(f"image_resize_table({in_size}, {out_size}, filter={filter}): sizes must be at least 1, the filter 2 or 3")
    first, count = np.zeros(out_size, dtype=np.int32), np.zeros(out_size, dtype=np.int32)
    coeff = np.zeros((out_size, ksize.value), dtype=np.int32)
    call(first.ctypes.data_as(C.POINTER(C.c_int)), count.ctypes.data_as(C.POINTER(C.c_int)), coeff.ctypes.data_as(C.POINTER(C.c_int32)),
         C.byref(ksize))
    return first, count, coeff


def named_tensors(source, only_trainable: bool = False):
    """``(name, tensor)`` pairs of what ``sync_from`` accepts: an ``nn.Module`` (its ``named_parameters()``, those with
    ``requires_grad`` when ``only_trainable``), a mapping, or an iterable of pairs."""
    if hasattr(source, "named_parameters"):
        return [(n, p) for n, p in source.named_parameters() if not only_trainable or p.requires_grad]
    if only_trainable:
        raise ValueError("only_trainable needs a module: a state dict does not say which of its tensors train")
    return list(source.items()) if isinstance(source, Mapping) else list(source)


def compute_dtype_code(dtype) -> int:
    """The ``e2v_dtype`` of an arithmetic mode named as a string or as the ``torch.dtype`` a caller of the reference passes."""
    names = {"fp32": _lib.E2V_F32, "f32": _lib.E2V_F32, "float32": _lib.E2V_F32, "bf16": _lib.E2V_BF16, "bfloat16": _lib.E2V_BF16,
             "fp16": _lib.E2V_F16, "f16": _lib.E2V_F16, "half": _lib.E2V_F16, "float16": _lib.E2V_F16, "f32x3": _lib.E2V_F32X3}
    if isinstance(dtype, torch.dtype):
        dtype = str(dtype).replace("torch.", "")
    if dtype not in names:
        raise ValueError(f"compute dtype {dtype!r}: one of {sorted(names)}")
    return names[dtype]


def describe_dispatch(dtype: str = "bf16", batch: int = 32, frames: int = 6, h: int = 36, w: int = 64, tokens: int = 77, config=None):
    """Which kernel and tile every launch of ``e2v_generate`` (one guided DDIM step + decode of ``batch`` clips) takes, as a list of
    ``"<launches>x <class> <shape> -> <kernel> <tile>"`` lines -- ``e2v_op_describe_dispatch`` on a host-only context: no GPU, no
    weights (``tests/test_dispatch_golden.py`` pins the SD-v1-4 table)."""
    lib = _lib.load()
    cfg = _lib.E2VConfig()
    lib.e2v_default_config(C.byref(cfg))
    if config is not None:
        for k, v in config.items():
            setattr(cfg, k, v)
    ctx = C.c_void_p()
    if lib.e2v_create(C.byref(cfg), -1, C.byref(ctx)) != _lib.E2V_OK:
        raise RuntimeError("e2v_create(host-only) failed")
    try:
        code = compute_dtype_code(dtype)
        need = C.c_int64(0)
        st = lib.e2v_op_describe_dispatch(ctx, code, batch, frames, h, w, tokens, None, 0, C.byref(need))
        if st != _lib.E2V_OK:
            raise RuntimeError(f"e2v_op_describe_dispatch: {(lib.e2v_last_error(ctx) or b'').decode()}")
        buf = C.create_string_buffer(need.value)
        st = lib.e2v_op_describe_dispatch(ctx, code, batch, frames, h, w, tokens, buf, need.value, C.byref(need))
        if st != _lib.E2V_OK:
            raise RuntimeError(f"e2v_op_describe_dispatch: {(lib.e2v_last_error(ctx) or b'').decode()}")
        return buf.value.decode().splitlines()
    finally:
        lib.e2v_destroy(ctx)
