"""``myTransformer`` -- the reference's Seq2Seq latent model (``EEG2Video_New/Seq2Seq/my_autoregressive_transformer.py:123-192``) on the
engine: EEG windows in, the UNet latents the reference's inference saves (``:383-387``: ``out[:, :-1]``) out.  Named after the
reference's class; ``Seq2Seq`` is an alias.

It loads the reference's ``seq2seqmodel.pt`` (``torch.save({'state_dict': model.state_dict()}, ...)``, ``:391``) or a bare state dict
with the reference's 125 names.  Of those the device holds what inference reads (``Engine.SEQ2SEQ``, keys under ``s2s.``); the rest --
``embedding.weight``, ``img_embedding.*``, every ``num_batches_tracked``, and the ``[1, 5000, d_model]`` position buffer of which
``windows`` rows are read -- stay on the host, so that ``state_dict()`` gives every entry back bit for bit.

``host_models.Seq2SeqLatents`` is NOT this model: it is a look-alike with random weights that was written from the shapes, differs on
purpose (it returns ``lat[:, 1:]``) and is left as the sweep's default stage.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional, Tuple

import numpy as np
import torch

from .engine import Engine
from .weights import (SEQ2SEQ_PE_KEY, Seq2SeqConfig, UNetConfig, VAEConfig, seq2seq_engine_spec, seq2seq_param_spec,
                      seq2seq_position_table, seq2seq_unused_key, synth_state_dict)

PREFIX = "s2s."


def scaler_to_windows(values, cfg: Seq2SeqConfig) -> torch.Tensor:
    """A per-feature vector of the reference's ``StandardScaler`` (``mean_`` or ``scale_``) -> ``[windows, electrodes, samples]``.
    The reference stacks the windows LAST and flattens ``[b, c, l, f]`` (``:314,320-321``), so feature ``(c * samples + l) * windows + f``
    belongs to sample ``l`` of electrode ``c`` of window ``f``; it then moves the window axis to the front (``:327-329``)."""
    v = torch.as_tensor(np.asarray(values), dtype=torch.float32)
    if v.numel() != cfg.electrodes * cfg.samples * cfg.windows:
        raise ValueError(f"the scaler has {v.numel()} features, expected electrodes * samples * windows = "
                         f"{cfg.electrodes * cfg.samples * cfg.windows}")
    return v.reshape(cfg.electrodes, cfg.samples, cfg.windows).permute(2, 0, 1).contiguous()


class myTransformer:  # noqa: N801  (the reference's name)
    """``myTransformer(config=Seq2SeqConfig(), engine=None, device=0)``: the model on an engine of its own, or on ``engine`` (one that
    was built with ``seq2seq_cfg=config``)."""

    def __init__(self, config: Seq2SeqConfig = Seq2SeqConfig(), engine: Optional[Engine] = None, device: int = 0):
        self.cfg = config
        if engine is not None and engine.seq2seq_cfg != config:
            raise RuntimeError("the engine was not built with this Seq2Seq config: create it with Engine(..., seq2seq_cfg=config)")
        self.engine = engine if engine is not None else Engine(UNetConfig(), VAEConfig(), device, seq2seq_cfg=config)
        self._host = OrderedDict()           # what the device does not hold, as loaded
        self._scaler = None
        self.window, self.step = config.samples, config.samples // 2      # the reference's sliding windows (:309-310)

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
        return seq2seq_param_spec(self.cfg)

    def load_state_dict(self, state_dict, strict: bool = True):
        """The reference's names.  ``positional_encoding.pe`` may be the checkpoint's ``[1, max_len, d_model]`` buffer (its first
        ``windows`` rows go to the device, all of it is kept for ``state_dict()``) or absent: the table is then computed with the
        reference's fp32 torch expression.  The other 124 entries must be there; with ``strict=False`` unknown names are ignored."""
        spec, cfg = self.state_dict_spec(), self.cfg
        missing = [k for k in spec if k not in state_dict and k != SEQ2SEQ_PE_KEY]
        unexpected = [k for k in state_dict if k not in spec]
        if missing or (strict and unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for myTransformer: missing {missing[:4]}... unexpected {unexpected[:4]}...")
        as_tensor = lambda v: v.detach().cpu() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))
        host, dev = OrderedDict(), OrderedDict()
        for k, shape in spec.items():
            if k == SEQ2SEQ_PE_KEY:
                if k in state_dict:
                    pe = as_tensor(state_dict[k])
                    if pe.dim() != 3 or pe.shape[0] != 1 or pe.shape[1] < cfg.windows or pe.shape[2] != cfg.d_model:
                        raise RuntimeError(f"size mismatch for {k}: {tuple(pe.shape)}, expected [1, >= {cfg.windows}, {cfg.d_model}]")
                    host[k] = pe.clone()
                    dev[k] = pe[0, :cfg.windows].float().contiguous()
                else:
                    dev[k] = seq2seq_position_table(cfg.windows, cfg.d_model)
                continue
            v = as_tensor(state_dict[k])
            if tuple(v.shape) != tuple(shape):
                raise RuntimeError(f"size mismatch for {k}: {tuple(v.shape)}, expected {tuple(shape)}")
            if seq2seq_unused_key(k):
                host[k] = v.clone()
            else:
                dev[k] = v
        self.engine.load_state_dict(dev, prefix=PREFIX)
        self.engine.finalize(Engine.SEQ2SEQ)
        self._host = host
        return self

    def state_dict(self, device="cpu"):
        """All 125 entries under the reference's names and in its order: the device's tensors read back (``Engine.read_tensor``), the
        entries inference never reads as they were loaded (a model built by ``init_synthetic`` or from a checkpoint without the position
        buffer gets the full ``[1, pe_max_len, d_model]`` table from the reference's expression)."""
        out = OrderedDict()
        held = seq2seq_engine_spec(self.cfg)
        for k in self.state_dict_spec():
            if k in self._host:
                out[k] = self._host[k].clone().to(device)
            elif k == SEQ2SEQ_PE_KEY:
                out[k] = seq2seq_position_table(self.cfg.pe_max_len, self.cfg.d_model)[None].to(device)
            elif k in held:
                out[k] = self.engine.read_tensor(PREFIX + k).to(device)
            else:
                raise RuntimeError(f"{k} was never loaded")
        return out

    def save_checkpoint(self, path: str) -> None:
        """``torch.save({'state_dict': ...}, path)``, the reference's own file (``:388-391``)."""
        torch.save({"state_dict": self.state_dict(device="cpu")}, path)

    @classmethod
    def from_checkpoint(cls, path: str, config: Seq2SeqConfig = Seq2SeqConfig(), *, engine: Optional[Engine] = None, device: int = 0):
        """A local ``.pt`` holding ``{'state_dict': ...}`` as the reference saves it, or a bare state dict."""
        obj = torch.load(path, map_location="cpu", weights_only=True)
        sd = obj["state_dict"] if isinstance(obj, dict) and "state_dict" in obj and not isinstance(obj["state_dict"], torch.Tensor) else obj
        return cls(config, engine=engine, device=device).load_state_dict(sd)

    def init_synthetic(self, seed: int = 47, mode: str = "perturbed"):
        sd = synth_state_dict(self.state_dict_spec(), seed=seed, mode=mode)
        del sd[SEQ2SEQ_PE_KEY]
        sd = {k: (np.zeros(v.shape, np.int64) if k.endswith("num_batches_tracked") else v) for k, v in sd.items()}
        return self.load_state_dict(sd)

    def set_input_scaler(self, mean=None, scale=None):
        """The reference's ``StandardScaler`` (``:323-326``) applied on the device as a value is read: ``mean`` / ``scale`` are its
        ``mean_`` / ``scale_`` (``electrodes * samples * windows`` features in sklearn's order) or already ``[windows, electrodes,
        samples]``.  ``None``: no scaler."""
        if (mean is None) != (scale is None):
            raise ValueError("the scaler is a mean AND a scale, or neither")
        if mean is None:
            self._scaler = None
            return self
        shape = (self.cfg.windows, self.cfg.electrodes, self.cfg.samples)
        conv = lambda v: (torch.as_tensor(np.asarray(v), dtype=torch.float32) if tuple(np.shape(v)) == shape else scaler_to_windows(v, self.cfg))
        self._scaler = (conv(mean).to(self.device).contiguous(), conv(scale).to(self.device).contiguous())
        return self

    # -- forward -----------------------------------------------------------------------------
    def _input(self, src, window=None, step=None):
        """-> (tensor, strides or None, batch): stacked windows ``[B, windows, electrodes, samples]`` or a raw segment
        ``[B, electrodes, L]`` read through sliding windows (no copy is made of either)."""
        c = self.cfg
        x = src if isinstance(src, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(src))
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if x.dim() == 4:
            if tuple(x.shape[1:]) != (c.windows, c.electrodes, c.samples):
                raise ValueError(f"expected src [B,{c.windows},{c.electrodes},{c.samples}], got {tuple(x.shape)}")
            return x, None, x.shape[0]
        if x.dim() != 3 or x.shape[1] != c.electrodes:
            raise ValueError(f"expected stacked windows [B,{c.windows},{c.electrodes},{c.samples}] or a segment [B,{c.electrodes},L], got {tuple(x.shape)}")
        window = self.window if window is None else int(window)
        step = self.step if step is None else int(step)
        length = x.shape[2]
        if window != c.samples or step < 1 or (length - window) // step + 1 != c.windows or length < window:
            raise ValueError(f"a segment of {length} samples under windows of {window} with step {step} does not give the model's "
                             f"{c.windows} windows of {c.samples}")
        return x, (c.electrodes * length, step, length), x.shape[0]

    def forward(self, src, tgt=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(txt_logits [B,classes], latents [B,steps+1,C,h,w])``, the reference's return order.  ``tgt`` contributes its shape only, as in
        the reference (``:157-158,176``): ``[B, steps+1, C, h, w]`` is checked when given."""
        x, strides, b = self._input(src)
        c = self.cfg
        if tgt is not None and tuple(tgt.shape) != (b, c.steps + 1) + tuple(c.latent):
            raise ValueError(f"expected tgt [{b},{c.steps + 1},{','.join(str(v) for v in c.latent)}], got {tuple(tgt.shape)}")
        out = self.engine.seq2seq_latents(x, strides=strides, batch=b, scaler=self._scaler, first=0, count=c.steps + 1, txt_logits=True)
        return out["txt_logits"], out["latents"]

    __call__ = forward

    def predict_latents(self, src_or_segment, layout: str = "bcfhw", window: Optional[int] = None, step: Optional[int] = None) -> torch.Tensor:
        """The latents the reference's inference keeps, ``forward(...)[1][:, :-1]`` (``:383-384``), without running the pass it throws
        away: ``[B,C,steps,h,w]`` (``layout='bcfhw'``, what the pipeline takes) or ``[B,steps,C,h,w]`` (``'bfchw'``, what
        ``Engine.dana_noise`` takes).  A raw segment ``[B, electrodes, L]`` is read through the reference's sliding windows
        (``window`` = ``samples``, ``step`` = half of it) where it lies."""
        x, strides, b = self._input(src_or_segment, window, step)
        return self.engine.seq2seq_latents(x, strides=strides, batch=b, scaler=self._scaler, first=0, count=self.cfg.steps,
                                           layout=layout)["latents"]


Seq2Seq = myTransformer
