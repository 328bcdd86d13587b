"""DE / PSD features of raw EEG on the device: the reference's ``DE_PSD`` (``EEG_preprocessing/DE_PSD.py:8-71``) and the loops of its
three extractors (2-s, 1-s and 500-ms sliding windows) as one kernel launch (``e2v_eeg_de_psd``).

* ``DE_PSD(data, fre, time_window)`` -- the reference's name, signature and shapes for one ``[n, m]`` array: ``(de, psd)``, each
  ``[n, 5]``.  numpy in means numpy out (float32: the reference computes in float64 and its callers store float32).
* ``de_psd(segments, window=, step=, scaler=)`` -- batched, over ``[B, C, L]`` device tensors, the windows read where they lie.

What the reference does and this keeps: the transform length is 200 whatever the row length, so a 400-sample row is truncated to its
first 200 windowed samples (the Hann row still has the row's length) and a 100-sample row is zero-padded; the bands overlap by a
bin.  What differs: an all-zero row gives ``psd`` 0 and ``de`` ``-inf`` where the reference raises ``ValueError``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .engine import Engine
from .weights import TINY_UNET, TINY_VAE

BANDS = ((1, 4), (4, 8), (8, 14), (14, 31), (31, 99))      # delta, theta, alpha, beta, gamma (Hz)
_ENGINES = {}


def default_engine(device: int = 0) -> Engine:
    """An engine for callers that have none: the features need no weights, so the smallest context will do (one per device)."""
    if device not in _ENGINES:
        _ENGINES[device] = Engine(TINY_UNET, TINY_VAE, device)
    return _ENGINES[device]


def DE_PSD(data, fre, time_window, engine: Optional[Engine] = None):  # noqa: N802  (the reference's name)
    """``data`` ``[n, m]`` (electrodes, time points), ``fre`` the sampling rate, ``time_window`` the window in seconds with
    ``int(time_window * fre) == m`` (the reference multiplies the row by a Hann row of that length) -> ``(de, psd)``, each ``[n, 5]``.
    A numpy array gives numpy arrays, a tensor gives tensors on the engine's device."""
    as_numpy = not isinstance(data, torch.Tensor)
    x = torch.as_tensor(np.asarray(data, dtype=np.float32)) if as_numpy else data
    if x.dim() != 2:
        raise ValueError(f"expected data [n, m], got {tuple(x.shape)}")
    n, m = x.shape
    if int(time_window * fre) != m:
        raise ValueError(f"int(time_window * fre) = {int(time_window * fre)} is not the row length {m}: the Hann row would not fit the data")
    if int(fre) != fre:
        raise ValueError(f"the sampling rate {fre!r} has to be a whole number of Hz")
    eng = engine if engine is not None else default_engine()
    x = x.to(device=eng.device, dtype=torch.float32).contiguous()
    de, psd = eng.eeg_de_psd(x.reshape(1, 1, n, m), fs=int(fre))
    de, psd = de.reshape(n, 5), psd.reshape(n, 5)
    return (de.cpu().numpy(), psd.cpu().numpy()) if as_numpy else (de, psd)


def de_psd(segments: torch.Tensor, window: Optional[int] = None, step: Optional[int] = None, scaler: Optional[Tuple] = None, fs: int = 200,
           engine: Optional[Engine] = None, de: bool = True, psd: bool = True):
    """``segments`` ``[B, C, L]``, a contiguous fp32 tensor on the engine's device.  ``window`` samples per window (``None``: ``L``, one
    window), ``step`` samples between window starts (``None``: ``window``) -- the reference's 500-ms extractor over a 2-s segment is
    ``window=100, step=50``, seven windows.  ``scaler``: ``(mean, scale)`` of ``C * 5`` values each (a fitted ``StandardScaler``'s
    ``mean_`` and ``scale_`` over the flattened ``[C, 5]`` features), applied to DE.  Returns ``(de, psd)``, each ``[B, windows, C, 5]``
    (``None`` where not asked for)."""
    if not isinstance(segments, torch.Tensor) or segments.dim() != 3:
        raise ValueError("expected segments [B, C, L] as a tensor")
    b, c, length = (int(v) for v in segments.shape)
    window = length if window is None else int(window)
    step = window if step is None else int(step)
    if window < 1 or window > length or step < 1:
        raise ValueError(f"window {window} / step {step} over rows of {length} samples")
    windows = (length - window) // step + 1
    eng = engine if engine is not None else default_engine(segments.device.index or 0)
    if scaler is not None:
        scaler = tuple(torch.as_tensor(np.asarray(v, dtype=np.float32)) if not isinstance(v, torch.Tensor) else v for v in scaler)
    return eng.eeg_de_psd(segments, samples=window, strides=(c * length, step, length), batch=b, windows=windows, electrodes=c, fs=fs,
                          scaler=scaler, de=de, psd=psd)
