"""The reference's ``DE_PSD`` (``EEG_preprocessing/DE_PSD.py:8-71``) restated in numpy, without scipy: what the fixture pins and the
device is compared with.

``de_psd(data, fs, dtype)`` over ``[..., m]`` rows -> ``(de, psd)`` ``[..., 5]``:
* the Hann row ``0.5 - 0.5 cos(2 pi k / (m + 1))``, ``k = 1 .. m`` (every caller of the reference passes ``time_window * fre = m``);
* ``fft(windowed, 200)``: the transform length is 200 WHATEVER ``m`` is -- a longer row is truncated to its first 200 windowed
  samples, a shorter one zero-padded -- here as the direct sum over the samples in index order;
* band ``p``: ``range(fStartNum - 1, fEndNum)`` with ``fStartNum = int(fStart / fs * 200)``, ``fEndNum = int(fEnd / fs * 200)``, i.e.
  bins ``fStartNum - 1 .. fEndNum - 1`` (at 200 Hz: 0..3, 3..7, 7..13, 13..30, 30..98 -- the bands overlap by a bin), summed in
  ascending order and divided by ``fEndNum - fStartNum + 1``;
* ``psd = E``, ``de = log2(100 E)``.

``dtype=np.float64`` is the restatement proper (it sits at rounding distance from the reference's float64).  ``dtype=np.float32`` rounds
the tables once from double and runs every product and every sum in fp32 in index order: an fp32 implementation's arithmetic, from
whose distance to the reference the tests take their bound.  An all-zero row gives ``psd`` 0 and ``de`` ``-inf`` (the reference
raises ``ValueError`` there).
"""
import numpy as np

STFTN = 200
F_START, F_END = (1, 4, 8, 14, 31), (4, 8, 14, 31, 99)


def band_bins(fs):
    """``[(first, last)]`` inclusive per band, or ``None`` where the reference would index from the end or past the half spectrum"""
    out = []
    for s, e in zip(F_START, F_END):
        s_num, e_num = int(s / fs * STFTN), int(e / fs * STFTN)
        if s_num < 1 or e_num > STFTN // 2 or e_num < s_num:
            return None
        out.append((s_num - 1, e_num - 1))
    return out


def de_psd(data, fs=200, dtype=np.float64):
    x = np.asarray(data)
    m = x.shape[-1]
    bins = band_bins(fs)
    assert bins is not None, fs
    n = min(m, STFTN)
    hann = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1, m + 1, dtype=np.float64) / (m + 1)))[:n].astype(dtype)
    ang = 2.0 * np.pi * np.arange(STFTN, dtype=np.float64) / STFTN
    cos, sin = np.cos(ang).astype(dtype), np.sin(ang).astype(dtype)
    rows = x.reshape(-1, m)[:, :n].astype(dtype) * hann
    nb = max(last for _, last in bins) + 1
    j = np.arange(nb)
    re, im = np.zeros((rows.shape[0], nb), dtype), np.zeros((rows.shape[0], nb), dtype)
    for k in range(n):                                   # index order: one running sum per bin
        idx = (j * k) % STFTN
        re = re + rows[:, k:k + 1] * cos[idx]
        im = im + rows[:, k:k + 1] * sin[idx]
    power = re * re + im * im
    psd = np.zeros((rows.shape[0], len(bins)), dtype)
    for p, (first, last) in enumerate(bins):
        e = np.zeros(rows.shape[0], dtype)
        for b in range(first, last + 1):
            e = e + power[:, b]
        psd[:, p] = e / dtype(last - first + 1)
    with np.errstate(divide="ignore"):
        de = np.log2(dtype(100) * psd)
    shape = x.shape[:-1] + (len(bins),)
    return de.reshape(shape), psd.reshape(shape)


def windows_of(segments, window, step):
    """``[B, C, L]`` -> the stacked windows ``[B, W, C, window]`` the strided read stands for"""
    x = np.asarray(segments)
    count = (x.shape[-1] - window) // step + 1
    return np.stack([x[..., w * step:w * step + window] for w in range(count)], axis=1)
