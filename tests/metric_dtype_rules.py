"""What the 16-bit metric-tower tests share: the two fixtures side by side, the bounds derived from them, and the ranking rules.
Pure numpy; no kernel is called from here (``tests/test_hip_metric_dtype.py`` on the device, ``tests/test_metric_dtype_host.py`` without one).

Bounds.  ``tests/golden/metric_towers_16bit.npz`` holds what torch on the CPU gives for the three tiny models run in fp16 and bf16
(``tests/golden/make_metric_dtype_golden.py``).  The device in the same mode and that CPU run are two independent draws of rounding
noise of the same class -- the same roundings per layer, another accumulation order, other rounding points -- around the fp32 result, so
the device is held to ``FACTOR`` = 4 x the CPU run's distance from the fp32 fixture, the factor ``tests/test_hip_full.py`` uses for its
bf16 tails (``far <= 4.0 * farp``).  The distances are recomputed here from the two fixtures, never read from a constant.

Ranking.  With every logit within ``bound`` of its fp32 value, two labels can change places only if their fp32 logits are within
``2 bound`` of each other.  So for a row with fp32 logits ``l`` (descending ``l1 >= l2 >= l3 >= l4 ...``):
  * a top-3 label is *ambiguous* if it lies within ``2 bound`` of ``l4`` (a label from outside could pass it), a label outside the top 3
    if it lies within ``2 bound`` of ``l3`` (it could pass the third);
  * the device's top 3 must contain every unambiguous top-3 label and nothing outside top 3 + ambiguous;
  * two labels further apart than ``2 bound`` keep their order.
Nothing exempts a row as a whole: the rule is applied label by label and pair by pair.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FACTOR = 4.0
DTYPES = ("fp16", "bf16")
#: tower -> (fp32 fixture file, {quantity in the 16-bit fixture: key in the fp32 fixture})
TOWERS = {
    "vit": ("vit_tiny.npz", {"logits": "logits", "probs": "probs"}),
    "videomae": ("videomae_tiny.npz", {"logits": "logits", "probs": "probs"}),
    "clip": ("clip_vision_tiny.npz", {"embeds": "image_embeds", "pairs": "pair_scores", "matrix": "matrix"}),
}


def load16():
    z = np.load(os.path.join(HERE, "golden", "metric_towers_16bit.npz"))
    return {k: z[k] for k in z.files}


def load32(tower):
    z = np.load(os.path.join(HERE, "golden", TOWERS[tower][0]))
    return {k: z[k] for k in z.files if not k.startswith("w.")}


def cpu_distance(z16, z32, tower, quantity, dtype):
    """max |torch-CPU 16-bit result - fp32 fixture|"""
    return float(np.abs(z16[f"{tower}_{quantity}_{dtype}"].astype(np.float64) - z32[TOWERS[tower][1][quantity]].astype(np.float64)).max())


def bound(z16, z32, tower, quantity, dtype):
    return FACTOR * cpu_distance(z16, z32, tower, quantity, dtype)


def top3_ascending(logits):
    """the three largest labels by (value, index), ascending: what ``logits.argsort(-1)[-3:]`` gives"""
    return np.argsort(np.asarray(logits), axis=-1, kind="stable")[..., -3:]


def ambiguous_labels(ref_row, b):
    srt = np.sort(ref_row)
    l3, l4 = srt[-3], srt[-4]
    top = set(int(i) for i in top3_ascending(ref_row))
    amb = set()
    for j, v in enumerate(ref_row):
        if (j in top and v - l4 <= 2 * b) or (j not in top and l3 - v <= 2 * b):
            amb.add(j)
    return top, amb


def check_top3(got_top3, ref_logits, b, what=""):
    """``got_top3`` ``[rows,3]`` ascending as the device lists them; returns how many rows had their top-3 SET fully determined"""
    determined = 0
    for r, (got, ref) in enumerate(zip(np.asarray(got_top3), np.asarray(ref_logits, dtype=np.float64))):
        top, amb = ambiguous_labels(ref, b)
        got = [int(i) for i in got]
        assert len(set(got)) == 3, f"{what} row {r}: top 3 {got} repeats a label"
        missing = (top - amb) - set(got)
        assert not missing, f"{what} row {r}: unambiguous top-3 labels {sorted(missing)} missing from {got} (fp32 top 3 {sorted(top)}, 2 x bound {2 * b:.3e})"
        foreign = set(got) - (top | amb)
        assert not foreign, f"{what} row {r}: labels {sorted(foreign)} are neither top 3 nor within 2 x bound = {2 * b:.3e} of the 3rd-largest logit"
        for i in range(3):
            for j in range(i + 1, 3):                         # got[i] is listed BELOW got[j]
                assert ref[got[i]] - ref[got[j]] <= 2 * b, \
                    f"{what} row {r}: label {got[i]} listed below {got[j]} though its fp32 logit is {ref[got[i]] - ref[got[j]]:.3e} higher"
        determined += not (amb & top) and not (amb - top)
    return determined


def check_row_ranking(got, ref, b, what=""):
    """every row of ``got``: columns whose ``ref`` scores differ by more than ``2 b`` keep their order; returns (pairs determined, pairs)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fixed = total = 0
    for r in range(ref.shape[0]):
        d_ref = ref[r][:, None] - ref[r][None, :]
        d_got = got[r][:, None] - got[r][None, :]
        far = d_ref > 2 * b
        bad = far & ~(d_got > 0)
        assert not bad.any(), f"{what} row {r}: columns {np.argwhere(bad)[0].tolist()} changed places though {d_ref[bad][0]:.3e} apart (2 x bound {2 * b:.3e})"
        fixed += int(far.sum())
        total += ref.shape[1] * (ref.shape[1] - 1) // 2
    return fixed, total
