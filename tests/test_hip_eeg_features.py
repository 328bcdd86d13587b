"""GPU: DE / PSD features on the device (``e2v_eeg_de_psd``, ``eeg2video_amd.features``) against the fixture the reference's own
``DE_PSD`` wrote and against the float64 restatement (``tests/eeg_features_restatement.py``).

Bounds, none fixed here.  PSD is compared relatively per element (``max |a - b| / |b|``), DE absolutely (``max |a - b|``):
* against the fixture: ten times the fixture's stored distance of the fp32 index-order restatement from ``DE_PSD``;
* at the other shapes: ten times the distance of the same fp32 restatement from the float64 one on the same rows, measured in the test.
"""
import numpy as np
import pytest
import torch

from eeg2video_amd.weights import TINY_UNET, TINY_VAE
from eeg_features_restatement import de_psd, windows_of
from test_eeg_features_host import load_fixture, maker
from test_hip_bounds import GUARD_KIB, environment, fenced, fenced_out, guarded_run, run_fenced, same_bits

pytestmark = pytest.mark.gpu


def rows_of(*shape, seed=0):
    """N(0, 20^2) as fp32: band energies far from zero, as the fixture's rows"""
    g = torch.Generator().manual_seed(seed)
    return (20.0 * torch.randn(*shape, generator=g, dtype=torch.float64)).float()


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def eng():
    from eeg2video_amd.engine import Engine
    return Engine(TINY_UNET, TINY_VAE, 0)


def distances(de, psd, de64, psd64):
    de, psd = (np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64) if v is not None else None for v in (de, psd))
    e_psd = float(np.max(np.abs(psd - psd64) / np.abs(psd64))) if psd is not None else 0.0
    e_de = float(np.max(np.abs(de - de64))) if de is not None else 0.0
    return e_de, e_psd


def held(de, psd, x, what, fs=200):
    """the device within 10 x the distance of the fp32 index-order restatement from the float64 one on the same rows"""
    de64, psd64 = de_psd(x.numpy(), fs, np.float64)
    de32, psd32 = de_psd(x.numpy(), fs, np.float32)
    d_de, d_psd = distances(de32, psd32, de64, psd64)
    e_de, e_psd = distances(de, psd, de64, psd64)
    print(f"{what}: device vs float64 de {e_de:.3e} (fp32 restatement {d_de:.3e}), psd {e_psd:.3e} ({d_psd:.3e})")
    assert e_de <= 10 * d_de and e_psd <= 10 * d_psd, (what, e_de, d_de, e_psd, d_psd)


# ------------------------------------------------------------------ 1. the reference's fixture --------------------------------------
@pytest.mark.parametrize("m", [100, 200, 400])
def test_fixture_parity(eng, m):
    fx = load_fixture()
    rows = torch.from_numpy(maker().de_psd_rows(m))
    de, psd = eng.eeg_de_psd(rows.cuda().reshape(1, 1, 62, m))
    e_de, e_psd = distances(de.reshape(62, 5), psd.reshape(62, 5), fx[f"de_{m}"], fx[f"psd_{m}"])
    d_de, d_psd = float(fx[f"d32_de_{m}"]), float(fx[f"d32_psd_{m}"])
    print(f"m = {m}: device vs DE_PSD de {e_de:.3e} (bound {10 * d_de:.3e}), psd {e_psd:.3e} (bound {10 * d_psd:.3e})")
    assert e_de <= 10 * d_de and e_psd <= 10 * d_psd


# ------------------------------------------------------------------ 2. the op over shapes -------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 62])
@pytest.mark.parametrize("m", [1, 99, 100, 199, 200, 201, 400])
def test_op_shapes_fenced(eng, m, C):
    """m = 1: the Hann row is 1; 99 / 100 / 199: zero-padded; 200: exact; 201 / 400: truncated to 200 windowed samples"""
    for B in (1, 2, 5):
        x = rows_of(B, 1, C, m, seed=1000 * m + 10 * C + B)
        fin, fde, fpsd = fenced(x, name="eeg"), fenced_out((B, 1, C, 5)), fenced_out((B, 1, C, 5))
        eng.eeg_de_psd(fin.t, out=dict(de=fde.t, psd=fpsd.t))
        torch.cuda.synchronize()
        for f in (fin, fde, fpsd):
            f.check()
        held(fde.view.reshape(B, 1, C, 5), fpsd.view.reshape(B, 1, C, 5), x, f"m{m} C{C} B{B}")


@pytest.mark.parametrize("B", [1, 2, 5])
def test_sliding_windows_of_one_segment(eng, B):
    """the seven 100-sample windows of a [B, 62, 400] segment, 50 samples apart, read where they lie: the bits of the stacked windows"""
    C, L = 62, 400
    seg = rows_of(B, C, L, seed=70 + B)
    win = torch.from_numpy(windows_of(seg.numpy(), 100, 50))
    fseg, fde, fpsd = fenced(seg, name="segment"), fenced_out((B, 7, C, 5)), fenced_out((B, 7, C, 5))
    eng.eeg_de_psd(fseg.t, samples=100, strides=(C * L, 50, L), batch=B, windows=7, electrodes=C, out=dict(de=fde.t, psd=fpsd.t))
    torch.cuda.synchronize()
    for f in (fseg, fde, fpsd):
        f.check()
    de, psd = fde.view.reshape(B, 7, C, 5).clone(), fpsd.view.reshape(B, 7, C, 5).clone()
    held(de, psd, win, f"7 windows B{B}")
    de2, psd2 = eng.eeg_de_psd(win.cuda())
    assert torch.equal(bits(de), bits(de2)) and torch.equal(bits(psd), bits(psd2))
    # the one 2-s window of the same segment: window stride 0
    de3, psd3 = eng.eeg_de_psd(fseg.t, samples=L, strides=(C * L, 0, L), batch=B, windows=1, electrodes=C)
    held(de3, psd3, seg[:, None], f"2-s window B{B}")
    fseg.check()


def test_source_at_odd_alignment_outputs_alone_and_scaler(eng):
    B, C, m = 2, 3, 100
    x = rows_of(B, 1, C, m, seed=5)
    de0, psd0 = eng.eeg_de_psd(x.cuda())
    flat = torch.zeros(x.numel() + 1, device="cuda")                  # one float into an allocation: 4-byte aligned, not 8
    flat[1:] = x.flatten().cuda()
    src = flat[1:]
    assert src.data_ptr() % 8 == 4 and src.is_contiguous()
    de1, psd1 = eng.eeg_de_psd(src, samples=m, strides=(C * m, 0, m), batch=B, windows=1, electrodes=C)
    assert torch.equal(bits(de1), bits(de0)) and torch.equal(bits(psd1), bits(psd0))
    # either output alone, fenced
    fin, fde = fenced(x, name="eeg"), fenced_out((B, 1, C, 5))
    got = run_fenced(lambda: eng.eeg_de_psd(fin.t, psd=False, out=dict(de=fde.t)), [fin], fde)
    assert torch.equal(bits(got.reshape(de0.shape)), bits(de0))
    fpsd = fenced_out((B, 1, C, 5))
    got = run_fenced(lambda: eng.eeg_de_psd(fin.t, de=False, out=dict(psd=fpsd.t)), [fin], fpsd)
    assert torch.equal(bits(got.reshape(psd0.shape)), bits(psd0))
    assert eng.eeg_de_psd(x.cuda(), de=False)[0] is None and eng.eeg_de_psd(x.cuda(), psd=False)[1] is None
    # the scaler: (de - mean) / scale per (electrode, band), true division in fp32 -- exactly that of the unscaled bits
    g = torch.Generator().manual_seed(9)
    mean, scale = 18 + torch.randn(C * 5, generator=g), 0.5 + torch.rand(C * 5, generator=g)
    fm, fs_ = fenced(mean, name="mean"), fenced(scale, name="scale")
    de2, psd2 = eng.eeg_de_psd(x.cuda(), scaler=(fm.t, fs_.t))
    torch.cuda.synchronize()
    fm.check(), fs_.check()
    want = (de0.cpu() - mean.reshape(1, 1, C, 5)) / scale.reshape(1, 1, C, 5)
    assert torch.equal(bits(de2.cpu()), bits(want)) and torch.equal(bits(psd2), bits(psd0))


def test_all_zero_row_is_the_stated_deviation(eng):
    """E = 0: psd 0 and de -inf (the reference raises ValueError in math.log); the rows around it are untouched by it"""
    x = rows_of(2, 1, 3, 200, seed=8)
    ref = eng.eeg_de_psd(x.cuda())
    x[1, 0, 1] = 0.0
    fin, fde, fpsd = fenced(x, name="eeg"), fenced_out((2, 1, 3, 5)), fenced_out((2, 1, 3, 5))
    eng.eeg_de_psd(fin.t, out=dict(de=fde.t, psd=fpsd.t))
    torch.cuda.synchronize()
    for f in (fin, fde, fpsd):
        f.check()
    de, psd = fde.view.reshape(2, 1, 3, 5).clone(), fpsd.view.reshape(2, 1, 3, 5).clone()
    assert torch.all(psd[1, 0, 1] == 0) and torch.all(torch.isneginf(de[1, 0, 1]))
    keep = torch.ones(2, 1, 3, dtype=torch.bool)
    keep[1, 0, 1] = False
    assert torch.isfinite(de.cpu()[keep]).all()
    assert torch.equal(bits(de.cpu()[keep]), bits(ref[0].cpu()[keep])) and torch.equal(bits(psd.cpu()[keep]), bits(ref[1].cpu()[keep]))
    mean, scale = torch.zeros(15), torch.ones(15)
    assert torch.all(torch.isneginf(eng.eeg_de_psd(x.cuda(), scaler=(mean, scale))[0][1, 0, 1]))


def test_other_sampling_rates(eng):
    x = rows_of(1, 1, 3, 198, seed=4)
    with pytest.raises(ValueError, match="sampling rate 100"):
        eng.eeg_de_psd(x.cuda(), fs=100)
    with pytest.raises(ValueError, match="sampling rate 256"):
        eng.eeg_de_psd(x.cuda(), fs=256)
    de, psd = eng.eeg_de_psd(x.cuda(), fs=198)                        # the last band ends at bin 99, the last of the half spectrum
    held(de, psd, x, "fs = 198", fs=198)


# ------------------------------------------------------------------ 3. same bits ----------------------------------------------------
def test_same_bits_alone_in_a_batch_and_in_every_compute_dtype(eng):
    C, L = 62, 400
    seg = rows_of(5, C, L, seed=21).cuda()
    kw = dict(samples=100, strides=(C * L, 50, L), windows=7, electrodes=C)
    whole = eng.eeg_de_psd(seg, batch=5, **kw)
    assert same_bits(eng.eeg_de_psd(seg, batch=5, **kw), whole)       # run to run
    for b in range(5):
        alone = eng.eeg_de_psd(seg[b:b + 1].contiguous(), batch=1, **kw)
        assert same_bits([alone[0][0], alone[1][0]], [whole[0][b], whole[1][b]]), b
    for mode in ("bf16", "fp16"):
        try:
            eng.set_compute_dtype(mode)
            assert same_bits(eng.eeg_de_psd(seg, batch=5, **kw), whole), mode
        finally:
            eng.set_compute_dtype("fp32")


# ------------------------------------------------------------------ 4. bounds and memory --------------------------------------------
def test_pool_guarded_and_steady_state(eng):
    from eeg2video_amd.engine import Engine
    C, L = 62, 400
    seg = rows_of(3, C, L, seed=33)
    kw = dict(samples=100, strides=(C * L, 50, L), batch=3, windows=7, electrodes=C)
    ref = eng.eeg_de_psd(seg.cuda(), **kw)
    torch.cuda.synchronize()
    before = eng.device_bytes()                                      # the plan's block is cached after the first call
    eng.eeg_de_psd(seg.cuda(), **kw)
    eng.eeg_de_psd(seg.cuda()[:1].contiguous(), **dict(kw, batch=1))
    eng.eeg_de_psd(seg.cuda(), samples=L, strides=(C * L, 0, L), batch=3, windows=1, electrodes=C)
    torch.cuda.synchronize()
    assert eng.device_bytes() == before
    with environment({}, GUARD_KIB):
        on = Engine(TINY_UNET, TINY_VAE, 0)
    y = guarded_run((eng, on), lambda e: list(e.eeg_de_psd(seg.cuda(), **kw)), what="eeg_de_psd")
    assert same_bits(y, list(ref))


# ------------------------------------------------------------------ 5. errors -------------------------------------------------------
def test_errors_in_order_and_nothing_enqueued(eng):
    x = torch.zeros(1, 1, 3, 100, device="cuda")
    gets = eng.pool_gets()
    for kw in (dict(de=False, psd=False), dict(fs=100), dict(fs=256), dict(scaler=(torch.zeros(3), torch.ones(3))), dict(batch=2),
               dict(strides=(300, 0, 100)), dict(samples=101, strides=(300, 0, 100), batch=1, windows=1, electrodes=3),
               dict(samples=100, strides=(300, -1, 100), batch=1, windows=1, electrodes=3),
               dict(samples=100, strides=(300, 0, 100), batch=0, windows=1, electrodes=3)):
        with pytest.raises(ValueError):
            eng.eeg_de_psd(x, **kw)
    with pytest.raises(ValueError):
        eng.eeg_de_psd(x.cpu())
    with pytest.raises(ValueError):
        eng.eeg_de_psd(x.double())
    with pytest.raises(ValueError, match="no output"):               # the missing output is reported before the bad rate
        eng.eeg_de_psd(x, de=False, psd=False, fs=100)
    assert eng.pool_gets() == gets                                   # nothing was taken from the pool: nothing was enqueued


# ------------------------------------------------------------------ 6. the mirrors --------------------------------------------------
def test_features_module(eng):
    from eeg2video_amd import features
    rows = maker().de_psd_rows(200)
    de, psd = features.DE_PSD(rows, 200, 1, engine=eng)               # the reference's call: fre = 200, time_window = 1
    assert isinstance(de, np.ndarray) and de.shape == (62, 5) and de.dtype == np.float32 and psd.shape == (62, 5)
    op = eng.eeg_de_psd(torch.from_numpy(rows).cuda().reshape(1, 1, 62, 200))
    assert np.array_equal(de.view(np.int32), op[0].cpu().numpy().reshape(62, 5).view(np.int32))
    assert np.array_equal(psd.view(np.int32), op[1].cpu().numpy().reshape(62, 5).view(np.int32))
    t_de, t_psd = features.DE_PSD(torch.from_numpy(rows), 200, 1, engine=eng)       # a tensor in: tensors on the device out
    assert t_de.is_cuda and torch.equal(bits(t_de.cpu()), bits(torch.from_numpy(de)))
    with pytest.raises(ValueError, match="row length"):
        features.DE_PSD(rows, 200, 2, engine=eng)
    # batched, over a raw segment; the scaler as sklearn holds it
    seg = rows_of(2, 62, 400, seed=12)
    mean, scale = np.full(310, 19.0), np.full(310, 2.0)
    de7, psd7 = features.de_psd(seg.cuda(), window=100, step=50, scaler=(mean, scale), engine=eng)
    raw7 = eng.eeg_de_psd(torch.from_numpy(windows_of(seg.numpy(), 100, 50)).cuda())
    assert tuple(de7.shape) == (2, 7, 62, 5) and torch.equal(bits(psd7), bits(raw7[1]))
    assert torch.equal(bits(de7), bits((raw7[0] - 19.0) / 2.0))
    one = features.de_psd(seg.cuda(), engine=eng, psd=False)
    assert tuple(one[0].shape) == (2, 1, 62, 5) and one[1] is None
    assert features.default_engine(0) is features.default_engine(0)
