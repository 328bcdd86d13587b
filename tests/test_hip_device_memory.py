"""GPU: who owns the library's device memory, seen from outside.  Every block the library allocates for itself -- workspace-pool blocks,
weight layouts, the GroupNorm workspaces, the timestep buffer, uploaded tensors -- is one owning block type (csrc/runtime.h: DevBlock);
these tests hold what a caller can observe of that: ``e2v_device_bytes`` returns to the same value when a part is finalized again, the
grow-only buffers grow once and are reused, and a context can be torn down and another built in the same process.  Guarded
(``E2V_POOL_GUARD`` = 64) and unguarded, results compared bit for bit.
"""
import gc

import pytest
import torch

from eeg2video_amd.weights import TINY_UNET, counter_normal
from test_hip_bounds import GUARD_KIB, U0, V0, _t, build_pipe, environment, same_bits

pytestmark = pytest.mark.gpu

D = TINY_UNET.cross_attention_dim
TOKENS = 5


def unet_inputs(n, seed=0):
    x = _t(counter_normal(50 + seed, "x", (n, 4, 2, 8, 8))).cuda()
    cond = _t(counter_normal(60 + seed, "c", (n, TOKENS, D))).cuda()
    return x, cond


def clean_report(eng, what):
    checked, violations, text = eng.pool_guard_report()
    assert violations == 0, f"{what}: {text}"
    return checked


# ------------------------------------------------------------------ 1. re-finalize returns the footprint ----------------------------
@pytest.mark.parametrize("guard", [0, GUARD_KIB])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_refinalize_returns_the_footprint(mode, guard):
    """Upload every UNet and VAE key again and finalize both parts, twice: the blocks of the replaced parts (eager copies and the layouts
    built on first use) are returned, the same ones are built again, and nothing else moved -- ``device_bytes`` and the results are
    those of the first round."""
    x, cond = unet_inputs(2)
    z = _t(counter_normal(70, "z", (2, 4, 8, 8))).cuda()
    with environment({}, guard):
        pipe = build_pipe()
        eng = pipe.unet.engine
        eng.set_compute_dtype(mode)
        if guard:
            clean_report(eng, "build")

        def run():
            y = eng.unet_forward(x, [301], cond), pipe.vae.decode(z).sample.float()
            torch.cuda.synchronize()
            return y

        first, held = run(), eng.device_bytes()
        checked = 0
        for again in (1, 2):
            pipe.unet.load_state_dict(U0)
            pipe.vae.load_state_dict(V0)
            y = run()
            print(f"{mode} guard {guard}: device_bytes {held} after the first round, {eng.device_bytes()} after re-finalize {again}")
            assert eng.device_bytes() == held
            assert same_bits(y, first), f"results differ after re-finalize {again}"
            if guard:
                checked += clean_report(eng, f"re-finalize {again}")
        assert not any(torch.isnan(t).any() for t in first)
        assert checked > 0 or not guard


# ------------------------------------------------------------------ 2. grow-only buffers ---------------------------------------------
GROW_CALLS = [(1, [301]), (3, [301, 517, 42]), (1, [301])]       # N and its timesteps: the buffers grow at the second call only
_fresh = {}


def grow_call(eng, n, ts):
    x, cond = unet_inputs(n, seed=n)
    y = eng.unet_forward(x, ts, cond)
    torch.cuda.synchronize()
    return y


def fresh_result(mode, n, ts):
    """the call on an engine that has run nothing else (unguarded: tests/test_hip_bounds.py holds guarded == unguarded)"""
    key = (mode, n, tuple(ts))
    if key not in _fresh:
        with environment({}, 0):
            eng = build_pipe().unet.engine
            eng.set_compute_dtype(mode)
            _fresh[key] = grow_call(eng, n, ts)
    return _fresh[key]


@pytest.mark.parametrize("guard", [0, GUARD_KIB])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_grow_only_buffers(mode, guard):
    """N = 1, N = 3 with three distinct timesteps, N = 1 on one engine: the GroupNorm workspaces and the timestep buffer are replaced by
    larger ones at the second call (the stream still holds work that reads the old ones) and serve the third as they are."""
    refs = [fresh_result(mode, n, ts) for n, ts in GROW_CALLS]
    with environment({}, guard):
        pipe = build_pipe()
        eng = pipe.unet.engine
        eng.set_compute_dtype(mode)
        held = []
        for (n, ts), ref in zip(GROW_CALLS, refs):
            y = grow_call(eng, n, ts)
            held.append(eng.device_bytes())
            assert not torch.isnan(y).any()
            assert same_bits(y, ref), f"N = {n}: differs from the call on a fresh engine"
        print(f"{mode} guard {guard}: device_bytes after each call {held}")
        assert held[2] == held[1]
        if guard:
            assert clean_report(eng, "grow-only buffers") > 0


# ------------------------------------------------------------------ 3. teardown --------------------------------------------------------
def test_teardown_and_rebuild_guarded():
    """Guarded bf16: a 2-step generate fills the step caches (pool blocks the context keeps); dropping the engine releases them while the
    pool is closing, then every other block.  A second engine in the same process starts clean and computes the same."""
    lat = _t(counter_normal(1, "lat", (1, 4, 3, 8, 12))).cuda()
    cond, unc = _t(counter_normal(2, "cond", (1, 7, D))).cuda(), _t(counter_normal(3, "unc", (1, 7, D))).cuda()
    with environment({}, GUARD_KIB):
        videos = []
        for which in ("first", "second"):
            pipe = build_pipe()
            eng = pipe.unet.engine
            eng.set_compute_dtype("bf16")
            assert clean_report(eng, f"{which} engine, after build") > 0
            videos.append(eng.generate(lat, cond, unc, 2, 12.5, 0.0))
            torch.cuda.synchronize()
            clean_report(eng, f"{which} engine, after generate")
            del pipe, eng
            gc.collect()
        assert not torch.isnan(videos[0]).any() and same_bits(videos[0], videos[1])
