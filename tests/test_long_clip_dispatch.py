"""CPU: long clips (video_length > 8) take temporal_attn_long_kernel in every transformer block, and F <= 8 keeps its kernels.

`e2v_op_describe_dispatch` walks e2v_generate as a dry run on a host-only context, so the whole UNet of a long clip is described without
a GPU: before the long-clip kernel existed the walk stopped at the first transformer block with E2V_EINVAL."""
import re

import pytest

LONG = "-> temporal_attn_long_kernel"


def _temporal(lines):
    """(launch count, record) of every temporal attention record of a description."""
    out = []
    for line in lines:
        m = re.match(r"(\d+)x temporal_attn\b", line)
        if m:
            out.append((int(m.group(1)), line))
    return out


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("frames", [9, 16, 24, 40])
def test_long_clip_takes_the_long_kernel_in_every_block(mode, frames):
    from eeg2video_amd.engine import describe_dispatch
    batch = 2
    ref = _temporal(describe_dispatch(mode, batch, frames=6))
    got = _temporal(describe_dispatch(mode, batch, frames=frames))
    assert got, "no temporal attention record"
    for _, line in got:
        assert line.endswith(LONG), line
        assert f" F{frames} " in line, line
    assert sum(c for c, _ in got) == sum(c for c, _ in ref)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("frames,kernel", [(6, "temporal_attn_wave_kernel"), (7, "temporal_attn_lds_kernel"), (8, "temporal_attn_lds_kernel")])
def test_short_clips_keep_their_kernels(mode, frames, kernel):
    from eeg2video_amd.engine import describe_dispatch
    got = _temporal(describe_dispatch(mode, 2, frames=frames))
    assert got
    for _, line in got:
        assert line.endswith("-> " + kernel), line
