"""CPU: the host-side logic of bench.py -- the self-launch of an N-rank job (the parent never touches the GPU and never
re-execs: it starts children), the CPU-share detection of the CPU baseline."""
import importlib.util
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_importing_bench_does_not_import_torch_cuda_state(bench):
    """The parent of a self-launch must be able to decide and spawn before anything initialises the GPU: the module
    imports no torch at top level."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    head = src.split("def main()")[0]
    assert "\nimport torch" not in head and "\nfrom torch" not in head


def test_self_launch_command(bench, monkeypatch):
    seen = {}

    class R:
        returncode = 7

    def fake_run(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return R()

    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    assert bench.main() == 7                                   # the children's exit code is passed on
    cmd = seen["cmd"]
    assert cmd[0] == sys.executable and cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert 1024 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    k = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[k + 1:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_rank_count_mismatch_is_refused(bench, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4"])
    assert bench.main() == 2


def test_host_cores_is_capped_by_affinity(bench):
    hc = bench.host_cores()
    assert 1 <= hc["cores"] <= hc["affinity"] <= (hc["os_cpu_count"] or 10**6)
    assert isinstance(hc["cpu_model"], str)


def test_gather_options_and_budget_guard_parse(bench):
    a = bench.parse_args(["--gpus", "8", "--dtype", "bf16", "--batch", "32", "--gather", "uint8", "--gather-impl", "cabi"])
    assert (a.gpus, a.dtype, a.batch, a.gather, a.gather_impl) == (8, "bf16", 32, "uint8", "cabi")
    d = bench.parse_args([])
    assert d.gather == "fp32" and d.gather_impl == "torch" and not d.no_configs2 and 300 < d.configs2_budget_s < 600
    assert 0 <= bench.process_age_s() < 3600


def test_committed_bench_lines_keep_the_contract_and_quote_the_committed_pmc_traffic():
    """profiles/r05_bench_*.json are the lines `bench.py` printed on the GPU box: the driver's contract keys, the `roofline` and
    `cpu_baseline` objects, the `configs2` leg in the default line (4 timed passes) -- and `roofline.traffic` must be the figure of
    profiles/pmc_dominant_kernel.json for that batch / dtype (the PMC passes and the bench lines are regenerated together)."""
    import json
    prof = os.path.join(ROOT, "profiles")
    pmc = json.load(open(os.path.join(prof, "pmc_dominant_kernel.json")))
    d = json.load(open(os.path.join(prof, "r05_bench_default.json")))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"] and d["unit"] == "clips/s" and d["n_gpus"] == 1 and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["kernel"] == "igemm_f32" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["traffic"] == pmc["igemm_f32"]["hbm_bytes_per_launch"] and pmc["igemm_f32"]["batch"] == 8
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] >= 1 and d["cpu_baseline"]["value"] > 0
    assert d["parity"]["frames_max_abs"] < d["parity"]["tolerance_frames_max_abs"]
    c2 = d["configs2"]
    assert c2["dtype"] == "bf16" and c2["value"] > 0 and c2["steps"] == 4 and c2["roofline"]["kernel"] == "igemm_bf16"
    assert c2["roofline"]["traffic"] == pmc["igemm_bf16"]["hbm_bytes_per_launch"] and pmc["igemm_bf16"]["batch"] == 32
    b = json.load(open(os.path.join(prof, "r05_bench_bf16_b32.json")))
    assert b["dtype"] == "bf16" and b["roofline"]["traffic"] == pmc["igemm_bf16"]["hbm_bytes_per_launch"]
    h = json.load(open(os.path.join(prof, "r05_bench_fp16_b32.json")))     # the fp16 mode's line: the same contract, its own class and tolerance
    assert h["dtype"] == "f16" and h["roofline"]["kernel"] == "igemm_fp16" and h["roofline"]["peak"] == b["roofline"]["peak"]
    assert h["roofline"]["traffic"] == pmc["igemm_fp16"]["hbm_bytes_per_launch"] and pmc["igemm_fp16"]["dtype"] == "fp16"
    assert h["parity"]["frames_max_abs"] < h["parity"]["tolerance_frames_max_abs"] <= 0.25 * b["parity"]["tolerance_frames_max_abs"]
    assert 8.0 * h["parity"]["frames_max_abs"] < 1.2 * b["parity"]["frames_max_abs"]      # an eighth of the bf16 distance (three more mantissa bits)
    # README / DESIGN quote the 16-bit parity figures of THESE committed lines (they move with every change of a rounding)
    for line in (b, h):
        quoted = f"{line['parity']['frames_max_abs']:.1e}".replace("e-0", "e-")
        for doc in ("README.md", "DESIGN.md"):
            assert quoted in open(os.path.join(ROOT, doc)).read(), (doc, quoted)
    wp = b["roofline"]["whole_path"]
    assert abs(wp["achieved_tflops"] - b["value"] * wp["algorithmic_tflop_per_clip"]) < 1e-6 and abs(wp["frac"] - wp["achieved_tflops"] / wp["peak"]) < 1e-9


class _StubEngine:
    """Stands where the HIP engine stands in rank_body (one rank, CPU): clip k's frames are a function of its latent."""
    device = "cpu"

    def __init__(self):
        self.calls, self.profiled = [], 0

    def generate(self, lat, cond, unc, steps, guidance, eta, decode=True, return_latents=False):
        import torch
        self.calls.append(steps)
        return torch.stack([torch.full((3, 2, 4, 6), float(lat[k].flatten()[0])) + torch.arange(144.).reshape(3, 2, 4, 6) / 144
                            for k in range(lat.shape[0])])

    def frames_to_uint8(self, f):
        import torch
        return (f * 255).to(torch.uint8)

    def profile_begin(self):
        self.profiled += 1

    def profile_end(self):
        return {"igemm_f32": {"ms": 1.0, "launches": 10, "flops": 1e9, "bytes": 1e6}}

    def device_bytes(self):
        return 0


def _one_rank(bench, argv):
    args = bench.parse_args(["--ddim-steps", "3"] + argv)
    eng = _StubEngine()
    r = bench.rank_body(args, 0, 1, eng, use_dist=False, B=2, frame_shape=(3, 2, 4, 6), latent_shape=(4, 2, 4, 6), cond_shape=(5, 8),
                        sync=lambda: None, pin=False, configs2=lambda *a: {"value": 1.0})
    return eng, r


def test_plain_run_does_only_the_headline(bench):
    """Without --full: the warm-up and timed steps run and nothing else (no instrumented pass, no exchange / D2H timing pass, no
    configs[2] leg, no CPU baseline); --steps sets the number of timed steps and ms_per_step is their mean."""
    eng, r = _one_rank(bench, ["--steps", "5", "--warmup", "2"])
    d = r["result"]
    assert eng.calls == [3] * 7 and eng.profiled == 0
    assert d["steps"] == 5 and d["warmup"] == 2 and d["ms_per_step"] > 0
    assert abs(d["value"] - 2 * 5 / (d["ms_per_step"] * 5 / 1e3)) < 1e-6 * d["value"]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["roofline"] is None and d["configs2"] is None and d["cpu_baseline"] is None and d["d2h_ms"] is None
    # --full brings them back: the instrumented last warm-up, the one-step exchange / D2H pass, the configs[2] leg
    eng, r = _one_rank(bench, ["--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"])
    d = r["result"]
    assert eng.calls == [3, 3, 3, 1] and eng.profiled == 1
    assert d["roofline"]["kernel"] == "igemm_f32" and d["configs2"] == {"value": 1.0} and d["d2h_ms"] is not None


def test_steps_must_be_positive(bench):
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_outputs_writes_the_last_timed_step(bench, tmp_path):
    """--dump-outputs DIR: float32 .npy of the frames the last timed step delivered to the host, the same from run to run."""
    import numpy as np
    out1, out2 = tmp_path / "a", tmp_path / "b"
    _, r = _one_rank(bench, ["--steps", "2", "--warmup", "1", "--dump-outputs", str(out1)])
    _one_rank(bench, ["--steps", "2", "--warmup", "1", "--dump-outputs", str(out2)])
    host = r["host_frames"].numpy()
    names = sorted(os.listdir(out1))
    assert names == ["frames_clip0.npy", "frames_sample.npy"] and sorted(os.listdir(out2)) == names
    c0, s = np.load(out1 / "frames_clip0.npy"), np.load(out1 / "frames_sample.npy")
    assert c0.dtype == np.float32 and s.dtype == np.float32
    assert np.array_equal(c0, host[0]) and np.array_equal(s, host.reshape(-1))       # small buffer: the sample is all of it
    for n in names:
        assert np.array_equal(np.load(out1 / n), np.load(out2 / n))


def test_dump_sample_of_a_large_buffer_is_fixed_and_bounded(bench, tmp_path):
    import numpy as np
    frames = np.arange(3 * (bench.DUMP_SAMPLE + 7), dtype=np.float32).reshape(3, -1)
    shapes = bench.dump_outputs(str(tmp_path / "a"), frames)
    bench.dump_outputs(str(tmp_path / "b"), frames)
    assert shapes == {"frames_clip0": [bench.DUMP_SAMPLE + 7], "frames_sample": [bench.DUMP_SAMPLE]}
    s = np.load(tmp_path / "a" / "frames_sample.npy")
    assert np.array_equal(s, np.load(tmp_path / "b" / "frames_sample.npy"))
    assert np.all(np.diff(s) >= 0) and s[-1] - s[0] > 2 * bench.DUMP_SAMPLE     # index order, spread over the whole buffer
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")) < 64 * 2**20
