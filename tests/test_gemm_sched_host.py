"""CPU: the tile schedule of the GEMM kernels (eeg2video_amd/csrc/gemm_sched.h: chunk range, tile decode, grid helpers, planner) on its
own.  tests/gemm_sched_driver.cpp -- a stand-alone program that includes only that header -- is built with the host compiler under
AddressSanitizer and UBSan and run directly: over M = 1 .. 70 000 at row-block boundaries +-1, eight widths, three batch counts, GEGLU on
and off and both (rows, slots) pairs it decodes the whole grid of every launch and fails unless the tiles cover the launch exactly once,
the invalid blocks lie only past a chunk's end and the grid helper equals 8 x the longest chunk.  The plans it prints are compared, launch by
launch, with the independent restatement of the planner in tests/igemm_schedule.py."""
import os
import re
import shutil
import subprocess

import pytest

import igemm_schedule as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eeg2video_amd", "csrc")
CXX = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("c++"), shutil.which("g++")) if c and os.path.isfile(c)), None)

_PLAN = re.compile(r"^plan M(\d+) N(\d+) b(\d+) g([01]) rows(\d+) slots(\d+): rb1=(\d+) w1=(\d+) s1=(\d+) s2=(\d+) nbm=(\d+) nbm_per=(\d+) "
                   r"tail_rb=(\d+) grid=(\d+) real=(\d+)$")


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_sched") / "gemm_sched_driver")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, os.path.join(ROOT, "tests", "gemm_sched_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r.stdout


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_decode_covers_every_launch_once(driver_output):
    m = re.search(r"^gemm_sched_driver: ok, (\d+) schedules checked$", driver_output, re.M)
    assert m and int(m.group(1)) > 5000, driver_output[-300:]


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_planner_matches_the_restatement(driver_output):
    plans = [m for m in map(_PLAN.match, driver_output.splitlines()) if m]
    assert len(plans) > 5000
    kinds, seen = set(), set()
    for m in plans:
        M, N, batch, geglu, rows, slots, *got = map(int, m.groups())
        s = sc.schedule(M, N, batch, bool(geglu), rows=rows, slots=slots)
        tiles = sc.chunk_tiles(s)
        want = [s["rb1"], s["w1"], s["s1"], s["s2"], s["nbm"], s["nbm_per"], s["tail_rb"], 8 * max(tiles), sum(tiles)]
        assert got == want, f"M{M} N{N} b{batch} geglu={geglu} rows={rows} slots={slots}: header {got}, restatement {want}"
        kinds.add((rows, sc.kind_of(s), s["s1"] > 0))
        seen.add((rows, N, batch, geglu))
    # the sweep is the one the header's docstring promises, and reaches every class with and without an s1 tile at both heights
    assert seen == {(r, n, b, g) for r in (128, 256) for n in (40, 64, 72, 128, 192, 320, 1024, 2560) for b in (1, 16, 36) for g in (0, 1)}
    assert kinds == {(r, k, s1) for r in (128, 256) for k in ("narrow", "wide", "mixed") for s1 in (False, True)}
