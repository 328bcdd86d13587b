"""The tile schedule of the fp32 GEMM launcher, restated (pure Python: no torch, no GPU).

``plan_tiles()`` (csrc/gemm_sched.h, the one home of the rule: ``igemm()`` calls it for every GEMM launch, every GEMM kernel decodes its
result with ``tile_decode()`` of the same header) cuts the ``nbm`` row blocks of 128 rows of a launch -- the row blocks of all batch entries
together -- into tiles of two shapes: row blocks of the *wide* part into ``w1`` tiles of 128x128 followed by ``s1`` tiles of 128x64,
row blocks of the *tail* part into ``s2`` tiles of 128x64 only.  ``rb1`` is the number of wide row blocks the rule asks for:

    narrow  rb1 == 0        every row block is tail (always so below one round of 512 tiles)
    wide    rb1 == nbm      no tail
    mixed   0 < rb1 < nbm

The kernels deal the row blocks to eight XCD chunks, chunk x owning ``[x * nbm // 8, (x + 1) * nbm // 8)``; the LAST ``min(length,
tail_rb)`` row blocks of every chunk are its tail, so the seam between wide and tail tiles lies inside every chunk.  The grid is eight
times the tile count of the longest chunk; the blocks a shorter chunk does not need return at once.

``schedule()`` restates the rule for the fp32 path (128-row blocks, 512 slots, ``E2V_IGEMM_SCHED`` at its default of 1, no split-K;
``rows`` / ``slots``: the same rule for the 256-row blocks of the 16-bit modes), independently of the header -- tests/
test_gemm_sched_host.py holds the header's planner to it over a sweep of launches --,
``klass()`` names the class of a launch, ``region()`` says which tile of the schedule owns an output element of a case of ``CASES`` --
the launches tests/test_hip_igemm_schedule.py runs, chosen so that every class of the production dispatch table
(tests/golden/dispatch_sd_v1_4.json) is reached (tests/test_igemm_schedule_host.py).
"""
import re

SLOTS = 512          # resident tiles the rule sizes a round by (2 workgroups per CU)
ROWS = 128           # rows of a row block


def schedule(M, N, batch=1, geglu=False, rows=ROWS, slots=SLOTS):
    """``M`` rows per batch entry, ``N`` GEMM columns (GEGLU: both halves, 2 x the output width).  ``rows``, ``slots``: the row-block
    height and the resident tiles of a round -- 128 and 512, or 256 and 256 for the 256-row tiles of the 16-bit modes."""
    nbm_per = (M + rows - 1) // rows
    nbm = nbm_per * batch
    s2 = (N + 63) // 64
    w1 = N // 128
    rem = N - w1 * 128
    s1 = 1 if 0 < rem <= 64 else 0
    if rem > 64:
        w1 += 1                                  # 65..127 leftover columns: one more (masked) wide tile
    rb1 = nbm
    if geglu:                                    # the GEGLU epilogue pairs the two 32-column halves of a wave: wide tiles only
        w1, s1 = (N + 127) // 128, 0
    elif w1 == 0:                                # N <= 64
        rb1 = 0
    else:
        per2 = 2 * w1 + s1                       # cost of a row block in units of half a 128x128 tile (the source's per_rb, doubled)
        nrb = (nbm + 7) // 8                     # row blocks of the longest chunk
        units2 = per2 * nrb
        xslots = slots // 8
        if units2 * 8 < 2 * slots:
            rb1 = 0                              # less than one round
        else:
            full = units2 // (2 * xslots)        # whole rounds of wide tiles
            wide_rb = (full * 2 * xslots) // per2
            tail = nrb - wide_rb
            if tail > 0 and tail * per2 <= xslots:           # what is left is at most half a round: half-size tiles
                rb1 = max(0, nbm - 8 * tail)
    tail_rb = nbm if rb1 == 0 else (nbm - rb1 + 7) // 8
    chunks = tuple(((x + 1) * nbm >> 3) - (x * nbm >> 3) for x in range(8))
    return dict(nbm=nbm, nbm_per=nbm_per, rb1=rb1, w1=w1, s1=s1, s2=s2, tail_rb=tail_rb, chunks=chunks)


def chunk_tiles(s):
    """tiles each XCD chunk runs; the grid is 8 x the largest"""
    out = []
    for nrb in s["chunks"]:
        tail = min(nrb, s["tail_rb"])
        out.append((nrb - tail) * (s["w1"] + s["s1"]) + tail * s["s2"])
    return tuple(out)


def kind_of(s):
    return "narrow" if s["rb1"] == 0 else "wide" if s["rb1"] == s["nbm"] else "mixed"


def klass(M, N, batch=1, geglu=False, taps=1, cat=False, stride=1):
    """(narrow | wide | mixed, taps, batched, geglu, cat, has s1, masked wide tile, stride 2).  ``has s1`` and ``masked wide tile``
    are the launcher's ``s1 > 0`` and ``w1 * 128 > N`` whether or not a wide tile runs (the dispatch table prints them for every launch)."""
    s = schedule(M, N, batch, geglu)
    return (kind_of(s), taps, batch > 1, bool(geglu), bool(cat), s["s1"] > 0, s["w1"] * 128 > N, stride == 2)


_LINE = re.compile(r"^\d+x igemm_f32 M(\d+) N(\d+) K(\d+) t([19])(?P<flags>(?: s2| up| cat| geglu| b\d+| k16)*) rb1=(\d+) w(\d+) s(\d+) -> (\S+)")


def parse_golden(line):
    """an ``igemm_f32`` line of the dispatch table -> (launch as ``klass()`` takes it, (rb1, w1, s1) the build recorded)"""
    m = _LINE.match(line)
    assert m, line
    flags = m.group("flags").split()
    batch = [int(f[1:]) for f in flags if re.fullmatch(r"b\d+", f)]
    launch = dict(M=int(m.group(1)), N=int(m.group(2)), batch=batch[0] if batch else 1, geglu="geglu" in flags, taps=int(m.group(4)),
                  cat="cat" in flags, stride=2 if "s2" in flags else 1)
    return launch, (int(m.group(6)), int(m.group(7)), int(m.group(8)))


# ------------------------------------------------------------------ the cases -------------------------------------------------------
# ``claim``: the class a case was chosen for -- (schedule, has s1, masked wide tile) --, ``more``: what else the table it came from says
# about it, as keys of schedule().  tests/test_igemm_schedule_host.py holds the restatement to both.
def _linear(M, N, K, epilogue, claim, c1=0, **more):
    name = f"linear {M}x{K}x{N} {epilogue}" if not c1 else f"linear_cat {M}x({K - c1}+{c1})x{N} {epilogue}"
    return dict(name=name, kind="linear", M=M, N=N, K=K, c1=c1, epilogue=epilogue, claim=claim, more=more)


def _conv(n, h, w, cin, cout, claim, *, c1=0, stride=1, up=1, rowbias=False, resid=False, algo="direct", **more):
    """``n`` images of ``h x w`` source pixels (``up``: nearest resize by that factor in front of the conv); ``cin`` = c0 + c1"""
    name = f"{algo} conv {n}x{h}x{w} {cin - c1}{'+' + str(c1) if c1 else ''}->{cout}" + (" s2" if stride == 2 else "") + \
           (f" up{up}" if up > 1 else "") + (" rowbias" if rowbias else "") + (" resid" if resid else "")
    return dict(name=name, kind="conv", algo=algo, n=n, h=h, w=w, cin=cin, c1=c1, cout=cout, stride=stride, up=up, rowbias=rowbias,
                resid=resid, claim=claim, more=more)


def conv_out_hw(case):
    hi, wi = case["h"] * case["up"], case["w"] * case["up"]
    return ((hi - 1) // 2 + 1, (wi - 1) // 2 + 1) if case["stride"] == 2 else (hi, wi)          # 3x3, pad 1


def wino_m(case):
    return {"winograd": 2, "winograd4": 4}.get(case.get("algo"), 0)


def wino_tiles_hw(case):
    m = wino_m(case)
    ho, wo = conv_out_hw(case)
    return (ho + m - 1) // m, (wo + m - 1) // m


def launch_of(case, images=None):
    """the GEMM launch of a case as ``klass()`` takes it; ``images``: of that many images of a conv only"""
    if case["kind"] == "linear":
        return dict(M=case["M"], N=case["N"], cat=case["c1"] > 0)
    if case["kind"] == "geglu":
        return dict(M=case["M"], N=8 * case["c"], geglu=True)
    n = case["n"] if images is None else images
    ho, wo = conv_out_hw(case)
    m = wino_m(case)
    if m:
        th, tw = wino_tiles_hw(case)
        return dict(M=n * th * tw, N=case["cout"], batch=(m + 2) ** 2, cat=case["c1"] > 0)
    return dict(M=n * ho * wo, N=case["cout"], taps=9, cat=case["c1"] > 0, stride=case["stride"])


def sched_args(launch):
    return {k: launch[k] for k in ("M", "N", "batch", "geglu") if k in launch}


def schedule_of(case):
    return schedule(**sched_args(launch_of(case)))


SLICE_ROWS = 1000        # linears are re-run in row slices of this many rows, convs one image at a time


def slice_launches(case):
    """The launches of the sliced re-run of a case.  Each must be narrow, the schedule the rest of the suite covers; a GEGLU launch
    never is (wide tiles only), its slices have at most 8 row blocks -- one per XCD chunk, as in the suite's other GEGLU cases."""
    if case["kind"] in ("linear", "geglu"):
        full = launch_of(case)
        sizes = {min(SLICE_ROWS, case["M"] - lo) for lo in range(0, case["M"], SLICE_ROWS)}
        return [dict(full, M=m) for m in sorted(sizes)]
    return [launch_of(case, images=1)]


def _smallest_images(h, w, cin, cout, algo, want, **kw):
    """the smallest image count at which the conv's launch is of class ``want`` = (schedule, has s1)"""
    for n in range(1, 200):
        k = klass(**launch_of(_conv(n, h, w, cin, cout, None, algo=algo, **kw)))
        if (k[0], k[5]) == want:
            return n
    raise AssertionError("no image count up to 200 reaches the class")


N_DIRECT_WIDE = _smallest_images(36, 64, 4, 320, "direct", ("wide", True))                  # 17
N_DIRECT_MIXED = _smallest_images(36, 64, 4, 320, "direct", ("mixed", True))                # 12
N_DIRECT_S2_MIXED = _smallest_images(36, 64, 4, 320, "direct", ("mixed", True), stride=2)   # 48
N_WINO4_WIDE = _smallest_images(35, 46, 32, 320, "winograd4", ("wide", True))               # 10
N_WINO4_WIDE_640 = _smallest_images(34, 39, 32, 640, "winograd4", ("wide", False))

MIXED, WIDE, NARROW = "mixed", "wide", "narrow"
CASES = [_linear(6500, 1280, k, e, (MIXED, False, False), nbm=51, rb1=43, chunks=(6, 6, 7, 6, 6, 7, 6, 7))
         for e in ("none", "bias", "bias_residual") for k in (16, 40)] + [
    _linear(6500, 1224, 40, "bias_residual", (MIXED, False, True), w1=10, s1=0, s2=20),         # ragged last narrow tile in the tail
    _linear(6500, 1160, 40, "bias_residual", (MIXED, True, False), w1=9, s1=1),
    _linear(26001, 320, 16, "bias_residual", (MIXED, True, False), nbm=204, rb1=196, w1=2, s1=1),
    _linear(33100, 200, 16, "none", (MIXED, False, True), w1=2, s1=0),                          # w1 2, of which one masked
    _linear(9500, 1224, 16, "bias_residual", (WIDE, False, True), nbm=75, chunks=(9, 9, 10, 9, 9, 10, 9, 10)),
    _linear(38200, 320, 16, "bias", (WIDE, True, False), w1=2, s1=1),
    _linear(6500, 1280, 20, "bias_residual", (MIXED, False, False), c1=8),                      # the seam inside the first k stage
    _linear(9500, 1280, 20, "bias_residual", (WIDE, False, False), c1=8),
    dict(name="geglu 1300x32", kind="geglu", M=1300, c=32, claim=(WIDE, False, False), more=dict(nbm=11)),
    _conv(3, 36, 60, 4, 1280, (MIXED, False, False), rowbias=True, resid=True),
    _conv(12, 36, 64, 4, 1280, (MIXED, False, False), stride=2, nbm=54),
    _conv(2, 27, 40, 4, 1280, (MIXED, False, False), up=2, nbm=68, tail_rb=3),
    _conv(3, 36, 60, 64, 1280, (MIXED, False, False), c1=32, resid=True),
    _conv(N_DIRECT_WIDE, 36, 64, 4, 320, (WIDE, True, False)),
    _conv(N_DIRECT_MIXED, 36, 64, 4, 320, (MIXED, True, False)),
    _conv(6, 35, 46, 32, 320, (MIXED, True, False), rowbias=True, resid=True, algo="winograd4", nbm_per=6, w1=2, s1=1),
    _conv(3, 34, 39, 32, 640, (MIXED, False, False), algo="winograd4", nbm_per=3, chunks=(13, 14, 13, 14, 13, 14, 13, 14)),
    _conv(3, 36, 58, 32, 320, (MIXED, True, False), algo="winograd", nbm_per=13),
    _conv(N_WINO4_WIDE, 35, 46, 32, 320, (WIDE, True, False), algo="winograd4"),
    # classes of the production table the rows above miss
    _linear(26001, 320, 20, "bias_residual", (MIXED, True, False), c1=8),
    _linear(38200, 320, 20, "bias", (WIDE, True, False), c1=8),
    _linear(9500, 1280, 16, "bias", (WIDE, False, False)),
    _conv(N_DIRECT_S2_MIXED, 36, 64, 4, 320, (MIXED, True, False), stride=2),
    _conv(N_WINO4_WIDE_640, 34, 39, 32, 640, (WIDE, False, False), algo="winograd4"),
    # ... and its narrow ones, at small shapes: the schedule the other op tests run, here with the same checks
    _linear(300, 256, 16, "bias_residual", (NARROW, False, False)),
    _linear(300, 320, 16, "bias", (NARROW, True, False)),
    _linear(300, 256, 20, "bias_residual", (NARROW, False, False), c1=8),
    _conv(2, 9, 12, 4, 128, (NARROW, False, False)),
    _conv(2, 9, 12, 4, 128, (NARROW, False, False), stride=2),
    _conv(2, 9, 12, 4, 320, (NARROW, True, False)),
    _conv(2, 9, 12, 4, 320, (NARROW, True, False), stride=2),
    _conv(2, 9, 10, 32, 128, (NARROW, False, False), algo="winograd4"),
]


def case_named(name):
    for c in CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)


# ------------------------------------------------------------------ who owns an output element --------------------------------------
def owner(s, rbg, gcol):
    """the tile of schedule ``s`` that computes GEMM column ``gcol`` of (global) row block ``rbg``"""
    nbm = s["nbm"]
    x = next(x for x in range(8) if (x * nbm >> 3) <= rbg < ((x + 1) * nbm >> 3))
    lo, nrb = x * nbm >> 3, s["chunks"][x]
    tail = min(nrb, s["tail_rb"])
    per1 = s["w1"] + s["s1"]
    r = rbg - lo
    if r < nrb - tail:
        if gcol < s["w1"] * 128:
            reg, j, shape, col0 = "wide", gcol // 128, "128x128", gcol // 128 * 128
        else:
            j = s["w1"] + (gcol - s["w1"] * 128) // 64
            reg, shape, col0 = "s1", "128x64", s["w1"] * 128 + (j - s["w1"]) * 64
        loc = r * per1 + j
    else:
        j = gcol // 64
        reg, shape, col0 = "tail", "128x64", j * 64
        loc = (nrb - tail) * per1 + (r - (nrb - tail)) * s["s2"] + j
    return dict(row_block=rbg, chunk=x, chunk_row=r, region=reg, tile=j, shape=shape, col0=col0, block=loc * 8 + x)


def region(case, row, col):
    """Which tile(s) of the case's launch own output element ``(row, col)`` -- row block, column tile and its shape, region
    (wide / s1 / tail), XCD chunk and workgroup -- as text.  A Winograd output pixel is owned by one tile in each of the 16 / 36 batch
    entries; the regions they fall in are all listed."""
    s = schedule_of(case)
    fmt = lambda o: (f"row block {o['row_block']} (no. {o['chunk_row']} of XCD chunk {o['chunk']}), {o['region']} region, column tile "
                     f"{o['tile']} ({o['shape']} at column {o['col0']}), workgroup {o['block']}")
    head = f"{kind_of(s)} rb1={s['rb1']} w{s['w1']} s{s['s1']} s2={s['s2']} tail_rb={s['tail_rb']} chunks {'/'.join(map(str, s['chunks']))}: "
    if case["kind"] == "geglu":                                         # h and gate of output column c: the two halves of one 64-wide group
        return head + fmt(owner(s, row // ROWS, col // 32 * 64 + col % 32))
    m = wino_m(case) if case["kind"] == "conv" else 0
    if not m:
        return head + fmt(owner(s, row // ROWS, col))
    ho, wo = conv_out_hw(case)
    th, tw = wino_tiles_hw(case)
    img, pix = divmod(row, ho * wo)
    t = (img * th + pix // wo // m) * tw + pix % wo // m
    owners = [owner(s, z * s["nbm_per"] + t // ROWS, col) for z in range((m + 2) ** 2)]
    regions = sorted({o["region"] for o in owners})
    return head + f"Winograd tile {t} (row block {t // ROWS} of each of the {len(owners)} batch entries; regions {', '.join(regions)}); entry 0: " + \
        fmt(owners[0]) + f"; entry {len(owners) - 1}: " + fmt(owners[-1])
