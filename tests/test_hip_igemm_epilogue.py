"""The fp32 GEMM epilogue (csrc/igemm_epi.h: igemm_epilogue) at the shapes where its batched, masked form can go wrong.

The epilogue requests the residual and time-embedding quads of a 32-row block in one batch of buffer loads and writes through buffer
stores; rows >= M, columns >= N and absent operands are out-of-window offsets instead of branches.  So the cases are ragged against
every unit it works in -- the 32-row block, the 128-row tile, the 4- and 8-row access groups, the quad, the 64- and 128-wide tiles, one
and two k-stages -- and every operand sits in a poisoned, fenced buffer (tests/test_hip_bounds.py): a masked lane that read or wrote a
word outside a tensor would change the fence or leave a NaN.  References are fp64 host products; tolerances are those of
tests/test_hip_ops.py::test_linear / test_linear_geglu (Winograd convs: the bound their own tests use).

``cases()`` lists every case as (name, run) for tools/igemm_epilogue_bits.py, which compares two builds of the library bit for bit.
"""
import pytest
import torch
import torch.nn.functional as F

from test_hip_bounds import BOUNDS, close, fenced, fenced_out, from_cl, make_engine, rnd, run_fenced, to_cl

pytestmark = pytest.mark.gpu

MS = (1, 31, 130, 257)            # ragged against the 32-row block, the 128-row tile and the 4- / 8-row access groups
NS = (4, 64, 132, 320)            # one quad; a lone 64-wide tile; a ragged last tile (N % 4 == 0); the 2 x 128 + 64 mix
KS = (16, 40)                     # one 16-k stage; a ragged second (32-k tile) / third (16-k tile) stage
EPILOGUES = ("none", "bias", "bias_residual")
GEGLU = [(m, c) for m in (31, 130) for c in (32, 64)]
# (algo, cin, cout, images, h, w): h * w rows per sample.  40: a 32-row block spans two samples; 12: up to four (the per-row form)
CONVS = [("direct", 32, 64, 4, 5, 8), ("direct", 32, 132, 4, 5, 8), ("direct", 32, 64, 6, 3, 4),
         ("winograd", 32, 64, 4, 5, 8), ("winograd4", 32, 64, 4, 5, 8)]


@pytest.fixture(scope="module")
def eng():
    return make_engine()


def linear_case(eng, m, k, n, epilogue):
    x, w = rnd(m, k, seed=20), rnd(n, k, seed=21, scale=0.05)
    b = rnd(n, seed=22) if epilogue != "none" else None
    r = rnd(m, n, seed=23) if epilogue == "bias_residual" else None
    ref = F.linear(x.double(), w.double(), b.double() if b is not None else None) + (r.double() if r is not None else 0)
    fx, fw, out = fenced(x, ld=k + 4, name="x"), fenced(w, name="w"), fenced_out((m, n))
    fb = fenced(b, name="bias") if b is not None else None
    fr = fenced(r, name="resid") if r is not None else None
    y = run_fenced(lambda: eng.op_linear(fx.t, fw.t, fb.t if fb else None, fr.t if fr else None, out=out.t), [fx, fw, fb, fr], out)
    return y, ref


def geglu_case(eng, m, c):
    x, w, b = rnd(m, c, seed=24), rnd(8 * c, c, seed=25, scale=0.1), rnd(8 * c, seed=26)
    h, g = F.linear(x.double(), w.double(), b.double()).chunk(2, dim=-1)
    fx, fw, fb, out = fenced(x, ld=c + 4, name="x"), fenced(w, name="w"), fenced(b, name="bias"), fenced_out((m, 4 * c))
    y = run_fenced(lambda: eng.op_linear(fx.t, fw.t, fb.t, geglu=True, out=out.t), [fx, fw, fb], out)
    return y, h * F.gelu(g)


def conv_case(eng, algo, cin, cout, n, h, w):
    """3x3 conv with bias, one time-embedding row per image and a residual; returns channels-last output and reference"""
    x, wt, b = rnd(n, cin, h, w, seed=1), rnd(cout, cin, 3, 3, seed=2, scale=0.1), rnd(cout, seed=3)
    temb, res = rnd(n, cout, seed=4), rnd(n, cout, h, w, seed=5)
    ref = F.conv2d(x.double(), wt.double(), b.double(), padding=1) + temb.double()[:, :, None, None] + res.double()
    fx, fw, fb = fenced(to_cl(x), name="x"), fenced(wt, name="w"), fenced(b, name="bias")
    ft, fr, out = fenced(temb, name="rowbias"), fenced(to_cl(res), name="resid"), fenced_out((n * h * w, cout))
    eng.set_conv_algo(algo)
    try:
        y = run_fenced(lambda: eng.op_conv3x3(fx.t, fw.t, fb.t, n_img=n, Hs=h, Ws=w, rowbias=ft.t, rows_per_sample=h * w, resid=fr.t,
                                              out=out.t), [fx, fw, fb, ft, fr], out)
    finally:
        eng.set_conv_algo("auto")
    return y, to_cl(ref)


def cases():
    for epilogue in EPILOGUES:
        for m in MS:
            for n in NS:
                for k in KS:
                    yield f"linear {m}x{k}x{n} {epilogue}", (lambda e, a=(m, k, n, epilogue): linear_case(e, *a))
    for m, c in GEGLU:
        yield f"geglu {m}x{c}", (lambda e, a=(m, c): geglu_case(e, *a))
    for cv in CONVS:
        yield "conv " + " ".join(map(str, cv)), (lambda e, a=cv: conv_case(e, *a))


@pytest.mark.parametrize("epilogue", EPILOGUES)
@pytest.mark.parametrize("m", MS)
def test_linear_epilogue_fenced(eng, m, epilogue):
    for n in NS:
        for k in KS:
            y, ref = linear_case(eng, m, k, n, epilogue)
            close(y, ref, what=f"linear {m}x{k}x{n} {epilogue}")


@pytest.mark.parametrize("m,c", GEGLU)
def test_geglu_epilogue_fenced(eng, m, c):
    y, ref = geglu_case(eng, m, c)
    close(y, ref, what=f"geglu {m}x{c}")


@pytest.mark.parametrize("algo,cin,cout,n,h,w", CONVS)
def test_conv_rowbias_residual_epilogue_fenced(eng, algo, cin, cout, n, h, w):
    y, ref = conv_case(eng, algo, cin, cout, n, h, w)
    close(y, ref, what=f"{algo} conv {cin}->{cout} {n}x{h}x{w}", **BOUNDS.get(algo, {}))
