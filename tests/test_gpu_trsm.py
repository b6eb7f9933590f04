"""One-triangle f64 triangular solve on the GPU (``trsm_tri.hip`` through
``ops/trsm.py`` and ``base.Trsm``).

Error measure, side L: ``e = max_ir |alpha B0 - op(T) X|_ir / (|op(T)| |X|)_ir``
(side R: ``X op(T)``), evaluated in f64 on the CPU from the stored triangle
only, with the unit diagonal inserted for diag U.  Bound: ``e <= 2 (n + 2)
2^-53``.  One ``(n + 1) u`` is Higham's componentwise backward error of
substitution in any order (Accuracy and Stability of Numerical Algorithms,
Thm 8.5) plus the alpha scaling; the other share is this file's own f64
evaluation.  ``torch.linalg.solve_triangular`` on the CPU stays at or below
0.82 (n + 1) u over these matrices.

Matrices, built on the CPU from seeded generators:
(a) the Cholesky factor of ``B B^T + n I``, B uniform in (-1, 1): condition
    about 1.5;
(b) the Cholesky factor of the Gaussian-kernel Gram (sigma = 1) of n uniform
    points in [0,1]^4 plus ``1e-6 I``: condition 6e3 .. 3e4, the case an
    inverse-multiplying diagonal solve fails.
Diag U: the same factor with each column divided by its diagonal entry, stored
with NaN on the diagonal.  Uplo U: the transpose.  A is the view ``[:, :n]`` of
an n x (n + 1) buffer whose other triangle and padding hold NaN; B is a view
of a buffer one column wider with a NaN pad.

Measured e on one MI355X over the 1416 solves of the shape and flag cases: 0 ..
2.2e-15, that is 0 .. 0.83 of (n + 1) u (the largest ratio at n = 1; 0.12 at
most from n = 63 on; the bound allows 2).
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NAN = float("nan")
_CACHE = {}
FLIP = {"L": "U", "U": "L", "N": "T", "T": "N"}
FLIP_SIDE = {"L": "R", "R": "L"}


def _block():
    from libskylark_amd.ops import trsm as tr
    if "blk" not in _CACHE:
        _CACHE["blk"] = tr.block()
    return _CACHE["blk"]


def _sizes():
    nb, t = 64, 128           # asserted against sl_trsm_tri_block() in test_block_sizes
    return sorted({1, 2, 3, nb - 1, nb, nb + 1, t - 1, t, t + 1, nb + t - 1, nb + t, nb + t + 1, 600, 1000})


THIN_T, WIDE_T = (1, 3, 8), (9, 17, 129)      # on both sides of the thin / wide threshold (8, asserted too)


def _mask(n, uplo):
    ones = torch.ones(n, n, dtype=torch.bool)
    return torch.tril(ones) if uplo == "L" else torch.triu(ones)


def _tri(fam, n, uplo, diag):
    """The triangular f64 test matrix (CPU) with zeros in the other triangle
    and, for diag U, ones on the diagonal; computed once and never changed."""
    key = ("T", fam, n, uplo, diag)
    if key not in _CACHE:
        if ("L0", fam, n) not in _CACHE:
            g = torch.Generator().manual_seed(1000 * (1 + "ab".index(fam)) + n)
            if fam == "a":
                Bm = torch.rand(n, n, generator=g, dtype=torch.float64) * 2 - 1
                A = Bm @ Bm.t() + n * torch.eye(n, dtype=torch.float64)
            else:
                X = torch.rand(n, 4, generator=g, dtype=torch.float64)
                A = torch.exp(-torch.cdist(X, X) ** 2 / 2.0) + 1e-6 * torch.eye(n, dtype=torch.float64)
            _CACHE[("L0", fam, n)] = torch.linalg.cholesky(torch.tril(A) + torch.tril(A, -1).t())
        L = _CACHE[("L0", fam, n)]
        if diag == "U":
            L = L / L.diagonal().view(1, -1)
        _CACHE[key] = (L if uplo == "L" else L.t()).contiguous()
    return _CACHE[key]


def _rhs(rows, cols, seed):
    key = ("B", rows, cols, seed)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(77 + 131 * seed + rows + 7 * cols)
        _CACHE[key] = torch.randn(rows, cols, generator=g, dtype=torch.float64)
    return _CACHE[key]


def _a_buf(Tm, uplo, diag, other=NAN, dval=NAN):
    """A fresh n x (n + 1) buffer on the GPU: the view [:, :n] holds Tm's
    ``uplo`` triangle (diag U: ``dval`` on the diagonal), all else ``other``."""
    n = Tm.shape[0]
    buf = torch.full((n, n + 1), other, dtype=torch.float64)
    buf[:, :n] = torch.where(_mask(n, uplo), Tm, buf[:, :n])
    if diag == "U":
        buf[:, :n].diagonal().fill_(dval)
    return buf.cuda()


def _b_buf(B0):
    buf = torch.full((B0.shape[0], B0.shape[1] + 1), NAN, dtype=torch.float64)
    buf[:, :B0.shape[1]] = B0
    return buf.cuda()


def _err(side, orient, alpha, Tm, B0, X):
    op = Tm if orient == "N" else Tm.t()
    if side == "L":
        R, D = alpha * B0 - op @ X, op.abs() @ X.abs()
    else:
        R, D = alpha * B0 - X @ op, X.abs() @ op.abs()
    return float((R.abs() / D).max())


def _solve_check(fam, n, t, side, uplo, orient, diag, alpha, seed=0):
    """One native solve on padded NaN-filled operands; asserts the bound, returns e."""
    from libskylark_amd.ops import trsm as tr
    Tm = _tri(fam, n, uplo, diag)
    B0 = _rhs(n, t, seed) if side == "L" else _rhs(t, n, seed)
    A = _a_buf(Tm, uplo, diag)[:, :n]
    Bb = _b_buf(B0)
    Bv = Bb[:, :B0.shape[1]]
    assert tr.ok(side, A, Bv)
    out = tr.trsm_tri(side, uplo, orient, diag, alpha, A, Bv)
    assert out is Bv
    X = Bv.cpu()
    assert torch.isfinite(X).all() and torch.isnan(Bb[:, -1]).all()
    e = _err(side, orient, alpha, Tm, B0, X)
    print(f"trsm_tri n={n} t={t} {side}{uplo}{orient}{diag} alpha={alpha} ({fam}): e {e:.3e} = "
          f"{e / ((n + 1) * U):.3f} (n + 1) u")
    assert e <= 2 * (n + 2) * U
    return e


def test_block_sizes():
    nb, tile, thin = _block()
    assert (nb, tile, thin) == (64, 128, 8)
    assert _sizes() == [1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 600, 1000]
    assert max(THIN_T) == thin and min(WIDE_T) == thin + 1


def test_empty():
    from libskylark_amd import base as B
    from libskylark_amd.ops import trsm as tr
    A0 = torch.empty(0, 0, dtype=torch.float64, device="cuda")
    B00 = torch.empty(0, 3, dtype=torch.float64, device="cuda")
    assert tr.trsm_tri("L", "L", "N", "N", 1.0, A0, B00) is B00
    assert B.Trsm("R", "U", "T", "U", 2.0, A0, B00.t()).shape == (3, 0)
    A = _a_buf(_tri("a", 5, "L", "N"), "L", "N")[:, :5]
    Bb = torch.full((5, 1), NAN, dtype=torch.float64, device="cuda")
    for side, Bv in (("L", Bb[:, :0]), ("R", Bb.t()[:0, :])):
        assert tr.ok(side, A, Bv)
        assert tr.trsm_tri(side, "L", "N", "N", -0.75, A, Bv) is Bv
        assert B.Trsm(side, "L", "N", "N", -0.75, A, Bv) is Bv
    assert torch.isnan(Bb).all()


@pytest.mark.parametrize("uplo,orient", [("L", "N"), ("L", "T"), ("U", "N"), ("U", "T")])
@pytest.mark.parametrize("n,fam", [(n, f) for n in _sizes() for f in "ab" if f == "a" or n >= 3])
def test_shapes_and_edges(n, fam, uplo, orient):
    ts = THIN_T + WIDE_T if n < 600 else (1, 8, 17)
    for i, t in enumerate(ts):
        for alpha in (1.0, -0.75):
            _solve_check(fam, n, t, "L", uplo, orient, "N", alpha, seed=i)


@pytest.mark.parametrize("side,uplo,orient,diag", list(itertools.product("LR", "LU", "NT", "NU")))
@pytest.mark.parametrize("n", [193, 600])
def test_all_flag_combinations(n, side, uplo, orient, diag):
    for fam in "ab":
        for t in (5, 17):
            for alpha in (1.0, -0.75):
                _solve_check(fam, n, t, side, uplo, orient, diag, alpha)


@pytest.mark.parametrize("t", [3, 17])
@pytest.mark.parametrize("side,uplo,orient,diag", list(itertools.product("LR", "LU", "NT", "NU")))
def test_untouched_storage_and_determinism(side, uplo, orient, diag, t):
    from libskylark_amd.ops import trsm as tr
    n = 200
    Tm = _tri("b", n, uplo, diag)
    B0 = _rhs(n, t, 3) if side == "L" else _rhs(t, n, 3)
    cols = B0.shape[1]

    def run(other, dval):
        Ab, Bb = _a_buf(Tm, uplo, diag, other, dval), _b_buf(B0)
        before = Ab.view(torch.int64).clone()
        tr.trsm_tri(side, uplo, orient, diag, -0.75, Ab[:, :n], Bb[:, :cols])
        assert torch.equal(Ab.view(torch.int64), before)          # A's whole buffer
        assert torch.isnan(Bb[:, -1]).all()                       # B's pad column
        assert torch.isfinite(Bb[:, :cols]).all()
        return Bb.view(torch.int64)

    ref = run(NAN, NAN)
    assert torch.equal(_b_buf(B0).view(torch.int64)[:, -1], ref[:, -1])
    assert torch.equal(run(0.0, NAN), ref)                        # zeros in the unstored triangle
    if diag == "U":
        assert torch.equal(run(NAN, 7.0), ref)                    # the diagonal is not read
    assert torch.equal(run(NAN, NAN), ref)                        # a second run
    assert _err(side, orient, -0.75, Tm, B0, ref.view(torch.float64)[:, :cols].cpu()) <= 2 * (n + 2) * U


@pytest.mark.parametrize("t", [5, 17])
@pytest.mark.parametrize("side,uplo,orient,diag", [("L", "L", "N", "N"), ("L", "U", "T", "U"), ("R", "L", "T", "N"),
                                                   ("R", "U", "N", "U")])
def test_column_major_operands(side, uplo, orient, diag, t):
    from libskylark_amd.ops import trsm as tr
    n, alpha = 193, -0.75
    Tm = _tri("b", n, uplo, diag)
    B0 = _rhs(n, t, 4) if side == "L" else _rhs(t, n, 4)
    cols = B0.shape[1]
    fu, fo, fs = FLIP[uplo], FLIP[orient], FLIP_SIDE[side]
    # a column-major A: the transposed view of the row-major buffer that holds T^T
    Abt = _a_buf(Tm.t().contiguous(), fu, diag)
    Ac = Abt[:, :n].t()
    assert Ac.stride() == (1, n + 1) and tr.ok(side, Ac, _b_buf(B0)[:, :cols])
    B1, B2 = _b_buf(B0), _b_buf(B0)
    assert tr.trsm_tri(side, uplo, orient, diag, alpha, Ac, B1[:, :cols]).data_ptr() == B1.data_ptr()
    tr.trsm_tri(side, fu, fo, diag, alpha, Abt[:, :n], B2[:, :cols])
    assert torch.equal(B1.view(torch.int64), B2.view(torch.int64))
    assert _err(side, orient, alpha, Tm, B0, B1[:, :cols].cpu()) <= 2 * (n + 2) * U
    # a column-major B: the transposed view of the row-major buffer that holds B0^T
    A = _a_buf(Tm, uplo, diag)[:, :n]
    B3, B4 = _b_buf(B0.t().contiguous()), _b_buf(B0.t().contiguous())
    rows = B0.shape[0]
    Bc = B3[:, :rows].t()
    assert Bc.stride() == (1, rows + 1) and tr.ok(side, A, Bc)
    assert tr.trsm_tri(side, uplo, orient, diag, alpha, A, Bc) is Bc
    tr.trsm_tri(fs, uplo, fo, diag, alpha, A, B4[:, :rows])
    assert torch.equal(B3.view(torch.int64), B4.view(torch.int64))
    assert torch.isnan(B3[:, -1]).all()
    assert _err(side, orient, alpha, Tm, B0, Bc.cpu()) <= 2 * (n + 2) * U


@pytest.mark.parametrize("orient", ["N", "T"])
@pytest.mark.parametrize("t", [1, 17])
@pytest.mark.parametrize("fam", ["a", "b"])
def test_against_library(fam, t, orient):
    n = 600
    Tm = _tri(fam, n, "L", "N")
    B0 = _rhs(n, t, 0)
    e = _solve_check(fam, n, t, "L", "L", orient, "N", 1.0)
    Tz = Tm.cuda()                                 # zeros in the other triangle
    Xl = torch.linalg.solve_triangular(Tz if orient == "N" else Tz.t(), B0.cuda(), upper=orient == "T", left=True)
    el = _err("L", orient, 1.0, Tm, B0, Xl.cpu())
    print(f"trsm_tri n={n} t={t} LL{orient}N ({fam}): e {e:.3e}, library {el:.3e}")
    assert e <= 2 * el + (n + 2) * U


@pytest.mark.parametrize("side,t", [("L", 3), ("R", 17)])
def test_alpha_zero(side, t):
    from libskylark_amd import base as B
    from libskylark_amd.ops import trsm as tr
    n = 65
    A = _a_buf(_tri("a", n, "L", "N"), "L", "N")[:, :n]
    shape = (n, t) if side == "L" else (t, n)
    for f in (tr.trsm_tri, B.Trsm):
        Bb = torch.full((shape[0], shape[1] + 1), NAN, dtype=torch.float64, device="cuda")
        Bv = Bb[:, :shape[1]]
        assert f(side, "L", "N", "N", 0.0, A, Bv) is Bv
        assert torch.equal(Bv, torch.zeros_like(Bv)) and not torch.signbit(Bv).any()
        assert torch.isnan(Bb[:, -1]).all()


@pytest.mark.parametrize("t", [3, 17])
@pytest.mark.parametrize("side,uplo,orient,diag", [("L", "L", "N", "N"), ("L", "U", "T", "U"), ("R", "L", "T", "N"),
                                                   ("R", "U", "N", "U")])
def test_base_routing(side, uplo, orient, diag, t):
    from libskylark_amd import base as B
    from libskylark_amd.ops import trsm as tr
    n, alpha = 129, -0.75
    Tm = _tri("a", n, uplo, diag)
    B0 = _rhs(n, t, 5) if side == "L" else _rhs(t, n, 5)
    cols = B0.shape[1]
    upper = (uplo == "U") != (orient == "T")

    def library(Af, Bt):       # base.Trsm's expression for operands the kernel does not take
        return torch.linalg.solve_triangular(Af if orient == "N" else Af.t(), alpha * Bt, upper=upper, left=side == "L",
                                             unitriangular=diag == "U")

    # a qualifying operand: the same B object, solved in place
    A = _a_buf(Tm, uplo, diag)[:, :n]
    B1, B2 = _b_buf(B0), _b_buf(B0)
    Bv = B1[:, :cols]
    assert tr.takes(side, A, Bv)
    out = B.Trsm(side, uplo, orient, diag, alpha, A, Bv)
    assert out is Bv
    if tr.regime(side, Bv) in tr.BASE_NATIVE_REGIMES:
        tr.trsm_tri(side, uplo, orient, diag, alpha, A, B2[:, :cols])
        assert torch.equal(B1.view(torch.int64), B2.view(torch.int64))
    else:
        assert torch.equal(Bv.view(torch.int64), library(A, B0.cuda()).view(torch.int64))
    assert _err(side, orient, alpha, Tm, B0, Bv.cpu()) <= 2 * (n + 2) * U
    # f32 on the GPU: the library way, bit for bit
    A32 = Tm.float().cuda()
    B32 = B0.float().cuda()
    assert not tr.takes(side, A32, B32)
    want = library(A32, B32.clone())
    out = B.Trsm(side, uplo, orient, diag, alpha, A32, B32)
    assert out is B32 and torch.equal(B32.view(torch.int32), want.view(torch.int32))
