"""One-triangle f64 triangular inverse on the GPU (``trtri_tri.hip`` through
``ops/trtri.py`` and ``base.TriangularInverse``), and the ``SKH_LS_TRINV=native``
opt-in of ``algorithms/regression.py``.

Error measure: ``e = max_ij |I - T X|_ij / (|T| |X|)_ij`` over the stored
triangle, evaluated in f64 on the CPU from the stored triangles only, with the
unit diagonal inserted for diag U.  Bound: ``e <= 2 (n + 2) 2^-53``.  One
``(n + 1) u`` is Higham's componentwise residual bound for substitution in any
summation order (Accuracy and Stability of Numerical Algorithms, Thm 8.5),
which the kernel's block forward substitution on ``T X = I`` is, column by
column; the other share is this file's own f64 evaluation.

Matrices, built on the CPU from seeded generators (the two families of
``tests/test_gpu_trsm.py``):
(a) the Cholesky factor of ``B B^T + n I``, B uniform in (-1, 1);
(b) the Cholesky factor of the Gaussian-kernel Gram (sigma = 1) of n uniform
    points in [0,1]^4 plus ``1e-6 I``, whose inverse has a 1-norm condition up
    to about 1e7.
Diag U: the same factor with each column divided by its diagonal entry, stored
with NaN on the diagonal.  Uplo U: the transpose.  A is the view ``[:, :n]`` of
an n x (n + 1) buffer whose other triangle and padding hold NaN (column-major:
the transposed view of the buffer that holds the transpose).

Measured e on one MI355X over the 448 inverses of the shape and flag cases:
0 .. 3.5e-15, that is 0 .. 0.24 of (n + 1) u (the largest ratio at n = 65, family
(b); 0.21 at n = 3; 0.14 at most at the other sizes up to 193, 0.052 at n = 600
and 0.023 at n = 1000; the bound allows 2).
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NAN = float("nan")
_CACHE = {}
FLIP = {"L": "U", "U": "L"}


def _sizes():
    nb, t = 64, 128           # asserted against sl_trtri_tri_block() in test_block_sizes
    return sorted({1, 2, 3, nb - 1, nb, nb + 1, t - 1, t, t + 1, nb + t - 1, nb + t, nb + t + 1, 600, 1000})


def _mask(n, uplo, diag="N"):
    """The stored triangle: with diag U without the diagonal."""
    ones = torch.ones(n, n, dtype=torch.bool)
    k = 0 if diag == "N" else 1
    return torch.tril(ones, -k) if uplo == "L" else torch.triu(ones, k)


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


def _operand(Tm, uplo, diag, major="R", other=NAN):
    """(buffer, A) on the GPU.  A holds Tm's stored triangle (diag U: not the
    diagonal); the rest of the n x (n + 1) buffer holds ``other``.  Row-major:
    A = buffer[:, :n]; column-major: A = buffer[:, :n].t(), stride (1, n + 1)."""
    n = Tm.shape[0]
    buf = torch.full((n, n + 1), other, dtype=torch.float64)
    if major == "R":
        buf[:, :n] = torch.where(_mask(n, uplo, diag), Tm, buf[:, :n])
    else:
        buf[:, :n] = torch.where(_mask(n, FLIP[uplo], diag), Tm.t(), buf[:, :n])
    buf = buf.cuda()
    A = buf[:, :n] if major == "R" else buf[:, :n].t()
    return buf, A


def _stored_in_buf(n, uplo, diag, major):
    """The buffer positions (n x (n + 1), bool) of A's stored triangle."""
    m = torch.zeros(n, n + 1, dtype=torch.bool)
    m[:, :n] = _mask(n, uplo if major == "R" else FLIP[uplo], diag)
    return m


def _full(Av, uplo, diag):
    """The triangular matrix that a CPU copy of the operand stores (zeros
    elsewhere, the unit diagonal inserted)."""
    n = Av.shape[0]
    X = torch.where(_mask(n, uplo, diag), Av, torch.zeros((), dtype=torch.float64))
    return X + torch.eye(n, dtype=torch.float64) if diag == "U" else X


def _err(Tm, X, uplo):
    n = Tm.shape[0]
    D = Tm.abs() @ X.abs()
    m = _mask(n, uplo)
    assert bool((D[m] > 0).all())
    return float(((torch.eye(n, dtype=torch.float64) - Tm @ X).abs() / D)[m].max())


def _inverse_check(fam, n, uplo, diag, major, f=None):
    """One native inverse on a padded NaN-filled operand; asserts finiteness,
    the bound, the untouched storage and the return value; returns (e, bits)."""
    from libskylark_amd.ops import trtri as ti
    Tm = _tri(fam, n, uplo, diag)
    buf, A = _operand(Tm, uplo, diag, major)
    assert A.stride() == ((n + 1, 1) if major == "R" else (1, n + 1)) and ti.ok(A)
    before = buf.cpu().view(torch.int64)
    out = (f or ti.trtri_tri)(uplo, diag, A)
    assert out is A
    after = buf.cpu()
    stored = _stored_in_buf(n, uplo, diag, major)
    assert torch.isfinite(after[stored]).all()
    # the other triangle, the pad and a unit diagonal keep their bits
    assert torch.equal(after.view(torch.int64)[~stored], before[~stored])
    Av = after[:, :n] if major == "R" else after[:, :n].t()
    e = _err(Tm, _full(Av, uplo, diag), uplo)
    print(f"trtri_tri n={n} {uplo}{diag} {major} ({fam}): e {e:.3e} = {e / ((n + 1) * U):.4f} (n + 1) u")
    assert e <= 2 * (n + 2) * U
    return e, after.view(torch.int64)


def test_block_sizes():
    from libskylark_amd.ops import trtri as ti
    assert ti.block() == (64, 128)
    assert _sizes() == [1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 600, 1000]


def test_empty():
    from libskylark_amd import base as B
    from libskylark_amd.ops import trtri as ti
    A0 = torch.empty(0, 0, dtype=torch.float64, device="cuda")
    assert ti.ok(A0) and ti.trtri_tri("L", "N", A0) is A0 and B.TriangularInverse("U", "U", A0) is A0


@pytest.mark.parametrize("fam", ["a", "b"])
@pytest.mark.parametrize("n", _sizes())
def test_shapes_flags_and_layouts(n, fam):
    worst = 0.0
    for uplo, diag, major in itertools.product("LU", "NU", "RC"):
        worst = max(worst, _inverse_check(fam, n, uplo, diag, major)[0])
    print(f"trtri_tri n={n} ({fam}): worst e {worst / ((n + 1) * U):.4f} (n + 1) u")


@pytest.mark.parametrize("uplo,diag", list(itertools.product("LU", "NU")))
@pytest.mark.parametrize("n", [193, 1000])
def test_determinism(n, uplo, diag):
    _, first = _inverse_check("b", n, uplo, diag, "R")
    _, second = _inverse_check("b", n, uplo, diag, "R")
    assert torch.equal(first, second)


@pytest.mark.parametrize("uplo,diag,major", [("L", "N", "R"), ("U", "U", "R"), ("U", "N", "C"), ("L", "U", "C")])
def test_base_gives_the_same_bits(uplo, diag, major):
    from libskylark_amd import base as B
    n = 193
    _, native = _inverse_check("a", n, uplo, diag, major)
    _, through_base = _inverse_check("a", n, uplo, diag, major, f=B.TriangularInverse)
    assert torch.equal(native, through_base)
    # f32 on the GPU: the library way on a masked copy, the other triangle untouched
    Tm = _tri("a", n, uplo, "N")
    A32 = torch.where(_mask(n, uplo), Tm, torch.full_like(Tm, NAN)).float().cuda()
    out = B.TriangularInverse(uplo, "N", A32)
    assert out is A32
    X32 = A32.cpu()
    assert torch.isnan(X32[~_mask(n, uplo)]).all() and torch.isfinite(X32[_mask(n, uplo)]).all()


def test_cholesky_then_inverse_in_one_buffer():
    from libskylark_amd import base as B
    n = 600
    g = torch.Generator().manual_seed(1600)
    Bm = torch.rand(n, n, generator=g, dtype=torch.float64) * 2 - 1
    S = Bm @ Bm.t() + n * torch.eye(n, dtype=torch.float64)
    buf = torch.full((n, n + 1), NAN, dtype=torch.float64)
    buf[:, :n] = torch.where(_mask(n, "L"), S, buf[:, :n])
    buf = buf.cuda()
    A = buf[:, :n]
    before = buf.cpu().view(torch.int64)
    assert B.Cholesky("L", A) is A
    F = torch.tril(A.cpu())
    assert B.TriangularInverse("L", "N", A) is A
    after = buf.cpu()
    stored = _stored_in_buf(n, "L", "N", "R")
    assert torch.equal(after.view(torch.int64)[~stored], before[~stored])     # the upper triangle and the pad
    assert torch.isfinite(after[stored]).all()
    e = _err(F, torch.tril(after[:, :n]), "L")
    print(f"Cholesky + TriangularInverse n={n}: e {e:.3e} = {e / ((n + 1) * U):.4f} (n + 1) u")
    assert e <= 2 * (n + 2) * U


def test_regression_opt_in(monkeypatch):
    from libskylark_amd.algorithms import regression as rg
    n = 600
    Tm = _tri("a", n, "U", "N")
    R = Tm.cuda()
    monkeypatch.setenv("SKH_LS_TRINV", "native")
    Rinv = rg._tri_inv_upper(R)
    assert Rinv is not R and torch.equal(R.cpu(), Tm)
    X = Rinv.cpu()
    assert torch.equal(torch.tril(X, -1), torch.zeros(n, n, dtype=torch.float64))
    assert not torch.signbit(torch.tril(X, -1)).any()
    e = _err(Tm, X, "U")
    print(f"_tri_inv_upper native n={n}: e {e:.3e} = {e / ((n + 1) * U):.4f} (n + 1) u")
    assert e <= 2 * (n + 2) * U
    # the CholeskyQR preconditioner accepts the same sketch either way
    g = torch.Generator().manual_seed(9)
    SA = torch.randn(4 * n, n, generator=g, dtype=torch.float32).cuda()
    rr1 = rg._cholqr_r(SA)
    monkeypatch.delenv("SKH_LS_TRINV")
    rr0 = rg._cholqr_r(SA)
    assert rr0 is not None and rr1 is not None
    d = float(torch.linalg.matrix_norm(rr1[1] - rr0[1], 1) / torch.linalg.matrix_norm(rr0[1], 1))
    print(f"_cholqr_r n={n}: R^-1 native vs default {d:.3e} (relative, 1-norm)")
    assert d <= 1e-10
