"""CPU side of ``base.TriangularInverse``: the ``torch.linalg.solve_triangular``
fallback, the routing predicate of ``ops/trtri.py``, the flag and shape errors
and the ``SKH_LS_TRINV`` opt-in of ``algorithms/regression.py`` on a CPU
operand.

Against ``torch.linalg.inv`` of the masked matrix the inverse is compared with
``max |X - X_ref| <= 8 n u cond_1(T) max |X_ref|``: both are forward errors of
backward-stable methods, each at most about ``n u cond`` (Higham, Accuracy and
Stability of Numerical Algorithms, Thm 8.5 and section 14.2); u = 2^-53 (f64),
2^-24 (f32).  The componentwise residual ``e = max |I - T X|_ij / (|T| |X|)_ij``
over the stored triangle is held to ``2 (n + 2) u`` as on the GPU
(``tests/test_gpu_trtri.py``).
"""
import itertools

import numpy as np
import pytest
import torch

from libskylark_amd import base as B
from libskylark_amd.base.exceptions import DimensionMismatchError, UnsupportedBaseOperation
from libskylark_amd.ops import trtri as ti

F64 = torch.float64
U_ = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24}
NAN = float("nan")
SIZES = (1, 5, 70)
_CACHE = {}


def _mask(n, uplo, diag="N"):
    ones = torch.ones(n, n, dtype=torch.bool)
    k = 0 if diag == "N" else 1
    return torch.tril(ones, -k) if uplo == "L" else torch.triu(ones, k)


def _tri(n, uplo, diag, dtype=F64):
    """A well-conditioned triangular matrix in f64 (exactly representable in
    ``dtype``), zeros in the other triangle, ones on a unit diagonal."""
    key = (n, uplo, diag, dtype)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(40 + n)
        Tm = torch.tril(torch.rand(n, n, generator=g, dtype=F64) * 2 - 1) + n * torch.eye(n, dtype=F64)
        if diag == "U":
            Tm = Tm / Tm.diagonal().view(1, -1)
        Tm = Tm.to(dtype).double()
        _CACHE[key] = (Tm if uplo == "L" else Tm.t()).contiguous()
    return _CACHE[key]


def _operand(Tm, uplo, diag, dtype=F64, layout="row"):
    """(buffer, view): the view holds Tm's stored triangle, everything else in
    the buffer (other triangle, pad, a unit diagonal) is NaN."""
    n = Tm.shape[0]
    m = _mask(n, uplo, diag)
    if layout == "col":
        buf = torch.full((n, n + 1), NAN, dtype=dtype)
        A = buf[:, :n].t()
    elif layout == "pitched":
        buf = torch.full((n, n + 3), NAN, dtype=dtype)
        A = buf[:, 1:n + 1]
    else:
        buf = torch.full((n, n), NAN, dtype=dtype)
        A = buf
    A.copy_(torch.where(m, Tm.to(dtype), A))
    return buf, A


def _resid(Tm, X, uplo):
    R = (torch.eye(Tm.shape[0], dtype=F64) - Tm @ X).abs() / (Tm.abs() @ X.abs())
    return float(R[_mask(Tm.shape[0], uplo)].max())


def _check(n, uplo, diag, dtype, layout):
    Tm = _tri(n, uplo, diag, dtype)
    buf, A = _operand(Tm, uplo, diag, dtype, layout)
    it = torch.int64 if dtype == F64 else torch.int32
    before = buf.clone()
    out = B.TriangularInverse(uplo, diag, A)
    assert out is A
    m = _mask(n, uplo, diag)
    # everything outside the stored triangle keeps its bits
    keep = torch.ones_like(buf, dtype=torch.bool)
    (keep[:, :n].t() if layout == "col" else keep[:, 1:n + 1] if layout == "pitched" else keep)[m] = False
    assert torch.equal(buf.view(it)[keep], before.view(it)[keep])
    X = torch.where(m, A.double(), torch.zeros((), dtype=F64))
    if diag == "U":
        X = X + torch.eye(n, dtype=F64)
    assert torch.isfinite(X).all()
    ref = torch.linalg.inv(Tm)
    u = U_[dtype]
    kappa = float(torch.linalg.matrix_norm(Tm, 1) * torch.linalg.matrix_norm(ref, 1))
    d, tol = float((X - ref).abs().max()), 8 * n * u * kappa * float(ref.abs().max())
    e = _resid(Tm, X, uplo)
    print(f"TriangularInverse cpu n={n} {uplo}{diag} {dtype} {layout}: |X - inv| {d:.3e} tol {tol:.3e}, "
          f"e {e / ((n + 1) * u):.3f} (n + 1) u")
    assert d <= tol
    assert e <= 2 * (n + 2) * u


def test_exports():
    from libskylark_amd.base import TriangularInverse  # noqa: F401
    from libskylark_amd.ops import trtri  # noqa: F401
    assert "TriangularInverse" in B.blas.__all__
    for name in ("_why_not", "takes", "ok", "block", "trtri_tri"):
        assert callable(getattr(trtri, name))


@pytest.mark.parametrize("layout", ["row", "col", "pitched"])
@pytest.mark.parametrize("uplo,diag", list(itertools.product("LU", "NU")))
@pytest.mark.parametrize("n", SIZES)
def test_fallback_f64(n, uplo, diag, layout):
    _check(n, uplo, diag, F64, layout)


@pytest.mark.parametrize("uplo,diag", list(itertools.product("LU", "NU")))
@pytest.mark.parametrize("n", SIZES)
def test_fallback_f32(n, uplo, diag):
    assert "f64" in ti._why_not(torch.zeros(n, n, dtype=torch.float32))
    _check(n, uplo, diag, torch.float32, "row")


def test_fallback_other_views_and_empty():
    # neither stride is one: still inverted, through the same fallback
    n = 5
    Tm = _tri(n, "U", "N")
    big = torch.full((2 * n, 2 * n), NAN, dtype=F64)
    A = big[::2, ::2]
    A.copy_(torch.where(_mask(n, "U"), Tm, A))
    assert "unit stride" in ti._why_not(A)
    assert B.TriangularInverse("u", "n", A) is A
    X = torch.triu(A)
    assert _resid(Tm, X, "U") <= 2 * (n + 2) * U_[F64]
    assert torch.isnan(A[~_mask(n, "U")]).all() and torch.isnan(big[1::2]).all() and torch.isnan(big[:, 1::2]).all()
    E = torch.zeros(0, 0, dtype=F64)
    assert B.TriangularInverse("L", "N", E) is E
    Z = torch.tril(torch.ones(3, 3, dtype=torch.complex128)) * (1 + 1j)
    ref = torch.linalg.inv(Z)
    assert B.TriangularInverse("L", "N", Z) is Z
    torch.testing.assert_close(Z, ref, rtol=1e-14, atol=1e-14)


def test_flag_and_shape_errors():
    A = _tri(5, "L", "N").clone()
    with pytest.raises(ValueError, match="uplo"):
        B.TriangularInverse("X", "N", A)
    with pytest.raises(ValueError, match="diag"):
        B.TriangularInverse("L", "T", A)
    with pytest.raises(ValueError, match="uplo"):
        ti.trtri_tri("X", "N", A)
    with pytest.raises(ValueError, match="diag"):
        ti.trtri_tri("L", "X", A)
    with pytest.raises(ValueError, match="CUDA"):          # good flags (any case) get as far as the operand
        ti.trtri_tri("u", "u", A)
    with pytest.raises(DimensionMismatchError):
        B.TriangularInverse("L", "N", torch.zeros(4, 5, dtype=F64))
    with pytest.raises(DimensionMismatchError):
        B.TriangularInverse("L", "N", torch.zeros(4, dtype=F64))
    with pytest.raises(DimensionMismatchError):
        B.TriangularInverse("L", "N", A.to_sparse())
    assert torch.equal(A, _tri(5, "L", "N"))               # nothing was touched on the way to an error


def test_dist_star_star_and_vc_star():
    from libskylark_amd.parallel.distmatrix import DistMatrix
    n = 30
    Tm = _tri(n, "U", "N")
    D = DistMatrix.from_global(torch.where(_mask(n, "U"), Tm, torch.full_like(Tm, 7.0)), "STAR_STAR")
    out = B.TriangularInverse("U", "N", D)
    assert out is D
    assert _resid(Tm, torch.triu(D.local), "U") <= 2 * (n + 2) * U_[F64]
    assert torch.equal(torch.tril(D.local, -1), torch.tril(torch.full_like(Tm, 7.0), -1))
    with pytest.raises(UnsupportedBaseOperation):
        B.TriangularInverse("U", "N", DistMatrix.from_global(Tm.clone(), "VC_STAR"))


def test_why_not_reasons():
    A = torch.zeros(6, 6, dtype=F64)
    # a CPU operand fails on the device alone, and last
    assert ti._why_not(A) == "A must be a CUDA tensor"
    assert not ti.takes(A) and not ti.ok(A)
    assert "dense 2-D" in ti._why_not(A[0])
    assert "dense 2-D" in ti._why_not(A.to_sparse())
    assert "dense 2-D" in ti._why_not(None)
    assert "A must be f64" in ti._why_not(A.float())
    assert "A must be f64" in ti._why_not(A.to(torch.complex128))
    assert "A must be square" in ti._why_not(A[:, :5])
    assert "A: needs unit stride" in ti._why_not(torch.zeros(12, 12, dtype=F64)[::2, ::2])
    assert "A's rows overlap" in ti._why_not(torch.zeros(11, dtype=F64).as_strided((6, 6), (1, 1)))
    assert "A's rows overlap" in ti._why_not(torch.zeros(40, dtype=F64).as_strided((6, 6), (5, 1)))
    assert "A's rows overlap" in ti._why_not(torch.zeros(40, dtype=F64).as_strided((6, 6), (1, 5)))
    raw = np.zeros(8 * 38, dtype=np.uint8)
    off = (-raw.ctypes.data) % 8 + 4                       # base off by 4 B
    mis = torch.from_numpy(np.frombuffer(raw, dtype=np.float64, count=36, offset=off)).view(6, 6)
    assert mis.data_ptr() % 8 == 4
    assert "A needs an 8-B aligned base" in ti._why_not(mis)
    # row-major, column-major, pitched, one-element and empty operands lack only the device
    for X in (torch.zeros(6, 7, dtype=F64)[:, :6], torch.zeros(6, 7, dtype=F64)[:, :6].t(),
              torch.zeros(6, 9, dtype=F64)[:, 2:8], torch.zeros(1, 1, dtype=F64), torch.zeros(0, 0, dtype=F64)):
        assert ti._why_not(X) == "A must be a CUDA tensor"
    assert ti.launches(0) == 0 and ti.launches(64) == 1 and ti.launches(65) == 4 and ti.launches(5000) == 235


def test_regression_opt_in_on_cpu_is_the_old_path(monkeypatch):
    from libskylark_amd.algorithms import regression as rg
    n = 70
    R = _tri(n, "U", "N")
    monkeypatch.delenv("SKH_LS_TRINV", raising=False)
    want = rg._tri_inv_upper(R, block=32)
    monkeypatch.setenv("SKH_LS_TRINV", "native")
    Rc = R.clone()
    got = rg._tri_inv_upper(R, block=32)
    assert torch.equal(R, Rc) and got is not R
    assert torch.equal(got.view(torch.int64), want.view(torch.int64))
    assert torch.equal(torch.tril(got, -1), torch.zeros(n, n, dtype=F64))
