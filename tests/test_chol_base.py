"""CPU side of ``base.Cholesky`` / ``CholeskySolveAfter`` / ``HPDSolve``: the
``torch.linalg.cholesky_ex`` fallback and the routing predicate of
``ops/cholesky.py``.

Error measure: with F the computed factor (L, or U^T),
``e = max |A - F F^T|_ij / (|F| |F|^T)_ij`` over the stored triangle, in f64.
Bound ``2 (n + 2) u``: ``(n + 1) u`` is Higham's componentwise bound for
Cholesky (Accuracy and Stability of Numerical Algorithms, Thm 10.3), the other
share is this file's own evaluation of ``F F^T``; u = 2^-53 (f64), 2^-24 (f32).
"""
import numpy as np
import pytest
import torch

from libskylark_amd import base as B
from libskylark_amd.base.exceptions import NLAError, UnsupportedBaseOperation
from libskylark_amd.ops import cholesky as ch

U_ = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24}


def _mask(n, uplo):
    ones = torch.ones(n, n, dtype=torch.bool)
    return torch.tril(ones) if uplo == "L" else torch.triu(ones)


def _spd(n, dtype, seed=0):
    """Family (a): B B^T + n I, B uniform in (-1, 1); exact in ``dtype``'s f64 image."""
    g = torch.Generator().manual_seed(100 + seed + n)
    Bm = torch.rand(n, n, generator=g, dtype=torch.float64) * 2 - 1
    A = Bm @ Bm.t() + n * torch.eye(n, dtype=torch.float64)
    A = A.to(dtype).double()
    return torch.tril(A) + torch.tril(A, -1).t()


def _operand(A64, dtype, uplo, seed=0):
    """An n x (n + 1) buffer whose view [:, :n] is the operand: the ``uplo``
    triangle is the data, the rest different random numbers."""
    n = A64.shape[0]
    g = torch.Generator().manual_seed(7 + seed)
    buf = torch.rand(n, n + 1, generator=g, dtype=torch.float64) + 3.0
    buf[:, :n] = torch.where(_mask(n, uplo), A64, buf[:, :n])
    return buf.to(dtype)


def _err(A64, Aout, uplo):
    F = torch.tril(Aout.double()) if uplo == "L" else torch.triu(Aout.double()).t()
    m = torch.tril(torch.ones_like(A64, dtype=torch.bool))
    return float(((A64 - F @ F.t()).abs() / (F.abs() @ F.abs().t()))[m].max())


def test_exports():
    from libskylark_amd.base import Cholesky, CholeskySolveAfter, HPDSolve  # noqa: F401
    assert {"Cholesky", "CholeskySolveAfter", "HPDSolve"} <= set(B.blas.__all__)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("n", [1, 3, 65, 200])
def test_fallback_bound_and_other_triangle(n, uplo, dtype):
    A64 = _spd(n, dtype)
    buf = _operand(A64, dtype, uplo)
    A = buf[:, :n]
    before = buf.clone()
    out = B.Cholesky(uplo, A)
    assert out is A
    e = _err(A64, A, uplo)
    print(f"Cholesky cpu n={n} {uplo} {dtype}: e {e:.3e} bound {2 * (n + 2) * U_[dtype]:.3e}")
    assert e <= 2 * (n + 2) * U_[dtype]
    other = ~_mask(n, uplo)
    it = torch.int64 if dtype == torch.float64 else torch.int32
    assert torch.equal(buf[:, :n][other].view(it), before[:, :n][other].view(it))
    assert torch.equal(buf[:, n].view(it), before[:, n].view(it))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("uplo", ["L", "U"])
def test_fallback_failure_index(uplo, dtype):
    n, p = 40, 17
    A = _spd(n, dtype).to(dtype)
    A[p, p] = -1.0
    with pytest.raises(NLAError, match=rf"pivot {p + 1} "):
        B.Cholesky(uplo, A.clone())
    info = torch.full((1,), -5, dtype=torch.int32)
    out = B.Cholesky(uplo, A, info)          # silent
    assert out is A and int(info) == p + 1
    good = _spd(n, dtype).to(dtype)
    B.Cholesky(uplo, good, info)
    assert int(info) == 0


def test_arguments():
    A = _spd(5, torch.float64)
    with pytest.raises(ValueError, match="uplo"):
        B.Cholesky("X", A)
    with pytest.raises(ValueError):
        B.Cholesky("L", torch.zeros(4, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="uplo"):
        B.CholeskySolveAfter("X", "N", A, torch.zeros(5, 1, dtype=torch.float64))
    with pytest.raises(ValueError):
        B.CholeskySolveAfter("L", "N", A, torch.zeros(4, 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="uplo"):
        ch.chol_tri(A, "X")


@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("t", [1, 5])
def test_hpdsolve_against_solve(uplo, t):
    n = 120
    A64 = _spd(n, torch.float64)
    g = torch.Generator().manual_seed(3)
    Bm = torch.randn(n, t, generator=g, dtype=torch.float64)
    ref = torch.linalg.solve(A64, Bm)
    A = torch.where(_mask(n, uplo), A64, torch.full_like(A64, float("nan")))
    X = Bm.clone()
    out = B.HPDSolve(uplo, "N", A, X)
    assert out is X and torch.isfinite(X).all()
    d = float((X - ref).abs().max() / ref.abs().max())
    tol = 8 * n * 2.0 ** -53 * float(torch.linalg.cond(A64))
    print(f"HPDSolve cpu n={n} t={t} {uplo}: {d:.3e} tol {tol:.3e}")
    assert d <= tol
    # A ends as the factor: SolveAfter on it gives the same solution again
    Y = Bm.clone()
    B.CholeskySolveAfter(uplo, "T", A, Y)
    assert torch.equal(Y, X)


def test_dist_star_star_and_vc_star():
    from libskylark_amd.parallel.distmatrix import DistMatrix
    n = 30
    A64 = _spd(n, torch.float64)
    D = DistMatrix.from_global(A64.clone(), "STAR_STAR")
    out = B.Cholesky("L", D)
    assert out is D
    assert _err(A64, D.local, "L") <= 2 * (n + 2) * 2.0 ** -53
    assert torch.equal(torch.triu(D.local, 1), torch.triu(A64, 1))
    X = torch.ones(n, 2, dtype=torch.float64)
    B.CholeskySolveAfter("L", "N", D, X)
    torch.testing.assert_close(A64 @ X, torch.ones(n, 2, dtype=torch.float64), rtol=1e-12, atol=1e-12)
    with pytest.raises(UnsupportedBaseOperation):
        B.Cholesky("L", DistMatrix.from_global(A64.clone(), "VC_STAR"))


def test_why_not_reasons():
    A = torch.zeros(20, 20, dtype=torch.float64)
    assert not ch.takes(A) and not ch.ok(A)
    assert "CUDA" in ch._why_not(A)
    with pytest.raises(ValueError, match="CUDA"):
        ch.chol_tri(A)
    assert "dense 2-D" in ch._why_not(torch.zeros(4, dtype=torch.float64))
    assert "dense 2-D" in ch._why_not(A.to_sparse())
    assert "dense 2-D" in ch._why_not(None)
    assert "square" in ch._why_not(torch.zeros(4, 5, dtype=torch.float64))
    assert "f64" in ch._why_not(A.float())
    assert "row-major" in ch._why_not(A[::2, ::2])
    assert "row-major" in ch._why_not(torch.zeros(20, 21, dtype=torch.float64)[:, :20].t())
    assert "overlap" in ch._why_not(torch.zeros(40, dtype=torch.float64).as_strided((20, 20), (1, 1)))
    raw = np.zeros(8 * 402, dtype=np.uint8)
    off = (-raw.ctypes.data) % 8 + 4                     # base off by 4 B
    mis = torch.from_numpy(np.frombuffer(raw, dtype=np.float64, count=400, offset=off)).view(20, 20)
    assert "8-B" in ch._why_not(mis)
    # an odd pitch is fine: only the device is missing
    assert "CUDA" in ch._why_not(torch.zeros(20, 21, dtype=torch.float64)[:, :20])
    assert "CUDA" in ch._why_not(torch.zeros(0, 0, dtype=torch.float64))


def test_krr_opt_in_cpu(monkeypatch):
    from libskylark_amd import ml
    from libskylark_amd.ml import krr
    g = torch.Generator().manual_seed(5)
    X = torch.randn(150, 4, generator=g, dtype=torch.float64) * 0.7
    Y = torch.sin(X.sum(1, keepdim=True))
    k = ml.Gaussian(4, 1.5)
    Z = torch.randn(300, 40, generator=g, dtype=torch.float64)
    T_ = torch.randn(300, 3, generator=g, dtype=torch.float64)
    monkeypatch.delenv("SKH_KRR_CHOL", raising=False)
    A0, W0 = ml.kernel_ridge(k, X, Y, 0.05), krr._ridge(Z, T_, 1e-2)
    monkeypatch.setenv("SKH_KRR_CHOL", "native")
    Yc = Y.clone()
    A1, W1 = ml.kernel_ridge(k, X, Y, 0.05), krr._ridge(Z, T_, 1e-2)
    assert torch.equal(Y, Yc)                 # the right-hand side is not overwritten
    assert A1.shape == A0.shape and W1.shape == W0.shape
    assert float((A1 - A0).norm() / A0.norm()) < 1e-10
    assert float((W1 - W0).norm() / W0.norm()) < 1e-13
