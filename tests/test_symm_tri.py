"""CPU side of the triangle-reading Symm: the ``SymTriOp`` torch fallback, the
routing predicate of ``ops/symm.py`` and the KRR opt-in."""
import pytest
import torch

import libskylark_amd as sk
from libskylark_amd import ml
from libskylark_amd.algorithms import operators as OPS
from libskylark_amd.ops import symm


def _tri_operand(n, uplo, dtype=torch.float64, seed=0):
    g = torch.Generator().manual_seed(seed)
    full = torch.rand(n, n, generator=g, dtype=torch.float64) + 0.5
    tri = torch.tril(full) if uplo == "L" else torch.triu(full)
    strict = torch.tril(full, -1) if uplo == "L" else torch.triu(full, 1)
    S = tri + strict.t()
    A = tri.clone()
    other = torch.triu(torch.ones(n, n, dtype=torch.bool), 1) if uplo == "L" else torch.tril(torch.ones(n, n, dtype=torch.bool), -1)
    A[other] = float("nan")
    return A.to(dtype), S


@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("k", [1, 3, 11])
def test_symtriop_cpu_against_fp64(uplo, k):
    n = 97
    A, S = _tri_operand(n, uplo)
    op = OPS.SymTriOp(A, uplo)
    assert op.shape == (n, n) and op.dtype == torch.float64 and not op.distributed
    X = torch.rand(n, k, dtype=torch.float64) + 0.5
    Y = op.matmul(X)
    assert torch.isfinite(Y).all()
    torch.testing.assert_close(Y, S @ X, rtol=1e-13, atol=0)
    assert torch.equal(op.rmatmul(X), Y)
    torch.testing.assert_close(op.matmul(X[:, 0]), S @ X[:, 0], rtol=1e-13, atol=0)


def test_symtriop_f32_and_arguments():
    A, S = _tri_operand(64, "L", torch.float32)
    op = OPS.SymTriOp(A, "l")
    assert op.dtype == torch.float32
    X = torch.rand(64, 2) + 0.5
    torch.testing.assert_close(op.matmul(X).double(), S.float().double() @ X.double(), rtol=1e-5, atol=0)
    with pytest.raises(ValueError):
        OPS.SymTriOp(A, "X")
    with pytest.raises(ValueError):
        OPS.SymTriOp(A[:10], "L")
    assert OPS.as_operator(op) is op


def test_takes_refuses_with_reasons():
    A = torch.zeros(260, 260)
    X = torch.zeros(260, 3)
    assert not symm.takes(A) and not symm.takes(A, X) and not symm.ok(A, X)
    assert "CUDA" in symm._why_not(A) and "CUDA" in symm._why_not(A, X)
    with pytest.raises(ValueError, match="CUDA"):
        symm.symm_tri(A, X)
    assert "f32 or f64" in symm._why_not(A.to(torch.bfloat16))
    assert "1..8" in symm._why_not(A, torch.zeros(260, 0))
    assert "1..8" in symm._why_not(A, torch.zeros(260, 9))
    assert "1..8" not in symm._why_not(A, torch.zeros(260, 8))
    assert "dtype" in symm._why_not(A, X.double())
    B = torch.zeros(258, 259)[:, :258]                  # pitch 259 x 4 B
    assert "16-B" in symm._why_not(B) and not symm.takes(B)
    assert "16-B" in symm._why_not(torch.zeros(256, 260)[:, 1:257])   # base off by 4 B
    assert "row-major" in symm._why_not(A.t()[:130, ::2])
    assert "square" in symm._why_not(torch.zeros(300, 260))
    for bad in (A, A.to(torch.bfloat16), B):
        assert not symm.takes(bad)


def test_krr_opt_in(monkeypatch):
    from libskylark_amd.ml import krr
    g = torch.Generator().manual_seed(5)
    X = torch.randn(200, 4, generator=g, dtype=torch.float64) * 0.7
    Y = torch.sin(X.sum(1, keepdim=True))
    k = ml.Gaussian(4, 1.5)
    p = ml.KrrParams(tolerance=1e-10, iter_lim=500)
    seen = []
    real_cg = krr.cg

    def spy(op, *a, **kw):
        seen.append(type(op))
        return real_cg(op, *a, **kw)

    monkeypatch.setattr(krr, "cg", spy)
    monkeypatch.delenv("SKH_KRR_SYMM", raising=False)
    A0 = ml.faster_kernel_ridge(k, X, Y, 0.05, 100, sk.Context(4), params=p)
    monkeypatch.setenv("SKH_KRR_SYMM", "tri")
    A1 = ml.faster_kernel_ridge(k, X, Y, 0.05, 100, sk.Context(4), params=p)
    assert seen == [OPS.DenseOp, OPS.SymTriOp]
    assert float((A1 - A0).norm() / A0.norm()) < 1e-5
