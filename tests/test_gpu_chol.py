"""One-triangle f64 Cholesky on the GPU (``chol_tri.hip`` through
``ops/cholesky.py``, ``base.Cholesky`` / ``CholeskySolveAfter`` / ``HPDSolve``
and the ``SKH_KRR_CHOL=native`` opt-in of ``ml/krr.py``).

Error measure: with F the computed factor (L for ``'L'``, U^T for ``'U'``),
``e = max |A - F F^T|_ij / (|F| |F|^T)_ij`` over the stored triangle,
evaluated in f64 on the CPU.  Bound: ``e <= 2 (n + 2) 2^-53``.  One
``(n + 1) u`` is Higham's componentwise bound for Cholesky with
substitution-based solves in any summation order (Accuracy and Stability of
Numerical Algorithms, Thm 10.3); the other share is this file's own f64
evaluation of ``F F^T``.

Matrices, built on the CPU from a seeded generator:
(a) ``B B^T + n I``, B uniform in (-1, 1): condition about 2.3, a dropped or
    doubled trailing tile costs O(1);
(b) the Gaussian-kernel Gram (sigma = 1) of n uniform points in [0,1]^4 plus
    ``1e-6 I``: condition 4e7 (n = 65) .. 4e8 (n = 600), the case an
    inverse-multiplying panel solve fails.
Every operand is the view ``[:, :n]`` of an n x (n + 1) buffer (odd pitch);
the triangle that is not stored and the padding column hold other random
numbers or NaN.

Measured e on one MI355X over the shape cases: 1.5e-16 .. 6.3e-15, that is
0.034 .. 0.69 of (n + 1) u (the bound allows 2).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
_CACHE = {}


def _block():
    from libskylark_amd.ops import cholesky as ch
    if "blk" not in _CACHE:
        _CACHE["blk"] = ch.block()
    return _CACHE["blk"]


def _sizes():
    nb, t = 64, 128           # asserted against sl_chol_tri_block() in test_block_sizes
    return sorted({1, 2, 3, nb - 1, nb, nb + 1, 2 * nb + 1, t - 1, t, t + 1,
                   nb + t - 1, nb + t, nb + t + 1, 600, 1000})


def _mask(n, uplo):
    ones = torch.ones(n, n, dtype=torch.bool)
    return torch.tril(ones) if uplo == "L" else torch.triu(ones)


def _matrix(fam, n):
    """The full symmetric f64 test matrix (CPU), computed once and never changed."""
    key = ("A", fam, n)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(1000 * (1 + "ab".index(fam)) + n)
        if fam == "a":
            Bm = torch.rand(n, n, generator=g, dtype=torch.float64) * 2 - 1
            A = Bm @ Bm.t() + n * torch.eye(n, dtype=torch.float64)
        else:
            X = torch.rand(n, 4, generator=g, dtype=torch.float64)
            A = torch.exp(-torch.cdist(X, X) ** 2 / 2.0) + 1e-6 * torch.eye(n, dtype=torch.float64)
        _CACHE[key] = torch.tril(A) + torch.tril(A, -1).t()
    return _CACHE[key]


def _operand(A64, uplo, other="rand"):
    """A fresh n x (n + 1) buffer on the GPU; its view [:, :n] holds A64's
    ``uplo`` triangle, everything else is ``other``."""
    n = A64.shape[0]
    g = torch.Generator().manual_seed(5 + n)
    buf = {"rand": torch.rand(n, n + 1, generator=g, dtype=torch.float64) + 3.0,
           "zero": torch.zeros(n, n + 1, dtype=torch.float64),
           "nan": torch.full((n, n + 1), float("nan"), dtype=torch.float64)}[other]
    buf[:, :n] = torch.where(_mask(n, uplo), A64, buf[:, :n])
    return buf.cuda()


def _factor(Aout, uplo):
    Ac = Aout.detach().cpu()
    return torch.tril(Ac) if uplo == "L" else torch.triu(Ac).t()


def _err(A64, F):
    m = torch.tril(torch.ones_like(A64, dtype=torch.bool))
    return float(((A64 - F @ F.t()).abs() / (F.abs() @ F.abs().t()))[m].max())


def test_block_sizes():
    assert _block() == (64, 128)


def test_empty():
    from libskylark_amd import base as B
    from libskylark_amd.ops import cholesky as ch
    A = torch.empty(0, 0, dtype=torch.float64, device="cuda")
    info = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    assert ch.ok(A)
    assert B.Cholesky("L", A, info) is A and int(info) == 0
    assert B.Cholesky("U", A) is A


@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("n,fam", [(n, f) for n in _sizes() for f in "ab" if f == "a" or n >= 3])
def test_shapes_and_edges(n, fam, uplo):
    from libskylark_amd import base as B
    from libskylark_amd.ops import cholesky as ch
    A64 = _matrix(fam, n)
    A = _operand(A64, uplo)[:, :n]
    assert ch.ok(A)
    out = B.Cholesky(uplo, A)
    assert out is A
    e = _err(A64, _factor(A, uplo))
    print(f"chol_tri n={n} {uplo} ({fam}): e {e:.3e} = {e / ((n + 1) * U):.3f} (n + 1) u")
    assert e <= 2 * (n + 2) * U


@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("n", [65, 200])
def test_untouched_storage_and_determinism(n, uplo):
    from libskylark_amd import base as B
    A64 = _matrix("b", n)
    buf = _operand(A64, uplo, "nan")
    before = buf.view(torch.int64).clone()
    B.Cholesky(uplo, buf[:, :n])
    after = buf.view(torch.int64)
    keep = torch.ones(n, n + 1, dtype=torch.bool)
    keep[:, :n] = ~_mask(n, uplo)
    keep = keep.cuda()
    assert torch.equal(after[keep], before[keep])
    assert torch.isnan(buf[keep]).all()
    assert torch.isfinite(buf[~keep]).all()
    bz = _operand(A64, uplo, "zero")
    B.Cholesky(uplo, bz[:, :n])
    assert torch.equal(bz.view(torch.int64)[~keep], after[~keep])
    b2 = _operand(A64, uplo, "nan")
    B.Cholesky(uplo, b2[:, :n])
    assert torch.equal(b2.view(torch.int64), after)


def test_column_major():
    from libskylark_amd import base as B
    n = 200
    A64 = _matrix("b", n)
    bu = _operand(A64, "U", "nan")
    B.Cholesky("U", bu[:, :n])
    bc = _operand(A64, "U", "nan")
    Ac = bc[:, :n].t()                      # column-major; its lower triangle is the data
    assert Ac.stride() == (1, n + 1)
    out = B.Cholesky("L", Ac)
    assert out is Ac
    m = _mask(n, "L").cuda()
    assert torch.equal(Ac[m].view(torch.int64), bu[:, :n].t()[m].view(torch.int64))
    assert _err(A64, _factor(Ac, "L")) <= 2 * (n + 2) * U


@pytest.mark.parametrize("fam", ["a", "b"])
@pytest.mark.parametrize("uplo", ["L", "U"])
def test_against_library(uplo, fam):
    from libskylark_amd import base as B
    n = 600
    A64 = _matrix(fam, n)
    A = _operand(A64, uplo)[:, :n]
    B.Cholesky(uplo, A)
    F = _factor(A, uplo)
    Ft = torch.linalg.cholesky(A64.cuda()).cpu()
    e, et = _err(A64, F), _err(A64, Ft)
    d = float((F - Ft).abs().max() / Ft.abs().max())
    print(f"chol_tri n={n} {uplo} ({fam}): e {e:.3e}, library {et:.3e}; max |F - F_lib| / |F_lib|_max {d:.3e}")
    assert e <= 2 * et + (n + 2) * U


@pytest.mark.parametrize("kind", ["negative", "nan"])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("pi", [0, 1, 2, 3])
def test_failure_index(pi, uplo, kind):
    from libskylark_amd import base as B
    from libskylark_amd.base.exceptions import NLAError
    nb = _block()[0]
    n = 2 * nb + 10
    p = [0, nb - 1, nb, 2 * nb + 3][pi]
    L0 = torch.linalg.cholesky(_matrix("a", n))
    good = L0 @ L0.t()
    good = torch.tril(good) + torch.tril(good, -1).t()
    bad = good.clone()
    bad[p, p] = bad[p, p] - (L0[p, p] ** 2 + 1) if kind == "negative" else float("nan")
    info = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    A = _operand(bad, uplo)[:, :n]
    out = B.Cholesky(uplo, A, info)
    assert out is A and int(info) == p + 1
    with pytest.raises(NLAError, match=rf"pivot {p + 1} "):
        B.Cholesky(uplo, _operand(bad, uplo)[:, :n])
    # nothing carries over: a good matrix next, both ways of reporting
    A = _operand(good, uplo)[:, :n]
    B.Cholesky(uplo, A)
    assert _err(good, _factor(A, uplo)) <= 2 * (n + 2) * U
    A = _operand(good, uplo)[:, :n]
    B.Cholesky(uplo, A, info)
    assert int(info) == 0 and _err(good, _factor(A, uplo)) <= 2 * (n + 2) * U


def _resid(A64, F, X, Bm):
    return float(((A64 @ X - Bm).abs() / (F.abs() @ (F.abs().t() @ X.abs()))).max())


@pytest.mark.parametrize("fam", ["a", "b"])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("t", [1, 5])
def test_hpdsolve_and_solve_after(t, uplo, fam):
    from libskylark_amd import base as B
    n = 600
    A64 = _matrix(fam, n)
    g = torch.Generator().manual_seed(11 + t)
    Bm = torch.randn(n, t, generator=g, dtype=torch.float64)
    A = _operand(A64, uplo, "nan")[:, :n]
    X = Bm.cuda()
    out = B.HPDSolve(uplo, "N", A, X)
    assert out is X and torch.isfinite(X).all()
    Lt = torch.linalg.cholesky(A64.cuda())
    Xt = torch.cholesky_solve(Bm.cuda(), Lt)
    r = _resid(A64, _factor(A, uplo), X.cpu(), Bm)
    rt = _resid(A64, Lt.cpu(), Xt.cpu(), Bm)
    print(f"HPDSolve n={n} t={t} {uplo} ({fam}): r {r:.3e}, library {rt:.3e}")
    assert r <= 2 * rt + (n + 2) * 2.0 ** -52
    # A is the factor now, NaN in its other triangle: the same solution from zeros there
    Fz = torch.zeros(n, n + 1, dtype=torch.float64, device="cuda")[:, :n]      # A's pitch
    Fz.copy_(torch.where(_mask(n, uplo).cuda(), A, Fz))
    X1, X2 = Bm.cuda(), Bm.cuda()
    B.CholeskySolveAfter(uplo, "N", A, X1)
    B.CholeskySolveAfter(uplo, "N", Fz, X2)
    assert torch.isfinite(X1).all()
    assert torch.equal(X1.view(torch.int64), X2.view(torch.int64))
    assert torch.equal(X1.view(torch.int64), X.view(torch.int64))


@pytest.mark.parametrize("gram", ["", "syrk"])
def test_krr_opt_in(monkeypatch, gram):
    from libskylark_amd.ml import krr
    g = torch.Generator().manual_seed(21)
    Z = torch.randn(2000, 256, generator=g).cuda()
    Y = torch.randn(2000, 3, generator=g).cuda()
    monkeypatch.setenv("SKH_KRR_GRAM", gram)
    monkeypatch.delenv("SKH_KRR_CHOL", raising=False)
    seen = []
    real = torch.linalg.cholesky

    def spy(C, *a, **kw):
        seen.append(C._base.detach().cpu().clone())     # [Z^T Z + lam I | Z^T Y]
        return real(C, *a, **kw)

    monkeypatch.setattr(torch.linalg, "cholesky", spy)
    W0 = krr._ridge(Z, Y, 1e-2)
    monkeypatch.setattr(torch.linalg, "cholesky", real)
    assert len(seen) == 1 and seen[0].shape == (256, 259)
    Wc = torch.cholesky_solve(seen[0][:, 256:], torch.linalg.cholesky(seen[0][:, :256]))
    monkeypatch.setenv("SKH_KRR_CHOL", "native")
    W1 = krr._ridge(Z, Y, 1e-2)
    d1 = float((W1 - W0).norm() / W0.norm())
    d0 = float((W0.cpu() - Wc).norm() / Wc.norm())
    print(f"_ridge 2000 x 256, t = 3, SKH_KRR_GRAM={gram!r}: native vs default {d1:.3e}, default vs CPU {d0:.3e}")
    assert d1 <= 8 * d0 + 1e-13
