"""CPU side of ``base.Trtrmm`` and ``base.HPDInverse``: the torch fallbacks,
the routing predicate of ``ops/trtrmm.py``, the flag and shape errors and the
``SKH_ADMM_INV`` opt-in of ``ml/admm.py`` on a CPU operand.

Product: ``e = max |C - C_ref|_ij / (|L|^T |L|)_ij`` over the stored triangle
(uplo U: ``|U| |U|^T``) is held to ``2 (n + 2) u`` as on the GPU
(``tests/test_gpu_trtrmm.py``): the any-order summation bound of a dot product
of length at most n, twice (the fallback's product and the f64 reference).
Inverse: ``max |Z - Z_ref| <= 8 n u cond_1(A) max |Z_ref|`` against
``torch.linalg.inv`` of the f64 matrix: two forward errors of about
``n u cond`` each (Higham, Accuracy and Stability of Numerical Algorithms,
section 14.2), the form of ``tests/test_trtri_base.py``; u = 2^-53 (f64),
2^-24 (f32).
"""
import numpy as np
import pytest
import torch

from libskylark_amd import base as B
from libskylark_amd.base.exceptions import DimensionMismatchError, NLAError, UnsupportedBaseOperation
from libskylark_amd.ops import trtrmm as tm

F64 = torch.float64
U_ = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24}
NAN = float("nan")
SIZES = (1, 5, 70)
_CACHE = {}


def _mask(n, uplo):
    ones = torch.ones(n, n, dtype=torch.bool)
    return torch.tril(ones) if uplo == "L" else torch.triu(ones)


def _tri(n, uplo, dtype=F64):
    """A triangular matrix in f64 (exactly representable in ``dtype``), zeros
    in the other triangle."""
    key = ("T", n, uplo, dtype)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(60 + n)
        Tm = torch.tril(torch.rand(n, n, generator=g, dtype=F64) * 2 - 1) + torch.eye(n, dtype=F64)
        Tm = Tm.to(dtype).double()
        _CACHE[key] = (Tm if uplo == "L" else Tm.t()).contiguous()
    return _CACHE[key]


def _spd(n, dtype=F64):
    """A symmetric positive definite matrix in f64, exactly symmetric and
    exactly representable in ``dtype``."""
    key = ("S", n, dtype)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(80 + n)
        Bm = torch.rand(n, n, generator=g, dtype=F64) * 2 - 1
        S = (Bm @ Bm.t() + n * torch.eye(n, dtype=F64)).to(dtype).double()
        _CACHE[key] = torch.tril(S) + torch.tril(S, -1).t()
    return _CACHE[key]


def _operand(M, uplo, dtype=F64, layout="row"):
    """(buffer, view): the view holds M's stored triangle, everything else in
    the buffer (other triangle, pad) is NaN."""
    n = M.shape[0]
    if layout == "col":
        buf = torch.full((n, n + 1), NAN, dtype=dtype)
        A = buf[:, :n].t()
    elif layout == "pitched":
        buf = torch.full((n, n + 3), NAN, dtype=dtype)
        A = buf[:, 1:n + 1]
    else:
        buf = torch.full((n, n), NAN, dtype=dtype)
        A = buf
    A.copy_(torch.where(_mask(n, uplo), M.to(dtype), A))
    return buf, A


def _kept(buf, before, n, uplo, layout, dtype):
    """Everything outside the stored triangle keeps its bits."""
    it = torch.int64 if dtype == F64 else torch.int32
    keep = torch.ones_like(buf, dtype=torch.bool)
    (keep[:, :n].t() if layout == "col" else keep[:, 1:n + 1] if layout == "pitched" else keep)[_mask(n, uplo)] = False
    return torch.equal(buf.view(it)[keep], before.view(it)[keep])


def _check_product(n, uplo, dtype, layout):
    Tm = _tri(n, uplo, dtype)
    buf, A = _operand(Tm, uplo, dtype, layout)
    before = buf.clone()
    assert B.Trtrmm(uplo, A) is A
    assert _kept(buf, before, n, uplo, layout, dtype)
    m = _mask(n, uplo)
    ref = Tm.t() @ Tm if uplo == "L" else Tm @ Tm.t()
    den = Tm.abs().t() @ Tm.abs() if uplo == "L" else Tm.abs() @ Tm.abs().t()
    assert torch.isfinite(A[m]).all() and bool((den[m] > 0).all())
    u = U_[dtype]
    e = float(((A.double() - ref).abs() / den)[m].max())
    print(f"Trtrmm cpu n={n} {uplo} {dtype} {layout}: e {e / ((n + 1) * u):.3f} (n + 1) u")
    assert e <= 2 * (n + 2) * u


def _check_inverse(n, uplo, dtype, layout):
    S = _spd(n, dtype)
    buf, A = _operand(S, uplo, dtype, layout)
    before = buf.clone()
    assert B.HPDInverse(uplo, A) is A
    assert _kept(buf, before, n, uplo, layout, dtype)
    m = _mask(n, uplo)
    assert torch.isfinite(A[m]).all()
    ref = torch.linalg.inv(S)
    u = U_[dtype]
    kappa = float(torch.linalg.matrix_norm(S, 1) * torch.linalg.matrix_norm(ref, 1))
    d, tol = float((A.double() - ref).abs()[m].max()), 8 * n * u * kappa * float(ref.abs().max())
    print(f"HPDInverse cpu n={n} {uplo} {dtype} {layout}: |Z - inv| {d:.3e} tol {tol:.3e}")
    assert d <= tol


def test_exports():
    from libskylark_amd.base import HPDInverse, Trtrmm  # noqa: F401
    from libskylark_amd.ops import trtrmm  # noqa: F401
    assert "Trtrmm" in B.blas.__all__ and "HPDInverse" in B.blas.__all__
    for name in ("_why_not", "takes", "ok", "block", "launches", "trtrmm_tri"):
        assert callable(getattr(trtrmm, name))


@pytest.mark.parametrize("layout", ["row", "col", "pitched"])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("n", SIZES)
def test_fallback_f64(n, uplo, layout):
    _check_product(n, uplo, F64, layout)
    _check_inverse(n, uplo, F64, layout)


@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("n", SIZES)
def test_fallback_f32(n, uplo):
    assert "f64" in tm._why_not(torch.zeros(n, n, dtype=torch.float32))
    _check_product(n, uplo, torch.float32, "row")
    _check_inverse(n, uplo, torch.float32, "row")


def test_fallback_other_views_empty_and_complex():
    # neither stride is one: still done, through the same fallbacks
    n = 5
    for f, M in ((B.Trtrmm, _tri(n, "U")), (B.HPDInverse, _spd(n))):
        big = torch.full((2 * n, 2 * n), NAN, dtype=F64)
        A = big[::2, ::2]
        A.copy_(torch.where(_mask(n, "U"), M, A))
        assert "unit stride" in tm._why_not(A)
        assert f("u", A) is A
        ref = M @ M.t() if f is B.Trtrmm else torch.linalg.inv(M)
        torch.testing.assert_close(torch.triu(A), torch.triu(ref), rtol=1e-13, atol=1e-15)
        assert torch.isnan(A[~_mask(n, "U")]).all() and torch.isnan(big[1::2]).all() and torch.isnan(big[:, 1::2]).all()
    E = torch.zeros(0, 0, dtype=F64)
    assert B.Trtrmm("L", E) is E and B.HPDInverse("U", E) is E
    # complex: L^H L and U U^H, and the inverse of a Hermitian matrix
    g = torch.Generator().manual_seed(3)
    Lc = torch.tril(torch.randn(4, 4, generator=g, dtype=torch.complex128)) + 2 * torch.eye(4, dtype=torch.complex128)
    Z = Lc.clone()
    assert B.Trtrmm("L", Z) is Z
    torch.testing.assert_close(torch.tril(Z), torch.tril(Lc.t().conj() @ Lc), rtol=1e-14, atol=1e-14)
    assert torch.equal(torch.triu(Z, 1), torch.zeros(4, 4, dtype=torch.complex128))
    Z = Lc.t().clone()
    assert B.Trtrmm("U", Z) is Z
    torch.testing.assert_close(torch.triu(Z), torch.triu(Lc.t() @ Lc.conj()), rtol=1e-14, atol=1e-14)
    H = Lc @ Lc.t().conj()
    for uplo in "LU":
        m = _mask(4, uplo)
        Z = torch.where(m, H, torch.full_like(H, complex(NAN, NAN)))
        assert B.HPDInverse(uplo, Z) is Z
        torch.testing.assert_close(Z[m], torch.linalg.inv(H)[m], rtol=1e-12, atol=1e-12)
        assert torch.isnan(Z[~m].real).all()


def test_hpd_inverse_not_positive_definite():
    n, k = 9, 4
    S = _spd(n).clone()
    S[k, k] = -1.0
    buf, A = _operand(S, "L")
    with pytest.raises(NLAError, match=f"pivot {k + 1} "):
        B.HPDInverse("L", A)
    assert torch.isnan(A[~_mask(n, "L")]).all()
    buf, A = _operand(S, "U")
    info = torch.zeros(1, dtype=torch.int32)
    assert B.HPDInverse("U", A, info) is A and int(info.item()) == k + 1
    assert torch.isnan(A[~_mask(n, "U")]).all()
    buf, A = _operand(_spd(n), "U")
    assert B.HPDInverse("U", A, info) is A and int(info.item()) == 0


def test_flag_and_shape_errors():
    A = _tri(5, "L").clone()
    for f in (B.Trtrmm, B.HPDInverse):
        with pytest.raises(ValueError, match="uplo"):
            f("X", A)
        with pytest.raises(DimensionMismatchError):
            f("L", torch.zeros(4, 5, dtype=F64))
        with pytest.raises(DimensionMismatchError):
            f("L", torch.zeros(4, dtype=F64))
        with pytest.raises(DimensionMismatchError):
            f("L", A.to_sparse())
    with pytest.raises(ValueError, match="uplo"):
        tm.trtrmm_tri("X", A)
    with pytest.raises(ValueError, match="CUDA"):          # a good flag (any case) gets as far as the operand
        tm.trtrmm_tri("u", A)
    with pytest.raises(ValueError, match="square"):
        tm.trtrmm_tri("L", A[:, :4])
    assert torch.equal(A, _tri(5, "L"))                    # nothing was touched on the way to an error


def test_dist_star_star_and_vc_star():
    from libskylark_amd.parallel.distmatrix import DistMatrix
    n = 30
    Tm, S = _tri(n, "U"), _spd(n)
    D = DistMatrix.from_global(torch.where(_mask(n, "U"), Tm, torch.full_like(Tm, 7.0)), "STAR_STAR")
    assert B.Trtrmm("U", D) is D
    torch.testing.assert_close(torch.triu(D.local), torch.triu(Tm @ Tm.t()), rtol=1e-13, atol=1e-15)
    assert torch.equal(torch.tril(D.local, -1), torch.tril(torch.full_like(Tm, 7.0), -1))
    D = DistMatrix.from_global(torch.where(_mask(n, "L"), S, torch.full_like(S, 7.0)), "STAR_STAR")
    assert B.HPDInverse("L", D) is D
    torch.testing.assert_close(torch.tril(D.local), torch.tril(torch.linalg.inv(S)), rtol=1e-11, atol=1e-15)
    assert torch.equal(torch.triu(D.local, 1), torch.triu(torch.full_like(S, 7.0), 1))
    for f in (B.Trtrmm, B.HPDInverse):
        with pytest.raises(UnsupportedBaseOperation):
            f("U", DistMatrix.from_global(S.clone(), "VC_STAR"))


def test_why_not_reasons():
    A = torch.zeros(6, 6, dtype=F64)
    # a CPU operand fails on the device alone, and last
    assert tm._why_not(A) == "A must be a CUDA tensor"
    assert not tm.takes(A) and not tm.ok(A)
    assert "dense 2-D" in tm._why_not(A[0])
    assert "dense 2-D" in tm._why_not(A.to_sparse())
    assert "dense 2-D" in tm._why_not(None)
    assert "A must be f64" in tm._why_not(A.float())
    assert "A must be f64" in tm._why_not(A.to(torch.complex128))
    assert "A must be f64" in tm._why_not(torch.zeros(4, 5))          # the dtype comes before the shape
    assert "A must be square" in tm._why_not(A[:, :5])
    assert "A: needs unit stride" in tm._why_not(torch.zeros(12, 12, dtype=F64)[::2, ::2])
    assert "A's rows overlap" in tm._why_not(torch.zeros(11, dtype=F64).as_strided((6, 6), (1, 1)))
    assert "A's rows overlap" in tm._why_not(torch.zeros(40, dtype=F64).as_strided((6, 6), (5, 1)))
    assert "A's rows overlap" in tm._why_not(torch.zeros(40, dtype=F64).as_strided((6, 6), (1, 5)))
    raw = np.zeros(8 * 38, dtype=np.uint8)
    off = (-raw.ctypes.data) % 8 + 4                       # base off by 4 B
    mis = torch.from_numpy(np.frombuffer(raw, dtype=np.float64, count=36, offset=off)).view(6, 6)
    assert mis.data_ptr() % 8 == 4
    assert "A needs an 8-B aligned base" in tm._why_not(mis)
    # the one reason the kernel adds to its siblings': 32-bit byte offsets inside a block
    wide = torch.empty_strided((2, 2), (tm.MAX_PITCH + 1, 1), dtype=F64)
    assert "pitch exceeds" in tm._why_not(wide) and "pitch exceeds" in tm._why_not(wide.t())
    assert tm._why_not(torch.empty_strided((2, 2), (tm.MAX_PITCH, 1), dtype=F64)) == "A must be a CUDA tensor"
    # row-major, column-major, pitched, one-element and empty operands lack only the device
    for X in (torch.zeros(6, 7, dtype=F64)[:, :6], torch.zeros(6, 7, dtype=F64)[:, :6].t(),
              torch.zeros(6, 9, dtype=F64)[:, 2:8], torch.zeros(1, 1, dtype=F64), torch.zeros(0, 0, dtype=F64)):
        assert tm._why_not(X) == "A must be a CUDA tensor"


def test_launches():
    nb = 128                                               # asserted against the kernel in tests/test_gpu_trtrmm.py
    assert tm.launches(0) == 0 and tm.launches(1) == 1 and tm.launches(nb) == 1 and tm.launches(nb + 1) == 3
    assert tm.launches(5000) == 79 and tm.launches(5000, nb=nb) == 79


def test_admm_opt_in_on_cpu_is_the_old_path(monkeypatch):
    from libskylark_amd.ml import admm
    C = _spd(70)
    monkeypatch.delenv("SKH_ADMM_INV", raising=False)
    want = admm._block_inverse(C.clone(), F64)
    assert torch.equal(want.view(torch.int64),
                       torch.cholesky_inverse(torch.linalg.cholesky(C)).to(F64).view(torch.int64))
    monkeypatch.setenv("SKH_ADMM_INV", "native")
    got = admm._block_inverse(C.clone(), F64)
    assert torch.equal(got.view(torch.int64), want.view(torch.int64))
    got32 = admm._block_inverse(C.clone(), torch.float32)
    assert got32.dtype == torch.float32 and torch.equal(got32, want.float())
