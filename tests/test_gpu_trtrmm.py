"""One-triangle f64 triangular-triangular product on the GPU (``trtrmm_tri.hip``
through ``ops/trtrmm.py`` and ``base.Trtrmm``), the native ``base.HPDInverse``
chain (Cholesky, TriangularInverse, Trtrmm in one triangle of one buffer) and
the ``SKH_ADMM_INV=native`` opt-in of ``ml/admm.py``.

Product.  ``e = max_ij |C_gpu - C_ref|_ij / (|X|^T |X|)_ij`` over the stored
triangle (uplo U: ``|U| |U|^T``), ``C_ref`` the f64 CPU product of the masked
operand.  Bound: ``e <= 2 (n + 2) 2^-53``: one ``n u`` is the any-order
summation bound on the kernel's dot products of length at most n, the other
is this file's own f64 evaluation.

Matrices, built on the CPU from seeded generators (the two families of
``tests/test_gpu_trtri.py``): (a) the Cholesky factor of ``B B^T + n I``, B
uniform in (-1, 1); (b) the Cholesky factor of the Gaussian-kernel Gram
(sigma = 1) of n uniform points in [0,1]^4 plus ``1e-6 I``.  The Trtrmm operand
is ``X = L^-1`` (``solve_triangular`` against the identity, f64, CPU): what the
chain feeds the kernel, with a wide dynamic range in family (b).  Uplo U: the
transpose.  A is the view ``[:, :n]`` of an n x (n + 1) buffer whose other
triangle and padding hold NaN (column-major: the transposed view of the buffer
that holds the transpose).

Chain.  ``max |Z - Z_ref| <= 8 n u cond_1(A) max |Z_ref|`` with ``Z_ref`` the CPU
f64 ``cholesky_inverse(cholesky(A))``: two forward errors of about ``n u cond``
each, the form of ``tests/test_trtri_base.py``.

Measured on one MI355X (printed per case, ``pytest -s``): product e = 0 .. 0.154
of (n + 1) u over the 88 cases of size, family, uplo and layout (the largest at
n = 3, family (b); 0.025 at most from n = 127 up, 0.0033 at n = 1000; exactly 0
at n = 600 in all eight cases: the kernel adds its products in order of k, one
fused multiply-add each, and there the CPU library's product evidently does the
same; the bound allows 2).  Chain: 0 .. 3.9e-3 of its tolerance (the largest at
n = 3, 1.8e-4 and 3.4e-7 at n = 600); ``_block_inverse`` native against the
default 8.8e-6 of it.
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NAN = float("nan")
F64 = torch.float64
_CACHE = {}
FLIP = {"L": "U", "U": "L"}


def _sizes():
    nb, t = 128, 128          # asserted against sl_trtrmm_tri_block() in test_block_sizes
    return sorted({1, 2, 3, nb - 1, nb, nb + 1, t - 1, t, t + 1, nb + t - 1, nb + t, nb + t + 1, 600, 1000})


def _mask(n, uplo):
    ones = torch.ones(n, n, dtype=torch.bool)
    return torch.tril(ones) if uplo == "L" else torch.triu(ones)


def _sym(fam, n):
    """The symmetric positive definite f64 matrix (CPU), exactly symmetric;
    computed once and never changed."""
    key = ("S", fam, n)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(1000 * (1 + "ab".index(fam)) + n)
        if fam == "a":
            Bm = torch.rand(n, n, generator=g, dtype=F64) * 2 - 1
            A = Bm @ Bm.t() + n * torch.eye(n, dtype=F64)
        else:
            X = torch.rand(n, 4, generator=g, dtype=F64)
            A = torch.exp(-torch.cdist(X, X) ** 2 / 2.0) + 1e-6 * torch.eye(n, dtype=F64)
        _CACHE[key] = torch.tril(A) + torch.tril(A, -1).t()
    return _CACHE[key]


def _factor_inverse(fam, n, uplo):
    """X = L^-1 of the family's Cholesky factor (uplo U: its transpose), zeros
    in the other triangle; with it the f64 reference product and the
    denominator of the measure."""
    key = ("X", fam, n, uplo)
    if key not in _CACHE:
        if ("X0", fam, n) not in _CACHE:
            L = torch.linalg.cholesky(_sym(fam, n))
            _CACHE[("X0", fam, n)] = torch.tril(
                torch.linalg.solve_triangular(L, torch.eye(n, dtype=F64), upper=False))
        X = _CACHE[("X0", fam, n)]
        X = (X if uplo == "L" else X.t()).contiguous()
        ref = X.t() @ X if uplo == "L" else X @ X.t()
        den = X.abs().t() @ X.abs() if uplo == "L" else X.abs() @ X.abs().t()
        _CACHE[key] = (X, ref, den)
    return _CACHE[key]


def _operand(Tm, uplo, major="R", other=NAN):
    """(buffer, A) on the GPU.  A holds Tm's ``uplo`` triangle; the rest of the
    n x (n + 1) buffer holds ``other``.  Row-major: A = buffer[:, :n];
    column-major: A = buffer[:, :n].t(), stride (1, n + 1)."""
    n = Tm.shape[0]
    buf = torch.full((n, n + 1), other, dtype=F64)
    if major == "R":
        buf[:, :n] = torch.where(_mask(n, uplo), Tm, buf[:, :n])
    else:
        buf[:, :n] = torch.where(_mask(n, FLIP[uplo]), Tm.t(), buf[:, :n])
    buf = buf.cuda()
    A = buf[:, :n] if major == "R" else buf[:, :n].t()
    return buf, A


def _stored_in_buf(n, uplo, major):
    m = torch.zeros(n, n + 1, dtype=torch.bool)
    m[:, :n] = _mask(n, uplo if major == "R" else FLIP[uplo])
    return m


def _product_check(fam, n, uplo, major, f=None):
    """One native product on a padded NaN-filled operand; asserts finiteness,
    the bound, the untouched storage and the return value; returns (e, bits)."""
    from libskylark_amd.ops import trtrmm as tm
    X, ref, den = _factor_inverse(fam, n, uplo)
    buf, A = _operand(X, uplo, major)
    assert A.stride() == ((n + 1, 1) if major == "R" else (1, n + 1)) and tm.ok(A)
    before = buf.cpu().view(torch.int64)
    out = (f or tm.trtrmm_tri)(uplo, A)
    assert out is A
    after = buf.cpu()
    stored = _stored_in_buf(n, uplo, major)
    assert torch.isfinite(after[stored]).all()
    # the other triangle and the pad keep their bits
    assert torch.equal(after.view(torch.int64)[~stored], before[~stored])
    Av = after[:, :n] if major == "R" else after[:, :n].t()
    m = _mask(n, uplo)
    assert bool((den[m] > 0).all())
    e = float(((Av - ref).abs() / den)[m].max())
    print(f"trtrmm_tri n={n} {uplo} {major} ({fam}): e {e:.3e} = {e / ((n + 1) * U):.4f} (n + 1) u")
    assert e <= 2 * (n + 2) * U
    return e, after.view(torch.int64)


def test_block_sizes():
    from libskylark_amd.ops import trtrmm as tm
    nb, t = tm.block()
    assert (nb, t) == (128, 128)
    want = sorted({1, 2, 3, nb - 1, nb, nb + 1, t - 1, t, t + 1, nb + t - 1, nb + t, nb + t + 1, 600, 1000})
    assert _sizes() == want == [1, 2, 3, 127, 128, 129, 255, 256, 257, 600, 1000]
    assert [tm.launches(n, nb) for n in (0, 1, 128, 129, 257, 1000)] == [0, 1, 1, 3, 5, 15]


def test_empty():
    from libskylark_amd import base as B
    from libskylark_amd.ops import trtrmm as tm
    A0 = torch.empty(0, 0, dtype=F64, device="cuda")
    assert tm.ok(A0) and tm.trtrmm_tri("L", A0) is A0 and B.Trtrmm("U", A0) is A0 and B.HPDInverse("L", A0) is A0


@pytest.mark.parametrize("fam", ["a", "b"])
@pytest.mark.parametrize("n", _sizes())
def test_shapes_flags_and_layouts(n, fam):
    worst = 0.0
    for uplo, major in itertools.product("LU", "RC"):
        worst = max(worst, _product_check(fam, n, uplo, major)[0])
    print(f"trtrmm_tri n={n} ({fam}): worst e {worst / ((n + 1) * U):.4f} (n + 1) u")


@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("n", [193, 1000])
def test_determinism(n, uplo):
    _, first = _product_check("b", n, uplo, "R")
    _, second = _product_check("b", n, uplo, "R")
    assert torch.equal(first, second)


@pytest.mark.parametrize("uplo,major", [("L", "R"), ("U", "R"), ("U", "C"), ("L", "C")])
def test_base_gives_the_same_bits(uplo, major):
    from libskylark_amd import base as B
    n = 193
    _, native = _product_check("a", n, uplo, major)
    _, through_base = _product_check("a", n, uplo, major, f=B.Trtrmm)
    assert torch.equal(native, through_base)
    # f32 on the GPU: the library way on a masked copy, the other triangle untouched
    X = _factor_inverse("a", n, uplo)[0]
    A32 = torch.where(_mask(n, uplo), X, torch.full_like(X, NAN)).float().cuda()
    out = B.Trtrmm(uplo, A32)
    assert out is A32
    C32 = A32.cpu()
    assert torch.isnan(C32[~_mask(n, uplo)]).all() and torch.isfinite(C32[_mask(n, uplo)]).all()


# ------------------------------------------------------------------ the chain
def _chain_ref(fam, n):
    key = ("Z", fam, n)
    if key not in _CACHE:
        S = _sym(fam, n)
        Z = torch.cholesky_inverse(torch.linalg.cholesky(S))
        kappa = float(torch.linalg.matrix_norm(S, 1) * torch.linalg.matrix_norm(Z, 1))
        _CACHE[key] = (Z, 8 * n * U * kappa * float(Z.abs().max()))
    return _CACHE[key]


def _chain_check(fam, n, uplo, major, f):
    S = _sym(fam, n)
    Z, tol = _chain_ref(fam, n)
    buf, A = _operand(S, uplo, major)
    before = buf.cpu().view(torch.int64)
    out = f(uplo, A)
    assert out is A
    after = buf.cpu()
    stored = _stored_in_buf(n, uplo, major)
    assert torch.isfinite(after[stored]).all()
    assert torch.equal(after.view(torch.int64)[~stored], before[~stored])
    Av = after[:, :n] if major == "R" else after[:, :n].t()
    d = float((Av - Z).abs()[_mask(n, uplo)].max())
    print(f"HPDInverse n={n} {uplo} {major} ({fam}): |Z - Z_ref| {d:.3e} = {d / tol:.3e} of 8 n u cond_1 max|Z|")
    assert d <= tol
    return after.view(torch.int64)


@pytest.mark.parametrize("fam", ["a", "b"])
@pytest.mark.parametrize("n", [3, 65, 193, 600])
def test_hpd_inverse_chain(n, fam):
    from libskylark_amd import base as B

    def by_hand(uplo, A):
        B.Cholesky(uplo, A)
        B.TriangularInverse(uplo, "N", A)
        return B.Trtrmm(uplo, A)

    for uplo, major in itertools.product("LU", "RC"):
        one = _chain_check(fam, n, uplo, major, B.HPDInverse)
        three = _chain_check(fam, n, uplo, major, by_hand)
        assert torch.equal(one, three)


@pytest.mark.parametrize("uplo", ["L", "U"])
def test_hpd_inverse_not_positive_definite(uplo):
    from libskylark_amd import base as B
    from libskylark_amd.base.exceptions import NLAError
    n, k = 193, 100
    S = _sym("a", n).clone()
    S[k, k] = -1.0
    stored = _stored_in_buf(n, uplo, "R")
    buf, A = _operand(S, uplo)
    before = buf.cpu().view(torch.int64)
    with pytest.raises(NLAError, match=f"pivot {k + 1} "):
        B.HPDInverse(uplo, A)
    assert torch.equal(buf.cpu().view(torch.int64)[~stored], before[~stored])
    buf, A = _operand(S, uplo)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert B.HPDInverse(uplo, A, info) is A
    assert int(info.item()) == k + 1
    assert torch.equal(buf.cpu().view(torch.int64)[~stored], before[~stored])


# ------------------------------------------------------------------ BlockADMM
def _admm_matrix(n=600):
    g = torch.Generator().manual_seed(77)
    Z = torch.randn(2 * n, n, generator=g, dtype=F64).cuda()
    C = Z.t() @ Z
    C.diagonal().add_(1.0)
    return C


def test_block_inverse_default_and_opt_in(monkeypatch):
    from libskylark_amd.ml import admm
    from libskylark_amd.ops import trtrmm as tm
    n = 600
    C = _admm_matrix(n)
    monkeypatch.delenv("SKH_ADMM_INV", raising=False)
    want = torch.cholesky_inverse(torch.linalg.cholesky(C)).to(F64)
    got = admm._block_inverse(C.clone(), F64)
    assert torch.equal(got.view(torch.int64), want.view(torch.int64))
    calls = []
    real = tm.trtrmm_tri

    def wrapper(uplo, A):
        calls.append((uplo, tuple(A.shape)))
        return real(uplo, A)

    monkeypatch.setattr(tm, "trtrmm_tri", wrapper)
    admm._block_inverse(C.clone(), F64)
    assert not calls                                   # the default never gets there
    monkeypatch.setenv("SKH_ADMM_INV", "native")
    nat = admm._block_inverse(C.clone(), F64)
    assert calls == [("L", (n, n))]
    assert nat.dtype == F64 and torch.equal(nat.view(torch.int64), nat.t().contiguous().view(torch.int64))
    Cc = C.cpu()
    kappa = float(torch.linalg.matrix_norm(Cc, 1) * torch.linalg.matrix_norm(want.cpu(), 1))
    tol = 8 * n * U * kappa * float(want.abs().max())
    d = float((nat - want).abs().max())
    print(f"_block_inverse native vs default n={n}: {d:.3e} = {d / tol:.3e} of 8 n u cond_1 max|Z|")
    assert d <= tol


def test_admm_trains_the_same_with_the_opt_in(monkeypatch):
    """Plumbing only: the run of tests/test_gpu_normal_eq.py::
    test_admm_one_pass_matches_four_products in f64, 4 iterations."""
    import libskylark_amd as sk
    from libskylark_amd import ml
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    m, d = 20000, 32
    lab = torch.randint(0, 3, (m,), generator=g, device=dev)
    centers = torch.randn(3, d, generator=torch.Generator(device=dev).manual_seed(9), device=dev)
    X = centers[lab] + 0.5 * torch.randn(m, d, generator=g, device=dev)
    obj = {}
    for name in ("default", "native"):
        if name == "native":
            monkeypatch.setenv("SKH_ADMM_INV", "native")
        else:
            monkeypatch.delenv("SKH_ADMM_INV", raising=False)
        kern = ml.Gaussian(d, sigma=float(d) ** 0.5)
        s = ml.BlockADMMSolver("squared", "l2", 1e-3, 512, kernel=kern, NumFeaturePartitions=2, context=sk.Context(5))
        s.set_cache_transform(True)
        s.set_maxiter(4)
        s.one_pass = False
        s.train(X.to(F64), lab.double(), regression=False, log=None, dtype=F64)
        obj[name] = [h["objective"] for h in s.history]
    assert len(obj["default"]) == len(obj["native"]) > 0
    for a, b in zip(obj["default"], obj["native"]):
        assert abs(a - b) <= 1e-3 * abs(a)
