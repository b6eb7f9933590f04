"""Triangle-reading symmetric product on the GPU (``symm_tri.hip`` through
``ops/symm.py``, ``base.Symm`` and ``SymTriOp``).

Error measure: ``err = max_i |Y_i - Y64_i| / (|S| |X|)_i`` with S the mirrored
triangle and Y64 its fp64 product.  Bounds: f32 ``2^-15`` (512 x 2^-24: one
rounding per product plus an addition chain of at most 510 terms; the kernel's
longest chain is 39), f64 ``2^-44``.  The data are positive (uniform in
(0.5, 1.5)), so nothing cancels: a diagonal counted twice or one missing
mirrored element is at least 8 times the f32 bound.  The triangle that is not
stored holds other numbers (or NaN), so using it fails too.

Measured err on one MI355X over the shape cases: f32 1.0e-8 .. 2.0e-7
(8.6e-8 at n = 2000), f64 0 .. 3.1e-15.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = {torch.float32: 2.0 ** -15, torch.float64: 2.0 ** -44}
_CACHE = {}


def _operand(n, dtype, uplo, other="rand", seed=0):
    """(A, S64): A an n x n view with pitch n rounded up to 16 B plus 16 B
    more; its ``uplo`` triangle is the data, the rest (other triangle, pitch
    padding) is ``other``: different random numbers, zeros or NaN."""
    key = (n, dtype, uplo, other, seed)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(1000 * seed + n)
        per = 16 // torch.empty(0, dtype=dtype).element_size()
        pitch = -(-n // per) * per + per
        full = torch.rand(n, n, generator=g, dtype=torch.float64) + 0.5
        tri = torch.tril(full) if uplo == "L" else torch.triu(full)
        tri = tri.to(dtype).double()
        strict = torch.tril(tri, -1) if uplo == "L" else torch.triu(tri, 1)
        S = tri + strict.t()
        buf = {"rand": torch.rand(n, pitch, generator=g, dtype=torch.float64) + 2.0,
               "zero": torch.zeros(n, pitch, dtype=torch.float64),
               "nan": torch.full((n, pitch), float("nan"), dtype=torch.float64)}[other]
        mask = torch.tril(torch.ones(n, n, dtype=torch.bool)) if uplo == "L" else torch.triu(torch.ones(n, n, dtype=torch.bool))
        buf[:, :n] = torch.where(mask, tri, buf[:, :n])
        _CACHE[key] = (buf.to(dtype).cuda()[:, :n], S.cuda())
    return _CACHE[key]


def _rhs(n, k, dtype, seed=0):
    g = torch.Generator().manual_seed(77 + seed + n + k)
    return (torch.rand(n, k, generator=g, dtype=torch.float64) + 0.5).to(dtype).cuda()


def _err(Y, S, X):
    ref = S @ X.double()
    return float(((Y.double() - ref).abs() / (S.abs() @ X.double().abs())).max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 600, 1000])
def test_shapes_and_tile_edges(n, k, uplo, dtype):
    from libskylark_amd.ops import symm
    A, S = _operand(n, dtype, uplo)
    X = _rhs(n, k, dtype)
    assert symm.ok(A, X)
    for wg in (1, 5, None):
        Y = symm.symm_tri(A, X, uplo=uplo, workgroups=wg)
        assert Y.shape == (n, k) and Y.dtype == dtype
        e = _err(Y, S, X)
        print(f"symm_tri n={n} k={k} {uplo} {dtype} workgroups={wg}: err {e:.3e}")
        assert e <= BOUND[dtype]


def test_n2000_f32():
    from libskylark_amd.ops import symm
    A, S = _operand(2000, torch.float32, "L")
    X = _rhs(2000, 4, torch.float32)
    e = _err(symm.symm_tri(A, X, uplo="L"), S, X)
    print(f"symm_tri n=2000 k=4 L f32: err {e:.3e}")
    assert e <= BOUND[torch.float32]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("n", [257, 600])
def test_poisoned_other_triangle(n, uplo, dtype):
    """NaN in the other triangle and in the pitch padding: the result is finite
    and bit-equal to the one with zeros there (straddling tiles at both sizes,
    a partial last tile)."""
    from libskylark_amd.ops import symm
    An, S = _operand(n, dtype, uplo, "nan")
    Az, _ = _operand(n, dtype, uplo, "zero")
    assert torch.isnan(An).any()
    X = _rhs(n, 3, dtype)
    for wg in (1, None):
        Yn = symm.symm_tri(An, X, uplo=uplo, workgroups=wg)
        Yz = symm.symm_tri(Az, X, uplo=uplo, workgroups=wg)
        assert torch.isfinite(Yn).all()
        assert torch.equal(Yn, Yz)
        assert _err(Yn, S, X) <= BOUND[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_alpha_beta(dtype):
    from libskylark_amd.ops import symm
    n, k = 600, 3
    A, S = _operand(n, dtype, "L")
    X = _rhs(n, k, dtype)
    Y0 = _rhs(n, k, dtype, seed=5)
    Y = Y0.clone()
    out = symm.symm_tri(A, X, uplo="L", alpha=-0.5, beta=0.25, out=Y)
    assert out is Y
    ref = -0.5 * (S @ X.double()) + 0.25 * Y0.double()
    scale = 0.5 * (S.abs() @ X.double().abs()) + 0.25 * Y0.double().abs()
    e = float(((Y.double() - ref).abs() / scale).max())
    print(f"symm_tri alpha/beta {dtype}: err {e:.3e}")
    assert e <= BOUND[dtype]
    # beta == 0: the output is not read
    Yn = torch.full((n, k), float("nan"), dtype=dtype, device="cuda")
    symm.symm_tri(A, X, uplo="L", alpha=1.0, beta=0.0, out=Yn)
    assert torch.isfinite(Yn).all()
    assert torch.equal(Yn, symm.symm_tri(A, X, uplo="L"))
    # an output with its own row pitch
    wide = torch.zeros(n, k + 5, dtype=dtype, device="cuda")
    symm.symm_tri(A, X, uplo="L", out=wide[:, :k])
    assert torch.equal(wide[:, :k], Yn) and not wide[:, k:].any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("uplo", ["L", "U"])
def test_row_blocks(uplo, dtype):
    """n = 600 cut at r0 = 217: each block's Y against the fp64 contribution of
    its trapezoid, their sum against the whole call."""
    from libskylark_amd.ops import symm
    n, k, cut = 600, 3, 217
    A, S = _operand(n, dtype, uplo)
    X = _rhs(n, k, dtype)
    X64 = X.double()
    tri = torch.tril(S) if uplo == "L" else torch.triu(S)
    strict = torch.tril(S, -1) if uplo == "L" else torch.triu(S, 1)
    parts = []
    for r0, r1 in ((0, cut), (cut, n)):
        Y = symm.symm_tri(A[r0:r1], X, uplo=uplo, r0=r0, n=n)
        rows = torch.zeros(n, 1, dtype=torch.float64, device="cuda")
        rows[r0:r1] = 1.0
        ref = (tri * rows) @ X64 + (strict * rows).t() @ X64
        scale = (tri * rows) @ X64.abs() + (strict * rows).t() @ X64.abs()
        ok = scale > 0
        assert not Y[~ok].any()
        e = float(((Y.double() - ref).abs()[ok] / scale[ok]).max())
        print(f"symm_tri rows [{r0}, {r1}) {uplo} {dtype}: err {e:.3e}")
        assert e <= BOUND[dtype]
        parts.append(Y.double())
    whole = symm.symm_tri(A, X, uplo=uplo)
    scale = S.abs() @ X64.abs()
    assert float(((parts[0] + parts[1] - whole.double()).abs() / scale).max()) <= 2 * BOUND[dtype]
    assert _err(parts[0] + parts[1], S, X) <= BOUND[dtype]


def test_deterministic():
    from libskylark_amd.ops import symm
    A, _ = _operand(1000, torch.float32, "L")
    X = _rhs(1000, 8, torch.float32)
    for wg in (5, None):
        assert torch.equal(symm.symm_tri(A, X, uplo="L", workgroups=wg), symm.symm_tri(A, X, uplo="L", workgroups=wg))


def _parent_symm64(side, uplo, alpha, A, B):
    """The full-matrix formula ``base.Symm`` had before the native route, in
    fp64: (product, |S| |B| scale)."""
    A, B = A.double(), B.double()
    tri = torch.tril(A) if uplo == "L" else torch.triu(A)
    S = tri + tri.t() - torch.diag(torch.diagonal(A))
    if side == "L":
        return alpha * (S @ B), abs(alpha) * (S.abs() @ B.abs())
    return alpha * (B @ S), abs(alpha) * (B.abs() @ S.abs())


@pytest.mark.parametrize("uplo", ["L", "U"])
def test_base_symm_sides(uplo):
    from libskylark_amd import base
    n, k = 600, 5
    A, S = _operand(n, torch.float32, uplo, "nan")
    X = _rhs(n, k, torch.float32)
    YL = base.Symm("L", uplo, 1.0, A, X)
    assert YL.shape == (n, k) and _err(YL, S, X) <= BOUND[torch.float32]
    Bt = X.t().contiguous()                       # k x n
    YR = base.Symm("R", uplo, 1.0, A, Bt)
    assert YR.shape == (k, n) and _err(YR.t(), S, X) <= BOUND[torch.float32]
    # alpha, beta and an existing C, both sides
    C0 = _rhs(n, k, torch.float32, seed=9)
    C = C0.clone()
    assert base.Symm("L", uplo, 2.0, A, X, 0.5, C) is C
    ref = 2.0 * (S @ X.double()) + 0.5 * C0.double()
    assert float(((C.double() - ref).abs() / ref.abs()).max()) <= BOUND[torch.float32]
    Ct = C0.t().contiguous()
    assert base.Symm("R", uplo, 2.0, A, Bt, 0.5, Ct) is Ct
    assert float(((Ct.t().double() - ref).abs() / ref.abs()).max()) <= BOUND[torch.float32]


def test_base_symm_column_major():
    from libskylark_amd import base
    n, k = 600, 5
    A, S = _operand(n, torch.float32, "U", "nan")
    X = _rhs(n, k, torch.float32)
    At = A.t()                                    # column-major, lower triangle stored
    assert At.stride(0) == 1
    Y = base.Symm("L", "L", 1.0, At, X)
    assert _err(Y, S, X) <= BOUND[torch.float32]


def test_base_symm_refused_operands_take_the_full_matrix_path():
    from libskylark_amd import base
    from libskylark_amd.ops import symm
    n = 258
    g = torch.Generator().manual_seed(3)
    full = (torch.rand(n, n + 1, generator=g) + 0.5).cuda()
    A = full[:, :n]                               # pitch 259 elements: not 16-B aligned
    assert not symm.takes(A)
    X = _rhs(n, 5, torch.float32)

    def check(side, alpha, A, B):
        # an f32 library product of 258-term dot products of positive numbers:
        # within n x 2^-24 = 1.6e-5 of the formula's fp64 value, below the bound
        ref, scale = _parent_symm64(side, "L", alpha, A, B)
        got = base.Symm(side, "L", alpha, A, B)
        assert got.shape == ref.shape
        assert float(((got.double() - ref).abs() / scale).max()) <= BOUND[torch.float32]

    check("L", 1.5, A, X)
    Ag, _ = _operand(256, torch.float32, "L", "zero")
    X9 = _rhs(256, 9, torch.float32)
    assert symm.takes(Ag) and not symm.takes(Ag, X9)
    check("L", 1.0, Ag, X9)
    check("R", 1.0, Ag, X9.t())


def test_base_symm_allocates_no_square_scratch():
    from libskylark_amd import base
    n, k = 4096, 8
    A = torch.rand(n, n, device="cuda") + 0.5
    X = _rhs(n, k, torch.float32)
    base.Symm("L", "L", 1.0, A, X)                # the cached workspace is allocated here
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    Y = base.Symm("L", "L", 1.0, A, X)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - start
    assert extra < A.nbytes // 4, (extra, A.nbytes)
    S = torch.tril(A.double()) + torch.tril(A.double(), -1).t()
    assert _err(Y, S, X) <= BOUND[torch.float32]


def test_no_square_scratch_from_a_cold_start():
    """Same bound with the workspace included: (16 + 16) slots of n k f32."""
    from libskylark_amd import base
    from libskylark_amd.ops import symm
    n, k = 4096, 8
    A = torch.rand(n, n, device="cuda") + 0.5
    X = _rhs(n, k, torch.float32)
    symm._WS.clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    base.Symm("L", "L", 1.0, A, X)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - start < A.nbytes // 4
    assert symm.workspace_bytes(n, n, k, torch.float32) == 32 * n * k * 4


def test_symtriop_in_cg():
    """SPD system, n = 512, k = 2, upper triangle overwritten with NaN.  The
    matrix is I + G G^T / n-scaled with condition number below 10; cg stops at
    a recursive residual below tol |b|, and in f32 the true residual drifts
    from it by about eps_f32 x cond x iterations (~1e-5), so the fp64 residual
    is held to 2 tol and the solution to cond x 2 tol."""
    from libskylark_amd.algorithms.krylov import KrylovIterParams, cg
    from libskylark_amd.algorithms.operators import SymTriOp
    n, k, tol = 512, 2, 1e-4
    g = torch.Generator().manual_seed(11)
    G = torch.randn(n, 64, generator=g, dtype=torch.float64)
    S = (torch.eye(n, dtype=torch.float64) + G @ G.t() / 64.0).cuda()
    ev = torch.linalg.eigvalsh(S)
    cond = float(ev[-1] / ev[0])
    assert cond < 20
    A = S.float().clone()
    S32 = torch.tril(A.double()) + torch.tril(A.double(), -1).t()
    A[torch.triu(torch.ones(n, n, dtype=torch.bool, device="cuda"), 1)] = float("nan")
    B = torch.randn(n, k, generator=g, dtype=torch.float64).cuda()
    op = SymTriOp(A, "L")
    assert torch.equal(op.matmul(B.float()), op.rmatmul(B.float()))
    Xs, code = cg(op, B.float(), params=KrylovIterParams(tolerance=tol, iter_lim=200))
    assert code == -1
    assert torch.isfinite(Xs).all()
    X64 = torch.linalg.solve(S32, B)
    res = (S32 @ Xs.double() - B).norm(dim=0) / B.norm(dim=0)
    err = (Xs.double() - X64).norm(dim=0) / X64.norm(dim=0)
    print(f"SymTriOp cg: residual {res.tolist()} error {err.tolist()} cond {cond:.2f}")
    assert float(res.max()) <= 2 * tol
    assert float(err.max()) <= cond * 2 * tol
