"""One-triangle f64 rank-k update on the GPU (``herk_tri.hip`` through
``ops/herk.py`` and ``base.Herk``), the Gram-to-weights chain in one triangle
and the ``SKH_KRR_GRAM=syrk`` opt-in of ``ml/krr.py`` on its f64 branch.

Measure and bound (``herk_reference``): ``e = max |C_gpu - ref| / den`` over the
stored triangle against the long-double ``ref = alpha op(A) op(A)^T + beta C0``,
``den = |alpha| |op(A)| |op(A)|^T + |beta| |C0|``; ``e <= (K + 4) u``, exact where
``den == 0``.

Operands, built on the CPU from seeded generators.  A is a view into a larger
NaN-filled buffer (the pad of every row, and the rows / columns just past its
last); with ``alpha == 0`` A itself is all NaN.  C is the ``[:, :s]`` view of an
s x (s + 1) NaN-filled buffer (column-major: the transposed view of the buffer
that holds the transpose): its other triangle and pad hold NaN, and with
``beta == 0`` the stored triangle does too.  Families: (a) uniform in (-1, 1);
(b) uniform times ``2^j``, j uniform in -20 .. 20 per entry.

Every case asserts the bound, finiteness of the stored triangle, bit equality
of everything outside it (viewed as int64), that the return value is C, and
that a second call on a fresh copy gives the same bits.

Measured on one MI355X (printed per case, ``pytest -s``; 329 calls checked):
the largest ``e / ((K + 4) u)`` per K over all cases: K = 1 0.385, K = 3 0.477
(s = 300, orient N, uplo U, family (b), alpha -2, beta 1: the largest of the
file), K = 31 0.301, K = 32 0.262, K = 33 0.300, K = 64 0.157, K = 100 0.153,
K = 257 0.083, K = 8197 (the plan's 257 splits on 256 CUs) 0.0017; exactly 0
for alpha == 0 and K == 0.  Per size the worst runs from 0.11 (s = 1) to 0.48
(s = 300); the bound allows 1.  Chain: 1.6e-4 of its tolerance (cond_1 = 150).
KRR opt-in: relative difference of the weights 2.3e-13 against the 1e-10
allowed.
"""
import itertools

import numpy as np
import pytest
import torch

import herk_reference as HR

pytestmark = pytest.mark.gpu

NAN = float("nan")
F64 = torch.float64
FLIP = {"L": "U", "U": "L"}
SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
KS = (1, 3, 31, 32, 33, 64, 100, 257)
SCALARS = ((1.0, 0.0), (0.5, 0.25), (-2.0, 1.0))
_CACHE = {}
_WORST = {}


def _matrix(fam, rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    M = torch.rand(rows, cols, generator=g, dtype=F64) * 2 - 1
    if fam == "b":
        M = M * torch.exp2(torch.randint(-20, 21, (rows, cols), generator=g).to(F64))
    return M


def _inputs(fam, s, K):
    """(P, C0): op(A) of order s x K and the s x s start of C, on the CPU;
    computed once and never changed."""
    key = (fam, s, K)
    if key not in _CACHE:
        _CACHE[key] = (_matrix(fam, s, K, 100000 * (1 + "ab".index(fam)) + 1000 * s + K),
                       _matrix(fam, s, s, 7000000 + 1000 * s + K))
    return _CACHE[key]


def _reference(fam, s, K, alpha, beta):
    key = (fam, s, K, alpha, beta)
    if key not in _CACHE:
        P, C0 = _inputs(fam, s, K)
        _CACHE[key] = HR.reference("N", alpha, P.numpy(), beta, C0.numpy())
    return _CACHE[key]


def _a_operand(P, orient, major, poison):
    """A on the GPU with op(A) = P, as a view into a NaN-filled buffer with two
    rows and three columns to spare."""
    M = P if orient == "N" else P.t()
    if poison:
        M = torch.full_like(M, NAN)
    Ml = M if major == "R" else M.t()
    buf = torch.full((Ml.shape[0] + 2, Ml.shape[1] + 3), NAN, dtype=F64)
    buf[:Ml.shape[0], :Ml.shape[1]] = Ml
    v = buf.cuda()[:Ml.shape[0], :Ml.shape[1]]
    return v if major == "R" else v.t()


def _c_view(buf, s, major):
    return buf[:, :s] if major == "R" else buf[:, :s].t()


def _check(fam, s, K, orient, uplo, amaj, cmaj, alpha, beta, splits=None, f=None):
    """One call on padded NaN-filled operands; returns (e, bits of C's buffer)."""
    from libskylark_amd.ops import herk
    P, C0 = _inputs(fam, s, K)
    ref, den = _reference(fam, s, K, alpha, beta)
    m = torch.from_numpy(HR.tri_mask(s, uplo))
    bits = []
    for _ in range(2):                        # the second call on a fresh copy
        A = _a_operand(P, orient, amaj, alpha == 0.0)
        host = torch.full((s, s + 1), NAN, dtype=F64)
        if beta != 0.0:
            Cv = _c_view(host, s, cmaj)
            Cv[m] = C0[m]
        before = host.view(torch.int64).clone()
        buf = host.cuda()
        C = _c_view(buf, s, cmaj)
        assert herk.ok(A, C, trans=orient != "N")
        if f is not None:
            out = f(uplo, orient, alpha, A, beta, C)
        else:
            out = herk.herk_tri(uplo, orient, alpha, A, beta, C, splits=splits)
        assert out is C
        after = buf.cpu()
        stored = torch.zeros(s, s + 1, dtype=torch.bool)
        stored[:, :s] = m if cmaj == "R" else m.t()
        assert torch.isfinite(after[stored]).all()
        # the other triangle and the pad keep their bits
        assert torch.equal(after.view(torch.int64)[~stored], before[~stored])
        bits.append(after.view(torch.int64))
    assert torch.equal(bits[0], bits[1])
    e = HR.measure(_c_view(after, s, cmaj).numpy(), ref, den, uplo)
    rel = e / HR.bound(K)
    tag = f"{'base.Herk' if f else 'herk_tri'} s={s} K={K} {orient}{uplo} A:{amaj} C:{cmaj} ({fam}) " \
          f"alpha={alpha} beta={beta} splits={splits}"
    print(f"{tag}: e {e:.3e} = {rel:.4f} (K + 4) u")
    _WORST[K] = max(_WORST.get(K, 0.0), rel)
    assert e <= HR.bound(K), tag
    return e, bits[0]


def _cases(s):
    """Sixteen cases for one s: every K twice, the five two-valued factors
    (orient, uplo, A's layout, C's layout, family) and the scalars from a
    counter that runs through all their combinations."""
    si = SIZES.index(s)
    out = []
    for ki, K in enumerate(KS):
        for v in range(2):
            n = 16 * si + 2 * ki + v
            b = (11 * n) % 32
            out.append((K, "NT"[b & 1], "LU"[b >> 1 & 1], "RC"[b >> 2 & 1], "RC"[b >> 3 & 1], "ab"[b >> 4 & 1],
                        SCALARS[n % 3]))
    return out


def test_block_sizes_and_coverage():
    from libskylark_amd.ops import herk
    t, kh = herk.block()
    assert (t, kh) == (128, 32)
    assert SIZES == (1, 2, 3, t // 2 - 1, t // 2, t // 2 + 1, t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1, 300)
    assert KS == (1, 3, kh - 1, kh, kh + 1, 2 * kh, 100, 8 * kh + 1)
    total = 0
    for s in SIZES:
        cs = _cases(s)
        total += len(cs)
        for col, want in enumerate((set(KS), set("NT"), set("LU"), set("RC"), set("RC"), set("ab"), set(SCALARS))):
            assert {c[col] for c in cs} == want, (s, col)
    assert total == 208
    # every pair of values of two different two-valued factors occurs somewhere
    every = [c for s in SIZES for c in _cases(s)]
    for i, j in itertools.combinations(range(1, 6), 2):
        assert len({(c[i], c[j]) for c in every}) == 4


@pytest.mark.parametrize("s", SIZES)
def test_sizes_flags_and_layouts(s):
    worst = 0.0
    for K, orient, uplo, amaj, cmaj, fam, (alpha, beta) in _cases(s):
        e, _ = _check(fam, s, K, orient, uplo, amaj, cmaj, alpha, beta)
        worst = max(worst, e / HR.bound(K))
    print(f"herk_tri s={s}: worst e {worst:.4f} (K + 4) u")


@pytest.mark.parametrize("alpha,beta,K", [(1.0, 0.0, 100), (0.5, 0.25, 100), (-2.0, 1.0, 100), (0.0, 0.5, 100),
                                          (0.0, 0.0, 100), (1.0, 0.0, 0), (0.5, 0.25, 0)])
def test_scalars(alpha, beta, K):
    """alpha == 0 (A all NaN) and K == 0 leave beta C, or zeros."""
    for s, orient, uplo, amaj, cmaj, fam in ((129, "T", "L", "R", "R", "a"), (65, "N", "U", "C", "R", "b"),
                                             (300, "N", "L", "R", "C", "b"), (3, "T", "U", "C", "C", "a")):
        e, bits = _check(fam, s, K, orient, uplo, amaj, cmaj, alpha, beta)
        if alpha == 0.0 or K == 0:
            assert e == 0.0                 # one product by beta, exactly rounded: the reference's own value
            if beta == 0.0:
                m = torch.zeros(s, s + 1, dtype=torch.bool)
                m[:, :s] = torch.from_numpy(HR.tri_mask(s, uplo if cmaj == "R" else FLIP[uplo]))
                assert not bits[m].any()    # +0.0


@pytest.mark.parametrize("K", [33, 100, 257])
@pytest.mark.parametrize("splits", [1, 2, 3, 7, 1000])
def test_forced_splits(splits, K):
    from libskylark_amd.ops import herk
    kh = herk.block()[1]
    S = min(splits, -(-K // kh))
    for s, orient, uplo, amaj, cmaj, fam, (alpha, beta) in (
            (129, "T", "L", "R", "R", "b", SCALARS[1]), (65, "N", "U", "R", "C", "a", SCALARS[0]),
            (257, "T", "U", "C", "R", "a", SCALARS[2]), (300, "N", "L", "C", "C", "b", SCALARS[1])):
        assert herk.launches(s, K, splits) == (1 if S == 1 else 2)
        _check(fam, s, K, orient, uplo, amaj, cmaj, alpha, beta, splits=splits)


def test_tall_takes_the_plan():
    from libskylark_amd.ops import herk
    s, K = 130, 8197
    tiles, S = herk.plan(s, K)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert (tiles, S) == herk.plan(s, K, cus) and tiles == 3 and S > 1
    assert S == min(4 * cus // tiles, -(-K // 32))
    assert herk.launches(s, K) == 2 and herk.launches(s, K, 1) == 1
    print(f"herk_tri plan s={s} K={K} on {cus} CUs: {tiles} tiles x {S} splits")
    _check("a", s, K, "T", "L", "R", "R", 1.0, 0.0)
    _check("b", s, K, "N", "U", "R", "R", 0.5, 0.25)


def test_empty():
    from libskylark_amd import base as B
    from libskylark_amd.ops import herk
    A = torch.full((0, 5), NAN, dtype=F64, device="cuda")
    C0 = torch.empty(0, 0, dtype=F64, device="cuda")
    assert herk.ok(A, C0, trans=False) and herk.herk_tri("L", "N", 1.0, A, 0.0, C0) is C0
    assert B.Herk("U", "N", 1.0, A, 0.5, C0) is C0
    C = herk.herk_tri("L", "T", 1.0, A)                   # K == 0: zeros
    assert tuple(C.shape) == (5, 5) and not C.view(torch.int64).any()
    A = torch.rand(40, 7, dtype=F64, device="cuda")
    C = herk.herk_tri("U", "T", 1.0, A)                   # C=None: zeros outside the triangle
    assert torch.equal(torch.tril(C, -1), torch.zeros_like(C)) and bool((torch.diagonal(C) > 0).all())


# ------------------------------------------------------------------ base.Herk
@pytest.fixture
def spy(monkeypatch):
    from libskylark_amd.ops import herk
    calls = []
    real = herk.herk_tri

    def wrapper(uplo, orient, alpha, A, beta=0.0, C=None, **kw):
        calls.append((uplo, orient, tuple(A.shape), None if C is None else C.dtype))
        return real(uplo, orient, alpha, A, beta, C, **kw)

    monkeypatch.setattr(herk, "herk_tri", wrapper)
    return calls


@pytest.mark.parametrize("orient,uplo,amaj,cmaj", [("N", "L", "R", "R"), ("T", "U", "R", "C"), ("T", "L", "C", "R"),
                                                   ("N", "U", "C", "C")])
def test_base_gives_the_same_bits(spy, orient, uplo, amaj, cmaj):
    from libskylark_amd import base as B
    _, through_base = _check("a", 193, 100, orient, uplo, amaj, cmaj, 0.5, 0.25, f=B.Herk)
    assert len(spy) == 2 and spy[0][:2] == (uplo, orient) and spy[0][3] == F64
    _, native = _check("a", 193, 100, orient, uplo, amaj, cmaj, 0.5, 0.25)
    assert torch.equal(native, through_base)


def test_base_routing(spy):
    from libskylark_amd import base as B
    from libskylark_amd.parallel.comm import Comm
    from libskylark_amd.parallel.distmatrix import DistMatrix
    g = torch.Generator().manual_seed(4)
    Ah = torch.rand(200, 70, generator=g, dtype=F64) * 2 - 1
    A = Ah.cuda()
    low = torch.tril(torch.ones(70, 70, dtype=torch.bool))
    want = torch.from_numpy(HR.reference("T", 1.0, Ah.numpy())[0].astype(np.float64))
    tol = HR.bound(200) * float((Ah.abs().t() @ Ah.abs()).max())
    # C=None and Syrk, the same entry point
    assert B.Syrk is B.Herk
    C = B.Syrk("L", "T", 1.0, A)
    assert spy == [("L", "T", (200, 70), F64)]
    assert torch.equal(torch.triu(C, 1), torch.zeros_like(C))
    assert float((C.cpu() - want)[low].abs().max()) <= tol
    # a one-rank [VC,*] matrix with orient T
    D = DistMatrix.from_global(A, "VC_STAR", Comm.single())
    G = B.Herk("L", "T", 1.0, D)
    assert len(spy) == 2 and spy[1][:3] == ("L", "T", (200, 70))
    assert torch.equal(G.view(torch.int64), C.view(torch.int64))
    del spy[:]
    # not the kernel's: f32 A, f64 A with an f32 C, a view with neither stride 1
    C32 = B.Herk("L", "T", 1.0, A.float())
    assert C32.dtype == torch.float32 and float((C32.double().cpu() - want)[low].abs().max()) <= 1e-4
    Cf = torch.zeros(70, 70, dtype=torch.float32, device="cuda")
    assert B.Herk("L", "T", 1.0, A, 0.0, Cf) is Cf
    assert float((Cf.double().cpu() - want)[low].abs().max()) <= 1e-4 and not Cf.triu(1).any()
    wide = torch.zeros(400, 140, dtype=F64, device="cuda")
    wide[::2, ::2] = A
    Cs = B.Herk("L", "T", 1.0, wide[::2, ::2])
    assert float((Cs.cpu() - want)[low].abs().max()) <= tol and not Cs.triu(1).any()
    assert spy == []


# ------------------------------------------------------------------ the chain
def test_gram_to_weights_in_one_triangle():
    """Herk, lam on the diagonal, HPDSolve: the upper triangle of G holds NaN
    from start to finish.  ``|W - W_ref| <= 8 s u cond_1(G) max |W_ref|``, the
    form of tests/test_gpu_trtrmm.py's chain check, against the f64 CPU normal
    equations."""
    from libskylark_amd import base as B
    n, s, t, lam = 400, 150, 3, 1e-2
    g = torch.Generator().manual_seed(12)
    Z = torch.rand(n, s, generator=g, dtype=F64) * 2 - 1
    Y = torch.rand(n, t, generator=g, dtype=F64) * 2 - 1
    Gh = Z.t() @ Z + lam * torch.eye(s, dtype=F64)
    Wref = torch.cholesky_solve(Z.t() @ Y, torch.linalg.cholesky(Gh))
    kappa = float(torch.linalg.matrix_norm(Gh, 1) * torch.linalg.matrix_norm(torch.linalg.inv(Gh), 1))
    tol = 8 * s * HR.U * kappa * float(Wref.abs().max())
    buf = torch.full((s, s + 1), NAN, dtype=F64, device="cuda")
    G = buf[:, :s]
    Zd = Z.cuda()
    assert B.Herk("L", "T", 1.0, Zd, 0.0, G) is G
    G.diagonal().add_(lam)
    Bm = Zd.t() @ Y.cuda()
    B.HPDSolve("L", "N", G, Bm)
    after = buf.cpu()
    up = torch.zeros(s, s + 1, dtype=torch.bool)
    up[:, :s] = torch.triu(torch.ones(s, s, dtype=torch.bool), 1)
    up[:, s] = True
    assert torch.isnan(after[up]).all() and torch.isfinite(after[~up]).all()
    d = float((Bm.cpu() - Wref).abs().max())
    print(f"Herk + HPDSolve {n} x {s}: |W - W_ref| {d:.3e} = {d / tol:.3e} of 8 s u cond_1 max|W| (cond_1 {kappa:.3e})")
    assert d <= tol


# ------------------------------------------------------------------ KRR
def test_krr_f64_gram_opt_in(spy, monkeypatch):
    """The problem of tests/test_gpu_syrk.py::test_krr_gram_syrk_opt_in with the
    f64 Gram: with SKH_KRR_GRAM=syrk it comes from herk_tri, and the weights
    agree with the default's to 1e-10 relative (both are f64 Grams; summation
    order times a condition number of about 1e4 at lambda = 1e-2)."""
    import libskylark_amd as sk
    from libskylark_amd import ml
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(5)
    X = torch.randn(2000, 16, generator=g, device=dev)
    Y = torch.sin(X[:, :1]) + 0.01 * torch.randn(2000, 1, generator=g, device=dev)
    k = ml.Gaussian(16, sigma=4.0)
    monkeypatch.setenv("SKH_KRR_F64_GRAM", "1")
    monkeypatch.delenv("SKH_KRR_CHOL", raising=False)
    monkeypatch.delenv("SKH_KRR_GRAM", raising=False)
    _, W64 = ml.approximate_kernel_ridge(k, X, Y, 1e-2, 256, context=sk.Context(3))
    assert spy == []
    monkeypatch.setenv("SKH_KRR_GRAM", "syrk")
    _, W = ml.approximate_kernel_ridge(k, X, Y, 1e-2, 256, context=sk.Context(3))
    assert spy == [("L", "T", (2000, 256), F64)]
    rel = float((W.double() - W64.double()).norm() / W64.double().norm())
    print(f"KRR 2000 x 16, s = 256, f64 Gram: herk_tri vs addmm weights, relative difference {rel:.3e}")
    assert rel <= 1e-10, rel


# ------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(monkeypatch):
    from libskylark_amd.ops import _lib, herk
    calls = []
    real = _lib.call

    def counting(name, *a):
        if name not in ("sl_herk_tri_block", "sl_herk_tri_plan"):
            calls.append(name)
        return real(name, *a)

    monkeypatch.setattr(_lib, "call", counting)
    A = torch.rand(40, 24, dtype=F64, device="cuda")
    C = torch.zeros(40, 40, dtype=F64, device="cuda")
    big = torch.zeros(80, 80, dtype=F64, device="cuda")
    for why, kw in (
            ("A must be f64", dict(A=A.float())),
            ("A must be a dense 2-D tensor", dict(A=A[0])),
            ("A: needs unit stride", dict(A=big[::2, :48:2])),
            ("A's rows overlap", dict(A=A[0].expand(40, 24))),
            ("A must be a CUDA tensor", dict(A=A.cpu(), C=None)),
            ("C must be f64", dict(C=C.float())),
            ("C must be square of order 40", dict(C=torch.zeros(24, 24, dtype=F64, device="cuda"))),
            ("C must be square of order 24", dict(orient="T")),
            ("C: needs unit stride", dict(C=big[::2, ::2])),
            ("C's rows overlap", dict(C=C[0].expand(40, 40))),
            ("C is on cpu", dict(C=C.cpu())),
            ("uplo must be", dict(uplo="X")),
            ("orientation must be", dict(orient="Q")),
            ("splits must be positive", dict(splits=0))):
        args = dict(uplo="L", orient="N", A=A, C=C, splits=None)
        args.update(kw)
        with pytest.raises(ValueError, match="herk_tri: " + why):
            herk.herk_tri(args["uplo"], args["orient"], 1.0, args["A"], 0.5, args["C"], splits=args["splits"])
        if why[0] in "AC":
            assert not herk.ok(args["A"], args["C"], trans=args["orient"] == "T")
    assert calls == [] and not C.any()
    herk.herk_tri("L", "N", 1.0, A, 0.5, C)
    assert calls == ["sl_herk_tri"]


def test_report_worst():
    """Not a check: the largest e / ((K + 4) u) per K over the cases run before it."""
    for K in sorted(_WORST):
        print(f"herk_tri worst over all cases, K={K}: {_WORST[K]:.4f} (K + 4) u")
