"""Native triangular rank-k update (``syrk_split.hip`` through ``ops/syrk.py``
and ``base.Herk``) on the GPU: tile map, chunk / owner cuts, triangle masking,
alpha / beta, strided C, determinism, and accuracy against the unchanged
``ml.krr._gram_split`` (same six plane products, another summation order).

err(C) = max over the triangle of |C - C64|_ij / sqrt(C64_ii C64_jj), C64 from
fp64 torch; the rule is err(Herk) <= 2 err(_gram_split) + 2^-40 (the factor 2
covers the summation order only).  Measured on an MI355X: err(Herk) 3.9e-8 ..
1.5e-7 over these cases against err(_gram_split) 3.4e-7 (200 x 64), 6.1e-7
(200 x 300) and 2.6e-6 (1000 x 520), f32 and f64 C alike; bf16 1.2e-7 against
7.8e-7 for the fp32 torch.mm; 4.2e6 x 16: 3.1e-9 against 2.3e-6."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -40
SHAPES = [(200, 64), (200, 300), (1000, 520)]
_cache = {}


def _mask(s, uplo, dev):
    ones = torch.ones(s, s, dtype=torch.bool, device=dev)
    return torch.tril(ones) if uplo == "L" else torch.triu(ones)


def _err(C, C64, uplo="L"):
    d = torch.sqrt(torch.diagonal(C64))
    m = _mask(C64.shape[0], uplo, C64.device)
    return float(((C.double() - C64).abs() / (d[:, None] * d[None, :]))[m].max())


def _case(dev, n, s):
    """Zero-mean f32 data, its fp64 Gram and the error of the existing split
    path on it: computed once per shape and shared, never modified."""
    key = (n, s)
    if key not in _cache:
        from libskylark_amd.ml import krr as K
        g = torch.Generator(device=dev).manual_seed(1000 * n + s)
        Z = torch.randn(n, s, generator=g, device=dev)
        C64 = Z.double().t() @ Z.double()
        G = torch.zeros(s, s, dtype=torch.float64, device=dev)
        K._gram_split(Z, G)
        _cache[key] = (Z, C64, _err(G, C64))
    return _cache[key]


def _check(C, C64, base, uplo="L", what=""):
    e = _err(C, C64, uplo)
    print(f"{what} err(Herk) {e:.3e} err(_gram_split) {base:.3e}")
    assert e <= 2 * base + EPS, f"{what}: err(Herk) {e:.3e} > 2 x err(_gram_split) {base:.3e} + 2^-40"


@pytest.mark.parametrize("workgroups", [1, 5, None])
@pytest.mark.parametrize("n,s", SHAPES)
def test_syrk_t_shapes_chunks_owners(dev, n, s, workgroups):
    """chunk_rows = 128: several chunks and a short last one; 1 / 5 / one-per-CU
    workgroups: tiles cut between owners mid-chunk."""
    from libskylark_amd.ops import syrk
    Z, C64, base = _case(dev, n, s)
    C = torch.zeros(s, s, dtype=torch.float64, device=dev)
    out = syrk.syrk_split(Z, C, trans=True, chunk_rows=128, workgroups=workgroups)
    assert out is C
    _check(C, C64, base, what=f"{n}x{s} wg={workgroups}")
    assert torch.equal(torch.triu(C, 1), torch.zeros_like(C))


def test_syrk_default_knobs_through_herk(dev):
    from libskylark_amd.base import Herk
    Z, C64, base = _case(dev, 1000, 520)
    C = Herk("L", "T", 1.0, Z)
    assert C.dtype == torch.float32 and torch.equal(torch.triu(C, 1), torch.zeros_like(C))
    _check(C, C64, base, what="f32 C, default knobs")


@pytest.mark.parametrize("workgroups", [5, None])
def test_syrk_every_plane_pair_counts(dev, workgroups):
    """Data on which each group of plane products is worth more than the
    bound: x = 1 + m + l with m = k 2^-15 (k = 64..127: eight bits, so M = m
    exactly, and m + l < 2^-8 keeps H = 1) and l = v 2^-18, v in (1/4, 1) (below
    half an ulp of m, so it stays in L).  H = 1, M and L all have positive mean, so H^T L + L^T H
    (~5e-6 of the Gram), H^T M + M^T H and M^T M (~9e-6) each shift it
    systematically, while 128 rows keep the f32 sums of both paths near 1e-7.
    One chunk, as _gram_split sums it.  The fp64 size of each group is checked
    to exceed twice the bound first, so a result that lacks one cannot pass."""
    from libskylark_amd.ml import krr as K
    from libskylark_amd.ops import syrk
    n, s = 128, 300
    g = torch.Generator(device=dev).manual_seed(77)
    k = torch.randint(64, 128, (n, s), generator=g, device=dev).double()
    v = torch.rand(n, s, generator=g, device=dev, dtype=torch.float64) * 0.75 + 0.25
    Z = (1.0 + k * 2.0 ** -15 + v * 2.0 ** -18).float()
    C64 = Z.double().t() @ Z.double()
    G = torch.zeros(s, s, dtype=torch.float64, device=dev)
    K._gram_split(Z, G)
    base = _err(G, C64)
    bound = 2 * base + EPS
    H, Mp, L = (p.double() for p in K._split3(Z))
    d = torch.sqrt(torch.diagonal(C64))
    dd = d[:, None] * d[None, :]
    groups = {"HL+LH": H.t() @ L + L.t() @ H, "HM+MH": H.t() @ Mp + Mp.t() @ H, "MM": Mp.t() @ Mp}
    for name, D in groups.items():
        worth = float((torch.tril(D).abs() / dd).max())
        print(f"{name} worth {worth:.3e} bound {bound:.3e}")
        assert worth > 2 * bound, f"{name}: {worth:.3e} would hide under the bound {bound:.3e}"
    C = torch.zeros(s, s, dtype=torch.float64, device=dev)
    syrk.syrk_split(Z, C, trans=True, chunk_rows=128, workgroups=workgroups)
    _check(C, C64, base, what=f"plane pairs wg={workgroups}")


def test_syrk_long_narrow(dev):
    """More K blocks in one super-chunk than a grid dimension holds (65535 x 64
    rows): the transposing split walks them in a loop."""
    from libskylark_amd.base import Herk
    from libskylark_amd.ml import krr as K
    n, s = 65536 * 64 + 200, 16
    g = torch.Generator(device=dev).manual_seed(78)
    Z = torch.randn(n, s, generator=g, device=dev)
    C64 = torch.zeros(s, s, dtype=torch.float64, device=dev)
    for r0 in range(0, n, 1 << 20):
        Zc = Z[r0:r0 + (1 << 20)].double()
        C64 += Zc.t() @ Zc
    G = torch.zeros(s, s, dtype=torch.float64, device=dev)
    K._gram_split(Z, G)
    C = Herk("L", "T", 1.0, Z, 0.0, torch.zeros(s, s, dtype=torch.float64, device=dev))
    _check(C, C64, _err(G, C64), what="long narrow")


def test_syrk_auto_workgroups_fit_the_work(dev):
    """The automatic workgroup count never exceeds the steps of a chunk, so a
    one-tile problem does not clear a slab per CU."""
    from libskylark_amd.ops import syrk
    slabs, wgs = syrk.plan(64, 200, 8192, 0, torch.float32)    # 1 tile x 6 pairs x 4 slices
    assert wgs == 24 and slabs == 24
    slabs, wgs = syrk.plan(4096, 40960, 8192, 0, torch.float32)
    assert wgs == torch.cuda.get_device_properties(dev).multi_processor_count and slabs == 2 * wgs


def test_syrk_super_chunks(dev, monkeypatch):
    """A workspace bound of 256 rows: four launches of one partition, the last
    one short, accumulating in the same slabs."""
    from libskylark_amd.ops import syrk
    Z, C64, base = _case(dev, 1000, 520)
    monkeypatch.setattr(syrk, "SPLIT_WS_BYTES", 6 * 520 * 256)
    C = torch.zeros(520, 520, dtype=torch.float64, device=dev)
    syrk.syrk_split(Z, C, trans=True, chunk_rows=128, workgroups=5)
    _check(C, C64, base, what="super-chunks")


def test_syrk_orient_n(dev):
    from libskylark_amd.base import Herk
    Z, C64, base = _case(dev, 200, 300)
    A = Z.t().contiguous()                      # 300 x 200, A A^T = Z^T Z
    C = torch.zeros(300, 300, dtype=torch.float64, device=dev)
    from libskylark_amd.ops import syrk
    syrk.syrk_split(A, C, trans=False, chunk_rows=128, workgroups=5)
    _check(C, C64, base, what="orient N")
    C2 = Herk("L", "N", 1.0, A, 0.0, torch.zeros(300, 300, dtype=torch.float64, device=dev))
    _check(C2, C64, base, what="orient N, default knobs")


def test_syrk_bf16_orient_n(dev):
    """bf16 A: every product is exact in f32, only the f32 sums differ from an
    fp32 torch.mm of the same operands."""
    from libskylark_amd.base import Herk
    g = torch.Generator(device=dev).manual_seed(31)
    A = torch.randn(300, 256, generator=g, device=dev).to(torch.bfloat16)
    C64 = A.double() @ A.double().t()
    base = _err(torch.mm(A.float(), A.float().t()), C64)
    C = torch.zeros(300, 300, dtype=torch.float32, device=dev)
    Herk("L", "N", 1.0, A, 0.0, C)
    # both results are f32: the final rounding is common to both sides
    _check(C, C64, base, what="bf16 N")
    assert torch.equal(torch.triu(C, 1), torch.zeros_like(C))


@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("cdtype", [torch.float32, torch.float64])
def test_syrk_uplo_alpha_beta_nan_triangle(dev, uplo, cdtype):
    from libskylark_amd.base import Herk
    Z, C64, base = _case(dev, 200, 300)
    s = 300
    m = _mask(s, uplo, dev)
    g = torch.Generator(device=dev).manual_seed(32)
    C0 = torch.randn(s, s, generator=g, device=dev, dtype=cdtype)
    C = torch.where(m, C0, torch.full_like(C0, float("nan")))
    before = C.clone()
    Herk(uplo, "T", 0.5, Z, 0.25, C)
    ref = 0.5 * C64 + 0.25 * C0.double()
    d = torch.sqrt(torch.diagonal(C64))
    dd = d[:, None] * d[None, :]
    e = float(((C.double() - ref).abs() / dd)[m].max())
    print(f"uplo {uplo} {cdtype}: err {e:.3e} base {base:.3e}")
    assert e <= 2 * base + EPS, f"err {e:.3e} > 2 x err(_gram_split) {base:.3e} + 2^-40"
    it = torch.int32 if cdtype == torch.float32 else torch.int64
    assert torch.equal(C[~m].view(it), before[~m].view(it))
    # beta == 0 does not read C: NaN in the target triangle does not survive
    Cn = torch.full((s, s), float("nan"), device=dev, dtype=cdtype)
    Herk(uplo, "T", 1.0, Z, 0.0, Cn)
    assert bool(torch.isfinite(Cn[m]).all()) and bool(torch.isnan(Cn[~m]).all())


def test_syrk_strided_c(dev):
    from libskylark_amd.ops import syrk
    Z, C64, base = _case(dev, 200, 300)
    g = torch.Generator(device=dev).manual_seed(33)
    big = torch.randn(300, 307, generator=g, device=dev, dtype=torch.float64)
    keep = big.clone()
    C = big[:, :300]
    assert C.stride(0) == 307
    syrk.syrk_split(Z, C, trans=True, chunk_rows=128, workgroups=5)
    _check(torch.tril(C), C64, base, what="strided C")
    assert torch.equal(big[:, 300:], keep[:, 300:])
    assert torch.equal(torch.triu(big[:, :300], 1), torch.triu(keep[:, :300], 1))


def test_syrk_deterministic(dev):
    from libskylark_amd.ops import syrk
    Z, C64, base = _case(dev, 1000, 520)
    runs = []
    for wg in (5, 5, 1):
        C = torch.zeros(520, 520, dtype=torch.float64, device=dev)
        runs.append(syrk.syrk_split(Z, C, trans=True, chunk_rows=128, workgroups=wg))
    assert torch.equal(runs[0], runs[1])
    _check(runs[0], C64, base, what="wg=5")
    _check(runs[2], C64, base, what="wg=1")
    d = torch.sqrt(torch.diagonal(C64))
    diff = float(((runs[0] - runs[2]).abs() / (d[:, None] * d[None, :])).max())
    assert diff <= 2 * (2 * base + EPS), diff


def test_syrk_invalid_arguments_launch_nothing(dev, monkeypatch):
    from libskylark_amd.ops import syrk
    calls = []
    monkeypatch.setattr(syrk._lib, "call", lambda name, *a: calls.append(name))
    A = torch.randn(200, 300, device=dev)
    with pytest.raises(ValueError):             # non-square C
        syrk.syrk_split(A, torch.zeros(300, 200, device=dev), trans=True)
    with pytest.raises(ValueError):             # wrong order
        syrk.syrk_split(A, torch.zeros(200, 200, device=dev), trans=True)
    with pytest.raises(ValueError):             # dtype mismatch: C
        syrk.syrk_split(A, torch.zeros(300, 300, device=dev, dtype=torch.float16), trans=True)
    with pytest.raises(ValueError):             # dtype mismatch: A
        syrk.syrk_split(A.double(), torch.zeros(300, 300, device=dev, dtype=torch.float64), trans=True)
    with pytest.raises(ValueError):             # bf16 is taken K-contiguous only
        syrk.syrk_split(A.to(torch.bfloat16), trans=True)
    wide = torch.zeros(300, 264, device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError):             # unaligned rows: base 2 B off a 16-B boundary
        syrk.syrk_split(wide[:, 1:257], trans=False)
    with pytest.raises(ValueError):             # unaligned rows: row stride 260 elements
        syrk.syrk_split(torch.zeros(300, 260, device=dev, dtype=torch.bfloat16)[:, :256], trans=False)
    with pytest.raises(ValueError):
        syrk.syrk_split(A, trans=True, chunk_rows=100)
    with pytest.raises(ValueError):
        syrk.syrk_split(A, trans=True, uplo="X")
    assert not syrk.ok(A.double()) and syrk.ok(A) and not syrk.ok(wide[:, 1:257], trans=False)
    assert calls == []


def test_krr_gram_syrk_opt_in(dev, monkeypatch):
    """approximate_kernel_ridge with SKH_KRR_GRAM=syrk against the all-fp64
    normal equations (the tolerance of test_gpu_ml's split-versus-f64 weight
    test), and the native path is the one taken."""
    import libskylark_amd as sk
    from libskylark_amd import ml
    from libskylark_amd.ops import syrk
    g = torch.Generator(device=dev).manual_seed(5)
    X = torch.randn(2000, 16, generator=g, device=dev)
    Y = torch.sin(X[:, :1]) + 0.01 * torch.randn(2000, 1, generator=g, device=dev)
    k = ml.Gaussian(16, sigma=4.0)
    seen = []
    real = syrk.syrk_split

    def spy(A, C=None, **kw):
        seen.append((A.shape[1] if kw["trans"] else A.shape[0], A.numel(), kw.get("uplo"), C.dtype))
        return real(A, C, **kw)

    monkeypatch.setattr(syrk, "syrk_split", spy)
    monkeypatch.setenv("SKH_KRR_GRAM", "syrk")
    _, W = ml.approximate_kernel_ridge(k, X, Y, 1e-2, 256, context=sk.Context(3))
    assert seen == [(256, 2000 * 256, "L", torch.float64)]
    monkeypatch.delenv("SKH_KRR_GRAM")
    monkeypatch.setenv("SKH_KRR_F64_GRAM", "1")
    _, W64 = ml.approximate_kernel_ridge(k, X, Y, 1e-2, 256, context=sk.Context(3))
    assert len(seen) == 1
    rel = float((W.double() - W64.double()).norm() / W64.double().norm())
    assert rel < 1e-4, rel
