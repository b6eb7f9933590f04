"""Every kernel-Gram GPU path against the long-double reference of
``gram_reference`` under its derived rounding bounds.

a. the exported kernels of ``distance_kernels.hip`` called directly
   (``sl_pairwise_map_strided``, ``sl_point_sqnorms``, ``sl_gram_map``) on
   operands inside NaN-poisoned, padded allocations, the output inside a
   sentinel-filled one: no NaN may leak in, no byte outside ``K[:m, :n]`` may
   change, and two runs are bit-identical (no atomics in that file);
b. the C API (``sl_create_kernel`` + ``sl_kernel_gram`` on ``DeviceMatrix``
   operands): six kernel types, three Matern orders, f32 / f64, points as rows
   and as columns, padded leading dimensions, and the error codes;
c. ``ml.kernels`` on the GPU: ``gram`` (``Y`` given / ``None`` / ``K=``),
   ``symmetric_gram``, ``"columns"`` operands, non-contiguous and mixed-dtype
   operands;
d. the fused split-bf16 Gram (``FUSED_GRAM_MIN`` lowered), with the zero-padded
   K tail in use.

Shapes: ``gram_reference.SHAPES`` cross the 64-wide output tile, the 32-wide d
slab, the 16-lane micro-tile stride, the four points per workgroup of the
norm kernel and its 64-lane stride over d.

Instantiation -> a case that launches it (``T`` = f32 and f64 by the id):

    k_gram_map<T, GM_MATERN05 / 15 / 25>   test_gram_map[65x63x33-f32|f64],
                                           test_capi_device_gram[matern05|15|25-f32|f64]
    k_gram_map<T, GAUSSIAN / POLYNOMIAL>   test_gram_map[*], test_python_gram[gaussian|poly2|poly3-*]
    k_gram_map grid-stride loop            test_gram_map_grid_stride[f32|f64]
    k_point_sqnorms<T>, both strides       test_point_sqnorms[f32|f64], test_capi_device_gram[gaussian-*]
    k_pairwise<T, L1 / SEMIGROUP, true>,   test_pairwise_map_strided[65x63x33-*], [130x67x70-*]
      coordinate stride != 1               (all four row / column layouts)
    k_pairwise<T, L1 / SEMIGROUP, false>   test_pairwise_map_strided[*] (scale = 0)
    C API expsemigroup / linear /          test_capi_device_gram[expsemigroup|linear|poly2|poly3-f32|f64]
      polynomial, every kernel in f32
    Python symmetric / columns / strided   test_python_symmetric_gram[*], test_python_gram[*],
      / mixed operands, Linear, Matern     test_python_gram_mixed_dtypes[*]
    fused Gram, padded K tail, symmetric   test_fused_gram[gaussian|poly2|poly3-257x129x33] ...

Measured on an MI355X (largest error / bound over every path, f32 / f64):
linear 0.16 / 0.17, gaussian 0.10 / 0.09, polynomial q = 2 0.47 / 0.41, q = 3
0.17 / 0.17, laplacian 0.19 / 0.17, expsemigroup 0.17 / 0.15, matern 0.5 0.23 /
0.22, 1.5 0.04 / 0.04, 2.5 0.04 / 0.05, raw L1 0.19 / 0.19, raw semigroup 0.24 /
0.19, squared norms 0.93 / 0.19 (half an ulp of T is the whole bound), fused
gaussian 0.31, polynomial 0.34.  E needed 0.894 (set 2), F needed 0.671 (set
2).  K(x, x) of coincident points: Matern 0.5 / 1.5 / 2.5 off 1 by 3.2e-3 /
1.6e-5 / 8.8e-6 in f32 (C path 2.3e-3 / 7.9e-6 / 4.4e-6), 1.6e-7 / 3.7e-14 /
2.0e-14 in f64; the fused Gaussian by 5.0e-5."""
import ctypes as C

import pytest
import torch

import gram_reference as GR
from libskylark_amd import ml
from libskylark_amd.ml import kernels as KM
from libskylark_amd.ops import _lib as L

pytestmark = pytest.mark.gpu

L.register("sl_pairwise_map_strided", [L.vp, L.i64, L.i64, L.vp, L.i64, L.i64, L.vp, L.i64, L.i32, L.i64, L.i64,
                                       L.i64, L.i32, L.f64, L.vp])
L.register("sl_point_sqnorms", [L.vp, L.i32, L.i64, L.i64, L.i64, L.i64, L.vp, L.vp])

DTYPES = [torch.float32, torch.float64]
DT_IDS = ["f32", "f64"]
# quiet-NaN bit patterns: a leaked sentinel also fails the NaN check
SENT = {torch.float32: (torch.int32, 0x7FC0DEAD), torch.float64: (torch.int64, 0x7FF8DEADBEEF0BAD)}
LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]   # (X points are rows, Y points are rows)


def _sid(s):
    return "x".join(map(str, s))


def _dn(dt):
    return str(dt)[6:]


def _kernel(kid):
    return next(k for k in GR.KERNELS if k[0] == kid)[1:]


def poisoned(A, dev):
    """``A`` (CPU, 2-D) as a device view with a padded pitch inside a larger
    allocation whose every other element is NaN."""
    r, c = A.shape
    buf = torch.full((r + 2, c + 5), float("nan"), dtype=A.dtype, device=dev)
    v = buf[1:1 + r, 3:3 + c]
    v.copy_(A)
    return v


def operand(P, rows, dev):
    """Points ``P`` (CPU, points x coordinates) stored with the points as rows
    or as columns -> (device view, point stride, coordinate stride)."""
    v = poisoned(P if rows else P.t(), dev)
    return (v, v.stride(0), 1) if rows else (v, 1, v.stride(0))


def sentinel_out(m, n, dt, dev):
    it, s = SENT[dt]
    buf = torch.full((m + 3, n + 5), s, dtype=it, device=dev)
    return buf, buf.view(dt)[1:1 + m, 2:2 + n]


def assert_untouched_outside(buf, m, n, dt):
    """No NaN inside K[:m, :n]; every element outside it still the sentinel."""
    it, s = SENT[dt]
    assert not bool(torch.isnan(buf.view(dt)[1:1 + m, 2:2 + n]).any()), "NaN leaked into K"
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[1:1 + m, 2:2 + n] = False
    assert bool((buf[outside] == s).all()), "store outside K[:m, :n]"


_DIST = {}


def _ref_distance(mode, shape, dt, signed, X, Y):
    key = (mode, shape, dt, signed)
    if key not in _DIST:
        _DIST[key] = GR.ref_distance(mode, X, Y)
    return _DIST[key]


# ------------------------------------------------------------ a. direct calls
def _pairwise(Xo, Yo, m, n, d, mode, scale, dt, dev):
    buf, K = sentinel_out(m, n, dt, dev)
    (xv, xsp, xsd), (yv, ysp, ysd) = Xo, Yo
    L.call("sl_pairwise_map_strided", L.ptr(xv), xsp, xsd, L.ptr(yv), ysp, ysd, L.ptr(K), K.stride(0),
           L.dtype_code(dt), m, n, d, mode, float(scale), L.stream_of(K))
    torch.cuda.synchronize()
    assert_untouched_outside(buf, m, n, dt)
    return buf, K


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", GR.SHAPES, ids=_sid)
def test_pairwise_map_strided(dev, shape, dt):
    """k_pairwise<T, L1 / SEMIGROUP, EXP = true / false>, both operands
    independently as row points and as column points."""
    m, n, d = shape
    u = GR.unit(dt)
    layouts = LAYOUTS if shape in GR.LAYOUT_SHAPES else [LAYOUTS[0], LAYOUTS[3]]
    for signed in (False, True):
        X, Y = GR.points(m, n, d, dt, signed)
        ops = {(w, r): operand(P, r, dev) for w, P in (("x", X), ("y", Y)) for r in (True, False)}
        for mode in ((0, 1) if not signed else (0,)):    # the exp-semigroup kernel is for non-negative data
            kind = "laplacian" if mode == 0 else "expsemigroup"
            params = dict(_kernel(kind)[1])
            if signed:
                params = GR.signed_params(kind, params, d)
            scale = 1.0 / params["sigma"] if mode == 0 else params["beta"]
            D = _ref_distance(mode, shape, dt, signed, X, Y)
            Kr, Q = GR.cached_ref(("xy", shape, dt, signed), kind, params, X, Y)
            for xr, yr in layouts:
                tag = f"pairwise/{kind}/{_dn(dt)}"
                b1, K1 = _pairwise(ops["x", xr], ops["y", yr], m, n, d, mode, scale, dt, dev)
                b2, _ = _pairwise(ops["x", xr], ops["y", yr], m, n, d, mode, scale, dt, dev)
                assert torch.equal(b1, b2), "two runs differ"
                GR.check(tag, K1, Kr, Q, u)
                # raw distances (scale = 0): EXP = false
                b1, K1 = _pairwise(ops["x", xr], ops["y", yr], m, n, d, mode, 0.0, dt, dev)
                b2, _ = _pairwise(ops["x", xr], ops["y", yr], m, n, d, mode, 0.0, dt, dev)
                assert torch.equal(b1, b2), "two runs differ"
                GR.check_abs(f"pairwise/raw{mode}/{_dn(dt)}", K1, D, GR.bound_distance(D, d, u))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_point_sqnorms(dev, dt):
    """k_point_sqnorms: both strided forms around the four points per
    workgroup and the 64-lane stride over d; f64 accumulation, one rounding."""
    it, s = SENT[dt]
    g = torch.Generator().manual_seed(5)
    for m in (1, 3, 4, 5, 9):
        for d in (1, 63, 64, 65, 200):
            X = torch.randn(m, d, generator=g, dtype=dt)
            nref = GR.ref_sqnorms(X)
            B = GR.bound_sqnorms(nref, d, GR.unit(dt))
            for rows in (True, False):
                v, sp, sd = operand(X, rows, dev)
                outs = []
                for _ in range(2):
                    buf = torch.full((m + 5,), s, dtype=it, device=dev)
                    out = buf.view(dt)[2:2 + m]
                    L.call("sl_point_sqnorms", L.ptr(v), L.dtype_code(dt), m, d, sp, sd, L.ptr(out), L.stream_of(out))
                    torch.cuda.synchronize()
                    assert bool((buf[:2] == s).all()) and bool((buf[2 + m:] == s).all()), "store outside out[:m]"
                    outs.append(buf)
                assert torch.equal(outs[0], outs[1]), "two runs differ"
                GR.check_abs(f"sqnorms/{_dn(dt)}", out, nref, B)


def _map_args(kind, params):
    if kind == "gaussian":
        return 0, 1.0 / (2.0 * params["sigma"] ** 2), 0.0, 1.0
    if kind == "polynomial":
        return 1, params["gamma"], params["c"], float(params["q"])
    return {0.5: 3, 1.5: 4, 2.5: 5}[params["nu"]], 1.0 / params["l"], 0.0, 1.0


def _gram_map(G, xn, yn, kind, params, dt, dev):
    m, n = G.shape
    buf, K = sentinel_out(m, n, dt, dev)
    K.copy_(G)
    code, a, c, q = _map_args(kind, params)
    L.call("sl_gram_map", L.ptr(K), L.dtype_code(dt), m, n, K.stride(0), L.ptr(xn), L.ptr(yn), code, a, c, q,
           L.stream_of(K))
    torch.cuda.synchronize()
    assert_untouched_outside(buf, m, n, dt)
    return buf, K


MAP_KIDS = ["gaussian", "poly2", "poly3", "matern05", "matern15", "matern25"]


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", GR.SHAPES, ids=_sid)
def test_gram_map(dev, shape, dt):
    """k_gram_map<T, GAUSSIAN / POLYNOMIAL / MATERN05 / 15 / 25> in place on a
    G = X Y^T that torch computed in the working dtype."""
    m, n, d = shape
    for signed in (False, True):
        X, Y = GR.points(m, n, d, dt, signed)
        Xd, Yd = X.to(dev), Y.to(dev)
        G = Xd @ Yd.t()
        xn, yn = poisoned((X * X).sum(1)[None, :], dev)[0], poisoned((Y * Y).sum(1)[None, :], dev)[0]
        for kid in (MAP_KIDS if not signed else MAP_KIDS[:3]):
            kind, params = _kernel(kid)
            if signed:
                params = GR.signed_params(kind, params, d)
            Kr, Q = GR.cached_ref(("xy", shape, dt, signed), kind, params, X, Y)
            if signed and kind == "polynomial" and m * n > 1:
                assert (Q["base"] < 0).any() and (Q["base"] > 0).any()
            b1, K1 = _gram_map(G, xn, yn, kind, params, dt, dev)
            b2, _ = _gram_map(G, xn, yn, kind, params, dt, dev)
            assert torch.equal(b1, b2), "two runs differ"
            GR.check(f"gram_map/{kid}/{_dn(dt)}", K1, Kr, Q, GR.unit(dt))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_gram_map_grid_stride(dev, dt):
    """m * n just above 8192 blocks x 256 threads: the grid-stride loop of
    k_gram_map runs.  Reference (this case only): torch f64 on the device from
    the definition; its own rounding, (d + 2) 2^-53 a d2 K + 4 2^-53 (1 + arg)
    K, is added to the bound."""
    m, n, d, sigma = 1025, 2050, 8, 1.3
    assert m * n > 8192 * 256
    g = torch.Generator().manual_seed(11)
    X = torch.rand(m, d, generator=g, dtype=dt).to(dev)
    Y = torch.rand(n, d, generator=g, dtype=dt).to(dev)
    Y[:3] = X[:3]
    G = X @ Y.t()
    xn, yn = (X * X).sum(1), (Y * Y).sum(1)
    b1, K1 = _gram_map(G, xn, yn, "gaussian", {"sigma": sigma}, dt, dev)
    b2, _ = _gram_map(G, xn, yn, "gaussian", {"sigma": sigma}, dt, dev)
    assert torch.equal(b1, b2), "two runs differ"
    X64, Y64 = X.double(), Y.double()
    a, u, u64 = 1.0 / (2.0 * sigma ** 2), GR.unit(dt), 2.0 ** -53
    d2 = torch.zeros(m, n, dtype=torch.float64, device=dev)
    for k in range(d):
        d2 += (X64[:, k, None] - Y64[None, :, k]) ** 2
    Kr = torch.exp(-a * d2)
    S = X64.abs() @ Y64.abs().t()
    delta = (d + 4) * u * ((X64 * X64).sum(1)[:, None] + (Y64 * Y64).sum(1)[None, :] + 2 * S)
    B = a * delta * Kr + GR.E * u * (1 + a * d2) * Kr
    B += (d + 2) * u64 * a * d2 * Kr + 4 * u64 * (1 + a * d2) * Kr
    ratio = float(((K1.double() - Kr).abs() / B).max())
    print(f"gram_map/grid-stride/{_dn(dt)}: err/bound {ratio:.3f}")
    assert ratio <= 1.0, ratio
    assert float(K1[:3, :3].diagonal().max()) <= 1.0


# ------------------------------------------------------------------ b. C API
@pytest.fixture(scope="module")
def capi():
    from libskylark_amd._native import build as B
    B.build_capi()
    lib = C.CDLL(B.CAPI_LIB)
    vp = C.c_void_p
    lib.sl_wrap_raw_device_matrix.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(vp)]
    lib.sl_free_raw_device_matrix_wrap.argtypes = [vp]
    lib.sl_kernel_gram.argtypes = [C.c_int, C.c_int, vp, C.c_char_p, vp, C.c_char_p, vp, C.c_char_p, vp]
    lib.sl_free_kernel.argtypes = [vp]
    lib.sl_create_kernel.restype = C.c_int
    lib.sl_strerror.restype = C.c_char_p
    return lib


def _c_kernel(lib, kind, params, d):
    kh = C.c_void_p()
    args = {"linear": [], "gaussian": ["sigma"], "laplacian": ["sigma"], "expsemigroup": ["beta"],
            "polynomial": ["q", "c", "gamma"], "matern": ["nu", "l"]}[kind]
    va = [C.c_int(int(params[a])) if a == "q" else C.c_double(float(params[a])) for a in args]
    assert lib.sl_create_kernel(kind.encode(), d, C.byref(kh), *va) == 0
    return kh


def _c_gram(lib, kh, dirX, dirY, xv, yv, K):
    hs = []
    for t in (xv, yv, K):
        h = C.c_void_p()
        assert lib.sl_wrap_raw_device_matrix(t.data_ptr(), L.dtype_code(t.dtype), t.shape[0], t.shape[1], t.stride(0),
                                             C.byref(h)) == 0
        hs.append(h)
    torch.cuda.synchronize()
    rc = lib.sl_kernel_gram(dirX, dirY, kh, b"DeviceMatrix", hs[0], b"DeviceMatrix", hs[1], b"DeviceMatrix", hs[2])
    torch.cuda.synchronize()
    for h in hs:
        lib.sl_free_raw_device_matrix_wrap(h)
    return rc


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kid", GR.KERNEL_IDS)
def test_capi_device_gram(dev, capi, kid, dt):
    """sl_create_kernel + sl_kernel_gram on DeviceMatrix operands: direction 1
    (points are columns) and 2 (rows) on each operand, ld > n everywhere."""
    kind, params0 = _kernel(kid)
    u = GR.unit(dt)
    for shape in GR.SHAPES:
        m, n, d = shape
        dirs = [(2, 2), (2, 1), (1, 2), (1, 1)] if shape in GR.LAYOUT_SHAPES else [(1, 1), (2, 2)]
        for signed in ((False, True) if kind in ("linear", "gaussian", "polynomial", "laplacian") else (False,)):
            if signed and shape not in GR.LAYOUT_SHAPES:
                continue
            params = GR.signed_params(kind, params0, d) if signed else params0
            X, Y = GR.points(m, n, d, dt, signed)
            Kr, Q = GR.cached_ref(("xy", shape, dt, signed), kind, params, X, Y)
            kh = _c_kernel(capi, kind, params, d)
            for dx, dy in dirs:
                xv, yv = operand(X, dx == 2, dev)[0], operand(Y, dy == 2, dev)[0]
                buf, K = sentinel_out(m, n, dt, dev)
                assert _c_gram(capi, kh, dx, dy, xv, yv, K) == 0
                assert_untouched_outside(buf, m, n, dt)
                GR.check(f"capi/{kid}/{_dn(dt)}", K, Kr, Q, u)
                if kind == "matern" and not signed:
                    h = min(m, n, 3)
                    GR._record(f"coincident/capi/{kid}/{_dn(dt)}", dev=float((K[:h, :h].diagonal() - 1).abs().max()))
            capi.sl_free_kernel(kh)


def test_capi_device_gram_errors(dev, capi):
    """A Matern order without a closed form, a dtype mismatch and a dimension
    mismatch are refused with their codes, and K is left untouched."""
    m, n, d = 9, 7, 5
    X, Y = GR.points(m, n, d, torch.float64)

    def run(kh, xv, yv, kdt=torch.float64, km=m, kn=n):
        buf, K = sentinel_out(km, kn, kdt, dev)
        rc = _c_gram(capi, kh, 2, 2, xv, yv, K)
        assert bool((buf == SENT[kdt][1]).all()), "a refused call wrote K"
        return rc

    xv, yv = operand(X, True, dev)[0], operand(Y, True, dev)[0]
    kh = _c_kernel(capi, "matern", {"nu": 1.0, "l": 1.7}, d)
    assert run(kh, xv, yv) == 103
    capi.sl_free_kernel(kh)
    kh = _c_kernel(capi, "gaussian", {"sigma": 1.3}, d)
    assert run(kh, operand(X.float(), True, dev)[0], yv) == 103          # X f32, Y / K f64
    assert run(kh, xv, yv, kdt=torch.float32) == 103                    # K f32
    assert run(kh, xv, operand(Y[:, :4], True, dev)[0]) == 104           # point dimensions differ
    assert run(kh, xv, yv, km=m + 1) == 104                              # K is not (#X points) x (#Y points)
    assert capi.sl_strerror(104) == b"Dimension mismatch"
    capi.sl_free_kernel(kh)
    kh = _c_kernel(capi, "gaussian", {"sigma": 1.3}, d + 1)              # the kernel's dimension differs
    assert run(kh, xv, yv) == 104
    capi.sl_free_kernel(kh)


# ------------------------------------------------------- c. ml.kernels on GPU
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kid", GR.KERNEL_IDS)
def test_python_gram(dev, kid, dt):
    """Kernel.gram with Y given, at every shape; operands as columns, as a
    non-contiguous row slice, and the K= output argument."""
    kind, params0 = _kernel(kid)
    u = GR.unit(dt)
    tag = f"python/{kid}/{_dn(dt)}"
    for shape in GR.SHAPES:
        m, n, d = shape
        for signed in ((False, True) if kind in ("linear", "gaussian", "polynomial", "laplacian") else (False,)):
            if signed and shape not in GR.LAYOUT_SHAPES:
                continue
            params = GR.signed_params(kind, params0, d) if signed else params0
            k = GR.make_kernel(ml, kind, params, d)
            X, Y = GR.points(m, n, d, dt, signed)
            Kr, Q = GR.cached_ref(("xy", shape, dt, signed), kind, params, X, Y)
            Xd, Yd = X.to(dev), Y.to(dev)
            GR.check(tag, k.gram(Xd, Y=Yd), Kr, Q, u)
            if shape not in GR.LAYOUT_SHAPES:
                continue
            Xc, Yc = Xd.t().contiguous(), Yd.t().contiguous()
            GR.check(tag, k.gram(Xc, dirX="columns", dirY="columns", Y=Yc), Kr, Q, u)
            GR.check(tag, k.gram(Xc, dirX="columns", dirY="rows", Y=Yd), Kr, Q, u)
            GR.check(tag, k.gram(Xd, dirX="rows", dirY="columns", Y=Yc), Kr, Q, u)
            # every other row of a twice-as-tall NaN-filled matrix
            Xb = torch.full((2 * m, d), float("nan"), dtype=dt, device=dev)
            Yb = torch.full((2 * n, d + 3), float("nan"), dtype=dt, device=dev)
            Xb[::2] = Xd
            Yb[1::2, 2:2 + d] = Yd
            Xs, Ys = Xb[::2], Yb[1::2, 2:2 + d]
            assert not Xs.is_contiguous() and not Ys.is_contiguous()
            GR.check(tag, k.gram(Xs, Y=Ys), Kr, Q, u)
            out = torch.full((m, n), float("nan"), dtype=dt, device=dev)
            assert k.gram(Xd, K=out, Y=Yd) is out
            GR.check(tag, out, Kr, Q, u)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kid", GR.KERNEL_IDS)
def test_python_symmetric_gram(dev, kid, dt):
    """gram(X) with Y = None and symmetric_gram (rows and columns): within the
    bound of the reference and of the general gram(X, X), and symmetric to
    within twice the bound."""
    kind, params = _kernel(kid)
    u = GR.unit(dt)
    tag = f"python-sym/{kid}/{_dn(dt)}"
    for shape in GR.LAYOUT_SHAPES + [(1, 1, 1), (5, 4, 200)]:
        m, n, d = shape
        k = GR.make_kernel(ml, kind, params, d)
        X, _ = GR.points(m, n, d, dt)
        Kr, Q = GR.cached_ref(("xx", shape, dt), kind, params, X, X)
        B = GR.bound(Kr, Q, u)
        Xd = X.to(dev)
        Kg = GR._ld(k.gram(Xd, Y=Xd.clone()))
        for Ks in (k.gram(Xd), k.symmetric_gram(Xd), k.symmetric_gram(Xd.t().contiguous(), "columns")):
            assert Ks.shape == (m, m)
            GR.check(tag, Ks, Kr, Q, u)
            GR.check_abs(tag + "/vs-general", Ks, Kg, B)
            GR.check_abs(tag + "/symmetry", Ks, GR._ld(Ks).T, 2 * B)
            if kind == "matern":
                GR._record(f"coincident/python/{kid}/{_dn(dt)}", dev=float((Ks.diagonal() - 1).abs().max()))


@pytest.mark.parametrize("kid", GR.KERNEL_IDS)
def test_python_gram_mixed_dtypes(dev, kid):
    """f32 X with f64 Y: the work dtype is f64, on the f32-representable X."""
    kind, params = _kernel(kid)
    for shape in GR.LAYOUT_SHAPES:
        m, n, d = shape
        k = GR.make_kernel(ml, kind, params, d)
        X, _ = GR.points(m, n, d, torch.float32)
        _, Y = GR.points(m, n, d, torch.float64)
        Y[:3] = X[:3].double()
        Kr, Q = GR.cached_ref(("mixed", shape), kind, params, X.double(), Y)
        K = k.gram(X.to(dev), Y=Y.to(dev))
        assert K.dtype == torch.float64
        GR.check(f"python-mixed/{kid}", K, Kr, Q, GR.unit(torch.float64))


# --------------------------------------------------------------- d. fused Gram
FUSED_SHAPES = [(257, 129, 33), (64, 385, 100), (300, 256, 64), (1, 1, 1)]


@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=_sid)
@pytest.mark.parametrize("kid", ["gaussian", "poly2", "poly3"])
def test_fused_gram(dev, monkeypatch, kid, shape):
    """The split-bf16 MFMA Gram with the kernel map in its epilogue, general
    and symmetric, at shapes whose K is no multiple of the padding.  The
    inner-product error is F * 2^-16 * sum |x y| (ops/fused.py)."""
    from libskylark_amd.ops import fused
    calls = []
    real = fused.feature_gemm

    def counting(*a, **kw):
        calls.append(kw.get("epi"))
        return real(*a, **kw)

    monkeypatch.setattr(KM, "FUSED_GRAM_MIN", 1)
    monkeypatch.setattr(fused, "feature_gemm", counting)
    kind, params0 = _kernel(kid)
    m, n, d = shape
    dt, u = torch.float32, GR.unit(torch.float32)
    tag = f"fused/{kid}"
    for signed in (False, True):
        params = GR.signed_params(kind, params0, d) if signed else params0
        k = GR.make_kernel(ml, kind, params, d)
        X, Y = GR.points(m, n, d, dt, signed)
        Xd, Yd = X.to(dev), Y.to(dev)
        Kr, Q = GR.cached_ref(("xy", shape, dt, signed), kind, params, X, Y)
        if signed and kind == "polynomial" and m * n > 1:
            assert (Q["base"] < 0).any() and (Q["base"] > 0).any()
        before = len(calls)
        K = k.gram(Xd, Y=Yd)
        assert len(calls) == before + 1, "the fused branch was not taken"
        GR.check(tag, K, Kr, Q, u, fused=GR.F)
        if kind == "gaussian":
            assert float(K.max()) <= 1.0
            h = min(m, n, 3)
            GR._record("coincident/fused/gaussian", dev=float((K[:h, :h].diagonal() - 1).abs().max()))
        Ks_r, Qs = GR.cached_ref(("xx", shape, dt, signed), kind, params, X, X)
        Bs = GR.bound(Ks_r, Qs, u, fused=GR.F)
        Kg = GR._ld(k.gram(Xd, Y=Xd.clone()))
        for Ks in (k.gram(Xd), k.symmetric_gram(Xd)):
            GR.check(tag, Ks, Ks_r, Qs, u, fused=GR.F)
            GR.check_abs(tag + "/vs-general", Ks, Kg, Bs)
            GR.check_abs(tag + "/symmetry", Ks, GR._ld(Ks).T, 2 * Bs)
            if kind == "gaussian":
                assert float(Ks.max()) <= 1.0
        assert len(calls) == before + 4, "the fused branch was not taken"
    assert set(calls) == {fused.EPI_GAUSS if kind == "gaussian" else fused.EPI_POLY}
