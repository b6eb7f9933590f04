"""The CPU (plain torch) kernel Grams of ``ml.kernels`` against the long-double
reference of ``gram_reference`` under its derived rounding bounds: all six
kernels (three Matern orders, two polynomial degrees), f32 and f64, through
``gram``, ``symmetric_gram`` and ``"columns"`` operands, at the shapes the GPU
tests use.  Checks the helper and the bounds without a GPU, and pins the
CPU / GPU parity of the formulas (the same E budget holds on both)."""
import pytest
import torch

import gram_reference as GR
from libskylark_amd import ml

DTYPES = [torch.float32, torch.float64]


def _case(kid, dt, shape, signed=False):
    _, kind, params = next(k for k in GR.KERNELS if k[0] == kid)
    m, n, d = shape
    if signed:
        params = GR.signed_params(kind, params, d)
    X, Y = GR.points(m, n, d, dt, signed)
    return kind, params, GR.make_kernel(ml, kind, params, d), X, Y


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", GR.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kid", GR.KERNEL_IDS)
def test_cpu_gram(kid, shape, dt):
    kind, params, k, X, Y = _case(kid, dt, shape)
    u = GR.unit(dt)
    K, Q = GR.cached_ref(("cpu", shape, dt, "xy"), kind, params, X, Y)
    tag = f"cpu/{kid}/{str(dt)[6:]}"
    GR.check(tag, k.gram(X, Y=Y), K, Q, u)
    # points as columns: the operands are the transposes, the Gram is the same
    GR.check(tag, k.gram(X.t().contiguous(), dirX="columns", dirY="columns", Y=Y.t().contiguous()), K, Q, u)
    GR.check(tag, k.gram(X.t().contiguous(), dirX="columns", dirY="rows", Y=Y), K, Q, u)
    out = torch.full((shape[0], shape[1]), float("nan"), dtype=dt)
    assert k.gram(X, K=out, Y=Y) is out
    GR.check(tag, out, K, Q, u)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", GR.LAYOUT_SHAPES + [(1, 1, 1), (5, 4, 200)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kid", GR.KERNEL_IDS)
def test_cpu_symmetric_gram(kid, shape, dt):
    kind, params, k, X, _ = _case(kid, dt, shape)
    u = GR.unit(dt)
    K, Q = GR.cached_ref(("cpu", shape, dt, "xx"), kind, params, X, X)
    B = GR.bound(K, Q, u)
    tag = f"cpu-sym/{kid}/{str(dt)[6:]}"
    Kg = k.gram(X, Y=X)
    for Ks in (k.gram(X), k.symmetric_gram(X), k.symmetric_gram(X.t().contiguous(), "columns")):
        GR.check(tag, Ks, K, Q, u)
        GR.check_abs(tag + "/vs-general", Ks, GR._ld(Kg), B)
        GR.check_abs(tag + "/symmetry", Ks, GR._ld(Ks).T, 2 * B)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kid", ["linear", "gaussian", "poly2", "poly3", "laplacian", "expsemigroup"])
def test_cpu_gram_signed_points(kid, dt):
    """Standard-normal points: negative polynomial bases with q = 2 and 3, and
    the exp-semigroup kernel on negative coordinates (both paths take
    sqrt(|x + y|))."""
    shape = (65, 63, 33)
    kind, params, k, X, Y = _case(kid, dt, shape, signed=True)
    K, Q = GR.cached_ref(("cpu-signed", shape, dt), kind, params, X, Y)
    if kind == "polynomial":
        assert (Q["base"] < 0).any() and (Q["base"] > 0).any()
    if kind == "expsemigroup":
        assert ((X[:, None, :] + Y[None, :, :]) < 0).any()
    GR.check(f"cpu-signed/{kid}/{str(dt)[6:]}", k.gram(X, Y=Y), K, Q, GR.unit(dt))


def test_reference_is_the_definition():
    """The helper against hand-evaluated values (two points in the plane)."""
    X = torch.tensor([[1.0, 2.0]], dtype=torch.float64)
    Y = torch.tensor([[0.5, -1.0], [1.0, 2.0]], dtype=torch.float64)
    import math
    want = {
        ("linear", ()): [-1.5, 5.0],
        ("gaussian", (("sigma", 2.0),)): [math.exp(-9.25 / 8), 1.0],
        ("polynomial", (("q", 3), ("c", 1.0), ("gamma", 0.5))): [0.25 ** 3, 3.5 ** 3],
        ("laplacian", (("sigma", 2.0),)): [math.exp(-3.5 / 2), 1.0],
        ("expsemigroup", (("beta", 0.5),)): [math.exp(-0.5 * (math.sqrt(1.5) + 1.0)), math.exp(-0.5 * (math.sqrt(2) + 2))],
        ("matern", (("nu", 0.5), ("l", 2.0))): [math.exp(-math.sqrt(9.25) / 2), 1.0],
        ("matern", (("nu", 1.5), ("l", 2.0))): [(1 + math.sqrt(3 * 9.25) / 2) * math.exp(-math.sqrt(3 * 9.25) / 2), 1.0],
        ("matern", (("nu", 2.5), ("l", 2.0))): [(1 + math.sqrt(5 * 9.25) / 2 + 5 * 9.25 / 12)
                                                 * math.exp(-math.sqrt(5 * 9.25) / 2), 1.0],
    }
    for (kind, p), w in want.items():
        K, _ = GR.ref(kind, dict(p), X, Y)
        assert abs(float(K[0, 0]) - w[0]) <= 1e-15 * max(1.0, abs(w[0])), (kind, p)
        assert abs(float(K[0, 1]) - w[1]) <= 1e-15 * max(1.0, abs(w[1])), (kind, p)
    n = GR.ref_sqnorms(Y)
    assert float(n[0]) == 1.25 and float(n[1]) == 5.0
    assert float(GR.ref_distance(0, X, Y)[0, 0]) == 3.5


def test_bound_rejects_a_wrong_stride():
    """The bound is tight enough to see one misplaced coordinate: a Gram whose
    last coordinate of Y is taken from the neighbouring point fails it."""
    for kid in GR.KERNEL_IDS:
        kind, params, k, X, Y = _case(kid, torch.float64, (65, 63, 33))
        K, Q = GR.cached_ref(("cpu", (65, 63, 33), torch.float64, "xy"), kind, params, X, Y)
        Yw = Y.clone()
        Yw[:-1, -1] = Y[1:, -1]
        with pytest.raises(AssertionError):
            GR.check("cpu/wrong-stride", k.gram(X, Y=Yw), K, Q, GR.unit(torch.float32))
