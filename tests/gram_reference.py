"""Long-double reference and rounding bounds for the kernel Grams.

``ref(kind, params, X, Y)`` evaluates the six kernels from their definitions
(never from the GEMM form ``|x|^2 + |y|^2 - 2 x.y``) in numpy ``longdouble``
on the CPU; ``bound`` gives the componentwise error a correct implementation
in the working dtype may show,

    B_ij = P_ij + E * u * (1 + |arg_ij|) * |K_ref_ij|

with ``u`` the unit roundoff of the working dtype, ``arg`` the argument handed
to ``exp`` (``q log|base|`` for ``pow``), ``P`` the first-order propagated
error of that argument and ``E`` the ulp budget of the transcendental.  The
native library is not imported here: the module also serves the CPU-only
tests.

Propagated terms (d = point dimension, S_ij = sum_k |x_ik y_jk|):

* Laplacian / exp-semigroup: D is a sum of d non-negative terms, so
  ``|dD| <= (d + 2) u D`` and ``P = scale (d + 2) u D K``; a raw distance has
  ``P = (d + 2) u D`` and nothing else.
* Gaussian: ``delta = (d + 4) u (xn_i + yn_j + 2 S_ij)`` bounds the error of
  the squared distance formed as ``xn + yn - 2 G`` (the clamp at 0 only moves
  it toward the truth); ``P = a delta K``.
* Matern: ``r = sqrt(d2) / l``, ``|dr| <= min(sqrt(delta), delta / (2
  sqrt(d2))) / l`` and all three closed forms have ``|dK/dr| <= 1``, so
  ``P = |dr|``.
* polynomial: ``base = gamma g + c``, ``P = q |base|^(q-1) gamma (d + 2) u S``.
* linear: ``P = (d + 2) u S`` with no E term.
* fused (split-bf16 MFMA) Gram: the inner-product term ``(d + 2) u S`` (or
  the ``2 S`` part of ``delta``) becomes ``F * 2^-16 * S``.
* squared norms (f64 accumulation, one rounding to T):
  ``|out - ref| <= (u_T + (d / 64 + 8) 2^-53) ref``.
"""
import math

import numpy as np

LD = np.longdouble
KINDS = ("linear", "gaussian", "polynomial", "laplacian", "expsemigroup", "matern")

# ulp budget of exp / __expf / pow / powf: twice the largest value any case
# needed against the long-double reference, rounded up to a power of two
# (ceiling 32).  Measured on an MI355X: 0.894 (sl_gram_map polynomial q = 2,
# f32; f64 0.765), every exp case 0 (the propagated term alone covers them);
# the CPU path needed 0.163 (polynomial q = 3, f64).
MEASURED_E = 0.894
E = 2.0
# factor on the documented 2^-16 inner-product error of the fused Gram
# (ceiling 4), set the same way.  Measured on an MI355X, with no help from the
# E term: 0.671 (polynomial q = 3; Gaussian 0.535).
MEASURED_F = 0.671
F = 2.0
FUSED_EPS = 2.0 ** -16

U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}

# largest error / bound, needed E and needed F seen by check(), keyed by tag
STATS = {}


def unit(dtype):
    """Unit roundoff of a torch / numpy dtype (or its name)."""
    return U[str(dtype).replace("torch.", "")]


def _ld(A):
    if hasattr(A, "detach"):
        A = A.detach().cpu().numpy()
    return np.asarray(A).astype(LD)


def _pair_sum(X, Y, f, chunk=1 << 22):
    """out[i, j] = sum_k f(X[i, k], Y[j, k]) in long double, rows in chunks."""
    m, d = X.shape
    n = Y.shape[0]
    out = np.empty((m, n), dtype=LD)
    step = max(1, chunk // max(1, n * d))
    for i in range(0, m, step):
        out[i:i + step] = f(X[i:i + step, None, :], Y[None, :, :]).sum(-1)
    return out


def ref(kind, params, X, Y):
    """``(K_ref, Q)``: the long-double Gram of the points X (m x d) and Y
    (n x d), already rounded to the working dtype, and the intermediates the
    bounds need (``d``, ``S``, and per kind ``G``, ``xn``, ``yn``, ``d2``,
    ``D``, ``arg``)."""
    X, Y = _ld(X), _ld(Y)
    p = dict(params)
    d = X.shape[1]
    Q = {"kind": kind, "params": p, "d": d}
    if kind in ("linear", "polynomial", "gaussian", "matern"):
        Q["S"] = _pair_sum(X, Y, lambda a, b: np.abs(a * b))
    if kind in ("linear", "polynomial"):
        Q["G"] = _pair_sum(X, Y, lambda a, b: a * b)
    if kind in ("gaussian", "matern"):
        Q["xn"], Q["yn"] = (X * X).sum(1), (Y * Y).sum(1)
        Q["d2"] = _pair_sum(X, Y, lambda a, b: (a - b) ** 2)
    if kind == "linear":
        K = Q["G"]
    elif kind == "polynomial":
        q, c, gamma = int(p["q"]), LD(p["c"]), LD(p["gamma"])
        base = gamma * Q["G"] + c
        Q["base"] = base
        with np.errstate(divide="ignore"):
            Q["arg"] = q * np.log(np.abs(base))
        Q["arg"][base == 0] = 0
        K = base ** q
    elif kind == "gaussian":
        a = 1 / (2 * LD(p["sigma"]) ** 2)
        Q["arg"] = a * Q["d2"]
        K = np.exp(-Q["arg"])
    elif kind == "laplacian":
        Q["D"] = _pair_sum(X, Y, lambda a, b: np.abs(a - b))
        Q["scale"] = 1 / LD(p["sigma"])
        Q["arg"] = Q["scale"] * Q["D"]
        K = np.exp(-Q["arg"])
    elif kind == "expsemigroup":
        Q["D"] = _pair_sum(X, Y, lambda a, b: np.sqrt(np.abs(a + b)))
        Q["scale"] = LD(p["beta"])
        Q["arg"] = Q["scale"] * Q["D"]
        K = np.exp(-Q["arg"])
    elif kind == "matern":
        nu, l = float(p["nu"]), LD(p["l"])  # noqa: E741
        r = np.sqrt(Q["d2"]) / l
        t = np.sqrt(LD(2 * nu)) * r
        Q["arg"] = t
        if nu == 0.5:
            K = np.exp(-t)
        elif nu == 1.5:
            K = (1 + t) * np.exp(-t)
        elif nu == 2.5:
            K = (1 + t + t * t / 3) * np.exp(-t)
        else:
            raise ValueError("matern reference: nu must be 0.5, 1.5 or 2.5")
    else:
        raise ValueError(f"unknown kernel {kind}")
    return K, Q


def ref_distance(mode, X, Y):
    """Raw distance matrices of the pairwise kernel: mode 0 sum_k |x_k - y_k|,
    mode 1 sum_k sqrt(|x_k + y_k|)."""
    X, Y = _ld(X), _ld(Y)
    if mode == 0:
        return _pair_sum(X, Y, lambda a, b: np.abs(a - b))
    return _pair_sum(X, Y, lambda a, b: np.sqrt(np.abs(a + b)))


def bound_distance(D, d, u):
    return (d + 2) * u * D


def ref_sqnorms(X):
    X = _ld(X)
    return (X * X).sum(1)


def bound_sqnorms(nref, d, u):
    return (u + (d / 64 + 8) * 2.0 ** -53) * nref


def _delta(Q, u, fused):
    xy = Q["xn"][:, None] + Q["yn"][None, :]
    if fused is None:
        return (Q["d"] + 4) * u * (xy + 2 * Q["S"])
    return (Q["d"] + 4) * u * xy + 2 * fused * FUSED_EPS * Q["S"]


def parts(K, Q, u, fused=None):
    """``(P, T)`` with ``bound = P + E * T``: the propagated term and the
    per-ulp transcendental term.  ``fused``: the factor F on 2^-16 for the
    split-bf16 path, None for plain working-precision inner products."""
    kind, p, d = Q["kind"], Q["params"], Q["d"]
    aK = np.abs(K)
    ip = (d + 2) * u if fused is None else fused * FUSED_EPS
    if kind == "linear":
        return ip * Q["S"], np.zeros_like(aK)
    T = u * (1 + np.abs(Q["arg"])) * aK
    if kind == "polynomial":
        q, gamma = int(p["q"]), abs(LD(p["gamma"]))
        return q * np.abs(Q["base"]) ** (q - 1) * gamma * ip * Q["S"], T
    if kind in ("laplacian", "expsemigroup"):
        return Q["scale"] * (d + 2) * u * Q["D"] * aK, T
    delta = _delta(Q, u, fused)
    if kind == "gaussian":
        return delta / (2 * LD(p["sigma"]) ** 2) * aK, T
    if kind == "matern":
        with np.errstate(divide="ignore", invalid="ignore"):
            lin = np.where(Q["d2"] > 0, delta / (2 * np.sqrt(Q["d2"])), np.inf)
        return np.minimum(np.sqrt(delta), lin) / LD(p["l"]), T
    raise ValueError(f"unknown kernel {kind}")


def bound(K, Q, u, fused=None, e=None):
    P, T = parts(K, Q, u, fused)
    return P + (E if e is None else e) * T


def _record(tag, **kw):
    s = STATS.setdefault(tag, {})
    for k, v in kw.items():
        s[k] = max(s.get(k, 0.0), float(v))


def check_abs(tag, got, want, B):
    """|got - want| <= B componentwise (NaN fails); records max error / bound."""
    got = _ld(got)
    err = np.abs(got - want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert not np.isnan(err).any(), f"{tag}: NaN in the result"
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / B, 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    _record(tag, ratio=worst)
    print(f"{tag}: max err {float(err.max()) if err.size else 0.0:.3e}  err/bound {worst:.3f}")
    assert worst <= 1.0, f"{tag}: error / bound = {worst:.3f} at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    return worst


def check(tag, got, K, Q, u, fused=None):
    """``got`` against the reference ``K`` under ``bound``; records, per tag,
    the largest error / bound and the E (or, fused, the F) the case needed."""
    gl = _ld(got)
    err = np.abs(gl - K)
    P, T = parts(K, Q, u, fused)
    with np.errstate(divide="ignore", invalid="ignore"):
        if fused is None:
            need_e = np.where(err > P, (err - P) / T, 0.0)
            need_e = np.where(np.isfinite(need_e), need_e, 0.0)
            _record(tag, need_E=need_e.max() if need_e.size else 0.0)
        else:
            # the F that covers the error with no help from the E term (an
            # upper estimate: the E term is ~2^-19 relative, the F term ~2^-16)
            P0, _ = parts(K, Q, u, 0.0)
            P1, _ = parts(K, Q, u, 1.0)
            need_f = np.where(err > P0, (err - P0) / (P1 - P0), 0.0)
            need_f = np.where(np.isfinite(need_f), need_f, 0.0)
            _record(tag, need_F=need_f.max() if need_f.size else 0.0)
    return check_abs(tag, got, K, P + E * T)


# the smallest shapes that cross every edge of the kernels: the 64-wide output
# tile, the 32-wide d slab, the 16-lane micro-tile stride, the four points per
# workgroup of the norm kernel and its 64-lane stride over d
SHAPES = [(1, 1, 1), (64, 64, 32), (65, 63, 33), (63, 65, 31), (130, 67, 70), (3, 129, 64), (5, 4, 200)]
LAYOUT_SHAPES = [(65, 63, 33), (130, 67, 70)]

# (id, kind, params): polynomial with distinct q, c, gamma (a swapped order
# gives another matrix), Laplacian sigma != 1 (sigma is not 1 / sigma)
KERNELS = [
    ("linear", "linear", {}),
    ("gaussian", "gaussian", {"sigma": 1.3}),
    ("poly2", "polynomial", {"q": 2, "c": 0.75, "gamma": 0.3}),
    ("poly3", "polynomial", {"q": 3, "c": -0.5, "gamma": 0.125}),
    ("laplacian", "laplacian", {"sigma": 2.5}),
    ("expsemigroup", "expsemigroup", {"beta": 0.1}),
    ("matern05", "matern", {"nu": 0.5, "l": 1.7}),
    ("matern15", "matern", {"nu": 1.5, "l": 1.7}),
    ("matern25", "matern", {"nu": 2.5, "l": 1.7}),
]
KERNEL_IDS = [k[0] for k in KERNELS]


def signed_params(kind, params, d):
    """Standard-normal points are ~sqrt(2 d) apart (L1: ~1.13 d): widen sigma
    with d so that the kernel value stays far above the f32 underflow
    threshold, where the relative bounds would not apply."""
    if kind == "gaussian":
        return {"sigma": params["sigma"] * math.sqrt(d)}
    if kind == "laplacian":
        return {"sigma": params["sigma"] + 0.125 * d}
    return params


def make_kernel(ml, kind, params, d):
    cls = {"linear": ml.Linear, "gaussian": ml.Gaussian, "polynomial": ml.Polynomial, "laplacian": ml.Laplacian,
           "expsemigroup": ml.ExpSemigroup, "matern": ml.Matern}[kind]
    return cls(d, **params)


def points(m, n, d, dtype, signed=False):
    """CPU points X (m x d), Y (n x d) in ``dtype``: uniform in [0, 1) (or
    standard normal), with a block of coincident points ``Y[:h] = X[:h]`` so
    that Gaussian and Matern meet d2 = 0."""
    import torch
    g = torch.Generator().manual_seed(1000 * m + 10 * n + d + (7 if signed else 0))
    f = torch.randn if signed else torch.rand
    X = f(m, d, generator=g, dtype=dtype)
    Y = f(n, d, generator=g, dtype=dtype)
    h = min(m, n, 3)
    Y[:h] = X[:h]
    return X, Y


_REF = {}


def cached_ref(key, kind, params, X, Y):
    """``ref`` once per ``key`` (shape, dtype, data and kernel): the
    parametrised cases share it and leave it unchanged."""
    k = (key, kind, tuple(sorted(params.items())))
    if k not in _REF:
        _REF[k] = ref(kind, params, X, Y)
    return _REF[k]


def pow2_ceil(x):
    return 2.0 ** math.ceil(math.log2(x)) if x > 0 else 0.0
