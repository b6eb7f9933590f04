"""Long-double reference and rounding bounds for the Krylov device steps.

One function per device step of ``krylov_kernels.hip``, written from the
definitions of the reference algorithms (``LSQR.hpp`` steps 1-12, ``CG.hpp``,
``FlexibleCG.hpp``) in numpy ``longdouble`` on the CPU.  A test hands each
function the device's own inputs (vectors and state copied off the GPU before
the call), so one call is judged at a time and errors do not compound.  The
native library is not imported here: the module also serves the CPU-only
tests.

Bounds (``u_T`` the unit roundoff of the working dtype, ``u`` = 2^-53):

* element-wise outputs: ``u_T |ref| + N u S`` with ``S`` the sum of the
  absolute addends; the kernel forms the element in f64 from ``N - 1``
  roundings at most and rounds once to ``T``.  N = 8 except ``lsqr_step``
  (N = 10), counted in each function's docstring;
* column reductions over m rows in f64: ``(m + 16) u sum|terms|``, against the
  long-double sum of the array the device wrote;
* ``rows_gemm``: ``u_T |ref| + (nc + 16) u sum|m x|``;
* scalar state: ``C u |ref|``, plus, where a row depends on a reduction, the
  change of that row when the sum moves by its bound (every row is monotone
  in its sums, so the two ends of the interval give the whole range);
* flags, the stagnation count and rows a call does not own: exact.

The oracle refuses inputs on which its verdict would be fragile
(``GuardError``): a flag comparison whose two sides are within a factor of
two, cancellation in the |x| recurrence (``|rhs| < (|phi| + |delta zz|) / 2``)
and a zero denominator the case did not announce.
"""
import itertools
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "krylov_reference needs the 64-bit-mantissa long double"

U64 = 2.0 ** -53
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}

# relative error of the scalar state (Givens quantities, |A^T r|, the |x|
# recurrence, CG alpha / beta given their dot) in units of u: twice the
# largest value any case needed against this reference, rounded up to a power
# of two (ceiling 64).  Measured on an MI355X: 4.602 (six real LSQR
# iterations, f64 vectors; the crafted and per-shape ``lsqr_step`` states 4.244,
# ``finish_state`` 1.478, ``setstate`` 1.326; every CG row 0: the reduction
# term alone covers alpha and beta).
MEASURED_C = 4.602
C = 16.0

# LSQR state rows (the layout ``ops.krylov_native`` documents)
LSQR_ROWS = ("alpha", "beta", "rhobar", "phibar", "nrm_a", "sq_d", "cnd_a", "nrm_x", "sq_x", "cs2", "sn2", "zz",
             "nrm_ar0", "stag", "rho", "phi", "theta", "nrm_ar")
(S_ALPHA, S_BETA, S_RHOBAR, S_PHIBAR, S_NRMA, S_SQD, S_CNDA, S_NRMX, S_SQX, S_CS2, S_SN2, S_ZZ, S_NRMAR0, S_STAG,
 S_RHO, S_PHI, S_THETA, S_NRMAR) = range(18)
# rows lsqr_step writes / leaves alone
LSQR_STEP_KEEPS = (S_ALPHA, S_BETA, S_NRMA, S_NRMAR0)
CG_ROWS = ("rho", "rho0", "alpha", "beta", "pq", "rr", "nrmb")
C_RHO, C_RHO0, C_ALPHA, C_BETA, C_PQ, C_RR, C_NRMB = range(7)

# largest error / bound and needed C seen by the checks, keyed by tag
STATS = {}


class GuardError(ValueError):
    """The case is too close to a branch (or divides by zero unannounced)."""


def unit(dtype):
    return U[str(dtype).replace("torch.", "")]


def _ld(A):
    if A is None:
        return None
    if hasattr(A, "detach"):
        A = A.detach().cpu().numpy()
    return np.asarray(A).astype(LD)


def _apart(tag, a, b, guard):
    """Both sides of a comparison at least a factor of two apart."""
    if not guard:
        return
    a, b = np.abs(a), np.abs(b)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    bad = ~(hi >= 2 * lo) | (hi == 0)
    if bad.any():
        raise GuardError(f"{tag}: sides within a factor of two in columns {np.nonzero(bad)[0].tolist()}")


def _nonzero(tag, v, zero_ok=()):
    z = np.nonzero(np.asarray(v) == 0)[0].tolist()
    bad = [c for c in z if c not in set(zero_ok)]
    if bad:
        raise GuardError(f"{tag}: zero denominator in columns {bad}")


# ------------------------------------------------------------- vector steps
def colred(X, Y=None):
    """Column sums of squares, or column dots with Y."""
    X = _ld(X)
    return (X * X).sum(0) if Y is None else (X * _ld(Y)).sum(0)


def colred_abs(X, Y=None):
    X = _ld(X)
    return (X * X).sum(0) if Y is None else np.abs(X * _ld(Y)).sum(0)


def red_bound(X, Y=None):
    """``(m + 16) u sum|terms|`` of the column reduction over X (and Y)."""
    return (np.shape(X)[0] + 16) * U64 * colred_abs(X, Y)


def axpby(X, Y, a=None, sa=1.0, b=None, sb=1.0, d=None):
    """``(sa a .* X + sb b .* Y) ./ d`` -> (ref, S).  None: a = 1, d = 1; a
    None b leaves the old Y unread; ``d[c] == 0`` gives a zero column.
    Device roundings: 1 / d, a / d, (a / d) x, b / d, (b / d) y, the sum: 6."""
    X = _ld(X)
    k = X.shape[1]
    av = np.ones(k, LD) if a is None else _ld(a)
    dv = np.ones(k, LD) if d is None else _ld(d)
    num = LD(sa) * av * X
    S = np.abs(av * X)
    if b is not None:
        Y = _ld(Y)
        num = num + LD(sb) * _ld(b) * Y
        S = S + np.abs(_ld(b) * Y)
    nz = dv != 0
    safe = np.where(nz, dv, 1)
    return np.where(nz, num / safe, 0), np.where(nz, S / np.abs(safe), 0)


def colscale(Y, s, inv=False):
    """``Y .* s`` or ``Y ./ s`` -> (ref, S); a zero divisor gives 0, a negative
    one divides.  Device roundings: 1 / s, the product: 2."""
    Y, s = _ld(Y), _ld(s)
    if inv:
        nz = s != 0
        ref = np.where(nz, Y / np.where(nz, s, 1), 0)
    else:
        ref = Y * s
    return ref, np.abs(ref)


def finish_state(st, sums, mode):
    """LSQR steps 1-3's scalars from a column sum of squares: mode 1 beta =
    sqrt(sum) and |A|' = sqrt(|A|^2 + alpha^2 + beta^2) (the alpha before the
    step); mode 2 alpha = sqrt(sum)."""
    st, sums = _ld(st).copy(), _ld(sums)
    if mode == 1:
        st[S_NRMA] = np.sqrt(st[S_NRMA] ** 2 + st[S_ALPHA] ** 2 + sums)
        st[S_BETA] = np.sqrt(sums)
    elif mode == 2:
        st[S_ALPHA] = np.sqrt(sums)
    else:
        raise ValueError("finish_state: mode 1 or 2")
    return st


# ---------------------------------------------------------------------- LSQR
def _rotation(st):
    """Step 4 from the state before the step."""
    rhobar, beta, alpha, phibar = st[S_RHOBAR], st[S_BETA], st[S_ALPHA], st[S_PHIBAR]
    rho = np.sqrt(rhobar * rhobar + beta * beta)
    _nonzero("lsqr rho", rho)
    cs, sn = rhobar / rho, beta / rho
    return dict(rho=rho, cs=cs, sn=sn, theta=sn * alpha, rhobar=-cs * alpha, phi=cs * phibar, phibar=sn * phibar)


def lsqr_xw(X, W, Z, st):
    """Step 5: ``X + (phi / rho) W`` and ``Z - (theta / rho) W`` -> (Xn, SX,
    Wn, SW).  Device roundings of the second addend: rho^2 (2, halved by the
    root), the root, cs or sn, phi or theta, the quotient by rho (+ rho's 2),
    the product with w, then the sum: 9, so N = 10 here."""
    X, W, Z, st = _ld(X), _ld(W), _ld(Z), _ld(st)
    g = _rotation(st)
    fx, fw = g["phi"] / g["rho"], g["theta"] / g["rho"]
    return X + fx * W, np.abs(X) + np.abs(fx * W), Z - fw * W, np.abs(Z) + np.abs(fw * W)


def lsqr_scalars(st, nw2, tol, eps, max_stag, guard=True):
    """Steps 4, 6-12 given ``nw2`` = |W|^2 of the new W -> (state, flags).
    Flag bits: 1 S1, 2 S2, 4 S3, 8 stagnation."""
    st, nw2 = _ld(st).copy(), _ld(nw2)
    tol, eps = LD(tol), LD(eps)
    g = _rotation(st)
    alpha, nrm_a = st[S_ALPHA], st[S_NRMA]
    nrm_w = np.sqrt(nw2)
    # 6-7
    nrm_r = g["phibar"]
    nrm_ar = np.abs(g["phibar"] * alpha * g["cs"])
    _apart("S1", nrm_ar, tol * st[S_NRMAR0], guard)
    _apart("S2", nrm_ar, eps * nrm_a * nrm_r, guard)
    flags = np.zeros(st.shape[1], np.int64)
    flags |= np.where(nrm_ar < tol * st[S_NRMAR0], 1, 0)
    flags |= np.where(nrm_ar < eps * nrm_a * nrm_r, 2, 0)
    # 9-10
    sq_d = st[S_SQD] + nw2 / (g["rho"] * g["rho"])
    cnd = nrm_a * np.sqrt(sq_d)
    _apart("S3", cnd, np.full_like(cnd, 1 / eps), guard)
    flags |= np.where(cnd > 1 / eps, 4, 0)
    # 11
    lhs, rhs_s = np.abs(g["phi"] / g["rho"]) * nrm_w, eps * st[S_NRMX]
    _apart("stagnation", lhs, rhs_s, guard)
    stag = np.where(lhs < rhs_s, st[S_STAG] + 1, 0)
    flags |= np.where(stag >= max_stag, 8, 0)
    # 12
    delta = st[S_SN2] * g["rho"]
    gambar = -st[S_CS2] * g["rho"]
    rhs = g["phi"] - delta * st[S_ZZ]
    if guard and (np.abs(rhs) < (np.abs(g["phi"]) + np.abs(delta * st[S_ZZ])) / 2).any():
        raise GuardError("|x| recurrence: phi - delta zz cancels")
    _nonzero("lsqr gambar", gambar)
    zbar = rhs / gambar
    gamma = np.sqrt(gambar * gambar + g["theta"] * g["theta"])
    zz = rhs / gamma
    st[S_NRMX] = np.sqrt(st[S_SQX] + zbar * zbar)
    st[S_CS2], st[S_SN2], st[S_ZZ] = gambar / gamma, g["theta"] / gamma, zz
    st[S_SQX] = st[S_SQX] + zz * zz
    st[S_SQD], st[S_CNDA], st[S_STAG] = sq_d, cnd, stag
    st[S_RHOBAR], st[S_PHIBAR] = g["rhobar"], g["phibar"]
    st[S_RHO], st[S_PHI], st[S_THETA], st[S_NRMAR] = g["rho"], g["phi"], g["theta"], nrm_ar
    return st, flags


def lsqr_step(X, W, Z, st, tol, eps, max_stag, guard=True):
    """Steps 4-12 -> (new X, new W, the 18 state rows, flags)."""
    Xn, _, Wn, _ = lsqr_xw(X, W, Z, st)
    stn, flags = lsqr_scalars(st, colred(Wn), tol, eps, max_stag, guard)
    return Xn, Wn, stn, flags


# ------------------------------------------------------------------ CG / FCG
def cg_scalars(mode, st, t1, t2=None, zero_ok=()):
    """The epilogue of ``cg_dot`` given the dot(s): mode 0 alpha = rho / t1;
    1 rho0 = rho, rho = t1, beta = rho / rho0; 2 (FCG) beta = t1 / pq; 3 (FCG)
    pq = t1, alpha = t2 / pq.  A zero denominator gives 0 (announced columns only)."""
    st, t1 = _ld(st).copy(), _ld(t1)

    def div(tag, a, b):
        _nonzero(tag, b, zero_ok)
        return np.where(b != 0, a / np.where(b != 0, b, 1), 0)
    if mode == 0:
        st[C_ALPHA] = div("cg alpha", st[C_RHO], t1)
    elif mode == 1:
        rho0 = st[C_RHO].copy()
        st[C_RHO0], st[C_RHO] = rho0, t1
        st[C_BETA] = div("cg beta", t1, rho0)
    elif mode == 2:
        st[C_BETA] = div("fcg beta", t1, st[C_PQ])
    elif mode == 3:
        st[C_PQ] = t1
        st[C_ALPHA] = div("fcg alpha", _ld(t2), t1)
    else:
        raise ValueError("cg_dot: mode 0..3")
    return st


def cg_dot(mode, X, Y, Y2, st, zero_ok=()):
    return cg_scalars(mode, st, colred(X, Y), colred(X, Y2) if mode == 3 else None, zero_ok)


def cg_p(Z, P, st, sb=1.0):
    """``Z + sb beta .* P`` -> (ref, S).  Device roundings: product, sum: 2."""
    Z, P, st = _ld(Z), _ld(P), _ld(st)
    t = LD(sb) * st[C_BETA] * P
    return Z + t, np.abs(Z) + np.abs(t)


def cg_xr_vectors(X, P, R, Q, st):
    """``X + alpha P``, ``R - alpha Q`` -> (Xn, SX, Rn, SR); 2 roundings each."""
    X, P, R, Q, al = _ld(X), _ld(P), _ld(R), _ld(Q), _ld(st)[C_ALPHA]
    return X + al * P, np.abs(X) + np.abs(al * P), R - al * Q, np.abs(R) + np.abs(al * Q)


def cg_xr_scalars(st, rr, idp, tol, guard=True, zero_ok=()):
    """rr = |R|^2, flag = |R| < tol |B|; idp: rho0 = rho, rho = rr, beta = rr / rho0."""
    st, rr = _ld(st).copy(), _ld(rr)
    _apart("cg stop", np.sqrt(rr), LD(tol) * st[C_NRMB], guard)
    flags = np.where(np.sqrt(rr) < LD(tol) * st[C_NRMB], 1, 0).astype(np.int64)
    st[C_RR] = rr
    if idp:
        rho0 = st[C_RHO].copy()
        _nonzero("cg beta", rho0, zero_ok)
        st[C_RHO0], st[C_RHO] = rho0, rr
        st[C_BETA] = np.where(rho0 != 0, rr / np.where(rho0 != 0, rho0, 1), 0)
    return st, flags


def cg_xr(X, P, R, Q, st, idp, tol, guard=True, zero_ok=()):
    Xn, _, Rn, _ = cg_xr_vectors(X, P, R, Q, st)
    stn, flags = cg_xr_scalars(st, colred(Rn), idp, tol, guard, zero_ok)
    return Xn, Rn, stn, flags


def rows_gemm(M, X):
    """``M X`` -> (ref, S = |M| |X|)."""
    M, X = _ld(M), _ld(X)
    return M @ X, np.abs(M) @ np.abs(X)


# ------------------------------------------------------------ whole solvers
def lsqr_init(A, B):
    """The state before the first iteration (LSQR.hpp:55-98) -> (U, V, Z, W, X, st)."""
    A, B = _ld(A), _ld(B)
    k = B.shape[1]
    beta = np.sqrt(colred(B))
    U = B / beta
    V = A.T @ U
    alpha = np.sqrt(colred(V))
    V = V / alpha
    st = np.zeros((len(LSQR_ROWS), k), LD)
    st[S_ALPHA], st[S_BETA], st[S_RHOBAR], st[S_PHIBAR] = alpha, beta, alpha, beta
    st[S_NRMAR0], st[S_CS2] = alpha * beta, -1
    return U, V, V.copy(), V.copy(), np.zeros((A.shape[1], k), LD), st


def lsqr_iteration(A, U, V, W, X, Z, st, tol, eps, max_stag=3, guard=False):
    """One iteration out of the one-step functions -> (U, V, W, X, Z, st, flags)."""
    U, _ = axpby(A @ Z, U, b=st[S_ALPHA], sb=-1.0)
    st = finish_state(st, colred(U), 1)
    U, _ = colscale(U, st[S_BETA], inv=True)
    V, _ = axpby(A.T @ U, V, b=st[S_BETA], sb=-1.0)
    st = finish_state(st, colred(V), 2)
    V, _ = colscale(V, st[S_ALPHA], inv=True)
    Z = V.copy()
    X, W, st, flags = lsqr_step(X, W, Z, st, tol, eps, max_stag, guard)
    return U, V, W, X, Z, st, flags


def lsqr_code(flags):
    """The reference's return code of an iteration's flags (None: go on)."""
    if ((flags & 1) != 0).all():
        return -2
    if ((flags & 2) != 0).all():
        return -3
    if ((flags & 4) != 0).any():
        return -4
    if ((flags & 8) != 0).any():
        return -5
    return None


def lsqr_solve(A, B, tol, eps, iter_lim, guard=False):
    """Unpreconditioned LSQR out of the one-step functions -> (X, code, iterations)."""
    A = _ld(A)
    U, V, Z, W, X, st = lsqr_init(A, B)
    for itn in range(iter_lim):
        U, V, W, X, Z, st, flags = lsqr_iteration(A, U, V, W, X, Z, st, tol, eps, 3, guard)
        code = lsqr_code(flags)
        if code is not None:
            return X, code, itn + 1
    return X, -6, iter_lim


def cg_solve(A, B, tol, iter_lim, Minv=None, flexible=False, guard=False):
    """(Preconditioned, flexible) CG out of the one-step functions in the
    order the device solver issues them -> (X, code, iterations)."""
    A, B = _ld(A), _ld(B)
    Minv = _ld(Minv)
    n, k = B.shape
    st = np.zeros((len(CG_ROWS), k), LD)
    X, R = np.zeros((n, k), LD), B.copy()
    st[C_NRMB] = np.sqrt(colred(B))
    idp = Minv is None and not flexible
    if idp:
        st[C_RHO] = colred(R)
    P, Q = np.zeros((n, k), LD), None
    allz = tuple(range(k))
    for itn in range(iter_lim):
        Z = R if Minv is None else Minv @ R
        if flexible:
            if itn == 0:
                P = Z.copy()
            else:
                st = cg_dot(2, Q, Z, None, st)
                P, _ = cg_p(Z, P, st, -1.0)
        elif idp:
            P, _ = cg_p(R, P, st)
        else:
            st = cg_dot(1, R, Z, None, st, zero_ok=allz if itn == 0 else ())
            P, _ = cg_p(Z, P, st)
        Q = A @ P
        st = cg_dot(3, P, Q, R, st) if flexible else cg_dot(0, P, Q, None, st)
        X, R, st, flags = cg_xr(X, P, R, Q, st, idp, tol, guard)
        if flags.all():
            return X, -1, itn + 1
    return X, -6, iter_lim


# ------------------------------------------------------------------- bounds
def elem_bound(ref, S, u_t, n=8):
    return u_t * np.abs(ref) + n * U64 * S


def gemm_bound(ref, S, u_t, nc):
    return u_t * np.abs(ref) + (nc + 16) * U64 * S


def spread(f, sums, deltas):
    """``f(*sums)`` and the largest change of each entry when every sum moves
    to either end of ``sum +- delta`` (f monotone in each sum)."""
    base = f(*sums)
    dev = np.zeros_like(base)
    for sg in itertools.product((-1, 1), repeat=len(sums)):
        dev = np.maximum(dev, np.abs(f(*[s + g * d for s, g, d in zip(sums, sg, deltas)]) - base))
    return base, dev


def _record(tag, **kw):
    s = STATS.setdefault(tag, {})
    for k, v in kw.items():
        s[k] = max(s.get(k, 0.0), float(v))


def check_abs(tag, got, want, B):
    """|got - want| <= B componentwise (NaN fails); records max error / bound."""
    got = _ld(got)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    err = np.abs(got - want)
    assert not np.isnan(err).any(), f"{tag}: NaN in the result"
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / B, 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    _record(tag, ratio=worst)
    assert worst <= 1.0, (f"{tag}: error / bound = {worst:.3f} at "
                          f"{np.unravel_index(ratio.argmax(), ratio.shape)}")
    return worst


def check_scalar(tag, got, want, red=None, c=None):
    """Scalar state: ``|got - want| <= C u |want| + red``; records the C the
    case needed (error beyond the reduction term, in units of u |want|)."""
    got = _ld(got)
    red = np.zeros_like(want) if red is None else red
    err = np.abs(got - want)
    assert not np.isnan(err).any(), f"{tag}: NaN in the state"
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.where(err > red, (err - red) / (U64 * np.abs(want)), 0.0)
    assert np.isfinite(need).all(), f"{tag}: non-zero where the reference is zero"
    worst = float(need.max()) if need.size else 0.0
    _record(tag, need_C=worst)
    cc = C if c is None else c
    assert worst <= cc, f"{tag}: needs C = {worst:.2f} > {cc} at {np.unravel_index(need.argmax(), need.shape)}"
    return worst


def pow2_ceil(x):
    return 2.0 ** math.ceil(math.log2(x)) if x > 0 else 0.0


# --------------------------------------------------------------------- data
def data(m, k, seed):
    """m x k float64 entries of magnitude in [0.5, 2) with random signs: one
    dropped, doubled or misplaced row or column moves a column sum by ~1/m."""
    g = np.random.default_rng(seed)
    return g.uniform(0.5, 2.0, (m, k)) * g.choice([-1.0, 1.0], (m, k))


def scalars(k, seed, lo=0.5, hi=2.0, signed=True):
    """k distinct per-column scalars of magnitude in [lo, hi)."""
    g = np.random.default_rng(seed)
    v = np.sort(g.uniform(lo, hi, k))[g.permutation(k)] * (1 + 1e-3 * np.arange(k))
    return v * g.choice([-1.0, 1.0], k) if signed else v


CRAFT_K = 9
CRAFT_TOL, CRAFT_EPS, CRAFT_MAX_STAG = 1e-3, 1e-6, 3
# expected flags of the crafted columns: none, S1, S2, S3, stagnation reached,
# stagnation count reset, S1 + S3, first iteration, stagnation count advancing
CRAFT_FLAGS = (0, 1, 2, 4, 8, 0, 5, 0, 0)
CRAFT_STAG = (0, 0, 0, 0, 3, 0, 0, 0, 2)


def crafted_lsqr_state():
    """18 x 9 LSQR state whose columns meet every stop branch of steps 7-11
    once (``CRAFT_FLAGS``) with the vectors of ``crafted_lsqr_vectors``; all
    rows distinct across columns, the output-only rows pre-filled with junk."""
    k = CRAFT_K
    f = 1 + 0.03 * np.arange(k)
    st = np.zeros((len(LSQR_ROWS), k))
    st[S_ALPHA], st[S_BETA], st[S_RHOBAR], st[S_PHIBAR] = 1.3 * f, 0.9 / f, 1.1 * f, 0.7 * f
    st[S_NRMA], st[S_SQD], st[S_NRMX], st[S_SQX] = 2.0 * f, 0.5 * f, 1.5 * f, 2.0 / f
    st[S_CS2], st[S_SN2], st[S_ZZ], st[S_NRMAR0] = -0.8 / f, 0.6 * f, -0.4 * f, 1.0 * f
    for r in (S_CNDA, S_RHO, S_PHI, S_THETA, S_NRMAR):
        st[r] = 99.0 + r + np.arange(k)
    st[S_NRMAR0, 1] = 1e4                               # S1
    st[S_ALPHA, 2], st[S_NRMAR0, 2] = 1e-7, 1e-6        # S2 only
    st[S_SQD, 3] = 1e13                                 # S3
    st[S_STAG, 4], st[S_NRMX, 4] = CRAFT_MAX_STAG - 1, 1e8    # stagnation reached
    st[S_STAG, 5] = 2                                   # not stagnating: count reset
    st[S_NRMAR0, 6], st[S_SQD, 6] = 1e4, 1e13           # S1 + S3
    # the first iteration as the solver builds it
    st[S_ALPHA, 7], st[S_BETA, 7], st[S_RHOBAR, 7], st[S_PHIBAR, 7] = 1.1, 0.8, 1.25, 3.0
    st[S_NRMA, 7], st[S_NRMAR0, 7], st[S_CS2, 7] = 1.5, 3.75, -1.0
    for r in (S_SQD, S_NRMX, S_SQX, S_SN2, S_ZZ):
        st[r, 7] = 0.0
    st[S_STAG, 8], st[S_NRMX, 8] = 1, 3e8               # stagnating, below the limit
    return st


def crafted_lsqr_vectors(n=37):
    return data(n, CRAFT_K, 901), data(n, CRAFT_K, 902), data(n, CRAFT_K, 903)


def lsqr_problem(m=200, n=24, k=5, seed=5):
    """Well-conditioned m x n operator (singular values in [1, 4]) and k right-hand sides."""
    g = np.random.default_rng(seed)
    Q1, _ = np.linalg.qr(g.standard_normal((m, n)))
    Q2, _ = np.linalg.qr(g.standard_normal((n, n)))
    return (Q1 * np.linspace(1.0, 4.0, n)) @ Q2.T, data(m, k, seed + 1)


def spd_problem(n=96, k=5, seed=9):
    """SPD n x n matrix (eigenvalues in [1, 30]), k right-hand sides and a
    diagonal-dominant SPD approximate inverse for the preconditioned runs."""
    g = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(g.standard_normal((n, n)))
    A = (Q * np.linspace(1.0, 30.0, n)) @ Q.T
    A = (A + A.T) / 2
    return A, data(n, k, seed + 1), np.diag(1.0 / np.diag(A))


# ----------------------------------------------------- shapes and CG cases
KS = (1, 2, 3, 5, 8, 9, 17, 33, 63, 64)


def kp_of(k):
    return 1 << max(0, (k - 1).bit_length())


def block_rows(k):
    """Rows one 256-thread block covers: 8 per thread row, 256 / KP thread rows."""
    return 8 * (256 // kp_of(k))


def small_ms(k):
    return (1, block_rows(k), block_rows(k) + 1)


# the smallest sizes that cross the clamps of the partial-block grid (1024
# blocks; 256 for the CG passes)
CLAMP_1024 = ((1024 * block_rows(33) + 37, 33), (1024 * block_rows(64) + 37, 64))
CLAMP_256 = ((256 * block_rows(64) + 37, 64), (256 * block_rows(17) + 37, 17))

CG_TOL = 0.5
# announced zero denominators of the crafted CG cases (k >= 3): X's column 0
# is zero (modes 0 and 3: X . Y = 0), rho[1] = 0 (mode 1 and cg_xr's rho0),
# pq[2] = 0 (mode 2)
CG_ZERO = {0: (0,), 1: (1,), 2: (2,), 3: (0,), "xr": (1,)}


def cg_zero_ok(which, k):
    return CG_ZERO[which] if k >= 3 else ()


def crafted_cg_state(k, m):
    """7 x k CG state, rows distinct across columns; |B| puts the even
    columns below ``CG_TOL |B|`` after ``cg_xr`` and the odd ones above."""
    st = np.zeros((len(CG_ROWS), k))
    st[C_RHO], st[C_RHO0] = scalars(k, 11, signed=False), scalars(k, 12, signed=False)
    st[C_ALPHA], st[C_BETA] = scalars(k, 13), scalars(k, 14)
    st[C_PQ], st[C_RR] = scalars(k, 15, signed=False), scalars(k, 16, signed=False)
    st[C_NRMB] = np.where(np.arange(k) % 2 == 0, 1e3, 1e-3) * math.sqrt(m) * (1 + 0.01 * np.arange(k))
    if k >= 3:
        st[C_RHO, 1] = 0.0
        st[C_PQ, 2] = 0.0
    return st


def cg_vectors(m, k, seed):
    """Four m x k operands; the first has a zero column 0 when k >= 3."""
    V = [data(m, k, seed + i) for i in range(4)]
    if k >= 3:
        V[0][:, 0] = 0.0
    return V


def generic_lsqr_state(k):
    """18 x k mid-solve LSQR state that raises no flag with ``CRAFT_TOL`` /
    ``CRAFT_EPS``; rows distinct across columns, the stagnation count
    non-zero (a correct step resets it)."""
    f = 1 + 0.5 * np.arange(k) / k
    st = np.zeros((len(LSQR_ROWS), k))
    st[S_ALPHA], st[S_BETA], st[S_RHOBAR], st[S_PHIBAR] = 1.3 * f, 0.9 / f, -1.1 * f, 0.7 * f
    st[S_NRMA], st[S_SQD], st[S_NRMX], st[S_SQX] = 2.0 * f, 0.5 * f, 1.5 * f, 2.0 / f
    st[S_CS2], st[S_SN2], st[S_ZZ], st[S_NRMAR0] = -0.8 / f, 0.6 * f, 0.4 * f, 1.0 * f
    st[S_STAG] = 1 + np.arange(k) % 2
    for r in (S_CNDA, S_RHO, S_PHI, S_THETA, S_NRMAR):
        st[r] = 99.0 + r + np.arange(k)
    return st


def lsqr_vectors(m, k):
    return data(m, k, 300 * k + m % 89), data(m, k, 300 * k + m % 89 + 1), data(m, k, 300 * k + m % 89 + 2)


def cg_seed(m, k):
    return 100 * k + m % 97
