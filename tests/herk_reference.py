"""Long-double reference and rounding bound for the one-triangle rank-k update
``C <- alpha op(A) op(A)^T + beta C`` (``herk_tri.hip``, ``base.Herk``).

``reference`` forms, in numpy ``longdouble`` on the CPU,

    ref = alpha op(A) op(A)^T + beta C0
    den = |alpha| |op(A)| |op(A)|^T + |beta| |C0|

and ``measure`` gives ``e = max |C - ref| / den`` over the stored triangle.
Where ``den == 0`` the result must equal ``ref`` exactly.  With ``beta == 0`` C0
is not looked at (it may hold NaN), with ``alpha == 0`` A is not.

Bound: ``e <= (K + 4) u``, ``u = 2^-53``.  ``K u`` covers a dot product of length K
summed in any order (the kernel's slices, its splits and the order inside an
MFMA); one u each covers the product by alpha, the product by beta and the
final add; one u absorbs the second-order terms for K <= 2^20.  The native
library is not imported here: the module also serves the CPU-only tests.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "herk_reference needs the 64-bit-mantissa long double"

U = 2.0 ** -53


def bound(K: int) -> float:
    return (K + 4) * U


def tri_mask(s: int, uplo: str) -> np.ndarray:
    ones = np.ones((s, s), dtype=bool)
    return np.tril(ones) if uplo.upper() == "L" else np.triu(ones)


def reference(orient: str, alpha, A, beta=0.0, C0=None):
    """``(ref, den)`` in long double.  A, C0: anything ``np.asarray`` takes
    (f64); orient N: op(A) = A, T / C: op(A) = A^T."""
    s, K = (A.shape[1], A.shape[0]) if orient.upper() != "N" else A.shape
    ref, den = np.zeros((s, s), dtype=LD), np.zeros((s, s), dtype=LD)
    if alpha != 0 and K > 0:
        P = np.asarray(A, dtype=np.float64).astype(LD)
        P = P.T if orient.upper() != "N" else P
        ref += LD(alpha) * (P @ P.T)
        den += abs(LD(alpha)) * (np.abs(P) @ np.abs(P).T)
    if beta != 0:
        Cl = np.asarray(C0, dtype=np.float64).astype(LD)
        ref += LD(beta) * Cl
        den += abs(LD(beta)) * np.abs(Cl)
    return ref, den


def measure(C, ref, den, uplo: str) -> float:
    """``max |C - ref| / den`` over the ``uplo`` triangle; asserts exact
    equality where ``den == 0``.  Non-finite entries of C there give ``inf``."""
    m = tri_mask(ref.shape[0], uplo)
    Cl = np.asarray(C, dtype=np.float64).astype(LD)
    if not m.any():
        return 0.0
    if not np.isfinite(Cl[m]).all():
        return float("inf")
    zero = m & (den == 0)
    assert (Cl[zero] == ref[zero]).all(), "den == 0 and the result is not the reference exactly"
    pos = m & (den > 0)
    if not pos.any():
        return 0.0
    return float((np.abs(Cl - ref)[pos] / den[pos]).max())
