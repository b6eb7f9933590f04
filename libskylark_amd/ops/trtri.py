"""Hand-written one-triangle f64 triangular inverse (``trtri_tri.hip``): the
``uplo`` triangle of a square ``A`` is overwritten by the same triangle of
``A^-1``, in place.

Reference: ``El::TriangularInverse(El::UPPER, El::NON_UNIT, invA)``
(``algorithms/regression/accelerated_linearl2_regression_solver_Elemental.hpp:63``),
the explicit ``R^-1`` preconditioner of Blendenpik / LSRN.  Only the ``uplo``
triangle is read or written, and with diag U not its diagonal; the other
triangle and the pitch padding may hold NaN.  Block forward substitution on
``L X = I`` over 64-wide diagonal blocks, true divisions in the block, no
inverse of a block multiplied in, ``n^3 / 3`` flops, no workspace, no
allocation, no atomics (bit-identical from run to run) and no host
synchronisation: ``3 ceil(n / 64) - 2`` launches (one for ``n <= 64``), the
update on the f64 matrix cores.  A column-major A is passed as the transposed
row-major operand with ``uplo`` flipped, never copied.
"""
from __future__ import annotations

import ctypes as C_

import torch

from . import _lib

vp, i32, i64 = C_.c_void_p, C_.c_int, C_.c_int64
_lib.register("sl_trtri_tri_block", [C_.POINTER(C_.c_int), C_.POINTER(C_.c_int)])
_lib.register("sl_trtri_tri", [vp, i32, i32, i64, i64, vp])


def _layout(A: torch.Tensor):
    """``("R" | "C", pitch)``: the unit-stride direction and the distance
    between rows (columns); a string when A has neither or its rows overlap."""
    n = A.shape[0]
    if n <= 1 or A.stride(1) == 1:
        if n > 1 and A.stride(0) < n:
            return "rows overlap"
        return "R", (A.stride(0) if n > 1 else max(n, 1))
    if A.stride(0) == 1:
        if A.stride(1) < n:
            return "rows overlap"
        return "C", A.stride(1)
    return "needs unit stride along rows or columns"


def _why_not(A) -> str | None:
    # the device is checked last, so every other reason can be had (and tested) without a GPU
    if not isinstance(A, torch.Tensor) or A.dim() != 2 or A.layout != torch.strided:
        return "A must be a dense 2-D tensor"
    if A.dtype != torch.float64:
        return f"A must be f64 (got {A.dtype})"
    if A.shape[0] != A.shape[1]:
        return f"A must be square (got {tuple(A.shape)})"
    lay = _layout(A)
    if isinstance(lay, str):
        return f"A: {lay}" if lay.startswith("needs") else f"A's {lay}"
    if A.data_ptr() % 8:
        return "A needs an 8-B aligned base"
    if not A.is_cuda:
        return "A must be a CUDA tensor"
    return None


def takes(A) -> bool:
    """Whether the kernel inverts this operand (shape, dtype, layout,
    alignment, device): the one definition ``base.TriangularInverse`` routes by."""
    return _why_not(A) is None


def ok(A) -> bool:
    """Whether :func:`trtri_tri` takes ``A`` and the native library is there."""
    return takes(A) and _lib.available()


def block() -> tuple[int, int]:
    """``(nb, T)``: the diagonal block width and the edge of an update tile."""
    nb, t = C_.c_int(0), C_.c_int(0)
    _lib.call("sl_trtri_tri_block", C_.byref(nb), C_.byref(t))
    return nb.value, t.value


def launches(n: int, nb: int = 64) -> int:
    """Kernel launches of one call at size n."""
    k = -(-n // nb)
    return 0 if n == 0 else max(1, 3 * k - 2)


def _flags(uplo, diag):
    u, d = str(uplo).upper(), str(diag).upper()
    if u not in ("L", "U"):
        raise ValueError(f"trtri_tri: uplo must be L or U (got {uplo})")
    if d not in ("N", "U"):
        raise ValueError(f"trtri_tri: diag must be N or U (got {diag})")
    return u, d


def trtri_tri(uplo, diag, A: torch.Tensor) -> torch.Tensor:
    """Overwrite the ``uplo`` triangle of ``A`` with that of ``A^-1``; returns
    ``A``.  Diag U: the diagonal is taken as ones and neither read nor written."""
    u, d = _flags(uplo, diag)
    why = _why_not(A)
    if why is not None:
        raise ValueError(f"trtri_tri: {why}")
    n = A.shape[0]
    if n == 0:
        return A
    An = A
    if _layout(A)[0] == "C":
        # a column-major A is the row-major transpose: the other triangle, and (A^T)^-1 = (A^-1)^T
        An, u = A.t(), ("U" if u == "L" else "L")
    _lib.call("sl_trtri_tri", _lib.ptr(An), ord(u), ord(d), n, _layout(An)[1], vp(_lib.stream_of(A)))
    return A
