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

from . import _lib, _tri

vp, i32, i64 = C_.c_void_p, C_.c_int, C_.c_int64
_lib.register("sl_trtri_tri", [vp, i32, i32, i64, i64, vp])


def _why_not(A) -> str | None:
    return _tri.why_not_square_f64(A) or (None if A.is_cuda else "A must be a CUDA tensor")


def takes(A) -> bool:
    """Whether the kernel inverts this operand (shape, dtype, layout,
    alignment, device): the one definition ``base.TriangularInverse`` routes by."""
    return _why_not(A) is None


def ok(A) -> bool:
    """Whether :func:`trtri_tri` takes ``A`` and the native library is there."""
    return takes(A) and _lib.available()


def block() -> tuple[int, int]:
    """``(nb, T)``: the diagonal block width and the edge of an update tile."""
    return _tri.block("sl_trtri_tri_block", 2)


def launches(n: int, nb: int = 64) -> int:
    """Kernel launches of one call at size n."""
    k = -(-n // nb)
    return 0 if n == 0 else max(1, 3 * k - 2)


def trtri_tri(uplo, diag, A: torch.Tensor) -> torch.Tensor:
    """Overwrite the ``uplo`` triangle of ``A`` with that of ``A^-1``; returns
    ``A``.  Diag U: the diagonal is taken as ones and neither read nor written."""
    u, d = _tri.flag(uplo, "uplo", "LU", "trtri_tri"), _tri.flag(diag, "diag", "NU", "trtri_tri")
    why = _why_not(A)
    if why is not None:
        raise ValueError(f"trtri_tri: {why}")
    n = A.shape[0]
    if n == 0:
        return A
    An, u = _tri.row_major(A, (u, "LU"))      # (A^T)^-1 = (A^-1)^T
    _lib.call("sl_trtri_tri", _lib.ptr(An), ord(u), ord(d), n, _tri.layout(An)[2], vp(_lib.stream_of(A)))
    return A
