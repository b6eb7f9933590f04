"""Hand-written one-triangle f64 triangular-triangular product
(``trtrmm_tri.hip``): the ``uplo`` triangle of a square ``A`` holds a
triangular factor and is overwritten by the same triangle of ``L^T L`` (L) or
``U U^T`` (U), in place.

Reference: Elemental's ``Trtrmm(uplo, A)`` (LAPACK's LAUUM), the last stage of
``El::HPDInverse`` / ``El::Inverse(*Cache[j])`` (``ml/BlockADMM.hpp:437``).  Only
the ``uplo`` triangle is read or written; the other triangle and the pitch
padding may hold NaN.  Row slabs of 128 from the top, every 128 x 128 tile
above a slab adds its rank-128 contribution on the f64 matrix cores:
``n^3 / 3`` flops, no workspace, no allocation, no atomics (bit-identical from
run to run) and no host synchronisation, ``2 ceil(n / 128) - 1`` launches.  A
column-major A is passed as the transposed row-major operand with ``uplo``
flipped, never copied.
"""
from __future__ import annotations

import ctypes as C_

import torch

from . import _lib, _tri

vp, i32, i64 = C_.c_void_p, C_.c_int, C_.c_int64
MAX_PITCH = 1 << 22      # the kernel's offsets inside a 128 x 128 block are 32-bit byte offsets
_lib.register("sl_trtrmm_tri", [vp, i32, i64, i64, vp])


def _why_not(A) -> str | None:
    why = _tri.why_not_square_f64(A)
    if why is None and _tri.layout(A)[2] > MAX_PITCH:
        why = f"A's pitch exceeds {MAX_PITCH} elements"
    return why or (None if A.is_cuda else "A must be a CUDA tensor")


def takes(A) -> bool:
    """Whether the kernel multiplies this operand (shape, dtype, layout,
    alignment, device): the one definition ``base.Trtrmm`` routes by."""
    return _why_not(A) is None


def ok(A) -> bool:
    """Whether :func:`trtrmm_tri` takes ``A`` and the native library is there."""
    return takes(A) and _lib.available()


def block() -> tuple[int, int]:
    """``(nb, T)``: the height of a row slab and the edge of a tile."""
    return _tri.block("sl_trtrmm_tri_block", 2)


def launches(n: int, nb: int = 128) -> int:
    """Kernel launches of one call at size n: two per row slab below the
    first, and the closing one."""
    return 0 if n == 0 else 2 * -(-n // nb) - 1


def trtrmm_tri(uplo, A: torch.Tensor) -> torch.Tensor:
    """Overwrite the ``uplo`` triangle of ``A`` with that of ``L^T L`` (L) or
    ``U U^T`` (U); returns ``A``."""
    u = _tri.flag(uplo, "uplo", "LU", "trtrmm_tri")
    why = _why_not(A)
    if why is not None:
        raise ValueError(f"trtrmm_tri: {why}")
    n = A.shape[0]
    if n == 0:
        return A
    An, u = _tri.row_major(A, (u, "LU"))      # (L^T L)^T = U U^T with U = L^T
    _lib.call("sl_trtrmm_tri", _lib.ptr(An), ord(u), n, _tri.layout(An)[2], vp(_lib.stream_of(A)))
    return A
