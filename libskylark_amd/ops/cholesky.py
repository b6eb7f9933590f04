"""Hand-written one-triangle f64 Cholesky (``chol_tri.hip``): the ``uplo``
triangle of a row-major square ``A`` is overwritten by its factor, ``A = L
L^T`` (``'L'``) or ``A = U^T U`` (``'U'``).

Reference: ``El::Cholesky(El::LOWER, C)`` between the Herk and the SolveAfter
of ``ml/krr.hpp:371-398`` and ``:639-650``.  The strict other triangle and the
pitch padding are never read and never written; they may hold NaN.  A call is
``3 ceil(n / 64) - 2`` ordinary launches on the current stream (diagonal
block, panel solve by substitution, trailing update on the f64 matrix cores),
with no atomics: results are bit-identical from run to run.  A pivot that is
not positive and finite ends up, as its 1-based index, in an int32 status
word on the device; nothing waits on it.
"""
from __future__ import annotations

import ctypes as C_

import torch

from . import _lib, _tri
from ..base.exceptions import NLAError

vp, i32, i64 = C_.c_void_p, C_.c_int, C_.c_int64
_lib.register("sl_chol_tri", [vp, i32, i64, i64, vp, vp])

_WS: dict = {}


def _why_not(A: torch.Tensor) -> str | None:
    # the device is checked last, so every other reason can be had (and tested) without a GPU
    return (_tri.why_not_square_f64(A, shape_first=True, row_major_only=True)
            or (None if A.is_cuda else "A must be a CUDA tensor"))


def takes(A: torch.Tensor) -> bool:
    """Whether ``A`` is an operand the kernel factors (shape, dtype, layout,
    alignment, device): the one definition ``base.Cholesky`` routes by."""
    return _why_not(A) is None


def ok(A: torch.Tensor) -> bool:
    """Whether :func:`chol_tri` takes ``A`` and the native library is there."""
    return takes(A) and _lib.available()


def block() -> tuple[int, int]:
    """``(nb, T)``: the panel width and the edge of a trailing-update tile."""
    return _tri.block("sl_chol_tri_block", 2)


def _status(A: torch.Tensor) -> torch.Tensor:
    """The call's own status word, per (device, stream): calls on different
    streams never share it, and every call zeroes it before its first launch."""
    key = (str(A.device), torch.cuda.current_stream(A.device).cuda_stream)
    ws = _WS.get(key)
    if ws is None:
        ws = _WS[key] = torch.zeros(1, dtype=torch.int32, device=A.device)
    return ws


def chol_tri(A: torch.Tensor, uplo: str = "L", info: torch.Tensor | None = None) -> torch.Tensor:
    """Factor the ``uplo`` triangle of ``A`` in place; returns ``A``.

    ``info``: an int32 one-element tensor on A's device.  The call zeroes it
    and the kernel leaves the 1-based index of the first failed pivot there (0:
    none), with no host synchronisation; the factor then holds NaN from that
    pivot on.  Without ``info`` the call reads its own status word (one
    synchronisation) and raises :class:`NLAError` naming the pivot."""
    up = _tri.flag(uplo, "uplo", "LU", "chol_tri")
    why = _why_not(A)
    if why is not None:
        raise ValueError(f"chol_tri: {why}")
    if info is not None and not (isinstance(info, torch.Tensor) and info.dtype == torch.int32 and info.numel() == 1
                                 and info.device == A.device):
        raise ValueError(f"chol_tri: info must be an int32 one-element tensor on {A.device}")
    n = A.shape[0]
    st = _status(A) if info is None else info
    _lib.call("sl_chol_tri", _lib.ptr(A), ord(up), n, A.stride(0) if n > 1 else max(n, 1), _lib.ptr(st),
              vp(_lib.stream_of(A)))
    if info is None:
        p = int(st.item())
        if p != 0:
            raise NLAError(f"Cholesky: the matrix is not positive definite: pivot {p} (1-based) "
                           f"is not positive and finite")
    return A
