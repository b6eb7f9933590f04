"""What the bindings of the one-triangle f64 kernel family (``cholesky``,
``trsm``, ``trtri``, ``trtrmm``) share: the operand checks behind their
``_why_not``, flag parsing, the ``sl_*_block`` reader and the column-major
step.  Every check returns ``None`` or the reason as the caller words it; the
device is never looked at here, so every reason can be had without a GPU.
"""
from __future__ import annotations

import ctypes as C_

import torch

from . import _lib


def flag(value, name: str, allowed: str, op: str | None = None) -> str:
    """``value`` in upper case if it is one of the letters of ``allowed``,
    else a ``ValueError`` naming the flag (and the entry point ``op``)."""
    v = str(value).upper()
    if v not in tuple(allowed):
        choice = f"{', '.join(allowed[:-1])} or {allowed[-1]}"
        raise ValueError(f"{op + ': ' if op else ''}{name} must be {choice} (got {value})")
    return v


def layout(X: torch.Tensor):
    """``("R" | "C", run, pitch)``: the unit-stride direction, the length of a
    contiguous run and the distance between runs; a string when X has neither."""
    r, c = X.shape
    if c <= 1 or X.stride(1) == 1:
        if r > 1 and X.stride(0) < c:
            return "rows overlap"
        return "R", c, (X.stride(0) if r > 1 else max(c, 1))
    if r <= 1 or X.stride(0) == 1:
        if c > 1 and X.stride(1) < r:
            return "rows overlap"
        return "C", r, (X.stride(1) if c > 1 else max(r, 1))
    return "needs unit stride along rows or columns"


def not_dense(nm: str, X) -> str | None:
    if not isinstance(X, torch.Tensor) or X.dim() != 2 or X.layout != torch.strided:
        return f"{nm} must be a dense 2-D tensor"
    return None


def not_f64(nm: str, X: torch.Tensor) -> str | None:
    return None if X.dtype == torch.float64 else f"{nm} must be f64 (got {X.dtype})"


def not_square(A: torch.Tensor) -> str | None:
    return None if A.shape[0] == A.shape[1] else f"A must be square (got {tuple(A.shape)})"


def bad_strides(nm: str, X: torch.Tensor) -> str | None:
    lay = layout(X)
    if isinstance(lay, str):
        return f"{nm}: {lay}" if lay.startswith("needs") else f"{nm}'s {lay}"
    return None


def misaligned(nm: str, X: torch.Tensor) -> str | None:
    return f"{nm} needs an 8-B aligned base" if X.data_ptr() % 8 else None


def why_not_square_f64(A, shape_first: bool = False, row_major_only: bool = False) -> str | None:
    """Why A is not a dense square f64 operand with unit stride along rows or
    columns and an 8-B aligned base.  ``shape_first``: the shape is looked at
    before the dtype.  ``row_major_only``: a column-major A is refused too."""
    why = not_dense("A", A)
    if why:
        return why
    shape, dtype = not_square(A), not_f64("A", A)
    if shape or dtype:
        return (shape or dtype) if shape_first else (dtype or shape)
    if row_major_only and A.shape[1] > 1 and A.stride(1) != 1:
        return "A must be row-major (unit column stride)"
    return bad_strides("A", A) or misaligned("A", A)


def block(symbol: str, count: int) -> tuple[int, ...]:
    """The ``count`` ints of ``sl_*_block``: the sizes at which a kernel's code changes path."""
    _lib.register(symbol, [C_.POINTER(C_.c_int)] * count)
    vals = [C_.c_int(0) for _ in range(count)]
    _lib.call(symbol, *(C_.byref(v) for v in vals))
    return tuple(v.value for v in vals)


def row_major(X: torch.Tensor, *flags):
    """``(Xn, *values)``: X as the kernels take it.  A column-major X is its
    row-major transpose, never a copy, and each flag, given as ``(value, pair)``
    with the pair one of ``"LU"`` (uplo), ``"NT"`` (orient), ``"LR"`` (side),
    turns into the other letter of its pair."""
    lay = layout(X)
    if isinstance(lay, str) or lay[0] != "C":
        return (X, *(f for f, _ in flags))
    return (X.t(), *(pair[1 - pair.index(f)] for f, pair in flags))
