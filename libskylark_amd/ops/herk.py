"""Hand-written one-triangle f64 rank-k update (``herk_tri.hip``): the ``uplo``
triangle of ``C <- alpha op(A) op(A)^T + beta C`` for f64 A and C on the GPU,
``op(A)`` of order s x K (orient N: ``A A^T``; orient T / C: ``A^T A``).

Reference: Elemental's ``Herk(uplo, orient, alpha, A, beta, C)``, the Gram of
``ml/krr.hpp:371`` / ``:639``, ``ml/kernels.hpp:241`` and ``base/distance.hpp:92``
that ``El::Cholesky`` takes next.  Only the ``uplo`` triangle of C is read or
written; the other triangle and the pitch padding may hold NaN, ``beta == 0``
reads nothing of C, and ``alpha == 0`` or ``K == 0`` reads nothing of A.  128 x 128
tiles of the triangle on the f64 matrix cores, half the flops of the full
product and no s x s temporary.  A tall ``A^T A`` whose tiles do not fill the
chip is split along K into ``S`` ranges: a first launch writes the raw partial
tiles to a workspace (``S x tiles x 128 KB``, allocated here), a second adds them
in split order.  No atomics, no workgroup waits on another: bit-identical from
run to run for a fixed ``(s, K, S)``.  Row- and column-major A and C are taken
as they are, never copied.
"""
from __future__ import annotations

import ctypes as C_

import torch

from . import _lib, _tri

vp, i32, i64, f64 = C_.c_void_p, C_.c_int, C_.c_int64, C_.c_double
MAX_S = 1 << 22          # the kernel's tile count is a grid dimension
MAX_SPLITS = 65535       # and so are the K ranges
_lib.register("sl_herk_tri", [vp, i64, i64, i64, i64, vp, i64, i32, f64, f64, i64, vp, i64, vp])
_lib.register("sl_herk_tri_plan", [i64, i64, i64, C_.POINTER(i64)])

# Orientations that base.Herk hands to the kernel.  One leaves this set only if
# it is slower than the parent's base.Herk path (the full torch product written
# through a triangle mask) at every size of profiles/r8/herk_f64_ab.jsonl
# (benchmarks/bench_herk64.py); the kernel stays reachable through herk_tri.
# Measured there (time over the old path's): orient T 0.48 x at K = 200000,
# s = 1024 and 1.15 x at K = 65536, s = 4096; orient N 1.04 x at K = s = 4096
# and 0.53 x at K = 512, s = 8192: neither is slower at every size, both stay
# native.
BASE_NATIVE_REGIMES = frozenset({"N", "T"})


def _why_not_operand(nm: str, X) -> str | None:
    return (_tri.not_dense(nm, X) or _tri.not_f64(nm, X) or _tri.bad_strides(nm, X)
            or _tri.misaligned(nm, X))


def _why_not(A, C=None, trans: bool = False) -> str | None:
    why = _why_not_operand("A", A)
    if why:
        return why
    s = A.shape[1] if trans else A.shape[0]
    if s > MAX_S:
        return f"op(A) has more than {MAX_S} rows"
    if C is not None:
        why = _tri.not_dense("C", C) or _tri.not_f64("C", C)
        if why:
            return why
        if tuple(C.shape) != (s, s):
            return f"C must be square of order {s} (got {tuple(C.shape)})"
        why = _tri.bad_strides("C", C) or _tri.misaligned("C", C)
        if why:
            return why
        if C.device != A.device:
            return f"C is on {C.device}, A on {A.device}"
    return None if A.is_cuda else "A must be a CUDA tensor"


def takes(A, C=None, *, trans: bool) -> bool:
    """Whether the kernel takes these operands (shape, dtype, layout,
    alignment, device): the one definition ``base.Herk`` routes by."""
    return _why_not(A, C, trans) is None


def ok(A, C=None, *, trans: bool) -> bool:
    """Whether :func:`herk_tri` takes the operands and the native library is there."""
    return takes(A, C, trans=trans) and _lib.available()


def block() -> tuple[int, int]:
    """``(T, KH)``: the edge of a tile and the K slice."""
    return _tri.block("sl_herk_tri_block", 2)


def plan(s: int, K: int, cus: int | None = None) -> tuple[int, int]:
    """``(tiles, S)`` of the static partition: the 128 x 128 tiles of the
    triangle and the number of K ranges, a pure function of (s, K, compute
    units); ``cus=None`` asks the current device."""
    out = (i64 * 2)()
    _lib.call("sl_herk_tri_plan", s, K, 0 if cus is None else cus, out)
    return int(out[0]), int(out[1])


def _splits(s: int, K: int, splits: int | None) -> tuple[int, int]:
    if splits is None:
        return plan(s, K)
    if splits < 1:
        raise ValueError(f"herk_tri: splits must be positive (got {splits})")
    t, kh = block()
    nt = -(-s // t)
    return nt * (nt + 1) // 2, max(1, min(splits, -(-K // kh), MAX_SPLITS))


def launches(s: int, K: int, splits: int | None = None) -> int:
    """Kernel launches of one call with ``alpha != 0``: one, or two when K is
    split; none for s == 0."""
    if s == 0:
        return 0
    return 1 if _splits(s, K, splits)[1] == 1 else 2


def herk_tri(uplo, orient, alpha, A: torch.Tensor, beta=0.0, C: torch.Tensor | None = None, *,
             splits: int | None = None) -> torch.Tensor:
    """The ``uplo`` triangle of ``C <- alpha op(A) op(A)^T + beta C``; returns C.
    ``C=None`` allocates zeros.  ``splits``: ``None`` takes the plan's number of
    K ranges, a positive value forces it (clamped to the number of 32-slices)."""
    u = _tri.flag(uplo, "uplo", "LU", "herk_tri")
    trans = _tri.flag(orient, "orientation", "NTC", "herk_tri") != "N"
    why = _why_not(A, C, trans)
    if why is not None:
        raise ValueError(f"herk_tri: {why}")
    s, K = (A.shape[1], A.shape[0]) if trans else A.shape
    if C is None:
        C, beta = torch.zeros(s, s, dtype=torch.float64, device=A.device), 0.0
    if s == 0:
        return C
    alpha, beta = float(alpha), float(beta)
    xs, ks = (A.stride(1), A.stride(0)) if trans else A.stride()
    Cn, u = _tri.row_major(C, (u, "LU"))          # C is symmetric: its transpose stores the other triangle
    tiles, S = _splits(s, 0 if alpha == 0.0 else K, splits)
    W = torch.empty(S * tiles * 128 * 128, dtype=torch.float64, device=A.device) if S > 1 else None
    _lib.call("sl_herk_tri", _lib.ptr(A), xs, ks, s, K, _lib.ptr(Cn), _tri.layout(Cn)[2], ord(u), alpha, beta, S,
              _lib.ptr(W) if S > 1 else None, W.numel() if S > 1 else 0, vp(_lib.stream_of(A)))
    return C
