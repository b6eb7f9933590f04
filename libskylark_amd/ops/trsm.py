"""Hand-written one-triangle f64 triangular solve (``trsm_tri.hip``): ``op(A)
X = alpha B`` (side L, B n x t) or ``X op(A) = alpha B`` (side R, B t x n),
in place on B.

Reference: ``El::Trsm`` and the two solves of ``El::cholesky::SolveAfter``
(``ml/krr.hpp:398``, ``:650``).  Only the ``uplo`` triangle of A is read, and
with diag U not its diagonal; the other triangle and the pitch padding of A
and B may hold NaN, A is never written.  A right-looking sweep over 64-wide
diagonal blocks, substitution with true divisions in the block, no inverse,
no workspace, no allocation, no atomics (bit-identical from run to run) and no
host synchronisation.  ``t <= 8`` right-hand sides take the thin regime,
``ceil(n / 64)`` launches; more take the wide one, ``2 ceil(n / 64) - 1``
launches with the update on the f64 matrix cores.  A column-major A or B is
passed as the transposed row-major operand with the flags flipped, never
copied.
"""
from __future__ import annotations

import ctypes as C_

import torch

from . import _lib, _tri
from ._tri import layout as _layout

vp, i32, i64 = C_.c_void_p, C_.c_int, C_.c_int64
_lib.register("sl_trsm_tri", [vp, i32, i32, i32, i32, i64, i64, i64, vp, i64, vp])

# Regimes that base.Trsm hands to the kernel ("thin": t <= block()[2], "wide":
# the rest).  A regime leaves this set only if it is slower than
# torch.linalg.solve_triangular at both sizes of profiles/r7/trsm_tri_ab.jsonl
# (benchmarks/bench_trsm.py); the kernel stays reachable through trsm_tri.
# Measured there: both regimes are slower at n = 4096 (1.1 x to 2.9 x) and
# faster at n = 16384 for t = 1, t = 4096 and t = 256 orient T (0.18 x to
# 0.71 x), slower for t = 8 and t = 256 orient N: neither is slower at both
# sizes, both stay native.
BASE_NATIVE_REGIMES = frozenset({"thin", "wide"})
_THIN = 8           # sl_trsm_tri_block's third value (asserted in tests/test_gpu_trsm.py)


def _span(X: torch.Tensor) -> int:
    """Bytes from the first to one past the last element."""
    return 8 * ((X.shape[0] - 1) * X.stride(0) + (X.shape[1] - 1) * X.stride(1) + 1)


def _overlap(A: torch.Tensor, B: torch.Tensor) -> bool:
    """Whether an element of A may share memory with one of B.  Disjoint byte
    ranges do not; neither do two views of one pitched buffer whose runs take
    different columns of it (``G[:, :s]`` and ``G[:, s:]``)."""
    a, b = A.data_ptr(), B.data_ptr()
    if a + _span(A) <= b or b + _span(B) <= a:
        return False
    (_, ra, pa), (_, rb, pb) = _layout(A), _layout(B)
    if pa != pb or (b - a) % 8:
        return True
    d = ((b - a) // 8) % pa
    return not (d >= ra and d + rb <= pa)


def _why_not(side, A, B) -> str | None:
    # the device is checked last, so every other reason can be had (and tested) without a GPU
    why = (_tri.not_dense("A", A) or _tri.not_dense("B", B) or _tri.not_f64("A", A) or _tri.not_f64("B", B)
           or _tri.not_square(A))
    if why:
        return why
    n = A.shape[0]
    if B.shape[0 if str(side).upper() == "L" else 1] != n:
        return f"B is {tuple(B.shape)}, side {side} needs {n} {'rows' if str(side).upper() == 'L' else 'columns'}"
    why = (_tri.bad_strides("A", A) or _tri.bad_strides("B", B) or _tri.misaligned("A", A)
           or _tri.misaligned("B", B))
    if why:
        return why
    if A.device != B.device:
        return f"A is on {A.device}, B on {B.device}"
    if A.numel() and B.numel() and _overlap(A, B):
        return "A and B overlap in memory"
    if not A.is_cuda:
        return "A and B must be CUDA tensors"
    return None


def takes(side, A, B) -> bool:
    """Whether the kernel solves with these operands (shape, dtype, layout,
    alignment, overlap, device): the one definition ``base.Trsm`` routes by."""
    return _why_not(side, A, B) is None


def ok(side, A, B) -> bool:
    """Whether :func:`trsm_tri` takes the operands and the native library is there."""
    return takes(side, A, B) and _lib.available()


def block() -> tuple[int, int, int]:
    """``(nb, T, thin)``: the diagonal block width, the edge of a wide-update
    tile and the largest number of right-hand sides of the thin regime."""
    return _tri.block("sl_trsm_tri_block", 3)


def regime(side, B: torch.Tensor) -> str:
    """``"thin"`` or ``"wide"``: the regime a solve with this B takes."""
    return "thin" if B.shape[1 if str(side).upper() == "L" else 0] <= _THIN else "wide"


def _flags(side, uplo, orient, diag):
    s, u = _tri.flag(side, "side", "LR", "trsm_tri"), _tri.flag(uplo, "uplo", "LU", "trsm_tri")
    o, d = _tri.flag(orient, "orient", "NTC", "trsm_tri"), _tri.flag(diag, "diag", "NU", "trsm_tri")
    return s, u, ("N" if o == "N" else "T"), d      # C is T for real data


def trsm_tri(side, uplo, orient, diag, alpha, A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """Solve ``op(A) X = alpha B`` (side L) or ``X op(A) = alpha B`` (side R)
    in place on B; returns B.  ``alpha != 1`` is one in-place scaling of B
    before the solve; ``alpha == 0`` zeroes B and launches nothing else."""
    s, u, o, d = _flags(side, uplo, orient, diag)
    why = _why_not(s, A, B)
    if why is not None:
        raise ValueError(f"trsm_tri: {why}")
    n = A.shape[0]
    t = B.shape[1] if s == "L" else B.shape[0]
    if n == 0 or t == 0:
        return B
    if alpha == 0:
        B.zero_()
        return B
    if alpha != 1:
        B.mul_(alpha)
    An, u, o = _tri.row_major(A, (u, "LU"), (o, "NT"))
    Bn, s, o = _tri.row_major(B, (s, "LR"), (o, "NT"))      # op(A) X = B is X^T op(A)^T = B^T
    _lib.call("sl_trsm_tri", _lib.ptr(An), ord(s), ord(u), ord(o), ord(d), n, t, _layout(An)[2], _lib.ptr(Bn),
              _layout(Bn)[2], vp(_lib.stream_of(B)))
    return B
