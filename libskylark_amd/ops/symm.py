"""Hand-written triangle-reading symmetric product (``symm_tri.hip``):
``Y <- alpha S X + beta Y`` for a symmetric ``S`` of which only the ``uplo``
triangle is stored (f32 or f64) and a short block ``X`` (1..8 columns).

Reference: ``El::Symm`` behind ``base/Symm.hpp`` ("only the uplo triangle is
referenced") and the ``K x`` product of the CG iteration of
``ml/krr.hpp:452-541``.  Every stored element is read once and used for two
output rows, so a product streams half the bytes of a full GEMV; the other
triangle and the pitch padding may hold anything, NaN included.  Sums are
f32 inside a 256 x 256 tile (chains of at most 39 terms), f64 across tiles;
no atomics, bit-identical from run to run for a fixed ``workgroups``.
"""
from __future__ import annotations

import ctypes as C_

import torch

from . import _lib

vp, i32, i64, f64 = C_.c_void_p, C_.c_int, C_.c_int64, C_.c_double
_lib.register("sl_symm_tri_workspace", [i64, i64, i32, i32], C_.c_int64)
_lib.register("sl_symm_tri", [vp, i32, i32, i64, i64, i64, i64, vp, i32, vp, i64, i32, vp, i64, f64, f64, vp])

MAX_K = 8
_WS: dict = {}


def _why_not(A: torch.Tensor, X: torch.Tensor | None = None) -> str | None:
    # the device is checked last, so every other reason can be had (and tested) without a GPU
    if not isinstance(A, torch.Tensor) or A.dim() != 2 or A.layout != torch.strided:
        return "A must be a dense 2-D tensor"
    if A.dtype not in (torch.float32, torch.float64):
        return f"A must be f32 or f64 (got {A.dtype})"
    if A.shape[0] == 0 or A.shape[1] == 0:
        return "A is empty"
    if A.shape[0] > A.shape[1]:
        return "A must be square or a row block of a square matrix"
    if A.stride(1) != 1:
        return "A must be row-major (unit column stride)"
    if A.shape[0] > 1 and A.stride(0) < A.shape[1]:
        return "A's rows overlap"
    es = A.element_size()
    if A.data_ptr() % 16 or (A.shape[0] > 1 and (A.stride(0) * es) % 16):
        return "A needs a 16-B aligned base and row pitch"
    if X is not None:
        if not isinstance(X, torch.Tensor) or X.dim() != 2 or X.layout != torch.strided:
            return "X must be a dense 2-D tensor"
        if X.dtype != A.dtype:
            return f"X must have A's dtype {A.dtype} (got {X.dtype})"
        if X.device != A.device:
            return "A and X live on different devices"
        if X.shape[0] != A.shape[1]:
            return f"X has {X.shape[0]} rows, A {A.shape[1]} columns"
        if not 1 <= X.shape[1] <= MAX_K:
            return f"X must have 1..{MAX_K} columns (got {X.shape[1]})"
    if not A.is_cuda:
        return "A must be a CUDA tensor"
    return None


def takes(A: torch.Tensor, X: torch.Tensor | None = None) -> bool:
    """Whether these operands are ones the kernel computes on (dtype, device,
    layout, alignment, width of X): the one definition ``base.Symm`` and
    ``SymTriOp`` route by."""
    return _why_not(A, X) is None


def ok(A: torch.Tensor, X: torch.Tensor | None = None) -> bool:
    """Whether :func:`symm_tri` takes these operands and the native library is there."""
    return takes(A, X) and _lib.available()


def workspace_bytes(n: int, m: int, k: int, dtype: torch.dtype) -> int:
    """Bytes of partial-sum workspace of one call: ``ceil(n / 256) + ceil(m / 256)``
    slots of ``n k`` elements."""
    nb = int(_lib.require().sl_symm_tri_workspace(int(n), int(m), int(k), _lib.dtype_code(dtype)))
    if nb < 0:
        raise ValueError(f"symm_tri: no workspace for n={n}, m={m}, k={k}, {dtype}")
    return nb


def _ws(A: torch.Tensor, nb: int) -> torch.Tensor:
    """Workspace per (device, stream): launches on different streams never
    share scratch.  Its contents never matter: every slot a call reads, that
    call has written."""
    key = (str(A.device), torch.cuda.current_stream(A.device).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nb:
        ws = _WS[key] = torch.empty(nb, dtype=torch.uint8, device=A.device)
    return ws


def symm_tri(A: torch.Tensor, X: torch.Tensor, *, uplo: str = "L", r0: int = 0, n: int | None = None,
             alpha: float = 1.0, beta: float = 0.0, out: torch.Tensor | None = None,
             workgroups: int | None = None) -> torch.Tensor:
    """``out <- alpha * (contribution of A to S X) + beta * out`` (n x k).

    ``A`` holds rows ``[r0, r0 + m)`` of the n x n symmetric ``S`` (``r0=0``
    with square ``A``: all of it); only elements of its ``uplo`` triangle are
    used.  Each stored ``a_ij`` with ``i != j`` adds ``a_ij x_j`` to row i and
    ``a_ij x_i`` to row j, diagonal elements count once, so the contributions
    of disjoint row blocks sum to ``S X``.  ``X`` (n x k, ``1 <= k <= 8``, any
    strides) is packed; ``beta == 0`` does not read ``out``; ``out=None``
    allocates.  ``workgroups`` (default one per CU) is a test knob; results
    are bit-identical from run to run for a fixed value."""
    up = str(uplo).upper()
    if up not in ("L", "U"):
        raise ValueError(f"symm_tri: uplo must be L or U (got {uplo})")
    why = _why_not(A, X)
    if why is not None:
        raise ValueError(f"symm_tri: {why}")
    m, nn = A.shape
    if n is not None and int(n) != nn:
        raise ValueError(f"symm_tri: n={n} but A has {nn} columns")
    r0 = int(r0)
    if r0 < 0 or r0 + m > nn:
        raise ValueError(f"symm_tri: rows [{r0}, {r0 + m}) are not inside a matrix of order {nn}")
    G = 0 if workgroups is None else int(workgroups)
    if workgroups is not None and not 1 <= G <= 4096:
        raise ValueError(f"symm_tri: workgroups must be in 1..4096 (got {workgroups})")
    k = X.shape[1]
    Xt = X.t().contiguous()
    if out is None:
        out = torch.empty(nn, k, dtype=A.dtype, device=A.device)
        beta = 0.0
    elif (not isinstance(out, torch.Tensor) or tuple(out.shape) != (nn, k) or out.dtype != A.dtype
          or out.device != A.device or out.stride(1) != 1 or (nn > 1 and out.stride(0) < k)):
        raise ValueError(f"symm_tri: out must be a row-major {nn} x {k} {A.dtype} tensor on {A.device}")
    per = 16 // A.element_size()
    lda = A.stride(0) if m > 1 else -(-nn // per) * per     # one row: its pitch is never used
    nb = workspace_bytes(nn, m, k, A.dtype)
    ws = _ws(A, nb)
    _lib.call("sl_symm_tri", _lib.ptr(A), _lib.dtype_code(A.dtype), ord(up), nn, r0, m, lda,
              _lib.ptr(Xt), k, _lib.ptr(ws), ws.numel(), G, _lib.ptr(out), out.stride(0) if nn > 1 else k,
              float(alpha), float(beta), vp(_lib.stream_of(A)))
    return out
