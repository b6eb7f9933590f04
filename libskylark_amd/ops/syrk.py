"""Hand-written triangular symmetric rank-k update (``syrk_split.hip``): the
``uplo`` triangle of ``C <- alpha op(A) op(A)^T + beta C`` for f32 ``A`` (exact
three-plane bf16 split, six plane products in one f32 accumulator per row
chunk, f64 across chunks) or bf16 ``A`` (one product), ``C`` f32 / f64.

Reference: ``El::Herk(El::LOWER, ...)`` of the KRR normal equations
(``ml/krr.hpp:371``), the linear kernel's symmetric Gram
(``ml/kernels.hpp:241``) and the distance matrices (``base/distance.hpp:92``).
The work (triangle tiles x K slices) is cut evenly over one workgroup per
CU; ``A`` is fed in super-chunks so the split workspace stays <= 1 GiB.
"""
from __future__ import annotations

import ctypes as C_

import torch

from . import _lib

vp, i32, i64, f64 = C_.c_void_p, C_.c_int, C_.c_int64, C_.c_double
_lib.register("sl_syrk_split_plan", [i32, i64, i32, i32, i32, vp])
_lib.register("sl_syrk_split", [vp, i32, i32, i32, i64, i64, i64, vp, i64, vp, i64, i32, i32, i32, vp, i32, i64, i32,
                                f64, f64, vp])

BK = 64
CHUNK_ROWS = 8192            # K rows per f32-accumulated chunk (ml/krr.py SPLIT_GRAM_ROWS)
SPLIT_WS_BYTES = 1 << 30     # bound of the bf16 plane workspace of one super-chunk
TILE = 256 * 256             # f64 elements of one slab tile


def _trans(trans) -> bool:
    if isinstance(trans, str):
        t = trans.upper()
        if t not in ("N", "T", "C"):
            raise ValueError(f"syrk_split: orientation must be N, T or C (got {trans})")
        return t != "N"
    return bool(trans)


def _why_not(A: torch.Tensor, C: torch.Tensor | None, trans: bool) -> str | None:
    if not isinstance(A, torch.Tensor) or A.dim() != 2 or not A.is_cuda or A.layout != torch.strided:
        return "A must be a dense 2-D CUDA tensor"
    if A.dtype not in (torch.float32, torch.bfloat16):
        return f"A must be f32 or bf16 (got {A.dtype})"
    if A.dtype == torch.bfloat16 and trans:
        return "bf16 A is taken for A A^T only (it must be K-contiguous)"
    if A.shape[0] == 0 or A.shape[1] == 0:
        return "A is empty"
    if A.stride(1) != 1:
        return "A must be row-major (unit column stride)"
    if A.dtype == torch.bfloat16 and (A.stride(0) % 8 or A.data_ptr() % 16):
        return "bf16 A needs 16-B aligned rows (row stride % 8 == 0, 16-B aligned base)"
    if A.dtype == torch.float32 and A.data_ptr() % 4:
        return "A is not aligned to its element size"
    if C is not None:
        s = A.shape[1] if trans else A.shape[0]
        if not isinstance(C, torch.Tensor) or C.dim() != 2 or C.shape[0] != C.shape[1] or C.shape[0] != s:
            return f"C must be square of order {s} (got {tuple(C.shape) if hasattr(C, 'shape') else C})"
        if C.dtype not in (torch.float32, torch.float64):
            return f"C must be f32 or f64 (got {C.dtype})"
        if C.device != A.device:
            return "A and C live on different devices"
        if C.stride(1) != 1 or (s > 1 and C.stride(0) < s):
            return "C must be a row-major view with row stride >= its order"
    return None


def takes(A: torch.Tensor, C: torch.Tensor | None = None, *, trans=True) -> bool:
    """Whether these operands are ones the kernel computes on (dtype, device,
    layout, alignment): the one definition ``base.Herk`` routes by."""
    return _why_not(A, C, _trans(trans)) is None


def ok(A: torch.Tensor, C: torch.Tensor | None = None, *, trans=True) -> bool:
    """Whether :func:`syrk_split` takes these operands and the native library is there."""
    return takes(A, C, trans=trans) and _lib.available()


def plan(s: int, k_full: int, chunk_rows: int, workgroups: int, dtype: torch.dtype) -> tuple[int, int]:
    """(slab tiles, workgroups) of the static partition of one call."""
    out = (i64 * 2)()
    _lib.call("sl_syrk_split_plan", int(s), int(k_full), int(chunk_rows), int(workgroups), _lib.dtype_code(dtype),
              C_.cast(out, vp))
    return int(out[0]), int(out[1])


def syrk_split(A: torch.Tensor, C: torch.Tensor | None = None, *, trans, uplo: str = "L", alpha: float = 1.0,
               beta: float = 0.0, chunk_rows: int | None = None, workgroups: int | None = None) -> torch.Tensor:
    """The ``uplo`` triangle of ``C <- alpha A^T A + beta C`` (``trans``) or
    ``alpha A A^T + beta C``; the other triangle of ``C`` is not touched and
    ``beta == 0`` does not read ``C``.  ``C=None`` allocates f32 zeros.

    ``chunk_rows`` (K rows summed in f32 before the f64 carry, default 8192,
    a multiple of 64) and ``workgroups`` (default one per CU) are test knobs;
    the result is bit-identical from run to run for fixed knobs."""
    tr = _trans(trans)
    up = str(uplo).upper()
    if up not in ("L", "U"):
        raise ValueError(f"syrk_split: uplo must be L or U (got {uplo})")
    why = _why_not(A, C, tr)
    if why is not None:
        raise ValueError(f"syrk_split: {why}")
    R = CHUNK_ROWS if chunk_rows is None else int(chunk_rows)
    if R <= 0 or R % BK:
        raise ValueError(f"syrk_split: chunk_rows must be a positive multiple of {BK} (got {chunk_rows})")
    G = 0 if workgroups is None else int(workgroups)
    if workgroups is not None and not 1 <= G <= 4096:
        raise ValueError(f"syrk_split: workgroups must be in 1..4096 (got {workgroups})")
    s, n = (A.shape[1], A.shape[0]) if tr else A.shape
    if C is None:
        C = torch.zeros(s, s, dtype=torch.float32, device=A.device)
    st = vp(_lib.stream_of(A))
    S, seg = None, 0
    if A.dtype == torch.bfloat16:
        if n % BK:
            A = torch.nn.functional.pad(A, (0, BK - n % BK))   # zero K columns: the DMA reads whole slices
            n = A.shape[1]
        k_full = n
    else:
        # super-chunks of whole row chunks, as even as the chunk size allows
        cap = max(R, SPLIT_WS_BYTES // (6 * s) // R * R)
        nl = -(-n // cap)
        k_full = n if nl == 1 else -(-n // (nl * R)) * R
        seg = -(-k_full // BK) * BK
        S = torch.empty(s, 3 * seg, dtype=torch.bfloat16, device=A.device)
    n_slabs, _ = plan(s, k_full, R, G, A.dtype)
    slabs = torch.zeros(n_slabs, TILE, dtype=torch.float64, device=A.device)
    for k0 in range(0, n, k_full):
        w = min(k_full, n - k0)
        Ab = A[k0:k0 + w] if tr else A[:, k0:k0 + w]
        _lib.call("sl_syrk_split", _lib.ptr(Ab), _lib.dtype_code(A.dtype), int(tr), s, w, k_full, A.stride(0),
                  _lib.ptr(S) if S is not None else None, seg, _lib.ptr(slabs), n_slabs, R, G,
                  int(k0 + w >= n), _lib.ptr(C), _lib.dtype_code(C.dtype), C.stride(0) if s > 1 else 1, ord(up), float(alpha),
                  float(beta), st)
    return C
