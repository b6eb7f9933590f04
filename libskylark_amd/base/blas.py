"""Cross-type dense / sparse / distributed BLAS: ``Gemm``, ``Gemv``, ``Symm``,
``Herk``, ``Cholesky`` / ``CholeskySolveAfter`` / ``HPDSolve``, ``Trsm``,
``TriangularInverse``, ``Trtrmm``, ``HPDInverse``, explicit-Q ``QR``, ``Axpy``, views, ``DenseCopy``, shape queries.

Reference: ``base/Gemm.hpp:19-583`` (local dense, sparse x dense in all four
orientations, ``[VC,*]^T [VC,*] -> [*,*]`` by local GEMM + all-reduce
(``:84-103``), ``[VC,*] [*,*] -> [VC,*]`` communication-free, computed
matrices materialised on demand ``:541-583``), ``base/Gemv.hpp`` (all-reduce
of ``A^T x``, ``:59``), ``base/Symm.hpp`` (sparse-local, sparse ``[VC,*]``
with broadcasts ``:217-222``), ``base/Trsm.hpp``, ``base/QR.hpp:11-36``
(``ExplicitUnitary``, TSQR for ``[VC,*]``), ``base/basic.hpp:48-70``
(``Axpy`` incl. per-column alphas), ``base/viewing.hpp``, ``base/copy.hpp``,
``base/query.hpp``.

Operands: torch tensors (dense or sparse CSR/CSC/COO, any device),
:class:`~libskylark_amd.base.sparse.SparseMatrix`,
:class:`~libskylark_amd.parallel.DistMatrix` (dense or sparse local shard),
and :class:`ComputedMatrix`.  Orientation flags follow Elemental:
``"N"`` (normal), ``"T"`` (transpose), ``"C"`` (adjoint; = T for real data).

MI355X mapping: local products are hipBLASLt GEMMs / hipSPARSE SpMM through
torch on the tensor's device; distributed products need exactly one RCCL
collective (all-reduce of the ``k x n`` result for ``[VC,*]^T [VC,*]``, an
all-gather of the replicated operand for ``[MC,MR]`` SUMMA panels), sized so
the big operand never moves.
"""
from __future__ import annotations

import torch

from .exceptions import DimensionMismatchError, UnsupportedBaseOperation


# ------------------------------------------------------------------ helpers
class ComputedMatrix:
    """Lazily materialised matrix (``base/computed_matrix.hpp:17-26``):
    sub-classes implement ``height``, ``width`` and ``materialize``."""

    def height(self) -> int:
        raise NotImplementedError

    def width(self) -> int:
        raise NotImplementedError

    def materialize(self) -> torch.Tensor:
        raise NotImplementedError


def _is_dist(X):
    from ..parallel.distmatrix import DistMatrix
    return isinstance(X, DistMatrix)


def _as_tensor(X):
    from .sparse import SparseMatrix
    if isinstance(X, ComputedMatrix):
        return X.materialize()
    if isinstance(X, SparseMatrix):
        return X.to_torch("csr")
    return X


def _op(X: torch.Tensor, o: str) -> torch.Tensor:
    o = o.upper()
    if o == "N":
        return X
    if o in ("T", "C"):
        if X.layout == torch.strided:
            Xt = X.t()
            return Xt.conj() if (o == "C" and X.is_complex()) else Xt
        return X.t()   # sparse: transpose view (CSR <-> CSC)
    raise ValueError(f"orientation must be N, T or C (got {o})")


def _mm(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """Local product with sparse operands allowed on either side."""
    if A.layout != torch.strided and B.layout != torch.strided:
        return torch.sparse.mm(A, B.to_dense()) if A.layout != torch.sparse_csc else torch.sparse.mm(
            A.to_sparse_csr(), B.to_dense())
    if A.layout != torch.strided:
        A = A if A.layout in (torch.sparse_csr, torch.sparse_coo) else A.to_sparse_csr()
        return torch.sparse.mm(A, B)
    if B.layout != torch.strided:
        Bt = B.t()
        Bt = Bt if Bt.layout in (torch.sparse_csr, torch.sparse_coo) else Bt.to_sparse_csr()
        return torch.sparse.mm(Bt, A.t()).t()
    return A @ B


def Height(X) -> int:
    if isinstance(X, ComputedMatrix):
        return X.height()
    return int(X.shape[0])


def Width(X) -> int:
    if isinstance(X, ComputedMatrix):
        return X.width()
    return int(X.shape[1])


# ---------------------------------------------------------------------- Gemm
def Gemm(oA: str, oB: str, alpha, A, B, beta=0.0, C=None):
    """``C = alpha op(A) op(B) + beta C`` across operand types; returns C.

    Distributed cases (reference ``base/Gemm.hpp`` / ``dist_mixed_gemm.hpp``):

    * ``[VC,*]^T [VC,*] -> [*,*]``: local GEMM + one all-reduce;
    * ``[VC,*] [*,*] -> [VC,*]`` (and local replicated B): no communication;
    * ``[*,VC] [VC,*] -> [*,*]``: local GEMM + all-reduce;
    * ``[MC,MR] x [MC,MR] -> [MC,MR]``: SUMMA over row / column panels;
    * anything else: redistribute to a supported pairing (all-to-all)."""
    if _is_dist(A) or _is_dist(B) or _is_dist(C):
        return _gemm_dist(oA, oB, alpha, A, B, beta, C)
    A, B = _as_tensor(A), _as_tensor(B)
    P = _mm(_op(A, oA), _op(B, oB))
    if P.layout != torch.strided:
        P = P.to_dense()
    if alpha != 1.0:
        P = P * alpha
    if C is None:
        return P
    if C.shape != P.shape:
        raise DimensionMismatchError(f"Gemm: C is {tuple(C.shape)}, product is {tuple(P.shape)}")
    if beta == 0.0:
        C.copy_(P)
    else:
        C.mul_(beta).add_(P.to(C.dtype))
    return C


def _gemm_dist(oA, oB, alpha, A, B, beta, C):
    from ..parallel.distmatrix import DistMatrix, is_col_dist, is_row_dist
    tA, tB = oA.upper() != "N", oB.upper() != "N"
    dA, dB = _is_dist(A), _is_dist(B)
    comm = (A if dA else B).comm
    out = None
    if dA and dB and is_row_dist(A.layout) and is_row_dist(B.layout) and tA and not tB:
        # [VC,*]^T [VC,*] -> [*,*]: local partial + all-reduce (base/Gemm.hpp:84-103)
        P = _mm(_op(_as_tensor(A.local), "T"), _as_tensor(B.local))
        P = (P.to_dense() if P.layout != torch.strided else P).contiguous()
        comm.all_reduce(P)
        out = DistMatrix(P, (A.shape[1], B.shape[1]), "STAR_STAR", comm)
    elif dA and is_row_dist(A.layout) and not tA and (not dB or B.layout == "STAR_STAR"):
        # [VC,*] [*,*] -> [VC,*]: communication free
        Bl = _op(_as_tensor(B.local if dB else B), oB)
        P = _mm(_as_tensor(A.local), Bl)
        P = P.to_dense() if P.layout != torch.strided else P
        out = DistMatrix(P, (A.shape[0], Bl.shape[1]), A.layout, comm)
    elif dA and dB and is_col_dist(A.layout) and is_row_dist(B.layout) and not tA and not tB:
        # [*,VC] [VC,*] -> [*,*]: contraction over the distributed index
        P = _mm(_as_tensor(A.local), _as_tensor(B.local))
        P = (P.to_dense() if P.layout != torch.strided else P).contiguous()
        comm.all_reduce(P)
        out = DistMatrix(P, (A.shape[0], B.shape[1]), "STAR_STAR", comm)
    elif dA and dB and A.layout == "MC_MR" and B.layout == "MC_MR" and not tA and not tB:
        out = _summa(A, B)
    elif dA and dB and A.layout == "STAR_STAR" and B.layout == "STAR_STAR":
        P = _mm(_op(_as_tensor(A.local), oA), _op(_as_tensor(B.local), oB))
        out = DistMatrix(P.to_dense() if P.layout != torch.strided else P,
                         (P.shape[0], P.shape[1]), "STAR_STAR", comm)
    elif dA and not dB and A.layout == "STAR_STAR":
        P = _mm(_op(_as_tensor(A.local), oA), _op(_as_tensor(B), oB))
        out = DistMatrix(P.to_dense() if P.layout != torch.strided else P, tuple(P.shape), "STAR_STAR", comm)
    else:
        # general: bring operands to a supported pairing
        if dA and A.local.layout != torch.strided:
            raise UnsupportedBaseOperation(f"Gemm {oA}{oB} with sparse {A.layout} operand")
        if tA and dA and not is_row_dist(A.layout):
            return _gemm_dist(oA, oB, alpha, A.redistribute("VC_STAR"), B, beta, C)
        if not tA and dA and not is_row_dist(A.layout) and A.layout != "STAR_STAR":
            return _gemm_dist(oA, oB, alpha, A.redistribute("VC_STAR"), B, beta, C)
        if dB and B.layout != "STAR_STAR" and not (tA and is_row_dist(B.layout)):
            return _gemm_dist(oA, oB, alpha, A, B.redistribute("STAR_STAR"), beta, C)
        if tA and dB and not is_row_dist(B.layout):
            return _gemm_dist(oA, oB, alpha, A, B.redistribute("VC_STAR"), beta, C)
        if not dA:
            A = DistMatrix(_as_tensor(A), tuple(A.shape), "STAR_STAR", comm)
            return _gemm_dist(oA, oB, alpha, A, B, beta, C)
        if not dB:
            B = DistMatrix(_as_tensor(B), tuple(B.shape), "STAR_STAR", comm)
            return _gemm_dist(oA, oB, alpha, A, B, beta, C)
        raise UnsupportedBaseOperation(f"Gemm {oA}{oB} {A.layout} x {getattr(B, 'layout', 'local')}")
    if alpha != 1.0:
        out.local = out.local * alpha
    if C is None:
        return out
    Cd = C if _is_dist(C) else None
    if Cd is not None and Cd.layout != out.layout:
        out = out.redistribute(Cd.layout, Cd.grid, Cd.block)
    target = Cd.local if Cd is not None else C
    if beta == 0.0:
        target.copy_(out.local)
    else:
        target.mul_(beta).add_(out.local.to(target.dtype))
    return C


def _summa(A, B):
    """``[MC,MR] x [MC,MR] -> [MC,MR]`` on the pr x pc grid: SUMMA (Elemental's
    ``Gemm`` for this layout; reference call sites e.g. ``ml/krr.hpp:423``).

    The inner dimension K is walked in super-panels of ``L = lcm(pr, pc)``
    consecutive K-blocks: every process column owns L / pc blocks of A's
    super-panel and every process row L / pr blocks of B's, so one
    all-gather in the row communicator (A: m/pr x L bK) and one in the
    column communicator (B: L bK x n/pc) bring rank (r, c) exactly the
    operands of its local update ``C_rc += A[R_r, panel] B[panel, C_c]``.
    Memory per rank is one super-panel of each operand (O(m/pr L bK)), not
    whole block rows; the collective volume is SUMMA's m K / pr + K n / pc."""
    import math as _m
    from ..parallel.distmatrix import DistMatrix, _cyclic_blocks
    m, K = A.shape
    K2, n = B.shape
    if K != K2:
        raise DimensionMismatchError("Gemm: inner dimensions differ")
    g = A.grid
    bK = A.block[1]
    if B.grid is not g or B.layout != "MC_MR" or B.block[0] != bK:
        B = B.redistribute("MC_MR", grid=g, block=(bK, B.block[1]))
    dev = A.local.device
    dt = torch.promote_types(A.dtype, B.dtype)
    Aloc = A.local.to(dt)
    Bloc = B.local.to(dt)
    C = torch.zeros(Aloc.shape[0], Bloc.shape[1], dtype=dt, device=dev)
    L = g.pr * g.pc // _m.gcd(g.pr, g.pc)
    nblk = (K + bK - 1) // bK
    # local column offsets of A's K-blocks (this process column) / row offsets of B's
    a_off, off = {}, 0
    for s0, e0 in _cyclic_blocks(K, bK, g.pc, g.mycol):
        a_off[s0 // bK] = (off, e0 - s0)
        off += e0 - s0
    b_off, off = {}, 0
    for s0, e0 in _cyclic_blocks(K, bK, g.pr, g.myrow):
        b_off[s0 // bK] = (off, e0 - s0)
        off += e0 - s0
    for j0 in range(0, nblk, L):
        blocks = list(range(j0, min(nblk, j0 + L)))
        # A super-panel: process column c contributes its blocks j (j % pc == c), in order
        mineA = [a_off[j] for j in blocks if j % g.pc == g.mycol]
        pieceA = torch.cat([Aloc[:, o:o + w] for o, w in mineA], 1) if mineA else Aloc[:, :0]
        cntA = [sum(min(K, (j + 1) * bK) - j * bK for j in blocks if j % g.pc == c) for c in range(g.pc)]
        GA = g.row_comm.all_gather_v(pieceA.contiguous(), cntA, 1) if g.pc > 1 else pieceA
        # B super-panel: process row r contributes its blocks j (j % pr == r)
        mineB = [b_off[j] for j in blocks if j % g.pr == g.myrow]
        pieceB = torch.cat([Bloc[o:o + w] for o, w in mineB], 0) if mineB else Bloc[:0]
        cntB = [sum(min(K, (j + 1) * bK) - j * bK for j in blocks if j % g.pr == r) for r in range(g.pr)]
        GB = g.col_comm.all_gather_v(pieceB.contiguous(), cntB, 0) if g.pr > 1 else pieceB
        # gathered order is owner-major; put both operands in K order
        posA, o = {}, 0
        for c in range(g.pc):
            for j in blocks:
                if j % g.pc == c:
                    w = min(K, (j + 1) * bK) - j * bK
                    posA[j] = (o, w)
                    o += w
        posB, o = {}, 0
        for r in range(g.pr):
            for j in blocks:
                if j % g.pr == r:
                    w = min(K, (j + 1) * bK) - j * bK
                    posB[j] = (o, w)
                    o += w
        Ap = torch.cat([GA[:, posA[j][0]:posA[j][0] + posA[j][1]] for j in blocks], 1)
        Bp = torch.cat([GB[posB[j][0]:posB[j][0] + posB[j][1]] for j in blocks], 0)
        C += Ap @ Bp
    return DistMatrix(C, (m, n), "MC_MR", A.comm, grid=g, block=(A.block[0], B.block[1]))


def Gemv(oA: str, alpha, A, x, beta=0.0, y=None):
    """``y = alpha op(A) x + beta y``; ``[VC,*]^T x`` all-reduces (``base/Gemv.hpp:59``)."""
    xx = x if (hasattr(x, "dim") and x.dim() == 2) or _is_dist(x) else x.reshape(-1, 1)
    yy = None
    if y is not None:
        yy = y if (hasattr(y, "dim") and y.dim() == 2) or _is_dist(y) else y.view(-1, 1)
    r = Gemm(oA, "N", alpha, A, xx, beta, yy)
    if y is not None:
        return y
    if _is_dist(r):
        return r
    return r.reshape(-1) if not (hasattr(x, "dim") and x.dim() == 2) else r


def _symm_native(side: str, uplo: str, alpha, A, B, beta, C):
    """The triangle-reading kernel (``ops/symm.py``) for a local dense A and
    at most 8 right-hand sides; ``None`` when the operands are not its own."""
    from ..ops import symm as _sy
    if not (isinstance(A, torch.Tensor) and isinstance(B, torch.Tensor) and A.dim() == 2 and B.dim() == 2
            and A.shape[0] == A.shape[1] and (C is None or isinstance(C, torch.Tensor))):
        return None
    up = uplo.upper()
    if A.stride(1) != 1 and A.stride(0) == 1:
        # a column-major A is the row-major transpose with the other triangle stored
        A, up = A.t(), ("U" if up == "L" else "L")
    X = B if side.upper() == "L" else B.t()          # B A = (A B^T)^T for symmetric A
    if up not in ("L", "U") or not _sy.takes(A, X):
        return None
    if C is None:
        Y = _sy.symm_tri(A, X, uplo=up, alpha=alpha)
        return Y if side.upper() == "L" else Y.t()
    Ct = C if side.upper() == "L" else C.t()
    if tuple(Ct.shape) != (A.shape[0], X.shape[1]):
        raise DimensionMismatchError(f"Symm: C is {tuple(C.shape)}, the product {(A.shape[0], X.shape[1])}")
    if Ct.dtype == A.dtype and Ct.device == A.device and Ct.stride(1) == 1 and (
            Ct.shape[0] == 1 or Ct.stride(0) >= Ct.shape[1]):
        _sy.symm_tri(A, X, uplo=up, alpha=alpha, beta=beta, out=Ct)
        return C
    Y = _sy.symm_tri(A, X, uplo=up, alpha=alpha)
    if beta == 0.0:
        Ct.copy_(Y)
    else:
        Ct.mul_(beta).add_(Y.to(Ct.dtype))
    return C


def Symm(side: str, uplo: str, alpha, A, B, beta=0.0, C=None):
    """``C = alpha A B + beta C`` (side L) or ``alpha B A + beta C`` (side R)
    with symmetric A stored in its ``uplo`` triangle (``base/Symm.hpp``);
    the other triangle is never used.

    A local dense f32 / f64 A on the GPU with 16-B aligned rows (row- or
    column-major) and a local B of at most 8 columns (side L) or rows (side
    R) run the native triangle-reading kernel (``ops/symm.py``): one pass
    over the stored triangle, no n x n temporary, f32 sums inside 256 x 256
    tiles and f64 across them.  Every other operand (distributed, sparse,
    CPU, wider B, unaligned A, other dtypes) forms the full symmetric matrix
    from the triangle (three n x n temporaries) and calls ``Gemm``."""
    if not _is_dist(A) and not _is_dist(B) and not _is_dist(C):
        out = _symm_native(side, uplo, alpha, A, B, beta, C)
        if out is not None:
            return out
    if _is_dist(A):
        Af = A.to_global()
    else:
        Af = _as_tensor(A)
    if Af.layout != torch.strided:
        Af = Af.to_dense()
    tri = torch.tril(Af) if uplo.upper() == "L" else torch.triu(Af)
    S = tri + tri.t() - torch.diag(torch.diagonal(Af))
    if side.upper() == "L":
        return Gemm("N", "N", alpha, S, B, beta, C) if not _is_dist(B) else _dist_left(S, alpha, B, beta, C)
    return Gemm("N", "N", alpha, B, S, beta, C)


def _tri_mask(s: int, uplo: str, device) -> torch.Tensor:
    ones = torch.ones(s, s, dtype=torch.bool, device=device)
    return torch.tril(ones) if uplo == "L" else torch.triu(ones)


def _tri_update(C: torch.Tensor, uplo: str, P: torch.Tensor, beta) -> torch.Tensor:
    """``uplo`` triangle of C <- P + beta C; the other triangle keeps its bits
    and ``beta == 0`` takes nothing from C."""
    new = P.to(C.dtype) if beta == 0.0 else (C * beta).add_(P.to(C.dtype))
    C.copy_(torch.where(_tri_mask(C.shape[0], uplo, C.device), new, C))
    return C


def _flag(value, name: str, allowed: str) -> str:
    from ..ops import _tri
    return _tri.flag(value, name, allowed)


def _masked(A: torch.Tensor, uplo: str):
    """``(mask, S)``: the mask of the ``uplo`` triangle and A with zeros outside it."""
    mask = _tri_mask(A.shape[0], uplo, A.device)
    return mask, torch.where(mask, A, torch.zeros((), dtype=A.dtype, device=A.device))


def _dense_square(name: str, A) -> None:
    if not isinstance(A, torch.Tensor) or A.layout != torch.strided or A.dim() != 2 or A.shape[0] != A.shape[1]:
        raise DimensionMismatchError(f"{name}: A must be a dense square matrix (got {tuple(getattr(A, 'shape', ()))})")


def _pivot_status(name: str, linfo: torch.Tensor, info) -> None:
    """``cholesky_ex``'s status into ``info``, or raised when there is none."""
    from .exceptions import NLAError
    if info is not None:
        info.copy_(linfo.reshape(info.shape))
        return
    p = int(linfo.item())
    if p != 0:
        raise NLAError(f"{name}: the matrix is not positive definite: pivot {p} (1-based) "
                       f"is not positive and finite")


def _tri_in_place(name: str, local, uplo, A, *rest, diag=None):
    """The frame of the in-place one-triangle operations: the flags, a
    DistMatrix only as ``[*,*]`` (done on every rank), ``local(uplo[, diag],
    tensor, *rest)`` on the local matrix; returns A."""
    flags = (_flag(uplo, "uplo", "LU"),)
    if diag is not None:
        flags += (_flag(diag, "diag", "NU"),)
    if _is_dist(A):
        if A.layout != "STAR_STAR":
            raise UnsupportedBaseOperation(f"{name} of a {A.layout} matrix (only [*,*] and local)")
        local(*flags, A.local, *rest)
    else:
        local(*flags, _as_tensor(A), *rest)
    return A


def _herk_local(uplo: str, trans: bool, alpha, A: torch.Tensor, beta, C: torch.Tensor | None) -> torch.Tensor:
    if A.layout != torch.strided:
        A = A.to_dense()
    s, k = (A.shape[1], A.shape[0]) if trans else A.shape
    if C is None:
        C = torch.zeros(s, s, dtype=A.dtype, device=A.device)
        beta = 0.0
    elif C.dim() != 2 or tuple(C.shape) != (s, s):
        raise DimensionMismatchError(f"Herk: C is {tuple(C.shape)}, op(A) op(A)^T is {(s, s)}")
    from ..ops import herk, syrk
    if (A.dtype == torch.float64 and A.is_cuda and ("T" if trans else "N") in herk.BASE_NATIVE_REGIMES
            and herk.takes(A, C, trans=trans)):
        # f64 GPU operands the kernel takes (C f64 on A's device): the native
        # library is mandatory there (ops/_lib.py), a missing one raises
        return herk.herk_tri(uplo, "T" if trans else "N", alpha, A, beta, C)
    An, tn = A, trans
    if A.is_cuda and k > 0 and s > 0:
        if A.dtype == torch.float32 and A.stride(1) != 1:
            # a column-major A is the row-major operand of the other orientation
            An, tn = (A.t(), not trans) if A.stride(0) == 1 else (A.contiguous(), trans)
        elif A.dtype == torch.bfloat16 and not trans and not syrk.takes(A, trans=False):
            An = torch.nn.functional.pad(A, (0, -k % 64)).contiguous()   # zero K columns, 16-B aligned rows
    if not (k > 0 and s > 0 and syrk.takes(An, trans=tn)):
        # f64, bf16 A^T A, CPU: a product in the operand's precision
        Ah = A.t().conj() if A.is_complex() else A.t()
        P = Ah @ A if trans else A @ Ah
        return _tri_update(C, uplo, P * alpha if alpha != 1.0 else P, beta)
    # a GPU operand the kernel takes: the native library is mandatory there
    # (ops/_lib.py), a missing one raises rather than falling back
    if syrk.takes(An, C, trans=tn):
        return syrk.syrk_split(An, C, trans=tn, uplo=uplo, alpha=alpha, beta=beta)
    P = syrk.syrk_split(An, None, trans=tn, uplo=uplo, alpha=alpha)
    return _tri_update(C, uplo, P.to(C.device), beta)


def Herk(uplo: str, orient: str, alpha, A, beta=0.0, C=None):
    """The ``uplo`` triangle of ``C = alpha A A^T + beta C`` (orient N) or
    ``alpha A^T A + beta C`` (orient T / C), Elemental's ``Herk`` (reference
    call sites ``ml/krr.hpp:371``, ``ml/kernels.hpp:241``,
    ``base/distance.hpp:92``).  Only that triangle of C is referenced or
    written; ``C=None`` allocates zeros in A's dtype.  Returns C.

    f32 A on the GPU (either orientation) and bf16 A on the GPU with orient N
    run the native triangular kernel (``ops/syrk.py``: exact bf16-split
    products, f64 across row chunks).  f64 A on the GPU with an f64 C on the
    same device (or none), each with unit stride along rows or columns, runs
    the native one-triangle kernel on the f64 matrix cores (``ops/herk.py``,
    ``herk_tri.hip``): half the flops of the product, no s x s temporary, the
    other triangle of C never read, ``beta == 0`` reads nothing of C,
    bit-identical from run to run.  Every other local case (CPU, complex,
    sparse, f64 A with an f32 C, views with neither unit stride) is a torch
    product in the operand's precision written through a triangle mask.
    ``[VC,*]`` A with orient T: local Herk + one all-reduce of the s x s
    block, replicated result; other distributed layouts are gathered."""
    up, o = _flag(uplo, "uplo", "LU"), _flag(orient, "orientation", "NTC")
    Ct = C.local if _is_dist(C) else C
    if _is_dist(A):
        from ..parallel.distmatrix import is_row_dist
        if o != "N" and is_row_dist(A.layout):
            P = _herk_local(up, True, 1.0, _as_tensor(A.local), 0.0, None).contiguous()
            A.comm.all_reduce(P)
            if alpha != 1.0:
                P = P * alpha
            if Ct is None:
                return P
            if tuple(Ct.shape) != tuple(P.shape):
                raise DimensionMismatchError(f"Herk: C is {tuple(Ct.shape)}, op(A) op(A)^T is {tuple(P.shape)}")
            _tri_update(Ct, up, P, beta)
            return C
        A = A.to_global()
    out = _herk_local(up, o != "N", alpha, _as_tensor(A), beta, Ct)
    return out if C is None else C


Syrk = Herk


def MakeSymmetric(uplo: str, C):
    """Copy the stored ``uplo`` triangle of C over the other one, in place."""
    up = _flag(uplo, "uplo", "LU")
    Ct = C.local if _is_dist(C) else C
    other = Ct.t().conj() if Ct.is_complex() else Ct.t()
    Ct.copy_(torch.where(_tri_mask(Ct.shape[0], up, Ct.device), Ct, other))
    return C


def _dist_left(S, alpha, B, beta, C):
    """Replicated symmetric S times a distributed B (all-gather B once)."""
    from ..parallel.distmatrix import DistMatrix
    Bf = B.to_global()
    P = alpha * (S.to(Bf.dtype) @ Bf)
    out = DistMatrix.from_global(P, B.layout, B.comm, B.grid, B.block)
    if C is None:
        return out
    C.local.mul_(beta).add_(out.local)
    return C


def Trsm(side: str, uplo: str, orient: str, diag: str, alpha, A, B):
    """Triangular solve in place on B: ``op(A) X = alpha B`` (side L) or
    ``X op(A) = alpha B`` (side R) (``base/Trsm.hpp``); A replicated.  Only
    the ``uplo`` triangle of A is read.

    A local (or ``[*,*]``) f64 A on the GPU and a local f64 block of B, each
    with unit stride along rows or columns, run the native blocked kernel
    (``ops/trsm.py``, ``trsm_tri.hip``): in place, no ``alpha B`` temporary,
    no allocation, the other triangle (and with diag U the diagonal) never
    touched, bit-identical from run to run.  The native library is mandatory
    there.  Every other operand (CPU, f32, complex, mixed dtypes, views with
    neither unit stride, a tensor ``alpha``) goes through
    ``torch.linalg.solve_triangular`` as before."""
    from ..ops import trsm as _tr
    Af = A.to_global() if _is_dist(A) else _as_tensor(A)
    Bt = B.local if _is_dist(B) else B
    left = side.upper() == "L"
    if left:
        if _is_dist(B) and B.layout not in ("STAR_STAR", "STAR_VC", "STAR_VR"):
            raise UnsupportedBaseOperation("Trsm left needs the rows of B replicated")
    else:
        if _is_dist(B) and B.layout not in ("STAR_STAR", "VC_STAR", "VR_STAR"):
            raise UnsupportedBaseOperation("Trsm right needs the columns of B replicated")
    if (isinstance(alpha, (int, float)) and side.upper() in ("L", "R") and _tr.takes(side, Af, Bt)
            and _tr.regime(side, Bt) in _tr.BASE_NATIVE_REGIMES):
        # GPU operands the kernel takes: the native library is mandatory there
        # (ops/_lib.py), a missing one raises rather than falling back
        _tr.trsm_tri(side, uplo, orient, diag, alpha, Af, Bt)
        return B
    upper = uplo.upper() == "U"
    unit = diag.upper() == "U"
    if orient.upper() != "N":
        Af, upper = Af.t(), not upper
    X = torch.linalg.solve_triangular(Af.to(Bt.dtype), alpha * Bt, upper=upper, left=left, unitriangular=unit)
    Bt.copy_(X)
    return B


def _triangular_inverse_local(up: str, dg: str, A: torch.Tensor) -> torch.Tensor:
    from ..ops import trtri as _ti
    _dense_square("TriangularInverse", A)
    if _ti.takes(A):
        # a GPU operand the kernel takes: the native library is mandatory there
        # (ops/_lib.py), a missing one raises rather than falling back
        _ti.trtri_tri(up, dg, A)
        return A
    n = A.shape[0]
    if n == 0:
        return A
    mask, S = _masked(A, up)
    eye = torch.eye(n, dtype=A.dtype, device=A.device)
    if dg == "U":
        mask = mask & ~eye.bool()
        S = torch.where(mask, S, eye)
    X = torch.linalg.solve_triangular(S, eye, upper=up == "U", unitriangular=dg == "U")
    A.copy_(torch.where(mask, X, A))
    return A


def TriangularInverse(uplo: str, diag: str, A):
    """Overwrite the ``uplo`` triangle of the triangular A with the same
    triangle of its inverse: Elemental's ``TriangularInverse`` (reference call
    site ``algorithms/regression/accelerated_linearl2_regression_solver_Elemental.hpp:63``,
    the explicit ``R^-1`` of Blendenpik / LSRN).  Only that triangle is read or
    written, and with diag U not its diagonal, which is taken as ones; the
    rest keeps its bits and may hold anything.  Returns A.

    A local f64 matrix on the GPU with unit stride along rows or columns runs
    the native blocked kernel (``ops/trtri.py``, ``trtri_tri.hip``): in place,
    ``n^3 / 3`` flops, no identity, no second n x n buffer, no allocation,
    bit-identical from run to run.  The native library is mandatory there.
    Every other local operand (CPU, f32, complex, views with neither unit
    stride) goes through ``torch.linalg.solve_triangular`` on a masked copy
    against the identity, written back through the triangle mask.  A ``[*,*]``
    DistMatrix is inverted on every rank; distributed layouts raise
    :class:`UnsupportedBaseOperation`."""
    return _tri_in_place("TriangularInverse", _triangular_inverse_local, uplo, A, diag=diag)


def _cholesky_local(up: str, A: torch.Tensor, info) -> torch.Tensor:
    from ..ops import _tri, cholesky as _ch
    _dense_square("Cholesky", A)
    An, un = _tri.row_major(A, (up, "LU"))
    if _ch.takes(An):
        # a GPU operand the kernel takes: the native library is mandatory there
        # (ops/_lib.py), a missing one raises rather than falling back
        _ch.chol_tri(An, un, info)
        return A
    F, linfo = torch.linalg.cholesky_ex(_masked(A, up)[1], upper=up == "U")
    _tri_update(A, up, F, 0.0)
    _pivot_status("Cholesky", linfo, info)
    return A


def Cholesky(uplo: str, A, info=None):
    """Overwrite the ``uplo`` triangle of the Hermitian positive definite A
    with its Cholesky factor, ``A = L L^H`` (L) or ``A = U^H U`` (U):
    Elemental's ``Cholesky`` (reference call sites ``ml/krr.hpp:372``,
    ``:640``).  Only that triangle is read or written; the other one keeps its
    bits and may hold anything.  Returns A.

    A local f64 matrix on the GPU with unit stride along rows or columns runs
    the native blocked kernel (``ops/cholesky.py``: substitution panel solves,
    trailing updates on the f64 matrix cores, no n x n temporary).  Every
    other local operand (CPU, f32, complex, views with neither unit stride)
    goes through ``torch.linalg.cholesky_ex`` on a masked copy.  A ``[*,*]``
    DistMatrix is factored on every rank; distributed layouts raise
    :class:`UnsupportedBaseOperation`.

    A pivot that is not positive raises :class:`NLAError` naming its 1-based
    index, unless ``info`` (an int32 one-element tensor on A's device) is
    given: then the index (0: none) is left there without a host
    synchronisation and nothing is raised."""
    return _tri_in_place("Cholesky", _cholesky_local, uplo, A, info)


def CholeskySolveAfter(uplo: str, orient: str, F, B):
    """Solve ``A X = B`` in place on B from the Cholesky factor of A in the
    ``uplo`` triangle of F (Elemental's ``cholesky::SolveAfter``, reference
    ``ml/krr.hpp:398``, ``:650``): two triangular solves through :func:`Trsm`.
    For f64 operands on the GPU both run the native kernel (``trsm_tri.hip``),
    which cannot read the other triangle of F; elsewhere the library solve
    gives finite, bit-equal solutions with NaN there
    (``tests/test_gpu_chol.py``), so F is never masked into a temporary.
    ``orient`` N, or T / C for real data (A is symmetric); B local or a
    DistMatrix with replicated rows.  Returns B."""
    up, o = _flag(uplo, "uplo", "LU"), _flag(orient, "orientation", "NTC")
    Fl = F.local if _is_dist(F) else _as_tensor(F)
    if _is_dist(F) and F.layout != "STAR_STAR":
        raise UnsupportedBaseOperation(f"CholeskySolveAfter with a {F.layout} factor (only [*,*] and local)")
    if Fl.dim() != 2 or Fl.shape[0] != Fl.shape[1] or Height(B) != Fl.shape[0]:
        raise DimensionMismatchError(f"CholeskySolveAfter: F is {tuple(Fl.shape)}, B has {Height(B)} rows")
    if Fl.is_complex():
        if o == "T":
            raise UnsupportedBaseOperation("CholeskySolveAfter with orient T on complex data")
        Fh = Fl.conj()            # Trsm's T does not conjugate
    else:
        Fh = Fl
    if up == "L":
        Trsm("L", "L", "N", "N", 1.0, Fl, B)
        Trsm("L", "L", "T", "N", 1.0, Fh, B)
    else:
        Trsm("L", "U", "T", "N", 1.0, Fh, B)
        Trsm("L", "U", "N", "N", 1.0, Fl, B)
    return B


def HPDSolve(uplo: str, orient: str, A, B):
    """``A X = B`` for Hermitian positive definite A stored in its ``uplo``
    triangle (Elemental's ``HPDSolve``): :func:`Cholesky` then
    :func:`CholeskySolveAfter`.  A ends as the factor, B as the solution;
    returns B.  With f64 operands on the GPU the whole chain is native and
    reads one triangle only (``chol_tri.hip``, ``trsm_tri.hip``)."""
    Cholesky(uplo, A)
    return CholeskySolveAfter(uplo, orient, A, B)


def _trtrmm_local(up: str, A: torch.Tensor) -> torch.Tensor:
    from ..ops import trtrmm as _tm
    _dense_square("Trtrmm", A)
    if _tm.takes(A):
        # a GPU operand the kernel takes: the native library is mandatory there
        # (ops/_lib.py), a missing one raises rather than falling back
        _tm.trtrmm_tri(up, A)
        return A
    n = A.shape[0]
    if n == 0:
        return A
    mask, S = _masked(A, up)
    Sh = S.t().conj() if S.is_complex() else S.t()
    A.copy_(torch.where(mask, Sh @ S if up == "L" else S @ Sh, A))
    return A


def Trtrmm(uplo: str, A):
    """Overwrite the ``uplo`` triangle of A, which holds a triangular factor,
    with the same triangle of ``L^H L`` (L) or ``U U^H`` (U): Elemental's
    ``Trtrmm`` (LAPACK's LAUUM), the last stage of :func:`HPDInverse`.  Only
    that triangle is read or written; the rest keeps its bits and may hold
    anything.  Returns A.

    A local f64 matrix on the GPU with unit stride along rows or columns runs
    the native kernel (``ops/trtrmm.py``, ``trtrmm_tri.hip``): in place,
    ``n^3 / 3`` flops, no second n x n buffer, no allocation, bit-identical
    from run to run.  The native library is mandatory there.  Every other
    local operand (CPU, f32, complex, views with neither unit stride) is one
    torch product of a masked copy, written back through the triangle mask.
    A ``[*,*]`` DistMatrix is done on every rank; distributed layouts raise
    :class:`UnsupportedBaseOperation`."""
    return _tri_in_place("Trtrmm", _trtrmm_local, uplo, A)


def _hpd_inverse_local(up: str, A: torch.Tensor, info) -> torch.Tensor:
    from ..ops import trtrmm as _tm
    _dense_square("HPDInverse", A)
    if _tm.takes(A):
        # the three native stages, in place on the one triangle; a pivot that
        # is not positive raises in Cholesky, before the other two run
        _cholesky_local(up, A, info)
        _triangular_inverse_local(up, "N", A)
        _trtrmm_local(up, A)
        return A
    n = A.shape[0]
    if n == 0:
        if info is not None:
            info.zero_()
        return A
    mask, S = _masked(A, up)
    Sh = S.t().conj() if S.is_complex() else S.t()
    S = S + Sh - torch.diag_embed(S.diagonal())          # the Hermitian matrix that the triangle stores
    F, linfo = torch.linalg.cholesky_ex(S, upper=up == "U")
    _pivot_status("HPDInverse", linfo, info)
    A.copy_(torch.where(mask, torch.cholesky_inverse(F, upper=up == "U"), A))
    return A


def HPDInverse(uplo: str, A, info=None):
    """Overwrite the ``uplo`` triangle of the Hermitian positive definite A
    with the same triangle of ``A^-1``: Elemental's ``HPDInverse`` (reference
    call site ``ml/BlockADMM.hpp:437``, ``El::Inverse(*Cache[j])``).  Three
    in-place stages on the one triangle: :func:`Cholesky`,
    :func:`TriangularInverse`, :func:`Trtrmm` (``A^-1 = X^H X`` with
    ``X = L^-1``, or ``Y Y^H`` with ``Y = U^-1``).  Only that triangle is read
    or written; the rest keeps its bits and may hold anything.  Returns A.

    A local f64 matrix on the GPU with unit stride along rows or columns runs
    native end to end (``chol_tri.hip``, ``trtri_tri.hip``,
    ``trtrmm_tri.hip``): one buffer, no allocation.  Every other local operand
    goes through ``torch.linalg.cholesky_ex`` and ``torch.cholesky_inverse``
    on a masked Hermitian copy, written back through the triangle mask.  A
    ``[*,*]`` DistMatrix is inverted on every rank; distributed layouts raise
    :class:`UnsupportedBaseOperation`.

    Failure is :func:`Cholesky`'s: a pivot that is not positive raises
    :class:`NLAError` naming its 1-based index before the other stages run,
    unless ``info`` (an int32 one-element tensor on A's device) is given: then
    the index (0: none) is left there without a host synchronisation and
    nothing is raised; on a non-zero status the triangle's contents are
    unspecified."""
    return _tri_in_place("HPDInverse", _hpd_inverse_local, uplo, A, info)


def ExplicitUnitary(A):
    """Overwrite A with the Q factor of its QR (``base/QR.hpp:11-36``): TSQR for
    ``[VC,*]`` (one all-gather of the k x k R factors), Householder locally."""
    from . import linalg as L
    if _is_dist(A):
        from ..parallel.distmatrix import is_row_dist
        if not is_row_dist(A.layout):
            B = A.redistribute("VC_STAR")
            ExplicitUnitary(B)
            A.local.copy_(B.redistribute(A.layout, A.grid, A.block).local)
            return A
        Q, _ = L.tsqr(A.local, A.comm)
        A.local.copy_(Q.to(A.local.dtype))
        return A
    Q, _ = torch.linalg.qr(A)
    A.copy_(Q)
    return A


def QR(A):
    """(Q, R) with Q explicit (distributed ``[VC,*]``: TSQR)."""
    from . import linalg as L
    if _is_dist(A):
        from ..parallel.distmatrix import DistMatrix
        B = A if A.layout in ("VC_STAR", "VR_STAR") else A.redistribute("VC_STAR")
        Q, R = L.tsqr(B.local, B.comm)
        return DistMatrix(Q.to(B.local.dtype), B.shape, B.layout, B.comm), R
    return torch.linalg.qr(A)


# ---------------------------------------------------------------- basic ops
def Axpy(alpha, X, Y):
    """``Y += alpha X``; ``alpha`` may be a per-column vector (``base/basic.hpp:48-70``)."""
    Xl = X.local if _is_dist(X) else X
    Yl = Y.local if _is_dist(Y) else Y
    if isinstance(alpha, torch.Tensor) and alpha.numel() > 1:
        Yl.add_(Xl * alpha.to(Yl.device, Yl.dtype).view(1, -1))
    else:
        Yl.add_(Xl, alpha=float(alpha))
    return Y


def Scale(alpha, X):
    (X.local if _is_dist(X) else X).mul_(alpha)
    return X


def ColumnView(X, j0: int, width: int):
    """Columns ``[j0, j0+width)`` as a view (``base/viewing.hpp``)."""
    if _is_dist(X):
        from ..parallel.distmatrix import is_row_dist
        if not is_row_dist(X.layout) and X.layout != "STAR_STAR":
            raise UnsupportedBaseOperation("ColumnView of a column-distributed matrix")
        return X.like(X.local[:, j0:j0 + width], (X.shape[0], width))
    return X[:, j0:j0 + width]


def RowView(X, i0: int, height: int):
    if _is_dist(X):
        from ..parallel.distmatrix import is_col_dist
        if not is_col_dist(X.layout) and X.layout != "STAR_STAR":
            raise UnsupportedBaseOperation("RowView of a row-distributed matrix")
        return X.like(X.local[i0:i0 + height], (height, X.shape[1]))
    return X[i0:i0 + height]


def DenseCopy(X) -> torch.Tensor:
    """Dense copy of a sparse operand (``base/copy.hpp:20-30``)."""
    from .sparse import SparseMatrix
    if isinstance(X, SparseMatrix):
        return X.to_dense()
    if isinstance(X, torch.Tensor) and X.layout != torch.strided:
        return X.to_dense()
    if _is_dist(X) and X.local.layout != torch.strided:
        return X.like(X.local.to_dense())
    return X.clone() if isinstance(X, torch.Tensor) else X


def RowDot(X, Y) -> torch.Tensor:
    """Row-wise dot products (``base/inner.hpp`` RowDot); row-distributed
    operands need no communication."""
    Xl = X.local if _is_dist(X) else X
    Yl = Y.local if _is_dist(Y) else Y
    return (Xl * Yl).sum(1)


__all__ = ["ComputedMatrix", "Gemm", "Gemv", "Symm", "Herk", "Syrk", "MakeSymmetric", "Trsm", "TriangularInverse", "Cholesky", "CholeskySolveAfter", "HPDSolve",
           "Trtrmm", "HPDInverse",
           "ExplicitUnitary", "QR", "Axpy", "Scale",
           "ColumnView", "RowView", "DenseCopy", "RowDot", "Height", "Width"]
