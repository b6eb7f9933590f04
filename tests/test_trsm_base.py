"""``ops/trsm.py`` without a GPU: what the kernel takes, the flag checks, and
``base.Trsm`` on CPU operands, which must stay on the expression it used
before the native kernel existed."""
import itertools

import pytest
import torch

from libskylark_amd.base import blas as B
from libskylark_amd.ops import trsm as tr

F64 = torch.float64


def _ab(n=6, t=3):
    return torch.zeros(n, n, dtype=F64), torch.zeros(n, t, dtype=F64)


def test_why_not_reasons():
    A, Bm = _ab()
    # CPU operands fail on the device alone, and last
    assert tr._why_not("L", A, Bm) == "A and B must be CUDA tensors"
    assert tr._why_not("R", A, Bm.t()) == "A and B must be CUDA tensors"
    assert not tr.takes("L", A, Bm) and not tr.ok("L", A, Bm)
    assert "A must be a dense 2-D tensor" in tr._why_not("L", A[0], Bm)
    assert "B must be a dense 2-D tensor" in tr._why_not("L", A, Bm[:, 0])
    assert "A must be a dense 2-D tensor" in tr._why_not("L", A.to_sparse(), Bm)
    assert "B must be a dense 2-D tensor" in tr._why_not("L", A, [[0.0]])
    assert "A must be f64" in tr._why_not("L", A.float(), Bm)
    assert "B must be f64" in tr._why_not("L", A, Bm.float())
    assert "B must be f64" in tr._why_not("L", A, Bm.to(torch.complex128))
    assert "A must be square" in tr._why_not("L", A[:, :5], Bm)
    assert "needs 6 rows" in tr._why_not("L", A, Bm[:5])
    assert "needs 6 columns" in tr._why_not("R", A, Bm)
    assert "A: needs unit stride" in tr._why_not("L", torch.zeros(12, 12, dtype=F64)[::2, ::2], Bm)
    assert "B: needs unit stride" in tr._why_not("L", A, torch.zeros(12, 6, dtype=F64)[::2, ::2])
    assert "A's rows overlap" in tr._why_not("L", torch.zeros(11, dtype=F64).as_strided((6, 6), (1, 1)), Bm)
    assert "B's rows overlap" in tr._why_not("L", A, torch.zeros(8, dtype=F64).as_strided((6, 3), (1, 1)))
    raw = bytearray(8 * 38)
    off = (4 - torch.frombuffer(raw, dtype=torch.uint8).data_ptr()) % 8
    mis = torch.frombuffer(raw, dtype=F64, count=36, offset=off).view(6, 6)
    assert mis.data_ptr() % 8 == 4
    assert "A needs an 8-B aligned base" in tr._why_not("L", mis, Bm)
    assert "B needs an 8-B aligned base" in tr._why_not("R", A, mis)
    assert "is on" in tr._why_not("L", A, torch.zeros(6, 3, dtype=F64, device="meta"))
    # overlap: the same memory, a shifted window of it, and B inside A's pitch padding
    G = torch.zeros(6, 10, dtype=F64)
    assert "overlap" in tr._why_not("L", G[:, :6], G[:, :3])
    assert "overlap" in tr._why_not("L", G[:, :6], G[:, 5:8])
    assert "overlap" in tr._why_not("R", G[:, :6], G[:, 4:10])
    assert "overlap" in tr._why_not("L", G[:, :6], G.view(10, 6)[:6, :3])      # another pitch: not decided, refused
    # [Gram | right-hand sides] in one pitched buffer does not overlap
    assert tr._why_not("L", G[:, :6], G[:, 6:]) == "A and B must be CUDA tensors"
    assert tr._why_not("L", G[:, :6], G[:, 7:9]) == "A and B must be CUDA tensors"
    # column-major operands and one-row / one-column ones are layouts the kernel takes
    Ac, Bc = torch.zeros(6, 7, dtype=F64)[:, :6].t(), torch.zeros(3, 8, dtype=F64)[:, :6].t()
    assert tr._why_not("L", Ac, Bc).endswith("CUDA tensors")
    assert tr._why_not("L", torch.zeros(1, 1, dtype=F64), torch.zeros(1, 4, dtype=F64)).endswith("CUDA tensors")
    assert tr._why_not("L", A, torch.zeros(6, dtype=F64).unsqueeze(1)).endswith("CUDA tensors")


def test_regime_threshold():
    A, _ = _ab()
    assert tr.regime("L", torch.zeros(6, 8, dtype=F64)) == "thin"
    assert tr.regime("L", torch.zeros(6, 9, dtype=F64)) == "wide"
    assert tr.regime("R", torch.zeros(8, 6, dtype=F64)) == "thin"
    assert tr.regime("R", torch.zeros(9, 6, dtype=F64)) == "wide"
    assert tr.BASE_NATIVE_REGIMES <= {"thin", "wide"}


@pytest.mark.parametrize("pos,bad", [(0, "X"), (1, "D"), (2, "H"), (3, "L")])
def test_flag_validation(pos, bad):
    A, Bm = _ab()
    flags = ["L", "L", "N", "N"]
    flags[pos] = bad
    with pytest.raises(ValueError, match=("side", "uplo", "orient", "diag")[pos]):
        tr.trsm_tri(*flags, 1.0, A, Bm)
    # good flags (any case, C as T) get as far as the operands
    for flags in (("l", "u", "c", "u"), ("R", "L", "T", "N")):
        with pytest.raises(ValueError, match="CUDA tensors|needs 6"):
            tr.trsm_tri(*flags, 1.0, A, Bm)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("side,uplo,orient,diag", list(itertools.product("LR", "LU", "NT", "NU")))
def test_base_trsm_on_cpu_is_unchanged(side, uplo, orient, diag, dtype):
    n, t, alpha = 37, 5, -0.75
    g = torch.Generator().manual_seed(3)
    A = (torch.randn(n, n, generator=g, dtype=F64) + n * torch.eye(n, dtype=F64)).to(dtype)
    B0 = torch.randn((n, t) if side == "L" else (t, n), generator=g, dtype=F64).to(dtype)
    upper = (uplo == "U") != (orient == "T")
    want = torch.linalg.solve_triangular(A if orient == "N" else A.t(), alpha * B0, upper=upper, left=side == "L",
                                         unitriangular=diag == "U")
    Bm = B0.clone()
    out = B.Trsm(side, uplo, orient, diag, alpha, A, Bm)
    assert out is Bm
    iv = torch.int64 if dtype == F64 else torch.int32
    assert torch.equal(Bm.view(iv), want.view(iv))
