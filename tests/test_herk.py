"""``Herk`` / ``Syrk`` / ``MakeSymmetric`` of ``base/blas.py`` on the CPU paths
(reference ``El::Herk`` call sites ``ml/krr.hpp:371``, ``ml/kernels.hpp:241``,
``base/distance.hpp:92``): only the requested triangle is referenced or
written, against fp64 torch products; ``[VC,*]^T [VC,*]`` on two gloo ranks."""
import pytest
import torch

from mp_utils import run_distributed

from libskylark_amd.base import Herk, MakeSymmetric, Syrk
from libskylark_amd.base import blas as B


def _mask(s, uplo):
    ones = torch.ones(s, s, dtype=torch.bool)
    return torch.tril(ones) if uplo == "L" else torch.triu(ones)


def _ref(A, orient):
    return A @ A.t() if orient == "N" else A.t() @ A


@pytest.mark.parametrize("beta", [0.0, 0.5])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("orient", ["N", "T"])
@pytest.mark.parametrize("shape", [(37, 11), (11, 37)])
def test_herk_triangle_fp64(shape, orient, uplo, beta):
    g = torch.Generator().manual_seed(7)
    A = torch.randn(*shape, generator=g, dtype=torch.float64)
    s = shape[0] if orient == "N" else shape[1]
    m = _mask(s, uplo)
    C0 = torch.randn(s, s, generator=g, dtype=torch.float64)
    # the other triangle is NaN and must stay NaN, bit for bit
    C = torch.where(m, C0, torch.full_like(C0, float("nan")))
    before = C.clone()
    out = Herk(uplo, orient, 0.75, A, beta, C)
    assert out is C
    ref = 0.75 * _ref(A, orient) + beta * C0
    assert torch.allclose(C[m], ref[m], rtol=1e-13, atol=1e-13)
    assert torch.equal(C[~m].view(torch.int64), before[~m].view(torch.int64))
    assert torch.isnan(C[~m]).all()


@pytest.mark.parametrize("uplo", ["L", "U"])
def test_herk_beta_zero_does_not_read_c(uplo):
    g = torch.Generator().manual_seed(8)
    A = torch.randn(37, 11, generator=g, dtype=torch.float64)
    C = torch.full((11, 11), float("nan"), dtype=torch.float64)
    Herk(uplo, "T", 1.0, A, 0.0, C)
    m = _mask(11, uplo)
    assert torch.isfinite(C[m]).all()
    assert torch.allclose(C[m], (A.t() @ A)[m], rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16])
def test_herk_allocates_zeros_outside_triangle(dtype):
    g = torch.Generator().manual_seed(9)
    A = torch.randn(11, 37, generator=g, dtype=torch.float64).to(dtype)
    C = Syrk("L", "N", 1.0, A)
    assert C.dtype == dtype and tuple(C.shape) == (11, 11)
    assert torch.equal(torch.triu(C, 1), torch.zeros_like(C))
    tol = {torch.float64: 1e-13, torch.float32: 1e-5, torch.bfloat16: 3e-2}[dtype]
    ref = A.double() @ A.double().t()
    assert float((torch.tril(C).double() - torch.tril(ref)).abs().max() / ref.abs().max()) < tol
    assert B.Syrk is B.Herk


def test_herk_argument_errors():
    A = torch.randn(5, 3, dtype=torch.float64)
    with pytest.raises(ValueError):
        Herk("X", "N", 1.0, A)
    with pytest.raises(ValueError):
        Herk("L", "Q", 1.0, A)
    with pytest.raises(B.DimensionMismatchError):
        Herk("L", "N", 1.0, A, 0.0, torch.zeros(3, 3, dtype=torch.float64))


@pytest.mark.parametrize("uplo", ["L", "U"])
def test_make_symmetric_round_trip(uplo):
    g = torch.Generator().manual_seed(10)
    A = torch.randn(23, 9, generator=g, dtype=torch.float64)
    full = A.t() @ A
    C = Herk(uplo, "T", 1.0, A)
    # garbage in the unstored triangle is overwritten, the stored one is kept
    C[~_mask(9, uplo)] = float("nan")
    out = MakeSymmetric(uplo, C)
    assert out is C
    assert torch.equal(C, C.t())
    assert torch.allclose(C, full, rtol=1e-13, atol=1e-13)


def _dist_worker(rank, world, n, s):
    from libskylark_amd.base import Herk
    from libskylark_amd.parallel.comm import world as W
    from libskylark_amd.parallel.distmatrix import DistMatrix
    comm = W()
    g = torch.Generator().manual_seed(11)
    A = torch.randn(n, s, generator=g, dtype=torch.float64)
    DA = DistMatrix.from_global(A, "VC_STAR", comm)
    one = Herk("L", "T", 2.0, A)
    P = Herk("L", "T", 2.0, DA)
    assert isinstance(P, torch.Tensor) and tuple(P.shape) == (s, s)
    assert torch.allclose(P, one, rtol=1e-12, atol=1e-12), (P - one).abs().max()
    assert torch.equal(torch.triu(P, 1), torch.zeros_like(P))
    # into a supplied C, upper triangle, beta
    C0 = torch.randn(s, s, generator=g, dtype=torch.float64)
    C = C0.clone()
    Herk("U", "T", 1.0, DA, 0.5, C)
    ref = torch.triu(A.t() @ A + 0.5 * C0) + torch.tril(C0, -1)
    assert torch.allclose(C, ref, rtol=1e-12, atol=1e-12)
    return P


def test_herk_vc_star_two_ranks():
    n, s = 101, 9
    res = run_distributed(_dist_worker, 2, n, s)
    g = torch.Generator().manual_seed(11)
    A = torch.randn(n, s, generator=g, dtype=torch.float64)
    ref = torch.tril(2.0 * (A.t() @ A))
    for P in res:
        assert torch.allclose(P, ref, rtol=1e-12, atol=1e-12)
