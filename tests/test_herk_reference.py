"""The long-double Herk oracle (``herk_reference``) checked on the CPU: hand
cases, the oracle against torch f64 products, every refusal of
``ops.herk._why_not`` (none needs a GPU), flag errors, and ``base.Herk`` on CPU
f64 operands (unchanged: the torch product through a triangle mask) against
the oracle and its ``(K + 4) u`` bound."""
import itertools

import numpy as np
import pytest
import torch

import herk_reference as HR

F64 = torch.float64
NAN = float("nan")


def test_hand_cases():
    A = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    ref, den = HR.reference("N", 1.0, A)
    assert np.array_equal(ref.astype(np.float64), [[14.0, 32.0], [32.0, 77.0]]) and np.array_equal(ref, den)
    ref, den = HR.reference("T", -2.0, A, 0.5, np.full((3, 3), 4.0))
    want = -2.0 * (A.T @ A) + 2.0
    assert np.array_equal(ref.astype(np.float64), want)
    assert np.array_equal(den.astype(np.float64), 2.0 * (A.T @ A) + 2.0)
    # beta == 0 does not look at C0, alpha == 0 not at A
    ref, den = HR.reference("N", 1.0, A, 0.0, np.full((2, 2), NAN))
    assert np.isfinite(ref).all()
    ref, den = HR.reference("C", 0.0, np.full((2, 3), NAN), 0.25, np.eye(3))
    assert np.array_equal(ref.astype(np.float64), 0.25 * np.eye(3)) and np.array_equal(ref, den)
    ref, den = HR.reference("N", 1.0, np.zeros((4, 0)))
    assert ref.shape == (4, 4) and not ref.any() and not den.any()
    assert HR.bound(0) == 4 * 2.0 ** -53 and HR.bound(60) == 2.0 ** -47


def test_measure():
    ref, den = HR.reference("N", 1.0, np.array([[1.0, 0.0], [0.0, 1.0]]))
    C = np.array([[1.0, NAN], [0.0, 1.0 + 2.0 ** -52]])
    assert HR.measure(C, ref, den, "L") == 2.0 ** -52          # the NaN lies outside the triangle
    assert HR.measure(C, ref, den, "U") == float("inf")
    C[1, 0] = 1e-300                                          # den == 0 there: must be exact
    with pytest.raises(AssertionError):
        HR.measure(C, ref, den, "L")
    assert HR.measure(np.zeros((0, 0)), *HR.reference("N", 1.0, np.zeros((0, 3))), "L") == 0.0


@pytest.mark.parametrize("orient,shape", [("N", (37, 300)), ("T", (300, 37)), ("N", (5, 1)), ("T", (1, 5))])
def test_oracle_against_torch(orient, shape):
    g = torch.Generator().manual_seed(3)
    A = torch.rand(*shape, generator=g, dtype=F64) * 2 - 1
    s, K = (shape[1], shape[0]) if orient == "T" else shape
    C0 = torch.rand(s, s, generator=g, dtype=F64)
    ref, den = HR.reference(orient, 0.5, A.numpy(), 0.25, C0.numpy())
    P = A.t() if orient == "T" else A
    got = 0.5 * (P @ P.t()) + 0.25 * C0
    for uplo in "LU":
        e = HR.measure(got.numpy(), ref, den, uplo)
        assert e <= HR.bound(K)
    sym = HR.reference(orient, 0.5, A.numpy())[0]
    assert float(np.abs(sym - sym.T).max()) == 0.0


def _f64(*shape):
    return torch.zeros(*shape, dtype=F64)


def _misaligned(r, c):
    raw = np.zeros(8 * (r * c + 2), dtype=np.uint8)
    off = (-raw.ctypes.data) % 8 + 4                       # base off by 4 B
    mis = torch.from_numpy(np.frombuffer(raw, dtype=np.float64, count=r * c, offset=off)).view(r, c)
    assert mis.data_ptr() % 8 == 4
    return mis


def test_why_not_reasons():
    from libskylark_amd.ops import herk
    why = herk._why_not
    A = _f64(6, 4)
    assert why(A, None, False) == why(A, _f64(6, 6), False) == why(A, _f64(4, 4), True) == "A must be a CUDA tensor"
    assert why(_f64(6), None, False) == why([[1.0]], None, False) == "A must be a dense 2-D tensor"
    assert why(A.to_sparse(), None, False) == "A must be a dense 2-D tensor"
    assert why(A.float(), None, False) == "A must be f64 (got torch.float32)"
    assert why(_f64(12, 8)[::2, ::2], None, False) == "A: needs unit stride along rows or columns"
    assert why(_f64(4).expand(6, 4), None, False) == "A's rows overlap"
    assert why(_misaligned(6, 4), None, False) == "A needs an 8-B aligned base"
    # C
    assert why(A, _f64(6), False) == "C must be a dense 2-D tensor"
    assert why(A, _f64(6, 6).float(), False) == "C must be f64 (got torch.float32)"
    assert why(A, _f64(4, 4), False) == "C must be square of order 6 (got (4, 4))"
    assert why(A, _f64(6, 6), True) == "C must be square of order 4 (got (6, 6))"
    assert why(A, _f64(6, 7), False) == "C must be square of order 6 (got (6, 7))"
    assert why(A, _f64(12, 12)[::2, ::2], False) == "C: needs unit stride along rows or columns"
    assert why(A, _f64(6).expand(6, 6), False) == "C's rows overlap"
    assert why(A, _misaligned(6, 6), False) == "C needs an 8-B aligned base"
    assert why(A, _f64(6, 6).to("meta"), False) == "C is on meta, A on cpu"
    # an empty dimension is not refused, and both layouts of both operands are taken
    for shape in ((0, 4), (4, 0), (0, 0)):
        assert why(_f64(*shape), None, False) == why(_f64(*shape), None, True) == "A must be a CUDA tensor"
    assert why(_f64(4, 6).t(), _f64(6, 7)[:, :6].t(), False) == "A must be a CUDA tensor"
    assert not herk.takes(A, trans=False) and not herk.ok(A, _f64(6, 6), trans=False)
    with pytest.raises(ValueError, match="herk_tri: A must be a CUDA tensor"):
        herk.herk_tri("L", "N", 1.0, A)
    with pytest.raises(ValueError, match="herk_tri: C must be square of order 4"):
        herk.herk_tri("L", "T", 1.0, A, 0.0, _f64(6, 6))


def test_flag_errors():
    from libskylark_amd.ops import herk
    A = _f64(6, 4)
    with pytest.raises(ValueError, match="herk_tri: uplo must be L or U"):
        herk.herk_tri("X", "N", 1.0, A)
    with pytest.raises(ValueError, match="herk_tri: orientation must be N, T or C"):
        herk.herk_tri("L", "Q", 1.0, A)


def test_plan_and_block():
    from libskylark_amd.ops import herk
    t, kh = herk.block()
    assert (t, kh) == (128, 32)
    # (tiles, S) on 256 compute units: 512 slots of two workgroups per CU
    assert herk.plan(0, 100, 256) == (0, 1)
    assert herk.plan(512, 200000, 256) == (10, 102)              # 2 x 512 / 10
    assert herk.plan(130, 8197, 256) == (3, 257)                 # clamped to the 257 slices of K
    assert herk.plan(1024, 200000, 256) == (36, 28)
    assert herk.plan(4096, 65536, 256) == (528, 1)               # the tiles alone fill the slots
    assert herk.plan(300, 0, 256) == (6, 1) and herk.plan(300, 31, 256) == (6, 1)
    assert herk.plan(300, 64, 1) == (6, 1) and herk.plan(128, 64, 1) == (1, 2)
    assert [herk.launches(s, K, sp) for s, K, sp in ((0, 5, 1), (5, 100, 1), (5, 100, 3), (5, 100, 1000), (5, 32, 7))] \
        == [0, 1, 2, 2, 1]
    with pytest.raises(ValueError):
        herk.launches(5, 100, 0)


@pytest.mark.parametrize("orient,uplo,beta", list(itertools.product("NT", "LU", (0.0, 0.5))))
def test_base_herk_cpu_f64_against_the_oracle(orient, uplo, beta):
    from libskylark_amd.base import Herk
    g = torch.Generator().manual_seed(11)
    A = torch.rand(37, 53, generator=g, dtype=F64) * 2 - 1
    s, K = (53, 37) if orient == "T" else (37, 53)
    m = torch.from_numpy(HR.tri_mask(s, uplo))
    C0 = torch.rand(s, s, generator=g, dtype=F64) * 2 - 1
    C = torch.where(m, C0 if beta else torch.full_like(C0, NAN), torch.full_like(C0, NAN))
    before = C.clone().view(torch.int64)
    assert Herk(uplo, orient, -0.75, A, beta, C) is C
    ref, den = HR.reference(orient, -0.75, A.numpy(), beta, C0.numpy())
    e = HR.measure(C.numpy(), ref, den, uplo)
    assert e <= HR.bound(K)
    assert torch.equal(C.view(torch.int64)[~m], before[~m])
