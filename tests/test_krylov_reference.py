"""The long-double Krylov oracle (``krylov_reference``) checked on the CPU:
hand-computed one-column steps, whole LSQR / CG solves composed from the
one-step functions against ``numpy.linalg`` and the torch solvers (so the
oracle is the algorithm, not a mirror of the kernels), the guards on inputs
built to violate them, and every crafted case the GPU file uses."""
import math

import numpy as np
import pytest
import torch

import krylov_reference as KR
from libskylark_amd.algorithms import krylov as K

LD = KR.LD


def _close(got, want, rtol=1e-17):
    got, want = np.asarray(got, LD), np.asarray(want, LD)
    return bool((np.abs(got - want) <= rtol * np.abs(want)).all())


def test_row_tables_match_the_native_module():
    from libskylark_amd.ops import krylov_native as kn
    for i, name in enumerate(KR.LSQR_ROWS):
        assert getattr(KR, "S_" + name.upper().replace("_", "")) == i
    assert [kn.S_ALPHA, kn.S_BETA, kn.S_RHOBAR, kn.S_PHIBAR, kn.S_NRMA, kn.S_SQD, kn.S_CNDA, kn.S_NRMX, kn.S_SQX,
            kn.S_CS2, kn.S_SN2, kn.S_ZZ, kn.S_NRMAR0, kn.S_STAG, kn.S_RHO, kn.S_PHI, kn.S_THETA, kn.S_NRMAR] == \
        [KR.S_ALPHA, KR.S_BETA, KR.S_RHOBAR, KR.S_PHIBAR, KR.S_NRMA, KR.S_SQD, KR.S_CNDA, KR.S_NRMX, KR.S_SQX,
         KR.S_CS2, KR.S_SN2, KR.S_ZZ, KR.S_NRMAR0, KR.S_STAG, KR.S_RHO, KR.S_PHI, KR.S_THETA, KR.S_NRMAR]
    assert [kn.C_RHO, kn.C_RHO0, kn.C_ALPHA, kn.C_BETA, kn.C_PQ, kn.C_RR, kn.C_NRMB] == \
        [KR.C_RHO, KR.C_RHO0, KR.C_ALPHA, KR.C_BETA, KR.C_PQ, KR.C_RR, KR.C_NRMB]


def test_lsqr_step_by_hand():
    """rhobar = 3, beta = 4 -> rho = 5, cs = 0.6, sn = 0.8; alpha = 2, phibar =
    10 -> theta = 1.6, rhobar' = -1.2, phi = 6, phibar' = 8, |A^T r| = 9.6."""
    st = np.zeros((18, 1))
    st[KR.S_ALPHA], st[KR.S_BETA], st[KR.S_RHOBAR], st[KR.S_PHIBAR] = 2, 4, 3, 10
    st[KR.S_NRMA], st[KR.S_SQD], st[KR.S_CS2], st[KR.S_NRMAR0], st[KR.S_STAG] = 2, 0.25, -1, 1, 2
    Xn, Wn, s, flags = KR.lsqr_step([[1.0]], [[2.0]], [[3.0]], st, 1e-3, 1e-6, 3)
    q = lambda a, b: LD(a) / LD(b)   # noqa: E731
    assert _close(Xn, [[1 + q(6, 5) * 2]]) and _close(Wn, [[3 - q(16, 50) * 2]])
    w = 3 - q(16, 50) * 2
    gamma = np.sqrt(LD(25) + q(256, 100))
    want = {KR.S_ALPHA: 2, KR.S_BETA: 4, KR.S_RHOBAR: -q(12, 10), KR.S_PHIBAR: 8, KR.S_NRMA: 2,
            KR.S_SQD: q(1, 4) + w * w / 25, KR.S_CNDA: 2 * np.sqrt(q(1, 4) + w * w / 25), KR.S_NRMX: q(6, 5),
            KR.S_SQX: 36 / (gamma * gamma), KR.S_CS2: 5 / gamma, KR.S_SN2: q(16, 10) / gamma, KR.S_ZZ: 6 / gamma,
            KR.S_NRMAR0: 1, KR.S_STAG: 0, KR.S_RHO: 5, KR.S_PHI: 6, KR.S_THETA: q(16, 10), KR.S_NRMAR: q(96, 10)}
    for r, v in want.items():
        assert _close(s[r], [v], 2e-18), (KR.LSQR_ROWS[r], s[r], v)
    assert flags.tolist() == [0]
    # the same column with |A^T r|_0 = 1e5 stops on S1; sq_d = 1e13 on S3 as well
    st[KR.S_NRMAR0] = 1e5
    assert KR.lsqr_step([[1.0]], [[2.0]], [[3.0]], st, 1e-3, 1e-6, 3)[3].tolist() == [1]
    st[KR.S_SQD] = 1e13
    assert KR.lsqr_step([[1.0]], [[2.0]], [[3.0]], st, 1e-3, 1e-6, 3)[3].tolist() == [5]


def test_finish_state_by_hand():
    st = np.zeros((18, 1))
    st[KR.S_NRMA], st[KR.S_ALPHA] = 2, 3
    s = KR.finish_state(st, [36.0], 1)
    assert s[KR.S_BETA, 0] == 6 and s[KR.S_NRMA, 0] == 7 and s[KR.S_ALPHA, 0] == 3
    s = KR.finish_state(st, [36.0], 2)
    assert s[KR.S_ALPHA, 0] == 6 and s[KR.S_NRMA, 0] == 2 and s[KR.S_BETA, 0] == 0


@pytest.mark.parametrize("mode,want", [(0, {KR.C_ALPHA: 8}), (1, {KR.C_RHO0: 8, KR.C_RHO: 1, KR.C_BETA: 0.125}),
                                       (2, {KR.C_BETA: 0.25}), (3, {KR.C_PQ: 1, KR.C_ALPHA: 6})])
def test_cg_dot_by_hand(mode, want):
    """X = (1, 2), Y = (3, -1), Y2 = (2, 2): X . Y = 1, X . Y2 = 6; rho = 8, pq = 4."""
    st = np.zeros((7, 1))
    st[KR.C_RHO], st[KR.C_PQ], st[KR.C_NRMB] = 8, 4, 11
    s = KR.cg_dot(mode, [[1.0], [2.0]], [[3.0], [-1.0]], [[2.0], [2.0]], st)
    for r in range(7):
        assert _close(s[r], [want.get(r, st[r, 0])], 1e-18), KR.CG_ROWS[r]


def test_vector_steps_by_hand():
    X, Y = np.array([[1.0, 2.0], [3.0, 4.0]]), np.array([[5.0, 6.0], [7.0, float("nan")]])
    assert KR.colred(X).tolist() == [10, 20] and KR.colred(X, X[::-1]).tolist() == [6, 16]
    ref, S = KR.axpby(X, Y, a=[2.0, 3.0], sa=-1.0, d=[4.0, 0.0])     # b None: the NaN in Y is not read
    assert ref.tolist() == [[-0.5, 0], [-1.5, 0]] and S.tolist() == [[0.5, 0], [1.5, 0]]
    ref, S = KR.axpby(X, X, b=[1.0, 2.0], sb=-1.0)
    assert ref.tolist() == [[0, -2], [0, -4]] and S.tolist() == [[2, 6], [6, 12]]
    assert KR.colscale(X, [-2.0, 0.0], inv=True)[0].tolist() == [[-0.5, 0], [-1.5, 0]]
    assert KR.colscale(X, [-2.0, 0.0])[0].tolist() == [[-2, 0], [-6, 0]]
    st = np.zeros((7, 2))
    st[KR.C_BETA], st[KR.C_ALPHA], st[KR.C_NRMB], st[KR.C_RHO] = [2, 3], [1, -1], [1e3, 1e-3], [4, 0]
    assert KR.cg_p(X, X, st, -1.0)[0].tolist() == [[-1, -4], [-3, -8]]
    Xn, Rn, s, flags = KR.cg_xr(X, X, X, X, st, True, 0.5, zero_ok=(1,))
    assert Xn.tolist() == [[2, 0], [6, 0]] and Rn.tolist() == [[0, 4], [0, 8]]
    assert s[KR.C_RR].tolist() == [0, 80] and s[KR.C_BETA].tolist() == [0, 0] and flags.tolist() == [1, 0]
    assert KR.rows_gemm(X, Y[:, :1])[0].tolist() == [[19], [43]]


def test_lsqr_composed_from_the_steps():
    A, B = KR.lsqr_problem(60, 12, 3)
    tol, eps = 1e-10, 32 * torch.finfo(torch.float64).eps
    X, code, its = KR.lsqr_solve(A, B, tol, eps, 100)
    want = np.linalg.lstsq(A, B, rcond=None)[0]
    assert code == -2 and its <= 40
    assert float(np.abs(X - want).max() / np.abs(want).max()) < 1e-9
    Xt, ct = K.lsqr(torch.from_numpy(A), torch.from_numpy(B), params=K.KrylovIterParams(tolerance=tol, iter_lim=100))
    assert ct == code
    assert float(np.abs(X - Xt.numpy()).max() / np.abs(want).max()) < 1e-11
    # the iteration limit is reported as such
    assert KR.lsqr_solve(A, B, tol, eps, 3)[1:] == (-6, 3)
    assert K.lsqr(torch.from_numpy(A), torch.from_numpy(B), params=K.KrylovIterParams(tolerance=tol, iter_lim=3))[1] == -6


@pytest.mark.parametrize("variant", ["cg", "pcg", "fcg"])
def test_cg_composed_from_the_steps(variant):
    A, B, Minv = KR.spd_problem(60, 3)
    tol = 1e-10
    Mi = None if variant == "cg" else Minv
    X, code, its = KR.cg_solve(A, B, tol, 200, Mi, flexible=variant == "fcg")
    want = np.linalg.solve(A, B)
    assert code == -1
    assert float(np.abs(X - want).max() / np.abs(want).max()) < 1e-9
    p = K.KrylovIterParams(tolerance=tol, iter_lim=200)
    M = None if Mi is None else K.MatPrecond(torch.from_numpy(Minv))
    f = K.flexible_cg if variant == "fcg" else K.cg
    Xt, ct = f(torch.from_numpy(A), torch.from_numpy(B), params=p, M=M)
    assert ct == code
    if variant != "fcg":
        assert p.iterations == its
    assert float(np.abs(X - Xt.numpy()).max() / np.abs(want).max()) < 1e-10
    assert KR.cg_solve(A, B, tol, 4, Mi, flexible=variant == "fcg")[1:] == (-6, 4)


def test_guards_fire():
    st = KR.crafted_lsqr_state()
    X, W, Z = KR.crafted_lsqr_vectors()
    args = (KR.CRAFT_TOL, KR.CRAFT_EPS, KR.CRAFT_MAX_STAG)
    nw2 = KR.colred(KR.lsqr_xw(X, W, Z, st)[2])
    base, _ = KR.lsqr_scalars(st, nw2, *args)
    for row, val, what in [(KR.S_NRMAR0, base[KR.S_NRMAR][0] / 1e-3 * 1.5, "S1"),
                           (KR.S_NRMX, 1.5 * float(abs(base[KR.S_PHI][0] / base[KR.S_RHO][0]) * np.sqrt(nw2[0])) / 1e-6,
                            "stagnation")]:
        bad = st.copy()
        bad[row, 0] = float(val)
        with pytest.raises(KR.GuardError, match=what):
            KR.lsqr_scalars(bad, nw2, *args)
        KR.lsqr_scalars(bad, nw2, *args, guard=False)
    bad = st.copy()
    bad[KR.S_NRMA, 0] = float(1.5 * base[KR.S_NRMAR][0] / (1e-6 * base[KR.S_PHIBAR][0]))
    with pytest.raises(KR.GuardError, match="S2"):
        KR.lsqr_scalars(bad, nw2, *args)
    bad = st.copy()
    bad[KR.S_SQD, 0] = (0.7e6 / st[KR.S_NRMA, 0]) ** 2
    with pytest.raises(KR.GuardError, match="S3"):
        KR.lsqr_scalars(bad, nw2, *args)
    bad = st.copy()
    bad[KR.S_ZZ, 0] = -bad[KR.S_ZZ, 0]          # phi and delta zz of one sign: the difference cancels
    with pytest.raises(KR.GuardError, match="cancels"):
        KR.lsqr_scalars(bad, nw2, *args)
    bad = st.copy()
    bad[KR.S_RHOBAR, 0] = bad[KR.S_BETA, 0] = 0.0
    with pytest.raises(KR.GuardError, match="zero denominator"):
        KR.lsqr_scalars(bad, nw2, *args)
    bad = st.copy()
    bad[KR.S_CS2, 0] = 0.0
    with pytest.raises(KR.GuardError, match="zero denominator"):
        KR.lsqr_scalars(bad, nw2, *args)
    cg = KR.crafted_cg_state(5, 8)
    with pytest.raises(KR.GuardError, match="zero denominator"):
        KR.cg_scalars(0, cg, np.array([1.0, 2, 0, 4, 5]), zero_ok=(0,))
    with pytest.raises(KR.GuardError, match="zero denominator"):
        KR.cg_scalars(1, cg, np.ones(5))
    with pytest.raises(KR.GuardError, match="zero denominator"):
        KR.cg_xr_scalars(cg, np.ones(5) * 1e9, True, KR.CG_TOL)
    with pytest.raises(KR.GuardError, match="cg stop"):
        KR.cg_xr_scalars(cg, (1.5 * KR.CG_TOL * cg[KR.C_NRMB]) ** 2, False, KR.CG_TOL)


def test_crafted_lsqr_state_meets_every_branch():
    st = KR.crafted_lsqr_state()
    X, W, Z = KR.crafted_lsqr_vectors()
    for dt in (np.float32, np.float64):
        _, _, s, flags = KR.lsqr_step(X.astype(dt), W.astype(dt), Z.astype(dt), st, KR.CRAFT_TOL, KR.CRAFT_EPS,
                                      KR.CRAFT_MAX_STAG)
        assert tuple(flags.tolist()) == KR.CRAFT_FLAGS
        assert tuple(int(v) for v in s[KR.S_STAG]) == KR.CRAFT_STAG
    for r in range(18):
        assert len(set(st[r].tolist())) >= KR.CRAFT_K - 1 or r == KR.S_STAG, KR.LSQR_ROWS[r]


def test_sequences_pass_the_guards():
    """Six guarded iterations of the problems the GPU file iterates on."""
    A, B = KR.lsqr_problem()
    Al = A.astype(LD)
    U, V, Z, W, X, st = KR.lsqr_init(Al, B)
    for _ in range(6):
        U, V, W, X, Z, st, flags = KR.lsqr_iteration(Al, U, V, W, X, Z, st, 1e-10, 1e-9, 3, guard=True)
        assert not flags.any()
    A, B, Minv = KR.spd_problem()
    for Mi, flex in ((None, False), (Minv, False), (Minv, True)):
        assert KR.cg_solve(A, B, 1e-10, 6, Mi, flex, guard=True)[1] == -6


def _cg_shapes():
    for k in KR.KS:
        for m in KR.small_ms(k):
            yield m, k
    yield from KR.CLAMP_256


def test_crafted_cg_cases_pass_the_guards():
    for m, k in _cg_shapes():
        st = KR.crafted_cg_state(m=m, k=k)
        for r in range(7):
            assert len(set(st[r].tolist())) == k, KR.CG_ROWS[r]
        for dt in (np.float32, np.float64):
            Xz, Y, Y2, Q = (v.astype(dt) for v in KR.cg_vectors(m, k, KR.cg_seed(m, k)))
            for mode in range(4):
                s = KR.cg_dot(mode, Xz, Y, Y2, st, zero_ok=KR.cg_zero_ok(mode, k))
                with np.errstate(invalid="ignore"):
                    assert np.isfinite(s.astype(np.float64)).all()
            for idp in (False, True):
                _, _, s, flags = KR.cg_xr(Y, Y2, Q, Xz, st, idp, KR.CG_TOL, zero_ok=KR.cg_zero_ok("xr", k))
                assert flags.tolist() == [1 - c % 2 for c in range(k)]


def test_generic_lsqr_state_passes_the_guards():
    for m, k in [(m, k) for k in KR.KS for m in KR.small_ms(k)] + list(KR.CLAMP_1024):
        st = KR.generic_lsqr_state(k)
        for r in range(18):
            assert len(set(st[r].tolist())) == k or r == KR.S_STAG, KR.LSQR_ROWS[r]
        for dt in (np.float32, np.float64):
            X, W, Z = (v.astype(dt) for v in KR.lsqr_vectors(m, k))
            _, _, s, flags = KR.lsqr_step(X, W, Z, st, KR.CRAFT_TOL, KR.CRAFT_EPS, KR.CRAFT_MAX_STAG)
            assert not flags.any() and not s[KR.S_STAG].any()


def test_shape_tables():
    assert [KR.kp_of(k) for k in KR.KS] == [1, 2, 4, 8, 8, 16, 32, 64, 64, 64]
    assert KR.block_rows(1) == 2048 and KR.block_rows(64) == 32 and KR.block_rows(17) == 64
    assert KR.CLAMP_1024 == ((32805, 33), (32805, 64)) and KR.CLAMP_256 == ((8229, 64), (16421, 17))
    assert math.isclose(KR.pow2_ceil(5.1), 8.0)
