"""Every Krylov device step (``krylov_kernels.hip``) against the long-double
oracle of ``krylov_reference``, one call at a time: the test copies vectors and
state off the GPU before a call and judges that call alone, so errors do not
compound and the derived bounds of the oracle's docstring hold.

Shapes: ``k`` in ``KR.KS`` reaches every column-group template (KP = 1 ... 64)
with full and partly idle lane groups; ``m`` in ``{1, 8 RS, 8 RS + 1}`` (one
row, one full block, one row into the second block); the clamp-crossing sizes
(``KR.CLAMP_1024``, ``KR.CLAMP_256``) and ``m = 0`` where the entry point takes
it.  Every in-place kernel runs on contiguous operands and on views of wider,
taller sentinel-filled buffers with a different leading dimension per operand;
outside the view not one bit may change.  The reduction workspaces are filled
with NaN before each call: a stale partial read would surface.

Measured on an MI355X (largest error / bound over every case, f32 / f64):
element-wise outputs ``axpby`` 0.999 / 0.343, ``colscale`` 0.997 / 0.200,
``lsqr_step`` X, W 0.999 / 0.279, ``cg_p`` 1.000 / 0.111, ``cg_xr`` 0.999 / 0.111
(in f32 half an ulp of T is the whole bound); column reductions 0.041 / 0.057;
``thin_gemm`` 0.989 / 0.053; scalar state needed C = 4.602 (set 16, see
``krylov_reference.MEASURED_C``).  ``_report`` prints the figures of a run."""
import json

import numpy as np
import pytest
import torch

import krylov_reference as KR
from libskylark_amd.base.exceptions import UnsupportedError
from libskylark_amd.ops import _lib as L
from libskylark_amd.ops import krylov_native as kn

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
DT_IDS = ["f32", "f64"]
LAYOUTS = ["contig", "strided"]
# quiet-NaN bit patterns: a leaked sentinel also fails the NaN check
SENT = {torch.float32: (torch.int32, 0x7FC0DEAD), torch.float64: (torch.int64, 0x7FF8DEADBEEF0BAD)}
PADS = (3, 1, 6, 2)         # leading dimension k + pad, per operand
ROW0, COL0 = 2, 1           # offset of a view inside its buffer
NAN = float("nan")
TOL, EPS, MAX_STAG = KR.CRAFT_TOL, KR.CRAFT_EPS, KR.CRAFT_MAX_STAG
SMALL = [(m, k) for k in KR.KS for m in KR.small_ms(k)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nKRYLOV_STATS " + json.dumps(KR.STATS, sort_keys=True))


def _dn(dt):
    return str(dt)[6:]


class Dev:
    """A CPU matrix on the device: contiguous, or a view at (ROW0, COL0) of a
    sentinel-filled buffer three rows taller and ``PADS[i]`` columns wider."""

    def __init__(self, A, dt, dev, layout="contig", i=0):
        t = A if isinstance(A, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(A))
        m, k = t.shape
        self.m, self.k = m, k
        if layout == "contig":
            self.v = self.buf = t.to(device=dev, dtype=dt).contiguous()
            self.view = False
        else:
            it, s = SENT[dt]
            self.buf = torch.full((m + 3, k + PADS[i % 4]), s, dtype=it, device=dev).view(dt)
            self.v = self.buf[ROW0:ROW0 + m, COL0:COL0 + k]
            self.v.copy_(t.to(dt))
            self.view = True
        self.before = None

    def host(self):
        return self.v.cpu().numpy()

    def snap(self):
        self.before = self.buf.clone()
        return self.host()

    def untouched(self, written=False):
        """Bit-identical to the snapshot: everywhere, or (written) outside the view."""
        it = SENT[self.buf.dtype][0]
        a, b = self.buf.view(it), self.before.view(it)
        if not written:
            assert torch.equal(a, b), "a read-only operand changed"
        elif self.view:
            out = torch.ones_like(a, dtype=torch.bool)
            out[ROW0:ROW0 + self.m, COL0:COL0 + self.k] = False
            assert bool((a[out] == b[out]).all()), "store outside the view"


def _vec(v, dev):
    return None if v is None else torch.tensor(np.asarray(v, dtype=np.float64), dtype=torch.float64, device=dev)


def _nan_ws(dev, k):
    kn._ws(dev, k).view(torch.float64).fill_(NAN)


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _rows_same(got, want, rows):
    for r in rows:
        assert torch.equal(_bits(got[r]), _bits(want[r])), f"state row {r} changed"


# ---------------------------------------------------------------- sl_colred
def _colred_case(dev, m, k, dt, layout):
    X = Dev(KR.data(m, k, 7 * k + m % 101), dt, dev, layout, 0)
    Y = Dev(KR.data(m, k, 7 * k + m % 101 + 1), dt, dev, layout, 1)
    Xh, Yh = X.snap(), Y.snap()
    tag = f"colred.{_dn(dt)}"
    _nan_ws(dev, k)
    KR.check_abs(tag + ".sumsq", kn.colsumsq(X.v), KR.colred(Xh), KR.red_bound(Xh))
    _nan_ws(dev, k)
    KR.check_abs(tag + ".dot", kn.coldot(X.v, Y.v), KR.colred(Xh, Yh), KR.red_bound(Xh, Yh))
    # do_sqrt, as the solvers form |B|
    out = torch.full((k,), NAN, dtype=torch.float64, device=dev)
    _nan_ws(dev, k)
    L.call("sl_colred", L.ptr(X.v), X.v.stride(0), None, 0, m, k, L.dtype_code(dt), 0, L.ptr(out), 1,
           L.ptr(kn._ws(dev, k)), kn._st(X.v))
    base, red = KR.spread(np.sqrt, [KR.colred(Xh)], [KR.red_bound(Xh)])
    KR.check_scalar(tag + ".norm", out, base, red)
    X.untouched()
    Y.untouched()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", KR.KS)
def test_colred(dev, k, dt, layout):
    for m in KR.small_ms(k):
        _colred_case(dev, m, k, dt, layout)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("m,k", KR.CLAMP_1024)
def test_colred_clamped_grid(dev, m, k, dt):
    _colred_case(dev, m, k, dt, "strided")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_colsumsq_no_rows(dev, dt):
    for k in (1, 5, 64):
        _nan_ws(dev, k)
        assert kn.colsumsq(torch.empty(0, k, dtype=dt, device=dev)).tolist() == [0.0] * k


# ------------------------------------------------------------- sl_axpby_red
def _lsqr_rows(k, seed):
    """18 x k state of distinct positive scalars."""
    return np.stack([KR.scalars(k, seed + r, signed=False) for r in range(len(KR.LSQR_ROWS))])


def _check_finish(tag, st0, got, Yh1, mode):
    """The state after a finish (mode 1 beta + |A|, 2 alpha) of |Y|^2 over the Y the device wrote."""
    base, red = KR.spread(lambda s: KR.finish_state(st0, s, mode), [KR.colred(Yh1)], [KR.red_bound(Yh1)])
    KR.check_scalar(tag, got, base, red)
    owned = (KR.S_NRMA, KR.S_BETA) if mode == 1 else (KR.S_ALPHA,)
    _rows_same(got, torch.from_numpy(st0).to(got.device), [r for r in range(18) if r not in owned])


def _axpby_case(dev, m, k, dt, layout, ua, ub, ud, sa, sb, red, st0=None, X=None, Y=None, a=None, b=None, d=None):
    """One ``kn.axpby`` call checked; operands random unless given (device tensors)."""
    seed = 13 * k + m % 103
    if X is None:
        X = Dev(KR.data(m, k, seed), dt, dev, layout, 2)
        Y = Dev(KR.data(m, k, seed + 1), dt, dev, layout, 3)
        a = _vec(KR.scalars(k, seed + 2), dev) if ua else None
        b = _vec(KR.scalars(k, seed + 3), dev) if ub else None
        dv = KR.scalars(k, seed + 4)
        if k >= 2:
            dv[k // 2] = 0.0                       # a zero divisor: zero column, zero sum
        d = _vec(dv, dev) if ud else None
        if not ub:
            Y.v.fill_(NAN)                         # b None: the old Y is not read
    st0 = _lsqr_rows(k, seed + 5) if st0 is None else st0
    st = _vec(st0, dev)
    Xh, Yh0 = X.snap(), Y.snap()
    ah, bh, dh = (None if v is None else v.cpu().numpy() for v in (a, b, d))
    tag = f"axpby.{_dn(dt)}"
    _nan_ws(dev, k)
    out = kn.axpby(X.v, Y.v, a=a, sa=sa, b=b, sb=sb, d=d, red=red, st=st)
    Yh1 = Y.host()
    ref, S = KR.axpby(Xh, Yh0 if b is not None else None, ah, sa, bh, sb, dh)
    assert np.isfinite(Yh1).all()
    KR.check_abs(tag, Yh1, ref, KR.elem_bound(ref, S, KR.unit(dt)))
    if dh is not None and m > 0:
        assert not Yh1[:, dh == 0].any()
    X.untouched()
    Y.untouched(written=True)
    if red == 0:
        assert out is None
        _rows_same(st, _vec(st0, dev), range(18))
    elif red == 1:
        KR.check_abs(tag + ".sumsq", out, KR.colred(Yh1), KR.red_bound(Yh1))
        _rows_same(st, _vec(st0, dev), range(18))
    else:
        _check_finish(f"finish_state.{red - 1}", st0, st, Yh1, red - 1)
    return out, st


COMBOS = [(ua, ub, ud) for ua in (False, True) for ub in (False, True) for ud in (False, True)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_axpby_every_combination(dev, dt, layout):
    """null / non-null a, b, d x signs x red 0-3 at k = 5 (KP = 8, three idle
    lanes), one row into the second block."""
    k = 5
    m = KR.block_rows(k) + 1
    for ua, ub, ud in COMBOS:
        for sa, sb in ((1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0)):
            for red in range(4):
                _axpby_case(dev, m, k, dt, layout, ua, ub, ud, sa, sb, red)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", KR.KS)
def test_axpby_shapes(dev, k, dt, layout):
    for i, m in enumerate(KR.small_ms(k)):
        ua, ub, ud = COMBOS[(k + i) % 8]
        for red in range(4):
            _axpby_case(dev, m, k, dt, layout, ua, ub, ud, -1.0, 1.0, red)
            _axpby_case(dev, m, k, dt, layout, True, True, True, 1.0, -1.0, red)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("m,k", KR.CLAMP_1024)
def test_axpby_clamped_grid(dev, m, k, dt):
    for red in (1, 2, 3):
        _axpby_case(dev, m, k, dt, "strided", True, True, True, 1.0, -1.0, red)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", [1, 5, 33])
def test_axpby_fused_finish_agrees_with_setstate(dev, k, dt):
    """red = 2 / 3 (single rank) against red = 1 then ``setstate`` (the
    distributed path) from the same operands: the same partials go through the
    same one-block finish, so the two states agree to a rounding or two."""
    m = KR.block_rows(k) + 1
    for red in (2, 3):
        _, st_a = _axpby_case(dev, m, k, dt, "contig", True, True, False, 1.0, -1.0, red)
        sums, st_b = _axpby_case(dev, m, k, dt, "contig", True, True, False, 1.0, -1.0, 1)
        st0 = st_b.cpu().numpy()
        kn.setstate(sums, st_b, red - 1)
        base = KR.finish_state(st0, sums.cpu().numpy(), red - 1)
        KR.check_scalar(f"setstate.{red - 1}", st_b, base)
        owned = (KR.S_NRMA, KR.S_BETA) if red == 2 else (KR.S_ALPHA,)
        _rows_same(st_b, _vec(st0, dev), [r for r in range(18) if r not in owned])
        KR.check_scalar("fused_vs_setstate", st_a, KR._ld(st_b), c=4)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_axpby_no_rows(dev, dt):
    k = 5
    Y = Dev(np.zeros((0, k)), dt, dev, "strided", 1)
    Y.snap()
    _nan_ws(dev, k)
    out = kn.axpby(torch.empty(0, k, dtype=dt, device=dev), Y.v, b=_vec(KR.scalars(k, 1), dev), red=1)
    assert out.tolist() == [0.0] * k
    Y.untouched()


# -------------------------------------------------------------- sl_colscale
def _colscale_case(dev, m, k, dt, layout, inv, s=None, Y=None):
    if Y is None:
        Y = Dev(KR.data(m, k, 17 * k + m % 107), dt, dev, layout, 0)
        sv = KR.scalars(k, 17 * k + 3)
        sv[0] = -abs(sv[0])                        # a negative divisor divides
        if k >= 2:
            sv[k - 1] = 0.0                        # a zero divisor gives 0
        s = _vec(sv, dev)
    Yh0 = Y.snap()
    kn.colscale(Y.v, s, inv=inv)
    ref, S = KR.colscale(Yh0, s.cpu().numpy(), inv)
    KR.check_abs(f"colscale.{_dn(dt)}", Y.host(), ref, KR.elem_bound(ref, S, KR.unit(dt)))
    Y.untouched(written=True)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", KR.KS)
def test_colscale(dev, k, dt, layout):
    for m in KR.small_ms(k):
        for inv in (False, True):
            _colscale_case(dev, m, k, dt, layout, inv)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_colscale_negative_and_zero_divisors(dev, dt):
    """``/= s[c]``: -2 divides (it used to zero the column), 0 gives 0."""
    Y = torch.ones(3, 3, dtype=dt, device=dev)
    kn.colscale(Y, torch.tensor([-2.0, 0.0, 4.0], dtype=torch.float64, device=dev), inv=True)
    assert Y.tolist() == [[-0.5, 0.0, 0.25]] * 3


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_colscale_no_rows(dev, dt):
    Y = Dev(np.zeros((0, 5)), dt, dev, "strided", 2)
    Y.snap()
    kn.colscale(Y.v, _vec(KR.scalars(5, 2), dev), inv=True)
    Y.untouched()


# ------------------------------------------------------------- sl_lsqr_step
def _lsqr_step_case(dev, dt, X, W, Z, st0, tol, eps, max_stag, tag):
    """One ``kn.lsqr_step`` call on device operands, all 18 rows, X, W and the flags checked."""
    k = X.k
    st = _vec(st0, dev)
    st0 = st.cpu().numpy()
    flags = torch.full((k,), 0x5A5A, dtype=torch.int32, device=dev)
    Xh, Wh, Zh = X.snap(), W.snap(), Z.snap()
    _nan_ws(dev, k)
    kn.lsqr_step(X.v, W.v, Z.v, st, flags, tol, eps, max_stag)
    X1, W1 = X.host(), W.host()
    Xr, SX, Wr, SW = KR.lsqr_xw(Xh, Wh, Zh, st0)
    KR.check_abs(tag + ".X", X1, Xr, KR.elem_bound(Xr, SX, KR.unit(dt), 10))
    KR.check_abs(tag + ".W", W1, Wr, KR.elem_bound(Wr, SW, KR.unit(dt), 10))
    X.untouched(written=True)
    W.untouched(written=True)
    Z.untouched()
    nw2 = KR.colred(W1)
    want, wflags = KR.lsqr_scalars(st0, nw2, tol, eps, max_stag)          # guarded
    base, red = KR.spread(lambda s: KR.lsqr_scalars(st0, s, tol, eps, max_stag, guard=False)[0], [nw2],
                          [KR.red_bound(W1)])
    KR.check_scalar(tag + ".state", st, base, red)
    got = st.cpu().numpy()
    assert got[KR.S_STAG].tolist() == want[KR.S_STAG].astype(np.float64).tolist()
    _rows_same(st, _vec(st0, dev), KR.LSQR_STEP_KEEPS)
    assert flags.tolist() == wflags.tolist()
    return st, flags


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_lsqr_step_crafted_states(dev, dt, layout):
    """k = 9: no flag, S1, S2, S3, stagnation reached, count reset, S1 + S3,
    the first iteration's state, count advancing below the limit."""
    X, W, Z = (Dev(v, dt, dev, layout, i) for i, v in enumerate(KR.crafted_lsqr_vectors()))
    st, flags = _lsqr_step_case(dev, dt, X, W, Z, KR.crafted_lsqr_state(), TOL, EPS, MAX_STAG, f"lsqr_step.{_dn(dt)}")
    assert tuple(flags.tolist()) == KR.CRAFT_FLAGS
    assert tuple(int(v) for v in st[KR.S_STAG].tolist()) == KR.CRAFT_STAG


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", KR.KS)
def test_lsqr_step_shapes(dev, k, dt, layout):
    for m in KR.small_ms(k):
        X, W, Z = (Dev(v, dt, dev, layout, i) for i, v in enumerate(KR.lsqr_vectors(m, k)))
        _lsqr_step_case(dev, dt, X, W, Z, KR.generic_lsqr_state(k), TOL, EPS, MAX_STAG, f"lsqr_step.{_dn(dt)}")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("m,k", KR.CLAMP_1024)
def test_lsqr_step_clamped_grid(dev, m, k, dt):
    X, W, Z = (Dev(v, dt, dev, "strided", i) for i, v in enumerate(KR.lsqr_vectors(m, k)))
    _lsqr_step_case(dev, dt, X, W, Z, KR.generic_lsqr_state(k), TOL, EPS, MAX_STAG, f"lsqr_step.{_dn(dt)}")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_lsqr_six_real_iterations(dev, dt):
    """The native sequence of ``_lsqr_native`` on a 200 x 24 operator, k = 5:
    ``axpby red=2``, ``colscale``, ``axpby red=3``, ``colscale``, ``lsqr_step``,
    each call judged against its oracle from the device's pre-call snapshot."""
    An, Bn = KR.lsqr_problem()
    A = torch.from_numpy(An).to(dev, dt)
    k = Bn.shape[1]
    U = torch.from_numpy(Bn).to(dev, dt)
    beta = kn.colsumsq(U).sqrt()
    kn.colscale(U, beta, inv=True)
    V = (A.t() @ U).contiguous()
    alpha = kn.colsumsq(V).sqrt()
    kn.colscale(V, alpha, inv=True)
    st = kn.lsqr_state(k, dev)
    st[kn.S_ALPHA], st[kn.S_BETA], st[kn.S_RHOBAR], st[kn.S_PHIBAR] = alpha, beta, alpha, beta
    st[kn.S_NRMAR0], st[kn.S_CS2] = alpha * beta, -1.0
    U, V = Dev(U, dt, dev), Dev(V, dt, dev)
    Z, W, X = Dev(V.v.clone(), dt, dev), Dev(V.v.clone(), dt, dev), Dev(torch.zeros_like(V.v), dt, dev)
    m, n = An.shape
    tag = f"lsqr_seq.{_dn(dt)}"
    for _ in range(6):
        AZ = Dev(A @ Z.v, dt, dev)
        _, st = _axpby_case(dev, m, k, dt, "contig", False, True, False, 1.0, -1.0, 2, st0=st.cpu().numpy(),
                            X=AZ, Y=U, b=st[kn.S_ALPHA].clone())
        _colscale_case(dev, m, k, dt, "contig", True, s=st[kn.S_BETA].clone(), Y=U)
        T = Dev(A.t() @ U.v, dt, dev)
        _, st = _axpby_case(dev, n, k, dt, "contig", False, True, False, 1.0, -1.0, 3, st0=st.cpu().numpy(),
                            X=T, Y=V, b=st[kn.S_BETA].clone())
        _colscale_case(dev, n, k, dt, "contig", True, s=st[kn.S_ALPHA].clone(), Y=V)
        Z = Dev(V.v.clone(), dt, dev)
        st, flags = _lsqr_step_case(dev, dt, X, W, Z, st.cpu().numpy(), 1e-10, 1e-9, 3, tag)
        assert not flags.any()
    # six steps of a cond-4 problem: the iterate is most of the way there
    want = np.linalg.lstsq(*KR.lsqr_problem(), rcond=None)[0]
    assert float(np.abs(X.host() - want).max() / np.abs(want).max()) < 0.2


# ------------------------------------------------------------------ CG / FCG
CSENT = 0x5A5A5A5A
CG_OWNS = {0: (KR.C_ALPHA,), 1: (KR.C_RHO0, KR.C_RHO, KR.C_BETA), 2: (KR.C_BETA,), 3: (KR.C_PQ, KR.C_ALPHA)}


def _cg_state(k, dev, st0):
    cs = kn.CGState(k, dev)
    cs.st.copy_(_vec(st0, dev))
    cs.counter[1:] = CSENT
    cs.flags.fill_(0x5A5A)
    return cs


def _cg_before(cs):
    cs.ws.view(torch.float64).fill_(NAN)           # both halves
    return cs.st.cpu().numpy(), cs.st.clone()


def _cg_after(cs, st_before, owned):
    assert cs.counter.tolist() == [0, CSENT, CSENT, CSENT], "ticket not handed back / counter overrun"
    _rows_same(cs.st, st_before, [r for r in range(7) if r not in owned])


def _cg_dot_case(dt, mode, X, Y, Y2, cs, zero_ok, tag):
    k = X.k
    Xh, Yh = X.snap(), Y.snap()
    Y2h = Y2.snap() if Y2 is not None else None
    st0, keep = _cg_before(cs)
    kn.cg_dot(X.v, Y.v, mode, cs, Y2=Y2.v if Y2 is not None else None)
    KR.cg_dot(mode, Xh, Yh, Y2h, st0, zero_ok=zero_ok)                 # guards on the announced zeros only
    sums, deltas = [KR.colred(Xh, Yh)], [KR.red_bound(Xh, Yh)]
    if mode == 3:
        sums.append(KR.colred(Xh, Y2h))
        deltas.append(KR.red_bound(Xh, Y2h))
    base, red = KR.spread(lambda *t: KR.cg_scalars(mode, st0, *t, zero_ok=range(k)), sums, deltas)
    KR.check_scalar(f"{tag}.{mode}", cs.st, base, red)
    _cg_after(cs, keep, CG_OWNS[mode])
    for o in (X, Y, Y2):
        if o is not None:
            o.untouched()


def _cg_dot_shape(dev, m, k, dt, layout):
    V = KR.cg_vectors(m, k, KR.cg_seed(m, k))
    X, Y, Y2 = (Dev(V[i], dt, dev, layout, i) for i in range(3))
    st0 = KR.crafted_cg_state(k, m)
    for mode in range(4):
        cs = _cg_state(k, dev, st0)
        _cg_dot_case(dt, mode, X, Y, Y2 if mode == 3 else None, cs, KR.cg_zero_ok(mode, k), f"cg_dot.{_dn(dt)}")
        # the same CGState again, the state rows reset, other operands
        cs.st.copy_(_vec(st0, dev))
        _cg_dot_case(dt, mode, X, Y2, Y if mode == 3 else None, cs, KR.cg_zero_ok(mode, k), f"cg_dot.{_dn(dt)}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", KR.KS)
def test_cg_dot(dev, k, dt, layout):
    for m in KR.small_ms(k):
        _cg_dot_shape(dev, m, k, dt, layout)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("m,k", KR.CLAMP_256)
def test_cg_dot_clamped_grid(dev, m, k, dt):
    _cg_dot_shape(dev, m, k, dt, "strided")


def _cg_p_case(dt, Z, P, cs, sb, tag):
    Zh, Ph = Z.snap(), P.snap()
    st0, keep = _cg_before(cs)
    kn.cg_p(Z.v, P.v, cs, sb)
    ref, S = KR.cg_p(Zh, Ph, st0, sb)
    KR.check_abs(tag, P.host(), ref, KR.elem_bound(ref, S, KR.unit(dt)))
    _cg_after(cs, keep, ())
    Z.untouched()
    P.untouched(written=True)


def _cg_p_shape(dev, m, k, dt, layout):
    V = KR.cg_vectors(m, k, KR.cg_seed(m, k))
    for sb in (1.0, -1.0):
        Z, P = Dev(V[1], dt, dev, layout, 0), Dev(V[2], dt, dev, layout, 1)
        _cg_p_case(dt, Z, P, _cg_state(k, dev, KR.crafted_cg_state(k, max(m, 1))), sb, f"cg_p.{_dn(dt)}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", KR.KS)
def test_cg_p(dev, k, dt, layout):
    for m in KR.small_ms(k):
        _cg_p_shape(dev, m, k, dt, layout)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("m,k", KR.CLAMP_256 + ((0, 5),))
def test_cg_p_clamped_grid_and_no_rows(dev, m, k, dt):
    _cg_p_shape(dev, m, k, dt, "strided")


def _cg_xr_case(dt, X, P, R, Q, cs, idp, tol, zero_ok, tag):
    k = X.k
    Xh, Ph, Rh, Qh = X.snap(), P.snap(), R.snap(), Q.snap()
    st0, keep = _cg_before(cs)
    kn.cg_xr(X.v, P.v, R.v, Q.v, cs, idp, tol)
    X1, R1 = X.host(), R.host()
    Xr, SX, Rr, SR = KR.cg_xr_vectors(Xh, Ph, Rh, Qh, st0)
    KR.check_abs(tag + ".X", X1, Xr, KR.elem_bound(Xr, SX, KR.unit(dt)))
    KR.check_abs(tag + ".R", R1, Rr, KR.elem_bound(Rr, SR, KR.unit(dt)))
    rr = KR.colred(R1)
    _, wflags = KR.cg_xr_scalars(st0, rr, idp, tol, zero_ok=zero_ok)   # guarded
    base, red = KR.spread(lambda s: KR.cg_xr_scalars(st0, s, idp, tol, guard=False, zero_ok=range(k))[0], [rr],
                          [KR.red_bound(R1)])
    KR.check_scalar(tag + ".state", cs.st, base, red)
    assert cs.flags.tolist() == wflags.tolist()
    _cg_after(cs, keep, (KR.C_RR, KR.C_RHO0, KR.C_RHO, KR.C_BETA) if idp else (KR.C_RR,))
    X.untouched(written=True)
    R.untouched(written=True)
    P.untouched()
    Q.untouched()
    return wflags


def _cg_xr_shape(dev, m, k, dt, layout):
    V = KR.cg_vectors(m, k, KR.cg_seed(m, k))
    for idp in (False, True):
        X, P, R, Q = (Dev(V[i], dt, dev, layout, i) for i in (1, 2, 3, 0))
        cs = _cg_state(k, dev, KR.crafted_cg_state(k, m))
        f = _cg_xr_case(dt, X, P, R, Q, cs, idp, KR.CG_TOL, KR.cg_zero_ok("xr", k), f"cg_xr.{_dn(dt)}")
        assert f.tolist() == [1 - c % 2 for c in range(k)]      # below tol |B| and above it in one call


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", KR.KS)
def test_cg_xr(dev, k, dt, layout):
    for m in KR.small_ms(k):
        _cg_xr_shape(dev, m, k, dt, layout)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("m,k", KR.CLAMP_256)
def test_cg_xr_clamped_grid(dev, m, k, dt):
    _cg_xr_shape(dev, m, k, dt, "strided")


def _thin_gemm_checked(dt, M, X, tag):
    Y = kn.thin_gemm(M, X)
    ref, S = KR.rows_gemm(M.cpu().numpy(), X.cpu().numpy())
    KR.check_abs(tag, Y.cpu().numpy(), ref, KR.gemm_bound(ref, S, KR.unit(dt), M.shape[1]))
    return Y


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("variant", ["cg", "pcg", "fcg"])
def test_cg_six_real_iterations(dev, variant, dt):
    """The call sequence of ``_cg_native`` (CG, preconditioned CG, flexible
    CG) on a 96 x 96 SPD matrix, k = 5, each call judged on its own."""
    An, Bn, Mn = KR.spd_problem()
    A, Minv = torch.from_numpy(An).to(dev, dt), torch.from_numpy(Mn).to(dev, dt)
    flexible, idp = variant == "fcg", variant == "cg"
    k = Bn.shape[1]
    B = torch.from_numpy(Bn).to(dev, dt)
    cs = _cg_state(k, dev, np.zeros((7, k)))
    cs.st[kn.C_NRMB] = kn.colsumsq(B).sqrt()
    X, R, P = Dev(torch.zeros_like(B), dt, dev), Dev(B.clone(), dt, dev), Dev(torch.zeros_like(B), dt, dev)
    if idp:
        cs.st[kn.C_RHO] = kn.colsumsq(R.v)
    tag = f"{variant}_seq.{_dn(dt)}"
    Q = None
    allz = tuple(range(k))
    for itn in range(6):
        if not idp:
            Z = Dev(_thin_gemm_checked(dt, Minv, R.v, f"thin_gemm.{_dn(dt)}"), dt, dev)
        if flexible:
            if itn == 0:
                P.v.copy_(Z.v)
            else:
                _cg_dot_case(dt, 2, Q, Z, None, cs, (), tag)
                _cg_p_case(dt, Z, P, cs, -1.0, tag + ".p")
        elif idp:
            _cg_p_case(dt, R, P, cs, 1.0, tag + ".p")
        else:
            _cg_dot_case(dt, 1, R, Z, None, cs, allz if itn == 0 else (), tag)
            _cg_p_case(dt, Z, P, cs, 1.0, tag + ".p")
        Q = Dev(A @ P.v, dt, dev)
        if flexible:
            _cg_dot_case(dt, 3, P, Q, R, cs, (), tag)
        else:
            _cg_dot_case(dt, 0, P, Q, None, cs, (), tag)
        f = _cg_xr_case(dt, X, P, R, Q, cs, idp, 1e-10, (), tag + ".xr")
        assert not f.any()
    An, Bn, _ = KR.spd_problem()
    res = An @ X.host().astype(np.float64) - Bn
    assert float(np.abs(res).max() / np.abs(Bn).max()) < 0.5


# ------------------------------------------------------------- sl_rows_gemm
def _gemm_operands(dev, dt, nr, nc, k, variant):
    """M (nr x nc) and X (nc x k) on the device.  aligned: contiguous; offset1:
    M's base one element past an aligned address (the scalar path); padded:
    ld a multiple of VEC with nc not (vector body and tail); ldx: X a view
    with a leading dimension above k."""
    vec = 16 // torch.empty(0, dtype=dt).element_size()
    Mh = torch.from_numpy(KR.data(nr, nc, 31 * nr + nc + k)).to(dt)
    Xh = torch.from_numpy(KR.data(nc, k, 37 * nc + k)).to(dt)
    X = Xh.to(dev)
    if variant == "aligned":
        M = Mh.to(dev)
    elif variant == "offset1":
        ld = nc + (3 if nc % 2 else 2)
        flat = torch.full((nr * ld + 1,), NAN, dtype=dt, device=dev)
        M = flat[1:].view(nr, ld)[:, :nc]
        M.copy_(Mh)
        assert M.data_ptr() % 16 != 0
    elif variant == "padded":
        ld = (nc + vec - 1) // vec * vec + vec
        M = torch.full((nr, ld), NAN, dtype=dt, device=dev)[:, :nc]
        M.copy_(Mh)
        assert M.stride(0) % vec == 0 and M.data_ptr() % 16 == 0
    else:
        M = Mh.to(dev)
        X = torch.full((nc, k + 3), NAN, dtype=dt, device=dev)[:, 2:2 + k]
        X.copy_(Xh)
    return M, X


@pytest.mark.parametrize("variant", ["aligned", "offset1", "padded", "ldx"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", range(1, 9))
def test_thin_gemm(dev, k, dt, variant):
    vec = 16 // torch.empty(0, dtype=dt).element_size()
    for nr in (1, 3, 4, 5):
        for nc in (1, vec - 1, 64 * vec, 64 * vec + 1, 64 * vec + vec + 1):
            M, X = _gemm_operands(dev, dt, nr, nc, k, variant)
            assert kn.thin_gemm_ok(M, X)
            _thin_gemm_checked(dt, M, X, f"thin_gemm.{_dn(dt)}")


# ---------------------------------------------------------------- refusals
def _refused(f, unchanged):
    before = [t.clone() for t in unchanged]
    with pytest.raises(UnsupportedError):
        f()
    torch.cuda.synchronize()
    for t, b in zip(unchanged, before):
        it = SENT[t.dtype][0] if t.dtype in SENT else t.dtype
        assert torch.equal(t.view(it), b.view(it)), "a refused call wrote"


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_refusals_write_nothing(dev, dt):
    k = 65
    A, Bm, Cm, Dm = (torch.from_numpy(KR.data(9, k, 50 + i)).to(dev, dt) for i in range(4))
    assert not kn.ok(A)
    s = _vec(KR.scalars(k, 3), dev)
    st = _vec(_lsqr_rows(k, 4), dev)
    flags = torch.full((k,), 0x5A5A, dtype=torch.int32, device=dev)
    out = torch.full((k,), NAN, dtype=torch.float64, device=dev)
    ws = kn._ws(dev, k)
    _refused(lambda: L.call("sl_colred", L.ptr(A), k, None, 0, 9, k, L.dtype_code(dt), 0, L.ptr(out), 0, L.ptr(ws),
                            kn._st(A)), [out])
    _refused(lambda: kn.axpby(A, Bm, b=s, red=2, st=st), [Bm, st])
    _refused(lambda: kn.colscale(Bm, s), [Bm])
    _refused(lambda: kn.lsqr_step(A, Bm, Cm, st, flags, TOL, EPS, MAX_STAG), [A, Bm, st, flags])
    cs = _cg_state(k, dev, np.stack([KR.scalars(k, 60 + r) for r in range(7)]))
    _refused(lambda: kn.cg_dot(A, Bm, 0, cs), [cs.st, cs.counter])
    _refused(lambda: kn.cg_p(A, Bm, cs), [Bm, cs.st])
    _refused(lambda: kn.cg_xr(A, Bm, Cm, Dm, cs, True, 0.5), [A, Cm, cs.st, cs.flags, cs.counter])
    # no rows: the last-block finish of the CG kernels needs a block to run
    k = 5
    E = [torch.empty(0, k, dtype=dt, device=dev) for _ in range(4)]
    cs = _cg_state(k, dev, KR.crafted_cg_state(k, 1))
    for mode in range(4):
        _refused(lambda: kn.cg_dot(E[0], E[1], mode, cs, Y2=E[2]), [cs.st, cs.counter])
    _refused(lambda: kn.cg_xr(E[0], E[1], E[2], E[3], cs, True, 0.5), [cs.st, cs.flags, cs.counter])
    # thin_gemm takes at most eight columns
    M, X9 = torch.from_numpy(KR.data(4, 7, 70)).to(dev, dt), torch.from_numpy(KR.data(7, 9, 71)).to(dev, dt)
    assert not kn.thin_gemm_ok(M, X9)
    Y = torch.full((4, 9), NAN, dtype=dt, device=dev)
    _refused(lambda: L.call("sl_rows_gemm", L.ptr(M), 7, 4, 7, L.ptr(X9), 9, 9, L.ptr(Y), 9, L.dtype_code(dt),
                            kn._st(M)), [Y])
    with pytest.raises(UnsupportedError):
        kn.thin_gemm(M, X9)
