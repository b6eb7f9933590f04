"""f64 triangular solves two ways, in one process and alternating:
``ops.trsm.trsm_tri`` (the one-triangle kernel ``trsm_tri.hip``, in place) and
``torch.linalg.solve_triangular`` (rocBLAS), for the two solves of a lower
Cholesky solve: side L, (uplo L, orient N) and (uplo L, orient T).  The
triangle is the Cholesky factor of ``B B^T + n I`` with B uniform in (-1, 1),
the right-hand sides are standard normal.  Each call is timed with device
events after a warm-up call; the restore of B before a native call is not
timed.  Each path's error ``e = max |B0 - op(T) X| / (|op(T)| |X|)`` over the
leading 2048 rows (orient N; the trailing 2048 for orient T) is reported with
it.  Then one pair of lines per n for ``base.HPDSolve`` against
``torch.linalg.cholesky`` + ``torch.cholesky_solve`` with t = 8, with the
residual ``max |A X - B0| / (|L| |L|^T |X|)`` over the leading 2048 rows.  One JSON
line per path, size and t, one summary line per pair.

    python benchmarks/bench_trsm.py [--n 4096 16384] [--t 1 8 256 4096] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libskylark_amd import base as B  # noqa: E402
from libskylark_amd.ops import _lib, trsm as tr  # noqa: E402

PREFIX = 2048
U = 2.0 ** -53


def spd(n, dev):
    g = torch.Generator(device=dev).manual_seed(7)
    Bm = torch.empty(n, n, dtype=torch.float64, device=dev).uniform_(-1.0, 1.0, generator=g)
    A = Bm @ Bm.t()
    del Bm
    A.diagonal().add_(float(n))
    return A


def err(L, orient, B0, X, p):
    """e over the p rows of the solution that depend on a p x p corner of L alone."""
    n = L.shape[0]
    if orient == "N":
        op, Xs, Bs = L[:p, :p], X[:p], B0[:p]
    else:
        op, Xs, Bs = L[n - p:, n - p:].t(), X[n - p:], B0[n - p:]
    return float(((Bs - op @ Xs).abs() / (op.abs() @ Xs.abs())).max())


def timed(paths, restore, reps):
    for f in paths.values():                 # warm-up
        restore()
        f()
    torch.cuda.synchronize()
    times = {nm: [] for nm in paths}
    for _ in range(reps):                    # alternating, one event pair per call
        for nm, f in paths.items():
            restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[nm].append(e0.elapsed_time(e1))
    return times


def stats(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--t", type=int, nargs="+", default=[1, 8, 256, 4096])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_trsm: needs the GPU")
    _lib.require()
    dev = torch.device("cuda:0")
    nb, _, thin = tr.block()
    name = torch.cuda.get_device_name(0)
    lines = []

    def emit(ln):
        lines.append(ln)
        print(json.dumps(ln), flush=True)

    for n in a.n:
        A0 = spd(n, dev)
        L = torch.linalg.cholesky(A0)            # zeros above the diagonal: the library path needs no mask
        p = min(PREFIX, n)
        nblk = -(-n // nb)
        for t in a.t:
            g = torch.Generator(device=dev).manual_seed(11 + t)
            B0 = torch.empty(n, t, dtype=torch.float64, device=dev).normal_(generator=g)
            W = torch.empty_like(B0)
            assert tr.ok("L", L, W)
            for orient in ("N", "T"):
                out = {}

                def native():
                    out["native"] = tr.trsm_tri("L", "L", orient, "N", 1.0, L, W)

                def library():
                    out["library"] = torch.linalg.solve_triangular(L if orient == "N" else L.t(), B0,
                                                                   upper=orient == "T", left=True)

                paths = {"ops.trsm.trsm_tri": native, "torch.linalg.solve_triangular": library}
                times = timed(paths, lambda: W.copy_(B0), a.reps)
                W.copy_(B0)                  # the last restore came after the last native call
                native()
                errs = {"ops.trsm.trsm_tri": err(L, orient, B0, out["native"], p),
                        "torch.linalg.solve_triangular": err(L, orient, B0, out["library"], p)}
                med = {}
                for nm in paths:
                    st = stats(times[nm])
                    med[nm] = st["ms_median"]
                    native_path = nm == "ops.trsm.trsm_tri"
                    emit({"path": nm, "n": n, "t": t, "dtype": "f64", "side": "L", "uplo": "L", "orient": orient,
                          "regime": ("thin" if t <= thin else "wide") if native_path else None, "reps": a.reps, **st,
                          "GB_per_s_triangle": round(4.0 * n * (n + 1) / st["ms_median"] / 1e6, 1),
                          "TFLOP_per_s": round(float(n) * n * t / st["ms_median"] / 1e9, 3),
                          "e_prefix": errs[nm], "e_over_n_plus_1_u": errs[nm] / ((p + 1) * U), "prefix": p,
                          "launches": (nblk if t <= thin else 2 * nblk - 1) if native_path else None, "device": name})
                emit({"summary": "ops.trsm.trsm_tri / torch.linalg.solve_triangular", "n": n, "t": t, "orient": orient,
                      "time_ratio": round(med["ops.trsm.trsm_tri"] / med["torch.linalg.solve_triangular"], 3)})
            del B0, W
        # HPDSolve against the library's factor-and-solve, t = 8
        t = 8
        g = torch.Generator(device=dev).manual_seed(5)
        B0 = torch.empty(n, t, dtype=torch.float64, device=dev).normal_(generator=g)
        Aw, Xw = torch.empty_like(A0), torch.empty_like(B0)

        def restore():
            Aw.copy_(A0)
            Xw.copy_(B0)

        def hpd():
            B.HPDSolve("L", "N", Aw, Xw)
            return torch.tril(Aw), Xw

        def lib():
            Lc = torch.linalg.cholesky(A0)
            return Lc, torch.cholesky_solve(B0, Lc)

        paths = {"base.HPDSolve": hpd, "torch cholesky + cholesky_solve": lib}
        times = timed(paths, restore, a.reps)
        med = {}
        for nm, f in paths.items():
            restore()
            Lf, Xf = f()
            R = (A0[:p] @ Xf - B0[:p]).abs()
            D = Lf[:p].abs() @ (Lf.abs().t() @ Xf.abs())
            st = stats(times[nm])
            med[nm] = st["ms_median"]
            emit({"path": nm, "n": n, "t": t, "dtype": "f64", "uplo": "L", "reps": a.reps, **st,
                  "resid_prefix": float((R / D).max()), "prefix": p,
                  "trsm_regimes_native": sorted(tr.BASE_NATIVE_REGIMES) if nm == "base.HPDSolve" else None,
                  "device": name})
            del Lf, Xf, R, D
        emit({"summary": "base.HPDSolve / torch cholesky + cholesky_solve", "n": n, "t": t,
              "time_ratio": round(med["base.HPDSolve"] / med["torch cholesky + cholesky_solve"], 3)})
        del A0, L, Aw, Xw, B0
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
