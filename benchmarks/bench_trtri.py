"""f64 upper-triangular inverse three ways, in one process and alternating:
``ops.trtri.trtri_tri`` (the one-triangle kernel ``trtri_tri.hip``, in place),
``algorithms.regression._tri_inv_upper`` with ``SKH_LS_TRINV`` unset (1024-column
blocks of ``torch.linalg.solve_triangular`` against a generated identity, the
path the explicit ``R^-1`` preconditioner takes by default) and one
``torch.linalg.solve_triangular(T, I)`` against the full identity.  The
triangle is ``R = L^T`` of the Cholesky factor of ``B B^T + n I`` with B uniform
in (-1, 1).  Each call is timed with device events after a warm-up call; the
restore of the native path's buffer is not timed, the identity of the one-solve
path is built outside the timed window.  Each path's residual ``e = max |I -
R X| / (|R| |X|)`` over the stored triangle of the leading 2048 x 2048 block
(which depends on that block of R alone) is reported with it.  One JSON line
per path and size, one summary line per pair.  A path that fails (the library
solve's workspace may not allocate at some sizes) is reported as such.

    python benchmarks/bench_trtri.py [--n 4096 5000 16384] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libskylark_amd.algorithms import regression as rg  # noqa: E402
from libskylark_amd.ops import _lib, trtri as ti  # noqa: E402

PREFIX = 2048
U = 2.0 ** -53
NATIVE, BLOCKED, ONE = "ops.trtri.trtri_tri", "regression._tri_inv_upper", "torch.linalg.solve_triangular(T, I)"


def factor(n, dev):
    g = torch.Generator(device=dev).manual_seed(7)
    Bm = torch.empty(n, n, dtype=torch.float64, device=dev).uniform_(-1.0, 1.0, generator=g)
    A = Bm @ Bm.t()
    del Bm
    A.diagonal().add_(float(n))
    L = torch.linalg.cholesky(A)
    del A
    return L.t().contiguous()                    # zeros below the diagonal: the library paths need no mask


def err(R, X, p):
    Rp, Xp = torch.triu(R[:p, :p]), torch.triu(X[:p, :p])
    E = (torch.eye(p, dtype=R.dtype, device=R.device) - Rp @ Xp).abs() / (Rp.abs() @ Xp.abs())
    return float(torch.triu(E).max())


def stats(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 5000, 16384])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_trtri: needs the GPU")
    _lib.require()
    os.environ.pop("SKH_LS_TRINV", None)         # the blocked path is the default one
    dev = torch.device("cuda:0")
    nb, _ = ti.block()
    name = torch.cuda.get_device_name(0)
    lines = []

    def emit(ln):
        lines.append(ln)
        print(json.dumps(ln), flush=True)

    for n in a.n:
        R = factor(n, dev)
        W = torch.empty_like(R)
        assert ti.ok(W)
        p = min(PREFIX, n)
        out = {}

        def native():
            out[NATIVE] = ti.trtri_tri("U", "N", W)

        def blocked():
            out[BLOCKED] = rg._tri_inv_upper(R)

        def one():
            out[ONE] = torch.linalg.solve_triangular(R, out["eye"], upper=True)

        paths = {NATIVE: native, BLOCKED: blocked, ONE: one}
        times, failed = {nm: [] for nm in paths}, {}
        out["eye"] = torch.eye(n, dtype=torch.float64, device=dev)
        for nm, f in list(paths.items()):        # warm-up; a path that cannot run is dropped
            if nm == NATIVE:
                W.copy_(R)
            try:
                f()
                torch.cuda.synchronize()
            except RuntimeError as ex:
                msg = str(ex).splitlines()[0][:200]
                if not any(k in msg.lower() for k in ("alloc", "out of memory", "workspace")):
                    raise                        # only a refused allocation drops a path
                failed[nm] = msg
                del paths[nm]
        for _ in range(a.reps):                  # alternating, one event pair per call
            for nm, f in paths.items():
                if nm == NATIVE:
                    W.copy_(R)               # the other paths leave W, the native result, alone
                out.pop(nm, None)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                times[nm].append(e0.elapsed_time(e1))
        med = {}
        for nm in (NATIVE, BLOCKED, ONE):
            if nm in failed:
                emit({"path": nm, "n": n, "dtype": "f64", "uplo": "U", "diag": "N", "failed": failed[nm], "device": name})
                continue
            st = stats(times[nm])
            med[nm] = st["ms_median"]
            e = err(R, out[nm], p)
            emit({"path": nm, "n": n, "dtype": "f64", "uplo": "U", "diag": "N", "reps": a.reps, **st,
                  "TFLOP_per_s_n3_over_3": round(float(n) ** 3 / 3.0 / st["ms_median"] / 1e9, 3),
                  "e_prefix": e, "e_over_n_plus_1_u": e / ((p + 1) * U), "prefix": p,
                  "launches": ti.launches(n, nb) if nm == NATIVE else None,
                  "extra_n_x_n_buffers": {NATIVE: 0, BLOCKED: 1, ONE: 2}[nm], "device": name})
        for other in (BLOCKED, ONE):
            if NATIVE in med and other in med:
                emit({"summary": f"{NATIVE} / {other}", "n": n, "time_ratio": round(med[NATIVE] / med[other], 3)})
        out.clear()
        del R, W
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
