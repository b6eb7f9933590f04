"""f64 inverse of a symmetric positive definite matrix three ways, in one
process and alternating: ``base.HPDInverse(uplo, C)`` (the one-triangle chain
``chol_tri.hip``, ``trtri_tri.hip``, ``trtrmm_tri.hip``, in place in one buffer;
its three stages are timed as well, and so is the ``MakeSymmetric`` that
``ml/admm.py::_block_inverse`` adds to get the full matrix),
``torch.cholesky_inverse(torch.linalg.cholesky(C))`` (what BlockADMM's cached
inverse takes by default) and ``torch.linalg.inv(C)``.  The matrix is
``C = B B^T + n I`` with B uniform in (-1, 1); the default sizes are BlockADMM
block widths.  Each call is timed with device events after a warm-up call; the
restore of the native path's buffer is not timed.  Each path's accuracy is
reported with it: ``resid = ||I - C Z||_1 / (||C||_1 ||Z||_1)`` of the full
(mirrored) inverse, also as a multiple of ``n u``.  One JSON line per path and
size, one summary line per pair.

    python benchmarks/bench_hpdinv.py [--n 1024 2048 4096 8192] [--reps 5] [--uplo L] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libskylark_amd import base as B  # noqa: E402
from libskylark_amd.ops import _lib, trtri as ti, trtrmm as tm  # noqa: E402

U = 2.0 ** -53
NATIVE, CHOLINV, INV = "base.HPDInverse", "torch.cholesky_inverse(torch.linalg.cholesky(C))", "torch.linalg.inv(C)"
STAGES = ("cholesky", "triangular_inverse", "trtrmm", "make_symmetric")


def matrix(n, dev):
    g = torch.Generator(device=dev).manual_seed(7)
    Bm = torch.empty(n, n, dtype=torch.float64, device=dev).uniform_(-1.0, 1.0, generator=g)
    C = Bm @ Bm.t()
    C.diagonal().add_(float(n))
    return torch.tril(C) + torch.tril(C, -1).t()         # exactly symmetric


def resid(C, Z):
    n = C.shape[0]
    R = torch.eye(n, dtype=C.dtype, device=C.device) - C @ Z
    return float(torch.linalg.matrix_norm(R, 1) / (torch.linalg.matrix_norm(C, 1) * torch.linalg.matrix_norm(Z, 1)))


def stats(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1024, 2048, 4096, 8192])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--uplo", choices=["L", "U"], default="L", help="the triangle the native chain works in")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_hpdinv: needs the GPU")
    _lib.require()
    dev = torch.device("cuda:0")
    name = torch.cuda.get_device_name(0)
    lines = []

    def emit(ln):
        lines.append(ln)
        print(json.dumps(ln), flush=True)

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    for n in a.n:
        C = matrix(n, dev)
        W = torch.empty_like(C)
        assert tm.ok(W)
        out = {}

        def native():
            ev = [event()]
            B.Cholesky(a.uplo, W)
            ev.append(event())
            B.TriangularInverse(a.uplo, "N", W)
            ev.append(event())
            B.Trtrmm(a.uplo, W)
            ev.append(event())
            B.MakeSymmetric(a.uplo, W)
            ev.append(event())
            out[NATIVE] = W
            return ev

        def cholinv():
            out[CHOLINV] = torch.cholesky_inverse(torch.linalg.cholesky(C))

        def inv():
            out[INV] = torch.linalg.inv(C)

        paths = {NATIVE: native, CHOLINV: cholinv, INV: inv}
        times = {nm: [] for nm in paths}
        stage = {s: [] for s in STAGES}
        for nm, f in paths.items():                  # warm-up
            if nm == NATIVE:
                W.copy_(C)
            f()
            torch.cuda.synchronize()
        for _ in range(a.reps):                      # alternating, one event pair per call
            for nm, f in paths.items():
                if nm == NATIVE:
                    W.copy_(C)                       # the other paths leave W, the native result, alone
                else:
                    out.pop(nm, None)
                e0 = event()
                ev = f()
                e1 = event()
                e1.synchronize()
                if nm == NATIVE:
                    for s, x, y in zip(STAGES, ev, ev[1:]):
                        stage[s].append(x.elapsed_time(y))
                    times[nm].append(ev[0].elapsed_time(ev[3]))      # the three stages of HPDInverse
                else:
                    times[nm].append(e0.elapsed_time(e1))
        med = {}
        for nm in (NATIVE, CHOLINV, INV):
            st = stats(times[nm])
            med[nm] = st["ms_median"]
            r = resid(C, out[nm])
            ln = {"path": nm, "n": n, "dtype": "f64", "uplo": a.uplo if nm == NATIVE else None, "reps": a.reps, **st,
                  "resid_1norm": r, "resid_over_n_u": r / (n * U),
                  "extra_n_x_n_buffers": {NATIVE: 0, CHOLINV: 2, INV: 2}[nm], "device": name}
            if nm == NATIVE:
                ln["stage_ms_median"] = {s: round(statistics.median(stage[s]), 4) for s in STAGES}
                ln["launches"] = {"triangular_inverse": ti.launches(n, ti.block()[0]),
                                  "trtrmm": tm.launches(n, tm.block()[0])}
                ms = ln["stage_ms_median"]["trtrmm"]
                ln["trtrmm_TFLOP_per_s_n3_over_3"] = round(float(n) ** 3 / 3.0 / ms / 1e9, 3)
            emit(ln)
        for other in (CHOLINV, INV):
            emit({"summary": f"{NATIVE} / {other}", "n": n, "time_ratio": round(med[NATIVE] / med[other], 3)})
        out.clear()
        del C, W
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
