"""f64 Cholesky of an n x n matrix two ways, in one process and alternating:
``base.Cholesky`` (the one-triangle kernel ``chol_tri.hip``, lower triangle in
place, status word on the device) and ``torch.linalg.cholesky`` (rocSOLVER).
The matrix is ``B B^T + n I`` with B uniform in (-1, 1).  Each call is timed
with device events after a warm-up call; the restore of the operand before a
native call is not timed.  Each path's error ``e = max |A - L L^T| / (|L|
|L|^T)`` on the leading 2048 x 2048 block is reported with it.  One JSON line
per path and size, one summary line per size.

    python benchmarks/bench_chol.py [--n 4096 16384] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libskylark_amd import base as B  # noqa: E402
from libskylark_amd.ops import _lib, cholesky as ch  # noqa: E402

PREFIX = 2048


def spd(n, dev):
    g = torch.Generator(device=dev).manual_seed(7)
    Bm = torch.empty(n, n, dtype=torch.float64, device=dev).uniform_(-1.0, 1.0, generator=g)
    A = Bm @ Bm.t()
    del Bm
    A.diagonal().add_(float(n))
    return A


def err(A0, L, p):
    F = torch.tril(L[:p, :p])
    R = ((A0[:p, :p] - F @ F.t()).abs() / (F.abs() @ F.abs().t()))
    return float(torch.tril(R).max())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_chol: needs the GPU")
    _lib.require()
    dev = torch.device("cuda:0")
    nb, _ = ch.block()
    lines = []
    for n in a.n:
        A0 = spd(n, dev)
        W = torch.empty_like(A0)
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        assert ch.ok(W)
        p = min(PREFIX, n)

        def native():
            B.Cholesky("L", W, info)
            return W

        def library():
            return torch.linalg.cholesky(A0)

        paths = {"base.Cholesky": native, "torch.linalg.cholesky": library}
        errs = {}
        for nm, f in paths.items():          # warm-up too
            W.copy_(A0)
            errs[nm] = err(A0, f(), p)
        assert int(info) == 0
        torch.cuda.synchronize()
        times = {nm: [] for nm in paths}
        for _ in range(a.reps):              # alternating, one event pair per call
            for nm, f in paths.items():
                W.copy_(A0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                times[nm].append(e0.elapsed_time(e1))
        med = {nm: statistics.median(t) for nm, t in times.items()}
        for nm in paths:
            lines.append({"path": nm, "n": n, "dtype": "f64", "uplo": "L", "reps": a.reps,
                          "ms_median": round(med[nm], 4), "ms_min": round(min(times[nm]), 4),
                          "ms_max": round(max(times[nm]), 4),
                          "TFLOP_per_s": round(n ** 3 / 3.0 / med[nm] / 1e9, 3),
                          "e_prefix": errs[nm], "e_over_n_plus_1_u": errs[nm] / ((p + 1) * 2.0 ** -53), "prefix": p,
                          "launches": 3 * -(-n // nb) - 2 if nm == "base.Cholesky" else None,
                          "device": torch.cuda.get_device_name(0)})
        lines.append({"summary": "base.Cholesky / torch.linalg.cholesky", "n": n,
                      "time_ratio": round(med["base.Cholesky"] / med["torch.linalg.cholesky"], 3)})
        del A0, W
        torch.cuda.empty_cache()
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
