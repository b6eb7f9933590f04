"""The lower triangle of the f64 Gram ``C = op(A) op(A)^T`` three ways, in one
process and alternating: ``base.Herk("L", orient, 1, A, 0, C)`` (the native
one-triangle kernel ``herk_tri.hip``), the path ``base.Herk`` took for f64
operands before that kernel (the full torch product written through a triangle
mask, copied here as the baseline) and the bare ``torch.mm``.  A is uniform in
(-1, 1); orient T is the tall ``A^T A`` of the ridge solvers (A is K x s), orient
N is ``A A^T`` (A is s x K).  Each call is timed with device events after a
warm-up call.  Reported per path and shape: the time, TFLOP/s counting the
triangle's ``s^2 K`` flops, the peak of extra device memory during a call
(``torch.cuda.max_memory_allocated`` over what was allocated before it), and the
error measure of ``tests/herk_reference.py`` on the leading 512 x 512 block of
the lower triangle, ``e = max |C - ref| / (|op(A)| |op(A)|^T)`` against an f64 CPU
product (so ``e`` holds that product's own rounding too), also as a multiple
of ``(K + 4) u``.  One JSON line per path and shape, one summary line per pair.

    python benchmarks/bench_herk64.py [--shapes T:200000:1024 N:512:8192] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libskylark_amd import base as B  # noqa: E402
from libskylark_amd.ops import _lib, herk  # noqa: E402

U = 2.0 ** -53
NATIVE, PARENT, MM = "base.Herk", "torch.mm + triangle mask (base.Herk before herk_tri)", "torch.mm"
SHAPES = ["T:200000:1024", "T:65536:4096", "N:4096:4096", "N:512:8192"]
LEAD = 512


def parent_herk(uplo, trans, alpha, A, beta, C):
    """``_herk_local``'s last branch and ``_tri_update`` as they were for f64 A."""
    P = A.t() @ A if trans else A @ A.t()
    P = P * alpha if alpha != 1.0 else P
    new = P.to(C.dtype) if beta == 0.0 else (C * beta).add_(P.to(C.dtype))
    ones = torch.ones(C.shape[0], C.shape[0], dtype=torch.bool, device=C.device)
    mask = torch.tril(ones) if uplo == "L" else torch.triu(ones)
    C.copy_(torch.where(mask, new, C))
    return C


def stats(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=SHAPES, help="orient:K:s")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_herk64: needs the GPU")
    _lib.require()
    dev = torch.device("cuda:0")
    name = torch.cuda.get_device_name(0)
    lines = []

    def emit(ln):
        lines.append(ln)
        print(json.dumps(ln), flush=True)

    for shape in a.shapes:
        orient, K, s = shape.split(":")
        K, s, trans = int(K), int(s), orient != "N"
        g = torch.Generator(device=dev).manual_seed(7)
        A = torch.empty((K, s) if trans else (s, K), dtype=torch.float64, device=dev).uniform_(-1.0, 1.0, generator=g)
        assert herk.ok(A, trans=trans)
        C = {nm: torch.zeros(s, s, dtype=torch.float64, device=dev) for nm in (NATIVE, PARENT)}
        out = {}

        def native():
            out[NATIVE] = B.Herk("L", orient, 1.0, A, 0.0, C[NATIVE])

        def parent():
            out[PARENT] = parent_herk("L", trans, 1.0, A, 0.0, C[PARENT])

        def mm():
            out[MM] = A.t() @ A if trans else A @ A.t()

        paths = {NATIVE: native, PARENT: parent, MM: mm}
        times = {nm: [] for nm in paths}
        peak = {}
        for nm, f in paths.items():                  # warm-up, and the peak of extra memory of one call
            out.pop(MM, None)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            f()
            torch.cuda.synchronize()
            peak[nm] = torch.cuda.max_memory_allocated() - before
        for _ in range(a.reps):                      # alternating, one event pair per call
            for nm, f in paths.items():
                out.pop(MM, None)
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                times[nm].append(e0.elapsed_time(e1))
        w = min(LEAD, s)
        Ph = (A[:, :w].t() if trans else A[:w]).cpu().contiguous()          # the leading rows of op(A)
        ref, den = Ph @ Ph.t(), Ph.abs() @ Ph.abs().t()
        low = torch.tril(torch.ones(w, w, dtype=torch.bool))
        tiles, S = herk.plan(s, K)
        med = {}
        for nm in (NATIVE, PARENT, MM):
            st = stats(times[nm])
            med[nm] = st["ms_median"]
            e = float(((out[nm][:w, :w].cpu() - ref).abs() / den)[low].max())
            ln = {"path": nm, "orient": orient, "K": K, "s": s, "dtype": "f64", "reps": a.reps, **st,
                  "TFLOP_per_s_s2K": round(float(s) * s * K / st["ms_median"] / 1e9, 3),
                  "peak_extra_bytes": int(peak[nm]), "peak_extra_s_x_s_buffers": round(peak[nm] / (8.0 * s * s), 3),
                  "e_lead512": e, "e_over_K_plus_4_u": e / ((K + 4) * U), "device": name}
            if nm == NATIVE:
                ln.update({"tiles": tiles, "splits": S, "launches": herk.launches(s, K)})
            emit(ln)
        for other in (PARENT, MM):
            emit({"summary": f"{NATIVE} / {other}", "orient": orient, "K": K, "s": s,
                  "time_ratio": round(med[NATIVE] / med[other], 3)})
        out.clear()
        del A, C
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
