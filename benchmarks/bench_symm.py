"""S X for a stored symmetric f32 matrix (n = 65536, 16 GiB) two ways, in one
process and alternating: the triangle-reading kernel through ``SymTriOp``
(``symm_tri.hip``, lower triangle only) and the full-matrix product the CG of
FasterKernelRidge uses today -- ``normal_eq.gemv`` (``gemv_kernels.hip``) at
k = 1, ``A @ X`` at k = 4 and 8.  Each call is timed with device events after
a warm-up call; both paths' error against the fp64 product of a 2048-row
prefix block is reported with it.  One JSON line per variant.

    python benchmarks/bench_symm.py [--n 65536] [--reps 5] [--out FILE] [--workgroups G]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libskylark_amd.algorithms.operators import SymTriOp  # noqa: E402
from libskylark_amd.ops import _lib, normal_eq, symm  # noqa: E402

PREFIX = 2048


def symmetric(n, dev):
    """A positive symmetric matrix, filled in row blocks and mirrored in place
    tile by tile (no second n x n temporary)."""
    g = torch.Generator(device=dev).manual_seed(7)
    A = torch.empty(n, n, device=dev)
    for r0 in range(0, n, 8192):
        A[r0:r0 + 8192].uniform_(0.5, 1.5, generator=g)
    B = 4096
    for r0 in range(0, n, B):
        for c0 in range(r0, n, B):
            blk = A[r0:r0 + B, c0:c0 + B]
            if c0 == r0:
                blk.copy_(torch.tril(blk) + torch.tril(blk, -1).t())
            else:
                blk.copy_(A[c0:c0 + B, r0:r0 + B].t())
    return A


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--workgroups", type=int, default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_symm: needs the GPU")
    _lib.require()
    dev = torch.device("cuda:0")
    n = a.n
    A = symmetric(n, dev)
    op = SymTriOp(A, "L")
    p = min(PREFIX, n)
    A64 = A[:p].double()
    lines = []
    for k in (1, 4, 8):
        X = torch.rand(n, k, device=dev, generator=torch.Generator(device=dev).manual_seed(k)) + 0.5
        if a.workgroups is None:
            tri = lambda: op.matmul(X)                                   # noqa: E731
        else:
            tri = lambda: symm.symm_tri(A, X, uplo="L", workgroups=a.workgroups)   # noqa: E731
        if k == 1:
            full, full_name = (lambda: normal_eq.gemv(A, X)), "gemv_rows_full"
        else:
            full, full_name = (lambda: A @ X), "matmul_full"
        paths = {"symm_tri": tri, full_name: full}
        ref = A64 @ X.double()
        scale = A64.abs() @ X.double().abs()
        errs = {nm: float(((f()[:p].double() - ref).abs() / scale).max()) for nm, f in paths.items()}   # warm-up too
        torch.cuda.synchronize()
        times = {nm: [] for nm in paths}
        for _ in range(a.reps):                 # alternating, one event pair per call
            for nm, f in paths.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                times[nm].append(e0.elapsed_time(e1))
        tri_bytes = 4.0 * n * (n + 1) / 2
        med = {nm: statistics.median(t) for nm, t in times.items()}
        for nm in paths:
            lines.append({"path": nm, "n": n, "k": k, "reps": a.reps, "ms_median": round(med[nm], 4),
                          "ms_min": round(min(times[nm]), 4), "ms_max": round(max(times[nm]), 4),
                          "triangle_TB_per_s": round(tri_bytes / med[nm] / 1e9, 3),
                          "read_TB_per_s": round((tri_bytes if nm == "symm_tri" else 4.0 * n * n) / med[nm] / 1e9, 3),
                          "err_vs_fp64_prefix": errs[nm], "prefix_rows": p, "workgroups": a.workgroups,
                          "device": torch.cuda.get_device_name(0)})
        lines.append({"summary": f"symm_tri / {full_name}", "k": k, "time_ratio": round(med["symm_tri"] / med[full_name], 3)})
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
