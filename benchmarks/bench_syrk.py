"""Z^T Z of f32 random features (config 4: 1e6 x 4096) two ways, in one
process and alternating: the split Gram of ``ml/krr.py`` (``_gram_split``,
two full hipBLASLt products per 8192-row chunk) and ``Herk`` with an f64 C
(``syrk_split.hip``: the lower triangle only, one f32 accumulator per tile and
chunk, f64 slabs).  Each is timed with device events around whole calls after
a warm-up call; both paths' error against the fp64 Gram of a 16384-row prefix
is reported with it.  One JSON line per path, then a summary line.

    python benchmarks/bench_syrk.py [--n 1000000] [--s 4096] [--reps 5] [--out FILE]
                                     [--chunk-rows R] [--workgroups G]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libskylark_amd.base import Herk  # noqa: E402
from libskylark_amd.ml import krr as K  # noqa: E402
from libskylark_amd.ops import _lib, syrk  # noqa: E402

PREFIX = 16384


def features(n, s, dev):
    """cos features scaled as the random Fourier map scales them, in row blocks
    (no second n x s temporary)."""
    g = torch.Generator(device=dev).manual_seed(4)
    Z = torch.empty(n, s, device=dev)
    for r0 in range(0, n, 65536):
        blk = Z[r0:r0 + 65536]
        blk.normal_(generator=g)
        blk.mul_(3.0).cos_().mul_((2.0 / s) ** 0.5)
    return Z


def err(G, ref):
    d = torch.sqrt(torch.diagonal(ref))
    e = (torch.tril(G.double()) - torch.tril(ref)).abs() / (d[:, None] * d[None, :])
    return float(e.max())


def run_split(Z):
    G = torch.zeros(Z.shape[1], Z.shape[1], dtype=torch.float64, device=Z.device)
    K._gram_split(Z, G)
    return G


KNOBS = {}      # --chunk-rows / --workgroups: the kernel's knobs, through ops.syrk directly


def run_herk(Z):
    G = torch.zeros(Z.shape[1], Z.shape[1], dtype=torch.float64, device=Z.device)
    if KNOBS:
        return syrk.syrk_split(Z, G, trans=True, uplo="L", **KNOBS)
    return Herk("L", "T", 1.0, Z, 0.0, G)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--s", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--chunk-rows", type=int, default=None)
    ap.add_argument("--workgroups", type=int, default=None)
    a = ap.parse_args(argv)
    if a.chunk_rows is not None:
        KNOBS["chunk_rows"] = a.chunk_rows
    if a.workgroups is not None:
        KNOBS["workgroups"] = a.workgroups
    if not torch.cuda.is_available():
        raise SystemExit("bench_syrk: needs the GPU")
    _lib.require()
    dev = torch.device("cuda:0")
    Z = features(a.n, a.s, dev)
    paths = {"gram_split": run_split, "herk_syrk_split": run_herk}
    pre = Z[:min(PREFIX, a.n)]
    ref = pre.double().t() @ pre.double()
    errs = {k: err(f(pre), ref) for k, f in paths.items()}
    del ref
    times = {k: [] for k in paths}
    for k, f in paths.items():          # warm-up: code objects, hipBLASLt's algorithm choice, the allocator
        f(Z)
    torch.cuda.synchronize()
    for _ in range(a.reps):             # alternating, one event pair per call
        for k, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f(Z)
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    # flops each path issues to the matrix cores: six plane products of the
    # full square, or of the lower triangle's 256 x 256 tiles
    nt = -(-a.s // 256)
    flops = {"gram_split": 12.0 * a.n * a.s * a.s, "herk_syrk_split": 12.0 * a.n * 65536.0 * (nt * (nt + 1) // 2)}
    lines = []
    for k in paths:
        med = statistics.median(times[k])
        lines.append({"path": k, "n": a.n, "s": a.s, "reps": a.reps, "ms_median": round(med, 3),
                      "ms_min": round(min(times[k]), 3), "ms_max": round(max(times[k]), 3),
                      "issued_PF": round(flops[k] / med / 1e12, 3), "err_vs_fp64_prefix": errs[k],
                      "prefix_rows": int(pre.shape[0]), "knobs": dict(KNOBS), "device": torch.cuda.get_device_name(0)})
    ms = {ln["path"]: ln["ms_median"] for ln in lines}
    lines.append({"summary": "herk_syrk_split / gram_split", "time_ratio": round(ms["herk_syrk_split"] / ms["gram_split"], 3),
                  "err_ratio": errs["herk_syrk_split"] / errs["gram_split"]})
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
