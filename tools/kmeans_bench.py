"""k-means kernels on one GPU, one process: assignment time / TF/s for bf16 and fp32 features against the torch formula
the reference's ApplyKmeans runs on a GPU (fp32 matmul + argmin, dump_km_label.py:36-42), accumulation GB/s, and the
wall time of a MiniBatchKMeans fit with the recipe's flags (learn_kmeans.py) on random rows.

    python tools/kmeans_bench.py [--fit-rows 1000000] [--no-fit]
Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unispeech_amd import kmeans as KM  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fit-rows", type=int, default=1_000_000)
    ap.add_argument("--no-fit", action="store_true")
    a = ap.parse_args()
    D, K = 768, 500
    out = {"device": torch.cuda.get_device_name(0), "D": D, "K": K, "assign": [], "torch_formula": [], "accumulate": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    c = torch.randn(K, D, device="cuda", generator=g)
    C = KM.Centres(c)
    Ct, Cn = c.t().contiguous(), c.pow(2).sum(1)[None]
    for N in (23968, 1_000_000):
        x32 = torch.randn(N, D, device="cuda", generator=g)
        reps = 20 if N < 100000 else 5
        for name, x in (("bf16", x32.bfloat16()), ("fp32", x32)):
            ms = timed(lambda: KM.assign(x, C), reps)
            out["assign"].append({"N": N, "x": name, "ms": round(ms, 4), "tflops": round(2 * N * K * D / ms / 1e9, 1)})
            xf = x.float()

            def formula():
                return (xf.pow(2).sum(1, keepdim=True) - 2 * xf @ Ct + Cn).argmin(1)

            ms = timed(formula, reps)
            out["torch_formula"].append({"N": N, "x": name, "ms": round(ms, 4),
                                         "tflops": round(2 * N * K * D / ms / 1e9, 1)})
            lab = KM.assign(x, C)
            ms = timed(lambda: KM.accumulate(x, lab, K), reps)
            nbytes = N * D * x.element_size() + N * 4 * 4 + K * D * 4
            out["accumulate"].append({"N": N, "x": name, "ms": round(ms, 4), "GBps": round(nbytes / ms / 1e6, 1)})
        del x32
    if not a.no_fit:
        x = torch.randn(a.fit_rows, D, device="cuda", generator=g)
        torch.cuda.synchronize()
        t = time.perf_counter()
        km = KM.MiniBatchKMeans(n_clusters=K, init="k-means++", max_iter=100, batch_size=10000, tol=0.0,
                                max_no_improvement=100, n_init=20, reassignment_ratio=0.0, seed=0).fit(x)
        torch.cuda.synchronize()
        out["fit"] = {"rows": a.fit_rows, "s": round(time.perf_counter() - t, 2), "steps": km.n_steps_,
                      "inertia_per_row": km.inertia_ / a.fit_rows}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
