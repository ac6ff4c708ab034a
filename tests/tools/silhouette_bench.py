"""The silhouette of a clustering on the device (blissgpu_silhouette_device) against what a user had before it: torch on the
same GPU -- row blocks of torch.cdist in f32, accumulated per cluster in f64 with index_add_, then a, b and s in f64.  Same
process, alternating, medians of `reps` after one warm-up of each.  Data: a seeded 32-component Gaussian mixture, d = 23, labels
= the nearest of K = 32 sampled centres (blissgpu_kmeans_device, max_iter = 0), euclidean; n in {10^4, 10^5}.  Per n: the wall
time of the call with the plan's column groups (col_groups = 0) and with one (col_groups = 1), silhouette_scan_kernel's HIP-event
time from the context profiler for both, the pairs per second it reaches, and beside it knn_scan_kernel's at the same n
(blissgpu_knn_device, k = 32, the rows against themselves as in tests/tools/knn_bench.py: the same per-pair arithmetic without
the root and the f64 add).  torch's sums are not the contract's (cdist is not the all-pairs kernel's distance, index_add_ has no
order), so only times are compared; max |s - s_torch| is recorded as a sanity check.  `--sweep` records the scan kernel's time
at forced column-group counts as well (what the plan's choice is judged by).  Writes one JSON file.

    python tests/tools/silhouette_bench.py [--ns 10000,100000] [--k 32] [--reps 3] [--sweep 2,4,8,16,32] [--out profiles/silhouette_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def mixture(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((32, d)).astype(np.float32)
    return (centres[rng.integers(0, 32, n)] + np.float32(0.5) * rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="10000,100000")
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--block", type=int, default=8192, help="rows per torch.cdist block of the baseline")
    ap.add_argument("--sweep", default="2,4,8,16,32", help="forced column-group counts whose scan kernel time is recorded too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "silhouette_bench.json"))
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    assert torch.cuda.is_available(), "silhouette_bench measures on the GPU: there is no CPU path"
    d, K = 23, args.k
    ctx = bliss.Context(0)

    def sync():
        ctx.synchronize()
        torch.cuda.synchronize()

    def timed(f):
        sync()
        t0 = time.perf_counter()
        r = f()
        sync()
        return time.perf_counter() - t0, r

    def profiled(f):
        sync()
        ctx.profile_enable(True)
        ctx.profile_reset()
        f()
        sync()
        prof = ctx.profile()
        ctx.profile_enable(False)
        return prof

    out = {"d": d, "K": K, "reps": args.reps, "device": torch.cuda.get_device_name(0), "cases": []}
    for n in (int(v) for v in args.ns.split(",")):
        Xh = mixture(n, d, 1)
        X = torch.from_numpy(Xh).cuda()
        C0 = torch.from_numpy(bliss.playlist.kmeans_init(Xh, K, 0, "sample")).cuda()
        labels = ctx.kmeans(X, C0, 0)[0]
        lab64 = labels.to(torch.int64)
        sizes = torch.bincount(lab64, minlength=K).to(torch.float64)

        def new(cg):
            return ctx.silhouette(X, labels, "euclidean", None, None, cg, K)

        def baseline():
            S = torch.zeros((K, n), dtype=torch.float64, device=X.device)  # S[c, i] = the distances of song i to cluster c
            for j0 in range(0, n, args.block):
                D = torch.cdist(X[j0:j0 + args.block], X)  # (torch's default: the matrix-multiply form, its fastest)
                S.index_add_(0, lab64[j0:j0 + args.block], D.to(torch.float64))
            own = sizes[lab64]
            a = S[lab64, torch.arange(n, device=X.device)] / (own - 1).clamp(min=1)
            Q = S / sizes[:, None]
            Q[lab64, torch.arange(n, device=X.device)] = float("inf")
            Q[sizes == 0] = float("inf")
            b = Q.min(dim=0).values
            return torch.where(own == 1, torch.zeros_like(a), (b - a) / torch.maximum(a, b))

        def knn():
            return ctx.knn(X, X, 32, "euclidean", None, torch.arange(n, dtype=torch.int32, device=X.device))

        new(0), new(1), baseline(), knn()  # warm-up of everything timed (workspace growth, code objects)
        t0, t1, tb = [], [], []
        for _ in range(args.reps):
            t0.append(timed(lambda: new(0))[0])
            t1.append(timed(lambda: new(1))[0])
            tb.append(timed(baseline)[0])
        s_new, s_ref = new(0)[0].to(torch.float64), baseline()
        p0, p1, pk = profiled(lambda: new(0)), profiled(lambda: new(1)), profiled(knn)
        sweep = {cg: round(profiled(lambda: new(cg))["silhouette_scan_kernel"][0], 4) for cg in (int(v) for v in args.sweep.split(",") if v)}
        pairs = n * n
        scan0, scan1, kscan = p0["silhouette_scan_kernel"][0], p1["silhouette_scan_kernel"][0], pk["knn_scan_kernel"][0]
        case = {
            "n": n, "K": K, "non_empty_clusters": int((sizes > 0).sum().item()), "largest_cluster": int(sizes.max().item()),
            "wall_ms_plan": round(1e3 * statistics.median(t0), 3), "wall_ms_col_groups_1": round(1e3 * statistics.median(t1), 3),
            "wall_ms_torch": round(1e3 * statistics.median(tb), 3),
            "wall_ms_plan_all": [round(1e3 * t, 3) for t in t0], "wall_ms_col_groups_1_all": [round(1e3 * t, 3) for t in t1],
            "wall_ms_torch_all": [round(1e3 * t, 3) for t in tb],
            "silhouette_scan_kernel_ms_plan": round(scan0, 4), "silhouette_scan_kernel_ms_col_groups_1": round(scan1, 4),
            "silhouette_scan_gpairs_per_s_plan": round(pairs / scan0 / 1e6, 2),
            "knn_scan_kernel_ms": round(kscan, 4), "knn_scan_gpairs_per_s": round(pairs / kscan / 1e6, 2),
            "silhouette_scan_kernel_ms_by_col_groups": sweep,
            "kernel_ms_plan": {k: [round(v[0], 4), int(v[1])] for k, v in p0.items()},
            "max_abs_s_minus_torch": float((s_new - s_ref).abs().max().item()),
        }
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
        del X
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
