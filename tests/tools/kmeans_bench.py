"""k-means of a song library on the device (blissgpu_kmeans_device) against the route a user had before it: per iteration
blissgpu_knn_device(queries = the n songs, candidates = the K centres, k = 1) for the labels and a torch scatter-mean
(index_add_ + bincount) for the centres -- same process, alternating, medians of `reps` after one warm-up of each.
Data: a seeded Gaussian mixture, d = 23; n in {10^5, 10^6}, K in {16, 256, 1024}; `iters` fixed iterations (the "sample"
initialisation; a run that converges earlier is reported with its n_iter and divided by it).  Per case: the wall time per
iteration of both, HIP-event kernel times per launch from the context profiler -- kmeans_assign_kernel and the parent's
knn_scan_kernel do the same n x K pair sums -- and the share of the sort (histogram, scan, scatter), the mean and the select in
the new call's kernel time.  The two routes do not give the same centres (torch's index_add_ does not add in row order), so only
times are compared here; the results are checked bit for bit in tests/test_gpu_kmeans.py.  Writes one JSON file.

    python tests/tools/kmeans_bench.py [--ns 100000,1000000] [--ks 16,256,1024] [--iters 20] [--reps 3] [--out profiles/kmeans_bench.json]
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
SORT_MEAN = ("kmeans_hist_kernel", "kmeans_scan_tiles_kernel", "kmeans_scan_add_kernel", "kmeans_scatter_kernel",
             "segment_mean_kernel", "kmeans_select_kernel")


def mixture(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((32, d)).astype(np.float32)
    return (centres[rng.integers(0, 32, n)] + np.float32(0.5) * rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="100000,1000000")
    ap.add_argument("--ks", default="16,256,1024")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_bench.json"))
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    assert torch.cuda.is_available(), "kmeans_bench measures on the GPU: there is no CPU path"
    d, iters = 23, args.iters
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

    out = {"d": d, "iters": iters, "reps": args.reps, "device": torch.cuda.get_device_name(0), "cases": []}
    for n in (int(v) for v in args.ns.split(",")):
        Xh = mixture(n, d, 1)
        X = torch.from_numpy(Xh).cuda()
        for K in (int(v) for v in args.ks.split(",")):
            C0 = torch.from_numpy(bliss.playlist.kmeans_init(Xh, K, 0, "sample")).cuda()

            def new():
                return ctx.kmeans(X, C0, iters)

            def route():
                C = C0.clone()
                for _ in range(iters + 1):  # the new call assigns iters + 1 times and updates iters times
                    idx, _dist = ctx.knn(X, C, 1)
                    labels = idx[:, 0].to(torch.int64)
                    sums = torch.zeros_like(C).index_add_(0, labels, X)
                    cnt = torch.bincount(labels, minlength=K)
                    C = torch.where(cnt[:, None] > 0, sums / cnt.clamp(min=1)[:, None].to(torch.float32), C)
                return C

            new(), route()  # warm-up of both (workspace growth, code objects)
            t_new, t_route, n_iter = [], [], None
            for _ in range(args.reps):
                dt, r = timed(new)
                t_new.append(dt)
                n_iter = r[4]
                t_route.append(timed(route)[0])
            p_new, p_route = profiled(new), profiled(route)
            steps = max(n_iter, 1)
            kern_ms = sum(v[0] for v in p_new.values())
            assign_ms, assign_launches = p_new["kmeans_assign_kernel"]
            scan_ms, scan_launches = p_route["knn_scan_kernel"]
            case = {
                "n": n, "K": K, "n_iter": n_iter, "converged": bool(r[5]),
                "new_wall_ms_per_iteration": round(1e3 * statistics.median(t_new) / steps, 4),
                "route_wall_ms_per_iteration": round(1e3 * statistics.median(t_route) / iters, 4),
                "new_wall_ms": [round(1e3 * t, 3) for t in t_new], "route_wall_ms": [round(1e3 * t, 3) for t in t_route],
                "kmeans_assign_kernel_ms_per_launch": round(assign_ms / assign_launches, 4),
                "knn_scan_kernel_ms_per_launch": round(scan_ms / scan_launches, 4),
                "knn_merge_kernel_ms_per_launch": round(p_route["knn_merge_kernel"][0] / p_route["knn_merge_kernel"][1], 4),
                "pairs_per_launch": n * K,
                "sort_mean_select_ms_per_iteration": round(sum(p_new[k][0] for k in SORT_MEAN if k in p_new) / steps, 4),
                "sort_mean_select_share_of_kernel_time": round(sum(p_new[k][0] for k in SORT_MEAN if k in p_new) / kern_ms, 4),
                "new_kernel_ms": {k: [round(v[0], 3), int(v[1])] for k, v in p_new.items()},
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
