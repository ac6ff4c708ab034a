"""A k-song playlist for every group of a 10^5-song library (d = 23, k = 32, members skipped): the one-call search
(blissgpu_group_knn_device: group_knn_scan_kernel + group_knn_merge_kernel) against the route that answers the same question
without it -- one Context.closest_to_songs per group -- timed in the same process, alternating, medians of `reps` after one
warm-up of each.  The groups partition the library: geometrically distributed sizes with mean about 10, plus one group of
20 000 songs.  The route is given the WHOLE library as the pool of every group (building each group's pool without its
members would cost it a 9 MB gather per group more), so its time is a lower bound of the parent route's.  Also reported:
knn_scan_kernel + knn_merge_kernel at q = n, which evaluate the same number of pairs (n^2) without the per-pair root and with
one row per query, and the kernel times of the one-call search from the context profiler.  Writes one JSON file.

    python tests/tools/group_knn_bench.py [--n 100000] [--reps 3] [--out profiles/group_knn_bench_100k.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--big", type=int, default=20_000)
    ap.add_argument("--mean", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--metrics", default="euclidean,cosine,weights")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_knn_bench_100k.json"))
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    n, d, k = args.n, 23, args.k
    rng = np.random.default_rng(1)
    tX = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).cuda()
    weights = np.zeros((d, d), np.float32)
    np.fill_diagonal(weights, [0.25] + [1.0] * 9 + [3.0 / 13.0] * 13)  # FeaturesVersion::feature_weights, Version2
    mats = {"euclidean": ("euclidean", None), "cosine": ("cosine", None), "weights": ("mahalanobis", torch.from_numpy(weights).cuda())}
    # a partition of the library: one big group, the rest in groups of geometric size
    sizes = [min(args.big, n)]
    while sum(sizes) < n:
        sizes.append(min(int(rng.geometric(1.0 / args.mean)), n - sum(sizes)))
    sizes = rng.permutation(np.asarray(sizes, np.int64))
    off = np.zeros(sizes.shape[0] + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    members = rng.permutation(n)
    t_members = torch.from_numpy(members).cuda()
    tS = tX[t_members].contiguous()
    skip = t_members.to(torch.int32)
    G = sizes.shape[0]
    ctx = bliss.Context(0)
    me = torch.arange(n, dtype=torch.int32, device="cuda")

    def sync():
        ctx.synchronize()
        torch.cuda.synchronize()

    def timed(f):
        sync()
        t0 = time.perf_counter()
        f()
        sync()
        return time.perf_counter() - t0

    def kernels(f, prefix):
        sync()
        ctx.profile_enable(True)
        ctx.profile_reset()
        f()
        sync()
        prof = ctx.profile()
        ctx.profile_enable(False)
        return {name: round(v[0], 3) for name, v in prof.items() if name.startswith(prefix)}

    out = {"n": n, "d": d, "k": k, "groups": int(G), "largest_group": int(sizes.max()), "mean_group": round(float(sizes.mean()), 2),
           "seeds": int(off[-1]), "pairs": int(off[-1]) * n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "cases": []}
    for name in args.metrics.split(","):
        metric, tM = mats[name]
        one_call = lambda: ctx.group_knn(tS, off, tX, k, metric, tM, skip)  # noqa: E731
        knn = lambda: ctx.knn(tX, tX, k, metric, tM, me)  # noqa: E731

        def route():
            for g in range(G):
                ctx.closest_to_songs(tS[off[g]:off[g + 1]], tX, metric, tM)

        timed(one_call)
        timed(route)
        timed(knn)
        t_one, t_route, t_knn = [], [], []
        for _ in range(args.reps):
            t_one.append(timed(one_call))
            t_route.append(timed(route))
            t_knn.append(timed(knn))
        row = {"metric": name, "group_knn_wall_ms": round(statistics.median(t_one) * 1e3, 2),
               "route_wall_ms": round(statistics.median(t_route) * 1e3, 2), "knn_q_eq_n_wall_ms": round(statistics.median(t_knn) * 1e3, 2),
               "group_knn_kernels_ms": kernels(one_call, "group_knn_"), "knn_kernels_ms": kernels(knn, "knn_")}
        print(json.dumps(row), flush=True)
        out["cases"].append(row)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
