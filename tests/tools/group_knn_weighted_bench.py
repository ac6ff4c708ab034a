"""A k-song VARIANCE-WEIGHTED playlist for every group of a 10^5-song library (d = 23, k = 32, members skipped): the one-call
search with derived weights (blissgpu_group_knn_weighted_device: group_weights_kernel + the per-group form of
group_knn_scan_kernel + group_knn_merge_kernel) against what answers the same question without it -- per group, the host
arithmetic of playlist.variance_based_weight_matrix, the upload of that matrix and one Context.closest_to_songs (a full sort of
n) -- and against the euclidean blissgpu_group_knn_device call on the same groups, timed in the same process, alternating,
medians of `reps` after one warm-up of each.  The partition into groups is tests/tools/group_knn_bench.py's: geometrically
distributed sizes with mean about 10, plus one group of 20 000 songs; a group of one song takes the identity in the one call
and euclidean in the route.  The route is given the WHOLE library as the pool of every group, so its time is a lower bound.
Also reported: the kernel times of both one-call searches from the context profiler.  Writes one JSON file.

    python tests/tools/group_knn_weighted_bench.py [--n 100000] [--reps 3] [--out profiles/group_knn_weighted_bench_100k.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_knn_weighted_bench_100k.json"))
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    n, d, k = args.n, 23, args.k
    rng = np.random.default_rng(1)
    X = rng.standard_normal((n, d)).astype(np.float32)
    tX = torch.from_numpy(X).cuda()
    # a partition of the library: one big group, the rest in groups of geometric size
    sizes = [min(args.big, n)]
    while sum(sizes) < n:
        sizes.append(min(int(rng.geometric(1.0 / args.mean)), n - sum(sizes)))
    sizes = rng.permutation(np.asarray(sizes, np.int64))
    off = np.zeros(sizes.shape[0] + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    members = rng.permutation(n)
    t_members = torch.from_numpy(members).cuda()
    S = X[members]
    tS = tX[t_members].contiguous()
    skip = t_members.to(torch.int32)
    G = sizes.shape[0]
    ctx = bliss.Context(0)

    def sync():
        ctx.synchronize()
        torch.cuda.synchronize()

    def timed(f):
        sync()
        t0 = time.perf_counter()
        f()
        sync()
        return time.perf_counter() - t0

    def kernels(f):
        sync()
        ctx.profile_enable(True)
        ctx.profile_reset()
        f()
        sync()
        prof = ctx.profile()
        ctx.profile_enable(False)
        return {name: round(v[0], 3) for name, v in prof.items() if name.startswith("group_")}

    weighted = lambda: ctx.group_knn(tS, off, tX, k, skip=skip, weights="variance")  # noqa: E731
    euclidean = lambda: ctx.group_knn(tS, off, tX, k, "euclidean", None, skip)  # noqa: E731
    host_s = [0.0]

    def route():  # what the library offers without the one call: host weights, upload, one full sort per group
        host_s[0] = 0.0
        for g in range(G):
            a, b = int(off[g]), int(off[g + 1])
            if b - a < 2:
                ctx.closest_to_songs(tS[a:b], tX, "euclidean", None)
                continue
            t0 = time.perf_counter()
            M = bliss.playlist.variance_based_weight_matrix(list(S[a:b]))
            host_s[0] += time.perf_counter() - t0
            ctx.closest_to_songs(tS[a:b], tX, "mahalanobis", torch.from_numpy(M).cuda())

    for f in (weighted, route, euclidean):
        timed(f)
    t_w, t_r, t_e, t_h = [], [], [], []
    for _ in range(args.reps):
        t_w.append(timed(weighted))
        t_r.append(timed(route))
        t_h.append(host_s[0])
        t_e.append(timed(euclidean))
    ms = lambda t: round(statistics.median(t) * 1e3, 2)  # noqa: E731
    out = {"n": n, "d": d, "k": k, "groups": int(G), "groups_under_two_seeds": int((sizes < 2).sum()),
           "largest_group": int(sizes.max()), "mean_group": round(float(sizes.mean()), 2), "seeds": int(off[-1]),
           "pairs": int(off[-1]) * n, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "group_knn_weighted_wall_ms": ms(t_w), "route_wall_ms": ms(t_r), "route_host_weights_ms": ms(t_h),
           "group_knn_euclidean_wall_ms": ms(t_e), "group_knn_weighted_kernels_ms": kernels(weighted),
           "group_knn_euclidean_kernels_ms": kernels(euclidean)}
    print(json.dumps(out), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
