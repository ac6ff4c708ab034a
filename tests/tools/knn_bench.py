"""k nearest songs of every song of a 10^5-song library (d = 23, queries = candidates, self skipped): the fused search
(blissgpu_knn_device: knn_scan_kernel + knn_merge_kernel) against the route that gives the same answer without it -- row
slabs of 4096 queries through Context.pairwise (A != B form) into one reused buffer and torch.topk(k, largest=False) per
slab -- timed in the same process, alternating, medians of `reps` after one warm-up of each.  k in {1, 32, 1024}, euclidean /
cosine / Mahalanobis with the diagonal feature_weights(2) / Mahalanobis with a full SPD matrix.  Per case: wall time of both,
HIP-event kernel times from the context profiler (the route's pairwise_kernel time alone is the floor of ANY route on those
kernels, not the route itself), and the device-memory high-water of both (how far torch.cuda.mem_get_info fell over the
warm-up call, where the library's grow-only workspace and torch's cache grow, and over a later call; torch's own peak; the
search's workspace q * k * 8 bytes as computed -- the route's 4096 x n buffer is allocated up front: route_buffer_mib).
A skinny shape (q = 16) runs against 16 calls of Context.closest_to_songs.  Writes one JSON file.

    python tests/tools/knn_bench.py [--n 100000] [--reps 3] [--ks 1,32,1024] [--out profiles/knn_bench_100k.json]
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
SLAB = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ks", default="1,32,1024")
    ap.add_argument("--metrics", default="euclidean,cosine,weights,spd")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bench_100k.json"))
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    n, d = args.n, 23
    rng = np.random.default_rng(1)
    tX = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).cuda()
    A = np.random.default_rng(7).standard_normal((d, d)) * 0.3
    weights = np.zeros((d, d), np.float32)
    np.fill_diagonal(weights, [0.25] + [1.0] * 9 + [3.0 / 13.0] * 13)  # FeaturesVersion::feature_weights, Version2
    mats = {"euclidean": ("euclidean", None), "cosine": ("cosine", None),
            "weights": ("mahalanobis", torch.from_numpy(weights).cuda()),
            "spd": ("mahalanobis", torch.from_numpy((A @ A.T + 0.1 * np.eye(d)).astype(np.float32)).cuda())}
    ctx = bliss.Context(0)
    me = torch.arange(n, dtype=torch.int32, device="cuda")
    buf = torch.empty((SLAB, n), dtype=torch.float32, device="cuda")

    def sync():
        ctx.synchronize()
        torch.cuda.synchronize()

    def timed(f):
        sync()
        t0 = time.perf_counter()
        f()
        sync()
        return time.perf_counter() - t0

    def measured(f, prefixes):
        """one profiled run: kernel ms by name prefix, and how far the device's free memory fell while it ran"""
        sync()
        torch.cuda.reset_peak_memory_stats()
        base, free0 = torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0]
        ctx.profile_enable(True)
        ctx.profile_reset()
        f()
        sync()
        prof = ctx.profile()
        ctx.profile_enable(False)
        free1 = torch.cuda.mem_get_info()[0]
        return ({k: round(v[0], 3) for k, v in prof.items() if k.startswith(prefixes)},
                {"free_memory_fell_mib": round((free0 - free1) / 2**20, 1),
                 "torch_peak_above_start_mib": round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)})

    out = {"n": n, "q": n, "d": d, "reps": args.reps, "slab_rows": SLAB, "device": torch.cuda.get_device_name(0),
           "route_buffer_mib": round(buf.numel() * 4 / 2**20, 1), "cases": [], "skinny": []}
    for name in args.metrics.split(","):
        metric, tM = mats[name]
        for k in [int(v) for v in args.ks.split(",")]:
            knn = lambda: ctx.knn(tX, tX, k, metric, tM, me)  # noqa: E731

            def route():
                idx = torch.empty((n, k), dtype=torch.int64, device="cuda")
                for r0 in range(0, n, SLAB):
                    rows = min(SLAB, n - r0)
                    o = ctx.pairwise(tX[r0:r0 + rows], tX, metric, tM, out=buf[:rows])
                    ar = torch.arange(rows, device="cuda")
                    o[ar, ar + r0] = float("inf")
                    idx[r0:r0 + rows] = torch.topk(o, k, dim=1, largest=False).indices
                return idx

            # the warm-up calls are where the library's grow-only workspace and torch's cache grow: their high-water
            sync()
            free0 = torch.cuda.mem_get_info()[0]
            timed(knn)
            free1 = torch.cuda.mem_get_info()[0]
            timed(route)
            free2 = torch.cuda.mem_get_info()[0]
            t_knn, t_route = [], []
            for _ in range(args.reps):
                t_knn.append(timed(knn))
                t_route.append(timed(route))
            k_ms, k_mem = measured(knn, ("knn_",))
            r_ms, r_mem = measured(route, ("pairwise",))
            row = {"metric": name, "k": k, "knn_wall_ms": round(statistics.median(t_knn) * 1e3, 2),
                   "route_wall_ms": round(statistics.median(t_route) * 1e3, 2), "knn_kernels_ms": k_ms,
                   "route_pairwise_kernel_ms": r_ms, "knn_memory": k_mem, "route_memory": r_mem,
                   "knn_warmup_free_memory_fell_mib": round((free0 - free1) / 2**20, 1),
                   "route_warmup_free_memory_fell_mib": round((free1 - free2) / 2**20, 1),
                   "knn_workspace_mib": round(n * k * 8 / 2**20, 1), "knn_outputs_mib": round(n * k * 8 / 2**20, 1)}
            print(json.dumps(row), flush=True)
            out["cases"].append(row)
    # a few queries against the whole library: one call, many workgroups per query, against one closest_to_songs call per query
    q = 16
    tQ = tX[:q].contiguous()
    pools = [torch.cat([tX[:i], tX[i + 1:]]) for i in range(q)]  # the library without song i, built outside the timing
    for name in args.metrics.split(","):
        metric, tM = mats[name]
        k = 32
        knn = lambda: ctx.knn(tQ, tX, k, metric, tM, me[:q].contiguous())  # noqa: E731

        def per_song():
            for i in range(q):
                ctx.closest_to_songs(tQ[i], pools[i], metric, tM)

        timed(knn)
        timed(per_song)
        t_knn, t_old = [], []
        for _ in range(args.reps):
            t_knn.append(timed(knn))
            t_old.append(timed(per_song))
        row = {"metric": name, "q": q, "k": k, "knn_wall_ms": round(statistics.median(t_knn) * 1e3, 3),
               "closest_to_songs_x16_wall_ms": round(statistics.median(t_old) * 1e3, 3), "knn_kernels_ms": measured(knn, ("knn_",))[0]}
        print(json.dumps(row), flush=True)
        out["skinny"].append(row)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
