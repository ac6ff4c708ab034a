"""Duplicate groups of a whole library (blissgpu_duplicate_groups_device: dup_init_kernel + dup_join_kernel +
dup_flatten_kernel, d = 23) against the k-nearest self-search with k = 1 (blissgpu_knn_device, every song skipping itself) on
the same matrix, timed in the same process, alternating, medians of `reps` after one warm-up of each.  Per case: wall time of
both and the HIP-event kernel times from the context profiler.  Cases: n in --ns, euclidean / cosine / Mahalanobis with the
diagonal feature_weights(2) / Mahalanobis with a full SPD matrix, and three duplicate rates -- none (0.5 N(0, 1) rows), 1 %
(chains of 6 planted as in tests/test_gpu_duplicates.py, every 100th row), and all rows identical (--identical rows, the
contention case of the union-find; without the k-nearest figure).  Writes one JSON file.

    python tests/tools/duplicates_bench.py [--ns 100000,1000000] [--reps 3] [--out profiles/duplicates_bench.json]
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
THR = 0.05


def rows(rng, n, d, rate):
    X = (0.5 * rng.standard_normal((n, d))).astype(np.float32)
    n_chains = int(n * rate) // 6
    if n_chains:
        chains = rng.choice(n, n_chains * 6, replace=False).reshape(n_chains, 6)
        U = rng.standard_normal((n_chains, d))
        U /= np.linalg.norm(U, axis=1, keepdims=True)
        base = X[chains[:, 0]].astype(np.float64)
        for t in range(6):
            X[chains[:, t]] = (base + t * 0.8 * THR * U).astype(np.float32)
    return X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--metrics", default="euclidean,cosine,weights,spd")
    ap.add_argument("--identical", type=int, default=20_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "duplicates_bench.json"))
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    d = 23
    A = np.random.default_rng(7).standard_normal((d, d)) * 0.3
    weights = np.zeros((d, d), np.float32)
    np.fill_diagonal(weights, [0.25] + [1.0] * 9 + [3.0 / 13.0] * 13)  # FeaturesVersion::feature_weights, Version2
    mats = {"euclidean": ("euclidean", None), "cosine": ("cosine", None),
            "weights": ("mahalanobis", torch.from_numpy(weights).cuda()),
            "spd": ("mahalanobis", torch.from_numpy((A @ A.T + 0.1 * np.eye(d)).astype(np.float32)).cuda())}
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

    def kernels(f, prefix):
        sync()
        ctx.profile_enable(True)
        ctx.profile_reset()
        f()
        sync()
        prof = ctx.profile()
        ctx.profile_enable(False)
        return {k: round(v[0], 3) for k, v in prof.items() if k.startswith(prefix)}

    out = {"d": d, "threshold": THR, "reps": args.reps, "device": torch.cuda.get_device_name(0), "cases": []}

    def case(tX, name, rate, with_knn):
        n = tX.shape[0]
        metric, tM = mats[name]
        me = torch.arange(n, dtype=torch.int32, device="cuda")
        res = {}
        join = lambda: res.__setitem__("n_pairs", ctx.duplicate_labels(tX, None, metric, tM, THR)[1])  # noqa: E731
        knn = lambda: ctx.knn(tX, tX, 1, metric, tM, me)  # noqa: E731
        timed(join)
        t_join, t_knn = [], []
        if with_knn:
            timed(knn)
        for _ in range(args.reps):
            t_join.append(timed(join))
            if with_knn:
                t_knn.append(timed(knn))
        row = {"n": n, "metric": name, "duplicates": rate, "n_pairs": int(res["n_pairs"].item()),
               "join_wall_ms": round(statistics.median(t_join) * 1e3, 2), "join_kernels_ms": kernels(join, "dup_")}
        if with_knn:
            row["knn_k1_wall_ms"] = round(statistics.median(t_knn) * 1e3, 2)
            row["knn_k1_kernels_ms"] = kernels(knn, "knn_")
            row["join_over_knn"] = round(row["join_wall_ms"] / row["knn_k1_wall_ms"], 3)
        print(json.dumps(row), flush=True)
        out["cases"].append(row)

    for n in [int(v) for v in args.ns.split(",")]:
        for rate in (0.0, 0.01):
            tX = torch.from_numpy(rows(np.random.default_rng(1), n, d, rate)).cuda()
            for name in args.metrics.split(","):
                case(tX, name, rate, True)
    if args.identical:
        one = (0.5 * np.random.default_rng(6).standard_normal((1, d))).astype(np.float32)
        tX = torch.from_numpy(np.tile(one, (args.identical, 1))).cuda()
        for name in args.metrics.split(","):
            case(tX, name, "all identical", False)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
