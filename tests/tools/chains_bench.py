"""Song-to-song chains cut after k over a 10^5-song library (d = 23, euclidean, k = 20, one-seed groups that skip their own
row, device forms), timed in one process, the variants alternating, medians of `reps` after one warm-up of each:

  1. one seed: Context.chains against the only other way to that playlist, Context.song_to_song over the whole pool;
  2. G = n/64, n/16, n/4 and n chains: the steps route against the lists route (both forced), and what `auto` picks;
  3. G = n: the lists route against its two searches timed alone -- Context.knn with k = L and Context.group_knn with k = 1 --
     and the kernel times of the route from the context profiler (chain_walk_kernel's own time among them).

The constant c of blissgpu_chains_plan (LISTS when c n < (k - 1) G) is read off (2): lists / steps = c n / ((k - 1) G), so each
size gives c = (lists ms / steps ms) (k - 1) G / n.  Writes one JSON file.

    python tests/tools/chains_bench.py [--n 100000] [--reps 3] [--out profiles/chains_bench_100k.json]
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
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chains_bench_100k.json"))
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    n, d, k = args.n, 23, args.k
    rng = np.random.default_rng(1)
    tX = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).cuda()
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

    def medians(fs):
        """fs: {name: callable} -> {name: median ms}, the callables alternating"""
        for f in fs.values():
            timed(f)
        t = {name: [] for name in fs}
        for _ in range(args.reps):
            for name, f in fs.items():
                t[name].append(timed(f))
        return {name: round(statistics.median(v) * 1e3, 3) for name, v in t.items()}, \
               {name: round((max(v) - min(v)) * 1e3, 3) for name, v in t.items()}

    def kernels(f):
        sync()
        ctx.profile_enable(True)
        ctx.profile_reset()
        f()
        sync()
        prof = ctx.profile()
        ctx.profile_enable(False)
        return {name: round(v[0], 3) for name, v in prof.items() if name.startswith(("chain_", "knn_", "group_knn_")) and v[0] > 0}

    def chains_of(G):
        rows = torch.from_numpy(np.sort(rng.choice(n, G, replace=False))).cuda()
        tS, skip, off = tX[rows].contiguous(), rows.to(torch.int32), np.arange(G + 1, dtype=np.int64)
        return tS, skip, off

    out = {"n": n, "d": d, "k": k, "metric": "euclidean", "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    # 1. one playlist
    tS, skip, off = chains_of(1)
    med, spread = medians({"chains_ms": lambda: ctx.chains(tS, off, tX, k, skip=skip),
                           "song_to_song_whole_pool_ms": lambda: ctx.song_to_song(tS, tX)})
    out["one_seed"] = dict(med, spread_ms=spread)
    print(json.dumps(out["one_seed"]), flush=True)
    # 2. steps against lists
    out["routes"] = []
    for G in (n // 64, n // 16, n // 4, n):
        tS, skip, off = chains_of(G)
        call = lambda route: (lambda: ctx.chains(tS, off, tX, k, skip=skip, route=route))  # noqa: E731
        med, spread = medians({"steps_ms": call("steps"), "lists_ms": call("lists"), "auto_ms": call("auto")})
        row = dict(med, groups=G, spread_ms=spread,
                   c=round(med["lists_ms"] / med["steps_ms"] * (k - 1) * G / n, 3))
        print(json.dumps(row), flush=True)
        out["routes"].append(row)
    # 3. the lists route against its parts (G = n: tS, skip, off are the last of the loop)
    med, spread = medians({"lists_ms": lambda: ctx.chains(tS, off, tX, k, skip=skip, route="lists"),
                           "knn_k_eq_L_ms": lambda: ctx.knn(tX, tX, k, skip=me),
                           "group_knn_k_eq_1_ms": lambda: ctx.group_knn(tS, off, tX, 1, skip=skip)})
    out["lists_parts"] = dict(med, spread_ms=spread, list_len=k,
                              kernels_ms=kernels(lambda: ctx.chains(tS, off, tX, k, skip=skip, route="lists")),
                              steps_kernels_ms=kernels(lambda: ctx.chains(tS, off, tX, k, skip=skip, route="steps")))
    print(json.dumps(out["lists_parts"]), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
