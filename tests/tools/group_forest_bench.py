"""Isolation-forest playlists for every album of a synthetic library in ONE call (blissgpu_group_forest_knn_device:
group_forest_scan_kernel + group_knn_merge_kernel, forests built on the host batch by batch while the device scores) against
the only way there was before it: a loop of playlist.Forest(S_g, options) + Context.forest_closest_to_songs per album.

Shapes: d = 23, album sizes drawn from 2..20 with a fixed seed, libraries of 10 000 and 100 000 songs (about 900 / 9 000 albums),
options (1000, 200, None, 10) and (100, 200, None, 10), k = 20, every album skipping its own songs.

Per point: wall times of the synchronised device form (median of `reps` after one warm-up), the HIP-event kernel times of one
profiled run, the host's build time and its wait for the device (blissgpu_debug_group_forest_stats), the fraction of the build
that was hidden behind the device, walks per second of the scan kernel, and the SHA-256 of (idx, score) for two runs.  The
baseline loop is timed on the first `--sample` albums and SCALED linearly to all of them (it builds the forest, scores and
sorts all n candidates and copies the first k indices back per album, and skips nothing: a lower bound of what the per-album
way costs).  Writes one JSON file.

    python tests/tools/group_forest_bench.py [--points 10000,100000] [--sample 200] [--out profiles/group_forest_bench.json]
"""
import argparse
import hashlib
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
    ap.add_argument("--points", default="10000,100000")
    ap.add_argument("--trees", default="1000,100")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_forest_bench.json"))
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    P = bliss.playlist
    d, k = 23, args.k
    out = {"d": d, "k": k, "reps": args.reps, "device": torch.cuda.get_device_name(0), "baseline": "scaled from the sample",
           "points": []}
    ctx = bliss.Context(0)
    for n in (int(v) for v in args.points.split(",")):
        rng = np.random.default_rng(1)
        sizes = []
        while sum(sizes) < n:
            sizes.append(int(rng.integers(2, 21)))
        sizes[-1] -= sum(sizes) - n
        if sizes[-1] < 2:  # (the last album absorbs the remainder)
            sizes[-2] += sizes.pop()
        A = len(sizes)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        X = rng.standard_normal((n, d)).astype(np.float32)
        rows = rng.permutation(n)  # album g's songs are the candidates rows[off[g]:off[g + 1]]
        S = np.ascontiguousarray(X[rows])
        tS, tX = torch.from_numpy(S).cuda(), torch.from_numpy(X).cuda()
        t_skip = torch.from_numpy(rows.astype(np.int32)).cuda()
        for trees in (int(v) for v in args.trees.split(",")):
            fo = P.ForestOptions(trees, 200, None, 10, seed=7)
            pt = {"n": n, "albums": A, "options": [trees, 200, None, 10]}

            def one_call():
                r = ctx.group_forest_knn(tS, off, tX, k, fo, skip=t_skip, seeds_host=S)
                ctx.synchronize()
                return r

            one_call()  # warm-up
            walls, hashes, stats = [], [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                idx, score, _ = one_call()
                walls.append(time.perf_counter() - t0)
                stats.append(ctx.group_forest_stats())
                hashes.append(hashlib.sha256(idx.cpu().numpy().tobytes() + score.cpu().numpy().tobytes()).hexdigest()[:16])
            pt["one_call_ms"] = round(statistics.median(walls) * 1e3, 2)
            pt["one_call_spread_ms"] = round((max(walls) - min(walls)) * 1e3, 2)
            pt["result_sha256"] = hashes[:2]
            assert len(set(hashes)) == 1, "two runs disagree"
            mid = sorted(range(args.reps), key=lambda i: walls[i])[args.reps // 2]
            build_ms, wait_ms, batches = stats[mid]
            ctx.profile_enable(True)
            ctx.profile_reset()
            one_call()
            prof = ctx.profile()
            ctx.profile_enable(False)
            ctx.profile_reset()
            scan_ms, merge_ms = prof["group_forest_scan_kernel"][0], prof["group_knn_merge_kernel"][0]
            device_ms = scan_ms + merge_ms
            wall_ms = walls[mid] * 1e3
            pt.update({"batches": batches, "host_build_ms": round(build_ms, 2), "host_wait_ms": round(wait_ms, 2),
                       "scan_kernel_ms": round(scan_ms, 2), "merge_kernel_ms": round(merge_ms, 2),
                       "host_build_ms_per_batch": round(build_ms / batches, 3), "device_ms_per_batch": round(device_ms / batches, 3),
                       # what a serial schedule would take beyond the wall time, as a share of the build
                       "build_hidden_fraction": round(max(0.0, min(1.0, (build_ms + device_ms - wall_ms) / build_ms)), 3),
                       "walks_per_s": round(float(A) * trees * n / (scan_ms * 1e-3), 0)})
            # the per-album loop on the first albums
            m = min(args.sample, A)

            def loop():
                for g in range(m):
                    f = P.Forest(S[off[g]:off[g + 1]], fo)
                    order = ctx.forest_closest_to_songs(f, tX)
                    ctx.synchronize()
                    order[:k].cpu()
                    f.close()

            loop()
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                loop()
                times.append(time.perf_counter() - t0)
            per_album = statistics.median(times) / m
            pt["loop_sample_albums"] = m
            pt["loop_ms_per_album"] = round(per_album * 1e3, 3)
            pt["loop_scaled_ms"] = round(per_album * A * 1e3, 1)
            pt["speedup"] = round(per_album * A * 1e3 / pt["one_call_ms"], 2)
            print(json.dumps(pt), flush=True)
            out["points"].append(pt)
    ctx.close()
    out["one_call_not_slower_at_every_point"] = all(p["speedup"] >= 1.0 for p in out["points"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    assert out["one_call_not_slower_at_every_point"], "the one-call form is slower than the per-album loop somewhere"


if __name__ == "__main__":
    main()
