"""Playlist deduplication on 10^5 songs: the old host loop (one blissgpu_set_distance call + a stream synchronisation per
kept song, 64 distances per call, re-implemented here as it stood) against the single call blissgpu_dedup_playlist, and the
device-resident form; median of 3 each, plus the per-kernel times of dedup_next_kernel / dedup_walk_kernel from the context
profiler.  Two playlists: about 1 % planted duplicates, and every song a duplicate of the first.  Prints one JSON line.

    python tests/tools/dedup_bench.py [--n 100000] [--reps 3] [--skip-old]
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


def old_loop(P, X, thr=np.float32(0.05), window=64):
    """dedup_playlist_custom_distance before the dedup kernels (no title / artist keys: distances only)."""
    out, i, n = [], 0, X.shape[0]
    while i < n:
        j = i + 1
        while j < n:
            hi = min(n, j + window)
            dist = P.set_distances(X[i:i + 1], X[j:hi])
            stop = None
            for k in range(j, hi):
                if np.isnan(dist[k - j]):
                    raise ValueError("NaN distance")
                if not dist[k - j] < thr:
                    stop = k
                    break
            if stop is not None:
                j = stop
                break
            j = hi
        out.append(i)
        i = j
    return np.asarray(out, np.int64)


def median_time(fn, reps):
    ts, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-old", action="store_true")
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    P = bliss.playlist
    rng = np.random.default_rng(1)
    n, d = args.n, 23
    few = rng.standard_normal((n, d)).astype(np.float32)
    dup = rng.random(n) < 0.01
    dup[0] = False
    for k in np.nonzero(dup)[0]:  # a near copy of the song before it (0.001 * sqrt(23) < 0.05)
        few[k] = few[k - 1] + np.float32(0.001)
    alldup = np.repeat(few[:1], n, axis=0)
    playlists = {"1pct_duplicates": few, "all_duplicates": alldup}
    dctx = bliss.Context.default(0)  # the context of the host-pointer entry points
    ctx = bliss.Context(0)
    out = {"n": n, "d": d, "reps": args.reps, "device": torch.cuda.get_device_name(0), "playlists": {}}
    for name, X in playlists.items():
        P.dedup_order(X)  # warm-up: buffers, code objects
        t_new, kept = median_time(lambda: P.dedup_order(X), args.reps)
        row = {"kept": int(kept.shape[0]), "new_call_s": round(t_new, 6)}
        Xd = torch.from_numpy(X).cuda()
        ctx.dedup_playlist(Xd)
        ctx.synchronize()

        def dev():
            k, nk = ctx.dedup_playlist(Xd)
            ctx.synchronize()
            return int(nk.item())

        t_dev, nk = median_time(dev, args.reps)
        assert nk == kept.shape[0]
        row["device_form_s"] = round(t_dev, 6)
        for c, label in ((dctx, "host_form"), (ctx, "device_form")):
            c.profile_enable(True)
            c.profile_reset()
            if label == "host_form":
                P.dedup_order(X)
            else:
                dev()
            prof = c.profile()
            c.profile_enable(False)
            row[f"{label}_kernels_ms"] = {k: round(v[0], 4) for k, v in prof.items() if k.startswith("dedup_")}
        if not args.skip_old:
            t_old, kept_old = median_time(lambda: old_loop(P, X), args.reps)
            assert np.array_equal(kept_old, kept)
            row["old_loop_s"] = round(t_old, 4)
            row["speedup_vs_old"] = round(t_old / t_new, 1)
        out["playlists"][name] = row
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
