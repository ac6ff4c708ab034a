"""Album playlists for every album of a synthetic 10^5-song / 10^4-album library (d = 23, k = 20 albums, every album a seed
group that skips its own songs), timed in one process:

  1. blissgpu_album_knn through the host form (playlist.nearest_albums: uploads, the three launches, copies back);
  2. the same through the device form (Context.album_knn on device tensors), with the per-kernel split of the context profiler;
  3. library.album_playlists(db, k) once, end to end (one database read, the grouping, the one call, the Song lists);
  4. the per-album way: library.album_playlist_from(db, title, k) for a sample of the albums, extrapolated to all of them.

(1) and (2) are medians of `reps` after one warm-up; (4) is the mean of its sample times the number of albums.  Writes one JSON
file.

    python tests/tools/album_playlists_bench.py [--n 100000] [--albums 10000] [--sample 50] [--out profiles/album_playlists_bench.json]
"""
import argparse
import json
import os
import sqlite3
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def build_library(bliss, path, X, album_of, rng):
    """the tables of library.create_schema, filled in one transaction"""
    n, d = X.shape
    bliss.library.create_schema(path)
    conn = sqlite3.connect(path)
    version = int(bliss.FeaturesVersion.LATEST)
    track, disc = rng.integers(1, 15, n), rng.integers(1, 3, n)
    conn.executemany(
        "insert into song (id, path, artist, title, album, album_artist, track_number, disc_number, genre, duration, analyzed, "
        "version) values (?, ?, ?, ?, ?, ?, ?, ?, ?, ?, true, ?)",
        ((i + 1, f"/music/{i:06d}.flac", f"artist {album_of[i] % 997}", f"title {i}", f"album {album_of[i]:05d}", None, int(track[i]),
          int(disc[i]), None, 180.0, version) for i in range(n)))
    conn.executemany("insert into feature (song_id, feature, feature_index) values (?, ?, ?)",
                     ((i + 1, float(X[i, j]), j) for i in range(n) for j in range(d)))
    conn.commit()
    conn.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--albums", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "album_playlists_bench.json"))
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    n, A, k = args.n, args.albums, args.k
    d = bliss.FeaturesVersion.LATEST.feature_count()
    rng = np.random.default_rng(1)
    X = rng.standard_normal((n, d)).astype(np.float32)
    album_of = np.concatenate([np.arange(A), rng.integers(0, A, n - A)])[rng.permutation(n)]
    # every album a group of its own songs, in id order, each seed skipping its own row
    rows = np.argsort(album_of, kind="stable")
    off = np.zeros(A + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(album_of, minlength=A))
    S = np.ascontiguousarray(X[rows])
    out = {"n": n, "albums": A, "d": d, "k": k, "reps": args.reps, "device": torch.cuda.get_device_name(0)}

    def median_ms(f, reps):
        f()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
        return round(statistics.median(t) * 1e3, 3), round((max(t) - min(t)) * 1e3, 3)

    # 1. host form
    host = lambda: bliss.playlist.nearest_albums((S, off), X, album_of, k, skip=rows)  # noqa: E731
    out["host_form_ms"], out["host_form_spread_ms"] = median_ms(host, args.reps)
    print(json.dumps({"host_form_ms": out["host_form_ms"]}), flush=True)
    # 2. device form
    ctx = bliss.Context(0)
    tS, tX = torch.from_numpy(S).cuda(), torch.from_numpy(X).cuda()
    t_album, t_skip = torch.from_numpy(album_of.astype(np.int32)).cuda(), torch.from_numpy(rows.astype(np.int32)).cuda()

    def device():
        r = ctx.album_knn(tS, off, tX, t_album, A, k, skip=t_skip)
        ctx.synchronize()
        torch.cuda.synchronize()
        return r

    out["device_form_ms"], out["device_form_spread_ms"] = median_ms(device, args.reps)
    ctx.profile_enable(True)
    ctx.profile_reset()
    dev = device()
    out["kernels_ms"] = {name: round(v[0], 3) for name, v in ctx.profile().items()}
    ctx.profile_enable(False)
    print(json.dumps({"device_form_ms": out["device_form_ms"], "kernels_ms": out["kernels_ms"]}), flush=True)
    idx_host = host()[0]
    assert np.array_equal(dev[0].cpu().numpy(), idx_host), "the two forms disagree"
    ctx.close()
    # 3. / 4. the library call against the per-album loop
    with tempfile.TemporaryDirectory() as tmp:
        db = os.path.join(tmp, "bliss.db")
        t0 = time.perf_counter()
        build_library(bliss, db, X, album_of, rng)
        out["build_library_s"] = round(time.perf_counter() - t0, 1)
        t0 = time.perf_counter()
        table = bliss.library.album_playlists(db, k)
        out["album_playlists_s"] = round(time.perf_counter() - t0, 2)
        print(json.dumps({"album_playlists_s": out["album_playlists_s"]}), flush=True)
        titles = list(table)
        sample = [titles[i] for i in rng.choice(len(titles), min(args.sample, len(titles)), replace=False)]
        times = []
        for t in sample:
            t0 = time.perf_counter()
            pl = bliss.library.album_playlist_from(db, t, k)
            times.append(time.perf_counter() - t0)
            assert [s.path for s in pl] == [s.path for s in table[t]], t
            print(json.dumps({"album_playlist_from_s": round(times[-1], 2)}), flush=True)
        out["per_album_sample"] = len(sample)
        out["per_album_mean_s"] = round(statistics.mean(times), 3)
        out["per_album_spread_s"] = round(max(times) - min(times), 3)
        out["per_album_loop_extrapolated_s"] = round(statistics.mean(times) * len(titles), 1)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
