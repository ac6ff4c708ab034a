"""Radio playlists over a 10^5-song library (d = 23, euclidean, k = 32, device forms): what the label rules cost.  The library is
seeded Gaussian songs in 3 000 artist clusters (centre + 0.3 * noise, so a song's nearest neighbours are its own artist), four
albums per artist.  For radios from 1, 1 024 and every song (radio g starts at a drawn row, skips it and carries its labels),
timed in one process, the variants alternating, medians of `reps` after one warm-up of each:

  journey          Context.journeys(CHAIN, no gate): the same pair count through the step kernel that existed before
  radio_none       Context.radio without a rule -- the same songs as the journey, bit for bit (checked)
  radio_artist5    no artist twice within 5 tracks
  radio_artist5_album20   ... and no album twice within 20
  nearest_quota2   mode "nearest": the k nearest songs, at most two per artist
  torch_loop       (1 and 1 024 radios only) the artist-5 + album-20 chain as a torch loop: per step one cdist block of
                   [radios, n] distances, the taken / skipped / banned songs masked to inf, argmin.  Its lists are compared with
                   the radio's (cdist's distances differ in the last bits, so a few picks may differ; the count is reported).

Every variant's ratio to the journey, each kernel's own time from the context profiler (a run of its own), and how many radios
the rules changed.  Writes one JSON file.

    python tests/tools/radio_bench.py [--n 100000] [--reps 5] [--out profiles/radio_bench.json]
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
    ap.add_argument("--artists", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radio_bench.json"))
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    n, d, k = args.n, 23, args.k
    rng = np.random.default_rng(1)
    artist = rng.integers(0, args.artists, n)
    centre = rng.standard_normal((args.artists, d))
    X = (centre[artist] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    album = artist * 4 + rng.integers(0, 4, n)
    labels = np.stack([artist, album]).astype(np.int32)
    tX, tL = torch.from_numpy(X).cuda(), torch.from_numpy(labels).cuda()
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

    def kernels_ms(f):
        sync()
        ctx.profile_enable(True)
        ctx.profile_reset()
        f()
        sync()
        prof = ctx.profile()
        ctx.profile_enable(False)
        return {name: round(v[0], 3) for name, v in prof.items() if v[0] > 0}

    def torch_loop(tA, rows, fl):
        """the artist-5 + album-20 chain: cdist blocks + masked argmin"""
        G = tA.shape[0]
        inf = torch.tensor(float("inf"), device="cuda")
        idx = torch.full((G, k), -1, dtype=torch.int64, device="cuda")
        hist = [torch.cat([fl[:, r:r + 1].long(), torch.full((G, k), -1, dtype=torch.int64, device="cuda")], dim=1) for r in range(2)]
        gone = torch.zeros((G, n), dtype=torch.bool, device="cuda")
        gone[torch.arange(G, device="cuda"), rows.long()] = True
        q = tA
        for t in range(k):
            D = torch.cdist(q, tX)
            bad = gone.clone()
            for r, w in ((0, 5), (1, 20)):
                for p in range(max(t - w, -1), t):  # (limit 1: a label anywhere in the window is banned)
                    bad |= tL[r].long()[None, :] == hist[r][:, p + 1:p + 2]
            j = torch.where(bad, inf, D).argmin(dim=1)
            idx[:, t] = j
            gone[torch.arange(G, device="cuda"), j] = True
            for r in range(2):
                hist[r][:, t + 1] = tL[r].long()[j]
            q = tX[j]
        return idx

    out = {"n": n, "d": d, "k": k, "artists": args.artists, "albums_per_artist": 4, "metric": "euclidean", "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "sizes": []}
    for G in sorted({1, min(1024, n), n}):
        a = np.sort(rng.choice(n, G, replace=False))
        ta = torch.from_numpy(a).cuda()
        tA = tX[ta].contiguous()
        own = torch.from_numpy(np.stack([a, np.full(G, -1)], axis=1).astype(np.int32)).cuda()
        fl = tL[:, ta].t().contiguous()
        fs = {"journey_ms": lambda: ctx.journeys(tA, None, tX, k, skip=own),
              "radio_none_ms": lambda: ctx.radio(tA, tX, k, skip=own),
              "radio_artist5_ms": lambda: ctx.radio(tA, tX, k, tL[:1], [5], [1], fl[:, :1].contiguous(), skip=own),
              "radio_artist5_album20_ms": lambda: ctx.radio(tA, tX, k, tL, [5, 20], [1, 1], fl, skip=own),
              "nearest_quota2_ms": lambda: ctx.radio(tA, tX, k, tL[:1], [k + 1], [2], fl[:, :1].contiguous(), mode="nearest", skip=own)}
        if G <= 1024:
            fs["torch_loop_ms"] = lambda: torch_loop(tA, ta, fl)
        med, spread = medians(fs)
        row = dict(med, radios=G, spread_ms=spread)
        for name in fs:
            if name != "journey_ms":
                row[name[:-3] + "_over_journey"] = round(med[name] / med["journey_ms"], 3)
        row["kernels_ms"] = {name: kernels_ms(f) for name, f in fs.items() if name != "torch_loop_ms"}
        res = {name: f() for name, f in fs.items()}
        sync()
        j, r0 = res["journey_ms"], res["radio_none_ms"]
        row["radio_none_equals_journey"] = bool(torch.equal(j[0], r0[0]) and torch.equal(j[1].view(torch.int32), r0[1].view(torch.int32)))
        for name in ("radio_artist5_ms", "radio_artist5_album20_ms"):
            row[name[:-3] + "_radios_changed"] = int((res[name][0] != j[0]).any(dim=1).sum().item())
        row["nearest_quota2_full_radios"] = int((res["nearest_quota2_ms"][0][:, k - 1] >= 0).sum().item())
        if G <= 1024:
            row["torch_loop_picks_differing"] = int((res["torch_loop_ms"] != res["radio_artist5_album20_ms"][0].long()).sum().item())
            row["picks"] = G * k
        print(json.dumps(row), flush=True)
        out["sizes"].append(row)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
