"""Waypoint and directed playlists over a 10^5-song library (d = 23, euclidean, k = 20, device forms), timed in one process, the
variants alternating, medians of `reps` after one warm-up of each:

  1. G = 1, n/64, n/16, n/4 and n journeys (journey g starts at a drawn row, a waypoint journey ends at another; both rows are
     skipped): WAYPOINT, CHAIN x DOWN on column 0 and CHAIN x NONE, each against Context.chains(route="steps") for the same
     start rows -- the same pair count through the code that existed before -- with the ratio to it, journey_step_kernel's and
     chain_step_kernel's own times from the context profiler, and how many gated journeys ran all k steps;
  2. G = n/4 gated journeys over data whose gated column is constant (the gate passes everyone, the picks are those without a
     gate) against the same journeys without a gate: what the gate's own instructions cost, apart from what it does to the bound;
  3. one waypoint journey against the only other way to the same k songs: a host loop of one playlist.set_distances call per
     step (an n x d upload and an n-float download each), masking and argmin on the host.  The two lists are compared.

Writes one JSON file.

    python tests/tools/journeys_bench.py [--n 100000] [--reps 3] [--out profiles/journeys_bench_100k.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "journeys_bench_100k.json"))
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    n, d, k = args.n, 23, args.k
    rng = np.random.default_rng(1)
    X = rng.standard_normal((n, d)).astype(np.float32)
    tX = torch.from_numpy(X).cuda()
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

    def step_kernel_ms(f):
        sync()
        ctx.profile_enable(True)
        ctx.profile_reset()
        f()
        sync()
        prof = ctx.profile()
        ctx.profile_enable(False)
        return round(sum(v[0] for name, v in prof.items() if name in ("journey_step_kernel", "chain_step_kernel")), 3)

    out = {"n": n, "d": d, "k": k, "metric": "euclidean", "reps": args.reps, "gate": "down on column 0",
           "device": torch.cuda.get_device_name(0), "sizes": []}
    for G in sorted({1, n // 64, n // 16, n // 4, n}):
        a = np.sort(rng.choice(n, G, replace=False))
        b = (a + n // 2) % n
        tA, tB = tX[torch.from_numpy(a).cuda()].contiguous(), tX[torch.from_numpy(b).cuda()].contiguous()
        both = torch.from_numpy(np.stack([a, b], axis=1).astype(np.int32)).cuda()
        own = torch.from_numpy(np.stack([a, np.full(G, -1)], axis=1).astype(np.int32)).cuda()
        rows, off = torch.from_numpy(a.astype(np.int32)).cuda(), np.arange(G + 1, dtype=np.int64)
        fs = {"waypoint_ms": lambda: ctx.journeys(tA, tB, tX, k, skip=both, mode="waypoint"),
              "chain_down_ms": lambda: ctx.journeys(tA, None, tX, k, skip=own, gate="down", feature=0),
              "chain_none_ms": lambda: ctx.journeys(tA, None, tX, k, skip=own),
              "chains_steps_ms": lambda: ctx.chains(tA, off, tX, k, skip=rows, route="steps")}
        med, spread = medians(fs)
        row = dict(med, journeys=G, spread_ms=spread)
        for name in ("waypoint", "chain_down", "chain_none"):
            row[name + "_over_chains_steps"] = round(med[name + "_ms"] / med["chains_steps_ms"], 3)
        row["step_kernels_ms"] = {name: step_kernel_ms(f) for name, f in fs.items()}
        gated = ctx.journeys(tA, None, tX, k, skip=own, gate="down", feature=0)[0]
        sync()
        row["gated_full_journeys"] = int((gated[:, k - 1] >= 0).sum().item())
        row["gated_songs"] = int((gated >= 0).sum().item())
        free, same = ctx.journeys(tA, None, tX, k, skip=own), ctx.chains(tA, off, tX, k, skip=rows, route="steps")
        sync()
        row["chain_none_equals_chains"] = bool(torch.equal(free[0], same[0]) and torch.equal(free[1].view(torch.int32), same[1].view(torch.int32)))
        print(json.dumps(row), flush=True)
        out["sizes"].append(row)

    # 2. what a gate costs when it keeps nobody out: column 0 the same in every row, so "down" passes every candidate and the
    # picks are those without a gate -- the ref load and the LDS read in `valid` are paid, the neighbourhood is not emptied
    G = n // 4
    flat = tX.clone()
    flat[:, 0] = 0.0
    a = np.sort(rng.choice(n, G, replace=False))
    tA = flat[torch.from_numpy(a).cuda()].contiguous()
    own = torch.from_numpy(np.stack([a, np.full(G, -1)], axis=1).astype(np.int32)).cuda()
    fs = {"gate_passes_all_ms": lambda: ctx.journeys(tA, None, flat, k, skip=own, gate="down", feature=0),
          "no_gate_ms": lambda: ctx.journeys(tA, None, flat, k, skip=own)}
    med, spread = medians(fs)
    r0, r1 = fs["gate_passes_all_ms"](), fs["no_gate_ms"]()
    sync()
    out["gate_that_passes_everyone"] = dict(med, journeys=G, spread_ms=spread, same_songs=bool(torch.equal(r0[0], r1[0])),
                                            ratio=round(med["gate_passes_all_ms"] / med["no_gate_ms"], 3))
    print(json.dumps(out["gate_that_passes_everyone"]), flush=True)

    # 3. one waypoint journey: the device call against a host loop of set_distances
    a, b = 17, n // 2 + 17
    tA, tB = tX[a:a + 1].contiguous(), tX[b:b + 1].contiguous()
    both = torch.tensor([[a, b]], dtype=torch.int32, device="cuda")
    songs = {}

    def device_call():
        songs["device"] = ctx.journeys(tA, tB, tX, k, skip=both, mode="waypoint")[0].cpu().numpy()[0].tolist()

    def host_loop():
        free = np.ones(n, bool)
        free[[a, b]] = False
        picks = []
        for t in range(k):
            w = X[a] + (X[b] - X[a]) * (np.float32(t + 1) / np.float32(k + 1))
            row = bliss.playlist.set_distances(w[None, :], X)
            j = int(np.argmin(np.where(free, row, np.float32(np.inf))))
            picks.append(j)
            free[j] = False
        songs["host"] = picks

    med, spread = medians({"journeys_ms": device_call, "set_distances_loop_ms": host_loop})
    out["one_waypoint_journey"] = dict(med, spread_ms=spread, same_songs=songs["device"] == songs["host"])
    print(json.dumps(out["one_waypoint_journey"]), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
