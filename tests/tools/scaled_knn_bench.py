"""The locally scaled k-nearest search on the device (blissgpu_scaled_knn_device) against (a) the project's own unscaled search
(blissgpu_knn_device) on the same data and (b) a torch loop on the same GPU: torch.cdist in row blocks, divided by the root of the
outer product of the scales, torch.topk.  And the k-occurrence pass (blissgpu_knn_occurrence_device) over the 10^5 x 32 result,
plain atomics against the windowed LDS histogram (BLISSGPU_OCCURRENCE_LDS=1) against torch.bincount.  Data: a seeded Gaussian
mixture, d = 23, euclidean, k = 32, queries = the library, every song skipping itself; the scales are the mean distance to the 10
nearest songs (NICDM), taken from Context.knn.

Every case runs in a child process of its own under a time limit, and the driver stops at the first child that fails.  Per case:
medians, minima and maxima of `reps` wall times after one warm-up of each route, the routes alternating in one process; the
HIP-event times of the kernels from the context profiler.  Where the scaled scan's extra time goes is split in two by a third
route: the scaled search with every scale = 1 selects what the unscaled search selects, with the same thresholds, so its time
over the unscaled one is the price of the scale loads, the per-candidate bound and the survivors' division and second root; the
real scales' time over that is the filter's (the thresholds are scaled distances, the lists differ).  The hubness of both
rankings is recorded with the times.  Writes one JSON file.

    python tests/tools/scaled_knn_bench.py [--ns 10000,100000] [--reps 5] [--out profiles/scaled_knn_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
K, M_SCALE, D = 32, 10, 23


def library(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = 2.0 * rng.standard_normal((32, d))
    return (centres[rng.integers(0, 32, n)] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)


def summary(ts):
    ms = [round(1e3 * t, 3) for t in ts]
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": min(ms), "max_ms": max(ms), "all_ms": ms}


def one_case(args):
    import torch

    import bliss_rs_amd as bliss

    assert torch.cuda.is_available(), "scaled_knn_bench measures on the GPU: there is no CPU path"
    n = args.case
    ctx = bliss.Context(0)
    X = torch.from_numpy(library(n, D, 1)).cuda()
    me = torch.arange(n, dtype=torch.int32, device=X.device)

    def sync():
        ctx.synchronize()
        torch.cuda.synchronize()

    def timed(f):
        sync()
        t0 = time.perf_counter()
        r = f()
        sync()
        return time.perf_counter() - t0, r

    scale = ctx.knn(X, X, M_SCALE, skip=me)[1].double().mean(dim=1).float().contiguous()
    ones = torch.ones_like(scale)

    def unscaled():
        return ctx.knn(X, X, K, skip=me)

    def scaled():
        return ctx.scaled_knn(X, scale, X, scale, K, skip=me)

    def scaled_unit():
        return ctx.scaled_knn(X, ones, X, ones, K, skip=me)

    def torch_loop():
        idx = torch.empty((n, K), dtype=torch.int64, device=X.device)
        for i0 in range(0, n, args.block):
            i1 = min(i0 + args.block, n)
            Dm = torch.cdist(X[i0:i1], X)
            Dm /= torch.sqrt(scale[i0:i1, None] * scale[None, :])
            ar = torch.arange(i1 - i0, device=X.device)
            Dm[ar, ar + i0] = float("inf")
            idx[i0:i1] = torch.topk(Dm, K, dim=1, largest=False).indices
        return idx

    routes = {"unscaled_knn": unscaled, "scaled_knn": scaled, "scaled_knn_unit_scales": scaled_unit, "torch_cdist_topk": torch_loop}
    times = {name: [] for name in routes}
    for f in routes.values():
        f()
    for _ in range(args.reps):
        for name, f in routes.items():
            times[name].append(timed(f)[0])
    case = {"n": n, "k": K, "d": D, "scale_m": M_SCALE, "wall": {name: summary(ts) for name, ts in times.items()}}
    med = lambda name: case["wall"][name]["median_ms"]  # noqa: E731
    case["scaled_over_unscaled_wall"] = round(med("scaled_knn") / med("unscaled_knn"), 3)
    case["torch_over_scaled_wall"] = round(med("torch_cdist_topk") / med("scaled_knn"), 3)
    # the kernels' own times
    kernel = {}
    ctx.profile_enable(True)
    for name in ("unscaled_knn", "scaled_knn", "scaled_knn_unit_scales"):
        per = []
        for _ in range(args.reps):
            sync()
            ctx.profile_reset()
            routes[name]()
            sync()
            per.append({k: v[0] for k, v in ctx.profile().items() if v[1]})
        kernel[name] = {k: round(statistics.median(p[k] for p in per), 4) for k in per[0]}
    ctx.profile_enable(False)
    case["kernel_ms"] = kernel
    scan_u, scan_s = kernel["unscaled_knn"]["knn_scan_kernel"], kernel["scaled_knn"]["scaled_knn_scan_kernel"]
    scan_1 = kernel["scaled_knn_unit_scales"]["scaled_knn_scan_kernel"]
    case["scan_scaled_over_unscaled"] = round(scan_s / scan_u, 3)
    case["scan_extra_ms"] = {"arithmetic_and_loads (unit scales - unscaled)": round(scan_1 - scan_u, 4),
                             "filter_and_lists (real scales - unit scales)": round(scan_s - scan_1, 4)}
    case["scan_gpairs_per_s"] = {"unscaled": round(n * n / scan_u / 1e6, 1), "scaled": round(n * n / scan_s / 1e6, 1)}
    # what it buys: the hubness of both rankings (and how far torch's lists are from the library's)
    raw_idx, sc_idx = unscaled()[0], scaled()[0]
    h_raw = bliss.playlist.Hubness.from_counts(ctx.knn_occurrence(raw_idx, n).cpu().numpy(), K)
    h_sc = bliss.playlist.Hubness.from_counts(ctx.knn_occurrence(sc_idx, n).cpu().numpy(), K)
    case["hubness"] = {"raw": {"skewness": round(h_raw.skewness, 3), "max_count": int(h_raw.counts.max()), "orphans": int(h_raw.orphans().size)},
                       "scaled": {"skewness": round(h_sc.skewness, 3), "max_count": int(h_sc.counts.max()), "orphans": int(h_sc.orphans().size)}}
    t_idx = torch_loop()
    case["rows_where_torch_lists_differ"] = int((t_idx != sc_idx.long()).any(dim=1).sum().item())  # (its distances have other bits)
    # the occurrence pass
    if n >= args.occurrence_from:
        def occ():
            return ctx.knn_occurrence(sc_idx, n)

        def bincount():
            return torch.bincount(sc_idx.reshape(-1).long(), minlength=n)

        assert torch.equal(occ().long(), bincount())
        ot = {"atomics": [], "lds_histogram": [], "torch_bincount": []}
        ok = {"atomics": [], "lds_histogram": []}
        ctx.profile_enable(True)
        for rep in range(args.reps + 1):  # (the first trip is the warm-up)
            for name in ot:
                if name == "lds_histogram":
                    os.environ["BLISSGPU_OCCURRENCE_LDS"] = "1"
                sync()
                ctx.profile_reset()
                t, r = timed(bincount if name == "torch_bincount" else occ)
                os.environ.pop("BLISSGPU_OCCURRENCE_LDS", None)
                if name == "lds_histogram":
                    assert torch.equal(r.long(), bincount())
                if rep:
                    ot[name].append(t)
                    if name in ok:
                        ok[name].append(ctx.profile()["knn_occurrence_kernel"][0])
        ctx.profile_enable(False)
        case["occurrence"] = {"entries": n * K, "wall": {name: summary(ts) for name, ts in ot.items()},
                              "kernel_ms": {name: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                                            for name, v in ok.items()}}
    print("CASE " + json.dumps(case), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="10000,100000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--block", type=int, default=4096, help="rows per torch.cdist block of the baseline")
    ap.add_argument("--occurrence-from", type=int, default=100000, help="the occurrence pass is timed from this n on")
    ap.add_argument("--limit", type=int, default=240, help="seconds a case's child process may take")
    ap.add_argument("--case", type=int, help="(internal) run one case: n")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scaled_knn_bench.json"))
    args = ap.parse_args()
    if args.case:
        return one_case(args)
    out = {"d": D, "k": K, "reps": args.reps, "block": args.block, "cases": []}
    for n in (int(v) for v in args.ns.split(",")):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--case", str(n), "--reps", str(args.reps),
               "--block", str(args.block), "--occurrence-from", str(args.occurrence_from)]
        child = subprocess.run(cmd, capture_output=True, text=True)
        if child.returncode != 0:  # a fault, an abort or the time limit: nothing more is started
            print(child.stdout[-2000:], child.stderr[-4000:], sep="\n")
            raise SystemExit(f"case n={n} ended with status {child.returncode}")
        case = json.loads(next(line for line in child.stdout.splitlines() if line.startswith("CASE "))[5:])
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
