"""Ward clustering on the device (blissgpu_ward) against the same rounds done by torch on the same GPU -- torch.cdist in row
blocks, the weights, argmin over the columns, the mutual pairs on the host, the merged centroids written with index_copy_ -- and,
at n <= 10^4, against scipy's linkage(X, "ward") on the CPU for scale.  Data: the planted libraries of tests/test_ward_host.py
(8 clusters, d = 23, euclidean); n in {10^4, 10^5}.

Every case runs in a child process of its own under a time limit, and the driver stops at the first child that fails.  Per case:
medians of `reps` wall times after one warm-up of each route, alternating in one process (the device's route as the library
chooses, and with the filter in front of the root, BLISSGPU_WARD_FILTER, forced on and off); the HIP-event times of the ward_ kernels from the context profiler; from
the library's own trace (BLISSGPU_WARD_TRACE) the rounds, the clusters, pairs and scan milliseconds per round, the total pairs
over n^2 and round 0's pairs per second.  The torch route's distances are not the all-pairs kernel's bits and its argmin breaks
ties to the lower index, so a near-tie may fall the other way: whether its cuts at K = 8 and 20 are the device's partitions is
recorded, not asserted.  Writes one JSON file.

    python tests/tools/ward_bench.py [--ns 10000,100000] [--reps 3] [--out profiles/ward_bench.json]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def planted(n):
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, 23)).astype(np.float32)
    lab = rng.integers(0, 8, n)
    X += (lab[:, None] == np.arange(8)).astype(np.float32) @ rng.standard_normal((8, 23)).astype(np.float32) * 3
    return X


def torch_ward(torch, X_host, block, dev="cuda"):
    """the same rounds with torch's own kernels -> (u, v int64 [n - 1] in merge order, cost f32, rounds, pairs evaluated)"""
    dev = torch.device(dev)
    C = torch.from_numpy(X_host).to(dev)
    n = C.shape[0]
    size = torch.ones(n, dtype=torch.float32, device=dev)
    low = torch.arange(n, dtype=torch.int64, device=dev)
    eu, ev, ec = [], [], []
    rounds, pairs = 0, 0
    while C.shape[0] > 1:
        m = C.shape[0]
        val = torch.empty(m, dtype=torch.float32, device=dev)
        arg = torch.empty(m, dtype=torch.int64, device=dev)
        for i0 in range(0, m, block):
            i1 = min(i0 + block, m)
            D = torch.cdist(C[i0:i1], C)
            s = size[i0:i1, None]
            D = (D * D) * ((s * size[None, :]) / (s + size[None, :]))
            D[torch.arange(i1 - i0, device=dev), torch.arange(i0, i1, device=dev)] = float("inf")
            val[i0:i1], arg[i0:i1] = D.min(dim=1)
        idx = torch.arange(m, device=dev)
        p = torch.nonzero((arg[arg] == idx) & (idx < arg)).reshape(-1)
        assert p.numel() >= 1, "a round merged nothing"
        q = arg[p]
        eu.append(low[p].cpu().numpy())
        ev.append(low[q].cpu().numpy())
        ec.append(val[p].cpu().numpy())
        sp, sq = size[p].double()[:, None], size[q].double()[:, None]
        C.index_copy_(0, p, ((sp * C[p].double() + sq * C[q].double()) / (sp + sq)).float())
        size.index_copy_(0, p, size[p] + size[q])
        keep = torch.ones(m, dtype=torch.bool, device=dev)
        keep[q] = False
        C, size, low = C[keep], size[keep], low[keep]
        pairs += m * (m - 1)
        rounds += 1
    u, v, c = np.concatenate(eu), np.concatenate(ev), np.concatenate(ec)
    order = np.argsort(c, kind="stable")
    return u[order], v[order], c[order], rounds, pairs


def cut(n, u, v, k):
    """the partition after the first n - k merges, as a canonical label array"""
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(u[:n - k].tolist(), v[:n - k].tolist()):
        ra, rb = find(a), find(b)
        parent[max(ra, rb)] = min(ra, rb)
    return np.asarray([find(i) for i in range(n)])


def one_case(args):
    import torch

    import bliss_rs_amd as bliss

    assert torch.cuda.is_available(), "ward_bench measures on the GPU: there is no CPU path"
    n = args.case
    P = bliss.playlist
    ctx = bliss.Context.default()
    X = planted(n)

    def sync():
        ctx.synchronize()
        torch.cuda.synchronize()

    def timed(f):
        sync()
        t0 = time.perf_counter()
        r = f()
        sync()
        return time.perf_counter() - t0, r

    def new(filter_on=None):  # None: the library's own choice, by the size of every scan
        if filter_on is not None:
            os.environ["BLISSGPU_WARD_FILTER"] = "1" if filter_on else "0"
        try:
            return P.ward_tree(X)
        finally:
            os.environ.pop("BLISSGPU_WARD_FILTER", None)

    def baseline():
        return torch_ward(torch, X, args.block)

    new(True), new(False), baseline()  # warm-up: code objects, the workspace, torch's algorithm choice
    ta, tf, tn, tb = [], [], [], []
    for _ in range(args.reps):
        ta.append(timed(new)[0])
        tf.append(timed(lambda: new(True))[0])
        tn.append(timed(lambda: new(False))[0])
        tb.append(timed(baseline)[0])
    tree, base = new(), baseline()
    for other in (new(True), new(False)):
        assert all(np.array_equal(getattr(tree, k), getattr(other, k)) for k in ("u", "v", "size", "round")) and tree.cost.tobytes() == other.cost.tobytes()
    same_cuts = {str(k): bool(np.array_equal(cut(n, tree.u, tree.v, k), cut(n, base[0], base[1], k))) for k in (8, 20)}
    sync()
    prof = {}
    for name, on in (("filter", True), ("every_root", False)):
        ctx.profile_enable(True)
        ctx.profile_reset()
        new(on)
        sync()
        prof[name] = {k: [round(v[0], 4), int(v[1])] for k, v in ctx.profile().items() if v[1]}
        ctx.profile_enable(False)
    case = {
        "n": n, "rounds": tree.rounds, "torch_rounds": base[3], "torch_pairs_over_n2": round(base[4] / float(n * n), 3),
        "wall_ms": round(1e3 * statistics.median(ta), 3), "wall_ms_all": [round(1e3 * t, 3) for t in ta],
        "wall_ms_filter": round(1e3 * statistics.median(tf), 3), "wall_ms_filter_all": [round(1e3 * t, 3) for t in tf],
        "wall_ms_every_root": round(1e3 * statistics.median(tn), 3), "wall_ms_every_root_all": [round(1e3 * t, 3) for t in tn],
        "wall_ms_torch": round(1e3 * statistics.median(tb), 3), "wall_ms_torch_all": [round(1e3 * t, 3) for t in tb],
        "torch_cuts_equal_device": same_cuts, "within_total": float(tree.within()[-1]), "kernel_ms": prof,
    }
    if n <= args.scipy_max:
        from scipy.cluster import hierarchy

        t0 = time.perf_counter()
        Z = hierarchy.linkage(X.astype(np.float64), "ward")
        case["wall_ms_scipy_cpu"] = round(1e3 * (time.perf_counter() - t0), 1)
        case["heights_vs_scipy_max_rel"] = float(np.max(np.abs(tree.heights() - Z[:, 2]) / Z[:, 2]))
        case["cuts_equal_scipy"] = {str(k): bool(len(set(zip(tree.cut(k).tolist(), hierarchy.fcluster(Z, k, "maxclust").tolist()))) == k)
                                      for k in (2, 8, 20, 100)}
    for name, on in (("filter", True), ("every_root", False)):  # one traced call each (the trace synchronises around the scan)
        print(f"TRACE {name} begin", file=sys.stderr, flush=True)
        os.environ["BLISSGPU_WARD_TRACE"] = "1"
        new(on)
        sync()
        del os.environ["BLISSGPU_WARD_TRACE"]
        print(f"TRACE {name} end", file=sys.stderr, flush=True)
    print("CASE " + json.dumps(case), flush=True)


def parse_trace(stderr, name):
    body = stderr.split(f"TRACE {name} begin")[1].split(f"TRACE {name} end")[0]
    rounds = [(int(c), int(p), float(s), float(r)) for c, p, s, r in
              re.findall(r"round \d+: (\d+) clusters, (\d+) pairs, scan ([0-9.]+) ms, round ([0-9.]+) ms", body)]
    tail = re.search(r"rounds, ([0-9.]+) pairs / n\^2, ([0-9.]+) ms in all", body)
    return rounds, float(tail.group(1)), float(tail.group(2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="10000,100000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--block", type=int, default=4096, help="rows per torch.cdist block of the baseline")
    ap.add_argument("--scipy-max", type=int, default=10000, help="largest n that scipy's linkage runs at")
    ap.add_argument("--limit", type=int, default=400, help="seconds a case's child process may take")
    ap.add_argument("--case", type=int, help="(internal) run one case: n")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ward_bench.json"))
    args = ap.parse_args()
    if args.case:
        return one_case(args)
    out = {"d": 23, "reps": args.reps, "block": args.block, "cases": []}
    for n in (int(v) for v in args.ns.split(",")):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--case", str(n), "--reps", str(args.reps),
               "--block", str(args.block), "--scipy-max", str(args.scipy_max)]
        child = subprocess.run(cmd, capture_output=True, text=True)
        if child.returncode != 0:  # a fault, an abort or the time limit: nothing more is started
            print(child.stdout[-2000:], child.stderr[-4000:], sep="\n")
            raise SystemExit(f"case n={n} ended with status {child.returncode}")
        case = json.loads(next(line for line in child.stdout.splitlines() if line.startswith("CASE "))[5:])
        for name in ("filter", "every_root"):
            rounds, pairs, total = parse_trace(child.stderr, name)
            scans = [s for _, _, s, _ in rounds]
            case["trace_" + name] = {
                "clusters_per_round": [c for c, _, _, _ in rounds], "pairs_per_round": [p for _, p, _, _ in rounds],
                "scan_ms_per_round": scans, "round_ms_per_round": [r for _, _, _, r in rounds], "call_ms": total,
                "pairs_over_n2": pairs, "scan_ms_total": round(sum(scans), 3),
                "host_between_rounds_ms": round(total - sum(r for _, _, _, r in rounds), 3),
                "round_0_gpairs_per_s": round(n * (n - 1) / scans[0] / 1e6, 2),
            }
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
