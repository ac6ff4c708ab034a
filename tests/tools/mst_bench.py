"""The minimum spanning tree on the device (blissgpu_mst_device) against the same Boruvka loop with the scan done by torch on the
same GPU: torch.cdist in row blocks, the entries of a song's own component set to +inf, min over the columns, one winner per
component on the host, and the same merge (components from the picked edges, renumbered).  Data: a seeded Gaussian mixture,
d = 23, euclidean; n in {10^4, 10^5}; without cores and with min_samples = 5 (the cores come from Context.knn and are shared by
both routes; their time is recorded on its own).

Every case runs in a child process of its own under a time limit, and the driver stops at the first child that fails.  Per case:
medians of `reps` wall times after one warm-up of each route, alternating in one process; the HIP-event times of the mst_ kernels
from the context profiler; from the library's own trace (BLISSGPU_MST_TRACE) the scan's time per round with the late-round skip
on and off (BLISSGPU_MST_SKIP), the components per round, and what is left of the call's time when the rounds are taken away --
the host's merges; round 1's pairs per second (n^2 / its scan); the total against rounds x the first round.  The torch route uses
cdist's default, fastest form for the times.  Its distances are not the all-pairs kernel's bits, so a near-tie may fall the other
way: the edges of the device's tree that torch's tree lacks are counted.  Up to n = 20 000 the same loop is also run over
Context.pairwise's rows -- the bits the tree is
defined with -- and there, on tie-free data (no cores), the same edges are asserted.  Writes one JSON file.

    python tests/tools/mst_bench.py [--ns 10000,100000] [--min-samples 0,5] [--reps 3] [--out profiles/mst_bench.json]
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


def library(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = 2.0 * rng.standard_normal((32, d))
    return (centres[rng.integers(0, 32, n)] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)


def torch_boruvka(torch, X, core, block, rows):
    """rows(i0, i1) -> the distances of songs i0 .. i1 - 1 to every song, f32 [i1 - i0, n] on the device
    -> (u, v int64 [n - 1] sorted by (u, v), rounds, seconds of host work)"""
    n = X.shape[0]
    comp = np.arange(n)
    eu, ev = [], []
    rounds, host = 0, 0.0
    while True:
        comp_d = torch.from_numpy(comp).to(X.device)
        val = torch.empty(n, dtype=torch.float32, device=X.device)
        arg = torch.empty(n, dtype=torch.int64, device=X.device)
        for i0 in range(0, n, block):
            D = rows(i0, min(i0 + block, n))
            if core is not None:
                D = torch.maximum(torch.maximum(D, core[i0:i0 + block, None]), core[None, :])
            D.masked_fill_(comp_d[i0:i0 + block, None] == comp_d[None, :], float("inf"))
            val[i0:i0 + block], arg[i0:i0 + block] = D.min(dim=1)
        val_h, arg_h = val.cpu().numpy(), arg.cpu().numpy()
        t0 = time.perf_counter()
        i = np.arange(n)
        lo, hi = np.minimum(i, arg_h), np.maximum(i, arg_h)
        order = np.lexsort((hi, lo, val_h.view(np.uint32), comp))
        first = order[np.concatenate([[True], comp[order][1:] != comp[order][:-1]])]  # every component's smallest key
        pu, pv = lo[first], hi[first]
        keep = np.unique(pu * n + pv)  # the doubles
        pu, pv = keep // n, keep % n
        eu.append(pu)
        ev.append(pv)
        # components of the forest so far, numbered by lowest member
        parent = np.arange(n)
        au, av = np.concatenate(eu), np.concatenate(ev)
        while True:  # pointer jumping over the picked edges
            m = np.minimum(parent[au], parent[av])
            before = parent.copy()
            np.minimum.at(parent, au, m)
            np.minimum.at(parent, av, m)
            parent = parent[parent]
            if np.array_equal(parent, before):
                break
        _, comp = np.unique(parent, return_inverse=True)
        rounds += 1
        host += time.perf_counter() - t0
        if comp.max() == 0:
            break
        assert rounds < 64
    u, v = np.concatenate(eu), np.concatenate(ev)
    order = np.lexsort((v, u))
    return u[order], v[order], rounds, host


def one_case(args):
    import torch

    import bliss_rs_amd as bliss

    assert torch.cuda.is_available(), "mst_bench measures on the GPU: there is no CPU path"
    n, m = args.case
    d = 23
    ctx = bliss.Context(0)
    X = torch.from_numpy(library(n, d, 1)).cuda()

    def sync():
        ctx.synchronize()
        torch.cuda.synchronize()

    def timed(f):
        sync()
        t0 = time.perf_counter()
        r = f()
        sync()
        return time.perf_counter() - t0, r

    core, core_ms = None, None
    if m:
        def cores():
            return ctx.knn(X, X, m, skip=torch.arange(n, dtype=torch.int32, device=X.device))[1][:, m - 1].contiguous()
        cores()
        core_ms = round(1e3 * statistics.median(timed(cores)[0] for _ in range(args.reps)), 3)
        core = cores()

    def new():
        return ctx.mst(X, core=core)

    def baseline():  # (torch's default: the matrix-multiply form, its fastest)
        return torch_boruvka(torch, X, core, args.block, lambda i0, i1: torch.cdist(X[i0:i1], X))

    def own_rows():  # the same loop over the library's own all-pairs distances: the bits the tree is defined with
        return torch_boruvka(torch, X, core, args.block, lambda i0, i1: ctx.pairwise(X[i0:i1], X).clone())

    new(), baseline()
    tn, tb, tb_host = [], [], []
    for _ in range(args.reps):
        tn.append(timed(new)[0])
        t, r = timed(baseline)
        tb.append(t)
        tb_host.append(r[3])
    u, v, w, rounds = new()
    key = np.lexsort((v.cpu().numpy(), u.cpu().numpy()))
    mine = (u.cpu().numpy().astype(np.int64)[key], v.cpu().numpy().astype(np.int64)[key])
    fast = baseline()

    def differing(other):
        a, b = set(zip(mine[0].tolist(), mine[1].tolist())), set(zip(other[0].tolist(), other[1].tolist()))
        return len(a - b)

    # torch's distances are not the all-pairs kernel's bits (another order of the sum), so near-ties may fall the other way:
    # the edges that differ are counted, not refused.  Over the library's own distances the loop must find the same tree
    diff_fast, diff_own = differing(fast), None
    if n <= 20000:
        diff_own = differing(own_rows())
        if not m:
            assert diff_own == 0, "the torch loop over the all-pairs kernel's distances found another tree on tie-free data"
    sync()
    ctx.profile_enable(True)
    ctx.profile_reset()
    new()
    sync()
    prof = {k: [round(v[0], 4), int(v[1])] for k, v in ctx.profile().items() if v[1]}
    ctx.profile_enable(False)
    case = {
        "n": n, "min_samples": m, "rounds": rounds, "torch_rounds": fast[2],
        "wall_ms": round(1e3 * statistics.median(tn), 3), "wall_ms_all": [round(1e3 * t, 3) for t in tn],
        "wall_ms_torch": round(1e3 * statistics.median(tb), 3), "wall_ms_torch_all": [round(1e3 * t, 3) for t in tb],
        "torch_host_ms": round(1e3 * statistics.median(tb_host), 3), "core_distances_ms": core_ms,
        "edges_not_in_torch_tree_default_cdist": diff_fast,
        "edges_not_in_torch_tree_over_pairwise_rows": diff_own,
        "tree_length": float(w.double().sum().item()), "kernel_ms": prof,
    }
    # the library's own trace, skip on and off: one traced call each (the trace synchronises around the scan)
    for skip in ("1", "0"):
        os.environ["BLISSGPU_MST_SKIP"] = skip
        new()
        sync()
        print(f"TRACE skip={skip} begin", file=sys.stderr, flush=True)
        os.environ["BLISSGPU_MST_TRACE"] = "1"
        new()
        sync()
        del os.environ["BLISSGPU_MST_TRACE"]
        print(f"TRACE skip={skip} end", file=sys.stderr, flush=True)
    del os.environ["BLISSGPU_MST_SKIP"]
    print("CASE " + json.dumps(case), flush=True)
    ctx.close()


def parse_trace(stderr, skip):
    body = stderr.split(f"TRACE skip={skip} begin")[1].split(f"TRACE skip={skip} end")[0]
    rounds = [(int(c), float(s), float(r)) for c, s, r in
              re.findall(r"round \d+: (\d+) components, scan ([0-9.]+) ms, round ([0-9.]+) ms", body)]
    total = float(re.search(r"rounds, ([0-9.]+) ms in all", body).group(1))
    return rounds, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="10000,100000")
    ap.add_argument("--min-samples", default="0,5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--block", type=int, default=4096, help="rows per torch.cdist block of the baseline")
    ap.add_argument("--limit", type=int, default=240, help="seconds a case's child process may take")
    ap.add_argument("--case", type=lambda s: tuple(int(v) for v in s.split(",")), help="(internal) run one case: n,min_samples")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mst_bench.json"))
    args = ap.parse_args()
    if args.case:
        return one_case(args)
    out = {"d": 23, "reps": args.reps, "block": args.block, "cases": []}
    for n in (int(v) for v in args.ns.split(",")):
        for m in (int(v) for v in args.min_samples.split(",")):
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--case", f"{n},{m}", "--reps",
                   str(args.reps), "--block", str(args.block)]
            child = subprocess.run(cmd, capture_output=True, text=True)
            if child.returncode != 0:  # a fault, an abort or the time limit: nothing more is started
                print(child.stdout[-2000:], child.stderr[-4000:], sep="\n")
                raise SystemExit(f"case n={n} min_samples={m} ended with status {child.returncode}")
            case = json.loads(next(line for line in child.stdout.splitlines() if line.startswith("CASE "))[5:])
            for skip, name in (("1", "skip_on"), ("0", "skip_off")):
                rounds, total = parse_trace(child.stderr, skip)
                scans = [s for _, s, _ in rounds]
                case[name] = {
                    "components_per_round": [c for c, _, _ in rounds], "scan_ms_per_round": scans,
                    "round_ms_per_round": [r for _, _, r in rounds], "call_ms": total,
                    "scan_ms_total": round(sum(scans), 3), "rounds_x_first_scan_ms": round(len(scans) * scans[0], 3),
                    "host_merge_ms": round(total - sum(r for _, _, r in rounds), 3),
                    "host_merge_share": round((total - sum(r for _, _, r in rounds)) / total, 4),
                    "round_1_gpairs_per_s": round(n * n / scans[0] / 1e6, 2),
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
