"""The 2-D map on the device (blissgpu_map_layout) against a torch loop of the same forces on the same GPU: the
repulsion in row blocks ([block, n] float32 temporaries: differences, 1 / (1 + s), the weighted sums), the attraction over the
CSR entries by index_add_, the same gain / momentum update -- float32 throughout, torch's own sum orders.  Data: a seeded
Gaussian mixture, d = 23; P from map_affinities of the device's nearest lists at perplexity 30; n in {10^4, 10^5}.

Every case runs in a child process of its own under a time limit, and the driver stops at the first child that fails.  Per case:
ms per iteration of the library for each way of feeding y_j to the scan (BLISSGPU_MAP_FEED = scalar / lds) -- the difference of
two calls of different length, so that the uploads and the first-call costs cancel, median of `reps` --, the HIP-event times of
the three kernels from the default context's profiler over one short call, ms per iteration of the torch loop, and the wall
time of the whole 750-iteration layout (and of the stages in front of it: nearest lists, affinities, starting positions).
Writes one JSON file.

    python tests/tools/map_bench.py [--ns 10000,100000] [--reps 3] [--out profiles/map_bench.json]
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
PARAMS = dict(exag_iters=250, exaggeration=12.0, momentum0=0.5, momentum1=0.8, min_gain=0.01)


def library(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = 2.0 * rng.standard_normal((32, d))
    return (centres[rng.integers(0, 32, n)] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)


def torch_iterations(torch, Y, row, col, val, n_iter, lr, block):
    """n_iter iterations of the same forces and update in torch, float32, exaggeration 12 / momentum 0.5 throughout"""
    n = Y.shape[0]
    U, gain = torch.zeros_like(Y), torch.ones_like(Y)
    for _ in range(n_iter):
        rep = torch.empty_like(Y)
        Z = torch.zeros((), dtype=torch.float64, device=Y.device)
        for i0 in range(0, n, block):
            d = Y[i0:i0 + block, None, :] - Y[None, :, :]
            q = 1.0 / (1.0 + (d * d).sum(-1))
            Z += q.sum(dtype=torch.float64) - q.shape[0]  # (the diagonal's q = 1; its force is 0)
            rep[i0:i0 + block] = ((q * q)[:, :, None] * d).sum(1)
        de = Y[row] - Y[col]
        w = val / (1.0 + (de * de).sum(-1))
        att = torch.zeros_like(Y).index_add_(0, row, w[:, None] * de)
        g = 4.0 * (12.0 * att - rep / Z.float())
        gain = torch.where(U * g < 0, gain + 0.2, gain * 0.8).clamp_min(0.01)
        U = 0.5 * U - lr * gain * g
        Y = Y + U
    return Y


def one_case(args):
    import torch

    import bliss_rs_amd as bliss

    assert torch.cuda.is_available(), "map_bench measures on the GPU: there is no CPU path"
    pl = bliss.playlist
    n = args.case
    X = library(n, 23, 1)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    k = min(n - 1, 90)
    t_knn, (idx, dist) = timed(lambda: pl.nearest_order(X, X, k, skip=np.arange(n)))
    t_aff, (ro, cols, vals) = timed(lambda: pl.map_affinities(idx, dist, 30.0))
    vals = vals.astype(np.float32)
    t_init, Y0 = timed(lambda: pl.map_init(X))
    lr = max(n / 12.0 / 4.0, 50.0)
    lengths = np.diff(ro.astype(np.int64))
    case = {"n": n, "k": k, "nnz": int(len(cols)), "longest_row": int(lengths.max()), "rows_past_256": int((lengths > 256).sum()),
            "col_groups": pl.map_plan(n, torch.cuda.get_device_properties(0).multi_processor_count),
            "knn_ms": round(1e3 * t_knn, 1), "affinities_ms": round(1e3 * t_aff, 1), "init_ms": round(1e3 * t_init, 1)}

    def layout(n_iter):
        return pl.map_layout(Y0, ro, cols, vals, n_iter=n_iter, learning_rate=lr, **PARAMS)

    short, long_ = args.iters
    results = {}
    for feed in ("scalar", "lds"):
        os.environ["BLISSGPU_MAP_FEED"] = feed
        layout(2)
        per = []
        for _ in range(args.reps):
            per.append((timed(lambda: layout(long_))[0] - timed(lambda: layout(short))[0]) / (long_ - short))
        case[f"ms_per_iteration_{feed}"] = round(1e3 * statistics.median(per), 4)
        case[f"ms_per_iteration_{feed}_all"] = [round(1e3 * t, 4) for t in per]
        results[feed] = layout(short)
    del os.environ["BLISSGPU_MAP_FEED"]
    assert np.array_equal(results["scalar"][0].view(np.uint32), results["lds"][0].view(np.uint32)), "the two feeds disagree"
    # the kernels' own times (HIP events around every launch) over one short call of the shipped feed
    ctx = bliss.Context.default()
    ctx.profile_enable(True)
    ctx.profile_reset()
    layout(short)
    prof = {name: [round(v[0] / short, 4), int(v[1])] for name, v in ctx.profile().items() if name.startswith("map_")}
    ctx.profile_enable(False)
    case["kernel_ms_per_iteration"] = prof
    # the torch loop
    Yd = torch.from_numpy(Y0).cuda()
    row = torch.from_numpy(np.repeat(np.arange(n), lengths)).cuda()
    col = torch.from_numpy(cols.astype(np.int64)).cuda()
    val = torch.from_numpy(vals).cuda()
    torch_iterations(torch, Yd, row, col, val, 1, lr, args.block)
    per = [timed(lambda: torch_iterations(torch, Yd, row, col, val, args.torch_iters, lr, args.block))[0] / args.torch_iters
           for _ in range(args.reps)]
    case["ms_per_iteration_torch"] = round(1e3 * statistics.median(per), 3)
    case["ms_per_iteration_torch_all"] = [round(1e3 * t, 3) for t in per]
    # the whole layout
    t_all, (Y, trace) = timed(lambda: layout(750))
    case["layout_750_ms"] = round(1e3 * t_all, 1)
    case["z_first_last"] = [float(trace[0]), float(trace[-1])]
    print("CASE " + json.dumps(case), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="10000,100000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=lambda s: tuple(int(v) for v in s.split(",")), default=(10, 40),
                    help="the two call lengths whose difference gives the time per iteration")
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--block", type=int, default=2048, help="rows per block of the torch loop")
    ap.add_argument("--limit", type=int, default=420, help="seconds a case's child process may take")
    ap.add_argument("--case", type=int, help="(internal) run one case: n")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_bench.json"))
    args = ap.parse_args()
    if args.case:
        return one_case(args)
    out = {"d": 23, "perplexity": 30, "reps": args.reps, "block": args.block, "cases": []}
    for n in (int(v) for v in args.ns.split(",")):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--case", str(n), "--reps", str(args.reps),
               "--iters", f"{args.iters[0]},{args.iters[1]}", "--torch-iters", str(args.torch_iters), "--block", str(args.block)]
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
