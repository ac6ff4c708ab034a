"""The group neighbours on the device (blissgpu_group_neighbours_device) against what a user had before it: torch on the same
GPU -- the rows sorted by label, row blocks of torch.cdist in f32, a segment minimum per label-sorted column range
(torch.segment_reduce), the minima added per row group in f64 with index_add_, then the means and their symmetrisation in f64.
Same process, alternating, medians of `reps` after one warm-up of each.  Data: a seeded Gaussian mixture, d = 23, euclidean; the
groups have skewed sizes (a song's group is drawn with probability ~ (c + 1)^-0.7) and each its own centre around one of 32
mixture components; n in {10^4, 10^5}, K in {32 (genres), 3 000 (artists), 10^4 (albums)}.  Per (n, K): the size histogram, the
wall time of the call (t = 10, every group queried, no matrix) and of the torch route, the HIP-event times of the three chamfer_
kernels and of the sort from the context profiler, chamfer_scan_kernel's pairs per second, and beside it silhouette_scan_kernel's
at the same n and K (Context.silhouette in the same process: the same walk with an f64 sum per pair in the minimum's place), the
share of the kernels' time spent in chamfer_reduce_kernel (re-reading the slab of minima), the bytes of the slab, and
max |A - A_torch| over the pairs of non-empty groups.  torch's distances are not the all-pairs kernel's and its sums have no
order, so only times are compared; the difference is a sanity check.  `--slabs` records the kernels' times at forced slab sizes
as well (what the plan's choice is judged by).  Writes one JSON file.

    python tests/tools/group_neighbours_bench.py [--ns 10000,100000] [--ks 32,3000,10000] [--reps 3] [--out profiles/group_neighbours_bench.json]
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


def library(n, d, K, seed):
    """-> (X float32 [n, d], labels int64 [n]): skewed group sizes, a centre per group around one of 32 components"""
    rng = np.random.default_rng(seed)
    p = (np.arange(K) + 1.0) ** -0.7
    labels = rng.choice(K, n, p=p / p.sum())
    comps = rng.standard_normal((32, d)).astype(np.float32)
    centres = comps[rng.integers(0, 32, K)] + np.float32(0.4) * rng.standard_normal((K, d)).astype(np.float32)
    X = centres[labels] + np.float32(0.3) * rng.standard_normal((n, d)).astype(np.float32)
    return X.astype(np.float32), labels.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="10000,100000")
    ap.add_argument("--ks", default="32,3000,10000")
    ap.add_argument("--t", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--block", type=int, default=4096, help="rows per torch.cdist block of the baseline")
    ap.add_argument("--slabs", default="64,512", help="forced slab sizes whose kernel times are recorded too (where below K)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_neighbours_bench.json"))
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    assert torch.cuda.is_available(), "group_neighbours_bench measures on the GPU: there is no CPU path"
    d = 23
    ctx = bliss.Context(0)

    def sync():
        ctx.synchronize()
        torch.cuda.synchronize()

    def timed(f):
        sync()
        t0 = time.perf_counter()
        r = f()
        sync()
        return time.perf_counter() - t0, r

    def profiled(f):
        sync()
        ctx.profile_enable(True)
        ctx.profile_reset()
        f()
        sync()
        prof = {k: v for k, v in ctx.profile().items() if v[1]}
        ctx.profile_enable(False)
        return prof

    out = {"d": d, "t": args.t, "reps": args.reps, "device": torch.cuda.get_device_name(0), "workspace_limit": ctx.workspace_limit(),
           "cases": []}
    for n in (int(v) for v in args.ns.split(",")):
        for K in (int(v) for v in args.ks.split(",")):
            Xh, lab_h = library(n, d, K, 1)
            X = torch.from_numpy(Xh).cuda()
            labels = torch.from_numpy(lab_h.astype(np.int32)).cuda()
            lab64 = labels.to(torch.int64)
            sizes = torch.bincount(lab64, minlength=K)
            order = torch.argsort(lab64, stable=True)
            Xs, ls = X[order].contiguous(), lab64[order].contiguous()
            live = sizes > 0
            lengths = sizes[live]
            live_ids = torch.nonzero(live).reshape(-1)

            def new(slab=0, matrix=False):
                return ctx.group_neighbours(X, labels, K, args.t, "euclidean", None, None, "symmetric", slab, matrix)

            def baseline():
                T = torch.zeros((K, K), dtype=torch.float64, device=X.device)
                for i0 in range(0, n, args.block):
                    D = torch.cdist(Xs[i0:i0 + args.block], Xs)  # (torch's default: the matrix-multiply form, its fastest)
                    m = torch.segment_reduce(D.t().contiguous(), "min", lengths=lengths, axis=0)  # [non-empty groups, block]
                    Tl = torch.zeros((K, m.shape[0]), dtype=torch.float64, device=X.device)
                    Tl.index_add_(0, ls[i0:i0 + args.block], m.t().to(torch.float64))
                    T[:, live_ids] += Tl
                Dd = T / sizes.to(torch.float64).clamp(min=1)[:, None]
                A = (Dd + Dd.t()) * 0.5
                A[~live] = float("inf")
                A[:, ~live] = float("inf")
                A.fill_diagonal_(float("inf"))
                v, i = torch.topk(A, min(args.t, K - 1), dim=1, largest=False)
                return A, v, i

            def sil():
                return ctx.silhouette(X, labels, "euclidean", None, None, 0, K)

            new(), baseline(), sil()  # warm-up of everything timed (workspace growth, code objects)
            tn, tb = [], []
            for _ in range(args.reps):
                tn.append(timed(new)[0])
                tb.append(timed(baseline)[0])
            A_new = new(matrix=True)[3]
            A_ref = baseline()[0]
            ok = live[:, None] & live[None, :] & ~torch.eye(K, dtype=torch.bool, device=X.device)
            diff = float((A_new[ok] - A_ref[ok]).abs().max().item()) if bool(ok.any()) else 0.0
            del A_new, A_ref
            p, ps = profiled(new), profiled(sil)
            pairs = n * n
            scan, red, sel = (p.get(name, (0.0, 0))[0] for name in ("chamfer_scan_kernel", "chamfer_reduce_kernel", "chamfer_select_kernel"))
            total = sum(v[0] for v in p.values())
            sscan = ps["silhouette_scan_kernel"][0]
            slab_times = {}
            for slab in (int(v) for v in args.slabs.split(",") if v):
                if slab < K:
                    q = profiled(lambda: new(slab))
                    slab_times[slab] = {k: [round(v[0], 4), int(v[1])] for k, v in q.items() if k.startswith("chamfer_")}
            sz = sizes.cpu().numpy()
            hist = {f"{lo}..{2 * lo - 1}" if lo else "0": int(((sz >= lo) & (sz < max(2 * lo, 1))).sum())
                    for lo in [0] + [2 ** e for e in range(0, 15)] if ((sz >= lo) & (sz < max(2 * lo, 1))).any()}
            passes = int(p["chamfer_scan_kernel"][1])
            case = {
                "n": n, "K": K, "non_empty_groups": int(live.sum().item()), "largest_group": int(sz.max()),
                "largest_group_share": round(float(sz.max()) / n, 4), "group_size_histogram": hist,
                "wall_ms": round(1e3 * statistics.median(tn), 3), "wall_ms_torch": round(1e3 * statistics.median(tb), 3),
                "wall_ms_all": [round(1e3 * v, 3) for v in tn], "wall_ms_torch_all": [round(1e3 * v, 3) for v in tb],
                "passes": passes, "slab_groups": -(-K // passes), "slab_bytes_written_and_read": 4 * n * int(live.sum().item()),
                "chamfer_scan_kernel_ms": round(scan, 4), "chamfer_reduce_kernel_ms": round(red, 4), "chamfer_select_kernel_ms": round(sel, 4),
                "kernels_ms_total": round(total, 4), "reduce_share_of_kernels": round(red / total, 4),
                "chamfer_scan_gpairs_per_s": round(pairs / scan / 1e6, 2),
                "silhouette_scan_kernel_ms": round(sscan, 4), "silhouette_scan_gpairs_per_s": round(pairs / sscan / 1e6, 2),
                "kernel_ms": {k: [round(v[0], 4), int(v[1])] for k, v in p.items()},
                "chamfer_kernel_ms_by_slab": slab_times,
                "max_abs_A_minus_torch": diff,
            }
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
            del X, Xs
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
