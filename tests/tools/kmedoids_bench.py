"""k-medoids on the device (blissgpu_pam_scan / blissgpu_kmedoids) against what a user had before it: a torch loop of the same
rounds on the same GPU -- row blocks of torch.cdist (or, for the cosine, of the normalised matrix product) in f32, the two terms
in f64, index_add_ per slot, the minimum over the slots; the state by cdist against the medoids and topk.  Same process,
alternating, medians of `reps` after one warm-up of each.  Data: the seeded 32-component Gaussian mixture of
tests/tools/silhouette_bench.py, d = 23, K = 32; n in {10^4, 10^5}; euclidean and cosine.  Per case: ONE scan under the state of
32 sampled medoids (wall time of the host-pointer call, pam_scan_kernel's HIP-event time from the context profiler, the pairs per
second it reaches, and beside it silhouette_scan_kernel's at the same n, K and -- for euclidean -- labels, as
tests/tools/silhouette_bench.py measures it), and the WHOLE clustering from BUILD (wall time, swaps, scans, every kernel's time).
torch's sums are not the contract's (cdist is not the all-pairs kernel's distance, index_add_ has no order), so only times are
compared; whether its medoids are the device's and the relative difference of TD are recorded as a sanity check.  Writes one
JSON file.

    python tests/tools/kmedoids_bench.py [--ns 10000,100000] [--k 32] [--reps 3] [--out profiles/kmedoids_bench.json]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from silhouette_bench import mixture  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="10000,100000")
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--block", type=int, default=8192, help="rows per block of the torch baseline")
    ap.add_argument("--metrics", default="euclidean,cosine")
    ap.add_argument("--torch-full-max", type=int, default=10000,
                    help="the largest n at which the torch loop runs the WHOLE clustering (64 times the scans' time per decade of n: "
                         "ten minutes a run at 10^5); above it the loop is priced as its measured scan and state times the scans")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmedoids_bench.json"))
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    assert torch.cuda.is_available(), "kmedoids_bench measures on the GPU: there is no CPU path"
    P = bliss.playlist
    d, K = 23, args.k
    ctx = bliss.Context.default()  # the host-pointer forms run on it
    dev = torch.device("cuda")

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
        r = f()
        sync()
        prof = {name: v for name, v in ctx.profile().items() if v[1]}
        ctx.profile_enable(False)
        return prof, r

    def ms(ts):
        return round(1e3 * statistics.median(ts), 3)

    out = {"d": d, "K": K, "reps": args.reps, "device": torch.cuda.get_device_name(0), "cases": []}
    for n in (int(v) for v in args.ns.split(",")):
        Xh = mixture(n, d, 1)
        X = torch.from_numpy(Xh).to(dev)
        med0 = np.sort(np.random.default_rng(2).choice(n, K, replace=False))
        for metric in args.metrics.split(","):
            builder = P.euclidean_distance if metric == "euclidean" else P.cosine_distance
            Xn = X / X.norm(dim=1, keepdim=True) if metric == "cosine" else None

            def block_dist(j0, j1, cols=None):
                """f32 distances of songs j0 .. j1 to the songs `cols` (None: all)"""
                if metric == "cosine":
                    return 1.0 - Xn[j0:j1] @ (Xn if cols is None else Xn[cols]).T
                return torch.cdist(X[j0:j1], X if cols is None else X[cols])

            def torch_state(med):
                D = torch.cat([block_dist(j0, min(j0 + args.block, n), med) for j0 in range(0, n, args.block)])
                two = torch.topk(D, min(2, D.shape[1]), dim=1, largest=False)
                d1 = two.values[:, 0].contiguous()
                d2 = two.values[:, 1].contiguous() if D.shape[1] > 1 else torch.full_like(d1, float("inf"))
                return two.indices[:, 0], d1, d2, d1.double().sum()

            def torch_scan(near, d1, d2, k):
                """-> btot, best, arg [n] of every candidate"""
                d1d = d1.double()
                btot, best, arg = [], [], []
                for j0 in range(0, n, args.block):
                    D = block_dist(j0, min(j0 + args.block, n))
                    A = torch.zeros((D.shape[0], k), dtype=torch.float64, device=dev)
                    B = torch.zeros_like(A)
                    A.index_add_(1, near, torch.minimum(D, d2).double() - d1d)
                    B.index_add_(1, near, (D.double() - d1d).clamp(max=0.0))
                    bt = B.sum(dim=1)
                    m = ((bt[:, None] - B) + A).min(dim=1)
                    btot.append(bt), best.append(m.values), arg.append(m.indices)
                return torch.cat(btot), torch.cat(best), torch.cat(arg)

            def torch_kmedoids(rounds_cap):
                """BUILD and the rounds, every scan by torch_scan; at most rounds_cap rounds (the device's count)"""
                sums = torch.cat([block_dist(j0, min(j0 + args.block, n)).double().sum(dim=1) for j0 in range(0, n, args.block)])
                med = [int(sums.argmin())]
                while len(med) < K:
                    near, d1, d2, _ = torch_state(torch.tensor(med, device=dev))
                    btot = torch_scan(near, d1, d2, len(med))[0]
                    btot[torch.tensor(med, device=dev)] = float("inf")
                    med.append(int(btot.argmin()))
                td, swaps = None, 0
                for _ in range(rounds_cap):
                    near, d1, d2, td = torch_state(torch.tensor(med, device=dev))
                    _, best, arg = torch_scan(near, d1, d2, K)
                    best[torch.tensor(med, device=dev)] = float("inf")
                    c = int(best.argmin())
                    if not float(best[c]) < 0:
                        break
                    med[int(arg[c])] = c
                    swaps += 1
                return med, float(td), swaps

            # one scan under the state of K sampled medoids
            idx, dist = P.nearest_order(Xh, Xh[med0], 2, metric)
            near_h, d1_h, d2_h = idx[:, 0].copy(), dist[:, 0].copy(), dist[:, 1].copy()
            near_t, d1_t, d2_t = torch.from_numpy(near_h).to(dev), torch.from_numpy(d1_h).to(dev), torch.from_numpy(d2_h).to(dev)
            scan_new = lambda: P.pam_scan(Xh, near_h, d1_h, d2_h, K, builder)  # noqa: E731
            scan_ref = lambda: torch_scan(near_t, d1_t, d2_t, K)  # noqa: E731
            got, ref = scan_new(), scan_ref()  # warm-up of both (workspace growth, code objects)
            t_new, t_ref = [], []
            for _ in range(args.reps):
                t_new.append(timed(scan_new)[0])
                t_ref.append(timed(scan_ref)[0])
            prof_scan = profiled(scan_new)[0]
            scan_ms = prof_scan["pam_scan_kernel"][0]
            case = {"n": n, "K": K, "metric": metric, "scan_wall_ms": ms(t_new), "scan_wall_ms_torch": ms(t_ref),
                    "scan_wall_ms_all": [round(1e3 * t, 3) for t in t_new], "scan_wall_ms_torch_all": [round(1e3 * t, 3) for t in t_ref],
                    "pam_scan_kernel_ms": round(scan_ms, 4), "pam_scan_gpairs_per_s": round(n * n / scan_ms / 1e6, 2),
                    "scan_kernel_ms": {k: [round(v[0], 4), int(v[1])] for k, v in prof_scan.items()},
                    "scan_max_rel_best_minus_torch": float(((torch.from_numpy(got[1]).to(dev) - ref[1]).abs().max() / ref[1].abs().max()).item())}
            if metric == "euclidean":  # the silhouette refuses the cosine
                sil = profiled(lambda: P.silhouette(Xh, near_h))[0]["silhouette_scan_kernel"][0]
                case["silhouette_scan_kernel_ms"] = round(sil, 4)
                case["silhouette_scan_gpairs_per_s"] = round(n * n / sil / 1e6, 2)
            # the whole clustering from BUILD
            res = P.kmedoids(Xh, K, builder)
            rounds = res.n_swaps + 1
            full = n <= args.torch_full_max
            if full:
                torch_kmedoids(rounds)
            t_new, t_ref, ref_run = [], [], None
            for _ in range(args.reps):
                t_new.append(timed(lambda: P.kmedoids(Xh, K, builder))[0])
                if full:
                    dt, ref_run = timed(lambda: torch_kmedoids(rounds))
                    t_ref.append(dt)
            prof_all = profiled(lambda: P.kmedoids(Xh, K, builder))[0]
            case.update({"swaps": res.n_swaps, "rounds": rounds, "converged": res.converged, "scans": K + rounds, "td": res.td,
                         "kmedoids_wall_ms": ms(t_new), "kmedoids_wall_ms_all": [round(1e3 * t, 3) for t in t_new],
                         "kmedoids_kernel_ms": {k: [round(v[0], 4), int(v[1])] for k, v in prof_all.items()}})
            if full:
                case.update({"kmedoids_wall_ms_torch": ms(t_ref), "kmedoids_wall_ms_torch_all": [round(1e3 * t, 3) for t in t_ref],
                             "torch_medoids_are_the_devices": sorted(ref_run[0]) == sorted(res.medoids.tolist()), "torch_swaps": ref_run[2],
                             "torch_td_rel_diff": abs(ref_run[1] - res.td) / res.td})
            else:  # not measured: the scans and states of the same rounds at the torch route's measured times
                med_t = torch.from_numpy(med0).to(dev)
                torch_state(med_t)
                t_state = statistics.median(timed(lambda: torch_state(med_t))[0] for _ in range(args.reps))
                case["torch_state_wall_ms"] = round(1e3 * t_state, 3)
                case["kmedoids_ms_torch_priced_not_measured"] = round((K + rounds) * (case["scan_wall_ms_torch"] + 1e3 * t_state), 1)
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
        del X
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
