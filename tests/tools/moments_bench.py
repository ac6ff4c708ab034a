"""The moments of a library on the device (blissgpu_moments_device: counts, means, m2, extrema and the pooled scatter matrix,
every f64 sum in the contract's blocked order) against what a user had before it: torch float64 on the same GPU -- X.double(),
index_add_ for the group sums and the squared deviations (without labels: mean and sum over the rows), U.T @ U for the scatter
(no extrema).  Same process, alternating,
medians of `reps` after one warm-up of each.  Data: seeded standard normal rows times per-feature scales, d = 23, uniformly
drawn labels; n in {10^5, 10^6, 10^7} x K in {1, 32, 4096} (K = 1 runs without labels: no sort).  Per case: the wall times, every
kernel's HIP-event time from the context profiler, and for the three kernels that read x (moments_sum_kernel, moments_m2_kernel,
moments_scatter_kernel) the bytes of x they read per second beside the HBM read rate DESIGN.md measures kernels against
(5.95 TB/s, probes/bw_probe).  torch's sums are not the contract's (index_add_ and the matrix product have no fixed order), so
only times are compared; the largest relative difference of S is recorded as a sanity value.  No threshold is fixed here.
Writes one JSON file.

    python tests/tools/moments_bench.py [--ns 100000,1000000,10000000] [--ks 1,32,4096] [--reps 5] [--out profiles/moments_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HBM_READ_TB_S = 5.95  # the rate a load-only loop reaches on this device (probes/bw_probe)
X_READERS = ("moments_sum_kernel", "moments_m2_kernel", "moments_scatter_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="100000,1000000,10000000")
    ap.add_argument("--ks", default="1,32,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments_bench.json"))
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    assert torch.cuda.is_available(), "moments_bench measures on the GPU: there is no CPU path"
    d = 23
    ctx = bliss.Context(0)
    dev = torch.device("cuda", 0)

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
        prof = ctx.profile()
        ctx.profile_enable(False)
        return prof

    out = {"d": d, "reps": args.reps, "device": torch.cuda.get_device_name(0), "hbm_read_tb_per_s": HBM_READ_TB_S, "cases": []}
    for n in (int(v) for v in args.ns.split(",")):
        gen = torch.Generator(device=dev)
        gen.manual_seed(n)
        scales = torch.logspace(-1, 1, d, device=dev, dtype=torch.float32)
        X = torch.randn((n, d), generator=gen, device=dev, dtype=torch.float32) * scales
        X[:, 2] += 100.0
        x_bytes = n * d * 4
        for K in (int(v) for v in args.ks.split(",")):
            labels = None if K == 1 else torch.randint(0, K, (n,), generator=gen, device=dev, dtype=torch.int32)
            lab64 = torch.zeros((n,), dtype=torch.int64, device=dev) if labels is None else labels.to(torch.int64)

            def new(scatter=True):
                return ctx.moments(X, labels, K, scatter)

            def baseline():
                Xd = X.double()
                counts = torch.bincount(lab64, minlength=K).to(torch.float64)
                if labels is None:  # (what one writes without labels; index_add_ into one row takes seconds: its adds collide)
                    mean = Xd.mean(dim=0, keepdim=True)
                else:
                    mean = torch.zeros((K, d), dtype=torch.float64, device=dev).index_add_(0, lab64, Xd) / counts.clamp(min=1)[:, None]
                U = Xd - mean[lab64]
                m2 = (U * U).sum(dim=0, keepdim=True) if labels is None else torch.zeros((K, d), dtype=torch.float64, device=dev).index_add_(
                    0, lab64, U * U)
                return counts, mean, m2, U.T @ U

            new(), new(False), baseline()  # warm-up of everything timed (workspace growth, code objects)
            t_new, t_nos, t_ref = [], [], []
            for _ in range(args.reps):
                t_new.append(timed(new)[0])
                t_nos.append(timed(lambda: new(False))[0])
                t_ref.append(timed(baseline)[0])
            S_new, S_ref = new()[5], baseline()[3]
            prof = profiled(new)
            kernels = {k: [round(v[0], 4), int(v[1])] for k, v in prof.items() if v[1]}
            case = {
                "n": n, "K": K, "x_mbytes": round(x_bytes / 1e6, 1),
                "wall_ms": round(1e3 * statistics.median(t_new), 3), "wall_ms_without_scatter": round(1e3 * statistics.median(t_nos), 3),
                "wall_ms_torch": round(1e3 * statistics.median(t_ref), 3),
                "wall_ms_all": [round(1e3 * t, 3) for t in t_new], "wall_ms_without_scatter_all": [round(1e3 * t, 3) for t in t_nos],
                "wall_ms_torch_all": [round(1e3 * t, 3) for t in t_ref],
                "kernel_ms": kernels,
                "kernel_ms_total": round(sum(v[0] for v in kernels.values()), 4),
                "x_tb_per_s": {k: round(x_bytes / (prof[k][0] * 1e-3) / 1e12, 3) for k in X_READERS if k in prof and prof[k][0] > 0},
                "share_of_hbm_read_rate": {k: round(x_bytes / (prof[k][0] * 1e-3) / 1e12 / HBM_READ_TB_S, 3) for k in X_READERS
                                           if k in prof and prof[k][0] > 0},
                "max_rel_S_minus_torch": float(((S_new - S_ref).abs().max() / S_ref.abs().max()).item()),
            }
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
            del labels, lab64
        del X
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
