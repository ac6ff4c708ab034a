"""One gradient evaluation of triplet metric learning on the device (blissgpu_triplet_step_device) against the route a user
has without it: torch float64 on the same device -- three row gathers, the three quadratic forms by einsum, the hinges, and G as
three weighted float64 matrix products -- same process, alternating, medians of `reps` after one warm-up of each.
Data: n = 10^6 seeded Gaussian rows, d = 23; T in {10^5, 10^6, 10^7} uniformly drawn triplets (about half of the hinges active);
M diagonal (the feature weights' shape) and full SPD.  One more case per M at T = 10^6 has the triplets labelled by M itself with
2 % of them flipped: late in a learning run most hinges are inactive and the kernel skips them.  Per case: wall ms per step of
both, HIP-event ms of triplet_step_kernel and triplet_reduce_kernel from the context profiler, active hinges.  The two routes
do not add in the same order; the results are compared in tests/test_gpu_metric.py, here only n_active (equal unless a hinge
sits within rounding of 0) and the relative difference of G are recorded.  A last section times
blissgpu_learn_metric_device itself: 20 updates at T = 10^6, wall per iteration.  Writes one JSON file.

    python tests/tools/metric_bench.py [--n 1000000] [--ts 100000,1000000,10000000] [--reps 3] [--out profiles/metric_bench.json]
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
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--ts", default="100000,1000000,10000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--margin", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metric_bench.json"))
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    assert torch.cuda.is_available(), "metric_bench measures on the GPU: there is no CPU path"
    d, n = 23, args.n
    ctx = bliss.Context(0)
    rng = np.random.default_rng(1)
    X = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).cuda()
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    mats = {"diagonal": np.diag(np.exp(rng.normal(0.0, 1.0, d))).astype(np.float32), "full": (A @ A.T + 0.05 * np.eye(d)).astype(np.float32)}

    def sync():
        ctx.synchronize()
        torch.cuda.synchronize()

    def timed(f):
        sync()
        t0 = time.perf_counter()
        r = f()
        sync()
        return time.perf_counter() - t0, r

    def route(tr, M, margin):
        """what a user writes today: float64 torch"""
        Xd = X  # gathered rows are widened, not the whole matrix
        a, b, o = (Xd[tr[:, k].long()].double() for k in range(3))
        u, v, w = a - b, a - o, b - o
        Md = M.double()
        qu, qv, qw = (torch.einsum("ti,ij,tj->t", t, Md, t) for t in (u, v, w))
        h1, h2 = margin + qu - qv, margin + qu - qw
        f1, f2 = (h1 > 0).double(), (h2 > 0).double()
        G = (u * (f1 + f2)[:, None]).T @ u - (v * f1[:, None]).T @ v - (w * f2[:, None]).T @ w
        loss = (h1 * f1).sum() + (h2 * f2).sum()
        return int((f1.sum() + f2.sum()).item()), float(loss.item()), G.cpu().numpy()

    def labelled(tr, M, flip):
        a, b, o = (X[tr[:, k].long()].double() for k in range(3))
        Md = M.double()
        q = lambda t: torch.einsum("ti,ij,tj->t", t, Md, t)  # noqa: E731
        d01, d02, d12 = q(a - b), q(a - o), q(b - o)
        out = tr.clone()
        m02 = (d02 < d01) & (d02 <= d12)
        m12 = (d12 < d01) & (d12 < d02)
        out[m02] = tr[m02][:, [0, 2, 1]]
        out[m12] = tr[m12][:, [1, 2, 0]]
        sel = torch.rand(tr.shape[0], device=tr.device) < flip
        out[sel] = out[sel][:, [0, 2, 1]]
        return out.contiguous()

    out = {"n": n, "d": d, "reps": args.reps, "margin": args.margin, "device": torch.cuda.get_device_name(0), "cases": []}
    torch.manual_seed(0)
    cases = [(T, kind, "uniform") for T in (int(v) for v in args.ts.split(",")) for kind in mats]
    cases += [(1000000, kind, "labelled, 2 % flipped") for kind in mats]
    for T, kind, draw in cases:
        M = torch.from_numpy(mats[kind]).cuda()
        tr = torch.from_numpy(rng.integers(0, n, (T, 3)).astype(np.int32)).cuda()
        margin = args.margin
        if draw != "uniform":
            tr, margin = labelled(tr, M, 0.02), 0.0
        new = lambda: ctx.triplet_step(X, tr, M, margin)  # noqa: E731
        old = lambda: route(tr, M, margin)  # noqa: E731
        r_new, r_old = new(), old()  # warm-up of both (workspace growth, code objects, the allocator's cache)
        t_new, t_old = [], []
        for _ in range(args.reps):
            t_new.append(timed(new)[0])
            t_old.append(timed(old)[0])
        sync()
        ctx.profile_enable(True)
        ctx.profile_reset()
        new()
        sync()
        prof = ctx.profile()
        ctx.profile_enable(False)
        scale = float(np.abs(r_old[2]).max())
        case = {
            "T": T, "M": kind, "triplets": draw, "n_active": r_new[0], "active_share": round(r_new[0] / (2.0 * T), 4),
            "n_active_torch": r_old[0],
            "new_wall_ms": round(1e3 * statistics.median(t_new), 4), "torch_f64_wall_ms": round(1e3 * statistics.median(t_old), 4),
            "speedup": round(statistics.median(t_old) / statistics.median(t_new), 2),
            "new_wall_ms_all": [round(1e3 * t, 4) for t in t_new], "torch_f64_wall_ms_all": [round(1e3 * t, 4) for t in t_old],
            "kernel_ms": {k: round(v[0] / max(v[1], 1), 4) for k, v in prof.items()},
            "G_max_rel_diff_to_torch": float(np.abs(r_new[2] - r_old[2]).max() / scale) if scale else 0.0,
            "loss_rel_diff_to_torch": abs(r_new[1] - r_old[1]) / abs(r_old[1]) if r_old[1] else 0.0,
        }
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
        del tr
        torch.cuda.empty_cache()
    # the loop: 20 updates at T = 10^6 (uniform triplets: they contradict each other, the run goes to max_iter), wall per iteration
    out["loops"] = []
    tr = torch.from_numpy(rng.integers(0, n, (1000000, 3)).astype(np.int32)).cuda()
    for form in ("diagonal", "full"):
        run = lambda: ctx.learn_metric(X, tr, form=form, margin=args.margin, lr=0.01, max_iter=20)  # noqa: E731
        run()
        dt, res = timed(run)
        loop = {"T": 1000000, "form": form, "n_iter": res.n_iter, "status": res.status, "wall_ms_per_iteration": round(1e3 * dt / (res.n_iter + 1), 4),
                "copies_up_down_bytes": list(ctx.metric_stats())}
        print(json.dumps(loop), flush=True)
        out["loops"].append(loop)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
