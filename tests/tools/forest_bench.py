"""Isolation-forest scoring (blissgpu_forest_score_device / blissgpu_forest_closest_to_songs_device: forest_walk_kernel +
forest_finish_kernel, then the radix sort) for n candidates in {10^4, 10^5, 10^6} x (psi, trees, extension_level) in
{(3, 1000, 10), (16, 1000, 10), (256, 100, 0), (256, 1000, 22)}, d = 23, seeds = psi rows.  Per case, medians of `reps` after
a warm-up: wall ms per call (host timer around a synchronised call) of the score alone and of score + order, the HIP-event
time of the two kernels from the context profiler, candidate-tree walks per second from the walk kernel's time -- for the
default launch and for the measurement forms (every tree walked from global memory; the trees never split over workgroups).
Beside each line two yardsticks that are not the code under test:
  (1) Context.closest_to_songs (euclidean, same n, same number of seeds): what a multi-seed playlist costs without the forest;
  (2) tests/tools/forest_walk_ref.cpp, compiled -O3 here: a one-thread and a 16-thread C++ walk of the exported forest over the
      first `--cpu-rows` candidates (walks per second; ms for all n extrapolated), whose sums must equal the device's.
Writes one JSON file.

    python tests/tools/forest_bench.py [--ns 10000,100000,1000000] [--reps 3] [--out profiles/forest_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
CASES = [(3, 1000, 10), (16, 1000, 10), (256, 100, 0), (256, 1000, 22)]


def cpu_walker(tmp):
    so = os.path.join(tmp, "libforest_walk_ref.so")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O3", "-std=c++17", "-shared", "-fPIC", "-pthread",
                           os.path.join(ROOT, "tests", "tools", "forest_walk_ref.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.forest_walk_ref.restype = None
    lib.forest_walk_ref.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32] + [C.c_void_p] * 6 + [C.c_uint32, C.c_void_p]
    return lib.forest_walk_ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="10000,100000,1000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-rows", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_bench.json"))
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    d = 23
    ctx = bliss.Context(0)
    tmp = tempfile.mkdtemp()
    walk_ref = cpu_walker(tmp)

    def sync():
        ctx.synchronize()
        torch.cuda.synchronize()

    def wall_ms(f):
        f()
        sync()
        ts = []
        for _ in range(args.reps):
            sync()
            t0 = time.perf_counter()
            f()
            sync()
            ts.append(time.perf_counter() - t0)
        return round(statistics.median(ts) * 1e3, 3)

    def kernel_ms(f):
        """medians of the HIP-event times of the forest kernels over `reps` profiled calls"""
        per = {}
        for _ in range(args.reps):
            sync()
            ctx.profile_enable(True)
            ctx.profile_reset()
            f()
            sync()
            for k, v in ctx.profile().items():
                if k.startswith("forest_") and v[1]:
                    per.setdefault(k, []).append(v[0])
            ctx.profile_enable(False)
        return {k: round(statistics.median(v), 4) for k, v in per.items()}

    out = {"d": d, "reps": args.reps, "device": torch.cuda.get_device_name(0), "cpu_rows": args.cpu_rows, "cases": []}
    rng = np.random.default_rng(1)
    for n in [int(v) for v in args.ns.split(",")]:
        X = rng.uniform(-1, 1, (n, d)).astype(np.float32)
        tX = torch.from_numpy(X).cuda()
        for psi, trees, ext in CASES:
            S = rng.uniform(-1, 1, (psi, d)).astype(np.float32)
            tS = torch.from_numpy(S).cuda()
            f = bliss.playlist.Forest(S, bliss.playlist.ForestOptions(trees, psi, None, ext, seed=1))
            row = {"n": n, "psi": psi, "trees": trees, "extension_level": ext, "nodes": f.n_nodes, "depth_limit": f.depth_limit}
            forms = {"default": (0, 0), "global_walk": (0, 1), "no_tree_split": (1, 0)}
            for name, (split, walk) in forms.items():
                ctx.set_option("forest_split", split)
                ctx.set_option("forest_walk", walk)
                k = kernel_ms(lambda: ctx.forest_scores(f, tX))
                row[name] = {"score_wall_ms": wall_ms(lambda: ctx.forest_scores(f, tX)), "kernels_ms": k,
                             "walks_per_s": round(n * trees / (k["forest_walk_kernel"] * 1e-3), 0)}
            ctx.set_option("forest_split", 0)
            ctx.set_option("forest_walk", 0)
            row["score_and_order_wall_ms"] = wall_ms(lambda: ctx.forest_closest_to_songs(f, tX))
            row["euclidean_closest_to_songs_wall_ms"] = wall_ms(lambda: ctx.closest_to_songs(tS, tX, "euclidean"))
            _, ps = ctx.forest_scores(f, tX, return_path_sum=True)
            sync()
            ps = ps.cpu().numpy().view(np.uint64)
            ex = f.export()
            m = min(n, args.cpu_rows)
            for threads in (1, 16):
                got = np.zeros(m, np.uint64)
                t0 = time.perf_counter()
                walk_ref(X.ctypes.data, m, d, trees, *[ex[k].ctypes.data for k in ("tree_first", "normal", "b", "left", "right",
                                                                                  "leaf_q")], threads, got.ctypes.data)
                dt = time.perf_counter() - t0
                assert np.array_equal(got, ps[:m]), "the CPU walk and the device disagree"
                row[f"cpu_{threads}_thread"] = {"walks_per_s": round(m * trees / dt, 0), "ms_for_n_extrapolated": round(dt * 1e3 * n / m, 1)}
            f.close()
            print(json.dumps(row), flush=True)
            out["cases"].append(row)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
