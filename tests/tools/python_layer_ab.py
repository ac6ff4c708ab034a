"""Microseconds per call through the Python layer, for an A/B of two trees (profiles/python_layer_ab.json): 200 back-to-back
calls each of playlist.nearest_order, nearest_to_groups, chain_order and radio_order (n = 1000, d = 23, k = 8, 8 queries or
8 groups of 2 seeds: the shapes of profiles/host_layer_ab.json) and of Context.knn / Context.group_knn on resident tensors,
after 20 warm-up calls; the median of the 200 per-call times.  One JSON line.
  usage: python tests/tools/python_layer_ab.py [ROOT]   (ROOT: the tree to time, default: this one)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bliss_rs_amd  # noqa: E402
from bliss_rs_amd import playlist as P  # noqa: E402

CALLS, WARM = 200, 20


def median_us(fn, sync=None):
    for _ in range(WARM):
        fn()
    if sync:
        sync()
    t = np.empty(CALLS)
    for i in range(CALLS):
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        t[i] = time.perf_counter() - t0
    return round(float(np.median(t)) * 1e6, 2)


def main():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((1000, 23)).astype(np.float32)
    Q = X[:8].copy()
    S = X[:16].copy()
    groups = (S, np.arange(0, 17, 2))
    labels = (np.arange(1000) % 50)[None, :]
    out = {"tree": os.path.relpath(ROOT), "calls": CALLS}
    out["nearest_order"] = median_us(lambda: P.nearest_order(Q, X, 8))
    out["nearest_to_groups"] = median_us(lambda: P.nearest_to_groups(groups, X, 8))
    out["chain_order"] = median_us(lambda: P.chain_order(groups, X, 8))
    out["radio_order"] = median_us(lambda: P.radio_order(Q, X, 8, labels, [5], [1]))
    ctx = bliss_rs_amd.Context(0)
    Xd, Qd, Sd = (torch.from_numpy(a).cuda() for a in (X, Q, S))
    off = list(range(0, 17, 2))
    out["Context.knn"] = median_us(lambda: ctx.knn(Qd, Xd, 8), ctx.synchronize)
    out["Context.group_knn"] = median_us(lambda: ctx.group_knn(Sd, off, Xd, 8), ctx.synchronize)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
