"""What the Python layer hands to the C ABI, recorded without a device: a stand-in for the loaded library records, for every
call, the function and per argument its scalar value, "ptr" or None (by the declared argtype), and returns BLISSGPU_OK.  The
host entry points of playlist.py, song.analyze_batch and song.fingerprint_batch are driven on 12 rows, d = 23, k = 3, groups
of 1, 2 and 4 seeds, every optional argument given once and left out once.  Two trees marshal alike when the two records
are equal (profiles/python_layer_calls.txt).  device.Node and the methods of device.Context that touch no tensor are driven too
(a Context made without its constructor, which needs a device).  --arrays adds, for a tree that has _ffi.call, one line per
array argument as call sees it: position, dtype, shape and the first bytes; those lines begin with "   array".
  usage: python tests/tools/python_layer_record.py [--arrays] [ROOT]   (ROOT: the tree to read, default: this one)"""
import ctypes as C
import os
import sys

import numpy as np

ARRAYS = "--arrays" in sys.argv
sys.argv = [a for a in sys.argv if a != "--arrays"]
ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bliss_rs_amd  # noqa: E402,F401
from bliss_rs_amd import _ffi, device, playlist as P, song  # noqa: E402

RECORD = []


class Recorder:
    def __getattr__(self, name):
        if name not in _ffi.SIGNATURES:
            raise AttributeError(name)
        restype, argtypes = _ffi.SIGNATURES[name]

        def fn(*args):
            row = []
            for a, t in zip(args, argtypes):
                pointer = t is C.c_void_p or hasattr(t, "contents") or issubclass(t, C._Pointer)
                if not pointer:
                    row.append(round(float(a), 6) if isinstance(a, (float, np.floating)) else int(a))
                else:
                    null = a is None or (isinstance(a, int) and a == 0) or (isinstance(a, C.c_void_p) and not a.value)
                    row.append(None if null else "ptr")
            RECORD.append(f"{name} {row}")
            return b"" if restype is C.c_char_p else 0

        return fn


def drive(label, fn):
    RECORD.append(f"-- {label}")
    try:
        fn()
    except Exception as e:  # (the stand-in fills no output: what the wrapper makes of zeros is part of the record)
        RECORD.append(f"   raised {type(e).__name__}: {e}"[:160])


def note_arrays():
    """wrap _ffi._arguments: what call sees of every array argument, written before the call's own line"""
    inner = _ffi._arguments

    def arguments(name, args, argtypes):
        for pos, a in enumerate(args):
            if isinstance(a, np.ndarray):
                RECORD.append(f"   array {name}[{pos}] {a.dtype} {list(a.shape)} {a.tobytes()[:8].hex()}")
        return inner(name, args, argtypes)

    _ffi._arguments = arguments


def drive_device():
    """device.Node, and the methods of device.Context that take no tensor"""
    node = device.Node(2, [0, 0])
    lengths = [9000, 30000, 8192]
    drive("Node.shard", lambda: node.shard(lengths))
    drive("Node.row_block", lambda: node.row_block(10, 1))
    drive("Node.synth_white_noise", lambda: node.synth_white_noise(1, 4096, [0, 9000], [9000, 100], [3, 4]))
    drive("Node.ctx_set_workspace_limit", lambda: node.ctx_set_workspace_limit(0, 1 << 20))
    drive("Node.analyze", lambda: node.analyze(np.zeros(47192, np.float64), [0, 9000, 39000], lengths))
    drive("Node.analyze_device", lambda: node.analyze_device([4096, 8192], [0, 9000, 0], lengths, [0, 0, 1], 1))
    drive("Node.features", lambda: node.features(1))
    for m in (None, np.eye(20)):
        drive(f"Node.pairwise m={m is not None}", lambda: node.pairwise("euclidean" if m is None else "mahalanobis", m))
    ctx = object.__new__(device.Context)  # (the constructor needs a device; these methods need the handle only)
    ctx._L, ctx._h, ctx._borrowed, ctx.device = _ffi.lib(), C.c_void_p(1), True, 0
    for label, fn in (("staged_bytes", ctx.staged_bytes), ("synchronize", ctx.synchronize),
                      ("set_option", lambda: ctx.set_option("cand_budget", 7)), ("set_workspace_limit", lambda: ctx.set_workspace_limit(1 << 20)),
                      ("workspace_limit", ctx.workspace_limit), ("last_chunks", ctx.last_chunks), ("last_tuning", lambda: ctx.last_tuning(3)),
                      ("debug_fetch_raw", lambda: ctx.debug_fetch_raw("chroma", 2)), ("flac_slow_songs", ctx.flac_slow_songs),
                      ("kmeans_stats", ctx.kmeans_stats), ("metric_stats", ctx.metric_stats), ("group_forest_stats", ctx.group_forest_stats),
                      ("profile_enable", lambda: ctx.profile_enable(True)), ("profile_reset", ctx.profile_reset), ("profile", ctx.profile)):
        drive(f"Context.{label}", fn)


def main():
    _ffi._lib = Recorder()
    if ARRAYS and hasattr(_ffi, "_arguments"):
        note_arrays()
    rng = np.random.default_rng(36)
    X = rng.standard_normal((12, 23)).astype(np.float32)
    M = np.eye(23, dtype=np.float32)
    groups = [X[0:1], X[1:3], X[3:7]]
    lab = np.arange(12) % 3
    skip_q = np.array([0, -1, 2], np.int64)
    flat_skip = np.array([-1, 1, -1, 3, -1, -1, 5], np.int64)
    skip2 = np.array([[0, -1], [1, 2], [-1, -1]], np.int64)
    scale = np.ones(12, np.float32)
    for m in (None, M):
        metric = "euclidean" if m is None else "mahalanobis"
        builder = P.euclidean_distance if m is None else P.MahalanobisBuilder(M)
        tag = metric
        drive(f"distance {tag}", lambda: P._single(X[0], X[1], P._METRICS[metric], m))
        drive(f"pairwise_distances {tag}", lambda: P.pairwise_distances(X[:3], X, metric, m))
        drive(f"set_distances {tag}", lambda: P.set_distances(X[3:7], X, metric, m))
        drive(f"closest_to_songs_order {tag}", lambda: P.closest_to_songs_order(X[3:7], X, metric, m))
        drive(f"song_to_song_order {tag}", lambda: P.song_to_song_order(X[3:7], X, metric, m))
        drive(f"song_to_song_order k {tag}", lambda: P.song_to_song_order(X[3:7], X, metric, m, k=3))
        for skip in (None, skip_q):
            drive(f"nearest_order {tag} skip={skip is not None}", lambda: P.nearest_order(X[:3], X, 3, metric, m, skip))
            drive(f"scaled_nearest_order {tag} skip={skip is not None}",
                  lambda: P.scaled_nearest_order(X[:3], scale[:3], X, scale, 3, metric, m, skip))
        for skip in (None, flat_skip):
            drive(f"nearest_to_groups {tag} skip={skip is not None}", lambda: P.nearest_to_groups(groups, X, 3, metric, m, skip))
            drive(f"chain_order {tag} skip={skip is not None}", lambda: P.chain_order(groups, X, 3, metric, m, skip))
            drive(f"nearest_albums skip={skip is not None}", lambda: P.nearest_albums(groups, X, np.arange(12) % 4, 3, skip))
        drive(f"chain_order lists {tag}", lambda: P.chain_order(groups, X, 3, metric, m, None, "lists"))
        for skip in (None, skip2):
            drive(f"journey_order waypoint {tag} skip={skip is not None}", lambda: P.journey_order(X[:3], X, 3, X[3:6], metric, m, skip))
            drive(f"journey_order down {tag} skip={skip is not None}",
                  lambda: P.journey_order(X[:3], X, 3, None, metric, m, skip, "down", 0))
            drive(f"radio_order {tag} skip={skip is not None}",
                  lambda: P.radio_order(X[:3], X, 3, (np.arange(12) % 5)[None, :], [2], [1], None, "chain", metric, m, skip))
        drive(f"radio_order from_labels nearest {tag}",
              lambda: P.radio_order(X[:3], X, 3, (np.arange(12) % 5)[None, :], [2], [1], [[0], [1], [-1]], "nearest", metric, m))
        drive(f"radio_order no rules {tag}", lambda: P.radio_order(X[:3], X, 3, None, [], [], None, "chain", metric, m))
        drive(f"kmeans {tag}", lambda: P.kmeans(X, X[:3], 10, metric, m))
        for rows in (None, [0, 5, 5]):
            drive(f"silhouette {tag} rows={rows is not None}", lambda: P.silhouette(X, lab, builder, rows))
            drive(f"pam_scan {tag} rows={rows is not None}",
                  lambda: P.pam_scan(X, lab, np.ones(12), np.ones(12) * 2, 3, builder, rows, return_sums=rows is not None))
        for q in (None, [2, 0]):
            drive(f"group_neighbours {tag} queries={q is not None}",
                  lambda: P.group_neighbours(X, lab, 2, builder, None, q, "symmetric" if q is None else "directed", q is not None))
        for ms in (None, 2):
            drive(f"minimum_spanning_tree {tag} min_samples={ms}", lambda: P.minimum_spanning_tree(X, builder, ms))
        drive(f"ward_tree {tag}", lambda: P.ward_tree(X, builder))
        for sizes in (None, np.arange(1, 13)):
            drive(f"ward_nearest {tag} sizes={sizes is not None}", lambda: P.ward_nearest(X, sizes, builder))
        for init in ("build", [0, 4, 8]):
            drive(f"kmedoids {tag} init={init}", lambda: P.kmedoids(X, 3, builder, init))
        for meta in (None, np.arange(12) % 2):
            drive(f"dedup_order {tag} meta={meta is not None}", lambda: P.dedup_order(X, None if meta is None else np.arange(6), meta, metric, m))
            drive(f"duplicate_labels {tag} meta={meta is not None}", lambda: P.duplicate_labels(X, meta, metric, m, None, meta is not None))
        drive(f"triplet_step {tag}", lambda: P.triplet_step(X, [[0, 1, 2], [3, 4, 5]], m, 0.1, m is not None))
    drive("nearest_to_groups variance", lambda: P.nearest_to_groups(groups, X, 3, "variance"))
    drive("nearest_to_groups diagonal", lambda: P.nearest_to_groups(groups, X, 3, "diagonal", np.ones((3, 23), np.float32)))
    drive("group_variance_weights", lambda: P.group_variance_weights(groups))
    drive("forest_nearest_to_groups", lambda: P.forest_nearest_to_groups(groups[1:], X, 3, P.ForestOptions(10, 4, None, 1, seed=1)))
    for labels in (None, lab):
        drive(f"moments labels={labels is not None}", lambda: P.moments(X, labels, None, labels is None))
    drive("metric_from_scatter", lambda: P.metric_from_scatter(np.eye(23), 11))
    for init in (None, np.ones(23)):
        drive(f"learn_metric init={init is not None}", lambda: P.learn_metric(X, [[0, 1, 2]], "full" if init is None else "diagonal", init, max_iter=2))
    drive("k_occurrence", lambda: P.k_occurrence(np.array([[0, 1, -1], [2, 2, 3]]), 12))
    drive("map_plan", lambda: P.map_plan(12))
    ro, co, va = np.array([0, 1, 2, 2] + [2] * 9, np.uint64), np.array([1, 0], np.uint32), np.array([0.5, 0.5])
    drive("map_step", lambda: P.map_step(X[:, :2], ro, co, va))
    drive("map_layout", lambda: P.map_layout(X[:, :2], ro, co, va, 3, 1))
    drive("fingerprint_match", lambda: P.fingerprint_match([np.arange(1, 300, dtype=np.uint32), np.arange(2, 301, dtype=np.uint32)], [[0, 1]]))
    drive("Forest", lambda: P.Forest(X[:4], P.ForestOptions(10, 4, None, 1, seed=1)).scores(X, True))
    drive("feature_weights", lambda: song.FeaturesVersion.Version2.feature_weights())
    pcm = [rng.standard_normal(9000).astype(np.float32) for _ in range(3)]
    drive("analyze_batch 3 songs", lambda: song.analyze_batch(pcm))
    drive("analyze_batch 1 song", lambda: song.analyze_batch(pcm[:1]))
    drive("analyze_batch empty song", lambda: song.analyze_batch([np.zeros(0, np.float32)]))
    for e in (False, True):
        drive(f"fingerprint_batch energies={e}", lambda: song.fingerprint_batch(pcm, e))
    drive_device()
    print("\n".join(RECORD))


if __name__ == "__main__":
    main()
