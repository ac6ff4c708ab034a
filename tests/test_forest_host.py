"""Device-free tests of the extended isolation forest (blissgpu_forest_*, playlist.ForestOptions): the C ABI surface, the
argument checks, reproducibility from the seed, the structure of the exported forest against the published algorithm, and
the Python errors of the entry points whose metric is built from one song.

`forest_walk` below is the independent walker of an EXPORTED forest (numpy f32, separate multiply and add); the GPU tests
import it for their expected values."""
import ctypes as C
import json
import math
import os
import re
import sqlite3
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
LEAF = 0xFFFFFFFF
INVALID = 2


def c_of(m):
    """Average path length of an unsuccessful search in a binary search tree of m samples (the paper's c)."""
    if m <= 1:
        return 0.0
    if m == 2:
        return 1.0
    return 2.0 * (math.log(m - 1.0) + 0.5772156649) - 2.0 * (m - 1.0) / m


def ceil_log2(psi):
    k = 0
    while (1 << k) < psi:
        k += 1
    return k


def forest_walk(ex, X, threads=16):
    """Walk every row of X (f32 [n, d]) through every tree of the export `ex` with the defined split test:
    s = +0; for j ascending with normal[j] != 0: s = f32(s + f32(normal[j] * x[j])); left iff s < b.
    -> (path_sum u64[n]: sum of leaf_q; depth_sum f64[n]: sum of depth + c(leaf_size), the unquantised definition;
        leaves int64[T, n]: the leaf reached in every tree when n is small, else None)."""
    X = np.ascontiguousarray(X, np.float32)
    n, d = X.shape
    XT = np.ascontiguousarray(X.T).reshape(-1)
    normal, b, left, right = ex["normal"], ex["b"], ex["left"].astype(np.int64), ex["right"].astype(np.int64)
    leaf_q, leaf_size, first = ex["leaf_q"].astype(np.uint64), ex["leaf_size"], ex["tree_first"].astype(np.int64)
    T = first.shape[0] - 1
    inner = ex["left"] != LEAF
    K = int((normal != 0).sum(1).max()) if normal.shape[0] else 0
    # per inner node: its non-zero components in ascending dimension (padded with a zero value that is never used)
    dims = np.zeros((normal.shape[0], max(K, 1)), np.int64)
    vals = np.zeros((normal.shape[0], max(K, 1)), np.float32)
    cnt = (normal != 0).sum(1)
    for i in np.nonzero(inner)[0]:
        nz = np.nonzero(normal[i])[0]
        dims[i, :nz.shape[0]] = nz
        vals[i, :nz.shape[0]] = normal[i, nz]
    c_leaf = np.array([c_of(int(m)) for m in range(int(leaf_size.max()) + 1)])
    keep = n <= 4096
    rows_all = np.arange(n, dtype=np.int64)

    def some(t_range):
        ps, ds = np.zeros(n, np.uint64), np.zeros(n, np.float64)
        lv = []
        for t in t_range:
            node = np.full(n, first[t], np.int64)
            depth = np.zeros(n, np.float64)
            for _ in range(300):
                act = inner[node]
                if not act.any():
                    break
                rows = rows_all[act]
                nn = node[act]
                s = np.zeros(rows.shape[0], np.float32)
                for k in range(int(cnt[nn].max())):
                    use = cnt[nn] > k
                    prod = (vals[nn, k] * XT[dims[nn, k] * n + rows]).astype(np.float32)
                    with np.errstate(invalid="ignore"):
                        s = np.where(use, (s + prod).astype(np.float32), s)
                with np.errstate(invalid="ignore"):
                    go_left = s < b[nn]
                node[act] = np.where(go_left, left[nn], right[nn])
                depth[act] += 1.0
            else:
                raise AssertionError("a walk did not end")
            ps += leaf_q[node]
            ds += depth + c_leaf[leaf_size[node]]
            if keep:
                lv.append(node.copy())
        return ps, ds, lv

    w = max(1, min(threads, T))
    with np.errstate(over="ignore", invalid="ignore"), ThreadPoolExecutor(w) as pool:
        parts = list(pool.map(some, [range(k, T, w) for k in range(w)]))
    ps = np.zeros(n, np.uint64)
    ds = np.zeros(n, np.float64)
    for p, q, _ in parts:
        ps += p
        ds += q
    leaves = None
    if keep:
        leaves = np.zeros((T, n), np.int64)
        for k, (_, _, lv) in enumerate(parts):
            for i, t in enumerate(range(k, T, w)):
                leaves[t] = lv[i]
    return ps, ds, leaves


def score_of(path_sum, n_trees, psi):
    return np.exp2(-(path_sum.astype(np.float64) / 16777216.0 / float(n_trees)) / c_of(psi))


def fixture_songs():
    with open(os.path.join(ROOT, "tests", "golden", "forest_songs.json")) as f:
        fx = json.load(f)
    groups = {g["name"]: np.asarray(g["songs"], np.float32) for g in fx["groups"]}
    return fx["options"], groups


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


def _build(S, d, n_trees, sample_size, depth, ext, seed=0, n_seeds=None):
    from bliss_rs_amd import _ffi

    h = _vp()
    rc = _ffi.lib().blissgpu_forest_build(None if S is None else S.ctypes.data, S.shape[0] if n_seeds is None else n_seeds, d,
                                          n_trees, sample_size, depth, ext, seed, C.byref(h))
    if h.value:
        _ffi.lib().blissgpu_forest_destroy(h)
    return rc


def test_forest_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "gpu.rs")).read()
    lib = C.CDLL(bliss.LIB_PATH)
    names = ("blissgpu_forest_build", "blissgpu_forest_destroy", "blissgpu_forest_info", "blissgpu_forest_export",
             "blissgpu_forest_score", "blissgpu_forest_score_device", "blissgpu_forest_closest_to_songs",
             "blissgpu_forest_closest_to_songs_device")
    for name in names:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name
        assert re.search(r"pub fn %s\(" % name, rust), name
    u64, u32 = C.c_uint64, C.c_uint32
    assert _ffi.SIGNATURES["blissgpu_forest_build"] == (C.c_int, [_vp, u64, u32, u32, u32, u32, u32, u64, C.POINTER(_vp)])
    assert _ffi.SIGNATURES["blissgpu_forest_score"] == (C.c_int, [_vp, _vp, u64, _vp, _vp])
    assert _ffi.SIGNATURES["blissgpu_forest_score_device"] == (C.c_int, [_vp, _vp, _vp, u64, _vp, _vp])
    assert _ffi.SIGNATURES["blissgpu_forest_closest_to_songs"] == (C.c_int, [_vp, _vp, u64, _vp, _vp])
    assert _ffi.SIGNATURES["blissgpu_forest_closest_to_songs_device"] == (C.c_int, [_vp, _vp, _vp, u64, _vp, _vp])
    for macro, least in (("MAX_TREES", 10000), ("MAX_PSI", 1024), ("MAX_D", 23), ("MAX_DEPTH", 128)):
        m = re.search(r"#define\s+BLISSGPU_FOREST_%s\s+(\d+)u?\b" % macro, header)
        assert m and int(m.group(1)) >= least, macro
    assert bliss.playlist.ForestOptions(1000, 200, None, 10, seed=3).seed == 3


def test_forest_arguments_are_checked_before_the_device(bliss, monkeypatch):
    from bliss_rs_amd import _ffi

    rng = np.random.default_rng(0)
    S = rng.uniform(-1, 1, (8, 23)).astype(np.float32)
    assert _build(S, 23, 10, 200, 0, 10) == 0
    assert _build(S, 20, 10, 200, 0, 10, n_seeds=8) == 0                   # the first 160 floats as 8 rows of 20
    assert _build(S[:1], 23, 10, 200, 0, 10) == INVALID                    # n_seeds < 2
    assert b"single song" in _ffi.lib().blissgpu_last_error()
    assert _build(S, 23, 10, 0, 0, 10, n_seeds=0) == INVALID
    assert _build(S, 23, 10, 1, 0, 10) == INVALID                          # psi < 2 through sample_size = 1
    assert _build(S, 23, 10, 0, 0, 10) == INVALID
    assert _build(S, 23, 10, 200, 0, 23) == INVALID                        # extension_level >= d
    assert _build(S, 20, 10, 200, 0, 20, n_seeds=8) == INVALID
    assert _build(S, 23, 0, 200, 0, 10) == INVALID                         # n_trees = 0
    assert _build(S, 23, 10, 200, 129, 10) == INVALID                      # depth beyond 128
    assert _build(S, 0, 10, 200, 0, 0) == INVALID
    assert _build(S, 65, 10, 200, 0, 0, n_seeds=2) == INVALID
    assert _build(None, 23, 10, 200, 0, 10, n_seeds=8) == INVALID          # NULL seeds
    assert _ffi.lib().blissgpu_forest_build(S.ctypes.data, 8, 23, 10, 200, 0, 10, 0, None) == INVALID   # NULL out
    bad = S.copy()
    bad[3, 5] = np.nan
    assert _build(bad, 23, 10, 200, 0, 10) == INVALID
    # scoring: NULL forest / pointers are refused before any device is looked for
    L = _ffi.lib()
    out, order = np.zeros(4, np.float32), np.zeros(4, np.uint32)
    assert L.blissgpu_forest_score(None, S.ctypes.data, 4, out.ctypes.data, None) == INVALID
    assert L.blissgpu_forest_closest_to_songs(None, S.ctypes.data, 4, order.ctypes.data, None) == INVALID
    assert L.blissgpu_forest_score_device(None, None, S.ctypes.data, 4, out.ctypes.data, None) == INVALID
    assert L.blissgpu_forest_info(None, None, None, None, None, None, None) == INVALID
    assert L.blissgpu_forest_export(None, None, None, None, None, None, None, None, None) == INVALID
    f = bliss.playlist.Forest(S, bliss.playlist.ForestOptions(10, 200, None, 10, seed=1))
    assert L.blissgpu_forest_score(f.handle, None, 4, out.ctypes.data, None) == INVALID
    assert L.blissgpu_forest_score(f.handle, S.ctypes.data, 4, None, None) == INVALID
    assert L.blissgpu_forest_closest_to_songs(f.handle, S.ctypes.data, 4, None, None) == INVALID
    assert L.blissgpu_forest_score_device(None, f.handle, S.ctypes.data, 4, out.ctypes.data, None) == INVALID   # NULL ctx
    assert L.blissgpu_forest_score(f.handle, None, 0, None, None) == 0                                         # n == 0
    assert L.blissgpu_forest_closest_to_songs(f.handle, None, 0, None, None) == 0
    f.close()


def _export_bytes(bliss, S, opts):
    f = bliss.playlist.Forest(S, opts)
    ex = f.export()
    f.close()
    return b"".join(np.ascontiguousarray(ex[k]).tobytes() for k in sorted(ex))


_CHILD = """
import hashlib, sys
import numpy as np
sys.path.insert(0, %r)
import bliss_rs_amd as bliss
S = np.random.default_rng(5).uniform(-1, 1, (40, 23)).astype(np.float32)
f = bliss.playlist.Forest(S, bliss.playlist.ForestOptions(50, 16, None, 10, seed=1234567890123))
ex = f.export()
print(hashlib.sha256(b"".join(np.ascontiguousarray(ex[k]).tobytes() for k in sorted(ex))).hexdigest())
"""


def test_forest_is_a_pure_function_of_rows_options_and_seed(bliss):
    import hashlib

    P = bliss.playlist
    S = np.random.default_rng(5).uniform(-1, 1, (40, 23)).astype(np.float32)
    a = _export_bytes(bliss, S, P.ForestOptions(50, 16, None, 10, seed=1234567890123))
    assert a == _export_bytes(bliss, S, P.ForestOptions(50, 16, None, 10, seed=1234567890123))
    child = subprocess.run([sys.executable, "-c", _CHILD % ROOT], capture_output=True, text=True, check=True)
    assert child.stdout.strip().splitlines()[-1] == hashlib.sha256(a).hexdigest()
    assert a != _export_bytes(bliss, S, P.ForestOptions(50, 16, None, 10, seed=1234567890124))
    # many trees (the builder goes multi-threaded) twice: the forest does not depend on the threading
    big = P.ForestOptions(300, 256, None, 3, seed=9)
    S2 = np.random.default_rng(6).uniform(-1, 1, (600, 23)).astype(np.float32)
    assert _export_bytes(bliss, S2, big) == _export_bytes(bliss, S2, P.ForestOptions(300, 256, None, 3, seed=9))
    # seed=None records what it drew
    drawn = P.ForestOptions(50, 16, None, 10)
    other = P.ForestOptions(50, 16, None, 10)
    assert isinstance(drawn.seed, int) and 0 <= drawn.seed < 2 ** 64 and drawn.seed != other.seed
    assert _export_bytes(bliss, S, drawn) == _export_bytes(bliss, S, P.ForestOptions(50, 16, None, 10, seed=drawn.seed))


GRID = [  # (n_seeds, sample_size, max_tree_depth, extension_level, d, n_trees)
    (3, 200, None, 10, 23, 200),
    (2, 2, None, 0, 23, 50),
    (16, 16, None, 0, 23, 100),
    (11, 200, None, 22, 23, 100),
    (300, 256, None, 22, 23, 20),
    (300, 64, None, 5, 20, 40),
    (300, 64, 3, 19, 20, 40),       # depth below ceil(log2 psi)
    (40, 16, 9, 4, 23, 60),         # depth above ceil(log2 psi)
    (64, 64, 128, 1, 23, 30),
    (50, 1024, 1, 7, 20, 30),
]


@pytest.mark.parametrize("n_seeds,sample_size,depth,ext,d,n_trees", GRID)
def test_exported_forest_follows_the_algorithm(bliss, n_seeds, sample_size, depth, ext, d, n_trees):
    rng = np.random.default_rng(n_seeds * 1000 + ext)
    S = rng.uniform(-1, 1, (n_seeds, d)).astype(np.float32)
    if n_seeds >= 16:
        S[5] = S[2]                                  # identical rows can never be separated
        S[7, :] = np.round(S[7] * 8) / 8
    f = bliss.playlist.Forest(S, bliss.playlist.ForestOptions(n_trees, sample_size, depth, ext, seed=77))
    psi = min(sample_size, n_seeds)
    limit = depth if depth is not None else ceil_log2(psi)
    assert (f.d, f.n_trees, f.psi, f.depth_limit, f.extension_level) == (d, n_trees, psi, limit, ext)
    ex = f.export()
    first = ex["tree_first"].astype(np.int64)
    assert first[0] == 0 and first[-1] == f.n_nodes and (np.diff(first) >= 1).all()
    left, right = ex["left"].astype(np.int64), ex["right"].astype(np.int64)
    is_leaf = ex["left"] == LEAF
    assert ((ex["right"] == LEAF) == is_leaf).all()
    # every inner normal has exactly extension_level + 1 non-zero components; a leaf has none
    nz = (ex["normal"] != 0).sum(1)
    assert (nz[~is_leaf] == ext + 1).all() and (nz[is_leaf] == 0).all()
    assert np.isfinite(ex["normal"]).all() and np.isfinite(ex["b"]).all()
    depth_of = np.full(f.n_nodes, -1, np.int64)
    for t in range(n_trees):
        lo, hi = first[t], first[t + 1]
        samp = ex["sample_idx"][t]
        assert samp.shape[0] == psi and np.unique(samp).shape[0] == psi and samp.max() < n_seeds
        # children stay inside the tree, every node but the root has exactly one parent
        kids = np.concatenate([left[lo:hi][~is_leaf[lo:hi]], right[lo:hi][~is_leaf[lo:hi]]])
        assert ((kids > lo) & (kids < hi)).all()
        assert np.array_equal(np.sort(kids), np.arange(lo + 1, hi))
        depth_of[lo] = 0
        for i in range(lo, hi):                      # parents come before their children (root first)
            assert depth_of[i] >= 0
            if not is_leaf[i]:
                assert left[i] > i and right[i] > i
                depth_of[left[i]] = depth_of[right[i]] = depth_of[i] + 1
    assert depth_of.max() <= limit
    assert (depth_of[~is_leaf] < limit).all()
    # the tree's own samples, walked with the defined test, fill every leaf with exactly leaf_size samples
    for t in range(n_trees):
        lo, hi = first[t], first[t + 1]
        one = {k: v for k, v in ex.items()}
        one["tree_first"] = np.array([lo, hi], np.uint64)
        _, _, leaves = forest_walk(one, S[ex["sample_idx"][t]], threads=1)
        got = np.bincount(leaves[0] - lo, minlength=hi - lo)
        want = np.where(is_leaf[lo:hi], ex["leaf_size"][lo:hi], 0)
        assert np.array_equal(got, want), t
    shallow = is_leaf & (depth_of < limit)
    assert (ex["leaf_size"][shallow] <= 1).all()
    assert (ex["leaf_size"][~is_leaf] == 0).all() and (ex["leaf_q"][~is_leaf] == 0).all()
    want_q = np.array([round((int(k) + c_of(int(m))) * 16777216.0) for k, m in zip(depth_of[is_leaf], ex["leaf_size"][is_leaf])],
                      np.uint64)
    assert np.array_equal(ex["leaf_q"][is_leaf].astype(np.uint64), want_q)
    f.close()


def test_python_entry_points_that_build_from_one_song_refuse_a_forest(bliss, tmp_path):
    from bliss_rs_amd import library

    P = bliss.playlist
    opts, groups = fixture_songs()
    fo = P.ForestOptions(opts["n_trees"], opts["sample_size"], opts["max_tree_depth"], opts["extension_level"], seed=0)
    songs = [bliss.Song(path=f"/m/{i}", analysis=bliss.Analysis(row, bliss.FeaturesVersion.LATEST))
             for i, row in enumerate(np.concatenate(list(groups.values())))]
    with pytest.raises(ValueError, match="single song"):
        P.song_to_song(songs[:3], songs, fo)
    with pytest.raises(ValueError, match="single song"):
        P.nearest_songs(songs[:2], songs, 3, fo)
    with pytest.raises(ValueError, match="single song"):
        P.dedup_playlist_custom_distance(songs, None, fo)
    with pytest.raises(ValueError, match="single song"):
        P.closest_to_songs(songs[:1], songs, fo)                      # one seed: psi < 2
    with pytest.raises(ValueError, match="single song"):
        P.forest_scores(groups["mozart_piano_19"], groups["kind_of_blue"], P.ForestOptions(10, 1, None, 10, seed=0))
    with pytest.raises(ValueError):
        P.forest_scores(groups["mozart_piano_19"], groups["kind_of_blue"], P.ForestOptions(10, 200, None, 23, seed=0))
    with pytest.raises(ValueError):
        P.forest_scores(groups["mozart_piano_19"], groups["kind_of_blue"], P.ForestOptions(0, 200, None, 10, seed=0))
    with pytest.raises(ValueError):
        P.forest_scores(groups["mozart_piano_19"], groups["kind_of_blue"], P.ForestOptions(10, 200, 0, 10, seed=0))
    with pytest.raises(TypeError):
        P._metric_of(fo)                                               # still only the three distance metrics
    with pytest.raises(TypeError):
        P._metric_of(lambda a, b: 0.0)
    db = str(tmp_path / "lib.db")
    library.create_schema(db)
    conn = sqlite3.connect(db)
    for song in songs:
        library.store_song(conn, song)
    conn.commit()
    conn.close()
    with pytest.raises(ValueError, match="single song"):
        library.playlist_from_custom(db, [s.path for s in songs[:3]], fo, P.closest_to_songs, deduplicate=True)
    with pytest.raises(ValueError, match="single song"):
        library.playlist_from_custom(db, [s.path for s in songs[:3]], fo, P.song_to_song, deduplicate=False)
    with pytest.raises(ValueError, match="single song"):
        library.similar_songs(db, 3, fo)
