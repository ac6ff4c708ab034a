"""Device-free tests of the isolation-forest playlists for every group in one call (blissgpu_group_forest_knn / _device / _plan,
playlist.forest_nearest_to_groups, playlist.forest_group_playlists, library.forest_playlists): the C ABI surface, the argument
checks that happen before the device is touched and before any forest is built, the batch plan, and what the Python layer
decides from the group sizes alone."""
import ctypes as C
import os
import re
import sqlite3

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
NO_DEVICE, INVALID = 1, 2
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


def test_group_forest_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "gpu.rs")).read()
    extern = re.search(r'extern "C" \{(.*?)\n    \}', rust, flags=re.S).group(1)
    lib = C.CDLL(bliss.LIB_PATH)
    for name in ("blissgpu_group_forest_knn", "blissgpu_group_forest_knn_device", "blissgpu_group_forest_plan"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name
        assert re.search(r"pub fn %s\(" % name, extern), name
    u64, u32 = C.c_uint64, C.c_uint32
    # (seeds, group_offsets, n_groups, cand, n, d, n_trees, sample_size, max_tree_depth, extension_level, seed, skip, k, idx, score,
    #  group_status); the device form with the context in front and the host copy of the seeds after the device pointer
    tail = [_vp, u64, _vp, u64, u32, u32, u32, u32, u32, u64, _vp, u32, _vp, _vp, _vp]
    assert _ffi.SIGNATURES["blissgpu_group_forest_knn"] == (C.c_int, [_vp] + tail)
    assert _ffi.SIGNATURES["blissgpu_group_forest_knn_device"] == (C.c_int, [_vp, _vp, _vp] + tail)
    # (group_offsets, n_groups, d, n_trees, sample_size, max_tree_depth, extension_level, node_budget, batch_first, max_batches, n_batches)
    assert _ffi.SIGNATURES["blissgpu_group_forest_plan"] == (C.c_int, [_vp, u64, u32, u32, u32, u32, u32, u64, _vp, u64,
                                                                       C.POINTER(u64)])
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    types = lambda name: [re.sub(r"\s*\w+$", "", re.sub(r"\s+", " ", a.strip())).replace(" *", "*")  # noqa: E731
                          for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, flat).group(1).split(",")]
    want = ["const uint64_t*", "uint64_t", "const float*", "uint64_t", "uint32_t", "uint32_t", "uint32_t", "uint32_t", "uint32_t",
            "uint64_t", "const uint32_t*", "uint32_t", "uint32_t*", "float*", "int32_t*"]
    assert types("blissgpu_group_forest_knn") == ["const float*"] + want
    assert types("blissgpu_group_forest_knn_device") == ["blissgpu_ctx*", "const float*", "const float*"] + want
    assert types("blissgpu_group_forest_plan") == ["const uint64_t*", "uint64_t", "uint32_t", "uint32_t", "uint32_t", "uint32_t",
                                                   "uint32_t", "uint64_t", "uint64_t*", "uint64_t", "uint64_t*"]
    assert re.search(r"#define\s+BLISSGPU_OPT_FOREST_GROUP_NODES\s+15\b", header) and _ffi.OPT_FOREST_GROUP_NODES == 15
    from bliss_rs_amd.device import Context

    assert Context.OPTIONS["forest_group_nodes"] == 15
    # the scan kernel is in the profiling table, once, behind every older name
    L = _ffi.lib()
    table = [L.blissgpu_profile_kernel_name(i).decode() for i in range(L.blissgpu_profile_kernel_count())]
    assert table.count("group_forest_scan_kernel") == 1 and len(set(table)) == len(table)
    assert table.index("album_knn_scan_kernel") < table.index("group_forest_scan_kernel")


def _p(a):
    return None if a is None else a.ctypes.data


def _call(S, off, X, k, opts=(10, 8, 0, 1), d=None, skip=None, idx=True, device_form=False, seed=3):
    from bliss_rs_amd import _ffi

    off = None if off is None else np.asarray(off, np.uint64)
    G = 0 if off is None else off.shape[0] - 1
    n = 0 if X is None else X.shape[0]
    d = X.shape[1] if d is None else d
    out_i, out_s = np.zeros((max(G, 1), max(k, 1)), np.uint32), np.zeros((max(G, 1), max(k, 1)), np.float32)
    status = np.zeros(max(G, 1), np.int32)
    tail = (_p(off), G, _p(X), n, d, opts[0], opts[1], opts[2], opts[3], seed, _p(skip), k, _p(out_i) if idx else None, _p(out_s),
            _p(status))
    if device_form:  # a NULL context: everything about the arguments is said before the context is looked at
        return _ffi.lib().blissgpu_group_forest_knn_device(None, None, _p(S), *tail)
    return _ffi.lib().blissgpu_group_forest_knn(_p(S), *tail)


def test_arguments_are_checked_before_the_device(bliss):
    import torch

    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    assert int(re.search(r"#define\s+BLISSGPU_KNN_MAX_K\s+(\d+)", header).group(1)) == 1024
    assert int(re.search(r"#define\s+BLISSGPU_FOREST_MAX_D\s+(\d+)", header).group(1)) == 32
    rng = np.random.default_rng(0)
    X = rng.standard_normal((50, 23)).astype(np.float32)
    S = X[:6].copy()
    off = [0, 1, 4, 4, 6]
    err = lambda: _ffi.lib().blissgpu_last_error()  # noqa: E731
    wide = np.zeros((6, 33), np.float32)
    for dev in (False, True):
        bad = lambda *a, **kw: _call(*a, device_form=dev, **kw) == INVALID and b"ctx" not in err()  # noqa: E731
        assert bad(S, off, X, 0) and b"k must" in err()
        assert bad(S, off, X, 1025) and b"k must" in err()
        assert bad(S, off, X, 3, d=0) and b"d must" in err()
        assert bad(wide, off, np.zeros((50, 33), np.float32), 3) and b"d must" in err()
        assert bad(S, off, X, 3, opts=(10, 8, 0, 23)) and b"extension_level" in err()
        assert bad(S, off, X, 3, opts=(0, 8, 0, 1)) and b"n_trees" in err()
        assert bad(S, off, X, 3, opts=(10, 8, 129, 1)) and b"max_tree_depth" in err()
        assert bad(S, [1, 1, 4, 6], X, 3) and b"group_offsets" in err()
        assert bad(S, [0, 4, 1, 6], X, 3) and b"group_offsets" in err()
        assert bad(None, off, X, 3) and b"seeds" in err()
        assert bad(S, off, X, 3, idx=False) and b"idx" in err()
        nan = S.copy()
        nan[4, 7] = np.nan
        assert bad(nan, off, X, 3) and b"finite" in err()
        inf = S.copy()
        inf[0, 0] = np.inf
        assert bad(inf, off, X, 3) and b"finite" in err()
    # cand NULL with n > 0 (the wrapper above derives n from X, so by hand), and the host form's skip on the host
    out_i = np.zeros((4, 3), np.uint32)
    offs = np.asarray(off, np.uint64)
    L = _ffi.lib()
    assert L.blissgpu_group_forest_knn(S.ctypes.data, offs.ctypes.data, 4, None, 50, 23, 10, 8, 0, 1, 3, None, 3, out_i.ctypes.data,
                                       None, None) == INVALID and b"cand" in err()
    assert L.blissgpu_group_forest_knn(S.ctypes.data, None, 4, X.ctypes.data, 50, 23, 10, 8, 0, 1, 3, None, 3, out_i.ctypes.data,
                                       None, None) == INVALID and b"group_offsets" in err()
    skip = np.full(6, NONE, np.uint32)
    skip[2] = 50
    assert _call(S, off, X, 3, skip=skip) == INVALID and b"skip" in err()
    skip[2] = 49
    if not torch.cuda.is_available():  # every argument is fine: the first thing that fails is the missing device
        assert _call(S, off, X, 3, skip=skip) == NO_DEVICE
    # nothing to do is fine without a device
    assert _call(S, [0], X, 3) == 0
    # no candidates: every row is padding, the status is written, and the host form needs no device for it
    out_i, out_s, status = np.zeros((4, 3), np.uint32), np.zeros((4, 3), np.float32), np.full(4, 7, np.int32)
    assert L.blissgpu_group_forest_knn(S.ctypes.data, offs.ctypes.data, 4, None, 0, 23, 10, 8, 0, 1, 3, None, 3, out_i.ctypes.data,
                                       out_s.ctypes.data, status.ctypes.data) == 0
    assert (out_i == NONE).all() and np.isinf(out_s).all() and status.tolist() == [1, 0, 1, 0]


def _plan(off, opts, budget, d=23, cap=None):
    from bliss_rs_amd import _ffi

    off = np.asarray(off, np.uint64)
    G = off.shape[0] - 1
    nb = C.c_uint64()
    first = np.zeros(G + 1 if cap is None else cap, np.uint64)
    rc = _ffi.lib().blissgpu_group_forest_plan(off.ctypes.data, G, d, opts[0], opts[1], opts[2], opts[3], budget, first.ctypes.data,
                                               first.shape[0], C.byref(nb))
    assert rc == 0, _ffi.lib().blissgpu_last_error()
    return first[:int(nb.value) + 1].astype(np.int64), int(nb.value)


def _planned_nodes(count, n_trees, sample_size):
    psi = min(count, sample_size)
    return 1 if psi < 2 else n_trees * (2 * psi - 1)


def test_plan_batches(bliss):
    rng = np.random.default_rng(5)
    sizes = rng.integers(0, 21, 300)
    sizes[17] = 400
    off = np.concatenate([[0], np.cumsum(sizes)])
    opts = (64, 16, 0, 10)
    nodes = np.asarray([_planned_nodes(int(c), opts[0], opts[1]) for c in sizes])
    for budget in (1, 64 * 31, 5000, 20000, 10 ** 9, 0):
        first, nb = _plan(off, opts, budget)
        again, nb2 = _plan(off, opts, budget)
        assert nb == nb2 and np.array_equal(first, again)                      # reproducible
        assert first[0] == 0 and first[-1] == 300 and (np.diff(first) >= 1).all()  # consecutive, every group once
        if budget == 0:
            assert nb == 1  # (a 64 MiB image holds these)
            continue
        for a, b in zip(first[:-1], first[1:]):
            total = nodes[a:b].sum()
            assert total <= budget or b - a == 1, (budget, a, b, total)      # within the budget, or one oversized group alone
            if b < 300:
                assert total + nodes[b] > budget                             # ... and no batch ends early
        if budget == 1:
            assert nb == 300 and np.array_equal(first, np.arange(301))
        if budget == 10 ** 9:
            assert nb == 1
    # the oversized group (min(400, 16) = 16 samples a tree: 64 x 31 nodes) is alone under a budget just below it
    first, _ = _plan(off, opts, 64 * 31 - 1)
    assert 17 in first and 18 in first
    # nothing is written past max_batches; the count is still reported
    first, nb = _plan(off, opts, 1, cap=5)
    assert nb == 300 and np.array_equal(first[:5], np.arange(5))
    # no groups: no batches
    first, nb = _plan([0], opts, 7)
    assert nb == 0
    # the plan checks its arguments too
    from bliss_rs_amd import _ffi

    offs = np.asarray([0, 2, 1], np.uint64)
    nbv = C.c_uint64()
    assert _ffi.lib().blissgpu_group_forest_plan(offs.ctypes.data, 2, 23, 10, 8, 0, 1, 5, None, 0, C.byref(nbv)) == INVALID
    offs = np.asarray([0, 2, 3], np.uint64)
    assert _ffi.lib().blissgpu_group_forest_plan(offs.ctypes.data, 2, 23, 10, 8, 0, 23, 5, None, 0, C.byref(nbv)) == INVALID
    assert _ffi.lib().blissgpu_group_forest_plan(offs.ctypes.data, 2, 23, 10, 8, 0, 1, 5, None, 0, None) == INVALID
    assert _ffi.lib().blissgpu_group_forest_plan(offs.ctypes.data, 2, 23, 10, 8, 0, 1, 1000, None, 0, C.byref(nbv)) == 0 and nbv.value == 1


def _songs(bliss, rows, albums):
    return [bliss.Song(path=f"/music/{albums[i]}-{i}", album=albums[i], analysis=bliss.Analysis(row, bliss.FeaturesVersion.LATEST),
                       features_version=bliss.FeaturesVersion.LATEST) for i, row in enumerate(rows)]


def test_few_seeds_is_decided_before_the_library(bliss, monkeypatch, tmp_path):
    from bliss_rs_amd import _ffi, library

    P = bliss.playlist
    rng = np.random.default_rng(1)
    X = rng.uniform(-1, 1, (12, 23)).astype(np.float32)
    groups = [X[:3], X[3:4], X[4:9]]
    fo = P.ForestOptions(10, 8, None, 1, seed=1)
    songs = _songs(bliss, X, ["a"] * 3 + ["single"] + ["b"] * 5 + ["c"] * 3)
    db = str(tmp_path / "bliss.db")
    library.create_schema(db)
    conn = sqlite3.connect(db)
    for s in songs:
        library.store_song(conn, s)
    conn.commit()
    conn.close()

    def no_library():
        raise AssertionError("the library must not be reached")

    monkeypatch.setattr(_ffi, "lib", no_library)
    song_groups = [songs[:3], songs[3:4], songs[4:9]]
    for call in (lambda fs: P.forest_nearest_to_groups(groups, X, 3, fo, few_seeds=fs),
                 lambda fs: P.forest_group_playlists(song_groups, songs, 3, fo, few_seeds=fs),
                 lambda fs: library.forest_playlists(db, 3, fo, few_seeds=fs)):
        with pytest.raises(ValueError) as e:
            call("raise")
        assert "single song" in str(e.value) and "isolation forest" in str(e.value)
        with pytest.raises(ValueError) as e:
            call("pad")  # unknown policies are refused
        assert "few_seeds" in str(e.value)
    # the default is "raise"
    with pytest.raises(ValueError):
        P.forest_nearest_to_groups(groups, X, 3, fo)
    # sample_size < 2 makes every group a single
    with pytest.raises(ValueError):
        P.forest_nearest_to_groups([X[:3], X[4:9]], X, 3, P.ForestOptions(10, 1, None, 1, seed=1))
    # "euclidean" belongs to the song forms only
    with pytest.raises(ValueError) as e:
        P.forest_nearest_to_groups(groups, X, 3, fo, few_seeds="euclidean")
    assert "few_seeds" in str(e.value)
    # "empty" and "euclidean" are accepted: they get as far as the library
    for call in (lambda: P.forest_nearest_to_groups(groups, X, 3, fo, few_seeds="empty"),
                 lambda: P.forest_group_playlists(song_groups, songs, 3, fo, few_seeds="empty"),
                 lambda: P.forest_group_playlists(song_groups, songs, 3, fo, few_seeds="euclidean"),
                 lambda: library.forest_playlists(db, 3, fo, few_seeds="empty"),
                 lambda: library.forest_playlists(db, 3, fo, few_seeds="euclidean")):
        with pytest.raises(AssertionError) as e:
            call()
        assert "must not be reached" in str(e.value)
    # arguments the Python layer refuses by itself
    with pytest.raises(TypeError):
        P.forest_nearest_to_groups([X[:3]], X, 3, "euclidean")
    with pytest.raises(ValueError):
        P.forest_nearest_to_groups([X[:3]], X, 0, fo)
    with pytest.raises(ValueError):
        P.forest_nearest_to_groups([X[:3]], X, 1025, fo)
    with pytest.raises(ValueError):
        P.forest_nearest_to_groups([X[:3]], X, 3, fo, skip=[[12]])
    with pytest.raises(ValueError):
        library.forest_playlists(db, 3, fo, by="year")
    with pytest.raises(TypeError):
        library.forest_playlists(db, 3, P.euclidean_distance)
    with pytest.raises(bliss.ProviderError):
        library.forest_playlists(db, 3, fo, groups={"x": ["/music/nowhere"]})


def test_the_old_refusals_still_raise_and_point_to_the_new_functions(bliss, tmp_path):
    from bliss_rs_amd import library

    P = bliss.playlist
    rng = np.random.default_rng(2)
    X = rng.uniform(-1, 1, (8, 23)).astype(np.float32)
    fo = P.ForestOptions(10, 8, None, 1, seed=1)
    songs = _songs(bliss, X, ["a"] * 4 + ["b"] * 4)
    db = str(tmp_path / "bliss.db")
    library.create_schema(db)
    conn = sqlite3.connect(db)
    for s in songs:
        library.store_song(conn, s)
    conn.commit()
    conn.close()
    for call, hint in ((lambda: P.nearest_to_groups([X[:4], X[4:]], X, 3, fo), "forest_nearest_to_groups"),
                       (lambda: P.group_playlists([songs[:4], songs[4:]], songs, 3, fo), "forest_group_playlists"),
                       (lambda: library.group_playlists(db, 3, metric_builder=fo), "forest_playlists")):
        with pytest.raises(ValueError) as e:
            call()
        assert "isolation forest" in str(e.value) and hint in str(e.value)
