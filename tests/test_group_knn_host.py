"""Device-free tests of the k-nearest search per seed group (blissgpu_group_knn / _device / _plan): the C ABI surface, the
argument checks that happen before the device is touched, the plan that deals out the groups x candidates plane, the checks of
playlist.nearest_to_groups that happen before the library is, and the grouping logic of library.group_playlists (with the
device call replaced by a numpy brute force)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
INVALID = 2


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


def test_group_knn_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    lib = C.CDLL(bliss.LIB_PATH)
    for name in ("blissgpu_group_knn", "blissgpu_group_knn_device", "blissgpu_group_knn_plan"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name
    u64, u32 = C.c_uint64, C.c_uint32
    # (seeds, group_offsets, n_groups, cand, n, d, metric, M, skip, k, idx, dist), the device form with the context in front
    host = [_vp, _vp, u64, _vp, u64, u32, C.c_int, _vp, _vp, u32, _vp, _vp]
    assert _ffi.SIGNATURES["blissgpu_group_knn"] == (C.c_int, host)
    assert _ffi.SIGNATURES["blissgpu_group_knn_device"] == (C.c_int, [_vp] + host)
    # (group_offsets, n_groups, n, k, n_cus, items, max_items, n_items, cand_block, seed_tile)
    assert _ffi.SIGNATURES["blissgpu_group_knn_plan"] == (C.c_int, [_vp, u64, u64, u32, u32, _vp, u64, C.POINTER(u64),
                                                                     C.POINTER(u32), C.POINTER(u32)])
    # the header's parameter lists, type by type
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    types = lambda name: [re.sub(r"\s*\w+$", "", re.sub(r"\s+", " ", a.strip())).replace(" *", "*")  # noqa: E731
                          for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, flat).group(1).split(",")]
    want = ["const float*", "const uint64_t*", "uint64_t", "const float*", "uint64_t", "uint32_t", "int", "const float*",
            "const uint32_t*", "uint32_t", "uint32_t*", "float*"]
    assert types("blissgpu_group_knn") == want
    assert types("blissgpu_group_knn_device") == ["blissgpu_ctx*"] + want
    assert types("blissgpu_group_knn_plan") == ["const uint64_t*", "uint64_t", "uint64_t", "uint32_t", "uint32_t", "uint32_t*",
                                                "uint64_t", "uint64_t*", "uint32_t*", "uint32_t*"]


def _call(bliss, S, off, X, k, d=None, metric=0, M=None, skip=None):
    from bliss_rs_amd import _ffi

    off = np.asarray(off, np.uint64)
    G, n = off.shape[0] - 1, X.shape[0]
    d = X.shape[1] if d is None else d
    idx, dist = np.zeros((G, max(k, 1)), np.uint32), np.zeros((G, max(k, 1)), np.float32)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return _ffi.lib().blissgpu_group_knn(p(S), p(off), G, p(X), n, d, metric, p(M), p(skip), k, p(idx), p(dist))


def test_group_knn_arguments_are_checked_before_the_device(bliss):
    import torch

    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    max_k = int(re.search(r"#define\s+BLISSGPU_KNN_MAX_K\s+(\d+)", header).group(1))
    rng = np.random.default_rng(0)
    X = rng.standard_normal((50, 23)).astype(np.float32)
    S = X[:6].copy()
    off = [0, 1, 4, 4, 6]
    assert _call(bliss, S, off, X, 0) == INVALID
    assert _call(bliss, S, off, X, max_k + 1) == INVALID
    assert _call(bliss, np.zeros((6, 65), np.float32), off, np.zeros((50, 65), np.float32), 3, d=65) == INVALID
    assert _call(bliss, S, off, X, 3, metric=2, M=None) == INVALID
    assert _call(bliss, S, off, X, 3, metric=3) == INVALID
    assert _call(bliss, S, off, X, 3, metric=-1) == INVALID
    assert _call(bliss, S, [1, 1, 4, 4, 6], X, 3) == INVALID
    assert _call(bliss, S, [0, 4, 1, 4, 6], X, 3) == INVALID
    skip = np.full(6, 0xFFFFFFFF, np.uint32)
    skip[3] = X.shape[0]
    assert _call(bliss, S, off, X, 3, skip=skip) == INVALID
    assert b"skip" in _ffi.lib().blissgpu_last_error()
    # the device form checks the same before it looks at its (NULL) context
    idx = np.zeros((4, 3), np.uint32)
    o = np.asarray(off, np.uint64)
    dev = lambda k, o: _ffi.lib().blissgpu_group_knn_device(None, S.ctypes.data, o.ctypes.data, 4, X.ctypes.data, 50, 23, 0,  # noqa: E731
                                                            None, None, k, idx.ctypes.data, None)
    assert dev(0, o) == INVALID and b"ctx" not in _ffi.lib().blissgpu_last_error()
    assert dev(3, np.asarray([0, 4, 1, 4, 6], np.uint64)) == INVALID and b"ctx" not in _ffi.lib().blissgpu_last_error()
    assert dev(3, o) == INVALID and b"ctx" in _ffi.lib().blissgpu_last_error()
    # nothing to do
    assert _call(bliss, S[:0], [0], X, 3) == 0
    # a valid call: BLISSGPU_ERR_NO_DEVICE without a GPU, BLISSGPU_OK with one
    skip[3] = 0
    assert _call(bliss, S, off, X, 3, skip=skip) == (0 if torch.cuda.is_available() else 1)


# ---- the plan ----
def _plan(sizes, n, k, n_cus, max_items=None):
    from bliss_rs_amd import _ffi

    off = np.zeros(len(sizes) + 1, np.uint64)
    off[1:] = np.cumsum(sizes)
    n_items, cb, st = C.c_uint64(), C.c_uint32(), C.c_uint32()
    L = _ffi.lib()
    assert L.blissgpu_group_knn_plan(off.ctypes.data, len(sizes), n, k, n_cus, None, 0, C.byref(n_items), C.byref(cb),
                                     C.byref(st)) == 0
    cap = n_items.value if max_items is None else max_items
    items = np.full((n_items.value + 3, 4), 0xABCDABCD, np.uint32)
    got = C.c_uint64()
    assert L.blissgpu_group_knn_plan(off.ctypes.data, len(sizes), n, k, n_cus, items.ctypes.data, cap, C.byref(got), None,
                                     None) == 0
    assert got.value == n_items.value
    assert (items[min(cap, n_items.value):] == 0xABCDABCD).all()  # nothing past max_items (or past the items)
    return items[:min(cap, n_items.value)].astype(np.int64), cb.value, st.value, n_items.value


def _plan_cases():
    rng = np.random.default_rng(11)
    mixed = np.concatenate([np.ones(120, np.int64), rng.integers(2, 9, 100), rng.integers(9, 65, 30), [300, 700]])
    return {
        "300 singles": (np.ones(300, np.int64), 3000),
        "mixed": (rng.permutation(mixed), 3000),
        "one big group": (np.concatenate([np.ones(5000, np.int64), [50_000], np.ones(5000, np.int64)]), 60_000),
        "empty groups": (np.array([0, 0, 3, 0, 1, 0, 0, 500, 0]), 2000),
        "only empty groups": (np.zeros(7, np.int64), 1000),
        "n below one block": (np.array([1, 5, 40, 1, 2]), 100),
    }


@pytest.mark.parametrize("n_cus", (1, 256))
@pytest.mark.parametrize("case", sorted(_plan_cases()))
def test_plan_covers_the_plane_once_within_the_cost_bound(bliss, case, n_cus):
    sizes, n = _plan_cases()[case]
    G = len(sizes)
    items, cand_block, seed_tile, n_items = _plan(sizes, n, 32, n_cus)
    assert cand_block >= 1 and seed_tile >= 1 and n_items == len(items) >= 1
    g_lo, g_hi, c_lo, c_hi = items.T
    assert (g_lo < g_hi).all() and (g_hi <= G).all() and (c_lo < c_hi).all() and (c_hi <= n).all()
    assert (c_lo % cand_block == 0).all()
    # exact single coverage: a difference array over the plane, compressed to the items' own boundaries
    gb = np.unique(np.concatenate([g_lo, g_hi, [0, G]]))
    cb = np.unique(np.concatenate([c_lo, c_hi, [0, n]]))
    cover = np.zeros((gb.size, cb.size), np.int64)
    gl, gh, cl, ch = np.searchsorted(gb, g_lo), np.searchsorted(gb, g_hi), np.searchsorted(cb, c_lo), np.searchsorted(cb, c_hi)
    np.add.at(cover, (gl, cl), 1)
    np.add.at(cover, (gh, cl), -1)
    np.add.at(cover, (gl, ch), -1)
    np.add.at(cover, (gh, ch), 1)
    cover = cover.cumsum(axis=0).cumsum(axis=1)[:-1, :-1]
    assert (cover == 1).all()
    # the derived bound: a group's chain cannot be split, so one block of one group is the smallest unit
    pre = np.concatenate([[0], np.cumsum(sizes)])
    cost = (pre[g_hi] - pre[g_lo]) * (c_hi - c_lo)
    total = int(pre[-1]) * n
    assert int(cost.sum()) == total
    assert int(cost.max()) <= max(total // n_cus, cand_block * int(sizes.max())), (case, n_cus, int(cost.max()))


def test_plan_edges(bliss):
    from bliss_rs_amd import _ffi

    sizes, n = _plan_cases()["one big group"]
    full = _plan(sizes, n, 32, 256)
    assert full[3] > 4
    cut = _plan(sizes, n, 32, 256, max_items=4)  # too small: the count is still reported, nothing is written past it
    assert cut[3] == full[3] and np.array_equal(cut[0], full[0][:4])
    big = np.flatnonzero((full[0][:, 1] - full[0][:, 0] == 1) & (sizes[full[0][:, 0]] == 50_000))
    assert big.size > 1 and 50_000 > full[2]  # the big group is cut by candidates and streams through the seed tile
    # nothing to tile
    assert _plan(np.array([1, 2]), 0, 32, 256)[3] == 0
    assert _plan(np.zeros(0, np.int64), 100, 32, 256)[3] == 0
    L, n_items = _ffi.lib(), C.c_uint64()
    off = np.array([0, 2, 1], np.uint64)
    assert L.blissgpu_group_knn_plan(off.ctypes.data, 2, 100, 32, 256, None, 0, C.byref(n_items), None, None) == INVALID
    off = np.array([0, 1, 2], np.uint64)
    assert L.blissgpu_group_knn_plan(off.ctypes.data, 2, 100, 0, 256, None, 0, C.byref(n_items), None, None) == INVALID
    assert L.blissgpu_group_knn_plan(off.ctypes.data, 2, 100, 32, 0, None, 0, C.byref(n_items), None, None) == INVALID
    assert L.blissgpu_group_knn_plan(off.ctypes.data, 2, 100, 32, 256, None, 0, None, None, None) == INVALID


# ---- playlist.nearest_to_groups: what is refused before the library is reached ----
def test_nearest_to_groups_checks_before_the_library(bliss, monkeypatch):
    from bliss_rs_amd import _ffi

    def boom():
        raise AssertionError("the library must not be reached")

    monkeypatch.setattr(_ffi, "lib", boom)
    P = bliss.playlist
    X = np.zeros((10, 23), np.float32)
    groups = [X[:1], X[1:4]]
    with pytest.raises(ValueError):
        P.nearest_to_groups([np.zeros((2, 20), np.float32)], X, 3)  # another d
    with pytest.raises(ValueError):
        P.nearest_to_groups([X[:1], np.zeros((2, 20), np.float32)], X, 3)
    with pytest.raises(ValueError):
        P.nearest_to_groups(groups, X, 0)
    with pytest.raises(ValueError):
        P.nearest_to_groups(groups, X, -1)
    with pytest.raises(ValueError):
        P.nearest_to_groups(groups, X, 1025)
    with pytest.raises(ValueError):
        P.nearest_to_groups(groups, X, 3, metric="manhattan")
    with pytest.raises(ValueError):
        P.nearest_to_groups(groups, X, 3, metric="mahalanobis")  # no m
    with pytest.raises(ValueError):
        P.nearest_to_groups((X[:4], [0, 1, 3]), X, 3)  # offsets do not end at the seed count
    with pytest.raises(ValueError):
        P.nearest_to_groups((X[:4], [0, 3, 1, 4]), X, 3)
    with pytest.raises(ValueError):
        P.nearest_to_groups(groups, X, 3, skip=np.array([0, 1, 2]))  # flat: one entry per seed row (4)
    with pytest.raises(ValueError):
        P.nearest_to_groups(groups, X, 3, skip=[[0], [1], [2]])  # per group: two groups
    with pytest.raises(ValueError):
        P.nearest_to_groups(groups, X, 3, skip=[[0, 1], [2]])  # more skips than seeds
    with pytest.raises(ValueError):
        P.nearest_to_groups(groups, X, 3, skip=np.array([0, 1, 10, -1]))  # not a candidate
    with pytest.raises(ValueError):
        P.nearest_to_groups(groups, X, 3, skip=np.array([0, 1, -2, -1]))
    with pytest.raises(ValueError) as e:
        P.nearest_to_groups(groups, X, 3, metric=P.ForestOptions(10, 8, None, 1, seed=1))
    assert "isolation forest" in str(e.value)
    with pytest.raises(ValueError):
        P.group_playlists([[]], [], 3, metric_builder=P.ForestOptions(10, 8, None, 1, seed=1))


# ---- library.group_playlists: the grouping, with the device call replaced by a numpy brute force ----
def _brute_force(record):
    def nearest_to_groups(seed_groups, candidates, k, metric="euclidean", m=None, skip=None):
        S, off = seed_groups
        S, X = np.asarray(S, np.float32), np.asarray(candidates, np.float32)
        off = np.asarray(off, np.int64)
        record.append((S.copy(), off.copy(), None if skip is None else np.asarray(skip).copy()))
        G = off.shape[0] - 1
        idx, dist = np.full((G, k), -1, np.int64), np.full((G, k), np.inf, np.float32)
        for g in range(G):
            score = np.zeros(X.shape[0], np.float32)
            for s in range(off[g], off[g + 1]):
                score = score + np.sqrt(((S[s] - X) ** 2).sum(axis=1, dtype=np.float32))
            order = np.argsort(score, kind="stable")
            if skip is not None:
                order = order[~np.isin(order, np.asarray(skip)[off[g]:off[g + 1]])]
            order = order[:k]
            idx[g, :order.size], dist[g, :order.size] = order, score[order]
        return idx, dist

    return nearest_to_groups


def _library(bliss, tmp_path, n=60):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, 23)).astype(np.float32)
    V2 = bliss.FeaturesVersion.Version2
    songs = []
    for i in range(n):
        tag = lambda name, mod, every: None if i % every == 3 else f"{name}{(i * 7) % mod}"  # noqa: E731
        songs.append(bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist=tag("artist", 5, 11), album=tag("album", 9, 7),
                                album_artist=tag("aa", 3, 13), genre=tag("genre", 4, 5), duration=1.0,
                                analysis=bliss.Analysis(X[i], V2), features_version=V2))
    db = str(tmp_path / "bliss.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs)
    return db, songs, X


@pytest.mark.parametrize("by", ("album", "artist", "album_artist", "genre"))
def test_library_group_playlists_grouping(bliss, tmp_path, monkeypatch, by):
    db, songs, X = _library(bliss, tmp_path)
    record = []
    monkeypatch.setattr(bliss.playlist, "nearest_to_groups", _brute_force(record))
    k = 5
    table = bliss.library.group_playlists(db, k, by=by)
    assert len(record) == 1  # one call for the whole library
    S, off, skip = record[0]
    # groups by first appearance in id order, members in id order, NULL keys in no group
    keys, members = [], {}
    for i, s in enumerate(songs):
        key = getattr(s, by)
        if key is not None:
            if key not in members:
                keys.append(key)
            members.setdefault(key, []).append(i)
    assert any(getattr(s, by) is None for s in songs)
    assert list(table) == keys
    rows = np.concatenate([members[key] for key in keys])
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(members[key]) for key in keys])]))
    assert np.array_equal(S, X[rows]) and np.array_equal(np.asarray(skip), rows)
    for key in keys:
        inside = set(members[key])
        got = table[key]
        assert len(got) == k and not ({int(p[7:10]) for p, _ in got} & inside)
        score = np.zeros(len(songs), np.float32)
        for s in members[key]:
            score = score + np.sqrt(((X[s] - X) ** 2).sum(axis=1, dtype=np.float32))
        order = [j for j in np.argsort(score, kind="stable") if j not in inside][:k]
        assert [p for p, _ in got] == [songs[j].path for j in order]
        assert [v for _, v in got] == [float(score[j]) for j in order]
    # a song without a key is still a candidate of the others
    nulls = {s.path for s in songs if getattr(s, by) is None}
    assert nulls & {p for got in table.values() for p, _ in got}


def test_library_group_playlists_custom_groups(bliss, tmp_path, monkeypatch):
    db, songs, X = _library(bliss, tmp_path)
    record = []
    monkeypatch.setattr(bliss.playlist, "nearest_to_groups", _brute_force(record))
    path = lambda i: songs[i].path  # noqa: E731
    groups = {"evening": [path(9), path(2), path(9)], "one": [path(40)], "none": []}
    table = bliss.library.group_playlists(db, 4, groups=groups)
    S, off, skip = record[0]
    assert list(table) == ["evening", "one", "none"]
    assert np.array_equal(off, [0, 3, 4, 4]) and np.array_equal(np.asarray(skip), [9, 2, 9, 40])  # order as given, twice a seed
    assert np.array_equal(S, X[[9, 2, 9, 40]])
    assert not ({p for p, _ in table["evening"]} & {path(9), path(2)})
    assert [p for p, _ in table["none"]] == [path(i) for i in range(4)]  # an empty seed set: the first k candidates, score 0
    assert [v for _, v in table["none"]] == [0.0] * 4
    with pytest.raises(bliss.ProviderError):
        bliss.library.group_playlists(db, 4, groups={"x": [path(1), "/music/none.flac"]})
    with pytest.raises(ValueError):
        bliss.library.group_playlists(db, 4, by="year")
    assert len(record) == 1
