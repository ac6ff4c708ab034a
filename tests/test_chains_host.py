"""Device-free tests of the song-to-song chains cut after k (blissgpu_chains / _device / _plan): the C ABI surface, the
argument checks that happen before the device is touched, the route blissgpu_chains_plan picks, and the host logic of
playlist.song_chains / library.chain_playlists (with the device call replaced by a numpy brute force)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
INVALID = 2
AUTO, STEPS, LISTS = 0, 1, 2


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


def test_chains_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    lib = C.CDLL(bliss.LIB_PATH)
    for name in ("blissgpu_chains", "blissgpu_chains_device", "blissgpu_chains_plan"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name
    for name, value in (("AUTO", 0), ("STEPS", 1), ("LISTS", 2)):
        assert re.search(r"#define\s+BLISSGPU_CHAINS_%s\s+%d\b" % (name, value), header), name
        assert getattr(_ffi, "CHAINS_" + name) == value
    u64, u32 = C.c_uint64, C.c_uint32
    # (seeds, group_offsets, n_groups, cand, n, d, metric, M, skip, k, route, idx, dist), the device form with the context in front
    host = [_vp, _vp, u64, _vp, u64, u32, C.c_int, _vp, _vp, u32, C.c_int, _vp, _vp]
    assert _ffi.SIGNATURES["blissgpu_chains"] == (C.c_int, host)
    assert _ffi.SIGNATURES["blissgpu_chains_device"] == (C.c_int, [_vp] + host)
    # (group_offsets, n_groups, n, k, workspace_bytes, route, list_len)
    assert _ffi.SIGNATURES["blissgpu_chains_plan"] == (C.c_int, [_vp, u64, u64, u32, u64, C.POINTER(C.c_int), C.POINTER(u32)])
    # the header's parameter lists, type by type
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    types = lambda name: [re.sub(r"\s*\w+$", "", re.sub(r"\s+", " ", a.strip())).replace(" *", "*")  # noqa: E731
                          for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, flat).group(1).split(",")]
    want = ["const float*", "const uint64_t*", "uint64_t", "const float*", "uint64_t", "uint32_t", "int", "const float*",
            "const uint32_t*", "uint32_t", "int", "uint32_t*", "float*"]
    assert types("blissgpu_chains") == want
    assert types("blissgpu_chains_device") == ["blissgpu_ctx*"] + want
    assert types("blissgpu_chains_plan") == ["const uint64_t*", "uint64_t", "uint64_t", "uint32_t", "uint64_t", "int*", "uint32_t*"]
    # the profiling table: the one list of X(id, "name") entries that the ids, the count and the library's names come from
    src = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "internal.hpp")).read()
    table = re.search(r"#define BLISSGPU_KERNEL_TABLE\(X\)(.*?)\nenum KernelId", src, flags=re.S).group(1)
    entries = re.findall(r'\bX\((\w+),\s*"(\w+)"\)', table)
    assert len(entries) == table.count("X(") == lib.blissgpu_profile_kernel_count()
    lib.blissgpu_profile_kernel_name.restype = C.c_char_p
    assert [lib.blissgpu_profile_kernel_name(i).decode() for i in range(len(entries))] == [name for _, name in entries]
    assert len({i for i, _ in entries}) == len(entries) and len({name for _, name in entries}) == len(entries)
    assert all(re.fullmatch(r"KX?_[A-Z0-9_]+", i) and name.endswith("_kernel") for i, name in entries)
    # the two kernels where they have always been, and no older id moved: the first 29 names by value
    assert entries[27] == ("K_CHAIN_STEP", "chain_step_kernel") and entries[28] == ("K_CHAIN_WALK", "chain_walk_kernel")
    assert [name for _, name in entries[:29]] == [
        "fft512_kernel", "onset_kernel", "beat_kernel", "stft8192_kernel", "tune_select_kernel", "tune_pass2_kernel",
        "tune_final_kernel", "chroma_kernel", "summary_kernel", "assemble_kernel", "pairwise_kernel", "set_distance_kernel",
        "song_to_song_kernel", "synth_kernel", "rolloff_fix_kernel", "dedup_next_kernel", "dedup_walk_kernel", "knn_scan_kernel",
        "knn_merge_kernel", "forest_walk_kernel", "forest_finish_kernel", "dup_init_kernel", "dup_join_kernel", "dup_flatten_kernel",
        "group_knn_scan_kernel", "group_knn_merge_kernel", "group_weights_kernel", "chain_step_kernel", "chain_walk_kernel"]


def _call(bliss, S, off, X, k, d=None, metric=0, M=None, skip=None, route=AUTO):
    from bliss_rs_amd import _ffi

    off = np.asarray(off, np.uint64)
    G, n = off.shape[0] - 1, X.shape[0]
    d = X.shape[1] if d is None else d
    idx, dist = np.zeros((G, max(k, 1)), np.uint32), np.zeros((G, max(k, 1)), np.float32)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return _ffi.lib().blissgpu_chains(p(S), p(off), G, p(X), n, d, metric, p(M), p(skip), k, route, p(idx), p(dist))


def test_chains_arguments_are_checked_before_the_device(bliss):
    import torch

    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    max_k = int(re.search(r"#define\s+BLISSGPU_KNN_MAX_K\s+(\d+)", header).group(1))
    assert max_k == 1024
    rng = np.random.default_rng(0)
    X = rng.standard_normal((50, 23)).astype(np.float32)
    S = X[:6].copy()
    off = [0, 1, 4, 4, 6]
    assert _call(bliss, S, off, X, 0) == INVALID
    assert _call(bliss, S, off, X, max_k + 1) == INVALID
    assert _call(bliss, S, off, X, 3, d=0) == INVALID
    assert _call(bliss, np.zeros((6, 65), np.float32), off, np.zeros((50, 65), np.float32), 3, d=65) == INVALID
    assert _call(bliss, S, off, X, 3, metric=2, M=None) == INVALID
    assert _call(bliss, S, off, X, 3, metric=3) == INVALID
    assert _call(bliss, S, [1, 1, 4, 4, 6], X, 3) == INVALID
    assert _call(bliss, S, [0, 4, 1, 4, 6], X, 3) == INVALID
    assert _call(bliss, S, off, X, 3, route=3) == INVALID and b"route" in _ffi.lib().blissgpu_last_error()
    assert _call(bliss, S, off, X, 3, route=-1) == INVALID
    skip = np.full(6, 0xFFFFFFFF, np.uint32)
    skip[3] = X.shape[0]
    assert _call(bliss, S, off, X, 3, skip=skip) == INVALID
    assert b"skip" in _ffi.lib().blissgpu_last_error()
    # a forced lists route whose lists would be longer than the k-nearest search allows: L = 1000 + 26 - 1
    big = np.zeros((26, 23), np.float32)
    assert _call(bliss, big, [0, 26], X, 1000, route=LISTS) == INVALID and b"lists" in _ffi.lib().blissgpu_last_error()
    # the device form checks the same before it looks at its (NULL) context
    idx = np.zeros((4, 3), np.uint32)
    o = np.asarray(off, np.uint64)
    dev = lambda k, o, route=AUTO, d=23: _ffi.lib().blissgpu_chains_device(  # noqa: E731
        None, S.ctypes.data, o.ctypes.data, o.shape[0] - 1, X.ctypes.data, 50, d, 0, None, None, k, route, idx.ctypes.data, None)
    for bad in (dev(0, o), dev(max_k + 1, o), dev(3, o, d=0), dev(3, o, d=65), dev(3, np.asarray([0, 4, 1, 4, 6], np.uint64)),
                dev(3, o, route=7), dev(1000, np.asarray([0, 26], np.uint64), route=LISTS)):
        assert bad == INVALID and b"ctx" not in _ffi.lib().blissgpu_last_error()
    assert dev(3, o) == INVALID and b"ctx" in _ffi.lib().blissgpu_last_error()
    # nothing to do
    assert _call(bliss, S[:0], [0], X, 3) == 0
    # a valid call: BLISSGPU_ERR_NO_DEVICE without a GPU, BLISSGPU_OK with one
    skip[3] = 0
    assert _call(bliss, S, off, X, 3, skip=skip) == (0 if torch.cuda.is_available() else 1)


# ---- the plan ----
def _plan(sizes, n, k, workspace=1 << 40):
    from bliss_rs_amd import _ffi

    off = np.zeros(len(sizes) + 1, np.uint64)
    off[1:] = np.cumsum(sizes)
    route, list_len = C.c_int(-1), C.c_uint32(0xABCD)
    assert _ffi.lib().blissgpu_chains_plan(off.ctypes.data, len(sizes), n, k, workspace, C.byref(route), C.byref(list_len)) == 0
    return route.value, list_len.value


def test_chains_plan(bliss):
    from bliss_rs_amd import _ffi

    ones = lambda g: np.ones(g, np.int64)  # noqa: E731
    assert _plan([3, 9, 0, 1], 1000, 5)[1] == 5 + 9 - 1
    assert _plan(ones(7), 1000, 20)[1] == 20
    assert _plan([1], 100_000, 20) == (STEPS, 20)  # one playlist: 19 scans of the library, not n x n pairs
    assert _plan(ones(100_000), 100_000, 20) == (LISTS, 20)  # every song of the library: n x n pairs instead of 19 n x n
    assert _plan(ones(100_000), 100_000, 1)[0] == STEPS  # step 0 alone
    assert _plan(ones(100_000), 100_000, 20, workspace=100_000 * 20 * 16 - 1)[0] == STEPS  # the lists do not fit
    assert _plan(ones(100_000), 100_000, 20, workspace=100_000 * 20 * 16 + 100_000 * 4)[0] == LISTS
    assert _plan([1, 1, 1200], 100_000, 20)[0] == STEPS  # L = 1219 > BLISSGPU_KNN_MAX_K
    # adding one-seed groups never turns LISTS into STEPS
    routes = [_plan(ones(g), 50_000, 20)[0] for g in (1, 10, 100, 1000, 5000, 10_000, 25_000, 50_000, 200_000)]
    assert routes[0] == STEPS and routes[-1] == LISTS
    assert all(b == LISTS for a, b in zip(routes, routes[1:]) if a == LISTS)
    # nothing to do, and the argument checks
    assert _plan([], 100, 20)[0] == STEPS and _plan([1, 2], 0, 20)[0] == STEPS
    L, route = _ffi.lib(), C.c_int()
    off = np.array([0, 2, 1], np.uint64)
    assert L.blissgpu_chains_plan(off.ctypes.data, 2, 100, 20, 1 << 30, C.byref(route), None) == INVALID
    off = np.array([0, 1, 2], np.uint64)
    assert L.blissgpu_chains_plan(off.ctypes.data, 2, 100, 0, 1 << 30, C.byref(route), None) == INVALID
    assert L.blissgpu_chains_plan(off.ctypes.data, 2, 100, 20, 1 << 30, None, None) == INVALID
    assert L.blissgpu_chains_plan(off.ctypes.data, 2, 100, 20, 1 << 30, C.byref(route), None) == 0


# ---- playlist.chain_order: what is refused before the library is reached ----
def test_chain_order_checks_before_the_library(bliss, monkeypatch):
    from bliss_rs_amd import _ffi

    def boom():
        raise AssertionError("the library must not be reached")

    monkeypatch.setattr(_ffi, "lib", boom)
    P = bliss.playlist
    X = np.zeros((10, 23), np.float32)
    groups = [X[:1], X[1:4]]
    with pytest.raises(ValueError):
        P.chain_order([np.zeros((2, 20), np.float32)], X, 3)  # another d
    for k in (0, -1, 1025):
        with pytest.raises(ValueError):
            P.chain_order(groups, X, k)
    with pytest.raises(ValueError):
        P.chain_order(groups, X, 3, metric="manhattan")
    with pytest.raises(ValueError):
        P.chain_order(groups, X, 3, metric="mahalanobis")  # no m
    with pytest.raises(ValueError):
        P.chain_order(groups, X, 3, route="fastest")
    with pytest.raises(ValueError):
        P.chain_order([X[:1], np.zeros((30, 23), np.float32)], X, 1000, route="lists")  # L = 1029
    with pytest.raises(ValueError):
        P.chain_order((X[:4], [0, 1, 3]), X, 3)  # offsets do not end at the seed count
    with pytest.raises(ValueError):
        P.chain_order(groups, X, 3, skip=np.array([0, 1, 2]))  # flat: one entry per seed row (4)
    with pytest.raises(ValueError):
        P.chain_order(groups, X, 3, skip=[[0, 1], [2]])  # more skips than seeds
    with pytest.raises(ValueError):
        P.chain_order(groups, X, 3, skip=np.array([0, 1, 10, -1]))  # not a candidate
    forest, variance = P.ForestOptions(10, 8, None, 1, seed=1), P.VarianceWeights()
    for call in (lambda b: P.chain_order(groups, X, 3, metric=b), lambda b: P.song_chains([[]], [], 3, metric_builder=b),
                 lambda b: P.song_to_song([], [], b, number_songs=3)):
        with pytest.raises(ValueError) as e:
            call(forest)
        assert "isolation forest" in str(e.value)
        with pytest.raises(ValueError) as e:
            call(variance)
        assert "variance" in str(e.value)


# ---- song_chains / chain_playlists: the grouping, with the device call replaced by a numpy brute force ----
def _brute_force(record):
    def chain_order(seed_groups, candidates, k, metric="euclidean", m=None, skip=None, route="auto"):
        S, off = seed_groups if isinstance(seed_groups, tuple) else (
            np.concatenate([np.asarray(g, np.float32).reshape(-1, np.shape(candidates)[1]) for g in seed_groups]),
            np.concatenate([[0], np.cumsum([len(g) for g in seed_groups])]))
        S, X = np.asarray(S, np.float32), np.asarray(candidates, np.float32)
        off = np.asarray(off, np.int64)
        record.append((S.copy(), off.copy(), None if skip is None else np.asarray(skip).copy()))
        G, n = off.shape[0] - 1, X.shape[0]
        euclid = lambda a: np.sqrt(((a - X) ** 2).sum(axis=1, dtype=np.float32))  # noqa: E731
        idx, dist = np.full((G, k), -1, np.int64), np.full((G, k), np.inf, np.float32)
        for g in range(G):
            free = np.ones(n, bool)
            if skip is not None:
                sk = np.asarray(skip)[off[g]:off[g + 1]]
                free[sk[sk >= 0]] = False
            row = np.zeros(n, np.float32)
            for s in range(off[g], off[g + 1]):
                row = row + euclid(S[s])
            for t in range(k):
                if not free.any():
                    break
                j = int(np.argmin(np.where(free, row, np.inf)))
                idx[g, t], dist[g, t] = j, row[j]
                free[j] = False
                row = euclid(X[j])
        return idx, dist

    return chain_order


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


def _chain(X, seeds, k, inside):
    """the chain by hand: -> (rows, distances)"""
    euclid = lambda a: np.sqrt(((a - X) ** 2).sum(axis=1, dtype=np.float32))  # noqa: E731
    row = np.zeros(X.shape[0], np.float32)
    for s in seeds:
        row = row + euclid(X[s])
    free = np.ones(X.shape[0], bool)
    free[list(inside)] = False
    out, val = [], []
    for _ in range(k):
        j = int(np.argmin(np.where(free, row, np.inf)))
        out.append(j)
        val.append(float(row[j]))
        free[j] = False
        row = euclid(X[j])
    return out, val


def test_library_chain_playlists_by_song(bliss, tmp_path, monkeypatch):
    db, songs, X = _library(bliss, tmp_path)
    record = []
    monkeypatch.setattr(bliss.playlist, "chain_order", _brute_force(record))
    k = 6
    table = bliss.library.chain_playlists(db, k)
    assert len(record) == 1  # one call for the whole library
    S, off, skip = record[0]
    assert np.array_equal(off, np.arange(len(songs) + 1)) and np.array_equal(S, X)
    assert np.array_equal(np.asarray(skip), np.arange(len(songs)))  # every song skips its own row
    assert list(table) == [s.path for s in songs]
    for i in (0, 7, 59):
        rows, val = _chain(X, [i], k, {i})
        assert [p for p, _ in table[songs[i].path]] == [songs[j].path for j in rows]
        assert [v for _, v in table[songs[i].path]] == val
    # some songs only: the order as given
    some = [songs[9].path, songs[2].path]
    table = bliss.library.chain_playlists(db, k, song_paths=some)
    assert list(table) == some and np.array_equal(np.asarray(record[1][2]), [9, 2])
    assert [p for p, _ in table[some[0]]] == [songs[j].path for j in _chain(X, [9], k, {9})[0]]
    with pytest.raises(bliss.ProviderError):
        bliss.library.chain_playlists(db, k, song_paths=[songs[1].path, "/music/none.flac"])
    assert bliss.library.chain_playlists(db, k, song_paths=[]) == {}


@pytest.mark.parametrize("by", ("album", "artist", "album_artist", "genre"))
def test_library_chain_playlists_grouping(bliss, tmp_path, monkeypatch, by):
    db, songs, X = _library(bliss, tmp_path)
    record = []
    monkeypatch.setattr(bliss.playlist, "chain_order", _brute_force(record))
    k = 5
    table = bliss.library.chain_playlists(db, k, by=by)
    assert len(record) == 1
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
        want, val = _chain(X, members[key], k, set(members[key]))
        assert [p for p, _ in table[key]] == [songs[j].path for j in want]
        assert [v for _, v in table[key]] == val
        assert not ({int(p[7:10]) for p, _ in table[key]} & set(members[key]))  # the members stay out


def test_library_chain_playlists_custom_groups_and_refusals(bliss, tmp_path, monkeypatch):
    db, songs, X = _library(bliss, tmp_path)
    record = []
    monkeypatch.setattr(bliss.playlist, "chain_order", _brute_force(record))
    path = lambda i: songs[i].path  # noqa: E731
    groups = {"evening": [path(9), path(2), path(9)], "one": [path(40)], "none": []}
    table = bliss.library.chain_playlists(db, 4, groups=groups)
    S, off, skip = record[0]
    assert list(table) == ["evening", "one", "none"]
    assert np.array_equal(off, [0, 3, 4, 4]) and np.array_equal(np.asarray(skip), [9, 2, 9, 40])  # order as given, twice a seed
    assert np.array_equal(S, X[[9, 2, 9, 40]])
    assert [p for p, _ in table["evening"]] == [path(j) for j in _chain(X, [9, 2, 9], 4, {9, 2})[0]]
    assert table["none"][0] == (path(0), 0.0)  # an empty seed set starts at the first candidate, score 0
    assert [p for p, _ in table["none"]] == [path(j) for j in _chain(X, [], 4, set())[0]]
    with pytest.raises(bliss.ProviderError):
        bliss.library.chain_playlists(db, 4, groups={"x": [path(1), "/music/none.flac"]})
    with pytest.raises(ValueError):
        bliss.library.chain_playlists(db, 4, by="year")
    P = bliss.playlist
    for builder, word in ((P.VarianceWeights(), "variance"), (P.ForestOptions(10, 8, None, 1, seed=1), "isolation forest")):
        with pytest.raises(ValueError) as e:
            bliss.library.chain_playlists(db, 4, metric_builder=builder)
        assert word in str(e.value)
    assert len(record) == 1


def test_song_chains_objects(bliss, tmp_path, monkeypatch):
    _, songs, X = _library(bliss, tmp_path, n=30)
    record = []
    monkeypatch.setattr(bliss.playlist, "chain_order", _brute_force(record))
    P = bliss.playlist
    groups = [[songs[4], songs[11]], [], [songs[20]]]
    got = P.song_chains(groups, songs, 5)
    S, off, skip = record[0]
    assert np.array_equal(off, [0, 2, 2, 3]) and np.array_equal(np.asarray(skip), [4, 11, 20])
    assert [s.path for s in got[0]] == [songs[j].path for j in _chain(X, [4, 11], 5, {4, 11})[0]]
    assert [s.path for s in got[1]] == [songs[j].path for j in _chain(X, [], 5, set())[0]]
    assert [s.path for s in got[2]] == [songs[j].path for j in _chain(X, [20], 5, {20})[0]]
    # members kept as candidates
    got = P.song_chains(groups, songs, 5, exclude_members=False)
    assert record[1][2] is None and got[2][0] is songs[20]
    assert P.song_chains([], songs, 5) == [] and P.song_chains(groups, [], 5) == [[], [], []]
    assert len(record) == 2


def test_song_to_song_order_without_k_is_the_full_chain(bliss, monkeypatch):
    """k=None must still reach blissgpu_song_to_song; k given goes through chain_order as ONE group."""
    from bliss_rs_amd import _ffi

    called = []

    class Lib:
        def blissgpu_song_to_song(self, *args):
            called.append(args)
            return 0

    monkeypatch.setattr(_ffi, "lib", lambda: Lib())
    P = bliss.playlist
    X = np.arange(12, dtype=np.float32).reshape(6, 2)
    P.song_to_song_order(X[:1], X)
    assert len(called) == 1 and called[0][1] == 1 and called[0][3] == 6
    seen = []

    def chain_order(seed_groups, candidates, k, metric="euclidean", m=None, skip=None, route="auto"):
        seen.append((len(seed_groups), np.asarray(seed_groups[0]).shape, k, skip))
        return np.array([[3, 1, -1][:k]], np.int64), np.zeros((1, k), np.float32)

    monkeypatch.setattr(P, "chain_order", chain_order)
    assert P.song_to_song_order(X[:2], X, k=3).tolist() == [3, 1]
    assert P.song_to_song_order(X[:2], X, k=100).tolist() == [3, 1]  # (cut at the candidates: take(k) of a shorter iterator)
    assert seen == [(1, (2, 2), 3, None), (1, (2, 2), 6, None)] and len(called) == 1
    assert P.song_to_song_order(X[:2], X, k=0).tolist() == []
