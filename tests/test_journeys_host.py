"""Device-free tests of the journeys (blissgpu_journeys / blissgpu_journeys_device): the C ABI surface, the argument checks that
happen before the device is touched, and the host logic of playlist.journey_order / waypoint_playlist / directed_playlist and
library.waypoint_playlists / directed_playlists (with the device call replaced by a numpy brute force)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
INVALID = 2
CHAIN, WAYPOINT = 0, 1
NONE, UP, DOWN = 0, 1, 2


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


def test_journeys_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    lib = C.CDLL(bliss.LIB_PATH)
    for name in ("blissgpu_journeys", "blissgpu_journeys_device"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name
    for name, value in (("JOURNEY_CHAIN", 0), ("JOURNEY_WAYPOINT", 1), ("GATE_NONE", 0), ("GATE_UP", 1), ("GATE_DOWN", 2)):
        assert re.search(r"#define\s+BLISSGPU_%s\s+%d\b" % (name, value), header), name
        assert getattr(_ffi, name) == value
    u64, u32 = C.c_uint64, C.c_uint32
    # (from, to, n_journeys, cand, n, d, metric, M, skip, k, mode, gate, gate_feature, idx, dist), the device form with the context in front
    host = [_vp, _vp, u64, _vp, u64, u32, C.c_int, _vp, _vp, u32, C.c_int, C.c_int, u32, _vp, _vp]
    assert _ffi.SIGNATURES["blissgpu_journeys"] == (C.c_int, host)
    assert _ffi.SIGNATURES["blissgpu_journeys_device"] == (C.c_int, [_vp] + host)
    # the header's parameter lists, type by type
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    types = lambda name: [re.sub(r"\s*\w+$", "", re.sub(r"\s+", " ", a.strip())).replace(" *", "*")  # noqa: E731
                          for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, flat).group(1).split(",")]
    want = ["const float*", "const float*", "uint64_t", "const float*", "uint64_t", "uint32_t", "int", "const float*",
            "const uint32_t*", "uint32_t", "int", "int", "uint32_t", "uint32_t*", "float*"]
    assert types("blissgpu_journeys") == want
    assert types("blissgpu_journeys_device") == ["blissgpu_ctx*"] + want
    # the header cites the two roadmap items the feature answers
    assert "A waypoint feature" in header and "A direction feature" in header
    # the step kernel is in the profiling table, once, behind every older name
    L = _ffi.lib()
    table = [L.blissgpu_profile_kernel_name(i).decode() for i in range(L.blissgpu_profile_kernel_count())]
    assert table.count("journey_step_kernel") == 1 and len(set(table)) == len(table)
    assert table[-1] == "journey_step_kernel" and table.index("group_forest_scan_kernel") == len(table) - 2


def _p(a):
    return None if a is None else a.ctypes.data


def _call(A, B, X, k, d=None, metric=0, M=None, skip=None, mode=None, gate=NONE, feature=0, idx=True, device_form=False, G=None):
    from bliss_rs_amd import _ffi

    G = A.shape[0] if G is None else G
    n = 0 if X is None else X.shape[0]
    d = X.shape[1] if d is None else d
    mode = (CHAIN if B is None else WAYPOINT) if mode is None else mode
    rows = max(1 if A is None else A.shape[0], 1)
    out_i, out_d = np.zeros((rows, max(k, 1)), np.uint32), np.zeros((rows, max(k, 1)), np.float32)
    args = (_p(A), _p(B), G, _p(X), n, d, metric, _p(M), _p(skip), k, mode, gate, feature, _p(out_i) if idx else None, _p(out_d))
    if device_form:  # a NULL context: everything about the arguments is said before the context is looked at
        return _ffi.lib().blissgpu_journeys_device(None, *args)
    return _ffi.lib().blissgpu_journeys(*args)


def test_journeys_arguments_are_checked_before_the_device(bliss):
    import torch

    from bliss_rs_amd import _ffi

    err = lambda: _ffi.lib().blissgpu_last_error()  # noqa: E731
    rng = np.random.default_rng(0)
    X = rng.standard_normal((50, 23)).astype(np.float32)
    A, B = X[:4].copy(), X[10:14].copy()
    big = np.zeros((50, 65), np.float32)
    for dev in (False, True):
        bad = [
            _call(A, None, X, 0, device_form=dev), _call(A, None, X, 1025, device_form=dev),
            _call(A, None, X, 3, d=0, device_form=dev), _call(big[:4], None, big, 3, device_form=dev),
            _call(A, None, X, 3, metric=2, M=None, device_form=dev), _call(A, None, X, 3, metric=3, device_form=dev),
            _call(A, None, X, 3, metric=-1, device_form=dev),
            _call(A, None, X, 3, mode=2, device_form=dev), _call(A, None, X, 3, mode=-1, device_form=dev),
            _call(A, None, X, 3, gate=3, device_form=dev), _call(A, None, X, 3, gate=-1, device_form=dev),
            _call(A, B, X, 3, gate=UP, device_form=dev), _call(A, B, X, 3, gate=DOWN, device_form=dev),  # a gate with WAYPOINT
            _call(A, None, X, 3, gate=DOWN, feature=23, device_form=dev), _call(A, None, X, 3, gate=UP, feature=0xFFFFFFFF, device_form=dev),
            _call(A, None, X, 3, mode=WAYPOINT, device_form=dev),  # WAYPOINT without to
            _call(A, B, X, 3, mode=CHAIN, device_form=dev),  # to without WAYPOINT
            _call(None, None, X, 3, G=4, device_form=dev), _call(A, None, X, 3, idx=False, device_form=dev),
            _call(A, None, X, 3, G=1 << 31, device_form=dev),
        ]
        assert all(rc == INVALID for rc in bad), (dev, bad)
        assert b"ctx" not in err()
    assert _call(A, B, X, 3, gate=DOWN) == INVALID and b"gate" in err()
    assert _call(A, None, X, 3, gate=DOWN, feature=23) == INVALID and b"gate_feature" in err()
    # the candidates are missing only when there are some
    out = np.zeros((4, 3), np.uint32)
    assert _ffi.lib().blissgpu_journeys(_p(A), None, 4, None, 5, 23, 0, None, None, 3, CHAIN, NONE, 0, _p(out), None) == INVALID
    # a skip entry that is no candidate and not 0xFFFFFFFF (host form: the device form cannot read it without the device)
    skip = np.full((4, 2), 0xFFFFFFFF, np.uint32)
    skip[2, 1] = X.shape[0]
    assert _call(A, None, X, 3, skip=skip) == INVALID and b"skip" in err()
    # the device form with valid arguments then looks at its (NULL) context
    assert _call(A, None, X, 3, device_form=True) == INVALID and b"ctx" in err()
    # nothing to do
    assert _call(A[:0], None, X, 3) == 0 and _call(A[:0], B[:0], X, 3) == 0
    # a gate's feature is not looked at without a gate
    skip[2, 1] = 7
    no_device = 0 if torch.cuda.is_available() else 1  # BLISSGPU_ERR_NO_DEVICE without a GPU, BLISSGPU_OK with one
    assert _call(A, None, X, 3, skip=skip, feature=99) == no_device
    assert _call(A, B, X, 3, skip=skip) == no_device
    assert _call(A, None, X, 3, gate=DOWN, feature=22) == no_device
    assert _call(A, None, X[:0], 3) == no_device  # (no candidates: every row is padding, still a call that needs its context)


# ---- playlist.journey_order: what is refused before the library is reached ----
def test_journey_order_checks_before_the_library(bliss, monkeypatch):
    from bliss_rs_amd import _ffi

    def boom():
        raise AssertionError("the library must not be reached")

    monkeypatch.setattr(_ffi, "lib", boom)
    P = bliss.playlist
    X = np.zeros((10, 23), np.float32)
    A, B = X[:3], X[3:6]
    with pytest.raises(ValueError):
        P.journey_order(np.zeros((2, 20), np.float32), X, 3)  # another d
    with pytest.raises(ValueError):
        P.journey_order(A, X, 3, to_rows=X[:2])  # another number of journeys
    for k in (0, -1, 1025):
        with pytest.raises(ValueError):
            P.journey_order(A, X, k)
    with pytest.raises(ValueError):
        P.journey_order(A, X, 3, metric="manhattan")
    with pytest.raises(ValueError):
        P.journey_order(A, X, 3, metric="mahalanobis")  # no m
    with pytest.raises(ValueError):
        P.journey_order(A, X, 3, metric="mahalanobis", m=np.eye(20, dtype=np.float32))
    with pytest.raises(ValueError):
        P.journey_order(A, X, 3, direction="sideways", feature=0)
    with pytest.raises(ValueError):
        P.journey_order(A, X, 3, direction="down")  # no feature
    with pytest.raises(ValueError):
        P.journey_order(A, X, 3, direction="down", feature=23)
    with pytest.raises(ValueError):
        P.journey_order(A, X, 3, to_rows=B, direction="down", feature=0)  # a gate with waypoints
    with pytest.raises(ValueError):
        P.journey_order(A, X, 3, skip=np.array([0, 1, 2]))  # not [G, 2]
    with pytest.raises(ValueError):
        P.journey_order(A, X, 3, skip=np.array([[0, 1], [2, 10], [3, -1]]))  # not a candidate
    forest, variance = P.ForestOptions(10, 8, None, 1, seed=1), P.VarianceWeights()
    calls = (lambda b: P.journey_order(A, X, 3, metric=b), lambda b: P.waypoint_playlist(None, None, [], 3, metric_builder=b),
             lambda b: P.directed_playlist(None, [], 3, 0, metric_builder=b),
             lambda b: bliss.library.waypoint_playlists(None, [], 3, metric_builder=b),
             lambda b: bliss.library.directed_playlists(None, 3, metric_builder=b))
    for call in calls:
        with pytest.raises(ValueError) as e:
            call(forest)
        assert "isolation forest" in str(e.value)
        with pytest.raises(ValueError) as e:
            call(variance)
        assert "variance" in str(e.value)
    with pytest.raises(ValueError):
        P.directed_playlist(None, [], 3, 0, direction="sideways")
    with pytest.raises(ValueError):
        bliss.library.directed_playlists(None, 3, direction=None)


def test_journey_order_arguments_reach_the_library(bliss, monkeypatch):
    """the host wrapper's translation: -1 -> 0xFFFFFFFF, AnalysisIndex -> column, to_rows -> WAYPOINT, padding -> -1"""
    from bliss_rs_amd import _ffi

    seen = []

    class Lib:
        def blissgpu_journeys(self, a, b, G, x, n, d, metric, m, skip, k, mode, gate, feature, idx, dist):
            sk = None if skip is None else np.ctypeslib.as_array(C.cast(C.c_void_p(skip), C.POINTER(C.c_uint32)), (G, 2)).copy()
            seen.append((b is not None, G, n, d, metric, sk, k, mode, gate, feature))
            out = np.ctypeslib.as_array(C.cast(C.c_void_p(idx), C.POINTER(C.c_uint32)), (G, k))
            out[:] = 0xFFFFFFFF
            out[:, 0] = 5
            return 0

    monkeypatch.setattr(_ffi, "lib", lambda: Lib())
    P = bliss.playlist
    X = np.zeros((10, 23), np.float32)
    idx, _ = P.journey_order(X[:2], X, 3, skip=[[0, -1], [1, 9]], direction="down", feature=bliss.AnalysisIndex.MeanLoudness)
    assert idx.tolist() == [[5, -1, -1], [5, -1, -1]]
    assert seen[0][:5] == (False, 2, 10, 23, 0) and seen[0][5].tolist() == [[0, 0xFFFFFFFF], [1, 9]]
    assert seen[0][6:] == (3, CHAIN, DOWN, 8)
    P.journey_order(X[:2], X, 4, to_rows=X[2:4], metric="cosine")
    assert seen[1][:5] == (True, 2, 10, 23, 1) and seen[1][5] is None and seen[1][6:] == (4, WAYPOINT, NONE, 0)
    P.journey_order(X[:1], X, 4, direction="up", feature=22)
    assert seen[2][6:] == (4, CHAIN, UP, 22)


# ---- the song-level helpers, with the device call replaced by a numpy brute force ----
def _brute_force(record):
    def journey_order(from_rows, candidates, k, to_rows=None, metric="euclidean", m=None, skip=None, direction=None, feature=None):
        A, X = np.asarray(from_rows, np.float32), np.asarray(candidates, np.float32)
        B = None if to_rows is None else np.asarray(to_rows, np.float32)
        record.append((A.copy(), None if B is None else B.copy(), None if skip is None else np.asarray(skip).copy(), direction, feature))
        G, n = A.shape[0], X.shape[0]
        euclid = lambda a: np.sqrt(((a - X) ** 2).sum(axis=1, dtype=np.float32))  # noqa: E731
        idx, dist = np.full((G, k), -1, np.int64), np.full((G, k), np.inf, np.float32)
        for g in range(G):
            free = np.ones(n, bool)
            if skip is not None:
                sk = np.asarray(skip)[g]
                free[sk[sk >= 0]] = False
            q, ref = A[g], None if feature is None else A[g, feature]
            for t in range(k):
                if B is not None:
                    q = A[g] + (B[g] - A[g]) * (np.float32(t + 1) / np.float32(k + 1))
                ok = free.copy()
                if direction is not None:
                    ok &= (X[:, feature] <= ref) if direction == "down" else (X[:, feature] >= ref)
                if not ok.any():
                    break
                row = euclid(q)
                j = int(np.argmin(np.where(ok, row, np.inf)))
                idx[g, t], dist[g, t] = j, row[j]
                free[j] = False
                q, ref = X[j], None if feature is None else X[j, feature]
        return idx, dist

    return journey_order


def _library(bliss, tmp_path, n=60):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, 23)).astype(np.float32)
    V2 = bliss.FeaturesVersion.Version2
    songs = [bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist=f"artist{i % 5}", album=f"album{i % 9}", duration=1.0,
                        analysis=bliss.Analysis(X[i], V2), features_version=V2) for i in range(n)]
    db = str(tmp_path / "bliss.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs)
    return db, songs, X


def test_waypoint_helpers(bliss, tmp_path, monkeypatch):
    db, songs, X = _library(bliss, tmp_path)
    record = []
    brute = _brute_force(record)
    monkeypatch.setattr(bliss.playlist, "journey_order", brute)
    P, k = bliss.playlist, 6
    path = lambda i: songs[i].path  # noqa: E731
    pairs = [(path(3), path(40)), (path(40), path(3)), (path(7), path(7)), (path(59), path(0))]
    ends = np.array([[3, 40], [40, 3], [7, 7], [59, 0]])
    got = bliss.library.waypoint_playlists(db, pairs, k)
    assert len(record) == 1  # one call for every pair
    A, B, skip, direction, feature = record[0]
    assert np.array_equal(A, X[ends[:, 0]]) and np.array_equal(B, X[ends[:, 1]]) and np.array_equal(skip, ends)
    assert direction is None and feature is None
    want = brute(X[ends[:, 0]], X, k, X[ends[:, 1]], skip=ends)[0]
    for g, row in enumerate(got):
        assert [s.path for s in row] == [path(j) for j in want[g]] and len(row) == k
        assert not {s.path for s in row} & set(pairs[g])  # the end points are absent
    assert [s.path for s in got[0]] != [s.path for s in got[1]]  # a direction of travel
    assert bliss.library.waypoint_playlists(db, [], k) == []
    with pytest.raises(bliss.ProviderError):
        bliss.library.waypoint_playlists(db, [(path(1), "/music/none.flac")], k)
    # the song form: the end points need not be candidates; those that are, are skipped
    record.clear()
    pool = songs[:30]
    one = P.waypoint_playlist(songs[4], songs[45], pool, k)
    A, B, skip, _, _ = record[0]
    assert np.array_equal(A, X[[4]]) and np.array_equal(B, X[[45]]) and skip.tolist() == [[4, -1]]
    assert [s.path for s in one] == [path(j) for j in brute(X[[4]], X[:30], k, X[[45]], skip=[[4, -1]])[0][0]]
    assert songs[4] not in one and len(one) == k
    assert P.waypoint_playlist(songs[4], songs[45], [], k) == []
    # fewer candidates than songs asked for: what there is
    assert len(P.waypoint_playlist(songs[0], songs[1], songs[:5], k)) == 3


def test_directed_helpers(bliss, tmp_path, monkeypatch):
    db, songs, X = _library(bliss, tmp_path)
    record = []
    brute = _brute_force(record)
    monkeypatch.setattr(bliss.playlist, "journey_order", brute)
    P, k = bliss.playlist, 6
    n = len(songs)
    table = bliss.library.directed_playlists(db, k)
    assert len(record) == 1  # one call for the whole library
    A, B, skip, direction, feature = record[0]
    assert np.array_equal(A, X) and B is None and direction == "down" and feature == 0 and type(feature) is int
    assert np.array_equal(skip, np.stack([np.arange(n), np.full(n, -1)], axis=1))  # every song skips its own row
    assert list(table) == [s.path for s in songs]
    short = 0
    for g, s in enumerate(songs):
        line = [X[g, 0]] + [t.analysis.as_vec()[0] for t in table[s.path]]
        assert all(b <= a for a, b in zip(line, line[1:])) and s.path not in [t.path for t in table[s.path]]
        short += len(table[s.path]) < k
    assert short >= 1 and any(len(v) == k for v in table.values())  # the lowest tempos run out of songs, the others do not
    # another feature, upwards, some songs only, in the order given
    some = [songs[9].path, songs[2].path]
    table = bliss.library.directed_playlists(db, k, bliss.AnalysisIndex.Chroma13, "up", song_paths=some)
    assert list(table) == some and record[1][2].tolist() == [[9, -1], [2, -1]] and record[1][3:] == ("up", 22)
    line = [X[9, 22]] + [t.analysis.as_vec()[22] for t in table[some[0]]]
    assert all(b >= a for a, b in zip(line, line[1:]))
    assert bliss.library.directed_playlists(db, k, song_paths=[]) == {}
    with pytest.raises(bliss.ProviderError):
        bliss.library.directed_playlists(db, k, song_paths=[songs[1].path, "/music/none.flac"])
    # the song form
    record.clear()
    one = P.directed_playlist(songs[9], songs, k, bliss.AnalysisIndex.Chroma13, "up")
    assert record[0][2].tolist() == [[9, -1]] and record[0][3:] == ("up", 22)
    assert [s.path for s in one] == [s.path for s in table[some[0]]]
    assert P.directed_playlist(songs[9], [], k, 0) == []
