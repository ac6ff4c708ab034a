"""Device-free tests of the per-group diagonal metric (blissgpu_group_weights / blissgpu_group_knn_weighted and their device
forms): the C ABI surface, the argument checks that happen before the device is touched, the few-seeds policy of
playlist.VarianceWeights (decided from the group sizes before the library is reached), the refusals of the entry points that
build one-song metrics, and how library.group_playlists / playlist_from_custom hand the builder on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
NO_DEVICE, INVALID = 1, 2


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


def test_group_weights_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    lib = C.CDLL(bliss.LIB_PATH)
    names = ("blissgpu_group_weights", "blissgpu_group_weights_device", "blissgpu_group_knn_weighted",
             "blissgpu_group_knn_weighted_device")
    for name in names:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name
    assert re.search(r"#define\s+BLISSGPU_GROUP_OK\s+0\b", header)
    assert re.search(r"#define\s+BLISSGPU_GROUP_TOO_FEW_SEEDS\s+1\b", header)
    u64, u32 = C.c_uint64, C.c_uint32
    # (seeds, group_offsets, n_groups, d, weights, group_status), the device form with the context in front
    w_host = [_vp, _vp, u64, u32, _vp, _vp]
    assert _ffi.SIGNATURES["blissgpu_group_weights"] == (C.c_int, w_host)
    assert _ffi.SIGNATURES["blissgpu_group_weights_device"] == (C.c_int, [_vp] + w_host)
    # (seeds, group_offsets, n_groups, cand, n, d, weights, skip, k, idx, dist, group_status)
    k_host = [_vp, _vp, u64, _vp, u64, u32, _vp, _vp, u32, _vp, _vp, _vp]
    assert _ffi.SIGNATURES["blissgpu_group_knn_weighted"] == (C.c_int, k_host)
    assert _ffi.SIGNATURES["blissgpu_group_knn_weighted_device"] == (C.c_int, [_vp] + k_host)
    # the header's parameter lists, type by type
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    types = lambda name: [re.sub(r"\s*\w+$", "", re.sub(r"\s+", " ", a.strip())).replace(" *", "*")  # noqa: E731
                          for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, flat).group(1).split(",")]
    want_w = ["const float*", "const uint64_t*", "uint64_t", "uint32_t", "float*", "int32_t*"]
    assert types("blissgpu_group_weights") == want_w
    assert types("blissgpu_group_weights_device") == ["blissgpu_ctx*"] + want_w
    want_k = ["const float*", "const uint64_t*", "uint64_t", "const float*", "uint64_t", "uint32_t", "const float*",
              "const uint32_t*", "uint32_t", "uint32_t*", "float*", "int32_t*"]
    assert types("blissgpu_group_knn_weighted") == want_k
    assert types("blissgpu_group_knn_weighted_device") == ["blissgpu_ctx*"] + want_k
    # the existing declarations did not move
    assert types("blissgpu_group_knn") == ["const float*", "const uint64_t*", "uint64_t", "const float*", "uint64_t", "uint32_t",
                                           "int", "const float*", "const uint32_t*", "uint32_t", "uint32_t*", "float*"]
    # the new kernel appears in the profiling table like the others
    L = _ffi.lib()
    table = [L.blissgpu_profile_kernel_name(i).decode() for i in range(L.blissgpu_profile_kernel_count())]
    assert "group_weights_kernel" in table and table.count("group_knn_scan_kernel") == 1


def _p(a):
    return None if a is None else a.ctypes.data


def _knn(S, off, X, k, d=None, weights=None, skip=None, idx=True, status=True, device_form=False):
    from bliss_rs_amd import _ffi

    off = np.asarray(off, np.uint64)
    G, n = off.shape[0] - 1, X.shape[0]
    d = X.shape[1] if d is None else d
    out_i, out_d = np.zeros((G, max(k, 1)), np.uint32), np.zeros((G, max(k, 1)), np.float32)
    st = np.zeros(max(G, 1), np.int32)
    args = (_p(S), _p(off), G, _p(X), n, d, _p(weights), _p(skip), k, _p(out_i) if idx else None, _p(out_d),
            _p(st) if status else None)
    if device_form:  # a NULL context: everything about the arguments is said before the context is looked at
        return _ffi.lib().blissgpu_group_knn_weighted_device(None, *args)
    return _ffi.lib().blissgpu_group_knn_weighted(*args)


def _weights(S, off, d=None, out=True, device_form=False):
    from bliss_rs_amd import _ffi

    off = np.asarray(off, np.uint64)
    G = off.shape[0] - 1
    d = S.shape[1] if d is None else d
    w, st = np.zeros((max(G, 1), max(d, 1)), np.float32), np.zeros(max(G, 1), np.int32)
    args = (_p(S), _p(off), G, d, _p(w) if out else None, _p(st))
    if device_form:
        return _ffi.lib().blissgpu_group_weights_device(None, *args)
    return _ffi.lib().blissgpu_group_weights(*args)


def test_arguments_are_checked_before_the_device(bliss):
    import torch

    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    max_k = int(re.search(r"#define\s+BLISSGPU_KNN_MAX_K\s+(\d+)", header).group(1))
    rng = np.random.default_rng(0)
    X = rng.standard_normal((50, 23)).astype(np.float32)
    S = X[:6].copy()
    off = [0, 1, 4, 4, 6]
    W = np.ones((4, 23), np.float32)
    err = lambda: _ffi.lib().blissgpu_last_error()  # noqa: E731
    for dev in (False, True):
        for w in (None, W):
            assert _knn(S, off, X, 0, weights=w, device_form=dev) == INVALID and b"ctx" not in err()
            assert _knn(S, off, X, max_k + 1, weights=w, device_form=dev) == INVALID and b"ctx" not in err()
            assert _knn(S, off, X, 3, d=0, weights=w, device_form=dev) == INVALID and b"ctx" not in err()
            assert _knn(np.zeros((6, 65), np.float32), off, np.zeros((50, 65), np.float32), 3, d=65, weights=w,
                        device_form=dev) == INVALID and b"ctx" not in err()
            assert _knn(S, [1, 1, 4, 4, 6], X, 3, weights=w, device_form=dev) == INVALID and b"ctx" not in err()
            assert _knn(S, [0, 4, 1, 4, 6], X, 3, weights=w, device_form=dev) == INVALID and b"ctx" not in err()
            assert _knn(S, off, X, 3, weights=w, idx=False, device_form=dev) == INVALID and b"ctx" not in err()
            assert _knn(None, off, X, 3, weights=w, device_form=dev) == INVALID and b"ctx" not in err()
        assert _weights(S, off, d=0, device_form=dev) == INVALID and b"ctx" not in err()
        assert _weights(np.zeros((6, 65), np.float32), off, device_form=dev) == INVALID and b"ctx" not in err()
        assert _weights(S, [1, 1, 4, 4, 6], device_form=dev) == INVALID and b"ctx" not in err()
        assert _weights(S, [0, 4, 1, 4, 6], device_form=dev) == INVALID and b"ctx" not in err()
        assert _weights(S, off, out=False, device_form=dev) == INVALID and b"weights" in err()
        assert _weights(None, off, d=23, device_form=dev) == INVALID and b"ctx" not in err()
    # a skip entry that is no candidate: the host form checks it on the host
    skip = np.full(6, 0xFFFFFFFF, np.uint32)
    skip[3] = X.shape[0]
    for w in (None, W):
        assert _knn(S, off, X, 3, weights=w, skip=skip) == INVALID and b"skip" in err()
    # the device forms with good arguments get as far as their (NULL) context
    assert _knn(S, off, X, 3, device_form=True) == INVALID and b"ctx" in err()
    assert _weights(S, off, device_form=True) == INVALID and b"ctx" in err()
    # nothing to do; the status pointer may be NULL
    assert _knn(S[:0], [0], X, 3) == 0 and _weights(S[:0], [0]) == 0
    # valid calls: BLISSGPU_ERR_NO_DEVICE without a GPU, BLISSGPU_OK with one
    ok = 0 if torch.cuda.is_available() else NO_DEVICE
    skip[3] = 0
    assert _knn(S, off, X, 3, skip=skip) == ok
    assert _knn(S, off, X, 3, weights=W, status=False) == ok
    assert _weights(S, off) == ok


def _boom():
    raise AssertionError("the library must not be reached")


def test_variance_weights_policy_is_decided_before_the_library(bliss, monkeypatch):
    from bliss_rs_amd import _ffi

    P = bliss.playlist
    monkeypatch.setattr(_ffi, "lib", _boom)
    X = np.zeros((10, 23), np.float32)
    with pytest.raises(ValueError):
        P.VarianceWeights(few_seeds="ignore")
    assert P.VarianceWeights().few_seeds == "raise"
    for groups in ([X[:1], X[1:4]], [X[:3], X[:0]], (X[:4], [0, 2, 2, 4])):
        with pytest.raises(bliss.ProviderError) as e:
            P.nearest_to_groups(groups, X, 3, metric=P.VarianceWeights())
        assert "seeds must contain more than one element" in str(e.value)
    with pytest.raises(bliss.ProviderError):
        P.set_distances(X[:1], X, P.VarianceWeights())
    with pytest.raises(bliss.ProviderError):
        P.closest_to_songs_order(X[:1], X, P.VarianceWeights())
    # the checks nearest_to_groups makes for every metric hold for the per-group ones, too
    with pytest.raises(ValueError):
        P.nearest_to_groups([X[:2], X[2:4]], X, 0, metric="variance")
    with pytest.raises(ValueError):
        P.nearest_to_groups([X[:2], X[2:4]], X, 3, metric="diagonal")  # no m
    with pytest.raises(ValueError):
        P.nearest_to_groups([X[:2], X[2:4]], X, 3, metric="diagonal", m=np.ones((23, 23), np.float32))  # not [G, d]
    with pytest.raises(ValueError):
        P.nearest_to_groups([X[:2], X[2:4]], X, 3, metric="variance", skip=np.array([0, 1, 10, -1]))
    with pytest.raises(ValueError):
        P.nearest_to_groups([X[:2], X[2:4]], X, 3, metric="manhattan")


class _Song:
    def __init__(self, bliss, row):
        self.analysis = bliss.Analysis(row, bliss.FeaturesVersion.Version2)
        self.title = self.artist = None


def test_one_song_metrics_refuse_variance_weights(bliss, monkeypatch, tmp_path):
    from bliss_rs_amd import _ffi

    P, L = bliss.playlist, bliss.library
    monkeypatch.setattr(_ffi, "lib", _boom)
    rng = np.random.default_rng(1)
    songs = [_Song(bliss, r) for r in rng.standard_normal((6, 23)).astype(np.float32)]
    vw = P.VarianceWeights()
    for call in (lambda: P.song_to_song(songs[:2], songs[2:], vw),
                 lambda: P.dedup_playlist_custom_distance(songs, None, vw),
                 lambda: P.nearest_songs(songs[:2], songs, 3, vw),
                 lambda: P.duplicate_groups(songs, None, vw),
                 lambda: L.similar_songs(":memory:", 3, vw),
                 lambda: L.duplicate_songs(":memory:", None, vw),
                 lambda: L.playlist_from_custom(":memory:", ["/a", "/b"], vw, P.closest_to_songs, True),
                 lambda: L.playlist_from_custom(":memory:", ["/a", "/b"], vw, P.song_to_song, False)):
        with pytest.raises(ValueError) as e:
            call()
        assert "variance-based weights need a seed set" in str(e.value)
    with pytest.raises(bliss.ProviderError):  # one initial song: the reference's error, before the database is opened
        L.playlist_from_custom(":memory:", ["/a"], vw, P.closest_to_songs, False)
    with pytest.raises(bliss.ProviderError):
        P.group_playlists([songs[:2], songs[2:3]], songs, 3, vw)
    with pytest.raises(TypeError):  # the one-metric builders still do not know it
        P._metric_of(vw)


def _library(bliss, tmp_path, n=40):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, 23)).astype(np.float32)
    V2 = bliss.FeaturesVersion.Version2
    songs = [bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist="a", album=f"album{i % 7}" if i else "alone",
                        duration=1.0, analysis=bliss.Analysis(X[i], V2), features_version=V2) for i in range(n)]
    db = str(tmp_path / "bliss.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs)
    return db, songs, X


def test_library_hands_the_builder_on_in_one_call(bliss, tmp_path, monkeypatch):
    db, songs, X = _library(bliss, tmp_path)
    P = bliss.playlist
    record = []

    def fake(seed_groups, candidates, k, metric="euclidean", m=None, skip=None):
        S, off = seed_groups
        record.append((np.asarray(S).copy(), np.asarray(off).copy(), metric, m, np.asarray(skip).copy()))
        G = len(off) - 1
        return np.tile(np.arange(k), (G, 1)), np.zeros((G, k), np.float32)

    monkeypatch.setattr(P, "nearest_to_groups", fake)
    vw = P.VarianceWeights(few_seeds="euclidean")
    table = bliss.library.group_playlists(db, 4, by="album", metric_builder=vw)
    assert len(record) == 1 and record[0][2] is vw and record[0][3] is None  # ONE call, the builder itself as the metric
    S, off, _, _, skip = record[0]
    assert list(table)[0] == "alone" and np.array_equal(off[:2], [0, 1])  # the single-song album is a group of one seed
    assert np.array_equal(S, X[skip]) and off[-1] == len(songs)
    monkeypatch.undo()
    # the default policy refuses that album from the group sizes alone: the library is not reached
    from bliss_rs_amd import _ffi

    monkeypatch.setattr(_ffi, "lib", _boom)
    with pytest.raises(bliss.ProviderError) as e:
        bliss.library.group_playlists(db, 4, by="album", metric_builder=P.VarianceWeights())
    assert "seeds must contain more than one element" in str(e.value)


def test_one_seed_set_entry_points_take_the_host_matrix(bliss, oracle, tmp_path, monkeypatch):
    """closest_to_songs / set_distances / playlist_from_custom(deduplicate=False) build ONE metric from ONE seed set: they compute
    M with the host arithmetic (held to the oracle bit for bit here) and take the existing device call with it."""
    db, songs, X = _library(bliss, tmp_path)
    P = bliss.playlist
    seeds = X[[3, 10, 17]]
    M = oracle.variance_based_weight_matrix(seeds)
    assert np.array_equal(P.variance_based_weight_matrix(list(seeds)).view(np.uint32), M.view(np.uint32))
    assert P.VarianceWeights(few_seeds="euclidean").matrix(seeds[:1]) == ("euclidean", None)
    seen = []

    def fake_order(S, C_, metric="euclidean", m=None):
        seen.append((np.asarray(S).copy(), metric, None if m is None else np.asarray(m).copy()))
        return np.arange(len(C_), dtype=np.uint32), np.zeros(len(C_), np.float32)

    real = P.closest_to_songs_order
    monkeypatch.setattr(_ffi_of(bliss), "lib", lambda: _FakeLib(seen))
    order, _ = real(seeds, X, P.VarianceWeights())
    assert seen[-1][0] == "blissgpu_closest_to_songs" and seen[-1][1] == 2  # Mahalanobis
    assert np.array_equal(seen[-1][2].view(np.uint32), M.view(np.uint32))
    P.set_distances(seeds, X, P.VarianceWeights())
    assert seen[-1][0] == "blissgpu_set_distance" and seen[-1][1] == 2
    assert np.array_equal(seen[-1][2].view(np.uint32), M.view(np.uint32))
    real(seeds[:1], X, P.VarianceWeights(few_seeds="euclidean"))
    assert seen[-1][0] == "blissgpu_closest_to_songs" and seen[-1][1] == 0 and seen[-1][2] is None
    monkeypatch.undo()
    monkeypatch.setattr(P, "closest_to_songs_order", fake_order)
    paths = [songs[i].path for i in (3, 10, 17)]
    out = bliss.library.playlist_from_custom(db, paths, P.VarianceWeights(), P.closest_to_songs, deduplicate=False)
    assert [s.path for s in out[:3]] == paths and len(out) == len(songs)
    assert isinstance(seen[-1][1], P.VarianceWeights) and np.array_equal(seen[-1][0], seeds)


def _ffi_of(bliss):
    from bliss_rs_amd import _ffi

    return _ffi


class _FakeLib:
    """stands in for the shared library: records (entry point, metric code, the M it was given) and reports success"""

    def __init__(self, seen):
        self._seen = seen

    def __getattr__(self, name):
        def call(*a):
            # (seeds, n_seeds, cand, n, d, metric, M, ...): the same leading arguments for both entry points
            d, metric, mp = int(a[4]), int(a[5]), a[6]
            M = None if mp is None else np.ctypeslib.as_array(C.cast(mp, C.POINTER(C.c_float)), (d, d)).copy()
            self._seen.append((name, metric, M))
            return 0

        return call
