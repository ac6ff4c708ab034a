"""Device-free tests of the album playlists (blissgpu_album_knn / blissgpu_album_knn_device, playlist.nearest_albums,
playlist.closest_albums_to_groups, library.album_playlists): the C ABI surface, the argument checks that happen before the
device is touched, what the Python layer refuses before the library is reached, and the grouping logic of
library.album_playlists -- one call with the expected arrays, and, with the two device calls replaced by the same host
arithmetic (sequential f32 means, the oracle's distances), the same playlists as library.album_playlist_from."""
import ctypes as C
import os
import re

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


def test_album_knn_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    lib = C.CDLL(bliss.LIB_PATH)
    for name in ("blissgpu_album_knn", "blissgpu_album_knn_device"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name
    assert "src/playlist.rs:424-485" in header and "src/library.rs:850-893" in header
    u64, u32 = C.c_uint64, C.c_uint32
    # (seeds, group_offsets, n_groups, cand, n, d, album_of, n_albums, skip, k, idx, dist, group_means, centroids)
    host = [_vp, _vp, u64, _vp, u64, u32, _vp, u64, _vp, u32, _vp, _vp, _vp, _vp]
    assert _ffi.SIGNATURES["blissgpu_album_knn"] == (C.c_int, host)
    assert _ffi.SIGNATURES["blissgpu_album_knn_device"] == (C.c_int, [_vp] + host)
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    types = lambda name: [re.sub(r"\s*\w+$", "", re.sub(r"\s+", " ", a.strip())).replace(" *", "*")  # noqa: E731
                          for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, flat).group(1).split(",")]
    want = ["const float*", "const uint64_t*", "uint64_t", "const float*", "uint64_t", "uint32_t", "const uint32_t*", "uint64_t",
            "const uint32_t*", "uint32_t", "uint32_t*", "float*", "float*", "float*"]
    assert types("blissgpu_album_knn") == want
    assert types("blissgpu_album_knn_device") == ["blissgpu_ctx*"] + want
    # the existing declaration did not move
    assert types("blissgpu_group_knn") == ["const float*", "const uint64_t*", "uint64_t", "const float*", "uint64_t", "uint32_t",
                                           "int", "const float*", "const uint32_t*", "uint32_t", "uint32_t*", "float*"]
    # the new kernels appear in the profiling table, once each, and no older name moved or repeats
    L = _ffi.lib()
    table = [L.blissgpu_profile_kernel_name(i).decode() for i in range(L.blissgpu_profile_kernel_count())]
    assert table.count("segment_mean_kernel") == 1 and table.count("album_knn_scan_kernel") == 1
    assert len(set(table)) == len(table)
    assert table.index("chain_walk_kernel") < table.index("segment_mean_kernel")
    assert table[:3] == ["fft512_kernel", "onset_kernel", "beat_kernel"] and table.count("knn_merge_kernel") == 1


def _p(a):
    return None if a is None else a.ctypes.data


def _call(S, off, X, album_of, A, k, d=None, skip=None, idx=True, device_form=False):
    from bliss_rs_amd import _ffi

    off = np.asarray(off, np.uint64)
    G, n = off.shape[0] - 1, X.shape[0]
    d = X.shape[1] if d is None else d
    out_i, out_d = np.zeros((max(G, 1), max(k, 1)), np.uint32), np.zeros((max(G, 1), max(k, 1)), np.float32)
    gm, cent = np.zeros((max(G, 1), max(d, 1)), np.float32), np.zeros((max(A, 1), max(d, 1)), np.float32)
    args = (_p(S), _p(off), G, _p(X), n, d, _p(album_of), A, _p(skip), k, _p(out_i) if idx else None, _p(out_d), _p(gm), _p(cent))
    if device_form:  # a NULL context: everything about the arguments is said before the context is looked at
        return _ffi.lib().blissgpu_album_knn_device(None, *args)
    return _ffi.lib().blissgpu_album_knn(*args)


def test_arguments_are_checked_before_the_device(bliss):
    import torch

    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    max_k = int(re.search(r"#define\s+BLISSGPU_KNN_MAX_K\s+(\d+)", header).group(1))
    rng = np.random.default_rng(0)
    X = rng.standard_normal((50, 23)).astype(np.float32)
    S = X[:6].copy()
    off = [0, 1, 4, 6]
    A = 9
    album_of = (np.arange(50) % A).astype(np.uint32)
    album_of[7] = NONE
    err = lambda: _ffi.lib().blissgpu_last_error()  # noqa: E731
    for dev in (False, True):
        assert _call(S, off, X, album_of, A, 0, device_form=dev) == INVALID and b"ctx" not in err() and b"k must" in err()
        assert _call(S, off, X, album_of, A, max_k + 1, device_form=dev) == INVALID and b"ctx" not in err() and b"k must" in err()
        assert _call(S, off, X, album_of, A, 3, d=0, device_form=dev) == INVALID and b"ctx" not in err() and b"d must" in err()
        assert _call(np.zeros((6, 65), np.float32), off, np.zeros((50, 65), np.float32), album_of, A, 3, d=65,
                     device_form=dev) == INVALID and b"ctx" not in err() and b"d must" in err()
        assert _call(S, [1, 1, 4, 6], X, album_of, A, 3, device_form=dev) == INVALID and b"ctx" not in err() and b"group_offsets" in err()
        assert _call(S, [0, 4, 1, 6], X, album_of, A, 3, device_form=dev) == INVALID and b"ctx" not in err() and b"group_offsets" in err()
        assert _call(S, [0, 1, 1, 6], X, album_of, A, 3, device_form=dev) == INVALID and b"ctx" not in err() and b"empty group" in err()
        assert _call(S, off, X, album_of, A, 3, idx=False, device_form=dev) == INVALID and b"ctx" not in err() and b"idx" in err()
        assert _call(S, off, X, album_of, 51, 3, device_form=dev) == INVALID and b"ctx" not in err() and b"n_albums" in err()
        assert _call(S, off, X, None, A, 3, device_form=dev) == INVALID and b"ctx" not in err() and b"album_of" in err()
    # an album index that is no album, a skip entry that is no candidate: the host form checks them on the host
    bad = album_of.copy()
    bad[3] = A
    assert _call(S, off, X, bad, A, 3) == INVALID and b"album_of" in err() and b"ctx" not in err()
    skip = np.full(6, NONE, np.uint32)
    skip[3] = X.shape[0]
    assert _call(S, off, X, album_of, A, 3, skip=skip) == INVALID and b"skip" in err() and b"ctx" not in err()
    # the device form with good arguments gets as far as its (NULL) context
    assert _call(S, off, X, album_of, A, 3, device_form=True) == INVALID and b"ctx" in err()
    # nothing to do
    assert _call(S[:0], [0], X, album_of, A, 3) == 0
    # a valid call: BLISSGPU_ERR_NO_DEVICE without a GPU, BLISSGPU_OK with one
    ok = 0 if torch.cuda.is_available() else NO_DEVICE
    skip[3] = 0
    assert _call(S, off, X, album_of, A, 3, skip=skip) == ok


def _boom():
    raise AssertionError("the library must not be reached")


def _library(bliss, tmp_path, n=40, n_albums=7):
    """n songs; song 0 is an album of its own, song 5 has no album, the rest share n_albums albums; disc and track numbers
    repeat and some are None, so the (disc, track) order is neither the id order nor free of ties"""
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, 23)).astype(np.float32)
    V2 = bliss.FeaturesVersion.Version2
    songs = []
    for i in range(n):
        album = "alone" if i == 0 else None if i == 5 else f"album{i % n_albums}"
        songs.append(bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist=f"artist{i % 3}", album=album,
                                genre=None if i % 4 == 0 else f"genre{i % 2}", track_number=None if i % 6 == 1 else (n - i) % 4,
                                disc_number=None if i % 5 == 2 else (i // 7) % 2, duration=1.0, analysis=bliss.Analysis(X[i], V2),
                                features_version=V2))
    db = str(tmp_path / "bliss.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs)
    return db, songs, X


def test_python_paths_that_do_not_reach_the_library(bliss, tmp_path, monkeypatch):
    from bliss_rs_amd import _ffi

    P = bliss.playlist
    db, songs, X = _library(bliss, tmp_path)
    monkeypatch.setattr(_ffi, "lib", _boom)
    album_of = np.arange(40) % 7
    groups = [X[:2], X[2:5]]
    for empty in ([X[:2], X[:0]], (X[:4], [0, 2, 2, 4])):
        with pytest.raises(bliss.ProviderError) as e:
            P.nearest_albums(empty, X, album_of, 3)
        assert "Mean of empty slice" in str(e.value)
    with pytest.raises(ValueError):
        P.nearest_albums([np.zeros((2, 20), np.float32)], X, album_of, 3)  # another d
    with pytest.raises(ValueError):
        P.nearest_albums(groups, X, album_of[:39], 3)  # one album index per candidate
    with pytest.raises(ValueError):
        P.nearest_albums(groups, X, album_of.astype(np.float32), 3)
    with pytest.raises(ValueError):
        P.nearest_albums(groups, X, np.where(album_of == 3, -2, album_of), 3)
    with pytest.raises(ValueError):
        P.nearest_albums(groups, X, np.where(album_of == 3, 40, album_of), 3)  # more albums than candidates
    for k in (0, -1, 1025):
        with pytest.raises(ValueError):
            P.nearest_albums(groups, X, album_of, k)
    with pytest.raises(ValueError):
        P.nearest_albums(groups, np.zeros((40, 65), np.float32)[:, :65], album_of, 3)
    with pytest.raises(ValueError):
        P.nearest_albums(groups, X, album_of, 3, skip=np.array([0, 1, 2]))  # flat: one entry per seed row (5)
    with pytest.raises(ValueError):
        P.nearest_albums(groups, X, album_of, 3, skip=np.array([0, 1, 2, 3, 40]))
    with pytest.raises(bliss.ProviderError):
        P.closest_albums_to_groups([songs[:2], []], songs, 3)
    assert P.closest_albums_to_groups([], songs, 3) == []
    assert P.closest_albums_to_groups([songs[:2]], songs, 0) == [songs[:2]]
    # no album to append: the albums alone, each in songs_from_album's order
    table = bliss.library.album_playlists(db, 0)
    assert list(table) == ["alone"] + [f"album{a}" for a in (1, 2, 3, 4, 6, 0, 5)]
    for title, pl in table.items():
        assert [s.path for s in pl] == [s.path for s in bliss.library.songs_from_album(db, title)]
    with pytest.raises(ValueError):
        bliss.library.album_playlists(db, 3, by="year")
    with pytest.raises(ValueError):
        bliss.library.album_playlists(db, -1)
    with pytest.raises(bliss.ProviderError):
        bliss.library.album_playlists(db, 3, groups={"x": [songs[1].path, "/music/none.flac"]})
    with pytest.raises(bliss.ProviderError):
        bliss.library.album_playlists(db, 3, groups={"x": []})


def _disc_track(s):
    return ((0, 0) if s.disc_number is None else (1, s.disc_number), (0, 0) if s.track_number is None else (1, s.track_number))


def test_library_album_playlists_is_one_call(bliss, tmp_path, monkeypatch):
    db, songs, X = _library(bliss, tmp_path)
    P = bliss.playlist
    record = []

    def fake(seed_groups, candidates, album_of, k, skip=None, return_means=False):
        S, off = seed_groups
        record.append((np.asarray(S).copy(), np.asarray(off).copy(), np.asarray(candidates).copy(), np.asarray(album_of).copy(), k,
                       np.asarray(skip).copy()))
        G = len(off) - 1
        return np.tile(np.arange(k), (G, 1)), np.zeros((G, k), np.float32)

    monkeypatch.setattr(P, "nearest_albums", fake)
    table = bliss.library.album_playlists(db, 3)
    assert len(record) == 1  # ONE call for the eight albums
    S, off, cand, album_of, k, skip = record[0]
    titles = ["alone"] + [f"album{a}" for a in (1, 2, 3, 4, 6, 0, 5)]  # in order of first appearance by id
    assert list(table) == titles and k == 3
    # every album's seeds are its songs in (disc, track) order, None first; each seed row skips its own library row
    rows = [i for t in titles for i in sorted((i for i, s in enumerate(songs) if s.album == t), key=lambda i: _disc_track(songs[i]))]
    assert np.array_equal(skip, rows) and sorted(rows) == [i for i in range(40) if i != 5]
    assert rows != sorted(rows)
    sizes = [sum(s.album == t for s in songs) for t in titles]
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(sizes)]))
    assert np.array_equal(S.view(np.uint32), X[rows].view(np.uint32)) and np.array_equal(cand.view(np.uint32), X.view(np.uint32))
    want_album = np.array([-1 if s.album is None else titles.index(s.album) for s in songs])
    assert want_album[5] == -1 and np.array_equal(album_of, want_album)
    # the fake ranked albums 0, 1, 2 for everyone: the seeds, then those albums without the seeds, each in (disc, track) order
    for t in titles:
        own = [songs[i] for i in rows if songs[i].album == t]
        rest = [s for a in titles[:3] for s in sorted((s for s in songs if s.album == a and s.album != t), key=_disc_track)]
        assert [s.path for s in table[t]] == [s.path for s in own + rest], t
    # seed sets by another column, and saved playlists: the ranked things are still albums
    record.clear()
    table = bliss.library.album_playlists(db, 2, by="artist")
    assert len(record) == 1 and list(table) == ["artist0", "artist1", "artist2"]
    assert np.array_equal(record[0][5], [i for a in range(3) for i in range(40) if i % 3 == a])  # members in id order
    assert np.array_equal(record[0][3], want_album)
    record.clear()
    saved = {"mix": [songs[9].path, songs[2].path, songs[9].path], "one": [songs[5].path]}
    table = bliss.library.album_playlists(db, 2, groups=saved)
    assert len(record) == 1 and np.array_equal(record[0][5], [9, 2, 9, 5]) and np.array_equal(record[0][1], [0, 3, 4])
    assert [s.path for s in table["mix"][:3]] == saved["mix"] and table["one"][0].path == songs[5].path
    assert all(s.path not in saved["mix"] for s in table["mix"][3:])
    with pytest.raises(bliss.ProviderError):
        bliss.library.album_playlists(db, 2, groups={"x": [songs[1].path, "/music/none.flac"]})
    assert len(record) == 1


def _seq_mean(rows):
    acc = np.zeros(rows.shape[1], np.float32)
    for r in rows:
        acc = acc + r
    return acc / np.float32(rows.shape[0])


def _host_nearest_albums(oracle):
    """playlist.nearest_albums in host arithmetic: sequential f32 means, the oracle's distances, stable (dist, album) order"""
    def nearest(seed_groups, candidates, album_of, k, skip=None, return_means=False):
        S, off = seed_groups
        X, album_of = np.asarray(candidates, np.float32), np.asarray(album_of)
        A = int(album_of.max()) + 1
        idx, dist = np.full((len(off) - 1, k), -1, np.int64), np.full((len(off) - 1, k), np.inf, np.float32)
        for g in range(len(off) - 1):
            gone = set(int(j) for j in skip[off[g]:off[g + 1]] if j >= 0)
            mean = _seq_mean(np.asarray(S[off[g]:off[g + 1]], np.float32))
            albums = [(a, [i for i in np.flatnonzero(album_of == a) if i not in gone]) for a in range(A)]
            albums = [(a, r) for a, r in albums if r]
            dm = oracle.pairwise(mean[None], np.stack([_seq_mean(X[r]) for _, r in albums]), "euclidean")[0]
            order = np.argsort(dm, kind="stable")[:k]
            idx[g, :order.size] = [albums[o][0] for o in order]
            dist[g, :order.size] = dm[order]
        return idx, dist
    return nearest


def test_album_playlists_group_like_album_playlist_from(bliss, oracle, tmp_path, monkeypatch):
    """The grouping, the seed order and the cut of library.album_playlists / playlist.closest_albums_to_groups against today's
    per-album code, both fed by the same host arithmetic instead of the device."""
    db, songs, X = _library(bliss, tmp_path, n=60, n_albums=9)
    P = bliss.playlist

    def order(seeds, candidates, metric="euclidean", m=None):
        assert metric == "euclidean" and len(seeds) == 1
        dm = oracle.pairwise(np.asarray(seeds, np.float32), np.asarray(candidates, np.float32), "euclidean")[0]
        o = np.argsort(dm, kind="stable")
        return o.astype(np.uint32), dm[o]

    monkeypatch.setattr(P, "closest_to_songs_order", order)
    monkeypatch.setattr(P, "nearest_albums", _host_nearest_albums(oracle))
    library = bliss.library.songs_from_library(db)
    titles = list(dict.fromkeys(s.album for s in library if s.album is not None))
    assert len(titles) == 10
    for n_albums in (1, 3, 40):
        table = bliss.library.album_playlists(db, n_albums)
        assert list(table) == titles
        groups = [bliss.library.songs_from_album(db, t) for t in titles]
        objects = P.closest_albums_to_groups(groups, library, n_albums)
        for t, got in zip(titles, objects):
            want = [s.path for s in bliss.library.album_playlist_from(db, t, n_albums)]
            assert [s.path for s in table[t]] == want, (t, n_albums)
            assert [s.path for s in got] == want, (t, n_albums)
            assert len(want) > len(bliss.library.songs_from_album(db, t))
    # closest_album_to_group itself, uncut, for by-album groups
    for t, got in zip(titles, P.closest_albums_to_groups(groups, library, len(titles))):
        want = P.closest_album_to_group(bliss.library.songs_from_album(db, t), library)
        assert [s.path for s in got] == [s.path for s in want], t
