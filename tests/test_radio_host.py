"""Device-free tests of the radio playlists (blissgpu_radio / blissgpu_radio_device): the C ABI surface (header,
.so, _ffi.SIGNATURES and the Rust declarations held to one another), the kernels' names in the profile table, the argument
checks that happen before the device is touched, rule_labels, and the host logic of playlist.radio_playlist /
library.radio_playlists with the device call replaced by a numpy brute force."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
OK, INVALID = 0, 2
CHAIN, NEAREST = 0, 1
NONE = 0xFFFFFFFF
NAMES = ("blissgpu_radio", "blissgpu_radio_device")


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


# ---- the surface ----
def test_radio_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "rust", "gpu.rs")).read())
    lib = C.CDLL(bliss.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, flat), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name

    def types(name):
        return [re.sub(r"\s*\b\w+$", "", " ".join(a.split())).replace(" *", "*")
                for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, flat).group(1).split(",")]

    def rust_types(name):
        args = re.search(r"pub fn %s\s*\(([^)]*)\)\s*->\s*c_int" % name, rust).group(1)
        return [" ".join(a.split(":", 1)[1].split()) for a in args.split(",")]

    to_rust = {"const float*": "*const f32", "float*": "*mut f32", "const uint32_t*": "*const u32", "uint32_t*": "*mut u32",
               "uint64_t": "u64", "uint32_t": "u32", "int": "c_int", "blissgpu_ctx*": "*mut blissgpu_ctx"}
    to_ffi = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int}
    # (from, n_radios, cand, n, d, metric, M, labels, from_labels, n_rules, window, limit, skip, k, mode, idx, dist)
    want = ["const float*", "uint64_t", "const float*", "uint64_t", "uint32_t", "int", "const float*", "const uint32_t*",
            "const uint32_t*", "uint32_t", "const uint32_t*", "const uint32_t*", "const uint32_t*", "uint32_t", "int", "uint32_t*",
            "float*"]
    for name, w in (("blissgpu_radio", want), ("blissgpu_radio_device", ["blissgpu_ctx*"] + want)):
        assert types(name) == w, name
        assert rust_types(name) == [to_rust[t] for t in w], name
        assert _ffi.SIGNATURES[name] == (C.c_int, [to_ffi.get(t, _vp) for t in w]), name
    # the three defines: header, _ffi and the Rust constants
    for name, value, rust_type in (("RADIO_MAX_RULES", 4, "u32"), ("RADIO_CHAIN", 0, "c_int"), ("RADIO_NEAREST", 1, "c_int")):
        assert re.search(r"#define\s+BLISSGPU_%s\s+%du?\b" % (name, value), header), name
        assert getattr(_ffi, name) == value, name
        assert re.search(r"pub const BLISSGPU_%s: %s = %d;" % (name, rust_type, value), rust), name
    for name in ("Rule", "rule_labels", "radio_order", "radio_playlist"):
        assert hasattr(bliss.playlist, name), name
    assert hasattr(bliss.library, "radio_playlists") and hasattr(bliss.Context, "radio")


def test_radio_kernels_are_in_the_profile_table(bliss):
    from bliss_rs_amd import _ffi

    L = _ffi.lib()
    names = [L.blissgpu_profile_kernel_name(k).decode() for k in range(L.blissgpu_profile_kernel_count())]
    assert len(set(names)) == len(names) and "" not in names
    src = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "kernels_radio.hip")).read()
    for name in ("radio_ban_kernel", "radio_step_kernel"):
        assert names.count(name) == 1, name
        assert re.search(r"\bvoid\s+%s\s*\(" % name, src), name
        assert names.index(name) < len(names) - 2
    assert names[-2:] == ["group_forest_scan_kernel", "journey_step_kernel"]  # (older ids keep their places)
    mk = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "Makefile")).read()
    line = [l for l in mk.splitlines() if "EXTRA := $(NOCONTRACT)" in l]
    assert len(line) == 1 and "kernels_radio.o" in line[0]  # compiled -ffp-contract=off
    assert "kernels_radio.o" in [l for l in mk.splitlines() if l.startswith("OBJS")][0]


# ---- the argument checks: before the device is touched ----
def _p(a):
    return None if a is None else a.ctypes.data


def _call(G=4, n=6, d=23, metric=0, M=None, n_rules=2, window=(3, 5), limit=(1, 2), k=3, mode=CHAIN, skip=None, null=(), device=False):
    from bliss_rs_amd import _ffi

    dd, R = min(max(d, 1), 64), max(n_rules, 1)
    a = {"from": np.zeros((max(G, 1) if G < 1024 else 1, dd), np.float32), "cand": np.zeros((max(min(n, 8), 1), dd), np.float32),
         "labels": np.zeros((R, max(min(n, 8), 1)), np.uint32), "from_labels": np.zeros((max(G, 1) if G < 1024 else 1, R), np.uint32),
         "window": np.asarray(list(window) + [1] * R, np.uint32)[:R], "limit": np.asarray(list(limit) + [1] * R, np.uint32)[:R],
         "idx": np.zeros((max(G, 1) if G < 1024 else 1, 1024), np.uint32), "dist": np.zeros((max(G, 1) if G < 1024 else 1, 1024), np.float32)}
    g = lambda name: None if name in null else _p(a[name])  # noqa: E731
    args = (g("from"), G, g("cand"), n, d, metric, _p(M), g("labels"), g("from_labels"), n_rules, g("window"), g("limit"), _p(skip), k,
            mode, g("idx"), g("dist"))
    L = _ffi.lib()
    rc = L.blissgpu_radio_device(None, *args) if device else L.blissgpu_radio(*args)
    return rc, L.blissgpu_last_error(), a


def test_radio_arguments_are_checked_before_the_device(bliss):
    for device in (False, True):
        bad = [(dict(limit=(1, 0)), b"limit must be"), (dict(limit=(0, 1)), b"limit must be"),
               (dict(n_rules=5, window=(1,) * 5, limit=(1,) * 5), b"n_rules"),
               (dict(null=("labels",)), b"labels is NULL"), (dict(null=("window",)), b"window is NULL"),
               (dict(null=("limit",)), b"limit is NULL"),
               (dict(k=0), b"k must be"), (dict(k=1025), b"k must be"), (dict(d=65), b"d must be"), (dict(d=0), b"d must be"),
               (dict(mode=2), b"unknown mode"), (dict(mode=-1), b"unknown mode"),
               (dict(metric=3), b"unknown metric"), (dict(metric=-1), b"unknown metric"), (dict(metric=2), b"mahalanobis needs M"),
               (dict(n=0xFFFFFFFF), b"n must be"), (dict(G=1 << 31), b"n_radios must be"),
               (dict(null=("from",)), b"from is NULL"), (dict(null=("cand",)), b"cand is NULL"), (dict(null=("idx",)), b"idx is NULL")]
        for kw, text in bad:
            rc, err, _ = _call(device=device, **kw)
            assert rc == INVALID and text in err, (device, kw, err)
    # a skip entry that is no candidate and not 0xFFFFFFFF (host form: the device form cannot read it without the device)
    skip = np.full((4, 2), NONE, np.uint32)
    skip[2, 1] = 6
    rc, err, _ = _call(skip=skip)
    assert rc == INVALID and b"skip entries" in err
    # the device form with valid arguments then looks at its (NULL) context
    rc, err, _ = _call(device=True)
    assert rc == INVALID and b"ctx is NULL" in err
    # no rule: labels, window and limit may be NULL
    rc, err, _ = _call(n_rules=0, null=("labels", "from_labels", "window", "limit"), device=True)
    assert rc == INVALID and b"ctx is NULL" in err
    # nothing to do: OK without a device
    assert _call(G=0, null=("from", "idx", "dist"))[0] == OK
    assert _call(G=0, n=0, null=("from", "cand", "idx", "dist", "labels"), n_rules=0)[0] == OK
    rc, _, a = _call(n=0, null=("cand",))
    assert rc == OK and (a["idx"].reshape(-1)[:12] == NONE).all() and np.isinf(a["dist"].reshape(-1)[:12]).all()  # [4][3] of padding
    assert (a["idx"].reshape(-1)[12:] == 0).all()
    assert _call(n=0, null=("cand", "dist"))[0] == OK


# ---- rule_labels and Rule ----
def _songs(bliss, X, artist, album, album_artist=None, genre=None):
    V2 = bliss.FeaturesVersion.Version2
    n = X.shape[0]
    return [bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist=artist[i], album=album[i],
                       album_artist=None if album_artist is None else album_artist[i], genre=None if genre is None else genre[i],
                       duration=1.0, analysis=bliss.Analysis(X[i], V2), features_version=V2) for i in range(n)]


def test_rule_labels(bliss):
    P = bliss.playlist
    X = np.zeros((6, 23), np.float32)
    songs = _songs(bliss, X, artist=["a", "b", None, "a", "b", "c"], album=["Greatest Hits", "Greatest Hits", "x", "Greatest Hits", None, "x"],
                   album_artist=[None, None, "va", "a", None, "va"], genre=["rock", None, "rock", "pop", "pop", None])
    rules = [P.Rule("artist", 5), P.Rule("album", 20), P.Rule("album_artist"), P.Rule("genre", None, 3),
             P.Rule(lambda s: None if s.title == "t5" else int(s.title[1:]) % 2, 2)]
    lab = P.rule_labels(songs, rules)
    assert lab.dtype == np.uint32 and lab.shape == (5, 6)
    assert lab[0].tolist() == [0, 1, NONE, 0, 1, 2]
    # "Greatest Hits" by a and by b are two albums; an album artist takes the artist's place; no album, no label
    assert lab[1].tolist() == [0, 1, 2, 0, NONE, 2]
    assert lab[2].tolist() == [NONE, NONE, 0, 1, NONE, 0]
    assert lab[3].tolist() == [0, NONE, 0, 1, 1, NONE]
    assert lab[4].tolist() == [0, 1, 0, 1, 0, NONE]  # a callable; its None is no label
    assert P.rule_labels(songs, []).shape == (0, 6) and P.rule_labels([], rules).shape == (5, 0)
    assert P.NO_LABEL == NONE
    # wrappers holding a Song (AsRef<Song>)
    class Wrapped:
        def __init__(self, s):
            self.bliss_song = s
    assert np.array_equal(P.rule_labels([Wrapped(s) for s in songs], rules[:4]), lab[:4])
    # window None is the whole list: k + 1
    assert P._rule_arrays(rules[:4], 30) == ([5, 20, 31, 31], [1, 1, 1, 3])
    for bad in (dict(by="composer"), dict(by="artist", window=-1), dict(by="artist", limit=0)):
        with pytest.raises(ValueError):
            P.Rule(**bad)
    with pytest.raises(ValueError):
        P._rule_arrays([P.Rule("artist")] * 5, 3)
    assert [(r.by, r.window, r.limit) for r in P.DEFAULT_RADIO_RULES] == [("artist", 5, 1), ("album", 20, 1)]


def test_radio_order_checks_before_the_library(bliss, monkeypatch):
    from bliss_rs_amd import _ffi

    def boom():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_ffi, "lib", boom)
    P = bliss.playlist
    X = np.zeros((5, 23), np.float32)
    lab = np.zeros((1, 5), np.int64)
    bad = [dict(k=0), dict(k=1025), dict(mode="walk"), dict(metric="manhattan"), dict(metric="mahalanobis"), dict(limits=[0]),
           dict(windows=[-1]), dict(windows=[1, 2]), dict(labels=np.zeros((1, 4), np.int64)), dict(labels=np.full((1, 5), -2)),
           dict(from_labels=np.zeros((3, 1), np.int64)), dict(skip=[[0, 5], [0, -1]]), dict(skip=[[0, -1]]),
           dict(windows=[1] * 5, limits=[1] * 5, labels=np.zeros((5, 5), np.int64))]
    for kw in bad:
        a = dict(from_rows=X[:2], candidates=X, k=3, labels=lab, windows=[2], limits=[1])
        a.update(kw)
        with pytest.raises(ValueError):
            P.radio_order(**a)
    for builder, text in ((P.ForestOptions(8, 4, 3, 0), "forest"), (P.VarianceWeights(), "variance-based weights")):
        for call in (lambda b: P.radio_order(X[:2], X, 3, lab, [2], [1], metric=b), lambda b: P.radio_playlist(None, [], 3, metric_builder=b),
                     lambda b: bliss.library.radio_playlists("none.db", 3, metric_builder=b)):
            with pytest.raises((TypeError, ValueError)) as e:
                call(builder)
            assert text.lower() in str(e.value).lower()


# ---- the song-level helpers, with the device call replaced by a numpy brute force ----
def _brute_force(record):
    def radio_order(from_rows, candidates, k, labels, windows, limits, from_labels=None, mode="chain", metric="euclidean", m=None,
                    skip=None):
        A, X = np.asarray(from_rows, np.float32), np.asarray(candidates, np.float32)
        labels = np.asarray(labels, np.int64).reshape(len(windows), X.shape[0])
        record.append(dict(A=A.copy(), X=X.copy(), k=k, labels=labels.copy(), windows=list(windows), limits=list(limits),
                           from_labels=None if from_labels is None else np.asarray(from_labels, np.int64).copy(), mode=mode,
                           metric=metric, skip=None if skip is None else np.asarray(skip).copy(), shared=from_rows is candidates))
        G, n = A.shape[0], X.shape[0]
        euclid = lambda a: np.sqrt(((a - X) ** 2).sum(axis=1, dtype=np.float32))  # noqa: E731
        idx, dist = np.full((G, k), -1, np.int64), np.full((G, k), np.inf, np.float32)
        for g in range(G):
            free = np.ones(n, bool)
            if skip is not None:
                sk = np.asarray(skip)[g]
                free[sk[sk >= 0]] = False
            hist = [[NONE if from_labels is None else int(from_labels[g][r])] for r in range(len(windows))]
            q = A[g]
            for t in range(k):
                ok = free.copy()
                for r, (w, lim) in enumerate(zip(windows, limits)):
                    if w >= 1:
                        H = np.asarray([hist[r][p + 1] for p in range(max(t - w, -1), t)], np.int64)
                        ok &= ~((labels[r] != NONE) & ((H[:, None] == labels[r][None, :]).sum(axis=0) >= lim))
                if not ok.any():
                    break
                row = euclid(q)
                j = int(np.argmin(np.where(ok, row, np.inf)))
                idx[g, t], dist[g, t] = j, row[j]
                free[j] = False
                for r in range(len(windows)):
                    hist[r].append(int(labels[r][j]))
                if mode == "chain":
                    q = X[j]
        return idx, dist

    return radio_order


def _library(bliss, tmp_path, n=60):
    rng = np.random.default_rng(5)
    artist = np.arange(n) % 8
    centre = rng.standard_normal((8, 23))
    X = (centre[artist] + 0.1 * rng.standard_normal((n, 23))).astype(np.float32)
    songs = _songs(bliss, X, artist=[None if i % 13 == 0 else f"artist{a}" for i, a in enumerate(artist)],
                   album=[f"album{i % 3}" for i in range(n)])
    db = str(tmp_path / "bliss.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs)
    return db, songs, X


def test_radio_helpers(bliss, tmp_path, monkeypatch):
    db, songs, X = _library(bliss, tmp_path)
    n, k = len(songs), 8
    record = []
    brute = _brute_force(record)
    P = bliss.playlist
    monkeypatch.setattr(P, "radio_order", brute)
    table = bliss.library.radio_playlists(db, k)
    assert len(record) == 1  # one call for the whole library
    r = record[0]
    labels = P.rule_labels(songs, P.DEFAULT_RADIO_RULES).astype(np.int64)
    assert np.array_equal(r["A"], X) and np.array_equal(r["X"], X) and r["shared"] and r["k"] == k and r["mode"] == "chain"
    assert r["windows"] == [5, 20] and r["limits"] == [1, 1] and np.array_equal(r["labels"], labels)
    assert np.array_equal(r["skip"], np.stack([np.arange(n), np.full(n, -1)], axis=1))  # every song skips its own row
    assert np.array_equal(r["from_labels"], labels.T)  # ... and carries its own labels
    assert list(table) == [s.path for s in songs]
    unruled = brute(X, X, k, labels[:0], [], [], None, skip=r["skip"])[0]
    differ = 0
    for g, s in enumerate(songs):
        line = [s] + table[s.path]
        assert s.path not in [t.path for t in table[s.path]] and len(table[s.path]) == k
        artists = [t.artist for t in line]
        assert all(a is None or a not in artists[max(0, i - 5):i] for i, a in enumerate(artists))  # no artist twice within 5 tracks
        differ += [t.path for t in table[s.path]] != [songs[j].path for j in unruled[g]]
    assert differ > n // 2  # a song's nearest neighbours are its own artist: the rules change the radios
    # some songs only, in the order given; other rules, the other mode
    some = [songs[9].path, songs[2].path]
    rules = (P.Rule("artist", None, 2), P.Rule(lambda s: s.album, 3))
    table = bliss.library.radio_playlists(db, k, rules, song_paths=some, mode="nearest")
    r = record[-1]
    assert list(table) == some and r["skip"].tolist() == [[9, -1], [2, -1]] and r["mode"] == "nearest" and not r["shared"]
    assert r["windows"] == [k + 1, 3] and r["limits"] == [2, 1] and np.array_equal(r["A"], X[[9, 2]])
    assert np.array_equal(r["from_labels"], P.rule_labels(songs, rules).astype(np.int64)[:, [9, 2]].T)
    for p in some:
        line = [songs[int(p[-8:-5])]] + table[p]
        counts = {}
        for t in line:
            counts[t.artist] = counts.get(t.artist, 0) + 1
        assert all(c <= 2 for a, c in counts.items() if a is not None)
    assert bliss.library.radio_playlists(db, k, song_paths=[]) == {}
    with pytest.raises(bliss.ProviderError):
        bliss.library.radio_playlists(db, k, song_paths=[songs[1].path, "/music/none.flac"])
    with pytest.raises(ValueError):
        bliss.library.radio_playlists(db, k, mode="walk")
    # the song form: the start need not be a candidate; when it is, it is skipped; either way it is labelled
    record.clear()
    pool = songs[:30]
    one = P.radio_playlist(songs[45], pool, k)
    r = record[0]
    assert np.array_equal(r["A"], X[[45]]) and r["skip"].tolist() == [[-1, -1]] and r["windows"] == [5, 20]
    assert songs[45].artist not in [t.artist for t in one[:4]] and len(one) == k
    lab = P.rule_labels(pool + [songs[45]], P.DEFAULT_RADIO_RULES).astype(np.int64)
    assert np.array_equal(r["labels"], lab[:, :-1]) and np.array_equal(r["from_labels"], lab[:, -1:].T)
    one = P.radio_playlist(songs[4], pool, k)
    assert record[1]["skip"].tolist() == [[4, -1]] and songs[4] not in one
    assert P.radio_playlist(songs[4], [], k) == []
    # a radio that runs dry: one song per artist in the whole list: seven other artists and the three songs without one
    dry = P.radio_playlist(songs[1], pool, 20, (P.Rule("artist"),))
    assert 0 < len(dry) < 20 and record[-1]["windows"] == [21]
