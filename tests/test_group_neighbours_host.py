"""Device-free tests of the group neighbours (blissgpu_group_neighbours / blissgpu_group_neighbours_device): the C ABI surface, the
kernels' names in the profile table, the argument checks that happen before the device is touched, and the host-side parts of the
Python layer with playlist.group_neighbours replaced by the contract of include/blissgpu.h written out in numpy (`contract`
below, which the GPU tests compare the device with)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
OK, NO_DEVICE, INVALID = 0, 1, 2
SYMMETRIC, DIRECTED = 0, 1
BLOCK = 256


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


# ---- the contract in numpy ----
def tree_sum(terms, order="tree"):
    """the contract's f64 sum of terms [m, ...] along axis 0: blocks of 256 padded with +0.0, eight halving levels inside a
    block, the block sums added sequentially from 0.0.  order "sequential" / "reversed" are what it is NOT"""
    terms = np.asarray(terms, np.float64)
    total = np.zeros(terms.shape[1:], np.float64)
    if order != "tree":
        for v in (terms if order == "sequential" else terms[::-1]):
            total = total + v
        return total
    for b0 in range(0, terms.shape[0], BLOCK):
        v = np.zeros((BLOCK,) + terms.shape[1:], np.float64)
        blk = terms[b0:b0 + BLOCK]
        v[:blk.shape[0]] = blk
        h = BLOCK // 2
        while h:
            v[:h] = v[:h] + v[h:2 * h]
            h //= 2
        total = total + v[0]
    return total


def directed(Dm, labels, k, order="tree"):
    """(D [k, k] f64 with NaN where D(a -> c) is not defined, sizes): Dm = the f32 all-pairs matrix"""
    labels = np.asarray(labels, np.int64)
    sizes = np.bincount(labels, minlength=k).astype(np.int64)
    n = Dm.shape[0]
    m = np.zeros((n, k), np.float32)
    for c in range(k):
        if sizes[c]:
            m[:, c] = Dm[:, labels == c].min(axis=1)  # (numpy's minimum keeps a NaN)
    D = np.full((k, k), np.nan, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(k):
            if sizes[a]:
                D[a] = tree_sum(m[labels == a].astype(np.float64), order) / np.float64(sizes[a])
    D[:, sizes == 0] = np.nan
    D[np.arange(k), np.arange(k)] = np.nan
    return D, sizes


def contract(Dm, labels, k, t, mode=SYMMETRIC, queries=None, order="tree"):
    """-> (idx int64 [q, t] with -1 as padding, dist f64 [q, t] with +inf, sizes int64 [k], matrix f64 [k, k])"""
    D, sizes = directed(Dm, labels, k, order)
    with np.errstate(invalid="ignore", over="ignore"):
        A = (D + D.T) * 0.5 if mode == SYMMETRIC else D
    live = (sizes[:, None] > 0) & (sizes[None, :] > 0) & ~np.eye(k, dtype=bool)
    matrix = np.where(live, A, np.inf)
    matrix[np.arange(k), np.arange(k)] = 0.0
    queries = np.arange(k) if queries is None else np.asarray(queries, np.int64)
    idx = np.full((len(queries), t), -1, np.int64)
    dist = np.full((len(queries), t), np.inf, np.float64)
    for g, a in enumerate(queries):
        cand = np.flatnonzero(live[a])
        cand = cand[np.argsort(A[a, cand], kind="stable")][:t]  # equal values keep the lower group first
        idx[g, :cand.size] = cand
        dist[g, :cand.size] = A[a, cand]
    return idx, dist, sizes, matrix


def test_tree_sum_is_the_written_order():
    rng = np.random.default_rng(1)
    v = (rng.random(600) * 10.0 ** rng.integers(-8, 8, 600))
    pad = np.concatenate([v, np.zeros(768 - 600)])
    want = 0.0
    for b in range(3):
        w = pad[256 * b:256 * b + 256].copy()
        for h in (128, 64, 32, 16, 8, 4, 2, 1):
            for u in range(h):
                w[u] = w[u] + w[u + h]
        want = want + w[0]
    assert tree_sum(v) == want
    assert tree_sum(v[:0]) == 0.0 and tree_sum(v[:1]) == v[0]


# ---- the surface ----
def test_group_neighbours_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    lib = C.CDLL(bliss.LIB_PATH)
    for name in ("blissgpu_group_neighbours", "blissgpu_group_neighbours_device"):
        assert re.search(r"\bint\s+%s\s*\(" % name, flat), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name

    def types(name):
        return [re.sub(r"\s*\b\w+$", "", " ".join(a.split())).replace(" *", "*")
                for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, flat).group(1).split(",")]

    # (x, n, d, labels, k, metric, M, queries, q, t, mode, slab_groups, idx, dist, sizes, matrix), the device form with the context
    want = ["const float*", "uint64_t", "uint32_t", "const uint32_t*", "uint32_t", "int", "const float*", "const uint32_t*", "uint64_t",
            "uint32_t", "int", "uint32_t", "uint32_t*", "double*", "uint32_t*", "double*"]
    assert types("blissgpu_group_neighbours") == want
    assert types("blissgpu_group_neighbours_device") == ["blissgpu_ctx*"] + want
    u64, u32 = C.c_uint64, C.c_uint32
    host = [_vp, u64, u32, _vp, u32, C.c_int, _vp, _vp, u64, u32, C.c_int, u32, _vp, _vp, _vp, _vp]
    assert _ffi.SIGNATURES["blissgpu_group_neighbours"] == (C.c_int, host)
    assert _ffi.SIGNATURES["blissgpu_group_neighbours_device"] == (C.c_int, [_vp] + host)
    for macro, value in (("BLISSGPU_GROUPS_SYMMETRIC", 0), ("BLISSGPU_GROUPS_DIRECTED", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), flat), macro
    assert (_ffi.GROUPS_SYMMETRIC, _ffi.GROUPS_DIRECTED) == (0, 1)
    assert "similar artists to the current one" in " ".join(header.split())  # the TODO.md line the feature answers


def test_group_neighbours_kernels_are_in_the_profile_table(bliss):
    from bliss_rs_amd import _ffi

    L = _ffi.lib()
    names = [L.blissgpu_profile_kernel_name(k).decode() for k in range(L.blissgpu_profile_kernel_count())]
    assert len(set(names)) == len(names) and "" not in names
    src = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "kernels_chamfer.hip")).read()
    mine = ("chamfer_scan_kernel", "chamfer_reduce_kernel", "chamfer_select_kernel")
    for name in mine:
        assert names.count(name) == 1, name
        assert re.search(r"\bvoid\s+%s\s*\(" % name, src), name
        assert names.index(name) < len(names) - 2
    assert sorted(n for n in names if n.startswith("chamfer_")) == sorted(mine)
    assert names[-2:] == ["group_forest_scan_kernel", "journey_step_kernel"]  # (older ids keep their places)


def _p(a):
    return None if a is None else a.ctypes.data


def _call(x, labels, k, t=2, n=None, d=None, metric=0, M=None, queries=None, q=None, mode=SYMMETRIC, slab=0, device=False,
          null=(), sizes=True, matrix=False):
    from bliss_rs_amd import _ffi

    n = x.shape[0] if n is None else n
    d = x.shape[1] if d is None else d
    q = (len(queries) if queries is not None else 0) if q is None else q
    kk = max(min(k, 70), 1)
    rows = max(q if queries is not None else kk, 1)
    out = dict(idx=np.full((rows, max(min(t, 2048), 1)), 7, np.uint32), dist=np.full((rows, max(min(t, 2048), 1)), 7.0),
               sizes=np.full(kk, 7, np.uint32), matrix=np.full((kk, kk), 7.0))
    args = (None if "x" in null else _p(x), n, d, None if "labels" in null else _p(labels), k, metric, _p(M), _p(queries), q, t, mode, slab,
            None if "idx" in null else _p(out["idx"]), None if "dist" in null else _p(out["dist"]), _p(out["sizes"]) if sizes else None,
            _p(out["matrix"]) if matrix else None)
    L = _ffi.lib()
    rc = L.blissgpu_group_neighbours_device(None, *args) if device else L.blissgpu_group_neighbours(*args)
    return rc, L.blissgpu_last_error(), out


def test_group_neighbours_arguments_are_checked_before_the_device(bliss):
    import torch

    rng = np.random.default_rng(0)
    X = rng.standard_normal((50, 23)).astype(np.float32)
    lab = (np.arange(50) % 4).astype(np.uint32)
    M = np.eye(23, dtype=np.float32)
    for device in (False, True):
        assert _call(X, lab, 4, d=0, device=device)[0] == INVALID
        assert _call(np.zeros((50, 65), np.float32), lab, 4, device=device)[0] == INVALID
        assert _call(X, lab, 0, device=device)[0] == INVALID
        assert _call(X, lab, 65536, device=device)[0] == INVALID
        assert _call(X, lab, 4, t=0, device=device)[0] == INVALID
        assert _call(X, lab, 4, t=1025, device=device)[0] == INVALID
        assert _call(X, lab, 4, n=0xFFFFFFFF, device=device)[0] == INVALID
        assert _call(X, lab, 4, mode=2, device=device)[0] == INVALID
        assert _call(X, lab, 4, mode=-1, device=device)[0] == INVALID
        assert _call(X, lab, 4, metric=3, device=device)[0] == INVALID
        assert _call(X, lab, 4, metric=2, device=device)[0] == INVALID  # mahalanobis without M
        for what in ("x", "labels", "idx", "dist"):
            rc, err, _ = _call(X, lab, 4, null=(what,), device=device)
            assert rc == INVALID and what.encode() in err, what
        rc, err, _ = _call(X, lab, 4, metric=1, device=device)
        assert rc == INVALID and b"cosine" in err
    # the device form checks the scalars before it looks at its context ...
    rc, err, _ = _call(X, lab, 0, device=True)
    assert rc == INVALID and b"k must be" in err
    rc, err, _ = _call(X, lab, 4, t=0, device=True)
    assert rc == INVALID and b"t must be" in err
    # ... and the context before anything else (the optional outputs may be NULL)
    rc, err, _ = _call(X, lab, 4, metric=2, M=M, device=True, sizes=False)
    assert rc == INVALID and b"ctx" in err
    # the host form's labels and queries are host memory: checked before the device is touched
    bad = lab.copy()
    bad[17] = 4
    rc, err, _ = _call(X, bad, 4)
    assert rc == INVALID and b"label" in err
    rc, err, _ = _call(X, lab, 4, queries=np.array([1, 4, 0], np.uint32))
    assert rc == INVALID and b"query" in err
    # no song: nothing for a device to do -- OK with rows of padding, zero sizes, an empty matrix
    rc, _, out = _call(X[:0], lab[:0], 4, matrix=True)
    assert rc == OK and (out["idx"][:4] == 0xFFFFFFFF).all() and (out["dist"][:4] == np.inf).all() and not out["sizes"][:4].any()
    assert np.array_equal(out["matrix"][:4, :4], np.where(np.eye(4, dtype=bool), 0.0, np.inf))
    rc, _, out = _call(X[:0], lab[:0], 4, queries=np.array([3, 3, 0], np.uint32), t=3)
    assert rc == OK and (out["idx"][:3] == 0xFFFFFFFF).all() and (out["dist"][:3] == np.inf).all()
    # no row to answer: OK, nothing is written to idx / dist, the sizes still are
    rc, _, out = _call(X, lab, 4, queries=np.zeros(0, np.uint32), q=0)
    assert rc == OK and (out["idx"] == 7).all() and (out["dist"] == 7.0).all() and out["sizes"][:4].tolist() == [13, 13, 12, 12]
    # a valid call: BLISSGPU_ERR_NO_DEVICE without a GPU, BLISSGPU_OK with one
    want = OK if torch.cuda.is_available() else NO_DEVICE
    assert _call(X, lab, 4)[0] == want
    assert _call(X, lab, 4, metric=2, M=M, queries=np.array([2, 2], np.uint32), mode=DIRECTED, slab=3, matrix=True)[0] == want
    assert _call(X, np.zeros(50, np.uint32), 1)[0] == want  # one group: not an error


# ---- the Python layer above a numpy stand-in ----
def _numpy_group_neighbours(P):
    """playlist.group_neighbours with the device call replaced by `contract` over numpy f32 euclidean distances"""
    calls = []

    def fake(songs_or_X, labels, t, metric_builder=P.euclidean_distance, k=None, queries=None, mode="symmetric", matrix=False,
             slab_groups=0):
        P._group_neighbours_metric(metric_builder)
        X = P._rows_of_input(songs_or_X)
        lab = np.asarray(labels).reshape(-1).astype(np.int64)
        keep = lab >= 0
        X, lab = X[keep], lab[keep]
        k = int(lab.max()) + 1 if k is None else int(k)
        diff = X[:, None, :].astype(np.float32) - X[None, :, :].astype(np.float32)
        Dm = np.sqrt((diff * diff).sum(axis=2, dtype=np.float32)).astype(np.float32)
        calls.append((X.shape[0], k, int(t), mode))
        idx, dist, sizes, mat = contract(Dm, lab, k, int(t), SYMMETRIC if mode == "symmetric" else DIRECTED, queries)
        return P.GroupNeighbours(idx, dist, sizes, mat if matrix else None)

    return fake, calls


def test_playlist_group_neighbours_host_logic(bliss):
    P = bliss.playlist
    rng = np.random.default_rng(5)
    X = rng.standard_normal((12, 23)).astype(np.float32)
    lab = np.arange(12) % 3
    # refused builders, in the style of the silhouette
    for builder, word in ((P.cosine_distance, "cosine"), ("cosine", "cosine"), (P.ForestOptions(10, 8, 3, 0), "forest"),
                          (P.VarianceWeights(), "MahalanobisBuilder")):
        with pytest.raises(ValueError) as e:
            P.group_neighbours(X, lab, 2, builder)
        assert word in str(e.value)
    with pytest.raises(TypeError):
        P.group_neighbours(X, lab, 2, lambda a, b: 0.0)
    with pytest.raises(ValueError):
        P.group_neighbours(X, lab, 2, mode="both")
    with pytest.raises(ValueError):
        P.group_neighbours(X, lab[:-1], 2)
    # rows with a negative label are left out before the call: here every row, so no device is needed
    res = P.group_neighbours(X, np.full(12, -1), 2, k=3, matrix=True)
    assert res.idx.tolist() == [[-1, -1]] * 3 and np.isinf(res.dist).all() and res.sizes.tolist() == [0, 0, 0]
    assert res.idx.dtype == np.int64 and res.dist.dtype == np.float64 and res.sizes.dtype == np.int64
    assert np.array_equal(res.matrix, np.where(np.eye(3, dtype=bool), 0.0, np.inf))
    assert P.group_neighbours(X, np.full(12, -1), 2, k=3).matrix is None
    # no query: the sizes of the rows that are left
    res = P.group_neighbours(X, np.where(np.arange(12) < 4, -1, lab), 2, queries=[])
    assert res.idx.shape == (0, 2) and res.sizes.tolist() == [2, 3, 3]
    # errors of the C layer arrive as BlissGpuError(ERR_INVALID) before a device is needed
    for kwargs in (dict(k=2), dict(queries=[3]), dict(t=0)):
        with pytest.raises(bliss.BlissGpuError) as e:
            P.group_neighbours(X, lab, **{"t": 2, **kwargs})
        assert e.value.code == INVALID


@pytest.fixture()
def artists_db(bliss, tmp_path):
    """five artists around planted centres; artist "e" has one song, songs 7, 17, 27 and 37 have no artist tag"""
    rng = np.random.default_rng(21)
    centre = {"a": 0.0, "b": 1.0, "c": 1.5, "d": 6.0, "e": 6.5}
    names = ["a", "b", "c", "d"]
    V2 = bliss.FeaturesVersion.Version2
    songs, rows = [], []
    for i in range(41):
        artist = "e" if i == 40 else (None if i % 10 == 7 else names[i % 4])
        x = (centre[artist or "a"] + 0.05 * rng.standard_normal(23)).astype(np.float32)
        rows.append(x)
        songs.append(bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist=artist, album=[None, "zeta", "alpha"][i % 3],
                                disc_number=[None, 2, 1][(i // 3) % 3], track_number=[5, None, 3, 1][(i // 9) % 4], duration=1.0,
                                genre="g", analysis=bliss.Analysis(x, V2), features_version=V2))
    db = str(tmp_path / "bliss.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs)
    return db, songs


def test_library_similar_groups_keys_and_order(bliss, monkeypatch, artists_db):
    P, Lb = bliss.playlist, bliss.library
    db, songs = artists_db
    fake, calls = _numpy_group_neighbours(P)
    monkeypatch.setattr(P, "group_neighbours", fake)
    sim = Lb.similar_artists(db, 2)
    assert list(sim) == ["a", "b", "c", "d", "e"]  # first appearance in id order; NULL tags are left out
    assert calls == [(37, 5, 2, "symmetric")]  # one call answers every key
    assert [[k for k, _ in sim[key]] for key in sim] == [["b", "c"], ["c", "a"], ["b", "a"], ["e", "c"], ["d", "c"]]
    for key in sim:
        v = [dist for _, dist in sim[key]]
        assert v == sorted(v) and all(isinstance(x, float) and np.isfinite(x) for x in v)
    assert sim["a"][0][1] == sim["b"][1][1]  # symmetric
    assert Lb.similar_groups(db, 2, "artist") == sim
    # more neighbours than other keys: every other key, no padding entry
    assert [len(v) for v in Lb.similar_groups(db, 9).values()] == [4] * 5 and calls[-1] == (37, 5, 4, "symmetric")
    directed = Lb.similar_groups(db, 1, "artist", mode="directed")
    assert calls[-1] == (37, 5, 1, "directed") and directed["e"][0][0] == "d"
    # another column: one key only -> nothing to rank, no call
    n_calls = len(calls)
    assert Lb.similar_groups(db, 3, "genre") == {"g": []} and len(calls) == n_calls
    assert Lb.similar_groups(db, 0) == {key: [] for key in "abcde"} and len(calls) == n_calls
    assert sorted(Lb.similar_groups(db, 1, "album")) == ["alpha", "zeta"]
    with pytest.raises(ValueError):
        Lb.similar_groups(db, 2, "title")
    with pytest.raises(ValueError):
        Lb.similar_groups(db, -1)
    with pytest.raises(ValueError):
        Lb.similar_groups(db, 2, metric_builder=P.cosine_distance)


def test_library_similar_artists_playlist(bliss, monkeypatch, artists_db):
    P, Lb = bliss.playlist, bliss.library
    db, songs = artists_db
    fake, calls = _numpy_group_neighbours(P)
    monkeypatch.setattr(P, "group_neighbours", fake)

    def key(s):  # (album, disc, track), None first
        return tuple((0, 0) if v is None else (1, v) for v in (s.album, s.disc_number, s.track_number))

    def of(artist):
        return [s.path for s in sorted((s for s in songs if s.artist == artist), key=key)]  # (stable: ties stay in id order)

    pl = Lb.similar_artists_playlist(db, "d", 2)
    assert [s.path for s in pl] == of("d") + of("e") + of("c") and len(calls) == 1
    first = [s for s in pl if s.artist == "d"]
    assert [s.album for s in first] == sorted((s.album for s in first), key=lambda a: (a is not None, a or ""))
    # the zero case: the artist's own songs, no call
    assert [s.path for s in Lb.similar_artists_playlist(db, "b", 0)] == of("b") and len(calls) == 1
    # an unknown artist: the ProviderError of songs_from_album, before any call
    with pytest.raises(bliss.ProviderError) as e:
        Lb.similar_artists_playlist(db, "nobody", 2)
    assert "was not found" in str(e.value) and len(calls) == 1
    with pytest.raises(ValueError):
        Lb.similar_artists_playlist(db, "a", -1)
