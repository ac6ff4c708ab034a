"""GPU tests (-m gpu) of the song-to-song chains cut after k (blissgpu_chains / blissgpu_chains_device: chain_step_kernel,
chain_walk_kernel): the first k songs of song_to_song(&group, candidates, metric) of the reference (src/playlist.rs:272-326) for
many seed groups in one call.  The expected values never come from the code under test: rows of the CPU oracle's distance
matrix (oracle.pairwise) -- added sequentially in numpy f32 in seed order for step 0, `0.0f +` a row of the candidates' own
matrix for every later step -- and np.argmin over the row with the skipped and taken columns set to +inf.  That restatement is
pinned to oracle.song_to_song in this file.  The distances are bit-identical by contract, so the chains are a discrete result:
every comparison is exact (np.array_equal on indices, bit equality on distances), for the host and the device form and for
every route (steps, lists, auto)."""
import json
import os
import sqlite3

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ("euclidean", "cosine", "weights", "spd")
ROUTES = ("steps", "lists", "auto")
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "playlist_cases.json")))
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "library_playlist_cases.json")))


@pytest.fixture(scope="module")
def bliss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import bliss_rs_amd

    return bliss_rs_amd


@pytest.fixture(scope="module")
def ctx(bliss):
    c = bliss.Context(0)
    yield c
    c.close()


def _metric(oracle, name, d):
    """-> (library metric name, M or None), as tests/test_gpu_group_knn.py builds them"""
    if name in ("euclidean", "cosine"):
        return name, None
    if name == "weights":
        return "mahalanobis", oracle.feature_weights(2 if d == 23 else 1) if d in (23, 20) else np.eye(d, dtype=np.float32)
    rng = np.random.default_rng(7)
    A = rng.standard_normal((d, d)) * 0.3
    return "mahalanobis", (A @ A.T + 0.1 * np.eye(d)).astype(np.float32)


def tie_rich(rng, n, d, copies=20):
    """features on a grid of eighths (many equal distances), one row in `copies` a copy of another row"""
    X = (rng.integers(-8, 9, (n, d)) / 8).astype(np.float32)
    dup = rng.choice(n, n // copies, replace=False)
    X[dup] = X[rng.integers(0, n, n // copies)]
    return X


def offsets_of(sizes):
    off = np.zeros(len(sizes) + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    return off


def restate(oracle, S, off, X, k, metric, M, skip=None, DX=None):
    """The chains as masked argmins over the oracle's distances -> (idx int64[G, k], dist f32[G, k], steps with two or more
    eligible candidates at the minimum).  A NaN among the eligible values of a step that runs raises ValueError.  DX: the
    candidates' own matrix when the caller has it (otherwise one oracle row per step)."""
    off = np.asarray(off, np.int64)
    G, n = off.shape[0] - 1, X.shape[0]
    idx, dist, ties = np.full((G, k), -1, np.int64), np.full((G, k), np.inf, np.float32), 0
    D0 = oracle.pairwise(S, X, metric, M, n_threads=16) if S.shape[0] else np.zeros((0, n), np.float32)
    for g in range(G):
        free = np.ones(n, bool)
        if skip is not None:
            sk = np.asarray(skip[off[g]:off[g + 1]], np.int64)
            free[sk[sk >= 0]] = False
        row = np.zeros(n, np.float32)
        for s in range(off[g], off[g + 1]):
            row = row + D0[s]  # sequentially in f32, in seed order
        for t in range(k):
            if not free.any():
                break
            if np.isnan(row[free]).any():
                raise ValueError("NaN distance")
            v = np.where(free, row, np.float32(np.inf))
            j = int(np.argmin(v))  # the first minimum: the lowest index among equals
            ties += int((row[free] == v[j]).sum() >= 2)
            idx[g, t], dist[g, t] = j, v[j]
            free[j] = False
            nxt = DX[j] if DX is not None else oracle.pairwise(X[j:j + 1], X, metric, M)[0]
            row = np.float32(0) + nxt
    return idx, dist, ties


def host_form(bliss, S, off, X, k, metric, M, skip, route):
    return bliss.playlist.chain_order((S, off), X, k, metric, M, skip, route)


def device_form(ctx, S, off, X, k, metric, M, skip, route):
    import torch

    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()  # noqa: E731
    idx, dist = ctx.chains(t(S, np.float32), off, t(X, np.float32), k, metric, t(M, np.float32), t(skip, np.int32), route)
    ctx.synchronize()
    return idx.cpu().numpy().astype(np.int64), dist.cpu().numpy()


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "indices", int((got[0] != want[0]).any(axis=1).sum()), "rows differ")
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (what, "distance bits")


def check_all(bliss, ctx, S, off, X, k, metric, M, skip, want, what="", routes=ROUTES):
    for route in routes:
        assert_same(host_form(bliss, S, off, X, k, metric, M, skip, route), want[:2], (what, route, "host form"))
        assert_same(device_form(ctx, S, off, X, k, metric, M, skip, route), want[:2], (what, route, "device form"))


def _ragged(rng, n, n_groups=60, most=9):
    """groups of 0 .. most seeds drawn from the rows, every seed skipping its own row"""
    sizes = rng.integers(0, most + 1, n_groups)
    sizes[:3] = (0, 1, most)
    off = offsets_of(sizes)
    rows = rng.integers(0, n, int(off[-1]))
    return off, rows


# ---- the restatement is the reference's song_to_song cut after k ----
def test_restatement_is_the_oracles_song_to_song(oracle):
    rng = np.random.default_rng(21)
    X = tie_rich(rng, 300, 23)
    for g, (size, metric) in enumerate(zip((1, 2, 5, 9, 3, 1), ("euclidean", "cosine", "weights", "spd", "euclidean", "cosine"))):
        name, M = _metric(oracle, metric, 23)
        rows = rng.integers(0, 300, size)
        S, k = X[rows], 40
        keep = np.setdiff1d(np.arange(300), rows)  # the skipped rows removed from the candidates, indices mapped back
        want = keep[oracle.song_to_song(S, X[keep], name, M).astype(np.int64)[:k]]
        got, _, _ = restate(oracle, S, offsets_of([size]), X, k, name, M, rows)
        assert np.array_equal(got[0], want), (g, metric)


# ---- (a) ties and ragged groups: three candidate blocks, the last one ragged ----
@pytest.mark.parametrize("metric", METRICS)
def test_ties_and_ragged_groups(bliss, ctx, oracle, metric):
    rng = np.random.default_rng(2)
    n, d = 700, 23
    X = tie_rich(rng, n, d)
    off, rows = _ragged(rng, n)
    name, M = _metric(oracle, metric, d)
    DX = oracle.pairwise(X, X, name, M, n_threads=16)
    for k in (1, 20, 64):
        want = restate(oracle, X[rows], off, X, k, name, M, rows, DX)
        if k == 20:
            assert want[2] >= 50, ("steps with a tie at the minimum", want[2])
        check_all(bliss, ctx, X[rows], off, X, k, name, M, rows, want, what=(metric, k))


# ---- (b) other feature counts: the second packed width and the generic path ----
@pytest.mark.parametrize("d", (20, 5, 64))
def test_other_feature_counts(bliss, ctx, oracle, d):
    rng = np.random.default_rng(3)
    n, k = 300, 64
    X = tie_rich(rng, n, d)
    off, rows = _ragged(rng, n, n_groups=20, most=5)
    for metric in METRICS:
        name, M = _metric(oracle, metric, d)
        DX = oracle.pairwise(X, X, name, M, n_threads=16)
        want = restate(oracle, X[rows], off, X, k, name, M, rows, DX)
        check_all(bliss, ctx, X[rows], off, X, k, name, M, rows, want, what=(d, metric))


# ---- (c) every song as a one-seed group with its own row skipped: the lists hold the whole library ----
def test_every_song_of_a_small_library(bliss, ctx, oracle):
    rng = np.random.default_rng(4)
    n = 130
    X = tie_rich(rng, n, 23)
    off, rows = np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int64)
    DX = oracle.pairwise(X, X, "euclidean", None, n_threads=16)
    want = restate(oracle, X, off, X, n - 1, "euclidean", None, rows, DX)
    assert (want[0] >= 0).all() and all(sorted(r.tolist() + [g]) == list(range(n)) for g, r in enumerate(want[0]))
    check_all(bliss, ctx, X, off, X, n - 1, "euclidean", None, rows, want, what="k = n - 1")
    # more songs asked than there are: every row ends in 11 entries of -1 / inf
    want = restate(oracle, X, off, X, 140, "euclidean", None, rows, DX)
    assert (want[0][:, 129:] == -1).all() and np.isinf(want[1][:, 129:]).all() and (want[0][:, :129] >= 0).all()
    check_all(bliss, ctx, X, off, X, 140, "euclidean", None, rows, want, what="k > n - 1")


# ---- (d) few chains: several workgroups share a chain's candidates; the split must not show ----
@pytest.mark.parametrize("n_chains", (1, 3))
def test_few_chains_share_their_candidates(bliss, ctx, oracle, n_chains):
    rng = np.random.default_rng(5)
    n, k = 5000, 8
    X = tie_rich(rng, n, 23)
    rows = rng.integers(0, n, n_chains)
    off = np.arange(n_chains + 1, dtype=np.int64)
    want = restate(oracle, X[rows], off, X, k, "euclidean", None, rows)
    for _ in range(2):
        check_all(bliss, ctx, X[rows], off, X, k, "euclidean", None, rows, want, what=n_chains)


# ---- (e) the largest k, by steps ----
def test_largest_k_by_steps(bliss, ctx, oracle):
    rng = np.random.default_rng(6)
    n, k = 1100, 1024
    X = tie_rich(rng, n, 23)
    rows = np.array([5, 900, 17], np.int64)
    off = np.array([0, 1, 3], np.int64)
    DX = oracle.pairwise(X, X, "euclidean", None, n_threads=16)
    want = restate(oracle, X[rows], off, X, k, "euclidean", None, rows, DX)
    check_all(bliss, ctx, X[rows], off, X, k, "euclidean", None, rows, want, routes=("steps", "auto"))
    with pytest.raises(ValueError):  # L = 1025
        host_form(bliss, X[rows], off, X, k, "euclidean", None, rows, "lists")


# ---- (f) NaN: an error exactly when a chain evaluates one within the steps it runs ----
def test_nan_only_where_a_chain_looks(bliss, ctx, oracle):
    rng = np.random.default_rng(8)
    n, k, bad = 400, 12, 123
    X = tie_rich(rng, n, 23)
    X[bad] = np.nan
    sizes = rng.integers(1, 5, 30)
    off = offsets_of(sizes)
    rows = rng.integers(0, n - 1, int(off[-1]))
    rows[rows == bad] = bad + 1
    skip = rows.copy()
    skip[off[:-1]] = bad  # every group's first seed skips the NaN row (its other seeds their own rows)
    want = restate(oracle, X[rows], off, X, k, "euclidean", None, skip)
    check_all(bliss, ctx, X[rows], off, X, k, "euclidean", None, skip, want, what="skipped NaN row")
    skip[off[7]] = -1  # one group looks at it
    with pytest.raises(ValueError):
        restate(oracle, X[rows], off, X, k, "euclidean", None, skip)
    for route in ROUTES:
        with pytest.raises(ValueError, match="NaN"):
            host_form(bliss, X[rows], off, X, k, "euclidean", None, skip, route)
        with pytest.raises(bliss.BlissGpuError):
            device_form(ctx, X[rows], off, X, k, "euclidean", None, skip, route)


def test_nan_beyond_the_last_step_is_never_looked_at(bliss, ctx, oracle):
    """Two rows whose cosine norms overflow: their distance to any ordinary row is 1.0, to each other inf / inf = NaN.  The
    chain seed -> near -> huge_a stops at its k-th song: the NaN between huge_a and huge_b is one step further."""
    rng = np.random.default_rng(9)
    n, d = 300, 23
    X = -rng.uniform(0.5, 1.0, (n, d)).astype(np.float32)  # farther than 1.0 from every all-positive row
    seed = np.ones((1, d), np.float32)
    near, huge_a, huge_b = 40, 100, 200
    X[near] = seed[0] + rng.uniform(0.0, 0.1, d).astype(np.float32)
    X[huge_a] = X[huge_b] = np.float32(1e30)
    off = np.array([0, 1], np.int64)
    want = restate(oracle, seed, off, X, 2, "cosine", None)
    assert want[0].tolist() == [[near, huge_a]] and want[1][0, 1] == 1.0
    assert np.isnan(oracle.pairwise(X[[huge_a]], X[[huge_b]], "cosine")[0, 0])
    check_all(bliss, ctx, seed, off, X, 2, "cosine", None, None, want, what="the NaN is one step further")
    for route in ROUTES:
        with pytest.raises(ValueError, match="NaN"):
            host_form(bliss, seed, off, X, 3, "cosine", None, None, route)


# ---- (g) the reference's own cases ----
def test_reference_song_to_song_cases_cut_after_k(bliss):  # src/playlist.rs:506-1007
    P = bliss.playlist
    S = {name: bliss.Song(path=f"path-to-{name}", analysis=bliss.Analysis(s["analysis"], bliss.FeaturesVersion.LATEST),
                          title=s.get("title"), artist=s.get("artist")) for name, s in CASES["songs"].items()}
    fn = {"euclidean": P.euclidean_distance, "cosine": P.cosine_distance}
    assert CASES["song_to_song"]
    for c in CASES["song_to_song"]:
        for k in range(1, len(c["expected"]) + 1):
            got = P.song_to_song([S[x] for x in c["initial"]], [S[x] for x in c["candidates"]], fn[c["metric"]], number_songs=k)
            assert [id(x) for x in got] == [id(S[x]) for x in c["expected"][:k]], (c, k)


@pytest.fixture(scope="module")
def db(bliss, tmp_path_factory):
    """the reference's test library (setup_test_library), as tests/test_gpu_library_playlist.py writes it"""
    path = str(tmp_path_factory.mktemp("chains") / "bliss.db")
    L = bliss.library
    L.create_schema(path)
    conn = sqlite3.connect(path)
    cols = ("id", "path", "artist", "title", "album", "album_artist", "track_number", "disc_number", "genre", "duration",
            "analyzed", "version", "extra_info", "cue_path", "audio_file_path", "error")
    for r in sorted(FIXTURE["rows"], key=lambda r: r["id"]):
        if r["analyzed"] and r["version"] == 2 and len(r["features"]) == 23:
            L.store_song(conn, bliss.Song(path=r["path"], artist=r["artist"], title=r["title"], album=r["album"],
                                          album_artist=r["album_artist"], track_number=r["track_number"],
                                          disc_number=r["disc_number"], genre=r["genre"], duration=float(r["duration"]),
                                          analysis=bliss.Analysis(r["features"], bliss.FeaturesVersion.Version2),
                                          features_version=bliss.FeaturesVersion.Version2))
        else:
            conn.execute("insert into song (%s) values (%s)" % (", ".join(cols), ", ".join("?" * len(cols))),
                         tuple(r[c] for c in cols))
            conn.executemany("insert into feature (song_id, feature, feature_index) values (?, ?, ?)",
                             [(r["id"], v, i) for i, v in enumerate(r["features"])])
    conn.commit()
    conn.close()
    return path


def test_library_chain_playlists_are_playlist_from_custom(bliss, db):
    L, P = bliss.library, bliss.playlist
    table = L.chain_playlists(db, 3, by="song")
    paths = [s.path for s in L.load_songs(db)]
    assert list(table) == paths and len(paths) >= 5
    for p in paths:
        full = L.playlist_from_custom(db, [p], P.euclidean_distance, P.song_to_song, deduplicate=False)
        assert [q for q, _ in table[p]] == [s.path for s in full[1:4]], p
    # an album as the seed set: the songs closest to the album, then from song to song
    albums = L.chain_playlists(db, 3, by="album")
    for key, got in albums.items():
        members = [s.path for s in L.load_songs(db) if s.album == key]
        full = L.playlist_from_custom(db, members, P.euclidean_distance, P.song_to_song, deduplicate=False)
        assert [q for q, _ in got] == [s.path for s in full[len(members):][:3]], key


# ---- the host form's staging: every optional argument given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("route", (1, 2))  # BLISSGPU_CHAINS_STEPS, BLISSGPU_CHAINS_LISTS
@pytest.mark.parametrize("skip,dist", ((True, True), (False, False), (True, False), (False, True)))
def test_host_form_stages_like_the_device_form(bliss, ctx, skip, dist, route):
    import staging_cases as sc

    def build(c, dev):
        idx, dd = dev(sc.out((c.G, c.k), np.uint32)), dev(sc.out((c.G, c.k), np.float32, dist))
        return [dev(c.S), c.off, c.G, dev(c.X), c.n, sc.D, 2, dev(c.M), dev(c.skip if skip else None), c.k, route, idx, dd], [idx, dd]

    sc.check(bliss, ctx, "chains", build)
