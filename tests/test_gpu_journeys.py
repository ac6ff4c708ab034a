"""GPU tests (-m gpu) of the journeys (blissgpu_journeys / blissgpu_journeys_device: journey_step_kernel): waypoint playlists
("from song1 to song2 in n songs, without repetitions") and directed playlists ("the tempo goes down or stays the same"), the
two playlist shapes the reference's TODO.md names and does not ship.  The expected values never come from the code under test:
rows of the CPU oracle's distance matrix (oracle.pairwise) for query rows built here in numpy f32 --
a + (b - a) * (float32(t + 1) / float32(k + 1)) for a waypoint, the previous pick's row for a chain -- then `0.0f +` the row and
the first minimum over the eligible columns (not skipped, not taken, and with a gate the feature comparison against the
previous pick).  Distances are bit-identical by contract, so a journey is a discrete result: every comparison is exact
(np.array_equal on indices, bit equality on distances), for the host and the device form."""
import json
import os
import sqlite3

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ("euclidean", "cosine", "weights", "spd")
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
    """-> (library metric name, M or None), as tests/test_gpu_chains.py builds them"""
    if name in ("euclidean", "cosine"):
        return name, None
    if name == "weights":
        return "mahalanobis", oracle.feature_weights(2 if d == 23 else 1) if d in (23, 20) else np.eye(d, dtype=np.float32)
    rng = np.random.default_rng(7)
    A = rng.standard_normal((d, d)) * 0.3
    return "mahalanobis", (A @ A.T + 0.1 * np.eye(d)).astype(np.float32)


def tie_rich(rng, n, d, copies=20):
    """features on a grid of eighths (many equal distances and equal features), one row in `copies` (5 %) a copy of another"""
    X = (rng.integers(-8, 9, (n, d)) / 8).astype(np.float32)
    dup = rng.choice(n, n // copies, replace=False)
    X[dup] = X[rng.integers(0, n, n // copies)]
    return X


def ends_of(n, G):
    """journey g starts at row g and ends at row n - 1 - g; both rows are skipped -> (from rows, to rows, skip [G, 2])"""
    a, b = np.arange(G), n - 1 - np.arange(G)
    return a, b, np.stack([a, b], axis=1).astype(np.int64)


def waypoints(A, B, k):
    """[G, k, d]: a + (b - a) * s_t in f32, every operation rounded on its own, s_t = float32(t + 1) / float32(k + 1)"""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    s = (np.arange(1, k + 1, dtype=np.float32) / np.float32(k + 1)).astype(np.float32)
    step = ((B - A)[:, None, :] * s[None, :, None]).astype(np.float32)
    return (A[:, None, :] + step).astype(np.float32)


class Count:
    """what a restatement met: a degenerate input cannot pass silently"""

    def __init__(self):
        self.early = self.full = self.ties = self.equal_feature = self.changed = 0


def restate(oracle, A, B, X, k, metric, M, skip=None, gate=None, feature=0, DX=None):
    """The journeys as masked first minima over the oracle's distances -> (idx int64[G, k], dist f32[G, k], Count).  B given:
    waypoint journeys; otherwise chains, `gate` "up" / "down" on column `feature`.  A NaN among the eligible values of a step
    that runs raises ValueError.  DX: the candidates' own matrix when the caller has it (otherwise one oracle row per step)."""
    A, X = np.asarray(A, np.float32), np.asarray(X, np.float32)
    G, n = A.shape[0], X.shape[0]
    idx, dist, c = np.full((G, k), -1, np.int64), np.full((G, k), np.inf, np.float32), Count()
    rows = lambda Q: oracle.pairwise(np.ascontiguousarray(Q, np.float32), X, metric, M, n_threads=16)  # noqa: E731
    if B is not None:
        assert gate is None
        W = rows(waypoints(A, B, k).reshape(G * k, -1)).reshape(G, k, n)
    else:
        D0 = rows(A)
    for g in range(G):
        free = np.ones(n, bool)
        if skip is not None:
            sk = np.asarray(skip[g], np.int64)
            free[sk[sk >= 0]] = False
        allowed = free.copy()  # everything but the skipped rows
        ref, prev = A[g, feature], None
        for t in range(k):
            if B is not None:
                row = W[g, t]
            elif t == 0:
                row = D0[g]
            else:
                row = DX[prev] if DX is not None else rows(X[prev:prev + 1])[0]
            row = np.float32(0) + row
            eligible = free.copy()
            if gate is not None:
                with np.errstate(invalid="ignore"):
                    eligible &= (X[:, feature] >= ref) if gate == "up" else (X[:, feature] <= ref)  # a NaN passes neither
            cand = np.nonzero(eligible)[0]
            if cand.size == 0:
                c.early += 1
                break
            if np.isnan(row[cand]).any():
                raise ValueError("NaN distance")
            j = int(cand[np.argmin(row[cand])])  # the first minimum: the lowest index among equals
            c.ties += int((row[cand] == row[j]).sum() >= 2)
            if gate is not None:
                c.equal_feature += int(X[j, feature] == ref)
            else:
                every = np.nonzero(allowed)[0]
                c.changed += int(not free[every[np.argmin(row[every])]])  # the unrestricted nearest was already taken
            idx[g, t], dist[g, t] = j, row[j]
            free[j] = False
            ref, prev = X[j, feature], j
        else:
            c.full += 1
    return idx, dist, c


def host_form(bliss, A, B, X, k, metric, M, skip, gate=None, feature=None):
    return bliss.playlist.journey_order(A, X, k, B, metric, M, skip, gate, feature)


def device_form(ctx, A, B, X, k, metric, M, skip, gate=None, feature=0):
    import torch

    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()  # noqa: E731
    idx, dist = ctx.journeys(t(A, np.float32), t(B, np.float32), t(X, np.float32), k, metric, t(M, np.float32), t(skip, np.int32),
                             "chain" if B is None else "waypoint", gate, feature or 0)
    ctx.synchronize()
    return idx.cpu().numpy().astype(np.int64), dist.cpu().numpy()


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "indices", int((got[0] != want[0]).any(axis=1).sum()), "rows differ")
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (what, "distance bits")


def check(bliss, ctx, oracle, A, B, X, k, metric, M, skip, gate=None, feature=None, DX=None, what=""):
    """both forms against the restatement -> its Count"""
    want = restate(oracle, A, B, X, k, metric, M, skip, gate, feature or 0, DX)
    assert_same(host_form(bliss, A, B, X, k, metric, M, skip, gate, feature), want[:2], (what, gate, feature, "host form"))
    assert_same(device_form(ctx, A, B, X, k, metric, M, skip, gate, feature), want[:2], (what, gate, feature, "device form"))
    return want[2]


GATES = (("down", 0), ("up", 0), ("down", -1), ("up", -1))  # (direction, column: -1 = the last)


# ---- (a) the two shapes of the issue: a ragged last block, more than 32 journeys (a second, ragged chain block), ties ----
@pytest.mark.parametrize("metric", METRICS)
def test_waypoints_and_gates(bliss, ctx, oracle, metric):
    d, k = 23, 20
    name, M = _metric(oracle, metric, d)
    early = full = 0
    for n, G in ((1000, 70), (300, 33)):
        X = tie_rich(np.random.default_rng(3), n, d)
        a, b, skip = ends_of(n, G)
        DX = oracle.pairwise(X, X, name, M, n_threads=16)
        c = check(bliss, ctx, oracle, X[a], X[b], X, k, name, M, skip, what=(metric, n, "waypoint"))
        assert c.changed >= 1 and c.full == G  # an exclusion changed a pick; a waypoint journey never ends early here
        c = check(bliss, ctx, oracle, X[a], None, X, k, name, M, skip, DX=DX, what=(metric, n, "chain"))
        assert c.full == G
        for gate, col in GATES:
            c = check(bliss, ctx, oracle, X[a], None, X, k, name, M, skip, gate, col % d, DX, what=(metric, n))
            assert c.equal_feature >= 1, (gate, col)
            if (gate, col) == ("down", 0):
                assert c.ties >= 1 or metric != "euclidean"
                early, full = early + c.early, full + c.full
    assert early >= 1 and full >= 1  # gated journeys that end early and gated journeys that run all k steps


# ---- (b) other feature counts: the second packed path and the generic path ----
@pytest.mark.parametrize("d,metric", [(20, m) for m in METRICS] + [(7, m) for m in METRICS])
def test_other_feature_counts(bliss, ctx, oracle, d, metric):
    n, G, k = 300, 33, 20
    name, M = _metric(oracle, metric, d)
    X = tie_rich(np.random.default_rng(3), n, d)
    a, b, skip = ends_of(n, G)
    DX = oracle.pairwise(X, X, name, M, n_threads=16)
    c = check(bliss, ctx, oracle, X[a], X[b], X, k, name, M, skip, what=(d, metric, "waypoint"))
    assert c.changed >= 1
    check(bliss, ctx, oracle, X[a], None, X, k, name, M, skip, DX=DX, what=(d, metric, "chain"))
    seen = Count()
    for gate, col in GATES:
        c = check(bliss, ctx, oracle, X[a], None, X, k, name, M, skip, gate, col % d, DX, what=(d, metric))
        seen.early, seen.full, seen.equal_feature = seen.early + c.early, seen.full + c.full, seen.equal_feature + c.equal_feature
    assert seen.early >= 1 and seen.equal_feature >= 1


# ---- (c) the edges of a 256-candidate block, one candidate, and more steps than candidates (padding) ----
@pytest.mark.parametrize("n", (1, 255, 256, 257))
def test_block_edges(bliss, ctx, oracle, n):
    d, k, G = 23, 6, 3
    rng = np.random.default_rng(3)
    X = tie_rich(rng, max(n, 20), d)[:n]
    A, B = tie_rich(rng, 20, d)[:G], tie_rich(rng, 20, d)[:G]  # end points that are no candidates: nothing skipped
    last = np.full((G, 2), -1, np.int64)
    last[:, 0] = n - 1  # ... or the block's last row skipped
    for skip in (None, last):
        c = check(bliss, ctx, oracle, A, B, X, k, "euclidean", None, skip, what=(n, "waypoint"))
        assert (c.full == G) == (n - (skip is not None) >= k)
        check(bliss, ctx, oracle, A, None, X, k, "euclidean", None, skip, what=(n, "chain"))
        for gate, col in GATES:
            check(bliss, ctx, oracle, A, None, X, k, "cosine", None, skip, gate, col % d, what=(n,))


@pytest.mark.parametrize("k", (1, 2, 20))
def test_step_counts_and_padding(bliss, ctx, oracle, k):
    """n = 12 candidates of which two are skipped: k = 20 leaves ten songs and ten entries of padding"""
    d, n, G = 23, 12, 5
    X = tie_rich(np.random.default_rng(3), n, d, copies=4)
    a, b, skip = ends_of(n, G)
    for B in (X[b], None):
        want = restate(oracle, X[a], B, X, k, "euclidean", None, skip)
        assert ((want[0] >= 0).sum(axis=1) == min(k, n - 2)).all() and (want[2].early == G) == (k > n - 2)
        assert_same(host_form(bliss, X[a], B, X, k, "euclidean", None, skip), want[:2], (k, "host form"))
        assert_same(device_form(ctx, X[a], B, X, k, "euclidean", None, skip), want[:2], (k, "device form"))
    check(bliss, ctx, oracle, X[a], None, X, k, "euclidean", None, skip, "down", d - 1, what=(k, "gated"))


# ---- (d) few journeys: several workgroups share a journey's candidates (atomicMin, then the put launch) ----
@pytest.mark.parametrize("G", (1, 3))
def test_few_journeys_share_their_candidates(bliss, ctx, oracle, G):
    n, d, k = 5000, 23, 20
    X = tie_rich(np.random.default_rng(3), n, d)
    a, b, skip = ends_of(n, G)
    for B, gate, col in ((X[b], None, None), (None, "down", 0), (None, "up", d - 1), (None, None, None)):
        want = restate(oracle, X[a], B, X, k, "euclidean", None, skip, gate, col or 0)
        first = device_form(ctx, X[a], B, X, k, "euclidean", None, skip, gate, col)
        assert_same(first, want[:2], (G, gate, "device form"))
        assert_same(device_form(ctx, X[a], B, X, k, "euclidean", None, skip, gate, col), first, (G, gate, "the same bits twice"))
        assert_same(host_form(bliss, X[a], B, X, k, "euclidean", None, skip, gate, col), want[:2], (G, gate, "host form"))


# ---- (e) identities with the entry points that exist ----
@pytest.mark.parametrize("metric", METRICS)
def test_chain_without_a_gate_is_chains_for_one_seed_groups(bliss, ctx, oracle, metric):
    import torch

    n, d, k, G = 1000, 23, 20, 70
    name, M = _metric(oracle, metric, d)
    X = tie_rich(np.random.default_rng(3), n, d)
    a, _, _ = ends_of(n, G)
    skip = np.stack([a, np.full(G, -1)], axis=1)
    got = device_form(ctx, X[a], None, X, k, name, M, skip)
    t = lambda v, dt: None if v is None else torch.from_numpy(np.ascontiguousarray(v).astype(dt)).cuda()  # noqa: E731
    for route in ("steps", "lists", "auto"):
        idx, dist = ctx.chains(t(X[a], np.float32), np.arange(G + 1), t(X, np.float32), k, name, t(M, np.float32), t(a, np.int32), route)
        ctx.synchronize()
        assert_same(got, (idx.cpu().numpy().astype(np.int64), dist.cpu().numpy()), (metric, route))


@pytest.mark.parametrize("metric", METRICS)
def test_waypoint_to_itself_is_knn_cut_after_k(bliss, ctx, oracle, metric):
    import torch

    n, d, k, G = 1000, 23, 20, 70
    name, M = _metric(oracle, metric, d)
    X = tie_rich(np.random.default_rng(3), n, d)
    a, _, _ = ends_of(n, G)
    skip = np.stack([a, np.full(G, -1)], axis=1)
    got = device_form(ctx, X[a], X[a], X, k, name, M, skip)
    t = lambda v, dt: None if v is None else torch.from_numpy(np.ascontiguousarray(v).astype(dt)).cuda()  # noqa: E731
    idx, dist = ctx.knn(t(X[a], np.float32), t(X, np.float32), k, name, t(M, np.float32), t(a, np.int32))
    ctx.synchronize()
    assert_same(got, (idx.cpu().numpy().astype(np.int64), dist.cpu().numpy()), metric)
    assert_same(host_form(bliss, X[a], X[a], X, k, name, M, skip), got, (metric, "host form"))


def test_one_waypoint_is_the_song_nearest_the_midpoint(bliss, ctx, oracle):
    n, d, G = 1000, 23, 70
    X = tie_rich(np.random.default_rng(3), n, d)
    a, b, skip = ends_of(n, G)
    mid = (X[a] + (X[b] - X[a]) * (np.float32(1) / np.float32(2))).astype(np.float32)
    D = np.float32(0) + oracle.pairwise(mid, X, "euclidean", None)
    D[np.arange(G)[:, None], skip] = np.inf
    want = D.argmin(axis=1)[:, None], D.min(axis=1)[:, None]
    assert_same(device_form(ctx, X[a], X[b], X, 1, "euclidean", None, skip), want, "device form")
    assert_same(host_form(bliss, X[a], X[b], X, 1, "euclidean", None, skip), want, "host form")


# ---- (f) NaN: an error exactly when a step that runs evaluates one for an eligible candidate ----
def test_nan_only_where_a_journey_looks(bliss, ctx, oracle):
    n, d, k, G, bad = 400, 23, 12, 30, 123
    X = tie_rich(np.random.default_rng(8), n, d)
    X[bad] = np.nan
    a, b, skip = ends_of(n, G)
    skip[:, 1] = bad  # every journey skips the NaN row (and its own start)
    for B, gate in ((X[b], None), (None, None), (None, "down")):
        check(bliss, ctx, oracle, X[a], B, X, k, "euclidean", None, skip, gate, 0, what="skipped NaN row")
    # nobody skips it, but its gated column is NaN: it is gated out (the comparison fails) and never evaluated
    skip[:, 1] = -1
    for gate in ("down", "up"):
        c = check(bliss, ctx, oracle, X[a], None, X, k, "euclidean", None, skip, gate, 0, what="gated-out NaN row")
        assert c.full >= 1
    # a NaN row whose gated column is a number passes the gate of some journey: evaluated -> an error
    X[bad, 0] = -2.0  # (below every other value of the column: eligible under "down" wherever a journey stands)
    with pytest.raises(ValueError):
        restate(oracle, X[a], None, X, k, "euclidean", None, skip, "down", 0)
    for B, gate in ((None, "down"), (None, None), (X[b], None)):
        with pytest.raises(ValueError, match="NaN"):
            host_form(bliss, X[a], B, X, k, "euclidean", None, skip, gate, 0)
        with pytest.raises(bliss.BlissGpuError):
            device_form(ctx, X[a], B, X, k, "euclidean", None, skip, gate, 0)
    # ... but not of a journey whose gate keeps it out: "up" from a start above -2
    assert (X[a, 0] > -2.0).all()
    check(bliss, ctx, oracle, X[a], None, X, k, "euclidean", None, skip, "up", 0, what="NaN row below the gate")


def test_nan_gate_reference_is_an_empty_journey(bliss, ctx, oracle):
    n, d, k, G = 300, 23, 5, 4
    X = tie_rich(np.random.default_rng(8), n, d)
    A = X[:G].copy()
    A[2, 0] = np.nan  # (column 0 is gated; the row's distances would be NaN, but no candidate is eligible: none is evaluated)
    for gate in ("down", "up"):
        want = restate(oracle, A, None, X, k, "euclidean", None, None, gate, 0)
        assert (want[0][2] == -1).all() and np.isinf(want[1][2]).all() and (want[0][[0, 1, 3], 0] >= 0).all()
        assert_same(host_form(bliss, A, None, X, k, "euclidean", None, None, gate, 0), want[:2], (gate, "host form"))
        assert_same(device_form(ctx, A, None, X, k, "euclidean", None, None, gate, 0), want[:2], (gate, "device form"))


# ---- (g) the Python layer on the reference's test library ----
@pytest.fixture(scope="module")
def db(bliss, tmp_path_factory):
    """the reference's test library (setup_test_library), as tests/test_gpu_chains.py writes it"""
    path = str(tmp_path_factory.mktemp("journeys") / "bliss.db")
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


def test_library_and_playlist_journeys(bliss, db, oracle):
    L, P = bliss.library, bliss.playlist
    songs = L.load_songs(db)
    n = len(songs)
    assert n >= 5
    X = np.stack([np.asarray(s.analysis.as_vec(), np.float32) for s in songs])
    paths = [s.path for s in songs]
    DX = oracle.pairwise(X, X, "euclidean", None)
    k = 3
    # waypoints: every ordered pair of the first four songs, in one call
    pairs = [(paths[i], paths[j]) for i in range(4) for j in range(4) if i != j]
    ends = np.asarray([(paths.index(p), paths.index(q)) for p, q in pairs])
    want = restate(oracle, X[ends[:, 0]], X[ends[:, 1]], X, k, "euclidean", None, ends)[0]
    got = L.waypoint_playlists(db, pairs, k)
    assert len(got) == len(pairs)
    for g, (pair, row) in enumerate(zip(pairs, got)):
        assert [s.path for s in row] == [paths[j] for j in want[g] if j >= 0], pair
        assert not set(pair) & {s.path for s in row} and len({s.path for s in row}) == len(row)  # the end points are absent
        one = P.waypoint_playlist(songs[ends[g, 0]], songs[ends[g, 1]], songs, k)
        assert [s.path for s in one] == [s.path for s in row], pair
    # directed: every song of the library, tempo never rising
    tempo = int(bliss.AnalysisIndex.Tempo)
    skip = np.stack([np.arange(n), np.full(n, -1)], axis=1)
    for direction in ("down", "up"):
        want = restate(oracle, X, None, X, k, "euclidean", None, skip, direction, tempo, DX)[0]
        table = L.directed_playlists(db, k, bliss.AnalysisIndex.Tempo, direction)
        assert list(table) == paths
        for g, p in enumerate(paths):
            assert [s.path for s in table[p]] == [paths[j] for j in want[g] if j >= 0], (direction, p)
            assert p not in [s.path for s in table[p]]
            line = [X[g, tempo]] + [s.analysis.as_vec()[tempo] for s in table[p]]
            assert all(y <= x if direction == "down" else y >= x for x, y in zip(line, line[1:])), (direction, p)
            one = P.directed_playlist(songs[g], songs, k, bliss.AnalysisIndex.Tempo, direction)
            assert [s.path for s in one] == [s.path for s in table[p]], (direction, p)
    some = [paths[3], paths[1]]
    assert list(L.directed_playlists(db, k, tempo, "down", song_paths=some)) == some


# ---- the host form's staging: every optional argument given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("waypoint", (True, False))  # with `to` behind `from` in the staged rows, and without
@pytest.mark.parametrize("skip,dist", ((True, True), (False, False), (True, False), (False, True)))
def test_host_form_stages_like_the_device_form(bliss, ctx, skip, dist, waypoint):
    import staging_cases as sc

    def build(c, dev):
        idx, dd = dev(sc.out((c.q, c.k), np.uint32)), dev(sc.out((c.q, c.k), np.float32, dist))
        to = np.ascontiguousarray(c.Q[::-1]) if waypoint else None
        return [dev(c.Q), dev(to), c.q, dev(c.X), c.n, sc.D, 2, dev(c.M), dev(c.qskip2 if skip else None), c.k, int(waypoint), 0, 0, idx,
                dd], [idx, dd]

    sc.check(bliss, ctx, "journeys", build)
