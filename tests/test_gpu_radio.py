"""GPU tests (-m gpu) of the radio playlists (blissgpu_radio / blissgpu_radio_device: radio_ban_kernel, radio_step_kernel,
DESIGN.md 3.28): greedy song-to-song chains, or the k nearest songs, under label rules -- among the last `window` songs of a
radio at most `limit` carry any one label.  The expected values are a numpy greedy loop over the `0.0f +` distances
blissgpu_pairwise returns, with the eligibility rule written as the contract states it (count the history positions
t - window <= p < t that carry the candidate's label; position -1 is the start song).  A radio is a discrete result: every
comparison is exact (np.array_equal on indices, bit equality on distances), for the host and the device form."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
METRICS = ("euclidean", "cosine", "weights", "spd")


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


def _metric(name, d):
    if name in ("euclidean", "cosine"):
        return name, None
    rng = np.random.default_rng(7)
    if name == "weights":  # a diagonal M: the library detects it
        return "mahalanobis", np.diag(rng.integers(1, 9, d) / 4).astype(np.float32)
    A = rng.standard_normal((d, d)) * 0.3
    return "mahalanobis", (A @ A.T + 0.1 * np.eye(d)).astype(np.float32)


def library(n, d, seed=0, artists=7, albums_per_artist=4, unlabelled=0.1):
    """-> (X [n, d], labels uint32 [4, n]): rows are their artist's centre + 0.1 * noise, rounded to quarters (many equal rows,
    so many equal distances; a song's neighbours are its own artist); rule 0 is the artist (one in ten songs has none), rule 1
    the album (albums_per_artist per artist), rules 2 and 3 coarser and finer groupings for the four-rule cases."""
    rng = np.random.default_rng(seed)
    artist = rng.integers(0, artists, n)
    centre = rng.standard_normal((artists, d))
    X = (np.round((centre[artist] + 0.1 * rng.standard_normal((n, d))) * 4) / 4).astype(np.float32)
    album = artist * albums_per_artist + rng.integers(0, albums_per_artist, n)
    lab = np.stack([artist, album, artist % 3, np.arange(n) % 11]).astype(np.uint32)
    lab[0, rng.random(n) < unlabelled] = NONE
    lab[3, rng.random(n) < 0.5] = NONE
    return X, lab


def greedy(bliss, A, X, k, labels, windows, limits, from_labels=None, mode="chain", metric="euclidean", M=None, skip=None):
    """The contract in numpy over blissgpu_pairwise's distances -> (idx int64 [G, k], dist f32 [G, k], banned, ended): `banned`
    counts the steps at which a rule made a candidate ineligible, `ended` the radios that ran dry.  A NaN among the eligible
    values of a step that runs raises ValueError."""
    A, X = np.ascontiguousarray(A, np.float32), np.ascontiguousarray(X, np.float32)
    G, n = A.shape[0], X.shape[0]
    R = len(windows)
    labels = np.asarray(labels, np.uint32).reshape(R, n)
    pair = lambda Q: bliss.playlist.pairwise_distances(Q, X, metric, M)  # noqa: E731
    D0 = pair(A)
    DX = pair(X) if mode == "chain" and n <= 2048 else None
    idx, dist = np.full((G, k), -1, np.int64), np.full((G, k), np.inf, np.float32)
    banned = ended = 0
    for g in range(G):
        free = np.ones(n, bool)
        if skip is not None:
            sk = np.asarray(skip[g], np.int64)
            free[sk[sk >= 0]] = False
        hist = [[NONE if from_labels is None else int(from_labels[g][r])] for r in range(R)]  # hist[r][p + 1]: position p
        prev = None
        for t in range(k):
            if t == 0 or mode == "nearest":
                row = D0[g]
            else:
                row = DX[prev] if DX is not None else pair(X[prev:prev + 1])[0]
            row = np.float32(0) + row
            eligible = free.copy()
            for r in range(R):
                if windows[r] < 1:
                    continue
                H = np.asarray([hist[r][p + 1] for p in range(max(t - int(windows[r]), -1), t)], np.uint32)
                count = (H[:, None] == labels[r][None, :]).sum(axis=0)
                eligible &= ~((labels[r] != NONE) & (count >= limits[r]))
            banned += int((free & ~eligible).any())
            cand = np.nonzero(eligible)[0]
            if cand.size == 0:
                ended += 1
                break
            if np.isnan(row[cand]).any():
                raise ValueError("NaN distance")
            j = int(cand[np.argmin(row[cand])])  # the first minimum: the lowest index among equals
            idx[g, t], dist[g, t] = j, row[j]
            free[j] = False
            for r in range(R):
                hist[r].append(int(labels[r][j]))
            prev = j
    return idx, dist, banned, ended


def same(got, want):
    gi, gd = got
    wi, wd = want[0], want[1]
    return np.array_equal(np.asarray(gi, np.int64), wi) and np.array_equal(np.asarray(gd, np.float32).view(np.uint32), wd.view(np.uint32))


def starts(X, labels, G, R=2):
    """radio g starts at row (5 g) % n, skips it and carries its labels of the first R rules"""
    n = X.shape[0]
    rows = (5 * np.arange(G)) % n
    skip = np.stack([rows, np.full_like(rows, -1)], axis=1).astype(np.int64)
    return X[rows], labels[:R, rows].T.copy(), skip


def device_form(ctx, A, X, k, labels, windows, limits, from_labels, mode, metric, M, skip):
    import torch

    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).cuda()  # noqa: E731
    lab = None if labels is None else np.asarray(labels, np.uint32).view(np.int32)
    fl = None if from_labels is None else np.asarray(from_labels, np.uint32).view(np.int32)
    idx, dist = ctx.radio(t(A, np.float32), t(X, np.float32), k, t(lab, np.int32), windows, limits, t(fl, np.int32), mode, metric,
                          t(M, np.float32), t(skip, np.int32))
    return idx.cpu().numpy().astype(np.int64), dist.cpu().numpy()


# ---- the inputs do what they are for ----
def test_inputs_make_the_rules_bite_and_make_ties(bliss):
    n, k, G = 300, 40, 60
    X, lab = library(n, 23)
    D = np.float32(0) + bliss.playlist.pairwise_distances(X[:1], X)[0]
    assert np.unique(D).size < n - 20  # equal distances occur
    A, fl, skip = starts(X, lab, G)
    free = greedy(bliss, A, X, k, lab[:0], [], [], None, "chain", skip=skip)
    ruled = greedy(bliss, A, X, k, lab[:2], [3, 10], [1, 2], fl, "chain", skip=skip)
    assert free[2] == 0 and all(not np.array_equal(a, b) for a, b in zip(free[0], ruled[0]))  # every radio differs
    near = greedy(bliss, A, X, k, lab[:2], [k, k], [2, 1], fl, "nearest", skip=skip)
    assert near[3] == G and (near[0][:, -1] == -1).all()  # every row ends before k
    assert same(bliss.playlist.radio_order(A, X, k, lab[:2], [3, 10], [1, 2], fl, "chain", skip=skip), ruled)
    assert same(bliss.playlist.radio_order(A, X, k, lab[:2], [k, k], [2, 1], fl, "nearest", skip=skip), near)


# ---- sizes, feature counts and metrics ----
@pytest.mark.parametrize("n,G,k,d,metric", [
    (1, 1, 1, 23, "euclidean"), (1, 33, 4, 20, "cosine"), (255, 33, 40, 23, "cosine"), (256, 1, 259, 23, "weights"),
    (257, 300, 1, 20, "spd"), (257, 33, 260, 5, "euclidean"), (700, 300, 40, 23, "spd"), (700, 33, 40, 20, "weights"),
    (700, 1, 40, 5, "cosine"), (255, 300, 40, 5, "spd")])
@pytest.mark.parametrize("mode", ["chain", "nearest"])
def test_radio_sizes_and_metrics(bliss, n, G, k, d, metric, mode):
    X, lab = library(n, d, seed=n + d)
    A, fl, skip = starts(X, lab, G)
    name, M = _metric(metric, d)
    windows, limits = [3, 10], [1, 2]
    want = greedy(bliss, A, X, k, lab[:2], windows, limits, fl, mode, name, M, skip)
    assert same(bliss.playlist.radio_order(A, X, k, lab[:2], windows, limits, fl, mode, name, M, skip), want)
    if n > 1:
        assert want[2] > 0  # a rule bit


# ---- few radios: several workgroups share the candidates ----
@pytest.mark.parametrize("mode", ["chain", "nearest"])
def test_radio_shared_candidates(bliss, ctx, mode):
    n, k = 5000, 40
    X, lab = library(n, 23, seed=3, artists=40)
    A, fl, skip = starts(X, lab, 1)
    want = greedy(bliss, A, X, k, lab[:2], [5, 20], [1, 1], fl, mode, skip=skip)
    assert want[2] > 0
    assert same(bliss.playlist.radio_order(A, X, k, lab[:2], [5, 20], [1, 1], fl, mode, skip=skip), want)
    assert same(device_form(ctx, A, X, k, lab[:2], [5, 20], [1, 1], fl, mode, "euclidean", None, skip), want)


# ---- the rules ----
@pytest.mark.parametrize("mode", ["chain", "nearest"])
def test_radio_rules(bliss, mode):
    n, k, G = 300, 40, 33
    X, lab = library(n, 23, seed=1)
    A, fl, skip = starts(X, lab, G, 4)
    D = {}
    bit = 0
    for window in (0, 1, 3, k, k + 7):
        for limit in (1, 2, 5):
            for given in (True, False):
                f = fl[:, :1] if given else None
                want = greedy(bliss, A, X, k, lab[:1], [window], [limit], f, mode, skip=skip)
                assert same(bliss.playlist.radio_order(A, X, k, lab[:1], [window], [limit], f, mode, skip=skip), want), (window, limit, given)
                D[(window, limit, given)] = want
                bit += want[2] > 0
    assert bit >= 12
    assert D[(0, 1, True)][2] == 0 and D[(1, 2, False)][2] == 0  # off; a limit no window can reach
    # the start song counts: with its label given the first pick differs somewhere
    assert not np.array_equal(D[(1, 1, True)][0][:, 0], D[(1, 1, False)][0][:, 0])
    # two and four rules at once, different windows and limits
    for R, windows, limits in ((2, [k + 7, 3], [2, 1]), (4, [3, 10, 2, k], [1, 2, 1, 5]), (4, [0, k, 1, 4], [1, 1, 1, 2])):
        for f in (fl[:, :R], None):
            want = greedy(bliss, A, X, k, lab[:R], windows, limits, f, mode, skip=skip)
            assert want[2] > 0
            assert same(bliss.playlist.radio_order(A, X, k, lab[:R], windows, limits, f, mode, skip=skip), want), (windows, limits)


def test_radio_long_banned_list(bliss):
    n, k, G = 2000, 200, 3
    X, lab = library(n, 23, seed=2, artists=300, albums_per_artist=2, unlabelled=0.0)
    A, fl, skip = starts(X, lab, G)
    for mode in ("chain", "nearest"):
        want = greedy(bliss, A, X, k, lab[:1], [k], [1], fl[:, :1], mode, skip=skip)
        # every pick bans its artist: more than 64 banned labels well before the end, and no artist twice
        assert (want[0] >= 0).all() and all(np.unique(lab[0][row]).size == k for row in want[0])
        assert same(bliss.playlist.radio_order(A, X, k, lab[:1], [k], [1], fl[:, :1], mode, skip=skip), want)


# ---- the equivalences of the contract ----
def test_radio_without_rules_is_the_journey_and_the_knn(bliss):
    n, k, G = 700, 40, 33
    X, lab = library(n, 23, seed=4)
    A, fl, skip = starts(X, lab, G)
    P = bliss.playlist
    for metric in METRICS:
        name, M = _metric(metric, 23)
        journey = P.journey_order(A, X, k, None, name, M, skip)
        knn = P.nearest_order(A, X, k, name, M, skip[:, 0])
        off = [(lab[:0], [], [], None),                      # no rule
               (np.full((2, n), NONE, np.uint32), [3, k], [1, 1], fl),  # no song has a label
               (lab[:2], [0, 0], [1, 1], fl),                # every window 0
               (lab[:2], [3, k], [4, k + 1], None)]          # limit > window, the start unlabelled
        for labels, windows, limits, f in off:
            assert same(P.radio_order(A, X, k, labels, windows, limits, f, "chain", name, M, skip), journey), (metric, windows)
            assert same(P.radio_order(A, X, k, labels, windows, limits, f, "nearest", name, M, skip), knn), (metric, windows)


# ---- NaN ----
def test_radio_nan(bliss):
    n, k = 300, 10
    X, lab = library(n, 23, seed=5, unlabelled=0.0)
    bad = 17
    X[bad] = np.nan
    A, fl, skip = starts(X, lab, 4)  # rows 0, 5, 10, 15
    P = bliss.playlist
    own = np.tile(lab[:1, bad], (4, 1))  # every start carries the NaN row's artist: the artist is banned throughout
    for mode in ("chain", "nearest"):
        want = greedy(bliss, A, X, k, lab[:1], [k + 1], [1], own, mode, skip=skip)
        assert same(P.radio_order(A, X, k, lab[:1], [k + 1], [1], own, mode, skip=skip), want)
        sk = skip.copy()
        sk[:, 1] = bad  # skipped instead
        want = greedy(bliss, A, X, k, lab[:0], [], [], None, mode, skip=sk)
        assert same(P.radio_order(A, X, k, lab[:0], [], [], None, mode, skip=sk), want)
        # the same row made eligible
        with pytest.raises(ValueError, match="NaN"):
            P.radio_order(A, X, k, lab[:1], [k + 1], [1], None, mode, skip=skip)
        with pytest.raises(ValueError, match="NaN"):
            greedy(bliss, A, X, k, lab[:1], [k + 1], [1], None, mode, skip=skip)


# ---- the device form ----
@pytest.mark.parametrize("metric", METRICS)
def test_radio_device_form(bliss, ctx, metric):
    n, k, G = 700, 40, 33
    X, lab = library(n, 20, seed=6)
    A, fl, skip = starts(X, lab, G)
    name, M = _metric(metric, 20)
    for mode in ("chain", "nearest"):
        host = bliss.playlist.radio_order(A, X, k, lab[:2], [3, 10], [1, 2], fl, mode, name, M, skip)
        assert same(device_form(ctx, A, X, k, lab[:2], [3, 10], [1, 2], fl, mode, name, M, skip), host)
        assert same(device_form(ctx, A, X, k, None, [], [], None, mode, name, M, None),
                    bliss.playlist.radio_order(A, X, k, None, [], [], None, mode, name, M, None))
    import torch

    empty = ctx.radio(torch.zeros((0, 20), device="cuda"), torch.from_numpy(X).cuda(), 3)
    assert tuple(empty[0].shape) == (0, 3)
    none = ctx.radio(torch.from_numpy(A).cuda(), torch.zeros((0, 20), device="cuda"), 3)
    assert (none[0].cpu().numpy() == -1).all() and np.isinf(none[1].cpu().numpy()).all()


# ---- the song form ----
def test_radio_playlist_is_radio_order(bliss):
    n, k = 300, 25
    X, lab = library(n, 23, seed=8)
    V2 = bliss.FeaturesVersion.Version2
    name = lambda kind, v: None if v == NONE else f"{kind}{v}"  # noqa: E731
    songs = [bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist=name("artist", lab[0, i]), album=name("album", lab[1, i]),
                        duration=1.0, analysis=bliss.Analysis(X[i], V2), features_version=V2) for i in range(n)]
    P = bliss.playlist
    rules = (P.Rule("artist", 4), P.Rule("album", None, 2), P.Rule(lambda s: s.path[-6], 2))
    labels = P.rule_labels(songs, rules)
    for first in (0, 7):
        for mode in ("chain", "nearest"):
            got = P.radio_playlist(songs[first], songs, k, rules, mode)
            idx, _ = P.radio_order(X[[first]], X, k, labels, [4, k + 1, 2], [1, 2, 1], labels[:, [first]].T, mode, skip=[[first, -1]])
            assert [s.path for s in got] == [songs[j].path for j in idx[0] if j >= 0] and songs[first] not in got
            artists = [s.artist for s in got]
            assert all(a is None or a not in artists[max(0, i - 3):i] for i, a in enumerate(artists))
    default = P.radio_playlist(songs[0], songs, k)
    idx, _ = P.radio_order(X[[0]], X, k, P.rule_labels(songs, P.DEFAULT_RADIO_RULES), [5, 20], [1, 1],
                           P.rule_labels(songs, P.DEFAULT_RADIO_RULES)[:, [0]].T, skip=[[0, -1]])
    assert [s.path for s in default] == [songs[j].path for j in idx[0] if j >= 0]


# ---- the host form's staging: every optional argument given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("skip,dist,rules,from_labels", ((True, True, True, True), (False, False, False, False), (True, False, True, False),
                                                         (False, True, True, True), (True, True, False, False)))
def test_host_form_stages_like_the_device_form(bliss, ctx, skip, dist, rules, from_labels):
    import staging_cases as sc

    def build(c, dev):
        idx, dd = dev(sc.out((c.q, c.k), np.uint32)), dev(sc.out((c.q, c.k), np.float32, dist))
        lab = np.stack([np.arange(c.n) % 7, np.arange(c.n) % 11]).astype(np.uint32) if rules else None  # [rule][candidate]
        fl = np.stack([np.arange(c.q) % 7, np.arange(c.q) % 11], 1).astype(np.uint32) if rules and from_labels else None
        window, limit = np.array([2, 4], np.uint32), np.array([1, 2], np.uint32)  # (host arrays in both forms)
        return [dev(c.Q), c.q, dev(c.X), c.n, sc.D, 2, dev(c.M), dev(lab), dev(fl), 2 if rules else 0, window, limit,
                dev(c.qskip2 if skip else None), c.k, 0, idx, dd], [idx, dd]

    sc.check(bliss, ctx, "radio", build)
