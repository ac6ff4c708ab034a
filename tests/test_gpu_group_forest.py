"""GPU tests (-m gpu) of the isolation-forest playlists for every group in one call (blissgpu_group_forest_knn and its device form:
group_forest_scan_kernel + group_knn_merge_kernel; playlist.forest_nearest_to_groups, playlist.forest_group_playlists,
library.forest_playlists).

Every expected value comes from the single-forest path that was there before, never from the new call: row g must equal, bit for
bit in idx and in the uint32 view of score, the first k of np.argsort(Forest(S_g, opts).scores(X), kind="stable") with the
group's skipped candidates removed, then padding (-1 / +inf); a group with min(sample_size, seeds) < 2 carries the status flag
and a row of padding.  One case is checked without any scoring code of the project (test_forest_host.forest_walk).

The option set (40, 256, None, 22) cannot be built at d = 20 (extension_level <= d - 1 is the contract): there it runs with
extension_level 19, the fullest normal d = 20 has."""
import sqlite3

import numpy as np
import pytest

from test_forest_host import fixture_songs, forest_walk, score_of
from test_gpu_forest import candidates, ulps

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 5, 16, 40, 1, 0, 300]
SMALL = [2, 3, 5, 16, 1, 0]
# (n_trees, sample_size, max_tree_depth, extension_level), the group sizes of the call
OPTIONS = [
    ((64, 16, None, 10), SIZES),
    ((500, 16, None, 10), SMALL),   # ~65 LDS chunks per group: the chunk loop and its barriers
    ((40, 256, None, 22), SIZES),   # the 300-seed group's trees exceed the node buffer: walked from global memory beside staged groups
    ((64, 16, None, 0), SIZES),
    ((60, 128, 3, 10), SIZES),
    ((60, 16, 9, 3), SIZES),
]
SEED = 11


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


def _options(bliss, opts, d):
    return bliss.playlist.ForestOptions(opts[0], opts[1], opts[2], min(opts[3], d - 1), seed=SEED)


_CASES = {}


def case(bliss, opts, sizes, d, n):
    """(seed groups, offsets, X, per-group full scores from the single-forest path or None, skip per seed row) -- computed once"""
    key = (opts, tuple(sizes), d, n)
    if key not in _CASES:
        rng = np.random.default_rng([opts[0], opts[1], opts[3], d, n])
        groups = [rng.uniform(-1, 1, (s, d)).astype(np.float32) for s in sizes]
        S = np.concatenate(groups)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        X = candidates(rng, S, n, d).reshape(n, d)
        fo = _options(bliss, opts, d)
        scores = []
        for g in groups:
            if min(g.shape[0], fo.sample_size) < 2:
                scores.append(None)
                continue
            f = bliss.playlist.Forest(g, fo)
            scores.append(f.scores(X))
            f.close()
        # skip: every other seed row names a candidate; the largest group names the candidates 0, 1, 2, ... (all of them when
        # n <= its size: an all-padding row)
        skip = np.full(S.shape[0], -1, np.int64)
        if n:
            for gi, s in enumerate(sizes):
                a = int(off[gi])
                if s == max(sizes):
                    m = min(s, n)
                    skip[a:a + m] = np.arange(m)
                else:
                    skip[a:a + s:2] = (np.arange(a, a + s, 2) * 7) % n
        for a in (S, X, skip):
            a.setflags(write=False)
        _CASES[key] = (groups, off, S, X, scores, skip)
    return _CASES[key]


def expected(scores, off, skip, n, k):
    """rows from the single-forest scores: stable argsort, skipped candidates removed, cut after k, padded"""
    G = len(scores)
    idx, sc, status = np.full((G, k), -1, np.int64), np.full((G, k), np.inf, np.float32), np.zeros(G, np.int32)
    for g, s in enumerate(scores):
        if s is None:
            status[g] = 1
            continue
        order = np.argsort(s, kind="stable")
        if skip is not None:
            gone = skip[off[g]:off[g + 1]]
            order = order[~np.isin(order, gone[gone >= 0])]
        order = order[:k]
        idx[g, :order.shape[0]] = order
        sc[g, :order.shape[0]] = s[order]
    return idx, sc, status


def same(got_idx, got_score, want_idx, want_score, what):
    assert np.array_equal(np.asarray(got_idx, np.int64), want_idx), what
    assert np.array_equal(np.asarray(got_score, np.float32).view(np.uint32), want_score.view(np.uint32)), what


def device_call(bliss, ctx, S, off, X, k, fo, skip, host_seeds=True):
    import torch

    dS, dX = torch.from_numpy(np.array(S)).cuda(), torch.from_numpy(np.array(X)).cuda()
    dskip = None if skip is None else torch.from_numpy(skip.astype(np.int32)).cuda()
    idx, score, status = ctx.group_forest_knn(dS, off, dX, k, fo, skip=dskip, seeds_host=S if host_seeds else None)
    return idx.cpu().numpy().astype(np.int64), score.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("d", [23, 20])
@pytest.mark.parametrize("oi", range(len(OPTIONS)), ids=lambda i: "-".join(str(v) for v in OPTIONS[i][0]))
def test_rows_equal_the_single_forest_path(bliss, ctx, oi, d):
    opts, sizes = OPTIONS[oi]
    n = 1000
    groups, off, S, X, scores, skip = case(bliss, opts, sizes, d, n)
    fo = _options(bliss, opts, d)
    assert any(s is not None for s in scores)                                   # a group with psi >= 2
    assert any(s is not None and np.unique(s).size < n for s in scores)         # ties: the stable order is exercised
    for k in (1, 5, 64, 1024):
        for sk in (None, skip):
            want_idx, want_sc, want_status = expected(scores, off, sk, n, k)
            idx, sc = bliss.playlist.forest_nearest_to_groups(groups, X, k, fo, skip=sk, few_seeds="empty")   # host pointers
            same(idx, sc, want_idx, want_sc, (opts, d, k, "host form"))
            if k in (5, 1024):
                di, ds, dstat = device_call(bliss, ctx, S, off, X, k, fo, sk, host_seeds=(k == 5))             # device pointers
                same(di, ds, want_idx, want_sc, (opts, d, k, "device form"))
                assert np.array_equal(dstat, want_status)
    # k = 1024 is above n: padded rows; the flagged groups are all padding
    assert (want_idx[:, n:] == -1).all() and np.isinf(want_sc[:, n:]).all()
    for g, s in enumerate(scores):
        if s is None:
            assert (idx[g] == -1).all() and np.isinf(sc[g]).all()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000])
def test_candidate_counts_and_skip(bliss, ctx, n):
    opts, sizes = OPTIONS[0]
    for d in (23, 20):
        groups, off, S, X, scores, skip = case(bliss, opts, sizes, d, n)
        fo = _options(bliss, opts, d)
        assert any(s is not None for s in scores)
        if n >= 64:
            assert any(s is not None and np.unique(s).size < n for s in scores)
        for k in (1, 5, 64, 1024):
            for sk in (None, skip):
                want_idx, want_sc, want_status = expected(scores, off, sk, n, k)
                idx, sc = bliss.playlist.forest_nearest_to_groups(groups, X, k, fo, skip=sk, few_seeds="empty")
                same(idx, sc, want_idx, want_sc, (n, d, k, "host form"))
                if sk is not None and 0 < n <= max(sizes):  # every candidate of the largest group is skipped: all padding
                    assert (idx[len(sizes) - 1] == -1).all() and np.isinf(sc[len(sizes) - 1]).all()
        di, ds, dstat = device_call(bliss, ctx, S, off, X, 5, fo, skip, host_seeds=False)
        want_idx, want_sc, want_status = expected(scores, off, skip, n, 5)
        same(di, ds, want_idx, want_sc, (n, d, "device form"))
        assert np.array_equal(dstat, want_status)


def test_every_batch_split_gives_the_same_bits(bliss, ctx):
    from test_group_forest_host import _plan

    opts, sizes = OPTIONS[0]
    d, n, k = 23, 1000, 64
    groups, off, S, X, scores, skip = case(bliss, opts, sizes, d, n)
    fo = _options(bliss, opts, d)
    want_idx, want_sc, want_status = expected(scores, off, skip, n, k)
    assert _plan(off, (opts[0], opts[1], 0, opts[3]), 3100)[1] == 3 and _plan(off, (opts[0], opts[1], 0, opts[3]), 1)[1] == len(sizes)
    runs = []
    try:
        for budget, batches in ((1, len(sizes)), (3100, 3), (0, 1), (0, 1)):
            ctx.set_option("forest_group_nodes", budget)
            di, ds, dstat = device_call(bliss, ctx, S, off, X, k, fo, skip)
            assert ctx.group_forest_stats()[2] == batches
            runs.append((di, ds, dstat))
    finally:
        ctx.set_option("forest_group_nodes", 0)
    for di, ds, dstat in runs:
        same(di, ds, want_idx, want_sc, "batch split")
        assert np.array_equal(dstat, want_status)
    hi, hs = bliss.playlist.forest_nearest_to_groups(groups, X, k, fo, skip=skip, few_seeds="empty")
    same(hi, hs, runs[0][0], runs[0][1], "host form == device form")
    # the scan kernel ran, merged by the k-nearest merge kernel: two launches per batch
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.set_option("forest_group_nodes", 3100)
    try:
        device_call(bliss, ctx, S, off, X, k, fo, skip)
        prof = ctx.profile()
    finally:
        ctx.set_option("forest_group_nodes", 0)
        ctx.profile_enable(False)
    assert prof["group_forest_scan_kernel"][1] == 3 and prof["group_knn_merge_kernel"][1] == 3 and len(prof) == 2


def test_a_skip_list_beyond_the_lds_copy_and_a_bad_entry(bliss, ctx):
    """A group of 1100 seeds skips 1100 candidates: the entries past the 1024 the kernel holds in LDS come from global memory.
    A skip entry >= n in a group that has a forest is BLISSGPU_ERR_INVALID in the device form."""
    import torch

    from bliss_rs_amd import _ffi

    d, n, k = 23, 1300, 64
    rng = np.random.default_rng(9)
    groups = [rng.uniform(-1, 1, (1100, d)).astype(np.float32), rng.uniform(-1, 1, (3, d)).astype(np.float32)]
    S, off = np.concatenate(groups), np.asarray([0, 1100, 1103], np.int64)
    X = candidates(rng, S, n, d)
    fo = bliss.playlist.ForestOptions(8, 16, None, 3, seed=SEED)
    scores = []
    for g in groups:
        f = bliss.playlist.Forest(g, fo)
        scores.append(f.scores(X))
        f.close()
    skip = np.full(1103, -1, np.int64)
    skip[:1100] = rng.permutation(1100)  # every candidate below 1100 is skipped, in no particular order
    skip[1101] = 1299
    want_idx, want_sc, _ = expected(scores, off, skip, n, k)
    assert set(want_idx[0].tolist()) <= set(range(1100, 1300)) and 1299 not in want_idx[1]
    idx, sc = bliss.playlist.forest_nearest_to_groups(groups, X, k, fo, skip=skip)
    same(idx, sc, want_idx, want_sc, "host form")
    di, ds, _ = device_call(bliss, ctx, S, off, X, k, fo, skip)
    same(di, ds, want_idx, want_sc, "device form")
    bad = skip.copy()
    bad[1050] = n  # no candidate, and not the "none" value either
    with pytest.raises(_ffi.BlissGpuError) as e:
        device_call(bliss, ctx, S, off, X, k, fo, bad)
    assert e.value.code == _ffi.ERR_INVALID and "skip" in str(e.value)
    with pytest.raises(ValueError):
        bliss.playlist.forest_nearest_to_groups(groups, X, k, fo, skip=bad)
    assert torch.cuda.is_available()


def test_against_the_numpy_walk_of_the_exported_forest(bliss):
    """No scoring code of the project: the u64 sums come from the numpy walker, the scores from numpy's exp2."""
    opts, d, n = (64, 16, None, 10), 23, 257
    rng = np.random.default_rng(77)
    S = rng.uniform(-1, 1, (16, d)).astype(np.float32)
    X = candidates(rng, S, n, d)
    fo = _options(bliss, opts, d)
    f = bliss.playlist.Forest(S, fo)
    ps, _, _ = forest_walk(f.export(), X)
    want = score_of(ps, f.n_trees, f.psi).astype(np.float32)
    f.close()
    idx, sc = bliss.playlist.forest_nearest_to_groups([S], X, 1024, fo)
    assert (idx[0, :n] >= 0).all() and (idx[0, n:] == -1).all() and np.isinf(sc[0, n:]).all()
    got = np.empty(n, np.float32)
    got[idx[0, :n]] = sc[0, :n]
    assert sorted(idx[0, :n].tolist()) == list(range(n))
    assert ulps(got, want).max() <= 1
    assert np.unique(got).size < n
    assert np.array_equal(idx[0, :n], np.argsort(got, kind="stable"))


def _library(bliss, tmp_path, rows, names):
    from bliss_rs_amd import library

    songs = [bliss.Song(path=f"/music/{names[i]}-{i}", album=names[i], analysis=bliss.Analysis(row, bliss.FeaturesVersion.LATEST),
                        features_version=bliss.FeaturesVersion.LATEST) for i, row in enumerate(rows)]
    db = str(tmp_path / "bliss.db")
    library.create_schema(db)
    conn = sqlite3.connect(db)
    for s in songs:
        library.store_song(conn, s)
    conn.commit()
    conn.close()
    return songs, db


def test_python_forms_on_the_fixture_albums(bliss, tmp_path):
    from bliss_rs_amd import library

    P = bliss.playlist
    opts, groups = fixture_songs()
    rows = np.concatenate([groups["mozart_piano_19"], groups["kind_of_blue"], groups["mozart_piano_23"]])
    names = ["m19"] * 3 + ["blue"] * 5 + ["m23"] * 3
    songs, db = _library(bliss, tmp_path, rows, names)
    fo = P.ForestOptions(opts["n_trees"], opts["sample_size"], opts["max_tree_depth"], opts["extension_level"], seed=4)
    k = 8
    albums = {a: [s for s in songs if s.album == a] for a in ("m19", "blue", "m23")}
    want = {a: [s.path for s in library.playlist_from_custom(db, [m.path for m in members], fo, P.closest_to_songs,
                                                             deduplicate=False)[len(members):][:k]]
            for a, members in albums.items()}
    got = library.forest_playlists(db, k, fo)
    assert list(got) == ["m19", "blue", "m23"]
    for a in albums:
        assert [p for p, _ in got[a]] == want[a], a
        assert all(np.isfinite(v) and 0.0 < v < 1.0 for _, v in got[a])
    assert {p.split("/")[-1].split("-")[0] for p in want["m19"][-5:]} == {"blue"}
    assert {p.split("/")[-1].split("-")[0] for p, _ in got["m19"][-5:]} == {"blue"}
    lists = P.forest_group_playlists(list(albums.values()), songs, k, fo)
    assert [[s.path for s in row] for row in lists] == [want[a] for a in albums]
    # the quick-start form: a path, k, the options
    assert library.forest_playlists(db, 3, fo)["blue"] == got["blue"][:3]
    # a saved playlist as the seed set
    saved = library.forest_playlists(db, k, fo, groups={"mine": [songs[0].path, songs[9].path]})
    ref = library.playlist_from_custom(db, [songs[0].path, songs[9].path], fo, P.closest_to_songs, deduplicate=False)[2:][:k]
    assert [p for p, _ in saved["mine"]] == [s.path for s in ref]


def test_few_seeds_euclidean_answers_the_singles(bliss, tmp_path):
    from bliss_rs_amd import library

    P = bliss.playlist
    opts, groups = fixture_songs()
    rows = np.concatenate([groups["mozart_piano_19"], groups["kind_of_blue"], groups["mozart_piano_23"]])
    names = ["m19"] * 3 + ["blue"] * 5 + ["m23"] * 2 + ["single"]
    songs, db = _library(bliss, tmp_path, rows, names)
    fo = P.ForestOptions(200, opts["sample_size"], opts["max_tree_depth"], opts["extension_level"], seed=4)
    k = 6
    with pytest.raises(ValueError):
        library.forest_playlists(db, k, fo)
    empty = library.forest_playlists(db, k, fo, few_seeds="empty")
    mixed = library.forest_playlists(db, k, fo, few_seeds="euclidean")
    euclid = library.group_playlists(db, k, metric_builder=P.euclidean_distance)
    assert empty["single"] == [] and mixed["single"] == euclid["single"] and len(mixed["single"]) == k
    for a in ("m19", "blue", "m23"):
        assert mixed[a] == empty[a] and len(empty[a]) == k
    by_album = [[s for s in songs if s.album == a] for a in ("m19", "blue", "m23", "single")]
    lists = P.forest_group_playlists(by_album, songs, k, fo, few_seeds="euclidean")
    assert [[s.path for s in row] for row in lists] == [[p for p, _ in mixed[a]] for a in ("m19", "blue", "m23", "single")]
    assert P.forest_group_playlists(by_album, songs, k, fo, few_seeds="empty")[3] == []


# ---- the host form's staging: every optional argument given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("skip,score,status", ((True, True, True), (False, False, False), (True, False, False), (False, True, True)))
def test_host_form_stages_like_the_device_form(bliss, ctx, skip, score, status):
    import staging_cases as sc

    def build(c, dev):
        idx, sco = dev(sc.out((c.G, c.k), np.uint32)), dev(sc.out((c.G, c.k), np.float32, score))
        st = dev(sc.out((c.G,), np.int32, status))
        seeds = [c.S] if dev(c.S) is c.S else [None, c.S]  # the device form with the seed rows on the host, as the host form has them
        return seeds + [c.off, c.G, dev(c.X), c.n, sc.D, 20, 8, 0, 1, 5, dev(c.skip if skip else None), c.k, idx, sco, st], [idx, sco, st]

    sc.check(bliss, ctx, "group_forest_knn", build)
