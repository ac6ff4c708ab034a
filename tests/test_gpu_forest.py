"""GPU tests (-m gpu) of the extended isolation forest metric (blissgpu_forest_score / _closest_to_songs and their device forms:
forest_walk_kernel + forest_finish_kernel).  Every expected value comes from the numpy walk of the EXPORTED forest
(test_forest_host.forest_walk), never from the code under test:
    path_sum   exactly (np.array_equal on u64)
    score      within 1 f32 ulp of exp2(-(path_sum / 2^24 / T) / c(psi)) evaluated in numpy f64 (same expression of the same
               integer: only the last rounding can differ), and within 2 f32 ulp of the unquantised definition (the
               quantisation of the leaves moves the score by at most a third of an ulp)
    order      numpy's stable argsort of the scores the same call returned."""
import sqlite3

import numpy as np
import pytest

from test_forest_host import c_of, fixture_songs, forest_walk, score_of

pytestmark = pytest.mark.gpu


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


def ulps(a, b):
    """distance in f32 ulps between two arrays of positive finite floats"""
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def candidates(rng, S, n, d):
    """n rows: uniform in [-1, 1], the seed rows themselves, rows copied from other rows, rows on a grid of eighths, rows holding
    NaN, +-inf, +-0"""
    X = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    k = min(S.shape[0], n // 8)
    X[:k] = S[:k]
    if n >= 64:
        q = n // 10
        X[q:2 * q] = X[rng.integers(2 * q, n, q)]                   # copies: equal scores, ties in the order
        X[2 * q:3 * q] = np.round(X[2 * q:3 * q] * 8) / 8
        sp = rng.integers(3 * q, 4 * q, (5, max(1, q // 8)))
        for rows, v in zip(sp, (np.nan, np.inf, -np.inf, 0.0, -0.0)):
            X[rows, rng.integers(0, d, rows.shape[0])] = v
        X[4 * q, :] = np.nan
        X[4 * q + 1, :] = np.inf
        X[4 * q + 2, :] = -0.0
    return X


# (n_seeds, sample_size, n_trees, extension_level, d, max_tree_depth)
CONFIGS = [
    (3, 200, 1000, 10, 23, None),
    (16, 16, 500, 0, 23, None),
    (1000, 256, 100, 22, 23, None),      # trees too large for the LDS node buffer: walked from global memory
    (500, 256, 100, 5, 20, None),
    (400, 128, 60, 10, 23, 4),           # depth below ceil(log2 psi) = 7
    (40, 16, 200, 3, 23, 9),             # depth above ceil(log2 psi) = 4
]


def _forest(bliss, cfg, seed=11):
    n_seeds, sample_size, n_trees, ext, d, depth = cfg
    rng = np.random.default_rng(list(cfg[:5]))
    S = rng.uniform(-1, 1, (n_seeds, d)).astype(np.float32)
    f = bliss.playlist.Forest(S, bliss.playlist.ForestOptions(n_trees, sample_size, depth, ext, seed=seed))
    return rng, S, f


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(str(v) for v in c))
def test_path_sums_are_exact_and_scores_within_one_ulp(bliss, ctx, cfg):
    import torch

    rng, S, f = _forest(bliss, cfg)
    n, T, psi = 100003, f.n_trees, f.psi
    X = candidates(rng, S, n, f.d)
    want_ps, want_depth, _ = forest_walk(f.export(), X)
    score, ps = f.scores(X, return_path_sum=True)                                     # host pointers
    assert np.array_equal(ps, want_ps)
    assert np.isfinite(score).all()
    u1 = ulps(score, score_of(want_ps, T, psi).astype(np.float32))
    u2 = ulps(score, np.exp2(-(want_depth / T) / c_of(psi)).astype(np.float32))
    print(cfg, "max ulp vs quantised", u1.max(), "vs unquantised definition", u2.max())
    assert u1.max() <= 1
    assert u2.max() <= 2
    # device pointers, twice, and every launch option: bit-identical
    dX = torch.from_numpy(X).cuda()
    runs = []
    for split, walk in ((0, 0), (0, 0), (1, 0), (3, 0), (7, 1), (0, 1), (65535, 0)):
        ctx.set_option("forest_split", split)
        ctx.set_option("forest_walk", walk)
        s, p = ctx.forest_scores(f, dX, return_path_sum=True)
        ctx.synchronize()
        runs.append((s.cpu().numpy(), p.cpu().numpy().view(np.uint64)))
    ctx.set_option("forest_split", 0)
    ctx.set_option("forest_walk", 0)
    for s, p in runs:
        assert np.array_equal(p, want_ps)
        assert np.array_equal(s.view(np.uint32), score.view(np.uint32))
    # the order: numpy's stable argsort of the scores the same call returned, on the tie-rich candidates
    order, sc = f.closest_to_songs_order(X)
    assert np.array_equal(sc.view(np.uint32), score.view(np.uint32))
    assert np.unique(sc).shape[0] < n
    assert np.array_equal(order.astype(np.int64), np.argsort(sc, kind="stable"))
    o2, s2 = ctx.forest_closest_to_songs(f, dX, return_scores=True)
    ctx.synchronize()
    assert np.array_equal(o2.cpu().numpy(), order.astype(np.int64))
    assert np.array_equal(s2.cpu().numpy().view(np.uint32), score.view(np.uint32))
    f.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_small_candidate_counts(bliss, ctx, n):
    import torch

    for cfg in (CONFIGS[1], CONFIGS[2]):
        rng, S, f = _forest(bliss, cfg)
        X = candidates(rng, S, n, f.d)
        score, ps = f.scores(X, return_path_sum=True)
        order, sc = f.closest_to_songs_order(X)
        assert score.shape == (n,) and order.shape == (n,)
        if n:
            want_ps, _, _ = forest_walk(f.export(), X)
            assert np.array_equal(ps, want_ps)
            assert ulps(score, score_of(want_ps, f.n_trees, f.psi).astype(np.float32)).max() <= 1
            assert np.array_equal(sc.view(np.uint32), score.view(np.uint32))
            assert np.array_equal(order.astype(np.int64), np.argsort(sc, kind="stable"))
        dX = torch.from_numpy(X.reshape(n, f.d)).cuda()
        s, p = ctx.forest_scores(f, dX, return_path_sum=True)
        o = ctx.forest_closest_to_songs(f, dX)
        ctx.synchronize()
        assert np.array_equal(s.cpu().numpy().view(np.uint32), score.view(np.uint32))
        assert np.array_equal(p.cpu().numpy().view(np.uint64), ps)
        assert np.array_equal(o.cpu().numpy(), order.astype(np.int64))
        f.close()


def test_unused_dimensions_never_reach_the_sum(bliss):
    """extension_level 0: a node looks at one dimension.  A NaN / inf in a dimension NO node of the forest uses must not move
    any path sum (a dense-normal kernel would multiply it by zero and get NaN)."""
    rng = np.random.default_rng(3)
    S = rng.uniform(-1, 1, (16, 23)).astype(np.float32)
    f = bliss.playlist.Forest(S, bliss.playlist.ForestOptions(1, 8, None, 0, seed=5))
    ex = f.export()
    unused = np.nonzero((ex["normal"] != 0).sum(0) == 0)[0]
    assert unused.shape[0] >= 1
    X = rng.uniform(-1, 1, (1000, 23)).astype(np.float32)
    _, base = f.scores(X, return_path_sum=True)
    for v in (np.nan, np.inf, -np.inf):
        Y = X.copy()
        Y[:, unused] = v
        _, ps = f.scores(Y, return_path_sum=True)
        assert np.array_equal(ps, base)
    f.close()


def test_reference_property_kind_of_blue_comes_last(bliss):
    """The reference's test_forest_options (src/playlist.rs:1262-1660): trained on Mozart's concerto 19, the five "Kind of Blue"
    tracks are the last five of closest_to_songs.  The reference's own options (1 000 trees); all eight seeds must hold."""
    opts, groups = fixture_songs()
    seeds = groups["mozart_piano_19"]
    songs = np.concatenate([groups["mozart_piano_19"], groups["kind_of_blue"], groups["mozart_piano_23"]])
    blue = set(range(3, 8))
    for seed in range(8):
        fo = bliss.playlist.ForestOptions(opts["n_trees"], opts["sample_size"], opts["max_tree_depth"], opts["extension_level"],
                                          seed=seed)
        order, score = bliss.playlist.closest_to_songs_order(seeds, songs, fo)
        gap = score[3:8].min() - np.delete(score, np.arange(3, 8)).max()
        print("seed", seed, "gap", gap, "scores", np.round(score, 3))
        assert set(order[-5:].tolist()) == blue, (seed, order, score)


@pytest.mark.parametrize("psi,trees,ext", [(256, 100, 22), (256, 100, 0), (16, 300, 10)])
def test_planted_outliers_score_above_every_inlier(bliss, psi, trees, ext):
    rng = np.random.default_rng(2024)
    c0 = rng.uniform(-0.5, 0.5, 23)
    c1 = c0 + 0.4 * rng.choice([-1.0, 1.0], 23)
    S = (c0 + 0.03 * rng.standard_normal((2000, 23))).astype(np.float32)
    near = (c0 + 0.03 * rng.standard_normal((50000, 23))).astype(np.float32)
    far = (c1 + 0.03 * rng.standard_normal((50000, 23))).astype(np.float32)
    score = bliss.playlist.forest_scores(S, np.concatenate([near, far]), bliss.playlist.ForestOptions(trees, psi, None, ext, seed=1))
    print((psi, trees, ext), "highest near", score[:50000].max(), "lowest far", score[50000:].min())
    assert score[:50000].max() < score[50000:].min()


def test_through_python_songs_and_library(bliss, tmp_path):
    from bliss_rs_amd import library

    P = bliss.playlist
    opts, groups = fixture_songs()
    rows = np.concatenate([groups["mozart_piano_19"], groups["kind_of_blue"], groups["mozart_piano_23"]])
    names = ["m19"] * 3 + ["blue"] * 5 + ["m23"] * 3
    songs = [bliss.Song(path=f"/music/{names[i]}-{i}", album=names[i], analysis=bliss.Analysis(row, bliss.FeaturesVersion.LATEST),
                        features_version=bliss.FeaturesVersion.LATEST) for i, row in enumerate(rows)]
    fo = P.ForestOptions(opts["n_trees"], opts["sample_size"], opts["max_tree_depth"], opts["extension_level"], seed=4)
    order, _ = P.closest_to_songs_order(rows[:3], rows, fo)
    got = P.closest_to_songs(songs[:3], songs, fo)
    assert [s.path for s in got] == [songs[i].path for i in order]
    assert {s.album for s in got[-5:]} == {"blue"}
    assert np.array_equal(P.forest_scores(rows[:3], rows, fo), P.forest_closest_to_songs_order(rows[:3], rows, fo)[1])
    db = str(tmp_path / "bliss.db")
    library.create_schema(db)
    conn = sqlite3.connect(db)
    for s in songs:
        library.store_song(conn, s)
    conn.commit()
    conn.close()
    seeds = [s.path for s in songs[:3]]
    pl = library.playlist_from_custom(db, seeds, fo, P.closest_to_songs, deduplicate=False)
    assert [s.path for s in pl[:3]] == seeds
    assert len(pl) == 11 and {s.album for s in pl[-5:]} == {"blue"}
    # the pool is the library without the seeds, in the order of the index form
    pool_order, _ = P.closest_to_songs_order(rows[:3], rows[3:], fo)
    assert [s.path for s in pl[3:]] == [songs[3 + i].path for i in pool_order]
    # a forest playlist is deduplicated with the euclidean rule afterwards
    assert len(P.dedup_playlist(pl)) <= len(pl)


# ---- the host forms' staging: every optional argument given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("family,extra", (("forest_score", True), ("forest_score", False), ("forest_closest_to_songs", True),
                                          ("forest_closest_to_songs", False)))
def test_host_form_stages_like_the_device_form(bliss, ctx, family, extra):
    import ctypes as C

    import staging_cases as sc
    from bliss_rs_amd import _ffi

    lib, forests = _ffi.lib(), []

    def build(c, dev):
        f = C.c_void_p()
        assert lib.blissgpu_forest_build(c.S.ctypes.data_as(C.c_void_p), len(c.S), sc.D, 20, 8, 0, 1, 5, C.byref(f)) == 0
        forests.append(f)
        if family == "forest_score":
            score, sums = dev(sc.out((c.n,), np.float32)), dev(sc.out((c.n,), np.uint64, extra))
            return [f, dev(c.X), c.n, score, sums], [score, sums]
        order, score = dev(sc.out((c.n,), np.uint32)), dev(sc.out((c.n,), np.float32, extra))
        return [f, dev(c.X), c.n, order, score], [order, score]

    try:
        sc.check(bliss, ctx, family, build, lists=family != "forest_score")
    finally:
        for f in forests:
            lib.blissgpu_forest_destroy(f)
