"""GPU tests (-m gpu) of the k-nearest search per seed group (blissgpu_group_knn / blissgpu_group_knn_device:
group_knn_scan_kernel + group_knn_merge_kernel): closest_to_songs(&group, candidates, metric) of the reference
(src/playlist.rs:36-59, 256-270) cut after k, for many groups in one call.  The expected values come from the CPU oracle's
distance matrix (oracle.pairwise), its rows added sequentially in numpy f32 in seed order, and numpy's stable argsort --
never from the code under test.  The scores are bit-identical by contract, so the selected indices are a discrete result:
every comparison is exact (np.array_equal on indices, bit equality on distances), ties at the cut included."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def _metric(oracle, name, d):
    """-> (library metric name, M or None), as tests/test_gpu_knn.py builds them"""
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


def scores_of(Dm, off):
    """rows of the oracle's seeds x candidates matrix -> f32[G, n]: 0.0 + row + row + ..., sequentially in f32 in seed order"""
    G = off.shape[0] - 1
    out = np.zeros((G, Dm.shape[1]), np.float32)
    for g in range(G):
        acc = np.zeros(Dm.shape[1], np.float32)
        for s in range(off[g], off[g + 1]):
            acc = acc + Dm[s]
        out[g] = acc
    return out


def expected_from_scores(score, off, k, skip=None):
    """-> (idx int64[G, k], dist f32[G, k]): stable ascending order without the group's skipped columns, cut after k, padded
    with -1 / inf"""
    G, n = score.shape
    idx = np.full((G, k), -1, np.int64)
    dist = np.full((G, k), np.inf, np.float32)
    for g in range(G):
        order = np.argsort(score[g], kind="stable")
        if skip is not None:
            sk = skip[off[g]:off[g + 1]]
            order = order[~np.isin(order, sk[sk >= 0])]
        order = order[:k]
        idx[g, :order.size] = order
        dist[g, :order.size] = score[g, order]
    return idx, dist


def host_form(bliss, S, off, X, k, metric, M, skip=None):
    return bliss.playlist.nearest_to_groups((S, off), X, k, metric, M, skip)


def device_form(ctx, S, off, X, k, metric, M, skip=None):
    import torch

    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()  # noqa: E731
    idx, dist = ctx.group_knn(t(S, np.float32), off, t(X, np.float32), k, metric, t(M, np.float32), t(skip, np.int32))
    ctx.synchronize()
    return idx.cpu().numpy().astype(np.int64), dist.cpu().numpy()


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "indices", int((got[0] != want[0]).any(axis=1).sum()), "rows differ")
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (what, "distance bits")


def check_both(bliss, ctx, S, off, X, k, metric, M, skip, want, what=""):
    assert_same(host_form(bliss, S, off, X, k, metric, M, skip), want, (what, "host form"))
    assert_same(device_form(ctx, S, off, X, k, metric, M, skip), want, (what, "device form"))


def _ties_at_cut(score, off, k, skip, groups):
    """how many of `groups` have equal scores on both sides of the cut after k (among their eligible candidates)"""
    hit = 0
    for g in groups:
        s = score[g].copy()
        sk = skip[off[g]:off[g + 1]]
        s[sk[sk >= 0]] = np.inf
        s = np.sort(s, kind="stable")
        hit += int(s[k - 1] == s[k])
    return hit


# ---- (a) one seed per group is blissgpu_knn ----
def test_single_seed_groups_are_knn(bliss, ctx, oracle):
    rng = np.random.default_rng(1)
    X = tie_rich(rng, 3000, 23)
    rows = np.sort(rng.choice(3000, 300, replace=False))
    S, off = X[rows], np.arange(301, dtype=np.int64)
    score = scores_of(oracle.pairwise(S, X, "euclidean", None, n_threads=16), off)
    for k in (1, 32, 33, 1024):
        want = expected_from_scores(score, off, k, rows)
        check_both(bliss, ctx, S, off, X, k, "euclidean", None, rows, want, what=k)
        knn = bliss.playlist.nearest_order(S, X, k, "euclidean", None, rows)
        assert np.array_equal(knn[0], want[0]) and np.array_equal(knn[1], want[1])  # (values: 0.0 + x == x)


# ---- (b) multi-seed groups on a tie-rich grid ----
def _mixed_groups(rng, n):
    """120 singles, 100 groups of 2-8, 30 of 9-64, one of 300, one of 700, shuffled; members are distinct rows of the library"""
    sizes = np.concatenate([np.ones(120, np.int64), rng.integers(2, 9, 100), rng.integers(9, 65, 30), [300, 700]])
    sizes = rng.permutation(sizes)
    assert sizes.sum() <= n
    return sizes, rng.permutation(n)[:sizes.sum()]


_SHARED = {}


def _mixed_case(oracle, d, name):
    """the inputs and the expected scores of (b), computed once per (d, metric)"""
    if (d, name) not in _SHARED:
        rng = np.random.default_rng(1)
        X = tie_rich(rng, 3000, d, copies=2)  # half of the rows are copies of other rows
        sizes, members = _mixed_groups(rng, 3000)
        off = offsets_of(sizes)
        metric, M = _metric(oracle, name, d)
        score = scores_of(oracle.pairwise(X[members], X, metric, M, n_threads=16), off)
        for a in (X, members, off, score):
            a.setflags(write=False)
        _SHARED[(d, name)] = (X, sizes, members, off, metric, M, score)
    return _SHARED[(d, name)]


@pytest.mark.parametrize("d", (23, 20))
@pytest.mark.parametrize("name", METRICS)
def test_multi_seed_groups_on_a_tie_rich_grid(bliss, ctx, oracle, d, name):
    X, sizes, members, off, metric, M, score = _mixed_case(oracle, d, name)
    S = X[members]
    multi = np.flatnonzero(sizes > 1)
    ties = _ties_at_cut(score, off, 32, members, multi)
    print(f"d={d} {name}: {ties} of {multi.size} multi-seed groups tie at the cut k=32")
    assert multi.size == 132 and ties >= 20  # on the expected values alone: the tie rule at the cut is exercised
    for k in (1, 8, 32):
        want = expected_from_scores(score, off, k, members)
        check_both(bliss, ctx, S, off, X, k, metric, M, members, want, what=(d, name, k))
    again = device_form(ctx, S, off, X, 32, metric, M, members)
    assert_same(device_form(ctx, S, off, X, 32, metric, M, members), again, "the same call twice")


# ---- (c) seed order is sum order ----
def test_seed_order_is_sum_order(bliss, ctx, oracle):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((2000, 23)).astype(np.float32)
    seeds = rng.choice(2000, 8, replace=False)
    members = np.concatenate([seeds, seeds[::-1]])
    off = np.array([0, 8, 16])
    for name in ("euclidean", "cosine", "weights"):
        metric, M = _metric(oracle, name, 23)
        score = scores_of(oracle.pairwise(X[members], X, metric, M, n_threads=16), off)
        want = expected_from_scores(score, off, 32, members)
        assert not np.array_equal(want[1][0].view(np.uint32), want[1][1].view(np.uint32))  # on the oracle alone
        check_both(bliss, ctx, X[members], off, X, 32, metric, M, members, want, what=name)


# ---- (d) skip and padding ----
def test_skip_and_padding(bliss, ctx, oracle):
    rng = np.random.default_rng(4)
    X = tie_rich(rng, 3000, 23)
    small = X[:40]

    def run(S, off, Xc, k, skip, metric="euclidean", what=""):
        off = np.asarray(off, np.int64)
        score = scores_of(oracle.pairwise(S, Xc, metric, None, n_threads=16) if S.shape[0] else np.zeros((0, Xc.shape[0]), np.float32),
                          off)
        want = expected_from_scores(score, off, k, skip)
        check_both(bliss, ctx, S, off, Xc, k, metric, None, skip, want, what=what)
        return want

    # fewer eligible candidates than k: a group of 30 of the 40 rows, members skipped, k = 16 > 10
    members = np.arange(5, 35)
    w = run(small[members], [0, 30], small, 16, members, what="fewer eligible than k")
    assert (w[0][0, :10] >= 0).all() and (w[0][0, 10:] == -1).all() and np.isinf(w[1][0, 10:]).all()
    assert not np.isin(w[0][0, :10], members).any()
    # k = 1024 with n = 40, groups of several sizes, one of them empty
    members = np.array([3, 9, 9, 1, 39, 0, 17])  # (row 9 is a seed twice: its distance counts twice, one skip is enough)
    w = run(small[members], [0, 1, 3, 3, 7], small, 1024, members, metric="cosine", what="k = 1024, n = 40")
    assert [(row >= 0).sum() for row in w[0]] == [39, 39, 40, 36]
    assert np.array_equal(w[0][2], np.concatenate([np.arange(40), np.full(984, -1)])) and (w[1][2, :40] == 0.0).all()
    twice = scores_of(oracle.pairwise(small[[9]], small, "cosine", None), np.array([0, 1]))
    twice = (twice + oracle.pairwise(small[[9]], small, "cosine", None)[0])[0]
    assert np.array_equal(w[1][1, :39], np.sort(np.delete(twice, 9), kind="stable"))
    # n = 1, with and without the skip
    S = X[100:103]
    run(S, [0, 2, 3], X[:1], 3, None, what="n = 1")
    run(S, [0, 2, 3], X[:1], 3, np.array([0, -1, -1]), what="n = 1, skipped by the first group")
    run(S, [0, 2, 3], X[:1], 3, np.array([-1, 0, 0]), what="n = 1, skipped by both")
    # seeds that are not candidates: nothing to skip
    outside = tie_rich(rng, 50, 23)
    run(outside, [0, 1, 8, 50], X, 8, None, what="seeds outside the candidates")
    run(outside, [0, 1, 8, 50], X, 8, np.full(50, -1), what="a skip array of -1")
    # only empty groups
    w = run(outside[:0], [0, 0, 0], X, 5, None, what="empty groups")
    assert np.array_equal(w[0], np.tile(np.arange(5), (2, 1)))
    # the per-group form of skip in the Python layer
    got = bliss.playlist.nearest_to_groups([small[[3]], small[[9, 1]]], small, 4, skip=[[3], [1, 9]])
    want = bliss.playlist.nearest_to_groups((small[[3, 9, 1]], [0, 1, 3]), small, 4, skip=np.array([3, 9, 1]))
    assert_same(got, want, "skip per group")


# ---- (e) one big group: cut by candidates, streamed through the seed tile ----
def test_one_big_group(bliss, ctx, oracle):
    import torch

    from bliss_rs_amd import _ffi

    rng = np.random.default_rng(5)
    n, big, k = 12_000, 3000, 32
    X = tie_rich(rng, n, 23)
    sizes = np.concatenate([np.ones(25, np.int64), [big], np.ones(25, np.int64)])
    members = rng.permutation(n)[:sizes.sum()]
    off = offsets_of(sizes)
    # what the entry points will do with it on this device
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    o64, n_items, seed_tile = off.astype(np.uint64), C.c_uint64(), C.c_uint32()
    items = np.zeros((4096, 4), np.uint32)
    _ffi.check(_ffi.lib().blissgpu_group_knn_plan(o64.ctypes.data, len(sizes), n, k, n_cus, items.ctypes.data, 4096,
                                                  C.byref(n_items), None, C.byref(seed_tile)))
    items = items[:n_items.value]
    of_big = items[(items[:, 0] == 25) & (items[:, 1] == 26)]
    print(f"{n_cus} CUs: {n_items.value} items, {len(of_big)} of them for the big group; seed tile {seed_tile.value}")
    assert len(of_big) > 1 and big > seed_tile.value
    for name in ("euclidean", "cosine", "weights"):
        metric, M = _metric(oracle, name, 23)
        score = scores_of(oracle.pairwise(X[members], X, metric, M, n_threads=16), off)
        want = expected_from_scores(score, off, k, members)
        check_both(bliss, ctx, X[members], off, X, k, metric, M, members, want, what=name)


# ---- (f) NaN ----
def test_nan_scores(bliss, ctx, oracle):
    rng = np.random.default_rng(6)
    X = rng.standard_normal((2000, 23)).astype(np.float32)
    X[1234] = 0.0  # cosine distance to the zero vector is 0 / 0
    S = rng.standard_normal((12, 23)).astype(np.float32)
    off = np.array([0, 1, 4, 12])
    with pytest.raises(ValueError):
        host_form(bliss, S, off, X, 8, "cosine", None)
    with pytest.raises(bliss.BlissGpuError) as e:
        device_form(ctx, S, off, X, 8, "cosine", None)
    assert e.value.code == 5
    score = scores_of(oracle.pairwise(S, X, "euclidean", None, n_threads=16), off)
    check_both(bliss, ctx, S, off, X, 8, "euclidean", None, None, expected_from_scores(score, off, 8), what="euclidean is finite")
    # the zero row skipped by every group: its score is never looked at
    skip = np.full(12, -1)
    skip[off[:-1]] = 1234
    score = scores_of(oracle.pairwise(S, X, "cosine", None, n_threads=16), off)
    assert np.isnan(score[:, 1234]).all() and np.isnan(score).sum() == 3
    want = expected_from_scores(np.where(np.isnan(score), np.inf, score), off, 8, skip)
    check_both(bliss, ctx, S, off, X, 8, "cosine", None, skip, want, what="skipped NaN")
    skip[off[1]] = -1  # one group looks at it again
    with pytest.raises(ValueError):
        host_form(bliss, S, off, X, 8, "cosine", None, skip)
    with pytest.raises(bliss.BlissGpuError) as e:
        device_form(ctx, S, off, X, 8, "cosine", None, skip)
    assert e.value.code == 5
    # the device form reports a skip entry that is no candidate (the host form checks it on the host)
    with pytest.raises(bliss.BlissGpuError) as e:
        device_form(ctx, S, off, X, 8, "euclidean", None, np.where(skip == 1234, 2000, skip))
    assert e.value.code == 2


# ---- (g) any feature count, general M ----
@pytest.mark.parametrize("d,name", ((7, "euclidean"), (64, "euclidean"), (23, "spd")))
def test_generic_path(bliss, ctx, oracle, d, name):
    rng = np.random.default_rng(8)
    X = tie_rich(rng, 1500, d)
    sizes = rng.permutation(np.concatenate([np.ones(40, np.int64), rng.integers(2, 9, 20), [100]]))
    members = rng.permutation(1500)[:sizes.sum()]
    off = offsets_of(sizes)
    metric, M = _metric(oracle, name, d)
    score = scores_of(oracle.pairwise(X[members], X, metric, M, n_threads=16), off)
    for k in (1, 32):
        check_both(bliss, ctx, X[members], off, X, k, metric, M, members, expected_from_scores(score, off, k, members), what=(d, k))


# ---- (h) structure ----
def test_launch_count_is_independent_of_the_shape(bliss, ctx):
    import torch

    rng = np.random.default_rng(9)
    counts = []
    ctx.profile_enable(True)
    try:
        for G, n in ((50, 5000), (2000, 20_000)):
            tX = torch.from_numpy(rng.standard_normal((n, 23)).astype(np.float32)).cuda()
            sizes = rng.integers(1, 12, G)
            sizes[G // 2] = n // 4
            members = rng.permutation(n)[:sizes.sum()]
            tS = tX[torch.from_numpy(members).cuda()].contiguous()
            skip = torch.from_numpy(members.astype(np.int32)).cuda()
            ctx.synchronize()
            ctx.profile_reset()
            ctx.group_knn(tS, offsets_of(sizes), tX, 32, "euclidean", None, skip)
            ctx.synchronize()
            prof = ctx.profile()
            counts.append(sum(v[1] for name, v in prof.items() if name.startswith("group_knn_")))
            assert counts[-1] >= 1
            for name, v in prof.items():
                assert not (v[1] and (name.startswith("pairwise") or name.startswith("set_distance") or name.startswith("radix_"))), prof
            print(f"G={G} n={n}: group_knn launches {counts[-1]}")
    finally:
        ctx.profile_enable(False)
    assert counts[0] == counts[1], counts


# ---- (i) the library ----
def test_library_group_playlists_is_one_call(bliss, oracle, tmp_path, monkeypatch):
    from bliss_rs_amd import _ffi

    rng = np.random.default_rng(10)
    n, k = 2000, 10
    X = tie_rich(rng, n, 23)
    V2 = bliss.FeaturesVersion.Version2
    album = [None if i % 17 == 5 else f"album {int(a):03d}" for i, a in enumerate(rng.integers(0, 150, n))]
    songs = [bliss.Song(path=f"/music/{i:05d}.flac", title=f"t{i}", artist="a", album=album[i], duration=1.0,
                        analysis=bliss.Analysis(X[i], V2), features_version=V2) for i in range(n)]
    db = str(tmp_path / "bliss.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs)
    lib = _ffi.lib()
    calls = []
    real = lib.blissgpu_group_knn

    def counted(*a):
        calls.append(1)
        return real(*a)

    monkeypatch.setattr(lib, "blissgpu_group_knn", counted)
    table = bliss.library.group_playlists(db, k, by="album")
    assert len(calls) == 1 and len(table) == len({a for a in album if a is not None}) == 150
    saved = {"saved": [songs[i].path for i in (7, 1500, 7, 33)]}
    custom = bliss.library.group_playlists(db, k, groups=saved)
    assert len(calls) == 2
    monkeypatch.undo()

    def contract(paths):
        return bliss.library.playlist_from_custom(db, paths, bliss.playlist.euclidean_distance, bliss.playlist.closest_to_songs,
                                                  deduplicate=False)[len(paths):][:k]

    def oracle_scores(rows):
        return scores_of(oracle.pairwise(X[rows], X, "euclidean", None, n_threads=16), np.array([0, len(rows)]))[0]

    path_row = {s.path: i for i, s in enumerate(songs)}
    for key in list(table)[::10]:
        rows = [i for i in range(n) if album[i] == key]
        assert [p for p, _ in table[key]] == [s.path for s in contract([songs[i].path for i in rows])], key
        score = oracle_scores(rows)
        assert [np.float32(v) for _, v in table[key]] == [score[path_row[p]] for p, _ in table[key]], key
    assert [p for p, _ in custom["saved"]] == [s.path for s in contract(saved["saved"])]
    score = oracle_scores([7, 1500, 7, 33])
    assert [np.float32(v) for _, v in custom["saved"]] == [score[path_row[p]] for p, _ in custom["saved"]]
    # the Song form
    groups = [[songs[i] for i in range(n) if album[i] == key] for key in list(table)[:3]]
    got = bliss.playlist.group_playlists(groups, songs, k)
    assert [[s.path for s in row] for row in got] == [[p for p, _ in table[key]] for key in list(table)[:3]]


# ---- the host form's staging: every optional argument given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("skip,dist", ((True, True), (False, False), (True, False), (False, True)))
def test_host_form_stages_like_the_device_form(bliss, ctx, skip, dist):
    import staging_cases as sc

    def build(c, dev):
        idx, dd = dev(sc.out((c.G, c.k), np.uint32)), dev(sc.out((c.G, c.k), np.float32, dist))
        return [dev(c.S), c.off, c.G, dev(c.X), c.n, sc.D, 2, dev(c.M), dev(c.skip if skip else None), c.k, idx, dd], [idx, dd]

    sc.check(bliss, ctx, "group_knn", build)
