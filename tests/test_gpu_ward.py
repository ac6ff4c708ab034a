"""GPU tests (-m gpu) of Ward clustering on the device (blissgpu_ward / blissgpu_ward_nearest: ward_scan_kernel, ward_join_kernel,
the merge of ward_merge.hpp between the rounds).  Expected values never come from the code under test: the reference is the
contract of include/blissgpu.h written out in numpy (tests/test_ward_host.py) applied to playlist.pairwise_distances(C, C) from
the device, which other tests hold to the oracle -- for the tree one all-pairs call per round, on the contract's own centroids.
Every comparison is exact -- indices, sizes, rounds and the bits of the costs; no tolerance appears anywhere."""
import numpy as np
import pytest

from test_ward_host import bits, contract_nearest, contract_tree, equal_input, grid_input, planted, same_tree, twice_input

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_OOM = 2, 4


@pytest.fixture(scope="module")
def bliss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import bliss_rs_amd

    return bliss_rs_amd


def random_input(n, d=23, seed=5):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def builder_of(P, metric, M):
    return P.euclidean_distance if metric == "euclidean" else P.MahalanobisBuilder(M)


def pd_matrix(d, seed, diagonal=False):
    rng = np.random.default_rng(seed)
    if diagonal:
        return np.diag(rng.uniform(0.2, 3.0, d)).astype(np.float32)
    A = rng.standard_normal((d, d))
    return (A @ A.T / d + 0.5 * np.eye(d)).astype(np.float32)


def as_tuple(t):
    return (t.u, t.v, t.cost, t.size, t.round, t.rounds)


def check_nearest(bliss, C, sizes=None, metric="euclidean", M=None, what=""):
    P = bliss.playlist
    want = contract_nearest(P.pairwise_distances(C, C, metric, M), sizes)
    nn, cost = P.ward_nearest(C, sizes, builder_of(P, metric, M))
    assert nn.dtype == np.int64 and cost.dtype == np.float32
    assert np.array_equal(nn, want[0]) and np.array_equal(bits(cost), bits(want[1])), (what, np.flatnonzero(nn != want[0])[:10])
    return want


def check_tree(bliss, X, metric="euclidean", M=None, what=""):
    """the device's tree against the contract's rounds over the device's all-pairs matrices; -> the tree"""
    P = bliss.playlist
    want = contract_tree(X, dist_fn=lambda C: P.pairwise_distances(C, C, metric, M))
    t = P.ward_tree(X, builder_of(P, metric, M))
    assert t.n == X.shape[0] and t.u.dtype == np.int64 and t.cost.dtype == np.float32
    assert same_tree(as_tuple(t), want), (what, t.rounds, want[5])
    return want


# ---- one scan ----
@pytest.mark.parametrize("m", [2, 3, 63, 64, 65, 255, 256, 257, 1000])
def test_nearest_sizes_at_23_features(bliss, m):
    C = random_input(m, 23, seed=100 + m)
    check_nearest(bliss, C, what=m)
    check_nearest(bliss, C, np.random.default_rng(m).integers(1, 5001, m), what=(m, "sizes"))


def test_nearest_on_ties(bliss):
    """equal costs everywhere: the XOR of the positions decides"""
    nn, _ = check_nearest(bliss, grid_input(600), what="grid")
    nn, _ = check_nearest(bliss, equal_input(300), what="equal")
    assert np.array_equal(nn, np.arange(300) ^ 1)  # every position's partner under XOR: the neighbour in the lowest bit
    nn, cost = check_nearest(bliss, twice_input(200), what="twice")
    assert not bits(cost).any() and np.array_equal(nn[nn], np.arange(200))
    sizes = np.random.default_rng(9).integers(1, 4, 600)  # few distinct weights on few distinct distances
    check_nearest(bliss, grid_input(600), sizes, what="grid with sizes")


# ---- the tree ----
@pytest.mark.parametrize("n", [2, 3, 5, 257, 1000])
def test_tree_sizes_at_23_features(bliss, n):
    want = check_tree(bliss, planted(1000)[:n], what=n)
    assert len(want[0]) == n - 1 and want[3][-1] == n


def test_3000_songs_and_several_column_groups(bliss, monkeypatch):
    """more than one tile per column group, and with the column groups forced, more than one partial winner per position; with
    the filter in front of the root forced on, forced off, and chosen by the size of the scan (off at this size)"""
    P = bliss.playlist
    X = planted(3000)
    want = check_tree(bliss, X, what=3000)
    assert want[5] == 41
    for filter_on in ("1", "0"):
        monkeypatch.setenv("BLISSGPU_WARD_FILTER", filter_on)
        for groups in (1, 3, 7, 47):
            monkeypatch.setenv("BLISSGPU_WARD_COL_GROUPS", str(groups))
            assert same_tree(as_tuple(P.ward_tree(X)), want), (filter_on, groups)
        monkeypatch.delenv("BLISSGPU_WARD_COL_GROUPS")
        assert same_tree(as_tuple(P.ward_tree(X)), want), filter_on


def test_the_filter_changes_no_bit(bliss, monkeypatch):
    """every family of test inputs with the filter forced on (by default it is off below 12 288 positions): sizes, ties, the
    other feature count, both Mahalanobis forms, NaN and inf"""
    monkeypatch.setenv("BLISSGPU_WARD_FILTER", "1")
    for m in (2, 65, 257, 1000):
        C = random_input(m, 23, seed=100 + m)
        check_nearest(bliss, C, what=m)
        check_nearest(bliss, C, np.random.default_rng(m).integers(1, 5001, m), what=(m, "sizes"))
    check_nearest(bliss, grid_input(600), np.random.default_rng(9).integers(1, 4, 600), what="grid with sizes")
    for X in (planted(1000), equal_input(300), twice_input(200), grid_input(600), random_input(700, 20, seed=32)):
        check_tree(bliss, X, what="filter")
    for d in (20, 23):
        X = random_input(300, d, seed=40)
        check_tree(bliss, X, "mahalanobis", pd_matrix(d, 41, diagonal=True), what=("diagonal", d))
        check_tree(bliss, X, "mahalanobis", pd_matrix(d, 42), what=("full", d))
    bad = X.copy()
    bad[123, 4] = np.nan
    rc, err, out = _raw_tree_call(bad)
    assert rc == ERR_INVALID and b"NaN" in err and all((a == 7).all() for a in out)
    M = np.eye(23, dtype=np.float32)
    M[3, 3] = -50.0
    rc, err, out = _raw_tree_call(X, 2, M)
    assert rc == ERR_INVALID and b"NaN" in err and all((a == 7).all() for a in out)
    far = X.copy()
    far[9, 2] = np.inf
    assert np.isinf(check_tree(bliss, far, what="inf")[2][-1])


def test_other_feature_counts(bliss):
    check_tree(bliss, random_input(1000, 20, seed=32), what="d=20")
    check_nearest(bliss, random_input(700, 20, seed=33), np.random.default_rng(3).integers(1, 5001, 700), what="d=20")
    for d in (7, 64):  # the generic form
        check_tree(bliss, random_input(500, d, seed=33 + d), what=d)
        check_nearest(bliss, random_input(300, d, seed=34 + d), np.random.default_rng(d).integers(1, 5001, 300), what=d)


@pytest.mark.parametrize("d,n", [(23, 1000), (20, 300), (7, 300)])
def test_mahalanobis(bliss, d, n):
    X = random_input(n, d, seed=40 + d)
    check_tree(bliss, X, "mahalanobis", pd_matrix(d, 41, diagonal=True), what=("diagonal", d))
    check_tree(bliss, X, "mahalanobis", pd_matrix(d, 42), what=("full", d))


def test_ties_in_the_tree(bliss):
    want = check_tree(bliss, equal_input(300), what="equal")
    assert want[5] == 9 and not bits(want[2]).any()  # 9 rounds on the device too (check_tree compares the rounds)
    want = check_tree(bliss, twice_input(200), what="twice")
    assert int((bits(want[2]) == 0).sum()) == 100
    check_tree(bliss, grid_input(600), what="grid")


# ---- what is refused ----
def _raw_tree_call(X, metric=0, M=None):
    from bliss_rs_amd import _ffi

    n, d = X.shape
    out = [np.full(n, 7, np.uint32), np.full(n, 7, np.uint32), np.full(n, 7.0, np.float32), np.full(n, 7, np.uint32), np.full(n, 7, np.uint32)]
    rounds = np.full(1, 7, np.uint32)
    rc = _ffi.lib().blissgpu_ward(X.ctypes.data, n, d, metric, None if M is None else M.ctypes.data, *(a.ctypes.data for a in out),
                                  rounds.ctypes.data)
    return rc, _ffi.lib().blissgpu_last_error(), out


def _raw_nearest_call(X, metric=0, M=None):
    from bliss_rs_amd import _ffi

    n, d = X.shape
    out = [np.full(n, 7, np.uint32), np.full(n, 7.0, np.float32)]
    rc = _ffi.lib().blissgpu_ward_nearest(X.ctypes.data, None, n, d, metric, None if M is None else M.ctypes.data, *(a.ctypes.data for a in out))
    return rc, _ffi.lib().blissgpu_last_error(), out


def test_nan_costs_are_invalid_and_nothing_is_written(bliss):
    X = random_input(300, 23, seed=50)
    bad = X.copy()
    bad[123, 4] = np.nan
    M = np.eye(23, dtype=np.float32)
    M[3, 3] = -50.0  # not positive semi-definite: negative sums
    assert (np.isnan(bliss.playlist.pairwise_distances(X, X, "mahalanobis", M))).any()
    for call in (_raw_tree_call, _raw_nearest_call):
        rc, err, out = call(bad)
        assert rc == ERR_INVALID and b"NaN" in err and all((a == 7).all() for a in out)
        rc, err, out = call(X, 2, M)
        assert rc == ERR_INVALID and b"NaN" in err and all((a == 7).all() for a in out)
        generic = random_input(100, 7, seed=51)  # the generic form too
        generic[5, 2] = np.nan
        rc, err, out = call(generic)
        assert rc == ERR_INVALID and b"NaN" in err and all((a == 7).all() for a in out)
    with pytest.raises(bliss.BlissGpuError) as e:
        bliss.playlist.ward_tree(bad)
    assert e.value.code == ERR_INVALID
    # an infinite feature is inf - inf against itself only, which is no pair: that song joins last, at cost +inf
    far = X.copy()
    far[9, 2] = np.inf
    want = check_tree(bliss, far, what="inf")
    assert np.isinf(want[2][-1]) and np.isfinite(want[2][:-1]).all() and 9 in (want[0][-1], want[1][-1])
    # the context is as good as before
    check_tree(bliss, X, what="afterwards")


def test_workspace_limit(bliss):
    ctx = bliss.Context.default()
    limit = ctx.workspace_limit()
    ctx.profile_enable(True)
    try:
        ctx.set_workspace_limit(1 << 20)  # (the smallest limit) 60 000 songs: the rows alone are 5.5 MB, the best keys 480 KB
        ctx.profile_reset()
        with pytest.raises(bliss.BlissGpuError) as e:
            bliss.playlist.ward_tree(np.zeros((60000, 23), np.float32))
        assert e.value.code == ERR_OOM
        with pytest.raises(bliss.BlissGpuError) as e:
            bliss.playlist.ward_nearest(np.zeros((200000, 23), np.float32))
        assert e.value.code == ERR_OOM
        assert not [name for name, v in ctx.profile().items() if v[1]]  # nothing was launched
    finally:
        ctx.set_workspace_limit(limit)
        ctx.profile_enable(False)
    check_tree(bliss, random_input(500, 23, seed=52), what="afterwards")


# ---- the rest ----
def test_two_runs_give_the_same_bytes_and_a_stale_workspace_does_not_show(bliss):
    P = bliss.playlist
    big, small = grid_input(2000, seed=70), random_input(130, 23, seed=71)
    first = [as_tuple(P.ward_tree(X)) for X in (big, small, big, small)]
    for a, b in ((first[0], first[2]), (first[1], first[3])):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:5], b[:5])) and a[5] == b[5]


def test_launches(bliss):
    P = bliss.playlist
    ctx = bliss.Context.default()
    X = random_input(1000, 23, seed=72)
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        t = P.ward_tree(X)
        prof = {name: v[1] for name, v in ctx.profile().items() if v[1]}
        print(prof)
        assert prof == {"ward_scan_kernel": t.rounds, "ward_join_kernel": t.rounds - 1}  # no distance matrix is formed
    finally:
        ctx.profile_enable(False)


def test_choose_k_tree(bliss):
    P = bliss.playlist
    X = planted(300)
    t = P.ward_tree(X)
    sel = P.choose_k_tree(X, t, range(2, 13))
    assert sel.ks == list(range(2, 13)) and len(sel.scores) == 11
    for k, score in zip(sel.ks, sel.scores):
        assert score == P.silhouette(X, t.cut(k)).score, k
    assert sel.best_k == P._best_k(sel.ks, sel.scores) and np.array_equal(sel.clustering, t.cut(sel.best_k))
    assert sel.best_k == 8  # the planted clusters


def test_library_ward_clusters(bliss, tmp_path):
    Lb = bliss.library
    rng = np.random.default_rng(23)
    V2 = bliss.FeaturesVersion.Version2
    songs = []
    for i in range(60):
        x = (3.0 * (i % 4) + 0.3 * rng.standard_normal(23)).astype(np.float32)
        songs.append(bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist="a", album="b", disc_number=1, track_number=i,
                                duration=1.0, genre=["a", "b"][i % 2], analysis=bliss.Analysis(x, V2), features_version=V2))
    db = str(tmp_path / "bliss.db")
    Lb.create_schema(db)
    Lb.store_songs(db, songs)
    paths, tree = Lb.ward_tree(db)
    assert paths == [s.path for s in songs] and tree.n == 60
    X = np.stack([s.analysis.as_vec() for s in songs]).astype(np.float32)
    assert same_tree(as_tuple(tree), contract_tree(X, dist_fn=lambda C: bliss.playlist.pairwise_distances(C, C)))
    for kw in (dict(k=4), dict(k=9, min_cluster_size=6), dict(cost=float(tree.cost[40]))):
        lists, loose = Lb.ward_clusters(db, **kw)
        labels = tree.cut(**kw)
        assert [[s.path for s in c] for c in lists] == [[paths[i] for i in np.flatnonzero(labels == c)] for c in range(labels.max() + 1)]
        assert [s.path for s in loose] == [paths[i] for i in np.flatnonzero(labels < 0)]
    lists, _ = Lb.ward_clusters(db, k=4)
    assert [len(c) for c in lists] == [15] * 4 and all(len({int(s.path[7:10]) % 4 for s in c}) == 1 for c in lists)
    sub, _ = Lb.ward_clusters(db, k=2, where=("genre", "a"))
    assert sorted(len(c) for c in sub) == [15, 15]
