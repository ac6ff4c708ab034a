"""GPU tests (-m gpu) of k-medoids on the device (blissgpu_pam_scan / blissgpu_kmedoids: pam_scan_kernel, pam_fold_kernel,
pam_pick_kernel and the state's helpers around the k-nearest core).  Expected values never come from the code under test: the
reference is the contract of include/blissgpu.h written out in numpy (tests/test_pam_host.py) applied to
playlist.pairwise_distances(X, X) from the device, which other tests hold to the oracle.  Every comparison is exact -- indices,
counts and the bits of every f32 and f64; no tolerance appears anywhere."""
import numpy as np
import pytest

from test_pam_host import (NanDistance, bits64, contract_kmedoids, contract_scan, contract_state, order_sensitive_input,
                           planted_labelled, same_result)
from test_ward_host import bits, equal_input, twice_input

pytestmark = pytest.mark.gpu
ERR_OOM, ERR_NAN = 4, 5
F32 = np.float32


@pytest.fixture(scope="module")
def bliss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import bliss_rs_amd

    return bliss_rs_amd


def random_input(n, d=23, seed=5):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(F32)


def builder_of(P, metric, M=None):
    return {"euclidean": P.euclidean_distance, "cosine": P.cosine_distance}.get(metric) or P.MahalanobisBuilder(M)


def pd_matrix(d, seed, diagonal=False):
    rng = np.random.default_rng(seed)
    if diagonal:
        return np.diag(rng.uniform(0.2, 3.0, d)).astype(F32)
    A = rng.standard_normal((d, d))
    return (A @ A.T / d + 0.5 * np.eye(d)).astype(F32)


_MATRICES = {}


def all_pairs(bliss, X, metric="euclidean", M=None):
    """the device's all-pairs matrix of X, computed once per input"""
    key = (X.tobytes(), X.shape, metric, None if M is None else M.tobytes())
    if key not in _MATRICES:
        _MATRICES[key] = bliss.playlist.pairwise_distances(X, X, metric, M)
    return _MATRICES[key]


def a_state(Dm, k, seed):
    """the state of k songs drawn at random"""
    med = np.sort(np.random.default_rng(seed).choice(Dm.shape[0], k, replace=False))
    return contract_state(Dm, med)[:3]


def same_scan(got, want):
    btot, best, arg, A, B = got
    return (np.array_equal(bits64(btot), bits64(want[0])) and np.array_equal(bits64(best), bits64(want[1])) and np.array_equal(arg, want[2])
            and np.array_equal(bits64(A), bits64(want[3])) and np.array_equal(bits64(B), bits64(want[4])))


def check_scan(bliss, X, k, metric="euclidean", M=None, rows=None, state=None, what="", want=None):
    """the device's scan against the contract over the device's all-pairs matrix; -> the contract's result"""
    P = bliss.playlist
    Dm = all_pairs(bliss, X, metric, M)
    near, d1, d2 = a_state(Dm, k, seed=k + X.shape[0]) if state is None else state
    want = contract_scan(Dm, near, d1, d2, k, rows) if want is None else want
    got = P.pam_scan(X, near, d1, d2, k, builder_of(P, metric, M), rows, return_sums=True)
    assert got[0].dtype == np.float64 and got[2].dtype == np.int64 and got[3].shape == (len(want[0]), k)
    assert same_scan(got, want), (what, [int(np.count_nonzero(bits64(g) != bits64(w))) for g, w in zip(got, want)])
    short = P.pam_scan(X, near, d1, d2, k, builder_of(P, metric, M), rows)  # A and B NULL
    assert len(short) == 3 and same_scan(short + got[3:], want), what
    return want


def check_clustering(bliss, X, k, metric="euclidean", M=None, init=None, max_swaps=None, what=""):
    P = bliss.playlist
    want = contract_kmedoids(all_pairs(bliss, X, metric, M), k, init, max_swaps)
    res = P.kmedoids(X, k, builder_of(P, metric, M), "build" if init is None else init, max_swaps)
    assert res.medoids.dtype == np.int64 and res.dist.dtype == F32 and res.td_trace.dtype == np.float64
    assert same_result(res, want), (what, res.medoids, want[0], res.n_swaps, want[5], res.td_trace[:3], want[4][:3])
    return want


# ---- one scan ----
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 255, 256, 257, 1000])
def test_scan_sizes_at_23_features(bliss, n):
    X = random_input(n, 23, seed=100 + n)
    rng = np.random.default_rng(n)
    for k in (1, 2, 7):
        if k > n:
            continue
        want = check_scan(bliss, X, k, what=(n, k))
        check_scan(bliss, X, k, rows=rng.integers(0, n, n // 2 + 3), what=(n, k, "a subset with repeats"))
        perm = rng.permutation(n)
        shuffled = check_scan(bliss, X, k, rows=perm, what=(n, k, "shuffled"))
        assert all(np.array_equal(bits64(s), bits64(w[perm])) for s, w in zip(shuffled[:2], want[:2]))  # no bit depends on the order of rows


def test_3000_songs_and_several_column_groups(bliss, monkeypatch):
    """more than one tile per slot and per column group; no bit depends on the groups"""
    X = planted_labelled(3000)[0]
    for k in (7, 40):
        want = check_scan(bliss, X, k, what=(3000, k))
        for groups in (1, 3, k + 5):
            monkeypatch.setenv("BLISSGPU_PAM_COL_GROUPS", str(groups))
            check_scan(bliss, X, k, what=(3000, k, groups), want=want)
        monkeypatch.delenv("BLISSGPU_PAM_COL_GROUPS")
    assert np.isfinite(want[1]).all()


def test_row_slabs_change_no_byte(bliss):
    """a workspace limit that forces several slabs of candidates"""
    P = bliss.playlist
    ctx = bliss.Context.default()
    limit = ctx.workspace_limit()
    X = planted_labelled(3000)[0]  # the O(n) part is about 0.1 MB; A and B of a candidate at k = 64 are 1 KiB: slabs of 768 candidates
    try:
        ctx.set_workspace_limit(1 << 20)
        check_scan(bliss, X, 64, what="slabs")
        check_scan(bliss, X, 64, rows=np.random.default_rng(3).integers(0, 3000, 2500), what="slabs of a subset")
        init = np.random.default_rng(4).choice(2000, 64, replace=False)
        check_clustering(bliss, X[:2000], 64, init=init, max_swaps=1, what="slabs in the rounds")
        # ... and there WERE several: a scan launch per slab
        near, d1, d2 = a_state(all_pairs(bliss, X), 64, seed=64 + 3000)
        ctx.profile_enable(True)
        ctx.profile_reset()
        P.pam_scan(X, near, d1, d2, 64, return_sums=True)
        assert ctx.profile()["pam_scan_kernel"][1] == 4 and ctx.profile()["kmeans_hist_kernel"][1] == 1  # 3000 candidates in slabs of 768
        ctx.profile_reset()
        res = P.kmedoids(X[:2000], 64, init=init, max_swaps=1)
        assert ctx.profile()["pam_scan_kernel"][1] == 3 * (res.n_swaps + 1) and res.n_swaps == 1
    finally:
        ctx.profile_enable(False)
        ctx.set_workspace_limit(limit)


@pytest.mark.parametrize("d", [20, 7, 1, 64])
def test_other_feature_counts(bliss, d):
    for n, k in ((257, 3), (700, 7)):
        X = random_input(n, d, seed=d + n)
        check_scan(bliss, X, k, what=(d, n))
        check_clustering(bliss, X, k, max_swaps=2, what=(d, n))


def test_the_order_of_the_sums(bliss):
    """the hand-made d = 1 input on which ascending and descending sums differ (tests/test_pam_host.py)"""
    x, near, d1b, k = order_sensitive_input()
    zero, inf = np.zeros(302, F32), np.full(302, np.inf, F32)
    want = check_scan(bliss, x, k, state=(near, zero, inf), what="A")
    assert want[3][0, 0] == 2.0 ** 60
    check_scan(bliss, x, k, state=(near, d1b, inf), what="B")


@pytest.mark.parametrize("d,n", [(23, 300), (20, 257), (7, 300)])
def test_mahalanobis(bliss, d, n):
    X = random_input(n, d, seed=40 + d)
    for diagonal in (True, False):
        M = pd_matrix(d, d, diagonal)
        check_scan(bliss, X, 5, "mahalanobis", M, what=(d, diagonal))
        check_clustering(bliss, X, 5, "mahalanobis", M, max_swaps=2, what=(d, diagonal))


@pytest.mark.parametrize("d,n", [(23, 300), (20, 257), (5, 300)])
def test_cosine(bliss, d, n):
    X = random_input(n, d, seed=60 + d)
    want = check_scan(bliss, X, 5, "cosine", what=d)
    assert np.isfinite(want[0]).all()
    check_clustering(bliss, X, 5, "cosine", what=d)
    check_clustering(bliss, X, 5, "cosine", init=[9, 3, 200, 77, 0], what=(d, "init"))


# ---- the clustering ----
def every_song_a_medoid_at_1000(bliss, X):
    """k = n = 1000.  The replay of BUILD is 1000 scans of up to 1000 slots in numpy, about half a minute: too slow for this suite
    (k = n = 257 goes through it in full).  From a given start the replay is one state and one scan and is held bit for bit: no
    candidate is left, over four wavefronts and several tiles.  BUILD's 1000 slots run on the device and are held to what k = n
    leaves no freedom in: every song a medoid once, its own slot's only song at distance 0 (the rows are distinct), TD = 0,
    converged without a swap."""
    P = bliss.playlist
    n = X.shape[0]
    start = np.random.default_rng(n).permutation(n)
    want = check_clustering(bliss, X, n, init=start, what=(n, n, "init"))
    assert want[5] == 0 and want[6] and np.array_equal(want[0], start)
    check_clustering(bliss, X, n, init=start, max_swaps=0, what=(n, n, "init", 0))
    res = P.kmedoids(X, n)
    assert sorted(res.medoids.tolist()) == list(range(n)) and np.array_equal(res.medoids[res.labels], np.arange(n))
    assert not bits(res.dist).any() and (res.sizes == 1).all() and res.n_swaps == 0 and res.converged
    assert res.td == 0.0 and res.td_trace.tolist() == [0.0]
    Dm = all_pairs(bliss, X)
    assert res.medoids[0] == int(np.argmin(np.cumsum(Dm.astype(np.float64), axis=1)[:, -1]))  # slot 0: the smallest sequential sum


@pytest.mark.parametrize("n", [2, 3, 5, 257, 1000])
def test_clustering_sizes_at_23_features(bliss, n):
    X = planted_labelled(1000)[0][:n]
    rng = np.random.default_rng(n)
    for k in (1, 2, 8, n):
        if k > n:
            continue
        if k == n == 1000:
            every_song_a_medoid_at_1000(bliss, X)
            continue
        want = check_clustering(bliss, X, k, what=(n, k, "build"))
        assert want[6]
        init = rng.choice(n, k, replace=False)
        check_clustering(bliss, X, k, init=init, what=(n, k, "init"))
        for max_swaps in (0, 1):
            check_clustering(bliss, X, k, init=init, max_swaps=max_swaps, what=(n, k, "init", max_swaps))
            if not (k == n and n > 5):  # (k = n = 257: BUILD's replay is 257 scans, done once above)
                check_clustering(bliss, X, k, max_swaps=max_swaps, what=(n, k, "build", max_swaps))


def test_planted_songs_under_cosine_and_euclidean(bliss):
    X, lab = planted_labelled(600)
    for metric in ("euclidean", "cosine"):
        want = check_clustering(bliss, X, 8, metric, what=metric)
        assert want[6] and all(len(set(lab[want[1] == c].tolist())) == 1 for c in range(8))


def test_ties_empty_slots_and_zero_second_distances(bliss):
    same = equal_input(300)
    want = check_clustering(bliss, same, 4, what="equal rows")
    assert want[0].tolist() == [0, 1, 2, 3] and want[3].tolist() == [300, 0, 0, 0] and want[5] == 0  # every song goes to slot 0
    check_scan(bliss, same, 4, state=contract_state(all_pairs(bliss, same), [0, 1, 2, 3])[:3], what="equal rows, empty slots")
    check_clustering(bliss, same, 4, init=[7, 290, 3, 100], what="equal rows, init")
    twice = twice_input(200)
    want = check_clustering(bliss, twice, 6, what="twice")
    check_clustering(bliss, twice, 100, max_swaps=3, what="twice, k = n / 2")
    Dm = all_pairs(bliss, twice)
    twin = int(np.flatnonzero((Dm[0] == 0) & (np.arange(200) != 0))[0])
    state = contract_state(Dm, [0, twin, 5])
    assert (state[2] == 0).any()  # a song and its twin are both medoids: d2 = 0 for them
    check_scan(bliss, twice, 3, state=state[:3], what="d2 = 0")
    check_clustering(bliss, twice, 3, init=[0, twin, 5], what="twins as the start")


def test_nan_distances(bliss):
    P = bliss.playlist
    X = random_input(300, 23, seed=9)
    near, d1, d2 = a_state(all_pairs(bliss, X), 3, seed=1)
    bad = X.copy()
    bad[77, 5] = np.nan
    zero = X.copy()
    zero[131] = 0.0
    for Y, builder in ((bad, P.euclidean_distance), (bad, P.cosine_distance), (zero, P.cosine_distance)):
        with pytest.raises(bliss.BlissGpuError) as e:
            P.pam_scan(Y, near, d1, d2, 3, builder)
        assert e.value.code == ERR_NAN
        with pytest.raises(bliss.BlissGpuError) as e:
            P.pam_scan(Y, near, d1, d2, 3, builder, rows=[77, 131])
        assert e.value.code == ERR_NAN
        for init in ("build", [1, 2, 3]):
            with pytest.raises(bliss.BlissGpuError) as e:
                P.kmedoids(Y, 3, builder, init)
            assert e.value.code == ERR_NAN
    with pytest.raises(NanDistance):
        contract_scan(all_pairs(bliss, zero, "cosine"), near, d1, d2, 3)
    # a zero row is no trouble under euclidean, and the context is as good as before
    check_clustering(bliss, zero, 3, what="a zero row, euclidean")
    check_clustering(bliss, X, 3, "cosine", what="afterwards")


def test_workspace_limit(bliss):
    P = bliss.playlist
    ctx = bliss.Context.default()
    limit = ctx.workspace_limit()
    ctx.profile_enable(True)
    try:
        ctx.set_workspace_limit(1 << 20)  # (the smallest limit) 60 000 songs: near, d1, d2 and the sort alone are 2.9 MB
        ctx.profile_reset()
        X = np.zeros((60000, 23), F32)
        with pytest.raises(bliss.BlissGpuError) as e:
            P.kmedoids(X, 4)
        assert e.value.code == ERR_OOM
        with pytest.raises(bliss.BlissGpuError) as e:
            P.pam_scan(X, np.zeros(60000, int), np.zeros(60000, F32), np.ones(60000, F32), 4, rows=[1, 2, 3])
        assert e.value.code == ERR_OOM
        assert not [name for name, v in ctx.profile().items() if v[1]]  # nothing was launched
    finally:
        ctx.set_workspace_limit(limit)
        ctx.profile_enable(False)
    check_clustering(bliss, random_input(500, 23, seed=52), 5, what="afterwards")


# ---- the rest ----
def test_two_runs_give_the_same_bytes_and_a_stale_workspace_does_not_show(bliss):
    P = bliss.playlist
    big, small = planted_labelled(2000)[0], random_input(130, 23, seed=71)
    runs = [P.kmedoids(X, k) for X, k in ((big, 12), (small, 3), (big, 12), (small, 3))]
    for a, b in ((runs[0], runs[2]), (runs[1], runs[3])):
        assert all(getattr(a, f).tobytes() == getattr(b, f).tobytes() for f in ("medoids", "labels", "dist", "sizes", "td_trace"))
        assert (a.n_swaps, a.converged) == (b.n_swaps, b.converged)
    assert same_result(runs[3], contract_kmedoids(all_pairs(bliss, small), 3))
    near, d1, d2 = a_state(all_pairs(bliss, small), 3, seed=2)
    scans = [P.pam_scan(X, *s, 3, return_sums=True) for X, s in ((big, a_state(all_pairs(bliss, big), 3, seed=2)), (small, (near, d1, d2)))] * 2
    assert all(x.tobytes() == y.tobytes() for x, y in zip(scans[1], scans[3]))


def test_launches(bliss):
    """a round is the medoids' rows, the k-nearest core, the state, TD, the sort of the slots, one scan, one fold, one pick"""
    P = bliss.playlist
    ctx = bliss.Context.default()
    X = planted_labelled(1000)[0]
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        res = P.kmedoids(X, 8, init=np.arange(8))
        prof = {name: v[1] for name, v in ctx.profile().items() if v[1]}
        print(prof)
        rounds = res.n_swaps + 1
        assert res.n_swaps >= 2 and res.converged
        assert prof == {name: rounds for name in ("pam_gather_kernel", "knn_scan_kernel", "knn_merge_kernel", "pam_state_kernel", "pam_td_kernel",
                                                   "kmeans_hist_kernel", "kmeans_scan_tiles_kernel", "kmeans_scan_add_kernel",
                                                   "kmeans_scatter_kernel", "pam_scan_kernel", "pam_fold_kernel", "pam_pick_kernel")}
        ctx.profile_reset()
        res = P.kmedoids(X, 8, max_swaps=0)  # BUILD: a scan per slot (the first without a state), then the one round
        prof = {name: v[1] for name, v in ctx.profile().items() if v[1]}
        assert prof["pam_scan_kernel"] == 9 and prof["pam_pick_kernel"] == 9 and prof["knn_scan_kernel"] == 8 and "pairwise_kernel" not in prof
    finally:
        ctx.profile_enable(False)


def test_library_medoid_songs(bliss, tmp_path):
    P, Lb = bliss.playlist, bliss.library
    rng = np.random.default_rng(23)
    V2 = bliss.FeaturesVersion.Version2
    songs = []
    for i in range(60):
        x = (3.0 * (i % 4) + 0.3 * rng.standard_normal(23)).astype(F32)
        songs.append(bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist="a", album="b", disc_number=1, track_number=i,
                                duration=1.0, genre=["a", "b"][i % 2], analysis=bliss.Analysis(x, V2), features_version=V2))
    db = str(tmp_path / "bliss.db")
    Lb.create_schema(db)
    Lb.store_songs(db, songs)
    X = np.stack([s.analysis.as_vec() for s in songs]).astype(F32)
    for builder, metric in ((P.euclidean_distance, "euclidean"), (P.cosine_distance, "cosine")):
        reps, clusters, res = Lb.medoid_songs(db, 4, builder, return_medoids=True)
        want = contract_kmedoids(all_pairs(bliss, X, metric), 4)
        assert same_result(res, want), metric
        assert [s.path for s in reps] == [songs[int(i)].path for i in want[0]]
        assert sum(len(c) for c in clusters) == 60
        if metric == "euclidean":
            assert sorted(len(c) for c in clusters) == [15] * 4 and all(len({int(s.path[7:10]) % 4 for s in c}) == 1 for c in clusters)
        for rep, cluster, c in zip(reps, clusters, range(4)):
            assert cluster[0].path == rep.path
            assert np.array_equal(bits(res.dist[[int(s.path[7:10]) for s in cluster]]), bits(np.sort(want[2][want[1] == c])))
    sub, lists = Lb.medoid_songs(db, 2, where=("genre", "a"))
    assert len(sub) == 2 and sorted(len(c) for c in lists) == [15, 15]
