"""GPU tests (-m gpu) of k-means on the device (blissgpu_kmeans / blissgpu_kmeans_device: kmeans_assign_kernel, the counting
sort of the labels, segment_mean_kernel, kmeans_select_kernel).  Expected values never come from the code under test: the
reference is the contract's loop written below -- distances from oracle.pairwise(X, C, metric, M), the first minimum of every
row (equal rounded distances go to the lower centre), the sequential f32 mean of test_gpu_albums.py (seq_mean) over a cluster's
rows in ascending order, an empty cluster keeps its centre -- on that file's mixed_grid data, where the order of an f32 sum
shows in its bits.  Every comparison is exact: labels, sizes, n_iter and converged by equality, dist and centroids by bits."""
import numpy as np
import pytest

from test_gpu_albums import bits, mixed_grid, seq_mean

pytestmark = pytest.mark.gpu

MAX_ITER = 100


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
    """-> (library metric name, M or None): euclidean, the diagonal feature weights, a full SPD matrix (as tests/test_gpu_knn.py)"""
    if name == "euclidean":
        return name, None
    if name == "weights":
        return "mahalanobis", oracle.feature_weights(2 if d == 23 else 1) if d in (23, 20) else np.diag(np.linspace(0.5, 2.0, d)).astype(np.float32)
    rng = np.random.default_rng(7)
    A = rng.standard_normal((d, d)) * 0.3
    return "mahalanobis", (A @ A.T + 0.1 * np.eye(d)).astype(np.float32)


def trajectory(oracle, X, C0, metric, M, max_iter=MAX_ITER):
    """The contract's loop: -> the states [(L_t, D_t, C_t)] for t = 0 .. T and converged, where T is the iteration the loop
    stops at with max_iter updates allowed.  State t is what a call with max_iter = t returns when t < T."""
    n, K = X.shape[0], C0.shape[0]
    C, prev = C0.copy(), np.full(n, -1, np.int64)
    states = []
    while True:
        D = oracle.pairwise(X, C, metric, M, n_threads=16)
        assert not np.isnan(D).any()
        L = np.argmin(D, axis=1)  # the first minimum: the lower centre of equal distances (-0.0 == +0.0)
        states.append((L, D[np.arange(n), L].copy(), C))
        if (L != prev).sum() == 0:
            return states, True
        if len(states) - 1 == max_iter:
            return states, False
        Cn = C.copy()
        for c in range(K):
            rows = np.flatnonzero(L == c)  # ascending
            if rows.size:
                Cn[c] = seq_mean(X[rows])
        C, prev = Cn, L


def expected(traj, max_iter, K):
    """what a call with `max_iter` must return, from the trajectory computed with MAX_ITER: (labels, dist, centroids, sizes,
    n_iter, converged)"""
    states, conv = traj
    t = min(max_iter, len(states) - 1)
    L, D, C = states[t]
    return L, D, C, np.bincount(L, minlength=K), t, bool(conv and t == len(states) - 1)


def host_form(bliss, X, C0, max_iter, metric, M):
    return bliss.playlist.kmeans(X, C0, max_iter, metric, M)


def device_form(ctx, X, C0, max_iter, metric, M):
    import torch

    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    labels, dist, cent, sizes, n_iter, conv = ctx.kmeans(t(X), t(C0), max_iter, metric, t(M))
    ctx.synchronize()
    return labels.cpu().numpy().astype(np.int64), dist.cpu().numpy(), cent.cpu().numpy(), sizes.cpu().numpy().astype(np.int64), n_iter, conv


def assert_same(got, want, what):
    print(what, "n_iter", got[4], "converged", got[5], "sizes max", int(np.max(got[3])), "empty", int((np.asarray(got[3]) == 0).sum()))
    assert (got[4], got[5]) == (want[4], want[5]), (what, "n_iter / converged", got[4], got[5], want[4], want[5])
    assert np.array_equal(got[0], want[0]), (what, "labels", int((got[0] != want[0]).sum()), "differ")
    assert np.array_equal(got[3], want[3]), (what, "sizes")
    assert np.array_equal(bits(got[1]), bits(want[1])), (what, "distance bits")
    assert np.array_equal(bits(got[2]), bits(want[2])), (what, "centroid bits")


def check_both(bliss, ctx, oracle, X, C0, metric, M, what, iters=(MAX_ITER, 0, 2)):
    traj = trajectory(oracle, X, C0, metric, M)
    K = C0.shape[0]
    for mi in iters:
        want = expected(traj, mi, K)
        assert_same(host_form(bliss, X, C0, mi, metric, M), want, (what, mi, "host form"))
        assert_same(device_form(ctx, X, C0, mi, metric, M), want, (what, mi, "device form"))
    return traj


def data(seed, n, d, K, init="rows"):
    """mixed_grid rows; the initial centres are K rows of it (distinct indices) or, init = "grid", K fresh grid points -- most of
    which no row is nearest to: many empty clusters"""
    rng = np.random.default_rng(seed)
    X = mixed_grid(rng, n, d)
    if init == "rows" and K <= n:
        C0 = X[np.sort(rng.choice(n, K, replace=False))].copy()
    else:
        C0 = mixed_grid(rng, K, d)
    return X, C0


# (n, d, K, metric, init): n is no multiple of any block, K = 300 and 1100 run past one LDS tile of centres (256 rows), d = 23 and
# 20 take the packed kernels, 1 and 64 the generic one
CASES = [
    (3001, 23, 65, "euclidean", "rows"),
    (3001, 23, 300, "euclidean", "rows"),
    (3001, 23, 1100, "euclidean", "grid"),
    (3001, 23, 65, "weights", "rows"),
    (3001, 23, 300, "spd", "rows"),
    (257, 23, 2, "spd", "rows"),
    (3001, 20, 65, "euclidean", "rows"),
    (3001, 20, 1100, "weights", "grid"),
    (257, 20, 65, "spd", "rows"),
    (3001, 1, 65, "euclidean", "grid"),
    (3001, 64, 2, "euclidean", "rows"),
    (257, 64, 65, "spd", "rows"),
    (257, 64, 300, "euclidean", "grid"),  # K > n
    (257, 23, 300, "euclidean", "grid"),  # K > n
    (257, 23, 1, "euclidean", "rows"),
    (1, 23, 1, "euclidean", "rows"),
    (1, 23, 2, "euclidean", "grid"),  # K > n
    (1, 1, 65, "weights", "grid"),
]


@pytest.mark.parametrize("n,d,K,name,init", CASES)
def test_kmeans_against_the_contract(bliss, ctx, oracle, n, d, K, name, init):
    X, C0 = data(100 + n + d + K, n, d, K, init)
    metric, M = _metric(oracle, name, d)
    traj = check_both(bliss, ctx, oracle, X, C0, metric, M, (n, d, K, name))
    if init == "grid" and K >= 300:
        assert (np.bincount(traj[0][-1][0], minlength=K) == 0).sum() >= K // 4  # on the reference alone: many empty clusters


def test_one_cluster_holds_almost_everything(bliss, ctx, oracle):
    rng = np.random.default_rng(5)
    n, d = 3001, 23
    X = mixed_grid(rng, n, d)
    X[:2800] = (X[:2800] * np.float32(1 / 64)).astype(np.float32)  # a dense core around the origin, the rest far out
    C0 = np.concatenate([X[:1], X[2800:2804]]).copy()
    traj = check_both(bliss, ctx, oracle, X, C0, "euclidean", None, "core")
    assert np.bincount(traj[0][-1][0], minlength=5).max() > 0.9 * n  # on the reference alone


def test_far_centre_stays_empty_and_keeps_its_bits(bliss, ctx, oracle):
    X, C0 = data(6, 3001, 23, 65)
    C0[3] = np.float32(3e7) + np.arange(23, dtype=np.float32)
    traj = check_both(bliss, ctx, oracle, X, C0, "euclidean", None, "far centre")
    assert len(traj[0]) > 2  # (several updates happened)
    got = device_form(ctx, X, C0, MAX_ITER, "euclidean", None)
    assert got[3][3] == 0 and np.array_equal(bits(got[2][3]), bits(C0[3]))


def test_identical_centres(bliss, ctx, oracle):
    X, C0 = data(7, 3001, 23, 2)
    C0[1] = C0[0]
    check_both(bliss, ctx, oracle, X, C0, "euclidean", None, "identical centres")
    for got in (host_form(bliss, X, C0, 0, "euclidean", None), device_form(ctx, X, C0, 0, "euclidean", None)):
        assert (got[0] == 0).all() and got[3].tolist() == [3001, 0] and np.array_equal(bits(got[2]), bits(C0))
    # ... and in the middle of a longer list, past the first tile of centres
    X, C0 = data(8, 3001, 23, 300)
    C0[290] = C0[17]
    traj = check_both(bliss, ctx, oracle, X, C0, "euclidean", None, "identical centres 17 / 290", iters=(0, MAX_ITER))
    assert (traj[0][0][0] == 17).any() and not (traj[0][0][0] == 290).any()


@pytest.mark.parametrize("name", ("euclidean", "weights", "spd"))
def test_equal_distances_from_distinct_sums(bliss, ctx, oracle, name):
    """tests/test_gpu_knn.py case b2 with the centres in the candidates' place: copies of a centre with one feature moved by
    1 .. 3 ulps -- the sums differ, the rounded distances often do not, and the lower index must win"""
    d = 23
    rng = np.random.default_rng(2)
    base = rng.standard_normal((40, d)).astype(np.float32)
    C0 = np.repeat(base, 8, axis=0)
    for c in range(1, 8):
        rows = np.arange(40) * 8 + c
        col = rng.integers(0, d, 40)
        v = C0[rows, col]
        toward = np.where(rng.integers(0, 2, 40) == 0, -np.inf, np.inf).astype(np.float32)
        ulps = rng.integers(1, 4, 40)
        for step in range(3):
            v = np.where(step < ulps, np.nextafter(v, toward), v)
        C0[rows, col] = v
    C0 = np.ascontiguousarray(C0[rng.permutation(C0.shape[0])])
    X = rng.standard_normal((3001, d)).astype(np.float32)
    metric, M = _metric(oracle, name, d)
    D = oracle.pairwise(X, C0, metric, M, n_threads=16)
    L = np.argmin(D, axis=1)
    tied = 0
    for i in range(X.shape[0]):
        same = np.flatnonzero(D[i] == D[i, L[i]])
        tied += any(not np.array_equal(C0[j], C0[L[i]]) for j in same)
    print(f"{name}: {tied} of {X.shape[0]} rows are equally near to two different centres")
    assert tied >= 300  # on the oracle alone
    check_both(bliss, ctx, oracle, X, C0, metric, M, ("b2", name), iters=(0, 2))


def test_nan(bliss, ctx):
    from bliss_rs_amd import _ffi

    X, C0 = data(9, 3001, 23, 65)
    X[2999, 4] = np.nan
    with pytest.raises(ValueError):
        host_form(bliss, X, C0, 5, "euclidean", None)
    with pytest.raises(_ffi.BlissGpuError) as e:
        device_form(ctx, X, C0, 5, "euclidean", None)
    assert e.value.code == _ffi.ERR_NAN
    X, C0 = data(9, 257, 7, 3)  # the generic kernel
    C0[2, 0] = np.nan
    with pytest.raises(ValueError):
        host_form(bliss, X, C0, 5, "euclidean", None)


def test_runs_repeat_and_stale_workspace(bliss, ctx, oracle):
    """two runs are identical, and so is a run after a differently shaped call on the same context"""
    X, C0 = data(10, 3001, 23, 300)
    first = device_form(ctx, X, C0, MAX_ITER, "euclidean", None)
    again = device_form(ctx, X, C0, MAX_ITER, "euclidean", None)
    Xb, Cb = data(11, 5000, 20, 1100, "grid")
    device_form(ctx, Xb, Cb, 3, "euclidean", None)
    Xs, Cs = data(12, 257, 64, 2)
    device_form(ctx, Xs, Cs, 3, "euclidean", None)
    third = device_form(ctx, X, C0, MAX_ITER, "euclidean", None)
    for other in (again, third):
        assert other[4:] == first[4:]
        for a, b in zip(first[:4], other[:4]):
            assert a.tobytes() == b.tobytes()
    assert_same(first, expected(trajectory(oracle, X, C0, "euclidean", None), MAX_ITER, 300), "first run")


def test_launches_and_copies_per_iteration(ctx):
    """the assignment runs n_iter + 1 times, the sort, the mean and the select once per update, and the loop copies nothing
    to the host but its pair of flag words per assignment"""
    X, C0 = data(13, 3001, 23, 65)
    ctx.profile_enable(True)
    try:
        for max_iter in (MAX_ITER, 2, 0):
            ctx.profile_reset()
            got = device_form(ctx, X, C0, max_iter, "euclidean", None)
            n_iter, conv = got[4], got[5]
            prof = {k: v[1] for k, v in ctx.profile().items()}
            print(max_iter, n_iter, conv, prof, ctx.kmeans_stats())
            assert (n_iter, conv) == ((2, False) if max_iter == 2 else (0, False) if max_iter == 0 else (n_iter, True))
            assert prof["kmeans_assign_kernel"] == n_iter + 1
            again = 0 if (conv and n_iter > 0) else 1  # the sizes of labels that moved since the last sort: its head once more
            for name in ("kmeans_hist_kernel", "kmeans_scan_tiles_kernel", "kmeans_scan_add_kernel"):
                assert prof.get(name, 0) == n_iter + again, name
            for name in ("kmeans_scatter_kernel", "segment_mean_kernel"):
                assert prof.get(name, 0) == n_iter, name
            assert prof["kmeans_select_kernel"] == n_iter + 1
            assert set(prof) <= {"kmeans_assign_kernel", "kmeans_hist_kernel", "kmeans_scan_tiles_kernel", "kmeans_scan_add_kernel",
                                 "kmeans_scatter_kernel", "segment_mean_kernel", "kmeans_select_kernel"}
            assert ctx.kmeans_stats() == (n_iter + 1, 8 * (n_iter + 1))
    finally:
        ctx.profile_enable(False)


def test_kmeans_init(bliss):
    P = bliss.playlist
    rng = np.random.default_rng(14)
    X = mixed_grid(rng, 3001, 23)
    for method in ("k-means++", "sample"):
        a, b = P.kmeans_init(X, 65, 3, method), P.kmeans_init(X, 65, 3, method)
        assert a.shape == (65, 23) and a.tobytes() == b.tobytes()
        assert a.tobytes() != P.kmeans_init(X, 65, 4, method).tobytes()
        rows = {r.tobytes() for r in X}
        assert all(r.tobytes() in rows for r in a) and len({r.tobytes() for r in a}) == 65
    # 50 distinct rows, ten copies of each, shuffled: D^2 sampling never draws a copy of a picked row while another row is left
    base = mixed_grid(rng, 50, 23)
    assert len({r.tobytes() for r in base}) == 50
    Xd = np.ascontiguousarray(np.repeat(base, 10, axis=0)[rng.permutation(500)])
    for seed in range(4):
        got = P.kmeans_init(Xd, 50, seed)
        assert len({r.tobytes() for r in got}) == 50, seed
    got = P.kmeans_init(Xd, 53, 0)  # more centres than distinct rows: the distinct ones first
    assert len({r.tobytes() for r in got[:50]}) == 50 and got.shape == (53, 23)


@pytest.fixture(scope="module")
def library(bliss, tmp_path_factory):
    rng = np.random.default_rng(15)
    n = 300
    centres = rng.standard_normal((6, 23)).astype(np.float32)
    X = (centres[rng.integers(0, 6, n)] + 0.2 * rng.standard_normal((n, 23))).astype(np.float32)
    V2 = bliss.FeaturesVersion.Version2
    songs = [bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist=f"artist{i % 11}", album=f"album {i % 40:02d}", duration=1.0,
                        analysis=bliss.Analysis(X[i], V2), features_version=V2) for i in range(n)]
    db = str(tmp_path_factory.mktemp("kmeans") / "bliss.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs)
    return db, songs, X


@pytest.mark.parametrize("builder", ("euclidean", "weights"))
def test_cluster_songs(bliss, oracle, library, builder):
    db, songs, X = library
    P = bliss.playlist
    k = 7
    mb = P.euclidean_distance if builder == "euclidean" else P.MahalanobisBuilder(oracle.feature_weights(2))
    metric, M = _metric(oracle, builder, 23)
    cl = P.cluster_songs(songs, k, seed=5, metric_builder=mb)
    init = P.kmeans_init(X, k, 5)
    want = expected(trajectory(oracle, X, init, metric, M), MAX_ITER, k)
    assert_same((cl.labels, cl.distances, cl.centroids, cl.sizes, cl.n_iter, cl.converged), want, ("cluster_songs", builder))
    assert cl.inertia == float(np.sum(want[1].astype(np.float64) ** 2))
    lists, cl2 = bliss.library.cluster_songs(db, k, seed=5, metric_builder=mb, return_clustering=True)
    assert np.array_equal(cl2.labels, cl.labels) and cl2.centroids.tobytes() == cl.centroids.tobytes()
    assert [[s.path for s in l] for l in bliss.library.cluster_songs(db, k, seed=5, metric_builder=mb)] == [[s.path for s in l] for l in lists]
    # the clusters partition the library, each in (distance, index) order
    assert sorted(s.path for l in lists for s in l) == sorted(s.path for s in songs)
    index = {s.path: i for i, s in enumerate(songs)}
    for c, l in enumerate(lists):
        rows = [index[s.path] for s in l]
        assert len(rows) == want[3][c] and all(want[0][i] == c for i in rows)
        keys = [(float(want[1][i]), i) for i in rows]
        assert keys == sorted(keys)
        assert rows == cl.members(c).tolist()


# ---- the host form's staging: every optional argument given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("dist,sizes", ((True, True), (False, False), (True, False), (False, True)))
def test_host_form_stages_like_the_device_form(bliss, ctx, dist, sizes):
    import staging_cases as sc

    def build(c, dev):
        k = 4
        labels, dd = dev(sc.out((c.n,), np.uint32)), dev(sc.out((c.n,), np.float32, dist))
        cent, sz = dev(sc.out((k, sc.D), np.float32)), dev(sc.out((k,), np.uint32, sizes))
        n_iter, conv = np.full(1, 99, np.uint32), np.full(1, 99, np.int32)  # (host memory in both forms)
        outs = [labels, dd, cent, sz, n_iter, conv]
        return [dev(c.X), c.n, sc.D, dev(np.ascontiguousarray(c.X[:k])), k, 2, dev(c.M), 6] + outs, outs

    sc.check(bliss, ctx, "kmeans", build, lists=False)
