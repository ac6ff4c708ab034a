"""GPU tests (-m gpu) of the silhouette on the device (blissgpu_silhouette / blissgpu_silhouette_device: the k-means sort of the
labels, silhouette_scan_kernel, silhouette_finish_kernel).  Expected values never come from the code under test: the reference
is the contract of include/blissgpu.h written out in numpy below -- distances from oracle.pairwise(X, X, metric, M), one
sequential f64 sum per (song, cluster) over the members in ascending index (np.add.accumulate), the quotients, the first minimum
over the other non-empty clusters, s from a and b.  Every comparison is exact: s, a and b by bits, neighbour and sizes by
equality, for both forms, for every split into column groups and for a scrambled subset of the songs with repeats."""
import numpy as np
import pytest

from test_gpu_albums import bits, mixed_grid

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


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _metric(oracle, name, d):
    """-> (library metric name, M or None): euclidean, diagonal weights, a full SPD matrix (as tests/test_gpu_kmeans.py)"""
    if name == "euclidean":
        return name, None
    if name == "weights":
        return "mahalanobis", oracle.feature_weights(2 if d == 23 else 1) if d in (23, 20) else np.diag(np.linspace(0.5, 2.0, d)).astype(np.float32)
    rng = np.random.default_rng(7)
    A = rng.standard_normal((d, d)) * 0.3
    return "mahalanobis", (A @ A.T + 0.1 * np.eye(d)).astype(np.float32)


def cluster_sums(D, labels, k, order="ascending"):
    """S [n, k] f64: S[i, c] = 0.0 + D[i, j0] + D[i, j1] + ... over the members of c, one sequential f64 sum (0 for an empty c).
    order: "ascending" is the contract; "descending" and "halves" (two sequential halves, added) are what it is NOT"""
    n = D.shape[0]
    S = np.zeros((n, k), np.float64)
    for c in range(k):
        members = np.flatnonzero(labels == c)
        if members.size == 0:
            continue
        if order == "descending":
            members = members[::-1]
        T = np.concatenate([np.zeros((n, 1), np.float64), D[:, members].astype(np.float64)], axis=1)
        if order == "halves":
            h = (T.shape[1] + 1) // 2
            S[:, c] = np.add.accumulate(T[:, :h], axis=1)[:, -1] + np.add.accumulate(np.concatenate([np.zeros((n, 1)), T[:, h:]], axis=1), axis=1)[:, -1]
        else:
            S[:, c] = np.add.accumulate(T, axis=1)[:, -1]
    return S


def from_sums(S, labels, k):
    """the contract from the sums on: -> (s f32, a f64, b f64, neighbour, sizes) for every song"""
    n = S.shape[0]
    sizes = np.bincount(labels, minlength=k).astype(np.int64)
    assert (sizes > 0).sum() >= 2
    own = sizes[labels]
    a = np.zeros(n, np.float64)
    many = own > 1
    a[many] = S[np.arange(n), labels][many] / (own[many] - 1).astype(np.float64)
    b, nb = np.zeros(n, np.float64), np.zeros(n, np.int64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for o in np.flatnonzero(sizes > 0):
            idx = np.flatnonzero(labels == o)
            cand = np.array([c for c in np.flatnonzero(sizes > 0) if c != o])
            Q = S[np.ix_(idx, cand)] / sizes[cand].astype(np.float64)[None, :]
            j = np.argmin(Q, axis=1)  # the first minimum: equal quotients go to the lower cluster
            b[idx], nb[idx] = Q[np.arange(idx.size), j], cand[j]
        s = np.where(a < b, 1.0 - a / b, b / a - 1.0)
        s = np.where((own == 1) | (a == b), 0.0, s)
    return s.astype(np.float32), a, b, nb, sizes


def reference(oracle, X, labels, k, metric, M):
    D = oracle.pairwise(X, X, metric, M, n_threads=16)
    assert not np.isnan(D).any()
    return from_sums(cluster_sums(D, labels, k), labels, k)


def host_form(bliss, X, labels, k, metric, M, rows, cg):
    P = bliss.playlist
    mb = P.euclidean_distance if metric == "euclidean" else P.MahalanobisBuilder(M)
    r = P.silhouette(X, labels, mb, rows, k=k, col_groups=cg)
    return r.values, r.a, r.b, r.neighbour, r.sizes


def device_form(ctx, X, labels, k, metric, M, rows, cg):
    import torch

    f = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    i = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()  # noqa: E731
    s, a, b, nb, sizes = ctx.silhouette(f(X), i(labels), metric, f(M), i(rows), cg, k)
    ctx.synchronize()
    return s.cpu().numpy(), a.cpu().numpy(), b.cpu().numpy(), nb.cpu().numpy().astype(np.int64), sizes.cpu().numpy().astype(np.int64)


def assert_same(got, want, rows, what):
    s, a, b, nb, sizes = want
    if rows is not None:
        s, a, b, nb = s[rows], a[rows], b[rows], nb[rows]
    assert np.array_equal(np.asarray(got[4], np.int64), sizes), (what, "sizes")
    assert np.array_equal(np.asarray(got[3], np.int64), nb), (what, "neighbour", int((np.asarray(got[3]) != nb).sum()), "differ")
    assert np.array_equal(bits64(got[1]), bits64(a)), (what, "a bits", int((bits64(got[1]) != bits64(a)).sum()), "differ")
    assert np.array_equal(bits64(got[2]), bits64(b)), (what, "b bits", int((bits64(got[2]) != bits64(b)).sum()), "differ")
    assert np.array_equal(bits(got[0]), bits(s)), (what, "s bits", int((bits(got[0]) != bits(s)).sum()), "differ")


def scrambled(n, seed):
    """a subset of the songs in random order, with repeats"""
    rng = np.random.default_rng(seed)
    m = max(1, (2 * n) // 3)
    rows = rng.choice(n, m, replace=False)
    return np.concatenate([rows, rows[: max(1, m // 5)], rows[:1]])[rng.permutation(m + max(1, m // 5) + 1)].astype(np.int64)


def check_all(bliss, ctx, want, X, labels, k, metric, M, what, groups=None, forms=("host", "device")):
    groups = (0, 1, 3, k + 5) if groups is None else groups
    for rows in (None, scrambled(X.shape[0], 3)):
        for cg in groups:
            if "host" in forms:
                assert_same(host_form(bliss, X, labels, k, metric, M, rows, cg), want, rows, (what, cg, rows is None, "host form"))
            if "device" in forms:
                assert_same(device_form(ctx, X, labels, k, metric, M, rows, cg), want, rows, (what, cg, rows is None, "device form"))


def labels_1500(rng):
    """7 clusters over 1500 songs, scattered: cluster 2 is empty, 4 a singleton, 1 has exactly 256 members and 5 has 257 (the
    LDS tile edge), 0 / 3 / 6 share the rest"""
    sizes = [400, 256, 0, 300, 1, 257, 286]
    assert sum(sizes) == 1500
    return np.repeat(np.arange(7), sizes)[rng.permutation(1500)].astype(np.int64)


# (n, d, k, metric): n is a multiple of neither 64 nor 256, 1500 songs are several workgroups; d = 23 and 20 take the packed
# kernels, 1 and 64 the generic one
CASES = [
    (1500, 23, 7, "euclidean"),
    (1500, 23, 7, "weights"),
    (700, 23, 5, "spd"),
    (1500, 20, 7, "euclidean"),
    (300, 20, 3, "spd"),
    (300, 20, 3, "weights"),
    (600, 1, 4, "euclidean"),
    (300, 64, 3, "spd"),
    (257, 23, 300, "euclidean"),  # k > n, mostly empty clusters
    (2, 23, 2, "euclidean"),
]


@pytest.mark.parametrize("n,d,k,name", CASES)
def test_silhouette_against_the_contract(bliss, ctx, oracle, n, d, k, name):
    rng = np.random.default_rng(200 + n + d + k)
    X = mixed_grid(rng, n, d)
    if n == 1500:
        labels = labels_1500(rng)
    elif n == 2:
        labels = np.array([1, 0], np.int64)
    else:
        labels = rng.integers(0, k, n).astype(np.int64)
    metric, M = _metric(oracle, name, d)
    want = reference(oracle, X, labels, k, metric, M)
    print((n, d, k, name), "sizes", want[4][:8].tolist(), "empty", int((want[4] == 0).sum()), "s range", float(want[0].min()), float(want[0].max()))
    if n == 1500:
        assert sorted(want[4].tolist()) == [0, 1, 256, 257, 286, 300, 400]
    if k > n:
        assert (want[4] == 0).sum() >= k // 4
    check_all(bliss, ctx, want, X, labels, k, metric, M, (n, d, k, name))


def test_the_order_of_the_sums_shows(bliss, ctx, oracle):
    """On ordinary data an f64 sum of f32 distances is exact and no order can be told from another; here the members of the
    first 300 are scaled by 2^30 (even) and 2^-10 (odd), and the sums are not exact any more"""
    rng = np.random.default_rng(31)
    n, d, k = 600, 23, 3
    X = rng.uniform(-1.0, 1.0, (n, d)).astype(np.float32)
    X[0:300:2] *= np.float32(2.0 ** 30)
    X[1:300:2] *= np.float32(2.0 ** -10)
    labels = (np.arange(n) % k).astype(np.int64)
    D = oracle.pairwise(X, X, "euclidean", None, n_threads=16)
    assert np.isfinite(D).all()
    S = cluster_sums(D, labels, k)
    changed_desc = (bits64(S) != bits64(cluster_sums(D, labels, k, "descending"))).any(axis=1).sum()
    changed_half = (bits64(S) != bits64(cluster_sums(D, labels, k, "halves"))).any(axis=1).sum()
    print("songs whose sums change: descending", int(changed_desc), "two halves", int(changed_half), "of", n)
    assert changed_desc >= n // 4 and changed_half >= 1  # on the reference alone
    want = from_sums(S, labels, k)
    check_all(bliss, ctx, want, X, labels, k, "euclidean", None, "order", groups=(1, 3))


def test_equal_quotients_go_to_the_lower_cluster(bliss, ctx, oracle):
    rng = np.random.default_rng(32)
    d, m = 23, 90
    A, B = mixed_grid(rng, 150, d), mixed_grid(rng, m, d)
    far = mixed_grid(rng, 70, d) + np.float32(3e5)
    # clusters 1 and 3 hold copies of the same rows in the same order; 0 and 2 look at them from outside
    X = np.concatenate([A, B, far, B]).astype(np.float32)
    labels = np.concatenate([np.zeros(150), np.ones(m), np.full(70, 2), np.full(m, 3)]).astype(np.int64)
    k = 5  # (cluster 4 is empty)
    D = oracle.pairwise(X, X, "euclidean", None, n_threads=16)
    S = cluster_sums(D, labels, k)
    want = from_sums(S, labels, k)
    outside = np.flatnonzero((labels == 0) | (labels == 2))
    tied = bits64(S[outside, 1] / m) == bits64(S[outside, 3] / m)
    assert tied.all()  # on the reference alone: equal f64 quotients occur
    assert (want[3][labels == 0] == 1).all() and not (want[3] == 3)[outside].any()
    check_all(bliss, ctx, want, X, labels, k, "euclidean", None, "ties", groups=(0, 1, 2, 3, 4))
    for cg in (1, 4):
        got = device_form(ctx, X, labels, k, "euclidean", None, None, cg)
        assert (got[3][labels == 0] == 1).all()


def test_degenerate_values(bliss, ctx, oracle):
    rng = np.random.default_rng(33)
    d = 23
    # a singleton: s == 0 and a == 0
    X = mixed_grid(rng, 300, d)
    labels = rng.integers(0, 3, 300).astype(np.int64)
    labels[123] = 3
    for got in (host_form(bliss, X, labels, 4, "euclidean", None, None, 0), device_form(ctx, X, labels, 4, "euclidean", None, None, 3)):
        assert got[0][123] == 0.0 and got[1][123] == 0.0 and got[2][123] > 0.0 and got[4].tolist()[3] == 1
    check_all(bliss, ctx, reference(oracle, X, labels, 4, "euclidean", None), X, labels, 4, "euclidean", None, "singleton", groups=(0, 2))
    # all rows identical: every s == 0
    X = np.repeat(mixed_grid(rng, 1, d), 300, axis=0)
    labels = (np.arange(300) % 2).astype(np.int64)
    for got in (host_form(bliss, X, labels, 2, "euclidean", None, None, 0), device_form(ctx, X, labels, 2, "euclidean", None, None, 2)):
        assert not got[0].any() and not got[1].any() and not got[2].any() and got[3].tolist() == (1 - labels).tolist()
    # a song at distance 0 from its whole cluster, the other cluster elsewhere: s == 1
    X = np.concatenate([np.repeat(mixed_grid(rng, 1, d), 100, axis=0), mixed_grid(rng, 200, d) + np.float32(5e4)]).astype(np.float32)
    labels = np.concatenate([np.zeros(100), np.ones(200)]).astype(np.int64)
    for got in (host_form(bliss, X, labels, 2, "euclidean", None, None, 0), device_form(ctx, X, labels, 2, "euclidean", None, None, 1)):
        assert (got[0][:100] == 1.0).all() and not got[1][:100].any() and (got[2][:100] > 0).all()
    check_all(bliss, ctx, reference(oracle, X, labels, 2, "euclidean", None), X, labels, 2, "euclidean", None, "distance 0", groups=(0,))


def test_errors_and_the_context_afterwards(bliss, ctx, oracle):
    from bliss_rs_amd import _ffi

    rng = np.random.default_rng(34)
    X = mixed_grid(rng, 700, 23)
    labels = rng.integers(0, 5, 700).astype(np.int64)
    want = reference(oracle, X, labels, 5, "euclidean", None)

    def both(X, labels, k, rows, code):
        if code == _ffi.ERR_NAN:
            with pytest.raises(ValueError):
                host_form(bliss, X, labels, k, "euclidean", None, rows, 0)
        else:
            with pytest.raises(_ffi.BlissGpuError) as e:
                host_form(bliss, X, labels, k, "euclidean", None, rows, 0)
            assert e.value.code == code
        with pytest.raises(_ffi.BlissGpuError) as e:
            device_form(ctx, X, labels, k, "euclidean", None, rows, 3)
        assert e.value.code == code
        # the context is usable afterwards
        assert_same(device_form(ctx, X0, labels0, 5, "euclidean", None, None, 0), want, None, "after an error")

    X0, labels0 = X, labels
    Xn = X.copy()
    Xn[698, 4] = np.nan
    both(Xn, labels, 5, None, _ffi.ERR_NAN)
    both(Xn, labels, 5, np.array([698, 5]), _ffi.ERR_NAN)
    both(X, np.full(700, 2, np.int64), 5, None, _ffi.ERR_INVALID)  # one non-empty cluster
    bad = labels.copy()
    bad[650] = 5
    both(X, bad, 5, None, _ffi.ERR_INVALID)  # a label equal to k
    both(X, bad, 5, np.array([1, 2, 3]), _ffi.ERR_INVALID)  # ... on a song that is not scored
    both(X, labels, 5, np.array([3, 700, 1]), _ffi.ERR_INVALID)  # a rows entry equal to n
    Xg = mixed_grid(rng, 300, 7)  # the generic kernel
    Xg[17, 0] = np.nan
    with pytest.raises(ValueError):
        host_form(bliss, Xg, rng.integers(0, 3, 300), 3, "euclidean", None, None, 0)


def test_stale_workspace(ctx):
    """a large call, a small one, then the large one again: the same bits"""
    rng = np.random.default_rng(35)
    X, labels = mixed_grid(rng, 1500, 23), labels_1500(rng)
    Xs, ls = mixed_grid(rng, 257, 64), rng.integers(0, 3, 257)
    first = device_form(ctx, X, labels, 7, "euclidean", None, None, 3)
    device_form(ctx, Xs, ls, 3, "euclidean", None, np.array([5, 5, 200]), 2)
    again = device_form(ctx, X, labels, 7, "euclidean", None, None, 3)
    other = device_form(ctx, X, labels, 7, "euclidean", None, None, 7)
    for got in (again, other):
        for u, v in zip(first, got):
            assert u.tobytes() == v.tobytes()


def test_launches(ctx):
    rng = np.random.default_rng(36)
    X, labels = mixed_grid(rng, 1500, 23), labels_1500(rng)
    ctx.profile_enable(True)
    try:
        for cg in (0, 3):
            ctx.profile_reset()
            device_form(ctx, X, labels, 7, "euclidean", None, None, cg)
            prof = {name: v[1] for name, v in ctx.profile().items()}
            print(cg, prof)
            assert prof["silhouette_scan_kernel"] == 1 and prof["silhouette_finish_kernel"] == 1
            assert not [name for name in prof if name.startswith(("pairwise", "set_distance", "radix_", "knn_"))]
            assert set(prof) == {"silhouette_scan_kernel", "silhouette_finish_kernel", "kmeans_hist_kernel", "kmeans_scan_tiles_kernel",
                                 "kmeans_scan_add_kernel", "kmeans_scatter_kernel"}
    finally:
        ctx.profile_enable(False)


def silhouette_f64(X, labels):
    """the plain definition in f64: euclidean distances and means in float64, s = (b - a) / max(a, b), 0 for a singleton"""
    X = X.astype(np.float64)
    n = X.shape[0]
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))
    ks = np.unique(labels)
    sizes = np.array([(labels == c).sum() for c in ks])
    S = np.stack([D[:, labels == c].sum(axis=1) for c in ks], axis=1)
    pos = np.searchsorted(ks, labels)
    own = sizes[pos]
    a = S[np.arange(n), pos] / np.maximum(own - 1, 1)
    Q = S / sizes[None, :]
    Q[np.arange(n), pos] = np.inf
    b = Q.min(axis=1)
    return np.where(own == 1, 0.0, (b - a) / np.maximum(a, b))


def f64_bound(d):
    # every f32 distance carries a relative error of at most about (d + 4) 2^-24 (the subtraction, the square, d - 1 adds, the
    # root); the means inherit it; 1 - a / b doubles it; the rounding of s adds 2^-24
    return 2 * (d + 5) * 2.0 ** -24


def test_against_the_plain_definition_in_f64(bliss, ctx):
    rng = np.random.default_rng(37)
    n, d, k = 700, 23, 5
    X = rng.uniform(-1.0, 1.0, (n, d)).astype(np.float32)
    labels = rng.integers(0, k, n).astype(np.int64)
    s64 = silhouette_f64(X, labels)
    for got in (host_form(bliss, X, labels, k, "euclidean", None, None, 0), device_form(ctx, X, labels, k, "euclidean", None, None, 0)):
        err = np.abs(got[0].astype(np.float64) - s64).max()
        print("max |s - s64|", err, "bound", f64_bound(d))
        assert err <= f64_bound(d)


def test_choose_k_finds_four_blobs(bliss):
    P = bliss.playlist
    rng = np.random.default_rng(38)
    d, sigma = 23, 0.1
    centres = (3.0 * rng.standard_normal((4, d))).astype(np.float32)
    gaps = [np.linalg.norm(centres[i].astype(np.float64) - centres[j]) for i in range(4) for j in range(i)]
    assert min(gaps) >= 10 * sigma
    truth = np.repeat(np.arange(4), 100)
    perm = rng.permutation(400)
    X, truth = (centres[truth] + sigma * rng.standard_normal((400, d))).astype(np.float32)[perm], truth[perm]
    # on the reference, in f64: the true labelling scores above every merge of two blobs
    score_true = silhouette_f64(X, truth).mean()
    for i in range(4):
        for j in range(i):
            assert silhouette_f64(X, np.where(truth == i, j, truth)).mean() < score_true
    sel = P.choose_k(X, range(2, 9), seed=0)
    print("scores", dict(zip(sel.ks, sel.scores)), "f64 score of the truth", score_true)
    assert sel.ks == list(range(2, 9)) and sel.best_k == 4 and len(sel.scores) == 7
    assert sel.scores[sel.ks.index(4)] == max(sel.scores)
    assert len(sel.clustering.sizes) == 4 and sorted(sel.clustering.sizes.tolist()) == [100] * 4
    assert abs(sel.scores[2] - silhouette_f64(X, sel.clustering.labels).mean()) <= f64_bound(d)
    # a sample: the same rule over the sampled rows
    part = P.choose_k(X, [3, 4, 5], seed=0, sample=150)
    assert part.best_k == 4
    rows = np.sort(np.random.Generator(np.random.PCG64(0)).choice(400, 150, replace=False))
    assert abs(part.scores[1] - silhouette_f64(X, part.clustering.labels)[rows].mean()) <= f64_bound(d)
    # choose_k's scores are those of silhouette on the same labels
    sil = P.silhouette(X, sel.clustering.labels)
    assert sil.score == sel.scores[2] and sil.sizes.tolist() == sel.clustering.sizes.tolist()


@pytest.fixture(scope="module")
def library(bliss, tmp_path_factory):
    rng = np.random.default_rng(39)
    n = 240
    centres = (2.0 * rng.standard_normal((3, 23))).astype(np.float32)
    blob = rng.integers(0, 3, n)
    X = (centres[blob] + 0.1 * rng.standard_normal((n, 23))).astype(np.float32)
    genres = ["rock", "jazz", "ambient"]
    V2 = bliss.FeaturesVersion.Version2
    songs = [bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist=f"artist{i % 9}", album=f"album {i % 30:02d}", duration=1.0,
                        genre=None if i % 10 == 7 else genres[blob[i]], analysis=bliss.Analysis(X[i], V2), features_version=V2)
             for i in range(n)]
    db = str(tmp_path_factory.mktemp("silhouette") / "bliss.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs)
    return db, songs, X, blob


def test_library_choose_clusters_and_label_silhouette(bliss, oracle, library):
    db, songs, X, blob = library
    P = bliss.playlist
    sel, lists = bliss.library.choose_clusters(db, ks=range(2, 6), seed=1)
    want = P.choose_k(X, range(2, 6), seed=1)
    assert sel.best_k == want.best_k == 3 and sel.scores == want.scores and len(lists) == 3
    assert sorted(s.path for l in lists for s in l) == sorted(s.path for s in songs)
    index = {s.path: i for i, s in enumerate(songs)}
    for c, l in enumerate(lists):
        assert [index[s.path] for s in l] == sel.clustering.members(c).tolist()
        assert len({blob[index[s.path]] for s in l}) == 1  # a cluster is a blob
    # the genre labelling: songs without the tag are left out before the call
    sil, tags = bliss.library.label_silhouette(db, "genre")
    keep = np.array([i for i, s in enumerate(songs) if s.genre is not None])
    assert len(keep) == 240 - 24 and sorted(tags) == ["ambient", "jazz", "rock"]
    labels = np.array([tags.index(songs[i].genre) for i in keep])
    ref = reference(oracle, X[keep], labels, 3, "euclidean", None)
    assert_same((sil.values, sil.a, sil.b, sil.neighbour, sil.sizes), ref, None, "label_silhouette")
    assert sil.labels.tolist() == labels.tolist() and sil.score > 0.8
    # ... under a metric: the before / after check of a learned M
    W = oracle.feature_weights(2)
    silw, tagsw = bliss.library.label_silhouette(db, "genre", P.MahalanobisBuilder(W))
    assert tagsw == tags
    assert_same((silw.values, silw.a, silw.b, silw.neighbour, silw.sizes), reference(oracle, X[keep], labels, 3, "mahalanobis", W), None, "weights")
    by_artist, artists = bliss.library.label_silhouette(db, "artist")
    assert len(artists) == 9 and len(by_artist.values) == 240 and by_artist.score < sil.score


# ---- the host form's staging: every optional argument given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("rows,extras", ((True, True), (False, False), (True, False), (False, True)))
def test_host_form_stages_like_the_device_form(bliss, ctx, rows, extras):
    import staging_cases as sc

    def build(c, dev):
        q = c.q if rows else c.n
        s, a, b = dev(sc.out((q,), np.float32)), dev(sc.out((q,), np.float64, extras)), dev(sc.out((q,), np.float64, extras))
        nb, sizes = dev(sc.out((q,), np.uint32, extras)), dev(sc.out((4,), np.uint32, extras))
        r = (np.arange(c.q) * 7 % c.n).astype(np.uint32) if rows else None
        return [dev(c.X), c.n, sc.D, dev((np.arange(c.n) % 4).astype(np.uint32)), 4, 2, dev(c.M), dev(r), c.q, 0, s, a, b, nb, sizes], [s, a, b, nb, sizes]

    sc.check(bliss, ctx, "silhouette", build, lists=False)
