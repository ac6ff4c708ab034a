"""GPU tests (-m gpu) of the group neighbours on the device (blissgpu_group_neighbours / blissgpu_group_neighbours_device: the
k-means sort of the labels, chamfer_scan_kernel, chamfer_reduce_kernel, chamfer_select_kernel).  Expected values never come from
the code under test: the reference is the contract of include/blissgpu.h written out in numpy (tests/test_group_neighbours_host.py:
the minimum per (song, group), the blocked tree sum in f64, the division, the symmetrisation, the selection) applied to
playlist.pairwise_distances(X, X) from the device, which other tests hold to the oracle.  Every comparison is exact: idx and sizes
by equality, dist and matrix by bits, for both forms, both modes and every slab."""
import numpy as np
import pytest

from test_group_neighbours_host import DIRECTED, SYMMETRIC, contract, directed

pytestmark = pytest.mark.gpu
MODES = {SYMMETRIC: "symmetric", DIRECTED: "directed"}
ERR_INVALID, ERR_OOM, ERR_NAN = 2, 4, 5


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


def builder_of(P, metric, M):
    return P.euclidean_distance if metric == "euclidean" else P.MahalanobisBuilder(M)


def host_form(P, X, labels, k, t, mode, metric="euclidean", M=None, queries=None, slab=0):
    r = P.group_neighbours(X, labels, t, builder_of(P, metric, M), k, queries, MODES[mode], True, slab)
    return r.idx, r.dist, r.sizes, r.matrix


def device_form(ctx, X, labels, k, t, mode, metric="euclidean", M=None, queries=None, slab=0):
    idx, dist, sizes, matrix = ctx.group_neighbours(X, labels, k, t, metric, M, queries, MODES[mode], slab, True)
    assert idx.dtype == np.int32 and dist.dtype == np.float64 and matrix.dtype == np.float64
    return idx.astype(np.int64), dist, sizes.astype(np.int64), matrix


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "idx", got[0], want[0])
    assert np.array_equal(got[2], want[2]), (what, "sizes")
    assert np.array_equal(bits64(got[1]), bits64(want[1])), (what, "dist", got[1], want[1])
    assert np.array_equal(bits64(got[3]), bits64(want[3])), (what, "matrix")


def check(bliss, ctx, X, labels, k, t, metric="euclidean", M=None, queries=None, slabs=(0,), what=""):
    """both modes and both forms against the contract; -> the all-pairs matrix"""
    P = bliss.playlist
    Dm = P.pairwise_distances(X, X, metric, M)
    for mode in (SYMMETRIC, DIRECTED):
        want = contract(Dm, labels, k, t, mode, queries)
        for slab in slabs:
            assert_same(device_form(ctx, X, labels, k, t, mode, metric, M, queries, slab), want, (what, "device", mode, slab))
        assert_same(host_form(P, X, labels, k, t, mode, metric, M, queries), want, (what, "host", mode))
    return Dm


# ---- the order-sensitive case ----
@pytest.fixture(scope="module")
def ordered(bliss):
    """n = 900, d = 23, k = 7 with magnitudes 2^30 / 1 / 2^-10 so that the order of an f64 sum shows in its bits; sizes
    501 / 74 / 80 / 71 / 173 / 1 / 0: a group of two blocks, a singleton and an empty group"""
    rng = np.random.default_rng(7)
    n, k = 900, 7
    X = rng.standard_normal((n, 23)).astype(np.float32)
    X[0:300:3] *= np.float32(2.0 ** 30)
    X[1:300:3] *= np.float32(2.0 ** -10)
    labels = rng.integers(0, 6, n)
    labels[(np.arange(n) < 520) & (rng.random(n) < 0.8)] = 0
    labels[labels == 5] = 4
    labels[899] = 5
    assert np.bincount(labels, minlength=k).tolist() == [501, 74, 80, 71, 173, 1, 0]
    Dm = bliss.playlist.pairwise_distances(X, X)
    assert np.isfinite(Dm).all()
    return X, labels, k, Dm


def test_the_order_of_the_sums_shows(ordered):
    """the case tells the contract's tree from a sequential and from a reversed sum"""
    X, labels, k, Dm = ordered
    tree = directed(Dm, labels, k)[0]
    live = ~np.isnan(tree)
    assert live.sum() == 30
    for order in ("sequential", "reversed"):
        other = directed(Dm, labels, k, order)[0]
        differ = int((bits64(tree)[live] != bits64(other)[live]).sum())
        print(order, differ, "of 30 ordered group pairs differ")
        assert differ >= 10


@pytest.mark.parametrize("mode", [SYMMETRIC, DIRECTED])
@pytest.mark.parametrize("t", [3, 9])
def test_the_contract_on_the_order_sensitive_case(bliss, ctx, ordered, mode, t):
    X, labels, k, Dm = ordered
    subset = np.array([4, 6, 0, 5, 4, 2])  # shuffled, a repeat, the empty group, the singleton
    for queries in (None, subset):
        want = contract(Dm, labels, k, t, mode, queries)
        if t == 9:
            assert (want[0][:, 5:] == -1).all() and np.isinf(want[1][:, 5:]).all()  # five other non-empty groups: padding
        if queries is not None:
            assert (want[0][1] == -1).all()  # the empty group's row
        for slab in (1, 3, 0, k + 5):
            assert_same(device_form(ctx, X, labels, k, t, mode, queries=queries, slab=slab), want, ("device", slab))
        for slab in (0, 2):
            assert_same(host_form(bliss.playlist, X, labels, k, t, mode, queries=queries, slab=slab), want, ("host", slab))


def test_outputs_that_are_not_asked_for(bliss, ctx, ordered):
    X, labels, k, Dm = ordered
    want = contract(Dm, labels, k, 2)
    idx, dist, sizes, matrix = ctx.group_neighbours(X, labels, k, 2)
    assert matrix is None and np.array_equal(idx, want[0]) and np.array_equal(bits64(dist), bits64(want[1]))
    r = bliss.playlist.group_neighbours(X, labels, 2)  # k from the labels: 6, the empty group 6 is not there
    assert r.matrix is None and r.sizes.shape == (6,) and np.array_equal(r.idx, want[0][:6])
    # no query: the matrix and the sizes are still written
    r = bliss.playlist.group_neighbours(X, labels, 2, k=k, queries=[], matrix=True)
    assert r.idx.shape == (0, 2) and np.array_equal(bits64(r.matrix), bits64(want[3])) and np.array_equal(r.sizes, want[2])


# ---- other shapes ----
def spd(d, seed):
    A = np.random.default_rng(seed).standard_normal((d, d)) * 0.3
    return (A @ A.T + 0.1 * np.eye(d)).astype(np.float32)


@pytest.mark.parametrize("d,n,name", [(20, 300, "euclidean"), (20, 300, "diagonal"), (20, 300, "full"), (23, 300, "diagonal"), (23, 300, "full"),
                                      (1, 120, "euclidean"), (64, 120, "euclidean"), (64, 120, "full"), (5, 120, "diagonal")])
def test_metrics_and_feature_counts(bliss, ctx, d, n, name):
    rng = np.random.default_rng(100 + d)
    X = (rng.standard_normal((n, d)) * 10.0 ** rng.integers(-2, 3, (n, 1))).astype(np.float32)
    k = 9
    labels = rng.integers(0, k - 1, n)  # group 8 stays empty
    labels[labels == 3] = 2             # and so does group 3
    metric, M = "euclidean", None
    if name == "diagonal":
        metric, M = "mahalanobis", np.diag(np.linspace(0.5, 2.0, d)).astype(np.float32)
    elif name == "full":
        metric, M = "mahalanobis", spd(d, 7)
    check(bliss, ctx, X, labels, k, 4, metric, M, np.array([8, 0, 7, 7, 3, 1]), slabs=(0, 2), what=(d, name))
    check(bliss, ctx, X, labels, k, 11, metric, M, None, slabs=(4,), what=(d, name, "all"))


def test_degenerate_labellings(bliss, ctx):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((70, 23)).astype(np.float32)
    pad = lambda q, t: (np.full((q, t), -1), np.full((q, t), np.inf))  # noqa: E731
    # one song; one group; every song in one group of several: rows of padding, BLISSGPU_OK
    for Xc, labels, k in ((X[:1], np.zeros(1, int), 1), (X[:1], np.array([2]), 4), (X, np.zeros(70, int), 1), (X, np.full(70, 2), 5)):
        for mode in (SYMMETRIC, DIRECTED):
            for form in (lambda *a: device_form(ctx, *a), lambda *a: host_form(bliss.playlist, *a)):
                idx, dist, sizes, matrix = form(Xc, labels, k, 3, mode)
                assert np.array_equal(idx, pad(k, 3)[0]) and np.array_equal(dist, pad(k, 3)[1])
                assert sizes.tolist() == np.bincount(labels, minlength=k).tolist()
                assert np.array_equal(matrix, np.where(np.eye(k, dtype=bool), 0.0, np.inf))
    # two songs in two groups: the one distance, both ways
    Dm = check(bliss, ctx, X[:2], np.array([1, 0]), 2, 1, what="two")
    assert ctx.group_neighbours(X[:2], np.array([1, 0]), 2, 1)[1].tolist() == [[float(Dm[0, 1])], [float(Dm[0, 1])]]
    # no song at all, through the device form: the select kernel alone
    idx, dist, sizes, matrix = device_form(ctx, X[:0], np.zeros(0, int), 3, 2, SYMMETRIC)
    assert (idx == -1).all() and np.isinf(dist).all() and not sizes.any() and np.array_equal(matrix, np.where(np.eye(3, dtype=bool), 0.0, np.inf))


@pytest.mark.parametrize("m", [255, 256, 257, 513])
def test_block_edges(bliss, ctx, m):
    """one group of m songs plus one song outside: the sum over the group has 1, 2 or 3 blocks, the last of them short"""
    rng = np.random.default_rng(m)
    X = (rng.standard_normal((m + 1, 23)) * 10.0 ** rng.integers(-6, 7, (m + 1, 1))).astype(np.float32)
    labels = np.ones(m + 1, int)
    labels[m // 2] = 0
    check(bliss, ctx, X, labels, 2, 1, what=m)


def test_many_small_groups_are_packed(bliss, ctx):
    """albums of a few songs: a wavefront's 256 positions span dozens of groups, more groups than one slab holds"""
    rng = np.random.default_rng(12)
    n, k = 1100, 300
    X = rng.standard_normal((n, 23)).astype(np.float32)
    labels = rng.integers(0, k, n)
    labels[labels % 17 == 3] = 1  # some empty groups, one larger
    check(bliss, ctx, X, labels, k, 5, queries=rng.integers(0, k, 40), slabs=(0, 7, 64), what="small groups")


def test_equal_values_go_to_the_lower_group(bliss, ctx):
    rng = np.random.default_rng(5)
    base = rng.standard_normal((20, 23)).astype(np.float32)
    far = (base + 100.0).astype(np.float32)
    # the same rows in groups 4, 1 and 2 (every distance between them is 0), other rows in 0 and 3
    X = np.concatenate([base, far[:7], base, base, far[7:]])
    labels = np.concatenate([np.full(20, 4), np.full(7, 0), np.full(20, 1), np.full(20, 2), np.full(13, 3)])
    perm = rng.permutation(X.shape[0])
    X, labels = X[perm], labels[perm]
    Dm = check(bliss, ctx, X, labels, 5, 3, slabs=(0, 1), what="ties")
    idx, dist, _, _ = device_form(ctx, X, labels, 5, 3, SYMMETRIC)
    assert idx[4].tolist()[:2] == [1, 2] and idx[1].tolist()[:2] == [2, 4] and idx[2].tolist()[:2] == [1, 4]
    assert (dist[[1, 2, 4], :2] == 0.0).all() and (Dm[labels == 4][:, labels == 1].min(axis=1) == 0.0).all()


def test_errors_and_the_context_afterwards(bliss, ctx, ordered):
    P = bliss.playlist
    X, labels, k, Dm = ordered
    want = contract(Dm, labels, k, 3)
    i1, i2 = int(np.flatnonzero(labels == 1)[0]), int(np.flatnonzero(labels == 2)[0])
    for bad in (np.nan, np.inf):  # +inf in the same feature of two songs of different groups: inf - inf between them
        Xb = X.copy()
        Xb[[i1, i2], 3] = bad
        with pytest.raises(bliss.BlissGpuError) as e:
            ctx.group_neighbours(Xb, labels, k, 3)
        assert e.value.code == ERR_NAN
        with pytest.raises(ValueError):
            P.group_neighbours(Xb, labels, 3)
    # one +inf feature alone makes infinite distances, which are values like any other
    Xb = X.copy()
    Xb[i1, 3] = np.inf
    assert_same(device_form(ctx, Xb, labels, k, 3, SYMMETRIC), contract(P.pairwise_distances(Xb, Xb), labels, k, 3), "inf")
    # a NaN that only pairs inside one group meet is no m(i, c)
    Xn = X[:50].copy()
    Xn[3, 0] = np.nan
    idx, _, _, _ = ctx.group_neighbours(Xn, np.zeros(50, int), 2, 1)
    assert (idx == -1).all()
    for kwargs in (dict(labels=np.where(np.arange(900) == 77, k, labels)), dict(queries=np.array([0, k]))):
        with pytest.raises(bliss.BlissGpuError) as e:
            ctx.group_neighbours(X, kwargs.get("labels", labels), k, 3, queries=kwargs.get("queries"))
        assert e.value.code == ERR_INVALID
    # the workspace limit: D [k][k] of 600 groups does not fit 1 MiB -> BLISSGPU_ERR_OOM before anything is launched
    limit = ctx.workspace_limit()
    try:
        ctx.set_workspace_limit(1 << 20)
        with pytest.raises(bliss.BlissGpuError) as e:
            ctx.group_neighbours(X[:600], np.arange(600), 600, 3)
        assert e.value.code == ERR_OOM
        # ... and a forced slab that does not fit is refused too
        with pytest.raises(bliss.BlissGpuError) as e:
            ctx.group_neighbours(np.zeros((60000, 23), np.float32), np.arange(60000) % 7, 7, 3, slab_groups=7)
        assert e.value.code == ERR_OOM
    finally:
        ctx.set_workspace_limit(limit)
    # the context is as good as before
    assert_same(device_form(ctx, X, labels, k, 3, SYMMETRIC), want, "afterwards")


def test_stale_workspace(ctx, ordered):
    """a large call, a small one, then the large one again: the same bits"""
    X, labels, k, _ = ordered
    rng = np.random.default_rng(35)
    first = device_form(ctx, X, labels, k, 4, SYMMETRIC, slab=3)
    device_form(ctx, rng.standard_normal((130, 64)).astype(np.float32), rng.integers(0, 3, 130), 3, 2, DIRECTED, slab=2)
    again = device_form(ctx, X, labels, k, 4, SYMMETRIC, slab=3)
    for u, v in zip(first, again):
        assert u.tobytes() == v.tobytes()


def test_launches(ctx, ordered):
    X, labels, k, _ = ordered
    sort = {"kmeans_hist_kernel", "kmeans_scan_tiles_kernel", "kmeans_scan_add_kernel", "kmeans_scatter_kernel"}
    ctx.profile_enable(True)
    try:
        for slab, passes in ((0, 1), (3, 3), (1, 7)):
            ctx.profile_reset()
            device_form(ctx, X, labels, k, 3, SYMMETRIC, slab=slab)
            prof = {name: v[1] for name, v in ctx.profile().items() if v[1]}
            print(slab, prof)
            assert prof["chamfer_scan_kernel"] == passes and prof["chamfer_reduce_kernel"] == passes and prof["chamfer_select_kernel"] == 1
            assert not [name for name in prof if name.startswith(("pairwise", "set_distance", "radix_", "knn_"))]
            assert set(prof) == sort | {"chamfer_scan_kernel", "chamfer_reduce_kernel", "chamfer_select_kernel"}
    finally:
        ctx.profile_enable(False)


# ---- what the distance means ----
def test_a_bimodal_artist_is_nearest_to_the_other_bimodal_artist(bliss):
    """Six artists of 80 songs with unit noise: 0 and 1 have two styles, half their songs at +5 e0 and half at -5 e0 (and sit
    at +1 / -1 along e1), 2 sits at the origin, 3 .. 5 are far away.  The set distance pairs the two bimodal artists; the
    distance of mean vectors -- what nearest_albums ranks by -- puts each of them next to the origin artist, who sounds like
    neither of their styles.  (Without the offset along e1 the three means would coincide up to noise.)"""
    rng = np.random.default_rng(2)
    X = rng.standard_normal((480, 23))
    labels = np.repeat(np.arange(6), 80)
    for a, side in ((0, 1.0), (1, -1.0)):
        rows = np.flatnonzero(labels == a)
        X[rows[:40], 0] += 5.0
        X[rows[40:], 0] -= 5.0
        X[rows, 1] += side
    for a in (3, 4, 5):
        X[labels == a, a] += 40.0
    X = X.astype(np.float32)
    perm = rng.permutation(480)
    X, labels = X[perm], labels[perm]
    r = bliss.playlist.group_neighbours(X, labels, 2)
    assert r.idx[0].tolist() == [1, 2] and r.idx[1].tolist() == [0, 2] and r.sizes.tolist() == [80] * 6
    assert r.dist[0, 0] == r.dist[1, 0] and r.dist[0, 1] - r.dist[0, 0] > 0.5
    means = np.stack([X[labels == a].astype(np.float64).mean(axis=0) for a in range(6)])
    md = np.sqrt(((means[:, None] - means[None]) ** 2).sum(axis=2))
    np.fill_diagonal(md, np.inf)
    assert md.argmin(axis=1)[:2].tolist() == [2, 2] and md[0, 1] - md[0, 2] > 0.5
    # directed: the origin artist is covered badly by an artist whose songs all sit 5 away
    rd = bliss.playlist.group_neighbours(X, labels, 1, queries=[2], mode="directed", matrix=True)
    assert rd.matrix[2, 0] > 4.0 and rd.idx.shape == (1, 1)


# ---- the library ----
def test_library_similar_artists_round_trip(bliss, tmp_path):
    rng = np.random.default_rng(39)
    n = 150
    names = [f"artist{j}" for j in range(7)]
    who = rng.integers(0, 7, n)
    centres = (2.0 * rng.standard_normal((7, 23))).astype(np.float32)
    X = (centres[who] + 0.3 * rng.standard_normal((n, 23))).astype(np.float32)
    V2 = bliss.FeaturesVersion.Version2
    songs = [bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist=None if i % 11 == 5 else names[who[i]],
                        album=f"album {i % 4}", disc_number=1 + i % 2, track_number=n - i, duration=1.0, genre="g",
                        analysis=bliss.Analysis(X[i], V2), features_version=V2) for i in range(n)]
    db = str(tmp_path / "bliss.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs)
    Xdb = bliss.library.load_feature_matrix(db)[2]
    code, labels = {}, []
    for s in songs:
        labels.append(-1 if s.artist is None else code.setdefault(s.artist, len(code)))
    keys = list(code)
    want = bliss.playlist.group_neighbours(Xdb, np.asarray(labels), 3, k=len(keys))
    sim = bliss.library.similar_artists(db, 3)
    assert list(sim) == keys
    for g, key in enumerate(keys):
        assert sim[key] == [(keys[int(c)], float(v)) for c, v in zip(want.idx[g], want.dist[g])]
    target = keys[2]
    pl = bliss.library.similar_artists_playlist(db, target, 2)
    order = [target] + [name for name, _ in sim[target][:2]]
    assert [s.artist for s in pl] == [a for a in order for _ in range(sum(s.artist == a for s in songs))]
    for a in order:
        part = [s for s in pl if s.artist == a]
        assert [(s.album, s.disc_number, s.track_number) for s in part] == sorted((s.album, s.disc_number, s.track_number) for s in part)
    sim_d = bliss.library.similar_groups(db, 2, "artist", mode="directed")
    want_d = bliss.playlist.group_neighbours(Xdb, np.asarray(labels), 2, k=len(keys), mode="directed")
    assert [[name for name, _ in sim_d[key]] for key in keys] == [[keys[int(c)] for c in row] for row in want_d.idx]


# ---- the host form's staging: every optional argument given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("queries,sizes,matrix", ((True, True, True), (False, False, False), (True, False, True), (False, True, False)))
def test_host_form_stages_like_the_device_form(bliss, ctx, queries, sizes, matrix):
    import staging_cases as sc

    K, T = 6, 2

    def build(c, dev):
        q = c.G if queries else K
        idx, dist = dev(sc.out((q, T), np.uint32)), dev(sc.out((q, T), np.float64))
        sz, mat = dev(sc.out((K,), np.uint32, sizes)), dev(sc.out((K, K), np.float64, matrix))
        qs = (np.arange(c.G) * 5 % K).astype(np.uint32) if queries else None
        return [dev(c.X), c.n, sc.D, dev((np.arange(c.n) % K).astype(np.uint32)), K, 2, dev(c.M), dev(qs), c.G, T, 0, 0, idx, dist, sz,
                mat], [idx, dist, sz, mat]

    sc.check(bliss, ctx, "group_neighbours", build, lists=False)
