"""GPU tests of the library moments (blissgpu_moments / blissgpu_moments_device) and the covariance metrics built on them:
every output bit for bit against a numpy restatement of the contract of include/blissgpu.h (the blocked f64 sum), the error
paths, the planted-genre check of the metric, and the library layer end to end."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 256
ERR_INVALID, ERR_NAN = 2, 5


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


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- the contract in numpy: the vectorised form, 256 sequential steps over all blocks at once ----
def blocked_sum(T):
    """B over axis 0 of the f64 terms T [m, w] -> [w]"""
    T = np.asarray(T, np.float64)
    w = T.shape[1]
    while True:
        m = T.shape[0]
        nb = max(1, -(-m // BLOCK))
        pad = np.zeros((nb * BLOCK, w))  # (+0.0 terms behind the end change nothing: a block sum is never -0.0)
        pad[:m] = T
        blocks = pad.reshape(nb, BLOCK, w)
        acc = np.zeros((nb, w))
        for j in range(BLOCK):
            acc = acc + blocks[:, j]
        if nb == 1:
            return acc[0]
        T = acc


def reference(X, labels, k):
    """-> counts u32 [k], mean f64 [k, d], m2 f64 [k, d], min f32, max f32, S f64 [d, d]"""
    n, d = X.shape
    lab = np.zeros(n, np.int64) if labels is None else np.asarray(labels, np.int64)
    Xd = X.astype(np.float64)
    counts = np.bincount(lab, minlength=k).astype(np.uint32)
    mean, m2 = np.zeros((k, d)), np.zeros((k, d))
    mn, mx = np.full((k, d), np.inf, np.float32), np.full((k, d), -np.inf, np.float32)
    for g in np.flatnonzero(counts):
        rows = np.flatnonzero(lab == g)  # ascending
        mean[g] = blocked_sum(Xd[rows]) / np.float64(counts[g])
        u = Xd[rows] - mean[g]
        m2[g] = blocked_sum(u * u)
        mn[g], mx[g] = X[rows].min(axis=0), X[rows].max(axis=0)
    U = Xd - mean[lab]
    iu, ju = np.triu_indices(d)
    S = np.zeros((d, d))
    for c0 in range(0, iu.size, 256):  # (the pairs in chunks: n x 2080 products do not have to exist at once)
        i, j = iu[c0:c0 + 256], ju[c0:c0 + 256]
        v = blocked_sum(U[:, i] * U[:, j])
        S[i, j] = v
        S[j, i] = v
    return counts, mean, m2, mn, mx, S


def make_x(rng, n, d):
    """standard normal times per-feature scales over 1e-3 .. 1e3, one feature offset by 100 so that centring matters"""
    X = rng.standard_normal((n, d)) * np.logspace(-3, 3, d)[None, :]
    X[:, min(2, d - 1)] += 100.0
    return X.astype(np.float32)


def make_labels(rng, n, case):
    """-> (labels or None, k)"""
    if case == "none":
        return None, 1
    if case == "k3":  # group 1 is empty, group 2 is a single row
        lab = np.zeros(n, np.int64)
        lab[int(rng.integers(0, n))] = 2
        return lab, 3
    if case == "g256":  # groups of exactly 256 and 257 members, scattered; the rest in group 3; group 2 empty
        lab = np.full(n, 3, np.int64)
        pick = rng.permutation(n)[:513]
        lab[pick[:256]] = 0
        lab[pick[256:]] = 1
        return lab, 4
    if case == "kbig":  # more groups than rows
        return rng.integers(0, 2 * n + 90, n), 2 * n + 90
    raise AssertionError(case)


@functools.lru_cache(maxsize=None)
def case_data(n, d, case):
    rng = np.random.default_rng(1000 * d + n + len(case))
    X = make_x(rng, n, d)
    labels, k = make_labels(rng, n, case)
    return X, labels, k, reference(X, labels, k)


def host_form(bliss, X, labels, k, scatter=True):
    mo = bliss.playlist.moments(X, labels, k, scatter)
    return mo.counts.astype(np.uint32), mo.mean, mo.m2, mo.min, mo.max, mo.scatter


def device_form(ctx, X, labels, k, scatter=True):
    import torch

    out = ctx.moments(torch.from_numpy(X).cuda(), None if labels is None else torch.from_numpy(np.asarray(labels, np.int64)).cuda(), k, scatter)
    return tuple(None if t is None else t.cpu().numpy() for t in out)


NAMES = ("counts", "mean", "m2", "min", "max", "S")


def assert_same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        if w is None or g is None:
            assert g is None and w is None, (what, name)
            continue
        g = np.asarray(g)
        if name == "counts":
            assert np.array_equal(g.astype(np.int64), w.astype(np.int64)), (what, name)
        else:
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
            bad = np.flatnonzero(bits(g).reshape(-1) != bits(w).reshape(-1))
            assert bad.size == 0, (what, name, bad[:5], g.reshape(-1)[bad[:5]], w.reshape(-1)[bad[:5]])


SMALL, LARGE, DIMS = (1, 255, 256, 257), (65536, 65537), (1, 20, 23, 64)
CASES = ([(n, d, c) for n in SMALL for d in DIMS for c in ("none", "k3")] + [(255, d, "kbig") for d in DIMS]
         + [(n, d, c) for n in LARGE for d in DIMS for c in ("none", "k3", "g256")])


@pytest.mark.parametrize("n,d,case", CASES)
def test_moments_against_the_contract(bliss, ctx, n, d, case):
    X, labels, k, want = case_data(n, d, case)
    what = f"n={n} d={d} {case}"
    for rep in range(2):  # twice each: identical bits
        assert_same(host_form(bliss, X, labels, k), want, what + f" host {rep}")
        assert_same(device_form(ctx, X, labels, k), want, what + f" device {rep}")
    S = want[5]
    assert np.array_equal(bits(S), bits(S.T))


def test_the_blocked_sum_is_not_a_sequential_sum():
    """the reference itself: the blocked order and one sequential sum differ on the squared deviations of this data, so the bit
    test can tell them apart.  (The sums of x themselves are exact in f64 at these sizes, whatever the order: float32 terms of
    one scale.  m2 and S are where the order shows.)"""
    X = make_x(np.random.default_rng(5), 65537, 23).astype(np.float64)
    T = (X - X.mean(axis=0)) ** 2
    seq = np.zeros(23)
    for row in T[:2000]:
        seq = seq + row
    assert (bits(blocked_sum(T[:2000])) != bits(seq)).any()
    assert np.array_equal(bits(blocked_sum(T[:256])), bits(functools.reduce(lambda a, r: a + r, T[:256], np.zeros(23))))
    assert np.allclose(blocked_sum(T), T.sum(axis=0), rtol=1e-12)


def test_scatter_is_symmetric_and_optional(bliss, ctx):
    X, labels, k, want = case_data(65537, 23, "g256")
    full = device_form(ctx, X, labels, k, True)
    assert np.array_equal(bits(full[5]), bits(full[5].T))
    none = device_form(ctx, X, labels, k, False)
    assert none[5] is None
    assert_same(none, want[:5] + (None,), "S is NULL, device")
    assert_same(host_form(bliss, X, labels, k, False), want[:5] + (None,), "S is NULL, host")
    # the optional outputs of the C ABI: NULL m2 / min / max leave the others as they are
    from bliss_rs_amd import _ffi

    lab = np.ascontiguousarray(labels, np.uint32)
    counts, mean, S = np.zeros(k, np.uint32), np.zeros((k, 23)), np.zeros((23, 23))
    _ffi.check(_ffi.lib().blissgpu_moments(X.ctypes.data, X.shape[0], 23, lab.ctypes.data, k, counts.ctypes.data, mean.ctypes.data, None,
                                           None, None, S.ctypes.data))
    assert np.array_equal(counts, want[0]) and np.array_equal(bits(mean), bits(want[1])) and np.array_equal(bits(S), bits(want[5]))


def test_no_rows(bliss, ctx):
    X = np.zeros((0, 23), np.float32)
    for got in (host_form(bliss, X, None, 1), device_form(ctx, X, None, 1), device_form(ctx, X, np.zeros(0, np.int64), 3)):
        counts, mean, m2, mn, mx, S = got
        assert not counts.any() and not mean.any() and not m2.any() and not S.any()
        assert (mn == np.inf).all() and (mx == -np.inf).all()


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_values_that_are_not_finite_are_refused(bliss, ctx, value):
    X, labels, k, _ = case_data(257, 23, "k3")
    X = X.copy()
    X[200, 7] = value
    for lab, kk in ((labels, k), (None, 1)):
        with pytest.raises(bliss._ffi.BlissGpuError) as e:
            device_form(ctx, X, lab, kk)
        assert e.value.code == ERR_NAN
        with pytest.raises(ValueError):
            host_form(bliss, X, lab, kk)


def test_a_label_past_k_is_refused_on_the_device(bliss, ctx):
    X, labels, k, want = case_data(65537, 23, "g256")
    for where in (0, 40000, 65536):
        bad = labels.copy()
        bad[where] = k
        for scatter in (True, False):
            with pytest.raises(bliss._ffi.BlissGpuError) as e:
                device_form(ctx, X, bad, k, scatter)
            assert e.value.code == ERR_INVALID and "label" in str(e.value)
    assert_same(device_form(ctx, X, labels, k), want, "after the refused calls")  # the context is as good as before


# ---- the planted check: genres that differ only along low-variance directions, hidden by five loud ones and a rotation ----
@pytest.fixture(scope="module")
def planted():
    rng = np.random.default_rng(5)
    d, K, n = 23, 6, 900
    std = np.full(d, 0.3)
    std[:5] = 5.0
    R = np.linalg.qr(rng.standard_normal((d, d)))[0]
    cent = np.zeros((K, d))
    cent[:, 5:] = rng.standard_normal((K, d - 5))
    lab = rng.integers(0, K, n)
    X = ((cent[lab] + rng.standard_normal((n, d)) * std) @ R.T).astype(np.float32)
    return X, lab


def test_planted_genres_are_recovered_by_the_within_covariance(bliss, planted):
    P = bliss.playlist
    X, lab = planted
    triplets = P.triplets_from_labels(lab, 4000, 1)
    within = P.covariance_metric(X, lab)
    total = P.covariance_metric(X)
    acc_id = P.triplet_accuracy(X, triplets)
    acc_total = P.triplet_accuracy(X, triplets, total.m)
    acc_within = P.triplet_accuracy(X, triplets, within.m)
    print(f"triplet accuracy: identity {acc_id:.4f}, total covariance {acc_total:.4f}, within-genre covariance {acc_within:.4f}")
    assert acc_within >= 0.95
    assert acc_id <= 0.75
    assert acc_total > acc_id
    assert within.dof == 900 - 6 and total.dof == 899
    assert abs(float(np.trace(within.m.astype(np.float64))) - 23.0) < 1e-4 and np.array_equal(within.m, within.m.T)
    sil_m = P.silhouette(X, lab, within.builder()).score
    sil_e = P.silhouette(X, lab).score
    print(f"silhouette: euclidean {sil_e:.4f}, within-genre covariance {sil_m:.4f}")
    assert sil_m > sil_e
    # the metric is the inverse covariance: f64 numpy agrees to what float32 keeps
    Xd = X.astype(np.float64)
    U = Xd - np.stack([Xd[lab == g].mean(axis=0) for g in range(6)])[lab]
    Cw = U.T @ U / within.dof
    Cw = 0.99 * Cw + 0.01 * np.trace(Cw) / 23 * np.eye(23)
    W = np.linalg.inv(Cw)
    W *= 23 / np.trace(W)
    assert np.abs(within.m - W).max() <= 1e-5 * np.abs(W).max()


def test_library_layer_end_to_end(bliss, planted, tmp_path):
    P, Lb = bliss.playlist, bliss.library
    X, lab = planted
    X, lab = X[:300], lab[:300]
    genres = ["rock", "jazz", "ambient", "folk", "metal", "soul"]
    V2 = bliss.FeaturesVersion.Version2
    songs = [bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist=f"artist{i % 9}", album=f"album {i % 30:02d}", duration=1.0,
                        genre=None if i % 10 == 7 else genres[lab[i]], analysis=bliss.Analysis(X[i], V2), features_version=V2)
             for i in range(300)]
    db = str(tmp_path / "bliss.db")
    Lb.create_schema(db)
    Lb.store_songs(db, songs)
    Xdb = Lb.load_feature_matrix(db)[2]
    tagged = np.array([s.genre is not None for s in songs])
    code = {}
    glab = np.array([-1 if s.genre is None else code.setdefault(s.genre, len(code)) for s in songs])
    # statistics
    mo = P.moments(Xdb, None, None, False)
    stats = Lb.statistics(db)
    for r in range(23):
        row = stats[bliss.AnalysisIndex(r).name]
        assert (row["mean"], row["std"], row["min"], row["max"], row["count"]) == (
            float(mo.mean[0, r]), float(mo.std[0, r]), float(mo.min[0, r]), float(mo.max[0, r]), 300)
        assert abs(row["mean"] - float(Xdb[:, r].astype(np.float64).mean())) <= 1e-12 * max(1.0, abs(row["mean"]))
    mg = P.moments(Xdb[tagged], glab[tagged], len(code), False)
    by = Lb.statistics(db, "genre")
    assert list(by) == list(code)
    for tag, g in code.items():
        assert by[tag]["Tempo"] == {"mean": float(mg.mean[g, 0]), "std": float(mg.std[g, 0]), "min": float(mg.min[g, 0]),
                                    "max": float(mg.max[g, 0]), "count": int(mg.counts[g])}
    # covariance_metric: total, by genre (NULL tags left out), by a label array, by a Clustering
    assert np.array_equal(bits(Lb.covariance_metric(db)), bits(P.covariance_metric(Xdb).m))
    want = P.covariance_metric(Xdb, glab)
    assert np.array_equal(bits(Lb.covariance_metric(db, "genre")), bits(want.m))
    assert np.array_equal(bits(Lb.covariance_metric(db, glab, "diagonal", 0.1)), bits(P.covariance_metric(Xdb, glab, "diagonal", 0.1).m))
    res = Lb.covariance_metric(db, "genre", return_result=True)
    assert res.dof == int(tagged.sum()) - len(code) and np.array_equal(bits(res.scatter), bits(want.scatter))
    clustering = P.Clustering(*P.kmeans(Xdb, P.kmeans_init(Xdb, 4, 1)))
    assert np.array_equal(bits(Lb.covariance_metric(db, clustering)), bits(P.covariance_metric(Xdb, clustering.labels).m))


# ---- the host form's staging: every optional argument given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("labels,m2,extrema,scatter", ((True, True, True, True), (False, False, False, False), (True, False, True, False),
                                                       (True, True, False, True), (False, True, True, False)))
def test_host_form_stages_like_the_device_form(bliss, ctx, labels, m2, extrema, scatter):
    import staging_cases as sc

    def build(c, dev):
        k = 4 if labels else 1
        counts, mean = dev(sc.out((k,), np.uint32)), dev(sc.out((k, sc.D), np.float64))
        s2, S = dev(sc.out((k, sc.D), np.float64, m2)), dev(sc.out((sc.D, sc.D), np.float64, scatter))
        mn, mx = dev(sc.out((k, sc.D), np.float32, extrema)), dev(sc.out((k, sc.D), np.float32, extrema))
        lab = (np.arange(c.n) % k).astype(np.uint32) if labels else None
        return [dev(c.X), c.n, sc.D, dev(lab), k, counts, mean, s2, mn, mx, S], [counts, mean, s2, mn, mx, S]

    sc.check(bliss, ctx, "moments", build, lists=False)
