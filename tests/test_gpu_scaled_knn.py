"""GPU tests (-m gpu) of the locally scaled k-nearest search and the k-occurrence counts (blissgpu_scaled_knn /
blissgpu_knn_occurrence and their _device forms: scaled_knn_scan_kernel + knn_merge_kernel, knn_occurrence_kernel; DESIGN.md
3.27).  The expected values come from the CPU oracle's distance matrix (oracle.pairwise), the float32 numpy expression of the
contract -- dist / sqrt(f32(qscale[i] * cscale[j])) -- and numpy's stable argsort, never from the code under test.  Every
comparison is exact: np.array_equal on indices, bit equality on the scaled distances, ties at the cut included."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ("euclidean", "cosine", "weights", "spd")
INVALID, NAN = 2, 5


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


def tie_rich(rng, n, d):
    """features on a grid of eighths (many equal distances), 5 % of the rows copies of other rows"""
    X = (rng.integers(-8, 9, (n, d)) / 8).astype(np.float32)
    dup = rng.choice(n, n // 20, replace=False)
    X[dup] = X[rng.integers(0, n, n // 20)]
    return X


def scaled_matrix(Dm, qs, cs):
    """the contract in float32 numpy: the product rounded once, the correctly rounded root, true division"""
    prod = np.asarray(qs, np.float32)[:, None] * np.asarray(cs, np.float32)[None, :]
    assert prod.dtype == np.float32
    r = np.sqrt(prod)
    S = np.asarray(Dm, np.float32) / r
    assert r.dtype == np.float32 and S.dtype == np.float32
    return S


def expected_from_matrix(Sm, k, skip=None):
    """rows of a (scaled) distance matrix -> (idx int64[q, k], dist f32[q, k]): stable ascending order without the skipped
    column, cut after k, padded with -1 / inf (expected_from_matrix of tests/test_gpu_knn.py)"""
    q, n = Sm.shape
    idx = np.full((q, k), -1, np.int64)
    dist = np.full((q, k), np.inf, np.float32)
    for i in range(q):
        order = np.argsort(Sm[i], kind="stable")
        if skip is not None and skip[i] >= 0:
            order = order[order != skip[i]]
        order = order[:k]
        idx[i, :order.size] = order
        dist[i, :order.size] = Sm[i, order]
    return idx, dist


def host_form(bliss, Q, qs, X, cs, k, metric, M, skip=None):
    return bliss.playlist.scaled_nearest_order(Q, qs, X, cs, k, metric, M, skip)


def device_form(ctx, Q, qs, X, cs, k, metric, M, skip=None):
    import torch

    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()  # noqa: E731
    idx, dist = ctx.scaled_knn(t(Q, np.float32), t(qs, np.float32), t(X, np.float32), t(cs, np.float32), k, metric,
                               t(M, np.float32), t(skip, np.int32))
    ctx.synchronize()
    return idx.cpu().numpy().astype(np.int64), dist.cpu().numpy()


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "indices", int((got[0] != want[0]).any(axis=1).sum()), "rows differ")
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (what, "distance bits")


def check_both(bliss, ctx, Q, qs, X, cs, k, metric, M, skip=None, what="", want=None, Sm=None, oracle=None):
    if want is None:
        if Sm is None:
            Sm = scaled_matrix(oracle.pairwise(Q, X, metric, M, n_threads=16), qs, cs)
        want = expected_from_matrix(Sm, k, skip)
    assert_same(host_form(bliss, Q, qs, X, cs, k, metric, M, skip), want, (what, "host form"))
    assert_same(device_form(ctx, Q, qs, X, cs, k, metric, M, skip), want, (what, "device form"))
    return want


def mixed_ties(Dm, Sm, cs, rows):
    """how many scaled distances of those rows are reached by more than one (distance, candidate scale) pair"""
    return sum(int(len({(Dm[r, c], cs[c]) for c in np.flatnonzero(Sm[r] == v)}) > 1) for r in rows for v in np.unique(Sm[r]))


# ---- (a) tie-rich data: distinct (distance, scale) pairs with equal scaled distances; a filter that discards too much shows here ----
@pytest.mark.parametrize("d", (23, 20))
@pytest.mark.parametrize("name", METRICS)
def test_tie_rich_against_oracle(bliss, ctx, oracle, d, name):
    rng = np.random.default_rng(1)
    n = 700
    X = tie_rich(rng, n, d)
    Q = tie_rich(rng, 200, d)
    cs = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), n)
    qs = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), 200)
    metric, M = _metric(oracle, name, d)
    Dm = oracle.pairwise(Q, X, metric, M, n_threads=16)
    Sm = scaled_matrix(Dm, qs, cs)
    if name == "euclidean":  # on the oracle alone: equal scaled distances from different (distance, scale) pairs do occur
        s = np.sort(Sm, axis=1, kind="stable")
        ties = int((s[:, 31] == s[:, 32]).sum())
        mixed = mixed_ties(Dm, Sm, cs, range(20))
        print(f"d={d}: {ties} of 200 queries tie at the cut k=32; {mixed} scaled distances of the first 20 rows come from "
              "more than one (distance, scale) pair")
        assert ties >= 5 and mixed >= 20
    for k in (1, 10, 32):
        check_both(bliss, ctx, Q, qs, X, cs, k, metric, M, what=(d, name, k), want=expected_from_matrix(Sm, k))


# ---- (b) continuous data, ragged blocks, scales over 40 octaves and at both ends of the accepted range ----
@pytest.mark.parametrize("n", (1, 255, 256, 257, 513))
def test_continuous_data_and_ragged_blocks(bliss, ctx, oracle, n):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((n, 23)).astype(np.float32)
    Q = rng.standard_normal((37, 23)).astype(np.float32)
    cs = np.exp2(rng.uniform(-20, 20, n)).astype(np.float32)
    qs = np.exp2(rng.uniform(-20, 20, 37)).astype(np.float32)
    cs[::97] = np.float32(2.0 ** -60)
    cs[n // 2::101] = np.float32(2.0 ** 60)
    qs[3], qs[5] = np.float32(2.0 ** -60), np.float32(2.0 ** 60)
    for name in ("euclidean", "cosine", "weights"):
        metric, M = _metric(oracle, name, 23)
        check_both(bliss, ctx, Q, qs, X, cs, min(8, n + 2), metric, M, what=(n, name), oracle=oracle)


# ---- (c) all scales 1: blissgpu_knn on the same inputs, bit for bit ----
def test_unit_scales_equal_knn(bliss, ctx, oracle):
    rng = np.random.default_rng(4)
    X, Q = tie_rich(rng, 900, 23), tie_rich(rng, 64, 23)
    one_q, one_c = np.ones(64, np.float32), np.ones(900, np.float32)
    for name in METRICS:
        metric, M = _metric(oracle, name, 23)
        plain = bliss.playlist.nearest_order(Q, X, 32, metric, M)
        assert_same(host_form(bliss, Q, one_q, X, one_c, 32, metric, M), plain, (name, "host form"))
        assert_same(device_form(ctx, Q, one_q, X, one_c, 32, metric, M), plain, (name, "device form"))


# ---- (d) the generic feature count ----
@pytest.mark.parametrize("d", (7, 64))
def test_generic_feature_count(bliss, ctx, oracle, d):
    rng = np.random.default_rng(5)
    X, Q = tie_rich(rng, 600, d), tie_rich(rng, 50, d)
    cs = rng.choice(np.array([0.5, 1.0, 2.0, 3.0], np.float32), 600)
    qs = rng.choice(np.array([0.5, 1.0, 2.0, 3.0], np.float32), 50)
    for name in ("euclidean", "cosine", "spd"):
        metric, M = _metric(oracle, name, d)
        Sm = scaled_matrix(oracle.pairwise(Q, X, metric, M, n_threads=16), qs, cs)
        for k in (1, 32):
            check_both(bliss, ctx, Q, qs, X, cs, k, metric, M, what=(d, name, k), want=expected_from_matrix(Sm, k))


# ---- (e) large k (the compaction path, one workgroup per CU) and the split path (few queries, at least nine blocks) ----
def test_large_k(bliss, ctx, oracle):
    rng = np.random.default_rng(6)
    X, Q = tie_rich(rng, 1500, 23), tie_rich(rng, 5, 23)
    cs = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), 1500)
    qs = np.array([0.5, 1.0, 2.0, 1.0, 0.5], np.float32)
    for name in ("euclidean", "cosine"):
        metric, M = _metric(oracle, name, 23)
        check_both(bliss, ctx, Q, qs, X, cs, 1024, metric, M, what=("k = 1024", name), oracle=oracle)


def test_split_path(bliss, ctx, oracle):
    rng = np.random.default_rng(7)
    X, Q = tie_rich(rng, 2305, 23), tie_rich(rng, 3, 23)
    cs = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), 2305)
    qs = np.array([2.0, 1.0, 0.5], np.float32)
    for name in METRICS:
        metric, M = _metric(oracle, name, 23)
        Sm = scaled_matrix(oracle.pairwise(Q, X, metric, M, n_threads=16), qs, cs)
        for k in (1, 32, 300):
            check_both(bliss, ctx, Q, qs, X, cs, k, metric, M, what=("split", name, k), want=expected_from_matrix(Sm, k))


# ---- (f) skip and padding ----
def test_skip_and_padding(bliss, ctx, oracle):
    rng = np.random.default_rng(8)
    n = 300
    X = tie_rich(rng, n, 23)
    X[17] = X[5]
    sc = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), n)
    me = np.arange(n, dtype=np.int64)
    Sm = scaled_matrix(oracle.pairwise(X, X, "euclidean", None, n_threads=16), sc, sc)
    # every song skipping itself with k = n: every row ends in one padding entry
    want = check_both(bliss, ctx, X, sc, X, sc, n, "euclidean", None, skip=me, what="k = n, self skipped",
                      want=expected_from_matrix(Sm, n, me))
    assert (want[0][:, n - 1] == -1).all() and np.isinf(want[1][:, n - 1]).all() and (want[0][:, :n - 1] >= 0).all()
    assert not (want[0] == me[:, None]).any() and want[0][5, 0] == 17 and want[1][5, 0] == 0.0
    # the same array objects as queries / candidates and as both scales: the single-upload path of the host form
    assert_same(bliss.playlist.scaled_nearest_order(X, sc, X, sc, n, "euclidean", None, me), want, "shared arrays")
    # -1 (the library's 0xFFFFFFFF) skips nothing
    mixed = me.copy()
    mixed[::3] = -1
    check_both(bliss, ctx, X, sc, X, sc, 8, "euclidean", None, skip=mixed, what="mixed skip", want=expected_from_matrix(Sm, 8, mixed))
    # a skip >= n: the host layer refuses it, the library's host form and the device form return ERR_INVALID
    with pytest.raises(ValueError):
        host_form(bliss, X[:2], sc[:2], X, sc, 4, "euclidean", None, np.array([n, 0]))
    from bliss_rs_amd import _ffi

    p = lambda a: a.ctypes.data  # noqa: E731
    idx, bad = np.zeros((2, 4), np.uint32), np.array([n, 0], np.uint32)
    Q2, s2 = np.ascontiguousarray(X[:2]), np.ascontiguousarray(sc[:2])
    assert _ffi.lib().blissgpu_scaled_knn(p(Q2), 2, p(s2), p(X), n, p(sc), 23, 0, None, p(bad), 4, p(idx), None) == INVALID
    with pytest.raises(bliss.BlissGpuError) as e:
        device_form(ctx, X[:2], sc[:2], X, sc, 4, "euclidean", None, np.array([n, 0]))
    assert e.value.code == INVALID
    # q == 0 and n == 0 through the device form
    import torch

    z = torch.zeros((0, 23), device="cuda")
    zs = torch.zeros((0,), device="cuda")
    tX, ts = torch.from_numpy(X).cuda(), torch.from_numpy(sc).cuda()
    assert ctx.scaled_knn(z, zs, tX, ts, 4)[0].shape == (0, 4)
    i0, d0 = ctx.scaled_knn(tX[:3].contiguous(), ts[:3].contiguous(), z, zs, 4)
    assert (i0.cpu().numpy() == -1).all() and np.isinf(d0.cpu().numpy()).all()


# ---- (g) scales outside [2^-60, 2^60] ----
@pytest.mark.parametrize("where,value", (("cscale", 0.0), ("cscale", -1.0), ("cscale", np.nan), ("cscale", np.inf),
                                         ("cscale", 2.0 ** -61), ("qscale", 2.0 ** 61)))
def test_bad_scales_are_refused(bliss, ctx, where, value):
    rng = np.random.default_rng(9)
    X, Q = rng.standard_normal((600, 23)).astype(np.float32), rng.standard_normal((9, 23)).astype(np.float32)
    cs, qs = np.ones(600, np.float32), np.ones(9, np.float32)
    (cs if where == "cscale" else qs)[[555, 7][where == "qscale"]] = np.float32(value)
    with pytest.raises(bliss.BlissGpuError) as e:
        host_form(bliss, Q, qs, X, cs, 5, "euclidean", None)
    assert e.value.code == INVALID and "scales must lie" in str(e.value)
    with pytest.raises(bliss.BlissGpuError) as e:
        device_form(ctx, Q, qs, X, cs, 5, "euclidean", None)
    assert e.value.code == INVALID
    # (the neighbouring values are fine)
    cs[:], qs[:] = np.float32(2.0 ** -60), np.float32(2.0 ** 60)
    host_form(bliss, Q, qs, X, cs, 5, "euclidean", None)


# ---- (h) a NaN feature in an evaluated row ----
def test_nan_feature(bliss, ctx, oracle):
    rng = np.random.default_rng(10)
    X, Q = rng.standard_normal((700, 23)).astype(np.float32), rng.standard_normal((2, 23)).astype(np.float32)
    cs, qs = np.exp2(rng.integers(-3, 4, 700)).astype(np.float32), np.ones(2, np.float32)
    X[321, 4] = np.nan
    for metric in ("euclidean", "cosine"):
        with pytest.raises(ValueError):
            host_form(bliss, Q, qs, X, cs, 8, metric, None)
        with pytest.raises(bliss.BlissGpuError) as e:
            device_form(ctx, Q, qs, X, cs, 8, metric, None)
        assert e.value.code == NAN
    # a skipped pair is not evaluated
    skip = np.array([321])
    keep = np.arange(700) != 321
    want = expected_from_matrix(scaled_matrix(oracle.pairwise(Q[:1], X[keep], "euclidean", None, n_threads=16), qs[:1], cs[keep]), 8)
    want = (np.where(want[0] >= 321, want[0] + 1, want[0]), want[1])
    assert_same(host_form(bliss, Q[:1], qs[:1], X, cs, 8, "euclidean", None, skip), want, "skipped NaN, host form")
    assert_same(device_form(ctx, Q[:1], qs[:1], X, cs, 8, "euclidean", None, skip), want, "skipped NaN, device form")


# ---- (i) k-occurrence ----
def occurrence_both(bliss, ctx, idx, n):
    import torch

    host = bliss.playlist.k_occurrence(idx, n)
    dev = ctx.knn_occurrence(torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).cuda(), n)
    ctx.synchronize()
    assert host.dtype == np.int64 and dev.dtype == torch.int32
    assert np.array_equal(host, dev.cpu().numpy().astype(np.int64))
    return host


def test_knn_occurrence(bliss, ctx, oracle, monkeypatch):
    rng = np.random.default_rng(11)
    n = 700
    X = tie_rich(rng, n, 23)
    sc = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), n)
    idx, _ = host_form(bliss, X, sc, X, sc, 10, "euclidean", None, np.arange(n))
    assert np.array_equal(occurrence_both(bliss, ctx, idx, n), np.bincount(idx.ravel(), minlength=n))
    # the worst contention: every row lists the same 32 songs
    same = np.tile(rng.choice(5000, 32, replace=False), (4096, 1)).astype(np.int64)
    want = np.bincount(same.ravel(), minlength=5000)
    assert np.array_equal(occurrence_both(bliss, ctx, same, 5000), want) and want.max() == 4096
    # padding entries are ignored
    pad = same.copy()
    pad[::2, 20:] = -1
    pad[1, :] = -1
    assert np.array_equal(occurrence_both(bliss, ctx, pad, 5000), np.bincount(pad[pad >= 0], minlength=5000))
    # the other side of the A/B counts the same (windows of 8 192 songs: 20 000 songs are three of them)
    wide = rng.integers(0, 20_000, (3000, 7)).astype(np.int64)
    wide[::5, 3] = -1
    plain = occurrence_both(bliss, ctx, wide, 20_000)
    assert np.array_equal(plain, np.bincount(wide[wide >= 0], minlength=20_000))
    monkeypatch.setenv("BLISSGPU_OCCURRENCE_LDS", "1")
    assert np.array_equal(occurrence_both(bliss, ctx, wide, 20_000), plain)
    assert np.array_equal(occurrence_both(bliss, ctx, pad, 5000), np.bincount(pad[pad >= 0], minlength=5000))
    monkeypatch.delenv("BLISSGPU_OCCURRENCE_LDS")
    # an entry >= n that is not padding
    import torch

    bad = same.copy()
    bad[77, 5] = 5000
    with pytest.raises(bliss.BlissGpuError) as e:
        bliss.playlist.k_occurrence(bad, 5000)
    assert e.value.code == INVALID
    with pytest.raises(bliss.BlissGpuError) as e:
        ctx.knn_occurrence(torch.from_numpy(bad.astype(np.int32)).cuda(), 5000)
    assert e.value.code == INVALID
    # q == 0: zeros
    z = ctx.knn_occurrence(torch.zeros((0, 32), dtype=torch.int32, device="cuda"), 50)
    assert z.shape == (50,) and int(z.abs().sum()) == 0
    assert bliss.playlist.k_occurrence(np.zeros((0, 32), np.int64), 50).tolist() == [0] * 50
    h = bliss.playlist.hubness(idx, n)
    assert np.array_equal(h.counts, np.bincount(idx.ravel(), minlength=n)) and h.k == 10


# ---- (j) end to end on a temporary SQLite library ----
def test_library_end_to_end(bliss, oracle, tmp_path, monkeypatch):
    from bliss_rs_amd import _ffi

    rng = np.random.default_rng(12)
    n, k, m = 600, 10, 10
    X = tie_rich(rng, n, 23)
    V2 = bliss.FeaturesVersion.Version2
    songs = [bliss.Song(path=f"/music/{i:05d}.flac", title=f"t{i}", artist="a", duration=1.0, analysis=bliss.Analysis(X[i], V2),
                        features_version=V2) for i in range(n)]
    db = str(tmp_path / "bliss.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs)
    lib = _ffi.lib()
    calls = {"blissgpu_knn": 0, "blissgpu_scaled_knn": 0}

    def counted(name):
        real = getattr(lib, name)

        def f(*a):
            calls[name] += 1
            return real(*a)

        return f

    for name in calls:
        monkeypatch.setattr(lib, name, counted(name))
    table = bliss.library.similar_songs_scaled(db, k, m=m)
    assert calls == {"blissgpu_knn": 1, "blissgpu_scaled_knn": 1} and len(table) == n
    some = [f"/music/{i:05d}.flac" for i in (0, 7, 599)]
    part = bliss.library.similar_songs_scaled(db, k, m=m, song_paths=some)
    assert calls == {"blissgpu_knn": 2, "blissgpu_scaled_knn": 2} and sorted(part) == sorted(some)
    monkeypatch.undo()
    # the numpy pipeline: the oracle's matrix, the m nearest others, their f64 mean, the scaled stable order
    Dm = oracle.pairwise(X, X, "euclidean", None, n_threads=16)
    me = np.arange(n)
    near = expected_from_matrix(Dm, m, me)[1]
    scale = np.asarray([np.float32(sum(np.float64(v) for v in row) / m) for row in near], np.float32)
    floor = scale[scale >= np.float32(2.0 ** -60)].min()
    scale = np.where(scale < np.float32(2.0 ** -60), floor, scale).astype(np.float32)
    assert np.array_equal(bliss.playlist.local_scales(X, m).view(np.uint32), scale.view(np.uint32))
    want = expected_from_matrix(scaled_matrix(Dm, scale, scale), k, me)
    paths = [s.path for s in songs]
    for i in range(n):
        got = table[paths[i]]
        assert [p for p, _ in got] == [paths[j] for j in want[0][i]], i
        assert np.array_equal(np.asarray([v for _, v in got], np.float32).view(np.uint32), want[1][i].view(np.uint32)), i
    for p in some:
        assert part[p] == table[p]
    with pytest.raises(bliss.ProviderError):
        bliss.library.similar_songs_scaled(db, k, song_paths=["/music/none.flac"])
    counts = np.bincount(want[0].ravel(), minlength=n)
    h, hp = bliss.library.hubness(db, k, scaled=True, m=m)
    assert hp == paths and np.array_equal(h.counts, counts) and h.k == k
    assert h.skewness == bliss.playlist.Hubness.from_counts(counts, k).skewness
    assert bliss.library.orphan_songs(db, k, scaled=True, m=m) == [paths[i] for i in np.flatnonzero(counts == 0)]
    raw = np.bincount(expected_from_matrix(Dm, k, me)[0].ravel(), minlength=n)
    h_raw, _ = bliss.library.hubness(db, k)
    assert np.array_equal(h_raw.counts, raw)
    assert bliss.library.orphan_songs(db, k) == [paths[i] for i in np.flatnonzero(raw == 0)]


# ---- (k) the property the feature exists for, on the device ----
def test_local_scaling_removes_most_of_the_hubness(bliss):
    n, k, m = 1500, 10, 10
    X = np.random.default_rng(0).standard_normal((n, 23)).astype(np.float32)
    me = np.arange(n)
    raw, _ = bliss.playlist.nearest_order(X, X, k, "euclidean", None, me)
    scale = bliss.playlist.local_scales(X, m, "mean")
    scaled, _ = bliss.playlist.scaled_nearest_order(X, scale, X, scale, k, "euclidean", None, me)
    h_raw, h_scaled = bliss.playlist.hubness(raw, n), bliss.playlist.hubness(scaled, n)
    print(f"raw: skewness {h_raw.skewness:.2f}, {h_raw.orphans().size} orphans; scaled: {h_scaled.skewness:.2f}, "
          f"{h_scaled.orphans().size} orphans")
    assert h_scaled.skewness < 0.5 * h_raw.skewness
    assert h_scaled.orphans().size < 0.1 * h_raw.orphans().size


# ---- the host forms' staging: every optional argument given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("shared", (False, True))  # the queries ARE the candidates with the same scales: they travel once
@pytest.mark.parametrize("skip,dist", ((True, True), (False, False), (True, False), (False, True)))
def test_host_form_stages_like_the_device_form(bliss, ctx, skip, dist, shared):
    import staging_cases as sc

    def build(c, dev):
        q = c.n if shared else c.q
        cs = np.linspace(0.5, 2.0, c.n).astype(np.float32)
        X = dev(c.X)  # (one array for both roles in the shared case: the host form tells by the pointers)
        dcs = dev(cs)
        Q, qs = (X, dcs) if shared else (dev(c.Q), dev(np.linspace(0.7, 1.5, c.q).astype(np.float32)))
        sk = (np.arange(c.n, dtype=np.uint32) if shared else c.qskip) if skip else None
        idx, dd = dev(sc.out((q, c.k), np.uint32)), dev(sc.out((q, c.k), np.float32, dist))
        return [Q, q, qs, X, c.n, dcs, sc.D, 2, dev(c.M), dev(sk), c.k, idx, dd], [idx, dd]

    sc.check(bliss, ctx, "scaled_knn", build)


def test_knn_occurrence_host_form_stages_like_the_device_form(bliss, ctx):
    import staging_cases as sc

    def build(c, dev):
        idx = (np.arange(c.q * c.k, dtype=np.uint32) * 37 % c.n).reshape(c.q, c.k)
        idx[0, -1] = sc.NONE
        count = dev(sc.out((c.n,), np.uint32))
        return [dev(idx), c.q, c.k, c.n, count], [count]

    sc.check(bliss, ctx, "knn_occurrence", build, lists=False)
