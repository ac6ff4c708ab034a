"""GPU tests (-m gpu) of the duplicate search (blissgpu_duplicate_groups / blissgpu_duplicate_groups_device: dup_init_kernel,
dup_join_kernel, dup_flatten_kernel): the duplicate rule of dedup_playlist_custom_distance (src/playlist.rs:381-388) over every
pair i < j of a collection, and the connected components of those edges.

The expected values never come from the code under test: the CPU oracle's distance matrix (oracle.pairwise, bit-identical to
the device by contract) in row slabs, a strict `<` in NumPy, and the ten-line union-find below; at n = 10^5 the k-nearest
search (playlist.nearest_order, merged and tested on its own).  The result is discrete, so every comparison is exact:
np.array_equal on labels, equality on n_pairs, set equality on pairs, bit equality on pair_dist."""
import ctypes as C
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ("euclidean", "cosine", "weights", "spd")
THR = np.float32(0.05)


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
    """-> (library metric name, M or None), built as in tests/test_gpu_knn.py::_metric"""
    if name in ("euclidean", "cosine"):
        return name, None
    if name == "weights":
        return "mahalanobis", oracle.feature_weights(2 if d == 23 else 1) if d in (23, 20) else np.eye(d, dtype=np.float32)
    rng = np.random.default_rng(7)
    A = rng.standard_normal((d, d)) * 0.3
    return "mahalanobis", (A @ A.T + 0.1 * np.eye(d)).astype(np.float32)


# ---- the expected result ----
def components(n, I, J):
    """labels of the graph on n vertices with edges (I[e], J[e]): the smallest vertex of every vertex's component"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(I.tolist(), J.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)], np.int64)


def expected(oracle, X, metric, M, thr, meta=None):
    """-> (labels int64[n], pairs int64[e, 2] ascending, dist f32[e]) from the oracle's matrix in row slabs (at most 256 MB
    live); raises FloatingPointError for a NaN distance of a pair i < j"""
    n = X.shape[0]
    thr = np.float32(thr)
    slab = max(1, min(1024, (64 << 20) // max(n, 1)))  # (short slabs: little of the lower triangle is computed)
    I, J, V = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
    for r0 in range(0, n, slab):
        Dm = oracle.pairwise(X[r0:r0 + slab], X[r0:], metric, M, n_threads=16)  # column c is row r0 + c
        rows = Dm.shape[0]
        upper = np.arange(n - r0)[None, :] > np.arange(rows)[:, None]
        if np.isnan(Dm[upper]).any():
            raise FloatingPointError("NaN distance")
        e = (Dm < thr) & upper
        if meta is not None:
            mi, mj = meta[r0:r0 + rows, None], meta[None, r0:]
            e |= upper & (mi != 0) & (mi == mj)
        a, b = np.nonzero(e)  # row-major: ascending (i, j)
        I.append(a + r0)
        J.append(b + r0)
        V.append(Dm[a, b])
    I, J, V = np.concatenate(I), np.concatenate(J), np.concatenate(V)
    return components(n, I, J), np.stack([I, J], axis=1).astype(np.int64), V.astype(np.float32)


def has_non_clique(labels, pairs):
    """is some component of the EXPECTED result not a clique (so that the transitive closure matters)?"""
    sizes = np.bincount(labels, minlength=labels.size)
    edges = np.bincount(labels[pairs[:, 0]], minlength=labels.size)
    return bool((edges < sizes * (sizes - 1) // 2).any())


# ---- the two forms ----
def host_form(bliss, X, meta, metric, M, thr):
    return bliss.playlist.duplicate_labels(X, meta, metric, M, thr, return_pairs=True)


def device_form(ctx, X, meta, metric, M, thr, max_pairs):
    """-> (labels int64, n_pairs, pairs int64 sorted ascending, dist in the same order); max_pairs = 0: no pair buffer"""
    import torch

    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()  # noqa: E731
    out = ctx.duplicate_labels(t(X, np.float32), t(meta, np.int32), metric, t(M, np.float32), float(thr), max_pairs)
    ctx.synchronize()
    labels, n_pairs = out[0].cpu().numpy().astype(np.int64), int(out[1].item())
    if max_pairs <= 0 or n_pairs > max_pairs:
        return labels, n_pairs, None, None
    pairs, dist = out[2][:n_pairs].cpu().numpy().astype(np.int64), out[3][:n_pairs].cpu().numpy()
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    return labels, n_pairs, pairs[order], dist[order]


def assert_pairs(got_pairs, got_dist, want, what):
    assert got_pairs.shape == want[1].shape and np.array_equal(got_pairs, want[1]), (what, "pairs")
    assert np.array_equal(got_dist.view(np.uint32), want[2].view(np.uint32)), (what, "pair_dist bits")


def check_both(bliss, ctx, X, meta, metric, M, thr, want, what=""):
    lab, pairs, dist = host_form(bliss, X, meta, metric, M, thr)
    assert np.array_equal(lab, want[0]), (what, "host form", "labels", int((lab != want[0]).sum()))
    assert pairs.shape[0] == want[1].shape[0], (what, "host form", "n_pairs", pairs.shape[0], want[1].shape[0])
    assert_pairs(pairs, dist, want, (what, "host form"))  # as returned: the host form's list is in ascending (i, j)
    lab, n_pairs, pairs, dist = device_form(ctx, X, meta, metric, M, thr, max(want[1].shape[0], 1))
    assert np.array_equal(lab, want[0]), (what, "device form", "labels", int((lab != want[0]).sum()))
    assert n_pairs == want[1].shape[0], (what, "device form", "n_pairs", n_pairs, want[1].shape[0])
    assert_pairs(pairs, dist, want, (what, "device form"))


# ---- 1. planted chains ----
def planted(rng, n, d, thr=THR, every=50):
    """rows 0.5 N(0, 1) in f32; 2 % of the rows planted as chains of 6: base + t * 0.8 * threshold * u, u a random unit vector
    -> (X, chains int[n_chains, 6])"""
    X = (0.5 * rng.standard_normal((n, d))).astype(np.float32)
    n_chains = (n // every) // 6
    chains = rng.choice(n, n_chains * 6, replace=False).reshape(n_chains, 6)
    for ch in chains:
        u = rng.standard_normal(d)
        u /= np.linalg.norm(u)
        base = X[ch[0]].astype(np.float64)
        for t in range(6):
            X[ch[t]] = (base + t * 0.8 * float(thr) * u).astype(np.float32)
    return X, chains


def planted_threshold(oracle, X, chains, metric, M):
    """the threshold that makes the planted neighbours edges under this metric: 1 / 0.8 of their largest oracle distance
    (euclidean: the recipe's own 0.05)"""
    if metric == "euclidean":
        return THR
    a, b = chains[:, :-1].reshape(-1), chains[:, 1:].reshape(-1)
    step = np.array([oracle.pairwise(X[i:i + 1], X[j:j + 1], metric, M)[0, 0] for i, j in zip(np.minimum(a, b), np.maximum(a, b))])
    return np.float32(step.max() / np.float32(0.8))


@pytest.mark.parametrize("n", (3000, 12_001))
@pytest.mark.parametrize("d", (23, 20, 7, 64))
@pytest.mark.parametrize("name", METRICS)
def test_planted_chains(bliss, ctx, oracle, name, d, n):
    rng = np.random.default_rng(1)
    X, chains = planted(rng, n, d)
    metric, M = _metric(oracle, name, d)
    thr = planted_threshold(oracle, X, chains, metric, M)
    want = expected(oracle, X, metric, M, thr)
    n_edges, n_comp = want[1].shape[0], int((np.bincount(want[0], minlength=n) >= 2).sum())
    print(f"{name} d={d} n={n}: threshold {float(thr):.6g}, {n_edges} edges, {n_comp} components, {chains.shape[0]} chains planted")
    # on the expected result alone: the planted neighbours are edges, and the closure is exercised
    have = set(map(tuple, want[1].tolist()))
    for ch in chains:
        for t in range(5):
            assert (min(ch[t], ch[t + 1]), max(ch[t], ch[t + 1])) in have
    assert n_edges >= 5 * chains.shape[0]
    if name == "euclidean" and d >= 20:
        assert n_edges == 5 * chains.shape[0] and n_comp == chains.shape[0]  # n = 3000: 50 edges in 10 components of 6
    assert has_non_clique(want[0], want[1])
    check_both(bliss, ctx, X, None, metric, M, thr, want, what=(name, d, n))


# ---- 2. strictness on exact ties ----
@pytest.mark.parametrize("d", (23, 20, 7))
def test_strict_less_than_on_exact_ties(bliss, ctx, oracle, d):
    rng = np.random.default_rng(2)
    base = (rng.integers(-8, 9, (300, d)) / 8).astype(np.float32)
    X = np.repeat(base, 4, axis=0)  # row 4b: the base; 4b + 1: one coordinate moved by 1/8; 4b + 2, 4b + 3: two coordinates
    for b in range(300):
        c = rng.choice(d, 3, replace=False)
        s = rng.choice((-0.125, 0.125), 3).astype(np.float32)
        X[4 * b + 1, c[0]] += s[0]
        X[4 * b + 2, c[0]] += s[0]
        X[4 * b + 2, c[1]] += s[1]
        X[4 * b + 3, c[1]] += s[1]
        X[4 * b + 3, c[2]] += s[2]
    X = np.ascontiguousarray(X[rng.permutation(X.shape[0])])
    Dm = oracle.pairwise(X, X, "euclidean", None, n_threads=16)
    up = np.triu(np.ones(Dm.shape, bool), 1)
    eighth = np.float32(0.125)
    root2 = np.float32(np.sqrt(np.float32(2.0)) / np.float32(8.0))
    near = Dm[up & (np.abs(Dm - root2) < 1e-6)]
    assert near.size and (near == near[0]).all()  # the oracle's own bits of sqrt(2) / 8
    root2 = near[0]
    for t in (eighth, root2):
        at = int((Dm[up] == t).sum())
        assert at >= 300  # pairs at exactly the threshold exist ...
        lo = expected(oracle, X, "euclidean", None, t)
        hi = expected(oracle, X, "euclidean", None, np.nextafter(t, np.float32(1)))
        assert hi[1].shape[0] == lo[1].shape[0] + at  # ... are no edges at the threshold and are edges one ulp above
        assert not np.array_equal(lo[0], hi[0])
        print(f"d={d} threshold {float(t):.9g}: {at} pairs at it, {lo[1].shape[0]} edges below")
        check_both(bliss, ctx, X, None, "euclidean", None, t, lo, what=(d, float(t), "at"))
        check_both(bliss, ctx, X, None, "euclidean", None, np.nextafter(t, np.float32(1)), hi, what=(d, float(t), "one ulp above"))


@pytest.mark.parametrize("name", METRICS)
def test_equal_roots_of_distinct_sums_around_the_threshold(bliss, ctx, oracle, name):
    """the construction of tests/test_gpu_knn.py::test_equal_distances_from_distinct_sums: seven copies of every base row with one
    feature moved by 1 .. 3 ulps.  The pairs between two such families have sums a few ulps apart and, often, the same rounded
    root: with that root as the threshold none of them is an edge, one ulp above all of them are -- whatever the sums say."""
    d = 23
    rng = np.random.default_rng(2)
    base = rng.standard_normal((500, d)).astype(np.float32)
    X = np.repeat(base, 8, axis=0)
    for c in range(1, 8):
        rows = np.arange(500) * 8 + c
        col = rng.integers(0, d, 500)
        v = X[rows, col]
        toward = np.where(rng.integers(0, 2, 500) == 0, -np.inf, np.inf).astype(np.float32)
        ulps = rng.integers(1, 4, 500)
        for step in range(3):
            v = np.where(step < ulps, np.nextafter(v, toward), v)
        X[rows, col] = v
    perm = rng.permutation(X.shape[0])
    X, family = np.ascontiguousarray(X[perm]), (np.arange(4000) // 8)[perm]
    metric, M = _metric(oracle, name, d)
    Dm = oracle.pairwise(X, X, metric, M, n_threads=16)
    other = np.triu(family[:, None] != family[None, :], 1)
    i, j = np.unravel_index(np.argmin(np.where(other, Dm, np.inf)), Dm.shape)  # the two closest families
    between = other & np.isin(family, (family[i], family[j]))[:, None] & np.isin(family, (family[i], family[j]))[None, :]
    vals, counts = np.unique(Dm[between], return_counts=True)
    t = np.float32(vals[np.argmax(counts)])
    a, b = np.nonzero(between & (Dm == t))
    rows_differ = len({(X[p].tobytes(), X[q].tobytes()) for p, q in zip(a, b)})
    print(f"{name}: {counts.max()} of the {between.sum()} pairs between the two closest families share the distance {float(t):.9g} "
          f"({rows_differ} different row pairs)")
    if name != "cosine":  # on the oracle alone: one root from different rows (the cosine has no root to share)
        assert counts.max() >= 2 and rows_differ >= 2
    lo = expected(oracle, X, metric, M, t)
    hi = expected(oracle, X, metric, M, np.nextafter(t, np.float32(np.inf)))
    assert hi[1].shape[0] == lo[1].shape[0] + int((Dm[np.triu(np.ones(Dm.shape, bool), 1)] == t).sum())
    check_both(bliss, ctx, X, None, metric, M, t, lo, what=(name, "at"))
    check_both(bliss, ctx, X, None, metric, M, np.nextafter(t, np.float32(np.inf)), hi, what=(name, "one ulp above"))


# ---- 3. the title and artist rule ----
def test_title_and_artist_rule(bliss, ctx, oracle):
    rng = np.random.default_rng(3)
    n = 1500
    X, chains = planted(rng, n, 23, every=100)  # two chains
    assert chains.shape[0] == 2
    meta = np.zeros(n, np.uint32)  # key 0: no title or no artist -- joins nothing, although most rows carry it
    free = np.setdiff1d(np.arange(n), chains.reshape(-1))
    far = rng.choice(free, 7, replace=False)
    meta[far[:2]] = 5        # two rows far apart: an edge through the key alone
    meta[far[2:5]] = 9       # three rows with one key: three edges
    meta[far[5]] = 11        # a key nobody shares
    meta[chains[0, 2]] = 4   # a member of each chain: the key bridges the two components into one
    meta[chains[1, 4]] = 4
    plain = expected(oracle, X, "euclidean", None, THR)
    want = expected(oracle, X, "euclidean", None, THR, meta)
    # on the expected result alone
    assert plain[0][chains[0, 0]] != plain[0][chains[1, 0]] and want[0][chains[0, 0]] == want[0][chains[1, 0]]
    assert want[1].shape[0] == plain[1].shape[0] + 1 + 3 + 1
    e = want[1].tolist().index(sorted(far[:2].tolist()))
    assert want[2][e] >= 1.0 and want[0][far[0]] == want[0][far[1]] == far[:2].min()  # the meta-only edge carries its true distance
    assert want[0][far[5]] == far[5] and (want[0][free] == free).sum() >= free.size - 6
    check_both(bliss, ctx, X, meta, "euclidean", None, THR, want, what="meta")
    check_both(bliss, ctx, X, None, "euclidean", None, THR, plain, what="no meta")
    check_both(bliss, ctx, X, np.zeros(n, np.uint32), "euclidean", None, THR, plain, what="all keys 0")
    # no distance edges at all: the keys alone
    only = expected(oracle, X, "euclidean", None, 0.0, meta)
    assert only[1].shape[0] == 5
    check_both(bliss, ctx, X, meta, "euclidean", None, 0.0, only, what="threshold 0")
    check_both(bliss, ctx, X, meta, "euclidean", None, -1.0, only, what="threshold < 0")
    # the generic-d path reads the keys the same way
    X7 = np.ascontiguousarray(X[:, :7])
    check_both(bliss, ctx, X7, meta, "cosine", None, 1e-4, expected(oracle, X7, "cosine", None, 1e-4, meta), what="meta, d = 7")
    # the song-level form: the caller's own objects, groups by first member
    V2 = bliss.FeaturesVersion.Version2
    songs = [bliss.Song(path=f"/m/{i}.flac", title=None if meta[i] == 0 else f"t{meta[i]}", artist="a",
                        analysis=bliss.Analysis(X[i], V2), features_version=V2) for i in range(n)]
    groups = bliss.playlist.duplicate_groups(songs)
    assert [[songs.index(s) for s in g] for g in groups] == [g.tolist() for g in bliss.playlist.groups_from_labels(want[0])]
    assert all(g[k] is songs[songs.index(g[k])] for g in groups for k in range(len(g)))


# ---- 4. the pair buffer ----
GUARD = 0xDEADBEEF


def _raw_host(bliss, X, thr, max_pairs, with_pairs=True, with_dist=True):
    from bliss_rs_amd import _ffi

    n, d = X.shape
    lab, n_pairs = np.zeros(n, np.uint32), C.c_uint64(0)
    pairs = np.full(2 * max_pairs + 16, GUARD, np.uint32)
    dist = np.full(max_pairs + 16, np.float32(-7.0), np.float32)
    rc = _ffi.lib().blissgpu_duplicate_groups(X.ctypes.data, n, d, None, 0, None, float(thr), lab.ctypes.data, C.byref(n_pairs),
                                              pairs.ctypes.data if with_pairs else None, dist.ctypes.data if with_dist else None,
                                              max_pairs)
    assert rc == 0
    return lab.astype(np.int64), n_pairs.value, pairs, dist


def _raw_device(ctx, X, thr, max_pairs, with_pairs=True, with_dist=True):
    import torch
    from bliss_rs_amd import _ffi

    n, d = X.shape
    tX = torch.from_numpy(X).cuda()
    lab = torch.zeros(n, dtype=torch.int32, device="cuda")
    n_pairs = torch.zeros(1, dtype=torch.int64, device="cuda")
    pairs = torch.from_numpy(np.full(2 * max_pairs + 16, GUARD, np.uint32).view(np.int32)).cuda()
    dist = torch.full((max_pairs + 16,), -7.0, dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ctx._pre()
    rc = ctx._L.blissgpu_duplicate_groups_device(ctx._h, p(tX), n, d, None, 0, None, float(thr), p(lab), p(n_pairs),
                                                 p(pairs) if with_pairs else None, p(dist) if with_dist else None, max_pairs)
    ctx._post()
    ctx.synchronize()
    assert rc == 0, _ffi.lib().blissgpu_last_error()
    return lab.cpu().numpy().astype(np.int64), int(n_pairs.item()), pairs.cpu().numpy().view(np.uint32), dist.cpu().numpy()


def test_pair_buffer(bliss, ctx, oracle):
    rng = np.random.default_rng(4)
    X, _ = planted(rng, 3000, 23)
    want = expected(oracle, X, "euclidean", None, THR)
    e = want[1].shape[0]
    assert e == 50
    for form, raw in (("host", lambda *a, **k: _raw_host(bliss, *a, **k)), ("device", lambda *a, **k: _raw_device(ctx, *a, **k))):
        # exactly enough room
        lab, n_pairs, pairs, dist = raw(X, THR, e)
        assert np.array_equal(lab, want[0]) and n_pairs == e, form
        got, gd = pairs[:2 * e].reshape(e, 2).astype(np.int64), dist[:e]
        if form == "host":
            assert np.array_equal(got, want[1]), "the host form returns the edges in ascending (i, j)"
        order = np.lexsort((got[:, 1], got[:, 0]))
        assert_pairs(got[order], gd[order], want, (form, "exact room"))
        assert (pairs[2 * e:] == GUARD).all() and (dist[e:] == -7.0).all(), form
        # one entry too few: labels and n_pairs unchanged, nothing past the buffer
        lab, n_pairs, pairs, dist = raw(X, THR, e - 1)
        assert np.array_equal(lab, want[0]) and n_pairs == e, form
        assert (pairs[2 * (e - 1):] == GUARD).all() and (dist[e - 1:] == -7.0).all(), form
        # no distances; no list at all (a pair_dist without pairs is not written either); max_pairs = 0 with a buffer
        lab, n_pairs, pairs, dist = raw(X, THR, e, with_dist=False)
        assert np.array_equal(lab, want[0]) and n_pairs == e and (dist == -7.0).all(), form
        got = pairs[:2 * e].reshape(e, 2).astype(np.int64)
        assert np.array_equal(got[np.lexsort((got[:, 1], got[:, 0]))], want[1]), form
        lab, n_pairs, pairs, dist = raw(X, THR, e, with_pairs=False)
        assert np.array_equal(lab, want[0]) and n_pairs == e and (pairs == GUARD).all() and (dist == -7.0).all(), form
        lab, n_pairs, pairs, dist = raw(X, THR, 0)
        assert np.array_equal(lab, want[0]) and n_pairs == e and (pairs == GUARD).all() and (dist == -7.0).all(), form
    # the Python form sizes the buffer itself and asks again when the first one was too small
    Xd = np.repeat(X[:40], 60, axis=0)  # 40 groups of 60 identical rows: 70 800 edges among 2400 rows
    lab, pairs, dist = bliss.playlist.duplicate_labels(Xd, threshold=THR, return_pairs=True)
    w = expected(oracle, Xd, "euclidean", None, THR)
    assert w[1].shape[0] >= 40 * 60 * 59 // 2 > 2400
    assert np.array_equal(lab, w[0])
    assert_pairs(pairs, dist, w, "second call")


# ---- 5. degenerate sizes ----
@pytest.mark.parametrize("d,metric", ((23, "euclidean"), (20, "cosine"), (7, "euclidean")))
def test_degenerate_sizes(bliss, ctx, oracle, d, metric):
    rng = np.random.default_rng(5)
    thr = np.float32(0.2) if metric == "euclidean" else np.float32(0.01)
    total = 0
    for n in (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1025):
        X = ((rng.integers(-1, 2, (n, d)) + (8 if metric == "cosine" else 0)) / 8).astype(np.float32)
        if n >= 2:
            dup = rng.choice(n, max(1, n // 4), replace=False)
            X[dup] = X[rng.integers(0, n, dup.size)]
        if n == 0:
            lab, pairs, dist = host_form(bliss, X, None, metric, None, thr)
            assert lab.shape == (0,) and pairs.shape == (0, 2) and dist.shape == (0,)
            lab, n_pairs, _, _ = device_form(ctx, X, None, metric, None, thr, 4)
            assert lab.shape == (0,) and n_pairs == 0
            continue
        want = expected(oracle, X, metric, None, thr)
        if n == 1:
            assert want[0].tolist() == [0] and want[1].shape[0] == 0
        total += want[1].shape[0]
        check_both(bliss, ctx, X, None, metric, None, thr, want, what=(d, metric, n))
    assert total >= 100  # the sizes did hold edges


def test_all_rows_identical(bliss, ctx):
    """the contention case of the union-find: every pair is an edge.  Must finish; the time is recorded, not gated."""
    import torch

    n = 20_000
    X = np.tile(np.random.default_rng(6).standard_normal((1, 23)).astype(np.float32), (n, 1))
    t0 = time.perf_counter()
    lab = bliss.playlist.duplicate_labels(X, threshold=THR)
    t_host = time.perf_counter() - t0
    assert lab.shape == (n,) and not lab.any()
    tX = torch.from_numpy(X).cuda()
    times = []
    for _ in range(3):
        ctx.synchronize()
        t0 = time.perf_counter()
        labels, n_pairs = ctx.duplicate_labels(tX, threshold=float(THR))
        ctx.synchronize()
        times.append(time.perf_counter() - t0)
        assert not labels.any().item() and int(n_pairs.item()) == n * (n - 1) // 2
    print(f"all {n} rows identical: device form {np.median(times) * 1e3:.1f} ms (median of 3), host form {t_host * 1e3:.1f} ms")
    # a pair buffer that is far too small for 2 * 10^8 edges: clamped, labels and count unchanged
    lab2, n_pairs, pairs, dist = _raw_device(ctx, X, THR, 1000)
    assert not lab2.any() and n_pairs == n * (n - 1) // 2
    assert (pairs[2000:] == GUARD).all() and (dist[1000:] == -7.0).all()


# ---- 6. NaN ----
def test_nan_distance(bliss, ctx, oracle):
    import torch

    rng = np.random.default_rng(6)
    X = rng.standard_normal((2000, 23)).astype(np.float32)
    X[1234] = 0.0  # the cosine distance to the zero vector is 0 / 0
    with pytest.raises(FloatingPointError):
        expected(oracle, X, "cosine", None, THR)
    with pytest.raises(ValueError):
        bliss.playlist.duplicate_labels(X, metric="cosine")
    with pytest.raises(bliss.BlissGpuError) as e:
        ctx.duplicate_labels(torch.from_numpy(X).cuda(), metric="cosine")
    assert e.value.code == 5
    Y = X.copy()
    Y[7, 3] = np.nan
    for metric in ("euclidean", "cosine"):
        with pytest.raises(ValueError):
            bliss.playlist.duplicate_labels(Y, metric=metric)
    with pytest.raises(ValueError):
        bliss.playlist.duplicate_labels(np.ascontiguousarray(Y[:, :7]), metric="euclidean")  # generic d
    # a negative sum under an indefinite M is a NaN distance as well
    M = -np.eye(23, dtype=np.float32)
    with pytest.raises(ValueError):
        bliss.playlist.duplicate_labels(X, metric="mahalanobis", m=M)
    # the same rows are fine under the euclidean metric, and the context is usable afterwards
    check_both(bliss, ctx, X, None, "euclidean", None, THR, expected(oracle, X, "euclidean", None, THR), what="finite")


# ---- 7. agreement with the playlist deduplication ----
def test_agrees_with_dedup_order(bliss, ctx, oracle):
    rng = np.random.default_rng(7)
    X, chains = planted(rng, 3000, 23)
    want = expected(oracle, X, "euclidean", None, THR)
    labels = bliss.playlist.duplicate_labels(X, threshold=THR)
    assert np.array_equal(labels, want[0])
    # a random playlist order in which the members of a chain follow one another, so that songs are absorbed: half of the
    # chains in their own order (0 absorbs 1, 2 absorbs 3, 4 absorbs 5), half shuffled
    in_chain = np.zeros(3000, bool)
    in_chain[chains.reshape(-1)] = True
    blocks = [[int(i)] for i in np.flatnonzero(~in_chain)]
    blocks += [ch.tolist() if k % 2 == 0 else rng.permutation(ch).tolist() for k, ch in enumerate(chains)]
    seq = np.array([i for b in rng.permutation(len(blocks)) for i in blocks[b]], np.uint32)
    kept = bliss.playlist.dedup_order(X, seq, None, "euclidean", None, THR)
    absorbed = 0
    for k, p in enumerate(kept):
        end = kept[k + 1] if k + 1 < kept.size else seq.size
        for r in range(p + 1, end):  # absorbed by the song at position p
            assert labels[seq[r]] == labels[seq[p]], (p, r)
            absorbed += 1
    print(f"{absorbed} songs absorbed by the playlist deduplication")
    assert absorbed >= 3 * ((chains.shape[0] + 1) // 2)


# ---- 8, 9, 11. scale ----
@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(1)
    return planted(rng, 100_000, 23)


def test_scale_against_the_k_nearest_search(bliss, ctx, big):
    import torch

    X, chains = big
    n = X.shape[0]
    idx, dist = bliss.playlist.nearest_order(X, X, 8, skip=np.arange(n))
    # a condition on the input: every row's 8th neighbour is no edge, so the lists hold every edge
    assert (dist[:, 7] >= THR).all()
    i, c = np.nonzero((dist < THR) & (idx > np.arange(n)[:, None]))
    I, J, V = i.astype(np.int64), idx[i, c], dist[i, c]
    order = np.lexsort((J, I))
    want = (components(n, I[order], J[order]), np.stack([I[order], J[order]], axis=1), V[order])
    assert want[1].shape[0] >= 5 * chains.shape[0] and has_non_clique(want[0], want[1])
    print(f"n={n}: {want[1].shape[0]} edges, {(np.bincount(want[0]) >= 2).sum()} components")
    check_both(bliss, ctx, X, None, "euclidean", None, THR, want, what="scale")
    # 9. determinism: two more runs of the device form, with a buffer larger than needed
    a = device_form(ctx, X, None, "euclidean", None, THR, 4 * want[1].shape[0])
    b = device_form(ctx, X, None, "euclidean", None, THR, 4 * want[1].shape[0])
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    assert np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32))
    assert np.array_equal(a[0], want[0])
    # structure: three launches whatever n, no matrix
    tX = torch.from_numpy(X).cuda()
    counts = []
    ctx.profile_enable(True)
    try:
        for rows in (5000, n):
            ctx.synchronize()
            torch.cuda.synchronize()
            ctx.profile_reset()
            free0 = torch.cuda.mem_get_info()[0]
            ctx.duplicate_labels(tX[:rows], threshold=float(THR))
            ctx.synchronize()
            free1 = torch.cuda.mem_get_info()[0]
            prof = ctx.profile()
            counts.append(sum(v[1] for name, v in prof.items() if name.startswith("dup_")))
            assert all(v[1] == 0 for name, v in prof.items() if not name.startswith("dup_")), prof
            assert free0 - free1 < 64 * 2**20, (rows, free0 - free1)  # the matrix would be 40 GB
    finally:
        ctx.profile_enable(False)
    assert counts[0] == counts[1] == 3, counts


def test_join_is_not_slower_than_knn_k1(bliss, ctx, big):
    """11. the join evaluates half the pairs of the k-nearest self-search and keeps no lists: device-form wall time without a
    pair buffer against Context.knn with k = 1 on the same matrix, same process, medians of 3, alternating.  Gate: join <= knn."""
    import torch

    X, _ = big
    n = X.shape[0]
    tX = torch.from_numpy(X).cuda()
    me = torch.arange(n, dtype=torch.int32, device="cuda")

    def timed(f):
        torch.cuda.synchronize()
        ctx.synchronize()
        t0 = time.perf_counter()
        f()
        ctx.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    join = lambda: ctx.duplicate_labels(tX, threshold=float(THR))  # noqa: E731
    knn = lambda: ctx.knn(tX, tX, 1, "euclidean", None, me)  # noqa: E731
    timed(join)
    timed(knn)
    t_join, t_knn = [], []
    for _ in range(3):
        t_join.append(timed(join))
        t_knn.append(timed(knn))
    t_join, t_knn = float(np.median(t_join)), float(np.median(t_knn))
    print(f"n={n}: join {t_join * 1e3:.2f} ms, knn k=1 {t_knn * 1e3:.2f} ms, ratio {t_join / t_knn:.2f}")
    assert t_join <= t_knn


# ---- 10. the library form ----
def test_library_duplicate_songs(bliss, tmp_path, monkeypatch):
    from bliss_rs_amd import _ffi

    rng = np.random.default_rng(10)
    n = 400
    X = (0.5 * rng.standard_normal((n, 23))).astype(np.float32)
    g1, g2, pair = [3, 77, 250], [40, 41, 42, 399], [10, 300]
    u = rng.standard_normal(23)
    u /= np.linalg.norm(u)
    for g in (g1, g2):
        for t, r in enumerate(g):
            X[r] = (X[g[0]].astype(np.float64) + t * 0.04 * u).astype(np.float32)  # a chain: the ends are not within 0.05
    V2 = bliss.FeaturesVersion.Version2
    songs = [bliss.Song(path=f"/music/{i:04d}.flac", title="Same Song" if i in pair else f"t{i}", artist="a", duration=1.0,
                        analysis=bliss.Analysis(X[i], V2), features_version=V2) for i in range(n)]
    db = str(tmp_path / "bliss.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs)
    lib = _ffi.lib()
    calls = []
    real = lib.blissgpu_duplicate_groups

    def counted(*a):
        calls.append(1)
        return real(*a)

    monkeypatch.setattr(lib, "blissgpu_duplicate_groups", counted)
    groups = bliss.library.duplicate_songs(db)
    monkeypatch.undo()
    assert len(calls) == 1
    assert all(isinstance(s, bliss.Song) for g in groups for s in g)
    want = sorted([g1, g2, pair])
    assert [[s.path for s in g] for g in groups] == [[f"/music/{i:04d}.flac" for i in g] for g in want]
    # without distance edges only the title / artist pair is left; nothing was deleted
    assert [[s.path for s in g] for g in bliss.library.duplicate_songs(db, distance_threshold=0.0)] == \
        [[f"/music/{i:04d}.flac" for i in pair]]
    assert len(bliss.library.load_songs(db)) == n
    assert bliss.library.duplicate_songs(db, metric_builder=bliss.playlist.cosine_distance)[0][0].path == "/music/0003.flac"


# ---- the host form's staging: every optional argument given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("meta,pairs,pair_dist", ((True, True, True), (False, False, False), (True, True, False), (False, True, True)))
def test_host_form_stages_like_the_device_form(bliss, ctx, meta, pairs, pair_dist):
    import staging_cases as sc

    def build(c, dev):
        X = c.X.copy()
        X[40:60] = X[10:30]  # twenty planted pairs
        label, n_pairs = dev(sc.out((c.n,), np.uint32)), dev(np.full(1, 0x5A5A, np.uint64))
        pr, pd = dev(sc.out((64, 2), np.uint32, pairs)), dev(sc.out((64,), np.float32, pairs and pair_dist))
        tags = np.arange(c.n, dtype=np.uint32)
        tags[71] = tags[70]  # one more pair, by the metadata rule
        outs = [label, n_pairs, pr, pd]
        return [dev(X), c.n, sc.D, dev(tags if meta else None), 2, dev(c.M), 0.01] + outs + [64 if pairs else 0], outs

    def canon(outs):  # the device form appends its pairs in the order the wavefronts meet them: ascending (i, j), as the host form returns them
        _, n_pairs, pr, pd = outs
        m = int(n_pairs.view(np.uint64)[0])
        if pr is not None and 0 < m <= 64:
            order = np.lexsort((pr[:m, 1], pr[:m, 0]))
            pr[:m] = pr[:m][order]
            if pd is not None:
                pd[:m] = pd[:m][order]

    sc.check(bliss, ctx, "duplicate_groups", build, lists=False, canon=canon)
