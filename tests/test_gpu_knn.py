"""GPU tests (-m gpu) of the k-nearest search (blissgpu_knn / blissgpu_knn_device: knn_scan_kernel + knn_merge_kernel):
closest_to_songs(&[query], candidates, metric) of the reference (src/playlist.rs:256-270) cut after k, for many queries.
The expected values come from the CPU oracle's distance matrix (oracle.pairwise) and numpy's stable argsort -- never from
the code under test.  The distances are bit-identical by contract, so the selected indices are a discrete result: every
comparison is exact (np.array_equal on indices, bit equality on distances), ties at the cut included."""
import json
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "playlist_cases.json")))
KS = (1, 2, 31, 32, 33, 64, 1000, 1024)
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
    """-> (library metric name, M or None); the full SPD matrix is built as in tests/test_gpu_dedup.py::_metrics"""
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


def expected_from_matrix(Dm, k, skip=None):
    """rows of the oracle's distance matrix -> (idx int64[q, k], dist f32[q, k]): stable ascending order without the
    skipped column, cut after k, padded with -1 / inf"""
    q, n = Dm.shape
    idx = np.full((q, k), -1, np.int64)
    dist = np.full((q, k), np.inf, np.float32)
    for i in range(q):
        order = np.argsort(Dm[i], kind="stable")
        if skip is not None and skip[i] >= 0:
            order = order[order != skip[i]]
        order = order[:k]
        idx[i, :order.size] = order
        dist[i, :order.size] = Dm[i, order]
    return idx, dist


def oracle_knn(oracle, Q, X, k, metric, M, skip=None):
    return expected_from_matrix(oracle.pairwise(Q, X, metric, M, n_threads=16), k, skip)


def host_knn(bliss, Q, X, k, metric, M, skip=None):
    return bliss.playlist.nearest_order(Q, X, k, metric, M, skip)


def device_knn(ctx, Q, X, k, metric, M, skip=None):
    import torch

    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()  # noqa: E731
    idx, dist = ctx.knn(t(Q, np.float32), t(X, np.float32), k, metric, t(M, np.float32), t(skip, np.int32))
    ctx.synchronize()
    return idx.cpu().numpy().astype(np.int64), dist.cpu().numpy()


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "indices", int((got[0] != want[0]).any(axis=1).sum()), "rows differ")
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (what, "distance bits")


def check_both(bliss, ctx, oracle, Q, X, k, metric, M, skip=None, what="", want=None):
    if want is None:
        want = oracle_knn(oracle, Q, X, k, metric, M, skip)
    assert_same(host_knn(bliss, Q, X, k, metric, M, skip), want, (what, "host form"))
    assert_same(device_knn(ctx, Q, X, k, metric, M, skip), want, (what, "device form"))
    return want


# ---- (a) the reference's own closest_to_songs cases (src/playlist.rs:860-1007): one seed, six candidates, one exact tie ----
@pytest.mark.parametrize("case", range(len(CASES["closest_to_songs"])))
@pytest.mark.parametrize("k", (6, 3))
def test_reference_cases(bliss, ctx, case, k):
    c, S = CASES["closest_to_songs"][case], CASES["songs"]
    Q = np.array([S[n]["analysis"] for n in c["initial"]], np.float32)
    X = np.array([S[n]["analysis"] for n in c["candidates"]], np.float32)
    want = c["expected"][:k]
    for form in (host_knn(bliss, Q, X, k, c["metric"], None), device_knn(ctx, Q, X, k, c["metric"], None)):
        assert [c["candidates"][j] for j in form[0][0]] == want
    mk = lambda n: bliss.Song(path=n, analysis=bliss.Analysis(S[n]["analysis"], bliss.FeaturesVersion.Version2),  # noqa: E731
                              features_version=bliss.FeaturesVersion.Version2)
    got = bliss.playlist.nearest_songs([mk(n) for n in c["initial"]], [mk(n) for n in c["candidates"]], k,
                                       bliss.playlist.euclidean_distance)
    assert [[s.path for s in row] for row in got] == [want]


# ---- (b) against the oracle on tie-rich data ----
def _ties_at_cut(Dm, k):
    s = np.sort(Dm, axis=1, kind="stable")
    return int((s[:, k - 1] == s[:, k]).sum())


@pytest.mark.parametrize("d", (23, 20))
@pytest.mark.parametrize("name", METRICS)
def test_tie_rich_against_oracle(bliss, ctx, oracle, d, name):
    rng = np.random.default_rng(1)
    X = tie_rich(rng, 4000, d)
    Q = tie_rich(rng, 256, d)
    metric, M = _metric(oracle, name, d)
    Dm = oracle.pairwise(Q, X, metric, M, n_threads=16)
    ties = _ties_at_cut(Dm, 32)
    print(f"d={d} {name}: {ties} of 256 queries tie at the cut k=32")
    assert ties >= (1 if name == "spd" else 10)  # on the oracle's matrix alone: the tie rule at the cut is exercised
    for k in KS:
        check_both(bliss, ctx, oracle, Q, X, k, metric, M, what=(d, name, k), want=expected_from_matrix(Dm, k))


@pytest.mark.parametrize("d", (7, 64))
def test_generic_feature_count(bliss, ctx, oracle, d):
    rng = np.random.default_rng(1)
    X, Q = tie_rich(rng, 4000, d), tie_rich(rng, 256, d)
    for k in (1, 32, 1024):
        check_both(bliss, ctx, oracle, Q, X, k, "euclidean", None, what=(d, k))


# ---- (b2) distinct sums, equal distances: what ordering by the sum before the root gets wrong ----
@pytest.mark.parametrize("name", METRICS)
def test_equal_distances_from_distinct_sums(bliss, ctx, oracle, name):
    d, k = 23, 32
    rng = np.random.default_rng(2)
    base = rng.standard_normal((500, d)).astype(np.float32)
    X = np.repeat(base, 8, axis=0)
    for c in range(1, 8):  # seven copies of every base row, one feature moved by 1 .. 3 ulps
        rows = np.arange(500) * 8 + c
        col = rng.integers(0, d, 500)
        v = X[rows, col]
        toward = np.where(rng.integers(0, 2, 500) == 0, -np.inf, np.inf).astype(np.float32)
        ulps = rng.integers(1, 4, 500)
        for step in range(3):
            v = np.where(step < ulps, np.nextafter(v, toward), v)
        X[rows, col] = v
    X = np.ascontiguousarray(X[rng.permutation(X.shape[0])])
    Q = rng.standard_normal((256, d)).astype(np.float32)
    metric, M = _metric(oracle, name, d)
    Dm = oracle.pairwise(Q, X, metric, M, n_threads=16)
    want = expected_from_matrix(Dm, k)
    hit = 0
    for i in range(256):
        j, v = want[0][i], want[1][i]
        same = v[1:] == v[:-1]
        hit += any(same[t] and not np.array_equal(X[j[t]], X[j[t + 1]]) for t in range(k - 1))
    print(f"{name}: {hit} of 256 queries hold two equal distances of different rows inside their top {k}")
    assert hit >= 128  # on the oracle alone
    check_both(bliss, ctx, oracle, Q, X, k, metric, M, what=name, want=want)


# ---- (c) continuous data ----
@pytest.mark.parametrize("name", METRICS)
def test_continuous_data(bliss, ctx, oracle, name):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((20_000, 23)).astype(np.float32)
    Q = rng.standard_normal((1000, 23)).astype(np.float32)
    metric, M = _metric(oracle, name, 23)
    check_both(bliss, ctx, oracle, Q, X, 32, metric, M, what=name)


# ---- (d) skip and padding ----
def test_skip_and_padding(bliss, ctx, oracle):
    rng = np.random.default_rng(4)
    n = 3000
    X = tie_rich(rng, n, 23)
    X[17] = X[5]  # an exact duplicate: row 5's nearest neighbour at distance 0 once row 5 skips itself
    me = np.arange(n, dtype=np.int64)
    want = check_both(bliss, ctx, oracle, X, X, 8, "euclidean", None, skip=me, what="self skipped")
    assert not (want[0] == me[:, None]).any()
    assert want[0][5, 0] == 17 and want[1][5, 0] == 0.0
    # the same array object as queries and candidates (the single-upload path of the host form)
    assert_same(bliss.playlist.nearest_order(X, X, 8, "euclidean", None, me), want, "queries is candidates")
    mixed = me.copy()
    mixed[::3] = -1
    check_both(bliss, ctx, oracle, X, X, 8, "euclidean", None, skip=mixed, what="mixed skip")
    # fewer eligible candidates than k: the 0xFFFFFFFF / +inf tail
    small = X[:40]
    for k, skip in ((64, None), (40, np.arange(40)), (41, np.arange(40)), (1024, None)):
        w = check_both(bliss, ctx, oracle, small, small, k, "cosine" if k == 41 else "euclidean", None, skip=skip, what=("padding", k))
        eligible = 40 - (skip is not None)
        assert (w[0][:, eligible:] == -1).all() and np.isinf(w[1][:, eligible:]).all() and (w[0][:, :eligible] >= 0).all()
    # n = 1, with and without skipping it
    check_both(bliss, ctx, oracle, X[:5], X[:1], 3, "euclidean", None, what="n = 1")
    check_both(bliss, ctx, oracle, X[:5], X[:1], 3, "euclidean", None, skip=np.array([0, -1, 0, -1, -1]), what="n = 1, skipped")


@pytest.mark.parametrize("q,k", ((1, 32), (1, 1024), (3, 1024)))
def test_few_queries_many_candidates(bliss, ctx, oracle, q, k):
    """several workgroups share a query's candidates; their partial lists are merged on the device"""
    rng = np.random.default_rng(5)
    X = tie_rich(rng, 100_000, 23)
    Q = tie_rich(rng, q, 23)
    for name in ("euclidean", "cosine", "weights"):
        metric, M = _metric(oracle, name, 23)
        check_both(bliss, ctx, oracle, Q, X, k, metric, M, what=(q, k, name))


# ---- (e) full size, every row ----
def _parent_route(ctx, tX, k, metric, tM, slab=4096, self_skipped=True, buf=None):
    """the same answer on the parent commit's own kernels: row slabs of Context.pairwise into one reused buffer, the self column
    set to +inf, a stable sort, the first k"""
    import torch

    n = tX.shape[0]
    if buf is None:
        buf = torch.empty((slab, n), dtype=torch.float32, device=tX.device)
    idx = torch.empty((n, k), dtype=torch.int64, device=tX.device)
    dist = torch.empty((n, k), dtype=torch.float32, device=tX.device)
    for r0 in range(0, n, slab):
        rows = min(slab, n - r0)
        out = ctx.pairwise(tX[r0:r0 + rows], tX, metric, tM, out=buf[:rows])
        ctx.synchronize()
        if self_skipped:
            ar = torch.arange(rows, device=tX.device)
            out[ar, ar + r0] = float("inf")
        v, j = torch.sort(out, dim=1, stable=True)
        idx[r0:r0 + rows], dist[r0:r0 + rows] = j[:, :k], v[:, :k]
    return idx, dist


@pytest.mark.parametrize("name", ("euclidean", "weights"))
def test_full_size_every_row(bliss, ctx, oracle, name):
    import torch

    n, k = 100_000, 32
    rng = np.random.default_rng(1)
    X = tie_rich(rng, n, 23)
    metric, M = _metric(oracle, name, 23)
    tX = torch.from_numpy(X).cuda()
    tM = None if M is None else torch.from_numpy(M).cuda()
    me = torch.arange(n, dtype=torch.int32, device="cuda")
    idx, dist = ctx.knn(tX, tX, k, metric, tM, me)
    ctx.synchronize()
    # (i) 512 random rows against the oracle
    rows = np.sort(rng.choice(n, 512, replace=False))
    Dm = oracle.pairwise(X[rows], X, metric, M, n_threads=16)
    if name == "euclidean":
        ties = _ties_at_cut(np.where(np.arange(n)[None, :] == rows[:, None], np.inf, Dm), k)
        print(f"{ties} of 512 sampled rows tie at the cut")
        assert ties >= 10
    want = expected_from_matrix(Dm, k, skip=rows)
    assert_same((idx[rows].cpu().numpy().astype(np.int64), dist[rows].cpu().numpy()), want, (name, "oracle rows"))
    # (ii) every row against the parent commit's kernels
    p_idx, p_dist = _parent_route(ctx, tX, k, metric, tM)
    assert torch.equal(idx.to(torch.int64), p_idx), (name, "indices", int((idx.to(torch.int64) != p_idx).any(dim=1).sum()))
    assert torch.equal(dist.view(torch.int32), p_dist.view(torch.int32)), (name, "distance bits")


# ---- (f) NaN ----
def test_nan_distances(bliss, ctx, oracle):
    rng = np.random.default_rng(6)
    X = rng.standard_normal((2000, 23)).astype(np.float32)
    X[1234] = 0.0  # cosine distance to the zero vector is 0 / 0
    Q = rng.standard_normal((2, 23)).astype(np.float32)
    with pytest.raises(ValueError):
        host_knn(bliss, Q, X, 8, "cosine", None)
    with pytest.raises(bliss.BlissGpuError) as e:
        device_knn(ctx, Q, X, 8, "cosine", None)
    assert e.value.code == 5
    check_both(bliss, ctx, oracle, Q, X, 8, "euclidean", None, what="euclidean is finite")
    # a skipped pair is not evaluated
    keep = np.arange(2000) != 1234
    want = oracle_knn(oracle, Q[:1], X[keep], 8, "cosine", None)
    want = (np.where(want[0] >= 1234, want[0] + 1, want[0]), want[1])
    skip = np.array([1234])
    assert_same(host_knn(bliss, Q[:1], X, 8, "cosine", None, skip), want, "skipped NaN, host form")
    assert_same(device_knn(ctx, Q[:1], X, 8, "cosine", None, skip), want, "skipped NaN, device form")
    with pytest.raises(ValueError):
        host_knn(bliss, Q, X, 8, "cosine", None, np.array([1234, -1]))
    with pytest.raises(bliss.BlissGpuError) as e:
        device_knn(ctx, Q, X, 8, "cosine", None, np.array([1234, -1]))
    assert e.value.code == 5


# ---- (g) structure ----
def test_launch_count_and_memory(bliss, ctx):
    import torch

    rng = np.random.default_rng(8)
    counts = []
    ctx.profile_enable(True)
    try:
        for q, n in ((1000, 10_000), (100_000, 100_000)):
            tX = torch.from_numpy(rng.standard_normal((n, 23)).astype(np.float32)).cuda()
            tQ = tX[:q].contiguous()
            idx = torch.empty((q, 32), dtype=torch.int32, device="cuda")  # (the allocator has the outputs' blocks before the reading)
            dist = torch.empty((q, 32), dtype=torch.float32, device="cuda")
            del idx, dist
            ctx.synchronize()
            torch.cuda.synchronize()
            ctx.profile_reset()
            free0 = torch.cuda.mem_get_info()[0]
            ctx.knn(tQ, tX, 32, "euclidean")
            ctx.synchronize()
            free1 = torch.cuda.mem_get_info()[0]
            prof = ctx.profile()
            counts.append(sum(v[1] for name, v in prof.items() if name.startswith("knn_")))
            assert counts[-1] >= 1
            for name in prof:
                assert not (name.startswith("pairwise") or name.startswith("set_distance") or name.startswith("radix_")), prof
            print(f"q={q} n={n}: knn launches {counts[-1]}, free memory fell by {(free0 - free1) / 2**20:.1f} MiB")
            if n == 100_000:
                assert free0 - free1 < 4 * 2**30  # the matrix would be 40 GB
    finally:
        ctx.profile_enable(False)
    assert counts[0] == counts[1], counts


def test_similar_songs_is_one_call(bliss, tmp_path, monkeypatch):
    from bliss_rs_amd import _ffi

    rng = np.random.default_rng(9)
    n, k = 2000, 10
    X = tie_rich(rng, n, 23)
    V2 = bliss.FeaturesVersion.Version2
    songs = [bliss.Song(path=f"/music/{i:05d}.flac", title=f"t{i}", artist="a", duration=1.0, analysis=bliss.Analysis(X[i], V2),
                        features_version=V2) for i in range(n)]
    db = str(tmp_path / "bliss.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs)
    lib = _ffi.lib()
    calls = []
    real = lib.blissgpu_knn

    def counted(*a):
        calls.append(1)
        return real(*a)

    monkeypatch.setattr(lib, "blissgpu_knn", counted)
    table = bliss.library.similar_songs(db, k)
    assert len(calls) == 1 and len(table) == n
    some = [f"/music/{i:05d}.flac" for i in (0, 7, 1999)]
    part = bliss.library.similar_songs(db, k, song_paths=some)
    assert len(calls) == 2 and sorted(part) == sorted(some)
    monkeypatch.undo()
    for i in list(range(0, n, 97)) + [7, 1999]:
        pool = songs[:i] + songs[i + 1:]
        want = [s.path for s in bliss.playlist.closest_to_songs([songs[i]], pool)[:k]]
        assert [p for p, _ in table[songs[i].path]] == want, i
        if songs[i].path in part:
            assert part[songs[i].path] == table[songs[i].path]
    with pytest.raises(bliss.ProviderError):
        bliss.library.similar_songs(db, k, song_paths=["/music/none.flac"])


# ---- (h) not slower than the route it replaces ----
def test_not_slower_than_the_parent_route(bliss, ctx):
    import torch

    n, k = 100_000, 32
    rng = np.random.default_rng(10)
    tX = torch.from_numpy(rng.standard_normal((n, 23)).astype(np.float32)).cuda()
    me = torch.arange(n, dtype=torch.int32, device="cuda")
    buf = torch.empty((4096, n), dtype=torch.float32, device="cuda")

    def route():
        """section 5's parent route: slabs of 4096 queries through Context.pairwise (A != B form), torch.topk per slab"""
        idx = torch.empty((n, k), dtype=torch.int64, device="cuda")
        for r0 in range(0, n, 4096):
            rows = min(4096, n - r0)
            out = ctx.pairwise(tX[r0:r0 + rows], tX, "euclidean", None, out=buf[:rows])
            ar = torch.arange(rows, device="cuda")
            out[ar, ar + r0] = float("inf")
            idx[r0:r0 + rows] = torch.topk(out, k, dim=1, largest=False).indices
        return idx

    def timed(f):
        torch.cuda.synchronize()
        ctx.synchronize()
        t0 = time.perf_counter()
        f()
        ctx.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    knn = lambda: ctx.knn(tX, tX, k, "euclidean", None, me)  # noqa: E731
    timed(knn)
    timed(route)
    t_knn, t_route = [], []
    for _ in range(3):
        t_knn.append(timed(knn))
        t_route.append(timed(route))
    t_knn, t_route = float(np.median(t_knn)), float(np.median(t_route))
    print(f"knn {t_knn * 1e3:.1f} ms, parent route {t_route * 1e3:.1f} ms")
    assert t_knn <= t_route


# ---- (i) a candidate matrix that does not start on a 16-byte boundary: the scalar copy of an odd-d block (d = 23) ----
def test_unaligned_candidates(ctx, oracle):
    """the same values as a fresh tensor (16-byte aligned: float4 copies of a block) and as a view that starts one float into
    an allocation (the flat scalar copy): a full block plus a ragged block of one row, and a single ragged block.  Through the
    k-nearest scan, the locally scaled one and one chain step: three kernels that each carry their own copy of the staging text"""
    import torch

    d, q, k = 23, 5, 3
    rng = np.random.default_rng(11)

    def pair(X):
        aligned = torch.from_numpy(X).cuda()
        buf = torch.empty(X.size + 1, dtype=torch.float32, device="cuda")
        offset = buf[1:].view(X.shape)
        offset.copy_(aligned)
        for t, want in ((aligned, True), (offset, False)):  # (what the Python layer passes on: contiguous() of a contiguous view)
            assert (t.data_ptr() % 16 == 0) == want and (t.contiguous().data_ptr() % 16 == 0) == want
        return aligned, offset

    def out(res):
        ctx.synchronize()
        return res[0].cpu().numpy().astype(np.int64), res[1].cpu().numpy()

    for n in (257, 255):
        X, Q = tie_rich(rng, n, d), tie_rich(rng, q, d)
        tQ = torch.from_numpy(Q).cuda()
        for metric in ("euclidean", "cosine"):
            Dm = oracle.pairwise(Q, X, metric, None, n_threads=16)
            want = expected_from_matrix(Dm, k)
            for name, tX in zip(("aligned", "offset"), pair(X)):
                assert_same(out(ctx.knn(tQ, tX, k, metric)), want, (n, metric, name))
            if (n, metric) != (257, "euclidean"):
                continue
            # the locally scaled scan: the contract of tests/test_gpu_scaled_knn.py::scaled_matrix in float32 numpy
            qs, cs = rng.uniform(0.5, 2.0, q).astype(np.float32), rng.uniform(0.5, 2.0, n).astype(np.float32)
            want = expected_from_matrix(Dm / np.sqrt(qs[:, None] * cs[None, :]), k)
            assert want[1].dtype == np.float32
            for name, tX in zip(("aligned", "offset"), pair(X)):
                got = out(ctx.scaled_knn(tQ, torch.from_numpy(qs).cuda(), tX, torch.from_numpy(cs).cuda(), k, metric))
                assert_same(got, want, (n, "scaled", name))
            # two chains of one seed each, two songs: the song nearest the seed, then one step -- the song nearest that one
            # which is not taken (equal distances to the lower index; `0.0f +` a distance, as the chain kernels add)
            idx, dist = np.zeros((2, 2), np.int64), np.zeros((2, 2), np.float32)
            for g in range(2):
                idx[g, 0] = np.argsort(Dm[g], kind="stable")[0]
                dist[g, 0] = np.float32(0.0) + Dm[g, idx[g, 0]]
                row = oracle.pairwise(X[idx[g, 0]:idx[g, 0] + 1], X, metric, None)[0]
                order = np.argsort(row, kind="stable")
                idx[g, 1] = order[order != idx[g, 0]][0]
                dist[g, 1] = np.float32(0.0) + row[idx[g, 1]]
            for name, tX in zip(("aligned", "offset"), pair(X)):
                assert_same(out(ctx.chains(tQ[:2], [0, 1, 2], tX, 2, metric, route="steps")), (idx, dist), (n, "chain", name))


# ---- the host form's staging: every optional argument given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("skip,dist", ((True, True), (False, False), (True, False), (False, True)))
def test_host_form_stages_like_the_device_form(bliss, ctx, skip, dist):
    import staging_cases as sc

    def build(c, dev):
        idx, dd = dev(sc.out((c.q, c.k), np.uint32)), dev(sc.out((c.q, c.k), np.float32, dist))
        return [dev(c.Q), c.q, dev(c.X), c.n, sc.D, 2, dev(c.M), dev(c.qskip if skip else None), c.k, idx, dd], [idx, dd]

    sc.check(bliss, ctx, "knn", build)
