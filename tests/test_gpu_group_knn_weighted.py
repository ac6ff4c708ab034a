"""GPU tests (-m gpu) of the per-group diagonal metric: blissgpu_group_weights (group_weights_kernel) and
blissgpu_group_knn_weighted (group_weights_kernel + the per-group form of group_knn_scan_kernel + group_knn_merge_kernel), host
and device forms.  The expected values never come from the code under test: the weights are the diagonal of
oracle.variance_based_weight_matrix (ones for a group under two seeds), the scores of group g are the rows of
oracle.pairwise(S_g, X, "mahalanobis", diag(w_g)) added sequentially in numpy f32 in seed order, the order is numpy's stable
argsort.  Every comparison is exact: np.array_equal on indices, bit equality on weights and distances.  (The one exception is
a weight that is NaN: IEEE 754 does not define a NaN's payload, so there the NaN-ness is compared, element by element.)"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


# ---- helpers (as in tests/test_gpu_group_knn.py) ----
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


def expected_weights(oracle, S, off):
    """-> (W f32[G, d], few bool[G]): the diagonal of the oracle's variance_based_weight_matrix per group, ones under two seeds"""
    G = off.shape[0] - 1
    W, few = np.ones((G, S.shape[1]), np.float32), np.zeros(G, bool)
    for g in range(G):
        a, b = int(off[g]), int(off[g + 1])
        if b - a < 2:
            few[g] = True
        else:
            W[g] = np.diagonal(oracle.variance_based_weight_matrix(S[a:b]))
    return W, few


def scores_of(oracle, S, off, X, W):
    """f32[G, n]: group g's rows of oracle.pairwise(S_g, X, "mahalanobis", diag(W[g])), added sequentially in f32 in seed order"""
    G = off.shape[0] - 1
    out = np.zeros((G, X.shape[0]), np.float32)
    for g in range(G):
        a, b = int(off[g]), int(off[g + 1])
        if b == a:
            continue
        Dm = oracle.pairwise(S[a:b], X, "mahalanobis", np.diag(W[g]).astype(np.float32), n_threads=16)
        acc = np.zeros(X.shape[0], np.float32)
        for row in Dm:
            acc = acc + row
        out[g] = acc
    return out


def host_form(bliss, S, off, X, k, W=None, skip=None):
    """the public host form; W = None: derived weights"""
    if W is None:
        return bliss.playlist.nearest_to_groups((S, off), X, k, "variance", None, skip)
    return bliss.playlist.nearest_to_groups((S, off), X, k, "diagonal", W, skip)


def raw_host_form(S, off, X, k, W=None, skip=None):
    """blissgpu_group_knn_weighted itself -> (rc, idx, dist, status)"""
    from bliss_rs_amd import _ffi

    S, X = np.ascontiguousarray(S, np.float32), np.ascontiguousarray(X, np.float32)
    off = np.asarray(off, np.uint64)
    G = off.shape[0] - 1
    idx, dist, st = np.zeros((G, k), np.uint32), np.zeros((G, k), np.float32), np.full(G, -7, np.int32)
    sk = None if skip is None else np.where(np.asarray(skip) < 0, 0xFFFFFFFF, skip).astype(np.uint32)
    W = None if W is None else np.ascontiguousarray(W, np.float32)
    p = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
    rc = _ffi.lib().blissgpu_group_knn_weighted(p(S), off.ctypes.data, G, p(X), X.shape[0], X.shape[1], p(W), p(sk), k,
                                                idx.ctypes.data, dist.ctypes.data, st.ctypes.data)
    out = idx.astype(np.int64)
    out[idx == 0xFFFFFFFF] = -1
    return rc, out, dist, st


def device_form(ctx, S, off, X, k, W=None, skip=None):
    """-> (idx, dist, status)"""
    import torch

    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()  # noqa: E731
    idx, dist, st = ctx.group_knn(t(S, np.float32), off, t(X, np.float32), k, skip=t(skip, np.int32),
                                  weights="variance" if W is None else t(W, np.float32))
    ctx.synchronize()
    return idx.cpu().numpy().astype(np.int64), dist.cpu().numpy(), st.cpu().numpy()


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "indices", int((got[0] != want[0]).any(axis=1).sum()), "rows differ")
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (what, "distance bits")


def check_both(bliss, ctx, S, off, X, k, W, skip, want, status, what=""):
    """W = None: derived weights, `status` the expected few-seeds flags; otherwise status must be all 0"""
    assert_same(host_form(bliss, S, off, X, k, W, skip), want, (what, "host form"))
    got = device_form(ctx, S, off, X, k, W, skip)
    assert_same(got, want, (what, "device form"))
    assert np.array_equal(got[2], np.asarray(status, np.int32)), (what, "status")


# ---- 1. the weights alone ----
_SIZES = (0, 1, 2, 3, 8, 9, 31, 32, 33, 64, 65, 300, 5000)


def _weights_case(rng, d, grid):
    draw = (lambda m: (rng.integers(-8, 9, (m, d)) / 8).astype(np.float32)) if grid else \
        (lambda m: rng.standard_normal((m, d)).astype(np.float32))
    groups = [draw(m) for m in _SIZES]
    groups.append(np.repeat(draw(1), 5, axis=0))  # identical rows: variance 0, every weight 1.0
    two = (2.0 * rng.standard_normal((2, d))).astype(np.float32)  # two seeds that agree in the first coordinate only
    two[1, 0] = two[0, 0]
    groups.append(two)
    nan = draw(4)
    nan[2, d // 2] = np.nan
    groups.append(nan)
    sizes = [g.shape[0] for g in groups]
    return np.ascontiguousarray(np.concatenate(groups)), offsets_of(sizes)


@pytest.mark.parametrize("d", (23, 20, 7, 64, 1))
def test_weights_alone(bliss, ctx, oracle, d):
    import torch

    rng = np.random.default_rng(100 + d)
    for grid in (True, False):
        S, off = _weights_case(rng, d, grid)
        W, few = expected_weights(oracle, S, off)
        G = off.shape[0] - 1
        ident, two, nan = G - 3, G - 2, G - 1
        # on the expected values alone: the cases are what they are meant to be
        assert few.tolist() == [True, True] + [False] * (G - 2)
        assert (W[ident] == 1.0).all() and np.isnan(W[nan]).all() and np.isfinite(W[:nan]).all()
        if d == 23:
            print(f"two-seed group: weights {W[two].min():.3g} .. {W[two].max():.5g}")
            assert W[two].min() < 1e-4 and W[two].max() > 22.9
        got_h = bliss.playlist.group_variance_weights((S, off))
        tw, ts = ctx.group_weights(torch.from_numpy(S).cuda(), off)
        ctx.synchronize()
        got_d = (tw.cpu().numpy(), ts.cpu().numpy() != 0)
        for name, (gw, gf) in (("host form", got_h), ("device form", got_d)):
            assert gw.shape == W.shape and gw.dtype == np.float32
            assert np.array_equal(gf, few), (d, grid, name, "status")
            bad = np.flatnonzero((gw[:nan].view(np.uint32) != W[:nan].view(np.uint32)).any(axis=1))
            assert bad.size == 0, (d, grid, name, "weight bits differ in groups", bad.tolist())
            assert np.isnan(gw[nan]).all(), (d, grid, name, "the group with a NaN row")
        assert np.array_equal(ts.cpu().numpy(), few.astype(np.int32))  # BLISSGPU_GROUP_TOO_FEW_SEEDS is 1


# ---- 2. mixed groups on the tie-rich grid, derived weights ----
def _mixed_groups(rng, n):
    """120 singles, 100 groups of 2-8, 30 of 9-64, one of 300, one of 700, shuffled; members are distinct rows of the library"""
    sizes = np.concatenate([np.ones(120, np.int64), rng.integers(2, 9, 100), rng.integers(9, 65, 30), [300, 700]])
    sizes = rng.permutation(sizes)
    assert sizes.sum() <= n
    return sizes, rng.permutation(n)[:sizes.sum()]


_SHARED = {}


def _mixed_case(oracle, d, n=3000):
    """the inputs and the expected weights and scores, computed once per d"""
    if d not in _SHARED:
        rng = np.random.default_rng(1)
        X = tie_rich(rng, n, d, copies=2)  # half of the rows are copies of other rows
        sizes, members = _mixed_groups(rng, n)
        off = offsets_of(sizes)
        W, few = expected_weights(oracle, X[members], off)
        score = scores_of(oracle, X[members], off, X, W)
        for a in (X, sizes, members, off, W, few, score):
            a.setflags(write=False)
        _SHARED[d] = (X, sizes, members, off, W, few, score)
    return _SHARED[d]


@pytest.mark.parametrize("d", (23, 20))
def test_mixed_groups_on_a_tie_rich_grid(bliss, ctx, oracle, d):
    X, sizes, members, off, W, few, score = _mixed_case(oracle, d)
    S = X[members]
    multi, single = np.flatnonzero(sizes > 1), np.flatnonzero(sizes == 1)
    ties = _ties_at_cut(score, off, 32, members, multi)
    print(f"d={d}: {ties} of {multi.size} multi-seed groups tie at the cut k=32")
    assert multi.size == 132 and ties >= 20  # on the expected values alone: the tie rule at the cut is exercised
    # the singles: the identity's scores, which on the oracle are its euclidean ones bit for bit
    assert few[single].all() and not few[multi].any()
    eu = oracle.pairwise(S[off[single]], X, "euclidean", None, n_threads=16)
    assert np.array_equal(score[single].view(np.uint32), (np.float32(0.0) + eu).view(np.uint32))
    for k in (1, 8, 32):
        want = expected_from_scores(score, off, k, members)
        check_both(bliss, ctx, S, off, X, k, None, members, want, few, what=(d, k))
    rc, idx, dist, st = raw_host_form(S, off, X, 32, None, members)
    assert rc == 0 and np.array_equal(st, few.astype(np.int32))
    again = device_form(ctx, S, off, X, 32, None, members)
    assert_same(device_form(ctx, S, off, X, 32, None, members), again, "the same call twice")
    assert_same((idx, dist), again, "host and device form")


# ---- 3. one big group: cut by candidates, streamed through the seed tile ----
def test_one_big_group(bliss, ctx, oracle):
    import torch

    from bliss_rs_amd import _ffi

    rng = np.random.default_rng(5)
    n, big, k = 12_000, 3000, 32
    X = tie_rich(rng, n, 23)
    sizes = np.concatenate([np.ones(25, np.int64), [big], np.ones(25, np.int64)])
    members = rng.permutation(n)[:sizes.sum()]
    off = offsets_of(sizes)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    o64, n_items, seed_tile = off.astype(np.uint64), C.c_uint64(), C.c_uint32()
    items = np.zeros((4096, 4), np.uint32)
    _ffi.check(_ffi.lib().blissgpu_group_knn_plan(o64.ctypes.data, len(sizes), n, k, n_cus, items.ctypes.data, 4096,
                                                  C.byref(n_items), None, C.byref(seed_tile)))
    items = items[:n_items.value]
    of_big = items[(items[:, 0] == 25) & (items[:, 1] == 26)]
    print(f"{n_cus} CUs: {n_items.value} items, {len(of_big)} of them for the big group; seed tile {seed_tile.value}")
    assert len(of_big) > 1 and big > seed_tile.value
    S = X[members]
    W, few = expected_weights(oracle, S, off)
    want = expected_from_scores(scores_of(oracle, S, off, X, W), off, k, members)
    check_both(bliss, ctx, S, off, X, k, None, members, want, few)


# ---- 4. given weights ----
def test_given_weights(bliss, ctx, oracle):
    rng = np.random.default_rng(12)
    n, d = 1500, 23
    X = tie_rich(rng, n, d)
    sizes = np.array([1, 0, 3, 1, 8, 0, 33, 40, 2, 1, 100, 0, 5, 17])
    members = rng.permutation(n)[:sizes.sum()]
    off = offsets_of(sizes)
    W = rng.uniform(0.05, 4.0, (len(sizes), d)).astype(np.float32)  # a positive row per group, singles and empty ones included
    S = X[members]
    score = scores_of(oracle, S, off, X, W)
    for k in (1, 32):
        want = expected_from_scores(score, off, k, members)
        check_both(bliss, ctx, S, off, X, k, W, members, want, np.zeros(len(sizes)), what=k)
    rc, idx, dist, st = raw_host_form(S, off, X, 32, W, members)
    assert rc == 0 and (st == 0).all()
    assert_same((idx, dist), expected_from_scores(score, off, 32, members), "the C host form")


# ---- 5. any other feature count ----
@pytest.mark.parametrize("d", (7, 64))
def test_generic_path(bliss, ctx, oracle, d):
    rng = np.random.default_rng(8)
    X = tie_rich(rng, 1500, d)
    sizes = rng.permutation(np.concatenate([np.ones(40, np.int64), rng.integers(2, 9, 20), [100]]))
    members = rng.permutation(1500)[:sizes.sum()]
    off = offsets_of(sizes)
    S = X[members]
    W, few = expected_weights(oracle, S, off)
    score = scores_of(oracle, S, off, X, W)
    print(f"d={d}: {_ties_at_cut(score, off, 32, members, np.flatnonzero(sizes > 1))} of {(sizes > 1).sum()} multi-seed groups "
          "tie at the cut k=32")
    for k in (1, 32):
        check_both(bliss, ctx, S, off, X, k, None, members, expected_from_scores(score, off, k, members), few, what=(d, k))
    Wg = rng.uniform(0.05, 4.0, (len(sizes), d)).astype(np.float32)
    want = expected_from_scores(scores_of(oracle, S, off, X, Wg), off, 32, members)
    check_both(bliss, ctx, S, off, X, 32, Wg, members, want, np.zeros(len(sizes)), what=(d, "given weights"))


# ---- 6. skip, padding, edges ----
def test_skip_padding_and_edges(bliss, ctx, oracle):
    rng = np.random.default_rng(4)
    X = tie_rich(rng, 3000, 23)
    small = X[:40]

    def run(S, off, Xc, k, skip, what=""):
        off = np.asarray(off, np.int64)
        W, few = expected_weights(oracle, S, off)
        want = expected_from_scores(scores_of(oracle, S, off, Xc, W), off, k, skip)
        check_both(bliss, ctx, S, off, Xc, k, None, skip, want, few, what=what)
        return want

    # fewer eligible candidates than k: a group of 30 of the 40 rows, members skipped, k = 16 > 10
    members = np.arange(5, 35)
    w = run(small[members], [0, 30], small, 16, members, what="fewer eligible than k")
    assert (w[0][0, :10] >= 0).all() and (w[0][0, 10:] == -1).all() and np.isinf(w[1][0, 10:]).all()
    assert not np.isin(w[0][0, :10], members).any()
    # k = 1024 with n = 40, groups of several sizes, one of them empty; row 9 is a seed twice (its distance counts twice and
    # its row counts twice in the variance; one skip is enough)
    members = np.array([3, 9, 9, 1, 39, 0, 17])
    w = run(small[members], [0, 1, 3, 3, 7], small, 1024, members, what="k = 1024, n = 40")
    assert [(row >= 0).sum() for row in w[0]] == [39, 39, 40, 36]
    assert np.array_equal(w[0][2], np.concatenate([np.arange(40), np.full(984, -1)])) and (w[1][2, :40] == 0.0).all()
    # n = 1, with and without the skip
    S = X[100:103]
    run(S, [0, 2, 3], X[:1], 3, None, what="n = 1")
    run(S, [0, 2, 3], X[:1], 3, np.array([0, -1, -1]), what="n = 1, skipped by the first group")
    run(S, [0, 2, 3], X[:1], 3, np.array([-1, 0, 0]), what="n = 1, skipped by both")
    # only empty groups: the first k candidates, scores 0
    w = run(X[:0], [0, 0, 0], X, 5, None, what="empty groups")
    assert np.array_equal(w[0], np.tile(np.arange(5), (2, 1))) and (w[1] == 0.0).all()
    # a seed that appears twice in a group of two: variance 0, every weight 1.0 -- twice the euclidean distance
    w = run(X[[7, 7]], [0, 2], X, 8, np.array([7, -1]), what="the same seed twice")
    eu = oracle.pairwise(X[[7]], X, "euclidean", None)[0]
    assert np.array_equal(w[1][0], np.sort(np.delete(eu + eu, 7), kind="stable")[:8])


# ---- 7. NaN ----
def test_nan_weights(bliss, ctx, oracle):
    rng = np.random.default_rng(6)
    X = rng.standard_normal((4, 23)).astype(np.float32)
    S = rng.standard_normal((9, 23)).astype(np.float32)
    S[4, 11] = np.nan  # in the second group: all of its weights are NaN, and so is every score of that group
    off = np.array([0, 2, 6, 9])
    W, few = expected_weights(oracle, S, off)
    assert np.isnan(W[1]).all() and np.isfinite(W[[0, 2]]).all()
    score = scores_of(oracle, S, off, X, W)
    assert np.isnan(score[1]).all() and np.isfinite(score[[0, 2]]).all()
    # every candidate skipped by the NaN group: none of its scores is looked at
    skip = np.full(9, -1)
    skip[2:6] = [0, 1, 2, 3]
    want = expected_from_scores(np.where(np.isnan(score), np.inf, score), off, 3, skip)
    assert (want[0][1] == -1).all()
    check_both(bliss, ctx, S, off, X, 3, None, skip, want, few, what="the NaN group skips every candidate")
    skip[5] = -1  # one eligible candidate
    with pytest.raises(ValueError):
        host_form(bliss, S, off, X, 3, None, skip)
    assert raw_host_form(S, off, X, 3, None, skip)[0] == 5  # BLISSGPU_ERR_NAN
    with pytest.raises(bliss.BlissGpuError) as e:
        device_form(ctx, S, off, X, 3, None, skip)
    assert e.value.code == 5
    # the device form reports a skip entry that is no candidate (the host form checks it on the host)
    skip[5], skip[0] = 3, 4
    with pytest.raises(bliss.BlissGpuError) as e:
        device_form(ctx, S, off, X, 3, None, skip)
    assert e.value.code == 2


# ---- 8. structure ----
def test_launch_count_is_independent_of_the_shape(bliss, ctx):
    import torch

    rng = np.random.default_rng(9)
    counts = {"derived": [], "given": []}
    ctx.profile_enable(True)
    try:
        for G, n in ((50, 5000), (2000, 20_000)):
            tX = torch.from_numpy(rng.standard_normal((n, 23)).astype(np.float32)).cuda()
            sizes = rng.integers(1, 12, G)
            sizes[G // 2] = n // 4
            members = rng.permutation(n)[:sizes.sum()]
            tS = tX[torch.from_numpy(members).cuda()].contiguous()
            skip = torch.from_numpy(members.astype(np.int32)).cuda()
            tW = torch.from_numpy(rng.uniform(0.5, 2.0, (G, 23)).astype(np.float32)).cuda()
            for mode, weights in (("derived", "variance"), ("given", tW)):
                ctx.synchronize()
                ctx.profile_reset()
                ctx.group_knn(tS, offsets_of(sizes), tX, 32, skip=skip, weights=weights)
                ctx.synchronize()
                prof = ctx.profile()
                launches = {name: v[1] for name, v in prof.items() if v[1]}
                counts[mode].append(sum(c for name, c in launches.items() if name == "group_weights_kernel" or name.startswith("group_knn_")))
                for name in launches:
                    assert not (name.startswith("pairwise") or name.startswith("set_distance") or name.startswith("radix_")), launches
                print(f"G={G} n={n} {mode}: {launches}")
    finally:
        ctx.profile_enable(False)
    assert counts["derived"] == [3, 3] and counts["given"] == [2, 2], counts


# ---- 9. the library ----
def test_library_group_playlists_is_one_call(bliss, oracle, tmp_path, monkeypatch):
    from bliss_rs_amd import _ffi

    P = bliss.playlist
    rng = np.random.default_rng(10)
    n, k = 2000, 10
    X = tie_rich(rng, n, 23)
    V2 = bliss.FeaturesVersion.Version2
    album = [None if i % 17 == 5 else f"album {int(a):03d}" for i, a in enumerate(rng.integers(0, 150, n))]
    for i in (40, 700, 1999):
        album[i] = f"single {i}"  # some single-song albums
    songs = [bliss.Song(path=f"/music/{i:05d}.flac", title=f"t{i}", artist="a", album=album[i], duration=1.0,
                        analysis=bliss.Analysis(X[i], V2), features_version=V2) for i in range(n)]
    db = str(tmp_path / "bliss.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs)
    lib = _ffi.lib()
    calls = []
    real = lib.blissgpu_group_knn_weighted

    def counted(*a):
        calls.append(1)
        return real(*a)

    monkeypatch.setattr(lib, "blissgpu_group_knn_weighted", counted)
    with pytest.raises(bliss.ProviderError):  # the default policy: the reference's error for the single-song albums
        bliss.library.group_playlists(db, k, by="album", metric_builder=P.VarianceWeights())
    assert not calls
    table = bliss.library.group_playlists(db, k, by="album", metric_builder=P.VarianceWeights(few_seeds="euclidean"))
    assert len(calls) == 1 and len(table) == len({a for a in album if a is not None}) == 153
    monkeypatch.undo()
    path_row = {s.path: i for i, s in enumerate(songs)}
    checked_single = 0
    for key in list(table)[::10] + ["single 700"]:
        rows = [i for i in range(n) if album[i] == key]
        paths = [songs[i].path for i in rows]
        if len(rows) >= 2:
            M = P.variance_based_weight_matrix(list(X[rows]))
            assert np.array_equal(M.view(np.uint32), oracle.variance_based_weight_matrix(X[rows]).view(np.uint32))
            builder = P.MahalanobisBuilder(M)
        else:
            M, builder = np.eye(23, dtype=np.float32), P.euclidean_distance
            checked_single += 1
        contract = bliss.library.playlist_from_custom(db, paths, builder, P.closest_to_songs, deduplicate=False)[len(paths):][:k]
        assert [p for p, _ in table[key]] == [s.path for s in contract], key
        score = scores_of(oracle, X[rows], np.array([0, len(rows)]), X, np.diagonal(M)[None, :])[0]
        assert [np.float32(v) for _, v in table[key]] == [score[path_row[p]] for p, _ in table[key]], key
    assert checked_single >= 1
    # the same metric through playlist_from_custom itself
    rows = [i for i in range(n) if album[i] == list(table)[0]]
    paths = [songs[i].path for i in rows]
    got = bliss.library.playlist_from_custom(db, paths, P.VarianceWeights(), P.closest_to_songs, deduplicate=False)
    assert [s.path for s in got[len(paths):][:k]] == [p for p, _ in table[list(table)[0]]]


# ---- the host form's staging: every optional argument given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("skip,dist,status,weights", ((True, True, True, True), (False, False, False, False), (True, True, True, False),
                                                      (False, True, False, True), (True, False, True, False), (False, False, True, True)))
def test_host_form_stages_like_the_device_form(bliss, ctx, skip, dist, status, weights):
    import staging_cases as sc

    def build(c, dev):
        idx, dd = dev(sc.out((c.G, c.k), np.uint32)), dev(sc.out((c.G, c.k), np.float32, dist))
        st = dev(sc.out((c.G,), np.int32, status))
        return [dev(c.S), c.off, c.G, dev(c.X), c.n, sc.D, dev(c.W if weights else None), dev(c.skip if skip else None), c.k, idx, dd,
                st], [idx, dd, st]

    sc.check(bliss, ctx, "group_knn_weighted", build)


@pytest.mark.parametrize("status", (True, False))
def test_group_weights_host_form_stages_like_the_device_form(bliss, ctx, status):
    import staging_cases as sc

    def build(c, dev):
        w, st = dev(sc.out((c.G, sc.D), np.float32)), dev(sc.out((c.G,), np.int32, status))
        return [dev(c.S), c.off, c.G, sc.D, w, st], [w, st]

    sc.check(bliss, ctx, "group_weights", build, lists=False)
