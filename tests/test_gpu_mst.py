"""GPU tests (-m gpu) of the minimum spanning tree on the device (blissgpu_mst / blissgpu_mst_device: mst_scan_kernel,
mst_pick_kernel, the merge of mst_merge.hpp between the rounds).  Expected values never come from the code under test: the
reference is the contract of include/blissgpu.h written out in numpy (tests/test_mst_host.py: Kruskal over all pairs under the
key (bits of w, i, j)) applied to playlist.pairwise_distances(X, X) from the device, which other tests hold to the oracle.  Every
comparison is exact -- edge_u, edge_v and the bits of edge_w -- for both forms; no tolerance appears anywhere."""
import math

import numpy as np
import pytest

from test_mst_host import bits, contract, core_of, equal_input, grid_input, random_input, same_tree, twice_input

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_OOM = 2, 4


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


def builder_of(P, metric, M):
    return P.euclidean_distance if metric == "euclidean" else P.MahalanobisBuilder(M)


def device_form(ctx, X, metric="euclidean", M=None, core=None):
    u, v, w, rounds = ctx.mst(X, metric, M, core)
    assert u.dtype == np.int32 and v.dtype == np.int32 and w.dtype == np.float32
    return (u.astype(np.int64), v.astype(np.int64), w), rounds


def check(bliss, ctx, X, metric="euclidean", M=None, core=None, what=""):
    """both forms against the contract over the device's all-pairs matrix; -> (the matrix, the tree)"""
    P = bliss.playlist
    n = X.shape[0]
    Dm = P.pairwise_distances(X, X, metric, M)
    want = contract(Dm, core)
    got, rounds = device_form(ctx, X, metric, M, core)
    assert same_tree(got, want), (what, "device", got, want)
    assert 1 <= rounds <= math.ceil(math.log2(n)), (what, rounds)
    if core is None:
        t = P.minimum_spanning_tree(X, builder_of(P, metric, M))
        assert same_tree((t.u, t.v, t.w), want) and t.rounds == rounds and t.n == n, (what, "host")
    return Dm, want


def pd_matrix(d, seed, diagonal=False):
    rng = np.random.default_rng(seed)
    if diagonal:
        return np.diag(rng.uniform(0.2, 3.0, d)).astype(np.float32)
    A = rng.standard_normal((d, d))
    return (A @ A.T / d + 0.5 * np.eye(d)).astype(np.float32)


# ---- sizes and shapes ----
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_at_23_features(bliss, ctx, n):
    check(bliss, ctx, random_input(n, 23, seed=100 + n), what=n)


def test_3000_songs_and_several_column_groups(bliss, ctx, monkeypatch):
    """more than one tile per column group, and with the column groups forced, more than one partial winner per song"""
    X = random_input(3000, 23, seed=31)
    Dm, want = check(bliss, ctx, X, what=3000)
    for groups in (1, 3, 7, 47):
        monkeypatch.setenv("BLISSGPU_MST_COL_GROUPS", str(groups))
        got, _ = device_form(ctx, X)
        assert same_tree(got, want), groups
    monkeypatch.delenv("BLISSGPU_MST_COL_GROUPS")
    # clustered and sorted: in the late rounds whole wavefronts and whole tiles lie in one component -- with and without the skip
    X = X.copy()
    X[1000:2000] += 40.0
    X[2000:] -= 40.0
    _, want = check(bliss, ctx, X, what="clustered")
    assert (np.sort(want[2])[-2:] > 100).all()
    monkeypatch.setenv("BLISSGPU_MST_SKIP", "0")
    got, _ = device_form(ctx, X)
    assert same_tree(got, want)


def test_other_feature_counts(bliss, ctx):
    check(bliss, ctx, random_input(1000, 20, seed=32), what="d=20")
    for d in (7, 64):  # the generic form
        check(bliss, ctx, random_input(500, d, seed=33 + d), what=d)


@pytest.mark.parametrize("d,n", [(23, 1000), (20, 300), (7, 300)])
def test_mahalanobis(bliss, ctx, d, n):
    X = random_input(n, d, seed=40 + d)
    check(bliss, ctx, X, "mahalanobis", pd_matrix(d, 41, diagonal=True), what=("diagonal", d))
    check(bliss, ctx, X, "mahalanobis", pd_matrix(d, 42), what=("full", d))


# ---- what is refused ----
def _raw_host_call(bliss, X, metric=0, M=None, core=None):
    from bliss_rs_amd import _ffi

    n, d = X.shape
    out = [np.full(n, 7, np.uint32), np.full(n, 7, np.uint32), np.full(n, 7.0, np.float32)]
    rc = _ffi.lib().blissgpu_mst(X.ctypes.data, n, d, metric, None if M is None else M.ctypes.data,
                                 None if core is None else core.ctypes.data, *(a.ctypes.data for a in out), None)
    return rc, _ffi.lib().blissgpu_last_error(), out


def test_nan_distances_are_invalid_and_nothing_is_written(bliss, ctx):
    X = random_input(300, 23, seed=50)
    bad = X.copy()
    bad[123, 4] = np.nan
    rc, err, out = _raw_host_call(bliss, bad)
    assert rc == ERR_INVALID and b"NaN" in err and all((a == 7).all() for a in out)
    M = np.eye(23, dtype=np.float32)
    M[3, 3] = -50.0  # not positive semi-definite: negative sums
    assert (np.isnan(bliss.playlist.pairwise_distances(X, X, "mahalanobis", M))).any()
    rc, err, out = _raw_host_call(bliss, X, 2, M)
    assert rc == ERR_INVALID and b"NaN" in err and all((a == 7).all() for a in out)
    for value in (np.nan, -1.0):
        core = np.ones(300, np.float32)
        core[77] = value
        rc, err, out = _raw_host_call(bliss, X, core=core)
        assert rc == ERR_INVALID and b"core" in err and all((a == 7).all() for a in out)
    for arrays in ((bad, "euclidean", None, None), (X, "mahalanobis", M, None), (X, "euclidean", None, np.full(300, np.nan, np.float32))):
        with pytest.raises(bliss.BlissGpuError) as e:
            ctx.mst(*arrays)
        assert e.value.code == ERR_INVALID
    for d in (7,):  # the generic form too
        bad = random_input(100, d, seed=51)
        bad[5, 2] = np.nan
        with pytest.raises(bliss.BlissGpuError) as e:
            ctx.mst(bad)
        assert e.value.code == ERR_INVALID
    with pytest.raises(bliss.BlissGpuError) as e:
        ctx.mst(X, "cosine")
    assert e.value.code == ERR_INVALID
    # an infinite feature is not a NaN distance: that song hangs on the tree by an edge of weight +inf
    far = X.copy()
    far[9] = np.inf
    _, want = check(bliss, ctx, far, what="inf")
    assert np.isinf(want[2][-1]) and np.isfinite(want[2][:-1]).all() and 9 in (want[0][-1], want[1][-1])
    # the context is as good as before
    check(bliss, ctx, X, what="afterwards")


def test_workspace_limit(bliss, ctx):
    X = random_input(3000, 23, seed=52)
    limit = ctx.workspace_limit()
    ctx.profile_enable(True)
    try:
        ctx.set_workspace_limit(1 << 20)  # (the smallest limit) 60 000 songs: order, components and picks alone are 1.2 MB
        ctx.profile_reset()
        with pytest.raises(bliss.BlissGpuError) as e:
            ctx.mst(np.zeros((60000, 23), np.float32))
        assert e.value.code == ERR_OOM
        assert not [name for name, v in ctx.profile().items() if v[1]]  # nothing was launched
    finally:
        ctx.set_workspace_limit(limit)
        ctx.profile_enable(False)
    check(bliss, ctx, X[:500], what="afterwards")


# ---- ties ----
def test_all_songs_identical(bliss, ctx):
    """every weight is +0: the tree is the star from song 0 in key order, whatever order the kernel walks in"""
    for n in (300, 1000):
        X = equal_input(n)
        _, want = check(bliss, ctx, X, what="equal")
        assert (want[0] == 0).all() and want[1].tolist() == list(range(1, n)) and not bits(want[2]).any()


def test_integer_grid(bliss, ctx):
    check(bliss, ctx, grid_input(1000), what="grid")


def test_every_row_twice(bliss, ctx):
    _, want = check(bliss, ctx, twice_input(200), what="twice")
    assert (bits(want[2])[:100] == 0).all() and bits(want[2])[100] != 0


@pytest.mark.parametrize("m", [5, 50])
def test_core_distances_make_plateaus(bliss, ctx, m):
    P = bliss.playlist
    X = random_input(1000, 23, seed=60)
    Dm = P.pairwise_distances(X, X)
    core = P.core_distances(X, m)
    assert np.array_equal(bits(core), bits(core_of(Dm, m)))  # the k-nearest search's distances are the all-pairs ones
    want = contract(Dm, core)
    assert len(np.unique(bits(want[2]))) < 999  # plateaus: the index decides
    got, rounds = device_form(ctx, X, core=core)
    assert same_tree(got, want) and rounds <= 10
    t = P.minimum_spanning_tree(X, min_samples=m)
    assert same_tree((t.u, t.v, t.w), want)
    if m == 5:  # a Mahalanobis metric and the generic form with cores
        M = pd_matrix(23, 61)
        DM = P.pairwise_distances(X[:400], X[:400], "mahalanobis", M)
        t = P.minimum_spanning_tree(X[:400], P.MahalanobisBuilder(M), min_samples=m)
        assert same_tree((t.u, t.v, t.w), contract(DM, core_of(DM, m)))
        Y = random_input(300, 9, seed=62)
        DY = P.pairwise_distances(Y, Y)
        t = P.minimum_spanning_tree(Y, min_samples=m)
        assert same_tree((t.u, t.v, t.w), contract(DY, core_of(DY, m)))


# ---- the rest ----
def test_two_runs_give_the_same_bytes_and_a_stale_workspace_does_not_show(ctx):
    big, small = grid_input(2000, seed=70), random_input(130, 23, seed=71)
    first = [device_form(ctx, X)[0] for X in (big, small, big, small)]
    for a, b in ((first[0], first[2]), (first[1], first[3])):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_launches(bliss, ctx):
    P = bliss.playlist
    X = random_input(1000, 23, seed=72)
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        _, rounds = device_form(ctx, X)
        prof = {name: v[1] for name, v in ctx.profile().items() if v[1]}
        print(prof)
        assert prof == {"mst_scan_kernel": rounds, "mst_pick_kernel": 2 * rounds}  # no distance matrix is formed
    finally:
        ctx.profile_enable(False)
    # with min_samples: the k-nearest search for the cores, then the tree -- tensors on the device throughout
    import torch

    Xt = torch.from_numpy(X).to(torch.device("cuda", ctx.device))
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        _, dist = ctx.knn(Xt, Xt, 5, skip=torch.arange(1000, dtype=torch.int32, device=Xt.device))
        u, v, w, rounds = ctx.mst(Xt, core=dist[:, 4].contiguous())
        prof = {name: v[1] for name, v in ctx.profile().items() if v[1]}
        print(prof)
        assert prof["mst_scan_kernel"] == rounds and any(name.startswith("knn_") for name in prof)
        assert all(name.startswith(("mst_", "knn_")) for name in prof)
        assert not [name for name in prof if name.startswith(("pairwise", "set_distance", "radix_"))]
    finally:
        ctx.profile_enable(False)
    assert torch.is_tensor(u) and u.is_cuda and u.dtype == torch.int32 and w.dtype == torch.float32
    t = P.minimum_spanning_tree(X, min_samples=5)
    assert same_tree((u.cpu().numpy().astype(np.int64), v.cpu().numpy().astype(np.int64), w.cpu().numpy()), (t.u, t.v, t.w))


# ---- the host form's staging: core given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("core", (True, False))
def test_host_form_stages_like_the_device_form(bliss, ctx, core):
    import staging_cases as sc

    def build(c, dev):
        X = c.X + (np.arange(c.n, dtype=np.float32) * np.float32(1e-3))[:, None]  # (no two rows equal)
        cr = np.linspace(0.0, 0.5, c.n).astype(np.float32) if core else None
        u, v, w = dev(sc.out((c.n - 1,), np.uint32)), dev(sc.out((c.n - 1,), np.uint32)), dev(sc.out((c.n - 1,), np.float32))
        rounds = np.full(1, 99, np.uint32)  # (host memory in both forms)
        return [dev(X), c.n, sc.D, 2, dev(c.M), dev(cr), u, v, w, rounds], [u, v, w, rounds]

    sc.check(bliss, ctx, "mst", build, lists=False)
