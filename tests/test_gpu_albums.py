"""GPU tests (-m gpu) of the k nearest albums per seed group (blissgpu_album_knn / blissgpu_album_knn_device:
segment_mean_kernel + album_knn_scan_kernel + knn_merge_kernel): closest_album_to_group of the reference
(src/playlist.rs:424-485) cut after k albums, for many groups in one call.  Expected values never come from the code under
test: means are sequential numpy-f32 row sums in this file, distances are oracle.pairwise(mean[None], centroids, "euclidean"),
the order is numpy's stable argsort over the existing albums in album order, i.e. over (dist, album index).  Every comparison is
exact: np.array_equal on indices, bit equality on dist, group_means and centroids (NaN rows of empty albums by NaN-ness)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, A, BIG = 1500, 700, 400  # songs, album indices (one of them unused), songs of the largest album
UNUSED = 3                  # the album index no song uses
DIMS = (23, 20, 1, 64)
KS = (1, 5, 64, 1024)


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


def mixed_grid(rng, n, d):
    """a coarse grid of eighths at two magnitudes, 1e4 x and 1e-3 y: the order of an f32 sum shows in its bits"""
    x = rng.integers(-8, 9, (n, d)) / 8
    return np.where(rng.random((n, d)) < 0.5, 1e4 * x, 1e-3 * x).astype(np.float32)


def seq_mean(rows):
    """(0.0f + row_0 + row_1 + ...) / (float)count, every operation in f32"""
    acc = np.zeros(rows.shape[1], np.float32)
    for r in rows:
        acc = acc + r
    return acc / np.float32(rows.shape[0])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def layout(rng):
    """-> (album_of int64[N], rows of every album): album UNUSED has no song, album 0 has BIG songs, about 100 songs have no
    album, the other albums hold 12, 3, 2 or 1 songs; the songs of an album are scattered over the candidates"""
    sizes = np.ones(A, np.int64)
    sizes[UNUSED], sizes[0] = 0, BIG
    small = np.array([a for a in range(A) if a not in (0, UNUSED)])
    sizes[small[:5]] = 12
    sizes[small[5:75]] = 3
    sizes[small[75:182]] = 2
    assert sizes.sum() == N - 100
    album_of = np.full(N, -1, np.int64)
    album_of[rng.permutation(N)[:sizes.sum()]] = np.repeat(np.arange(A), sizes)
    return album_of, [np.flatnonzero(album_of == a) for a in range(A)]


def reference(oracle, S, off, X, album_of, rows, skip):
    """-> (group means [G, d], full-album centroids [A, d], dist [G, A], exists bool[G, A], patched {(g, a): centroid}): the
    contract in numpy f32 and the oracle's distances; dist[g, a] is only meaningful where exists[g, a]"""
    G = off.shape[0] - 1
    means = np.stack([seq_mean(S[off[g]:off[g + 1]]) for g in range(G)])
    centroids = np.stack([seq_mean(X[r]) if r.size else np.full(X.shape[1], np.nan, np.float32) for r in rows])
    dist = oracle.pairwise(means, centroids, "euclidean")
    exists = np.tile(np.array([r.size > 0 for r in rows]), (G, 1))
    patched = {}  # (group, album) -> the centroid of what the group leaves of the album
    for g in range(G):
        gone = set(int(j) for j in skip[off[g]:off[g + 1]] if j >= 0)
        touched = sorted(set(int(album_of[j]) for j in gone if album_of[j] >= 0))
        left = [np.array([i for i in rows[a] if i not in gone], np.int64) for a in touched]
        for a, r in zip(touched, left):
            if r.size == 0:
                exists[g, a] = False
            else:
                patched[g, a] = seq_mean(X[r])
        some = [a for a, r in zip(touched, left) if r.size]
        if some:
            dist[g, some] = oracle.pairwise(means[g][None], np.stack([patched[g, a] for a in some]), "euclidean")[0]
    return means, centroids, dist, exists, patched


def expected(dist, exists, k):
    G = dist.shape[0]
    idx, out = np.full((G, k), -1, np.int64), np.full((G, k), np.inf, np.float32)
    for g in range(G):
        cols = np.flatnonzero(exists[g])
        order = cols[np.argsort(dist[g, cols], kind="stable")][:k]  # cols ascend: equal distances in album order
        idx[g, :order.size] = order
        out[g, :order.size] = dist[g, order]
    return idx, out


class Case:
    """one data set of feature count d with its groups and everything the reference arithmetic says about it"""

    def __init__(self, oracle, d):
        rng = np.random.default_rng(1000 + d)
        self.d = d
        album_of, rows = layout(rng)
        X = mixed_grid(rng, N, d)
        size = np.array([r.size for r in rows])
        # planted ties: albums with identical rows, hence equal centroids -- six of two songs, seventy of one song
        twos, ones = np.flatnonzero(size == 2), np.flatnonzero(size == 1)
        self.tied2, self.tied1 = twos[:6], ones[:70]
        for a in self.tied2[1:]:
            X[rows[a]] = X[rows[self.tied2[0]]]
        for a in self.tied1[1:]:
            X[rows[a]] = X[rows[self.tied1[0]]]
        groups = []  # (seed rows f32[s, d], skip int64[s])
        # every album as its own group, all its rows skipped: the own album must be absent
        self.own = [a for a in range(A) if size[a]]
        for a in self.own:
            groups.append((X[rows[a]], rows[a]))
        # seeds that are no candidates; the first two sit exactly on the tied albums' centroids
        self.on_ties = [len(groups), len(groups) + 1]
        groups.append((X[rows[self.tied2[0]]].copy(), np.full(2, -1)))
        groups.append((X[rows[self.tied1[0]]].copy(), np.full(1, -1)))
        for s in (1, 4, 7):
            groups.append((mixed_grid(rng, s, d), np.full(s, -1)))
        # a group that takes some, not all, songs of five albums
        self.partial = len(groups)
        self.partial_albums = [0, int(np.flatnonzero(size == 12)[0])] + [int(a) for a in np.flatnonzero(size == 3)[:3]]
        take = np.concatenate([rows[0][[5, 200, 399]], rows[self.partial_albums[1]][::2]] + [rows[a][1:2] for a in self.partial_albums[2:]])
        groups.append((X[take], take))
        # a group that removes ALL songs of an album it is not named after, and one song of another
        self.removes_all = len(groups)
        self.removed_album = int(twos[10])
        take = np.concatenate([rows[self.removed_album], rows[int(np.flatnonzero(size == 3)[5])][:1]])
        groups.append((X[take], take))
        # a repeated seed
        take = np.array([rows[0][7], rows[int(twos[11])][0], rows[0][7]])
        groups.append((X[take], take))
        # 3 000 seeds: far more than anything staged at once; the first fifty leave the pool
        take = rng.integers(0, N, 3000)
        groups.append((X[take], np.where(np.arange(3000) < 50, take, -1)))
        self.huge = len(groups) - 1
        self.S = np.concatenate([g[0] for g in groups])
        self.skip = np.concatenate([g[1] for g in groups]).astype(np.int64)
        self.off = np.zeros(len(groups) + 1, np.int64)
        self.off[1:] = np.cumsum([g[0].shape[0] for g in groups])
        self.X, self.album_of, self.rows = X, album_of, rows
        self.reference(oracle)

    def reference(self, oracle):
        self.means, self.centroids, self.dist, self.exists, self.patched = reference(oracle, self.S, self.off, self.X, self.album_of,
                                                                                     self.rows, self.skip)

    def expected(self, k):
        return expected(self.dist, self.exists, k)

    def ties_at_cut(self, k):
        """groups with equal distances on both sides of the cut after k"""
        hit = 0
        for g in range(self.off.shape[0] - 1):
            s = np.sort(self.dist[g, self.exists[g]])
            hit += int(s.size > k and s[k - 1] == s[k])
        return hit


_CASES = {}


@pytest.fixture(scope="module")
def case(oracle):
    def get(d):
        if d not in _CASES:
            _CASES[d] = Case(oracle, d)
        return _CASES[d]
    return get


def host_form(bliss, c, k):
    return bliss.playlist.nearest_albums((c.S, c.off), c.X, c.album_of, k, skip=c.skip, return_means=True)


def device_form(ctx, c, k):
    import torch

    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()  # noqa: E731
    idx, dist, means, cent = ctx.album_knn(t(c.S, np.float32), c.off, t(c.X, np.float32), t(c.album_of, np.int32), A, k,
                                           t(c.skip, np.int32))
    ctx.synchronize()
    return idx.cpu().numpy().astype(np.int64), dist.cpu().numpy(), means.cpu().numpy(), cent.cpu().numpy()


def assert_same(got, c, want, what):
    idx, dist, means, cent = got
    assert np.array_equal(bits(means), bits(c.means)), (what, "group means", int((bits(means) != bits(c.means)).any(axis=1).sum()))
    empty = np.isnan(c.centroids).all(axis=1)
    assert np.array_equal(np.isnan(cent).all(axis=1), empty) and empty.sum() == 1 and empty[UNUSED], (what, "empty albums")
    assert np.array_equal(bits(cent[~empty]), bits(c.centroids[~empty])), (what, "centroids")
    bad = (idx != want[0]).any(axis=1)
    assert not bad.any(), (what, "indices", int(bad.sum()), "rows differ, first", int(np.flatnonzero(bad)[0]))
    assert np.array_equal(bits(dist), bits(want[1])), (what, "distance bits")


def test_the_data_asks_what_it_should(case):
    """the properties of the data sets that make the cases below mean something"""
    for d in DIMS:
        c = case(d)
        G = c.off.shape[0] - 1
        assert G >= 100 and c.X.shape == (N, d) and (c.album_of == -1).sum() == 100 and c.rows[UNUSED].size == 0
        assert c.rows[0].size == BIG and c.off[c.huge + 1] - c.off[c.huge] == 3000
        # the own album is absent for its group, and only it (those groups skip nothing else)
        for g, a in enumerate(c.own):
            assert not c.exists[g, a] and c.exists[g].sum() == len(c.own) - 1
        # the partial group's five patched centroids differ from the full ones
        assert len(c.partial_albums) == 5
        for a in c.partial_albums:
            assert c.exists[c.partial, a] and not np.array_equal(bits(c.patched[c.partial, a]), bits(c.centroids[a])), (d, a)
        assert not c.exists[c.removes_all, c.removed_album] and c.exists[c.removes_all].sum() == len(c.own) - 1
        # planted ties: equal centroids, and distance 0 from the groups that sit on them
        assert (bits(c.centroids[c.tied2]) == bits(c.centroids[c.tied2[0]])).all()
        assert (c.dist[c.on_ties[0], c.tied2] == 0).all() and (c.dist[c.on_ties[1], c.tied1] == 0).all()
        if d > 1:
            # rounding: the order of the sum shows.  numpy's mean(axis=0) of a row-major array IS the sequential sum (the
            # reduction runs over the outer axis, row by row), so it cannot differ; its pairwise summation -- the mean along the
            # contiguous axis of the transposed rows -- and the sum in reverse order do, for the albums and for the groups
            pairwise = sum(not np.array_equal(bits(np.ascontiguousarray(c.X[r].T).mean(axis=1)), bits(c.centroids[a]))
                           for a, r in enumerate(c.rows) if r.size)
            backwards = sum(not np.array_equal(bits(seq_mean(c.X[r[::-1]])), bits(c.centroids[a])) for a, r in enumerate(c.rows) if r.size)
            assert pairwise >= 1 and backwards >= 10, (d, pairwise, backwards)
            huge = c.S[c.off[c.huge]:c.off[c.huge + 1]]
            assert not np.array_equal(bits(np.ascontiguousarray(huge.T).mean(axis=1)), bits(c.means[c.huge]))
    assert sum(case(d).ties_at_cut(k) for d in DIMS for k in KS) > 0


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", DIMS)
def test_album_knn_host_and_device_forms(bliss, ctx, case, d, k):
    c = case(d)
    want = c.expected(k)
    if k < 1024:
        ties = c.ties_at_cut(k)
        print(f"d = {d}, k = {k}: {ties} groups with equal distances on both sides of the cut")
        assert ties > 0
    else:
        assert (want[0][:, -1] == -1).all() and np.isinf(want[1][:, -1]).all()  # k > A: padding
    host = host_form(bliss, c, k)
    assert_same(host, c, want, (d, k, "host form"))
    dev = device_form(ctx, c, k)
    assert_same(dev, c, want, (d, k, "device form"))
    for h, v in zip(host, dev):  # and the two forms agree bit for bit, NaN rows included
        assert np.array_equal(h.view(np.uint32) if h.dtype == np.float32 else h, v.view(np.uint32) if v.dtype == np.float32 else v)


def test_dist_may_be_null_and_means_stay_in_the_workspace(bliss, case):
    from bliss_rs_amd import _ffi

    c = case(23)
    idx, dist = bliss.playlist.nearest_albums((c.S, c.off), c.X, c.album_of, 5, skip=c.skip)
    want = c.expected(5)
    assert np.array_equal(idx, want[0]) and np.array_equal(bits(dist), bits(want[1]))
    G = c.off.shape[0] - 1
    out = np.empty((G, 5), np.uint32)
    album_u32 = np.where(c.album_of < 0, 0xFFFFFFFF, c.album_of).astype(np.uint32)
    skip_u32 = np.where(c.skip < 0, 0xFFFFFFFF, c.skip).astype(np.uint32)
    off = c.off.astype(np.uint64)
    _ffi.check(_ffi.lib().blissgpu_album_knn(c.S.ctypes.data, off.ctypes.data, G, c.X.ctypes.data, N, 23, album_u32.ctypes.data, A,
                                             skip_u32.ctypes.data, 5, out.ctypes.data, None, None, None))
    assert np.array_equal(np.where(out == 0xFFFFFFFF, -1, out.astype(np.int64)), want[0])
    # no candidates, or no albums: every row is padding
    for X, album_of in ((c.X[:0], c.album_of[:0]), (c.X, np.full(N, -1))):
        idx, dist = bliss.playlist.nearest_albums((c.S[:9], [0, 2, 9]), X, album_of, 4)
        assert (idx == -1).all() and np.isinf(dist).all()


def test_albums_shared_between_workgroups(bliss, ctx, oracle):
    """few groups, 6 000 albums: several workgroups share a group's albums (each walks a range of 256-album blocks and starts
    its cursor into the group's patches at its own first album), their partial lists are merged"""
    import torch

    rng = np.random.default_rng(31)
    n, n_albums, d, k = 6200, 6000, 23, 5
    marked = [10, 2047, 2048, 2100, 3000, 4095, 4096, 5999]  # two songs each: first / last albums of blocks, of the splits
    album_of = np.concatenate([np.arange(n_albums), np.repeat(marked, 2), rng.integers(0, n_albums, 200 - 2 * len(marked))])
    album_of = album_of[rng.permutation(n)]
    rows = [np.flatnonzero(album_of == a) for a in range(n_albums)]
    X = mixed_grid(rng, n, d)
    partial = np.array([rows[a][1] for a in marked])               # one of three songs of every marked album
    whole = np.concatenate([rows[a] for a in (2047, 4096, 5999)])  # every song of three of them
    lone = np.array([rows[a][0] for a in (1, 255, 256, 2049, 5998) if rows[a].size == 1])
    seeds = [(mixed_grid(rng, 3, d), np.full(3, -1)), (X[partial], partial), (X[whole], whole), (X[lone], lone),
             (X[np.concatenate([partial, whole])], np.concatenate([partial, whole])), (X[partial[::-1]], partial[::-1])]
    S = np.concatenate([g[0] for g in seeds])
    skip = np.concatenate([g[1] for g in seeds]).astype(np.int64)
    off = np.zeros(len(seeds) + 1, np.int64)
    off[1:] = np.cumsum([g[0].shape[0] for g in seeds])
    means, centroids, dist, exists, patched = reference(oracle, S, off, X, album_of, rows, skip)
    assert all(rows[a].size == 3 for a in marked) and not exists[2, 4096] and not exists[4, 5999] and (1, 2048) in patched
    want = expected(dist, exists, k)
    got = bliss.playlist.nearest_albums((S, off), X, album_of, k, skip=skip, return_means=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    assert np.array_equal(bits(got[2]), bits(means)) and np.array_equal(bits(got[3]), bits(centroids))
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()  # noqa: E731
    dev = ctx.album_knn(t(S, np.float32), off, t(X, np.float32), t(album_of, np.int32), n_albums, k, t(skip, np.int32))
    ctx.synchronize()
    assert np.array_equal(dev[0].cpu().numpy(), want[0]) and np.array_equal(bits(dev[1].cpu().numpy()), bits(want[1]))
    # the nearest albums of a group that sits on a patched centroid of the last split: that album, at distance 0, comes first
    on = np.stack([patched[1, 5999], patched[1, 10]])
    idx, dd = bliss.playlist.nearest_albums((on, [0, 1, 2]), X, album_of, 1, skip=np.array([partial[-1], partial[0]]))
    assert idx[:, 0].tolist() == [5999, 10] and (dd[:, 0] == 0).all()


def test_nan(bliss, ctx, case, oracle):
    """a NaN feature in an album that exists for some group is the reference's n32() panic; the same NaN in a song every group
    skips is never looked at"""
    import torch

    from bliss_rs_amd import _ffi

    c = case(23)
    a = c.partial_albums[2]  # three songs
    song = int(c.rows[a][1])
    X = c.X.copy()
    X[song, 11] = np.nan
    seeds = [np.array([song, c.rows[0][3]]), np.array([c.rows[a][0], song]), np.array([song])]
    S = np.concatenate([X[s] for s in seeds])
    off = np.array([0, 2, 4, 5])
    skip = np.concatenate(seeds)
    S[np.isnan(S)] = 0.25  # (the seeds themselves are clean: only the pool holds the NaN)
    # every group skips the song: its album is patched everywhere, the full-album centroid (NaN) is never looked at
    idx, dist, means, cent = bliss.playlist.nearest_albums((S, off), X, c.album_of, 5, skip=skip, return_means=True)
    assert np.isnan(cent[a]).any() and not np.isnan(dist).any()
    ref_means, _, ref_dist, ref_exists, _ = reference(oracle, S, off, X, c.album_of, c.rows, skip)
    want = expected(ref_dist, ref_exists, 5)
    assert np.array_equal(bits(means), bits(ref_means)) and np.array_equal(idx, want[0]) and np.array_equal(bits(dist), bits(want[1]))
    # one group that does not skip it: the album exists for that group with a NaN centroid
    skip2 = skip.copy()
    skip2[4] = -1
    with pytest.raises(ValueError):
        bliss.playlist.nearest_albums((S, off), X, c.album_of, 5, skip=skip2)
    t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).astype(dt)).cuda()  # noqa: E731
    with pytest.raises(_ffi.BlissGpuError) as e:
        ctx.album_knn(t(S, np.float32), off, t(X, np.float32), t(c.album_of, np.int32), A, 5, t(skip2, np.int32))
    assert e.value.code == _ffi.ERR_NAN
    out = ctx.album_knn(t(S, np.float32), off, t(X, np.float32), t(c.album_of, np.int32), A, 5, t(skip, np.int32))
    ctx.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), idx) and np.array_equal(bits(out[1].cpu().numpy()), bits(dist))


# ---- against today's per-album code ----
@pytest.fixture(scope="module")
def library(bliss, tmp_path_factory):
    """300 songs, 40 albums of uneven size, ten songs without an album; disc / track numbers repeat and some are None"""
    rng = np.random.default_rng(77)
    n = 300
    X = rng.standard_normal((n, 23)).astype(np.float32)
    V2 = bliss.FeaturesVersion.Version2
    album = rng.integers(0, 40, n)
    album[:40] = rng.permutation(40)
    songs = [bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist=f"artist{i % 11}",
                        album=None if i % 30 == 17 else f"album {album[i]:02d}", track_number=None if i % 9 == 4 else int(rng.integers(1, 6)),
                        disc_number=None if i % 7 == 3 else int(rng.integers(1, 3)), duration=1.0, analysis=bliss.Analysis(X[i], V2),
                        features_version=V2) for i in range(n)]
    db = str(tmp_path_factory.mktemp("albums") / "bliss.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs)
    return db, songs


@pytest.mark.parametrize("n_albums", (1, 3, 40))
def test_library_album_playlists_against_album_playlist_from(bliss, library, n_albums):
    db, songs = library
    titles = list(dict.fromkeys(s.album for s in songs if s.album is not None))
    assert len(titles) == 40
    table = bliss.library.album_playlists(db, n_albums)
    assert list(table) == titles
    for t in titles:
        want = [s.path for s in bliss.library.album_playlist_from(db, t, n_albums)]
        assert [s.path for s in table[t]] == want, (t, n_albums)
        assert len({s.album for s in table[t]}) == 1 + min(n_albums, 39)


def test_closest_albums_to_groups_against_closest_album_to_group(bliss, library):
    db, songs = library
    P = bliss.playlist
    pool = bliss.library.songs_from_library(db)
    titles = list(dict.fromkeys(s.album for s in songs if s.album is not None))[:12]
    groups = [bliss.library.songs_from_album(db, t) for t in titles]
    got = P.closest_albums_to_groups(groups, pool, 40)
    for t, g, pl in zip(titles, groups, got):
        want = P.closest_album_to_group(g, pool)
        assert [s.path for s in pl] == [s.path for s in want], t
    cut = P.closest_albums_to_groups(groups, pool, 2)
    for g, pl, full in zip(groups, cut, got):
        assert len({s.album for s in pl[len(g):]}) == 2 and [s.path for s in pl] == [s.path for s in full[:len(pl)]]


# ---- the host form's staging: every optional argument given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("skip,dist,means,cents", ((True, True, True, True), (False, False, False, False), (True, True, False, False),
                                                   (False, False, True, True), (True, False, True, False), (False, True, False, True)))
def test_host_form_stages_like_the_device_form(bliss, ctx, skip, dist, means, cents):
    import staging_cases as sc

    def build(c, dev):
        idx, dd = dev(sc.out((c.G, c.k), np.uint32)), dev(sc.out((c.G, c.k), np.float32, dist))
        gm, ce = dev(sc.out((c.G, sc.D), np.float32, means)), dev(sc.out((c.n_albums, sc.D), np.float32, cents))
        return [dev(c.S), c.off, c.G, dev(c.X), c.n, sc.D, dev(c.album_of), c.n_albums, dev(c.skip if skip else None), c.k, idx, dd, gm,
                ce], [idx, dd, gm, ce]

    sc.check(bliss, ctx, "album_knn", build)
