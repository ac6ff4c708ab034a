"""GPU parity tests (-m gpu) for the playlist-ordering row: the HIP kernels, called through the C ABI
(blissgpu_set_distance / _closest_to_songs / _song_to_song), against the reference's own ordering tests
(tests/golden/playlist_cases.json) and against the CPU oracle on seeded random libraries.  Everything here is
discrete (index permutations) or a bit-exact f32 distance: the bar is exact equality, ties included."""
import json
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "playlist_cases.json")))


@pytest.fixture(scope="module")
def bliss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import bliss_rs_amd

    return bliss_rs_amd


@pytest.fixture(scope="module")
def songs(bliss):
    out = {}
    for name, s in CASES["songs"].items():
        out[name] = bliss.Song(path=f"path-to-{name}", analysis=bliss.Analysis(s["analysis"], bliss.FeaturesVersion.LATEST),
                               title=s.get("title"), artist=s.get("artist"))
    return out


class CustomSong:  # the reference's tests repeat every case with a wrapper that is AsRef<Song>
    def __init__(self, bliss_song):
        self.bliss_song = bliss_song
        self.something = True


@pytest.mark.parametrize("wrap", [False, True])
def test_reference_ordering_cases(bliss, songs, wrap):  # src/playlist.rs:506-1007
    S = {k: (CustomSong(v) if wrap else v) for k, v in songs.items()}
    P = bliss.playlist
    fn = {"euclidean": P.euclidean_distance, "cosine": P.cosine_distance}
    for c in CASES["closest_to_songs"]:
        got = P.closest_to_songs([S[n] for n in c["initial"]], [S[n] for n in c["candidates"]], fn[c["metric"]])
        assert [id(x) for x in got] == [id(S[n]) for n in c["expected"]]
    for c in CASES["song_to_song"]:
        got = P.song_to_song([S[n] for n in c["initial"]], [S[n] for n in c["candidates"]], fn[c["metric"]])
        assert [id(x) for x in got] == [id(S[n]) for n in c["expected"]]
    for c in CASES["dedup"]:
        got = P.dedup_playlist_custom_distance([S[n] for n in c["playlist"]], c["threshold"], fn[c["metric"]])
        assert [id(x) for x in got] == [id(S[n]) for n in c["expected"]]
        if c["metric"] == "euclidean":
            got = P.dedup_playlist([S[n] for n in c["playlist"]], c["threshold"])
            assert [id(x) for x in got] == [id(S[n]) for n in c["expected"]]


def test_closest_album_to_group_reference_case(bliss):  # src/playlist.rs:1112-1260
    for version in (bliss.FeaturesVersion.Version1, bliss.FeaturesVersion.Version2):
        d = 20 if version == bliss.FeaturesVersion.Version1 else 23

        def song(path, album, artist, track, disc, value):
            return bliss.Song(path=path, album=album, artist=artist, track_number=track, disc_number=disc,
                              analysis=bliss.Analysis([value] * d, version), features_version=version)

        first = song("path-to-first", "Album", "Artist", 1, 1, 0.0)
        second = song("path-to-third", "Album", "Another Artist", 2, 1, 10.0)
        a1 = song("path-to-second-2", "Another Album", "Artist", 1, 1, 0.15)
        a2 = song("path-to-second", "Another Album", "Artist", 2, 1, 0.1)
        b1 = song("path-to-fourth", "Another Album", "Another Artist", 1, 2, 20.0)
        b2 = song("path-to-fourth", "Another Album", "Another Artist", 4, 2, 20.0)
        no_album = song("path-to-fifth", None, "Third Artist", None, None, 40.0)
        pool = [first, a2, b2, second, b1, a1, no_album]
        got = bliss.playlist.closest_album_to_group([first, second], pool)
        assert [id(x) for x in got] == [id(x) for x in (first, second, a1, a2, b1, b2)]


@pytest.mark.parametrize("d", [23, 20, 7])
def test_ordering_bit_exact_vs_oracle(bliss, oracle, d):
    rng = np.random.default_rng(100 + d)
    n = 5000
    X = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    X[1234] = X[17]  # exact duplicates: ties must resolve like the reference (first in pool order / stable)
    X[4000] = X[17]
    X[4001] = X[3999]
    A = rng.standard_normal((d, d)).astype(np.float32)
    M_full = (A @ A.T / d + np.eye(d, dtype=np.float32)).astype(np.float32)  # PSD, non-diagonal
    M_diag = oracle.feature_weights(2) if d == 23 else np.diag(rng.uniform(0.1, 2, d)).astype(np.float32)
    P = bliss.playlist
    for n_seeds in (1, 3):
        seeds = X[rng.integers(0, n, n_seeds)].copy()
        for metric, m in (("euclidean", None), ("cosine", None), ("mahalanobis", M_diag), ("mahalanobis", M_full)):
            ref_order, ref_dist = oracle.closest_to_songs(seeds, X, metric, m)
            got_dist = P.set_distances(seeds, X, metric, m)
            assert np.array_equal(got_dist.view(np.uint32), ref_dist.view(np.uint32)), (metric, n_seeds)
            got_order, got_dist2 = P.closest_to_songs_order(seeds, X, metric, m)
            assert np.array_equal(got_dist2.view(np.uint32), ref_dist.view(np.uint32))
            assert np.array_equal(got_order, ref_order), (metric, n_seeds)
    # the greedy chain is O(n^2) on the CPU oracle: a 1500-song pool (with the duplicates) keeps it in seconds
    sub = np.concatenate([X[:1495], X[[17, 17, 3999, 4001, 1234]]])
    for metric, m in (("euclidean", None), ("cosine", None), ("mahalanobis", M_full)):
        for seeds in (sub[[5]], sub[[5, 700, 1400]]):
            ref = oracle.song_to_song(seeds, sub, metric, m)
            got = P.song_to_song_order(seeds, sub, metric, m)
            assert np.array_equal(got, ref), metric


def test_small_pools_and_edge_cases(bliss, oracle):
    P = bliss.playlist
    rng = np.random.default_rng(3)
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 513):
        X = rng.uniform(-1, 1, (n, 23)).astype(np.float32)
        seeds = rng.uniform(-1, 1, (2, 23)).astype(np.float32)
        assert np.array_equal(P.song_to_song_order(seeds, X), oracle.song_to_song(seeds, X))
        assert np.array_equal(P.closest_to_songs_order(seeds, X)[0], oracle.closest_to_songs(seeds, X)[0])
    assert P.closest_to_songs([], []) == [] and P.song_to_song([], []) == []
    # NaN distances: n32() / argmin().unwrap() panic in the reference -> ValueError here, never a silent order
    X = rng.uniform(-1, 1, (300, 23)).astype(np.float32)
    X[100] = 0.0  # cosine distance to the zero vector is NaN (no zero-norm guard, src/playlist.rs:76-79)
    with pytest.raises(ValueError, match="NaN"):
        P.closest_to_songs_order(X[:1], X, "cosine")
    with pytest.raises(ValueError, match="NaN"):
        P.song_to_song_order(X[:1], X, "cosine")
    assert np.isnan(P.set_distances(X[:1], X, "cosine")[100])  # DistanceMetric::distance itself just returns NaN


def test_device_resident_forms_and_full_library_size(bliss, oracle):
    """100 000-vector library (BASELINE configs[3] size) resident in HBM: order properties + oracle spot checks."""
    import torch

    ctx = bliss.Context(0)
    n, d = 100000, 23
    g = torch.Generator(device="cuda").manual_seed(77)
    X = torch.rand((n, d), generator=g, device="cuda", dtype=torch.float32) * 2 - 1
    X[500] = X[40]
    seeds = X[[40, 9000]].clone()
    M = torch.from_numpy(oracle.feature_weights(2)).cuda()
    order, dist = ctx.closest_to_songs(seeds, X, "mahalanobis", M, return_distances=True)
    order_h, dist_h, X_h = order.cpu().numpy(), dist.cpu().numpy(), X.cpu().numpy()
    assert sorted(order_h.tolist()) == list(range(n))
    assert np.array_equal(order_h, np.argsort(dist_h, kind="stable"))
    idx = np.random.default_rng(0).integers(0, n, 2000)
    ref = np.array([oracle.set_distance(seeds.cpu().numpy(), X_h[i], "mahalanobis", oracle.feature_weights(2)) for i in idx],
                   np.float32)
    assert np.array_equal(dist_h[idx].view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(ctx.set_distance(seeds, X, "mahalanobis", M).cpu().numpy().view(np.uint32), dist_h.view(np.uint32))

    t0 = time.perf_counter()
    chain = ctx.song_to_song(seeds[:1], X, "euclidean").cpu().numpy()
    dt = time.perf_counter() - t0
    print(f"song_to_song over {n} songs: {dt:.3f} s ({n / dt:.0f} steps/s)")
    assert sorted(chain.tolist()) == list(range(n))
    # the chain rule itself, verified independently on the first 200 links with the oracle's distance
    alive = np.ones(n, bool)
    cur = seeds[:1].cpu().numpy()
    for k in range(200):
        dk = oracle.pairwise(cur, X_h, "euclidean")[0]
        dk[~alive] = np.inf
        assert chain[k] == int(np.argmin(dk)), k  # np.argmin = first minimum
        alive[chain[k]] = False
        cur = X_h[chain[k]][None, :]


def test_library_drives_the_ordering_kernels(bliss, oracle, tmp_path):
    """an existing feature table feeds the device matrix directly -- no re-analysis -- and the order is
    the one the Song-object API produces."""
    import torch

    rng = np.random.default_rng(8)
    db = str(tmp_path / "lib.db")
    bliss.library.create_schema(db)
    songs = [bliss.Song(path=f"/m/{i:04d}.flac", title=f"t{i}", artist=f"a{i % 7}",
                        analysis=bliss.Analysis(rng.uniform(-1, 1, 23).astype(np.float32), bliss.FeaturesVersion.LATEST))
             for i in range(400)]
    bliss.library.store_songs(db, songs)
    ids, paths, m = bliss.library.load_feature_matrix(db)
    ctx = bliss.Context(0)
    X = torch.from_numpy(m).cuda()
    W = torch.from_numpy(oracle.feature_weights(2)).cuda()
    order = ctx.closest_to_songs(X[:2], X, "mahalanobis", W).cpu().numpy()
    via_songs = bliss.playlist.closest_to_songs(songs[:2], songs, bliss.playlist.MahalanobisBuilder(oracle.feature_weights(2)))
    assert [paths[i] for i in order] == [s.path for s in via_songs]
    chain = ctx.song_to_song(X[:1], X, "euclidean").cpu().numpy()
    assert np.array_equal(chain, oracle.song_to_song(m[:1], m, "euclidean"))


# ---- the host forms' staging: every optional argument given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("family,dist", (("set_distance", False), ("closest_to_songs", True), ("closest_to_songs", False),
                                         ("song_to_song", False)))
def test_host_form_stages_like_the_device_form(bliss, family, dist):
    import staging_cases as sc

    def build(c, dev):
        head = [dev(c.S), len(c.S), dev(c.X), c.n, sc.D, 2, dev(c.M)]
        if family == "set_distance":
            outs = [dev(sc.out((c.n,), np.float32))]
        elif family == "song_to_song":
            outs = [dev(sc.out((c.n,), np.uint32))]
        else:
            outs = [dev(sc.out((c.n,), np.uint32)), dev(sc.out((c.n,), np.float32, dist))]
        return head + outs, outs

    ctx = bliss.Context(0)
    try:
        sc.check(bliss, ctx, family, build, lists=family != "set_distance")
    finally:
        ctx.close()
