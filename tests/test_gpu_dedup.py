"""GPU tests (-m gpu) of playlist deduplication on the device (blissgpu_dedup_playlist / _device: dedup_next_kernel +
dedup_walk_kernel) against dedup_playlist_custom_distance of the reference (src/playlist.rs:367-402) as the CPU oracle
restates it (bo_dedup_playlist).  Kept positions are discrete: the bar is exact equality, ties and distances exactly at
the threshold included."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "playlist_cases.json")))
D = 23


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


def device_dedup(ctx, X, seq=None, meta=None, metric="euclidean", M=None, threshold=None):
    """blissgpu_dedup_playlist_device through Context.dedup_playlist -> kept positions (numpy int64)"""
    import torch

    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()  # noqa: E731
    kept, n_kept = ctx.dedup_playlist(t(X, np.float32), t(seq, np.int32), t(meta, np.int32), metric, t(M, np.float32),
                                      threshold)
    ctx.synchronize()
    return kept[:int(n_kept.item())].cpu().numpy().astype(np.int64)


def both(bliss, ctx, X, seq=None, meta=None, metric="euclidean", M=None, threshold=None):
    host = bliss.playlist.dedup_order(X, seq, meta, metric, M, threshold)
    dev = device_dedup(ctx, X, seq, meta, metric, M, threshold)
    assert np.array_equal(host, dev)
    return host


# ---- (a) the reference's dedup cases (src/playlist.rs:506-731) through both entry points ----
@pytest.mark.parametrize("k", range(len(CASES["dedup"])))
def test_reference_cases_both_entry_points(bliss, ctx, k):
    c = CASES["dedup"][k]
    S = CASES["songs"]
    pl = c["playlist"]
    X = np.array([S[n]["analysis"] for n in pl], np.float32)
    songs = [bliss.Song(path=n, title=S[n].get("title"), artist=S[n].get("artist")) for n in pl]
    meta = bliss.playlist.meta_keys(songs)
    got = both(bliss, ctx, X, None, meta, c["metric"], None, c["threshold"])
    assert [pl[i] for i in got] == c["expected"]


# ---- (b) 10^5 songs with planted duplicate runs, thresholds 0.05 and 0.3, four metrics ----
def _metrics(oracle):
    rng = np.random.default_rng(7)
    A = rng.standard_normal((D, D)) * 0.3
    spd = (A @ A.T + 0.1 * np.eye(D)).astype(np.float32)
    return {"euclidean": None, "cosine": None, "weights": oracle.feature_weights(2), "spd": spd}


def _planted(oracle, metric, M, thr, seed, n=100_000):
    """Runs of 1 ... 200 songs right after a head song, each jittered so that its distance to the head lies below, at
    (up to f32 rounding) or above the threshold; a few members are then moved EXACTLY onto the threshold."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)).astype(np.float32)
    factors = np.array([0.5, 0.9, 0.999, 0.99999, 1.00001, 1.001, 1.1, 2.0])
    probs = np.array([0.4, 0.2, 0.1, 0.1, 0.1, 0.05, 0.03, 0.02])
    special = [1, 2, 63, 64, 65, 66, 127, 128, 129, 130, 200]

    def jitter(head, L):
        f = rng.choice(factors, size=L, p=probs)
        u = rng.standard_normal((L, D))
        if metric == "cosine":
            h = head.astype(np.float64)
            u -= np.outer(u @ h / (h @ h), h)
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            return u * (np.linalg.norm(h) * np.sqrt(2.0 * thr * f))[:, None]
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        if M is not None:
            u /= np.sqrt(np.einsum("ij,jk,ik->i", u, M.astype(np.float64), u))[:, None]
        return u * (thr * f)[:, None]

    heads, i = [], 0
    while i < n - 202:
        if rng.random() < 0.02:
            L = int(rng.choice(special)) if rng.random() < 0.3 else int(rng.integers(1, 201))
            X[i + 1:i + 1 + L] = (X[i].astype(np.float64) + jitter(X[i], L)).astype(np.float32)
            heads.append(i)
            i += L + 1
        else:
            i += 1
    name = "mahalanobis" if M is not None else metric
    dist = lambda a, b: np.float32(oracle.set_distance(a, b, name, M))  # noqa: E731
    exact = 0
    for h in heads[:24]:
        e = X[h + 1].astype(np.float64) - X[h]
        lo, hi = 0.5, 2.0
        if not (dist(X[h], (X[h] + e * lo).astype(np.float32)) < thr <= dist(X[h], (X[h] + e * hi).astype(np.float32))):
            continue
        for _ in range(60):  # bisection on the scale of the jitter: a member just at or above the threshold
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if dist(X[h], (X[h] + e * mid).astype(np.float32)) < thr else (lo, mid)
        # then one ulp at a time towards the head along the feature the distance depends on least (a step moves the
        # distance by less than one of its own ulps), until it lands on the threshold or passes it
        r = (X[h] + e * hi).astype(np.float32)
        k = int(np.argmin(np.abs(e) + (e == 0)))
        for _ in range(5000):
            dm = dist(X[h], r)
            if dm == np.float32(thr):
                X[h + 1] = r
                exact += 1
                break
            if dm < thr:
                break
            r[k] = np.nextafter(r[k], X[h, k])
    return X, exact


@pytest.mark.parametrize("thr", [0.05, 0.3])
@pytest.mark.parametrize("which", ["euclidean", "cosine", "weights", "spd"])
def test_planted_runs_match_oracle(bliss, oracle, which, thr):
    M = _metrics(oracle)[which]
    metric = "mahalanobis" if M is not None else which
    seed = 100 * ["euclidean", "cosine", "weights", "spd"].index(which) + int(thr * 100)
    X, exact = _planted(oracle, which, M, np.float32(thr), seed)
    # 1 - q never equals 0.05f for an f32 q (0.95 - 7.5e-10 is not one): cosine cannot land on that threshold
    if not (which == "cosine" and thr == 0.05):
        assert exact >= 3, "no song lies exactly on the threshold: the boundary is not exercised"
    want = oracle.dedup_playlist(X, np.float32(thr), metric, M)
    got = bliss.playlist.dedup_order(X, None, None, metric, M, np.float32(thr))
    assert 0.1 * len(X) < len(want) < 0.95 * len(X)  # duplicates were removed, and not everything
    assert np.array_equal(got, want.astype(np.int64))


# ---- (b2) the other feature counts (the second packed width, the generic kernels) past one block of 256 positions ----
@pytest.mark.parametrize("d", [20, 5])
def test_other_feature_counts_match_oracle(bliss, ctx, oracle, d):
    rng = np.random.default_rng(40 + d)
    n, thr = 300, np.float32(0.3)
    X = rng.standard_normal((n, d)).astype(np.float32)
    for head, L in ((10, 5), (100, 40), (250, 12)):  # runs of near-copies behind a head song, the last across position 256
        X[head + 1:head + 1 + L] = X[head] + (0.01 * rng.standard_normal((L, d))).astype(np.float32)
    diag = np.diag(rng.uniform(0.5, 2.0, d)).astype(np.float32)
    for metric, M in (("euclidean", None), ("cosine", None), ("mahalanobis", diag)):
        want = oracle.dedup_playlist(X, thr, metric, M)
        assert 0.5 * n < len(want) <= n - 57  # the planted copies went, and not everything
        assert np.array_equal(both(bliss, ctx, X, None, None, metric, M, thr), want.astype(np.int64)), (d, metric)


# ---- (c) planted title / artist runs: the oracle's n x n same_meta matrix ----
def test_title_artist_runs_match_oracle(bliss, ctx, oracle):
    rng = np.random.default_rng(11)
    n = 2000
    X = rng.standard_normal((n, D)).astype(np.float32)
    keys = np.zeros(n, np.uint32)
    i = 0
    while i < n:
        L = int(rng.integers(1, 90))
        if rng.random() < 0.6:
            keys[i:i + L] = rng.integers(1, 40)  # few distinct keys: the same (title, artist) recurs after a break too
        if rng.random() < 0.1:
            X[i + 1:i + L] = X[i] + np.float32(0.001)  # close AND with metadata
        i += L
    keys[rng.random(n) < 0.05] = 0  # a None title or artist inside a run breaks it
    same = (keys[:, None] == keys[None, :]) & (keys[:, None] != 0)
    for metric in ("euclidean", "cosine"):
        want = oracle.dedup_playlist(X, np.float32(0.05), metric, None, same_meta=same)
        got = both(bliss, ctx, X, None, keys, metric)
        assert len(want) < 0.7 * n
        assert np.array_equal(got, want.astype(np.int64))


# ---- (d) a permuted seq equals deduplicating the gathered matrix ----
def test_permuted_seq_equals_gathered(bliss, ctx, oracle):
    rng = np.random.default_rng(5)
    X, _ = _planted(oracle, "euclidean", None, np.float32(0.05), seed=3, n=20_000)
    keys = rng.integers(0, 30, X.shape[0]).astype(np.uint32)
    perm = rng.permutation(X.shape[0])
    for meta in (None, keys):
        got = both(bliss, ctx, X, perm, meta)
        gathered = bliss.playlist.dedup_order(X[perm], None, None if meta is None else meta[perm])
        assert np.array_equal(got, gathered)
    # a longer playlist than the matrix (songs repeat) and a shorter one
    seq = np.concatenate([perm, perm[:500]])
    assert np.array_equal(both(bliss, ctx, X, seq), bliss.playlist.dedup_order(X[seq]))
    assert np.array_equal(both(bliss, ctx, X, perm[:777]), bliss.playlist.dedup_order(X[perm[:777]]))
    with pytest.raises(bliss.BlissGpuError):
        bliss.playlist.dedup_order(X, np.array([0, X.shape[0]], np.uint32))  # entries must be < n
    with pytest.raises(bliss.BlissGpuError):
        device_dedup(ctx, X, np.array([0, 1, X.shape[0] + 5], np.int32))
    assert both(bliss, ctx, X, np.zeros(0, np.uint32)).tolist() == []
    assert both(bliss, ctx, X, np.array([9], np.uint32)).tolist() == [0]


# ---- (e) NaN: only a distance the reference evaluates is its panic ----
def test_nan_off_the_chain_is_not_an_error(bliss, ctx, oracle):
    """[c, p, q]: p has c's title and artist, d(c, p) and d(c, q) are finite, d(p, q) is NaN -- but the reference never
    evaluates it (p is absorbed through its metadata, the walk goes on from c).  Cosine, with p and q so large that
    their dot products overflow: d(c, .) = 1 - finite / inf = 1, d(p, q) = 1 - inf / inf.  (Under the reference's
    euclidean distance, (a - b).dot(eye).dot(a - b), an infinite feature makes every distance of its song NaN.)"""
    X = np.zeros((3, D), np.float32)
    X[0, :] = 0.25
    X[1, 4] = X[2, 4] = np.float32(3e38)
    songs = [bliss.Song(path="c", title="T", artist="A"), bliss.Song(path="p", title="T", artist="A"),
             bliss.Song(path="q", title="U", artist="A")]
    meta = bliss.playlist.meta_keys(songs)
    assert oracle.cosine_distance(X[0], X[1]) == 1.0 and np.isnan(oracle.cosine_distance(X[1], X[2]))
    assert both(bliss, ctx, X, None, meta, "cosine").tolist() == [0, 2]
    same = np.array([[m1 != 0 and m1 == m2 for m2 in meta] for m1 in meta])
    assert oracle.dedup_playlist(X, np.float32(0.05), "cosine", None, same_meta=same).tolist() == [0, 2]
    # the same playlist as songs; without the metadata p is kept and d(p, q) is evaluated: the reference's panic
    for s, x in zip(songs, X):
        s.analysis = bliss.Analysis(x, bliss.FeaturesVersion.LATEST)
    P = bliss.playlist
    assert [s.path for s in P.dedup_playlist_custom_distance(songs, None, P.cosine_distance)] == ["c", "q"]
    with pytest.raises(ValueError, match="NaN"):
        both(bliss, ctx, X, None, None, "cosine")


def test_nan_on_the_chain_raises_where_the_oracle_does(bliss, ctx, oracle):
    rng = np.random.default_rng(4)
    X = rng.standard_normal((1000, D)).astype(np.float32)
    X[500] = 0.0  # cosine distance to the zero vector is NaN
    with pytest.raises(ValueError):
        oracle.dedup_playlist(X, np.float32(0.05), "cosine")
    with pytest.raises(ValueError, match="NaN"):
        bliss.playlist.dedup_order(X, metric="cosine")
    with pytest.raises(bliss.BlissGpuError) as e:
        device_dedup(ctx, X, metric="cosine")
    assert e.value.code == 5  # BLISSGPU_ERR_NAN
    # the prefix before the zero row is fine for both, and identical
    want = oracle.dedup_playlist(X[:500], np.float32(0.05), "cosine")
    assert np.array_equal(both(bliss, ctx, X[:500], None, None, "cosine"), want.astype(np.int64))
    # a zero row inside a window of duplicates of its head is evaluated too (a run of 200, zero at 150): the reference panics
    Y = np.repeat(X[:1], 300, axis=0)
    Y[150] = 0.0
    with pytest.raises(ValueError):
        oracle.dedup_playlist(Y, np.float32(0.05), "cosine")
    with pytest.raises(ValueError, match="NaN"):
        bliss.playlist.dedup_order(Y, metric="cosine")
    # the distance comes before the title / artist rule: a zero row with the head's metadata still panics
    with pytest.raises(ValueError, match="NaN"):
        bliss.playlist.dedup_order(np.stack([X[0], np.zeros(D, np.float32)]), None, np.array([1, 1], np.uint32), "cosine")


# ---- (f) a playlist of 10^5 identical songs keeps the first ----
def test_all_duplicates(bliss, ctx):
    X = np.repeat(np.arange(D, dtype=np.float32)[None, :], 100_000, axis=0)
    assert both(bliss, ctx, X).tolist() == [0]
    assert both(bliss, ctx, X, None, None, "cosine").tolist() == [0]
    # the same with a break every 1000 songs: the workgroup's scan resumes from far OPEN nodes
    X[::1000, 0] += 1.0
    assert both(bliss, ctx, X).tolist() == sorted(set(range(0, 100_000, 1000)) | set(range(1, 100_000, 1000)))


# ---- (g) structure: two launches per call whatever the length, one library call per playlist ----
def test_two_launches_per_call_and_no_per_song_loop(bliss, monkeypatch):
    from bliss_rs_amd import _ffi

    P = bliss.playlist
    ctx = bliss.Context.default(0)  # the context of the host-pointer entry points
    rng = np.random.default_rng(9)
    ctx.profile_enable(True)
    try:
        for n in (10, 20_000, 100_000):
            ctx.profile_reset()
            P.dedup_order(rng.standard_normal((n, D)).astype(np.float32))
            prof = ctx.profile()
            assert prof["dedup_next_kernel"][1] == 1 and prof["dedup_walk_kernel"][1] == 1, prof
            assert "set_distance_kernel" not in prof
    finally:
        ctx.profile_enable(False)
    L = _ffi.lib()
    calls = {"blissgpu_dedup_playlist": 0, "blissgpu_set_distance": 0}
    for name in calls:
        fn = getattr(L, name)

        def counted(*a, _fn=fn, _name=name):
            calls[_name] += 1
            return _fn(*a)

        monkeypatch.setattr(L, name, counted)
    X = rng.standard_normal((20_000, D)).astype(np.float32)
    X[1::2] = X[::2] + np.float32(0.001)  # every other song a duplicate
    songs = [bliss.Song(path=str(i), analysis=bliss.Analysis(x, bliss.FeaturesVersion.LATEST)) for i, x in enumerate(X)]
    got = P.dedup_playlist_custom_distance(songs, None, P.euclidean_distance, window=64)
    assert calls == {"blissgpu_dedup_playlist": 1, "blissgpu_set_distance": 0}
    assert [s.path for s in got] == [str(i) for i in range(0, 20_000, 2)]


# ---- the host form's staging: every optional argument given and NULL, then a call of another size (tests/staging_cases.py) ----
@pytest.mark.parametrize("seq,meta", ((True, True), (False, False), (True, False), (False, True)))
def test_host_form_stages_like_the_device_form(bliss, ctx, seq, meta):
    import staging_cases as sc

    def build(c, dev):
        order = np.arange(c.n, dtype=np.uint32)[::-1].copy() if seq else None  # (seq == NULL: the rows in their own order, len == n)
        kept, n_kept = dev(sc.out((c.n,), np.uint32)), dev(np.full(1, 0x5A5A, np.uint64))
        return [dev(c.X), c.n, sc.D, dev(order), c.n, dev((np.arange(c.n) % 9).astype(np.uint32) if meta else None), 2, dev(c.M), 1.5, kept,
                n_kept], [kept, n_kept]

    sc.check(bliss, ctx, "dedup_playlist", build, lists=False)
