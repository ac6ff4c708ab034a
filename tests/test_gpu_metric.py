"""GPU tests (-m gpu) of triplet metric learning on the device (blissgpu_triplet_step / blissgpu_learn_metric:
triplet_step_kernel, triplet_reduce_kernel, metric_learn.hpp).  Expected values never come from the code under test.

The step is checked against the contract of include/blissgpu.h restated in numpy float64 (ref_step: every product and every sum
of the hinges rounded on its own, ascending from 0.0 -- flags and n_active must be EQUAL), and its two sums against a reference
that has no error of its own to speak of: loss against math.fsum of the restated hinges, G against the EXACT sum of its terms
(the differences of mixed_grid rows are integers in units of 2^-36; exact_gram adds their products in integers).  The bound is derived, not
measured: loss and every G[r][c] are sums of at most 3T products, each rounded once, added in some order, so they lie within
(3T + 2) 2^-52 S of the exact sum, S the sum of the absolute values of the terms.
The loop is replayed by tests/test_metric_host.py's restatement on the device's own steps, bit for bit.
Data: 500 rows of test_gpu_albums.mixed_grid, whose two magnitudes (1e4 and 1e-3) make every rounding show."""
import math
import sqlite3
import warnings

import numpy as np
import pytest

from test_gpu_albums import mixed_grid
from test_metric_host import CONVERGED, DIAGONAL, DIVERGED, FULL, MAX_ITER, NAN_CODE, f32_bits, f64_bits, ref_learn

pytestmark = pytest.mark.gpu

N = 500
TS = (1, 63, 64, 65, 1000, 70001)
DS = (23, 20, 5, 33, 64)
MARGIN = 3.0e7  # between the hinges' two magnitudes: about half of them are active


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


def matrix(kind, d):
    if kind == "null":
        return None
    if kind == "diagonal":
        return np.diag(np.linspace(0.5, 2.0, d)).astype(np.float32)
    rng = np.random.default_rng(7)
    A = rng.standard_normal((d, d)) * 0.3
    return (A @ A.T + 0.1 * np.eye(d)).astype(np.float32)


def ref_step(X, tr, M, margin):
    """the contract: -> (flags uint8[T], h1, h2 float64[T], u, v, w float64[T, d]).  The triplets side by side, the sums in
    Python loops over r and c."""
    Xd = X.astype(np.float64)
    T, d = tr.shape[0], X.shape[1]
    Md = np.eye(d) if M is None else M.astype(np.float64)
    diffs = [Xd[tr[:, 0]] - Xd[tr[:, 1]], Xd[tr[:, 0]] - Xd[tr[:, 2]], Xd[tr[:, 1]] - Xd[tr[:, 2]]]
    qs = []
    with np.errstate(all="ignore"):
        for t in diffs:
            tc = np.ascontiguousarray(t.T)  # tc[c] = column c of every triplet
            q = np.zeros(T)
            for r in range(d):
                s = np.zeros(T)
                for c in range(d):
                    s = s + Md[r, c] * tc[c]
                q = q + tc[r] * s
            qs.append(q)
        base = np.float64(margin) + qs[0]
        h1, h2 = base - qs[1], base - qs[2]
    flags = (h1 > 0).astype(np.uint8) | ((h2 > 0).astype(np.uint8) << 1)
    return flags, h1, h2, diffs


SCALE = 36  # every mixed_grid value is a multiple of 2^-36 below 2^14 (asserted): differences are integers D 2^-36, |D| < 2^51
LIMB = 17


def exact_gram(D, coef):
    """sum_t coef[t] D[t] D[t]' as Python integers, object[d, d].  D int64 [T, d] is split into three 17-bit limbs; a product of
    limbs is below 2^34 and a sum of T < 2^17 of them times |coef| <= 2 below 2^53, so every float64 matrix product is exact
    whatever order it adds in."""
    assert D.shape[0] < 2 ** LIMB and np.abs(coef).max(initial=0) <= 2 and np.abs(D).max(initial=0) < 2 ** 51
    mask = (1 << LIMB) - 1
    limbs = [(D & mask).astype(np.float64), ((D >> LIMB) & mask).astype(np.float64), (D >> (2 * LIMB)).astype(np.float64)]
    out = np.zeros((D.shape[1], D.shape[1]), object)
    for i in range(3):
        left = (limbs[i] * coef[:, None].astype(np.float64)).T
        for j in range(3):
            out = out + (left @ limbs[j]).astype(np.int64).astype(object) * (1 << (LIMB * (i + j)))
    return out


def ref_sums(flags, h1, h2, diffs):
    """-> (n_active, loss, S_loss, G, S_G): loss by math.fsum; G and the sum of its terms' absolute values EXACTLY, as Python
    integers in units of 2^-72"""
    f1, f2 = (flags & 1).astype(bool), (flags & 2).astype(bool)
    terms = np.concatenate([h1[f1], h2[f2]])
    loss, s_loss = math.fsum(terms), math.fsum(np.abs(terms))
    ints = []
    for t in diffs:
        scaled = t * 2.0 ** SCALE
        assert (scaled == np.rint(scaled)).all()
        ints.append(scaled.astype(np.int64))
    u, v, w = ints
    c0, c1, c2 = f1.astype(np.int64) + f2.astype(np.int64), f1.astype(np.int64), f2.astype(np.int64)
    G = exact_gram(u, c0) - exact_gram(v, c1) - exact_gram(w, c2)
    S = exact_gram(np.abs(u), c0) + exact_gram(np.abs(v), c1) + exact_gram(np.abs(w), c2)
    return int(f1.sum()) + int(f2.sum()), loss, s_loss, G, S


def host_form(bliss, X, tr, M, margin):
    na, loss, G, flags = bliss.playlist.triplet_step(X, tr, M, margin, return_flags=True)
    return na, loss, G, flags


def device_form(ctx, X, tr, M, margin):
    import torch

    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    na, loss, G, flags = ctx.triplet_step(t(X), torch.from_numpy(tr.astype(np.int32)).cuda(), t(M), margin, return_flags=True)
    return na, loss, G, flags.cpu().numpy()


def check_step(got, ref, sums, T, what):
    from fractions import Fraction

    na, loss, G, flags = got
    r_flags = ref[0]
    r_na, r_loss, s_loss, r_G, S = sums
    assert np.array_equal(flags, r_flags), (what, "flags", int((flags != r_flags).sum()), "differ")
    assert na == r_na, (what, "n_active", na, r_na)
    assert np.isfinite(G).all() and math.isfinite(loss)
    eps = Fraction(3 * T + 2, 2 ** 52)
    unit = 2 ** (2 * SCALE)
    err_loss = abs(Fraction(loss) - Fraction(r_loss))  # (fsum is the correctly rounded sum: within 2^-53 of it)
    worst = Fraction(0)
    for g, r, a in zip(G.reshape(-1).tolist(), r_G.reshape(-1).tolist(), S.reshape(-1).tolist()):
        err = abs(Fraction(g) * unit - r)
        if a:
            worst = max(worst, err / (eps * a))
        assert err <= eps * a, (what, "G", g, float(Fraction(r, unit)), float(err / unit), float(eps * a / unit))
    print(what, "active", na, "of", 2 * T, "loss err / bound", float(err_loss / (eps * Fraction(s_loss))) if s_loss else 0.0,
          "worst G err / bound", float(worst))
    assert err_loss <= eps * Fraction(s_loss), (what, "loss", loss, r_loss)
    assert np.array_equal(f64_bits(G), f64_bits(G.T)), (what, "G is not exactly symmetric")


@pytest.mark.parametrize("kind", ("null", "diagonal", "full"))
@pytest.mark.parametrize("d", DS)
def test_step_against_the_contract(bliss, ctx, d, kind):
    rng = np.random.default_rng(1000 + d)
    X = mixed_grid(rng, N, d)
    M = matrix(kind, d)
    for T in TS:
        tr = rng.integers(0, N, (T, 3)).astype(np.int64)
        ref = ref_step(X, tr, M, MARGIN)
        sums = ref_sums(*ref)
        if T >= 1000:
            assert 0.2 * 2 * T < sums[0] < 0.8 * 2 * T  # on the reference alone: both outcomes are common
        first = None
        for name, form in (("host form", lambda: host_form(bliss, X, tr, M, MARGIN)), ("device form", lambda: device_form(ctx, X, tr, M, MARGIN))):
            got = form()
            check_step(got, ref, sums, T, (d, kind, T, name))
            again = form()  # a second call: identical bits
            assert got[0] == again[0] and f64_bits(np.float64(got[1])) == f64_bits(np.float64(again[1]))
            assert got[2].tobytes() == again[2].tobytes() and got[3].tobytes() == again[3].tobytes()
            if first is None:
                first = got
            else:  # ... and the two forms agree to the bit
                assert got[2].tobytes() == first[2].tobytes() and got[1] == first[1]


def test_shortcuts_give_the_full_form_bits(bliss, ctx):
    """NULL and an explicit identity matrix take different kernels' paths (identity / detected diagonal) and must agree to the
    bit with each other and, in their flags, with the restatement, which runs the full form for every M"""
    rng = np.random.default_rng(3)
    for d in (23, 5):
        X = mixed_grid(rng, N, d)
        tr = rng.integers(0, N, (4000, 3))
        want = ref_step(X, tr, None, MARGIN)[0]
        for M in (None, np.eye(d, dtype=np.float32)):
            assert np.array_equal(host_form(bliss, X, tr, M, MARGIN)[3], want)
        a = host_form(bliss, X, tr, None, MARGIN)
        b = host_form(bliss, X, tr, np.eye(d, dtype=np.float32), MARGIN)
        assert a[2].tobytes() == b[2].tobytes() and a[1] == b[1]


def test_edges(bliss, ctx):
    from bliss_rs_amd import _ffi

    P = bliss.playlist
    rng = np.random.default_rng(4)
    d = 23
    X = mixed_grid(rng, N, d)
    tr = rng.integers(0, N, (300, 3))
    # M = 0 with margin > 0: every hinge is exactly the margin, all active, and G cancels only where u, v, w say so
    na, loss, G, flags = P.triplet_step(X, tr, np.zeros((d, d), np.float32), 0.5, return_flags=True)
    assert na == 600 and (flags == 3).all() and loss == 300.0
    ref = ref_step(X, tr, np.zeros((d, d), np.float32), 0.5)
    check_step((na, loss, G, flags), ref, ref_sums(*ref), 300, "M = 0")
    # margin = 0 and b == o: v == u, h1 is exactly 0 -- inactive; w == 0 so h2 = q(u) - 0 > 0 unless a == b too
    t2 = tr.copy()
    t2[:, 2] = t2[:, 1]
    t2[:10, 0] = t2[:10, 1]  # a == b == o: both hinges exactly 0
    for M in (None, matrix("diagonal", d), matrix("full", d)):
        na, loss, G, flags = P.triplet_step(X, t2, M, 0.0, return_flags=True)
        assert (flags & 1 == 0).all() and (flags[:10] == 0).all()
        ref = ref_step(X, t2, M, 0.0)
        check_step((na, loss, G, flags), ref, ref_sums(*ref), 300, "b == o")
    # a == b: u = 0, q(u) = 0: h = margin - q(v), v == w
    t3 = tr.copy()
    t3[:, 1] = t3[:, 0]
    na, loss, G, flags = P.triplet_step(X, t3, None, MARGIN, return_flags=True)
    assert ((flags == 0) | (flags == 3)).all()
    ref = ref_step(X, t3, None, MARGIN)
    check_step((na, loss, G, flags), ref, ref_sums(*ref), 300, "a == b")
    # T = 0
    na, loss, G = P.triplet_step(X, np.zeros((0, 3), np.int64), None, 1.0)
    assert (na, loss) == (0, 0.0) and not G.any() and G.shape == (d, d)
    import torch

    na, loss, G = ctx.triplet_step(torch.from_numpy(X).cuda(), torch.zeros((0, 3), dtype=torch.int32).cuda(), None, 1.0)
    assert (na, loss) == (0, 0.0) and not G.any()
    # an index == n, anywhere in the list and in any column: INVALID, found on the device, nothing read outside X
    for pos, col in ((0, 0), (299, 2), (150, 1)):
        bad = tr.copy()
        bad[pos, col] = N
        with pytest.raises(_ffi.BlissGpuError) as e:
            P.triplet_step(X, bad, None, 1.0)
        assert e.value.code == _ffi.ERR_INVALID
    bad = tr.copy()
    bad[7] = 0xFFFFFFFF
    with pytest.raises(_ffi.BlissGpuError) as e:
        ctx.triplet_step(torch.from_numpy(X).cuda(), torch.from_numpy(bad.astype(np.uint32).view(np.int32)).cuda(), None, 1.0)
    assert e.value.code == _ffi.ERR_INVALID
    # a NaN row that a triplet names: ERR_NAN; one that none names: OK
    Xn = X.copy()
    Xn[N - 1, 3] = np.nan
    low = rng.integers(0, N - 1, (300, 3))
    for M in (None, matrix("full", d)):
        ok = P.triplet_step(Xn, low, M, MARGIN)
        assert ok[0] == ref_sums(*ref_step(X, low, M, MARGIN))[0]
        named = low.copy()
        named[123, 2] = N - 1
        with pytest.raises(ValueError):
            P.triplet_step(Xn, named, M, MARGIN)
        with pytest.raises(_ffi.BlissGpuError) as e:
            ctx.triplet_step(torch.from_numpy(Xn).cuda(), torch.from_numpy(named.astype(np.int32)).cuda(),
                             None if M is None else torch.from_numpy(M).cuda(), MARGIN)
        assert e.value.code == _ffi.ERR_NAN
    # an infinite difference under a diagonal M: the full form multiplies it by the zeros off the diagonal -- NaN there too
    Xi = X.copy()
    Xi[N - 1, 3] = np.inf
    with pytest.raises(ValueError):
        P.triplet_step(Xi, named, matrix("diagonal", d), MARGIN)


def replay(bliss, X, tr, form, init, margin, lr, reg, max_iter):
    """the loop of the restatement on the device's own steps"""
    P = bliss.playlist
    from bliss_rs_amd import _ffi

    def step(M):
        try:
            na, loss, G = P.triplet_step(X, tr, M, margin)
        except ValueError:
            return NAN_CODE, 0.0, 0, None
        except _ffi.BlissGpuError as e:
            return e.code, 0.0, 0, None
        return 0, loss, na, G

    return ref_learn(DIAGONAL if form == "diagonal" else FULL, X.shape[1], init, tr.shape[0], lr, reg, max_iter, step)


STATUS = {CONVERGED: "converged", MAX_ITER: "max_iter", DIVERGED: "diverged"}


def assert_same_run(got, want, what):
    print(what, got.status, got.n_iter, got.best_iter, got.objective[:3], got.active[:3])
    assert (got.status, got.n_iter, got.best_iter) == (STATUS[want["status"]], want["n_iter"], want["best_iter"]), what
    assert np.array_equal(f32_bits(got.m), f32_bits(want["M"])), (what, "M bits")
    assert np.array_equal(f64_bits(got.objective), f64_bits(want["obj"])), (what, got.objective, want["obj"])
    assert np.array_equal(got.active, want["active"]), what


def learn_both(bliss, ctx, X, tr, **kw):
    import torch

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        a = bliss.playlist.learn_metric(X, tr, **kw)
        b = ctx.learn_metric(torch.from_numpy(X).cuda(), torch.from_numpy(tr.astype(np.int32)).cuda(), **kw)
    stats = ctx.metric_stats()
    return a, b, stats


@pytest.mark.parametrize("form", ("diagonal", "full"))
def test_loop_replayed_on_the_device_steps(bliss, ctx, form):
    rng = np.random.default_rng(5)
    d = 23
    X = (mixed_grid(rng, N, d) * np.float32(1e-4)).astype(np.float32)  # entries of about 1: lr = 1 moves M without overflow
    tr = rng.integers(0, N, (3000, 3))
    init = (0.5 + rng.random(d)).astype(np.float32)
    for reg in (0.0, 0.01):
        for max_iter in (0, 1, 5):
            for ini in (None, init):
                kw = dict(form=form, init=ini, margin=0.1, lr=0.05, reg=reg, max_iter=max_iter)
                want = replay(bliss, X, tr, **kw)
                a, b, stats = learn_both(bliss, ctx, X, tr, **kw)
                assert_same_run(a, want, (form, reg, max_iter, "host form"))
                assert_same_run(b, want, (form, reg, max_iter, "device form"))
                assert want["status"] == MAX_ITER and want["n_iter"] == max_iter
                # one upload of M and one download of (G, loss, n_active, error word) per iteration
                assert stats == (max_iter + 1, max_iter + 1, (max_iter + 1) * (d * d + 3) * 8), stats
    # a run that converges: a handful of triplets the identity already satisfies by more than the margin
    Xc = np.zeros((6, d), np.float32)
    Xc[1, 0], Xc[2, 1], Xc[3, 2], Xc[4, 0], Xc[5, 1] = 0.1, 5.0, -6.0, 7.0, 0.2
    easy = np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4], [0, 5, 2]])
    kw = dict(form=form, init=None, margin=0.1, lr=1.0, reg=0.01, max_iter=5)
    want = replay(bliss, Xc, easy, **kw)
    a, b, stats = learn_both(bliss, ctx, Xc, easy, **kw)
    assert want["status"] == CONVERGED and want["n_iter"] == 0 and want["obj"][0] == 0.0
    assert_same_run(a, want, (form, "converges at once, host form"))
    assert_same_run(b, want, (form, "converges at once, device form"))
    assert stats[:2] == (1, 1)
    # ... and one that needs a few updates first: one violated triplet among them
    hard = np.concatenate([easy, [[0, 2, 1]]])
    kw = dict(form=form, init=None, margin=0.1, lr=0.01, reg=0.0, max_iter=200)
    want = replay(bliss, Xc, hard, **kw)
    a, b, stats = learn_both(bliss, ctx, Xc, hard, **kw)
    print("contradicting triplets", STATUS[want["status"]], want["n_iter"])
    assert_same_run(a, want, (form, "contradiction, host form"))
    assert_same_run(b, want, (form, "contradiction, device form"))
    # lr chosen to diverge: M leaves float32 within a few updates; the result is the best finite iterate.  (The clamp at 0 keeps
    # the diagonal form bounded for any lr > 0 -- a weight that grows large turns its own gradient positive -- so it gets a
    # negative one: gradient ASCENT.)
    kw = dict(form=form, init=None, margin=0.1, lr=-3e38 if form == "diagonal" else 1e36, reg=0.0, max_iter=30)
    want = replay(bliss, X, tr, **kw)
    assert want["status"] == DIVERGED and 1 <= want["n_iter"] < 30
    with pytest.warns(RuntimeWarning):
        a = bliss.playlist.learn_metric(X, tr, **kw)
    assert_same_run(a, want, (form, "diverges"))
    assert np.isfinite(a.m).all() and not np.isfinite(a.objective[-1]) and a.best_iter < a.n_iter


def test_profile_table_counts_the_steps(ctx):
    import torch

    rng = np.random.default_rng(6)
    X = torch.from_numpy(mixed_grid(rng, N, 23) * np.float32(1e-4)).cuda()
    tr = torch.from_numpy(rng.integers(0, N, (1000, 3)).astype(np.int32)).cuda()
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        res = ctx.learn_metric(X, tr, form="diagonal", margin=0.1, lr=0.05, max_iter=3)
        ctx.synchronize()
        prof = {k: v[1] for k, v in ctx.profile().items()}
        assert res.n_iter == 3 and prof == {"triplet_step_kernel": 4, "triplet_reduce_kernel": 4}, prof
    finally:
        ctx.profile_enable(False)


# ---- end to end: a planted metric is recovered well enough to halve the held-out violations ---------------------------------
def planted(kind, d, rng):
    if kind == "diagonal":
        return np.diag(np.exp(rng.normal(0.0, 1.0, d)))
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    return A @ A.T + 0.05 * np.eye(d)


def labelled_triplets(X, Mp, T, rng):
    """T triplets of three distinct rows, ordered so that (a, b) is the pair closest under the planted metric"""
    n = X.shape[0]
    idx = np.zeros((0, 3), np.int64)
    while idx.shape[0] < T:
        more = rng.integers(0, n, (T, 3))
        idx = np.concatenate([idx, more[(more[:, 0] != more[:, 1]) & (more[:, 0] != more[:, 2]) & (more[:, 1] != more[:, 2])]])
    idx = idx[:T]
    Xd = X.astype(np.float64)

    def q(i, j):
        t = Xd[i] - Xd[j]
        return np.einsum("ti,ij,tj->t", t, Mp, t)

    d01, d02, d12 = q(idx[:, 0], idx[:, 1]), q(idx[:, 0], idx[:, 2]), q(idx[:, 1], idx[:, 2])
    out = idx.copy()
    m02 = (d02 < d01) & (d02 <= d12)
    m12 = (d12 < d01) & (d12 < d02)
    out[m02] = idx[m02][:, [0, 2, 1]]
    out[m12] = idx[m12][:, [1, 2, 0]]
    return out


@pytest.mark.parametrize("kind", ("diagonal", "full"))
def test_planted_metric_end_to_end(bliss, kind):
    """lr = 1, margin = 0.1, 60 iterations, the matching form: held-out violations at most HALF the identity's.  (The numpy
    loop alone reaches at most 0.22 x on three seeds of each form, computed on a CPU -- DESIGN.md 3.22 has the table; 0.5 leaves
    room for a different rounding of G.  A condition, not a measurement.)"""
    P = bliss.playlist
    rng = np.random.default_rng(0)
    n, d = 1000, 23
    X = rng.standard_normal((n, d)).astype(np.float32)
    Mp = planted(kind, d, rng)
    train, held = labelled_triplets(X, Mp, 5000, rng), labelled_triplets(X, Mp, 5000, rng)
    res = P.learn_metric(X, train, form=kind, margin=0.1, lr=1.0, max_iter=60)
    before, after = 1.0 - P.triplet_accuracy(X, held), 1.0 - P.triplet_accuracy(X, held, res.m)
    print(kind, res, "held-out violations", before, "->", after)
    assert 0.05 < before < 0.5  # on the data alone: the identity is wrong often enough to measure
    assert after <= 0.5 * before
    assert P.triplet_accuracy(X, held, Mp.astype(np.float32)) > 0.99  # the planted metric itself (f32) satisfies its own labels
    if kind == "diagonal":
        assert np.count_nonzero(res.m - np.diag(np.diag(res.m))) == 0 and (np.diag(res.m) >= 0).all()
    else:
        assert np.array_equal(res.m, res.m.T) and np.linalg.eigvalsh(res.m.astype(np.float64)).min() > -1e-5 * np.abs(res.m).max()


def test_library_learn_metric_from_genres(bliss):
    lib = bliss.library
    V2 = bliss.FeaturesVersion.Version2
    rng = np.random.default_rng(8)
    d, n = 23, 240
    centres = rng.standard_normal((4, d)).astype(np.float32)
    centres[:, 8:] = 0.0  # the genres differ in the first eight features; the rest is noise three times as wide
    genre = rng.integers(0, 4, n)
    feats = centres[genre] + np.concatenate([0.3 * rng.standard_normal((n, 8)), 1.0 * rng.standard_normal((n, d - 8))], axis=1)
    songs = [bliss.Song(path=f"/m/{i}.flac", analysis=bliss.Analysis(feats[i].astype(np.float32), V2), features_version=V2,
                        genre=None if i % 40 == 0 else f"genre {genre[i]}") for i in range(n)]
    db = sqlite3.connect(":memory:")
    lib.create_schema(db)
    lib.store_songs(db, songs)
    M = lib.learn_metric(db, source="genre", max_iter=40)
    assert M.shape == (d, d) and M.dtype == np.float32 and np.isfinite(M).all()
    assert np.array_equal(M, M.T) and np.linalg.eigvalsh(M.astype(np.float64)).min() > -1e-5 * np.abs(M).max()  # SPD within rounding
    assert np.diag(M)[:8].mean() > np.diag(M)[8:].mean()  # the features the genres differ in weigh more
    table = lib.similar_songs(db, 5, bliss.playlist.MahalanobisBuilder(M))
    assert len(table) == n and all(len(v) == 5 for v in table.values())
    # the survey table as the source, and a label array
    lib.store_training_triplet(db, "/m/1.flac", "/m/2.flac", "/m/3.flac")
    lib.store_training_triplet(db, "/m/5.flac", "/m/2.flac", "/m/7.flac")
    res = lib.learn_metric(db, source="triplets", form="diagonal", max_iter=10, return_result=True)
    assert res.m.shape == (d, d) and res.active.shape[0] == res.n_iter + 1 and res.active[0] <= 4
    M2 = lib.learn_metric(db, source=genre, form="diagonal", max_iter=10, n_triplets=2000, seed=1)
    assert np.count_nonzero(M2 - np.diag(np.diag(M2))) == 0
