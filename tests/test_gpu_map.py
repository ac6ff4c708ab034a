"""GPU tests (-m gpu) of the 2-D map (blissgpu_map_step / blissgpu_map_layout: map_repulse_kernel, map_attract_kernel,
map_update_kernel).  The expected values come from a numpy loop written from the arithmetic contract of
include/blissgpu.h alone -- float32 pair quantities, every operation rounded on its own, sequential float64 sums by
np.cumsum(...)[..., -1] in the stated order -- never from the code under test, and every comparison is on bits."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, ONE = np.float32, np.float32(1.0)


@pytest.fixture(scope="module")
def bliss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import bliss_rs_amd

    return bliss_rs_amd


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- the contract in numpy ----
def _seq(a):
    """the sequential float64 sum of the last axis from +0.0 ([..., 0] -> +0.0)"""
    a = np.asarray(a, np.float64)
    z = np.zeros(a.shape[:-1] + (1,), np.float64)
    return np.cumsum(np.concatenate([z, a], axis=-1), axis=-1)[..., -1]


def _pairs(Yi, Yj):
    """dx, dy, q of every (row of Yi, row of Yj): float32, each operation rounded on its own"""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = Yi[:, None, 0] - Yj[None, :, 0]
        dy = Yi[:, None, 1] - Yj[None, :, 1]
        s = dx * dx + dy * dy
        q = ONE / (ONE + s)
    assert dx.dtype == q.dtype == np.float32
    return dx, dy, q


def ref_step(Y, ro, cols, vals, exaggeration, C, reverse=False, flat_z=False):
    """-> grad f64 [n, 2], z_rows f64 [n], Z: the statements of include/blissgpu.h, one after the other.  reverse (every chunk's
    j descending) and flat_z (Z as one sequential sum over the rows) are NOT the contract: test_the_expectation_is_order_sensitive
    uses them to show that the inputs of this file tell such a kernel from the right one"""
    Y = np.asarray(Y, np.float32)
    n = Y.shape[0]
    if n < 2:
        return np.zeros((n, 2)), np.zeros(n), 0.0
    ro = np.asarray(ro, np.int64)
    cols = np.asarray(cols, np.int64)
    vals = np.asarray(vals, np.float32)
    w = 256 * -(-(-(-n // C)) // 256)
    rows = np.arange(n)
    parts = np.zeros((3, n, C))  # an empty chunk's sums stay +0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(C):
            j0, j1 = c * w, min(n, (c + 1) * w)
            if j0 >= n:
                break
            dx, dy, q = _pairs(Y, Y[j0:j1])
            terms = [q.astype(np.float64), ((q * q) * dx).astype(np.float64), ((q * q) * dy).astype(np.float64)]
            # j != i: the diagonal entry is taken out of the sequence (the entries behind it move up, +0.0 is appended: the
            # sequence of additions of the other entries is untouched)
            inside = (rows >= j0) & (rows < j1)
            for t in terms:
                for i in rows[inside]:
                    t[i, i - j0:-1] = t[i, i - j0 + 1:]
                    t[i, -1] = 0.0
            for k in range(3):
                parts[k, :, c] = _seq(terms[k][:, ::-1] if reverse else terms[k])
        z, rx, ry = _seq(parts[0]), _seq(parts[1]), _seq(parts[2])
        # attraction: the row's CSR entries in stored order
        att = np.zeros((n, 2))
        row = np.repeat(rows, np.diff(ro))
        dxe = Y[row, 0] - Y[cols, 0]
        dye = Y[row, 1] - Y[cols, 1]
        qe = ONE / (ONE + (dxe * dxe + dye * dye))
        we = vals * qe
        tx, ty = (we * dxe).astype(np.float64), (we * dye).astype(np.float64)
        assert we.dtype == np.float32
        for i in range(n):
            att[i, 0], att[i, 1] = _seq(tx[ro[i]:ro[i + 1]]), _seq(ty[ro[i]:ro[i + 1]])
        Z = _seq(z) if flat_z else _seq(np.asarray([_seq(z[b:b + 256]) for b in range(0, n, 256)]))
        E = np.float64(np.float32(exaggeration))
        r = np.stack([rx, ry], axis=1)
        grad = 4.0 * (E * att - r / Z)
    return grad, z, float(Z)


def ref_update(Y, grad, U, gain, lr, mom, min_gain):
    with np.errstate(over="ignore", invalid="ignore"):
        gain = np.where(U * grad < 0.0, gain + 0.2, gain * 0.8)
        gain = np.maximum(gain, min_gain)
        U = mom * U - (lr * gain) * grad
        Y = (Y.astype(np.float64) + U).astype(np.float32)
    return Y, U, gain


def ref_layout(Y0, ro, cols, vals, n_iter, exag_iters, exaggeration, lr, mom0, mom1, min_gain, C):
    Y = np.asarray(Y0, np.float32).copy()
    U, gain, trace = np.zeros(Y.shape), np.ones(Y.shape), np.zeros(n_iter)
    for it in range(n_iter):
        E, mom = (exaggeration, mom0) if it < exag_iters else (1.0, mom1)
        grad, _, trace[it] = ref_step(Y, ro, cols, vals, E, C)
        Y, U, gain = ref_update(Y, grad, U, gain, lr, mom, min_gain)
    return Y, trace


# ---- inputs ----
def planted(n, seed=0, k=8, d=23, sigma=0.6):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((k, d))
    labels = rng.integers(0, k, n)
    return (centres[labels] + sigma * rng.standard_normal((n, d))).astype(np.float32), labels


def wide_points(n, seed, lo=-20.0, hi=16.0):
    """n points whose pair terms do not fit one float64 window: magnitudes log-uniform over 2^lo .. 2^hi with random signs,
    and every eighth point a near-duplicate (2^-18 relative) of the one before it.  Sums of float32 terms are exact in
    float64 -- and so the same in ANY order -- while the terms' bits span fewer than 53 binary places; Gaussian points of
    one scale stay inside that, and a kernel with another chunk width, another order inside a chunk or another Z reduction
    would pass.  With these points it does not (test_the_expectation_is_order_sensitive)."""
    rng = np.random.default_rng(seed)
    Y = (rng.choice([-1.0, 1.0], (n, 2)) * np.exp2(rng.uniform(lo, hi, (n, 2)))).astype(np.float32)
    dup = np.arange(7, n, 8)
    Y[dup] = Y[dup - 1] * np.float32(1.0 + 2.0 ** -18)
    return Y


@functools.lru_cache(maxsize=None)
def _case(n):
    """(Y, row_offsets, cols, vals float32) of n planted songs: P from map_affinities of the device's nearest lists"""
    from bliss_rs_amd import playlist as pl

    X, _ = planted(n, seed=0 if n == 600 else n)
    Y = wide_points(n, 100 + n)
    if n < 2:
        return Y, np.zeros(n + 1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32)
    k = min(n - 1, 90)
    idx, dist = pl.nearest_order(X, X, k, skip=np.arange(n))
    ro, cols, vals = pl.map_affinities(idx, dist, 30.0)
    for a in (Y, ro, cols, vals):
        a.setflags(write=False)
    return Y, ro, cols, vals.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _expected(n, C, exaggeration=1.0):
    Y, ro, cols, vals = _case(n)
    return ref_step(Y, ro, cols, vals, exaggeration, C)


def _n_cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- 1. map_step, plain shapes ----
@pytest.mark.parametrize("col_groups", [1, 2, 3, 7, 0])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 600, 700, 1100])
def test_map_step_equals_the_contract(bliss, n, col_groups):
    pl = bliss.playlist
    Y, ro, cols, vals = _case(n)
    C = col_groups if col_groups else pl.map_plan(n, _n_cus())
    if n == 600:  # the longest row (312 entries) is past one wavefront, past one tile, and past what a lane walks alone
        assert np.diff(ro.astype(np.int64)).max() > 256
    grad, z_rows, Z = pl.map_step(Y, ro, cols, vals, 1.0, col_groups)
    want_grad, want_z, want_Z = _expected(n, C)
    assert same_bits(z_rows, want_z)
    assert same_bits(np.float64(Z), np.float64(want_Z))
    assert same_bits(grad, want_grad)
    if n >= 2:
        assert np.isfinite(grad).all() and Z > 0 and np.abs(grad).max() > 0


def _differing(a, b):
    return int((_bits(a) != _bits(b)).sum())


@pytest.mark.parametrize("n", [600, 700, 1100])
def test_the_expectation_is_order_sensitive(bliss, n):
    """What the bit comparisons above can see.  Sums of float32 terms that fit one 53-bit window are exact in float64 and the
    same in any order; with wide_points they are not, and the numpy expectation itself changes with the chunking, with the
    order inside a chunk and with the shape of the Z reduction -- so a kernel that got any of those wrong fails
    test_map_step_equals_the_contract.  (n = 1100 is there for col_groups = 7: up to 768 rows it cuts j exactly as 3 does.)"""
    Y, ro, cols, vals = _case(n)
    e = {C: _expected(n, C) for C in (1, 2, 3, 7)}
    for a, b in ((1, 2), (1, 3), (2, 3)) + (((3, 7), (2, 7)) if n > 768 else ()):
        changed = _differing(e[a][0], e[b][0]), _differing(e[a][1], e[b][1])
        print(f"n={n}: col_groups {a} against {b}: {changed[0]} entries of grad and {changed[1]} of z_rows differ")
        assert changed[0] > n // 4 and changed[1] > n // 8, (a, b, changed)
    # col_groups = 0: whatever map_plan names cuts j unlike at least one of the others
    plan = _expected(n, bliss.playlist.map_plan(n, _n_cus()))
    assert max(_differing(plan[1], e[C][1]) for C in (1, 2, 3, 7)) > n // 8
    back = ref_step(Y, ro, cols, vals, 1.0, 3, reverse=True)
    flat = ref_step(Y, ro, cols, vals, 1.0, 3, flat_z=True)
    print(f"n={n}: j descending: {_differing(e[3][1], back[1])} of z_rows differ; Z by blocks {e[3][2]!r}, flat {flat[2]!r}")
    assert _differing(e[3][1], back[1]) > n // 8 and _differing(e[3][0], back[0]) > n // 4
    assert same_bits(e[3][1], flat[1]) and flat[2] != e[3][2] and _differing(e[3][0], flat[0]) > n // 4


# ---- 2. map_step, edge cases ----
@pytest.mark.parametrize("exaggeration", [1.0, 12.0])
def test_map_step_edge_cases(bliss, exaggeration):
    pl = bliss.playlist
    Y, ro, cols, vals = _case(600)
    Y = Y.copy()
    # emptied rows (the CSR arithmetic reads rows only: nothing asks the rest to stay symmetric)
    keep = np.ones(len(cols), bool)
    r64 = ro.astype(np.int64)
    assert np.diff(r64).max() > 256 and np.diff(r64).argmax() not in (0, 17, 255, 256)  # the long row stays
    for i in (0, 17, 255, 256):
        keep[r64[i]:r64[i + 1]] = False
    counts = np.diff(r64)
    counts[[0, 17, 255, 256]] = 0
    ro2 = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    cols2, vals2 = cols[keep], vals[keep]
    Y[5] = Y[6] = Y[7]                        # duplicate points: dx = 0, q = 1
    Y[40], Y[41] = (1e19, 1e19), (-1e19, -1e19)  # s overflows against each other: q = +0
    Y[42] = (-1e19, 3.0)                      # against (1e19, 1e19): s = inf; against ordinary points: dx^2 = 1e38, q subnormal
    with np.errstate(over="ignore"):
        _, _, q = _pairs(Y[42:43], Y[100:101])
        _, _, q0 = _pairs(Y[40:41], Y[41:42])
    assert 0 < q[0, 0] < np.finfo(np.float32).tiny and q0[0, 0] == 0  # a subnormal q, and a q of +0
    want_grad, want_z, want_Z = ref_step(Y, ro2, cols2, vals2, exaggeration, 3)
    grad, z_rows, Z = pl.map_step(Y, ro2, cols2, vals2, exaggeration, 3)
    assert same_bits(z_rows, want_z) and same_bits(np.float64(Z), np.float64(want_Z)) and same_bits(grad, want_grad)
    assert np.isfinite(grad).all()
    assert (grad[[0, 17, 255, 256]] != 0).any()  # an emptied row is still pushed


# ---- 3. map_layout ----
LAYOUT = dict(exaggeration=12.0, learning_rate=80.0, momentum0=0.5, momentum1=0.8, min_gain=0.01)


@functools.lru_cache(maxsize=None)
def _layout_case():
    from bliss_rs_amd import playlist as pl

    n = 300
    X, _ = planted(n, seed=1)
    idx, dist = pl.nearest_order(X, X, 90, skip=np.arange(n))
    ro, cols, vals = pl.map_affinities(idx, dist, 30.0)
    Y0 = wide_points(n, 5)  # (starting positions of one small scale would leave every sum exact: see wide_points)
    return Y0, ro, cols, vals.astype(np.float32)


def test_map_layout_equals_thirty_numpy_steps(bliss):
    pl = bliss.playlist
    Y0, ro, cols, vals = _layout_case()
    Y, trace = pl.map_layout(Y0, ro, cols, vals, n_iter=30, exag_iters=10, col_groups=3, **LAYOUT)
    want_Y, want_trace = ref_layout(Y0, ro, cols, vals, 30, 10, 12.0, 80.0, 0.5, 0.8, 0.01, 3)
    assert same_bits(trace, want_trace)
    assert same_bits(Y, want_Y)
    assert np.abs(Y - Y0).max() > 0 and (trace > 0).all()
    # the comparison sees the chunking: one chunk gives another trace (Y is rounded to float32 in every iteration, which
    # swallows a last-bit difference of the float64 gradient, so the trace is where it shows)
    _, other = ref_layout(Y0, ro, cols, vals, 30, 10, 12.0, 80.0, 0.5, 0.8, 0.01, 1)
    print("iterations whose Z differs between col_groups 3 and 1:", int((other != want_trace).sum()))
    assert (other != want_trace).any()


def test_map_layout_of_one_iteration_is_a_step_and_an_update(bliss):
    pl = bliss.playlist
    Y0, ro, cols, vals = _layout_case()
    grad, _, Z = pl.map_step(Y0, ro, cols, vals, 12.0, 2)
    want_Y, _, _ = ref_update(Y0, grad, np.zeros(Y0.shape), np.ones(Y0.shape), 80.0, 0.5, 0.01)
    Y, trace = pl.map_layout(Y0, ro, cols, vals, n_iter=1, exag_iters=10, col_groups=2, **LAYOUT)
    assert same_bits(Y, want_Y) and same_bits(trace, np.asarray([Z]))
    # past the exaggeration: (1.0, momentum1) from the first iteration on
    grad, _, Z = pl.map_step(Y0, ro, cols, vals, 1.0, 2)
    want_Y, _, _ = ref_update(Y0, grad, np.zeros(Y0.shape), np.ones(Y0.shape), 80.0, 0.8, 0.01)
    Y, trace = pl.map_layout(Y0, ro, cols, vals, n_iter=1, exag_iters=0, col_groups=2, **LAYOUT)
    assert same_bits(Y, want_Y) and same_bits(trace, np.asarray([Z]))


def test_map_layout_reports_a_nan(bliss):
    from bliss_rs_amd import _ffi

    pl = bliss.playlist
    Y0, ro, cols, vals = _layout_case()
    bad = Y0.copy()
    bad[123, 1] = np.nan
    with pytest.raises(_ffi.BlissGpuError) as e:
        pl.map_layout(bad, ro, cols, vals, n_iter=3, exag_iters=1, **LAYOUT)
    assert e.value.code == _ffi.ERR_NAN
    Y, trace = pl.map_layout(Y0, ro, cols, vals, n_iter=3, exag_iters=1, **LAYOUT)  # the context is fine afterwards
    assert np.isfinite(Y).all() and (trace > 0).all()


# ---- 4. end to end ----
def _label_share(xy, labels, k=10):
    D = ((xy[:, None, :].astype(np.float64) - xy[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(D, np.inf)
    nb = np.argsort(D, axis=1, kind="stable")[:, :k]
    return float((labels[nb] == labels[:, None]).mean())


def test_song_map_separates_planted_clusters(bliss):
    pl = bliss.playlist
    X, labels = planted(600, seed=0)
    start = _label_share(pl.map_init(X), labels)
    m = pl.song_map(X, n_iter=300, exag_iters=100)
    share = _label_share(m.xy, labels)
    print(f"share of the 10 nearest map neighbours with the song's label: PCA start {start:.3f}, map {share:.3f}; kl {m.kl:.4f}; "
          f"Z {m.z_trace[0]:.6g} -> {m.z_trace[-1]:.6g}")
    assert m.xy.dtype == np.float32 and m.xy.shape == (600, 2) and m.z_trace.shape == (300,)
    assert share >= 0.95
    assert start < 0.95  # the initialisation alone does not meet it
    assert np.isfinite(m.kl) and m.z_trace[-1] < m.z_trace[0]
    again = pl.song_map(X, n_iter=300, exag_iters=100)
    assert same_bits(again.xy, m.xy) and same_bits(again.z_trace, m.z_trace)  # fixed sum orders: the same bits every run


# ---- 5. the library ----
def test_library_song_map(bliss, tmp_path):
    X, labels = planted(80, seed=4)
    V2 = bliss.FeaturesVersion.Version2
    songs = [bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist="a", album=f"album {int(labels[i])}", duration=1.0,
                        analysis=bliss.Analysis(X[i], V2), features_version=V2) for i in range(80)]
    db = str(tmp_path / "bliss.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs[40:] + songs[:40])  # ids are not in path order
    m, paths = bliss.library.song_map(db, perplexity=10.0, n_iter=60, exag_iters=20)
    assert paths == [s.path for s in songs[40:] + songs[:40]]
    order = np.r_[40:80, 0:40]
    want = bliss.playlist.song_map(X[order], perplexity=10.0, n_iter=60, exag_iters=20)
    assert same_bits(m.xy, want.xy) and same_bits(m.z_trace, want.z_trace) and m.kl == want.kl
    assert m.xy.shape == (80, 2) and np.isfinite(m.xy).all() and np.isfinite(m.kl)
    empty = str(tmp_path / "empty.db")
    bliss.library.create_schema(empty)
    m0, p0 = bliss.library.song_map(empty, n_iter=5)
    assert p0 == [] and m0.xy.shape == (0, 2) and m0.z_trace.shape == (5,)
