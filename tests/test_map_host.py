"""Device-free tests of the 2-D map (blissgpu_map_step / blissgpu_map_layout / blissgpu_map_plan): the C ABI
surface (header, .so and _ffi.SIGNATURES held to one another), the build (the translation unit, its compile flags, the kernels'
names in the profile table), the argument checks that happen before the device is touched, blissgpu_map_plan against a Python
restatement, and the numpy half of the feature: map_affinities and map_init."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
OK, INVALID = 0, 2
NAMES = ("blissgpu_map_step", "blissgpu_map_layout", "blissgpu_map_plan")
KERNELS = ("map_repulse_kernel", "map_attract_kernel", "map_update_kernel")


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


# ---- the surface ----
def test_map_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    lib = C.CDLL(bliss.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, flat), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name
    # host-pointer forms only: no device-pointer form is exported, declared or bound
    for name in NAMES:
        assert not hasattr(lib, name + "_device") and name + "_device" not in _ffi.SIGNATURES and name + "_device" not in flat
    assert not any(hasattr(bliss.Context, m) for m in ("map_step", "map_layout", "song_map"))

    def types(name):
        return [re.sub(r"\s*\b\w+$", "", " ".join(a.split())).replace(" *", "*")
                for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, flat).group(1).split(",")]

    to_ffi = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int, "float": C.c_float, "double": C.c_double}
    csr = ["const float*", "uint64_t", "const uint64_t*", "const uint32_t*", "const float*"]  # (y, n, row_offsets, cols, vals)
    want = {
        # (..., exaggeration, col_groups, grad, z_rows, Z)
        "blissgpu_map_step": csr + ["float", "uint32_t", "double*", "double*", "double*"],
        # (..., n_iter, exag_iters, exaggeration, learning_rate, momentum0, momentum1, min_gain, col_groups, y_out, z_trace)
        "blissgpu_map_layout": csr + ["uint32_t", "uint32_t", "float", "double", "double", "double", "double", "uint32_t", "float*",
                                      "double*"],
    }
    for name, w in want.items():
        assert types(name) == w, name
        assert _ffi.SIGNATURES[name] == (C.c_int, [to_ffi.get(t, _vp) for t in w]), name
    assert types("blissgpu_map_plan") == ["uint64_t", "uint32_t", "uint32_t*"]
    assert _ffi.SIGNATURES["blissgpu_map_plan"] == (C.c_int, [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32)])
    # the header and the table stay equal sets
    declared = set(re.findall(r"\b(blissgpu_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_ffi.SIGNATURES)
    for name in ("map_affinities", "map_init", "map_step", "map_layout", "map_plan", "song_map", "SongMap"):
        assert hasattr(bliss.playlist, name), name
    assert hasattr(bliss.library, "song_map")


def test_map_build_and_profile_table(bliss):
    from bliss_rs_amd import _ffi

    L = _ffi.lib()
    names = [L.blissgpu_profile_kernel_name(k).decode() for k in range(L.blissgpu_profile_kernel_count())]
    assert len(set(names)) == len(names) and "" not in names
    src = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "kernels_map.hip")).read()
    for name in KERNELS:
        assert names.count(name) == 1, name
        assert re.search(r"\bvoid\s+%s\s*\(" % name, src), name
        assert names.index(name) < len(names) - 2
    assert names[-2:] == ["group_forest_scan_kernel", "journey_step_kernel"]  # (older ids keep their places)
    mk = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "Makefile")).read()
    line = [l for l in mk.splitlines() if "EXTRA := $(NOCONTRACT)" in l]
    assert len(line) == 1 and "kernels_map.o" in line[0]  # compiled -ffp-contract=off
    assert "kernels_map.o" in [l for l in mk.splitlines() if l.startswith("OBJS")][0]


# ---- the argument checks: before the device is touched ----
def _p(a):
    return None if a is None else a.ctypes.data


def _csr(n=4):
    """a ring: row i holds its two neighbours"""
    cols = np.asarray([sorted(((i - 1) % n, (i + 1) % n)) for i in range(n)], np.uint32).reshape(-1)
    return np.arange(0, 2 * n + 1, 2, dtype=np.uint64), cols, np.full(2 * n, 0.125, np.float32)


def _call(layout=False, n=4, ro=None, cols=None, vals=None, null=(), exaggeration=1.0, col_groups=1, n_iter=3, lr=10.0, mom=(0.5, 0.8),
          min_gain=0.01):
    from bliss_rs_amd import _ffi

    r0, c0, v0 = _csr(4)
    a = {"y": np.arange(8, dtype=np.float32).reshape(4, 2), "ro": r0 if ro is None else np.asarray(ro, np.uint64),
         "cols": c0 if cols is None else np.asarray(cols, np.uint32), "vals": v0 if vals is None else np.asarray(vals, np.float32),
         "grad": np.full((4, 2), 7.0), "z_rows": np.full(4, 7.0), "Z": np.full(1, 7.0), "y_out": np.full((4, 2), 7.0, np.float32),
         "trace": np.full(max(n_iter, 1), 7.0)}
    g = lambda name: None if name in null else _p(a[name])  # noqa: E731
    L = _ffi.lib()
    if layout:
        rc = L.blissgpu_map_layout(g("y"), n, g("ro"), g("cols"), g("vals"), n_iter, 1, exaggeration, lr, mom[0], mom[1], min_gain,
                                   col_groups, g("y_out"), g("trace"))
    else:
        rc = L.blissgpu_map_step(g("y"), n, g("ro"), g("cols"), g("vals"), exaggeration, col_groups, g("grad"), g("z_rows"), g("Z"))
    return rc, L.blissgpu_last_error(), a


def test_map_arguments_are_checked_before_the_device(bliss):
    nan, inf = float("nan"), float("inf")
    bad = [(dict(null=("y",)), b"y is NULL"), (dict(null=("ro",)), b"row_offsets is NULL"), (dict(null=("cols",)), b"cols is NULL"),
           (dict(null=("vals",)), b"vals is NULL"),
           (dict(n=1 << 24), b"n must be below 2^24"), (dict(n=1 << 40), b"n must be below 2^24"),
           (dict(n=2, ro=[0, 1 << 32, 1 << 32]), b"nnz must be below 2^32"),
           (dict(ro=[1, 2, 4, 6, 8]), b"row_offsets[0]"), (dict(ro=[0, 2, 1, 6, 8]), b"must not decrease"),
           (dict(cols=[3, 1, 0, 2, 1, 3, 0, 2]), b"strictly ascending"),     # row 0 unsorted
           (dict(cols=[1, 1, 0, 2, 1, 3, 0, 2]), b"strictly ascending"),     # row 0 holds a duplicate
           (dict(cols=[1, 3, 0, 1, 1, 3, 0, 2]), b"holds itself"),           # row 1 holds itself
           (dict(cols=[1, 4, 0, 2, 1, 3, 0, 2]), b">= n"),                   # row 0 points past the rows
           (dict(cols=[1, 0xFFFFFFFF, 0, 2, 1, 3, 0, 2]), b">= n"),
           (dict(vals=[0.1, -0.1] + [0.1] * 6), b"vals must be"), (dict(vals=[0.1, nan] + [0.1] * 6), b"vals must be"),
           (dict(vals=[0.1] * 7 + [inf]), b"vals must be"),
           (dict(col_groups=65), b"col_groups"), (dict(col_groups=0xFFFFFFFF), b"col_groups"),
           (dict(exaggeration=nan), b"finite"), (dict(exaggeration=inf), b"finite")]
    for layout in (False, True):
        for kw, text in bad:
            rc, err, _ = _call(layout=layout, **kw)
            assert rc == INVALID and text in err, (layout, kw, err)
    for kw, text in [(dict(null=("grad",)), b"grad is NULL"), (dict(null=("Z",)), b"Z is NULL")]:
        rc, err, _ = _call(**kw)
        assert rc == INVALID and text in err, (kw, err)
    for kw in (dict(null=("y_out",)), dict(lr=nan), dict(lr=inf), dict(mom=(nan, 0.8)), dict(mom=(0.5, -inf)), dict(min_gain=nan)):
        rc, err, _ = _call(layout=True, **kw)
        assert rc == INVALID and (b"y_out is NULL" in err or b"finite" in err), (kw, err)
    # nothing to do: OK without a device
    rc, _, a = _call(n=0, null=("y", "ro", "cols", "vals", "grad", "z_rows"))
    assert rc == OK and a["Z"][0] == 0.0
    assert _call(layout=True, n=0, null=("y", "ro", "cols", "vals", "y_out", "trace"))[0] == OK
    # one point: no pair; grad = 0, Z = 0, the layout stays where it is and traces zeros
    rc, _, a = _call(n=1, ro=[0, 0], null=("cols", "vals"))
    assert rc == OK and a["Z"][0] == 0.0 and (a["grad"][0] == 0.0).all() and a["z_rows"][0] == 0.0 and (a["grad"][1:] == 7.0).all()
    rc, _, a = _call(layout=True, n=1, ro=[0, 0], null=("cols", "vals"))
    assert rc == OK and (a["y_out"][0] == a["y"][0]).all() and (a["trace"] == 0.0).all() and (a["y_out"][1:] == 7.0).all()
    # no iteration: y_out = y0
    rc, _, a = _call(layout=True, n_iter=0, null=("trace",))
    assert rc == OK and np.array_equal(a["y_out"], a["y"])
    # blissgpu_map_plan
    L = __import__("bliss_rs_amd")._ffi.lib()
    assert L.blissgpu_map_plan(100, 256, None) == INVALID and b"col_groups is NULL" in L.blissgpu_last_error()
    out = C.c_uint32(9)
    assert L.blissgpu_map_plan(1 << 24, 256, C.byref(out)) == INVALID


def test_map_wrappers_reject_bad_csr_before_the_library(bliss):
    pl = bliss.playlist
    ro, cols, vals = _csr(4)
    Y = np.zeros((4, 2), np.float32)
    bad = [(ro[:-1], cols, vals), (ro + 1, cols, vals), (ro, cols[:-1], vals), (ro, cols, vals[:-1]),
           (ro, np.asarray([3, 1, 0, 2, 1, 3, 0, 2]), vals), (ro, np.asarray([1, 1, 0, 2, 1, 3, 0, 2]), vals),
           (ro, np.asarray([1, 3, 0, 1, 1, 3, 0, 2]), vals), (ro, np.asarray([1, 4, 0, 2, 1, 3, 0, 2]), vals),
           (ro, np.asarray([1, -1, 0, 2, 1, 3, 0, 2]), vals), (ro, cols, -vals), (ro, cols, vals * np.nan),
           (np.asarray([0, 2, 1, 6, 8]), cols, vals)]
    for r, c, v in bad:
        with pytest.raises(ValueError):
            pl.map_step(Y, r, c, v)
        with pytest.raises(ValueError):
            pl.map_layout(Y, r, c, v, n_iter=2)
    for kw in (dict(col_groups=65), dict(col_groups=-1), dict(exaggeration=float("nan"))):
        with pytest.raises(ValueError):
            pl.map_step(Y, ro, cols, vals, **kw)
    for kw in (dict(learning_rate=float("inf")), dict(n_iter=-1), dict(min_gain=float("nan"))):
        with pytest.raises(ValueError):
            pl.map_layout(Y, ro, cols, vals, **kw)
    with pytest.raises(ValueError):
        pl.map_step(np.zeros((4, 3), np.float32), ro, cols, vals)
    for builder in (pl.ForestOptions(100, 64, None, 1, seed=0), pl.VarianceWeights()):
        with pytest.raises(ValueError):
            pl.song_map(np.zeros((8, 3), np.float32), metric_builder=builder)
        with pytest.raises(ValueError):
            bliss.library.song_map(":memory:", metric_builder=builder)


# ---- blissgpu_map_plan ----
def _plan(n, n_cus):
    cus = n_cus if n_cus > 0 else 256
    blocks = -(-n // 256)
    if blocks <= 1:
        return 1
    return max(1, min(-(-4 * cus // blocks), blocks, 64))


def test_map_plan_matches_its_statement(bliss):
    pl = bliss.playlist
    for n_cus in (0, 1, 8, 64, 104, 256, 304, 1024):
        for n in (0, 1, 2, 255, 256, 257, 511, 512, 513, 600, 700, 1000, 4096, 10 ** 4, 65535, 10 ** 5, 262143, 262144, 262145,
                  10 ** 6, (1 << 24) - 1):
            got = pl.map_plan(n, n_cus)
            assert got == _plan(n, n_cus), (n, n_cus, got)
            assert 1 <= got <= 64
            blocks = -(-n // 256)
            if blocks >= 4 * (n_cus or 256):
                assert got == 1  # the rows alone fill the device
            # the partials a plan asks for: 24 bytes per row and group, below 24 * 2 * 256 * 4 * n_cus
            if got > 1:
                assert 24 * got * n <= 24 * 2 * 256 * 4 * (n_cus or 256)


# ---- map_affinities ----
def _planted(n=600, seed=0, k=8, d=23, sigma=0.6):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((k, d))
    labels = rng.integers(0, k, n)
    return (centres[labels] + sigma * rng.standard_normal((n, d))).astype(np.float32), labels


def _knn(X, k):
    """every row's k nearest other rows by numpy (what nearest_order answers on the device)"""
    D = np.sqrt(((X[:, None, :].astype(np.float64) - X[None, :, :]) ** 2).sum(-1))
    np.fill_diagonal(D, np.inf)
    idx = np.argsort(D, axis=1, kind="stable")[:, :k]
    return idx, np.take_along_axis(D, idx, axis=1).astype(np.float32)


def _row_entropies(idx, dist, perplexity):
    """the entropy of every row's conditional distribution, recovered from P's construction by its own search"""
    from bliss_rs_amd import playlist as pl

    d2 = dist.astype(np.float64) ** 2
    d2 = d2 - d2.min(axis=1, keepdims=True)
    beta, lo, hi = np.ones(len(d2)), np.zeros(len(d2)), np.full(len(d2), np.inf)
    for _ in range(pl.MAP_BISECTIONS):
        p = np.exp(-beta[:, None] * d2)
        s = p.sum(1)
        h = np.log(s) + beta * (d2 * p).sum(1) / s
        more = h > np.log(perplexity)
        lo, hi = np.where(more, beta, lo), np.where(more, hi, beta)
        beta = np.where(np.isinf(hi), beta * 2.0, (lo + hi) / 2.0)
    p = np.exp(-beta[:, None] * d2)
    p /= p.sum(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return p, -(np.where(p > 0, p * np.log(p), 0.0)).sum(1)


def test_map_affinities(bliss):
    pl = bliss.playlist
    X, _ = _planted(300)
    n, perplexity = 300, 30.0
    idx, dist = _knn(X, 90)
    ro, cols, vals = pl.map_affinities(idx, dist, perplexity)
    assert ro.dtype == np.uint64 and cols.dtype == np.uint32 and vals.dtype == np.float64
    assert ro.shape == (n + 1,) and ro[0] == 0 and int(ro[-1]) == len(cols) == len(vals)
    # every row's conditional distribution has the asked perplexity.  map_affinities returns only the symmetrised P, from which
    # the rows' p cannot be recovered, so the entropies are taken from a restatement of the search (_row_entropies) and the
    # product is tied to exactly those rows by the comparison with (p + p^T) / 2n below, to 1e-12
    p, H = _row_entropies(idx, dist, perplexity)
    print("largest |entropy - log(perplexity)|:", np.abs(H - np.log(perplexity)).max())
    assert np.abs(H - np.log(perplexity)).max() <= 1e-9
    # ... and P is (p + p^T) / 2n of exactly those rows
    dense = np.zeros((n, n))
    np.put_along_axis(dense, idx, p, axis=1)
    dense = (dense + dense.T) / (2.0 * n)
    got = np.zeros((n, n))
    row = np.repeat(np.arange(n), np.diff(ro.astype(np.int64)))
    got[row, cols] = vals
    assert np.allclose(got, dense, rtol=1e-12, atol=0.0) and ((got > 0) == (dense > 0)).all()
    # sorted, no diagonal, symmetric in value, summing to 1
    assert (cols.astype(np.int64) != row).all()
    inside = row[1:] == row[:-1]
    assert (cols.astype(np.int64)[1:][inside] > cols.astype(np.int64)[:-1][inside]).all()
    assert np.array_equal(got, got.T)
    assert abs(vals.sum() - 1.0) <= 1e-12
    assert (vals >= 0).all() and np.isfinite(vals).all()
    # the wrappers' own CSR check accepts it
    pl._map_csr(n, ro, cols, vals)
    # padding entries are left out: the lists cut to 40 and padded back to 90 give what the lists of 40 give
    idx2, dist2 = idx.copy(), dist.copy()
    idx2[:, 40:], dist2[:, 40:] = -1, np.inf
    a = pl.map_affinities(idx2, dist2, perplexity)
    b = pl.map_affinities(idx[:, :40], dist[:, :40], perplexity)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_map_affinities_uniform_row_and_small_inputs(bliss):
    pl = bliss.playlist
    # row 0: every neighbour at the same distance -> uniform p, whatever the search does with beta
    idx = np.asarray([[1, 2, 3, 4], [0, 2, 3, 4], [0, 1, 3, 4], [0, 1, 2, 4], [0, 1, 2, 3]])
    dist = np.asarray([[2.0, 2.0, 2.0, 2.0], [2.0, 1.0, 3.0, 4.0], [2.0, 1.0, 2.5, 3.0], [2.0, 3.0, 2.5, 1.5], [2.0, 4.0, 3.0, 1.5]], np.float32)
    ro, cols, vals = pl.map_affinities(idx, dist, 2.0)
    n = 5
    got = np.zeros((n, n))
    got[np.repeat(np.arange(n), np.diff(ro.astype(np.int64))), cols] = vals
    p, _ = _row_entropies(idx, dist, 2.0)
    assert np.array_equal(p[0], np.full(4, 0.25))
    dense = np.zeros((n, n))
    np.put_along_axis(dense, idx, p, axis=1)
    assert np.allclose(got, (dense + dense.T) / (2.0 * n), rtol=1e-12, atol=0.0)
    assert abs(vals.sum() - 1.0) <= 1e-12
    # nothing in, nothing out
    ro, cols, vals = pl.map_affinities(np.zeros((0, 3), np.int64), np.zeros((0, 3), np.float32), 5.0)
    assert ro.tolist() == [0] and len(cols) == 0 and len(vals) == 0
    ro, cols, vals = pl.map_affinities(np.full((1, 3), -1), np.full((1, 3), np.inf, np.float32), 5.0)
    assert ro.tolist() == [0, 0] and len(cols) == 0
    with pytest.raises(ValueError):
        pl.map_affinities(idx, dist[:, :3], 2.0)
    with pytest.raises(ValueError):
        pl.map_affinities(idx, dist, 0.0)


# ---- map_init ----
def _moments_of(pl, X):
    """playlist.Moments of X by numpy (one group): what moments(X) answers on the device"""
    X64 = X.astype(np.float64)
    mean = X64.mean(0, keepdims=True)
    Xc = X64 - mean
    return pl.Moments([len(X)], mean, (Xc * Xc).sum(0, keepdims=True), X.min(0, keepdims=True), X.max(0, keepdims=True), Xc.T @ Xc)


def test_map_init_sign_rule_and_scale(bliss):
    pl = bliss.playlist
    rng = np.random.default_rng(3)
    X = (rng.standard_normal((400, 6)) * np.asarray([5.0, 3.0, 1.0, 0.5, 0.2, 0.1])).astype(np.float32)
    X = X @ np.linalg.qr(rng.standard_normal((6, 6)))[0].astype(np.float32) + 7.0
    mom = _moments_of(pl, X)
    Y = pl.map_init(X, mom)
    assert Y.dtype == np.float32 and Y.shape == (400, 2)
    assert abs(float(Y[:, 0].astype(np.float64).std()) / 1e-4 - 1.0) < 1e-5
    # the two leading principal axes, signs fixed so that the largest-magnitude entry is positive
    w, vec = np.linalg.eigh(mom.scatter)
    Xc = X.astype(np.float64) - mom.mean
    scale = 1e-4 / (Xc @ vec[:, -1]).std()
    for c in range(2):
        v = vec[:, -1 - c]
        v = v if v[np.argmax(np.abs(v))] > 0 else -v
        assert np.allclose(Y[:, c], (Xc @ v) * scale, rtol=1e-4, atol=1e-9), c
    assert Y[:, 0].astype(np.float64).var() > Y[:, 1].astype(np.float64).var() > 0
    # the rule decides the sign, not the solver: the scatter matrix of the mirrored library gives the same axes, so the
    # mirrored library's map is the mirror image
    Ym = pl.map_init(-X, _moments_of(pl, -X))
    assert np.allclose(Ym, -Y, rtol=1e-4, atol=1e-9)
    assert np.array_equal(pl.map_init(X, mom), Y)  # deterministic
    # one feature: the second coordinate is 0; rows that do not vary: all 0
    X1 = rng.standard_normal((50, 1)).astype(np.float32)
    Y1 = pl.map_init(X1, _moments_of(pl, X1))
    assert (Y1[:, 1] == 0).all() and abs(float(Y1[:, 0].astype(np.float64).std()) / 1e-4 - 1.0) < 1e-5
    Xc0 = np.ones((5, 3), np.float32)
    assert (pl.map_init(Xc0, _moments_of(pl, Xc0)) == 0).all()
    assert pl.map_init(np.zeros((0, 4), np.float32)).shape == (0, 2)
