"""Device-free tests of the locally scaled k-nearest search and the hubness measure (blissgpu_scaled_knn / blissgpu_knn_occurrence,
DESIGN.md 3.27): the C ABI surface (header, _ffi.SIGNATURES and the Rust declarations held to one another), the kernels' names
in the profile table, the argument checks that happen before the device is touched, the host-side parts of the Python layer
(scales_from_distances against a literal restatement of its definition, Hubness, neighbour_agreement), and the numpy fact the
feature rests on: local scaling takes most of the skewness out of the k-occurrence counts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
OK, NO_DEVICE, INVALID = 0, 1, 2
NAMES = ("blissgpu_scaled_knn", "blissgpu_scaled_knn_device", "blissgpu_knn_occurrence", "blissgpu_knn_occurrence_device")
LO, HI = np.float32(2.0 ** -60), np.float32(2.0 ** 60)


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


# ---- the surface ----
def test_scaled_knn_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "rust", "gpu.rs")).read())
    lib = C.CDLL(bliss.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, flat), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name

    def types(name):
        return [re.sub(r"\s*\b\w+$", "", " ".join(a.split())).replace(" *", "*")
                for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, flat).group(1).split(",")]

    def rust_types(name):
        args = re.search(r"pub fn %s\s*\(([^)]*)\)\s*->\s*c_int" % name, rust).group(1)
        return [" ".join(a.split(":", 1)[1].split()) for a in args.split(",")]

    to_rust = {"const float*": "*const f32", "float*": "*mut f32", "const uint32_t*": "*const u32", "uint32_t*": "*mut u32",
               "uint64_t": "u64", "uint32_t": "u32", "int": "c_int", "blissgpu_ctx*": "*mut blissgpu_ctx"}
    to_ffi = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int}
    # (queries, q, qscale, cand, n, cscale, d, metric, M, skip, k, idx, dist), the device form with the context
    knn = ["const float*", "uint64_t", "const float*", "const float*", "uint64_t", "const float*", "uint32_t", "int", "const float*",
           "const uint32_t*", "uint32_t", "uint32_t*", "float*"]
    occ = ["const uint32_t*", "uint64_t", "uint32_t", "uint64_t", "uint32_t*"]  # (idx, q, k, n, count)
    for name, want in (("blissgpu_scaled_knn", knn), ("blissgpu_scaled_knn_device", ["blissgpu_ctx*"] + knn),
                       ("blissgpu_knn_occurrence", occ), ("blissgpu_knn_occurrence_device", ["blissgpu_ctx*"] + occ)):
        assert types(name) == want, name
        assert rust_types(name) == [to_rust[t] for t in want], name
        assert _ffi.SIGNATURES[name] == (C.c_int, [to_ffi.get(t, _vp) for t in want]), name
    # the same prefix as blissgpu_knn with the two scales put in: the rest of the list is blissgpu_knn's
    base = types("blissgpu_knn")
    assert knn[:2] + knn[3:5] + knn[6:] == base
    for name in ("scales_from_distances", "local_scales", "scaled_nearest_order", "k_occurrence", "Hubness", "hubness",
                 "neighbour_agreement"):
        assert hasattr(bliss.playlist, name), name
    for name in ("similar_songs_scaled", "hubness", "orphan_songs"):
        assert hasattr(bliss.library, name), name
    assert hasattr(bliss.Context, "scaled_knn") and hasattr(bliss.Context, "knn_occurrence")


def test_scaled_knn_kernels_are_in_the_profile_table(bliss):
    from bliss_rs_amd import _ffi

    L = _ffi.lib()
    names = [L.blissgpu_profile_kernel_name(k).decode() for k in range(L.blissgpu_profile_kernel_count())]
    assert len(set(names)) == len(names) and "" not in names
    src = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "kernels_scaled_knn.hip")).read()
    for name in ("scaled_knn_scan_kernel", "knn_occurrence_kernel"):
        assert names.count(name) == 1, name
        assert re.search(r"\bvoid\s+%s\s*\(" % name, src), name
        assert names.index(name) < len(names) - 2
    assert names[-2:] == ["group_forest_scan_kernel", "journey_step_kernel"]  # (older ids keep their places)
    # the scan is its own kernel: knn_scan_kernel has no new template parameter
    knn_src = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "kernels_knn.hip")).read()
    assert re.search(r"template <int D, int METRIC, bool DIAG, int KEYS>\s*__global__[^\n]*void knn_scan_kernel\(", knn_src)
    mk = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "Makefile")).read()
    line = [l for l in mk.splitlines() if "EXTRA := $(NOCONTRACT)" in l]
    assert len(line) == 1 and "kernels_scaled_knn.o" in line[0]  # compiled -ffp-contract=off


# ---- the argument checks: before the device is touched ----
def _p(a):
    return None if a is None else a.ctypes.data


def _knn(q=4, n=6, d=23, metric=0, M=None, k=3, null=(), device=False):
    from bliss_rs_amd import _ffi

    a = dict(queries=np.zeros((max(q, 1), min(max(d, 1), 64)), np.float32), qscale=np.ones(max(q, 1), np.float32),
             cand=np.zeros((min(max(n, 1), 8), min(max(d, 1), 64)), np.float32), cscale=np.ones(min(max(n, 1), 8), np.float32),
             idx=np.zeros((max(q, 1), 1024), np.uint32), dist=np.zeros((max(q, 1), 1024), np.float32))
    g = lambda name: None if name in null else _p(a[name])  # noqa: E731
    args = (g("queries"), q, g("qscale"), g("cand"), n, g("cscale"), d, metric, _p(M), None, k, g("idx"), g("dist"))
    L = _ffi.lib()
    rc = L.blissgpu_scaled_knn_device(None, *args) if device else L.blissgpu_scaled_knn(*args)
    return rc, L.blissgpu_last_error()


def test_scaled_knn_arguments_are_checked_before_the_device(bliss):
    import torch

    for device in (False, True):
        for null in ("queries", "qscale", "cand", "cscale", "idx"):
            rc, err = _knn(null=(null,), device=device)
            assert rc == INVALID and null.encode() in err, (null, device, err)
        for k in (0, 1025):
            rc, err = _knn(k=k, device=device)
            assert rc == INVALID and b"k must be" in err
        for d in (0, 65):
            rc, err = _knn(d=d, device=device)
            assert rc == INVALID and b"d must be" in err
        for metric in (-1, 3):
            rc, err = _knn(metric=metric, device=device)
            assert rc == INVALID and b"unknown metric" in err
        rc, err = _knn(metric=2, device=device)
        assert rc == INVALID and b"mahalanobis needs M" in err
        rc, err = _knn(n=0xFFFFFFFF, device=device)
        assert rc == INVALID and b"n must be" in err
    # nothing to do: OK whatever the pointers (the device form needs its context first: q == 0 through it is a GPU test)
    assert _knn(q=0, null=("queries", "qscale", "idx", "dist"))[0] == OK
    rc, err = _knn(q=0, null=("queries", "qscale", "idx", "dist"), device=True)
    assert rc == INVALID and b"ctx is NULL" in err
    # n == 0 with queries: the host form needs a device for the padding rows, the device form its context
    assert _knn(q=0, n=0)[0] == OK
    rc, err = _knn(n=0, null=("cand", "cscale"), device=True)
    assert rc == INVALID and b"ctx is NULL" in err
    if not torch.cuda.is_available():
        rc, _ = _knn(n=0, null=("cand", "cscale"))
        assert rc in (OK, NO_DEVICE)
    # a skip entry >= n is refused by the host form before the device
    from bliss_rs_amd import _ffi

    Q, X, one = np.zeros((2, 23), np.float32), np.zeros((5, 23), np.float32), np.ones(5, np.float32)
    idx = np.zeros((2, 3), np.uint32)
    skip = np.array([0xFFFFFFFF, 5], np.uint32)
    L = _ffi.lib()
    assert L.blissgpu_scaled_knn(_p(Q), 2, _p(one), _p(X), 5, _p(one), 23, 0, None, _p(skip), 3, _p(idx), None) == INVALID
    assert b"skip entries" in L.blissgpu_last_error()


def test_knn_occurrence_arguments_are_checked_before_the_device(bliss):
    from bliss_rs_amd import _ffi

    L = _ffi.lib()
    idx = np.zeros((4, 3), np.uint32)
    count = np.full(5, 7, np.uint32)
    for device in (False, True):
        f = (lambda *a: L.blissgpu_knn_occurrence_device(None, *a)) if device else L.blissgpu_knn_occurrence
        assert f(None, 4, 3, 5, _p(count)) == INVALID and b"idx is NULL" in L.blissgpu_last_error()
        assert f(_p(idx), 4, 3, 5, None) == INVALID and b"count is NULL" in L.blissgpu_last_error()
        assert f(_p(idx), 4, 0, 5, _p(count)) == INVALID and b"k must be" in L.blissgpu_last_error()
        assert f(_p(idx), 4, 3, 0xFFFFFFFF, _p(count)) == INVALID and b"n must be" in L.blissgpu_last_error()
        assert f(_p(idx), 1 << 40, 3, 5, _p(count)) == INVALID and b"q * k" in L.blissgpu_last_error()
    assert L.blissgpu_knn_occurrence(None, 0, 3, 0, None) == OK
    assert L.blissgpu_knn_occurrence_device(None, None, 0, 3, 0, None) == INVALID and b"ctx is NULL" in L.blissgpu_last_error()
    # the host form: a bad entry is found before the device, q == 0 writes zeros without one
    bad = idx.copy()
    bad[2, 1] = 5
    assert L.blissgpu_knn_occurrence(_p(bad), 4, 3, 5, _p(count)) == INVALID and b"idx entries" in L.blissgpu_last_error()
    assert (count == 7).all()
    assert L.blissgpu_knn_occurrence(None, 0, 3, 5, _p(count)) == OK and (count == 0).all()
    assert bliss.playlist.k_occurrence(np.zeros((0, 3), np.int64), 4).tolist() == [0, 0, 0, 0]


# ---- scales_from_distances against its definition, restated literally ----
def scales_by_definition(dist, m, kind):
    dist = np.asarray(dist, np.float32)
    out = []
    for row in dist:
        finite = [v for v in row if np.isfinite(v)]
        c = min(m, len(finite))
        if c == 0:
            out.append(np.float32(1.0))
        elif kind == "mean":
            s = np.float64(0.0)
            for v in finite[:c]:
                s = s + np.float64(v)
            out.append(np.float32(s / np.float64(c)))
        else:
            out.append(np.float32(finite[c - 1]))
    ok = [v for v in out if v >= LO]
    floor = min(ok) if ok else np.float32(1.0)
    out = [floor if v < LO else v for v in out]
    return np.asarray([min(v, HI) for v in out], np.float32)


def test_scales_from_distances(bliss):
    f = bliss.playlist.scales_from_distances
    inf = np.inf
    rng = np.random.default_rng(0)
    D = np.sort(rng.random((50, 12)).astype(np.float32) * 3, axis=1)
    D[3, 5:] = inf      # a short row
    D[4, :] = inf       # nobody near
    D[5, :] = 0.0       # its neighbours are exact duplicates
    D[6, :4] = 0.0
    D[7, :] = [1e-30] * 12  # below 2^-60 but not zero
    D[8, :] = 3e38      # the mean is finite in f64 and above 2^60
    D[9, 11] = inf
    for kind in ("mean", "kth"):
        for m in (1, 4, 10, 12, 40):  # (40: larger than the row)
            got, want = f(D, m, kind), scales_by_definition(D, m, kind)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (kind, m)
            assert (got >= LO).all() and (got <= HI).all()
            assert got[4] == 1.0 and got[8] == HI
            assert got[5] == got[7] == want[want >= LO].min()  # raised to the smallest admissible result
    assert f(D, 10, "kth")[3] == D[3, 4] and f(D, 4, "kth")[3] == D[3, 3]
    # all rows zero (or empty): 1
    assert f(np.zeros((3, 5), np.float32), 3).tolist() == [1.0, 1.0, 1.0]
    assert f(np.full((2, 5), inf, np.float32), 3, "kth").tolist() == [1.0, 1.0]
    assert f(np.zeros((0, 5), np.float32), 3).shape == (0,)
    # the sum is f64, in order, rounded once at the end: f32 accumulation gives other bits here
    one_up = np.float32(1.0) + np.float32(2.0 ** -23)
    row = np.array([[1.0, one_up, one_up]], np.float32)  # 1 + (1 + ulp) ties to 2 in f32; f64 keeps both ulps
    s32 = np.float32(0)
    for v in row[0]:
        s32 = np.float32(s32 + v)
    want = np.float32((np.float64(1.0) + np.float64(one_up) + np.float64(one_up)) / 3)
    assert np.float32(s32 / np.float32(3)) == 1.0 and want == one_up
    assert f(row, 3)[0] == want == scales_by_definition(row, 3, "mean")[0]
    for bad in (dict(m=0), dict(m=3, kind="median")):
        with pytest.raises(ValueError):
            f(D, **bad)
    with pytest.raises(ValueError):
        f(np.array([[0.0, np.nan]], np.float32), 2)


def test_builders_that_cannot_be_scaled_are_refused(bliss):
    pl = bliss.playlist
    X = np.zeros((4, 23), np.float32)
    for builder, text in ((pl.ForestOptions(8, 4, 3, 0), "forest"), (pl.VarianceWeights(), "variance-based weights")):
        for call in (lambda b: pl.local_scales(X, 2, "mean", b), lambda b: bliss.library.similar_songs_scaled("none.db", 3, metric_builder=b),
                     lambda b: bliss.library.hubness("none.db", 3, metric_builder=b), lambda b: bliss.library.orphan_songs("none.db", 3, metric_builder=b)):
            with pytest.raises((TypeError, ValueError)) as e:
                call(builder)
            assert text.lower() in str(e.value).lower()


# ---- hubness and neighbour agreement ----
def test_hubness_on_hand_made_counts(bliss):
    H = bliss.playlist.Hubness
    h = H.from_counts([3, 0, 3, 1, 0, 5], 2)
    c = np.array([3, 0, 3, 1, 0, 5], np.float64)
    dev = c - c.mean()
    assert h.skewness == float((dev ** 3).mean() / (dev ** 2).mean() ** 1.5) and h.k == 2 and h.counts.dtype == np.int64
    assert h.hubs(3).tolist() == [5, 0, 2] and h.hubs(0).tolist() == [] and h.hubs(99).tolist() == [5, 0, 2, 3, 1, 4]
    assert h.orphans().tolist() == [1, 4]
    assert H.from_counts([4, 4, 4], 4).skewness == 0.0 and H.from_counts([4, 4, 4], 4).orphans().size == 0
    assert H.from_counts([], 4).skewness == 0.0
    # one hub, everyone else once: (n - 2) / sqrt(n - 1) for counts (n, 1, ..., 1) shifted -- a closed form
    n = 10
    h = H.from_counts([n] + [1] * (n - 1), 1)
    assert abs(h.skewness - (n - 2) / np.sqrt(n - 1)) < 1e-12
    assert H.from_counts([0, 2, 2, 2], 1).skewness < 0  # the sign: a tail of UNDER-listed songs is negative


def test_neighbour_agreement(bliss):
    f = bliss.playlist.neighbour_agreement
    labels = np.array([0, 0, 1, -1, 1, 2])
    idx = np.array([[1, 2, 3],      # song 0 (label 0): 1 agrees, 2 does not, 3 is unlabelled -> 1 / 2
                    [0, -1, -1],    # song 1: one counted neighbour, agrees -> 1
                    [4, 0, 1],      # song 2 (label 1): 1 / 3
                    [0, 1, 2],      # song 3 is unlabelled: left out
                    [3, -1, -1],    # song 4: its only neighbour is unlabelled: nothing counted, left out
                    [-1, -1, -1]])  # song 5: padding only: left out
    assert f(idx, labels) == (0.5 + 1.0 + 1.0 / 3.0) / 3.0
    assert f(idx.astype(np.int32), labels) == f(idx, labels)
    u = np.where(idx < 0, 0xFFFFFFFF, idx).astype(np.uint32)  # the library's own padding value
    assert f(u, labels) == f(idx, labels)
    assert np.isnan(f(np.full((2, 2), -1), [0, 1]))
    with pytest.raises(ValueError):
        f(idx, labels[:4])


# ---- the fact the feature rests on, in numpy over the oracle's distances ----
def scaled_lists(Dm, scale, k):
    """the contract in numpy: f32 product, root and division, stable order, every song skipping itself"""
    n = Dm.shape[0]
    r = np.sqrt((scale[:, None] * scale[None, :]).astype(np.float32)).astype(np.float32)
    S = (Dm / r).astype(np.float32)
    np.fill_diagonal(S, np.inf)
    return np.argsort(S, axis=1, kind="stable")[:, :k]


def test_local_scaling_removes_most_of_the_hubness(bliss, oracle):
    n, k, m = 1500, 10, 10
    X = np.random.default_rng(0).standard_normal((n, 23)).astype(np.float32)
    Dm = oracle.pairwise(X, X, "euclidean", None, n_threads=16)
    raw = Dm.copy()
    np.fill_diagonal(raw, np.inf)
    order = np.argsort(raw, axis=1, kind="stable")
    near = np.take_along_axis(raw, order[:, :m], axis=1)
    scale = bliss.playlist.scales_from_distances(near, m, "mean")
    H = bliss.playlist.Hubness
    h_raw = H.from_counts(np.bincount(order[:, :k].ravel(), minlength=n), k)
    h_scaled = H.from_counts(np.bincount(scaled_lists(Dm, scale, k).ravel(), minlength=n), k)
    print(f"raw: skewness {h_raw.skewness:.2f}, most-listed in {h_raw.counts.max()} lists, {h_raw.orphans().size} orphans; "
          f"scaled: {h_scaled.skewness:.2f}, {h_scaled.counts.max()}, {h_scaled.orphans().size}")
    assert h_raw.counts.sum() == h_scaled.counts.sum() == n * k
    assert h_scaled.skewness < 0.5 * h_raw.skewness
    assert h_scaled.orphans().size < 0.1 * h_raw.orphans().size
