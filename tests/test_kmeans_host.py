"""Device-free tests of k-means (blissgpu_kmeans / blissgpu_kmeans_device): the C ABI surface, the kernels' names in the
profile table, the argument checks that happen before the device is touched, and the host-side parts of the Python layer (the
"sample" initialisation, Clustering, the refusals of metric builders k-means cannot run)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
INVALID = 2


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


def test_kmeans_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    m = re.search(r"#define\s+BLISSGPU_KMEANS_MAX_K\s+(\d+)u?\b", header)
    assert m and int(m.group(1)) == 65535 == _ffi.KMEANS_MAX_K
    lib = C.CDLL(bliss.LIB_PATH)
    for name in ("blissgpu_kmeans", "blissgpu_kmeans_device", "blissgpu_debug_kmeans_stats"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name
    u64, u32 = C.c_uint64, C.c_uint32
    # (x, n, d, init, k, metric, M, max_iter, labels, dist, centroids, sizes, n_iter, converged), the device form with the context in front
    host = [_vp, u64, u32, _vp, u32, C.c_int, _vp, u32, _vp, _vp, _vp, _vp, C.POINTER(u32), C.POINTER(C.c_int32)]
    assert _ffi.SIGNATURES["blissgpu_kmeans"] == (C.c_int, host)
    assert _ffi.SIGNATURES["blissgpu_kmeans_device"] == (C.c_int, [_vp] + host)


def test_kmeans_kernels_are_in_the_profile_table(bliss):
    from bliss_rs_amd import _ffi

    L = _ffi.lib()
    names = [L.blissgpu_profile_kernel_name(k).decode() for k in range(L.blissgpu_profile_kernel_count())]
    assert len(set(names)) == len(names) and "" not in names
    for name in ("kmeans_assign_kernel", "kmeans_hist_kernel", "kmeans_scan_tiles_kernel", "kmeans_scan_add_kernel",
                 "kmeans_scatter_kernel", "kmeans_select_kernel", "segment_mean_kernel"):
        assert name in names, name
    # every name is a kernel of the sources
    src = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "kernels_kmeans.hip")).read()
    for name in names:
        if name.startswith("kmeans_"):
            assert re.search(r"\bvoid\s+%s\s*\(" % name, src), name


def _call(x, init, n=None, d=None, k=None, metric=0, M=None, max_iter=3, labels=True, cent=True, n_iter=True, conv=True):
    from bliss_rs_amd import _ffi

    n = x.shape[0] if n is None else n
    d = x.shape[1] if d is None else d
    k = init.shape[0] if k is None else k
    lab, dist = np.zeros(max(x.shape[0], 1), np.uint32), np.zeros(max(x.shape[0], 1), np.float32)
    ce, sz = np.zeros((max(init.shape[0], 1), x.shape[1]), np.float32), np.zeros(max(init.shape[0], 1), np.uint32)
    it, cv = C.c_uint32(7), C.c_int32(7)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = _ffi.lib().blissgpu_kmeans(p(x), n, d, p(init), k, metric, p(M), max_iter, p(lab) if labels else None, p(dist),
                                    p(ce) if cent else None, p(sz), C.byref(it) if n_iter else None, C.byref(cv) if conv else None)
    return rc, lab, ce, sz, it.value, cv.value


def test_kmeans_arguments_are_checked_before_the_device(bliss):
    import torch

    from bliss_rs_amd import _ffi

    rng = np.random.default_rng(0)
    X = rng.standard_normal((50, 23)).astype(np.float32)
    C0 = X[:4].copy()
    assert _call(X, C0, k=0)[0] == INVALID
    assert _call(X, C0, k=65536)[0] == INVALID
    assert _call(X, C0, d=0)[0] == INVALID
    assert _call(np.zeros((50, 65), np.float32), np.zeros((4, 65), np.float32))[0] == INVALID
    assert _call(X, C0, metric=1)[0] == INVALID  # cosine
    assert b"cosine" in _ffi.lib().blissgpu_last_error()
    assert _call(X, C0, metric=3)[0] == INVALID
    assert _call(X, C0, metric=-1)[0] == INVALID
    assert _call(X, C0, metric=2, M=None)[0] == INVALID
    assert _call(X, C0, n=0xFFFFFFFF)[0] == INVALID
    for kw in ({"labels": False}, {"cent": False}, {"n_iter": False}, {"conv": False}):
        assert _call(X, C0, **kw)[0] == INVALID, kw
    p = lambda a: a.ctypes.data  # noqa: E731
    it, cv = C.c_uint32(), C.c_int32()
    L = _ffi.lib()
    lab, ce = np.zeros(50, np.uint32), np.zeros((4, 23), np.float32)
    assert L.blissgpu_kmeans(None, 50, 23, p(C0), 4, 0, None, 3, p(lab), None, p(ce), None, C.byref(it), C.byref(cv)) == INVALID
    assert L.blissgpu_kmeans(p(X), 50, 23, None, 4, 0, None, 3, p(lab), None, p(ce), None, C.byref(it), C.byref(cv)) == INVALID
    # the device form checks the same before it looks at its context
    assert L.blissgpu_kmeans_device(None, p(X), 50, 23, p(C0), 0, 0, None, 3, p(lab), None, p(ce), None, C.byref(it), C.byref(cv)) == INVALID
    assert b"k must be" in L.blissgpu_last_error()
    assert L.blissgpu_kmeans_device(None, p(X), 50, 23, p(C0), 4, 0, None, 3, p(lab), None, p(ce), None, C.byref(it), C.byref(cv)) == INVALID
    assert b"ctx" in L.blissgpu_last_error()
    # no song: nothing for a device to do -- OK, no update, converged, the centres as given, every size zero
    rc, _, ce, sz, n_iter, conv = _call(X[:0], C0)
    assert (rc, n_iter, conv) == (0, 0, 1) and ce.tobytes() == C0.tobytes() and not sz.any()
    # a valid call: BLISSGPU_ERR_NO_DEVICE without a GPU, BLISSGPU_OK with one
    assert _call(X, C0)[0] == (0 if torch.cuda.is_available() else 1)


def test_sample_init_is_host_only(bliss, monkeypatch):
    from bliss_rs_amd import _ffi

    def boom():
        raise AssertionError("the library must not be reached")

    monkeypatch.setattr(_ffi, "lib", boom)
    P = bliss.playlist
    X = np.arange(40 * 3, dtype=np.float32).reshape(40, 3)
    got = P.kmeans_init(X, 6, seed=9, method="sample")
    want = np.sort(np.random.Generator(np.random.PCG64(9)).choice(40, 6, replace=False))
    assert got.tobytes() == X[want].tobytes()
    assert P.kmeans_init(X, 6, 9, "sample").tobytes() == got.tobytes()
    assert P.kmeans_init(X, 40, 1, "sample").tobytes() == X.tobytes()  # every row, sorted
    for bad in (0, 41, -1):
        with pytest.raises(ValueError):
            P.kmeans_init(X, bad, 0, "sample")
        with pytest.raises(ValueError):
            P.kmeans_init(X, bad, 0)
    with pytest.raises(ValueError):
        P.kmeans_init(X, 3, 0, "random")


def test_clustering_members_and_inertia(bliss):
    P = bliss.playlist
    labels = [1, 0, 1, 1, 0, 1, 2]
    dist = np.array([0.5, 0.25, 0.125, 0.5, -0.0, 0.0, 3.0], np.float32)
    cl = P.Clustering(labels, dist, np.zeros((4, 2), np.float32), [2, 4, 1, 0], 3, True)
    assert cl.members(1).tolist() == [5, 2, 0, 3]  # by distance, equal distances by index
    assert cl.members(0).tolist() == [4, 1]
    assert cl.members(2).tolist() == [6] and cl.members(3).tolist() == []
    assert cl.inertia == 0.25 + 0.0625 + 0.015625 + 0.25 + 9.0
    assert cl.labels.dtype == np.int64 and cl.sizes.dtype == np.int64 and cl.distances.dtype == np.float32
    assert (cl.n_iter, cl.converged) == (3, True)
    big = P.Clustering([0, 0], np.array([3e-30, 2e30], np.float32), np.zeros((1, 1)), [2], 0, False)
    assert big.inertia == float(np.float64(np.float32(3e-30)) ** 2 + np.float64(np.float32(2e30)) ** 2)  # f64: no overflow, no underflow


def test_unsupported_metric_builders_are_refused(bliss, monkeypatch, tmp_path):
    from bliss_rs_amd import _ffi

    def boom():
        raise AssertionError("the library must not be reached")

    monkeypatch.setattr(_ffi, "lib", boom)
    P = bliss.playlist
    V2 = bliss.FeaturesVersion.Version2
    songs = [bliss.Song(path=f"/m/{i}.flac", analysis=bliss.Analysis(np.full(23, i, np.float32), V2), features_version=V2) for i in range(5)]
    db = str(tmp_path / "never_read.db")  # (refused before the database is opened: the file does not exist)
    refused = [(P.ForestOptions(10, 4, None, 1, seed=1), ValueError), (P.VarianceWeights(), ValueError), (P.cosine_distance, ValueError),
               ("cosine", ValueError), (lambda a, b: 0.0, TypeError)]
    for builder, err in refused:
        with pytest.raises(err):
            P.cluster_songs(songs, 2, metric_builder=builder)
        with pytest.raises(err):
            bliss.library.cluster_songs(db, 2, metric_builder=builder)
    assert not os.path.exists(db)
    with pytest.raises(ValueError):
        P.kmeans(np.zeros((5, 3), np.float32), np.zeros((2, 3), np.float32), metric="cosine")
    with pytest.raises(ValueError):
        P.kmeans(np.zeros((5, 3), np.float32), np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError):
        P.kmeans(np.zeros((5, 3), np.float32), np.zeros((2, 3), np.float32), max_iter=-1)
    with pytest.raises(ValueError):
        P.cluster_songs([], 2)
