"""Device-free tests of the silhouette (blissgpu_silhouette / blissgpu_silhouette_device): the C ABI surface, the kernels' names
in the profile table, the argument checks that happen before the device is touched (for the host form the labels and the rows
too), and the host-side parts of the Python layer (Silhouette's aggregates, choose_k's tie rule and sample draw, the refusals of
metric builders the silhouette cannot run)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
OK, NO_DEVICE, INVALID = 0, 1, 2


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


def test_silhouette_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    lib = C.CDLL(bliss.LIB_PATH)
    for name in ("blissgpu_silhouette", "blissgpu_silhouette_device"):
        assert re.search(r"\bint\s+%s\s*\(" % name, flat), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name

    def types(name):
        return [re.sub(r"\s*\b\w+$", "", " ".join(a.split())).replace(" *", "*")
                for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, flat).group(1).split(",")]

    # (x, n, d, labels, k, metric, M, rows, q, col_groups, s, a, b, neighbour, sizes), the device form with the context in front
    want = ["const float*", "uint64_t", "uint32_t", "const uint32_t*", "uint32_t", "int", "const float*", "const uint32_t*", "uint64_t",
            "uint32_t", "float*", "double*", "double*", "uint32_t*", "uint32_t*"]
    assert types("blissgpu_silhouette") == want
    assert types("blissgpu_silhouette_device") == ["blissgpu_ctx*"] + want
    u64, u32 = C.c_uint64, C.c_uint32
    host = [_vp, u64, u32, _vp, u32, C.c_int, _vp, _vp, u64, u32, _vp, _vp, _vp, _vp, _vp]
    assert _ffi.SIGNATURES["blissgpu_silhouette"] == (C.c_int, host)
    assert _ffi.SIGNATURES["blissgpu_silhouette_device"] == (C.c_int, [_vp] + host)


def test_silhouette_kernels_are_in_the_profile_table(bliss):
    from bliss_rs_amd import _ffi

    L = _ffi.lib()
    names = [L.blissgpu_profile_kernel_name(k).decode() for k in range(L.blissgpu_profile_kernel_count())]
    assert len(set(names)) == len(names) and "" not in names
    src = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "kernels_silhouette.hip")).read()
    for name in ("silhouette_scan_kernel", "silhouette_finish_kernel"):
        assert names.count(name) == 1, name
        assert re.search(r"\bvoid\s+%s\s*\(" % name, src), name
    assert not [n for n in names if n.startswith("silhouette_") and not re.search(r"\bvoid\s+%s\s*\(" % n, src)]
    assert names[-2:] == ["group_forest_scan_kernel", "journey_step_kernel"]  # (older ids keep their places)


def _p(a):
    return None if a is None else a.ctypes.data


def _call(x, labels, k, n=None, d=None, metric=0, M=None, rows=None, q=None, col_groups=0, s=True, device=False, x_null=False,
          labels_null=False):
    from bliss_rs_amd import _ffi

    n = x.shape[0] if n is None else n
    d = x.shape[1] if d is None else d
    q = (0 if rows is None else rows.shape[0]) if q is None else q
    m = max(x.shape[0], 1 if rows is None else rows.shape[0], 1)
    sv, a, b = np.full(m, 7, np.float32), np.full(m, 7, np.float64), np.full(m, 7, np.float64)
    nb, sizes = np.full(m, 7, np.uint32), np.full(max(min(k, 70000), 1), 7, np.uint32)
    args = (None if x_null else _p(x), n, d, None if labels_null else _p(labels), k, metric, _p(M), _p(rows), q, col_groups,
            _p(sv) if s else None, _p(a), _p(b), _p(nb), _p(sizes))
    L = _ffi.lib()
    rc = L.blissgpu_silhouette_device(None, *args) if device else L.blissgpu_silhouette(*args)
    return rc, L.blissgpu_last_error(), sizes


def test_silhouette_arguments_are_checked_before_the_device(bliss):
    import torch

    rng = np.random.default_rng(0)
    X = rng.standard_normal((50, 23)).astype(np.float32)
    lab = (np.arange(50) % 4).astype(np.uint32)
    for device in (False, True):
        assert _call(X, lab, 0, device=device)[0] == INVALID
        assert _call(X, lab, 65536, device=device)[0] == INVALID
        assert _call(X, lab, 4, d=0, device=device)[0] == INVALID
        assert _call(np.zeros((50, 65), np.float32), lab, 4, device=device)[0] == INVALID
        rc, err, _ = _call(X, lab, 4, metric=1, device=device)
        assert rc == INVALID and b"cosine" in err
        assert _call(X, lab, 4, metric=3, device=device)[0] == INVALID
        assert _call(X, lab, 4, metric=-1, device=device)[0] == INVALID
        assert _call(X, lab, 4, metric=2, M=None, device=device)[0] == INVALID
        assert _call(X, lab, 4, n=0xFFFFFFFF, device=device)[0] == INVALID
        assert _call(X, lab, 4, x_null=True, device=device)[0] == INVALID
        assert _call(X, lab, 4, labels_null=True, device=device)[0] == INVALID
        assert _call(X, lab, 4, s=False, device=device)[0] == INVALID
    # the device form checks the scalars before it looks at its context ...
    rc, err, _ = _call(X, lab, 0, device=True)
    assert rc == INVALID and b"k must be" in err
    # ... and the context before anything else
    rc, err, _ = _call(X, lab, 4, device=True)
    assert rc == INVALID and b"ctx" in err
    # the host form's labels and rows are host memory: checked before the device is touched
    bad = lab.copy()
    bad[17] = 4
    rc, err, _ = _call(X, bad, 4)
    assert rc == INVALID and b"label" in err
    rc, err, _ = _call(X, np.full(50, 2, np.uint32), 4)
    assert rc == INVALID and b"two non-empty clusters" in err
    rows = np.array([3, 49, 50, 1], np.uint32)
    rc, err, _ = _call(X, lab, 4, rows=rows)
    assert rc == INVALID and b"rows" in err
    # no song: nothing for a device to do -- OK, every size zero; nothing to score is OK too
    rc, _, sizes = _call(X[:0], lab[:0], 4)
    assert rc == OK and not sizes[:4].any()
    assert _call(X, lab, 4, rows=np.zeros(0, np.uint32))[0] == OK
    # a valid call: BLISSGPU_ERR_NO_DEVICE without a GPU, BLISSGPU_OK with one
    want = OK if torch.cuda.is_available() else NO_DEVICE
    assert _call(X, lab, 4)[0] == want
    assert _call(X, lab, 4, rows=np.array([3, 49, 3, 1], np.uint32), col_groups=3)[0] == want


def _no_library(monkeypatch):
    from bliss_rs_amd import _ffi

    def boom():
        raise AssertionError("the library must not be reached")

    monkeypatch.setattr(_ffi, "lib", boom)


def test_silhouette_aggregates_are_fsum_means(bliss, monkeypatch):
    _no_library(monkeypatch)
    P = bliss.playlist
    values = np.array([1e-8, 1.0, -1.0, 0.25, 1e-8, 0.5, -0.125], np.float32)
    labels = [0, 2, 0, 2, 0, 4, 2]
    sil = P.Silhouette(values, np.zeros(7), np.ones(7), [2, 0, 2, 0, 2, 0, 0], [3, 0, 3, 0, 1], labels)
    f = [float(v) for v in values]
    assert sil.score == math.fsum(f) / 7
    assert sil.score != float(np.sum(values, dtype=np.float32)) / 7  # (the order-free sum is not the f32 one on this data)
    want = [math.fsum([f[0], f[2], f[4]]) / 3, None, math.fsum([f[1], f[3], f[6]]) / 3, None, f[5]]
    for c, w in enumerate(want):
        assert (np.isnan(sil.cluster_scores[c]) if w is None else sil.cluster_scores[c] == w), c
    assert sil.values.dtype == np.float32 and sil.a.dtype == np.float64 and sil.b.dtype == np.float64
    assert sil.neighbour.dtype == np.int64 and sil.sizes.dtype == np.int64 and sil.labels.tolist() == labels
    # a subset: clusters none of whose members was scored have no score
    sub = P.Silhouette(values[:2], np.zeros(2), np.ones(2), [2, 0], [3, 0, 3, 0, 1], [0, 2])
    assert sub.score == math.fsum(f[:2]) / 2 and np.isnan(sub.cluster_scores[[1, 3, 4]]).all()
    assert (sub.cluster_scores[0], sub.cluster_scores[2]) == (f[0], f[1])


def test_choose_k_tie_rule_and_sample_draw(bliss, monkeypatch):
    _no_library(monkeypatch)
    P = bliss.playlist
    assert P._best_k([2, 3, 4, 5], [0.1, 0.7, 0.7, 0.3]) == 3
    assert P._best_k([5, 4, 3, 2], [0.3, 0.7, 0.7, 0.1]) == 3  # the lower k, not the earlier one
    assert P._best_k([7], [-0.5]) == 7
    assert P._best_k([2, 9], [0.5, 0.5000001]) == 9
    sel = P.KSelection(range(2, 5), [0.25, 0.5, 0.125], 3, "the clustering")
    assert (sel.ks, sel.scores, sel.best_k, sel.clustering) == ([2, 3, 4], [0.25, 0.5, 0.125], 3, "the clustering")
    got = P._sample_rows(1000, 37, 9)
    want = np.sort(np.random.Generator(np.random.PCG64(9)).choice(1000, 37, replace=False))
    assert got.tolist() == want.tolist() and len(set(got.tolist())) == 37
    assert P._sample_rows(1000, 37, 9).tolist() == got.tolist() and P._sample_rows(1000, 37, 10).tolist() != got.tolist()
    assert P._sample_rows(1000, None, 9) is None and P._sample_rows(1000, 1000, 9) is None and P._sample_rows(10, 50, 9) is None
    with pytest.raises(ValueError):
        P._sample_rows(1000, 0, 9)
    with pytest.raises(ValueError):
        P.choose_k(np.zeros((5, 3), np.float32), [])
    with pytest.raises(ValueError):
        P.choose_k(np.zeros((0, 3), np.float32), [2])


def test_unsupported_metric_builders_are_refused(bliss, monkeypatch, tmp_path):
    _no_library(monkeypatch)
    P = bliss.playlist
    X = np.zeros((6, 23), np.float32)
    labels = [0, 1, 0, 1, 0, 1]
    db = str(tmp_path / "never_read.db")  # (refused before the database is opened: the file does not exist)
    refused = [(P.ForestOptions(10, 4, None, 1, seed=1), ValueError), (P.VarianceWeights(), ValueError), (P.cosine_distance, ValueError),
               ("cosine", ValueError), (lambda a, b: 0.0, TypeError)]
    for builder, err in refused:
        with pytest.raises(err):
            P.silhouette(X, labels, metric_builder=builder)
        with pytest.raises(err):
            P.choose_k(X, [2, 3], metric_builder=builder)
        with pytest.raises(err):
            bliss.library.choose_clusters(db, [2, 3], metric_builder=builder)
        with pytest.raises(err):
            bliss.library.label_silhouette(db, "genre", metric_builder=builder)
    assert not os.path.exists(db)
    with pytest.raises(ValueError):
        bliss.library.label_silhouette(db, "title")
    assert not os.path.exists(db)
    with pytest.raises(ValueError):
        P.silhouette(X, labels[:5])
    with pytest.raises(ValueError):
        P.silhouette(X, [0, 1, 0, 1, 0, -1])
    with pytest.raises(ValueError):
        P.silhouette(X[:0], [])
