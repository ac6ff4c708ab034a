"""Device-free tests of the k-nearest search (blissgpu_knn / blissgpu_knn_device): the C ABI surface, the argument checks
that happen before the device is touched, and the checks of playlist.nearest_order that happen before the library is."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


def test_knn_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    m = re.search(r"#define\s+BLISSGPU_KNN_MAX_K\s+(\d+)u?\b", header)
    assert m and int(m.group(1)) >= 1024
    lib = C.CDLL(bliss.LIB_PATH)
    for name in ("blissgpu_knn", "blissgpu_knn_device"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name
    u64, u32 = C.c_uint64, C.c_uint32
    # (queries, q, cand, n, d, metric, M, skip, k, idx, dist), the device form with the context in front
    host = [_vp, u64, _vp, u64, u32, C.c_int, _vp, _vp, u32, _vp, _vp]
    assert _ffi.SIGNATURES["blissgpu_knn"] == (C.c_int, host)
    assert _ffi.SIGNATURES["blissgpu_knn_device"] == (C.c_int, [_vp] + host)


def _call(bliss, Q, X, k, d=None, metric=0, M=None, skip=None):
    from bliss_rs_amd import _ffi

    q, n = Q.shape[0], X.shape[0]
    d = Q.shape[1] if d is None else d
    idx, dist = np.zeros((q, max(k, 1)), np.uint32), np.zeros((q, max(k, 1)), np.float32)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return _ffi.lib().blissgpu_knn(p(Q), q, p(X), n, d, metric, p(M), p(skip), k, p(idx), p(dist))


def test_knn_arguments_are_checked_before_the_device(bliss):
    import torch

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    max_k = int(re.search(r"#define\s+BLISSGPU_KNN_MAX_K\s+(\d+)", header).group(1))
    rng = np.random.default_rng(0)
    X = rng.standard_normal((50, 23)).astype(np.float32)
    Q = X[:4].copy()
    wide = np.zeros((4, 65), np.float32)
    INVALID = 2
    assert _call(bliss, Q, X, 0) == INVALID
    assert _call(bliss, Q, X, max_k + 1) == INVALID
    assert _call(bliss, wide, np.zeros((50, 65), np.float32), 3, d=65) == INVALID
    assert _call(bliss, Q, X, 3, metric=2, M=None) == INVALID
    assert _call(bliss, Q, X, 3, metric=3) == INVALID
    skip = np.full(4, 0xFFFFFFFF, np.uint32)
    skip[0] = X.shape[0]
    assert _call(bliss, Q, X, 3, skip=skip) == INVALID
    from bliss_rs_amd import _ffi

    assert b"skip" in _ffi.lib().blissgpu_last_error()
    # a valid call: BLISSGPU_ERR_NO_DEVICE without a GPU, BLISSGPU_OK with one
    skip[0] = 0
    assert _call(bliss, Q, X, 3, skip=skip) == (0 if torch.cuda.is_available() else 1)


def test_nearest_order_checks_before_the_library(bliss, monkeypatch):
    from bliss_rs_amd import _ffi

    def boom():
        raise AssertionError("the library must not be reached")

    monkeypatch.setattr(_ffi, "lib", boom)
    X = np.zeros((10, 23), np.float32)
    with pytest.raises(ValueError):
        bliss.playlist.nearest_order(np.zeros((2, 20), np.float32), X, 3)
    with pytest.raises(ValueError):
        bliss.playlist.nearest_order(X[:2], X, 0)
    with pytest.raises(ValueError):
        bliss.playlist.nearest_order(X[:2], X, -1)
    with pytest.raises(ValueError):
        bliss.playlist.nearest_order(X[:2], X, 3, skip=[0, 1, 2])
