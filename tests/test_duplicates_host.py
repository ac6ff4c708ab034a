"""Device-free tests of the duplicate search (blissgpu_duplicate_groups / blissgpu_duplicate_groups_device): the C ABI
surface, the argument checks that happen before the device is touched, the pure helper playlist.groups_from_labels and the
checks of playlist.duplicate_labels / duplicate_groups that happen before the library is reached."""
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


def test_duplicates_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    lib = C.CDLL(bliss.LIB_PATH)
    for name in ("blissgpu_duplicate_groups", "blissgpu_duplicate_groups_device"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name
    u64, u32 = C.c_uint64, C.c_uint32
    # (x, n, d, meta, metric, M, threshold, label, n_pairs, pairs, pair_dist, max_pairs), the device form with the context in front
    host = [_vp, u64, u32, _vp, C.c_int, _vp, C.c_float, _vp, C.POINTER(u64), _vp, _vp, u64]
    dev = [_vp, _vp, u64, u32, _vp, C.c_int, _vp, C.c_float, _vp, _vp, _vp, _vp, u64]
    assert _ffi.SIGNATURES["blissgpu_duplicate_groups"] == (C.c_int, host)
    assert _ffi.SIGNATURES["blissgpu_duplicate_groups_device"] == (C.c_int, dev)
    # the kernels appear in the profiling table like the others
    names = [lib_name.decode() for lib_name in (_name(_ffi, k) for k in range(_ffi.lib().blissgpu_profile_kernel_count()))]
    assert "dup_join_kernel" in names and "dup_flatten_kernel" in names


def _name(_ffi, k):
    return _ffi.lib().blissgpu_profile_kernel_name(k)


def _call(bliss, X, n=None, d=None, meta=None, metric=0, M=None, thr=0.05, label=True, n_pairs=True, device_form=False):
    from bliss_rs_amd import _ffi

    n = X.shape[0] if n is None else n
    d = X.shape[1] if d is None else d
    lab = np.zeros(max(X.shape[0], 1), np.uint32)
    np_out = C.c_uint64(77)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    if device_form:  # a NULL context: the argument checks come first, as for the k-nearest search
        return _ffi.lib().blissgpu_duplicate_groups_device(None, p(X), n, d, p(meta), metric, p(M), thr, p(lab) if label else None,
                                                           C.addressof(np_out) if n_pairs else None, None, None, 0)
    return _ffi.lib().blissgpu_duplicate_groups(p(X), n, d, p(meta), metric, p(M), thr, p(lab) if label else None,
                                                C.byref(np_out) if n_pairs else None, None, None, 0)


@pytest.mark.parametrize("device_form", (False, True))
def test_duplicates_arguments_are_checked_before_the_device(bliss, device_form):
    import torch
    from bliss_rs_amd import _ffi

    rng = np.random.default_rng(0)
    X = rng.standard_normal((50, 23)).astype(np.float32)
    call = lambda *a, **k: _call(bliss, *a, device_form=device_form, **k)  # noqa: E731
    assert call(np.zeros((50, 65), np.float32)) == INVALID  # d > 64
    assert call(X, d=0) == INVALID
    assert call(X, metric=2, M=None) == INVALID  # Mahalanobis without M
    assert b"mahalanobis" in _ffi.lib().blissgpu_last_error()
    assert call(X, metric=3) == INVALID
    assert call(X, metric=-1) == INVALID
    assert call(X, n=0xFFFFFFFF) == INVALID  # n < 2^32 - 1
    assert call(X, thr=float("nan")) == INVALID
    assert b"threshold" in _ffi.lib().blissgpu_last_error()
    assert call(X, n_pairs=False) == INVALID
    assert call(X, label=False) == INVALID
    if device_form:
        assert call(X) == INVALID  # everything else is fine: only now the NULL context is looked at
        assert b"ctx" in _ffi.lib().blissgpu_last_error()
    else:
        # a valid call: BLISSGPU_ERR_NO_DEVICE without a GPU, BLISSGPU_OK with one
        assert call(X) == (0 if torch.cuda.is_available() else 1)
        assert call(X, thr=0.0) == (0 if torch.cuda.is_available() else 1)


def test_duplicates_of_nothing_need_no_device(bliss):
    from bliss_rs_amd import _ffi

    np_out = C.c_uint64(77)
    assert _ffi.lib().blissgpu_duplicate_groups(None, 0, 23, None, 0, None, 0.05, None, C.byref(np_out), None, None, 0) == 0
    assert np_out.value == 0


def test_groups_from_labels(bliss):
    g = bliss.playlist.groups_from_labels
    assert g([]) == []
    assert g([0]) == []
    assert g([0, 1, 2, 3]) == []
    got = g([0, 1, 0, 3, 1, 0, 6])
    assert [x.tolist() for x in got] == [[0, 2, 5], [1, 4]]
    assert all(x.dtype == np.int64 for x in got)
    got = g(np.array([0, 0, 2, 2, 2, 5, 0], np.uint32))
    assert [x.tolist() for x in got] == [[0, 1, 6], [2, 3, 4]]
    # all in one component
    assert [x.tolist() for x in g(np.zeros(5, np.int64))] == [[0, 1, 2, 3, 4]]
    # ordered by the smallest member, whatever the order of first appearance of a label's rows
    got = g([0, 1, 2, 1, 0])
    assert [x.tolist() for x in got] == [[0, 4], [1, 3]]


def test_duplicate_groups_refuses_a_forest(bliss):
    V2 = bliss.FeaturesVersion.Version2
    songs = [bliss.Song(path=f"/m/{i}.flac", analysis=bliss.Analysis(np.full(23, i, np.float32), V2), features_version=V2)
             for i in range(3)]
    opts = bliss.playlist.ForestOptions(n_trees=10, sample_size=4, max_tree_depth=None, extension_level=1, seed=1)
    with pytest.raises(ValueError):
        bliss.playlist.duplicate_groups(songs, metric_builder=opts)
    with pytest.raises(ValueError):
        bliss.library.duplicate_songs(":memory:", metric_builder=opts)
    assert bliss.playlist.duplicate_groups([]) == []


def test_duplicate_labels_checks_before_the_library(bliss, monkeypatch):
    from bliss_rs_amd import _ffi

    def boom():
        raise AssertionError("the library must not be reached")

    monkeypatch.setattr(_ffi, "lib", boom)
    X = np.zeros((10, 23), np.float32)
    dl = bliss.playlist.duplicate_labels
    with pytest.raises(ValueError):
        dl(np.zeros(23, np.float32))  # not a matrix
    with pytest.raises(ValueError):
        dl(np.zeros((4, 65), np.float32))
    with pytest.raises(ValueError):
        dl(X, meta=np.zeros(9, np.uint32))  # one key per row
    with pytest.raises(ValueError):
        dl(X, threshold=float("nan"))
    with pytest.raises(ValueError):
        dl(X, metric="mahalanobis")  # needs m
    with pytest.raises(ValueError):
        dl(X, metric="mahalanobis", m=np.eye(20, dtype=np.float32))
    with pytest.raises(ValueError):
        dl(X, metric="manhattan")
