"""The marshalling layer of the Python bindings, without a device and without the built library: _ffi.call
against a small fake library set as _ffi._lib, the numpy shaping helpers of _marshal.py on their edge cases, and the
metric-acceptance functions of playlist.py against the outcomes the code before _plain_metric gave, as literals."""
import ctypes as C

import numpy as np
import pytest


class FakeLib:
    """Stands in for the loaded library: every function records what it was given; `reader` may look through a pointer while
    the call is running; `rc` is what every status function returns."""

    def __init__(self, rc=0, reader=None):
        self.calls, self.rc, self.reader = [], rc, reader

    def __getattr__(self, name):
        if not name.startswith("blissgpu_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            if self.reader is not None:
                self.reader(*args)
            return self.rc

        return fn

    def blissgpu_last_error(self):
        return b"the fake library says no"

    def blissgpu_strerror(self, rc):
        return b"strerror"


@pytest.fixture
def ffi(bliss_host, monkeypatch):
    from bliss_rs_amd import _ffi

    lib = FakeLib()
    monkeypatch.setattr(_ffi, "_lib", lib)
    return _ffi, lib


@pytest.fixture(scope="module")
def bliss_host():
    import bliss_rs_amd  # noqa: F401  (the import shim; no library is loaded by it)

    return bliss_rs_amd


def test_a_void_pointer_argument_gets_the_arrays_own_address(ffi):
    _ffi, lib = ffi
    m = np.arange(12, dtype=np.float32).reshape(3, 4)
    assert _ffi.SIGNATURES["blissgpu_feature_weights"][1] == [C.c_uint32, C.c_void_p]
    assert _ffi.call("blissgpu_feature_weights", 2, m) is None
    (name, (version, p)), = lib.calls
    assert name == "blissgpu_feature_weights" and version == 2
    assert C.c_void_p(p).value == m.ctypes.data == m.__array_interface__["data"][0]  # no copy was made on the way


def test_a_typed_pointer_argument_gets_a_typed_pointer(ffi):
    _ffi, lib = ffi
    lengths, ranks = np.array([5, 6, 7], np.uint64), np.zeros(3, np.uint32)
    assert _ffi.SIGNATURES["blissgpu_shard_plan"][1][0] is _ffi._u64p
    _ffi.call("blissgpu_shard_plan", lengths, 3, 2, ranks)
    (_, (lp, n, world, rp)), = lib.calls
    assert isinstance(lp, _ffi._u64p) and isinstance(rp, _ffi._u32p) and (n, world) == (3, 2)
    assert [lp[i] for i in range(3)] == [5, 6, 7] and C.addressof(lp.contents) == lengths.ctypes.data
    # signed and unsigned words of one size are the same pointee to C: the int32 status words go to an int32_t *
    info, table = np.zeros(12, np.uint64), np.zeros((2, 4), np.uint64)
    _ffi.call("blissgpu_flac_index", np.zeros(8, np.uint8), 8, 0, info, table, 2, None)
    assert isinstance(lib.calls[-1][1][4], _ffi._u64p)


@pytest.mark.parametrize("what", ["transposed", "u32 for u64p", "i64 for i32p"])
def test_a_bad_array_raises_type_error_and_the_function_is_not_called(ffi, what):
    _ffi, lib = ffi
    if what == "transposed":
        bad = np.zeros((3, 4), np.float32).T
        assert not bad.flags.c_contiguous
        with pytest.raises(TypeError, match=r"blissgpu_feature_weights: argument 1 is not C-contiguous"):
            _ffi.call("blissgpu_feature_weights", 2, bad)
    elif what == "u32 for u64p":
        with pytest.raises(TypeError, match=r"blissgpu_shard_plan: argument 0 is uint32, the C argument points to uint64"):
            _ffi.call("blissgpu_shard_plan", np.zeros(3, np.uint32), 3, 2, np.zeros(3, np.uint32))
    else:
        assert _ffi.SIGNATURES["blissgpu_analyze"][1][4] is _ffi._i32p
        with pytest.raises(TypeError, match=r"blissgpu_analyze: argument 4 is int64, the C argument points to int32"):
            _ffi.call("blissgpu_analyze", np.zeros(9, np.float32), 9, 2, np.zeros(23, np.float32), np.zeros(1, np.int64))
    assert lib.calls == []


def test_none_scalars_and_ctypes_objects_pass_as_they_are(ffi):
    _ffi, lib = ffi
    out = C.c_uint32(0)
    ref = C.byref(out)
    h = C.c_void_p(1234)
    _ffi.call("blissgpu_map_plan", 1000, 0, ref)
    _ffi.call("blissgpu_ctx_set_stream", h, None)
    assert lib.calls[0][1][0] == 1000 and lib.calls[0][1][2] is ref
    assert lib.calls[1][1][0] is h and lib.calls[1][1][1] is None


def test_a_status_is_checked_and_a_value_is_returned(ffi, monkeypatch):
    _ffi, lib = ffi
    from bliss_rs_amd import playlist as P

    lib.rc = _ffi.ERR_OOM
    with pytest.raises(_ffi.BlissGpuError) as e:
        _ffi.call("blissgpu_ctx_synchronize", C.c_void_p(1))
    assert e.value.code == _ffi.ERR_OOM and "the fake library says no" in str(e.value)
    # the functions that return a value, a count among them, are not read as a status
    lib.rc = 7
    assert _ffi.call("blissgpu_resampled_len", 100, 44100) == 7 and _ffi.call("blissgpu_default_device_count") == 7
    assert _ffi.call_unchecked("blissgpu_ctx_synchronize", C.c_void_p(1)) == 7
    # playlist._call: ERR_NAN is the reference's panic, every other code stays what it is
    lib.rc = _ffi.ERR_NAN
    with pytest.raises(ValueError) as e:
        P._call("blissgpu_ctx_synchronize", C.c_void_p(1))
    assert str(e.value) == "NaN distance (noisy_float::n32 / argmin().unwrap() panic in the reference)"
    assert isinstance(e.value.__cause__, _ffi.BlissGpuError)
    lib.rc = _ffi.ERR_INVALID
    with pytest.raises(_ffi.BlissGpuError) as e:
        P._call("blissgpu_ctx_synchronize", C.c_void_p(1))
    assert e.value.code == _ffi.ERR_INVALID


def test_an_array_built_in_the_call_expression_is_alive_while_the_function_runs(ffi):
    _ffi, lib = ffi
    seen = []

    def reader(version, p):
        import gc

        gc.collect()
        junk = [np.full(12, -1.0, np.float32) for _ in range(64)]  # what would land on freed memory
        seen.append(np.ctypeslib.as_array(C.cast(C.c_void_p(p), C.POINTER(C.c_float)), (12,)).copy())
        del junk

    lib.reader = reader
    _ffi.call("blissgpu_feature_weights", 2, np.arange(12, dtype=np.float64).astype(np.float32) * np.float32(2.0))
    assert np.array_equal(seen[0], np.arange(12, dtype=np.float32) * 2)


def test_signed_idx(bliss_host):
    from bliss_rs_amd._marshal import signed_idx

    idx = np.array([[0, 0xFFFFFFFF, 0xFFFFFFFE], [7, 0xFFFFFFFF, 0xFFFFFFFF]], np.uint32)
    out = signed_idx(idx)
    assert out.dtype == np.int64 and out.tolist() == [[0, -1, 0xFFFFFFFE], [7, -1, -1]]
    assert idx[0, 1] == 0xFFFFFFFF  # the words themselves are left alone
    assert signed_idx(np.zeros((0, 3), np.uint32)).shape == (0, 3)


def test_skip_words(bliss_host):
    from bliss_rs_amd._marshal import skip_words

    out = skip_words([-1, 0, 4], 3, 5)
    assert out.dtype == np.uint32 and out.flags.c_contiguous and out.tolist() == [0xFFFFFFFF, 0, 4]
    with pytest.raises(ValueError, match=r"^skip entries must be candidate indices or -1$"):
        skip_words([-2, 0, 4], 3, 5)
    with pytest.raises(ValueError, match=r"^skip entries must be candidate indices or -1$"):
        skip_words([-1, 0, 5], 3, 5)  # n itself is no candidate
    with pytest.raises(ValueError, match=r"^skip needs one entry per query$"):
        skip_words([-1, 0], 3, 5)
    # the [G, 2] form of the journeys and the radios, with its own wording
    out = skip_words([[1, -1], [0, 2]], (2, 2), 3, "skip must be [G, 2]")
    assert out.shape == (2, 2) and out.tolist() == [[1, 0xFFFFFFFF], [0, 2]]
    with pytest.raises(ValueError, match=r"^skip must be \[G, 2\]$"):
        skip_words([1, -1, 0, 2], (2, 2), 3, "skip must be [G, 2]")
    with pytest.raises(ValueError, match=r"^skip entries must be candidate indices or -1$"):
        skip_words([0], 1, 0)  # no candidate at all


def test_metric_matrix(bliss_host):
    from bliss_rs_amd._marshal import metric_matrix

    eye = np.eye(3)
    # an entry point that leaves the check to the library: any m goes through as float32, whatever its shape
    assert metric_matrix("euclidean", None) is None and metric_matrix("mahalanobis", None) is None
    m = metric_matrix("mahalanobis", eye[:2])
    assert m.dtype == np.float32 and m.shape == (2, 3) and m.flags.c_contiguous
    f32 = np.eye(3, dtype=np.float32)
    assert metric_matrix("mahalanobis", f32) is f32  # no copy of what is right already
    # an entry point that checks on the host (d given)
    assert metric_matrix("mahalanobis", eye, 3).shape == (3, 3)
    with pytest.raises(ValueError, match=r"^mahalanobis needs m$"):
        metric_matrix("mahalanobis", None, 3)
    with pytest.raises(ValueError, match=r"^m must be \[d, d\]$"):
        metric_matrix("mahalanobis", eye[:2], 3)
    assert metric_matrix("euclidean", eye[:2], 3) is None and metric_matrix("cosine", None, 3) is None  # not looked at
    # one diagonal per group
    assert metric_matrix("diagonal", np.ones((4, 3)), 3, groups=4).shape == (4, 3)
    with pytest.raises(ValueError, match=r"^m must be \[G, d\]$"):
        metric_matrix("diagonal", np.ones((3, 3)), 3, groups=4)


def test_rows_f32_and_check_k_d(bliss_host):
    from bliss_rs_amd._marshal import check_k_d, rows_f32

    X = np.zeros((4, 3), np.float32)
    assert rows_f32(X) is X and rows_f32(X[0]).shape == (1, 3)
    for a in (X.astype(np.float64), np.asfortranarray(X), np.zeros((8, 3), np.float32)[::2]):
        r = rows_f32(a)
        assert r.dtype == np.float32 and r.flags.c_contiguous and r.shape == (4, 3)
    check_k_d(1, 1), check_k_d(1024, 64), check_k_d(3, 32, 32)
    for k, d, d_max, text in ((0, 23, 64, "k must be 1 .. 1024"), (1025, 23, 64, "k must be 1 .. 1024"), (3, 0, 64, "d must be 1 .. 64"),
                              (3, 65, 64, "d must be 1 .. 64"), (3, 33, 32, "d must be 1 .. 32"), (0, 0, 64, "k must be 1 .. 1024")):
        with pytest.raises(ValueError) as e:
            check_k_d(k, d, d_max)
        assert str(e.value) == text


# ---- the metric-acceptance functions: the outcomes of the code before _plain_metric, as literals ----
FOREST = "the isolation forest does not work for a single song (min(sample_size, seeds) < 2, src/playlist.rs:230-240): "
VARIANCE = "variance-based weights need a seed set of more than one song (variance_based_weight_matrix, src/playlist.rs:173-178): "
CALLABLE = ("metric builder must be euclidean_distance / cosine_distance / MahalanobisBuilder(m): distances are evaluated on the GPU, "
            "arbitrary callables are not supported")
# family -> (further arguments, the forest sentence, the variance sentence, the cosine refusal or None where cosine runs)
FAMILIES = {
    "_kmeans_metric": ((), "k-means assigns single songs to centres and needs a metric its means minimise",
                       "k-means has no seed set to take variances from; pass MahalanobisBuilder(m)",
                       "k-means needs a metric its means minimise: euclidean or mahalanobis, not cosine"),
    "_silhouette_metric": ((), "the silhouette compares single songs; a forest scores songs against a seed set",
                           "the silhouette has no seed set to take variances from; pass MahalanobisBuilder(m)",
                           "the silhouette needs the metric the groups are judged by: euclidean or mahalanobis, not cosine"),
    "_group_neighbours_metric": ((), "the group distances compare single songs; a forest scores songs against a seed set",
                                 "the group distances have no seed set to take variances from; pass MahalanobisBuilder(m)",
                                 "the group distances need a distance a nearest member is defined with: euclidean or mahalanobis, not cosine"),
    "_mst_metric": ((), "the spanning tree compares single songs; a forest scores songs against a seed set",
                    "the spanning tree has no seed set to take variances from; pass MahalanobisBuilder(m)",
                    "the spanning tree needs a distance whose bits order as integers: euclidean or mahalanobis, not cosine"),
    "_ward_metric": ((), "Ward clustering merges clusters by their centroids; a forest scores songs against a seed set",
                     "Ward clustering has no seed set to take variances from; pass MahalanobisBuilder(m)",
                     "Ward clustering needs a metric whose squares its centroids minimise: euclidean or mahalanobis, not cosine"),
    "_pam_metric": ((), "k-medoids compares single songs; a forest scores songs against a seed set",
                    "k-medoids has no seed set to take variances from; pass MahalanobisBuilder(m)", None),
    "_scaled_metric": (("local_scales",), "local_scales compares single songs; a forest scores songs against a seed set",
                       "local_scales has no seed set to take variances from; pass MahalanobisBuilder(m)", None),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_metric_acceptance_of_every_family(bliss_host, family):
    from bliss_rs_amd import playlist as P

    extra, forest, variance, cosine = FAMILIES[family]
    accept = getattr(P, family)

    def refused(builder, kind, text):
        with pytest.raises(kind) as e:
            accept(builder, *extra)
        assert type(e.value) is kind and str(e.value) == text

    assert accept(P.euclidean_distance, *extra) == ("euclidean", None)
    if cosine is None:
        assert accept(P.cosine_distance, *extra) == ("cosine", None)
    else:
        refused(P.cosine_distance, ValueError, cosine)
    builder = P.MahalanobisBuilder(np.eye(2, dtype=np.float32))
    metric, m = accept(builder, *extra)
    assert metric == "mahalanobis" and m is builder.m and m.tolist() == [[1.0, 0.0], [0.0, 1.0]]
    refused(P.ForestOptions(10, 8, None, 1, seed=1), ValueError, FOREST + forest)
    refused(P.VarianceWeights(), ValueError, VARIANCE + variance)
    refused(lambda a, b: 0.0, TypeError, CALLABLE)
