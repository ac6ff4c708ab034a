"""Device-free tests of triplet metric learning (blissgpu_triplet_step / blissgpu_learn_metric): the C ABI surface, the kernels'
names in the profile table, the argument checks that happen before the device is touched, the host parts of the Python layer
(triplets_from_labels, the training_triplet table) and metric_learn.hpp -- the loop around the device's gradient -- as a
stand-alone program fed recorded gradients, plain and under AddressSanitizer + UBSan, against the restatement below.

The restatement (ref_learn) is the header's contract in numpy float64: one rounding per multiply and per add, every sum
ascending from 0.0 -- a Python loop over the summation index with independent entries side by side, np.cumsum for the one
row-major sum.  tests/test_gpu_metric.py replays blissgpu_learn_metric with it on the device's own gradients."""
import ctypes as C
import os
import re
import sqlite3
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_metric_learn.cpp")
SAN_CXX = "/opt/rocm/lib/llvm/bin/clang++"
_vp = C.c_void_p
INVALID, NAN_CODE = 2, 5
DIAGONAL, FULL = 0, 1
CONVERGED, MAX_ITER, DIVERGED = 0, 1, 2


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


# ---- the restatement -------------------------------------------------------------------------------------------------------
def seq_sum(a) -> float:
    """0.0 + a[0] + a[1] + ... in that order"""
    a = np.asarray(a, np.float64).reshape(-1)
    return float(np.cumsum(a)[-1]) + 0.0 if a.size else 0.0


class RefLearner:
    def __init__(self, form, d, init, T, lr, reg):
        self.form, self.d, self.T, self.lr, self.reg = form, d, T, np.float64(lr), np.float64(reg)
        init = np.ones(d, np.float32) if init is None else np.asarray(init, np.float32)
        self.M0 = np.diag(init).astype(np.float32)
        self.w = init.astype(np.float64)
        self.L = np.diag(np.sqrt(init.astype(np.float64)))

    def build_m(self):
        d = self.d
        if self.form == DIAGONAL:
            return np.diag(self.w.astype(np.float32))
        S = np.zeros((d, d), np.float64)
        for k in range(d):
            S = S + np.outer(self.L[k], self.L[k])  # S[i][j] += L[k][i] * L[k][j]: x * y == y * x, so S is symmetric
        return S.astype(np.float32)

    def objective(self, M, loss):
        diff = M.astype(np.float64) - self.M0.astype(np.float64)
        fit = np.float64(loss) / (np.float64(2.0) * np.float64(self.T)) if self.T else np.float64(0.0)
        return float(fit + self.reg * np.float64(seq_sum(diff * diff)))

    def update(self, M, G):
        d = self.d
        diff = M.astype(np.float64) - self.M0.astype(np.float64)
        fit = np.asarray(G, np.float64) / (np.float64(2.0) * np.float64(self.T)) if self.T else np.zeros((d, d))
        Gt = fit + (np.float64(2.0) * self.reg) * diff
        if self.form == DIAGONAL:
            v = self.w - self.lr * np.diag(Gt)
            self.w = np.where(v > 0.0, v, 0.0)
            return
        P = np.zeros((d, d), np.float64)
        for k in range(d):
            P = P + np.outer(self.L[:, k], Gt[k])  # P[i][j] += L[i][k] * Gt[k][j]
        self.L = self.L - (np.float64(2.0) * self.lr) * P


def ref_learn(form, d, init, T, lr, reg, max_iter, step):
    """step(M float32[d, d]) -> (rc, loss, active, G).  -> dict of the loop's outputs, and `seen`: every M_t a step got."""
    with np.errstate(all="ignore"):
        s = RefLearner(form, d, init, T, lr, reg)
        best, best_obj, best_m = None, None, s.M0.copy()
        obj, active, seen = [], [], []
        t = 0
        while True:
            M = s.build_m()
            rc, loss, act, G, o = NAN_CODE, 0.0, 0, None, float("nan")
            if np.isfinite(M).all():
                seen.append(M.copy())
                rc, loss, act, G = step(M)
            if rc and not (rc == NAN_CODE and t > 0):
                return {"rc": rc, "seen": seen}
            if not rc:
                o = s.objective(M, loss)
            obj.append(o)
            active.append(0 if rc else int(act))
            if not np.isfinite(o):
                status = DIVERGED
                break
            if best is None or o < best_obj:
                best, best_obj, best_m = t, o, M.copy()
            if act == 0:
                status = CONVERGED
                break
            if t == max_iter:
                status = MAX_ITER
                break
            s.update(M, G)
            t += 1
        return {"rc": 0, "M": best_m, "obj": np.asarray(obj, np.float64), "active": np.asarray(active, np.int64), "n_iter": t,
                "best_iter": best or 0, "status": status, "seen": seen}


def f64_bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def f32_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
NAMES = ("blissgpu_triplet_step", "blissgpu_triplet_step_device", "blissgpu_learn_metric", "blissgpu_learn_metric_device",
         "blissgpu_debug_metric_stats")


def test_metric_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    for macro, value in (("METRIC_FORM_DIAGONAL", _ffi.METRIC_FORM_DIAGONAL), ("METRIC_FORM_FULL", _ffi.METRIC_FORM_FULL),
                         ("LEARN_CONVERGED", _ffi.LEARN_CONVERGED), ("LEARN_MAX_ITER", _ffi.LEARN_MAX_ITER),
                         ("LEARN_DIVERGED", _ffi.LEARN_DIVERGED)):
        m = re.search(r"#define\s+BLISSGPU_%s\s+(\d+)\b" % macro, header)
        assert m and int(m.group(1)) == value, macro
    lib = C.CDLL(bliss.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name
    u64, u32, f64 = C.c_uint64, C.c_uint32, C.c_double
    # (x, n, d, triplets, T, M, margin, flags, n_active, loss, G), the device form with the context in front
    step = [_vp, u64, u32, _vp, u64, _vp, f64, _vp, C.POINTER(u64), C.POINTER(f64), _vp]
    assert _ffi.SIGNATURES["blissgpu_triplet_step"] == (C.c_int, step)
    assert _ffi.SIGNATURES["blissgpu_triplet_step_device"] == (C.c_int, [_vp] + step)
    # (x, n, d, triplets, T, form, init, margin, lr, reg, max_iter, M, obj, active, n_iter, best_iter, status)
    learn = [_vp, u64, u32, _vp, u64, C.c_int, _vp, f64, f64, f64, u32, _vp, _vp, _vp, C.POINTER(u32), C.POINTER(u32),
             C.POINTER(C.c_int32)]
    assert _ffi.SIGNATURES["blissgpu_learn_metric"] == (C.c_int, learn)
    assert _ffi.SIGNATURES["blissgpu_learn_metric_device"] == (C.c_int, [_vp] + learn)
    # the header's argument lists say the same
    flat = re.sub(r"\s+", " ", header)
    types = lambda name: [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*")  # noqa: E731
                          for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, flat).group(1).split(",")]
    want = ["const float*", "uint64_t", "uint32_t", "const uint32_t*", "uint64_t", "const float*", "double", "uint8_t*", "uint64_t*",
            "double*", "double*"]
    assert types("blissgpu_triplet_step") == want and types("blissgpu_triplet_step_device") == ["blissgpu_ctx*"] + want
    # the header cites what the feature answers
    assert "training_triplet" in header and "a way to learn a metric with a user survey" in header


def test_metric_kernels_are_in_the_profile_table(bliss):
    from bliss_rs_amd import _ffi

    L = _ffi.lib()
    names = [L.blissgpu_profile_kernel_name(k).decode() for k in range(L.blissgpu_profile_kernel_count())]
    assert len(set(names)) == len(names) and "" not in names
    src = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "kernels_metric.hip")).read()
    for name in ("triplet_step_kernel", "triplet_reduce_kernel"):
        assert names.count(name) == 1, name
        assert re.search(r"\bvoid\s+%s\s*\(" % name, src), name
    # the translation unit keeps every product and sum of the hinges apart
    mk = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "Makefile")).read()
    assert re.search(r"^[^\n#]*\bkernels_metric\.o\b[^\n]*: EXTRA := \$\(NOCONTRACT\)", mk, flags=re.M)
    assert "atomic" not in re.sub(r"//[^\n]*", "", src)  # no atomics, floating-point or other


def _step(x, tr, n=None, d=None, T=None, M=None, margin=0.0, outs=(True, True, True), device_form=False):
    from bliss_rs_amd import _ffi

    n = x.shape[0] if n is None else n
    d = x.shape[1] if d is None else d
    T = tr.shape[0] if T is None else T
    G = np.full((64, 64), 7.0)
    na, loss = C.c_uint64(7), C.c_double(7.0)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    args = [p(x), n, d, p(tr), T, p(M), margin, None, C.byref(na) if outs[0] else None, C.byref(loss) if outs[1] else None,
            p(G) if outs[2] else None]
    L = _ffi.lib()
    rc = L.blissgpu_triplet_step_device(None, *args) if device_form else L.blissgpu_triplet_step(*args)
    return rc, na.value, loss.value, G


def _learn(x, tr, d=None, form=FULL, init=None, margin=0.1, lr=1.0, reg=0.0, max_iter=3, outs=(True, True, True, True),
           device_form=False):
    from bliss_rs_amd import _ffi

    d = x.shape[1] if d is None else d
    M, obj, act = np.zeros((64, 64), np.float32), np.zeros(max_iter + 1), np.zeros(max_iter + 1, np.uint64)
    it, best, st = C.c_uint32(7), C.c_uint32(7), C.c_int32(7)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    args = [p(x), x.shape[0], d, p(tr), tr.shape[0], form, p(init), margin, lr, reg, max_iter, p(M) if outs[0] else None, p(obj),
            p(act), C.byref(it) if outs[1] else None, C.byref(best) if outs[2] else None, C.byref(st) if outs[3] else None]
    L = _ffi.lib()
    rc = L.blissgpu_learn_metric_device(None, *args) if device_form else L.blissgpu_learn_metric(*args)
    return rc, M, obj, act, it.value, best.value, st.value


def test_metric_arguments_are_checked_before_the_device(bliss):
    import torch

    from bliss_rs_amd import _ffi

    L = _ffi.lib()
    rng = np.random.default_rng(0)
    X = rng.standard_normal((50, 23)).astype(np.float32)
    tr = rng.integers(0, 50, (40, 3)).astype(np.uint32)
    wide = np.zeros((50, 65), np.float32)
    for dev in (False, True):
        assert _step(wide, tr, device_form=dev)[0] == INVALID and b"d must be" in L.blissgpu_last_error()
        assert _step(X, tr, d=0, device_form=dev)[0] == INVALID
        assert _step(X, tr, margin=-1e-300, device_form=dev)[0] == INVALID and b"margin" in L.blissgpu_last_error()
        assert _step(X, tr, margin=float("nan"), device_form=dev)[0] == INVALID
        assert _step(X, tr, margin=float("inf"), device_form=dev)[0] == INVALID
        assert _step(X, None, T=40, device_form=dev)[0] == INVALID
        assert _step(None, tr, n=50, d=23, device_form=dev)[0] == INVALID
        for k in range(3):
            outs = tuple(j != k for j in range(3))
            assert _step(X, tr, outs=outs, device_form=dev)[0] == INVALID, outs
        assert _learn(wide, tr, device_form=dev)[0] == INVALID
        assert _learn(X, tr, margin=-0.5, device_form=dev)[0] == INVALID
        assert _learn(X, tr, reg=-1e-9, device_form=dev)[0] == INVALID and b"reg" in L.blissgpu_last_error()
        assert _learn(X, tr, lr=float("nan"), device_form=dev)[0] == INVALID
        for form in (2, -1):
            assert _learn(X, tr, form=form, device_form=dev)[0] == INVALID and b"form" in L.blissgpu_last_error()
        bad = np.ones(23, np.float32)
        bad[22] = -1e-30
        assert _learn(X, tr, init=bad, device_form=dev)[0] == INVALID and b"init" in L.blissgpu_last_error()
        bad[22] = np.inf
        assert _learn(X, tr, init=bad, device_form=dev)[0] == INVALID
        for k in range(4):
            outs = tuple(j != k for j in range(4))
            assert _learn(X, tr, outs=outs, device_form=dev)[0] == INVALID, outs
    # a valid call of the device forms gets as far as its context
    assert _step(X, tr, device_form=True)[0] == INVALID and b"ctx" in L.blissgpu_last_error()
    assert _learn(X, tr, device_form=True)[0] == INVALID and b"ctx" in L.blissgpu_last_error()
    # no triplet: nothing for a device to do -- OK, zero outputs
    rc, na, loss, G = _step(X, tr[:0])
    assert (rc, na, loss) == (0, 0, 0.0) and not G.reshape(-1)[:529].any()
    # a valid call: BLISSGPU_ERR_NO_DEVICE without a GPU, BLISSGPU_OK with one
    want = 0 if torch.cuda.is_available() else 1
    assert _step(X, tr)[0] == want
    assert _learn(X, tr)[0] == want


# ---- the Python layer's host parts ---------------------------------------------------------------------------------------------
def test_triplets_from_labels(bliss, monkeypatch):
    from bliss_rs_amd import _ffi

    def boom():
        raise AssertionError("the library must not be reached")

    monkeypatch.setattr(_ffi, "lib", boom)
    P = bliss.playlist
    rng = np.random.default_rng(1)
    labels = rng.integers(-1, 6, 300)
    labels[labels == 4] = 40  # (labels need not be dense)
    labels[7] = 99  # a label of one row: never (a, b), sometimes o
    t = P.triplets_from_labels(labels, 4000, seed=3)
    assert t.shape == (4000, 3) and t.dtype == np.int64
    assert t.tobytes() == P.triplets_from_labels(labels.tolist(), 4000, 3).tobytes()  # a function of its arguments
    assert t.tobytes() != P.triplets_from_labels(labels, 4000, 4).tobytes()
    la, lb, lo = labels[t[:, 0]], labels[t[:, 1]], labels[t[:, 2]]
    assert (la == lb).all() and (t[:, 0] != t[:, 1]).all() and (lo != la).all()
    assert (la >= 0).all() and (lo >= 0).all() and (la != 99).all() and (lo == 99).any()
    assert set(np.unique(la)) == set(np.unique(labels[labels >= 0])) - {99}  # every label with two rows is drawn from
    assert np.unique(t[:, 2]).size == (labels >= 0).sum()  # ... and every labelled row is somebody's odd one out
    assert P.triplets_from_labels(labels, 0).shape == (0, 3)
    two = P.triplets_from_labels([5, 5, 9], 50, 0)  # the smallest legal input
    assert set(map(tuple, two)) == {(0, 1, 2), (1, 0, 2)}
    for bad in ([3, 3, 3, 3], [-1, -1, 2, 2], [0, 1, 2, 3], [-1, -1], []):
        with pytest.raises(ValueError):
            P.triplets_from_labels(bad, 10)
    with pytest.raises(ValueError):
        P.triplets_from_labels([0, 0, 1], -1)
    # argument errors of learn_metric that need no device
    X = np.zeros((5, 3), np.float32)
    with pytest.raises(ValueError):
        P.learn_metric(X, [[0, 1, 2]], form="lower")
    with pytest.raises(ValueError):
        P.learn_metric(X, [[0, 1, 2]], max_iter=-1)
    with pytest.raises(ValueError):
        P.learn_metric(X, [[0, 1, 2]], init=np.ones(4))
    with pytest.raises(ValueError):
        P.triplet_step(X, [[0, 1, -2]])
    with pytest.raises(ValueError):
        P.triplet_step(X, [[0, 1, 2]], m=np.eye(4))
    assert P.triplet_accuracy(X, np.zeros((0, 3), np.int64)) == 1.0


def _song(bliss, i, analysed=True):
    V2 = bliss.FeaturesVersion.Version2
    return bliss.Song(path=f"/m/{i}.flac", analysis=bliss.Analysis(np.full(23, i, np.float32), V2), features_version=V2,
                      genre="g%d" % (i % 2))


def test_training_triplet_table(bliss, monkeypatch):
    from bliss_rs_amd import _ffi

    def boom():
        raise AssertionError("the library must not be reached")

    monkeypatch.setattr(_ffi, "lib", boom)
    lib = bliss.library
    # a fresh database: create_schema makes no training_triplet table -- nothing, and the first answer creates it
    db = sqlite3.connect(":memory:")
    lib.create_schema(db)
    lib.store_songs(db, [_song(bliss, i) for i in range(6)])
    assert lib.training_triplets(db).shape == (0, 3) and lib.training_triplets(db).dtype == np.int64
    lib.store_training_triplet(db, "/m/4.flac", "/m/5.flac", "/m/0.flac")
    lib.store_training_triplet(db, "/m/1.flac", "/m/1.flac", "/m/3.flac")
    assert lib.training_triplets(db).tolist() == [[4, 5, 0], [1, 1, 3]]
    with pytest.raises(bliss.ProviderError):
        lib.store_training_triplet(db, "/m/4.flac", "/m/nowhere.flac", "/m/0.flac")
    # a song that is not analysed (or of another features version) takes its triplets with it, and the rows are those of
    # load_feature_matrix: the songs left, in id order
    db.execute("update song set analyzed = false where path = '/m/0.flac'")
    assert lib.training_triplets(db).tolist() == [[0, 0, 2]]
    ids, paths, _ = lib.load_feature_matrix(db)
    assert [paths[i] for i in lib.training_triplets(db)[0]] == ["/m/1.flac", "/m/1.flac", "/m/3.flac"]
    db.execute("update song set version = 1 where path = '/m/3.flac'")
    assert lib.training_triplets(db).shape == (0, 3)
    # a database migrated from an older schema has the crate's table: rows written by the crate's statement are read
    old = sqlite3.connect(":memory:")
    lib.create_schema(old)
    old.execute("pragma user_version = 3")
    assert lib.upgrade(old) == 5
    lib.store_songs(old, [_song(bliss, i) for i in range(4)])
    old.execute("insert into training_triplet (song_1_id, song_2_id, odd_one_out_id) values (2, 3, 1)")
    old.execute("insert into training_triplet (song_1_id, song_2_id, odd_one_out_id) values (1, 4, 2)")
    assert lib.training_triplets(old).tolist() == [[1, 2, 0], [0, 3, 1]]
    lib.store_training_triplet(old, "/m/0.flac", "/m/1.flac", "/m/2.flac")
    assert lib.training_triplets(old).tolist() == [[1, 2, 0], [0, 3, 1], [0, 1, 2]]
    # no triplet, unknown source: refused before any device call
    empty = sqlite3.connect(":memory:")
    lib.create_schema(empty)
    lib.store_songs(empty, [_song(bliss, i) for i in range(4)])
    with pytest.raises(ValueError):
        lib.learn_metric(empty)
    with pytest.raises(ValueError):
        lib.learn_metric(empty, source="mood")
    with pytest.raises(ValueError):
        lib.learn_metric(empty, source=[0, 0, 1])  # three labels for four songs


# ---- metric_learn.hpp as a stand-alone program ---------------------------------------------------------------------------------
def _write_case(path, form, d, T, lr, reg, max_iter, init, recs):
    with open(path, "wb") as f:
        f.write(struct.pack("<iIQddIII", form, d, T, lr, reg, max_iter, len(recs), 0 if init is None else 1))
        if init is not None:
            f.write(np.asarray(init, np.float32).tobytes())
        for rc, loss, act, G in recs:
            f.write(struct.pack("<iQd", rc, act, loss))
            f.write(np.ascontiguousarray(G, np.float64).tobytes())


def _read_result(path, d):
    b = open(path, "rb").read()
    rc, status, n_iter, best_iter, used = struct.unpack_from("<iiIII", b, 0)
    at, dd = 20, d * d
    M = np.frombuffer(b, np.float32, dd, at).reshape(d, d)
    at += 4 * dd
    k = 0 if rc else n_iter + 1
    obj = np.frombuffer(b, np.float64, k, at)
    at += 8 * k
    act = np.frombuffer(b, np.uint64, k, at)
    at += 8 * k
    seen = np.frombuffer(b, np.float32, used * dd, at).reshape(used, d, d)
    assert at + 4 * used * dd == len(b)
    return {"rc": rc, "status": status, "n_iter": n_iter, "best_iter": best_iter, "M": M, "obj": obj, "active": act, "seen": seen}


def _cases():
    """(name, form, d, T, lr, reg, max_iter, init, recs): gradient sequences a device could have returned -- the loop does not
    care where G comes from, so these are seeded symmetric matrices with entries the sums round on"""
    rng = np.random.default_rng(11)

    def grads(k, d, scale=1.0, active=None, rc=None):
        out = []
        for i in range(k):
            A = rng.standard_normal((d, d)) * scale * 1000.0
            out.append((0 if rc is None else rc[i], float(rng.random() * 500.0), int(rng.integers(1, 2000)) if active is None else active[i],
                        A + A.T))
        return out

    w23 = (rng.random(23) * 3.0).astype(np.float32)
    cases = []
    for form, name in ((DIAGONAL, "diag"), (FULL, "full")):
        cases.append((f"{name}_d23", form, 23, 1000, 1.0, 0.0, 5, None, grads(6, 23)))
        cases.append((f"{name}_d23_reg_init", form, 23, 777, 0.3, 0.01, 5, w23, grads(6, 23)))
        cases.append((f"{name}_d5_converges", form, 5, 64, 1.0, 0.01, 9, None, grads(4, 5, active=[9, 4, 1, 0])))
        cases.append((f"{name}_max_iter_0", form, 7, 50, 1.0, 0.0, 0, None, grads(1, 7)))
        cases.append((f"{name}_d64", form, 64, 12345, 0.5, 0.001, 2, None, grads(3, 64)))
        # lr far too large: M overflows float32 (FULL squares L) or a NaN hinge comes back after the first iteration
        cases.append((f"{name}_diverges", form, 6, 10, 1e37, 0.0, 20, None, grads(21, 6)))
        cases.append((f"{name}_nan_hinge_later", form, 6, 10, 0.01, 0.0, 20, None, grads(3, 6, rc=[0, 0, NAN_CODE])))
        cases.append((f"{name}_nan_hinge_first", form, 6, 10, 0.01, 0.0, 20, None, grads(1, 6, rc=[NAN_CODE])))
        cases.append((f"{name}_no_triplets", form, 4, 0, 1.0, 0.5, 3, None, grads(1, 4, active=[0])))
    # the clamp at 0: a positive gradient on the diagonal, lr large enough to push every weight below zero, then back up
    G = np.diag(np.linspace(50.0, 900.0, 8))
    cases.append(("diag_clamp", DIAGONAL, 8, 10, 1.0, 0.0, 3, np.linspace(0.0, 2.0, 8).astype(np.float32),
                  [(0, 10.0, 5, G), (0, 9.0, 5, -G * 0.001), (0, 8.0, 5, G * 1e-6), (0, 7.0, 5, G)]))
    return cases


def _check_program(exe, tmp, env=None):
    seen_status = set()
    for name, form, d, T, lr, reg, max_iter, init, recs in _cases():
        fin, fout = str(tmp / f"{name}.in"), str(tmp / f"{name}.out")
        _write_case(fin, form, d, T, lr, reg, max_iter, init, recs)
        out = subprocess.run([str(exe), fin, fout], capture_output=True, text=True, timeout=120, env=env)
        assert out.returncode == 0, (name, out.stdout[-500:], out.stderr[-3000:])
        assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, (name, out.stderr[-3000:])
        got = _read_result(fout, d)
        it = iter(recs)
        want = ref_learn(form, d, init, T, lr, reg, max_iter, lambda M: next(it))
        assert got["rc"] == want["rc"], name
        assert len(got["seen"]) == len(want["seen"]), name
        for a, b in zip(got["seen"], want["seen"]):  # every M_t, bit for bit
            assert np.array_equal(f32_bits(a), f32_bits(b)), name
        if want["rc"]:
            assert name.endswith("nan_hinge_first")
            continue
        assert (got["status"], got["n_iter"], got["best_iter"]) == (want["status"], want["n_iter"], want["best_iter"]), (name, got, want)
        assert np.array_equal(f32_bits(got["M"]), f32_bits(want["M"])), name
        assert np.array_equal(f64_bits(got["obj"]), f64_bits(want["obj"])), (name, got["obj"], want["obj"])
        assert np.array_equal(got["active"].astype(np.int64), want["active"]), name
        seen_status.add((form, got["status"]))
        if name == "diag_clamp":
            w1 = np.diag(got["seen"][1])
            assert (w1 == 0.0).all() and (np.diag(got["seen"][2]) > 0.0).all()  # clamped, then free again
        if name.endswith("_diverges"):
            assert got["status"] == DIVERGED and got["n_iter"] >= 1 and np.isfinite(got["M"]).all() and not np.isfinite(got["obj"][-1])
        if name.endswith("nan_hinge_later"):
            assert got["status"] == DIVERGED and got["n_iter"] == 2 and np.isnan(got["obj"][2])
        if name.endswith("_no_triplets"):
            assert got["status"] == CONVERGED and got["n_iter"] == 0 and got["obj"][0] == 0.0
    assert seen_status == {(f, s) for f in (DIAGONAL, FULL) for s in (CONVERGED, MAX_ITER, DIVERGED)}


def test_metric_learn_header_against_the_restatement(tmp_path):
    exe = tmp_path / "test_metric_learn"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", SRC, "-o", str(exe)])
    _check_program(exe, tmp_path)


@pytest.mark.skipif(not os.path.exists(SAN_CXX), reason="needs the ROCm clang for -fsanitize=address,undefined")
def test_metric_learn_header_under_address_and_ub_sanitizer(tmp_path):
    """the same stand-alone program built with -fsanitize=address,undefined: same bits, exit 0, no report"""
    exe = tmp_path / "test_metric_learn_san"
    subprocess.check_call([SAN_CXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", SRC, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    _check_program(exe, tmp_path, env)


def test_metric_learn_header_is_device_free():
    src = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "metric_learn.hpp")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "hip" not in code.lower() and "fma" not in code
    assert re.findall(r"#include\s+[<\"]([^>\"]+)", code) == ["math.h", "stdint.h", "vector"]
