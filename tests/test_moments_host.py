"""Device-free tests of the library moments and the covariance metrics (blissgpu_moments / blissgpu_moments_device /
blissgpu_covariance_metric): the C ABI surface, the kernels' names in the profile table, the argument checks that happen before the
device is touched, covariance_metric.hpp against a scalar-loop restatement of the contract (a stand-alone program, plain and under
sanitizers), and the host-side parts of the Python layer."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_covariance_metric.cpp")
HPP = os.path.join(ROOT, "bliss-rs_amd", "csrc", "covariance_metric.hpp")
SAN_CXX = "/opt/rocm/lib/llvm/bin/clang++"
_vp = C.c_void_p
OK, NO_DEVICE, INVALID = 0, 1, 2
DIAGONAL, FULL = 0, 1
COV_OK, COV_NOT_POSITIVE = 0, 1


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


def test_moments_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    lib = C.CDLL(bliss.LIB_PATH)
    for name in ("blissgpu_moments", "blissgpu_moments_device", "blissgpu_covariance_metric"):
        assert re.search(r"\bint\s+%s\s*\(" % name, flat), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name

    def types(name):
        return [re.sub(r"\s*\b\w+$", "", " ".join(a.split())).replace(" *", "*")
                for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, flat).group(1).split(",")]

    # (x, n, d, labels, k, counts, mean, m2, min, max, S), the device form with the context in front
    want = ["const float*", "uint64_t", "uint32_t", "const uint32_t*", "uint32_t", "uint32_t*", "double*", "double*", "float*", "float*",
            "double*"]
    assert types("blissgpu_moments") == want
    assert types("blissgpu_moments_device") == ["blissgpu_ctx*"] + want
    assert types("blissgpu_covariance_metric") == ["const double*", "uint32_t", "uint64_t", "int", "double", "float*", "int32_t*"]
    u64, u32 = C.c_uint64, C.c_uint32
    host = [_vp, u64, u32, _vp, u32, _vp, _vp, _vp, _vp, _vp, _vp]
    assert _ffi.SIGNATURES["blissgpu_moments"] == (C.c_int, host)
    assert _ffi.SIGNATURES["blissgpu_moments_device"] == (C.c_int, [_vp] + host)
    assert _ffi.SIGNATURES["blissgpu_covariance_metric"] == (C.c_int, [_vp, u32, u64, C.c_int, C.c_double, _vp, C.POINTER(C.c_int32)])
    for macro, value in (("BLISSGPU_MOMENTS_BLOCK", 256), ("BLISSGPU_COV_OK", 0), ("BLISSGPU_COV_NOT_POSITIVE", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), flat), macro
    assert (_ffi.MOMENTS_BLOCK, _ffi.COV_OK, _ffi.COV_NOT_POSITIVE) == (256, 0, 1)


def test_moments_kernels_are_in_the_profile_table(bliss):
    from bliss_rs_amd import _ffi

    L = _ffi.lib()
    names = [L.blissgpu_profile_kernel_name(k).decode() for k in range(L.blissgpu_profile_kernel_count())]
    assert len(set(names)) == len(names) and "" not in names
    src = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "kernels_moments.hip")).read()
    mine = ("moments_plan_kernel", "moments_sum_kernel", "moments_m2_kernel", "moments_scatter_kernel", "moments_reduce_kernel",
            "moments_finish_kernel")
    for name in mine:
        assert names.count(name) == 1, name
        assert re.search(r"\bvoid\s+%s\s*\(" % name, src), name
        assert names.index(name) < len(names) - 2
    assert sorted(n for n in names if n.startswith("moments_")) == sorted(mine)
    assert names[-2:] == ["group_forest_scan_kernel", "journey_step_kernel"]  # (older ids keep their places)


def _p(a):
    return None if a is None else a.ctypes.data


def _call(x, labels, k, n=None, d=None, device=False, x_null=False, counts=True, mean=True, m2=True, mn=True, mx=True, S=True):
    from bliss_rs_amd import _ffi

    n = x.shape[0] if n is None else n
    d = x.shape[1] if d is None else d
    kk, dd = max(min(k, 70000), 1), max(x.shape[1], 1)
    out = dict(counts=np.full(kk, 7, np.uint32), mean=np.full((kk, dd), 7.0), m2=np.full((kk, dd), 7.0),
               mn=np.full((kk, dd), 7, np.float32), mx=np.full((kk, dd), 7, np.float32), S=np.full((dd, dd), 7.0))
    args = (None if x_null else _p(x), n, d, _p(labels), k, _p(out["counts"]) if counts else None, _p(out["mean"]) if mean else None,
            _p(out["m2"]) if m2 else None, _p(out["mn"]) if mn else None, _p(out["mx"]) if mx else None, _p(out["S"]) if S else None)
    L = _ffi.lib()
    rc = L.blissgpu_moments_device(None, *args) if device else L.blissgpu_moments(*args)
    return rc, L.blissgpu_last_error(), out


def test_moments_arguments_are_checked_before_the_device(bliss):
    import torch

    rng = np.random.default_rng(0)
    X = rng.standard_normal((50, 23)).astype(np.float32)
    lab = (np.arange(50) % 4).astype(np.uint32)
    for device in (False, True):
        assert _call(X, lab, 4, d=0, device=device)[0] == INVALID
        assert _call(np.zeros((50, 65), np.float32), lab, 4, device=device)[0] == INVALID
        assert _call(X, lab, 0, device=device)[0] == INVALID
        assert _call(X, lab, 65536, device=device)[0] == INVALID
        assert _call(X, None, 4, device=device)[0] == INVALID  # NULL labels: k must be 1
        assert _call(X, None, 0, device=device)[0] == INVALID
        assert _call(X, lab, 4, n=0xFFFFFFFF, device=device)[0] == INVALID
        assert _call(X, lab, 4, x_null=True, device=device)[0] == INVALID
        assert _call(X, lab, 4, counts=False, device=device)[0] == INVALID
        assert _call(X, lab, 4, mean=False, device=device)[0] == INVALID
        assert _call(X, lab, 4, mn=False, device=device)[0] == INVALID  # min and max: both or neither
        assert _call(X, lab, 4, mx=False, device=device)[0] == INVALID
    # the device form checks the scalars before it looks at its context ...
    rc, err, _ = _call(X, lab, 0, device=True)
    assert rc == INVALID and b"k must be" in err
    rc, err, _ = _call(X, None, 2, device=True)
    assert rc == INVALID and b"labels" in err
    # ... and the context before anything else (the optional outputs may all be NULL)
    rc, err, _ = _call(X, lab, 4, device=True, m2=False, mn=False, mx=False, S=False)
    assert rc == INVALID and b"ctx" in err
    # the host form's labels are host memory: checked before the device is touched
    bad = lab.copy()
    bad[17] = 4
    rc, err, _ = _call(X, bad, 4)
    assert rc == INVALID and b"label" in err
    # no row: nothing for a device to do -- OK with zero outputs and empty extrema
    rc, _, out = _call(X[:0], lab[:0], 4)
    assert rc == OK and not out["counts"][:4].any() and not out["mean"][:4].any() and not out["m2"][:4].any() and not out["S"].any()
    assert (out["mn"][:4] == np.inf).all() and (out["mx"][:4] == -np.inf).all()
    assert _call(X[:0], None, 1, m2=False, mn=False, mx=False, S=False)[0] == OK
    # a valid call: BLISSGPU_ERR_NO_DEVICE without a GPU, BLISSGPU_OK with one
    want = OK if torch.cuda.is_available() else NO_DEVICE
    assert _call(X, lab, 4)[0] == want
    assert _call(X, None, 1, m2=False, mn=False, mx=False, S=False)[0] == want


def test_covariance_metric_arguments(bliss):
    from bliss_rs_amd import _ffi

    L = _ffi.lib()
    S = np.eye(3)
    M = np.full((3, 3), 7, np.float32)
    st = C.c_int32(5)

    def call(S_=S, d=3, dof=10, form=FULL, shrink=0.01, M_=M, st_=st):
        return L.blissgpu_covariance_metric(_p(S_), d, dof, form, shrink, _p(M_), C.byref(st_) if st_ is not None else None)

    assert call(dof=0) == INVALID
    assert call(shrink=-0.001) == INVALID and call(shrink=1.001) == INVALID and call(shrink=float("nan")) == INVALID
    assert call(form=2) == INVALID and call(form=-1) == INVALID
    assert call(d=0) == INVALID and call(d=65) == INVALID
    assert call(S_=None) == INVALID and call(M_=None) == INVALID and call(st_=None) == INVALID
    assert (M == 7).all() and st.value == 5
    assert call() == OK and st.value == COV_OK and np.array_equal(M, np.eye(3, dtype=np.float32))
    # not positive definite: OK with the status set, M untouched
    M[:] = 7
    assert call(S_=np.zeros((3, 3)), shrink=0.0) == OK and st.value == COV_NOT_POSITIVE and (M == 7).all()


# ---- covariance_metric.hpp against a restatement of include/blissgpu.h in scalar loops (Python floats are IEEE f64: one
# rounding per operation, sums ascending from 0.0) ----
def ref_covariance_metric(S, dof, form, shrink):
    """-> (status, M float32 or None, W float64 or None, C' as nested lists)"""
    d = len(S)
    S = [[float(v) for v in row] for row in S]
    Cm = [[0.0] * d for _ in range(d)]
    for r in range(d):
        for c in range(r, d):
            Cm[r][c] = Cm[c][r] = S[r][c] / float(dof)
    T = 0.0
    for r in range(d):
        T = T + Cm[r][r]
    T = T / float(d)
    keep, target = 1.0 - shrink, shrink * T
    W = [[0.0] * d for _ in range(d)]

    def pos(v):
        return v > 0.0 and math.isfinite(v)

    Cp = [[keep * Cm[r][c] + target if r == c else keep * Cm[r][c] for c in range(d)] for r in range(d)]
    if form == DIAGONAL:
        for r in range(d):
            den = keep * Cm[r][r] + target
            w = 1.0 / den if den != 0.0 else math.inf
            if not pos(w):
                return COV_NOT_POSITIVE, None, None, Cp
            W[r][r] = w
    else:
        L = [[0.0] * d for _ in range(d)]
        for i in range(d):
            for j in range(i + 1):
                s = 0.0
                for k in range(j):
                    s = s + L[i][k] * L[j][k]
                rest = Cp[i][j] - s
                if j == i:
                    if not pos(rest):
                        return COV_NOT_POSITIVE, None, None, Cp
                    L[i][i] = math.sqrt(rest)
                else:
                    L[i][j] = rest / L[j][j]
        Li = [[0.0] * d for _ in range(d)]
        for j in range(d):
            Li[j][j] = 1.0 / L[j][j]
            for i in range(j + 1, d):
                s = 0.0
                for k in range(j, i):
                    s = s + L[i][k] * Li[k][j]
                Li[i][j] = (0.0 - s) / L[i][i]
        for r in range(d):
            for c in range(r, d):
                s = 0.0
                for k in range(c, d):
                    s = s + Li[k][r] * Li[k][c]
                W[r][c] = W[c][r] = s
    tr = 0.0
    for r in range(d):
        tr = tr + W[r][r]
    scale = float(d) / tr if tr != 0.0 else math.inf
    if not pos(scale):
        return COV_NOT_POSITIVE, None, None, Cp
    M = np.array([[np.float32(W[r][c] * scale) for c in range(d)] for r in range(d)], np.float32)
    return COV_OK, M, np.array(W, np.float64), Cp


def _scatter(rng, d, constant=None):
    n = 3 * d + 5
    X = rng.standard_normal((n, d)) * np.logspace(-2, 2, d)[None, :]
    if constant is not None:
        X[:, constant] = 0.25
    U = X - X.mean(axis=0)
    return U.T @ U, n - 1


def _run_program(exe, tmp, name, S, dof, form, shrink, env=None):
    d = S.shape[0]
    fin, fout = str(tmp / f"{name}.in"), str(tmp / f"{name}.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<IIQd", d, form, dof, shrink))
        f.write(np.ascontiguousarray(S, np.float64).tobytes())
    out = subprocess.run([str(exe), fin, fout], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, (name, out.stdout[-500:], out.stderr[-3000:])
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, (name, out.stderr[-3000:])
    raw = open(fout, "rb").read()
    status = struct.unpack_from("<i", raw, 0)[0]
    M = np.frombuffer(raw, np.float32, d * d, 4).reshape(d, d)
    W = np.frombuffer(raw, np.float64, d * d, 4 + 4 * d * d).reshape(d, d)
    return status, M, W


def _check_program(exe, tmp, env=None):
    rng = np.random.default_rng(24)
    eps = np.finfo(np.float64).eps
    for d in (1, 2, 23, 64):
        S, dof = _scatter(rng, d)
        for form in (DIAGONAL, FULL):
            for shrink in (0.0, 0.01, 1.0):
                name = f"d{d}_f{form}_s{shrink}"
                status, M, W = _run_program(exe, tmp, name, S, dof, form, shrink, env)
                want_status, want_M, want_W, Cp = ref_covariance_metric(S, dof, form, shrink)
                assert status == want_status == COV_OK, name
                assert np.array_equal(M.view(np.uint32), want_M.view(np.uint32)), name  # bit for bit
                assert np.array_equal(W.view(np.uint64), want_W.view(np.uint64)), name
                assert np.array_equal(M, M.T) and abs(float(np.trace(M.astype(np.float64))) - d) <= 1e-5 * d, name
                Cp = np.array(Cp)
                if form == DIAGONAL:
                    Cp = np.diag(np.diag(Cp))
                    assert np.count_nonzero(M - np.diag(np.diag(M))) == 0, name
                # the unscaled inverse against C': the bound of a backward-stable solve, 64 d eps cond(C')
                resid = np.abs(W @ Cp - np.eye(d)).max()
                assert resid <= 64 * d * eps * np.linalg.cond(Cp), (name, resid)
                if shrink == 1.0:  # all weight on the mean variance: the identity
                    assert np.array_equal(M, np.eye(d, dtype=np.float32)), name
    # a constant feature: singular at shrink 0 (both forms), cured by the default shrinkage
    S, dof = _scatter(rng, 23, constant=11)
    assert S[11, 11] == 0.0
    for form in (DIAGONAL, FULL):
        status, M, _ = _run_program(exe, tmp, f"singular_f{form}", S, dof, form, 0.0, env)
        assert status == COV_NOT_POSITIVE == ref_covariance_metric(S, dof, form, 0.0)[0]
        assert (M == 7.0).all()  # untouched
        status, M, _ = _run_program(exe, tmp, f"cured_f{form}", S, dof, form, 0.01, env)
        want = ref_covariance_metric(S, dof, form, 0.01)
        assert status == want[0] == COV_OK and np.array_equal(M.view(np.uint32), want[1].view(np.uint32))
        assert np.isfinite(M).all() and M[11, 11] == M.diagonal().max()
    # not finite: never OK
    bad = S.copy()
    bad[3, 3] = np.inf
    assert _run_program(exe, tmp, "inf", bad, dof, FULL, 0.01, env)[0] == COV_NOT_POSITIVE
    # an indefinite matrix fails at a later pivot
    ind = np.eye(4)
    ind[0, 3] = ind[3, 0] = 2.0
    assert _run_program(exe, tmp, "indefinite", ind, 5, FULL, 0.0, env)[0] == COV_NOT_POSITIVE


def test_covariance_metric_header_against_the_restatement(tmp_path):
    exe = tmp_path / "test_covariance_metric"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", SRC, "-o", str(exe)])
    _check_program(exe, tmp_path)


@pytest.mark.skipif(not os.path.exists(SAN_CXX), reason="needs the ROCm clang for -fsanitize=address,undefined")
def test_covariance_metric_header_under_address_and_ub_sanitizer(tmp_path):
    """the same stand-alone program built with -fsanitize=address,undefined: same bits, exit 0, no report"""
    exe = tmp_path / "test_covariance_metric_san"
    subprocess.check_call([SAN_CXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", SRC, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    _check_program(exe, tmp_path, env)


def test_covariance_metric_header_is_device_free():
    code = re.sub(r"//[^\n]*", "", open(HPP).read())
    assert "hip" not in code.lower() and "fma" not in code
    assert re.findall(r"#include\s+[<\"]([^>\"]+)", code) == ["math.h", "stdint.h", "vector"]


def test_the_library_solve_equals_the_restatement(bliss):
    """blissgpu_covariance_metric itself (the header compiled into the library) touches no device and gives the same bits"""
    P = bliss.playlist
    rng = np.random.default_rng(7)
    S, dof = _scatter(rng, 23)
    for form, code in (("diagonal", DIAGONAL), ("full", FULL)):
        got = P.metric_from_scatter(S, dof, form, 0.01)
        want = ref_covariance_metric(S, dof, code, 0.01)[1]
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    S, dof = _scatter(rng, 23, constant=4)
    with pytest.raises(ValueError, match="shrink"):
        P.metric_from_scatter(S, dof, "full", 0.0)
    with pytest.raises(ValueError, match="dof"):
        P.metric_from_scatter(S, 0, "full")
    with pytest.raises(ValueError):
        P.metric_from_scatter(S, dof, "cholesky")
    with pytest.raises(ValueError):
        P.metric_from_scatter(S, dof, "full", 1.5)
    assert P.COV_SHRINK == 0.01


# ---- the Python layer, with the device call replaced by numpy ----
def _numpy_moments(P):
    calls = []

    def fake(X, labels=None, k=None, scatter=True):
        X = np.asarray(X, np.float64)
        n, d = X.shape
        lab = np.zeros(n, np.int64) if labels is None else np.asarray(labels, np.int64)
        assert lab.size == 0 or lab.min() >= 0, "rows without a label must be left out before the call"
        k = (int(lab.max()) + 1 if (n and labels is not None) else 1) if k is None else k
        counts = np.bincount(lab, minlength=k)
        mean, m2 = np.zeros((k, d)), np.zeros((k, d))
        mn, mx = np.full((k, d), np.inf, np.float32), np.full((k, d), -np.inf, np.float32)
        S = np.zeros((d, d))
        for g in range(k):
            rows = X[lab == g]
            if len(rows):
                mean[g] = rows.mean(axis=0)
                U = rows - mean[g]
                m2[g] = (U * U).sum(axis=0)
                mn[g], mx[g] = rows.min(axis=0), rows.max(axis=0)
                S += U.T @ U
        calls.append((n, k, scatter))
        return P.Moments(counts, mean, m2, mn, mx, S if scatter else None)

    return fake, calls


def test_moments_result_and_label_filtering(bliss, monkeypatch):
    P = bliss.playlist
    mo = P.Moments([3, 0, 1], np.ones((3, 2)), [[12.0, 3.0], [0.0, 0.0], [0.0, 0.0]], np.zeros((3, 2)), np.ones((3, 2)), np.eye(2))
    assert mo.dof == 4 - 2 and mo.counts.dtype == np.int64 and mo.min.dtype == np.float32
    assert mo.var.tolist() == [[4.0, 1.0], [0.0, 0.0], [0.0, 0.0]] and mo.std.tolist() == [[2.0, 1.0], [0.0, 0.0], [0.0, 0.0]]
    assert P.Moments([2], np.zeros((1, 2)), np.zeros((1, 2)), np.zeros((1, 2)), np.zeros((1, 2)), None).scatter is None

    fake, calls = _numpy_moments(P)
    monkeypatch.setattr(P, "moments", fake)
    rng = np.random.default_rng(3)
    X = rng.standard_normal((40, 5)).astype(np.float32)
    lab = rng.integers(0, 3, 40)
    lab[[2, 9, 30]] = -1
    res = P.covariance_metric(X, lab)
    assert calls[-1] == (37, 3, True) and res.dof == 37 - 3 and res.form == "full" and res.shrink == P.COV_SHRINK
    assert res.m.shape == (5, 5) and res.m.dtype == np.float32 and np.array_equal(res.m, res.m.T)
    assert isinstance(res.builder(), P.MahalanobisBuilder) and np.array_equal(res.builder().m, res.m)
    keep = lab >= 0
    same = P.covariance_metric(X[keep], lab[keep])
    assert np.array_equal(same.m, res.m) and np.array_equal(same.scatter, res.scatter)
    total = P.covariance_metric(X, None, "diagonal")
    assert calls[-1] == (40, 1, True) and total.dof == 39 and np.count_nonzero(total.m - np.diag(np.diag(total.m))) == 0
    # dof <= 0: every row alone in its group; no row at all; only rows without a label
    with pytest.raises(ValueError, match="dof"):
        P.covariance_metric(X[:4], [0, 1, 2, 3])
    with pytest.raises(ValueError, match="dof"):
        P.covariance_metric(X[:0])
    with pytest.raises(ValueError, match="dof"):
        P.covariance_metric(X[:3], [-1, -1, -1])
    # not positive definite names the cure
    Xc = X.copy()
    Xc[:, 2] = 1.5
    with pytest.raises(ValueError, match="shrink"):
        P.covariance_metric(Xc, None, "full", 0.0)
    assert np.isfinite(P.covariance_metric(Xc, None, "full").m).all()
    with pytest.raises(ValueError):
        P.covariance_metric(X, lab[:-1])
    with pytest.raises(ValueError):
        P.covariance_metric(X, lab, "triangular")


def test_library_statistics_naming_and_sources(bliss, monkeypatch, tmp_path):
    P, Lb = bliss.playlist, bliss.library
    fake, calls = _numpy_moments(P)
    monkeypatch.setattr(P, "moments", fake)
    rng = np.random.default_rng(11)
    n = 30
    X = rng.uniform(-1, 1, (n, 23)).astype(np.float32)
    genres = ["rock", "jazz", None]
    V2 = bliss.FeaturesVersion.Version2
    songs = [bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist=f"artist{i % 4}", album=f"album {i % 5}", duration=1.0,
                        genre=genres[i % 3], analysis=bliss.Analysis(X[i], V2), features_version=V2) for i in range(n)]
    db = str(tmp_path / "bliss.db")
    Lb.create_schema(db)
    Lb.store_songs(db, songs)
    Xdb = Lb.load_feature_matrix(db)[2]
    stats = Lb.statistics(db)
    assert list(stats) == [bliss.AnalysisIndex(r).name for r in range(23)] and list(stats)[0] == "Tempo" and list(stats)[22] == "Chroma13"
    assert calls[-1] == (n, 1, False)
    for r, name in enumerate(stats):
        assert set(stats[name]) == {"mean", "std", "min", "max", "count"} and stats[name]["count"] == n
        assert stats[name]["min"] == float(Xdb[:, r].min()) and stats[name]["max"] == float(Xdb[:, r].max())
        assert abs(stats[name]["mean"] - float(Xdb[:, r].astype(np.float64).mean())) < 1e-12
        assert abs(stats[name]["std"] - float(Xdb[:, r].astype(np.float64).std())) < 1e-12
    by = Lb.statistics(db, "genre")
    assert list(by) == ["rock", "jazz"] and calls[-1] == (20, 2, False)  # NULL tags are left out
    assert by["jazz"]["Zcr"]["count"] == 10 and by["rock"]["Tempo"]["min"] == float(Xdb[0::3, 0].min())
    assert sorted(Lb.statistics(db, "artist")) == [f"artist{i}" for i in range(4)]
    with pytest.raises(ValueError):
        Lb.statistics(db, "title")
    # covariance_metric's sources: None, a column (NULL tags left out), a label array
    M = Lb.covariance_metric(db)
    assert M.shape == (23, 23) and M.dtype == np.float32 and calls[-1] == (n, 1, True)
    assert np.array_equal(M, P.covariance_metric(Xdb).m)
    Mg = Lb.covariance_metric(db, "genre", return_result=True)
    assert calls[-1] == (20, 2, True) and Mg.dof == 18
    lab = np.array([-1 if g is None else genres.index(g) for g in (genres[i % 3] for i in range(n))])
    assert np.array_equal(Mg.m, Lb.covariance_metric(db, lab)) and np.array_equal(Mg.m, P.covariance_metric(Xdb, lab).m)
    diag = Lb.covariance_metric(db, "album", "diagonal", 0.5)
    assert np.count_nonzero(diag - np.diag(np.diag(diag))) == 0
    with pytest.raises(ValueError):
        Lb.covariance_metric(db, "title")
    with pytest.raises(ValueError):
        Lb.covariance_metric(db, lab[:-1])
    empty = str(tmp_path / "empty.db")
    Lb.create_schema(empty)
    assert Lb.statistics(empty) == {} and Lb.statistics(empty, "genre") == {}
