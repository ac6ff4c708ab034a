"""Host tests (no GPU) of k-medoids (blissgpu_kmedoids / blissgpu_pam_scan): the contract of include/blissgpu.h
written out in numpy -- every f64 sum sequential (cumsum), every minimum with the header's tie rule -- and what it promises on
planted inputs; the ABI surface, the argument checks that come before the device, the refused builders, the profile table and
the Makefile, and library.medoid_songs over a temporary database with the device call replaced.  tests/test_gpu_pam.py holds
the device to this replay bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_ward_host import bits, equal_input, euclid, twice_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = C.c_void_p
OK, NO_DEVICE, INVALID, ERR_NAN = 0, 1, 2, 5
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


# ---- the contract in numpy ----
class NanDistance(Exception):
    """BLISSGPU_ERR_NAN"""


def cosine(X):
    """f32 cosine distances 1 - a.b / (|a| |b|) (for the host tests only: the GPU tests take the device's all-pairs matrix)"""
    X = np.asarray(X, F32)
    norm = np.sqrt((X * X).sum(axis=1, dtype=F32)).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (F32(1) - (X @ X.T).astype(F32) / (norm[:, None] * norm[None, :])).astype(F32)


def bits64(a):
    return np.ascontiguousarray(a, F64).view(np.uint64)


def seq_sum(T, order="ascending"):
    """0.0 + T[:, 0] + T[:, 1] + ...: one sequential f64 sum per row (cumsum adds in order)"""
    T = np.asarray(T, F64)
    if order == "descending":
        T = T[:, ::-1]
    return np.cumsum(np.concatenate([np.zeros((T.shape[0], 1)), T], axis=1), axis=1)[:, -1]


def contract_state(Dm, med, tie="lower"):
    """near, d1, d2, TD of the medoids med: blissgpu_knn over the medoids' columns, min(k, 2) neighbours, ties to the lower slot"""
    med = np.asarray(med, np.int64)
    cols = np.asarray(Dm, F32)[:, med] + F32(0)  # (-0.0 and +0.0 are one value to the search, which answers +0.0)
    if np.isnan(cols).any():
        raise NanDistance
    k = len(med)
    if tie == "lower":
        order = np.argsort(cols, axis=1, kind="stable")
    else:
        order = k - 1 - np.argsort(cols[:, ::-1], axis=1, kind="stable")
    near = order[:, 0]
    rows = np.arange(cols.shape[0])
    d1 = cols[rows, near]
    d2 = cols[rows, order[:, 1]] if k >= 2 else np.full(cols.shape[0], np.inf, F32)
    td = float(seq_sum(d1[None, :].astype(F64))[0])
    return near, d1, d2, td


def contract_scan(Dm, near, d1, d2, k, rows=None, tie="lower", use_d2=True, order="ascending"):
    """-> btot, best, arg, A, B of the header's ONE SCAN for the candidates `rows` (None: every song)"""
    Dm = np.asarray(Dm, F32)
    n = Dm.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    doc = Dm[rows]  # [q, n]
    if np.isnan(doc).any():
        raise NanDistance
    d1, d2 = np.asarray(d1, F32), np.asarray(d2, F32)
    capped = np.fmin(doc, d2[None, :]) if use_d2 else doc
    ta = capped.astype(F64) - d1.astype(F64)[None, :]
    tb = np.fmin(doc.astype(F64) - d1.astype(F64)[None, :], 0.0)
    q = len(rows)
    A, B = np.zeros((q, k)), np.zeros((q, k))
    for m in range(k):
        sel = np.flatnonzero(np.asarray(near) == m)  # ascending o
        A[:, m] = seq_sum(ta[:, sel], order)
        B[:, m] = seq_sum(tb[:, sel], order)
    btot = seq_sum(B, order)
    with np.errstate(invalid="ignore"):
        delta = (btot[:, None] - B) + A
    best, arg = delta[:, 0].copy(), np.zeros(q, np.int64)
    for m in range(1, k):
        with np.errstate(invalid="ignore"):
            better = delta[:, m] < best if tie == "lower" else delta[:, m] <= best
        best[better], arg[better] = delta[better, m], m
    return btot, best, arg, A, B


def pick(values, excluded=()):
    """the smallest (value, c) as f64 (-0.0 == +0.0), ties to the lower c, a NaN and an excluded c never -> c or None"""
    ok = ~np.isnan(values)
    ok[list(excluded)] = False
    idx = np.flatnonzero(ok)
    return int(idx[np.argmin(values[idx])]) if idx.size else None


def contract_build(Dm, k, tie="lower", use_d2=True, medoid_candidates=False):
    n = Dm.shape[0]
    zero = np.zeros(n, F32)
    A = contract_scan(Dm, np.zeros(n, np.int64), zero, np.full(n, np.inf, F32), 1, tie=tie, use_d2=use_d2)[3]
    med = [pick(A[:, 0])]
    for _ in range(1, k):
        near, d1, d2, _ = contract_state(Dm, med, tie)
        btot = contract_scan(Dm, near, d1, d2, len(med), tie=tie, use_d2=use_d2)[0]
        med.append(pick(btot, () if medoid_candidates else med))
    return med


def contract_kmedoids(Dm, k, init=None, max_swaps=None, tie="lower", use_d2=True, medoid_candidates=False):
    """-> medoids, labels, dist, sizes, td_trace, n_swaps, converged, deltas (the delta of every swap made) of the header's
    CLUSTERING over the all-pairs matrix Dm"""
    Dm = np.asarray(Dm, F32)
    n = Dm.shape[0]
    max_swaps = 4 * k + 64 if max_swaps is None else max_swaps
    med = contract_build(Dm, k, tie, use_d2, medoid_candidates) if init is None else [int(i) for i in init]
    trace, deltas, swaps, conv = [], [], 0, False
    while True:
        near, d1, d2, td = contract_state(Dm, med, tie)
        trace.append(td)
        _, best, arg, _, _ = contract_scan(Dm, near, d1, d2, k, tie=tie, use_d2=use_d2)
        c = pick(best, () if medoid_candidates else med)
        if c is None or not best[c] < 0:
            conv = True
            break
        if swaps == max_swaps:
            break
        deltas.append(float(best[c]))
        med[int(arg[c])] = c
        swaps += 1
    return (np.asarray(med, np.int64), near.astype(np.int64), d1, np.bincount(near, minlength=k).astype(np.int64), np.asarray(trace, F64),
            swaps, conv, deltas)


def same_result(res, want):
    """a playlist.Medoids against contract_kmedoids' tuple, bit for bit"""
    return (np.array_equal(res.medoids, want[0]) and np.array_equal(res.labels, want[1]) and np.array_equal(bits(res.dist), bits(want[2]))
            and np.array_equal(res.sizes, want[3]) and np.array_equal(bits64(res.td_trace), bits64(want[4])) and res.n_swaps == want[5]
            and res.converged == want[6] and bits64([res.td])[0] == bits64(want[4][-1:])[0])


def planted_labelled(n, classes=8, d=23):
    """test_ward_host.planted's mixture with its labels"""
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, d)).astype(F32)
    lab = rng.integers(0, classes, n)
    X += (lab[:, None] == np.arange(classes)).astype(F32) @ rng.standard_normal((classes, d)).astype(F32) * 3
    return X, lab


def order_sensitive_input():
    """d = 1, hand-made: under d1 = 0 and d2 = +inf the terms of A are the distances themselves, here 2^60 and three hundred
    ones -- 2^60 + 1 rounds back to 2^60 in f64, so adding the ones first or last gives other bits.  With d1 = twice those
    distances the terms of B are their negatives.  -> X [302, 1], near, d1 for B, k"""
    x = np.ones(302, F32)
    x[0], x[1] = 0.0, 2.0 ** 60
    near = np.zeros(302, np.int64)
    near[200:] = 1
    return x[:, None].copy(), near, (2 * np.abs(x)).astype(F32), 2


# ---- what the contract promises ----
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("n", [300, 600])
def test_build_and_a_random_start_agree_on_planted_songs(metric, n):
    X, lab = planted_labelled(n)
    Dm = euclid(X) if metric == "euclidean" else cosine(X)
    runs = [contract_kmedoids(Dm, 8), contract_kmedoids(Dm, 8, init=np.random.default_rng(n + 1).choice(n, 8, replace=False))]
    for med, labels, dist, sizes, trace, swaps, conv, deltas in runs:
        assert conv and len(trace) == swaps + 1 and len(set(med.tolist())) == 8 and sizes.sum() == n
        # every predicted delta is the realised change of TD
        for t, dlt in enumerate(deltas):
            assert dlt < 0 and abs((trace[t + 1] - trace[t]) - dlt) <= 1e-6 * abs(dlt), (t, dlt, trace[t + 1] - trace[t])
        # the planted labels: every cluster holds one of them and every one of them has a cluster
        assert all(len(set(lab[labels == c].tolist())) == 1 for c in range(8))
        assert len({int(lab[labels == c][0]) for c in range(8)}) == 8
    assert 0 <= runs[0][5] <= 19 and 1 <= runs[1][5] <= 40  # BUILD needs few swaps, a random start about k
    assert runs[0][4][-1] == pytest.approx(runs[1][4][-1], rel=1e-9)  # both starts end at the same TD
    assert sorted(runs[0][0].tolist()) == sorted(runs[1][0].tolist())


def test_small_cases_of_the_contract():
    X, _ = planted_labelled(300)
    Dm = euclid(X[:5])
    med, labels, dist, sizes, trace, swaps, conv, _ = contract_kmedoids(Dm, 5)  # k == n: every song is a medoid, nothing to scan
    assert sorted(med.tolist()) == [0, 1, 2, 3, 4] and conv and swaps == 0 and trace[0] == 0.0 and np.array_equal(med[labels], np.arange(5))
    med, labels, dist, sizes, trace, swaps, conv, _ = contract_kmedoids(Dm, 1)
    assert med[0] == int(np.argmin(Dm.astype(F64).sum(axis=1))) and conv and not labels.any() and np.array_equal(dist, Dm[med[0]])
    # max_swaps: the labels are those of the medoids returned
    start = [0, 1]
    full = contract_kmedoids(euclid(X[:60]), 2, init=start)
    assert full[5] >= 1
    cut = contract_kmedoids(euclid(X[:60]), 2, init=start, max_swaps=0)
    assert cut[5] == 0 and not cut[6] and cut[0].tolist() == start and len(cut[4]) == 1 and cut[4][0] == full[4][0]
    one = contract_kmedoids(euclid(X[:60]), 2, init=start, max_swaps=1)
    assert one[5] == 1 and len(one[4]) == 2 and np.array_equal(one[1], contract_state(euclid(X[:60]), one[0])[0])


def test_the_expectation_moves_with_every_clause():
    twice = euclid(twice_input(200))
    want = contract_kmedoids(twice, 6)
    # ties to the higher slot: every song has a twin, so each medoid's twin sits at distance 0 from two slots once both are medoids
    init = [0, int(np.flatnonzero((twice[0] == 0) & (np.arange(200) != 0))[0]), 5]
    lower, higher = contract_state(twice, init), contract_state(twice, init, tie="higher")
    assert not np.array_equal(lower[0], higher[0]) and np.array_equal(lower[1], higher[1])
    # d2 ignored: removing a medoid then costs nothing beyond the candidate's own distance
    X, _ = planted_labelled(300)
    Dm = euclid(X)
    near, d1, d2, _ = contract_state(Dm, [3, 50, 120, 200])
    a, b = contract_scan(Dm, near, d1, d2, 4), contract_scan(Dm, near, d1, d2, 4, use_d2=False)
    assert not np.array_equal(bits64(a[3]), bits64(b[3])) and np.array_equal(bits64(a[4]), bits64(b[4]))
    assert not np.array_equal(a[2], b[2])
    # a medoid allowed as its own candidate: among identical songs BUILD would take song 0 again
    same = euclid(equal_input(40))
    assert contract_build(same, 3) == [0, 1, 2] and contract_build(same, 3, medoid_candidates=True) == [0, 0, 0]
    # the order of the sums: a hand-made input on which ascending and descending o differ
    x, near, d1b, k = order_sensitive_input()
    Dx = euclid(x)
    zero, inf = np.zeros(302, F32), np.full(302, np.inf, F32)
    up, down = contract_scan(Dx, near, zero, inf, k), contract_scan(Dx, near, zero, inf, k, order="descending")
    assert up[3][0, 0] == 2.0 ** 60 and down[3][0, 0] == 2.0 ** 60 + 256 and not np.array_equal(bits64(up[3]), bits64(down[3]))
    up, down = contract_scan(Dx, near, d1b, inf, k), contract_scan(Dx, near, d1b, inf, k, order="descending")
    assert not np.array_equal(bits64(up[4]), bits64(down[4])) and not np.array_equal(bits64(up[0]), bits64(down[0]))
    assert want[6]


# ---- the surface ----
def test_pam_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    assert "DESIGN.md 3.33" in header
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    lib = C.CDLL(bliss.LIB_PATH)
    for name in ("blissgpu_pam_scan", "blissgpu_kmedoids"):
        assert re.search(r"\bint\s+%s\s*\(" % name, flat), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name
    assert not re.search(r"blissgpu_(pam|kmedoids)\w*_device", header)
    assert not hasattr(lib, "blissgpu_kmedoids_device") and not hasattr(lib, "blissgpu_pam_scan_device")
    assert not hasattr(bliss.Context, "kmedoids") and not hasattr(bliss.Context, "pam_scan")  # host-pointer forms only

    def types(name):
        return [re.sub(r"\s*\b\w+$", "", " ".join(a.split())).replace(" *", "*")
                for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, flat).group(1).split(",")]

    assert types("blissgpu_pam_scan") == ["const float*", "uint64_t", "uint32_t", "const uint32_t*", "const float*", "const float*", "uint32_t",
                                          "int", "const float*", "const uint32_t*", "uint64_t", "double*", "double*", "uint32_t*", "double*",
                                          "double*"]
    assert types("blissgpu_kmedoids") == ["const float*", "uint64_t", "uint32_t", "uint32_t", "int", "const float*", "const uint32_t*", "uint32_t",
                                          "uint32_t*", "uint32_t*", "float*", "uint32_t*", "double*", "uint32_t*", "int32_t*"]
    assert _ffi.SIGNATURES["blissgpu_pam_scan"] == (C.c_int, [_vp, C.c_uint64, C.c_uint32, _vp, _vp, _vp, C.c_uint32, C.c_int, _vp, _vp,
                                                               C.c_uint64, _vp, _vp, _vp, _vp, _vp])
    assert _ffi.SIGNATURES["blissgpu_kmedoids"] == (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, _vp, _vp, C.c_uint32, _vp,
                                                               _vp, _vp, _vp, _vp, _vp, _vp])
    for name in ("pam_scan", "kmedoids", "Medoids", "medoid_songs"):
        assert hasattr(bliss.playlist, name), name
    assert hasattr(bliss.library, "medoid_songs")


def test_pam_kernels_are_in_the_profile_table(bliss):
    from bliss_rs_amd import _ffi

    L = _ffi.lib()
    names = [L.blissgpu_profile_kernel_name(k).decode() for k in range(L.blissgpu_profile_kernel_count())]
    assert len(set(names)) == len(names) and "" not in names
    src = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "kernels_pam.hip")).read()
    mine = ("pam_scan_kernel", "pam_fold_kernel", "pam_pick_kernel", "pam_gather_kernel", "pam_state_kernel", "pam_td_kernel")
    for name in mine:
        assert names.count(name) == 1, name
        assert re.search(r"\bvoid\s+%s\s*\(" % name, src), name
        assert names.index("ward_join_kernel") < names.index(name) < len(names) - 2
    assert sorted(n for n in names if n.startswith("pam_")) == sorted(mine)
    assert names[-2:] == ["group_forest_scan_kernel", "journey_step_kernel"]  # (older ids keep their places)
    make = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "Makefile")).read()
    assert re.search(r"kernels_pam\.o[^\n]*: EXTRA := \$\(NOCONTRACT\)", make)
    assert re.search(r"^OBJS\s*:=[^\n]*\bkernels_pam\.o", make, flags=re.M)
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomicAdd" not in code and "atomicMin" not in code  # no sum and no minimum is left to the order of arrival


def sort_needs(n, K):
    """(histogram words, scan totals) of the k-means counting sort of n songs into K slots (kmeans_plan of kernels_kmeans.hip:
    chunks of at least 256 songs, at most 2^21 / K of them, rounded to whole wavefronts; 2048-word scan tiles); K may be an array"""
    K = np.asarray(K, np.int64)
    W = np.maximum(1, np.minimum((n + 255) // 256, (1 << 21) // np.maximum(K, 1)))
    W = np.minimum(W, 1 << 20)
    chunk = np.maximum(1, -(-n // W))
    chunk = (chunk + 63) // 64 * 64
    W = np.maximum(1, -(-n // chunk))
    words = K * W
    return words, (words + 2047) // 2048


def _plan(n, d, k, q, build, limit=1 << 62):
    from bliss_rs_amd import _ffi

    plan = np.full(4, 7, np.uint64)
    rc = _ffi.lib().blissgpu_pam_plan(n, d, k, q, build, limit, plan.ctypes.data)
    return rc, [int(v) for v in plan]


def test_the_workspace_holds_the_sort_of_every_number_of_slots(bliss):
    """BUILD sorts K = 1 .. k slots, and the sort's table K * W is not monotone in K (W is capped at 2^21 / K and the chunks are
    rounded to 64 songs): the workspace reserves for the largest K, not for k.  No device is needed."""
    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    assert re.search(r"\bint\s+blissgpu_pam_plan\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    # where the table of k slots is NOT the largest
    words_k, _ = sort_needs(100000, 6000)
    words_K, _ = sort_needs(100000, 5363)
    assert (int(words_k), int(words_K)) == (1878000, 2096933)
    for n, k in ((100000, 6000), (1000000, 600), (100000, 65535), (1 << 22, 4096), (3000000, 1000), (300, 300), (257, 1), (70000, 40000),
                 (1, 1), (255, 255), (16385, 8191), (5000000, 65535)):
        Ks = np.arange(1, k + 1)
        words, tiles = sort_needs(n, Ks)
        rc, plan = _plan(n, 23, k, n, 1)
        assert rc == OK and plan[2] == int(words.max()) and plan[3] == int(tiles.max()), (n, k, plan, int(words.max()))
        assert plan[2] >= int(words[-1]) and plan[1] == n
        rc, scan = _plan(n, 23, k, 17, 0)  # a scan sorts k slots only
        assert rc == OK and scan[2] == int(words[-1]) and scan[3] == int(tiles[-1]) and scan[1] == 17
        # nothing else differs (up to the 8-byte alignment of A)
        assert abs(plan[0] - 16 * k * n - (scan[0] - 16 * k * 17) - 4 * ((plan[2] - scan[2]) + (plan[3] - scan[3]))) <= 4
    # the slab under a limit, and the limit below one candidate's share
    rc, plan = _plan(3000, 23, 64, 3000, 0, 1 << 20)
    assert rc == OK and plan[1] == 768 and plan[0] <= 1 << 20
    rc, plan = _plan(60000, 23, 4, 60000, 1, 1 << 20)
    assert rc == 4 and plan[1] == 0
    assert _plan(100, 0, 4, 100, 1)[0] == INVALID and _plan(100, 23, 0, 100, 1)[0] == INVALID


def _p(a):
    return None if a is None else a.ctypes.data


def _scan_call(x, n=None, d=None, k=2, metric=0, M=None, rows=None, q=0, null=(), near=None, d1=None, d2=None):
    from bliss_rs_amd import _ffi

    n = x.shape[0] if n is None else n
    d = x.shape[1] if d is None else d
    m = max(min(n, 4096), 2)
    ins = dict(near=np.zeros(m, np.uint32) if near is None else near, d1=np.zeros(m, F32) if d1 is None else d1,
               d2=np.ones(m, F32) if d2 is None else d2)
    out = dict(btot=np.full(m, 7.0), best=np.full(m, 7.0), arg=np.full(m, 7, np.uint32), A=np.full(m * k, 7.0), B=np.full(m * k, 7.0))
    L = _ffi.lib()
    rc = L.blissgpu_pam_scan(None if "x" in null else _p(x), n, d, *(None if w in null else _p(ins[w]) for w in ins), k, metric, _p(M),
                             _p(rows), q, *(None if w in null else _p(out[w]) for w in out))
    return rc, L.blissgpu_last_error(), out


def _kmedoids_call(x, n=None, d=None, k=2, metric=0, M=None, init=None, max_swaps=3, null=()):
    from bliss_rs_amd import _ffi

    n = x.shape[0] if n is None else n
    d = x.shape[1] if d is None else d
    m = max(min(n, 4096), 2)
    out = dict(medoids=np.full(max(k, 1), 7, np.uint32), labels=np.full(m, 7, np.uint32), dist=np.full(m, 7.0, F32),
               sizes=np.full(max(k, 1), 7, np.uint32), td_trace=np.full(max_swaps + 1, 7.0))
    swaps, conv = C.c_uint32(99), C.c_int32(99)
    L = _ffi.lib()
    rc = L.blissgpu_kmedoids(None if "x" in null else _p(x), n, d, k, metric, _p(M), _p(init), max_swaps,
                             *(None if w in null else _p(out[w]) for w in out), None if "n_swaps" in null else C.byref(swaps),
                             None if "converged" in null else C.byref(conv))
    return rc, L.blissgpu_last_error(), out, swaps.value, conv.value


def test_pam_arguments_are_checked_before_the_device(bliss):
    import torch

    X = planted_labelled(300)[0][:50]
    M = np.eye(23, dtype=F32)
    untouched = lambda out: all((a == 7).all() for a in out.values())
    for call in (_scan_call, _kmedoids_call):
        rc, err, out = call(X, d=0)[:3]
        assert rc == INVALID and b"d must be" in err and untouched(out)
        rc, err = call(np.zeros((50, 65), F32))[:2]
        assert rc == INVALID and b"d must be" in err
        rc, err = call(X, metric=3)[:2]
        assert rc == INVALID and b"metric" in err
        assert call(X, metric=-1)[0] == INVALID
        rc, err = call(X, metric=2)[:2]  # mahalanobis without M
        assert rc == INVALID and b"M" in err
        rc, err = call(X, k=0)[:2]
        assert rc == INVALID and b"k must be" in err
        rc, err = call(X, k=65536)[:2]
        assert rc == INVALID and b"k must be" in err
        rc, err, out = call(X, n=(1 << 32) - 1)[:3]
        assert rc == INVALID and b"n must be" in err and untouched(out)
    for what in ("x", "near", "d1", "d2", "btot", "best", "arg"):
        rc, err, out = _scan_call(X, null=(what,))
        assert rc == INVALID and what.encode() in err and untouched(out), what
    for what in ("x", "medoids", "labels", "td_trace", "n_swaps", "converged"):
        rc, err, out = _kmedoids_call(X, null=(what,))[:3]
        assert rc == INVALID and what.encode() in err and untouched(out), what
    # what is wrong with the state, the rows and the start is found on the host
    near = np.zeros(50, np.uint32)
    near[17] = 2
    rc, err, out = _scan_call(X, near=near)
    assert rc == INVALID and b"near" in err and untouched(out)
    bad = np.zeros(50, F32)
    bad[31] = np.nan
    rc, err, out = _scan_call(X, d1=bad)
    assert rc == INVALID and b"d1" in err and untouched(out)
    rc, err, out = _scan_call(X, d2=bad)
    assert rc == INVALID and b"d2" in err and untouched(out)
    rc, err, out = _scan_call(X, rows=np.asarray([3, 50], np.uint32), q=2)
    assert rc == INVALID and b"rows" in err and untouched(out)
    rc, err, out = _scan_call(X, rows=np.asarray([3], np.uint32), q=(1 << 32) - 1)
    assert rc == INVALID and b"q must be" in err and untouched(out)
    rc, err, out = _kmedoids_call(X, k=51)[:3]
    assert rc == INVALID and b"k must be at most n" in err and untouched(out)
    rc, err, out = _kmedoids_call(X, init=np.asarray([4, 50], np.uint32))[:3]
    assert rc == INVALID and b"init" in err and untouched(out)
    rc, err, out = _kmedoids_call(X, k=3, init=np.asarray([4, 9, 4], np.uint32))[:3]
    assert rc == INVALID and b"init" in err and b"twice" in err and untouched(out)
    # nothing to do: OK without a device, nothing written (NULL pointers are fine then)
    rc, _, out = _scan_call(X, n=0, null=("x", "near", "d1", "d2", "btot", "best", "arg", "A", "B"))
    assert rc == OK
    rc, _, out = _scan_call(X, rows=np.zeros(1, np.uint32), q=0)
    assert rc == OK and untouched(out)
    rc, _, out, swaps, conv = _kmedoids_call(X, n=0, null=("x", "medoids", "labels", "dist", "sizes", "td_trace"))
    assert rc == OK and swaps == 0 and conv == 1
    # a valid call: BLISSGPU_ERR_NO_DEVICE without a GPU, BLISSGPU_OK with one
    want = OK if torch.cuda.is_available() else NO_DEVICE
    assert _scan_call(X)[0] == want
    assert _scan_call(X, metric=1, null=("A", "B"))[0] == want
    assert _scan_call(X, metric=2, M=M, null=("A",))[0] == want
    assert _kmedoids_call(X)[0] == want
    assert _kmedoids_call(X, metric=1, null=("dist", "sizes"))[0] == want
    assert _kmedoids_call(X, metric=2, M=M, init=np.asarray([7, 3], np.uint32))[0] == want


# ---- the Python layer ----
def test_pam_refuses_forests_variance_weights_and_callables(bliss):
    P, Lb = bliss.playlist, bliss.library
    X = planted_labelled(300)[0][:12]
    for builder, exc in ((P.ForestOptions(10, 8, 3, 0), ValueError), (P.VarianceWeights(), ValueError), (lambda a, b: 0.0, TypeError)):
        for call in (lambda b: P.kmedoids(X, 3, b), lambda b: P.pam_scan(X, np.zeros(12, int), np.zeros(12), np.ones(12), 1, b),
                     lambda b: P.medoid_songs([], 3, b), lambda b: Lb.medoid_songs("/nowhere/at/all.db", 3, b)):  # before the database is read
            with pytest.raises(exc):
                call(builder)
    assert P._pam_metric(P.cosine_distance) == ("cosine", None) and P._pam_metric(P.euclidean_distance) == ("euclidean", None)
    name, m = P._pam_metric(P.MahalanobisBuilder(np.eye(23, dtype=F32)))
    assert name == "mahalanobis" and m.shape == (23, 23)
    with pytest.raises(ValueError):
        P.kmedoids(X, 13)
    with pytest.raises(ValueError):
        P.kmedoids(X, 0)
    with pytest.raises(ValueError):
        P.kmedoids(X, 3, init="random")
    with pytest.raises(ValueError):
        P.kmedoids(X, 3, init=[1, 2])
    with pytest.raises(ValueError):
        P.kmedoids(X, 3, max_swaps=-1)
    with pytest.raises(ValueError):
        P.pam_scan(X, np.zeros(11, int), np.zeros(12), np.ones(12), 1)
    with pytest.raises(ValueError):
        P.medoid_songs([], 3)


def test_medoids_members(bliss):
    P = bliss.playlist
    res = P.Medoids(np.asarray([4, 1]), np.asarray([0, 1, 1, 0, 0, 1]), np.asarray([2.0, 0.0, 1.0, 2.0, 0.0, 0.5], F32), np.asarray([3, 3]), 5.5,
                    np.asarray([6.0, 5.5]), 1, True)
    assert res.members(0).tolist() == [4, 0, 3] and res.members(1).tolist() == [1, 5, 2]


def test_library_medoid_songs(bliss, monkeypatch, tmp_path):
    """the database side, with the device call replaced by the contract"""
    P, Lb = bliss.playlist, bliss.library
    rng = np.random.default_rng(23)
    V2 = bliss.FeaturesVersion.Version2
    songs = []
    for i in range(60):
        x = (3.0 * (i % 4) + 0.3 * rng.standard_normal(23)).astype(F32)
        songs.append(bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist="a", album="b", disc_number=1, track_number=i,
                                duration=1.0, genre=["a", "b"][i % 2], analysis=bliss.Analysis(x, V2), features_version=V2))
    db = str(tmp_path / "bliss.db")
    Lb.create_schema(db)
    Lb.store_songs(db, songs)
    seen = []

    def fake(X, k, metric_builder=P.euclidean_distance, init="build", max_swaps=None):
        seen.append((X.shape, k, metric_builder))
        Dm = cosine(X) if metric_builder is P.cosine_distance else euclid(X)
        med, labels, dist, sizes, trace, swaps, conv, _ = contract_kmedoids(Dm, k)
        return P.Medoids(med, labels, dist, sizes, float(trace[-1]), trace, swaps, conv)

    monkeypatch.setattr(P, "kmedoids", fake)
    reps, clusters = Lb.medoid_songs(db, 4)
    assert seen == [((60, 23), 4, P.euclidean_distance)]
    assert len(reps) == 4 and sorted(len(c) for c in clusters) == [15] * 4
    for rep, cluster in zip(reps, clusters):
        assert cluster[0].path == rep.path and len({int(s.path[7:10]) % 4 for s in cluster}) == 1
    reps, clusters, res = Lb.medoid_songs(db, 2, P.cosine_distance, where=("genre", "a"), return_medoids=True)
    assert seen[-1] == ((30, 23), 2, P.cosine_distance) and res.converged and sum(len(c) for c in clusters) == 30
    assert all(s.genre == "a" for c in clusters for s in c)
    with pytest.raises(ValueError):
        Lb.medoid_songs(db, 2, where=("genre", "nothing"))
