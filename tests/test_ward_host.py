"""Device-free tests of Ward clustering (blissgpu_ward / blissgpu_ward_nearest): the contract of include/blissgpu.h written out in
numpy (`contract_nearest`, `contract_tree`, which the GPU tests compare the device with) against scipy's Ward linkage and against
its own mutations, ward_merge.hpp as a stand-alone program (plain and under sanitizers), the C ABI surface, the kernels' names in
the profile table, the argument checks that happen before the device is touched, and the host-side parts of the Python layer."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_ward_merge.cpp")
HPP = os.path.join(ROOT, "bliss-rs_amd", "csrc", "ward_merge.hpp")
SAN_CXX = "/opt/rocm/lib/llvm/bin/clang++"
_vp = C.c_void_p
OK, NO_DEVICE, INVALID = 0, 1, 2
WARD_OK = 0
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


# ---- the contract in numpy ----
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def euclid(X, block=256):
    """f32 euclidean distances as test_mst_host.euclid computes them (the same expression, taken in blocks of rows to bound the
    memory; for the host tests only: the GPU tests take the device's all-pairs matrix)"""
    X = np.asarray(X, np.float32)
    out = np.empty((X.shape[0], X.shape[0]), np.float32)
    for i in range(0, X.shape[0], block):
        diff = X[i:i + block, None, :] - X[None, :, :]
        out[i:i + block] = np.sqrt((diff * diff).sum(axis=2, dtype=np.float32)).astype(np.float32)
    return out


def euclid_seq(X):
    """the same distances with the sum taken feature by feature in ascending order: what tests/cpp/test_ward_merge.cpp computes"""
    X = np.asarray(X, np.float32)
    acc = np.zeros((X.shape[0], X.shape[0]), np.float32)
    for k in range(X.shape[1]):
        diff = X[:, None, k] - X[None, :, k]
        acc = acc + diff * diff
    return np.sqrt(acc)


def pair_costs(Dm, sizes=None, weight="contract"):
    """cost [m, m] f32 = (dist * dist) * w, w = (s_i * s_j) / (s_i + s_j), every operation rounded in f32; a NaN off the diagonal
    is refused as the library refuses it"""
    Dm = np.asarray(Dm, np.float32)
    m = Dm.shape[0]
    s = np.ones(m, np.float32) if sizes is None else np.asarray(sizes).astype(np.float32)
    si, sj = s[:, None], s[None, :]
    if weight == "contract":
        w = (si * sj) / (si + sj)
    else:  # a mutation: the same number before rounding, other roundings
        w = si / (si + sj) * sj
    cost = ((Dm * Dm) * w).astype(np.float32)
    if np.isnan(cost[~np.eye(m, dtype=bool)]).any():
        raise ValueError("NaN cost")
    return cost


def contract_nearest(Dm, sizes=None, tie="xor", weight="contract"):
    """-> (nn int64 [m], cost f32 [m]): per position the j != i with the smallest key (bits(cost) << 32) | (i XOR j)"""
    cost = pair_costs(Dm, sizes, weight)
    m = cost.shape[0]
    if m == 1:
        return np.array([-1], np.int64), np.array([np.inf], np.float32)
    idx = np.arange(m, dtype=np.uint64)
    low = (idx[:, None] ^ idx[None, :]) if tie == "xor" else np.broadcast_to(idx[None, :], (m, m))  # "lower": a mutation
    key = (bits(cost).astype(np.uint64) << np.uint64(32)) | low
    key[np.arange(m), np.arange(m)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    nn = key.argmin(axis=1)
    return nn.astype(np.int64), cost[np.arange(m), nn]


def contract_tree(X, dist_fn=euclid, tie="xor", update="f64", weight="contract", trace=None):
    """the rounds of include/blissgpu.h -> (u, v int64 [n - 1], cost f32 [n - 1], size, round int64 [n - 1], rounds).
    dist_fn(rows) gives the f32 matrix of the current rows (the GPU tests pass the device's).  trace: a list that receives
    (positions, pairs) per round."""
    Cr = np.array(X, np.float32)
    n = Cr.shape[0]
    size, low = np.ones(n, np.int64), np.arange(n, dtype=np.int64)
    edges, r = [], 0
    while Cr.shape[0] > 1:
        m = Cr.shape[0]
        nn, cost = contract_nearest(dist_fn(Cr), size, tie, weight)
        p = np.flatnonzero((nn[nn] == np.arange(m)) & (np.arange(m) < nn))
        assert len(p) >= 1, "a round merged nothing"
        q = nn[p]
        if trace is not None:
            trace.append((m, len(p)))
        cb = bits(cost)
        for a, b in zip(p.tolist(), q.tolist()):
            edges.append((int(cb[a]), r, int(low[a]), int(low[b]), int(size[a] + size[b])))
        if update == "f64":
            sp, sq = size[p].astype(np.float64)[:, None], size[q].astype(np.float64)[:, None]
            Cr[p] = ((sp * Cr[p].astype(np.float64) + sq * Cr[q].astype(np.float64)) / (size[p] + size[q]).astype(np.float64)[:, None]).astype(np.float32)
        else:  # a mutation: the same expression rounded in f32
            sp, sq = size[p].astype(np.float32)[:, None], size[q].astype(np.float32)[:, None]
            Cr[p] = (sp * Cr[p] + sq * Cr[q]) / (sp + sq)
        size[p] += size[q]
        keep = np.ones(m, bool)
        keep[q] = False
        Cr, size, low = Cr[keep], size[keep], low[keep]
        r += 1
    edges.sort(key=lambda e: e[:3])
    col = lambda k: np.asarray([e[k] for e in edges], np.int64)
    return col(2), col(3), col(0).astype(np.uint32).view(np.float32), col(4), col(1), r


def same_tree(a, b):
    return (all(np.array_equal(a[k], b[k]) for k in (0, 1, 3, 4)) and np.array_equal(bits(a[2]), bits(b[2])) and a[5] == b[5])


def planted(n):
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, 23)).astype(np.float32)
    lab = rng.integers(0, 8, n)
    X += (lab[:, None] == np.arange(8)).astype(np.float32) @ rng.standard_normal((8, 23)).astype(np.float32) * 3
    return X


def equal_input(n=300, d=23):
    return np.full((n, d), 0.375, np.float32)


def twice_input(n=200, d=23, seed=4):
    """every row appears twice"""
    rng = np.random.default_rng(seed)
    half = rng.standard_normal((n // 2, d)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([half, half])[rng.permutation(n)])


def grid_input(n=600, d=23, seed=3):
    """points on an integer grid in 3 of the d dimensions: thousands of equal costs"""
    rng = np.random.default_rng(seed)
    X = np.zeros((n, d), np.float32)
    X[:, [2, 9, 17][:min(3, d)]] = rng.integers(0, 7, (n, min(3, d))).astype(np.float32)
    return X


def cut_labels(n, u, v, k):
    """labels of the k clusters left when the k - 1 last merges are undone, by union-find"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(u[:n - k].tolist(), v[:n - k].tolist()):
        ra, rb = find(a), find(b)
        parent[max(ra, rb)] = min(ra, rb)
    return np.asarray([find(i) for i in range(n)], np.int64)


def same_partition(a, b):
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


def inversions(tree):
    """merges cheaper than one of their children, counted in the order the rounds emitted them"""
    u, v, cost, _, rnd, _ = tree
    last = {}
    bad = 0
    for e in np.lexsort((u, rnd)).tolist():
        c = float(cost[e])
        if c < max(last.get(int(u[e]), 0.0), last.get(int(v[e]), 0.0)):
            bad += 1
        last[int(u[e])] = c  # (the merged cluster's lowest member is u)
    return bad


_TREES = {}


def planted_tree(n):
    if n not in _TREES:
        trace = []
        _TREES[n] = (contract_tree(planted(n), trace=trace), trace)
    return _TREES[n]


# ---- properties of the contract itself ----
def test_the_contract_is_a_whole_tree():
    for n in (2, 3, 5, 300):
        X = planted(n)
        u, v, cost, size, rnd, rounds = tree = contract_tree(X) if n != 300 else planted_tree(300)[0]
        assert len(u) == n - 1 and (u < v).all() and size[-1] == n and size.max() == n
        key = list(zip(bits(cost).tolist(), rnd.tolist(), u.tolist()))
        assert key == sorted(key) and len(set(key)) == n - 1
        assert rnd.max() == rounds - 1 and set(rnd.tolist()) == set(range(rounds))  # every round merges at least one pair
        assert inversions(tree) == 0
    two = contract_tree(planted(300)[:2])
    assert two[0].tolist() == [0] and two[1].tolist() == [1] and two[3].tolist() == [2] and two[5] == 1
    d01 = euclid(planted(300)[:2])[0, 1]
    assert bits(two[2])[0] == bits((d01 * d01) * np.float32(0.5))[()]
    for n in (0, 1):
        assert len(contract_tree(planted(5)[:n])[0]) == 0
    with pytest.raises(ValueError):
        bad = planted(20)
        bad[3, 7] = np.nan
        contract_tree(bad)


def test_the_contract_nearest_rule():
    X = planted(300)[:40]
    Dm = euclid(X)
    sizes = np.random.default_rng(1).integers(1, 5001, 40)
    nn, cost = contract_nearest(Dm, sizes)
    full = pair_costs(Dm, sizes)
    assert np.array_equal(bits(full), bits(full.T))  # cost(i, j) and cost(j, i): the same bits
    np.fill_diagonal(full, np.inf)
    assert np.array_equal(nn, full.argmin(axis=1)) and np.array_equal(bits(cost), bits(full.min(axis=1)))  # (tie-free data)
    # four equal rows: 0 <-> 1 and 2 <-> 3 under XOR, everything at 0 (and 0 at 1) under "lower index"
    eq = euclid(equal_input(4))
    assert contract_nearest(eq)[0].tolist() == [1, 0, 3, 2]
    assert contract_nearest(eq, tie="lower")[0].tolist() == [1, 0, 0, 0]
    one = contract_nearest(np.zeros((1, 1), np.float32))
    assert one[0].tolist() == [-1] and np.isinf(one[1][0])


def test_equal_and_double_rows_pair_up_like_a_trie():
    trace = []
    tree = contract_tree(equal_input(300), trace=trace)
    assert tree[5] == 9 and len(trace) == 9 and not bits(tree[2]).any()  # = ceil(log2 300)
    assert [m for m, _ in trace] == [300, 150, 75, 38, 19, 10, 5, 3, 2]
    # every row twice: the 100 doubles merge first, at cost +0
    tw = contract_tree(twice_input())
    assert int((bits(tw[2]) == 0).sum()) == 100 and (tw[4][:100] == 0).all() and (tw[3][:100] == 2).all()
    # the tie rule decides: "lower index" needs a round per equal row
    slow = contract_tree(equal_input(40), tie="lower")
    fast = contract_tree(equal_input(40))
    assert slow[5] == 39 and fast[5] == 6 and not same_tree(slow, fast)
    assert inversions(contract_tree(grid_input(200))) == 0


@pytest.mark.parametrize("n", [300, 1000, 3000])
def test_the_contract_against_scipy_ward(n):
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    tree, trace = planted_tree(n)
    u, v, cost, size, rnd, rounds = tree
    pairs = sum(m * (m - 1) for m, _ in trace) / float(n * n)
    print(f"n = {n}: {rounds} rounds, {pairs:.2f} n^2 pairs")
    assert rounds == {300: 20, 1000: 28, 3000: 41}[n]  # what the issue's replay of the same rounds measured
    assert all(k >= 1 for _, k in trace) and inversions(tree) == 0
    Z = hierarchy.linkage(planted(n).astype(np.float64), "ward")
    for K in (2, 8, 20, 100):
        assert same_partition(cut_labels(n, u, v, K), hierarchy.fcluster(Z, K, "maxclust")), K
    # the heights: sqrt(2 cost) in f64 against scipy's f64 column.  The costs are f32 (u = 2^-24 = 6e-8 per operation: the sum of
    # 23 squares, the root, the square, the weight, the product, on centroids rounded to f32 at every merge); the root halves
    # the relative error.  The numpy contract measures 2.8e-7 here; the bound is 1e-6 = 16 u
    h = np.sqrt(2.0 * cost.astype(np.float64))
    rel = float(np.max(np.abs(h - Z[:, 2]) / Z[:, 2]))
    print(f"n = {n}: heights against scipy: {rel:.3g} relative (bound 1e-6)")
    assert rel <= 1e-6


def test_the_expectation_moves_with_every_clause():
    """the tie rule, the f64 centroid update and the order of the weight's operations all reach the tree's bits: a device that
    got one of them wrong could not pass the GPU tests"""
    X = planted(300)
    want = planted_tree(300)[0]
    assert same_tree(want, contract_tree(X))
    f32 = contract_tree(X, update="f32")
    assert not np.array_equal(bits(want[2]), bits(f32[2]))
    other_w = contract_tree(X, weight="other")
    assert not np.array_equal(bits(want[2]), bits(other_w[2]))
    sizes = np.random.default_rng(2).integers(1, 5001, 300)
    a, b = contract_nearest(euclid(X), sizes), contract_nearest(euclid(X), sizes, weight="other")
    assert not np.array_equal(bits(a[1]), bits(b[1]))
    assert contract_tree(equal_input(64), tie="lower")[5] == 63 and contract_tree(equal_input(64))[5] == 6


# ---- ward_merge.hpp as a stand-alone program ----
def _run_program(exe, tmp, name, X, env=None):
    n, d = X.shape
    fin, fout = str(tmp / f"{name}.in"), str(tmp / f"{name}.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<II", n, d))
        f.write(np.ascontiguousarray(X, np.float32).tobytes())
    out = subprocess.run([str(exe), fin, fout], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, (name, out.stdout[-500:], out.stderr[-3000:])
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, (name, out.stderr[-3000:])
    raw = open(fout, "rb").read()
    status, rounds = struct.unpack_from("<iI", raw, 0)
    m = max(n - 1, 0)
    u, v, c, s, r = (np.frombuffer(raw, np.uint32, m, 8 + 4 * m * k) for k in range(5))
    return status, (u.astype(np.int64), v.astype(np.int64), c.view(np.float32), s.astype(np.int64), r.astype(np.int64), rounds)


_WANT = {}


def _check_program(exe, tmp, env=None):
    out = subprocess.run([str(exe), "--direct"], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    cases = {"equal300": equal_input(300), "twice": twice_input(), "grid": grid_input(200), "equal7": equal_input(7, 5)}
    for n in (1, 2, 3, 64, 257):
        cases[f"planted{n}"] = planted(300)[:n]
    cases["d7"] = np.random.default_rng(7).standard_normal((100, 7)).astype(np.float32)
    for name, X in cases.items():
        if name not in _WANT:
            _WANT[name] = contract_tree(X, dist_fn=euclid_seq)  # (computed once for the plain and the sanitizer build)
        status, tree = _run_program(exe, tmp, name, X, env)
        assert status == WARD_OK and same_tree(tree, _WANT[name]), name
    assert _WANT["equal300"][5] == 9


def test_ward_merge_header_against_the_contract(tmp_path):
    exe = tmp_path / "test_ward_merge"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", SRC, "-o", str(exe)])
    _check_program(exe, tmp_path)


@pytest.mark.skipif(not os.path.exists(SAN_CXX), reason="needs the ROCm clang for -fsanitize=address,undefined")
def test_ward_merge_header_under_address_and_ub_sanitizer(tmp_path):
    """the same stand-alone program built with -fsanitize=address,undefined: same trees, exit 0, no report"""
    exe = tmp_path / "test_ward_merge_san"
    subprocess.check_call([SAN_CXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", SRC, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    _check_program(exe, tmp_path, env)


def test_ward_merge_header_is_device_free():
    code = re.sub(r"//[^\n]*", "", open(HPP).read())
    assert "hip" not in code.lower() and "float" not in code and "double" not in code
    assert re.findall(r"#include\s+[<\"]([^>\"]+)", code) == ["stdint.h", "algorithm", "vector"]


# ---- the surface ----
def test_ward_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    assert "DESIGN.md 3.32" in header
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    lib = C.CDLL(bliss.LIB_PATH)
    for name in ("blissgpu_ward", "blissgpu_ward_nearest"):
        assert re.search(r"\bint\s+%s\s*\(" % name, flat), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name
    assert not re.search(r"blissgpu_ward\w*_device", header) and not hasattr(lib, "blissgpu_ward_device")
    assert not hasattr(bliss.Context, "ward") and not hasattr(bliss.Context, "ward_tree")  # host-pointer forms only

    def types(name):
        return [re.sub(r"\s*\b\w+$", "", " ".join(a.split())).replace(" *", "*")
                for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, flat).group(1).split(",")]

    assert types("blissgpu_ward_nearest") == ["const float*", "const uint32_t*", "uint64_t", "uint32_t", "int", "const float*", "uint32_t*", "float*"]
    assert types("blissgpu_ward") == ["const float*", "uint64_t", "uint32_t", "int", "const float*", "uint32_t*", "uint32_t*", "float*",
                                      "uint32_t*", "uint32_t*", "uint32_t*"]
    assert _ffi.SIGNATURES["blissgpu_ward_nearest"] == (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, _vp])
    assert _ffi.SIGNATURES["blissgpu_ward"] == (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
    for name in ("ward_nearest", "ward_tree", "WardTree", "choose_k_tree"):
        assert hasattr(bliss.playlist, name), name
    for name in ("ward_tree", "ward_clusters"):
        assert hasattr(bliss.library, name), name


def test_ward_kernels_are_in_the_profile_table(bliss):
    from bliss_rs_amd import _ffi

    L = _ffi.lib()
    names = [L.blissgpu_profile_kernel_name(k).decode() for k in range(L.blissgpu_profile_kernel_count())]
    assert len(set(names)) == len(names) and "" not in names
    src = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "kernels_ward.hip")).read()
    mine = ("ward_scan_kernel", "ward_join_kernel")
    for name in mine:
        assert names.count(name) == 1, name
        assert re.search(r"\bvoid\s+%s\s*\(" % name, src), name
        assert names.index(name) < len(names) - 2
    assert sorted(n for n in names if n.startswith("ward_")) == sorted(mine)
    assert names[-2:] == ["group_forest_scan_kernel", "journey_step_kernel"]  # (older ids keep their places)
    make = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "Makefile")).read()
    assert re.search(r"kernels_ward\.o[^\n]*: EXTRA := \$\(NOCONTRACT\)", make)


def _p(a):
    return None if a is None else a.ctypes.data


def _tree_call(x, n=None, d=None, metric=0, M=None, null=(), rounds=True):
    from bliss_rs_amd import _ffi

    n = x.shape[0] if n is None else n
    d = x.shape[1] if d is None else d
    m = max(min(n, 4096), 2)
    out = dict(edge_u=np.full(m, 7, np.uint32), edge_v=np.full(m, 7, np.uint32), edge_cost=np.full(m, 7.0, np.float32),
               edge_size=np.full(m, 7, np.uint32), edge_round=np.full(m, 7, np.uint32))
    r = C.c_uint32(99)
    L = _ffi.lib()
    rc = L.blissgpu_ward(None if "x" in null else _p(x), n, d, metric, _p(M), *(None if k in null else _p(out[k]) for k in out),
                         C.byref(r) if rounds else None)
    return rc, L.blissgpu_last_error(), out, r.value


def _nearest_call(c, size=None, m=None, d=None, metric=0, M=None, null=()):
    from bliss_rs_amd import _ffi

    m = c.shape[0] if m is None else m
    d = c.shape[1] if d is None else d
    k = max(min(m, 4096), 2)
    out = dict(nn=np.full(k, 7, np.uint32), cost=np.full(k, 7.0, np.float32))
    L = _ffi.lib()
    rc = L.blissgpu_ward_nearest(None if "c" in null else _p(c), _p(size), m, d, metric, _p(M), *(None if k in null else _p(out[k]) for k in out))
    return rc, L.blissgpu_last_error(), out


def test_ward_arguments_are_checked_before_the_device(bliss):
    import torch

    X = planted(300)[:50]
    M = np.eye(23, dtype=np.float32)
    untouched = lambda out: all((a == 7).all() for a in out.values())
    for call in (_tree_call, _nearest_call):
        rc, err = call(X, d=0)[:2]
        assert rc == INVALID and b"d must be" in err
        rc, err = call(np.zeros((50, 65), np.float32))[:2]
        assert rc == INVALID and b"d must be" in err
        rc, err = call(X, metric=3)[:2]
        assert rc == INVALID and b"metric" in err
        assert call(X, metric=-1)[0] == INVALID
        rc, err = call(X, metric=1)[:2]
        assert rc == INVALID and b"cosine" in err
        rc, err = call(X, metric=2)[:2]  # mahalanobis without M
        assert rc == INVALID and b"M" in err
    rc, err, out, _ = _tree_call(X, n=1 << 24)
    assert rc == INVALID and b"2^24" in err and untouched(out)
    rc, err, out = _nearest_call(X, m=1 << 24)
    assert rc == INVALID and b"2^24" in err and untouched(out)
    for what in ("x", "edge_u", "edge_v", "edge_cost"):
        rc, err, out, _ = _tree_call(X, null=(what,))
        assert rc == INVALID and what.encode() in err and untouched(out), what
    for what in ("c", "nn", "cost"):
        rc, err, out = _nearest_call(X, null=(what,))
        assert rc == INVALID and what.encode() in err and untouched(out), what
    sizes = np.full(50, 3, np.uint32)
    sizes[17] = 0
    rc, err, out = _nearest_call(X, sizes)
    assert rc == INVALID and b"size" in err and untouched(out)
    sizes[:] = (1 << 24) // 50 + 1
    rc, err, out = _nearest_call(X, sizes)
    assert rc == INVALID and b"2^24" in err and untouched(out)
    # no edge: OK without a device, nothing written, no round (NULL pointers are fine then)
    for n in (0, 1):
        rc, _, out, rounds = _tree_call(X, n=n)
        assert rc == OK and rounds == 0 and untouched(out)
        assert _tree_call(X, n=n, null=("x", "edge_u", "edge_v", "edge_cost", "edge_size", "edge_round"), rounds=False)[0] == OK
    rc, _, out = _nearest_call(X, m=0, null=("c", "nn", "cost"))
    assert rc == OK
    rc, _, out = _nearest_call(X, m=1, null=("c",))
    assert rc == OK and out["nn"][0] == NONE and np.isinf(out["cost"][0]) and out["nn"][1] == 7 and out["cost"][1] == 7
    # a valid call: BLISSGPU_ERR_NO_DEVICE without a GPU, BLISSGPU_OK with one
    want = OK if torch.cuda.is_available() else NO_DEVICE
    assert _tree_call(X)[0] == want
    assert _tree_call(X, metric=2, M=M, null=("edge_size", "edge_round"), rounds=False)[0] == want
    assert _nearest_call(X)[0] == want
    assert _nearest_call(X, np.full(50, 3, np.uint32))[0] == want


# ---- the Python layer ----
def _tree_of(P, t):
    return P.WardTree(t[0], t[1], t[2], t[3], t[4], t[5], len(t[0]) + 1)


def test_ward_refuses_what_the_spanning_tree_refuses(bliss):
    P = bliss.playlist
    X = planted(300)[:12]
    for builder, word in ((P.cosine_distance, "cosine"), ("cosine", "cosine"), (P.ForestOptions(10, 8, 3, 0), "forest"),
                          (P.VarianceWeights(), "MahalanobisBuilder")):
        for call in (lambda b: P.ward_tree(X, b), lambda b: P.ward_nearest(X, None, b),
                     lambda b: P.choose_k_tree(X, _tree_of(P, contract_tree(X)), [2, 3], b)):
            with pytest.raises(ValueError) as e:
                call(builder)
            assert word in str(e.value)
    with pytest.raises(TypeError):
        P.ward_tree(X, lambda a, b: 0.0)
    # no edge: no device is needed
    for n in (0, 1):
        t = P.ward_tree(X[:n])
        assert t.n == n and len(t.u) == 0 and t.u.dtype == np.int64 and t.cost.dtype == np.float32 and t.rounds == 0
        assert t.cut().tolist() == [0] * n and t.linkage().shape == (0, 4) and t.within().shape == (0,)
    nn, cost = P.ward_nearest(X[:1])
    assert nn.tolist() == [-1] and nn.dtype == np.int64 and np.isinf(cost[0]) and cost.dtype == np.float32
    with pytest.raises(ValueError):
        P.ward_nearest(X, np.ones(5))
    with pytest.raises(ValueError):
        P.choose_k_tree(X, _tree_of(P, contract_tree(X)), [1, 2])
    with pytest.raises(ValueError):
        P.choose_k_tree(X[:5], _tree_of(P, contract_tree(X)), [2])
    # errors of the C layer arrive as BlissGpuError(ERR_INVALID) before a device is needed
    with pytest.raises(bliss.BlissGpuError) as e:
        P.ward_tree(np.zeros((5, 65), np.float32))
    assert e.value.code == INVALID
    with pytest.raises(bliss.BlissGpuError) as e:
        P.ward_nearest(X, np.zeros(12))
    assert e.value.code == INVALID


def test_ward_tree_cut_linkage_within(bliss):
    P = bliss.playlist
    # a hand-made tree over 6 songs: {0, 3} at 1, {1, 2} at 1 (a later round), {4, 5} at 2, {0, 3, 4, 5} at 4.5, all at 8
    t = P.WardTree(np.array([0, 1, 4, 0, 0]), np.array([3, 2, 5, 4, 1]), np.array([1, 1, 2, 4.5, 8], np.float32),
                   np.array([2, 2, 2, 4, 6]), np.array([0, 1, 0, 2, 3]), 4, 6)
    assert t.cut().tolist() == [0] * 6 and t.cut(1).tolist() == [0] * 6
    assert t.cut(2).tolist() == [0, 1, 1, 0, 0, 0]
    assert t.cut(3).tolist() == [0, 1, 1, 0, 2, 2]
    assert t.cut(4).tolist() == [0, 1, 1, 0, 2, 3]
    assert t.cut(6).tolist() == [0, 1, 2, 3, 4, 5]
    assert t.cut(cost=2.0).tolist() == [0, 1, 1, 0, 2, 2]  # a merge of exactly that cost stays
    assert t.cut(cost=float(np.nextafter(np.float32(2), np.float32(0)))).tolist() == [0, 1, 1, 0, 2, 3]
    assert t.cut(cost=np.inf).tolist() == [0] * 6 and t.cut(cost=-1.0).tolist() == list(range(6))
    assert t.cut(4, min_cluster_size=2).tolist() == [0, 1, 1, 0, -1, -1]
    assert t.cut(2, min_cluster_size=3).tolist() == [0, -1, -1, 0, 0, 0]
    for bad in (dict(k=0), dict(k=7), dict(k=2, cost=1.0)):
        with pytest.raises(ValueError):
            t.cut(**bad)
    # nested: the clusters of k are unions of the clusters of k + 1
    for k in range(1, 6):
        a, b = t.cut(k), t.cut(k + 1)
        assert len(set(zip(a.tolist(), b.tolist()))) == k + 1
    assert t.heights().dtype == np.float64 and np.array_equal(t.heights(), np.sqrt(2.0 * np.array([1, 1, 2, 4.5, 8])))
    assert t.within().tolist() == [1.0, 2.0, 4.0, 8.5, 16.5]
    Z = t.linkage()
    assert Z.dtype == np.float64 and Z.tolist() == [[0, 3, np.sqrt(2.0), 2], [1, 2, np.sqrt(2.0), 2], [4, 5, 2.0, 2], [6, 8, 3.0, 4], [7, 9, 4.0, 6]]


def test_ward_linkage_against_scipy(bliss):
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    P = bliss.playlist
    n = 300
    tree = planted_tree(n)[0]
    t = _tree_of(P, tree)
    Z = t.linkage()
    want = hierarchy.linkage(planted(n).astype(np.float64), "ward")
    assert Z.shape == want.shape and (Z[:, 0] < Z[:, 1]).all() and Z[-1, 3] == n
    assert np.allclose(Z[:, 2], want[:, 2], rtol=1e-6, atol=0) and np.array_equal(np.sort(Z[:, 3]), np.sort(want[:, 3]))
    for k in (1, 2, 8, 20, 100, n):
        a = hierarchy.fcluster(Z, k, "maxclust")
        assert same_partition(a, hierarchy.fcluster(want, k, "maxclust")) and same_partition(a, t.cut(k)) and len(set(a.tolist())) == k
    # within(): the within-cluster sum of squares after each merge, against the definition in f64
    X64 = planted(n).astype(np.float64)
    for k in (8, 100):
        lab = t.cut(k)
        wss = sum(((X64[lab == c] - X64[lab == c].mean(axis=0)) ** 2).sum() for c in range(k))
        assert abs(t.within()[n - k - 1] - wss) <= 1e-5 * wss


# ---- the library ----
def test_library_ward_clusters(bliss, monkeypatch, tmp_path):
    P, Lb = bliss.playlist, bliss.library
    rng = np.random.default_rng(22)
    centre = {"jazz": 0.0, "metal": 4.0, "folk": 9.0}
    names = ["jazz", "metal", "folk"]
    V2 = bliss.FeaturesVersion.Version2
    songs = []
    for i in range(41):
        x = (centre[names[i % 3]] + 0.05 * rng.standard_normal(23)).astype(np.float32)
        songs.append(bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist="a", album="b", disc_number=1, track_number=i,
                                duration=1.0, genre=names[i % 3], analysis=bliss.Analysis(x, V2), features_version=V2))
    db = str(tmp_path / "bliss.db")
    Lb.create_schema(db)
    Lb.store_songs(db, songs)
    calls = []

    def fake(songs_or_X, metric_builder=P.euclidean_distance):
        P._ward_metric(metric_builder)
        X = P._rows_of_input(songs_or_X)
        calls.append(X.shape[0])
        return _tree_of(P, contract_tree(X))

    monkeypatch.setattr(P, "ward_tree", fake)
    paths, tree = Lb.ward_tree(db)
    assert paths == [s.path for s in songs] and tree.n == 41 and len(tree.u) == 40 and calls == [41]
    paths, tree = Lb.ward_tree(db, where=("genre", "metal"))
    assert paths == [s.path for s in songs if s.genre == "metal"] and tree.n == len(paths) and calls[-1] == len(paths)
    lists, loose = Lb.ward_clusters(db, k=3)
    assert loose == [] and [len(c) for c in lists] == [14, 14, 13] and len(calls) == 3
    assert [c[0].path for c in lists] == ["/music/000.flac", "/music/001.flac", "/music/002.flac"]
    for c in lists:
        assert [s.path for s in c] == sorted(s.path for s in c) and len({s.genre for s in c}) == 1
    lists, loose = Lb.ward_clusters(db, cost=1.0, min_cluster_size=14)
    assert [len(c) for c in lists] == [14, 14] and len(loose) == 13
    assert Lb.ward_clusters(db, k=1, where=("genre", "nobody")) == ([], [])
    assert Lb.ward_tree(db, where=("genre", "nobody"))[1].n == 0
    n_calls = len(calls)
    for builder in (P.cosine_distance, P.ForestOptions(10, 8, 3, 0), P.VarianceWeights()):
        with pytest.raises(ValueError):
            Lb.ward_tree(db, metric_builder=builder)
        with pytest.raises(ValueError):
            Lb.ward_clusters(db, k=2, metric_builder=builder)
    with pytest.raises(ValueError):
        Lb.ward_tree(db, where=("title", "t1"))
    assert len(calls) == n_calls  # every refusal comes before the device
