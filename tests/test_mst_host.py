"""Device-free tests of the minimum spanning tree (blissgpu_mst / blissgpu_mst_device): the contract of include/blissgpu.h written
out in numpy (`contract` below, which the GPU tests compare the device with) against a second restatement, mst_merge.hpp as a
stand-alone program (plain and under sanitizers), the C ABI surface, the kernels' names in the profile table, the argument checks
that happen before the device is touched, and the host-side parts of the Python layer with the device call replaced by
`contract`."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_mst_merge.cpp")
HPP = os.path.join(ROOT, "bliss-rs_amd", "csrc", "mst_merge.hpp")
SAN_CXX = "/opt/rocm/lib/llvm/bin/clang++"
_vp = C.c_void_p
OK, NO_DEVICE, INVALID = 0, 1, 2
MST_OK = 0


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


def weights(Dm, core=None):
    """w [n, n] f32 = max(dist, core[i], core[j]); a NaN anywhere, or a negative weight, is refused as the library refuses it"""
    W = np.asarray(Dm, np.float32)
    if core is not None:
        core = np.asarray(core, np.float32)
        W = np.maximum(np.maximum(W, core[:, None]), core[None, :])
    off = ~np.eye(W.shape[0], dtype=bool)
    if np.isnan(W[off]).any() or (W[off] < 0).any():
        raise ValueError("NaN or negative weight")
    return W


def contract(Dm, core=None):
    """Kruskal over all pairs i < j of the f32 matrix Dm under the key (bits of w, i, j) -> (u int64 [n - 1], v int64 [n - 1],
    w f32 [n - 1]) in ascending key: THE minimum spanning tree (the order is strict and total)"""
    W = weights(Dm, core)
    n = W.shape[0]
    if n < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    iu, ju = np.triu_indices(n, 1)  # (row-major: ascending (i, j))
    wb = bits(W[iu, ju]).astype(np.int64)
    order = np.argsort(wb, kind="stable")  # ties keep ascending (i, j)
    iu, ju, wb = iu[order], ju[order], wb[order]
    parent = np.arange(n)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    eu, ev, ew = [], [], []
    pos, chunk = 0, 1024
    while len(eu) < n - 1:
        assert pos < len(iu)
        lab = np.fromiter((find(i) for i in range(n)), np.int64, n)
        a, b, c = iu[pos:pos + chunk], ju[pos:pos + chunk], wb[pos:pos + chunk]
        live = np.flatnonzero(lab[a] != lab[b])  # (an edge inside a component now stays inside one)
        for e in live:
            ra, rb = find(a[e]), find(b[e])
            if ra != rb:
                parent[rb] = ra
                eu.append(a[e]); ev.append(b[e]); ew.append(c[e])
        pos += chunk
        chunk *= 2
    return np.asarray(eu, np.int64), np.asarray(ev, np.int64), np.asarray(ew, np.int64).astype(np.uint32).view(np.float32)


def prim(Dm, core=None):
    """the second restatement: Prim from song 0, the next edge = the smallest key (bits of w, lower, higher) that leaves the
    tree; the edges sorted by key at the end"""
    W = weights(Dm, core)
    n = W.shape[0]
    wb = bits(W).astype(np.int64)
    inside = np.zeros(n, bool)
    inside[0] = True
    edges = []
    idx = np.arange(n)
    best_w, best_from = wb[0].copy(), np.zeros(n, np.int64)  # per outside song: its smallest key into the tree
    for _ in range(n - 1):
        lo, hi = np.minimum(idx, best_from), np.maximum(idx, best_from)
        cand = np.flatnonzero(~inside)
        j = cand[np.lexsort((hi[cand], lo[cand], best_w[cand]))[0]]
        edges.append((int(best_w[j]), int(lo[j]), int(hi[j])))
        inside[j] = True
        # song j joins: an outside song k switches to the edge {j, k} where its key is smaller
        nl, nh = np.minimum(idx, j), np.maximum(idx, j)
        better = (wb[j] < best_w) | ((wb[j] == best_w) & ((nl < lo) | ((nl == lo) & (nh < hi))))
        best_w = np.where(better, wb[j], best_w)
        best_from = np.where(better, j, best_from)
    edges.sort()
    w = np.asarray([e[0] for e in edges], np.int64).astype(np.uint32).view(np.float32)
    return np.asarray([e[1] for e in edges], np.int64), np.asarray([e[2] for e in edges], np.int64), w


def same_tree(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))


def euclid(X):
    """f32 euclidean distances in numpy (for the host tests only: the GPU tests take the device's all-pairs matrix)"""
    X = np.asarray(X, np.float32)
    diff = X[:, None, :] - X[None, :, :]
    return np.sqrt((diff * diff).sum(axis=2, dtype=np.float32)).astype(np.float32)


def core_of(Dm, m):
    """the distance to the m-th nearest other song, from a matrix"""
    D = np.array(Dm, np.float32)
    np.fill_diagonal(D, np.inf)
    return np.sort(D, axis=1)[:, min(m, D.shape[0] - 1) - 1].astype(np.float32)


# ---- the tie-heavy inputs (the GPU tests use the same) ----
def grid_input(n=1000, d=23, seed=3):
    """points on an integer grid in 3 of the d dimensions: thousands of equal distances"""
    rng = np.random.default_rng(seed)
    X = np.zeros((n, d), np.float32)
    X[:, [2, 9, 17][:min(3, d)]] = rng.integers(0, 7, (n, min(3, d))).astype(np.float32)
    return X


def twice_input(n=200, d=23, seed=4):
    """every row appears twice"""
    rng = np.random.default_rng(seed)
    half = rng.standard_normal((n // 2, d)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([half, half])[rng.permutation(n)])


def equal_input(n=300, d=23):
    return np.full((n, d), 0.375, np.float32)


def random_input(n, d=23, seed=5):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def tied_edge_pairs(W, tree):
    """pairs of distinct edges {i < j} that share their weight bits, counted at the weights the tree uses: what the tie-break
    had to decide"""
    n = W.shape[0]
    iu, ju = np.triu_indices(n, 1)
    values, counts = np.unique(bits(W[iu, ju]), return_counts=True)
    used = np.isin(values, np.unique(bits(tree[2])))
    c = counts[used].astype(np.int64)
    return int((c * (c - 1) // 2).sum())


def test_the_contract_against_a_second_restatement():
    X = random_input(200)
    Dm = euclid(X)
    tree = contract(Dm)
    assert same_tree(tree, prim(Dm))
    assert len(tree[0]) == 199 and (tree[0] < tree[1]).all()
    key = list(zip(bits(tree[2]).tolist(), tree[0].tolist(), tree[1].tolist()))
    assert key == sorted(key) and len(set(key)) == 199
    assert tied_edge_pairs(Dm, tree) == 0  # (random data is tie-free: what the bench tool's torch baseline relies on)
    # with cores: plateaus
    for m in (5, 50):
        core = core_of(Dm, m)
        assert same_tree(contract(Dm, core), prim(Dm, core))
    for n in (0, 1):
        assert len(contract(Dm[:n, :n])[0]) == 0
    two = contract(Dm[:2, :2])
    assert two[0].tolist() == [0] and two[1].tolist() == [1] and bits(two[2])[0] == bits(Dm[0, 1])
    with pytest.raises(ValueError):
        bad = Dm.copy()
        bad[3, 7] = bad[7, 3] = np.nan
        contract(bad)


def test_the_tie_heavy_inputs_are_tie_heavy():
    """every input the GPU tests call tie-heavy has at least 100 pairs of distinct edges with equal weight bits at the tree's own
    weights, and on each the two restatements agree: the tests cannot pass by accident of tie-free data"""
    cases = {"equal": (euclid(equal_input(120)), None), "grid": (euclid(grid_input(300)), None), "twice": (euclid(twice_input()), None)}
    Dr = euclid(random_input(300))
    for m in (5, 50):
        cases[f"core{m}"] = (Dr, core_of(Dr, m))
    for name, (Dm, core) in cases.items():
        tree = contract(Dm, core)
        pairs = tied_edge_pairs(weights(Dm, core), tree)
        print(name, pairs, "tied pairs of edges")
        assert pairs >= 100, name
        assert same_tree(tree, prim(Dm, core)), name
    # all songs equal: every weight is +0, the tree is the star from song 0 in key order
    star = contract(cases["equal"][0])
    assert (star[0] == 0).all() and star[1].tolist() == list(range(1, 120)) and not bits(star[2]).any()


# ---- mst_merge.hpp as a stand-alone program ----
def _run_program(exe, tmp, name, Dm, core=None, env=None):
    n = Dm.shape[0]
    fin, fout = str(tmp / f"{name}.in"), str(tmp / f"{name}.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<II", n, 0 if core is None else 1))
        f.write(np.ascontiguousarray(Dm, np.float32).tobytes())
        if core is not None:
            f.write(np.ascontiguousarray(core, np.float32).tobytes())
    out = subprocess.run([str(exe), fin, fout], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, (name, out.stdout[-500:], out.stderr[-3000:])
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, (name, out.stderr[-3000:])
    raw = open(fout, "rb").read()
    status, rounds = struct.unpack_from("<iI", raw, 0)
    m = max(n - 1, 0)
    u, v, w = (np.frombuffer(raw, np.uint32, m, 8 + 4 * m * k) for k in range(3))
    return status, rounds, (u.astype(np.int64), v.astype(np.int64), w.view(np.float32))


_WANT = {}


def _check_program(exe, tmp, env=None):
    out = subprocess.run([str(exe), "--direct"], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    for n in (1, 2, 3, 64, 257, 1000):
        inputs = {"random": random_input(n, seed=n), "equal": equal_input(n), "grid": grid_input(n, seed=n)}
        for name, X in inputs.items():
            Dm = euclid(X)
            if (name, n) not in _WANT:
                _WANT[(name, n)] = contract(Dm)  # (computed once for the plain and the sanitizer build)
            status, rounds, tree = _run_program(exe, tmp, f"{name}{n}", Dm, None, env)
            assert status == MST_OK and same_tree(tree, _WANT[(name, n)]), (name, n)
            assert rounds <= max(int(np.ceil(np.log2(max(n, 1)))), 0), (name, n, rounds)
    Dm = euclid(random_input(257, seed=9))
    core = core_of(Dm, 5)
    status, _, tree = _run_program(exe, tmp, "core", Dm, core, env)
    assert status == MST_OK and same_tree(tree, contract(Dm, core))


def test_mst_merge_header_against_the_contract(tmp_path):
    exe = tmp_path / "test_mst_merge"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", SRC, "-o", str(exe)])
    _check_program(exe, tmp_path)


@pytest.mark.skipif(not os.path.exists(SAN_CXX), reason="needs the ROCm clang for -fsanitize=address,undefined")
def test_mst_merge_header_under_address_and_ub_sanitizer(tmp_path):
    """the same stand-alone program built with -fsanitize=address,undefined: same trees, exit 0, no report"""
    exe = tmp_path / "test_mst_merge_san"
    subprocess.check_call([SAN_CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC,
                           "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    _check_program(exe, tmp_path, env)


def test_mst_merge_header_is_device_free():
    code = re.sub(r"//[^\n]*", "", open(HPP).read())
    assert "hip" not in code.lower() and "float" not in code and "double" not in code
    assert re.findall(r"#include\s+[<\"]([^>\"]+)", code) == ["stdint.h", "algorithm", "vector"]


# ---- the surface ----
def test_mst_abi_surface(bliss):
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    lib = C.CDLL(bliss.LIB_PATH)
    for name in ("blissgpu_mst", "blissgpu_mst_device"):
        assert re.search(r"\bint\s+%s\s*\(" % name, flat), name
        assert hasattr(lib, name), name
        assert name in _ffi.SIGNATURES, name

    def types(name):
        return [re.sub(r"\s*\b\w+$", "", " ".join(a.split())).replace(" *", "*")
                for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, flat).group(1).split(",")]

    # (x, n, d, metric, M, core, edge_u, edge_v, edge_w, rounds), the device form with the context
    want = ["const float*", "uint64_t", "uint32_t", "int", "const float*", "const float*", "uint32_t*", "uint32_t*", "float*", "uint32_t*"]
    assert types("blissgpu_mst") == want
    assert types("blissgpu_mst_device") == ["blissgpu_ctx*"] + want
    host = [_vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]
    assert _ffi.SIGNATURES["blissgpu_mst"] == (C.c_int, host)
    assert _ffi.SIGNATURES["blissgpu_mst_device"] == (C.c_int, [_vp] + host)
    assert re.search(r"#define\s+BLISSGPU_ERR_INTERNAL\s+8\b", flat) and _ffi.ERR_INTERNAL == 8
    for name in ("minimum_spanning_tree", "core_distances", "SpanningTree"):
        assert hasattr(bliss.playlist, name), name
    for name in ("song_tree", "linked_clusters", "tour"):
        assert hasattr(bliss.library, name), name
    assert hasattr(bliss.Context, "mst")


def test_mst_kernels_are_in_the_profile_table(bliss):
    from bliss_rs_amd import _ffi

    L = _ffi.lib()
    names = [L.blissgpu_profile_kernel_name(k).decode() for k in range(L.blissgpu_profile_kernel_count())]
    assert len(set(names)) == len(names) and "" not in names
    src = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "kernels_mst.hip")).read()
    mine = ("mst_scan_kernel", "mst_pick_kernel")
    for name in mine:
        assert names.count(name) == 1, name
        assert re.search(r"\bvoid\s+%s\s*\(" % name, src), name
        assert names.index(name) < len(names) - 2
    assert sorted(n for n in names if n.startswith("mst_")) == sorted(mine)
    assert names[-2:] == ["group_forest_scan_kernel", "journey_step_kernel"]  # (older ids keep their places)


def _p(a):
    return None if a is None else a.ctypes.data


def _call(x, n=None, d=None, metric=0, M=None, core=None, device=False, null=(), rounds=True):
    from bliss_rs_amd import _ffi

    n = x.shape[0] if n is None else n
    d = x.shape[1] if d is None else d
    m = max(min(n, 4096), 2)
    out = dict(edge_u=np.full(m, 7, np.uint32), edge_v=np.full(m, 7, np.uint32), edge_w=np.full(m, 7.0, np.float32))
    r = C.c_uint32(99)
    args = (None if "x" in null else _p(x), n, d, metric, _p(M), _p(core), *(None if k in null else _p(out[k]) for k in out),
            C.byref(r) if rounds else None)
    L = _ffi.lib()
    rc = L.blissgpu_mst_device(None, *args) if device else L.blissgpu_mst(*args)
    return rc, L.blissgpu_last_error(), out, r.value


def test_mst_arguments_are_checked_before_the_device(bliss):
    import torch

    X = random_input(50)
    M = np.eye(23, dtype=np.float32)
    for device in (False, True):
        rc, err, _, _ = _call(X, d=0, device=device)
        assert rc == INVALID and b"d must be" in err
        rc, err, _, _ = _call(np.zeros((50, 65), np.float32), device=device)
        assert rc == INVALID and b"d must be" in err
        rc, err, _, _ = _call(X, metric=3, device=device)
        assert rc == INVALID and b"metric" in err
        assert _call(X, metric=-1, device=device)[0] == INVALID
        rc, err, _, _ = _call(X, metric=1, device=device)
        assert rc == INVALID and b"cosine" in err
        rc, err, _, _ = _call(X, metric=2, device=device)  # mahalanobis without M
        assert rc == INVALID and b"M" in err
        rc, err, _, _ = _call(X, n=0xFFFFFFFF, device=device)
        assert rc == INVALID and b"n must be" in err
        for what in ("x", "edge_u", "edge_v", "edge_w"):
            rc, err, out, _ = _call(X, null=(what,), device=device)
            assert rc == INVALID and what.encode() in err, what
            assert all((a == 7).all() for a in out.values())
    # the device form checks the scalars before it looks at its context, and the context before anything else
    rc, err, _, _ = _call(X, d=65, device=True)
    assert rc == INVALID and b"d must be" in err
    rc, err, _, _ = _call(X, metric=2, M=M, device=True, rounds=False)
    assert rc == INVALID and b"ctx" in err
    rc, err, _, _ = _call(X, n=1, device=True)
    assert rc == INVALID and b"ctx" in err
    # no edge: OK without a device, nothing written, no round (NULL pointers are fine then)
    for n in (0, 1):
        rc, _, out, rounds = _call(X, n=n)
        assert rc == OK and rounds == 0 and all((a == 7).all() for a in out.values())
        assert _call(X, n=n, null=("x", "edge_u", "edge_v", "edge_w"), rounds=False)[0] == OK
    # a valid call: BLISSGPU_ERR_NO_DEVICE without a GPU, BLISSGPU_OK with one
    want = OK if torch.cuda.is_available() else NO_DEVICE
    assert _call(X)[0] == want
    assert _call(X, metric=2, M=M, core=np.ones(50, np.float32), rounds=False)[0] == want
    assert _call(X[:2])[0] == want


# ---- the Python layer above a numpy stand-in ----
def _numpy_mst(P):
    """playlist.minimum_spanning_tree with the device call replaced by `contract` over numpy f32 euclidean distances"""
    calls = []

    def fake(songs_or_X, metric_builder=P.euclidean_distance, min_samples=None):
        P._mst_metric(metric_builder)
        X = P._rows_of_input(songs_or_X)
        Dm = euclid(X)
        core = None if min_samples is None or X.shape[0] < 2 else core_of(Dm, int(min_samples))
        calls.append((X.shape[0], min_samples))
        u, v, w = contract(Dm, core)
        return P.SpanningTree(u, v, w, 0, X.shape[0])

    return fake, calls


def _flood(n, u, v):
    """labels by flood fill over the edges, numbered by lowest member"""
    adj = [[] for _ in range(n)]
    for a, b in zip(u.tolist(), v.tolist()):
        adj[a].append(b)
        adj[b].append(a)
    lab = np.full(n, -1, np.int64)
    c = 0
    for s in range(n):
        if lab[s] >= 0:
            continue
        lab[s] = c
        todo = [s]
        while todo:
            i = todo.pop()
            for j in adj[i]:
                if lab[j] < 0:
                    lab[j] = c
                    todo.append(j)
        c += 1
    return lab


def test_spanning_tree_refuses_what_group_neighbours_refuses(bliss):
    P = bliss.playlist
    X = random_input(12)
    for builder, word in ((P.cosine_distance, "cosine"), ("cosine", "cosine"), (P.ForestOptions(10, 8, 3, 0), "forest"),
                          (P.VarianceWeights(), "MahalanobisBuilder")):
        for call in (lambda b: P.minimum_spanning_tree(X, b), lambda b: P.core_distances(X, 3, b)):
            with pytest.raises(ValueError) as e:
                call(builder)
            assert word in str(e.value)
    with pytest.raises(TypeError):
        P.minimum_spanning_tree(X, lambda a, b: 0.0)
    with pytest.raises(ValueError):
        P.core_distances(X, 0)
    # no edge: no device is needed
    for n in (0, 1):
        t = P.minimum_spanning_tree(X[:n], min_samples=4)
        assert t.n == n and len(t.u) == 0 and t.u.dtype == np.int64 and t.w.dtype == np.float32 and t.rounds == 0
        assert t.cut().tolist() == [0] * n and t.tour().tolist() == list(range(n)) and t.linkage().shape == (0, 4)
    assert P.core_distances(X[:1], 3).tolist() == [0.0]
    # errors of the C layer arrive as BlissGpuError(ERR_INVALID) before a device is needed
    with pytest.raises(bliss.BlissGpuError) as e:
        P.minimum_spanning_tree(np.zeros((5, 65), np.float32))
    assert e.value.code == INVALID


def test_spanning_tree_cut(bliss):
    P = bliss.playlist
    fake, _ = _numpy_mst(P)
    n = 60
    X = random_input(n, seed=11)
    X[40:] += 6.0  # two far groups
    t = fake(X)
    assert t.u.dtype == np.int64 and t.w.dtype == np.float32 and t.n == n
    for k in range(1, n + 1):
        got = t.cut(k)
        want = _flood(n, t.u[:n - k], t.v[:n - k])  # remove the k - 1 last edges, flood-fill
        assert np.array_equal(got, want), k
        assert got.max() == k - 1
        first = [int(np.flatnonzero(got == c)[0]) for c in range(k)]
        assert first == sorted(first)  # numbered by lowest member
    assert np.array_equal(t.cut(), np.zeros(n, np.int64))
    two = t.cut(2)
    assert (two[:40] == 0).all() and (two[40:] == 1).all()
    # height: `>` removes, so an edge of exactly that weight stays
    for e in (0, 17, n - 2):
        h = float(t.w[e])
        stays = int((t.w <= t.w[e]).sum())
        assert np.array_equal(t.cut(height=h), _flood(n, t.u[:stays], t.v[:stays]))
        below = float(np.nextafter(t.w[e], np.float32(-np.inf)))
        gone = int((t.w < t.w[e]).sum())
        assert np.array_equal(t.cut(height=below), _flood(n, t.u[:gone], t.v[:gone]))
    assert t.cut(height=np.inf).max() == 0 and t.cut(height=-1.0).tolist() == list(range(n))
    # min_cluster_size: small clusters are -1, the others keep the order of their lowest members
    k = 12
    plain = t.cut(k)
    sizes = np.bincount(plain)
    got = t.cut(k, min_cluster_size=3)
    assert (sizes < 3).any() and (sizes >= 3).any()
    assert np.array_equal(got < 0, sizes[plain] < 3)
    kept = [c for c in range(k) if sizes[c] >= 3]
    for new, old in enumerate(kept):
        assert np.array_equal(got == new, plain == old)
    assert (t.cut(n, min_cluster_size=2) == -1).all()
    with pytest.raises(ValueError):
        t.cut(0)
    with pytest.raises(ValueError):
        t.cut(n + 1)
    with pytest.raises(ValueError):
        t.cut(2, height=1.0)


def test_spanning_tree_tour(bliss):
    P = bliss.playlist
    fake, _ = _numpy_mst(P)
    n = 60
    t = fake(random_input(n, seed=12))
    edges = set(zip(t.u.tolist(), t.v.tolist()))
    rank = {e: k for k, e in enumerate(zip(t.u.tolist(), t.v.tolist()))}
    for start in (0, 17, n - 1):
        tour = t.tour(start)
        assert tour.dtype == np.int64 and tour[0] == start and sorted(tour.tolist()) == list(range(n))
        # a depth-first preorder: every song's parent -- the LAST earlier song it shares an edge with on the walk's stack -- is
        # a tree neighbour heard before it, and the children of a song come in ascending edge key
        seen, parent = {start}, {}
        for s in tour[1:].tolist():
            nb = [p for p in seen if (min(p, s), max(p, s)) in edges]
            assert len(nb) == 1, s  # (a tree: exactly one neighbour is already in the walk)
            parent[s] = nb[0]
            seen.add(s)
        where = {s: k for k, s in enumerate(tour.tolist())}
        for p in range(n):
            kids = sorted((c for c in parent if parent[c] == p), key=where.get)
            keys = [rank[(min(p, c), max(p, c))] for c in kids]
            assert keys == sorted(keys), p
        # consecutive songs are joined by a tree path that only climbs from the first to an ancestor of the second's parent
        for a, b in zip(tour[:-1].tolist(), tour[1:].tolist()):
            up = a
            while up != parent[b]:
                up = parent[up]  # (a KeyError here would mean: not connected that way)
    with pytest.raises(ValueError):
        t.tour(n)
    # a chain of 10^5 songs: no recursion
    m = 100_000
    chain = P.SpanningTree(np.arange(m - 1), np.arange(1, m), np.ones(m - 1, np.float32), 0, m)
    assert np.array_equal(chain.tour(0), np.arange(m))
    back = chain.tour(m - 1)
    assert np.array_equal(back, np.arange(m)[::-1])
    mid = chain.tour(5)
    assert mid[:6].tolist() == [5, 4, 3, 2, 1, 0] and mid[6] == 6  # (edge {4, 5} is below edge {5, 6} in the order)


def test_spanning_tree_linkage_against_scipy(bliss):
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    P = bliss.playlist
    n = 80
    iu = np.triu_indices(n, 1)
    for seed in range(13, 33):  # the first seed whose distances stay apart when rounded to f32: both orders are then the same
        X = np.random.default_rng(seed).standard_normal((n, 5)).astype(np.float32)
        diff = X.astype(np.float64)[:, None, :] - X.astype(np.float64)[None, :, :]
        Dm = np.sqrt((diff * diff).sum(axis=2)).astype(np.float32)
        if len(np.unique(Dm[iu])) == len(iu[0]):
            break
    assert len(np.unique(Dm[iu])) == len(iu[0])
    u, v, w = contract(Dm)
    t = P.SpanningTree(u, v, w, 0, n)
    Z = t.linkage()
    want = hierarchy.linkage(X.astype(np.float64), "single")
    assert Z.shape == want.shape == (n - 1, 4) and Z.dtype == np.float64
    assert np.allclose(Z[:, 2], want[:, 2], rtol=1e-6, atol=0)  # (f32 heights against f64 ones)
    assert np.array_equal(Z[:, 3], want[:, 3]) and (Z[:, 0] < Z[:, 1]).all() and Z[-1, 3] == n
    for k in range(1, n + 1):  # the partition at every height
        a = hierarchy.fcluster(Z, k, "maxclust")
        b = hierarchy.fcluster(want, k, "maxclust")
        assert len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist())) == k
        mine = t.cut(k)
        assert len(set(zip(mine.tolist(), b.tolist()))) == k


# ---- the library ----
@pytest.fixture()
def genres_db(bliss, tmp_path):
    """three genres around planted centres, 41 songs; songs 7, 17, 27 and 37 have no genre tag"""
    rng = np.random.default_rng(22)
    centre = {"jazz": 0.0, "metal": 4.0, "folk": 9.0}
    names = ["jazz", "metal", "folk"]
    V2 = bliss.FeaturesVersion.Version2
    songs = []
    for i in range(41):
        genre = None if i % 10 == 7 else names[i % 3]
        x = (centre[genre or "jazz"] + 0.05 * rng.standard_normal(23)).astype(np.float32)
        songs.append(bliss.Song(path=f"/music/{i:03d}.flac", title=f"t{i}", artist="a", album="b", disc_number=1, track_number=i,
                                duration=1.0, genre=genre, analysis=bliss.Analysis(x, V2), features_version=V2))
    db = str(tmp_path / "bliss.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs)
    return db, songs


def test_library_song_tree_clusters_and_tour(bliss, monkeypatch, genres_db):
    P, Lb = bliss.playlist, bliss.library
    db, songs = genres_db
    fake, calls = _numpy_mst(P)
    monkeypatch.setattr(P, "minimum_spanning_tree", fake)
    got, tree = Lb.song_tree(db)
    assert got == [s.path for s in songs] and tree.n == 41 and len(tree.u) == 40  # the keys: paths in id order
    assert calls == [(41, None)]  # one device call per library call
    got, tree = Lb.song_tree(db, min_samples=3, where=("genre", "metal"))
    assert got == [s.path for s in songs if s.genre == "metal"] and tree.n == len(got)
    assert calls[-1] == (len(got), 3) and len(calls) == 2
    # the three planted genres (the untagged songs sit with jazz), clusters in order of their first song, songs in id order
    lists, loose = Lb.linked_clusters(db, k=3)
    assert len(calls) == 3 and loose == [] and [len(c) for c in lists] == [17, 12, 12]
    assert [c[0].path for c in lists] == ["/music/000.flac", "/music/001.flac", "/music/002.flac"]
    for c in lists:
        assert [s.path for s in c] == sorted(s.path for s in c)
        assert len({s.genre for s in c if s.genre is not None}) == 1
    lists, loose = Lb.linked_clusters(db, height=1.0, min_cluster_size=13)
    assert [len(c) for c in lists] == [17] and len(loose) == 24 and len(calls) == 4
    assert Lb.linked_clusters(db, k=1, where=("genre", "nobody")) == ([], []) and len(calls) == 4
    # the tour: every song once, from the start, one call
    order = Lb.tour(db)
    assert order[0].path == songs[0].path and sorted(s.path for s in order) == sorted(s.path for s in songs) and len(calls) == 5
    order = Lb.tour(db, start_path="/music/004.flac", where=("genre", "metal"))
    assert order[0].path == "/music/004.flac" and {s.genre for s in order} == {"metal"} and len(order) == 12 and len(calls) == 6
    n_calls = len(calls)
    with pytest.raises(bliss.ProviderError) as e:
        Lb.tour(db, start_path="/music/nobody.flac")
    assert "was not found" in str(e.value)
    with pytest.raises(bliss.ProviderError):
        Lb.tour(db, start_path="/music/000.flac", where=("genre", "metal"))  # a jazz song
    with pytest.raises(ValueError):
        Lb.song_tree(db, where=("title", "t1"))
    with pytest.raises(ValueError):
        Lb.tour(db, metric_builder=P.cosine_distance)
    with pytest.raises(ValueError):
        Lb.linked_clusters(db, k=2, metric_builder=P.cosine_distance)
    assert len(calls) == n_calls  # every refusal comes before the device
