"""Host-pointer form against device form of one C-ABI family, bit for bit, through the raw C ABI (the Python layer always
asks for every output: only here can an optional output be NULL).  The shape is the smallest at which a staging offset of
the host layer can go wrong: 300 candidates (a ragged block, no power of two anywhere in the staging buffers), d = 23,
k = 3, three seed groups of 1, 2 and 4 seeds, 5 rows where a family takes rows; every call is followed by one of ANOTHER
size on the same (default) context, which regrows every staging buffer under the pointers of the first.  Each family's
tests/test_gpu_*.py calls check() with the optional arguments it has, given and NULL.  The triplet forms and
blissgpu_pairwise, which did not move onto the staging helper, have no case here."""
import ctypes as C

import numpy as np

D = 23
SHAPES = ((300, (1, 2, 4), 3, 5), (517, (3, 1, 5, 2), 5, 7))  # candidates, seed-group sizes, k, rows
NONE = 0xFFFFFFFF


class Case:
    """the inputs of one shape: X [n, d], the groups' seeds S with offsets off and one skip entry per seed (its own row; one
    of them "none"), q rows Q with their skip entries, labels for the albums and the radio rules, a full Mahalanobis M.
    seed: None = the bytes every staging test has always had; a number = another draw of the same shapes, as valid as the
    first (tests/test_gpu_streams.py takes seed=1 as the decoy its buffers hold before the real inputs arrive)"""

    def __init__(self, n, sizes, k, q, seed=None):
        rng = np.random.default_rng(n if seed is None else (n, seed))
        self.n, self.k, self.q, self.G = n, k, q, len(sizes)
        self.X = (rng.integers(-8, 9, (n, D)) / 8).astype(np.float32)  # a grid of eighths: ties at the cut
        self.off = np.concatenate(([0], np.cumsum(sizes))).astype(np.uint64)
        rows = rng.choice(n, int(self.off[-1]), replace=False)
        self.S = np.ascontiguousarray(self.X[rows])
        self.skip = rows.astype(np.uint32)
        self.skip[-1] = NONE
        qrows = rng.choice(n, q, replace=False)
        self.Q = np.ascontiguousarray(self.X[qrows])
        self.qskip = qrows.astype(np.uint32)
        self.qskip2 = np.stack([qrows, (qrows + 1) % n], 1).astype(np.uint32)  # journeys and radios: two entries per row
        self.n_albums = 40
        self.album_of = rng.integers(0, self.n_albums, n).astype(np.uint32)
        self.album_of[::17] = NONE
        A = rng.standard_normal((D, D)) * 0.3
        self.M = (A @ A.T + 0.1 * np.eye(D)).astype(np.float32)
        self.W = rng.uniform(0.1, 2.0, (self.G, D)).astype(np.float32)


def _run(lib, name, args):
    """one call; numpy arrays and torch tensors go in as their addresses"""
    fn, conv = getattr(lib, name), []
    for a, t in zip(args, fn.argtypes):
        if isinstance(a, np.ndarray):
            a = a.ctypes.data_as(t)
        elif hasattr(a, "data_ptr"):
            a = C.c_void_p(a.data_ptr())
        conv.append(a)
    assert len(conv) == len(fn.argtypes), name
    rc = fn(*conv)
    assert rc == 0, (name, rc, lib.blissgpu_last_error().decode())


def check(bliss, ctx, family, build, lists=True, canon=None):
    """build(case, dev) -> (args, outs): the argument list after the context and the output arrays among them (None: the
    optional output left out); dev(a) is the array's place on the device for the device form, a itself for the host form (an
    output that is host memory in both forms is not passed through dev).  Runs blissgpu_<family> and blissgpu_<family>_device
    on both shapes, one after the other, and compares every output.  lists: the first output is an index matrix.  canon(outs):
    brings a form's outputs (numpy arrays) into one order first, where the device form's order is not defined."""
    import torch

    from bliss_rs_amd import _ffi

    def on_device(a):  # (64-bit words travel as int64: the bytes are what is compared)
        return None if a is None else torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()

    lib = _ffi.lib()
    for shape in SHAPES:
        case = Case(*shape)
        h_args, h_outs = build(case, lambda a: a)
        _run(lib, "blissgpu_" + family, h_args)
        d_args, d_outs = build(case, on_device)
        _run(lib, "blissgpu_" + family + "_device", [ctx._h] + list(d_args))
        ctx.synchronize()
        d_outs = [t if t is None or isinstance(t, np.ndarray) else np.ascontiguousarray(t.cpu().numpy()) for t in d_outs]
        assert len(h_outs) == len(d_outs)
        if canon:
            canon(h_outs), canon(d_outs)
        for i, (h, got) in enumerate(zip(h_outs, d_outs)):
            assert (h is None) == (got is None)
            if h is not None:
                assert np.array_equal(h.view(np.uint8), got.view(np.uint8)), (family, shape[0], "output", i, "host and device forms differ")
                assert not (h.view(np.uint8) == 0x5A).all(), (family, shape[0], "output", i, "was not written")
        idx = h_outs[0]
        assert not lists or (((idx < case.n) | (idx == NONE)).all() and (idx != NONE).any()), (family, "indices")


def out(shape, dtype, given=True):
    """an output array filled with a pattern no result holds, or None"""
    if not given:
        return None
    return np.frombuffer(b"\x5a" * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype).reshape(shape).copy()
