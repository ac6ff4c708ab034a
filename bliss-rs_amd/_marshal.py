"""The numpy shaping every host entry point of playlist.py does before _ffi.call, one copy each.  The helpers return arrays,
never addresses: the address is taken inside _ffi.call, from an array it has checked and holds until the C function returns."""
import numpy as np

NONE = 0xFFFFFFFF  # the library's "no index": padding of a short list, "skip nothing"


def rows_f32(a) -> np.ndarray:
    """[n, d] float32, C-contiguous (the array itself when it already is that)"""
    return np.ascontiguousarray(np.atleast_2d(a), dtype=np.float32)


def metric_matrix(metric, m, d=None, groups=None):
    """The M argument of an entry point: `m` as a contiguous float32 array, or None when none was given.  With `d`, the
    entry point is one that checks M on the host: it looks at m under "mahalanobis" only, where there must be one, [d, d];
    with `groups` too, m is one diagonal per group, [groups, d]."""
    if d is None:
        return None if m is None else np.ascontiguousarray(m, dtype=np.float32)
    if groups is not None:
        m = np.ascontiguousarray(m, dtype=np.float32)
        if m.shape != (groups, d):
            raise ValueError("m must be [G, d]")
        return m
    if metric != "mahalanobis":
        return None
    if m is None:
        raise ValueError("mahalanobis needs m")
    m = np.ascontiguousarray(m, dtype=np.float32)
    if m.shape != (d, d):
        raise ValueError("m must be [d, d]")
    return m


def signed_idx(idx) -> np.ndarray:
    """uint32 indices with 0xFFFFFFFF as padding -> int64 with -1"""
    out = idx.astype(np.int64)
    out[idx == NONE] = -1
    return out


def skip_words(skip, shape, n, per="skip needs one entry per query"):
    """Candidate indices to leave out, -1 = none, as the uint32 words the library takes (0xFFFFFFFF = none).  `shape`: the
    length (every entry point flattens) or the shape the entry point asks for; `per`: what it says when that is not met."""
    skip = np.asarray(skip, dtype=np.int64)
    if isinstance(shape, tuple):
        if skip.shape != shape:
            raise ValueError(per)
    else:
        skip = skip.reshape(-1)
        if skip.shape[0] != shape:
            raise ValueError(per)
    if ((skip < -1) | (skip >= max(n, 0))).any():
        raise ValueError("skip entries must be candidate indices or -1")
    return np.ascontiguousarray(np.where(skip < 0, NONE, skip).astype(np.uint32))


def check_k_d(k, d, d_max=64):
    """the list lengths and row widths the group families take"""
    if not 1 <= k <= 1024:
        raise ValueError("k must be 1 .. 1024")
    if not 1 <= d <= d_max:
        raise ValueError(f"d must be 1 .. {d_max}")
