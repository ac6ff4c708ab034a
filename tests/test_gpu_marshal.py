"""GPU tests (-m gpu) of the conversion path of the Python bindings: every host entry point of playlist.py is
called with its inputs as float64, as Fortran-ordered arrays and as every-second-row views of a larger array, and must
return, bit for bit, what it returns on the C-contiguous float32 copy; Context.knn / group_knn / chains / kmeans likewise
with strided device tensors.  The contiguous path is held to the oracle by the family tests; this file holds the conversion
to it, the one thing the marshalling layer can break that those tests would not see."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, K = 300, 23, 3
OFFSETS = [0, 1, 3, 7]  # groups of 1, 2 and 4 seeds
VARIANTS = ("float64", "fortran", "strided")


@pytest.fixture(scope="module")
def bliss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import bliss_rs_amd

    return bliss_rs_amd


@pytest.fixture(scope="module")
def ctx(bliss):
    c = bliss.Context(0)
    yield c
    c.close()


def _rows():
    rng = np.random.default_rng(336)
    return rng.standard_normal((N, D)).astype(np.float32)


def variant(a, how):
    """the same numbers as the float32 array `a` in a layout or type the library cannot take as it is"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if how == "float64":
        return a.astype(np.float64)  # (every float32 is a float64: the way back is exact)
    if how == "fortran":
        return np.asfortranarray(a)
    big = np.full((2 * a.shape[0],) + a.shape[1:], 99.0, np.float32)
    big[::2] = a
    view = big[::2]
    assert a.shape[0] < 2 or not view.flags.c_contiguous
    return view


def _groups(S, v):
    return [v(S[OFFSETS[g]:OFFSETS[g + 1]]) for g in range(len(OFFSETS) - 1)]


# name -> call(P, X, v, aux): v converts an array, aux holds what was computed once on the contiguous rows
def _families():
    lab = np.arange(N) % 3
    return {
        "set_distances": lambda P, X, v, aux: P.set_distances(v(X[3:7]), v(X)),
        "closest_to_songs_order": lambda P, X, v, aux: P.closest_to_songs_order(v(X[3:7]), v(X)),
        "nearest_order": lambda P, X, v, aux: P.nearest_order(v(X[:8]), v(X), K),
        "scaled_nearest_order": lambda P, X, v, aux: P.scaled_nearest_order(v(X[:8]), v(aux["scale"][:8]), v(X), v(aux["scale"]), K),
        "nearest_to_groups": lambda P, X, v, aux: P.nearest_to_groups(_groups(X[:7], v), v(X), K),
        "chain_order": lambda P, X, v, aux: P.chain_order(_groups(X[:7], v), v(X), K),
        "journey_order": lambda P, X, v, aux: P.journey_order(v(X[:3]), v(X), K, v(X[3:6])),
        "radio_order": lambda P, X, v, aux: P.radio_order(v(X[:3]), v(X), K, (np.arange(N) % 7)[None, :], [2], [1]),
        "kmeans": lambda P, X, v, aux: P.kmeans(v(X), v(X[:3])),
        "silhouette": lambda P, X, v, aux: P.silhouette(v(X), lab),
        "group_neighbours": lambda P, X, v, aux: P.group_neighbours(v(X), lab, 2),
        "minimum_spanning_tree": lambda P, X, v, aux: P.minimum_spanning_tree(v(X)),
        "ward_tree": lambda P, X, v, aux: P.ward_tree(v(X)),
        "kmedoids": lambda P, X, v, aux: P.kmedoids(v(X), K),
        "moments": lambda P, X, v, aux: P.moments(v(X), lab),
        "dedup_order": lambda P, X, v, aux: P.dedup_order(v(X)),
    }


FAMILIES = _families()


def flat(result):
    """every array and number of a result, in a fixed order"""
    if isinstance(result, np.ndarray):
        return [result]
    if isinstance(result, (tuple, list)):
        return [a for r in result for a in flat(r)]
    if dataclasses.is_dataclass(result):
        return flat([getattr(result, f.name) for f in dataclasses.fields(result)])
    if hasattr(result, "__dict__"):
        return flat([val for _, val in sorted(vars(result).items())])
    return [] if result is None else [np.asarray(result)]


def same_bits(got, want):
    got, want = flat(got), flat(want)
    assert len(got) == len(want) and len(want) >= 1
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


@pytest.fixture(scope="module")
def reference(bliss):
    """every family once on the contiguous float32 rows; shared by the cases and left unchanged"""
    P = bliss.playlist
    X = _rows()
    aux = {"scale": P.local_scales(X, 5)}
    keep = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    return X, aux, {name: call(P, X, keep, aux) for name, call in FAMILIES.items()}


@pytest.mark.parametrize("how", VARIANTS)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_converted_inputs_give_the_bits_of_the_contiguous_call(bliss, reference, family, how):
    X, aux, want = reference
    got = FAMILIES[family](bliss.playlist, X, lambda a: variant(a, how), aux)
    same_bits(got, want[family])


@pytest.mark.parametrize("method", ["knn", "group_knn", "chains", "kmeans"])
def test_strided_device_tensors_give_the_bits_of_contiguous_ones(bliss, ctx, method):
    import torch

    def strided(t):
        big = torch.full((2 * t.shape[0], t.shape[1]), 99.0, dtype=torch.float32, device=t.device)
        big[::2] = t
        view = big[::2]
        assert not view.is_contiguous()
        return view

    X = torch.from_numpy(_rows()).cuda()
    S = X[:7].contiguous()
    calls = {
        "knn": lambda v: ctx.knn(v(X[:8].contiguous()), v(X), K),
        "group_knn": lambda v: ctx.group_knn(v(S), OFFSETS, v(X), K),
        "chains": lambda v: ctx.chains(v(S), OFFSETS, v(X), K),
        "kmeans": lambda v: ctx.kmeans(v(X), v(X[:3].contiguous())),
    }
    want = calls[method](lambda t: t)
    got = calls[method](strided)
    ctx.synchronize()
    host = lambda r: [a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a) for a in r]  # noqa: E731
    same_bits(host(got), host(want))
