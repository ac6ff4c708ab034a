"""Distance metrics and playlist ordering -- mirror of src/playlist.rs.

    euclidean / cosine / mahalanobis distance, builders          :65-79, 129-142
    DistanceMetricBuilder / FunctionDistanceMetric               :24-59
    variance_based_weight_matrix                                 :173-221
    ForestOptions (the extended isolation forest metric)         :19-23, 230-251
    VarianceWeights (that matrix as a metric builder), group_variance_weights (every seed group's, one device call)
    closest_to_songs, song_to_song                               :256-326
    nearest_order, nearest_songs (closest_to_songs cut after k, for many seeds at once)
    dedup_playlist, dedup_playlist_custom_distance               :343-402
    duplicate_labels, duplicate_groups (the rule of :381-388 over every pair of a collection, closed transitively)
    closest_album_to_group                                       :424-485
    journey_order, waypoint_playlist, directed_playlist (the waypoint and direction features of the reference's TODO.md)
    Rule, rule_labels, radio_order, radio_playlist (radio playlists: song-to-song chains or the k nearest songs under artist /
    album separation rules -- no artist twice within w tracks, at most c songs per artist -- exact, stepped on the device)
    kmeans, kmeans_init, cluster_songs (the clustering the reference's TODO.md asks for: Lloyd's algorithm on the device)
    silhouette, choose_k (the "objective way to evaluate" of the reference's TODO.md: how well a labelling separates the songs
    under a metric, all pairs on the device without the distance matrix; and the k whose k-means clusters separate them best)
    group_neighbours (the "similar artists to the current one" of the reference's TODO.md: the nearest groups of a labelling
    under the average nearest-member distance, all pairs on the device without the distance matrix)
    triplet_step, learn_metric, triplet_accuracy, triplets_from_labels (the metric learning the reference's TODO.md and its
    training_triplet table ask for: a Mahalanobis M from "a and b are closer than o" triplets, the gradient on the device)
    map_affinities, map_init, map_step, map_layout, song_map (a 2-D map of a library, a point per song: exact t-SNE, every
    pair in every iteration and every iteration on the device)

A metric builder is one of the strings "euclidean" / "cosine", a `MahalanobisBuilder` (or the pair
("mahalanobis", M)), a `ForestOptions` (closest_to_songs and library.playlist_from_custom only: the forest needs at
least two seed songs) or a `VarianceWeights` (the entry points that build a metric from a seed SET: closest_to_songs,
set_distances, nearest_to_groups, group_playlists and their library forms), i.e. the metrics the device implements; arbitrary Python callables are not accepted
because the distances are evaluated by the HIP kernels (there is no CPU path).  Songs are anything with an
`.analysis` (Analysis) -- `Song` or a wrapper holding one in `.bliss_song`, like the reference's
`AsRef<Song>`."""
import ctypes as C
import dataclasses
import os
from typing import Callable, Optional, Sequence

import numpy as np

from . import _ffi
from ._marshal import check_k_d, metric_matrix, rows_f32, signed_idx, skip_words


def _vec(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1)


def _call(name, *args):
    """_ffi.call for the entry points whose NaN distance is the reference's panic: ERR_NAN becomes that ValueError"""
    try:
        return _ffi.call(name, *args)
    except _ffi.BlissGpuError as e:
        _nan_to_panic(e)


def _single(a, b, metric, m=None) -> float:
    a, b = _vec(a), _vec(b)
    if a.shape != b.shape:
        raise ValueError("vectors must have the same length")
    out = C.c_float()
    _ffi.call("blissgpu_distance", a, b, a.shape[0], metric, metric_matrix(metric, m), C.byref(out))
    return float(out.value)


def euclidean_distance(a, b) -> float:
    """src/playlist.rs:65-71"""
    return _single(a, b, _ffi.METRIC_EUCLIDEAN)


def cosine_distance(a, b) -> float:
    """src/playlist.rs:76-79"""
    return _single(a, b, _ffi.METRIC_COSINE)


def mahalanobis_distance(a, b, m) -> float:
    """src/playlist.rs:140-142"""
    return _single(a, b, _ffi.METRIC_MAHALANOBIS, m)


def mahalanobis_distance_builder(m) -> Callable[[np.ndarray, np.ndarray], float]:
    """src/playlist.rs:129-131"""
    m = np.ascontiguousarray(m, dtype=np.float32).copy()
    return lambda a, b: mahalanobis_distance(a, b, m)


_METRICS, _ROUTES, _JOURNEY_MODES, _GATES = _ffi.METRICS, _ffi.ROUTES, _ffi.JOURNEY_MODES, _ffi.GATES
_GROUP_MODES, _RADIO_MODES, _FORMS = _ffi.GROUP_MODES, _ffi.RADIO_MODES, _ffi.FORMS


def pairwise_distances(A, B, metric="euclidean", m=None) -> np.ndarray:
    """All-pairs matrix out[i, j] = metric(A[i], B[j]) (batched form of DistanceMetric::distance,
    src/playlist.rs:24-59, 256-270)."""
    A = np.ascontiguousarray(A, dtype=np.float32)
    B = np.ascontiguousarray(B, dtype=np.float32)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1]:
        raise ValueError("A and B must be [n, d] and [m, d]")
    out = np.empty((A.shape[0], B.shape[0]), np.float32)
    _ffi.call("blissgpu_pairwise", A, A.shape[0], B, B.shape[0], A.shape[1], _METRICS[metric], metric_matrix(metric, m), out)
    return out


class FunctionDistanceMetric:
    """Distance to a seed set = sum of the distances to each seed (src/playlist.rs:36-59)."""

    def __init__(self, metric: str, vectors: Sequence[np.ndarray], m=None):
        self.metric, self.m = metric, m
        self.state = np.ascontiguousarray(np.stack([_vec(v) for v in vectors]), dtype=np.float32)

    def distance(self, vector) -> float:
        row = pairwise_distances(self.state, _vec(vector)[None, :], self.metric, self.m)[:, 0]
        acc = np.float32(0.0)
        for v in row:  # iter().sum::<f32>() is sequential
            acc = np.float32(acc + v)
        return float(acc)


# ---------------------------------------------------------------------------------------------------
# playlist ordering (src/playlist.rs:173-485)
# ---------------------------------------------------------------------------------------------------
class MahalanobisBuilder:
    """mahalanobis_distance_builder(m) as a metric builder (src/playlist.rs:129-131)."""

    def __init__(self, m):
        self.m = np.ascontiguousarray(m, dtype=np.float32).copy()


class ForestOptions:
    """extended_isolation_forest::ForestOptions as a metric builder (src/playlist.rs:230-251): the metric meant for
    playlists grown from SEVERAL seed songs (:19-23).  The four fields of the reference are required (`max_tree_depth`
    may be None: ceil(log2(min(sample_size, number of seeds)))).  `seed` makes the forest a pure function of (seed songs,
    options, seed), which the reference's (thread RNG) is not; None draws one from os.urandom and keeps it in `.seed`, so
    any playlist can be reproduced after the fact."""

    def __init__(self, n_trees, sample_size, max_tree_depth, extension_level, seed=None):
        self.n_trees, self.sample_size, self.extension_level = int(n_trees), int(sample_size), int(extension_level)
        self.max_tree_depth = None if max_tree_depth is None else int(max_tree_depth)
        self.seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF

    def __repr__(self):
        return (f"ForestOptions(n_trees={self.n_trees}, sample_size={self.sample_size}, max_tree_depth={self.max_tree_depth}, "
                f"extension_level={self.extension_level}, seed={self.seed})")


_FOREST_SINGLE = ("the isolation forest does not work for a single song (min(sample_size, seeds) < 2, "
                  "src/playlist.rs:230-240): {what}")


def _no_forest(builder, what):
    """The entry points whose metric is built from ONE song refuse a ForestOptions (psi < 2)."""
    if isinstance(builder, ForestOptions):
        raise ValueError(_FOREST_SINGLE.format(what=what))


_TOO_FEW_SEEDS = "seeds must contain more than one element"  # variance_based_weight_matrix, src/playlist.rs:174-178


class VarianceWeights:
    """mahalanobis_distance_builder(variance_based_weight_matrix(seeds)) as a metric builder (src/playlist.rs:129-131,
    173-221): a diagonal metric built from the seed SET, so an album whose songs agree on tempo and timbre but not on key
    gets a playlist that follows tempo and timbre.  `few_seeds`: what a seed set of fewer than two songs means -- "raise"
    (the default) is the reference's ProviderError("seeds must contain more than one element"), decided before the device is
    touched; "euclidean" takes the identity (euclidean_distance's own M, src/playlist.rs:69) for such a set."""

    def __init__(self, few_seeds="raise"):
        if few_seeds not in ("raise", "euclidean"):
            raise ValueError('few_seeds must be "raise" or "euclidean"')
        self.few_seeds = few_seeds

    def __repr__(self):
        return f"VarianceWeights(few_seeds={self.few_seeds!r})"

    def check_counts(self, counts):
        """the policy for seed sets of these sizes (nothing but the sizes is looked at)"""
        from .song import ProviderError

        if self.few_seeds == "raise" and any(int(c) < 2 for c in counts):
            raise ProviderError(_TOO_FEW_SEEDS)

    def matrix(self, seeds):
        """-> ("mahalanobis", M) for ONE seed set, M from the host arithmetic (variance_based_weight_matrix); ("euclidean",
        None) for fewer than two seeds when few_seeds is "euclidean" """
        seeds = np.atleast_2d(np.asarray(seeds, dtype=np.float32))
        self.check_counts([seeds.shape[0]])
        if seeds.shape[0] < 2:
            return "euclidean", None
        return "mahalanobis", variance_based_weight_matrix(list(seeds))


_VARIANCE_SINGLE = ("variance-based weights need a seed set of more than one song (variance_based_weight_matrix, "
                    "src/playlist.rs:173-178): {what}")


def _no_variance(builder, what):
    """The entry points whose metric is built from ONE song refuse a VarianceWeights (fewer than two seeds)."""
    if isinstance(builder, VarianceWeights):
        raise ValueError(_VARIANCE_SINGLE.format(what=what))


def _seed_set_metric(metric, m, seeds):
    """(metric, m) of an entry point that builds ONE metric from ONE seed set: a VarianceWeights becomes its matrix"""
    if isinstance(metric, VarianceWeights):
        return metric.matrix(seeds)
    return metric, m


class Forest:
    """A forest built from seed rows (host code, no device needed): the DistanceMetric ForestOptions::build returns
    (src/playlist.rs:230-251).  `export()` gives the canonical dense form documented in include/blissgpu.h."""

    def __init__(self, seeds, options: ForestOptions):
        S = rows_f32(seeds)
        if not isinstance(options, ForestOptions):
            raise TypeError("options must be a ForestOptions")
        depth = options.max_tree_depth
        if depth is not None and not 1 <= depth <= 128:
            raise ValueError("max_tree_depth must be None or 1 .. 128")
        for name in ("n_trees", "sample_size", "extension_level"):
            if not 0 <= getattr(options, name) <= 0xFFFFFFFF:
                raise ValueError(f"{name} out of range")
        if min(options.sample_size, S.shape[0]) < 2:
            raise ValueError(_FOREST_SINGLE.format(what=f"{S.shape[0]} seed(s), sample_size {options.sample_size}"))
        self.options, self._h = options, None
        h = C.c_void_p()
        try:
            _ffi.call("blissgpu_forest_build", S, S.shape[0], S.shape[1], options.n_trees, options.sample_size, depth or 0,
                      options.extension_level, options.seed, C.byref(h))
        except _ffi.BlissGpuError as e:
            if e.code == _ffi.ERR_INVALID:
                raise ValueError(str(e)) from e
            raise
        self._h = h
        v = [C.c_uint32() for _ in range(5)]
        nn = C.c_uint64()
        _ffi.call("blissgpu_forest_info", h, *[C.byref(x) for x in v], C.byref(nn))
        self.d, self.n_trees, self.psi, self.depth_limit, self.extension_level = (int(x.value) for x in v)
        self.n_nodes = int(nn.value)

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h is not None:
            _ffi.lib().blissgpu_forest_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter shutdown
            pass

    def export(self) -> dict:
        T, N, d = self.n_trees, self.n_nodes, self.d
        out = {"sample_idx": np.empty((T, self.psi), np.uint32), "tree_first": np.empty(T + 1, np.uint64),
               "normal": np.empty((N, d), np.float32), "b": np.empty(N, np.float32), "left": np.empty(N, np.uint32),
               "right": np.empty(N, np.uint32), "leaf_size": np.empty(N, np.uint32), "leaf_q": np.empty(N, np.uint32)}
        _ffi.call("blissgpu_forest_export", self._h, *out.values())
        return out

    def _cand(self, candidates):
        X = rows_f32(candidates)
        if X.ndim != 2 or (X.shape[0] and X.shape[1] != self.d):
            raise ValueError(f"candidates must be [n, {self.d}]")
        return X

    def scores(self, candidates, return_path_sum=False):
        """-> score f32[n] (and the exact u64 path sums)."""
        X = self._cand(candidates)
        n = X.shape[0]
        score, ps = np.empty(n, np.float32), np.empty(n, np.uint64)
        _ffi.call("blissgpu_forest_score", self._h, X, n, score, ps if return_path_sum else None)
        return (score, ps) if return_path_sum else score

    def closest_to_songs_order(self, candidates):
        """-> (order u32[n], score f32[n]): stable ascending order of the scores."""
        X = self._cand(candidates)
        n = X.shape[0]
        order, score = np.empty(n, np.uint32), np.empty(n, np.float32)
        _ffi.call("blissgpu_forest_closest_to_songs", self._h, X, n, order, score)
        return order, score


def forest_scores(seeds, candidates, options: ForestOptions) -> np.ndarray:
    """ForestOptions::build(seeds).distance(candidate) for every row of `candidates` (src/playlist.rs:230-251): f32[n],
    low for songs like the seeds, high for outliers."""
    f = Forest(seeds, options)
    try:
        return f.scores(candidates)
    finally:
        f.close()


def forest_closest_to_songs_order(seeds, candidates, options: ForestOptions):
    """Index form of closest_to_songs with a forest: -> (order u32[n], scores f32[n])."""
    f = Forest(seeds, options)
    try:
        return f.closest_to_songs_order(candidates)
    finally:
        f.close()


def _metric_of(builder):
    """-> (metric name, M or None)"""
    if isinstance(builder, MahalanobisBuilder):
        return "mahalanobis", builder.m
    if isinstance(builder, tuple) and len(builder) == 2 and builder[0] == "mahalanobis":
        return "mahalanobis", np.ascontiguousarray(builder[1], dtype=np.float32)
    if builder in (euclidean_distance, "euclidean"):
        return "euclidean", None
    if builder in (cosine_distance, "cosine"):
        return "cosine", None
    raise TypeError("metric builder must be euclidean_distance / cosine_distance / MahalanobisBuilder(m): distances "
                    "are evaluated on the GPU, arbitrary callables are not supported")


def _plain_metric(metric_builder, why_forest, why_variance, cosine=None):
    """(metric, m) of an entry point that compares single songs: a ForestOptions and a VarianceWeights are refused with the
    entry point's reasons, cosine with the text `cosine` where the entry point cannot run it"""
    _no_forest(metric_builder, why_forest)
    _no_variance(metric_builder, why_variance)
    metric, m = _metric_of(metric_builder)
    if cosine is not None and metric == "cosine":
        raise ValueError(cosine)
    return metric, m


def _song_of(s):
    return getattr(s, "bliss_song", s)  # AsRef<Song>


def _matrix(songs) -> np.ndarray:
    rows = [np.asarray(_song_of(s).analysis.as_vec(), dtype=np.float32) for s in songs]
    if not rows:
        return np.zeros((0, 1), np.float32)
    return np.ascontiguousarray(np.stack(rows), dtype=np.float32)


def _nan_to_panic(e: "_ffi.BlissGpuError"):
    if e.code == _ffi.ERR_NAN:
        raise ValueError("NaN distance (noisy_float::n32 / argmin().unwrap() panic in the reference)") from e
    raise e


def set_distances(seeds, candidates, metric="euclidean", m=None) -> np.ndarray:
    """FunctionDistanceMetric::distance (src/playlist.rs:52-58) for every row of `candidates`.  `metric` may be a
    VarianceWeights: M is then variance_based_weight_matrix(seeds)."""
    S = rows_f32(seeds)
    metric, m = _seed_set_metric(metric, m, S)
    X = rows_f32(candidates)
    out = np.empty(X.shape[0], np.float32)
    _ffi.call("blissgpu_set_distance", S, S.shape[0], X, X.shape[0], X.shape[1], _METRICS[metric], metric_matrix(metric, m), out)
    return out


def closest_to_songs_order(seeds, candidates, metric="euclidean", m=None):
    """Index form of closest_to_songs: -> (order u32[n], distances f32[n]).  `metric` may be a ForestOptions (the forest
    scores are the distances; see forest_closest_to_songs_order)."""
    if isinstance(metric, ForestOptions):
        return forest_closest_to_songs_order(seeds, candidates, metric)
    S = rows_f32(seeds)
    metric, m = _seed_set_metric(metric, m, S)  # (a VarianceWeights: M = variance_based_weight_matrix(seeds))
    X = rows_f32(candidates)
    order, dist = np.empty(X.shape[0], np.uint32), np.empty(X.shape[0], np.float32)
    _call("blissgpu_closest_to_songs", S, S.shape[0], X, X.shape[0], X.shape[1], _METRICS[metric], metric_matrix(metric, m), order,
          dist)
    return order, dist


def song_to_song_order(seeds, candidates, metric="euclidean", m=None, k=None) -> np.ndarray:
    """Index form of song_to_song.  `k`: only the first k songs of the chain, through one chain_order call (k steps instead
    of one per candidate); None walks the whole pool."""
    if k is not None:
        X = rows_f32(candidates)
        k = min(int(k), X.shape[0])
        if k < 1:
            return np.zeros(0, np.uint32)
        idx, _ = chain_order([np.atleast_2d(np.asarray(seeds, dtype=np.float32))], X, k, metric, m)
        return idx[0][idx[0] >= 0].astype(np.uint32)
    S, X = rows_f32(seeds), rows_f32(candidates)
    order = np.empty(X.shape[0], np.uint32)
    _call("blissgpu_song_to_song", S, S.shape[0], X, X.shape[0], X.shape[1], _METRICS[metric], metric_matrix(metric, m), order)
    return order


def closest_to_songs(initial_songs, candidate_songs, metric_builder=euclidean_distance):
    """src/playlist.rs:256-270: candidates sorted (stably) by their distance to the set of initial songs."""
    candidate_songs = list(candidate_songs)
    if not candidate_songs:
        return []
    if isinstance(metric_builder, ForestOptions):
        order, _ = forest_closest_to_songs_order(_matrix(initial_songs), _matrix(candidate_songs), metric_builder)
        return [candidate_songs[i] for i in order]
    metric, m = (metric_builder, None) if isinstance(metric_builder, VarianceWeights) else _metric_of(metric_builder)
    order, _ = closest_to_songs_order(_matrix(initial_songs), _matrix(candidate_songs), metric, m)
    return [candidate_songs[i] for i in order]


def song_to_song(initial_songs, candidate_songs, metric_builder=euclidean_distance, number_songs=None):
    """src/playlist.rs:272-326: each song is followed by the remaining song closest to it.  `number_songs`: the first that
    many songs only (the reference's iterator with .take(number_songs)), computed in that many steps."""
    _no_forest(metric_builder, "song_to_song rebuilds its metric from one song after the first step (:285-295)")
    _no_variance(metric_builder, "song_to_song rebuilds its metric from one song after the first step (:285-295)")
    candidate_songs = list(candidate_songs)
    if not candidate_songs:
        return []
    metric, m = _metric_of(metric_builder)
    order = song_to_song_order(_matrix(initial_songs), _matrix(candidate_songs), metric, m, k=number_songs)
    return [candidate_songs[i] for i in order]


def nearest_order(queries, candidates, k, metric="euclidean", m=None, skip=None):
    """The k nearest candidates of every query in one device call, without the distance matrix: row i of the result is
    closest_to_songs(&[queries[i]], candidates without skip[i], metric) (src/playlist.rs:256-270) cut after k -- what
    Library::playlist_from(&[song]).take(k) asks per song (src/library.rs:762-850).  -> (idx int64[q, k], dist
    float32[q, k]); equal distances come in candidate order; rows with fewer than k eligible candidates end in -1 / inf.
    `skip`: None, or one candidate index per query that is left out of that query's list (-1: none).  Passing the same
    array object as queries and candidates uploads it once.  A NaN distance raises ValueError (the reference's n32()
    panic)."""
    X = rows_f32(candidates)
    Q = X if queries is candidates else rows_f32(queries)
    if Q.ndim != 2 or X.ndim != 2 or Q.shape[1] != X.shape[1]:
        raise ValueError("queries and candidates must be [q, d] and [n, d]")
    k = int(k)
    if k < 1:
        raise ValueError("k must be at least 1")
    q, d = Q.shape
    n = X.shape[0]
    if skip is not None:
        skip = skip_words(skip, q, n)
    idx, dist = np.empty((q, k), np.uint32), np.empty((q, k), np.float32)
    _call("blissgpu_knn", Q, q, X, n, d, _METRICS[metric], metric_matrix(metric, m), skip, k, idx, dist)
    return signed_idx(idx), dist


def nearest_songs(songs, candidate_songs, k, metric_builder=euclidean_distance, exclude_self=False):
    """For every song of `songs`, closest_to_songs(&[song], candidate_songs, metric_builder)[..k] (src/playlist.rs:256-270)
    -- all of them in one device call.  `exclude_self`: the first candidate that == the song (Song: PartialEq, as
    closest_album_to_group removes the group from its pool) is left out of that song's list."""
    _no_forest(metric_builder, "nearest_songs builds one metric per query song")
    _no_variance(metric_builder, "nearest_songs builds one metric per query song; use nearest_to_groups for seed sets")
    songs, candidate_songs = list(songs), list(candidate_songs)
    if not songs:
        return []
    if not candidate_songs:
        return [[] for _ in songs]
    metric, m = _metric_of(metric_builder)
    skip = None
    if exclude_self:
        skip = np.full(len(songs), -1, np.int64)
        for i, s in enumerate(songs):
            for j, c in enumerate(candidate_songs):
                if _song_of(c) == _song_of(s):
                    skip[i] = j
                    break
    idx, _ = nearest_order(_matrix(songs), _matrix(candidate_songs), k, metric, m, skip)
    return [[candidate_songs[j] for j in row if j >= 0] for row in idx]


def kmeans(X, init, max_iter=100, metric="euclidean", m=None):
    """Lloyd's k-means of the rows of X from the centres `init` [k, d] in one device call (blissgpu_kmeans): the nearest centre
    by the all-pairs distances with equal rounded distances going to the lower centre, the sequential f32 mean of every
    cluster's rows in row order, an empty cluster keeps its centre; stops when no label moves (converged) or after max_iter
    updates.  -> (labels int64[n], dist float32[n], centroids float32[k, d], sizes int64[k], n_iter, converged).  metric:
    "euclidean" or "mahalanobis" with m; "cosine" is refused (a mean does not minimise it).  A NaN distance raises ValueError."""
    if metric == "cosine":
        raise ValueError("k-means needs a metric its means minimise: euclidean or mahalanobis, not cosine")
    X, init = rows_f32(X), rows_f32(init)
    if X.ndim != 2 or init.ndim != 2 or X.shape[1] != init.shape[1]:
        raise ValueError("X and init must be [n, d] and [k, d]")
    max_iter = int(max_iter)
    if max_iter < 0:
        raise ValueError("max_iter must be at least 0")
    (n, d), k = X.shape, init.shape[0]
    labels, dist = np.empty(n, np.uint32), np.empty(n, np.float32)
    cent, sizes = np.empty((k, d), np.float32), np.empty(k, np.uint32)
    n_iter, conv = C.c_uint32(0), C.c_int32(0)
    _call("blissgpu_kmeans", X, n, d, init, k, _METRICS[metric], metric_matrix(metric, m), max_iter, labels, dist, cent, sizes,
          C.byref(n_iter), C.byref(conv))
    return labels.astype(np.int64), dist, cent, sizes.astype(np.int64), int(n_iter.value), bool(conv.value)


_KMEANS_INITS = ("k-means++", "sample")


def kmeans_init(X, k, seed=0, method="k-means++", _device=None):
    """k rows of X to start k-means from, [k, d]; the same seed gives the same rows (numpy's PCG64).
    "sample": rows numpy.random.Generator(PCG64(seed)).choice(n, k, replace=False), sorted -- host only.
    "k-means++": D^2 sampling -- the first row uniformly, every further row with probability proportional to the squared
    euclidean distance to the nearest row picked so far.  Each pick's n distances come from the device (Context.pairwise against
    the last pick); the running minimum and the draw are numpy.  A row at distance 0 from the picks (a picked row, or a
    duplicate of one) is never drawn while a row at a non-zero distance exists; after that the lowest unpicked rows follow."""
    X = rows_f32(X)
    n, k = X.shape[0], int(k)
    if method not in _KMEANS_INITS:
        raise ValueError(f"method must be one of {_KMEANS_INITS}")
    if k < 1 or k > n:
        raise ValueError("k must be 1 .. the number of rows")
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    if method == "sample":
        return X[np.sort(rng.choice(n, k, replace=False))].copy()
    if _device is None:
        import torch

        from .device import Context

        ctx = Context.default()
        Xd = torch.from_numpy(X).to(torch.device("cuda", ctx.device))
    else:  # (choose_k: the context and the rows it has uploaded already)
        ctx, Xd = _device
    picks = [int(rng.integers(n))]
    picked = np.zeros(n, bool)
    picked[picks[0]] = True
    d2 = None
    while len(picks) < k:
        last = ctx.pairwise(Xd, Xd[picks[-1]:picks[-1] + 1])[:, 0].cpu().numpy().astype(np.float64)
        d2 = last * last if d2 is None else np.minimum(d2, last * last)
        if np.isnan(d2).any():
            raise ValueError("NaN distance (noisy_float::n32 / argmin().unwrap() panic in the reference)")
        cum = np.cumsum(d2)
        total = cum[-1]
        if total > 0.0:
            # cum[i - 1] <= r < cum[i]: row i has d2 > 0; a product rounded up to the total falls back to the last such row
            i = int(np.searchsorted(cum, rng.random() * total, side="right"))
            if i >= n or d2[i] == 0.0:
                i = int(np.flatnonzero(d2 > 0.0)[-1])
        else:
            i = int(np.flatnonzero(~picked)[0])
        picks.append(i)
        picked[i] = True
    return X[np.asarray(picks)].copy()


class Clustering:
    """The result of cluster_songs: labels int64[n], distances float32[n] (to the song's own centre), centroids float32[k, d],
    sizes int64[k], n_iter (updates made), converged, and inertia = the float64 sum of the squared distances."""

    def __init__(self, labels, distances, centroids, sizes, n_iter, converged):
        self.labels = np.asarray(labels, dtype=np.int64)
        self.distances = np.asarray(distances, dtype=np.float32)
        self.centroids = np.asarray(centroids, dtype=np.float32)
        self.sizes = np.asarray(sizes, dtype=np.int64)
        self.n_iter, self.converged = int(n_iter), bool(converged)
        self.inertia = float(np.sum(self.distances.astype(np.float64) ** 2))

    def members(self, c) -> np.ndarray:
        """Row indices of cluster c ordered by (distance, index): the songs most typical of the cluster first."""
        rows = np.flatnonzero(self.labels == int(c))
        return rows[np.lexsort((rows, self.distances[rows]))]

    def __repr__(self):
        return (f"Clustering(k={len(self.sizes)}, n={len(self.labels)}, n_iter={self.n_iter}, converged={self.converged}, "
                f"inertia={self.inertia:.6g})")


def _kmeans_metric(metric_builder):
    """the metrics k-means can run: euclidean, or Mahalanobis with the caller's matrix"""
    return _plain_metric(metric_builder, "k-means assigns single songs to centres and needs a metric its means minimise",
                         "k-means has no seed set to take variances from; pass MahalanobisBuilder(m)",
                         "k-means needs a metric its means minimise: euclidean or mahalanobis, not cosine")


def cluster_songs(songs, k, seed=0, metric_builder=euclidean_distance, max_iter=100, init="k-means++") -> Clustering:
    """Which k groups the songs fall into: k-means of their analyses (kmeans) from kmeans_init(rows, k, seed, init).
    -> Clustering; `members(c)` lists cluster c's songs, the most typical first.  metric_builder: euclidean_distance or a
    MahalanobisBuilder (its M); a ForestOptions, a VarianceWeights, cosine and arbitrary callables are refused."""
    metric, m = _kmeans_metric(metric_builder)
    songs = list(songs)
    if not songs:
        raise ValueError("cluster_songs needs at least one song")
    X = _matrix(songs)
    return Clustering(*kmeans(X, kmeans_init(X, k, seed, init), max_iter, metric, m))


def _silhouette_metric(metric_builder):
    """the metrics the silhouette can run: euclidean, or Mahalanobis with the caller's matrix"""
    return _plain_metric(metric_builder, "the silhouette compares single songs; a forest scores songs against a seed set",
                         "the silhouette has no seed set to take variances from; pass MahalanobisBuilder(m)",
                         "the silhouette needs the metric the groups are judged by: euclidean or mahalanobis, not cosine")


def _rows_of_input(songs_or_X) -> np.ndarray:
    """[n, d] float32 from an array or from songs"""
    if isinstance(songs_or_X, np.ndarray):
        return rows_f32(songs_or_X)
    items = list(songs_or_X)
    if items and hasattr(_song_of(items[0]), "analysis"):
        return _matrix(items)
    return rows_f32(np.asarray(items, dtype=np.float32))


def _index_array(a, what):
    a = np.asarray(a, dtype=np.int64).reshape(-1)
    if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
        raise ValueError(f"{what} must be non-negative indices")
    return np.ascontiguousarray(a, dtype=np.uint32)


class Silhouette:
    """The silhouette of a labelling: values float32[q] (s of every scored song), a and b float64[q] (the mean distance to the
    own cluster / to the nearest other one), neighbour int64[q] (that cluster), sizes int64[k], labels int64[q] (the cluster of
    every scored song), and the aggregates -- score = math.fsum(values) / q and cluster_scores float64[k] = the fsum mean of
    every cluster's scored members, NaN where none was scored.  fsum is correctly rounded: the aggregates have no order."""

    def __init__(self, values, a, b, neighbour, sizes, labels):
        import math

        self.values = np.asarray(values, dtype=np.float32)
        self.a, self.b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        self.neighbour = np.asarray(neighbour, dtype=np.int64)
        self.sizes = np.asarray(sizes, dtype=np.int64)
        self.labels = np.asarray(labels, dtype=np.int64)
        q = self.values.shape[0]
        self.score = math.fsum(float(v) for v in self.values) / q if q else float("nan")
        self.cluster_scores = np.full(self.sizes.shape[0], np.nan, np.float64)
        for c in np.unique(self.labels):
            v = self.values[self.labels == c]
            self.cluster_scores[int(c)] = math.fsum(float(x) for x in v) / v.shape[0]

    def __repr__(self):
        return f"Silhouette(score={self.score:.6g}, scored={len(self.values)}, k={len(self.sizes)})"


def silhouette(X, labels, metric_builder=euclidean_distance, rows=None, k=None, col_groups=0) -> Silhouette:
    """How well the labelling `labels` (one cluster index per row) separates the rows of X (an array, or songs) under a
    metric, in one device call without the distance matrix (blissgpu_silhouette): for every scored song
    a = the mean distance to the other songs of its cluster, b = the smallest mean distance to another non-empty cluster,
    s = (b - a) / max(a, b) in [-1, 1]; a singleton scores 0.  Every value is defined to the bit by include/blissgpu.h.
    rows: the songs to score (any order, repeats allowed; value p belongs to song rows[p]), None = all.  k: the number of
    clusters, None = labels.max() + 1.  col_groups is for the tests and the bench tool (no result bit depends on it).
    metric_builder: euclidean_distance or a MahalanobisBuilder (its M) -- the before / after check of learn_metric; a
    ForestOptions, a VarianceWeights, cosine and arbitrary callables are refused.  Fewer than two non-empty clusters, a label
    >= k or a row past the songs raise BlissGpuError(ERR_INVALID), a NaN distance ValueError."""
    metric, m = _silhouette_metric(metric_builder)
    X = _rows_of_input(X)
    lab = _index_array(labels, "labels")
    n, d = X.shape
    if lab.shape[0] != n:
        raise ValueError("a label per row of X is needed")
    if n == 0:
        raise ValueError("silhouette needs at least one song")
    k = int(lab.max()) + 1 if k is None else int(k)
    q = n
    if rows is not None:
        rows = _index_array(rows, "rows")
        q = rows.shape[0]
    s, a, b = np.zeros(q, np.float32), np.zeros(q, np.float64), np.zeros(q, np.float64)
    nb, sizes = np.zeros(q, np.uint32), np.zeros(max(k, 0), np.uint32)
    _call("blissgpu_silhouette", X, n, d, lab, k, _METRICS[metric], metric_matrix(metric, m), rows, q, int(col_groups), s, a, b, nb,
          sizes)
    return Silhouette(s, a, b, nb, sizes, lab if rows is None else lab[rows])


@dataclasses.dataclass
class GroupNeighbours:
    """The result of group_neighbours: idx int64[q, t] (row g: the t groups nearest to queries[g], ascending; -1 = padding),
    dist float64[q, t] (their distances; +inf = padding), sizes int64[k] (the members per group) and matrix float64[k, k] (every
    A(a, c); None unless asked for)."""

    idx: np.ndarray
    dist: np.ndarray
    sizes: np.ndarray
    matrix: Optional[np.ndarray] = None


def _group_neighbours_metric(metric_builder):
    """the metrics the group distances can run: euclidean, or Mahalanobis with the caller's matrix"""
    return _plain_metric(metric_builder, "the group distances compare single songs; a forest scores songs against a seed set",
                         "the group distances have no seed set to take variances from; pass MahalanobisBuilder(m)",
                         "the group distances need a distance a nearest member is defined with: euclidean or mahalanobis, not cosine")


def group_neighbours(songs_or_X, labels, t, metric_builder=euclidean_distance, k=None, queries=None, mode="symmetric", matrix=False,
                     slab_groups=0) -> GroupNeighbours:
    """Which groups of a labelling (artists, albums, genres, clusters) are like each other: for every queried group its t
    nearest groups under the average nearest-member (Chamfer) distance, in one device call without the distance matrix
    (blissgpu_group_neighbours).  For every song of group a the distance to the closest song of group c,
    averaged over a: mode "directed" keeps that ("how well c covers a"), "symmetric" takes the mean of the two directions.
    Every value is defined to the bit by include/blissgpu.h.  labels: one group index per row (an array, or songs' rows); rows
    with a label < 0 are left out.  k: the number of groups, None = labels.max() + 1.  queries: the groups to answer for (any
    order, repeats allowed), None = all k in order.  matrix: also return every A(a, c).  slab_groups is for the tests and the
    bench tool (no result bit depends on it).  metric_builder: euclidean_distance or a MahalanobisBuilder (its M); a
    ForestOptions, a VarianceWeights, cosine and arbitrary callables are refused.  A label >= k or a query >= k raise
    BlissGpuError(ERR_INVALID), a NaN distance ValueError."""
    metric, m = _group_neighbours_metric(metric_builder)
    if mode not in _GROUP_MODES:
        raise ValueError(f"mode must be one of {tuple(_GROUP_MODES)}")
    X = _rows_of_input(songs_or_X)
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    if lab.shape[0] != X.shape[0]:
        raise ValueError("a label per row of X is needed")
    keep = lab >= 0
    if not keep.all():
        X, lab = np.ascontiguousarray(X[keep]), lab[keep]
    lab = _index_array(lab, "labels")
    n, d = X.shape
    k = (int(lab.max()) + 1 if n else 1) if k is None else int(k)
    t = int(t)
    q = max(k, 0)
    if queries is not None:
        queries = _index_array(queries, "queries")
        q = queries.shape[0]
    idx, dist = np.full((q, max(t, 0)), 0xFFFFFFFF, np.uint32), np.full((q, max(t, 0)), np.inf, np.float64)
    sizes = np.zeros(max(k, 0), np.uint32)
    mat = np.zeros((max(k, 0), max(k, 0)), np.float64) if matrix else None
    _call("blissgpu_group_neighbours", X, n, d, lab, k, _METRICS[metric], metric_matrix(metric, m), queries, q, t, _GROUP_MODES[mode],
          int(slab_groups), idx, dist, sizes, mat)
    return GroupNeighbours(signed_idx(idx), dist, sizes.astype(np.int64), mat)


def _mst_metric(metric_builder):
    """the metrics the spanning tree can run: euclidean, or Mahalanobis with the caller's matrix"""
    return _plain_metric(metric_builder, "the spanning tree compares single songs; a forest scores songs against a seed set",
                         "the spanning tree has no seed set to take variances from; pass MahalanobisBuilder(m)",
                         "the spanning tree needs a distance whose bits order as integers: euclidean or mahalanobis, not cosine")


def _uf_find(parent, x):
    r = x
    while parent[r] != r:
        r = parent[r]
    while parent[x] != r:
        parent[x], x = r, parent[x]
    return r


@dataclasses.dataclass
class SpanningTree:
    """The result of minimum_spanning_tree: the n - 1 edges of the library's minimum spanning tree in ascending order of
    (bits of w, u, v) -- u int64[n - 1] (the lower song), v int64[n - 1] (the higher), w float32[n - 1] -- and `rounds`, the
    Boruvka rounds the device ran.  n is the number of songs.  linkage / cut / tour are host work on those arrays."""

    u: np.ndarray
    v: np.ndarray
    w: np.ndarray
    rounds: int
    n: int

    def linkage(self) -> np.ndarray:
        """The single-linkage dendrogram as scipy lays it out: float64 [n - 1, 4], row e = (cluster a, cluster b, height, size)
        with a < b; the merges are the edges in their order, the cluster made by row e is numbered n + e."""
        m = len(self.u)
        Z = np.zeros((m, 4), np.float64)
        parent, ident, size = list(range(self.n)), list(range(self.n)), [1] * self.n
        for e in range(m):
            ra, rb = _uf_find(parent, int(self.u[e])), _uf_find(parent, int(self.v[e]))
            a, b = sorted((ident[ra], ident[rb]))
            parent[rb] = ra
            size[ra] += size[rb]
            ident[ra] = self.n + e
            Z[e] = (a, b, float(self.w[e]), size[ra])
        return Z

    def cut(self, k: int = None, height: float = None, min_cluster_size: int = 1) -> np.ndarray:
        """Single-linkage clusters: int64 labels [n].  k: remove the k - 1 last edges of the order (k clusters); height: remove
        every edge with w > height (an edge of exactly that weight stays); neither: one cluster.  The clusters are numbered
        0, 1, ... by their lowest member; clusters of fewer than min_cluster_size songs get -1 (which silhouette,
        group_neighbours and moments leave out) and the others keep the order of their lowest members."""
        if k is not None and height is not None:
            raise ValueError("cut takes k or height, not both")
        m = len(self.u)
        keep = m
        if k is not None:
            k = int(k)
            if not 1 <= k <= max(self.n, 1):
                raise ValueError("k must be 1 .. n")
            keep = max(self.n - k, 0)
        elif height is not None:
            keep = int(np.count_nonzero(~(self.w > np.float32(height))))  # (ascending weights: a prefix of the order)
        parent = list(range(self.n))
        for e in range(keep):
            ra, rb = _uf_find(parent, int(self.u[e])), _uf_find(parent, int(self.v[e]))
            parent[max(ra, rb)] = min(ra, rb)  # the root is the lowest member
        roots = np.fromiter((_uf_find(parent, i) for i in range(self.n)), np.int64, self.n)
        sizes = np.bincount(roots, minlength=self.n)
        big = sizes[roots] >= int(min_cluster_size)
        label_of = np.full(max(self.n, 1), -1, np.int64)
        live = np.unique(roots[big])  # ascending roots = ascending lowest members
        label_of[live] = np.arange(live.size)
        return label_of[roots]

    def tour(self, start: int = 0) -> np.ndarray:
        """Every song once, int64 [n]: the depth-first preorder of the tree from `start`, a song's neighbours taken in ascending
        edge order.  Each song is a neighbour in the tree of one heard before it, and the whole walk is at most twice the
        tree's length: no jumps across the library once the near songs run out."""
        if self.n == 0:
            return np.zeros(0, np.int64)
        start = int(start)
        if not 0 <= start < self.n:
            raise ValueError("start must be a song of the tree")
        deg = np.bincount(np.concatenate([self.u, self.v]).astype(np.int64), minlength=self.n)
        off = np.concatenate([[0], np.cumsum(deg)]).tolist()
        fill, adj = off[:-1], [0] * (2 * len(self.u))
        for a, b in zip(self.u.tolist(), self.v.tolist()):  # edge order: every list ascends in edge key
            adj[fill[a]] = b
            fill[a] += 1
            adj[fill[b]] = a
            fill[b] += 1
        out, seen, stack = [], [False] * self.n, [start]
        while stack:  # (iterative: a chain of a million songs is a valid tree)
            i = stack.pop()
            if seen[i]:
                continue
            seen[i] = True
            out.append(i)
            stack.extend(j for j in reversed(adj[off[i]:off[i + 1]]) if not seen[j])
        return np.asarray(out, np.int64)


def core_distances(songs_or_X, min_samples, metric_builder=euclidean_distance) -> np.ndarray:
    """Every song's distance to its min_samples-th nearest OTHER song (float32 [n]; with fewer other songs, to the farthest of
    them; 0 for a lone song): the "core distance" of HDBSCAN, from the k-nearest search on the device (nearest_order).  Small
    in dense regions, large for outliers."""
    metric, m = _mst_metric(metric_builder)
    X = _rows_of_input(songs_or_X)
    n = X.shape[0]
    k = int(min_samples)
    if k < 1:
        raise ValueError("min_samples must be at least 1")
    k = min(k, n - 1)
    if k < 1:
        return np.zeros(n, np.float32)
    _, dist = nearest_order(X, X, k, metric, m, skip=np.arange(n))
    return np.ascontiguousarray(dist[:, k - 1], dtype=np.float32)


def minimum_spanning_tree(songs_or_X, metric_builder=euclidean_distance, min_samples=None) -> SpanningTree:
    """The minimum spanning tree of the songs (or rows of an array) under a metric, exact and without the distance matrix
    (blissgpu_mst): Boruvka's rounds on the device, at most ceil(log2 n) all-pairs scans.  The tree is the
    unique one under the edge order (bits of the weight, lower song, higher song), so ties -- duplicate songs -- change nothing.
    -> SpanningTree; its cut() gives clusters without a number of clusters and of any shape (single linkage), its linkage() the
    whole dendrogram, its tour() every song in an order without jumps.  min_samples = m: the weights become the mutual
    reachability max(distance, core[i], core[j]) with core = core_distances(songs, m): sparse songs are pushed away from
    everything, which keeps single linkage from chaining through noise (the tree HDBSCAN starts from).  metric_builder:
    euclidean_distance or a MahalanobisBuilder (its M); a ForestOptions, a VarianceWeights, cosine and arbitrary callables are
    refused.  A NaN distance raises BlissGpuError(ERR_INVALID)."""
    metric, m = _mst_metric(metric_builder)
    X = _rows_of_input(songs_or_X)
    n, d = X.shape
    core = None if min_samples is None else core_distances(X, min_samples, metric_builder)
    e = max(n - 1, 0)
    u, v, w = np.zeros(e, np.uint32), np.zeros(e, np.uint32), np.zeros(e, np.float32)
    rounds = C.c_uint32(0)
    _ffi.call("blissgpu_mst", X, n, d, _METRICS[metric], metric_matrix(metric, m), core, u, v, w, C.byref(rounds))
    return SpanningTree(u.astype(np.int64), v.astype(np.int64), w, int(rounds.value), n)


# ---- Ward clustering: the whole dendrogram (blissgpu_ward / blissgpu_ward_nearest) ----
def _ward_metric(metric_builder):
    """the metrics Ward clustering can run: euclidean, or Mahalanobis with the caller's matrix"""
    return _plain_metric(metric_builder, "Ward clustering merges clusters by their centroids; a forest scores songs against a seed set",
                         "Ward clustering has no seed set to take variances from; pass MahalanobisBuilder(m)",
                         "Ward clustering needs a metric whose squares its centroids minimise: euclidean or mahalanobis, not cosine")


def ward_nearest(C_rows, sizes=None, metric_builder=euclidean_distance):
    """One scan of Ward clustering (blissgpu_ward_nearest): for every row of C_rows -- a cluster's centroid, with `sizes` songs in
    it (None: 1 each) -- the other row that is cheapest to merge with under cost = |A| |B| / (|A| + |B|) * dist^2, ties to the
    smallest i XOR j.  -> (nn int64 [m], cost float32 [m]); one row alone has nn = -1 and cost = +inf.  Every bit is defined by
    include/blissgpu.h.  metric_builder: as ward_tree."""
    metric, m = _ward_metric(metric_builder)
    X = _rows_of_input(C_rows)
    n, d = X.shape
    if sizes is not None:
        sizes = _index_array(sizes, "sizes")
        if sizes.shape[0] != n:
            raise ValueError("a size per row is needed")
    nn, cost = np.zeros(n, np.uint32), np.zeros(n, np.float32)
    _ffi.call("blissgpu_ward_nearest", X, sizes, n, d, _METRICS[metric], metric_matrix(metric, m), nn, cost)
    return signed_idx(nn), cost


@dataclasses.dataclass
class WardTree:
    """The result of ward_tree: the n - 1 merges of Ward's dendrogram in ascending order of (bits of cost, round, u) -- u int64
    (the lowest song of the one cluster), v int64 (of the other, u < v), cost float32 (the growth of the within-cluster sum of
    squares), size int64 (songs in the merged cluster), round int64 (the device round that made it) -- and `rounds`, the rounds
    run.  n is the number of songs.  heights / within / linkage / cut are host work on those arrays."""

    u: np.ndarray
    v: np.ndarray
    cost: np.ndarray
    size: np.ndarray
    round: np.ndarray
    rounds: int
    n: int

    def heights(self) -> np.ndarray:
        """float64 [n - 1]: sqrt(2 cost), the height scipy's linkage(X, "ward") gives the merge (under euclidean)"""
        return np.sqrt(2.0 * self.cost.astype(np.float64))

    def within(self) -> np.ndarray:
        """float64 [n - 1]: the running sum of the costs = the within-cluster sum of squares after each merge (the elbow curve),
        up to the rounding of the costs"""
        return np.cumsum(self.cost.astype(np.float64))

    def linkage(self) -> np.ndarray:
        """The dendrogram as scipy lays it out: float64 [n - 1, 4], row e = (cluster a, cluster b, height, size) with a < b and
        height = heights()[e]; the merges are the edges in their order, the cluster made by row e is numbered n + e."""
        m = len(self.u)
        Z = np.zeros((m, 4), np.float64)
        h = self.heights()
        parent, ident, size = list(range(self.n)), list(range(self.n)), [1] * self.n
        for e in range(m):
            ra, rb = _uf_find(parent, int(self.u[e])), _uf_find(parent, int(self.v[e]))
            a, b = sorted((ident[ra], ident[rb]))
            parent[rb] = ra
            size[ra] += size[rb]
            ident[ra] = self.n + e
            Z[e] = (a, b, h[e], size[ra])
        return Z

    def cut(self, k: int = None, cost: float = None, min_cluster_size: int = 1) -> np.ndarray:
        """Ward's clusters: int64 labels [n].  k: undo the k - 1 last merges of the order (k clusters, each a union of clusters
        of k + 1); cost: undo every merge with cost > `cost` (a merge of exactly that cost stays); neither: one cluster.  The
        clusters are numbered 0, 1, ... by their lowest member; clusters of fewer than min_cluster_size songs get -1 (which
        silhouette, group_neighbours and moments leave out) and the others keep the order of their lowest members."""
        if k is not None and cost is not None:
            raise ValueError("cut takes k or cost, not both")
        m = len(self.u)
        keep = m
        if k is not None:
            k = int(k)
            if not 1 <= k <= max(self.n, 1):
                raise ValueError("k must be 1 .. n")
            keep = max(self.n - k, 0)
        elif cost is not None:
            keep = int(np.count_nonzero(~(self.cost > np.float32(cost))))  # (ascending costs: a prefix of the order)
        parent = list(range(self.n))
        for e in range(keep):
            ra, rb = _uf_find(parent, int(self.u[e])), _uf_find(parent, int(self.v[e]))
            parent[max(ra, rb)] = min(ra, rb)  # the root is the lowest member
        roots = np.fromiter((_uf_find(parent, i) for i in range(self.n)), np.int64, self.n)
        sizes = np.bincount(roots, minlength=self.n)
        big = sizes[roots] >= int(min_cluster_size)
        label_of = np.full(max(self.n, 1), -1, np.int64)
        live = np.unique(roots[big])  # ascending roots = ascending lowest members
        label_of[live] = np.arange(live.size)
        return label_of[roots]


def _empty_ward_tree(n=0) -> WardTree:
    z = np.zeros(0, np.int64)
    return WardTree(z, z.copy(), np.zeros(0, np.float32), z.copy(), z.copy(), 0, int(n))


def ward_tree(songs_or_X, metric_builder=euclidean_distance) -> WardTree:
    """Ward's minimum-variance dendrogram of the songs (or rows of an array), without the distance matrix (blissgpu_ward,
    DESIGN.md 3.32): a nested hierarchy of compact clusters -- any K by cutting one tree, K clusters always a refinement of
    K - 1; the hierarchical counterpart of k-means.  Every pair of clusters that are each other's nearest merges in the same
    round: a few dozen all-pairs scans of a shrinking set of centroids on the device.  The rounds and their roundings are
    defined to the bit by include/blissgpu.h.  -> WardTree; its cut() gives the clusters, its linkage() scipy's layout, its
    within() the elbow curve.  metric_builder: euclidean_distance or a MahalanobisBuilder (its M); a ForestOptions, a
    VarianceWeights, cosine and arbitrary callables are refused.  A NaN cost raises BlissGpuError(ERR_INVALID)."""
    metric, m = _ward_metric(metric_builder)
    X = _rows_of_input(songs_or_X)
    n, d = X.shape
    e = max(n - 1, 0)
    u, v, size, rnd = (np.zeros(e, np.uint32) for _ in range(4))
    cost = np.zeros(e, np.float32)
    rounds = C.c_uint32(0)
    _ffi.call("blissgpu_ward", X, n, d, _METRICS[metric], metric_matrix(metric, m), u, v, cost, size, rnd, C.byref(rounds))
    return WardTree(u.astype(np.int64), v.astype(np.int64), cost, size.astype(np.int64), rnd.astype(np.int64), int(rounds.value), n)


# ---- k-medoids: K songs that summarise a library, under any metric (blissgpu_kmedoids / blissgpu_pam_scan) ----
def _pam_metric(metric_builder):
    """the metrics k-medoids can run: every one the all-pairs kernel knows -- euclidean, cosine, Mahalanobis with the caller's M"""
    return _plain_metric(metric_builder, "k-medoids compares single songs; a forest scores songs against a seed set",
                         "k-medoids has no seed set to take variances from; pass MahalanobisBuilder(m)")


def pam_scan(songs_or_X, near, d1, d2, k, metric_builder=euclidean_distance, rows=None, return_sums=False):
    """One scan of k-medoids (blissgpu_pam_scan): under the state near int [n] (every song's medoid slot, < k), d1 / d2 float32 [n]
    (its distances to the nearest and the second nearest medoid), what would the total distance change by if song c became a
    medoid?  For every candidate c of `rows` (None: every song; any order, repeats allowed): btot float64 -- c joins and every
    medoid stays --, best float64 and arg int64 -- c takes the place of the medoid in slot arg, the best slot for it.
    return_sums: also A and B float64 [q, k], the two sums per (candidate, slot) that best is made of.  -> (btot, best, arg) or
    (btot, best, arg, A, B).  Every bit is defined by include/blissgpu.h.  A NaN distance raises BlissGpuError(ERR_NAN)."""
    metric, m = _pam_metric(metric_builder)
    X = _rows_of_input(songs_or_X)
    n, d = X.shape
    k = int(k)
    near = _index_array(near, "near")
    d1 = np.ascontiguousarray(d1, dtype=np.float32).reshape(-1)
    d2 = np.ascontiguousarray(d2, dtype=np.float32).reshape(-1)
    if not (near.shape[0] == d1.shape[0] == d2.shape[0] == n):
        raise ValueError("near, d1 and d2 hold one entry per row")
    q = n
    if rows is not None:
        rows = _index_array(rows, "rows")
        q = rows.shape[0]
    btot, best, arg = np.zeros(q, np.float64), np.zeros(q, np.float64), np.zeros(q, np.uint32)
    A = np.zeros((q, k), np.float64) if return_sums else None
    B = np.zeros((q, k), np.float64) if return_sums else None
    _ffi.call("blissgpu_pam_scan", X, n, d, near, d1, d2, k, _METRICS[metric], metric_matrix(metric, m), rows, q, btot, best, arg, A, B)
    out = (btot, best, arg.astype(np.int64))
    return out + (A, B) if return_sums else out


@dataclasses.dataclass
class Medoids:
    """The result of kmedoids: medoids int64 [k] (songs, in slot order), labels int64 [n] (every song's slot: its nearest
    medoid, equal distances to the lower slot), dist float32 [n] (the distance to it), sizes int64 [k], td (the total distance
    float64 = td_trace[-1]), td_trace float64 [n_swaps + 1] (TD before every round), n_swaps, converged."""

    medoids: np.ndarray
    labels: np.ndarray
    dist: np.ndarray
    sizes: np.ndarray
    td: float
    td_trace: np.ndarray
    n_swaps: int
    converged: bool

    def members(self, c) -> np.ndarray:
        """the songs of slot c, nearest to the medoid first (equal distances in song order)"""
        idx = np.flatnonzero(self.labels == c)
        return idx[np.argsort(self.dist[idx], kind="stable")]


def kmedoids(songs_or_X, k, metric_builder=euclidean_distance, init="build", max_swaps=None) -> Medoids:
    """k-medoids (PAM) of the songs (or rows of an array) on the device (blissgpu_kmedoids): the k SONGS whose
    total distance TD = sum over the songs of the distance to the nearest of them is a local minimum under single swaps.  It
    needs only pairwise distances, so cosine_distance and a MahalanobisBuilder work as euclidean_distance does.  init: "build"
    (the greedy start: the song with the smallest sum of distances, then k - 1 times the song that lowers TD most) or k distinct
    row indices.  Each round scans every (candidate, song) pair and makes the one swap that lowers TD most; it ends when no swap
    lowers it (converged) or after max_swaps swaps (None: 4 k + 64).  Every bit is defined by include/blissgpu.h.  A
    ForestOptions, a VarianceWeights and arbitrary callables are refused.  A NaN distance (a zero row under cosine) raises
    BlissGpuError(ERR_NAN)."""
    metric, m = _pam_metric(metric_builder)
    X = _rows_of_input(songs_or_X)
    n, d = X.shape
    k = int(k)
    if not 1 <= k <= max(n, 1):
        raise ValueError("k must be 1 .. the number of rows")
    if isinstance(init, str):
        if init != "build":
            raise ValueError('init must be "build" or k row indices')
        init = None
    else:
        init = _index_array(init, "init")
        if init.shape[0] != k:
            raise ValueError("init must hold k row indices")
    max_swaps = 4 * k + 64 if max_swaps is None else int(max_swaps)
    if max_swaps < 0:
        raise ValueError("max_swaps must be at least 0")
    med, sizes, labels = np.zeros(k, np.uint32), np.zeros(k, np.uint32), np.zeros(n, np.uint32)
    dist, trace = np.zeros(n, np.float32), np.zeros(max_swaps + 1, np.float64)
    swaps, conv = C.c_uint32(0), C.c_int32(0)
    _ffi.call("blissgpu_kmedoids", X, n, d, k, _METRICS[metric], metric_matrix(metric, m), init, max_swaps, med, labels, dist, sizes,
              trace, C.byref(swaps), C.byref(conv))
    trace = trace[: int(swaps.value) + 1] if n else trace[:0]
    return Medoids(med.astype(np.int64), labels.astype(np.int64), dist, sizes.astype(np.int64), float(trace[-1]) if n else 0.0, trace,
                   int(swaps.value), bool(conv.value))


def medoid_songs(songs, k, metric_builder=euclidean_distance, init="build", max_swaps=None, return_medoids=False):
    """The k songs that summarise `songs` (kmedoids), and what each stands for.  -> (representatives, clusters): k `Song`s, and
    per representative the list of the songs nearest to it, nearest first (the representative itself leads its list, unless a
    duplicate of it comes earlier).  The representatives can seed playlist_from, radio_playlist or group_playlists as they are.
    return_medoids: -> (representatives, clusters, Medoids)."""
    _pam_metric(metric_builder)
    songs = list(songs)
    if not songs:
        raise ValueError("medoid_songs needs at least one song")
    res = kmedoids(_matrix(songs), k, metric_builder, init, max_swaps)
    reps = [songs[int(i)] for i in res.medoids]
    clusters = [[songs[int(i)] for i in res.members(c)] for c in range(len(res.medoids))]
    return (reps, clusters, res) if return_medoids else (reps, clusters)


# ---- locally scaled nearest songs and hubness (blissgpu_scaled_knn / blissgpu_knn_occurrence) ----
SCALE_MIN, SCALE_MAX = np.float32(2.0 ** -60), np.float32(2.0 ** 60)  # the scales blissgpu_scaled_knn accepts


def _scaled_metric(metric_builder, what):
    return _plain_metric(metric_builder, f"{what} compares single songs; a forest scores songs against a seed set",
                         f"{what} has no seed set to take variances from; pass MahalanobisBuilder(m)")


def scales_from_distances(dist, m, kind="mean") -> np.ndarray:
    """A local scale per row of `dist` (float32 [q, k]: every song's ascending neighbour distances as nearest_order returns
    them, short rows padded with inf), device-free.  With c = min(m, the row's finite entries): kind="mean" (NICDM) is the
    float64 sum of the first c distances, added in order, divided by c and rounded to float32; kind="kth" (Zelnik-Manor and
    Perona's sigma) is entry c - 1, which with min_samples = m is core_distances.  A row without a finite entry gets 1.
    Results below 2^-60 -- songs whose m nearest are exact duplicates -- are raised to the smallest result that is not below
    2^-60 (1 when there is none), results above 2^60 become 2^60: every scale is one blissgpu_scaled_knn accepts."""
    if kind not in ("mean", "kth"):
        raise ValueError('kind must be "mean" or "kth"')
    m = int(m)
    if m < 1:
        raise ValueError("m must be at least 1")
    D = np.asarray(dist, dtype=np.float32)
    if D.ndim != 2:
        raise ValueError("dist must be [q, k]")
    if np.isnan(D).any():
        raise ValueError("NaN distance")
    q = D.shape[0]
    c = np.minimum(m, np.isfinite(D).sum(axis=1))
    out = np.ones(q, np.float32)
    rows = np.flatnonzero(c > 0)
    last = c[rows] - 1
    if kind == "mean":
        sums = np.cumsum(D.astype(np.float64), axis=1)  # (sequential: the first c terms in order)
        out[rows] = (sums[rows, last] / c[rows]).astype(np.float32)
    else:
        out[rows] = D[rows, last]
    ok = out >= SCALE_MIN
    out[~ok] = out[ok].min() if ok.any() else np.float32(1.0)
    return np.minimum(out, SCALE_MAX)


def local_scales(songs_or_X, m=10, kind="mean", metric_builder=euclidean_distance) -> np.ndarray:
    """Every song's own idea of "near" (float32 [n]): scales_from_distances over its m nearest OTHER songs, from one k-nearest
    search on the device (nearest_order, every song skipping itself).  A lone song gets 1."""
    metric, mm = _scaled_metric(metric_builder, "local_scales")
    X = _rows_of_input(songs_or_X)
    n = X.shape[0]
    m = int(m)
    if m < 1:
        raise ValueError("m must be at least 1")
    k = min(m, n - 1)
    if k < 1:
        return np.ones(n, np.float32)
    _, dist = nearest_order(X, X, k, metric, mm, skip=np.arange(n))
    return scales_from_distances(dist, m, kind)


def scaled_nearest_order(queries, qscale, candidates, cscale, k, metric="euclidean", m=None, skip=None):
    """nearest_order under the locally scaled distance dist(i, j) / sqrt(qscale[i] * cscale[j]) (float32 throughout: the
    product rounded once, the correctly rounded root, true division; blissgpu_scaled_knn) -- the cure for
    hubs, the few songs a raw search puts into everyone's list.  -> (idx int64[q, k], scaled dist float32[q, k]); equal SCALED
    distances come in candidate order; rows with fewer than k eligible candidates end in -1 / inf.  Scales must lie in
    [2^-60, 2^60] (local_scales / scales_from_distances return such), else BlissGpuError(ERR_INVALID).  Passing the same array
    objects as queries / candidates and as qscale / cscale uploads each once.  A NaN distance raises ValueError."""
    X = rows_f32(candidates)
    Q = X if queries is candidates else rows_f32(queries)
    if Q.ndim != 2 or X.ndim != 2 or Q.shape[1] != X.shape[1]:
        raise ValueError("queries and candidates must be [q, d] and [n, d]")
    cs = np.ascontiguousarray(cscale, dtype=np.float32).reshape(-1)
    qs = cs if (qscale is cscale and Q is X) else np.ascontiguousarray(qscale, dtype=np.float32).reshape(-1)
    k = int(k)
    if k < 1:
        raise ValueError("k must be at least 1")
    q, d = Q.shape
    n = X.shape[0]
    if qs.shape[0] != q or cs.shape[0] != n:
        raise ValueError("qscale needs one entry per query and cscale one per candidate")
    if skip is not None:
        skip = skip_words(skip, q, n)
    idx, dist = np.empty((q, k), np.uint32), np.empty((q, k), np.float32)
    _call("blissgpu_scaled_knn", Q, q, qs, X, n, cs, d, _METRICS[metric], metric_matrix(metric, m), skip, k, idx, dist)
    return signed_idx(idx), dist


def _lists(idx):
    """[q, k] int64 with -1 padding from an index matrix"""
    idx = np.asarray(idx)
    if idx.ndim != 2:
        raise ValueError("idx must be [q, k]")
    if idx.dtype == np.uint32:
        return signed_idx(idx)
    out = idx.astype(np.int64)
    if (out < -1).any() or (out >= 0xFFFFFFFF).any():
        raise ValueError("idx entries must be song indices or -1")
    return out


def k_occurrence(idx, n) -> np.ndarray:
    """In how many lists every song is: int64 [n], count[j] = the entries of idx [q, k] equal to j, counted on the device
    (blissgpu_knn_occurrence).  -1 entries (padding) are ignored; any other entry outside 0 .. n - 1 is
    BlissGpuError(ERR_INVALID)."""
    L = _lists(idx)
    n = int(n)
    if n < 0:
        raise ValueError("n must not be negative")
    q, k = L.shape
    if k < 1:
        raise ValueError("idx needs at least one column")
    u = np.ascontiguousarray(np.where(L < 0, 0xFFFFFFFF, L), dtype=np.uint32)
    count = np.zeros(max(n, 1), np.uint32)
    _ffi.call("blissgpu_knn_occurrence", u if q else None, q, k, n, count if n else None)
    return count[:n].astype(np.int64)


@dataclasses.dataclass
class Hubness:
    """How unevenly a ranking spreads its recommendations: `counts` int64 [n] (k_occurrence: in how many lists every song is),
    `skewness` (the population skewness m3 / m2^1.5 of the counts in float64, 0 when all are equal: about 0 for a fair ranking,
    2 - 3 for raw distances in 20 dimensions), and `k`, the length of the lists."""

    counts: np.ndarray
    skewness: float
    k: int

    @classmethod
    def from_counts(cls, counts, k) -> "Hubness":
        c = np.asarray(counts, dtype=np.int64).reshape(-1)
        x = c.astype(np.float64)
        skew = 0.0
        if x.size:
            dev = x - x.mean()
            m2, m3 = (dev ** 2).mean(), (dev ** 3).mean()
            skew = 0.0 if m2 == 0 else float(m3 / m2 ** 1.5)
        return cls(c, skew, int(k))

    def hubs(self, t) -> np.ndarray:
        """the t most-listed songs, int64, most-listed first, ties to the lower song"""
        order = np.lexsort((np.arange(self.counts.size), -self.counts))
        return order[:max(int(t), 0)].astype(np.int64)

    def orphans(self) -> np.ndarray:
        """the songs no list contains, ascending"""
        return np.flatnonzero(self.counts == 0).astype(np.int64)


def hubness(idx, n) -> Hubness:
    """The hubness of the lists idx [q, k] over n songs: the counts from the device (k_occurrence), their skewness on the host."""
    L = _lists(idx)
    return Hubness.from_counts(k_occurrence(L, n), L.shape[1])


def neighbour_agreement(idx, labels) -> float:
    """The second yardstick of a ranking (Schnitzer et al. 2012): per song, the share of its listed neighbours that carry its
    label; row i of idx [n, k] is song i's list.  Unlabelled songs (-1) and padding entries are left out on both sides.  -> the
    float64 mean over the songs with at least one counted neighbour (nan when there is none).  Pure numpy."""
    L = _lists(idx)
    lab = np.asarray(labels, dtype=np.int64).reshape(-1)
    if lab.shape[0] != L.shape[0]:
        raise ValueError("labels needs one entry per row of idx")
    if (L >= lab.shape[0]).any():
        raise ValueError("idx entries must be rows of labels")
    nb = np.where(L >= 0, lab[np.maximum(L, 0)], -1)  # the neighbours' labels, -1 where nothing counts
    counted = (nb >= 0) & (lab[:, None] >= 0)
    same = counted & (nb == lab[:, None])
    tot = counted.sum(axis=1)
    rows = tot > 0
    if not rows.any():
        return float("nan")
    return float((same.sum(axis=1)[rows].astype(np.float64) / tot[rows]).mean())


# ---- a 2-D map of a library: exact t-SNE stepped on the device (blissgpu_map_step / blissgpu_map_layout) ----
MAP_BISECTIONS = 64  # steps of every row's perplexity search: always all of them


def map_affinities(idx, dist, perplexity):
    """The symmetric affinities P of a map from every song's nearest-neighbour list: idx int [n, k] and dist float [n, k] as
    nearest_order(X, X, k, skip=arange(n)) returns them (-1 / inf padding is left out).  Per row, p_j = exp(-beta (d_j^2 - min
    d^2)) normalised to sum 1, with beta found by exactly MAP_BISECTIONS bisection steps on the row's entropy against
    log(perplexity) -- beta starts at 1 and doubles while no upper bound is known; no tolerance ends the search early --, all
    rows at once in float64.  Then P = (p + p^T) / 2n.  -> (row_offsets uint64[n + 1], cols uint32[nnz], vals float64[nnz]) in
    the CSR form blissgpu_map_step reads: columns ascending within a row, no diagonal, symmetric in value, summing to 1.  The
    device takes vals rounded to float32 (map_step and map_layout round them).  Pure numpy."""
    idx = np.asarray(idx, dtype=np.int64)
    d = np.asarray(dist, dtype=np.float64)
    if idx.ndim != 2 or d.shape != idx.shape:
        raise ValueError("idx and dist must both be [n, k]")
    perplexity = float(perplexity)
    if not (perplexity > 0.0 and np.isfinite(perplexity)):
        raise ValueError("perplexity must be positive and finite")
    n, k = idx.shape
    rows = np.arange(n, dtype=np.int64)[:, None]
    valid = (idx >= 0) & np.isfinite(d) & (idx != rows)
    if (idx[valid] >= n).any():
        raise ValueError("idx entries must be rows of the library")
    if n == 0 or k == 0 or not valid.any():
        return np.zeros(n + 1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float64)
    d2 = np.where(valid, d * d, np.inf)
    d2 = np.where(valid, d2 - d2.min(axis=1, keepdims=True), np.inf)  # rows without a neighbour stay all-inf: p = 0
    target = np.log(perplexity)
    beta, lo, hi = np.ones(n), np.zeros(n), np.full(n, np.inf)

    def weights(b):
        with np.errstate(invalid="ignore", over="ignore"):
            return np.where(valid, np.exp(-b[:, None] * np.where(valid, d2, 0.0)), 0.0)

    for _ in range(MAP_BISECTIONS):
        p = weights(beta)
        s = np.maximum(p.sum(axis=1), np.finfo(np.float64).tiny)
        h = np.log(s) + beta * (np.where(valid, d2, 0.0) * p).sum(axis=1) / s
        more = h > target  # too flat: a larger beta
        lo = np.where(more, beta, lo)
        hi = np.where(more, hi, beta)
        beta = np.where(np.isinf(hi), beta * 2.0, (lo + hi) / 2.0)
    p = weights(beta)
    p = p / np.maximum(p.sum(axis=1, keepdims=True), np.finfo(np.float64).tiny)
    # (p + p^T) / 2n: both directions as (row n + column) keys, equal keys added (at most two, so the order cannot matter)
    r = np.broadcast_to(rows, idx.shape)[valid]
    c = idx[valid]
    v = p[valid]
    keys = np.concatenate([r * n + c, c * n + r])
    order = np.argsort(keys, kind="stable")
    keys, v2 = keys[order], np.concatenate([v, v])[order]
    first = np.concatenate([[True], keys[1:] != keys[:-1]])
    starts = np.flatnonzero(first)
    vals = np.add.reduceat(v2, starts) / (2.0 * n)
    keys = keys[starts]
    counts = np.bincount(keys // n, minlength=n)
    row_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return row_offsets, (keys % n).astype(np.uint32), vals


def map_init(X, mom: "Moments" = None) -> np.ndarray:
    """The starting positions of a map, float32 [n, 2]: the rows of X (an array, or songs) projected onto the two leading
    eigenvectors of their scatter matrix -- moments(X), from the device; `mom` passes a Moments that is already there -- and
    scaled so that the first coordinate has standard deviation 1e-4.  Each eigenvector's sign is fixed so that its entry of
    the largest magnitude is positive (the first such entry), so two runs start alike.  With one feature the second coordinate
    is 0; rows that do not vary start at 0."""
    X = _rows_of_input(X)
    n, d = X.shape
    if n == 0:
        return np.zeros((0, 2), np.float32)
    if mom is None:
        mom = moments(X)
    S = np.asarray(mom.scatter, dtype=np.float64)
    _, vec = np.linalg.eigh((S + S.T) / 2.0)  # ascending eigenvalues
    V = np.zeros((d, 2), np.float64)
    for c in range(min(2, d)):
        v = vec[:, d - 1 - c]
        V[:, c] = v if v[int(np.argmax(np.abs(v)))] > 0 else -v
    Y = (X.astype(np.float64) - np.asarray(mom.mean, np.float64).reshape(1, d)) @ V
    sd = float(Y[:, 0].std())
    if not (sd > 0.0 and np.isfinite(sd)):
        return np.zeros((n, 2), np.float32)
    return np.ascontiguousarray(Y * (1e-4 / sd), dtype=np.float32)


def _map_csr(n, row_offsets, cols, vals):
    """the CSR arrays of a map call, checked (ValueError) and in the dtypes the library reads"""
    ro = np.ascontiguousarray(np.asarray(row_offsets).reshape(-1))
    if ro.dtype.kind not in "iu":
        raise ValueError("row_offsets must be integers")
    if ro.shape[0] != n + 1:
        raise ValueError("row_offsets needs n + 1 entries")
    if (ro.astype(np.int64) < 0).any():
        raise ValueError("row_offsets must not be negative")
    ro = ro.astype(np.uint64)
    if ro[0] != 0 or (ro[1:] < ro[:-1]).any():
        raise ValueError("row_offsets must start at 0 and must not decrease")
    nnz = int(ro[-1])
    co = np.asarray(cols).reshape(-1)
    va = np.ascontiguousarray(np.asarray(vals).reshape(-1), dtype=np.float32)
    if co.shape[0] != nnz or va.shape[0] != nnz:
        raise ValueError("cols and vals need row_offsets[n] entries")
    if nnz >= 2 ** 32:
        raise ValueError("nnz must be below 2^32")
    if nnz:
        if co.dtype.kind not in "iu" or co.min() < 0 or co.max() >= n:
            raise ValueError("cols must be row indices below n")
        co64 = co.astype(np.int64)
        row = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro.astype(np.int64)))
        if (co64 == row).any():
            raise ValueError("a row holds itself")
        inside = row[1:] == row[:-1]
        if (inside & (co64[1:] <= co64[:-1])).any():
            raise ValueError("a row's columns must be strictly ascending")
        if not np.isfinite(va).all() or (va < 0).any():
            raise ValueError("vals must be finite and >= 0")
    return ro, np.ascontiguousarray(co, dtype=np.uint32), va


def _map_points(Y):
    Y = np.ascontiguousarray(Y, dtype=np.float32)
    if Y.ndim != 2 or Y.shape[1] != 2:
        raise ValueError("the points must be [n, 2]")
    if Y.shape[0] >= 2 ** 24:
        raise ValueError("a map holds fewer than 2^24 points")
    return Y


def _map_col_groups(col_groups):
    col_groups = int(col_groups)
    if not 0 <= col_groups <= 64:
        raise ValueError("col_groups must be 0 .. 64")
    return col_groups


def map_plan(n, n_cus=0) -> int:
    """The column groups col_groups = 0 stands for on a device of n_cus compute units (blissgpu_map_plan; device-free)."""
    out = C.c_uint32(0)
    _ffi.call("blissgpu_map_plan", int(n), int(n_cus), C.byref(out))
    return int(out.value)


def map_step(Y, row_offsets, cols, vals, exaggeration=1.0, col_groups=0):
    """One gradient of the map's cost at the points Y float32 [n, 2] under the affinities (row_offsets, cols, vals) -- the CSR
    form map_affinities returns; vals are rounded to float32 -- on the device (blissgpu_map_step; include/blissgpu.h states
    every operation and its order).  -> (grad float64 [n, 2], z_rows float64 [n], Z float).  Bad CSR input raises ValueError."""
    Y = _map_points(Y)
    n = Y.shape[0]
    ro, co, va = _map_csr(n, row_offsets, cols, vals)
    exaggeration = float(exaggeration)
    if not np.isfinite(exaggeration):
        raise ValueError("exaggeration must be finite")
    grad, z_rows, Z = np.zeros((n, 2), np.float64), np.zeros(n, np.float64), C.c_double(0.0)
    _ffi.call("blissgpu_map_step", Y, n, ro, co, va, exaggeration, _map_col_groups(col_groups), grad, z_rows, C.byref(Z))
    return grad, z_rows, float(Z.value)


def map_layout(Y0, row_offsets, cols, vals, n_iter=750, exag_iters=250, exaggeration=12.0, learning_rate=200.0, momentum0=0.5,
               momentum1=0.8, min_gain=0.01, col_groups=0):
    """n_iter iterations of gradient, gain and momentum from the points Y0 in one device call (blissgpu_map_layout): the first
    exag_iters of them with (exaggeration, momentum0), the rest with (1, momentum1); nothing crosses to the host between two
    iterations.  -> (Y float32 [n, 2], z_trace float64 [n_iter], every iteration's normaliser).  Bad CSR input or a parameter
    that is not finite raises ValueError; a normaliser that is not finite and positive (a NaN in Y0) BlissGpuError(ERR_NAN)."""
    Y0 = _map_points(Y0)
    n = Y0.shape[0]
    ro, co, va = _map_csr(n, row_offsets, cols, vals)
    n_iter, exag_iters = int(n_iter), int(exag_iters)
    if n_iter < 0 or exag_iters < 0 or max(n_iter, exag_iters) >= 2 ** 32:
        raise ValueError("n_iter and exag_iters must be counts")
    params = [float(exaggeration), float(learning_rate), float(momentum0), float(momentum1), float(min_gain)]
    if not np.isfinite(params).all():
        raise ValueError("exaggeration, learning_rate, the momenta and min_gain must be finite")
    Y, trace = np.zeros((n, 2), np.float32), np.zeros(n_iter, np.float64)
    _ffi.call("blissgpu_map_layout", Y0, n, ro, co, va, n_iter, exag_iters, *params, _map_col_groups(col_groups), Y, trace)
    return Y, trace


@dataclasses.dataclass
class SongMap:
    """The result of song_map: xy float32 [n, 2] (a point per song), z_trace float64 [n_iter] (every iteration's normaliser Z:
    it falls as the map spreads out) and kl, the Kullback-Leibler divergence of the map's similarities from the affinities P
    at xy -- the cost the iterations lower; two maps of the same library are compared by it."""
    xy: np.ndarray
    z_trace: np.ndarray
    kl: float


def map_kl(xy, row_offsets, cols, vals, Z) -> float:
    """sum over the stored entries of P log(P / Q) with Q = q / Z, q = 1 / (1 + |y_i - y_j|^2): float64 on the host, O(nnz)"""
    xy = np.asarray(xy, dtype=np.float64)
    ro = np.asarray(row_offsets, dtype=np.int64)
    row = np.repeat(np.arange(xy.shape[0], dtype=np.int64), np.diff(ro))
    co = np.asarray(cols, dtype=np.int64)
    p = np.asarray(vals, dtype=np.float64)
    keep = p > 0
    if not keep.any():
        return 0.0
    diff = xy[row[keep]] - xy[co[keep]]
    q = 1.0 / (1.0 + (diff * diff).sum(axis=1))
    return float((p[keep] * (np.log(p[keep]) - np.log(q) + np.log(Z))).sum())


def song_map(songs_or_X, perplexity=30.0, n_iter=750, metric_builder=euclidean_distance, init="pca", exag_iters=250,
             exaggeration=12.0, learning_rate=None, momentum0=0.5, momentum1=0.8, min_gain=0.01, col_groups=0) -> SongMap:
    """A picture of a library: a point per song (or row of an array) on a plane where sonic neighbours are neighbours -- exact
    t-SNE (van der Maaten and Hinton 2008), every pair in every iteration, on the device.  Three device stages: every song's
    k = min(n - 1, 3 perplexity) nearest other songs under metric_builder (nearest_order: euclidean, cosine or a
    MahalanobisBuilder, a learned M included; ForestOptions and VarianceWeights are refused), the starting positions
    (init="pca": map_init; or an [n, 2] array), and the n_iter iterations in one call (map_layout).  The affinities between
    them are numpy (map_affinities).  learning_rate None = max(n / 12 / 4, 50).  -> SongMap."""
    metric, m = _scaled_metric(metric_builder, "song_map")
    X = _rows_of_input(songs_or_X)
    n = X.shape[0]
    if isinstance(init, str):
        if init != "pca":
            raise ValueError('init must be "pca" or an [n, 2] array')
    else:
        init = _map_points(init)
        if init.shape[0] != n:
            raise ValueError("init needs a point per song")
    n_iter = int(n_iter)
    if n < 2:
        return SongMap(np.zeros((n, 2), np.float32), np.zeros(max(n_iter, 0), np.float64), 0.0)
    k = min(n - 1, max(1, int(3.0 * float(perplexity))))
    idx, dist = nearest_order(X, X, k, metric, m, skip=np.arange(n))
    ro, co, va = map_affinities(idx, dist, perplexity)
    va = va.astype(np.float32)
    Y0 = map_init(X) if isinstance(init, str) else init
    lr = max(n / 12.0 / 4.0, 50.0) if learning_rate is None else float(learning_rate)
    xy, trace = map_layout(Y0, ro, co, va, n_iter, exag_iters, exaggeration, lr, momentum0, momentum1, min_gain, col_groups)
    _, _, Z = map_step(xy, ro, co, va, 1.0, col_groups)  # the normaliser AT xy (the trace ends one update before it)
    return SongMap(xy, trace, map_kl(xy, ro, co, va, Z))


class KSelection:
    """The result of choose_k: ks (as given), scores (the silhouette score of each k's clustering), best_k (the k with the
    highest score; equal scores go to the lower k) and clustering (that k's Clustering)."""

    def __init__(self, ks, scores, best_k, clustering):
        self.ks = [int(k) for k in ks]
        self.scores = [float(v) for v in scores]
        self.best_k = int(best_k)
        self.clustering = clustering

    def __repr__(self):
        return f"KSelection(best_k={self.best_k}, scores={dict(zip(self.ks, self.scores))})"


def _best_k(ks, scores) -> int:
    """the k with the highest score; equal scores go to the lower k"""
    best = None
    for k, v in zip(ks, scores):
        if best is None or v > best[1] or (v == best[1] and k < best[0]):
            best = (int(k), float(v))
    return best[0]


def _sample_rows(n, sample, seed):
    """the rows choose_k scores: None = all, else `sample` of them drawn without replacement with the seed, sorted"""
    if sample is None or int(sample) >= n:
        return None
    if int(sample) < 1:
        raise ValueError("sample must be at least 1")
    return np.sort(np.random.Generator(np.random.PCG64(int(seed))).choice(n, int(sample), replace=False))


def choose_k(songs_or_X, ks, seed=0, metric_builder=euclidean_distance, max_iter=100, init="k-means++", sample=None) -> KSelection:
    """Which k suits the songs: for every k of `ks`, k-means from kmeans_init(rows, k, seed, init) (Context.kmeans) and the
    silhouette of its labels (Context.silhouette), on rows uploaded once.  -> KSelection: the highest silhouette score wins,
    equal scores go to the lower k.  sample = m scores m rows only -- numpy.random.Generator(PCG64(seed)).choice(n, m,
    replace=False), sorted -- which makes a k cost n m distances, not n n.  A k whose clustering leaves fewer than two
    non-empty clusters raises BlissGpuError(ERR_INVALID).  metric_builder: as cluster_songs."""
    metric, m = _kmeans_metric(metric_builder)
    ks = [int(k) for k in ks]
    if not ks:
        raise ValueError("choose_k needs at least one k")
    X = _rows_of_input(songs_or_X)
    n = X.shape[0]
    if n == 0:
        raise ValueError("choose_k needs at least one song")
    rows = _sample_rows(n, sample, seed)
    import math

    import torch

    from .device import Context

    ctx = Context.default()
    dev = torch.device("cuda", ctx.device)
    Xd = torch.from_numpy(X).to(dev)
    Md = None if m is None else torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).to(dev)
    rows_d = None if rows is None else torch.from_numpy(rows.astype(np.int32)).to(dev)
    scores, best = [], None
    try:
        for k in ks:
            init_d = torch.from_numpy(kmeans_init(X, k, seed, init, _device=(ctx, Xd))).to(dev)
            labels, dist, cent, sizes, n_iter, conv = ctx.kmeans(Xd, init_d, max_iter, metric, Md)
            s = ctx.silhouette(Xd, labels, metric, Md, rows_d, 0, k)[0]
            score = math.fsum(float(v) for v in s.cpu().numpy()) / s.shape[0]
            scores.append(score)
            if best is None or _best_k(ks, scores) != best[0]:  # (only the winner's clustering is brought to the host)
                best = (k, Clustering(labels.cpu().numpy(), dist.cpu().numpy(), cent.cpu().numpy(), sizes.cpu().numpy(), n_iter, conv))
    except _ffi.BlissGpuError as e:
        _nan_to_panic(e)
    return KSelection(ks, scores, best[0], best[1])


def choose_k_tree(songs_or_X, tree: "WardTree", ks, metric_builder=euclidean_distance) -> KSelection:
    """Which k suits the songs, from ONE Ward tree: for every k of `ks` the silhouette (Context.silhouette, on rows uploaded once)
    of tree.cut(k) -- a cut per k where choose_k runs a whole k-means per k, and the clusterings are nested.  -> KSelection:
    the highest silhouette score wins, equal scores go to the lower k; `clustering` is the winner's labels (int64 [n], as
    tree.cut(best_k) gives them).  Every k must be 2 .. n.  metric_builder: as ward_tree."""
    metric, m = _ward_metric(metric_builder)
    ks = [int(k) for k in ks]
    if not ks:
        raise ValueError("choose_k_tree needs at least one k")
    X = _rows_of_input(songs_or_X)
    n = X.shape[0]
    if n != tree.n:
        raise ValueError("the tree was made from another number of songs")
    if min(ks) < 2 or max(ks) > n:
        raise ValueError("every k must be 2 .. n")
    import math

    import torch

    from .device import Context

    ctx = Context.default()
    dev = torch.device("cuda", ctx.device)
    Xd = torch.from_numpy(X).to(dev)
    Md = None if m is None else torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).to(dev)
    scores, best = [], None
    try:
        for k in ks:
            labels = tree.cut(k)
            s = ctx.silhouette(Xd, torch.from_numpy(labels).to(dev), metric, Md, None, 0, k)[0]
            scores.append(math.fsum(float(v) for v in s.cpu().numpy()) / s.shape[0])
            if best is None or _best_k(ks, scores) != best[0]:
                best = (k, labels)
    except _ffi.BlissGpuError as e:
        _nan_to_panic(e)
    return KSelection(ks, scores, best[0], best[1])


def _triplet_args(X, triplets, m):
    X = rows_f32(X)
    tr = np.asarray(triplets)
    if tr.size and (tr.min() < 0 or tr.max() > 0xFFFFFFFF):
        raise ValueError("triplets must be row indices")
    tr = np.ascontiguousarray(tr, dtype=np.uint32).reshape(-1, 3)
    m = metric_matrix(None, m)  # (None: the identity)
    if m is not None and m.shape != (X.shape[1], X.shape[1]):
        raise ValueError("m must be [d, d]")
    return X, tr, m


def triplet_step(X, triplets, m=None, margin=0.0, return_flags=False):
    """One gradient evaluation of triplet metric learning on the device (blissgpu_triplet_step).  A triplet
    (a, b, o) of rows of X says "a and b are closer together than either is to o"; with u = x_a - x_b, v = x_a - x_o,
    w = x_b - x_o and q(t) = t' m t (m None: the identity) its hinges are h1 = margin + q(u) - q(v), h2 = margin + q(u) - q(w).
    -> (n_active, loss, G float64[d, d]) or, return_flags, (n_active, loss, G, flags uint8[T]) with flags = (h1 > 0) |
    (h2 > 0) << 1: the number of hinges above 0, their sum, and the sum over the active hinges of u u' - v v' (u u' - w w'),
    the gradient of the loss in m.  All f64.  An index past the rows or a negative margin raises BlissGpuError(ERR_INVALID), a
    NaN hinge ValueError."""
    X, tr, m = _triplet_args(X, triplets, m)
    (n, d), T = X.shape, tr.shape[0]
    G, flags = np.zeros((d, d), np.float64), np.zeros(T, np.uint8)
    n_active, loss = C.c_uint64(0), C.c_double(0.0)
    _call("blissgpu_triplet_step", X, n, d, tr if T else None, T, m, float(margin), flags if return_flags and T else None,
          C.byref(n_active), C.byref(loss), G)
    out = (int(n_active.value), float(loss.value), G)
    return out + (flags,) if return_flags else out


_LEARN_STATUS = {_ffi.LEARN_CONVERGED: "converged", _ffi.LEARN_MAX_ITER: "max_iter", _ffi.LEARN_DIVERGED: "diverged"}
# DESIGN.md 3.22 has the table behind these (planted metrics, numpy on a CPU); nobody has measured them on a real library
LEARN_MARGIN, LEARN_LR, LEARN_MAX_ITER = 0.1, 1.0, 100


class LearnedMetric:
    """The result of learn_metric: m float32[d, d] (the iterate with the lowest objective, positive semi-definite by
    construction), objective float64[n_iter + 1], active int64[n_iter + 1] (hinges above 0 per iteration), n_iter (updates
    made), best_iter, status ("converged": no active hinge; "max_iter"; "diverged": the objective or m left the finite numbers)."""

    def __init__(self, m, objective, active, n_iter, best_iter, status):
        self.m = np.asarray(m, dtype=np.float32)
        self.objective = np.asarray(objective, dtype=np.float64)
        self.active = np.asarray(active, dtype=np.int64)
        self.n_iter, self.best_iter, self.status = int(n_iter), int(best_iter), str(status)

    def builder(self) -> "MahalanobisBuilder":
        return MahalanobisBuilder(self.m)

    def __repr__(self):
        return (f"LearnedMetric(d={self.m.shape[0]}, n_iter={self.n_iter}, best_iter={self.best_iter}, status={self.status!r}, "
                f"objective={self.objective[self.best_iter] if self.objective.size else float('nan'):.6g})")


def _learn_args(form, init, d, max_iter):
    if form not in _FORMS:
        raise ValueError(f"form must be one of {tuple(_FORMS)}")
    max_iter = int(max_iter)
    if max_iter < 0:
        raise ValueError("max_iter must be at least 0")
    if init is not None:
        init = np.ascontiguousarray(init, dtype=np.float32).reshape(-1)
        if init.shape[0] != d:
            raise ValueError("init must hold d weights (the diagonal of the starting matrix)")
    return init, max_iter


def _learned(M, obj, act, n_iter, best_iter, status):
    k = int(n_iter.value) + 1
    res = LearnedMetric(M, obj[:k].copy(), act[:k].astype(np.int64), n_iter.value, best_iter.value, _LEARN_STATUS[status.value])
    if res.status == "diverged":
        import warnings

        warnings.warn(f"learn_metric diverged at iteration {res.n_iter}; m is iteration {res.best_iter}'s: lower lr", RuntimeWarning,
                      stacklevel=3)
    return res


def learn_metric(X, triplets, form="full", init=None, margin=LEARN_MARGIN, lr=LEARN_LR, reg=0.0, max_iter=LEARN_MAX_ITER) -> LearnedMetric:
    """Learn a Mahalanobis matrix from training triplets (blissgpu_learn_metric): projected gradient descent
    on  sum of the hinges / (2 T) + reg * |m - m_0|^2  over m = diag(w), w >= 0 (form "diagonal") or m = L'L (form "full"),
    starting from m_0 = diag(init) (None: the identity; FeaturesVersion.feature_weights' diagonal is the obvious other start).
    X and the triplets stay on the device; an iteration uploads m and downloads the gradient.  -> LearnedMetric; `.m` goes into
    MahalanobisBuilder.  A RuntimeWarning says when the run diverged (m is then the best iterate before that)."""
    X, tr, _ = _triplet_args(X, triplets, None)
    (n, d), T = X.shape, tr.shape[0]
    init, max_iter = _learn_args(form, init, d, max_iter)
    M, obj, act = np.zeros((d, d), np.float32), np.zeros(max_iter + 1, np.float64), np.zeros(max_iter + 1, np.uint64)
    n_iter, best_iter, status = C.c_uint32(0), C.c_uint32(0), C.c_int32(0)
    _call("blissgpu_learn_metric", X, n, d, tr if T else None, T, _FORMS[form], init, float(margin), float(lr), float(reg), max_iter, M,
          obj, act, C.byref(n_iter), C.byref(best_iter), C.byref(status))
    return _learned(M, obj, act, n_iter, best_iter, status)


# ---- library statistics and covariance-based metrics (blissgpu_moments, blissgpu_covariance_metric) ----
# the share of the mean variance mixed into the covariance before it is inverted, so that a constant feature does not make it
# singular.  Nobody has measured this default on a real library
COV_SHRINK = 0.01


class Moments:
    """The result of moments: counts int64[k], mean / var / std float64[k, d] (var = m2 / count, the population variance; an
    empty group has 0), m2 float64[k, d] (the sums of squared deviations), min / max float32[k, d] (+inf / -inf for an empty
    group), scatter float64[d, d] (the pooled within-group scatter; without labels the total scatter; None when not asked for)
    and dof = n - the number of non-empty groups, what the scatter is divided by to estimate a covariance."""

    def __init__(self, counts, mean, m2, mn, mx, scatter):
        self.counts = np.asarray(counts, dtype=np.int64)
        self.mean, self.m2 = np.asarray(mean, dtype=np.float64), np.asarray(m2, dtype=np.float64)
        self.min, self.max = np.asarray(mn, dtype=np.float32), np.asarray(mx, dtype=np.float32)
        self.scatter = None if scatter is None else np.asarray(scatter, dtype=np.float64)
        self.var = self.m2 / np.maximum(self.counts, 1)[:, None].astype(np.float64)
        self.std = np.sqrt(self.var)
        self.dof = int(self.counts.sum()) - int(np.count_nonzero(self.counts))

    def __repr__(self):
        return f"Moments(n={int(self.counts.sum())}, k={len(self.counts)}, d={self.mean.shape[1]}, dof={self.dof})"


def moments(X, labels=None, k=None, scatter=True) -> Moments:
    """The first and second moments of the rows of X (an array, or songs) in one device call (blissgpu_moments):
    per group of the labelling `labels` (None: one group) the count, mean, variance, minimum and maximum of every feature, and
    the d x d scatter matrix of the rows about their group's mean.  Every sum is f64 in the fixed blocked order of
    include/blissgpu.h: two calls return the same bits.  k: the number of groups, None = labels.max() + 1.  A label >= k raises
    BlissGpuError(ERR_INVALID), a NaN or an infinity in X ValueError."""
    X = _rows_of_input(X)
    n, d = X.shape
    lab = None
    if labels is None:
        k = 1 if k is None else int(k)
    else:
        lab = _index_array(labels, "labels")
        if lab.shape[0] != n:
            raise ValueError("a label per row of X is needed")
        k = (int(lab.max()) + 1 if n else 1) if k is None else int(k)
    kk = max(k, 0)
    counts, mean, m2 = np.zeros(kk, np.uint32), np.zeros((kk, d), np.float64), np.zeros((kk, d), np.float64)
    mn, mx = np.zeros((kk, d), np.float32), np.zeros((kk, d), np.float32)
    S = np.zeros((d, d), np.float64) if scatter else None
    _call("blissgpu_moments", X, n, d, lab, k, counts, mean, m2, mn, mx, S)
    return Moments(counts, mean, m2, mn, mx, S)


class CovarianceMetric:
    """The result of covariance_metric: m float32[d, d] (the inverse of the shrunk covariance scaled to trace d, positive
    definite), scatter float64[d, d] (what it was formed from), dof (what the scatter was divided by), form, shrink."""

    def __init__(self, m, scatter, dof, form, shrink):
        self.m = np.asarray(m, dtype=np.float32)
        self.scatter = np.asarray(scatter, dtype=np.float64)
        self.dof, self.form, self.shrink = int(dof), str(form), float(shrink)

    def builder(self) -> "MahalanobisBuilder":
        return MahalanobisBuilder(self.m)

    def __repr__(self):
        return f"CovarianceMetric(d={self.m.shape[0]}, form={self.form!r}, shrink={self.shrink:g}, dof={self.dof})"


def metric_from_scatter(scatter, dof, form="full", shrink=COV_SHRINK) -> np.ndarray:
    """A scatter matrix turned into a Mahalanobis matrix on the host (blissgpu_covariance_metric; no device is touched):
    C = scatter / dof shrunk towards its mean variance, inverted ("full": by Cholesky; "diagonal": feature by feature) and
    scaled to trace d.  -> m float32[d, d].  ValueError for dof <= 0, and for a covariance that is not positive definite: that
    message names `shrink`, which cures it."""
    if form not in _FORMS:
        raise ValueError(f"form must be one of {tuple(_FORMS)}")
    shrink = float(shrink)
    if not 0.0 <= shrink <= 1.0:
        raise ValueError("shrink must be within 0 .. 1")
    if int(dof) <= 0:
        raise ValueError("covariance_metric needs more rows than non-empty groups (dof = n - groups must be positive)")
    S = np.ascontiguousarray(scatter, dtype=np.float64)
    d = S.shape[0]
    if S.shape != (d, d):
        raise ValueError("scatter must be a square matrix")
    M, status = np.zeros((d, d), np.float32), C.c_int32(0)
    _ffi.call("blissgpu_covariance_metric", S, d, int(dof), _FORMS[form], shrink, M, C.byref(status))
    if status.value != _ffi.COV_OK:
        raise ValueError(f"the covariance is not positive definite at shrink = {shrink:g} (a constant feature, or fewer rows than "
                         "features): raise shrink")
    return M


def covariance_metric(X, labels=None, form="full", shrink=COV_SHRINK, k=None) -> CovarianceMetric:
    """A Mahalanobis matrix in closed form from the second moments of the rows of X (an array, or songs): the inverse of their
    covariance -- "diagonal": per-feature standardisation, "full": whitening.  With `labels` (genre, album, artist, a k-means
    label per row) it is the inverse of the pooled WITHIN-group covariance (relevant component analysis): directions in which
    songs of one group differ count for little, the others for much.  Rows with a label < 0 are left out.  The scatter comes
    from one device call (moments), the solve runs on the host (metric_from_scatter).  It is the baseline learn_metric is to be
    compared with: judge both with triplet_accuracy and silhouette.  -> CovarianceMetric; `.m` goes into MahalanobisBuilder."""
    if form not in _FORMS:
        raise ValueError(f"form must be one of {tuple(_FORMS)}")
    X = _rows_of_input(X)
    if labels is not None:
        labels = np.asarray(labels).reshape(-1).astype(np.int64)
        if labels.shape[0] != X.shape[0]:
            raise ValueError("a label per row of X is needed")
        keep = labels >= 0
        if not keep.all():
            X, labels = np.ascontiguousarray(X[keep]), labels[keep]
    if X.shape[0] == 0:
        raise ValueError("covariance_metric needs more rows than non-empty groups (dof = n - groups must be positive)")
    mo = moments(X, labels, k, True)
    return CovarianceMetric(metric_from_scatter(mo.scatter, mo.dof, form, shrink), mo.scatter, mo.dof, form, shrink)


def triplet_accuracy(X, triplets, m=None) -> float:
    """The share of the 2 T constraints d(a, b) < d(a, o), d(a, b) < d(b, o) that hold under m (None: euclidean): 1 - the
    active hinges of triplet_step at margin 0 over 2 T.  No triplet: 1.0."""
    T = np.asarray(triplets).reshape(-1, 3).shape[0]
    if T == 0:
        return 1.0
    return 1.0 - triplet_step(X, triplets, m, 0.0)[0] / (2.0 * T)


def triplets_from_labels(labels, n_triplets, seed=0) -> np.ndarray:
    """n_triplets training triplets (a, b, o) drawn from class labels (genre, album, artist, a k-means label per song): a and b
    are two DISTINCT rows of one label, o is a row of another label.  int64[n_triplets, 3]; host numpy, a function of its
    arguments only (numpy.random.default_rng(seed)).  Rows with a label < 0 take no part.  The label of (a, b) is drawn in
    proportion to its number of pairs, o uniformly from the rows outside it.  ValueError when fewer than two labels are present
    or no label has two rows."""
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    n_triplets = int(n_triplets)
    if n_triplets < 0:
        raise ValueError("n_triplets must be at least 0")
    rows = np.flatnonzero(labels >= 0)
    order = rows[np.argsort(labels[rows], kind="stable")]  # rows grouped by label, ascending inside a label
    values, start, count = np.unique(labels[order], return_index=True, return_counts=True)
    if values.size < 2:
        raise ValueError("triplets_from_labels needs at least two different labels")
    pairs = count.astype(np.float64) * (count - 1)
    if not (pairs > 0).any():
        raise ValueError("triplets_from_labels needs a label with at least two rows")
    rng = np.random.default_rng(int(seed))
    g = rng.choice(values.size, n_triplets, p=pairs / pairs.sum())
    ia = rng.integers(0, count[g])
    ib = rng.integers(0, count[g] - 1)
    ib = ib + (ib >= ia)  # the other rows of the label, uniformly
    io = rng.integers(0, order.size - count[g])
    io = np.where(io >= start[g], io + count[g], io)  # the rows outside the label's block of `order`
    return np.stack([order[start[g] + ia], order[start[g] + ib], order[io]], axis=1).astype(np.int64).reshape(n_triplets, 3)


def _seed_groups(seed_groups):
    """-> (S f32[total, d] or None when there is no seed at all, offsets u64[G + 1])"""
    if isinstance(seed_groups, tuple) and len(seed_groups) == 2 and not isinstance(seed_groups[0], (list, tuple)) \
            and np.ndim(seed_groups[0]) == 2 and np.ndim(seed_groups[1]) == 1:
        S = np.ascontiguousarray(seed_groups[0], dtype=np.float32)
        off = np.asarray(seed_groups[1], dtype=np.int64).reshape(-1)
        if off.shape[0] < 1 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != S.shape[0]:
            raise ValueError("offsets must start at 0, not decrease and end at the number of seed rows")
        return S, off.astype(np.uint64)
    groups = [np.asarray(g, dtype=np.float32) for g in seed_groups]
    groups = [g.reshape(0, g.shape[-1] if g.ndim == 2 else 0) if g.size == 0 else np.atleast_2d(g) for g in groups]
    off = np.zeros(len(groups) + 1, np.uint64)
    off[1:] = np.cumsum([g.shape[0] for g in groups])
    full = [g for g in groups if g.shape[0]]
    if any(g.ndim != 2 for g in full) or len({g.shape[1] for g in full}) > 1:
        raise ValueError("every seed group must be [s_g, d] with the same d")
    return (np.ascontiguousarray(np.concatenate(full)) if full else None), off


def _group_skip(skip, off, n):
    """The `skip` argument of nearest_to_groups / chain_order -> None or u32[seed rows] (0xFFFFFFFF: none): one array of
    candidate indices per group, or one flat array with an entry per seed row (-1: none)."""
    if skip is None:
        return None
    G, total = off.shape[0] - 1, int(off[-1])
    if isinstance(skip, np.ndarray) and skip.dtype != object and skip.ndim == 1 or \
            (len(skip) != G or total == G) and all(np.ndim(s) == 0 for s in skip):
        flat = np.asarray(skip, dtype=np.int64).reshape(-1)  # one entry per seed row
        if flat.shape[0] != total:
            raise ValueError("a flat skip needs one entry per seed row")
    else:
        if len(skip) != G:
            raise ValueError("skip needs one index array per group")
        flat = np.full(total, -1, np.int64)
        for g, sk in enumerate(skip):
            sk = np.unique(np.asarray(sk, dtype=np.int64).reshape(-1))
            sk = sk[sk != -1]
            a, b = int(off[g]), int(off[g + 1])
            if sk.shape[0] > b - a:
                raise ValueError(f"group {g} skips {sk.shape[0]} candidates but has {b - a} seeds (one skip per seed row)")
            flat[a:a + sk.shape[0]] = sk
    if ((flat < -1) | (flat >= max(n, 0))).any():
        raise ValueError("skip entries must be candidate indices or -1")
    return np.where(flat < 0, 0xFFFFFFFF, flat).astype(np.uint32)


def nearest_to_groups(seed_groups, candidates, k, metric="euclidean", m=None, skip=None):
    """The k nearest candidates of every seed GROUP in one device call, without a groups x candidates matrix: row g of the
    result is closest_to_songs(seed_groups[g], candidates without skip[g], metric) (src/playlist.rs:36-59, 256-270) cut
    after k -- what Library::playlist_from(&[several songs]).take(k) asks per album, artist or saved playlist
    (src/library.rs:762-842).  A candidate's score is the sequential f32 sum of its distances to the group's seeds, in seed
    order (set_distances bit for bit); an empty group scores 0 everywhere.  -> (idx int64[G, k], dist float32[G, k]); equal
    scores come in candidate order; rows with fewer than k eligible candidates end in -1 / inf.
    `seed_groups`: a sequence of [s_g, d] arrays, or (S [total, d], offsets [G + 1]).  `skip`: None, one array of
    candidate indices per group (left out of that group's list), or one flat array with an entry per seed row (-1: none).
    A NaN score raises ValueError (the reference's n32() panic).  A ForestOptions is refused here: a forest is built per seed
    set, which is forest_nearest_to_groups.
    One DIAGONAL Mahalanobis metric per group, still one call (blissgpu_group_knn_weighted): metric="diagonal" with m a [G, d]
    array, row g the diagonal of group g's M; metric="variance" for variance_based_weight_matrix (src/playlist.rs:173-221) of
    each group's own seeds, computed on the device, a group of fewer than two seeds taking the identity (euclidean); or a
    VarianceWeights, which is "variance" under its few_seeds policy (ProviderError for such a group by default, decided from
    the group sizes before the device is touched)."""
    _no_forest(metric, "nearest_to_groups takes the distance metrics; forest_nearest_to_groups builds one forest per seed group")
    S, off = _seed_groups(seed_groups)
    X = rows_f32(candidates)
    if X.ndim != 2 or (S is not None and S.shape[1] != X.shape[1]):
        raise ValueError("seed groups and candidates must be [s_g, d] and [n, d]")
    if isinstance(metric, VarianceWeights):
        metric.check_counts(np.diff(off.astype(np.int64)))
        metric = "variance"
    per_group = isinstance(metric, str) and metric in ("variance", "diagonal")
    if not per_group and metric not in _METRICS:
        raise ValueError(f"unknown metric {metric!r}")
    k = int(k)
    n, d = X.shape
    check_k_d(k, d)
    G = off.shape[0] - 1
    skip = _group_skip(skip, off, n)
    if metric == "diagonal":
        if m is None:
            raise ValueError("diagonal needs m, one row of d weights per group")
        m = metric_matrix(metric, m, d, groups=G)
    else:
        m = metric_matrix(metric, m, d)
    idx, dist = np.empty((G, k), np.uint32), np.empty((G, k), np.float32)
    if per_group:
        _call("blissgpu_group_knn_weighted", S, off, G, X, n, d, m, skip, k, idx, dist, None)
    else:
        _call("blissgpu_group_knn", S, off, G, X, n, d, _METRICS[metric], m, skip, k, idx, dist)
    return signed_idx(idx), dist


def group_variance_weights(seed_groups):
    """variance_based_weight_matrix (src/playlist.rs:173-221) of every seed group in one device call
    (blissgpu_group_weights).  `seed_groups` as for nearest_to_groups.  -> (weights float32[G, d], few_seeds bool[G]): row g is
    the DIAGONAL of the reference's matrix, bit for bit variance_based_weight_matrix(seed_groups[g]); a group of fewer than
    two seeds (where the reference returns its ProviderError) gets ones, the identity, and few_seeds[g] = True."""
    S, off = _seed_groups(seed_groups)
    G = off.shape[0] - 1
    if S is None:  # (a list of groups without a single seed: the width of an empty [0, d] array, if one was given)
        d = max([np.shape(g)[1] for g in seed_groups if np.ndim(g) == 2] + [0])
        if d == 0:
            raise ValueError("the feature count cannot be told from empty seed groups; pass (S [0, d], offsets)")
        S = np.zeros((0, d), np.float32)
    d = S.shape[1]
    if not 1 <= d <= 64:
        raise ValueError("d must be 1 .. 64")
    weights, status = np.empty((G, d), np.float32), np.empty(G, np.int32)
    _ffi.call("blissgpu_group_weights", S if S.shape[0] else None, off, G, d, weights, status)
    return weights, status != 0


def _member_skip(groups, candidate_songs):
    """One entry per member of every group: the first candidate that == it (Song: PartialEq), -1 when there is none."""
    skip = np.full(sum(len(g) for g in groups), -1, np.int64)
    row = 0
    for g in groups:
        for s in g:
            for j, c in enumerate(candidate_songs):
                if _song_of(c) == _song_of(s):
                    skip[row] = j
                    break
            row += 1
    return skip


def group_playlists(groups, candidate_songs, k, metric_builder=euclidean_distance, exclude_members=True):
    """For every group of songs, closest_to_songs(group, candidate_songs without the group's songs, metric_builder)[..k]
    (src/playlist.rs:256-270) -- a playlist "in the vibe of these songs" per album, artist or saved playlist, all of them
    in one device call.  `exclude_members`: the first candidate that == each member (Song: PartialEq, as
    nearest_songs(exclude_self=True)) is left out of that group's list."""
    _no_forest(metric_builder, "group_playlists takes the distance metrics; forest_group_playlists builds one forest per group")
    groups, candidate_songs = [list(g) for g in groups], list(candidate_songs)
    if not groups:
        return []
    if isinstance(metric_builder, VarianceWeights):
        metric_builder.check_counts([len(g) for g in groups])
    if not candidate_songs:
        return [[] for _ in groups]
    metric, m = (metric_builder, None) if isinstance(metric_builder, VarianceWeights) else _metric_of(metric_builder)
    X = _matrix(candidate_songs)
    seeds = [_matrix(g) if g else np.zeros((0, X.shape[1]), np.float32) for g in groups]
    skip = _member_skip(groups, candidate_songs) if exclude_members else None
    idx, _ = nearest_to_groups(seeds, X, k, metric, m, skip)
    return [[candidate_songs[j] for j in row if j >= 0] for row in idx]


_FEW_SEEDS = ("raise", "empty")


def _forest_few_seeds(few_seeds, counts, options, allowed=_FEW_SEEDS):
    """The few_seeds policy of the forest-per-group entry points, decided from the group sizes alone: -> bool[G], True where
    min(sample_size, seeds) < 2"""
    if few_seeds not in allowed:
        raise ValueError("few_seeds must be one of " + ", ".join(repr(a) for a in allowed))
    if not isinstance(options, ForestOptions):
        raise TypeError("options must be a ForestOptions")
    few = np.minimum(np.asarray(counts, np.int64), options.sample_size) < 2
    if few_seeds == "raise" and few.any():
        g = int(np.nonzero(few)[0][0])
        raise ValueError(_FOREST_SINGLE.format(what=f"group {g} has {int(np.asarray(counts)[g])} seed(s), sample_size "
                                                    f"{options.sample_size}; few_seeds chooses what such a group gets"))
    return few


def forest_nearest_to_groups(seed_groups, candidates, k, options, skip=None, few_seeds="raise"):
    """nearest_to_groups with the extended isolation forest as the metric (ForestOptions, src/playlist.rs:230-251), for every
    seed group in ONE call (blissgpu_group_forest_knn): group g's forest is Forest(seed_groups[g], options) -- every group
    with the same options and the same options.seed -- and row g holds the first k of the stable ascending order of its
    scores over the candidates without skip[g], bit for bit Forest(...).scores().  No groups x candidates array is stored;
    the forests are built on the host, batch by batch, while the device scores the previous batch.
    -> (idx int64[G, k], score float32[G, k]); rows with fewer than k eligible candidates end in -1 / inf.  `seed_groups` and
    `skip` as for nearest_to_groups.  `few_seeds`: a group with min(sample_size, seeds) < 2 has no forest ("does not work for
    a single song") -- "raise" (the default) is a ValueError, decided from the group sizes before the device is touched;
    "empty" gives such a group a row of -1 / inf."""
    S, off = _seed_groups(seed_groups)
    _forest_few_seeds(few_seeds, np.diff(off.astype(np.int64)), options)
    X = rows_f32(candidates)
    if X.ndim != 2 or (S is not None and S.shape[1] != X.shape[1]):
        raise ValueError("seed groups and candidates must be [s_g, d] and [n, d]")
    k = int(k)
    n, d = X.shape
    check_k_d(k, d, 32)
    depth = options.max_tree_depth
    if depth is not None and not 1 <= depth <= 128:
        raise ValueError("max_tree_depth must be None or 1 .. 128")
    for name in ("n_trees", "sample_size", "extension_level"):
        if not 0 <= getattr(options, name) <= 0xFFFFFFFF:
            raise ValueError(f"{name} out of range")
    G = off.shape[0] - 1
    skip = _group_skip(skip, off, n)
    idx, score, status = np.empty((G, k), np.uint32), np.empty((G, k), np.float32), np.zeros(G, np.int32)
    try:
        _ffi.call("blissgpu_group_forest_knn", S, off, G, X, n, d, options.n_trees, options.sample_size, depth or 0,
                  options.extension_level, options.seed, skip, k, idx, score, status)
    except _ffi.BlissGpuError as e:
        if e.code == _ffi.ERR_INVALID:
            raise ValueError(str(e)) from e
        raise
    return signed_idx(idx), score


def forest_group_playlists(groups, candidate_songs, k, options, exclude_members=True, few_seeds="raise"):
    """group_playlists with a ForestOptions: for every group of songs, closest_to_songs(group, candidate_songs without the
    group's songs, options)[..k] (src/playlist.rs:230-251, 256-270), every group in one device call
    (forest_nearest_to_groups).  `few_seeds` as there, and additionally "euclidean": the groups without a forest are answered
    by ONE nearest_to_groups call under euclidean_distance (their lists are ordered by euclidean sums, not forest scores)."""
    groups, candidate_songs = [list(g) for g in groups], list(candidate_songs)
    few = _forest_few_seeds(few_seeds, [len(g) for g in groups], options, _FEW_SEEDS + ("euclidean",))
    if not groups:
        return []
    if not candidate_songs:
        return [[] for _ in groups]
    X = _matrix(candidate_songs)
    seeds = [_matrix(g) if g else np.zeros((0, X.shape[1]), np.float32) for g in groups]
    skip = _member_skip(groups, candidate_songs) if exclude_members else None
    idx, _ = forest_nearest_to_groups(seeds, X, k, options, skip, "empty")
    if few_seeds == "euclidean" and few.any():
        off = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
        rows = np.nonzero(few)[0]
        sub_skip = None if skip is None else np.concatenate([skip[off[g]:off[g + 1]] for g in rows] + [np.zeros(0, np.int64)])
        sub, _ = nearest_to_groups([seeds[g] for g in rows], X, k, "euclidean", None, sub_skip)
        idx[rows] = sub
    return [[candidate_songs[j] for j in row if j >= 0] for row in idx]


def chain_order(seed_groups, candidates, k, metric="euclidean", m=None, skip=None, route="auto"):
    """The first k songs of song_to_song(seed_groups[g], candidates without skip[g], metric) (src/playlist.rs:272-326) for
    every seed GROUP in one device call (blissgpu_chains): song 0 is the candidate closest to the group's seed set (the score
    of nearest_to_groups), song t the candidate not yet in the chain that is closest to song t - 1; equal distances go to the
    lower index.  -> (idx int64[G, k], dist float32[G, k]): dist[g][t] is the distance that chose idx[g][t]; rows with fewer
    than k eligible candidates end in -1 / inf.  `seed_groups` and `skip` as for nearest_to_groups.  `route`: "auto", "steps"
    (one launch per step over every chain) or "lists" (the candidates' own k-nearest lists, then one walk; needs
    k + largest group - 1 <= 1024); the result does not depend on it.  A NaN distance on a chain raises ValueError (the
    reference's argmin().unwrap() panic).  VarianceWeights and ForestOptions are refused: song_to_song rebuilds a one-song
    metric after the first step."""
    _no_forest(metric, "song_to_song rebuilds its metric from one song after the first step (:285-295)")
    _no_variance(metric, "song_to_song rebuilds its metric from one song after the first step (:285-295)")
    S, off = _seed_groups(seed_groups)
    X = rows_f32(candidates)
    if X.ndim != 2 or (S is not None and S.shape[1] != X.shape[1]):
        raise ValueError("seed groups and candidates must be [s_g, d] and [n, d]")
    if metric not in _METRICS:
        raise ValueError(f"unknown metric {metric!r}")
    if route not in _ROUTES:
        raise ValueError(f"route must be one of {tuple(_ROUTES)}")
    k = int(k)
    n, d = X.shape
    check_k_d(k, d)
    G = off.shape[0] - 1
    if route == "lists" and k >= 2 and G and k + int(np.diff(off.astype(np.int64)).max()) - 1 > 1024:
        raise ValueError("the lists route needs k + largest group - 1 <= 1024")
    skip = _group_skip(skip, off, n)
    m = metric_matrix(metric, m, d)
    idx, dist = np.empty((G, k), np.uint32), np.empty((G, k), np.float32)
    _call("blissgpu_chains", S, off, G, X, n, d, _METRICS[metric], m, skip, k, _ROUTES[route], idx, dist)
    return signed_idx(idx), dist


def song_chains(groups, candidate_songs, k, metric_builder=euclidean_distance, exclude_members=True):
    """For every group of songs, the first k songs of song_to_song(group, candidate_songs without the group's songs,
    metric_builder) (src/playlist.rs:272-326) -- a playlist that starts "in the vibe of these songs" and then wanders from
    each song to its nearest remaining neighbour, all groups in one device call.  `exclude_members` as for group_playlists."""
    _no_forest(metric_builder, "song_to_song rebuilds its metric from one song after the first step (:285-295)")
    _no_variance(metric_builder, "song_to_song rebuilds its metric from one song after the first step (:285-295)")
    groups, candidate_songs = [list(g) for g in groups], list(candidate_songs)
    if not groups:
        return []
    if not candidate_songs:
        return [[] for _ in groups]
    metric, m = _metric_of(metric_builder)
    X = _matrix(candidate_songs)
    seeds = [_matrix(g) if g else np.zeros((0, X.shape[1]), np.float32) for g in groups]
    skip = _member_skip(groups, candidate_songs) if exclude_members else None
    idx, _ = chain_order(seeds, X, k, metric, m, skip)
    return [[candidate_songs[j] for j in row if j >= 0] for row in idx]


_JOURNEY_WHY = "a journey's metric compares single songs, step by step"


def journey_order(from_rows, candidates, k, to_rows=None, metric="euclidean", m=None, skip=None, direction=None, feature=None):
    """Waypoint and directed playlists in one device call (blissgpu_journeys; the reference's roadmap names both under "New
    features" in TODO.md and ships neither).  Journey g starts at from_rows[g].
    to_rows given (a WAYPOINT journey): song t is the candidate nearest from + (to - from) * ((t + 1) / (k + 1)), t = 0 .. k - 1
    -- k songs spread along the segment between the two end points, none twice.
    to_rows None (a CHAIN): song 0 is the candidate nearest from_rows[g], song t the candidate nearest song t - 1; with
    `direction` "up" / "down" only the candidates whose column `feature` is >= / <= that of the song before (of from_rows[g]
    for song 0) are eligible -- equality passes, a NaN on either side does not.  A direction cannot be combined with to_rows.
    Equal distances go to the lower index.  `skip`: [G, 2] candidate indices that are never eligible (-1: none), or None.
    -> (idx int64[G, k], dist float32[G, k]); a journey that runs out of eligible candidates ends in -1 / inf.  A NaN distance
    of an eligible candidate raises ValueError.  VarianceWeights and ForestOptions are refused."""
    _no_forest(metric, _JOURNEY_WHY)
    _no_variance(metric, _JOURNEY_WHY)
    A, X = rows_f32(from_rows), rows_f32(candidates)
    if A.ndim != 2 or X.ndim != 2 or A.shape[1] != X.shape[1]:
        raise ValueError("from_rows and candidates must be [G, d] and [n, d]")
    B = None
    if to_rows is not None:
        B = rows_f32(to_rows)
        if B.shape != A.shape:
            raise ValueError("to_rows must have the shape of from_rows")
    if metric not in _METRICS:
        raise ValueError(f"unknown metric {metric!r}")
    if direction not in _GATES:
        raise ValueError('direction must be None, "up" or "down"')
    k = int(k)
    (G, d), n = A.shape, X.shape[0]
    check_k_d(k, d)
    if direction is not None:
        if B is not None:
            raise ValueError("a direction cannot be combined with to_rows")
        if feature is None or not 0 <= int(feature) < d:
            raise ValueError("a direction needs a feature: an AnalysisIndex or a column number below d")
    if skip is not None:
        skip = skip_words(skip, (G, 2), n, "skip must be [G, 2]")
    m = metric_matrix(metric, m, d)
    idx, dist = np.empty((G, k), np.uint32), np.empty((G, k), np.float32)
    _call("blissgpu_journeys", A, B, G, X, n, d, _METRICS[metric], m, skip, k,
          _ffi.JOURNEY_CHAIN if B is None else _ffi.JOURNEY_WAYPOINT, _GATES[direction], 0 if direction is None else int(feature),
          idx, dist)
    return signed_idx(idx), dist


def _end_point_skip(journeys, candidate_songs):
    """[G, 2]: the first candidate that == each end point of every journey (one or two songs each), as _member_skip; -1: none."""
    flat = _member_skip(journeys, candidate_songs)
    skip, row = np.full((len(journeys), 2), -1, np.int64), 0
    for g, ends in enumerate(journeys):
        skip[g, :len(ends)] = flat[row:row + len(ends)]
        row += len(ends)
    return skip


def waypoint_playlist(from_song, to_song, candidate_songs, number_songs, metric_builder=euclidean_distance):
    """"Go from song1 to song2, both picked by the users, in n songs, without any repetitions" (the reference's TODO.md): the
    `number_songs` songs between the two, in order -- song t is the candidate nearest the point (t + 1) / (number_songs + 1) of
    the way from from_song to to_song (journey_order).  The end points themselves are kept out of the pool (the first
    candidate that == each, as group_playlists does for members) and are not part of the result."""
    _no_forest(metric_builder, _JOURNEY_WHY)
    _no_variance(metric_builder, _JOURNEY_WHY)
    candidate_songs = list(candidate_songs)
    if not candidate_songs:
        return []
    metric, m = _metric_of(metric_builder)
    ends = [from_song, to_song]
    idx, _ = journey_order(_matrix(ends[:1]), _matrix(candidate_songs), number_songs, _matrix(ends[1:]), metric, m,
                           _end_point_skip([ends], candidate_songs))
    return [candidate_songs[j] for j in idx[0] if j >= 0]


def directed_playlist(first_song, candidate_songs, number_songs, feature, direction="down", metric_builder=euclidean_distance):
    """"I want the tempo to go down or stay the same" (the reference's TODO.md): up to `number_songs` songs after first_song,
    each the nearest candidate not yet played whose `feature` (an AnalysisIndex or a column number) is <= ("down") or >= ("up")
    that of the song before it.  The playlist ends early when no candidate qualifies.  first_song is kept out of the pool and
    is not part of the result."""
    _no_forest(metric_builder, _JOURNEY_WHY)
    _no_variance(metric_builder, _JOURNEY_WHY)
    if direction not in ("up", "down"):
        raise ValueError('direction must be "up" or "down"')
    candidate_songs = list(candidate_songs)
    if not candidate_songs:
        return []
    metric, m = _metric_of(metric_builder)
    idx, _ = journey_order(_matrix([first_song]), _matrix(candidate_songs), number_songs, None, metric, m,
                           _end_point_skip([[first_song]], candidate_songs), direction, int(feature))
    return [candidate_songs[j] for j in idx[0] if j >= 0]


# ---- radio playlists: chains (or the k nearest songs) under artist / album separation rules (blissgpu_radio) ----
_RADIO_WHY = "a radio's metric compares single songs, step by step"
_RULE_COLUMNS = ("artist", "album", "album_artist", "genre")
NO_LABEL = 0xFFFFFFFF  # a song without a label: no rule constrains it


@dataclasses.dataclass(frozen=True)
class Rule:
    """Among the last `window` songs of a radio (the start song included while it is that near) at most `limit` carry any one
    key.  `by`: "artist", "album", "album_artist", "genre" or a callable Song -> key (None: the song has no key and the rule
    never constrains it).  window=None: the whole list, i.e. at most `limit` songs per key in it.  Rule("artist", 5): no artist
    twice within five tracks; Rule("artist", None, 2): at most two songs per artist."""
    by: object
    window: Optional[int] = None
    limit: int = 1

    def __post_init__(self):
        if not callable(self.by) and self.by not in _RULE_COLUMNS:
            raise ValueError(f"by must be one of {_RULE_COLUMNS} or a callable Song -> key")
        if self.window is not None and int(self.window) < 0:
            raise ValueError("window must be None (the whole list) or >= 0 (0: the rule is off)")
        if int(self.limit) < 1:
            raise ValueError("limit must be at least 1")


def _rule_key(song, by):
    s = _song_of(song)
    if callable(by):
        return by(s)
    if by == "album":  # two albums called "Greatest Hits" are two albums
        owner = s.album_artist if s.album_artist is not None else s.artist
        return None if s.album is None else (owner, s.album)
    return getattr(s, by)


def rule_labels(songs, rules) -> np.ndarray:
    """uint32 [len(rules), len(songs)]: one label per rule and song, equal labels exactly for equal keys (a dictionary per rule,
    so there are no collisions), NO_LABEL for a key of None.  The key of "album" is (album_artist or artist, album)."""
    songs, rules = list(songs), list(rules)
    out = np.full((len(rules), len(songs)), NO_LABEL, np.uint32)
    for r, rule in enumerate(rules):
        seen = {}
        for i, s in enumerate(songs):
            key = _rule_key(s, rule.by)
            if key is not None:
                out[r, i] = seen.setdefault(key, len(seen))
    return out


def _rule_arrays(rules, k):
    """(windows, limits) of blissgpu_radio: None (the whole list) is k + 1"""
    rules = list(rules)
    if len(rules) > _ffi.RADIO_MAX_RULES:
        raise ValueError(f"at most {_ffi.RADIO_MAX_RULES} rules")
    return [int(k) + 1 if r.window is None else int(r.window) for r in rules], [int(r.limit) for r in rules]


def radio_order(from_rows, candidates, k, labels, windows, limits, from_labels=None, mode="chain", metric="euclidean", m=None,
                skip=None):
    """Radio playlists in one device call (blissgpu_radio): radio g starts at from_rows[g]; mode "chain": song 0 is the eligible
    candidate nearest from_rows[g], song t the eligible candidate nearest song t - 1; mode "nearest": every song is the
    eligible candidate nearest from_rows[g].  labels: [R, n] integers, one label per rule and candidate, -1 or 0xFFFFFFFF = no
    label; from_labels: [G, R], the start songs' labels, or None (they carry none).  Rule r: among the last windows[r] songs of
    the radio -- the start song is position -1, the picks follow -- at most limits[r] carry any one label; a candidate whose
    label has reached that count is not eligible, nor is one already played or in `skip` ([G, 2] candidate indices, -1: none).
    windows[r] == 0 switches the rule off, windows[r] > k is the whole list.  Equal distances go to the lower index.
    -> (idx int64[G, k], dist float32[G, k]); a radio that runs out of eligible candidates ends in -1 / inf.  A NaN distance
    of an eligible candidate raises ValueError.  VarianceWeights and ForestOptions are refused."""
    _no_forest(metric, _RADIO_WHY)
    _no_variance(metric, _RADIO_WHY)
    A = rows_f32(from_rows)
    # (the same object for both: a radio from each candidate, and the library uploads the rows once)
    X = A if candidates is from_rows else rows_f32(candidates)
    if A.ndim != 2 or X.ndim != 2 or A.shape[1] != X.shape[1]:
        raise ValueError("from_rows and candidates must be [G, d] and [n, d]")
    if metric not in _METRICS:
        raise ValueError(f"unknown metric {metric!r}")
    if mode not in _RADIO_MODES:
        raise ValueError('mode must be "chain" or "nearest"')
    k = int(k)
    (G, d), n = A.shape, X.shape[0]
    check_k_d(k, d)
    windows = np.ascontiguousarray(np.asarray(windows, dtype=np.int64).reshape(-1))
    limits = np.ascontiguousarray(np.asarray(limits, dtype=np.int64).reshape(-1))
    R = windows.shape[0]
    if limits.shape[0] != R:
        raise ValueError("windows and limits must have one entry per rule")
    if R > _ffi.RADIO_MAX_RULES:
        raise ValueError(f"at most {_ffi.RADIO_MAX_RULES} rules")
    if (windows < 0).any() or (limits < 1).any():
        raise ValueError("windows must be >= 0 and limits >= 1")
    windows = np.minimum(windows, k + 1).astype(np.uint32)
    limits = np.minimum(limits, 0xFFFFFFFF).astype(np.uint32)
    lab = fl = None
    if R:
        lab = np.asarray(labels, dtype=np.int64).reshape(R, -1) if np.size(labels) else np.zeros((R, 0), np.int64)
        if lab.shape != (R, n):
            raise ValueError("labels must be [rules, n]")
        if ((lab < -1) | (lab > 0xFFFFFFFF)).any():
            raise ValueError("labels must be -1 (none) or fit 32 bits")
        lab = np.ascontiguousarray(np.where(lab < 0, NO_LABEL, lab).astype(np.uint32))
        if from_labels is not None:
            fl = np.asarray(from_labels, dtype=np.int64)
            if fl.shape != (G, R):
                raise ValueError("from_labels must be [G, rules]")
            if ((fl < -1) | (fl > 0xFFFFFFFF)).any():
                raise ValueError("from_labels must be -1 (none) or fit 32 bits")
            fl = np.ascontiguousarray(np.where(fl < 0, NO_LABEL, fl).astype(np.uint32))
    if skip is not None:
        skip = skip_words(skip, (G, 2), n, "skip must be [G, 2]")
    m = metric_matrix(metric, m, d)
    idx, dist = np.empty((G, k), np.uint32), np.empty((G, k), np.float32)
    _call("blissgpu_radio", A, G, X, n, d, _METRICS[metric], m, lab, fl, R, windows if R else None, limits if R else None, skip, k,
          _RADIO_MODES[mode], idx, dist)
    return signed_idx(idx), dist


DEFAULT_RADIO_RULES = (Rule("artist", 5), Rule("album", 20))


def radio_playlist(first_song, candidate_songs, number_songs, rules=DEFAULT_RADIO_RULES, mode="chain",
                   metric_builder=euclidean_distance):
    """A radio from one song: up to `number_songs` songs after first_song, each the nearest candidate not yet played (mode
    "chain": nearest the song before it; "nearest": nearest first_song) that breaks none of `rules` -- by default no artist
    twice within 5 tracks and no album twice within 20, first_song counting as the track before the first.  The radio ends
    early when every remaining candidate is ruled out.  first_song is kept out of the pool (the first candidate that == it)
    and is not part of the result."""
    _no_forest(metric_builder, _RADIO_WHY)
    _no_variance(metric_builder, _RADIO_WHY)
    candidate_songs, rules = list(candidate_songs), list(rules)
    if not candidate_songs:
        return []
    metric, m = _metric_of(metric_builder)
    labels = rule_labels(candidate_songs + [first_song], rules)
    windows, limits = _rule_arrays(rules, number_songs)
    idx, _ = radio_order(_matrix([first_song]), _matrix(candidate_songs), number_songs, labels[:, :-1], windows, limits,
                         labels[:, -1:].T, mode, metric, m, _end_point_skip([[first_song]], candidate_songs))
    return [candidate_songs[j] for j in idx[0] if j >= 0]


def meta_keys(songs) -> np.ndarray:
    """One u32 key per song for the title / artist rule of dedup_playlist_custom_distance (src/playlist.rs:383-389:
    both titles and both artists Some, and equal): 0 when the title or the artist is None, otherwise equal keys
    exactly for equal (title, artist) -- a dictionary, so there are no collisions."""
    seen, keys = {}, np.zeros(len(songs), np.uint32)
    for i, s in enumerate(songs):
        s = _song_of(s)
        if s.title is not None and s.artist is not None:
            keys[i] = seen.setdefault((s.title, s.artist), len(seen) + 1)
    return keys


def dedup_order(X, seq=None, meta=None, metric="euclidean", m=None, threshold=None) -> np.ndarray:
    """Index form of dedup_playlist_custom_distance (src/playlist.rs:367-402) in one device call: the playlist is
    X[seq] (seq = None: every row of X in order), meta holds one key per ROW of X (see meta_keys; None: no title /
    artist rule).  Returns the kept positions into seq (int64).  A NaN distance the reference would evaluate raises
    ValueError, like its n32() panic."""
    X = rows_f32(X)
    n, d = X.shape
    if seq is not None:
        seq = np.ascontiguousarray(seq, dtype=np.uint32).reshape(-1)
    length = n if seq is None else seq.shape[0]
    if meta is not None:
        meta = np.ascontiguousarray(meta, dtype=np.uint32).reshape(-1)
        if meta.shape[0] != n:
            raise ValueError("meta needs one key per row of X")
    kept, n_kept = np.empty(max(length, 1), np.uint32), C.c_uint64()
    try:
        _ffi.call("blissgpu_dedup_playlist", X, n, d, seq, length, meta, _METRICS[metric], metric_matrix(metric, m),
                  np.float32(0.05 if threshold is None else threshold), kept, C.byref(n_kept))
    except _ffi.BlissGpuError as e:
        if e.code == _ffi.ERR_NAN:
            raise ValueError("NaN distance (noisy_float::n32 panic in the reference)") from e
        raise
    return kept[:n_kept.value].astype(np.int64)


def dedup_playlist_custom_distance(playlist, distance_threshold=None, metric_builder=euclidean_distance, window=64):
    """src/playlist.rs:367-402: a song absorbs the songs that follow it while they are closer than the threshold
    (default 0.05) or carry the same non-empty title and artist.  One device call for the whole playlist
    (dedup_order); `window` is accepted for compatibility and unused."""
    _no_forest(metric_builder, "dedup_playlist_custom_distance builds its metric from single songs (:367-402)")
    _no_variance(metric_builder, "dedup_playlist_custom_distance builds its metric from single songs (:367-402)")
    playlist = list(playlist)
    if not playlist:
        return []
    metric, m = _metric_of(metric_builder)
    kept = dedup_order(_matrix(playlist), None, meta_keys(playlist), metric, m, distance_threshold)
    return [playlist[i] for i in kept]


def dedup_playlist(playlist, distance_threshold=None):
    """src/playlist.rs:343-348"""
    return dedup_playlist_custom_distance(playlist, distance_threshold, euclidean_distance)


def duplicate_labels(X, meta=None, metric="euclidean", m=None, threshold=None, return_pairs=False):
    """Which rows of X are the same song: the duplicate rule of dedup_playlist_custom_distance (src/playlist.rs:381-388)
    over EVERY pair i < j -- distance < threshold (default 0.05; the distance is bit for bit pairwise_distances(X, X)[i, j]),
    or meta[i] != 0 and meta[i] == meta[j] (see meta_keys; None: no title / artist rule) -- and the connected components of
    those edges, in one device call without the distance matrix.  -> labels int64[n]: the smallest row of each row's
    component.  With `return_pairs` -> (labels, pairs int64[e, 2] in ascending (i, j), dist float32[e]).  A NaN distance
    raises ValueError, like the reference's n32() panic."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    if X.ndim != 2:
        raise ValueError("X must be [n, d]")
    n, d = X.shape
    if not 1 <= d <= 64:
        raise ValueError("d must be 1 .. 64")
    if metric not in _METRICS:
        raise ValueError(f"unknown metric {metric!r}")
    thr = np.float32(0.05 if threshold is None else threshold)
    if np.isnan(thr):
        raise ValueError("threshold is NaN")
    if meta is not None:
        meta = np.ascontiguousarray(meta, dtype=np.uint32).reshape(-1)
        if meta.shape[0] != n:
            raise ValueError("meta needs one key per row of X")
    if m is not None:  # (this entry point checks, and passes, an m beside any metric)
        m = metric_matrix(metric, m)
        if m.shape != (d, d):
            raise ValueError("m must be [d, d]")
    elif metric == "mahalanobis":
        raise ValueError("mahalanobis needs m")
    labels, n_pairs = np.empty(max(n, 1), np.uint32), C.c_uint64()

    def run(cap):
        pairs = np.empty((max(cap, 1), 2), np.uint32) if return_pairs else None
        dist = np.empty(max(cap, 1), np.float32) if return_pairs else None
        try:
            _ffi.call("blissgpu_duplicate_groups", X, n, d, meta, _METRICS[metric], m, thr, labels, C.byref(n_pairs), pairs, dist,
                      cap if return_pairs else 0)
        except _ffi.BlissGpuError as e:
            if e.code == _ffi.ERR_NAN:
                raise ValueError("NaN distance (noisy_float::n32 panic in the reference)") from e
            raise
        return pairs, dist

    cap = max(1024, n)  # duplicates are rare in a real library; a fuller list is fetched by the second call
    pairs, dist = run(cap)
    if return_pairs and n_pairs.value > cap:
        cap = n_pairs.value
        pairs, dist = run(cap)
    out = labels[:n].astype(np.int64)
    if not return_pairs:
        return out
    e = n_pairs.value
    return out, pairs[:e].astype(np.int64), dist[:e].copy()


def groups_from_labels(labels):
    """Component labels (label = smallest member, as duplicate_labels returns them) -> the components of two or more
    members as index arrays (int64, ascending), ordered by their smallest member."""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    if labels.size == 0:
        return []
    order = np.argsort(labels, kind="stable")  # by label; members of one label stay ascending
    cuts = np.flatnonzero(np.diff(labels[order])) + 1
    return [g for g in np.split(order, cuts) if g.size >= 2]


def duplicate_groups(songs, distance_threshold=None, metric_builder=euclidean_distance):
    """The songs of a collection that are the same song: groups (lists of the caller's own objects, two or more each) of
    songs joined -- directly or through a chain -- by the duplicate rule of dedup_playlist_custom_distance
    (src/playlist.rs:381-388): closer than the threshold (default 0.05) or the same non-empty title and artist.  Unlike
    dedup_playlist, which compares the neighbours of an ordered playlist, every pair is looked at.  Groups come by their
    first member, members in the order of `songs`."""
    _no_forest(metric_builder, "duplicate_groups builds its metric from single songs")
    _no_variance(metric_builder, "duplicate_groups builds its metric from single songs")
    songs = list(songs)
    if not songs:
        return []
    metric, m = _metric_of(metric_builder)
    labels = duplicate_labels(_matrix(songs), meta_keys(songs), metric, m, distance_threshold)
    return [[songs[i] for i in g] for g in groups_from_labels(labels)]


# ---- acoustic fingerprints: the same RECORDING, whatever the features say (blissgpu_fingerprint_match) ----
FINGERPRINT_MAX_OFFSET = 430   # hops of 512 samples: +-10 s
FINGERPRINT_MIN_OVERLAP = 256  # valid positions an alignment needs: 6 s
FINGERPRINT_THRESHOLD = 0.35   # bit error rate below which two excerpts are one recording (Haitsma & Kalker 2002, section 4.3)
FINGERPRINT_ALL_PAIRS_MAX = 4096


def _fingerprints(fps):
    fps = [np.ascontiguousarray(f, dtype=np.uint32).reshape(-1) for f in fps]
    offsets = np.zeros(len(fps) + 1, np.uint64)
    if fps:
        offsets[1:] = np.cumsum([f.shape[0] for f in fps], dtype=np.uint64)
    return fps, offsets


def _pair_array(pairs, n):
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if pairs.size and (pairs.min() < 0 or pairs.max() >= n):
        raise ValueError("pairs must index the fingerprints")
    return pairs


def fingerprint_match(fps, pairs, max_offset=FINGERPRINT_MAX_OFFSET, min_overlap=FINGERPRINT_MIN_OVERLAP):
    """How well do two fingerprints (fingerprint_batch) align?  For every pair (i, j) of `pairs` and every offset o in
    [-max_offset, max_offset], the words fps[i][t] and fps[j][t + o] that are both non-zero (a zero word is silence) are
    compared bit by bit; an offset counts when at least min_overlap positions are compared, and the best one has the smallest
    errors / bits (compared exactly; ties to the smaller (|o|, o)).  -> (offset int32 [P], errors uint32 [P], bits uint32 [P]);
    bits == 0 (and offset == errors == 0) where no offset counts, as for a pair with an empty fingerprint, which never reaches
    the device.  The defaults are +-10 s and 6 s.  One device call; the result is defined to the bit by include/blissgpu.h."""
    fps, offsets = _fingerprints(fps)
    pairs = _pair_array(pairs, len(fps))
    P = pairs.shape[0]
    offset, errors, bits = np.zeros(P, np.int32), np.zeros(P, np.uint32), np.zeros(P, np.uint32)
    if not 0 <= int(max_offset) <= 4096:
        raise ValueError("max_offset must be 0 .. 4096")
    if int(min_overlap) < 1:
        raise ValueError("min_overlap must be >= 1")
    if P == 0:
        return offset, errors, bits
    lens = np.diff(offsets.astype(np.int64))
    live = np.flatnonzero((lens[pairs[:, 0]] > 0) & (lens[pairs[:, 1]] > 0))
    if live.size == 0:
        return offset, errors, bits
    words = np.concatenate(fps)
    sent = np.ascontiguousarray(pairs[live], dtype=np.uint32)
    o, e, b = np.zeros(live.size, np.int32), np.zeros(live.size, np.uint32), np.zeros(live.size, np.uint32)
    _ffi.call("blissgpu_fingerprint_match", words, offsets, len(fps), sent, live.size, int(max_offset), int(min_overlap), o, e, b)
    offset[live], errors[live], bits[live] = o, e, b
    return offset, errors, bits


def _threshold_fraction(threshold):
    """threshold as an exact fraction (numerator, denominator): a float at its shortest decimal form (0.35 is 7 / 20, not the
    binary number next to it), a Fraction or an int as it is"""
    import fractions

    f = threshold if isinstance(threshold, (fractions.Fraction, int)) else fractions.Fraction(repr(float(threshold)))
    f = fractions.Fraction(f)
    if f < 0:
        raise ValueError("threshold must not be negative")
    return f.numerator, f.denominator


def fingerprint_edges(errors, bits, threshold=FINGERPRINT_THRESHOLD) -> np.ndarray:
    """bool [P]: bits > 0 and errors < threshold * bits, evaluated exactly in integers (errors * den < num * bits with
    threshold = num / den, see _threshold_fraction)."""
    num, den = _threshold_fraction(threshold)
    errors, bits = np.asarray(errors), np.asarray(bits)
    if max(num, den) < 2 ** 31:  # errors, bits < 2^32: the products fit 63 bits
        lhs, rhs = errors.astype(np.int64) * den, bits.astype(np.int64) * num
    else:
        lhs, rhs = errors.astype(object) * den, bits.astype(object) * num
    return (bits > 0) & np.asarray(lhs < rhs, dtype=bool)


def labels_from_edges(n, pairs, edge) -> np.ndarray:
    """Connected components of the pairs whose `edge` is set, on the host (union-find): int64 [n], the smallest index of
    every index's component -- the labels duplicate_labels returns."""
    parent = list(range(n))
    for (i, j), on in zip(np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist(), np.asarray(edge, dtype=bool).tolist()):
        if on:
            a, b = _uf_find(parent, i), _uf_find(parent, j)
            if a != b:
                parent[max(a, b)] = min(a, b)  # the root is always the component's smallest index
    return np.asarray([_uf_find(parent, i) for i in range(n)], dtype=np.int64)


def fingerprint_duplicates(fps, pairs=None, threshold=FINGERPRINT_THRESHOLD, max_offset=FINGERPRINT_MAX_OFFSET,
                           min_overlap=FINGERPRINT_MIN_OVERLAP, return_match=False):
    """Which fingerprints are the same recording: the pairs (None: every pair i < j, refused above 4096 fingerprints -- build
    candidate pairs instead, as library.fingerprint_duplicates does) are matched in one device call (fingerprint_match); a pair
    is an edge when bits > 0 and errors < threshold * bits, exactly (fingerprint_edges; 0.35 is the paper's threshold), and
    the edges' connected components are found on the host.  -> labels int64 [n], the smallest index of every component, as
    duplicate_labels returns them (groups_from_labels makes groups).  return_match: -> (labels, pairs, offset, errors, bits)."""
    fps = list(fps)
    n = len(fps)
    if pairs is None:
        if n > FINGERPRINT_ALL_PAIRS_MAX:
            raise ValueError(f"all pairs of {n} fingerprints: pass candidate pairs above {FINGERPRINT_ALL_PAIRS_MAX}")
        i, j = np.triu_indices(n, 1)
        pairs = np.stack([i, j], axis=1)
    pairs = _pair_array(pairs, n)
    offset, errors, bits = fingerprint_match(fps, pairs, max_offset, min_overlap)
    labels = labels_from_edges(n, pairs, fingerprint_edges(errors, bits, threshold))
    return (labels, pairs, offset, errors, bits) if return_match else labels


def variance_based_weight_matrix(seeds) -> np.ndarray:
    """src/playlist.rs:173-221: diagonal Mahalanobis weights ~ 1 / (variance + 1e-6), normalised to sum to d.
    O(seeds x d) host arithmetic in the reference's f32 evaluation order."""
    from .song import ProviderError

    seeds = [np.asarray(s, dtype=np.float32).reshape(-1) for s in seeds]
    if len(seeds) < 2:
        raise ProviderError("seeds must contain more than one element")
    n = seeds[0].shape[0]
    if n == 0:
        raise ProviderError("seed feature vectors must not be empty")
    if any(s.shape[0] != n for s in seeds):
        raise ProviderError("all seed feature vectors must have the same length")
    ns = np.float32(len(seeds))
    mean = np.zeros(n, np.float32)
    for s in seeds:
        mean = mean + s
    mean = mean / ns
    var = np.zeros(n, np.float32)
    for s in seeds:
        diff = s - mean
        var = var + diff * diff
    var = var / ns
    w = np.float32(1.0) / (var + np.float32(1e-6))
    # ndarray's sum(): unrolled_fold, 8 partial sums combined (p0+p4)+(p1+p5)+(p2+p6)+(p3+p7), then the tail
    p = np.zeros(8, np.float32)
    k = 0
    while k + 8 <= n:
        p = p + w[k:k + 8]
        k += 8
    total = np.float32(0.0)
    for u in range(4):
        total = np.float32(total + np.float32(p[u] + p[u + 4]))
    for x in w[k:]:
        total = np.float32(total + x)
    w = w * np.float32(np.float32(n) / total)
    return np.diag(w).astype(np.float32)


def closest_album_to_group(group, pool):
    """src/playlist.rs:424-485: albums of `pool` ordered by the euclidean distance of their mean analysis to the
    group's mean analysis (distances on the device), each album ordered by (disc, track) number."""
    from .song import ProviderError

    group, pool = list(group), list(pool)
    pool = [s for s in pool if not any(_song_of(g) == _song_of(s) for g in group)]
    albums = {}
    for s in pool:
        album = _song_of(s).album
        if album is not None:
            albums.setdefault(album, []).append(np.asarray(_song_of(s).analysis.as_vec(), dtype=np.float32))

    def mean_axis0(rows):  # ndarray mean_axis: sequential f32 row sum / n
        if not rows:
            raise ProviderError("Mean of empty slice")
        acc = np.zeros_like(rows[0])
        for r in rows:
            acc = acc + r
        return acc / np.float32(len(rows))

    first = mean_axis0([np.asarray(_song_of(s).analysis.as_vec(), dtype=np.float32) for s in group])
    names = list(albums.keys())
    playlist = list(group)
    if names:
        means = np.stack([mean_axis0(albums[a]) for a in names])
        order, _ = closest_to_songs_order(first[None, :], means, "euclidean")  # sort_by_key is stable as well
        for a in (names[i] for i in order):
            al = [s for s in pool if _song_of(s).album == a]

            def key(s):
                s = _song_of(s)
                d, t = s.disc_number, s.track_number
                return ((0, 0) if d is None else (1, d), (0, 0) if t is None else (1, t))  # Option: None < Some

            al.sort(key=key)
            playlist.extend(al)
    return playlist


def nearest_albums(seed_groups, candidates, album_of, k, skip=None, return_means=False):
    """The k nearest ALBUMS of every seed group in one device call (blissgpu_album_knn), without a groups x albums matrix: row
    g is closest_album_to_group (src/playlist.rs:424-485) cut after k albums, as album indices.  `album_of`: one integer per
    candidate, its album's index (0 .. album_of.max()), -1 = the song has no album.  `seed_groups` and `skip` as for
    nearest_to_groups: the skipped candidates leave their albums BEFORE the album means are formed, an album that loses every
    song does not exist for that group.  Means are sequential f32 row sums divided by the count (ndarray's mean_axis), the
    distance is euclidean_distance(group mean, album mean) bit for bit.  -> (idx int64[G, k], dist float32[G, k]): the albums
    in ascending (distance, album index); rows with fewer than k existing albums end in -1 / inf.  return_means=True: ->
    (idx, dist, group_means float32[G, d], centroids float32[A, d]), centroids being the FULL-album means (NaN rows for album
    indices no song uses).  An empty group raises ProviderError("Mean of empty slice") before the library is reached; a NaN
    distance raises ValueError (the reference's n32() panic)."""
    from .song import ProviderError

    S, off = _seed_groups(seed_groups)
    X = rows_f32(candidates)
    if X.ndim != 2 or (S is not None and S.shape[1] != X.shape[1]):
        raise ValueError("seed groups and candidates must be [s_g, d] and [n, d]")
    n, d = X.shape
    album_of = np.asarray(album_of)
    if album_of.ndim != 1 or album_of.shape[0] != n or (album_of.size and album_of.dtype.kind not in "iu"):
        raise ValueError("album_of must hold one integer per candidate")
    album_of = album_of.astype(np.int64)
    if (album_of < -1).any() or (album_of >= max(n, 0)).any():
        raise ValueError("album_of entries must be album indices below the number of candidates, or -1")
    k = int(k)
    check_k_d(k, d)
    G = off.shape[0] - 1
    if (np.diff(off.astype(np.int64)) == 0).any():
        raise ProviderError("Mean of empty slice")
    skip = _group_skip(skip, off, n)
    A = int(album_of.max()) + 1 if album_of.size else 0
    album_u32 = np.where(album_of < 0, 0xFFFFFFFF, album_of).astype(np.uint32)
    idx, dist = np.empty((G, k), np.uint32), np.empty((G, k), np.float32)
    means = np.empty((G, d), np.float32) if return_means else None
    centroids = np.empty((A, d), np.float32) if return_means else None
    _call("blissgpu_album_knn", S, off, G, X, n, d, album_u32, A, skip, k, idx, dist, means, centroids)
    out = signed_idx(idx)
    return (out, dist, means, centroids) if return_means else (out, dist)


def _disc_track_key(s):
    s = _song_of(s)
    d, t = s.disc_number, s.track_number
    return ((0, 0) if d is None else (1, d), (0, 0) if t is None else (1, t))  # Option: None < Some


def closest_albums_to_groups(groups, pool, number_albums):
    """For every group of songs, closest_album_to_group(group, pool) (src/playlist.rs:424-485) cut after the `number_albums`
    closest albums: the group, then each chosen album's pool songs ordered by (disc_number, track_number), None < Some -- "play
    these songs, then the albums most like them", all groups in ONE device call (nearest_albums).  Albums are numbered in order
    of first appearance in `pool`; the first pool song that == each member (Song: PartialEq) leaves the pool of that group
    before its album's mean is formed.  Equal distances come in order of first appearance."""
    from .song import ProviderError

    groups, pool = [list(g) for g in groups], list(pool)
    if not groups:
        return []
    if any(not g for g in groups):
        raise ProviderError("Mean of empty slice")
    number_albums = int(number_albums)
    if number_albums <= 0 or not pool:
        return [list(g) for g in groups]
    names, album_of = {}, np.full(len(pool), -1, np.int64)
    for i, s in enumerate(pool):
        album = _song_of(s).album
        if album is not None:
            album_of[i] = names.setdefault(album, len(names))
    if not names:
        return [list(g) for g in groups]
    k = min(number_albums, len(names))
    if k > 1024:
        raise ValueError("at most 1024 albums per playlist")
    skip = _member_skip(groups, pool)
    off = np.zeros(len(groups) + 1, np.int64)
    off[1:] = np.cumsum([len(g) for g in groups])
    idx, _ = nearest_albums((_matrix([s for g in groups for s in g]), off), _matrix(pool), album_of, k, skip)
    rows = [[] for _ in names]
    for i, a in enumerate(album_of):
        if a >= 0:
            rows[a].append(i)
    out, at = [], 0
    for g, row in zip(groups, idx):
        gone = set(int(j) for j in skip[at:at + len(g)] if j >= 0)
        at += len(g)
        playlist = list(g)
        for a in row:
            if a >= 0:
                playlist.extend(sorted((pool[i] for i in rows[a] if i not in gone), key=_disc_track_key))
        out.append(playlist)
    return out
