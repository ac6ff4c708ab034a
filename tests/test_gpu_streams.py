"""Stream order of every device entry point on streams the caller owns (-m gpu).

The C ABI promises three things about streams (include/blissgpu.h: blissgpu_ctx_wait_stream / _signal_stream / _set_stream),
and every method of device.Context rests on them: it brackets its C call with `_pre()` / `_post()`.  The rest of the suite
uploads on the legacy default stream, calls a family and synchronises the host, which orders everything whatever the library
does.  Here the inputs arrive LATE and the results are read EARLY:

  * the buffers a method is given hold a DECOY (valid inputs of the same shapes: tests/staging_cases.py::Case(seed=1) and its
    like) -- a delay is queued on the producer stream P, and only behind it the copies that bring the real inputs;
  * with P as torch's current stream the method is called, and straight behind it, still on P, its outputs are cloned;
  * only then is the host synchronised.  The clones must equal, byte for byte, what the same call gives with the host
    synchronised before and after it (the path every other test file holds to the oracle).

A method that does not wait for P computes on the decoy; one that does not make P wait for it, or whose last launch or copy
is on another stream than the context's, has its outputs cloned before they are written.  Four stream modes (MODES) put the
context on its own stream, on P itself, and on a second caller stream.

The delay is calibrated per module: at least 20 ms and at least ten times the longest call of the synchronous pass.  Whether
losing the race SHOWS on this machine (two streams mapped onto one hardware queue serialise, which hides a missing wait) is
what test_control_a_call_that_does_not_wait_computes_on_the_decoy establishes; the stream it finds is the side stream of
every other test.

CASES is the one table all of this runs on; tests/test_host_logic.py holds it to _ffi.SIGNATURES, so this module imports
without torch or a device."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import staging_cases as sc

pytestmark = pytest.mark.gpu

MODES = ("own/default", "own/side", "adopted", "adopted/other")
SONG = 6 * 22050  # samples of one analysed song
F32 = np.float32

# `*_device` names of _ffi.SIGNATURES that have no case here, each with its reason (tests/test_host_logic.py)
EXCLUDED = {
    "blissgpu_node_analyze_device": "the node_* API owns one context per rank and synchronises all of them before it returns",
    "blissgpu_default_device": "no entry point: it returns the device ordinal of a default context",
}


# ---------------------------------------------------------------------------------------------------------------------------
# inputs: every builder gives the real set (decoy=False) and a decoy of the same shapes and dtypes that is as valid as the real
# one.  Keys that start with "h_" are host arguments (offsets, lengths, file bytes): they never sit in a device buffer, the
# ordered passes always pass the real ones; a decoy differs in them only where an output depends on nothing else.

@functools.lru_cache(maxsize=None)
def _grid(decoy):
    return sc.Case(*sc.SHAPES[0], seed=1 if decoy else None)


@functools.lru_cache(maxsize=None)
def _scan(decoy):
    c, rng = _grid(decoy), np.random.default_rng((77, int(decoy)))
    occ = rng.integers(0, c.n, (c.q, c.k)).astype(np.int32)
    occ[0, 0] = -1
    labels4 = rng.integers(0, 4, c.n).astype(np.int32)
    return dict(
        X=c.X, S=c.S, Q=c.Q, M=c.M, skip=c.skip.view(np.int32), qskip=c.qskip.view(np.int32),
        qskip2=c.qskip2.view(np.int32), album_of=c.album_of.view(np.int32),
        B=np.ascontiguousarray(c.X[rng.choice(c.n, c.q, replace=False)]),
        qscale=rng.uniform(0.5, 2.0, c.q).astype(F32), cscale=rng.uniform(0.5, 2.0, c.n).astype(F32),
        rules=np.stack([rng.integers(0, 7, c.n), rng.integers(0, 11, c.n)]).astype(np.int32),
        from_rules=np.stack([rng.integers(0, 7, c.q), rng.integers(0, 11, c.q)], 1).astype(np.int32),
        labels4=labels4, labels4_i64=labels4.astype(np.int64), core=rng.uniform(0.1, 1.0, c.n).astype(F32),
        init=np.ascontiguousarray(c.X[rng.choice(c.n, 4, replace=False)]),
        XU=rng.uniform(-1.0, 1.0, (c.n, sc.D)).astype(F32),  # (the grid's minima and maxima are -1 and 1 in every draw)
        triplets=np.stack([rng.permutation(c.n)[:3] for _ in range(64)]).astype(np.int32), occ=occ,
        # the group sizes decide the status words of group_weights and its users: the decoy's groups are 2, 1 and 4 seeds
        h_off=np.array([0, 2, 3, 7], np.uint64) if decoy else c.off)


@functools.lru_cache(maxsize=None)
def _twins(decoy):
    """the grid with every row present twice (the copies shuffled), a playlist over it in which some copies follow their
    original and are absorbed, and title / artist keys that add a few edges"""
    c, rng = _grid(decoy), np.random.default_rng((78, int(decoy)))
    perm = rng.permutation(c.n)
    twin = np.empty(c.n, np.int64)
    twin[perm] = c.n + np.arange(c.n)  # where row i's copy is
    follows = rng.random(c.n) < (0.6 if decoy else 0.3)
    seq = []
    for i in range(c.n):
        seq.append(i)
        if follows[i]:
            seq.append(int(twin[i]))
    seq += [int(twin[i]) for i in range(c.n) if not follows[i]]
    meta = np.zeros(2 * c.n, np.int32)
    if decoy:
        meta[[4, 11, 20]] = 9
    else:
        meta[[3, 10]] = 7
    return dict(X2=np.concatenate([c.X, c.X[perm]]), seq=np.array(seq, np.int32), meta=meta)


@functools.lru_cache(maxsize=None)
def _frames(decoy):
    rng = np.random.default_rng((79, int(decoy)))
    return dict(frames=rng.integers(-20000, 20000, (3000, 2), dtype=np.int16))


@functools.lru_cache(maxsize=None)
def _songs(decoy):
    """three white-noise songs of 6 s; the status words depend on the lengths alone, so the decoy's last song is too short"""
    rng = np.random.default_rng((80, int(decoy)))
    return dict(pcm=rng.uniform(-0.5, 0.5, 3 * SONG).astype(F32), h_offsets=[0, SONG, 2 * SONG],
                h_lengths=[SONG, SONG, 5000 if decoy else SONG], h_first=300007 if decoy else 300000,
                h_index=[6, 1, 3] if decoy else [5, 9, 2])


@functools.lru_cache(maxsize=None)
def _flac(decoy):
    """flac_craft's "bs192" stream (two frames of 192 stereo samples and one of 1); the decoy is another stream whose second
    frame has a reserved subframe type, so that its status words differ too"""
    import flac_craft

    samples = flac_craft._rng_samples(99 if decoy else 20, 2 * 192 + 1, 2, 16)
    recipe = [dict(blocksize=192), dict(blocksize=192, subframes=dict(type=5)), dict(blocksize=1)] if decoy else dict(blocksize=192)
    data, _ = flac_craft.stream(samples, 16, recipe)
    return dict(h_data=np.frombuffer(data, np.uint8).copy(), pcm16=samples.astype(np.int16))


@functools.lru_cache(maxsize=None)
def _flac_frames(decoy):
    """what flac_decode hands to flac_crc16 for the REAL stream: status 0 and the end of every frame; the decoy has a frame
    that failed and ends one byte early (inside the file: a CRC over the wrong bytes)"""
    import flac_craft

    data, table = flac_craft.stream(flac_craft._rng_samples(20, 2 * 192 + 1, 2, 16), 16, dict(blocksize=192))
    table = np.array(table, np.uint64)
    status, end = np.zeros(len(table), np.int32), (table[:, 0] + table[:, 1]).astype(np.int64) - 2
    if decoy:
        status[1], end = 1, end - 1
    return dict(h_data=np.frombuffer(data, np.uint8).copy(), h_table=table, status=status, end=end)


_FOREST = {}


def _forest_options():
    from bliss_rs_amd import playlist

    return playlist.ForestOptions(10, 16, None, 1, seed=5)


def _forest():
    """10 trees with psi = 16 over the first 64 real rows: host data, built once (the candidates are the device input)"""
    if "f" not in _FOREST:
        from bliss_rs_amd import playlist

        _FOREST["f"] = playlist.Forest(_grid(False).X[:64], _forest_options())
    return _FOREST["f"]


# ---------------------------------------------------------------------------------------------------------------------------
# the table

class StreamCase:
    """name; entry: the C symbols the call goes through; source(decoy) -> the input sets, keys: the ones this case passes;
    run(ctx, t) -> the outputs (device tensors; numpy arrays where the method returns host data); host: the inputs go in as
    numpy arrays (the wrapper uploads them itself); options: context options for the adopted modes"""

    def __init__(self, name, entry, source, keys, run, host=False, options=None):
        self.name, self.entry, self.source, self.keys, self.run = name, tuple(entry), source, tuple(keys), run
        self.host, self.options = host, dict(options or {})

    def inputs(self, decoy):
        s = self.source(decoy)
        return {k: s[k] for k in self.keys}

    def __repr__(self):
        return self.name


CASES = []
K, WINDOWS, LIMITS = sc.SHAPES[0][2], (2, 4), (1, 2)


def _add(name, entry, source, keys, run, **kw):
    CASES.append(StreamCase(name, ["blissgpu_" + e for e in entry.split()], source, keys.split(), run, **kw))


def _zeros(ctx, n):
    return ctx.torch.zeros(n, dtype=ctx.torch.float32, device=f"cuda:{ctx.device}")


def _synth(ctx, t, **kw):
    pcm = _zeros(ctx, 3 * 22050)  # (queued on the caller's stream: the generator must come behind it)
    ctx.synth_white_noise(pcm, [0, 22050, 44100], [22050] * 3, **kw)
    return (pcm,)


def _learn(ctx, t):
    r = ctx.learn_metric(t["X"], t["triplets"], max_iter=5)
    return r.m, r.objective, r.active


def _triplet(ctx, t):
    n_active, loss, G, flags = ctx.triplet_step(t["X"], t["triplets"], t["M"], margin=0.1, return_flags=True)
    return G, flags, np.array([n_active, loss], np.float64)


def _dedup(ctx, t):
    kept, n_kept = ctx.dedup_playlist(t["X2"], seq=t["seq"])
    slot = ctx.torch.arange(kept.shape[0], device=kept.device)
    return ctx.torch.where(slot < n_kept, kept, -1), n_kept  # (the slots behind n_kept are not written; no host read here)


def _md5(ctx, t):
    return (np.frombuffer(bytes.fromhex(ctx.flac_md5(t["pcm16"], 16)), np.uint8),)


def _flac_decode(ctx, t):
    pcm, _, status, end, _ = ctx.flac_decode(t["h_data"], return_frames=True)
    return pcm, status, end


_add("analyze", "analyze_batch_device", _songs, "pcm h_offsets h_lengths",
     lambda ctx, t: ctx.analyze(t["pcm"], t["h_offsets"], t["h_lengths"]), options={"pipeline_chunks": 2, "workspace_limit": 3 << 20})  # (pipeline_chunks cuts big batches only; 3 MiB: two songs)
_add("synth_white_noise", "synth_white_noise_device", _songs, "h_first", lambda ctx, t: _synth(ctx, t, first_song_index=t["h_first"]))
_add("synth_white_noise_indexed", "synth_white_noise_indexed_device", _songs, "h_index",
     lambda ctx, t: _synth(ctx, t, song_index=t["h_index"]))
_add("pcm_s16_to_f32", "pcm_s16_to_f32_device", _frames, "frames", lambda ctx, t: (ctx.pcm_s16_to_f32(t["frames"]),))
_add("pcm_downmix", "pcm_downmix_device", _frames, "frames", lambda ctx, t: (ctx.pcm_downmix(t["frames"]),))
_add("pcm_decode", "pcm_decode_device", _frames, "frames", lambda ctx, t: (ctx.pcm_decode(t["frames"], 44100),))
_add("flac_decode[host]", "flac_decode_device", _flac, "h_data", _flac_decode, host=True)
_add("flac_crc16", "flac_crc16_device", _flac_frames, "h_data h_table status end",
     lambda ctx, t: (ctx.flac_crc16(t["h_data"], t["h_table"], t["status"], t["end"]),))
_add("flac_md5", "flac_md5_device", _flac, "pcm16", _md5)
_add("pairwise", "pairwise_device", _scan, "Q X M", lambda ctx, t: (ctx.pairwise(t["Q"], t["X"], "mahalanobis", t["M"]),))
_add("set_distance", "set_distance_device", _scan, "S X M", lambda ctx, t: (ctx.set_distance(t["S"], t["X"], "mahalanobis", t["M"]),))
_add("closest_to_songs", "closest_to_songs_device", _scan, "S X M",
     lambda ctx, t: ctx.closest_to_songs(t["S"], t["X"], "mahalanobis", t["M"], return_distances=True))
_add("song_to_song", "song_to_song_device", _scan, "S X M", lambda ctx, t: (ctx.song_to_song(t["S"], t["X"], "mahalanobis", t["M"]),))
_add("dedup_playlist", "dedup_playlist_device", _twins, "X2 seq", lambda ctx, t: _dedup(ctx, t))
_add("duplicate_labels", "duplicate_groups_device", _twins, "X2 meta", lambda ctx, t: ctx.duplicate_labels(t["X2"], meta=t["meta"]))
_add("knn", "knn_device", _scan, "Q X M qskip", lambda ctx, t: ctx.knn(t["Q"], t["X"], K, "mahalanobis", t["M"], skip=t["qskip"]))
_add("scaled_knn", "scaled_knn_device", _scan, "Q qscale X cscale M qskip",
     lambda ctx, t: ctx.scaled_knn(t["Q"], t["qscale"], t["X"], t["cscale"], K, "mahalanobis", t["M"], skip=t["qskip"]))
_add("knn_occurrence", "knn_occurrence_device", _scan, "occ", lambda ctx, t: (ctx.knn_occurrence(t["occ"], sc.SHAPES[0][0]),))
for _h in (False, True):
    _tag, _lab = ("[host]", "labels4") if _h else ("", "labels4_i64")  # (int64 labels are narrowed on the caller's stream)
    _add("kmeans" + _tag, "kmeans_device", _scan, "X init", lambda ctx, t: ctx.kmeans(t["X"], t["init"], max_iter=5)[:4], host=_h)
    _add("silhouette" + _tag, "silhouette_device", _scan, "X " + _lab,
         lambda ctx, t, lab=_lab: ctx.silhouette(t["X"], t[lab], k=4), host=_h)
    _add("group_neighbours" + _tag, "group_neighbours_device", _scan, "X " + _lab,
         lambda ctx, t, lab=_lab: ctx.group_neighbours(t["X"], t[lab], k=4, t=2, want_matrix=True), host=_h)
    _add("mst" + _tag, "mst_device", _scan, "X", lambda ctx, t: ctx.mst(t["X"])[:3], host=_h)
    _add("mst_core" + _tag, "mst_device", _scan, "X core", lambda ctx, t: ctx.mst(t["X"], core=t["core"])[:3], host=_h)
    _add("moments" + _tag, "moments_device", _scan, "XU " + _lab, lambda ctx, t, lab=_lab: ctx.moments(t["XU"], t[lab], k=4), host=_h)
_add("triplet_step", "triplet_step_device", _scan, "X triplets M", _triplet)
_add("learn_metric", "learn_metric_device", _scan, "X triplets", _learn)
_add("group_weights", "group_weights_device", _scan, "S h_off", lambda ctx, t: ctx.group_weights(t["S"], t["h_off"]))
_add("group_knn", "group_knn_device", _scan, "S h_off X M skip",
     lambda ctx, t: ctx.group_knn(t["S"], t["h_off"], t["X"], K, "mahalanobis", t["M"], skip=t["skip"]))
_add("group_knn_weighted", "group_knn_weighted_device", _scan, "S h_off X skip",
     lambda ctx, t: ctx.group_knn(t["S"], t["h_off"], t["X"], K, skip=t["skip"], weights="variance"))
_add("album_knn", "album_knn_device", _scan, "S h_off X album_of skip",
     lambda ctx, t: ctx.album_knn(t["S"], t["h_off"], t["X"], t["album_of"], 40, K, skip=t["skip"]))
_add("chains", "chains_device", _scan, "S h_off X M skip",
     lambda ctx, t: ctx.chains(t["S"], t["h_off"], t["X"], K, "mahalanobis", t["M"], skip=t["skip"]))
_add("journeys_chain", "journeys_device", _scan, "Q X M qskip2",
     lambda ctx, t: ctx.journeys(t["Q"], None, t["X"], K, "mahalanobis", t["M"], skip=t["qskip2"], mode="chain", gate="up", feature=0))
_add("journeys_waypoint", "journeys_device", _scan, "Q B X M qskip2",
     lambda ctx, t: ctx.journeys(t["Q"], t["B"], t["X"], K, "mahalanobis", t["M"], skip=t["qskip2"], mode="waypoint"))
for _mode in ("chain", "nearest"):
    _add("radio_" + _mode, "radio_device", _scan, "Q X M rules from_rules qskip2",
         lambda ctx, t, mode=_mode: ctx.radio(t["Q"], t["X"], K, labels=t["rules"], windows=WINDOWS, limits=LIMITS,
                                               from_labels=t["from_rules"], mode=mode, metric="mahalanobis", M=t["M"], skip=t["qskip2"]))
_add("forest_scores", "forest_score_device", _scan, "X", lambda ctx, t: ctx.forest_scores(_forest(), t["X"], return_path_sum=True))
_add("forest_closest_to_songs", "forest_closest_to_songs_device", _scan, "X",
     lambda ctx, t: ctx.forest_closest_to_songs(_forest(), t["X"], return_scores=True))
_add("group_forest_knn", "group_forest_knn_device", _scan, "S h_off X skip",
     lambda ctx, t: ctx.group_forest_knn(t["S"], t["h_off"], t["X"], K, _forest_options(), skip=t["skip"]),
     options={"forest_group_nodes": 1})  # (a group beyond the budget is a batch of its own: three batches through gf_ev)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------------------
# the passes

@pytest.fixture(scope="module")
def bliss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import bliss_rs_amd

    return bliss_rs_amd


def _upload(inputs):
    import torch

    return {k: v if k.startswith("h_") else torch.from_numpy(v).cuda() for k, v in inputs.items()}


def _to_host(outs):
    return [np.ascontiguousarray(o if isinstance(o, np.ndarray) else o.detach().cpu().numpy()) for o in outs]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def _apply(ctx, options):
    for k, v in options.items():
        if k == "workspace_limit":
            ctx.set_workspace_limit(v)
        else:
            ctx.set_option(k, v)


@pytest.fixture(scope="module")
def sync(bliss):
    """-> sync(case): the synchronous pass of one case, run once per module on a fresh context: the decoy, the real inputs, and
    the real inputs again -- that third call is the timed one (the first two also pay for workspaces and code objects, which
    the ordered passes pay for in a warm-up call of their own).  It gives dict(real, again, decoy: host arrays; seconds; keep:
    the real runs' device outputs, referenced until the module ends so that no later run is handed a block that already holds
    the answer)"""
    import torch

    done = {}

    def run(case):
        if case.name in done:
            return done[case.name]
        ctx = bliss.Context(0)
        try:
            res = {"keep": []}
            for which in ("decoy", "real", "again"):
                inp = case.inputs(which == "decoy")
                t = inp if case.host else _upload(inp)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs = tuple(case.run(ctx, t))
                ctx.synchronize()
                res["seconds"] = time.perf_counter() - t0
                torch.cuda.synchronize()
                res[which] = _to_host(outs)
                if which != "decoy":
                    res["keep"].append((outs, t))
        finally:
            ctx.close()
        done[case.name] = res
        return res

    yield run
    done.clear()
    _FOREST.clear()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_synchronous_pass_tells_real_from_decoy(sync, case):
    """the expected values of every ordered pass, and the proof that a call on the decoy cannot pass for one on the real
    inputs: every output differs in at least one byte"""
    res = sync(case)
    assert len(res["real"]) == len(res["decoy"]) > 0
    for i, (r, d) in enumerate(zip(res["real"], res["decoy"])):
        assert r.size > 0, (case.name, "output", i, "is empty")
        assert _same(r, res["again"][i]), (case.name, "output", i, "two synchronous calls on the same inputs differ")
        assert not _same(r, d), (case.name, "output", i, "is the same for the decoy: the decoy tells nothing about it")


@pytest.fixture(scope="module")
def delay(sync):
    """-> a function that queues the calibrated delay on torch's current stream"""
    import torch

    slowest = max(CASES, key=lambda c: sync(c)["seconds"])
    longest = sync(slowest)["seconds"]
    target = max(0.020, 10.0 * longest)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if hasattr(torch.cuda, "_sleep"):
        def queue(amount):
            torch.cuda._sleep(int(amount))
        amount, unit = 1 << 20, "cycles"
    else:
        big = torch.randn(4096, 4096, device="cuda")

        def queue(amount):
            for _ in range(int(amount)):
                torch.mm(big, big)
        amount, unit = 4, "matrix products"
    measured = 0.0
    for _ in range(12):
        torch.cuda.synchronize()
        a.record()
        queue(amount)
        b.record()
        b.synchronize()
        measured = a.elapsed_time(b) / 1e3
        if measured >= target:
            break
        amount = int(amount * max(1.25, min(64.0, 1.25 * target / max(measured, 1e-6)))) + 1
    assert measured >= target, ("the delay could not be calibrated", amount, measured, target)
    times = sorted(((sync(c)["seconds"], c.name) for c in CASES), reverse=True)
    print("\nstream order: synchronous call times, ms: " + ", ".join(f"{n} {t * 1e3:.2f}" for t, n in times))
    print(f"stream order: delay {amount} {unit} = {measured * 1e3:.1f} ms on the device (floor 20 ms; 10 x the longest synchronous "
          f"call: {slowest.name}, {longest * 1e3:.2f} ms)")
    return lambda: queue(amount)


def _pairwise_raw(bliss, ctx, t, out):
    """blissgpu_pairwise_device as Context.pairwise calls it, WITHOUT the wait for the caller's stream"""
    from bliss_rs_amd import _ffi

    q, n = t["Q"].shape[0], t["X"].shape[0]
    _ffi.check(ctx._L.blissgpu_pairwise_device(ctx._h, C.c_void_p(t["Q"].data_ptr()), q, C.c_void_p(t["X"].data_ptr()), n, sc.D,
                                               _ffi.METRIC_MAHALANOBIS, C.c_void_p(t["M"].data_ptr()), C.c_void_p(out.data_ptr()),
                                               out.stride(0)))


@pytest.fixture(scope="module")
def side(bliss, sync, delay):
    """The side stream of the module: the first of at most 8 streams of torch's pool on which a call that does NOT wait for its
    producer is seen to lose the race (it computes on the decoy).  -> dict(stream, held, tried)"""
    import torch

    case = BY_NAME["pairwise"]
    want = sync(case)["decoy"][0]
    streams = [torch.cuda.Stream() for _ in range(8)]
    found = None
    for i, P in enumerate(streams):
        ctx = bliss.Context(0)
        try:
            real, bufs = _upload(case.inputs(False)), _upload(case.inputs(True))
            out = torch.empty(want.shape, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(P):
                delay()
                for k in bufs:
                    bufs[k].copy_(real[k], non_blocking=True)
            _pairwise_raw(bliss, ctx, bufs, out)
            ctx.synchronize()
            P.synchronize()
            torch.cuda.synchronize()
            if _same(_to_host([out])[0], want):
                found = i
        finally:
            ctx.close()
        if found is not None:
            break
    held = found is not None
    print(f"\nstream order: control {'held on stream %d of 8 (handle 0x%x)' % (found, streams[found].cuda_stream) if held else 'held on NONE of 8 streams'}")
    return dict(stream=streams[found or 0], other=torch.cuda.Stream(), held=held, tried=(found + 1) if held else 8)


def test_control_a_call_that_does_not_wait_computes_on_the_decoy(side):
    """The teeth of every ordered test: pairwise called through the raw C ABI without blissgpu_ctx_wait_stream, while its
    buffers still hold the (valid) decoy and the real inputs are queued behind the delay, must give the DECOY's result.  Where
    it never does, the runtime serialises the library's stream with every producer stream tried, and a missing wait could not
    show in the ordered tests (which then still cannot fail falsely)."""
    assert side["held"], ("on none of 8 producer streams did an unordered call lose the race against its inputs: the ordered "
                          "tests of this module cannot see a missing wait on this machine")


def _streams(mode, side):
    """-> (P: torch's current stream during the call, A: the stream the context adopts or None)"""
    import torch

    if mode == "own/default":
        return torch.cuda.default_stream(), None
    if mode == "own/side":
        return side["stream"], None
    if mode == "adopted":
        return side["stream"], side["stream"]
    return side["stream"], side["other"]


def _context(bliss, mode, side, options=None):
    import torch

    P, A = _streams(mode, side)
    ctx = bliss.Context(0)  # (created under the legacy default stream: on its own stream)
    try:
        if A is not None:
            with torch.cuda.stream(A):
                ctx.bind_current_stream()
            assert ctx._L.blissgpu_ctx_get_stream(ctx._h) == A.cuda_stream
            _apply(ctx, options or {})
    except BaseException:
        ctx.close()
        raise
    return ctx, P


def _prepare(case):
    """the device buffers of one ordered call, uploaded on the legacy default stream: `bufs` hold the decoy (host arguments:
    the real ones), `real` the inputs that arrive late"""
    real_host = case.inputs(False)
    if case.host:
        return dict(bufs=dict(case.inputs(True), **{k: v for k, v in real_host.items() if k.startswith("h_")}), real=real_host)
    bufs = _upload(case.inputs(True))
    bufs.update({k: v for k, v in real_host.items() if k.startswith("h_")})
    return dict(bufs=bufs, real=_upload(real_host))


def _warm(ctx, P, case, prep):
    """one call on the decoy, then everything settled: workspaces and code objects are in place, so that the ordered call costs
    what the timed call of the synchronous pass did"""
    import torch

    with torch.cuda.stream(P):
        case.run(ctx, prep["bufs"])
    torch.cuda.synchronize()
    ctx.synchronize()


def _late(ctx, P, delay, case, prep):
    """One ordered call of `case` on `ctx` with P as torch's current stream; nothing here waits for the device.  -> the clones
    of the outputs, queued on P straight behind the call (and what must stay alive until the streams are settled)"""
    import torch

    with torch.cuda.stream(P):
        delay()
        if case.host:
            t = prep["real"]  # (the wrapper's own upload is the producer)
        else:
            t = prep["bufs"]
            for k in t:
                if not k.startswith("h_"):
                    t[k].copy_(prep["real"][k], non_blocking=True)
        outs = tuple(case.run(ctx, t))
        snap = [o.copy() if isinstance(o, np.ndarray) else o.clone() for o in outs]
    return snap, outs


def _ordered(ctx, P, delay, case):
    prep = _prepare(case)
    _warm(ctx, P, case, prep)
    return _late(ctx, P, delay, case, prep) + (prep,)


def _settle(ctx, P):
    import torch

    P.synchronize()
    ctx.synchronize()
    torch.cuda.synchronize()


def _check(sync, case, snap, what):
    want = sync(case)["real"]
    got = _to_host(snap)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w), (case.name, what, "output", i, "read in stream order differs from the synchronous result",
                             "it is the DECOY's" if _same(g, sync(case)["decoy"][i]) else "")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_late_inputs_and_early_reads_are_ordered(bliss, sync, delay, side, case, mode):
    ctx, P = _context(bliss, mode, side, case.options)
    try:
        snap, *keep = _ordered(ctx, P, delay, case)
        _settle(ctx, P)
        if mode == "adopted" and case.name == "group_forest_knn":
            assert ctx.group_forest_stats()[2] >= 2, "the groups went through one batch: gf_ev was not exercised"
        if mode == "adopted" and case.name == "analyze":
            assert ctx.last_chunks() >= 2, "the songs went through one chunk"
        _check(sync, case, snap, mode)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------
# further checks

def test_own_stream_comes_back_after_set_stream_null(bliss, sync, delay, side):
    import torch

    ctx = bliss.Context(0)
    try:
        L, P = ctx._L, side["stream"]
        own = L.blissgpu_ctx_get_stream(ctx._h)
        assert own and own != P.cuda_stream
        with torch.cuda.stream(P):
            ctx.bind_current_stream()
        assert L.blissgpu_ctx_get_stream(ctx._h) == P.cuda_stream
        assert L.blissgpu_ctx_set_stream(ctx._h, None) == 0
        assert L.blissgpu_ctx_get_stream(ctx._h) == own
        snap, *keep = _ordered(ctx, P, delay, BY_NAME["knn"])
        _settle(ctx, P)
        _check(sync, BY_NAME["knn"], snap, "own stream restored")
    finally:
        ctx.close()


def _host_form_calls():
    """(case name, family, arguments of the host-pointer form, its outputs): the same calls as the table's, on host arrays"""
    c, s = _grid(False), _scan(False)
    win, lim = np.array(WINDOWS, np.uint32), np.array(LIMITS, np.uint32)
    o = lambda rows, dt: sc.out((rows, c.k), dt)  # noqa: E731
    i1, d1, i2, d2, i3, d3 = o(c.q, np.uint32), o(c.q, F32), o(c.G, np.uint32), o(c.G, F32), o(c.q, np.uint32), o(c.q, F32)
    return [("knn", "knn", [s["Q"], c.q, s["X"], c.n, sc.D, 2, s["M"], s["qskip"], c.k, i1, d1], [i1, d1]),
            ("group_knn", "group_knn", [s["S"], c.off, c.G, s["X"], c.n, sc.D, 2, s["M"], s["skip"], c.k, i2, d2], [i2, d2]),
            ("radio_chain", "radio", [s["Q"], c.q, s["X"], c.n, sc.D, 2, s["M"], s["rules"], s["from_rules"], 2, win, lim, s["qskip2"],
                                      c.k, 0, i3, d3], [i3, d3])]


def test_host_pointer_forms_return_finished_on_a_busy_adopted_stream(bliss, sync, delay, side):
    """the forms without a context argument run on the default context; bound to a caller's stream that is busy, they must
    still hand back finished host arrays"""
    import torch

    from bliss_rs_amd import _ffi

    lib, P = _ffi.lib(), side["stream"]
    dctx = bliss.Context.default(0)
    try:
        with torch.cuda.stream(P):
            dctx.bind_current_stream()
        for name, family, args, outs in _host_form_calls():
            with torch.cuda.stream(P):
                delay()
            sc._run(lib, "blissgpu_" + family, args)  # no synchronisation of ours behind it
            want = sync(BY_NAME[name])["real"]
            for i, (g, w) in enumerate(zip(outs, want)):
                assert np.array_equal(g.reshape(-1).view(np.uint8), w.reshape(-1).view(np.uint8)), (family, "output", i)
    finally:
        torch.cuda.synchronize()
        _ffi.check(lib.blissgpu_ctx_set_stream(dctx._h, None))
        dctx.close()


@pytest.mark.parametrize("mode", MODES)
def test_two_families_back_to_back_share_their_workspaces_in_order(bliss, sync, delay, side, mode):
    """knn and then chains (both use the pl_* workspaces) on one context, the second one's inputs late again, no host
    synchronisation between them"""
    ctx, P = _context(bliss, mode, side)
    try:
        first, second = BY_NAME["knn"], BY_NAME["chains"]
        prep1, prep2 = _prepare(first), _prepare(second)
        _warm(ctx, P, first, prep1)
        _warm(ctx, P, second, prep2)
        snap1, keep1 = _late(ctx, P, delay, first, prep1)
        snap2, keep2 = _late(ctx, P, delay, second, prep2)
        _settle(ctx, P)
        _check(sync, BY_NAME["knn"], snap1, mode + ", first call")
        _check(sync, BY_NAME["chains"], snap2, mode + ", second call")
    finally:
        ctx.close()
