"""Host tests (no GPU) of the acoustic fingerprints (blissgpu_fingerprint_batch / blissgpu_fingerprint_match): the
contract of include/blissgpu.h replayed in float64 numpy (`replay`) and in integer numpy (`match_table` / `match_pick`), the fixed
test inputs, what the replay itself promises on them, the device-free entry points, the argument checks that come before the
device, the exact threshold and the union-find of playlist.fingerprint_duplicates, and the sidecar table of the library.
tests/test_gpu_fingerprint.py holds the device to these replays."""
import ctypes as C
import os
import re
import sqlite3
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, W, HOP, BANDS = 22050, 8192, 512, 33
OK, INVALID = 0, 2
K_ORACLE = 132.0  # tests/test_gpu_stage_frames.py: the per-bin bound of the STFT, |X^ - X| <= 2 K_ORACLE 2^-24 ||w x_f||
EDGES = np.array([111, 118, 125, 132, 140, 149, 157, 167, 177, 187, 198, 210, 222, 235, 249, 264, 280, 296, 314, 332, 352, 373, 395,
                  418, 443, 469, 497, 526, 557, 590, 625, 662, 702, 743], np.int64)
LEFT_OUT_CAP = 0.02  # at most this share of a song's bits may be too close to call


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


# ---- the contract, section 1, in float64 ----
def hann_f32():
    """the project's Hann table, as tests/test_gpu_stage_frames.py computes it: f32 arithmetic, the cosine rounded to f32"""
    k = np.arange(W, dtype=np.float32)
    arg = np.float32(2.0) * k * np.float32(np.pi) / np.float32(W)
    return (np.float32(0.5) - np.float32(0.5) * np.cos(arg.astype(np.float64)).astype(np.float32)).astype(np.float32)


def words_of(n):
    return 0 if n < W + HOP else (n - W) // HOP


class Replay:
    """words uint32 [frames - 1], E f64 [frames, 33], m f64 [frames - 1, 32], norms f64 [frames] = ||w . x_f||_2, and tau f64
    [frames - 1, 32]: the sum of the four energies' bounds of every m"""

    def __init__(self, words, E, m, norms, tau):
        self.words, self.E, self.m, self.norms, self.tau = words, E, m, norms, tau


def energy_bound(E, norms):
    """|E^ - E| <= 2 delta sqrt(n_b E) + n_b delta^2 with delta = 2 K_ORACLE 2^-24 ||w x_f||: from the per-bin bound
    |X^|^2 - |X|^2 <= delta (2 |X| + delta) and Cauchy-Schwarz over the band's n_b bins"""
    nb = np.diff(EDGES).astype(np.float64)[None, :]
    delta = (2.0 * K_ORACLE * 2.0 ** -24 * norms)[:, None]
    return 2.0 * delta * np.sqrt(nb * E) + nb * delta * delta


def replay(x) -> Replay:
    x = np.asarray(x, np.float32)
    nw = words_of(len(x))
    if nw == 0:
        return Replay(np.zeros(0, np.uint32), np.zeros((0, BANDS)), np.zeros((0, 32)), np.zeros(0), np.zeros((0, 32)))
    frames = nw + 1
    idx = HOP * np.arange(frames)[:, None] + np.arange(W)[None, :]
    xw = (x[idx] * hann_f32()[None, :]).astype(np.float32)  # the window product, rounded to f32
    norms = np.sqrt((xw.astype(np.float64) ** 2).sum(axis=1))
    X = np.fft.rfft(xw.astype(np.float64), axis=1)[:, EDGES[0]:EDGES[-1]]
    P = X.real * X.real + X.imag * X.imag
    E = np.stack([P[:, EDGES[b] - EDGES[0]:EDGES[b + 1] - EDGES[0]].sum(axis=1) for b in range(BANDS)], axis=1)
    m = (E[1:, :-1] - E[1:, 1:]) - (E[:-1, :-1] - E[:-1, 1:])
    words = ((m > 0).astype(np.uint64) << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)
    eb = energy_bound(E, norms)
    tau = eb[1:, :-1] + eb[1:, 1:] + eb[:-1, :-1] + eb[:-1, 1:]
    return Replay(words, E, m, norms, tau)


def left_out(r: Replay) -> float:
    """the share of a song's bits the bound cannot call: |m| <= tau"""
    return float((np.abs(r.m) <= r.tau).mean())


# ---- the test inputs: fixed in code ----
def noise():
    return (0.3 * np.random.default_rng(9200).standard_normal(4 * SR)).astype(np.float32)


def music(seed):
    """6 s, a note every 0.5 s: 110 * 2^(k / 12) Hz, k in [0, 36), 8 harmonics of amplitude uniform(0.2, 1) / h and random
    phase under clip(20 (t - a), 0, 1) exp(-3 (t - a)); 0.01 noise; peak 0.4"""
    rng = np.random.default_rng(seed)
    n = 6 * SR
    t = np.arange(n) / SR
    x = np.zeros(n)
    for note in range(12):
        a = 0.5 * note
        f0 = 110.0 * 2.0 ** (int(rng.integers(0, 36)) / 12.0)
        amp, phase = rng.uniform(0.2, 1.0, 8), rng.uniform(0.0, 2.0 * np.pi, 8)
        dt = np.maximum(t - a, 0.0)
        env = np.clip(20.0 * dt, 0.0, 1.0) * np.exp(-3.0 * dt)
        for h in range(1, 9):
            x += env * (amp[h - 1] / h) * np.sin(2.0 * np.pi * f0 * h * t + phase[h - 1])
    x += 0.01 * rng.standard_normal(n)
    return (0.4 * x / np.abs(x).max()).astype(np.float32)


COPY_CUT = 256 + 3 * 512  # three and a half hops


def degraded(x):
    """noise at 20 dB SNR, gain 0.7, the first three and a half hops cut, 16-bit quantisation"""
    x = np.asarray(x, np.float64)
    rng = np.random.default_rng(9201)
    y = x + np.sqrt((x * x).mean() / 100.0) * rng.standard_normal(len(x))
    y = (0.7 * y)[COPY_CUT:]
    return (np.clip(np.rint(y * 32768.0), -32768, 32767) / 32768.0).astype(np.float32)


def silence_noise_silence():
    mid = (0.3 * np.random.default_rng(9202).standard_normal(2 * SR)).astype(np.float32)
    return np.concatenate([np.zeros(SR, np.float32), mid, np.zeros(SR, np.float32)])


def tone_5k():
    """out of the bands: for the energy bound only (its bits are 26 % too close to call)"""
    t = np.arange(2 * SR) / SR
    return (0.5 * np.sin(2.0 * np.pi * 5000.0 * t) + 1e-3 * np.random.default_rng(9203).standard_normal(len(t))).astype(np.float32)


def run_length():
    text = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "internal.hpp")).read()
    return int(re.search(r"\bFP_RUN\s*=\s*(\d+)", text).group(1))


def length_cases():
    """the table of the issue, and frames on and either side of the band kernel's run length and of 64"""
    r = run_length()
    frames = sorted({r - 1, r, r + 1, 2 * r, 2 * r + 1, 63, 64, 65} - {0, 1})
    return [8703, 8704, 9215, 9216] + [W + HOP * (f - 1) for f in frames]


def length_song(n, seed=9300):
    return (0.3 * np.random.default_rng(seed + n).standard_normal(n)).astype(np.float32)


_REPLAYS = {}


def replay_of(name):
    """the replay of a named input, computed once"""
    if name not in _REPLAYS:
        x = {"noise": noise, "silence_noise_silence": silence_noise_silence, "tone_5k": tone_5k}.get(name)
        if x is not None:
            x = x()
        elif name == "copy":
            x = degraded(music(7))
        else:
            x = music(int(name.split("_")[1]))
        _REPLAYS[name] = (x, replay(x))
    return _REPLAYS[name]


# ---- the contract, section 2, in integers ----
_POP16 = np.array([bin(i).count("1") for i in range(65536)], np.uint8)


def popcount(v):
    v = np.asarray(v, np.uint32)
    return _POP16[v & 0xFFFF].astype(np.int64) + _POP16[v >> 16].astype(np.int64)


def match_table(a, b, max_offset):
    """{o: (errors, valid)} for every offset in [-max_offset, max_offset] with at least one position"""
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    la, lb = len(a), len(b)
    out = {}
    for o in range(max(-max_offset, -(la - 1)), min(max_offset, lb - 1) + 1):
        lo, hi = max(0, -o), min(la, lb - o)
        if hi <= lo:
            continue
        av, bv = a[lo:hi], b[lo + o:hi + o]
        valid = (av != 0) & (bv != 0)
        out[o] = (int(popcount(av ^ bv)[valid].sum()), int(valid.sum()))
    return out


def match_pick(table, max_offset, min_overlap):
    """-> (offset, errors, bits): the smallest errors / bits by exact comparison, ties to the smaller (|o|, o)"""
    best = None
    for o in sorted(table, key=lambda o: (abs(o), o)):
        e, v = table[o]
        if abs(o) > max_offset or v < min_overlap:
            continue
        if best is None or e * best[2] < best[1] * 32 * v:  # (strictly better only: an equal ratio keeps the earlier (|o|, o))
            best = (o, e, 32 * v)
    return best or (0, 0, 0)


def match_replay(a, b, max_offset, min_overlap):
    return match_pick(match_table(a, b, max_offset), max_offset, min_overlap)


# ---- tests ----
def test_band_table_is_its_formula(bliss):
    b = np.arange(BANDS + 1, dtype=np.float64)
    assert np.array_equal(np.rint(300.0 * (2000.0 / 300.0) ** (b / 33.0) * W / SR).astype(np.int64), EDGES)
    got = (C.c_uint32 * 34)()
    from bliss_rs_amd import _ffi

    assert _ffi.lib().blissgpu_fingerprint_bands(got) == OK
    assert list(got) == EDGES.tolist()
    assert _ffi.lib().blissgpu_fingerprint_bands(None) == INVALID
    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    assert " ".join(str(v) for v in EDGES) in " ".join(header.replace("*", " ").split())
    assert bliss.FINGERPRINT_VERSION == 1


def test_fingerprint_len_is_the_frame_formula(bliss):
    L = bliss._ffi.lib()
    for n in [0, 1, 8191, 8192] + length_cases() + [3 * 60 * SR, 2 ** 40]:
        frames = (n - W) // HOP + 1 if n >= W + HOP else 0
        assert L.blissgpu_fingerprint_len(n) == max(frames - 1, 0) == words_of(n) == bliss.fingerprint_len(n), n
    assert [words_of(n) for n in (8703, 8704, 9215, 9216)] == [0, 1, 1, 2]
    for n in length_cases():
        assert len(replay(length_song(n)).words) == L.blissgpu_fingerprint_len(n), n


def test_the_replay_calls_all_but_two_percent_of_the_bits():
    """the inputs of the GPU bits test must leave the bound room: the float64 replay alone stays well inside the cap"""
    for name in ("noise", "music_7", "music_8", "music_9"):
        share = left_out(replay_of(name)[1])
        print(f"{name}: {100 * share:.2f} % of the bits have |m| <= tau")
        assert share <= LEFT_OUT_CAP, (name, share)
    assert left_out(replay_of("tone_5k")[1]) > LEFT_OUT_CAP  # why the tone is no bits input


def test_silence_gives_word_zero_in_the_replay():
    x, r = replay_of("silence_noise_silence")
    silent = np.array([not x[HOP * f:HOP * f + W].any() for f in range(len(r.words) + 1)])
    assert silent.sum() >= 40 and (r.E[silent] == 0.0).all()
    assert (r.words[silent[:-1] & silent[1:]] == 0).all() and (r.words != 0).sum() > 90


def test_the_copy_matches_and_the_others_do_not_in_the_replay():
    """0.35 separates the degraded copy from another piece and from noise, with room on both sides"""
    a = replay_of("music_7")[1].words
    rates = {}
    for name in ("copy", "music_8", "noise"):
        o, e, bits = match_replay(a, replay_of(name)[1].words, 32, 64)
        assert bits > 0
        rates[name] = (e / bits, o)
    print(rates)
    assert rates["copy"][0] < 0.30 and rates["copy"][1] in (-4, -3)
    assert rates["music_8"][0] > 0.40 and rates["noise"][0] > 0.40


def test_match_replay_on_hand_made_fingerprints():
    a = np.tile(np.array([1, 2, 4, 8], np.uint32), 20)
    assert match_replay(a, a, 8, 16) == (0, 0, 2560)        # offsets 0, +-4, +-8 all have no error: the smallest |o| wins
    assert match_replay(a, a, 8, 81) == (0, 0, 0)           # 80 positions at the most
    s, lead = np.array([1, 2, 4, 8, 16], np.uint32), np.full(4, 32, np.uint32)
    assert match_replay(s, np.concatenate([lead, s]), 8, 5) == (4, 0, 160)   # a[t] = b[t + 4]
    assert match_replay(np.concatenate([lead, s]), s, 8, 5) == (-4, 0, 160)
    assert match_replay(np.concatenate([lead, s]), s, 3, 1) == (0, 10, 160)  # out of reach: two bits differ everywhere, the tie goes to 0
    z = np.array([0, 0, 5, 7, 0, 9, 0], np.uint32)
    assert match_replay(z, z, 0, 1) == (0, 0, 96) and match_replay(z, z, 0, 4) == (0, 0, 0)
    assert match_replay(np.array([3], np.uint32), np.array([1], np.uint32), 4096, 1) == (0, 1, 32)


def test_edges_are_exact_and_components_take_their_smallest_index(bliss):
    P = bliss.playlist
    # 7 / 20 of 2560 bits is 896: 895 errors is an edge, 896 is not (0.35 is taken as 7 / 20, not as the binary number beside it)
    assert P.fingerprint_edges([895, 896, 897, 0, 0], [2560, 2560, 2560, 0, 32], 0.35).tolist() == [True, False, False, False, True]
    assert P.fingerprint_edges([895, 896], [2560, 2560], Fraction(7, 20)).tolist() == [True, False]
    assert P.fingerprint_edges([1, 1], [2, 4], Fraction(10 ** 12 - 1, 2 * 10 ** 12)).tolist() == [False, True]  # (the object path)
    assert P.fingerprint_edges([0], [32], 0).tolist() == [False]
    with pytest.raises(ValueError):
        P.fingerprint_edges([0], [32], -0.1)
    pairs = [(5, 3), (3, 4), (1, 2), (6, 0), (2, 6), (7, 7)]
    edge = [True, True, True, True, False, True]
    assert P.labels_from_edges(8, pairs, edge).tolist() == [0, 1, 1, 3, 3, 3, 0, 7]
    assert P.labels_from_edges(8, pairs, [True] * 6).tolist() == [0, 0, 0, 3, 3, 3, 0, 7]
    assert [g.tolist() for g in P.groups_from_labels(P.labels_from_edges(8, pairs, edge))] == [[0, 6], [1, 2], [3, 4, 5]]


def test_python_layer_with_the_replay_in_the_device_call(bliss, monkeypatch):
    """playlist.fingerprint_match keeps pairs with an empty fingerprint from the device; fingerprint_duplicates labels by the match"""
    P = bliss.playlist
    sent = {}

    class Lib:
        @staticmethod
        def blissgpu_fingerprint_match(words, offsets, n, pairs, n_pairs, max_offset, min_overlap, o, e, b):
            off = np.ctypeslib.as_array(C.cast(offsets, C.POINTER(C.c_uint64)), (n + 1,)).astype(np.int64)
            w = np.ctypeslib.as_array(C.cast(words, C.POINTER(C.c_uint32)), (int(off[-1]),))
            pr = np.ctypeslib.as_array(C.cast(pairs, C.POINTER(C.c_uint32)), (n_pairs, 2))
            sent["pairs"] = pr.tolist()
            out = [np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), (n_pairs,)) for p, t in ((o, C.c_int32), (e, C.c_uint32), (b, C.c_uint32))]
            for k, (i, j) in enumerate(pr.tolist()):
                assert off[i + 1] > off[i] and off[j + 1] > off[j]
                out[0][k], out[1][k], out[2][k] = match_replay(w[off[i]:off[i + 1]], w[off[j]:off[j + 1]], max_offset, min_overlap)
            return OK

    monkeypatch.setattr(P._ffi, "lib", lambda: Lib)
    rng = np.random.default_rng(3)
    a = rng.integers(1, 2 ** 32, 300, dtype=np.uint64).astype(np.uint32)
    b = np.concatenate([rng.integers(1, 2 ** 32, 5, dtype=np.uint64).astype(np.uint32), a[:280] ^ np.uint32(1 << 7)])
    fps = [a, np.zeros(0, np.uint32), b, rng.integers(1, 2 ** 32, 300, dtype=np.uint64).astype(np.uint32)]
    o, e, bits = P.fingerprint_match(fps, [(0, 2), (0, 1), (1, 1), (0, 3)], 8, 64)
    assert sent["pairs"] == [[0, 2], [0, 3]]
    assert (o[0], e[0], bits[0]) == (5, 280, 32 * 280) and (o[1], e[1], bits[1]) == (0, 0, 0) and bits[2] == 0 and bits[3] > 0
    labels, pairs, o, e, bits = P.fingerprint_duplicates(fps, None, 0.35, 8, 64, return_match=True)
    assert pairs.tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]] and labels.tolist() == [0, 1, 0, 3]
    with pytest.raises(ValueError):
        P.fingerprint_match(fps, [(0, 4)])
    with pytest.raises(ValueError):
        P.fingerprint_duplicates([a] * 4097)
    for bad in (dict(max_offset=4097), dict(min_overlap=0)):
        with pytest.raises(ValueError):
            P.fingerprint_match(fps, [(0, 2)], **bad)


def test_arguments_are_checked_before_the_device(bliss):
    from bliss_rs_amd import _ffi

    L = _ffi.lib()
    words, off = np.arange(1, 11, dtype=np.uint32), np.array([0, 4, 4, 10], np.uint64)
    res = [np.zeros(2, t) for t in (np.int32, np.uint32, np.uint32)]

    def match(pairs, max_offset=4, min_overlap=1, n_songs=3, off=off):
        pairs = np.asarray(pairs, np.uint32)
        return L.blissgpu_fingerprint_match(words.ctypes.data, off.ctypes.data, n_songs, pairs.ctypes.data, len(pairs), max_offset, min_overlap,
                                            res[0].ctypes.data, res[1].ctypes.data, res[2].ctypes.data)

    assert match([(0, 2)], max_offset=4097) == INVALID and b"max_offset" in L.blissgpu_last_error()
    assert match([(0, 2)], min_overlap=0) == INVALID
    assert match([(0, 3)]) == INVALID and b"n_songs" in L.blissgpu_last_error()     # out of range
    assert match([(0, 1)]) == INVALID and b"without words" in L.blissgpu_last_error()  # an empty song
    assert match([(0, 2)], off=np.array([0, 4, 3, 10], np.uint64)) == INVALID
    assert match([(0, 1)], n_songs=2, off=np.array([0, 4, 2 ** 22 + 5], np.uint64)) == INVALID
    assert match(np.zeros((0, 2), np.uint32)) == OK                                  # no pair: nothing to do
    # the batch: word_offsets must be the caller's blissgpu_fingerprint_len sums; a batch of too-short songs needs no device
    pcm = np.zeros(8703 + 100, np.float32)
    so, st = np.array([0, 8703, 8803], np.uint64), np.full(2, -1, np.int32)
    en = np.ones((2, 33))

    def batch(wo):
        wo = np.asarray(wo, np.uint64)
        return L.blissgpu_fingerprint_batch(pcm.ctypes.data, so.ctypes.data, wo.ctypes.data, 2, words.ctypes.data, st.ctypes.data, en.ctypes.data)

    assert batch([0, 1, 1]) == INVALID and b"blissgpu_fingerprint_len" in L.blissgpu_last_error()
    assert batch([1, 1, 1]) == INVALID
    assert batch([0, 0, 0]) == OK and st.tolist() == [1, 1] and not en.any()
    out = bliss.fingerprint_batch([pcm[:8703], pcm[:0]])
    assert [len(w) for w in out] == [0, 0] and all(w.dtype == np.uint32 for w in out)
    with pytest.raises(bliss.ProviderError):
        bliss.fingerprint_batch([np.zeros((10, 2), np.float32)])
    with pytest.raises(bliss.ProviderError):
        bliss.fingerprint_batch([np.zeros(10, np.int16)])


def test_surface_profile_table_and_makefile(bliss):
    from bliss_rs_amd import _ffi

    for name in ("blissgpu_fingerprint_len", "blissgpu_fingerprint_bands", "blissgpu_fingerprint_batch", "blissgpu_fingerprint_match"):
        assert name in _ffi.SIGNATURES
    assert not [s for s in _ffi.SIGNATURES if "fingerprint" in s and s.endswith("_device")]
    for name in ("fingerprint_batch", "fingerprint_decoded_batch", "fingerprint_len"):
        assert hasattr(bliss, name)
    for name in ("fingerprint_match", "fingerprint_duplicates", "fingerprint_edges", "labels_from_edges"):
        assert hasattr(bliss.playlist, name)
    for name in ("store_fingerprints", "load_fingerprints", "fingerprint_duplicates"):
        assert hasattr(bliss.library, name)
    L = _ffi.lib()
    names = [L.blissgpu_profile_kernel_name(k).decode() for k in range(L.blissgpu_profile_kernel_count())]
    src = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "kernels_fingerprint.hip")).read()
    for name in ("fp_bands_kernel", "fp_bits_kernel", "fp_match_kernel", "fp_pick_kernel"):
        assert names.count(name) == 1 and re.search(r"\bvoid\s+%s\s*\(" % name, src), name
    assert names[-2:] == ["group_forest_scan_kernel", "journey_step_kernel"]  # (older ids keep their places)
    code = re.sub(r"//[^\n]*", "", src)
    assert "stft8192_kernel" not in code and "kernels_chroma" not in code and "radix16(" in code
    make = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "Makefile")).read()
    assert re.search(r"kernels_fingerprint\.o[^\n]*: EXTRA := \$\(NOCONTRACT\)", make)
    assert re.search(r"^OBJS\s*:=[^\n]*\bkernels_fingerprint\.o", make, flags=re.M)


def _library(bliss, tmp_path, songs):
    db = str(tmp_path / "library.db")
    bliss.library.create_schema(db)
    bliss.library.store_songs(db, songs)
    return db


def _song(bliss, path, feats, title=None, artist=None):
    return bliss.Song(path=path, title=title, artist=artist, analysis=bliss.Analysis(np.asarray(feats, np.float32), bliss.FeaturesVersion.LATEST))


def test_fingerprints_round_trip_through_the_sidecar_table(bliss, tmp_path):
    lib = bliss.library
    d = bliss.FeaturesVersion.LATEST.feature_count()
    db = _library(bliss, tmp_path, [_song(bliss, f"/m/{i}.flac", np.full(d, 0.1 * i)) for i in range(3)])
    assert lib.load_fingerprints(db) == {}  # no table yet, and none is made by reading
    conn = sqlite3.connect(db)
    assert conn.execute("select count(*) from sqlite_master where name = 'gpu_fingerprint'").fetchone()[0] == 0
    fp = {"/m/2.flac": np.array([1, 0xFFFFFFFF, 0, 0x80000000], np.uint32), "/m/0.flac": np.zeros(0, np.uint32)}
    lib.store_fingerprints(db, fp)
    back = lib.load_fingerprints(db)
    assert list(back) == ["/m/0.flac", "/m/2.flac"]
    assert all(back[p].dtype == np.uint32 and np.array_equal(back[p], fp[p]) for p in fp)
    lib.store_fingerprints(conn, {"/m/2.flac": np.array([7], np.uint32)})  # replaced, through an open connection
    assert lib.load_fingerprints(conn)["/m/2.flac"].tolist() == [7]
    cols = [(r[1], r[2].upper(), r[5]) for r in conn.execute("pragma table_info(gpu_fingerprint)")]
    assert cols == [("song_id", "INTEGER", 1), ("version", "INTEGER", 0), ("words", "BLOB", 0)]
    assert conn.execute("select version from gpu_fingerprint").fetchall() == [(1,), (1,)]
    conn.execute("update gpu_fingerprint set version = 2 where song_id = 1")  # another contract's words are not this one's
    assert list(lib.load_fingerprints(conn)) == ["/m/2.flac"]
    with pytest.raises(bliss.ProviderError):
        lib.store_fingerprints(conn, {"/m/none.flac": np.array([1], np.uint32)})
    conn.close()
    assert len(lib.load_songs(db)) == 3  # the crate's tables are as they were


def test_library_candidates_and_groups(bliss, tmp_path, monkeypatch):
    """library.fingerprint_duplicates: the k nearest by features and the same title and artist make the pairs; one match call"""
    lib, P = bliss.library, bliss.playlist
    d = bliss.FeaturesVersion.LATEST.feature_count()
    rng = np.random.default_rng(4)
    rec = [rng.integers(1, 2 ** 32, 400, dtype=np.uint64).astype(np.uint32) for _ in range(4)]
    at = [0.0, 0.01, 1.0, 1.01, 5.0, 9.0]  # songs 0, 1 and 2, 3 are feature neighbours; 4 and 5 are far from everything
    songs = [_song(bliss, f"/m/{i}.flac", np.full(d, v), *(("T", "A") if i in (1, 5) else (None, None))) for i, v in enumerate(at)]
    db = _library(bliss, tmp_path, songs)
    # 0 ~ 1 (a copy, shifted), 2 and 3 different recordings, 5 a copy of 1 that only the tags bring in, 4 has no fingerprint
    fps = {0: rec[0], 1: np.concatenate([rec[3][:3], rec[0][:390]]), 2: rec[1], 3: rec[2], 5: rec[0][2:]}
    lib.store_fingerprints(db, {f"/m/{i}.flac": w for i, w in fps.items()})

    def nearest(Q, X, k, metric="euclidean", m=None, skip=None):
        D = np.abs(np.asarray(Q)[:, None, 0].astype(np.float64) - np.asarray(X)[None, :, 0])
        D[np.arange(len(Q)), skip] = np.inf
        idx = np.argsort(D, axis=1, kind="stable")[:, :k]
        return idx, np.take_along_axis(D, idx, axis=1).astype(np.float32)

    calls = []

    def match(f, pairs, max_offset, min_overlap):
        calls.append(np.asarray(pairs).tolist())
        res = [match_replay(f[i], f[j], max_offset, min_overlap) for i, j in np.asarray(pairs).tolist()]
        return tuple(np.asarray([r[c] for r in res], t) for c, t in enumerate((np.int32, np.uint32, np.uint32)))

    monkeypatch.setattr(P, "nearest_order", nearest)
    monkeypatch.setattr(P, "fingerprint_match", match)
    groups = lib.fingerprint_duplicates(db, k=1, max_offset=8, min_overlap=64)
    assert calls == [[[0, 1], [1, 5], [2, 3]]]  # (5's nearest, 4, has no fingerprint)
    assert [[s.path for s in g] for g in groups] == [["/m/0.flac", "/m/1.flac", "/m/5.flac"]]
    assert lib.duplicate_songs.__doc__ and "fingerprint" not in lib.duplicate_songs.__doc__  # duplicate_songs is as it was
