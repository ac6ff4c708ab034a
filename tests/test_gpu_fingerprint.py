"""GPU tests (-m gpu) of the acoustic fingerprints (blissgpu_fingerprint_batch: fp_bands_kernel, fp_bits_kernel;
blissgpu_fingerprint_match: fp_match_kernel, fp_pick_kernel).  Expected values never come from the code under
test: the energies are held to the float64 replay of the contract (tests/test_fingerprint_host.py) within the bound the device
STFT is already held to, the bits wherever that bound can call them, and the match bit for bit to the integer replay."""
import numpy as np
import pytest

from test_fingerprint_host import (BANDS, HOP, LEFT_OUT_CAP, SR, W, energy_bound, length_cases, length_song, match_pick, match_table,
                                   replay, replay_of, run_length, words_of)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bliss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import bliss_rs_amd

    return bliss_rs_amd


NAMED = ("noise", "music_7", "music_8", "music_9", "copy", "silence_noise_silence", "tone_5k")


@pytest.fixture(scope="module")
def device(bliss):
    """{name: (words, energies)} of every named input and every length case, from ONE batch call"""
    names = list(NAMED) + [f"len_{n}" for n in length_cases()]
    songs = [replay_of(k)[0] for k in NAMED] + [length_song(n) for n in length_cases()]
    words, energies = bliss.fingerprint_batch(songs, return_energies=True)
    return dict(zip(names, zip(words, energies))), dict(zip(names, songs))


def test_energies_within_the_stft_bound(device):
    """|E^ - E| <= 2 delta sqrt(n_b E) + n_b delta^2, delta = 2 K_ORACLE 2^-24 ||w x_f||, for every frame and band; exactly 0.0
    for all-zero frames"""
    got, songs = device
    worst = 0.0
    for name, x in songs.items():
        r = replay_of(name)[1] if name in NAMED else replay(x)
        E = got[name][1]
        assert E.shape == r.E.shape == (len(r.words) + 1 if len(r.words) else 0, BANDS), name
        if not len(r.words):
            continue
        bound = energy_bound(r.E, r.norms)
        err = np.abs(E - r.E)
        zero = r.norms == 0.0
        assert (E[zero] == 0.0).all(), name
        ratio = float((err[~zero] / bound[~zero]).max())
        print(f"{name}: {E.shape[0]} frames, worst |E^ - E| / bound = {ratio:.4g}")
        assert (err <= bound).all(), (name, ratio)
        worst = max(worst, ratio)
    print(f"worst ratio over all inputs = {worst:.4g}")
    assert (replay_of("silence_noise_silence")[1].norms == 0.0).sum() >= 40  # (the all-zero frames were there to be checked)


def test_bits_wherever_the_bound_can_call_them(device):
    """the device bit is the replay's wherever |m| > tau; at most 2 % of a song's bits are left out"""
    got, _ = device
    for name in ("noise", "music_7", "music_8", "music_9"):
        r = replay_of(name)[1]
        words = got[name][0]
        assert words.dtype == np.uint32 and words.shape == r.words.shape
        sure = np.abs(r.m) > r.tau
        share = 1.0 - float(sure.mean())
        differ = ((words[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(bool) != (r.m > 0)
        print(f"{name}: {100 * share:.2f} % left out, {int(differ.sum())} bits differ from the replay, {int((differ & sure).sum())} of them callable")
        assert share <= LEFT_OUT_CAP, (name, share)
        assert not (differ & sure).any(), name


def test_silence_gives_word_zero(device):
    got, songs = device
    x = songs["silence_noise_silence"]
    words, E = got["silence_noise_silence"]
    silent = np.array([not x[HOP * f:HOP * f + W].any() for f in range(len(words) + 1)])
    assert silent.sum() >= 40 and (E[silent] == 0.0).all()
    assert (words[silent[:-1] & silent[1:]] == 0).all() and (words != 0).sum() > 90


def test_lengths_statuses_and_batches(bliss, device):
    """word counts and statuses at every length case; a batch gives the words of its songs one by one"""
    from bliss_rs_amd import _ffi

    got, songs = device
    L = _ffi.lib()
    for n in length_cases():
        assert len(got[f"len_{n}"][0]) == L.blissgpu_fingerprint_len(n) == words_of(n), n
    assert [len(got[f"len_{n}"][0]) for n in (8703, 8704, 9215, 9216)] == [0, 1, 1, 2]
    # the C entry point itself: statuses, and the too-short song's energy row
    r = run_length()
    pick = [8703, 8704, W + HOP * r, W + HOP * 64, 9216, 100]  # (frames r + 1 and 65)
    xs = [length_song(n) for n in pick]
    so = np.concatenate([[0], np.cumsum(pick)]).astype(np.uint64)
    wo = np.concatenate([[0], np.cumsum([words_of(n) for n in pick])]).astype(np.uint64)
    pcm = np.concatenate(xs)
    words, status = np.zeros(int(wo[-1]), np.uint32), np.full(len(pick), -1, np.int32)
    en = np.full((int(wo[-1]) + len(pick), BANDS), -1.0)
    _ffi.check(L.blissgpu_fingerprint_batch(pcm.ctypes.data, so.ctypes.data, wo.ctypes.data, len(pick), words.ctypes.data, status.ctypes.data,
                                            en.ctypes.data))
    assert status.tolist() == [1, 0, 0, 0, 0, 1]
    assert not en[0].any() and not en[-1].any() and (en[1:-1] > 0).all()
    # one by one, and two songs of different lengths in one batch: the same words and the same energies, bit for bit
    for k, n in enumerate(pick):
        one_w, one_e = bliss.fingerprint_batch([xs[k]], return_energies=True)
        assert np.array_equal(one_w[0], words[int(wo[k]):int(wo[k + 1])]), n
        if words_of(n):
            assert np.array_equal(one_e[0], en[int(wo[k]) + k:int(wo[k + 1]) + k + 1]), n
            assert np.array_equal(one_w[0], got[f"len_{n}"][0]), n
    two = bliss.fingerprint_batch([xs[3], xs[2]])
    assert np.array_equal(two[0], got[f"len_{pick[3]}"][0]) and np.array_equal(two[1], got[f"len_{pick[2]}"][0])
    for name in ("music_7", "noise"):
        assert np.array_equal(bliss.fingerprint_batch([songs[name]])[0], got[name][0]), name


def test_groups_of_a_batch_under_a_small_workspace_limit(bliss, device):
    """a batch larger than the budgets goes through the device in groups of consecutive songs (a quarter of the workspace limit
    of energies, half of it of PCM, one song at the least): the same words and energies, bit for bit, too-short songs between"""
    got, songs = device
    names = ["len_8703", "noise", "len_9216", "music_7", "len_8703", "len_40960", "silence_noise_silence", "len_10752", "len_8703"]
    ctx = bliss.Context.default()
    before = ctx.workspace_limit()
    ctx.set_workspace_limit(1 << 20)  # 256 KiB of energies (992 frames), 512 KiB of PCM (131 072 samples; music_7 has 132 300)
    try:
        words, energies = bliss.fingerprint_batch([songs[k] for k in names], return_energies=True)
    finally:
        ctx.set_workspace_limit(before)
    for k, w, e in zip(names, words, energies):
        assert np.array_equal(w, got[k][0]) and np.array_equal(e, got[k][1]), k
    assert bliss.Context.default().workspace_limit() == before


def test_decoded_batch_goes_through_the_device_conversion(bliss, device):
    """mono f32 at 22 050 Hz passes the conversion unchanged: the same words; int16 stereo at 44 100 Hz gives a fingerprint of the
    length the resampled song has"""
    got, songs = device
    x = songs["music_7"]
    assert np.array_equal(bliss.fingerprint_decoded_batch([x], SR)[0], got["music_7"][0])
    s16 = np.repeat((np.repeat(x, 2)[:, None] * 32767.0).astype(np.int16), 2, axis=1)  # 44.1 kHz by sample doubling, two channels
    out = bliss.fingerprint_decoded_batch([s16, x[:100]], [44100, SR])
    assert len(out[0]) == words_of(bliss.resampled_len(len(s16), 44100)) > 200 and len(out[1]) == 0


# ---- the match: bit for bit ----
def _random_fp(rng, n):
    w = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    w[w == 0] = 1
    return w


def _flip(rng, w, share=0.10):
    flips = (rng.random((len(w), 32)) < share).astype(np.uint64)
    return w ^ (flips << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)


PLANTED = (0, 1, -1, 255, -255, 256, -256, 257, -257)


@pytest.fixture(scope="module")
def match_set():
    """fingerprints, the pairs to match and {pair: match_table at the widest offset range}: the replay's tables, computed once"""
    rng = np.random.default_rng(9400)
    fps = [_random_fp(rng, n) for n in (1, 63, 64, 65, 255, 256, 257, 1000)]
    pairs = [(i, j) for i in range(8) for j in range(i, 8) if (i + j) % 2 == 0 or j == 7]  # (i, i) among them
    base = 7  # the fingerprint of 1000 words
    for o in PLANTED:  # b[t + o] = a[t] with 10 % of the bits flipped
        b = _random_fp(rng, 1000)
        lo, hi = max(0, -o), min(1000, 1000 - o)
        b[lo + o:hi + o] = _flip(rng, fps[base][lo:hi])
        b[b == 0] = 1
        fps.append(b)
        pairs += [(base, len(fps) - 1), (len(fps) - 1, base)]
    z = _random_fp(rng, 300)  # runs of zero words at the ends and in the middle
    z[:40], z[130:170], z[-25:] = 0, 0, 0
    zc = _flip(rng, np.concatenate([_random_fp(rng, 7), z[:280]]))
    zc[np.concatenate([np.zeros(7, bool), z[:280] == 0])] = 0
    zc[60:64] = 0
    fps += [z, zc, np.tile(np.array([1, 2, 4, 8], np.uint32), 20)]
    nz = len(fps) - 3
    pairs += [(nz, nz + 1), (nz + 1, nz), (nz, nz), (nz, 5), (nz + 2, nz + 2), (nz + 2, 2)]
    tables = {p: match_table(fps[p[0]], fps[p[1]], 4096) for p in set(pairs)}
    return fps, pairs, tables


def _expect(tables, pairs, max_offset, min_overlap):
    once = {p: match_pick(tables[p], max_offset, min_overlap) for p in {tuple(p) for p in pairs}}
    res = [once[tuple(p)] for p in pairs]
    return tuple(np.asarray([r[c] for r in res], t) for c, t in enumerate((np.int32, np.uint32, np.uint32)))


@pytest.mark.parametrize("max_offset", [0, 1, 300, 4096])
def test_match_is_the_replay_bit_for_bit(bliss, match_set, max_offset):
    fps, pairs, tables = match_set
    seen_none = seen_some = 0
    # 64 and 256: on the overlap two of the lengths allow, with one below and one above; 16 is the tie case's
    for min_overlap in (1, 16, 63, 64, 65, 255, 256, 257, 1001):
        got = bliss.playlist.fingerprint_match(fps, pairs, max_offset, min_overlap)
        want = _expect(tables, pairs, max_offset, min_overlap)
        for g, w, what in zip(got, want, ("offset", "errors", "bits")):
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, max_offset, min_overlap, np.flatnonzero(g != w)[:8])
        seen_none += int((want[2] == 0).sum())
        seen_some += int((want[2] > 0).sum())
    assert seen_none > 20 and seen_some > 100
    if max_offset >= 300:  # every planted copy is found where it was planted, at about the planted error rate
        got = bliss.playlist.fingerprint_match(fps, pairs, max_offset, 64)
        for k, o in enumerate(PLANTED):
            at = pairs.index((7, 8 + k))
            assert got[0][at] == o and got[0][at + 1] == -o and 0.07 < got[1][at] / got[2][at] < 0.13, o


def test_match_tie_case_and_a_long_pair_list(bliss, match_set):
    """a = b = tile([1, 2, 4, 8], 20): (0, 0, 2560); and more pairs than one launch takes, every output equal"""
    fps, pairs, tables = match_set
    tie = len(fps) - 1
    got = bliss.playlist.fingerprint_match(fps, [(tie, tie)], 8, 16)
    assert (int(got[0][0]), int(got[1][0]), int(got[2][0])) == (0, 0, 2560)
    many = (pairs * (70001 // len(pairs) + 1))[:70001]  # 65 536 pairs a launch: two launches
    got = bliss.playlist.fingerprint_match(fps, many, 1, 64)
    want = _expect(tables, many, 1, 64)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    from bliss_rs_amd import _ffi

    with pytest.raises(_ffi.BlissGpuError) as e:  # an empty song in a pair is an error status of the C entry point, not a fault
        words, off, pr = np.arange(1, 6, dtype=np.uint32), np.array([0, 5, 5], np.uint64), np.array([[0, 1]], np.uint32)
        out = [np.zeros(1, np.uint32) for _ in range(3)]
        _ffi.check(_ffi.lib().blissgpu_fingerprint_match(words.ctypes.data, off.ctypes.data, 2, pr.ctypes.data, 1, 4, 1, out[0].ctypes.data,
                                                         out[1].ctypes.data, out[2].ctypes.data))
    assert e.value.code == _ffi.ERR_INVALID


def test_duplicates_end_to_end(bliss, device):
    """music(7) and its degraded copy are one group at 0.35; music(8) and noise stay alone"""
    got, _ = device
    fps = [got[k][0] for k in ("music_7", "copy", "music_8", "noise")]
    labels, pairs, offset, errors, bits = bliss.playlist.fingerprint_duplicates(fps, None, 0.35, 32, 64, return_match=True)
    rate = {tuple(p): e / b for p, e, b in zip(pairs.tolist(), errors.tolist(), bits.tolist())}
    print({p: round(v, 4) for p, v in rate.items()}, offset.tolist())
    assert (bits > 0).all()
    assert rate[(0, 1)] < 0.35 and int(offset[pairs.tolist().index([0, 1])]) in (-4, -3)
    assert all(v > 0.35 for p, v in rate.items() if p != (0, 1))
    assert labels.tolist() == [0, 0, 2, 3]
    assert [g.tolist() for g in bliss.playlist.groups_from_labels(labels)] == [[0, 1]]
