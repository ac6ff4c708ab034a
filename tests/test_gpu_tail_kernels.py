"""Edge cases of the two kernels that fill the stretch between the FFT-8192 kernel and the chroma contraction.

beat_acf_kernel: a workgroup takes eight consecutive runs of one song and each of its wavefronts a quarter of the lags of all
eight, so the number of runs of a song decides how many workgroups it gets, how full the last one is, and which runs share a
wavefront.  tune_pass2_kernel: a workgroup takes a 64-frame tile, a wavefront every fourth frame of it, and all four count
into one LDS histogram.

Both are held to the checks of test_gpu_stage_frames.py (whose helpers this file imports): the oracle's chain replayed on the
device's own flux tap, bit for bit, and the reference's pitch histogram on the device's own spectrogram tap.  No tolerance
appears below.
"""
import numpy as np
import pytest

from test_gpu_parity import _run
from test_gpu_stage_frames import (BT_STEP, HOP, SR, _chain, _check_tuning, _clicks, _first_run_difference, _n_b, _same,
                                   bliss, stft_frames)  # noqa: F401  (bliss: the fixture)

ACF_RUNS = 8   # runs per workgroup of beat_acf_kernel (kernels_tempo.hip)

# tempo-frame counts n_b -> floor(n_b / 128) runs: 0, 1, 2, 3, 4, 5 runs (the frames of runs 0..3 start before the song), the
# counts around one full workgroup (7, 8, 9) and around two (15, 16, 17), each at its first and, for some, its last n_b
RUN_EDGE_NB = (127, 128, 255, 256, 383, 384, 512, 639, 640, 767, 896, 1024, 1151, 1152, 1920, 2048, 2176)
RUN_EDGE_RUNS = (0, 1, 1, 2, 2, 3, 4, 4, 5, 5, 7, 8, 8, 9, 15, 16, 17)


def _samples(n_b, extra=0):
    """the shortest song with n_b tempo frames (n_b = (n - 512) // 256 + 1), plus `extra` < 256 samples"""
    return 256 * (n_b - 1) + 512 + extra


def run_edge_songs():
    rng = np.random.default_rng(70707)
    songs = {}
    for k, n_b in enumerate(RUN_EDGE_NB):
        songs[f"nb_{n_b}"] = _clicks(rng, _samples(n_b, (0, 100, 255)[k % 3]), (120, 90, 160)[k % 3], floor=0.01)
        if k == len(RUN_EDGE_NB) // 2:   # in the middle of the batch
            songs["silence"] = np.zeros(_samples(600), np.float32)
            songs["too_short"] = _clicks(rng, 4000, 120, floor=0.01)
    return songs


def test_run_edge_songs_have_the_run_counts():
    songs = run_edge_songs()
    for n_b, runs in zip(RUN_EDGE_NB, RUN_EDGE_RUNS):
        got = _n_b(songs[f"nb_{n_b}"])
        assert got == n_b and (got // BT_STEP if got >= BT_STEP else 0) == runs, (n_b, got, runs)
    assert {0, 1, 2, 3, 4, 5, 8, 9} <= set(RUN_EDGE_RUNS)
    assert {r % ACF_RUNS for r in RUN_EDGE_RUNS} >= {0, 1, ACF_RUNS - 1} and max(RUN_EDGE_RUNS) > 2 * ACF_RUNS
    assert len(songs["too_short"]) < 8192 and not songs["silence"].any()
    names = list(songs)
    assert 0 < names.index("silence") < len(names) - 2 and names.index("too_short") == names.index("silence") + 1


def _tempo_taps(ctx, oracle, names, songs, what):
    """analyses the songs in the order of `names`; -> {song: (thresholded, run_bpm, run_count)}, each held to the replay of
    the oracle's chain on the song's own flux tap"""
    rows, status = _run(ctx, [songs[k] for k in names])
    n_bpms = ctx.last_tuning(len(names))[1]
    taps = {}
    for i, k in enumerate(names):
        if k == "too_short":
            assert status[i] != 0, (what, status[i])
            continue
        assert status[i] == 0, (what, k, status[i])
        x = songs[k]
        flux, thr, run_bpm, run_count = (ctx.debug_fetch(t, i) for t in ("flux", "thresholded", "run_bpm", "run_count"))
        assert len(flux) == len(thr) == _n_b(x), (what, k, len(flux), len(thr), _n_b(x))
        r_thr, r_bpms, r_value, runs = _chain(oracle.BPMDesc().run_onsets(x, flux))
        assert _same(thr, r_thr), f"{what} {k}: thresholded differs from the replay"
        bad = _first_run_difference(run_bpm, run_count, runs)
        assert bad is None, f"{what} {k}: {bad[1]}"
        assert len(run_bpm) == (_n_b(x) // BT_STEP if _n_b(x) >= BT_STEP else 0), (what, k, len(run_bpm))
        assert _same(rows[i, 0], np.float32(r_value)), (what, k, rows[i, 0], r_value)
        assert int(n_bpms[i]) == len(r_bpms), (what, k, n_bpms[i], len(r_bpms))
        taps[k] = (thr, run_bpm, run_count)
    return taps


@pytest.mark.gpu
def test_beat_acf_run_count_edges(bliss, oracle):
    """Songs with 0 .. 17 runs, digital silence and a too-short song in one ragged batch: thresholded, run_bpm and run_count
    equal the oracle's chain replayed on the device's flux, bit for bit; the same songs in reverse batch order (another
    context) give the same bits."""
    songs = run_edge_songs()
    names = list(songs)
    oracle.set_exp_via_double(True)
    try:
        ctx = bliss.Context(0)
        fwd = _tempo_taps(ctx, oracle, names, songs, "forward")
        ctx.close()
        assert len(fwd) == len(names) - 1
        assert not fwd["silence"][2].any() and len(fwd["silence"][1]) == 600 // BT_STEP
        assert sum(int(t[2].sum()) for t in fwd.values()) > 0, "no beat in the whole batch"
        c2 = bliss.Context(0)
        rev = _tempo_taps(c2, oracle, names[::-1], songs, "reversed")
        c2.close()
        for k in fwd:
            for tap, a, b in zip(("thresholded", "run_bpm", "run_count"), fwd[k], rev[k]):
                assert _same(a, b), f"{k}: tap {tap} depends on the batch order"
    finally:
        oracle.set_exp_via_double(False)


# ---------------------------------------------------------------------------------------------
# chroma-frame counts: the fewest an analysed song can have (8192 samples: 4 frames; a song is never shorter), a partial
# tile, exactly one tile, one tile + one frame, two tiles + one frame
HIST_EDGE_FRAMES = (4, 63, 64, 65, 129)


def hist_edge_songs(oracle):
    songs = {}
    for j, n_c in enumerate(HIST_EDGE_FRAMES):
        n = 8192 if n_c == 4 else n_c * HOP
        assert stft_frames(n) == n_c and stft_frames(n + 1) == (n_c + 1 if n_c != 4 else 4)
        t = np.arange(n) / SR
        tone = np.sin(2 * np.pi * 440.0 * 2.0 ** (0.31 / 12.0) * t)   # 31 cents sharp: every peak in one pitch bin
        noise = oracle.white_noise(9700 + j, n)
        songs[f"silent_{n_c}"] = np.zeros(n, np.float32)
        songs[f"tone_{n_c}"] = (0.3 * tone).astype(np.float32)
        songs[f"noise_{n_c}"] = noise
        songs[f"tone_noise_{n_c}"] = (0.3 * tone + 0.2 * noise).astype(np.float32)
    return songs


def _pitch_hists(ctx, oracle, names, songs, what):
    """_check_tuning's check of every song: the device's tuning is estimate_tuning of its own spectrogram tap, and no bin of
    the pitch_hist tap holds more peaks than the reference's histogram of that spectrogram.  (The tap is what pass 2 counted:
    the peaks above the median's coarse magnitude bins.  The peaks inside those bins are candidates, which tune_final_kernel
    adds to its own copy once it knows the exact median -- the tuning is the first argmax of that completed histogram, so a
    count lost or doubled by pass 2 shows in one of the two assertions.)"""
    _, status = _run(ctx, [songs[k] for k in names])
    assert (status == 0).all(), (what, status)
    tuning, _ = ctx.last_tuning(len(names))
    hists, _ = _check_tuning(ctx, oracle, names, tuning, lambda i: ctx.debug_fetch("spectrogram", i), what)
    assert len(hists) == len(names)
    for i, k in enumerate(names):
        if k.startswith("silent_"):
            assert not hists[k].any() and tuning[i] == 0.0, (what, k)
    return hists, tuning


@pytest.mark.gpu
def test_tune_pass2_histogram_edges(bliss, oracle):
    """4, 63, 64, 65 and 129 chroma frames x silence, a detuned tone, white noise and tone + noise, held to _check_tuning on
    the device's own spectrogram, and again with the candidate pool starved (the re-scan path): same tunings, same taps."""
    songs = hist_edge_songs(oracle)
    names = list(songs)
    ctx = bliss.Context(0)
    hists, tuning = _pitch_hists(ctx, oracle, names, songs, "default")
    for n_c in HIST_EDGE_FRAMES:
        for kind in ("tone", "tone_noise"):
            h = hists[f"{kind}_{n_c}"]
            print(f"{kind}, {n_c} frames: tuning {tuning[names.index(f'{kind}_{n_c}')]}, {int(h.sum())} peaks counted by pass 2, "
                  f"{int(h.max())} of them in bin {int(h.argmax())}")
        assert np.count_nonzero(hists[f"noise_{n_c}"]) > 50, n_c
    ctx.set_option("cand_budget", 0)
    h2, t2 = _pitch_hists(ctx, oracle, names, songs, "cand_budget=0")
    ctx.close()
    assert np.array_equal(t2.view(np.uint64), tuning.view(np.uint64))
    for k in names:
        assert np.array_equal(h2[k], hists[k]), k
