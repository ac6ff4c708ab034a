"""Every analysis stage frame by frame, against float64 references.

The feature tests see a stage through a mean over thousands of frames, so one wrong frame moves a feature by 1/n of its
error.  Here every frame of every tap is held to a reference of its own:

  1. frame counts: the spectrogram has ceil_f32(n / 2205) rows like the reference's (src/utils.rs:29-32), including the
     all-zero row past the last window that the f32 ceiling adds for some songs of 2^26 samples and more; every other tap
     has the length of its formula
  2. the spectrogram against an independent float64 FFT (NumPy), per frame, within a bound calibrated on the oracle's
     own f32 FFT (the CPU tests below pin the NumPy reference and the calibration)
  3. the tuning stage, free of FFT rounding: the reference's estimate_tuning on the device's OWN spectrogram must give the
     device's tuning bit for bit, and the pitch_hist tap must be a sub-histogram of the reference's
  4. the FFT-512 series at every framing / tiling boundary length, frame by frame
  5. songs stay inside their bounds: odd offsets, NaN (or -32768) gaps, adjacent and overlapping songs give the same
     rows and taps, bit for bit, as the aligned zero-gap layout
  6. the tempo chain, free of FFT rounding: the oracle's peak picker, beat tracker and median replayed on the device's OWN
     flux tap must give the device's thresholded series, every run's bpm and beat count and the tempo feature bit for bit
     (the CPU tests of the section pin the replay, the per-run trace and what the song set reaches)
  7. features 1..9, free of FFT rounding: utils::mean and ndarray's std_axis (the oracle's mean / std) replayed on the device's
     OWN centroid, rolloff, flatness, energy256 and crossings256 taps must give the row's features 1..7 bit for bit and its
     features 8, 9 within the image of log10f's error bound (the CPU tests pin the oracle's Welford step on an exact fused
     multiply-add, the replay on the oracle's zcr / loudness, and what the song set reaches from its lengths alone)
  8. features 10..22, on the device's OWN interval tap: ChromaDesc::get_values / get_values_version_1 in plain NumPy must give
     features 10..21 bit for bit and feature 22 within one f32 ulp (double atan2), with songs on and off the 1.0 clamps of
     features 20 and 21 (the CPU tests pin the replay on the oracle and which songs sit on which clamp)

The CPU tests (no marker) run in the default `-m "not gpu"` pass; the GPU tests are marked one by one.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from conftest import assert_row_matches_oracle
from test_gpu_parity import _run, frame_and_tile_boundary_lengths

SR, W, HOP = 22050, 8192, 2205
EPS32 = 2.0 ** -24

# Per-frame spectrogram bound: max_k |spec - ref| <= K * 2^-24 * ||w . x_f||_2 against the float64 FFT below.
# K_ORACLE is the worst ratio of the oracle's own f32 STFT (radix-2) over spectro_songs(), measured on the CPU (131.96, on
# the tone on a bin centre: the error gathers at the peak bin, 1024 against ||w x|| = 19.6) and pinned by
# test_spectrogram_bound_calibration.  The device is held to 2 * K_ORACLE; on the MI355X it measured K_GPU (tone half a bin
# off centre; white noise and the boundary lengths 11 .. 15, where the oracle's ratio is 7 .. 12).  Scaling every magnitude
# below 1e-3 of its frame's maximum by 1 + 1e-3 -- what a wrong twiddle in a quiet band leaves -- gives 820 on the tone on
# a bin centre, and stays inside test_stage_taps_vs_oracle's 3e-6 * spec.max() and every feature bound.
K_ORACLE = 132.0
K_GPU = 133.9


# ---------------------------------------------------------------------------------------------
# the float64 reference of src/utils.rs:26-64, in plain NumPy (not built on the oracle)
# ---------------------------------------------------------------------------------------------
def stft_frames(n):
    """rows = (n as f32 / 2205 as f32).ceil() (src/utils.rs:29-32), the oracle's bo_stft_frames"""
    return int(np.ceil(np.float32(n) / np.float32(HOP)))


def hann_f32():
    """src/utils.rs:37-39: 0.5 - 0.5 * (2. * n as f32 * PI / W as f32).cos(), f32 arithmetic, the cosine rounded to f32"""
    k = np.arange(W, dtype=np.float32)
    arg = np.float32(2.0) * k * np.float32(np.pi) / np.float32(W)
    return (np.float32(0.5) - np.float32(0.5) * np.cos(arg.astype(np.float64)).astype(np.float32)).astype(np.float32)


def stft_f64(x, frames=None):
    """-> (spec [rows, 4097] float64, norms [rows] = ||w . x_f||_2, zero_window [rows] bool: the padded window is all zero).
    Rows past the last window (the f32 row count can exceed it by one) are zero, as the reference leaves them."""
    x = np.asarray(x, np.float32)
    n = len(x)
    rows = stft_frames(n)
    windows = n // HOP + 1
    padded = np.pad(x, W // 2, mode="reflect")
    w = hann_f32()
    frames = range(rows) if frames is None else frames
    frames = np.asarray(list(frames), np.int64)
    spec = np.zeros((len(frames), W // 2 + 1), np.float64)
    norms = np.zeros(len(frames), np.float64)
    zero = np.ones(len(frames), bool)
    for a in range(0, len(frames), 256):
        fr = frames[a:a + 256]
        ok = fr < windows
        idx = fr[ok, None] * HOP + np.arange(W)[None, :]
        seg = padded[idx]                                   # f32
        prod = (seg * w[None, :]).astype(np.float32)        # the windowed product in f32
        spec[a:a + 256][ok] = np.abs(np.fft.rfft(prod.astype(np.float64), axis=1))
        norms[a:a + 256][ok] = np.sqrt((prod.astype(np.float64) ** 2).sum(axis=1))
        zero[a:a + 256][ok] = ~(seg != 0).any(axis=1)
    return spec, norms, zero


def frame_ratios(got, ref, norms, zero, what):
    """Per-frame max_k |got - ref| / (2^-24 ||w . x_f||); a frame whose padded window is all zero must be exactly 0.0.
    -> (ratios, worst (frame, bin, |err|))"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    zr = np.flatnonzero(zero)
    if len(zr):
        bad = np.flatnonzero(got[zr].any(axis=1))
        assert not len(bad), f"{what}: frame {zr[bad[0]]} has an all-zero window but bin {int(np.flatnonzero(got[zr[bad[0]]])[0])} " \
                             f"= {got[zr[bad[0]]].max():.3g}"
    nz = norms > 0
    assert not err[~nz].any(), f"{what}: frame {int(np.flatnonzero(~nz & err.any(axis=1))[0])} has a zero product but nonzero magnitudes"
    ratios = np.zeros(len(ref))
    ratios[nz] = err[nz].max(axis=1) / (EPS32 * norms[nz])
    f = int(ratios.argmax())
    return ratios, (f, int(err[f].argmax()), float(err[f].max()))


def spectro_songs(oracle):
    """Section 2's songs: tones on and between bins, a 100 dB pair, a chirp, noise, DC, silence around noise, the minimum
    length, hop multiples and their neighbours, frame counts on and either side of the 16-frame workgroup and the 64-frame
    super-tile of the FFT-8192 kernel."""
    t = np.arange(5 * SR) / SR
    bin_hz = SR / W

    def tone(b, amp=0.5, tt=t):
        return amp * np.sin(2 * np.pi * b * bin_hz * tt + 0.3)

    songs = {
        "tone_bin_centre": tone(100.0).astype(np.float32),
        "tone_half_bin": tone(100.5).astype(np.float32),
        "tones_100dB_apart": (tone(300.0) + tone(1000.5, 0.5e-5)).astype(np.float32),
        "chirp": (0.5 * np.sin(2 * np.pi * (50.0 * t + 0.5 * (10000.0 - 50.0) / 5.0 * t * t))).astype(np.float32),
        "white_noise": oracle.white_noise(9100, 4 * SR),
        "dc": np.full(2 * SR, 0.25, np.float32),
        "silence_noise_silence": np.concatenate([np.zeros(3 * SR, np.float32), oracle.white_noise(9101, 2 * SR),
                                                 np.zeros(3 * SR, np.float32)]),
        "min_len_8192": oracle.white_noise(9102, 8192),
        "len_8193": oracle.white_noise(9103, 8193),
    }
    for d in (-1, 0, 1):
        songs[f"hop_x40{d:+d}"] = oracle.white_noise(9110 + d, HOP * 40 + d)
    for k, rows in enumerate((15, 16, 17, 63, 64, 65)):
        n = HOP * rows - 700
        assert stft_frames(n) == rows
        songs[f"rows_{rows}"] = oracle.white_noise(9120 + k, n)
    return songs


# ---------------------------------------------------------------------------------------------
# CPU: the NumPy reference against the oracle in f64 mode, and the calibration of K
# ---------------------------------------------------------------------------------------------
def test_numpy_stft_matches_f64_oracle(oracle):
    """The NumPy reference is the reference's STFT: against the oracle with its FFTs evaluated in f64 (then rounded to f32),
    every bin within one f32 ulp of itself plus 2 x 2^-24 ||w . x_f|| (measured: 1.54)."""
    oracle.set_fft_double(True)
    try:
        worst = 0.0
        for name, x in spectro_songs(oracle).items():
            ref, norms, zero = stft_f64(x)
            o = oracle.stft(x, W, HOP).T
            frame_ratios(o, ref, norms, zero, f"oracle f64, {name}")       # shapes and all-zero frames
            excess = np.abs(o - ref) - 2.0 ** -23 * ref - 2.0 * EPS32 * norms[:, None]
            f, k = np.unravel_index(int(excess.argmax()), excess.shape)
            assert excess[f, k] <= 0.0, f"{name}: frame {f} bin {k}: oracle_f64 {o[f, k]!r} numpy {ref[f, k]!r}"
            nz = norms > 0
            r = (np.abs(o - ref) - 2.0 ** -23 * ref)[nz].max(axis=1) / (EPS32 * norms[nz])
            worst = max(worst, float(r.max()))
        print(f"oracle (f64 FFT) vs NumPy: worst {worst:.3f} x 2^-24 ||w x|| beyond one ulp of the bin")
    finally:
        oracle.set_fft_double(False)


def test_spectrogram_bound_calibration(oracle):
    """K_ORACLE is what the oracle's own f32 STFT reaches over the same songs: the recorded constant must stay a tight upper
    bound (a looser K would let the device test pass a larger error)."""
    oracle.set_fft_double(False)
    k = 0.0
    for name, x in spectro_songs(oracle).items():
        ref, norms, zero = stft_f64(x)
        ratios, _ = frame_ratios(oracle.stft(x, W, HOP).T, ref, norms, zero, f"oracle f32, {name}")
        k = max(k, float(ratios.max()))
    print(f"K_oracle = {k:.3f} (recorded {K_ORACLE})")
    assert 0.9 * K_ORACLE <= k <= K_ORACLE, k


def test_stft_frame_count_formula():
    """The lengths of section 1 are the cases they claim to be (f32 ceiling against the exact one and the window count)."""
    for n in FRAME_COUNT_LENGTHS:
        rows, exact, windows = stft_frames(n), -(-n // HOP), n // HOP + 1
        kind = FRAME_COUNT_KIND[n]
        if kind == "extra_row":
            assert rows == windows + 1, n
        elif kind == "ceil_above_exact":
            assert rows == exact + 1 == windows, n
        elif kind == "ceil_below_exact":
            assert rows == exact - 1 and rows < windows, n
        else:
            assert rows == exact == windows, n


# ---------------------------------------------------------------------------------------------
# 1. frame counts, including the zero row past the last window
# ---------------------------------------------------------------------------------------------
FRAME_COUNT_KIND = {
    67_140_044: "extra_row",         # the first length where ceil_f32(n / 2205) exceeds the window count: 30 450 rows, 30 449 windows
    67_175_324: "extra_row",
    67_122_405: "ceil_above_exact",  # f32 ceiling one above the exact one, but within the window count
    16_784_461: "ceil_below_exact",  # f32 ceiling one below the exact one
    33_557_896: "ceil_below_exact",
    67_140_044 - 1_000: "control",
}
FRAME_COUNT_LENGTHS = list(FRAME_COUNT_KIND)


@pytest.fixture(scope="module")
def bliss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import bliss_rs_amd

    return bliss_rs_amd


def _tap_lengths_ok(ctx, i, n):
    n_t, n_b, n_e = (n - 512) // 128 + 1, (n - 512) // 256 + 1, -(-n // 256)
    for tap, want in (("centroid", n_t), ("rolloff", n_t), ("flatness", n_t), ("flux", n_b), ("thresholded", n_b),
                      ("energy256", n_e), ("crossings256", n_e), ("pitch_hist", 100)):
        got = len(ctx.debug_fetch_raw(tap, i))
        assert got == want, (n, tap, got, want)


@pytest.mark.gpu
def test_frame_counts_and_zero_rows(bliss, oracle):
    """The spectrogram keeps the reference's ceil_f32(n / 2205) rows; a row past the last window is exactly 0.0 and counts
    in the chroma means (kernels_finalize.hip divides by the row count), under every shape of the FFT-8192 kernel."""
    import torch

    lens = np.array(FRAME_COUNT_LENGTHS, np.uint64)
    offs = np.zeros(len(lens), np.uint64)
    offs[1:] = np.cumsum((lens + 63) // 64 * 64)[:-1]
    total = int(offs[-1] + lens[-1]) + 64
    c = bliss.Context(0)
    pcm = torch.empty(total, dtype=torch.float32, device="cuda")
    c.synth_white_noise(pcm, offs, lens, first_song_index=6100)
    rows, tails = {}, {}
    try:
        for shape in (0, 1, 2, 3):
            c.set_option("stft_shape", shape)
            out, status = c.analyze(pcm, offs, lens, 2)
            c.synchronize()
            assert (status.cpu().numpy() == 0).all()
            rows[shape] = out.cpu().numpy()
            tails[shape] = []
            for i, n in enumerate(FRAME_COUNT_LENGTHS):
                spec = c.debug_fetch("spectrogram", i)
                want, windows = stft_frames(n), n // HOP + 1
                assert spec.shape[0] == want, f"n = {n}, stft_shape {shape}: {spec.shape[0]} spectrogram rows, the reference has {want}"
                assert (spec[windows:] == 0.0).all(), (n, shape, "a row past the last window is not zero")
                assert spec[min(windows, want) - 1].max() > 0.0, (n, shape, "the last window's row is empty")
                tails[shape].append(spec[-3:].copy())
                del spec
                if shape == 0:
                    _tap_lengths_ok(c, i, n)
        for shape in (1, 2, 3):
            assert np.array_equal(rows[shape].view(np.uint32), rows[0].view(np.uint32)), shape
            for a, b in zip(tails[shape], tails[0]):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), shape
    finally:
        c.set_option("stft_shape", 0)
        del pcm
        c.close()
    # the rows against the oracle (six threads: the oracle's analysis of a 50-minute song takes ~17 s on one core)
    host = np.empty(total, np.float32)
    for i, (o, n) in enumerate(zip(offs, lens)):
        host[int(o):int(o) + int(n)] = oracle.white_noise(6100 + i, int(n))
    ref, rstatus = oracle.song_analyze_batch(host, offs, lens, 2, n_threads=len(lens))
    assert (rstatus == 0).all()
    for i, n in enumerate(FRAME_COUNT_LENGTHS):
        assert_row_matches_oracle(rows[0][i], ref[i], white_noise=True, what=f"n = {n}")


# ---------------------------------------------------------------------------------------------
# 2. the spectrogram against the float64 FFT, every frame
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_spectrogram_frames_vs_float64_fft(bliss, oracle):
    songs = spectro_songs(oracle)
    names = list(songs)
    ctx = bliss.Context(0)
    _, status = _run(ctx, [songs[k] for k in names])
    assert (status == 0).all()
    worst, report = 0.0, []
    for i, k in enumerate(names):
        x = songs[k]
        gspec = ctx.debug_fetch("spectrogram", i)
        ref, norms, zero = stft_f64(x)
        ratios, (f, b, e) = frame_ratios(gspec, ref, norms, zero, k)
        report.append(f"{k:24s} frames {len(ref):4d}  worst {ratios.max():.3f} (frame {f}, bin {b})")
        assert ratios.max() <= 2.0 * K_ORACLE, \
            f"{k}: frame {f} bin {b}: |gpu - float64 FFT| = {e:.3g} = {ratios.max():.3g} x 2^-24 ||w x_f|| > 2 K_oracle = {2 * K_ORACLE}"
        worst = max(worst, float(ratios.max()))
        if k == "silence_noise_silence":
            assert zero.sum() >= 10 and (gspec[zero] == 0.0).all()
    print("\n".join(report))
    print(f"K_gpu = {worst:.3f} (recorded {K_GPU}), K_oracle = {K_ORACLE}")
    ctx.close()


# ---------------------------------------------------------------------------------------------
# 3. the tuning stage on the device's own spectrogram
# ---------------------------------------------------------------------------------------------
def _reference_pitch_hist(oracle, spec_f64):
    """estimate_tuning's histogram (src/chroma.rs:361-391, oracle bo_estimate_tuning / bo_pitch_tuning) of the peaks at or
    above the Midpoint median, and the number of peaks with a positive pitch"""
    pit, mag = oracle.pip_track(SR, spec_f64.T, W)
    keep = pit > 0.0
    pit, mag = pit[keep], mag[keep]
    hist = np.zeros(100, np.int64)
    if len(pit) == 0:
        return hist, 0
    s = np.sort(mag)
    fi = 0.5 * (len(s) - 1)
    lo, hi = int(np.floor(fi)), int(np.ceil(fi))
    thr = s[lo] + (s[hi] - s[lo]) / 2.0
    p = pit[mag >= thr]
    r = np.fmod(12.0 * np.log2(p / (440.0 / 16.0)), 1.0)
    r = np.where(r >= 0.5, r - 1.0, r)
    q = (r + 0.5) / 0.01
    idx = np.minimum(np.where(q > 0.0, q, 0.0).astype(np.int64), 99)
    np.add.at(hist, idx, 1)
    return hist, len(pit)


def tuning_songs(oracle):
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
    import musical_check

    rng = np.random.default_rng(4242)
    songs = {"white_noise": oracle.white_noise(9200, 30 * SR)}
    for i in range(12):
        songs[f"musical_{i}"] = musical_check.make_song(rng)[0]
    t = np.arange(20 * SR) / SR
    for cents in (49.5, -49.5):   # residues at +-0.495: the histogram's wrap, bins 99 and 0
        f = [220.0 * 2.0 ** ((s + cents / 100.0) / 12.0) for s in (0, 4, 7, 12)]
        songs[f"chord_{cents:+.1f}_cents"] = (sum(np.sin(2 * np.pi * fr * t) for fr in f) * 0.2).astype(np.float32)
    songs["silence"] = np.zeros(5 * SR, np.float32)
    # one frame period repeated: every interior frame is the same frame, so the same peak magnitudes recur in every frame
    songs["repeated_frames"] = np.tile(oracle.white_noise(9201, HOP), 200)
    songs["single_tone"] = (0.3 * np.sin(2 * np.pi * 330.0 * np.arange(6 * SR) / SR)).astype(np.float32)
    return songs


def _check_tuning(ctx, oracle, names, tuning, spec_of, what):
    """-> ({song: pitch_hist} of the songs whose taps are in the last chunk, {peak count mod 2})"""
    from bliss_rs_amd import BlissGpuError

    hists, parities = {}, set()
    for i, k in enumerate(names):
        try:
            gspec = spec_of(i)
        except BlissGpuError:   # not in the last chunk
            continue
        spec64 = gspec.astype(np.float64)
        t_ref = oracle.estimate_tuning(SR, spec64.T, W, 0.01, 12)
        assert t_ref == tuning[i], f"{what} {k}: estimate_tuning on the device's spectrogram = {t_ref!r}, device tuning {tuning[i]!r}"
        ph = ctx.debug_fetch("pitch_hist", i).astype(np.int64)
        rh, n_peaks = _reference_pitch_hist(oracle, spec64)
        bad = np.flatnonzero(ph > rh)
        assert not len(bad), f"{what} {k}: pitch_hist bin {bad[0]} holds {ph[bad[0]]} peaks, the reference's histogram {rh[bad[0]]}"
        if k == "silence":
            assert tuning[i] == 0.0 and n_peaks == 0 and not ph.any()
        parities.add(n_peaks % 2)
        hists[k] = ph
    return hists, parities


@pytest.mark.gpu
def test_tuning_on_the_device_spectrogram(bliss, oracle):
    songs = tuning_songs(oracle)
    names = list(songs)
    ctx = bliss.Context(0)
    _, status = _run(ctx, [songs[k] for k in names])
    assert (status == 0).all()
    tuning, _ = ctx.last_tuning(len(names))
    hists, parities = _check_tuning(ctx, oracle, names, tuning, lambda i: ctx.debug_fetch("spectrogram", i), "default")
    assert len(hists) == len(names)
    assert parities == {0, 1}, "the songs must give both an odd and an even peak count (the two Midpoint median cases)"
    wrap = {int(np.argmax(hists[k])) for k in names if k.startswith("chord_")}
    print("tuning:", {k: float(t) for k, t in zip(names, tuning)}, "chord histogram modes:", wrap)
    assert wrap & {0, 99}, wrap
    for opt, val in (("cand_budget", 0), ("cand_budget", 1)):
        c2 = bliss.Context(0)
        c2.set_option(opt, val)
        _, st = _run(c2, [songs[k] for k in names])
        t2, _ = c2.last_tuning(len(names))
        assert (st == 0).all() and np.array_equal(t2.view(np.uint64), tuning.view(np.uint64)), (opt, val, t2, tuning)
        h2, _ = _check_tuning(c2, oracle, names, t2, lambda i: c2.debug_fetch("spectrogram", i), f"{opt}={val}")
        for k in names:
            assert np.array_equal(h2[k], hists[k]), (opt, val, k)
        c2.close()
    c3 = bliss.Context(0)
    c3.set_workspace_limit(24 << 20)
    _, st = _run(c3, [songs[k] for k in names])
    t3, _ = c3.last_tuning(len(names))
    assert c3.last_chunks() > 1
    assert (st == 0).all() and np.array_equal(t3.view(np.uint64), tuning.view(np.uint64)), (t3, tuning)
    h3, _ = _check_tuning(c3, oracle, names, t3, lambda i: c3.debug_fetch("spectrogram", i), "chunked")
    assert 0 < len(h3) < len(names)
    for k in h3:
        assert np.array_equal(h3[k], hists[k]), ("chunked", k)
    c3.close()
    ctx.close()


# ---------------------------------------------------------------------------------------------
# 4. the FFT-512 taps at every boundary length
# ---------------------------------------------------------------------------------------------
def boundary_songs(oracle):
    return [oracle.white_noise(700 + i, n) for i, n in enumerate(frame_and_tile_boundary_lengths())]


@pytest.mark.gpu
def test_fft512_taps_at_boundary_lengths(bliss, oracle):
    """Per-frame centroid / rolloff / flatness / flux / thresholded against the oracle's streaming descriptors, energy
    blocks against float64 NumPy and crossings exactly, under the bounds of test_stage_taps_vs_oracle (white noise: no
    rolloff flip at all)."""
    songs = boundary_songs(oracle)
    ctx = bliss.Context(0)
    _, status = _run(ctx, songs)
    assert (status == 0).all()
    for i, x in enumerate(songs):
        n = len(x)
        n_t, n_b, n_e = (n - 512) // 128 + 1, (n - 512) // 256 + 1, -(-n // 256)
        c, r, f = oracle.SpectralDesc().run(x).series()
        gc, gr, gf = (ctx.debug_fetch(k, i) for k in ("centroid", "rolloff", "flatness"))
        assert len(gc) == len(gr) == len(gf) == len(c) == n_t, (n, len(gc), len(c), n_t)
        t = int(np.abs(gc - c).argmax())
        assert abs(gc[t] - c[t]) < 2e-2, f"n = {n}: centroid frame {t}: {gc[t]} vs {c[t]}"
        flips = np.flatnonzero(np.abs(gr - r) > 1e-3)
        assert len(flips) == 0, f"n = {n}: rolloff frames {flips[:8].tolist()} differ (gpu {gr[flips[:4]]}, oracle {r[flips[:4]]})"
        t = int(np.abs(gf - f).argmax())
        assert abs(gf[t] - f[t]) < 3e-5, f"n = {n}: flatness frame {t}: {gf[t]} vs {f[t]}"
        onset, thr = oracle.BPMDesc().run(x).series()
        gflux, gthr = ctx.debug_fetch("flux", i), ctx.debug_fetch("thresholded", i)
        assert len(gflux) == len(gthr) == len(onset) == n_b, (n, len(gflux), len(onset), n_b)
        scale = 2e-6 * max(1.0, np.abs(onset).max())
        t = int(np.abs(gflux - onset).argmax())
        assert abs(gflux[t] - onset[t]) <= scale, f"n = {n}: flux frame {t}: {gflux[t]} vs {onset[t]}"
        t = int(np.abs(gthr - thr).argmax())
        assert abs(gthr[t] - thr[t]) <= scale, f"n = {n}: thresholded frame {t}: {gthr[t]} vs {thr[t]}"
        e, zc = ctx.debug_fetch("energy256", i), ctx.debug_fetch("crossings256", i)
        assert len(e) == len(zc) == n_e, (n, len(e), n_e)
        ref_e = np.add.reduceat(x.astype(np.float64) ** 2, np.arange(0, n, 256))
        bad = np.flatnonzero(~np.isclose(e, ref_e, rtol=1e-5, atol=1e-12))
        assert not len(bad), f"n = {n}: energy block {bad[0]} of {n_e}: {e[bad[0]]} vs {ref_e[bad[0]]}"
        assert int(zc.sum()) == oracle.number_crossings(x), n
        assert ctx.debug_fetch("spectrogram", i).shape[0] == stft_frames(n), n
    ctx.close()


# ---------------------------------------------------------------------------------------------
# 5. songs stay inside their bounds
# ---------------------------------------------------------------------------------------------
TAPS = ("centroid", "rolloff", "flatness", "flux", "thresholded", "run_bpm", "run_count", "spectrogram", "energy256",
        "crossings256", "pitch_hist")
GUARD = 8192


def _layout(songs, fill):
    """Songs of sections 2 and 4 packed with offsets = 1, 2, 3 (mod 4), gaps of `fill`, one adjacent pair, one song that
    overlaps the one before it, and GUARD samples of `fill` after the last song.  -> (buffer, offsets, lengths, songs as
    separate arrays in the same order) -- the overlapping song is the slice of its host."""
    rng = np.random.default_rng(5)
    dt = songs[0].dtype
    offs, lens, parts, pos = [], [], [], 1
    out_songs = []
    for i, x in enumerate(songs):
        if i > 0:
            if i == 5:
                gap = 0                                            # adjacent to the song before
            else:
                gap = int(rng.integers(1, 200)) * 4 + (i % 3) + 1 - (pos % 4)
                gap = gap if gap > 0 else gap + 4
            pos += gap
        assert pos % 64 != 0
        offs.append(pos)
        lens.append(len(x))
        out_songs.append(x)
        pos += len(x)
    # the overlapping song: a part of the longest one, starting inside it (a re-analysed section of a track)
    host = int(np.argmax(lens))
    start, length = offs[host] + 3001, lens[host] // 2
    offs.append(start)
    lens.append(length)
    buf = np.full(pos + GUARD, fill, dt)
    for o, x in zip(offs, out_songs):
        buf[o:o + len(x)] = x
    out_songs.append(buf[start:start + length].copy())
    assert {o % 4 for o in offs} >= {1, 2, 3} and all(o % 64 for o in offs)
    return buf, np.array(offs, np.uint64), np.array(lens, np.uint64), out_songs


def _layout_songs(oracle):
    return list(spectro_songs(oracle).values()) + boundary_songs(oracle)


def _taps(ctx, n_songs):
    return [[ctx.debug_fetch_raw(k, i) for k in TAPS] for i in range(n_songs)]


@pytest.mark.gpu
def test_songs_stay_inside_their_bounds(bliss, oracle):
    import torch

    from bliss_rs_amd import _ffi

    songs = _layout_songs(oracle)
    buf, offs, lens, separate = _layout(songs, np.float32(np.nan))
    ctx = bliss.Context(0)
    ref, st = _run(ctx, separate)
    assert (st == 0).all()
    ref_taps = _taps(ctx, len(separate))
    out, status = ctx.analyze(torch.from_numpy(buf).cuda(), offs, lens, 2)
    ctx.synchronize()
    got = out.cpu().numpy()
    assert (status.cpu().numpy() == 0).all()
    for i in range(len(separate)):
        assert np.array_equal(got[i].view(np.uint32), ref[i].view(np.uint32)), f"song {i} (offset {offs[i]}, length {lens[i]}): row differs"
    for i, taps in enumerate(_taps(ctx, len(separate))):
        for name, a, b in zip(TAPS, taps, ref_taps[i]):
            assert a.shape == b.shape and np.array_equal(a.view(a.dtype.str.replace("f", "u")), b.view(b.dtype.str.replace("f", "u"))), \
                f"song {i} (offset {offs[i]}, length {lens[i]}): tap {name} differs"
    ctx.close()

    L = _ffi.lib()
    # s16 through blissgpu_analyze_batch_s16, gaps of -32768: rows equal the aligned f32 run of the widened samples
    s16 = [np.clip(np.round(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16) for x in songs]
    buf16, offs16, lens16, sep16 = _layout(s16, np.int16(-32768))
    assert np.array_equal(offs16, offs) and np.array_equal(lens16, lens)
    ctx = bliss.Context(0)
    ref16, _ = _run(ctx, [(q.astype(np.float32) / np.float32(32768.0)).astype(np.float32) for q in sep16])
    ctx.close()
    n = len(offs)
    out16 = np.zeros((n, 23), np.float32)
    st16 = np.full(n, -1, np.int32)
    _ffi.check(L.blissgpu_analyze_batch_s16(C.c_void_p(buf16.ctypes.data), offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                            lens.ctypes.data_as(C.POINTER(C.c_uint64)), n, 2, C.c_void_p(out16.ctypes.data),
                                            st16.ctypes.data_as(C.POINTER(C.c_int32))))
    assert (st16 == 0).all()
    for i in range(n):
        assert np.array_equal(out16[i].view(np.uint32), ref16[i].view(np.uint32)), f"s16 song {i} (offset {offs[i]}): row differs"
    # f32 host entry point from pageable memory, large enough for the staging ring
    assert buf.nbytes >= 8 << 20
    dctx = bliss.Context.default(0)
    before = dctx.staged_bytes()
    outh = np.zeros((n, 23), np.float32)
    sth = np.full(n, -1, np.int32)
    _ffi.check(L.blissgpu_analyze_batch(buf.ctypes.data_as(C.POINTER(C.c_float)), offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        lens.ctypes.data_as(C.POINTER(C.c_uint64)), n, 2,
                                        outh.ctypes.data_as(C.POINTER(C.c_float)), sth.ctypes.data_as(C.POINTER(C.c_int32))))
    assert (sth == 0).all()
    assert dctx.staged_bytes() > before, "the batch did not go through the staging ring"
    for i in range(n):
        assert np.array_equal(outh[i].view(np.uint32), ref[i].view(np.uint32)), f"host f32 song {i} (offset {offs[i]}): row differs"


# ---------------------------------------------------------------------------------------------
# 6. the tempo chain on the device's own flux
# ---------------------------------------------------------------------------------------------
# Everything after SpecFlux (onset_kernel, beat_acf_kernel, beat_track_kernel) is written to round like the reference, so
# the oracle's chain fed the device's flux tap must reproduce the device's taps exactly.  No tolerance appears below: the
# only f32 operations whose rounding is not pinned by IEEE 754 are the three expf calls of checkstate, which the device
# evaluates as (float)exp((double)x); the oracle is switched to the same form (set_exp_via_double) and the reference's expf
# is measured beside it.
BT_STEP = 128
TRACE = ("rp", "gp", "bp", "timesig", "flagstep", "counter", "lastbeat")
TEMPO_BOUNDARY_NB = (127, 128, 129, 255, 256, 257, 511, 512, 513, 639, 640, 641)   # first run; padded frames 0..3; m >= 4
TEMPO_CHUNK_LIMIT = 64 << 20   # 0.2 MB of scratch per second of audio: the set (~ 760 s) is cut into three or more chunks


def _clicks(rng, n, bpm, amp=0.8, accent=0, floor=0.0):
    """n samples of 60-sample uniform noise bursts at `bpm`; with accent = k every beat but each k-th has half the amplitude;
    floor: amplitude of a uniform noise bed (0 = digital silence between the clicks)"""
    x = rng.uniform(-floor, floor, n) if floor else np.zeros(n)
    period = 60.0 / bpm * SR
    for k in range(int(n / period) + 1):
        a = int(round(k * period))
        m = min(60, n - a)
        if m <= 0:
            break
        x[a:a + m] = rng.uniform(-amp, amp, 60)[:m] * (0.5 if accent and k % accent else 1.0)
    return x.astype(np.float32)


def tempo_songs(oracle, golden_pcm):
    rng = np.random.default_rng(60606)
    n40 = 40 * SR
    songs = {}
    for bpm, accent in ((60, 0), (90, 3), (120, 4), (140, 0), (192, 3), (250, 4)):
        songs[f"click_{bpm}" + (f"_accent{accent}" if accent else "")] = _clicks(rng, n40, bpm, accent=accent)
    songs["change_120_to_90"] = np.concatenate([_clicks(rng, n40 // 2, 120), _clicks(rng, n40 // 2, 90)])
    songs["change_100_to_160"] = np.concatenate([_clicks(rng, n40 // 2, 100, accent=4), _clicks(rng, n40 // 2, 160, accent=4)])
    z = np.zeros(10 * SR, np.float32)
    songs["silence_clicks_silence"] = np.concatenate([z, _clicks(rng, 20 * SR, 120), z])
    loud = _clicks(rng, n40 // 2, 120)
    songs["loud_then_quiet"] = np.concatenate([loud, loud * np.float32(2e-6 / 0.8)])
    songs["noise"] = (0.3 * rng.standard_normal(n40)).astype(np.float32)
    # found by mutating the oracle (a period below 25 frames that is not noise; a phase comb that needs its last tooth; the
    # two thresholds of the lock): songs on which a changed constant of checkstate / the phase comb changes a run
    songs["click_211"] = _clicks(rng, n40, 211)
    r2 = np.random.default_rng(102)
    songs["medley"] = np.concatenate([_clicks(r2, int(r2.integers(6, 12)) * SR, float(r2.uniform(55, 230)),
                                              accent=int(r2.choice([0, 3, 4]))) for _ in range(4)])
    t = np.arange(n40)
    songs["am_noise"] = (0.15 * (1.1 + np.sin(2 * np.pi * t / (120 * 256.0))) * rng.uniform(-1, 1, n40)).astype(np.float32)
    songs["am_tone"] = (0.2 * (1.1 + np.sin(2 * np.pi * t / (90 * 256.0))) * np.sin(2 * np.pi * 1000.0 * t / SR)).astype(np.float32)
    songs["long_click_110"] = _clicks(rng, 104 * SR, 110, accent=4)      # 8957 tempo frames, 69 runs
    songs["short_no_run"] = _clicks(rng, 20000, 120, floor=0.01)         # 77 tempo frames
    songs["silence"] = np.zeros(10 * SR, np.float32)
    songs["dc"] = np.full(10 * SR, 0.25, np.float32)
    songs["white_noise"] = oracle.white_noise(9600, n40)
    songs["golden"] = golden_pcm
    for n_b in TEMPO_BOUNDARY_NB:
        for r in (0, 100, 255):
            songs[f"nb_{n_b}+{r}"] = _clicks(rng, 256 * (n_b - 1) + 512 + r, 120, floor=0.01)
    return songs


def _n_b(x):
    return (len(x) - 512) // 256 + 1


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(a.dtype.str.replace("f", "u"))


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _chain(d):
    """What a BPMDesc holds after a run: (thresholded, bpms, value, runs)"""
    return d.series()[1], d.bpms(), d.get_value(), d.runs()


def _same_runs(a, b):
    return a.dtype == b.dtype and all(_same(a[k], b[k]) for k in a.dtype.names)


@pytest.fixture(scope="module")
def tempo_set(oracle, golden_pcm):
    """(songs, {song: (flux, thresholded, bpms, value, runs)} of the oracle's own analysis), computed once"""
    oracle.set_exp_via_double(False)
    songs = tempo_songs(oracle, golden_pcm)
    own = {}
    for k, x in songs.items():
        d = oracle.BPMDesc().run(x)
        own[k] = (d.series()[0],) + _chain(d)
    return songs, own


def test_tempo_replay_reproduces_the_oracle(oracle, tempo_set):
    """Fed its own SpecFlux series, the replay entry point is the oracle: thresholded, bpms, value and the trace bit for bit."""
    songs, own = tempo_set
    for k, x in songs.items():
        flux, thr, bpms, value, runs = own[k]
        assert len(flux) == _n_b(x), k
        r_thr, r_bpms, r_value, r_runs = _chain(oracle.BPMDesc().run_onsets(x, flux))
        assert _same(r_thr, thr) and _same(r_bpms, bpms), k
        assert _same(np.float32(r_value), np.float32(value)), (k, r_value, value)
        assert _same_runs(r_runs, runs), k


def test_tempo_trace_is_consistent(tempo_set):
    """The trace's bpm and count columns are the bpms series run by run, and there is one record per 128 tempo frames."""
    songs, own = tempo_set
    for k, x in songs.items():
        _, _, bpms, value, runs = own[k]
        n_b = _n_b(x)
        assert len(runs) == ((n_b - BT_STEP) // BT_STEP + 1 if n_b >= BT_STEP else 0), (k, n_b, len(runs))
        count = runs.count.astype(np.int64)
        assert (count == runs.count).all() and int(count.sum()) == len(bpms), (k, count.sum(), len(bpms))
        assert _same(np.repeat(runs.bpm, count), bpms), k
        assert (value == -1.0) == (len(bpms) == 0), (k, value)


def _locks(runs):
    """Runs in which checkstate locked onto a new period (flagconst): the counter went from 1 straight to 0"""
    return np.flatnonzero((runs.counter[1:] == 0) & (runs.counter[:-1] == 1)) + 1


def test_tempo_song_set_reaches_the_chain(tempo_set):
    """Conditions on the oracle alone, so that the device test cannot pass on a degenerate set.

    `bp == 0` (a run_bpm of 0) is NOT among them: it cannot occur.  The Rayleigh period rp is either the interpolated
    position of a maximum at lag 1 .. 126 (at least 0.5: the last index attaining the maximum is taken, so the parabola's
    offset lies within half a lag) or rayparam = 43; the Gaussian-weighted period gp is taken from comb sums whose last
    entry is always (+-)0.0 (the comb loop stops at lag 126), so its maximum search never falls through to index 0 with
    gp == 0; and the doubling loop only raises bp.  A song in which no beat is ever found (silence: rp = 43 in every run)
    therefore has run_bpm = 60 / (256 * 43 / 22050) = 120.18 until the tracker locks (onto 43, then onto the last lag, 127:
    40.69), with a count of 0 in every run, and the value -1."""
    songs, own = tempo_set
    all_runs = np.concatenate([own[k][4] for k in songs if len(own[k][4])]).view(np.recarray)
    assert (all_runs.bp > 0).all() and (all_runs.bpm > 0).all()
    silent = own["silence"][4]
    assert (silent.bpm[silent.timesig == 0] == np.float32(60.0) / (np.float32(256.0 * 43.0) / np.float32(22050.0))).all()
    assert (silent.rp == 43.0).all() and (silent.nbeats > 1).all() and not silent.count.any()
    assert {0, 3, 4} <= set(all_runs.timesig.astype(int).tolist())
    two_locks, gaussian, doubled = [], [], []
    for k in songs:
        runs = own[k][4]
        if not len(runs):
            continue
        locks = _locks(runs)
        if len(locks) >= 2 and (runs.flagstep == 1).any():
            two_locks.append(k)
        lock = np.zeros(len(runs), bool)
        lock[locks] = True
        prev_lastbeat = np.concatenate([[np.float32(0.0)], runs.lastbeat[:-1]])
        if ((runs.timesig > 0) & ~lock & (prev_lastbeat < BT_STEP)).any():
            gaussian.append(k)
        source = np.where(runs.timesig > 0, runs.gp, runs.rp)   # what checkstate assigns to bp before the doubling loop
        assert ((source >= 25.0) <= (runs.bp == source)).all(), k
        if (source < 25.0).any():
            assert (runs.bp[source < 25.0] >= 25.0).all(), k
            doubled.append(k)
    print(f"two locks: {two_locks}\ngaussian phase weight: {len(gaussian)} songs, doubled period: {doubled}")
    assert "change_120_to_90" in two_locks or "change_100_to_160" in two_locks, two_locks
    assert gaussian and doubled
    assert len(own["silence"][4]) > 0 and len(own["silence"][2]) == 0 and own["silence"][3] == -1.0
    assert len(own["short_no_run"][4]) == 0 and own["short_no_run"][3] == -1.0 and _n_b(songs["short_no_run"]) < BT_STEP
    assert {len(own[k][2]) % 2 for k in songs if len(own[k][2])} == {0, 1}, "both Midpoint-median cases"
    # beats in windows that is_silence drops: the quiet half has beats in its runs' output but none recorded
    runs = own["loud_then_quiet"][4]
    half = len(runs) // 2
    assert runs.count[:half].sum() > 0 and (runs.nbeats[half + 4:-1] > 1).all() and runs.count[half + 4:].sum() == 0, runs
    assert 0.3 * runs.count[:half].sum() < len(own["loud_then_quiet"][2]) / 2 < runs.count[:half].sum()
    assert len(own["long_click_110"][4]) > 64 and len(songs["long_click_110"]) >= 100 * SR


def test_tempo_windows_are_clear_of_the_silence_threshold(tempo_set):
    """The device sums a window's level from its two energy256 blocks, the reference sequentially over 512 samples: the test
    must not depend on which side of -90 dB (1e-9) a rounding puts a window.  Every tempo window's level, in float64, is
    exactly 0 or a factor of 10 in power away from the threshold -- every window from 127 on, that is: is_silence is
    evaluated only where a beat of a finished run falls, and the first run happens at window 127 (the reference's
    recording fades in through the threshold in its windows 0 and 1, which nothing reads)."""
    songs, _ = tempo_set
    for k, x in songs.items():
        n_b = _n_b(x)
        e = np.add.reduceat(x.astype(np.float64) ** 2, np.arange(0, len(x), 256))
        level = (e[:n_b] + e[1:n_b + 1]) / 512.0
        bad = np.flatnonzero((level != 0.0) & (level >= 1e-10) & (level <= 1e-8))
        bad = bad[bad >= BT_STEP - 1]
        assert not len(bad), f"{k}: window {bad[0]} has level {level[bad[0]]:.3g}"


def test_tempo_set_is_clear_of_expf_rounding(oracle, tempo_set):
    """(float)exp((double)x) and expf(x) give the same chain on the oracle's own flux for every song of the set, so a
    difference between the two replays of the device test is about the device's flux, not about the set."""
    songs, own = tempo_set
    oracle.set_exp_via_double(True)
    try:
        for k, x in songs.items():
            flux, thr, bpms, value, runs = own[k]
            _, r_bpms, r_value, r_runs = _chain(oracle.BPMDesc().run_onsets(x, flux))
            assert _same_runs(r_runs, runs) and _same(r_bpms, bpms), k
            assert _same(np.float32(r_value), np.float32(value)), (k, r_value, value)
    finally:
        oracle.set_exp_via_double(False)


def _record(runs, m):
    return "{" + ", ".join(f"{f} {runs[f][m]!r}" for f in ("bpm",) + TRACE + ("nbeats", "count")) + "}"


def _first_run_difference(run_bpm, run_count, runs):
    """-> None, or (run, description with the oracle's trace of that run and the one before)"""
    n = min(len(run_bpm), len(runs))
    diff = (_bits(run_bpm[:n]) != _bits(runs.bpm[:n])) | (run_count[:n] != runs.count[:n].astype(np.int64))
    if len(run_bpm) == len(run_count) == len(runs) and not diff.any():
        return None
    if not diff.any():
        return n, f"{len(run_bpm)} / {len(run_count)} device runs, the replay has {len(runs)}"
    m = int(np.flatnonzero(diff)[0])
    text = f"first differing run {m}: device bpm {run_bpm[m]!r} count {run_count[m]}, replay {_record(runs, m)}"
    if m > 0:
        text += f"; run {m - 1}: device bpm {run_bpm[m - 1]!r} count {run_count[m - 1]}, replay {_record(runs, m - 1)}"
    return m, text


def _check_tempo_chain(ctx, oracle, names, songs, rows, n_bpms, what):
    """Replays the oracle's chain on the flux tap of every song whose taps can be fetched (those of the last chunk) and
    demands the device's taps, feature 0 and bpm count bit for bit.  -> {song: (flux, thresholded, run_bpm, run_count, runs)}"""
    from bliss_rs_amd import BlissGpuError

    checked = {}
    for i, k in enumerate(names):
        try:
            flux = ctx.debug_fetch("flux", i)
        except BlissGpuError:   # not in the last chunk
            continue
        x = songs[k]
        thr, run_bpm, run_count = (ctx.debug_fetch(t, i) for t in ("thresholded", "run_bpm", "run_count"))
        assert len(flux) == len(thr) == _n_b(x), (what, k, len(flux), len(thr), _n_b(x))
        r_thr, r_bpms, r_value, runs = _chain(oracle.BPMDesc().run_onsets(x, flux))
        if not _same(thr, r_thr):
            t = int(np.flatnonzero(_bits(thr) != _bits(r_thr))[0])
            raise AssertionError(f"{what} {k}: thresholded frame {t} (run {max(0, t - 127) // 128}): device {thr[t]!r}, replay {r_thr[t]!r}")
        bad = _first_run_difference(run_bpm, run_count, runs)
        assert bad is None, f"{what} {k}: {bad[1]}"
        assert _same(rows[i, 0], np.float32(r_value)), \
            f"{what} {k}: tempo feature {rows[i, 0]!r}, replay {np.float32(r_value)!r} over {len(r_bpms)} bpms (taps equal)"
        assert int(n_bpms[i]) == len(r_bpms), f"{what} {k}: n_bpms {n_bpms[i]}, replay {len(r_bpms)}"
        checked[k] = (flux, thr, run_bpm, run_count, runs)
    return checked


def _analyze_tempo_set(ctx, names, songs):
    rows, status = _run(ctx, [songs[k] for k in names])
    assert (status == 0).all(), status
    return rows, ctx.last_tuning(len(names))[1]


@pytest.mark.gpu
def test_tempo_chain_on_the_device_flux(bliss, oracle, tempo_set):
    """Every song, every run, bit for bit, with the oracle's checkstate exponentials in the device's form; then the
    reference's expf: the songs whose replay leaves the device are printed (expected: none) and held to TEMPO_TOL."""
    from conftest import TEMPO_TOL

    songs, _ = tempo_set
    names = list(songs)
    ctx = bliss.Context(0)
    try:
        rows, n_bpms = _analyze_tempo_set(ctx, names, songs)
        oracle.set_exp_via_double(True)
        checked = _check_tempo_chain(ctx, oracle, names, songs, rows, n_bpms, "default")
        assert len(checked) == len(names) and ctx.last_chunks() == 1
        n_runs = sum(len(v[4]) for v in checked.values())
        print(f"tempo chain on the device's flux: {len(checked)} songs, {n_runs} runs, {int(n_bpms.sum())} beats, all bit for bit")
        oracle.set_exp_via_double(False)
        differing = []
        for i, k in enumerate(names):
            flux, thr, run_bpm, run_count, _ = checked[k]
            r_thr, r_bpms, r_value, runs = _chain(oracle.BPMDesc().run_onsets(songs[k], flux))
            assert _same(thr, r_thr), k   # (no exponential before the peak picker)
            bad = _first_run_difference(run_bpm, run_count, runs)
            if bad is not None or not _same(rows[i, 0], np.float32(r_value)):
                differing.append(k)
                print(f"reference expf, {k}: {bad[1] if bad else 'runs equal'}; feature {rows[i, 0]!r} vs {np.float32(r_value)!r}")
                assert abs(float(rows[i, 0]) - r_value) <= TEMPO_TOL, (k, rows[i, 0], r_value)
        print(f"reference expf: {len(differing)} of {len(names)} songs differ from the device: {differing}")
    finally:
        oracle.set_exp_via_double(False)
        ctx.close()


@pytest.mark.gpu
def test_tempo_chain_options_do_not_change_a_bit(bliss, oracle, tempo_set):
    """The same batch with SpecFlux in the reference's bin order, with the beat tracker forced before / after the FFT-8192
    kernel and with the batch cut into chunks: each run's taps equal the replay of its OWN flux tap, and (flux_order aside,
    which may round the flux differently) equal the default run's taps."""
    songs, _ = tempo_set
    names = list(songs)
    oracle.set_exp_via_double(True)
    try:
        ctx = bliss.Context(0)
        rows, n_bpms = _analyze_tempo_set(ctx, names, songs)
        base = _check_tempo_chain(ctx, oracle, names, songs, rows, n_bpms, "default")
        ctx.close()
        assert len(base) == len(names)
        for what, option, value in (("flux_order=1", "flux_order", 1), ("tail_mode=0", "tail_mode", 0),
                                    ("tail_mode=1", "tail_mode", 1), ("chunked", None, None)):
            c = bliss.Context(0)
            if option:
                c.set_option(option, value)
            else:
                c.set_workspace_limit(TEMPO_CHUNK_LIMIT)
            r2, nb2 = _analyze_tempo_set(c, names, songs)
            got = _check_tempo_chain(c, oracle, names, songs, r2, nb2, what)
            if option:
                assert len(got) == len(names) and c.last_chunks() == 1, (what, len(got), c.last_chunks())
            else:
                assert c.last_chunks() > 1 and 0 < len(got) < len(names), (c.last_chunks(), len(got))
            if option != "flux_order":
                assert _same(r2[:, 0], rows[:, 0]) and np.array_equal(nb2, n_bpms), what
                for k, taps in got.items():
                    for tap, a, b in zip(("flux", "thresholded", "run_bpm", "run_count"), taps, base[k]):
                        assert _same(a, b), f"{what} {k}: tap {tap} differs from the default run's"
            print(f"{what}: {len(got)} songs checked, {c.last_chunks()} chunk(s)")
            c.close()
    finally:
        oracle.set_exp_via_double(False)


# ---------------------------------------------------------------------------------------------
# 7. features 1..9 on the device's own series
# ---------------------------------------------------------------------------------------------
# summary_kernel (kernels_finalize.hip) is sequential f32 arithmetic in the reference's order: fed the device's taps, the
# oracle's mean / std and the f32 expressions below must reproduce features 1..7 exactly.  Features 8 and 9 end in log10f,
# whose rounding IEEE 754 does not fix.  No header or document of the ROCm installation states an error bound for the device
# library's log10f (the HIP headers hand it to __builtin_log10f without a word on accuracy), so the bound is LOG10F_ULP = 2
# ulp of the logarithm.  Its image in the feature is taken exactly, not by a derivative: every f32 within 2 ulp of the true
# log10(v) lies between the two f32 values `lo` and `hi` below, every later step (x 10, + 90, x 2, / 90, - 1, each rounded to
# f32) is monotone, so the feature lies between the f32 features of `lo` and `hi`; one more f32 ulp is allowed on either side
# for the rounding of the result.  (A derivative would be unsound here: 10 log10(v) + 90 has an ulp of 7.6e-6 near 85, which the
# later steps turn into 1.7e-7 = 3 ulp of a feature near 0.9, however small the error of the logarithm that tipped it.)
F32 = np.float32
LOUD_W = 1024
LOG10F_ULP = 2
SUMMARY_SERIES = (("centroid", 2, 11025.0), ("rolloff", 4, 11025.0), ("flatness", 6, 1.0))   # tap, feature of the mean, max
SUMMARY_RESIDUES = (0, 1, 255, 256, 257, 511, 768, 1023)
SUMMARY_SHORT = {7: 0, 49: 1, 96: 100, 139: 8191}   # position in the batch: length of a too-short song


def _normalize(v, mn, mx):
    """Normalize (src/utils.rs: 2. * (value - min) / (max - min) - 1.) in f32 scalars, in that order of operations"""
    v, mn, mx = F32(v), F32(mn), F32(mx)
    return F32(F32(F32(2.0) * F32(v - mn)) / F32(mx - mn)) - F32(1.0)


def _ord32(a):
    """f32 -> integers in which neighbouring floats differ by one, so that a difference is a distance in ulp"""
    i = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _ulps(a, b):
    return np.abs(_ord32(a) - _ord32(b))


def _same_f32(a, b):
    """bit for bit"""
    a, b = F32(a), F32(b)
    return a.view(np.uint32) == b.view(np.uint32)


def _round_to_f32(q):
    """An exact rational rounded ONCE to f32, to nearest, ties to even"""
    if q == 0:
        return F32(0.0)
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if a < Fraction(2) ** e:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    m = a / quantum
    n = m.numerator // m.denominator
    r = m - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n & 1):
        n += 1
    return F32(float(n * quantum) * (-1.0 if q < 0 else 1.0))   # n <= 2^24 times a power of two: exact in a double


def welford_std(x, fused):
    """ndarray's std_axis(Axis(0), 0.) on a 1-D f32 array, restated apart from the oracle.  fused: sum_sq = fma(x - mean,
    delta, sum_sq) from exact rationals rounded once (math.fma is a float64 operation: rounding its result to f32 would round
    twice); not fused: the product rounded to f32, then the sum"""
    mean, sum_sq = F32(0.0), F32(0.0)
    for i, v in enumerate(np.asarray(x, F32)):
        delta = F32(v - mean)
        mean = F32(mean + F32(delta / F32(i + 1)))
        d2 = F32(v - mean)
        if fused:
            sum_sq = _round_to_f32(Fraction(float(d2)) * Fraction(float(delta)) + Fraction(float(sum_sq)))
        else:
            sum_sq = F32(F32(d2 * delta) + sum_sq)
    return F32(np.sqrt(F32(sum_sq / F32(F32(len(x)) - F32(0.0)))))


def replay_timbral(oracle, series, mx):
    """features (2, 3), (4, 5) or (6, 7) from one per-frame series (src/timbral.rs:54-63, 78-87, 108-117)"""
    return _normalize(F32(oracle.mean(series)), 0.0, mx), _normalize(F32(oracle.std(series)), 0.0, mx)


def replay_zcr(crossings256, n):
    """feature 1 (src/timbral.rs:250-252) from the crossings of the 256-sample blocks"""
    return _normalize(F32(int(np.sum(crossings256, dtype=np.int64))) / F32(int(n)), 0.0, 1.0)


def replay_levels(e256, n):
    """level of every 1024-sample chunk (src/misc.rs:12-18, 44-48): its up to four block energies added in order in f32 from
    0.0f, over the chunk's true length"""
    assert len(e256) == -(-n // 256), (len(e256), n)
    n_l = -(-n // LOUD_W)
    e = np.zeros((n_l, 4), F32)
    e.reshape(-1)[:len(e256)] = e256          # a missing block adds +0.0f to a non-negative sum: no change
    en = F32(0.0) + e[:, 0]
    for k in (1, 2, 3):
        en = (en + e[:, k]).astype(F32)
    lens = np.full(n_l, LOUD_W, np.int64)
    lens[-1] = n - LOUD_W * (n_l - 1)
    return (en / lens.astype(F32)).astype(F32)


def _f32_at_or_below(v):
    f = F32(v)
    return f if float(f) <= v else np.nextafter(f, F32(-np.inf))


def _f32_at_or_above(v):
    f = F32(v)
    return f if float(f) >= v else np.nextafter(f, F32(np.inf))


def loudness_feature(v):
    """v: the clamped f32 mean or std of the levels.  -> (reference, lowest, highest f32 the device may give): the reference
    is 10 log10(v) in float64, rounded to f32 and normalised in f32; the range is the image of LOG10F_ULP ulp of the logarithm
    (see the section's head) widened by one f32 ulp of the feature"""
    log = math.log10(float(v))
    ref = _normalize(F32(10.0 * log), -90.0, 0.0)
    ulp = float(np.spacing(_f32_at_or_below(abs(log))))
    lo, hi = _f32_at_or_below(log - LOG10F_ULP * ulp), _f32_at_or_above(log + LOG10F_ULP * ulp)
    f_lo, f_hi = (_normalize(F32(F32(10.0) * w), -90.0, 0.0) for w in (lo, hi))
    assert f_lo <= ref <= f_hi
    return ref, np.nextafter(f_lo, F32(-np.inf)), np.nextafter(f_hi, F32(np.inf))


def replay_loudness(oracle, levels):
    """features 8 and 9 (src/misc.rs:51-65) -> [(reference, lowest, highest, clamp taken)] for the mean and the std"""
    out = []
    for v in (F32(oracle.mean(levels)), F32(oracle.std(levels))):
        clamped = bool(v < F32(1e-9))
        out.append(loudness_feature(F32(1e-9) if clamped else v) + (clamped,))
    return out


def gated_tone(n, period):
    """A 10 kHz tone switched on and off (digital silence) every period / 2 samples.  Its per-frame series jump between
    nothing and the top of their range, so their std lies near the middle of it and the std features (3, 5, 7) near 0, where
    an f32 is fine enough to show one ulp of the std.  On white noise the std is a few per cent of the range, `2 std / max - 1`
    sits near -1 and swallows four of its bits: no white-noise song of the set tells a fused Welford step from a separately
    rounded one in its row, one gated song in four does (test_summary_song_set_reaches_the_kernel counts them)."""
    t = np.arange(n)
    return (0.5 * np.sin(2 * np.pi * 10000.0 * t / SR) * ((t // (period // 2)) % 2 == 0)).astype(F32)


def summary_songs(oracle):
    """-> (names, songs) of section 7's batch, in the caller's order"""
    live = [(f"noise_nt{61 + j}", oracle.white_noise(9700 + j, 8192 + 128 * j)) for j in range(41)]
    k = 0
    for base in (8192, 12288, 20480, 30720, 38912):
        for r in SUMMARY_RESIDUES:
            if base + r > 8192:   # 8192 itself is noise_nt61
                live.append((f"res_{base}+{r}", oracle.white_noise(9800 + k, base + r)))
                k += 1
    live += [(f"filler_{k}", oracle.white_noise(9900 + k, 8192 + 613 * k + k % 7)) for k in range(26)]
    live += [(f"gated_{k}", gated_tone(8192 + 613 * k + k % 7, 1536 + 128 * (k % 9))) for k in range(26, 52)]
    t = np.arange(33333)
    live += [
        ("silence", np.zeros(30000, F32)),
        ("dc", np.full(25000, 0.25, F32)),
        ("square", np.where(np.arange(20001) % 50 < 25, 1.0, -1.0).astype(F32)),
        ("tone_440", (0.5 * np.sin(2 * np.pi * 440.0 * t / SR)).astype(F32)),
        ("noise_1e-12", (oracle.white_noise(9990, 22222) * F32(1e-12)).astype(F32)),
        ("noise_1e4", (oracle.white_noise(9991, 17777) * F32(1e4)).astype(F32)),
        ("noise_60s", oracle.white_noise(9992, 60 * SR)),
    ]
    names, songs = [k for k, _ in live], [x for _, x in live]
    for pos in sorted(SUMMARY_SHORT):
        n = SUMMARY_SHORT[pos]
        names.insert(pos, f"short_{n}")
        songs.insert(pos, oracle.white_noise(9995, 8191)[:n])
    return names, songs


@pytest.fixture(scope="module")
def summary_set(oracle):
    return summary_songs(oracle)


def _blocks_of(x):
    """(energy, crossings) of the 256-sample blocks of x, the energies in float64 (exact for the inputs of the CPU test)"""
    edges = np.arange(0, len(x), 256)
    pos = x > 0.0
    flips = np.concatenate([[False], pos[1:] != pos[:-1]])   # number_crossings (src/utils.rs:81-95): was_positive starts at x[0]
    return np.add.reduceat(x.astype(np.float64) ** 2, edges), np.add.reduceat(flips.astype(np.int64), edges)


def test_oracle_std_is_the_fused_welford(oracle):
    """oracle.std, the `std` of every replay below, is ndarray's Welford step with ONE rounding in its multiply-add: bit for
    bit against exact rationals rounded once, on series among which the separately rounded form gives another f32."""
    rng = np.random.default_rng(707)
    series = {
        "noise_200": oracle.white_noise(9701, 200),
        "noise_97": oracle.white_noise(9008, 97),
        "noise_61": oracle.white_noise(9002, 61),
        "noise_5": oracle.white_noise(9011, 5),
        "centroids_97": rng.uniform(500.0, 6000.0, 97).astype(F32),
        "rolloffs_61": (rng.integers(20, 250, 61) * 43.06640625).astype(F32),
        "levels_33": (rng.uniform(0.0, 1.0, 33) ** 2).astype(F32),
        "constant_64": np.full(64, 0.0625, F32),
        "single": np.array([3.5], F32),
        "tiny_50": (rng.standard_normal(50) * 1e-20).astype(F32),
    }
    differs = []
    for k, s in series.items():
        assert len(s) <= 200
        fused, plain = welford_std(s, True), welford_std(s, False)
        got = F32(oracle.std(s))
        assert _same_f32(got, fused), f"{k}: oracle.std {got!r}, Welford with an exact fused multiply-add {fused!r} (separately rounded {plain!r})"
        if not _same_f32(fused, plain):
            differs.append(k)
    print("series on which a separately rounded multiply-add gives another std:", differs)
    # (a rounding of the product moves the sum only while the sum is small, and most such differences are absorbed as the sum
    # grows: about one white-noise series in eight ends in another f32 -- the device test has over 500 series)
    assert differs, "no series of the set tells a fused multiply-add from a separately rounded one"
    assert _same_f32(welford_std(series["constant_64"], True), F32(0.0))


def test_summary_replay_reproduces_the_oracle(oracle):
    """The replay of features 1, 8 and 9 is the oracle's zcr / loudness.  The songs take values k / 16, |k| <= 16: every f32
    sum of up to 1024 of their squares is exact, so block sums added in order ARE the reference's sequential sums, and the
    only difference left is the host's log10f against float64 -- held to the allowance of the device test."""
    rng = np.random.default_rng(708)
    worst = [0, 0]
    lengths = [8192 + r for r in SUMMARY_RESIDUES] + [20480 + r for r in SUMMARY_RESIDUES] + [8192 + 613 * 7 + 3]
    songs = [(rng.integers(-16, 17, n) / 16.0).astype(F32) for n in lengths]
    songs += [np.zeros(9000, F32), np.full(25000, 0.25, F32), np.where(np.arange(20001) % 50 < 25, 1.0, -1.0).astype(F32)]
    clamps = []
    for x in songs:
        n = len(x)
        e, zc = _blocks_of(x)
        assert int(zc.sum()) == oracle.number_crossings(x), n
        assert _same_f32(replay_zcr(zc, n), F32(oracle.zcr(x))), n
        levels = replay_levels(e.astype(F32), n)
        assert len(levels) == -(-n // LOUD_W)
        ref = oracle.loudness(x)
        for k, (want, lo, hi, clamped) in enumerate(replay_loudness(oracle, levels)):
            assert lo <= ref[k] <= hi, (n, 8 + k, ref[k], want, lo, hi)
            if clamped:
                assert ref[k] == F32(-1.0) and want == F32(-1.0), (n, 8 + k, ref[k], want)
            worst[k] = max(worst[k], int(_ulps(ref[k], want)))
            clamps.append((n, 8 + k, clamped))
    print(f"oracle.loudness against the replay: worst {worst[0]} / {worst[1]} ulp of features 8 / 9")
    assert {(f, c) for _, f, c in clamps} == {(8, False), (8, True), (9, False), (9, True)}


def _scheduler_order(lengths):
    """The batch scheduler keeps a chunk's songs longest first, equal lengths in the caller's order"""
    return sorted(range(len(lengths)), key=lambda i: -lengths[i])


def test_summary_song_set_reaches_the_kernel(oracle, summary_set):
    """From the lengths alone: what section 7's batch puts in front of seq_for_each, of the loudness chunks and of the
    64-songs-per-wavefront mapping; from the oracle, which songs take the two clamps."""
    names, songs = summary_set
    lengths = [len(x) for x in songs]
    live = [n for n in lengths if n >= 8192]
    assert 140 <= len(songs) <= 160 and sum(8192 <= n <= 40000 for n in lengths) >= len(songs) - 6
    # three blocks of 64 lanes, the last one part filled, also when only the live songs count
    assert 128 < len(live) <= len(songs) < 192 and len(songs) % 64 and len(live) % 64
    short = [i for i, n in enumerate(lengths) if n < 8192]
    assert [lengths[i] for i in short] == [0, 1, 100, 8191] and short == sorted(SUMMARY_SHORT)
    assert short[0] > 0 and short[-1] < len(songs) - 1 and min(np.diff(short)) > 32, short   # live songs on both sides of each
    # the white-noise ladder: every residue of n_t mod 4 and mod 32, one or two whole chunks (and more) after a prologue
    n_t = [(n - 512) // 128 + 1 for n in lengths[:7] + lengths[8:42]]
    assert n_t == list(range(61, 102)), n_t
    assert {v % 32 for v in n_t} == set(range(32)) and {v % 4 for v in n_t} == set(range(4))
    assert {(v - 3) // 32 for v in n_t} | {v // 32 for v in n_t} >= {1, 2, 3}
    # every start alignment of a series (float index mod 4 within a 256-byte aligned buffer), in the scheduler's order and in
    # the caller's; the series lie back to back, so an offset is the sum of the counts before it
    for order in (_scheduler_order(lengths), list(range(len(lengths)))):
        ordered = [lengths[i] for i in order if lengths[i] >= 8192]
        for count in (lambda n: (n - 512) // 128 + 1, lambda n: -(-n // 256)):
            starts = np.concatenate([[0], np.cumsum([count(n) for n in ordered])[:-1]])
            assert all((starts % 4 == a).sum() >= 8 for a in range(4)), [(starts % 4 == a).sum() for a in range(4)]
    # the loudness chunks: every listed residue, a last chunk of 1, 2, 3 and 4 blocks, short last blocks, and series of
    # 32 .. 35 blocks (less than one whole 32-element step once a prologue of 1 .. 3 has run)
    assert {n % LOUD_W for n in live} >= set(SUMMARY_RESIDUES)
    assert {-(-(n % LOUD_W or LOUD_W) // 256) for n in live} == {1, 2, 3, 4}
    assert sum(n % 256 != 0 for n in live) > 100
    assert {-(-n // 256) for n in live} >= {32, 33, 34, 35}
    assert max(live) == 60 * SR and -(-max(live) // 256) > 5000      # the long chain
    # the Welford step's fused multiply-add must show in a ROW: on the oracle's own series, the std features of the gated songs
    # that come out differently when the product is rounded on its own (5 of 78)
    shows = []
    for k, x in zip(names, songs):
        if k.startswith("gated_"):
            for series, (_, f, mx) in zip(oracle.SpectralDesc().run(x).series(), SUMMARY_SERIES):
                if not _same_f32(_normalize(welford_std(series, True), 0.0, mx), _normalize(welford_std(series, False), 0.0, mx)):
                    shows.append((k, f + 1))
    print("std features that tell a fused multiply-add from a separately rounded one:", shows)
    assert len(shows) >= 3, shows
    # the clamps, on the oracle (exact inputs, or clear of the threshold by orders of magnitude)
    taken = {8: [], 9: []}
    for k, x in zip(names, songs):
        if len(x) >= 8192 and not k.startswith(("noise_nt", "res_", "filler_", "gated_")):
            e, _ = _blocks_of(x)
            for f, (want, _, _, clamped) in zip((8, 9), replay_loudness(oracle, replay_levels(e.astype(F32), len(x)))):
                if clamped:
                    taken[f].append(k)
                    assert want == F32(-1.0) and oracle.loudness(x)[f - 8] == F32(-1.0), (k, f)
    print("oracle: mean clamp (feature 8):", taken[8], " std clamp (feature 9):", taken[9])
    assert taken[8] == ["silence", "noise_1e-12"] and taken[9] == ["silence", "dc", "square", "noise_1e-12"], taken


@pytest.mark.gpu
def test_summary_features_on_the_device_series(bliss, oracle, summary_set):
    """Features 1..7 of every live song bit for bit, features 8 and 9 within the image of LOG10F_ULP = 2 ulp of log10f plus
    one ulp of the feature, exactly -1.0f where a clamp is taken; too-short songs: status 1, a NaN row, no taps, and the rows
    of the others are those of the batch without them.

    Measured on the MI355X: 973 values bit for bit (139 songs x features 1..7); features 8 / 9 at most 4 / 8 ulp of the
    feature from the float64 reference (noise_nt82 / filler_13; the widest allowed range is 17 ulp: the bound on log10f is
    2 ulp, but one ulp of 10 log10(v) + 90 near 85 is 1.7e-7 in the feature, many ulp of a feature near 0); mean clamp:
    silence, noise_1e-12; std clamp: silence, dc, square, noise_1e-12.  With the Welford step's fused multiply-add replaced
    by a product and a sum, 10 of the 973 values differ (by one ulp); with the last loudness chunk over 1024, features 8 / 9
    are up to 220 202 ulp away; with the prologue of seq_for_each starting at 1, 684 of the 973 differ."""
    names, songs = summary_set
    ctx = bliss.Context(0)
    try:
        rows, status = _run(ctx, songs)
        assert ctx.last_chunks() == 1
        bad, exact, differ, worst, widest, taken = [], 0, 0, {8: (0, ""), 9: (0, "")}, 0, {8: [], 9: []}
        for i, (k, x) in enumerate(zip(names, songs)):
            n = len(x)
            if n < 8192:
                assert status[i] == 1 and np.isnan(rows[i]).all(), (k, status[i], rows[i])
                assert all(len(ctx.debug_fetch_raw(tap, i)) == 0 for tap in ("centroid", "energy256", "crossings256")), k
                continue
            assert status[i] == 0 and np.isfinite(rows[i]).all(), (k, status[i], rows[i])
            want = {}
            for tap, f, mx in SUMMARY_SERIES:
                series = ctx.debug_fetch(tap, i)
                assert len(series) == (n - 512) // 128 + 1, (k, tap, len(series))
                want[f], want[f + 1] = replay_timbral(oracle, series, mx)
            e, zc = ctx.debug_fetch("energy256", i), ctx.debug_fetch("crossings256", i)
            assert int(zc.sum(dtype=np.int64)) == oracle.number_crossings(x), k
            want[1] = replay_zcr(zc, n)
            for f in range(1, 8):
                exact += 1
                if not _same_f32(rows[i, f], want[f]):
                    differ += 1
                    bad.append(f"{k} (n = {n}): feature {f}: device {rows[i, f]!r}, replay {want[f]!r} ({int(_ulps(rows[i, f], want[f]))} ulp)")
            for f, (ref, lo, hi, clamped) in zip((8, 9), replay_loudness(oracle, replay_levels(e, n))):
                got = rows[i, f]
                d = int(_ulps(got, ref))
                widest = max(widest, int(_ulps(lo, ref)), int(_ulps(hi, ref)))
                if d > worst[f][0]:
                    worst[f] = (d, k)
                if clamped:
                    taken[f].append(k)
                    if got != F32(-1.0):
                        bad.append(f"{k}: feature {f} takes the 1e-9 clamp and must be -1.0f: device {got!r}")
                elif not lo <= got <= hi:
                    bad.append(f"{k} (n = {n}): feature {f}: device {got!r}, float64 reference {ref!r} ({d} ulp), allowed {lo!r} .. {hi!r}")
        print(f"features 1..7 of {exact // 7} songs: {exact} values compared bit for bit, {differ} differ")
        print(f"features 8 / 9 against the float64 reference: worst {worst[8][0]} ulp ({worst[8][1]}) / {worst[9][0]} ulp ({worst[9][1]}); "
              f"the widest allowed range is {widest} ulp")
        print("mean clamp (feature 8):", taken[8], " std clamp (feature 9):", taken[9])
        assert not bad, f"{len(bad)} differences; the first: " + "; ".join(bad[:6])
        assert taken[8] == ["silence", "noise_1e-12"] and taken[9] == ["silence", "dc", "square", "noise_1e-12"], taken
        # the too-short songs do not shift their neighbours: the same rows without them
        keep = [i for i, x in enumerate(songs) if len(x) >= 8192]
        rows2, status2 = _run(ctx, [songs[i] for i in keep])
        assert (status2 == 0).all() and _same(rows2, rows[keep])
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# 8. the chroma features on the device's own interval means
# ---------------------------------------------------------------------------------------------
CHORDS = {   # semitones from A = 440, equal tempered
    "chord_augmented": (-9, -5, -1),
    "chord_dim7": (-9, -6, -3, 0),
    "chord_tritone": (-9, -3),
    "chord_major": (-9, -5, -2),
}
CLAMP_20 = ["chord_augmented", "chord_dim7", "chord_tritone"]   # the songs whose feature 20 (21) sits on the 1.0 clamp
CLAMP_21 = ["chord_augmented", "chord_dim7"]


def chroma_songs(oracle, musical=True):
    """Section 8's songs: those of test_chroma_stage_on_detuned_songs, and four-second sine chords"""
    songs = {}
    if musical:
        import os
        import sys

        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
        import musical_check

        rng = np.random.default_rng(404)
        for i in range(12):
            songs[f"musical_{i}"] = musical_check.make_song(rng)[0]
    songs["noise_64_frames+17"] = oracle.white_noise(31, 64 * HOP + 17)
    songs["min_len_8192"] = oracle.white_noise(32, 8192)
    songs["silence"] = np.zeros(3 * SR, F32)
    t = np.arange(4 * SR) / SR
    for k, semis in CHORDS.items():
        songs[k] = (0.2 * sum(np.sin(2 * np.pi * 440.0 * 2.0 ** (s / 12.0) * t) for s in semis)).astype(F32)
    return songs


def replay_chroma_v1(interval):
    """ChromaDesc::get_values_version_1 (src/chroma.rs:128-132) of the ten interval means -> features 10..19"""
    return np.array([_normalize(F32(v), 0.0, 0.12) for v in interval], F32)


def replay_chroma_v2(interval):
    """ChromaDesc::get_values (src/chroma.rs:97-126) of the ten interval means -> features 10..22: the two norms summed in
    index order, the divisions where a norm is positive, the f32 cast and 2 v - 1, the two clamped norms, the angle"""
    raw = [float(v) for v in interval]
    n1 = n2 = 0.0
    for t in range(6):
        n1 += raw[t] * raw[t]
    for t in range(6, 10):
        n2 += raw[t] * raw[t]
    n1, n2 = math.sqrt(n1), math.sqrt(n2)
    if n1 > 0.0:
        raw[:6] = [v / n1 for v in raw[:6]]
    if n2 > 0.0:
        raw[6:] = [v / n2 for v in raw[6:]]
    out = [_normalize(F32(v), 0.0, 1.0) for v in raw]
    out.append(min(_normalize(F32(n1), 0.0, 0.25), F32(1.0)))
    out.append(min(_normalize(F32(n2), 0.0, 0.025), F32(1.0)))
    out.append(_normalize(F32(math.atan2(20.0 * n2, n1 + 1e-12)), 0.0, F32(1.57079632679489661923)))
    return np.array(out, F32)


def _check_chroma_row(row, interval, version, what):
    """-> (values equal bit for bit, 1 if feature 22 differs (by one ulp) else 0)"""
    want = replay_chroma_v1(interval) if version == 1 else replay_chroma_v2(interval)
    assert len(row) == 10 + len(want), (what, len(row))
    exact = min(len(want), 12)
    got = np.ascontiguousarray(row[10:], F32)
    diff = np.flatnonzero(got[:exact].view(np.uint32) != want[:exact].view(np.uint32))
    assert not len(diff), f"{what}: feature {10 + diff[0]}: {got[diff[0]]!r}, replay {want[diff[0]]!r}; interval means {interval.tolist()}"
    if version == 1:
        return exact, 0
    d = int(_ulps(got[12], want[12]))
    assert d <= 1, f"{what}: feature 22: {got[12]!r}, replay {want[12]!r}: {d} ulp"
    return exact, d


def test_chroma_replay_and_clamps_on_the_oracle(oracle):
    """The NumPy replay is the oracle's get_values / get_values_version_1 on the oracle's own interval means (features
    10..21 bit for bit, 22 within an ulp), and the chords sit where section 8 needs them: the augmented triad and the
    diminished seventh on both 1.0 clamps, the tritone on the first with feature 21 near -0.96, the major triad and the
    other songs on neither; silence has a uniform chroma and positive norms."""
    on20, on21 = [], []
    for k, x in chroma_songs(oracle, musical=False).items():
        chroma, _ = oracle.chroma_desc(x)
        interval = oracle.chroma_interval_features(chroma)
        v2 = oracle.chroma_get_values(chroma, 2)
        _check_chroma_row(np.concatenate([np.zeros(10, F32), v2]), interval, 2, k)
        _check_chroma_row(np.concatenate([np.zeros(10, F32), oracle.chroma_get_values(chroma, 1)]), interval, 1, k)
        assert (v2[10:12] <= 1.0).all()
        if v2[10] == 1.0:
            on20.append(k)
        if v2[11] == 1.0:
            on21.append(k)
        if k == "chord_tritone":
            assert abs(float(v2[11]) + 0.96) < 0.02, v2[11]
        if k == "silence":
            # chroma_stft gives zeros; exp(15 x) and the column normalisation of chroma_interval_features make every pitch
            # class 1 / 12: the interval means are 1 / 12 and 1 / 144, neither norm is zero and both divisions happen
            assert not chroma.any() and np.allclose(interval, [1 / 12] * 6 + [1 / 144] * 4, rtol=1e-12), (chroma[:, 0], interval)
            assert (v2[:10] > -1.0).all() and (v2[10:12] < 1.0).all(), v2
    print("oracle: feature 20 on the clamp:", on20, " feature 21 on the clamp:", on21)
    assert on20 == CLAMP_20 and on21 == CLAMP_21, (on20, on21)


@pytest.mark.gpu
def test_chroma_features_on_the_device_interval(bliss, oracle):
    """Features 10..19 (v1) and 10..21 (v2) of every song bit for bit from the interval tap of the same run, feature 22 within
    one f32 ulp; features 0..9 of the v1 and v2 rows identical.

    Measured on the MI355X: 19 songs, 190 + 228 values bit for bit; feature 22 differs (by one ulp) on 0 songs; feature 20 on
    the clamp: the augmented triad, the diminished seventh, the tritone; feature 21: the first two."""
    songs = chroma_songs(oracle)
    names = list(songs)
    ctx = bliss.Context(0)
    ctx.set_option("debug_chroma", 1)
    try:
        rows, exact, differ22 = {}, {1: 0, 2: 0}, []
        for version in (1, 2):
            rows[version], status = _run(ctx, [songs[k] for k in names], version)
            assert (status == 0).all() and ctx.last_chunks() == 1
            assert rows[version].shape == (len(names), 20 if version == 1 else 23)
            for i, k in enumerate(names):
                interval = ctx.debug_fetch("interval", i)
                assert interval.shape == (10,) and interval.dtype == np.float64
                n, d = _check_chroma_row(rows[version][i], interval, version, f"v{version} {k}")
                exact[version] += n
                if d:
                    differ22.append(k)
        assert _same(rows[1][:, :10], rows[2][:, :10]), "features 0..9 differ between the v1 and the v2 row"
        on20 = [k for i, k in enumerate(names) if rows[2][i, 20] == 1.0]
        on21 = [k for i, k in enumerate(names) if rows[2][i, 21] == 1.0]
        print(f"{len(names)} songs: {exact[1]} (v1) + {exact[2]} (v2) chroma features compared bit for bit; feature 22 differs by "
              f"one ulp on {len(differ22)} songs: {differ22}")
        print("feature 20 on the clamp:", on20, " feature 21 on the clamp:", on21)
        assert (rows[2][:, 20:22] <= 1.0).all()
        assert on20 == CLAMP_20 and on21 == CLAMP_21, (on20, on21)
    finally:
        ctx.set_option("debug_chroma", 0)
        ctx.close()
