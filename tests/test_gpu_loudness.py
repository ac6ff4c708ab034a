"""GPU tests of the loudness measurement: the device's sub-block energies and both peaks bit for bit against the
numpy replay of the contract (tests/loudness_replay.py), the standards' known answers at their real lengths, batch
independence, albums and the FLAC path."""
import ctypes as C
import math
import sqlite3

import numpy as np
import pytest

import loudness_replay as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    return bliss_rs_amd


def _tables(rate):
    """the two tables of a rate as the library states them: the tables, not the formulas, are the contract"""
    from bliss_rs_amd import _ffi

    coef, factor, h = np.zeros(10), C.c_uint32(0), np.zeros(49)
    _ffi.call("blissgpu_loudness_kweighting", rate, coef.ctypes.data_as(C.POINTER(C.c_double)))
    _ffi.call("blissgpu_true_peak_filter", rate, C.byref(factor), h.ctypes.data_as(C.POINTER(C.c_double)))
    return coef, h


def _content(kind, n, channels, rng):
    if kind == "zero":
        x = np.zeros((n, channels))
    elif kind == "dc":
        x = 0.6 + 1e-3 * rng.standard_normal((n, channels))
    else:  # noise with a silent lead-in, another level per channel
        x = 0.2 * rng.standard_normal((n, channels)) * (1.0 + 0.5 * np.arange(channels))
        x[:n // 5] = 0.0
    return np.clip(x, -0.999, 0.999)


def _as_format(x, fmt):
    x = x[:, 0] if x.shape[1] == 1 else x
    if fmt == "s16":
        return np.round(x * 32767.0).astype(np.int16)
    if fmt == "s32":
        return np.round(x * 2147483647.0).astype(np.int32)
    return x.astype(np.float32)


def _mixed_songs():
    """(array, rate, kind) of the mixed batch: every length at which the segmentation takes another path at 22 050 Hz mono f32,
    every (format, channel count) with more than one segment at the low rates, the other rates and oversampling factors short"""
    S, W = R.header_constants()
    rng = np.random.default_rng(2024)
    H = R.hop(22050)
    plan = [("f32", 1, 22050, n, kind) for n, kind in (
        (4 * H - 1, "noise"), (4 * H, "dc"), (S * H - 1, "noise"), (S * H, "dc"), (S * H + 1, "noise"), ((S + W) * H + 1, "dc"),
        (int(2.5 * S * H) + 7, "noise"), (5 * H + 3, "zero"))]
    plan += [("s16", 2, 8000, int(2.5 * S * 800) + 5, "noise"), ("s16", 1, 8000, (S + 1) * 800 + 799, "dc"),
             ("s32", 2, 11025, (S + W + 1) * 1103 + 2, "noise"), ("f32", 2, 11025, (S + 2) * 1103, "dc"),
             ("s16", 2, 44100, 10 * 4410 + 13, "noise"), ("s32", 1, 48000, 9 * 4800 + 5, "noise"),
             ("f32", 1, 96000, 4 * 9600 + 7, "noise"), ("s16", 1, 192000, 4 * 19200, "dc")]
    return [(_as_format(_content(kind, n, ch, rng), fmt), rate, kind) for fmt, ch, rate, n, kind in plan]


@pytest.fixture(scope="module")
def mixed(bliss):
    """ONE loudness_batch call over the mixed songs with the energies tapped, and the replay of the same songs, each computed once"""
    songs = _mixed_songs()
    arrays, rates = [s[0] for s in songs], [s[1] for s in songs]
    results, taps = bliss.loudness_batch(arrays, rates, return_energies=True)
    S, W = R.header_constants()
    wide = [(R.widen(a), r) for a, r in zip(arrays, rates)]
    tables = {r: _tables(r) for r in set(rates)}
    want_z = R.segment_energies(wide, S, W, coefs=[tables[r][0] for r in rates])
    want_peaks = [R.peaks(x, r, tables[r][1]) for x, r in wide]
    return songs, results, taps, want_z, want_peaks


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_energies_and_peaks_are_the_replays_bit_for_bit(bliss, mixed):
    songs, results, taps, want_z, want_peaks = mixed
    assert isinstance(results[0], bliss.AnalysisError) and not taps[0][0].any() and taps[0][1:] == (0.0, 0.0)  # 4 H - 1 samples
    for i in range(1, len(songs)):
        (a, rate, kind), (z, sp, tp) = songs[i], taps[i]
        what = (i, a.dtype.name, a.shape, rate, kind)
        assert isinstance(results[i], bliss.Loudness), what
        assert z.shape == want_z[i].shape and z.shape[1] == a.shape[0] // R.hop(rate), what
        diff = np.flatnonzero(_bits(z).reshape(-1) != _bits(want_z[i]).reshape(-1))
        assert diff.size == 0, (what, "sub-block energies differ at", diff[:8].tolist(), z.reshape(-1)[diff[:4]], want_z[i].reshape(-1)[diff[:4]])
        assert (sp, tp) == want_peaks[i], (what, (sp, tp), want_peaks[i])
        if kind == "zero":
            assert not z.any() and results[i].lufs == -math.inf and results[i].power == 0.0 and (sp, tp) == (0.0, 0.0), what
        else:
            assert z.min() >= 0.0 and z.max() > 0.0 and tp > 0.0 and math.isfinite(results[i].lufs), what
        # behind the energies: the Python replay of the blocks and the gates
        P, ST = R.blocks(z, R.hop(rate))
        assert _bits(results[i].power) == _bits(R.gate(P)[0]) and (results[i].sample_peak, results[i].true_peak) == (sp, tp), what
        if kind != "zero":
            assert abs(results[i].lufs - R.gate(P)[1]) <= 1e-12 and abs(results[i].range_lu - R.loudness_range(ST)[0]) <= 1e-12, what


def test_the_standards_known_answers_on_the_device(bliss):
    cases = [(48000, levels, seconds) for levels, seconds, _, _ in R.TECH_3341]
    cases += [(48000, levels, [20.0] * len(levels)) for levels, _, _ in R.TECH_3342]
    cases += [(44100,) + R.TECH_3341[0][:2], (44100, R.TECH_3342[0][0], [20.0, 20.0])]
    arrays = [R.sine(rate, 1000.0, levels, seconds).astype(np.float32) for rate, levels, seconds in cases]
    arrays.append(R.sine(48000, 997.0, [0.0], [20.0], channels=1)[:, 0].astype(np.float32))
    rates = [c[0] for c in cases] + [48000]
    peak_rates = (22050, 44100, 48000)
    for rate in peak_rates:  # a sine at fs / 4, amplitude 0.5, phase 45 degrees: every sample sits at 0.3536, the peaks between them
        arrays.append((0.5 * np.sin(2.0 * np.pi * 0.25 * np.arange(rate) + np.pi / 4.0)).astype(np.float32))
        rates.append(rate)
    out = bliss.loudness_batch(arrays, rates)
    for k, (_, _, want, tol) in enumerate(R.TECH_3341):
        print(f"Tech 3341 case {k + 1} on the device: {out[k].lufs:.3f} LUFS (wanted {want} +- {tol})")
        assert abs(out[k].lufs - want) <= tol, (k + 1, out[k])
    for k, (_, want, tol) in enumerate(R.TECH_3342):
        print(f"Tech 3342 case {k + 1} on the device: LRA {out[5 + k].range_lu:.3f} LU (wanted {want} +- {tol})")
        assert abs(out[5 + k].range_lu - want) <= tol, (k + 1, out[5 + k])
    print(f"at 44 100 Hz: {out[9].lufs:.3f} LUFS, LRA {out[10].range_lu:.3f} LU")
    assert abs(out[9].lufs + 23.0) <= 0.1 and abs(out[10].range_lu - 10.0) <= 1.0
    print(f"997 Hz full-scale sine, one channel: {out[11].lufs:.4f} LUFS")
    assert abs(out[11].lufs + 3.01) <= 0.05
    for rate, ld in zip(peak_rates, out[12:]):
        sample_db, true_db = 20.0 * math.log10(ld.sample_peak), 20.0 * math.log10(ld.true_peak)
        print(f"fs / 4 sine at {rate} Hz: sample peak {sample_db:.3f} dBFS, true peak {true_db:.3f} dBTP")
        assert abs(sample_db + 9.03) <= 0.01 and -6.02 - 0.4 <= true_db <= -6.02 + 0.2, (rate, sample_db, true_db)


def _same(a, b, bliss):
    if isinstance(a, bliss.AnalysisError) or isinstance(b, bliss.AnalysisError):
        return type(a) is type(b)
    return all(_bits(getattr(a, f)) == _bits(getattr(b, f)) for f in ("power", "lufs", "range_lu", "sample_peak", "true_peak"))


def test_a_song_is_independent_of_its_batch_and_of_a_split(bliss, mixed):
    from bliss_rs_amd import _ffi

    songs, results, taps, _, _ = mixed
    arrays, rates = [s[0] for s in songs], [s[1] for s in songs]
    for i in (6, 8, 10, 15):  # alone: the same bytes
        alone, tap = bliss.loudness_batch([arrays[i]], [rates[i]], return_energies=True)
        assert _same(alone[0], results[i], bliss) and np.array_equal(_bits(tap[0][0]), _bits(taps[i][0])) and tap[0][1:] == taps[i][1:], i
    whole = bliss.loudness_batch(arrays, rates)  # blissgpu_loudness_batch: the gates in the library, the same figures
    assert all(_same(a, b, bliss) for a, b in zip(whole, results))
    ctx = C.c_void_p()
    _ffi.call("blissgpu_default_ctx", 0, C.byref(ctx))
    limit = int(_ffi.call("blissgpu_ctx_get_workspace_limit", ctx))
    _ffi.call("blissgpu_ctx_set_workspace_limit", ctx, 1 << 20)  # half of it holds PCM: the batch runs in several groups
    try:
        assert sum(a.nbytes for a in arrays) > 2 * (1 << 19)  # more PCM than two groups hold: at least three
        split, split_taps = bliss.loudness_batch(arrays, rates, return_energies=True)
        split_whole = bliss.loudness_batch(arrays, rates)
    finally:
        _ffi.call("blissgpu_ctx_set_workspace_limit", ctx, limit)
    for i in range(len(songs)):
        assert _same(split[i], results[i], bliss) and _same(split_whole[i], results[i], bliss), i
        assert np.array_equal(_bits(split_taps[i][0]), _bits(taps[i][0])) and split_taps[i][1:] == taps[i][1:], i


def test_albums_are_gated_over_their_songs_blocks(bliss, mixed, tmp_path):
    songs, results, taps, _, _ = mixed
    pick = [6, 12, 0, 8, 13, 7]  # song 0 is too short, song 7 is digital silence
    labels = ["a", "a", "b", "b", "c", "c"]
    arrays, rates = [songs[i][0] for i in pick], [songs[i][1] for i in pick]
    out, albums = bliss.loudness_batch(arrays, rates, albums=labels)
    assert list(albums) == ["a", "b", "c"] and all(_same(o, results[i], bliss) for o, i in zip(out, pick))
    for name in albums:
        members = [i for i, l in zip(pick, labels) if l == name and not isinstance(results[i], bliss.AnalysisError)]
        P, ST = [], []
        for i in members:
            p, st = R.blocks(taps[i][0], R.hop(songs[i][1]))
            P += p
            ST += st
        ld = albums[name]
        assert _bits(ld.power) == _bits(R.gate(P)[0]) and abs(ld.lufs - R.gate(P)[1]) <= 1e-12, name
        assert abs(ld.range_lu - R.loudness_range(ST)[0]) <= 1e-12, name
        assert ld.sample_peak == max(taps[i][1] for i in members) and ld.true_peak == max(taps[i][2] for i in members), name
    assert albums["b"].power == results[8].power  # the too-short song adds nothing
    tapped = bliss.loudness_batch(arrays, rates, albums=labels, return_energies=True)[1]
    assert all(_same(tapped[name], albums[name], bliss) for name in albums)
    # into the sidecar table and back
    lib = bliss.library
    db = str(tmp_path / "library.db")
    lib.create_schema(db)
    d = bliss.FeaturesVersion.LATEST.feature_count()
    paths = [f"/m/{k}.flac" for k in range(len(pick))]
    lib.store_songs(db, [bliss.Song(path=p, analysis=bliss.Analysis(np.full(d, 0.1 * k, np.float32), bliss.FeaturesVersion.LATEST))
                         for k, p in enumerate(paths)])
    measured = {p: o for p, o in zip(paths, out) if isinstance(o, bliss.Loudness)}
    lib.store_loudness(db, measured, albums={p: albums[l] for p, l in zip(paths, labels)})
    back = lib.load_loudness(db)
    assert list(back) == [p for p in paths if p in measured]
    for p, l in zip(paths, labels):
        if p in measured:
            got, album_lufs, album_peak = back[p]
            assert (got.lufs, got.range_lu, got.sample_peak, got.true_peak) == (measured[p].lufs, measured[p].range_lu,
                                                                               measured[p].sample_peak, measured[p].true_peak)
            assert (album_lufs, album_peak) == (albums[l].lufs, albums[l].true_peak)
    rows = sqlite3.connect(db).execute("select count(*), min(version), max(version) from gpu_loudness").fetchone()
    assert rows == (len(measured), bliss.LOUDNESS_VERSION, bliss.LOUDNESS_VERSION)
    stats = lib.loudness_statistics(db)
    assert stats["count"] == len(measured) and stats["silent"] == 1


def test_flac_files_measure_like_their_samples(bliss):
    import flac_craft

    rng = np.random.default_rng(5)
    files, pcm, rates = [], [], []
    for bps, channels, rate, n in ((16, 1, 8000, 5 * 800 + 9), (16, 2, 11025, 6 * 1103), (24, 2, 8000, 4 * 800 + 1), (24, 1, 22050, 4 * 2205 + 3)):
        lim = (1 << (bps - 1)) - 1
        a = np.clip(np.round(0.3 * lim * rng.standard_normal((n, channels))), -lim - 1, lim).astype(np.int64)
        data, _ = flac_craft.stream(a if channels > 1 else a[:, 0], bps, {"blocksize": 1152}, rate=rate)
        files.append(data)
        # what the decoder hands on: int16 up to 16 bits, int32 left-justified above
        pcm.append(a.astype(np.int16) if bps <= 16 else (a << (32 - bps)).astype(np.int32))
        rates.append(rate)
    files.append(b"not a flac file")
    labels = ["x", "y", "x", "y", "y"]
    got, got_albums = bliss.loudness_flac_batch(files, albums=labels)
    want, want_albums = bliss.loudness_batch(pcm, rates, albums=labels[:4])
    assert isinstance(got[4], bliss.DecodingError)
    assert all(_same(g, w, bliss) and isinstance(g, bliss.Loudness) for g, w in zip(got[:4], want))
    assert list(got_albums) == ["x", "y"] and all(_same(got_albums[k], want_albums[k], bliss) for k in want_albums)
    assert all(_same(g, w, bliss) for g, w in zip(bliss.loudness_flac_batch(files[:2]), want[:2]))
