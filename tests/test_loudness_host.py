"""CPU-only tests of the loudness measurement: the coefficient and interpolator tables, the segmented filter of
the contract against the sequential one (numpy and scipy only), the device-free blocks, gates and range against a plain Python
replay and the standards' known answers, the argument checks, the sidecar table, and loudness_gate.hpp as a stand-alone program
under AddressSanitizer."""
import ctypes as C
import math
import os
import re
import sqlite3
import subprocess

import numpy as np
import pytest

import loudness_replay as R
from conftest import ROOT

HPP = os.path.join(ROOT, "bliss-rs_amd", "csrc", "loudness_gate.hpp")
SRC = os.path.join(ROOT, "tests", "cpp", "test_loudness_gate.cpp")
SAN_CXX = "/opt/rocm/lib/llvm/bin/clang++"
RATES = (8000, 11025, 22050, 44100, 96000, 192000)
BS1770_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
              -1.99004745483398, 0.99007225036621)


@pytest.fixture(scope="module")
def bliss():
    import bliss_rs_amd

    if not os.path.exists(bliss_rs_amd.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return bliss_rs_amd


def _table(bliss, rate):
    from bliss_rs_amd import _ffi

    coef = np.zeros(10)
    _ffi.call("blissgpu_loudness_kweighting", rate, coef.ctypes.data_as(C.POINTER(C.c_double)))
    return coef


def _peak_table(bliss, rate):
    from bliss_rs_amd import _ffi

    factor, h = C.c_uint32(0), np.zeros(49)
    _ffi.call("blissgpu_true_peak_filter", rate, C.byref(factor), h.ctypes.data_as(C.POINTER(C.c_double)))
    return factor.value, h


def test_symbols_kernel_table_and_build_flags(bliss):
    from bliss_rs_amd import _ffi

    for name in ("blissgpu_loudness_subblocks", "blissgpu_loudness_kweighting", "blissgpu_true_peak_filter", "blissgpu_loudness_blocks",
                 "blissgpu_loudness_gate", "blissgpu_loudness_range", "blissgpu_loudness_energies", "blissgpu_loudness_batch"):
        assert name in _ffi.SIGNATURES and hasattr(_ffi.lib(), name), name
    assert not [s for s in _ffi.SIGNATURES if "loudness" in s and s.endswith("_device")]
    for name in ("Loudness", "loudness_batch", "loudness_flac_batch", "LOUDNESS_VERSION"):
        assert hasattr(bliss, name)
    for name in ("store_loudness", "load_loudness", "loudness_statistics"):
        assert hasattr(bliss.library, name)
    L = _ffi.lib()
    names = [L.blissgpu_profile_kernel_name(k).decode() for k in range(L.blissgpu_profile_kernel_count())]
    src = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "kernels_loudness.hip")).read()
    for name in ("loud_energy_kernel", "loud_peak_kernel"):
        assert names.count(name) == 1 and re.search(r"\bvoid\s+%s\s*\(" % name, src), name
    assert names[-2:] == ["group_forest_scan_kernel", "journey_step_kernel"]  # (older ids keep their places)
    code = re.sub(r"//[^\n]*", "", src)
    assert "asm" not in code and not re.search(r"atomic\w*\([^)]*(double|float)", code)
    make = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "Makefile")).read()
    assert re.search(r"kernels_loudness\.o[^\n]*: EXTRA := \$\(NOCONTRACT\)", make)
    assert re.search(r"^OBJS\s*:=[^\n]*\bkernels_loudness\.o", make, flags=re.M)
    S, W = R.header_constants()
    assert 8 <= S <= 64 and W == 4


def test_kweighting_table_is_bs1770_at_48k_and_the_formula_elsewhere(bliss):
    t = _table(bliss, 48000)
    got = (t[0], t[1], t[2], t[3], t[4], t[8], t[9])
    assert max(abs(g - w) for g, w in zip(got, BS1770_48K)) <= 1e-13, got
    assert t[5:8].tolist() == [1.0, -2.0, 1.0]
    for rate in RATES:
        got, want = _table(bliss, rate), R.kweighting(rate)
        rel = np.abs(got - want) / np.abs(want)
        print(f"k-weighting at {rate} Hz: worst relative difference from the formula {rel.max():.3g}")
        assert rel.max() <= 1e-15, (rate, got, want)
    from bliss_rs_amd import _ffi

    for rate in (7999, 768001, 0):
        assert _ffi.call_unchecked("blissgpu_loudness_kweighting", rate, np.zeros(10).ctypes.data_as(C.POINTER(C.c_double))) == _ffi.ERR_INVALID


def test_true_peak_filter_table_and_factors(bliss):
    for rate, factor in ((8000, 4), (44100, 4), (95999, 4), (96000, 2), (191999, 2), (192000, 1), (768000, 1)):
        f, h = _peak_table(bliss, rate)
        assert f == factor == R.peak_factor(rate), rate
        want = R.peak_filter(factor)
        print(f"true-peak filter, factor {factor}: worst difference from the formula {np.abs(h - want).max():.3g}")
        assert np.abs(h - want).max() <= 1e-15
        assert h[24] == 1.0 and h[0] == 0.0 and np.abs(h - h[::-1]).max() <= 1e-15


def _signals(rate, seconds, seed):
    rng = np.random.default_rng(seed)
    n = int(seconds * rate)
    noise = 0.1 * rng.standard_normal(n)
    noise[:rate // 2] = 0.0  # a silent lead-in
    dc = 0.9 + 1e-3 * rng.standard_normal(n)
    t = np.arange(n) / rate
    chirp = 0.5 * np.sin(2.0 * np.pi * (20.0 * t + (10000.0 - 20.0) / (2.0 * seconds) * t * t))
    return {"noise": noise, "dc": dc, "chirp": chirp}


def test_segmented_filter_against_the_sequential_one():
    """the contract's segments (zero state W sub-blocks early) against scipy's sosfilt over the whole signal; no code under test"""
    from scipy.signal import sosfilt

    S, W = R.header_constants()
    songs, names = [], []
    for rate in (22050, 44100, 48000):
        for name, x in _signals(rate, (2.5 * S + 0.5) / 10.0, rate).items():
            songs.append((x[:, None], rate))
            names.append((name, rate))
    got = R.segment_energies(songs, S, W)
    worst = {}
    for (x, rate), (name, _), z in zip(songs, names, got):
        co = R.kweighting(rate)
        y = sosfilt(np.array([[co[0], co[1], co[2], 1.0, co[3], co[4]], [co[5], co[6], co[7], 1.0, co[8], co[9]]]), x[:, 0])
        H = R.hop(rate)
        n_sub = x.shape[0] // H
        assert z.shape == (1, n_sub) and n_sub > 2 * S
        ref = (y[:n_sub * H].reshape(n_sub, H) ** 2).sum(axis=1)
        assert np.array_equal(z[0][ref == 0.0], ref[ref == 0.0])  # the silent lead-in stays exactly silent
        rel = np.abs(z[0] - ref)[ref > 0.0] / ref[ref > 0.0]
        worst[name] = max(worst.get(name, 0.0), float(rel.max()))
        assert rel.max() <= 1e-9, (name, rate, float(rel.max()))
    print("segmented against sequential, worst relative sub-block energy error:", {k: f"{v:.3g}" for k, v in worst.items()})


def _fixed_point_block():
    """g with ((g + 1.0) / 2.0) * 0.1 == g in floats: a block exactly AT the relative gate of [g, 1.0]"""
    g = 0.05
    for _ in range(200):
        nxt = ((g + 1.0) / 2.0) * 0.1
        if nxt == g:
            return g
        g = nxt
    raise AssertionError("no fixed point")


def _gate_inputs():
    rng = np.random.default_rng(11)
    g = _fixed_point_block()
    return {
        "empty": [],
        "all below -70": [1e-8, 5e-8, R.ABS_GATE, 0.0],
        "at the absolute gate": [R.ABS_GATE, R.ABS_GATE, float(np.nextafter(R.ABS_GATE, 1.0)), 1e-3],
        "at the relative gate": [g, 1.0],
        "just above the relative gate": [float(np.nextafter(g, 1.0)), 1.0],
        "one block": [0.01],
        "equal blocks": [0.02] * 7,
        "random": (10.0 ** rng.uniform(-8.0, -1.0, 500)).tolist(),
        "random short-term": (10.0 ** rng.uniform(-7.5, -1.5, 331)).tolist(),
    }


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _close(a, b, tol=1e-12):
    return a == b or abs(a - b) <= tol


def test_gates_and_range_against_the_python_replay(bliss):
    for name, values in _gate_inputs().items():
        power, lufs = bliss.loudness_gate(values)
        want_power, want_lufs = R.gate(values)
        assert _same_bits(power, want_power) and _close(lufs, want_lufs), (name, power, want_power, lufs, want_lufs)
        r, lo, hi = bliss.loudness_range(values)
        want = R.loudness_range(values)
        assert _same_bits([lo, hi], want[1:]) and _close(r, want[0]), (name, (r, lo, hi), want)
    assert bliss.loudness_gate([]) == (0.0, -math.inf) and bliss.loudness_range([]) == (0.0, 0.0, 0.0)
    assert bliss.loudness_gate([1e-8, R.ABS_GATE]) == (0.0, -math.inf)
    assert bliss.loudness_gate(_gate_inputs()["at the relative gate"])[0] == 1.0  # the block AT the gate is out
    # blocks, and an album of songs with different H: the gates over the concatenation, blocks never span songs
    rng = np.random.default_rng(12)
    album_P, album_ST, want_P, want_ST = [], [], [], []
    for rate, channels, n_sub in ((44100, 2, 47), (48000, 1, 31), (11025, 2, 4), (8000, 1, 29), (96000, 2, 30)):
        z = rng.uniform(0.0, 50.0, (channels, n_sub))
        P, ST = bliss.loudness_blocks(z, rate)
        wP, wST = R.blocks(z, R.hop(rate))
        assert P.shape == (n_sub - 3,) and ST.shape == (max(n_sub - 29, 0),)
        assert _same_bits(P, wP) and _same_bits(ST, wST), (rate, channels, n_sub)
        album_P.append(P), album_ST.append(ST), want_P.extend(wP), want_ST.extend(wST)
    power, lufs = bliss.loudness_gate(np.concatenate(album_P))
    assert _same_bits(power, R.gate(want_P)[0]) and _close(lufs, R.gate(want_P)[1])
    got, want = bliss.loudness_range(np.concatenate(album_ST)), R.loudness_range(want_ST)
    assert _same_bits(got[1:], want[1:]) and _close(got[0], want[0])
    P, ST = bliss.loudness_blocks(np.zeros((2, 3)), 48000)
    assert P.size == 0 and ST.size == 0


def _sequential_energies(x, rate):
    from scipy.signal import sosfilt

    co = R.kweighting(rate)
    sos = np.array([[co[0], co[1], co[2], 1.0, co[3], co[4]], [co[5], co[6], co[7], 1.0, co[8], co[9]]])
    H = R.hop(rate)
    n_sub = x.shape[0] // H
    return np.stack([(sosfilt(sos, x[:, c])[:n_sub * H].reshape(n_sub, H) ** 2).sum(axis=1) for c in range(x.shape[1])])


def test_the_standards_known_answers_through_the_gates(bliss):
    """EBU Tech 3341 / 3342 and the 997 Hz calibration tone: energies from scipy's sequential filter, everything behind them from
    the library's device-free entry points -- and bit for bit the Python replay of the same contract"""
    rate = 48000
    for k, (levels, seconds, want, tol) in enumerate(R.TECH_3341):
        z = _sequential_energies(R.sine(rate, 1000.0, levels, seconds), rate)
        P, _ = bliss.loudness_blocks(z, rate)
        power, lufs = bliss.loudness_gate(P)
        print(f"Tech 3341 case {k + 1}: {lufs:.3f} LUFS (wanted {want} +- {tol})")
        assert abs(lufs - want) <= tol, (k + 1, lufs)
        assert _same_bits(power, R.gate(R.blocks(z, R.hop(rate))[0])[0])
    z = _sequential_energies(R.sine(rate, 997.0, [0.0], [20.0], channels=1), rate)
    lufs = bliss.loudness_gate(bliss.loudness_blocks(z, rate)[0])[1]
    print(f"997 Hz full-scale sine, one channel: {lufs:.4f} LUFS (wanted -3.01 +- 0.05)")
    assert abs(lufs + 3.01) <= 0.05
    for k, (levels, want, tol) in enumerate(R.TECH_3342):
        z = _sequential_energies(R.sine(rate, 1000.0, levels, [20.0] * len(levels)), rate)
        _, ST = bliss.loudness_blocks(z, rate)
        lra, lo, hi = bliss.loudness_range(ST)
        print(f"Tech 3342 case {k + 1}: LRA {lra:.3f} LU (wanted {want} +- {tol})")
        assert abs(lra - want) <= tol, (k + 1, lra)
        assert _same_bits([lo, hi], R.loudness_range(R.blocks(z, R.hop(rate))[1])[1:])


def test_subblocks_short_songs_and_refusals(bliss):
    from bliss_rs_amd import _ffi

    sub = lambda frames, rate: int(_ffi.call("blissgpu_loudness_subblocks", frames, rate))
    assert R.hop(11025) == 1103 and sub(1103 * 7 + 1102, 11025) == 7 and sub(1103 * 8, 11025) == 8
    assert sub(4410 * 4 - 1, 44100) == 3 and sub(441000, 44100) == 100 and sub(10 ** 6, 8000) == 1250
    assert sub(10 ** 6, 7999) == 0 and sub(10 ** 6, 768001) == 0 and sub(0, 48000) == 0
    # too short: fewer than four sub-blocks, decided without a device
    out = bliss.loudness_batch([np.zeros(4 * 2205 - 1, np.float32), np.zeros((0, 2), np.int16)], [22050, 44100])
    assert all(isinstance(r, bliss.AnalysisError) for r in out)
    out, albums, taps = bliss.loudness_batch([np.zeros(3 * 800, np.int16)], 8000, albums=["a"], return_energies=True)
    assert isinstance(out[0], bliss.AnalysisError) and albums["a"].lufs == -math.inf and albums["a"].true_peak == 0.0
    assert taps[0][0].shape == (1, 3) and not taps[0][0].any()
    assert bliss.loudness_batch([], 44100) == []
    # refused before the device is touched: more than two channels, a rate out of range
    for arrays, rate in (([np.zeros((48000, 3), np.float32)], 48000), ([np.zeros(48000, np.float32)], 7000),
                         ([np.zeros(10, np.float32), np.zeros((96000, 6), np.int16)], 48000)):
        for kwargs in ({}, {"return_energies": True}):
            with pytest.raises(bliss.BlissGpuError) as e:
                bliss.loudness_batch(arrays, rate, **kwargs)
            assert e.value.code == _ffi.ERR_INVALID, (rate, kwargs)
    with pytest.raises(bliss.ProviderError):
        bliss.loudness_batch([np.zeros(10, np.float32)], 48000, albums=["a", "b"])
    ld = bliss.Loudness(lufs=-9.5, range_lu=4.0, sample_peak=0.98, true_peak=1.02, power=0.1)
    assert ld.replaygain() == (-8.5, 1.02) and ld.replaygain(-23.0) == (-13.5, 1.02)


def _song(bliss, path, value):
    d = bliss.FeaturesVersion.LATEST.feature_count()
    return bliss.Song(path=path, analysis=bliss.Analysis(np.full(d, value, np.float32), bliss.FeaturesVersion.LATEST))


def test_loudness_round_trip_through_the_sidecar_table(bliss, tmp_path):
    lib = bliss.library
    db = str(tmp_path / "library.db")
    lib.create_schema(db)
    lib.store_songs(db, [_song(bliss, f"/m/{i}.flac", 0.1 * i) for i in range(4)])
    assert lib.load_loudness(db) == {} and lib.loudness_statistics(db)["count"] == 0  # no table yet, and none is made by reading
    conn = sqlite3.connect(db)
    assert conn.execute("select count(*) from sqlite_master where name = 'gpu_loudness'").fetchone()[0] == 0
    L = bliss.Loudness
    songs = {"/m/2.flac": L(-9.25, 3.5, 0.99, 1.04, 0.1), "/m/0.flac": L(-23.0, 17.0, 0.5, 0.51, 0.005),
             "/m/3.flac": L(-math.inf, 0.0, 0.0, 0.0, 0.0)}
    album = L(-11.0, 9.0, 0.99, 1.04, 0.07)
    lib.store_loudness(db, songs, albums={"/m/2.flac": album, "/m/0.flac": album})
    back = lib.load_loudness(db)
    assert list(back) == ["/m/0.flac", "/m/2.flac", "/m/3.flac"]
    for p, ld in songs.items():
        got, album_lufs, album_peak = back[p]
        assert (got.lufs, got.range_lu, got.sample_peak, got.true_peak) == (ld.lufs, ld.range_lu, ld.sample_peak, ld.true_peak)
        assert (album_lufs, album_peak) == ((-11.0, 1.04) if p != "/m/3.flac" else (None, None))
    assert abs(back["/m/0.flac"][0].power - 10.0 ** ((-23.0 + 0.691) / 10.0)) < 1e-15 and back["/m/3.flac"][0].power == 0.0
    stats = lib.loudness_statistics(conn)
    assert stats["count"] == 3 and stats["silent"] == 1
    assert stats["lufs"] == {"mean": (-23.0 + -9.25) / 2, "min": -23.0, "max": -9.25}
    assert stats["range_lu"] == {"mean": (17.0 + 3.5) / 2, "min": 3.5, "max": 17.0}
    lib.store_loudness(conn, {"/m/2.flac": L(-14.0, 6.0, 0.7, 0.71, 0.03)})  # replaced, through an open connection
    assert lib.load_loudness(conn)["/m/2.flac"][0].lufs == -14.0 and lib.load_loudness(conn)["/m/2.flac"][1] is None
    cols = [(r[1], r[2].upper(), r[5]) for r in conn.execute("pragma table_info(gpu_loudness)")]
    assert cols == [("song_id", "INTEGER", 1), ("version", "INTEGER", 0)] + [(c, "REAL", 0) for c in (
        "lufs", "range_lu", "sample_peak", "true_peak", "album_lufs", "album_peak")]
    assert set(conn.execute("select version from gpu_loudness").fetchall()) == {(bliss.LOUDNESS_VERSION,)}
    conn.execute("update gpu_loudness set version = 2 where song_id = 1")  # another contract's figures are not this one's
    conn.commit()
    assert list(lib.load_loudness(conn)) == ["/m/2.flac", "/m/3.flac"]
    with pytest.raises(bliss.ProviderError):
        lib.store_loudness(conn, {"/m/none.flac": L(-10.0, 1.0, 0.1, 0.1, 0.1)})
    conn.close()
    assert len(lib.load_songs(db)) == 4  # the crate's tables are as they were


def _check_program(exe, tmp, env=None):
    """every gate input, blocks of three shapes and the tables of every rate through the program, against the Python replay"""
    words, want = [], []
    for values in _gate_inputs().values():
        words += [0.0, float(len(values))] + list(values)
        want += list(R.gate(values))
        words += [1.0, float(len(values))] + list(values)
        want += list(R.loudness_range(values))
    rng = np.random.default_rng(13)
    for channels, n_sub, H in ((2, 47, 4410), (1, 30, 1103), (2, 4, 800), (1, 3, 4800), (1, 0, 4800)):
        z = rng.uniform(0.0, 50.0, (channels, n_sub))
        words += [2.0, float(channels), float(n_sub), float(H)] + z.reshape(-1).tolist()
        P, ST = R.blocks(z, H) if n_sub else ([], [])
        want += P + ST
    tables = []
    for rate in RATES + (48000,):
        words += [3.0, float(rate)]
        tables.append((len(want), rate))
        want += [0.0] * 62
    src, dst = tmp / "in.f64", tmp / "out.f64"
    np.asarray(words, np.float64).tofile(src)
    out = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, (out.returncode, out.stdout[-500:], out.stderr[-3000:])
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    got = np.fromfile(dst, np.float64)
    assert got.size == len(want)
    want = np.asarray(want, np.float64)
    logs = np.zeros(want.size, bool)  # lufs and range_lu pass through log10
    at = 0
    for values in _gate_inputs().values():
        logs[at + 1] = logs[at + 2] = True
        at += 5
    for at, rate in tables:
        row = got[at:at + 62]
        assert np.abs(row[:10] - R.kweighting(rate)).max() <= 1e-15 * np.abs(R.kweighting(rate)).max()
        assert row[10] == R.peak_factor(rate) and np.abs(row[11:60] - R.peak_filter(R.peak_factor(rate))).max() <= 1e-15
        assert row[60] == R.hop(rate) and row[61] == 1000000 // R.hop(rate)
        want[at:at + 62] = row
    assert _same_bits(got[~logs], want[~logs])
    assert all(_close(g, w) for g, w in zip(got[logs], want[logs]))


def test_loudness_gate_header_against_the_replay(tmp_path):
    exe = tmp_path / "test_loudness_gate"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", SRC, "-o", str(exe)])
    _check_program(exe, tmp_path)


def test_loudness_gate_header_under_address_and_ub_sanitizer(tmp_path):
    """the same stand-alone program built with -fsanitize=address,undefined: same bits, exit 0, no report"""
    exe = tmp_path / "test_loudness_gate_san"
    cxx = SAN_CXX if os.path.exists(SAN_CXX) else "g++"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", SRC, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    _check_program(exe, tmp_path, env)


def test_loudness_gate_header_is_device_free():
    text = open(HPP).read()
    assert "hip" not in re.sub(r"//[^\n]*", "", text).lower() and "__device__" not in text
