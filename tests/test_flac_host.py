"""CPU tests of the FLAC path (-m "not gpu"): the host half (STREAMINFO, both frame-table modes), the frame decoder the device
runs -- built here as a stand-alone host program, plain and under AddressSanitizer + UBSan --, the ABI and the tags.

The inputs are tests/flac_craft.py's crafted set (the smallest shapes at which a decoder can go wrong; the samples are known
before encoding) and the FLAC fixtures under tests/golden/.  Every crafted stream is first decoded by the independent
pure-Python reader tests/tools/flac_decode.py and has to give its samples back: that holds the writer."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

import flac_craft  # noqa: E402
import flac_decode  # noqa: E402

FIXTURES = ["s32_mono_44_1_kHz.flac", "s32_stereo_44_1_kHz.flac", "testcue.flac", "tone_11080Hz.flac", "s16_mono_22_5kHz.flac", "no_tags.flac"]
SAN_CXX = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "cpp", "test_flac.cpp")


def _kv(text):
    return dict(line.split("=", 1) for line in text.splitlines() if "=" in line)


def _table_text(table):
    return ",".join(":".join(str(int(v)) for v in row) for row in table)


@pytest.fixture(scope="module")
def crafted():
    return flac_craft.crafted_set()


@pytest.fixture(scope="module")
def workdir(tmp_path_factory, crafted):
    """every crafted and malformed stream as a file, and the stand-alone program built with g++"""
    d = tmp_path_factory.mktemp("flac")
    for name, data, *_ in crafted:
        (d / f"good_{name}.flac").write_bytes(data)
    for name, data in flac_craft.malformed_set():
        (d / f"bad_{name}.flac").write_bytes(data)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", str(d / "test_flac")])
    return d


@pytest.fixture(scope="module")
def fixture_walk():
    """the fixtures through flac_decode.py, ONCE: name -> (samples [n, channels], rate, bps, block sizes of the frames it walked)"""
    out = {}
    inner = flac_decode._subframe
    for name in FIXTURES:
        sizes = []

        def recording(br, blocksize, bps, _sizes=sizes):
            _sizes.append(blocksize)
            return inner(br, blocksize, bps)

        flac_decode._subframe = recording
        try:
            a, rate, bps = flac_decode.decode_flac(os.path.join(GOLDEN, name))
        finally:
            flac_decode._subframe = inner
        out[name] = (a, rate, bps, sizes[::a.shape[1]])
    return out


def _lib_index(data, verified):
    from bliss_rs_amd import _ffi

    L = _ffi.lib()
    buf = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
    info = np.zeros(_ffi.FLAC_INFO_WORDS, np.uint64)
    u64p = C.POINTER(C.c_uint64)
    rc = L.blissgpu_flac_info(C.c_void_p(buf.ctypes.data), len(data), info.ctypes.data_as(u64p))
    if rc:
        return rc, None, None
    n = C.c_uint64(0)
    L.blissgpu_flac_index(C.c_void_p(buf.ctypes.data), len(data), verified, None, None, 0, C.byref(n))
    table = np.zeros((max(1, n.value), 4), np.uint64)
    rc = L.blissgpu_flac_index(C.c_void_p(buf.ctypes.data), len(data), verified, info.ctypes.data_as(u64p), table.ctypes.data_as(u64p),
                               n.value, C.byref(n))
    return rc, info, table[:n.value]


def test_the_writer_is_held_by_the_independent_reader(crafted, tmp_path):
    assert len(crafted) >= 60
    for name, data, samples, bps, _ in crafted:
        blob = bytearray(data[data.index(b"fLaC"):])   # (flac_decode.py knows neither ID3v2 nor an unknown total)
        if name == "total_unknown":
            assert int.from_bytes(blob[18:26], "big") & ((1 << 36) - 1) == 0
            blob[18:26] = (int.from_bytes(blob[18:26], "big") | len(samples)).to_bytes(8, "big")
        path = tmp_path / "x.flac"
        path.write_bytes(bytes(blob))
        got, rate, got_bps = flac_decode.decode_flac(str(path))
        assert got_bps == bps and got.shape == samples.shape and np.array_equal(got, samples), name


def test_info_and_both_index_modes_against_the_writers_table(crafted):
    differing = []
    for name, data, samples, bps, table in crafted:
        rc_f, info, fast = _lib_index(data, 0)
        rc_v, info_v, exact = _lib_index(data, 1)
        assert rc_f == 0 and rc_v == 0, name
        assert len(data) == table[-1][0] + table[-1][1], name
        assert (int(info[0]), int(info[1]), int(info[2])) == (44100, samples.shape[1], bps), name
        assert int(info[3]) == len(samples) and int(info[7]) == table[0][0], name
        md5 = hashlib.md5(samples.astype("<i8").reshape(-1).view(np.uint8).reshape(-1, 8)[:, :(bps + 7) // 8].tobytes()).digest()
        assert info[8:10].tobytes() == (bytes(16) if name == "md5_zero" else md5), name
        assert exact.tolist() == [list(r) for r in table], name
        if fast.tolist() != exact.tolist():
            differing.append(name)
    # a header-shaped run of bytes inside a frame fools the fast filter -- there, and nowhere else
    assert differing == [flac_craft.FOOLING]
    stream_base = {name: int(_lib_index(data, 0)[1][10]) for name, data, *_ in crafted if name.startswith("variable_past")}
    assert stream_base == {"variable_past_2_31": (1 << 31) - 20, "variable_past_2_35": (1 << 35) + 12345}


def test_index_of_the_fixtures_is_the_walk_of_the_python_reader(fixture_walk):
    for name, (samples, rate, bps, sizes) in fixture_walk.items():
        data = open(os.path.join(GOLDEN, name), "rb").read()
        for verified in (0, 1):
            rc, info, table = _lib_index(data, verified)
            assert rc == 0 and (int(info[0]), int(info[1]), int(info[2]), int(info[3])) == (rate, samples.shape[1], bps, len(samples)), name
            assert table[:, 3].tolist() == sizes, name
            assert table[:, 2].tolist() == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist(), name
            assert (table[1:, 0] == table[:-1, 0] + table[:-1, 1]).all() and table[-1, 0] + table[-1, 1] == len(data), name
    # ordinary files stay on the fast road: 106 candidates for 106 frames
    assert len(fixture_walk["s32_stereo_44_1_kHz.flac"][3]) == 106


def test_malformed_streams_are_refused_by_the_index_or_left_to_the_decoder():
    refused = {name for name, data in flac_craft.malformed_set() if _lib_index(data, 1)[0] != 0}
    assert {"not_flac", "garbage", "empty", "cut_in_metadata", "cut_in_header", "cut_in_residual", "cut_at_frame_boundary",
            "reserved_assignment", "depth32_frame_only"} <= refused


def test_standalone_decoder_on_the_crafted_set(crafted, workdir):
    for name, data, samples, bps, table in crafted:
        pcm_path = workdir / "out.pcm"
        out = subprocess.run([str(workdir / "test_flac"), str(workdir / f"good_{name}.flac"), str(pcm_path)], capture_output=True, text=True)
        kv = _kv(out.stdout)
        assert out.returncode == 0 and kv["status"] == "0", (name, out.stdout[-400:], out.stderr[-400:])
        pcm = np.fromfile(pcm_path, "<i4" if bps > 16 else "<i2").reshape(-1, samples.shape[1])
        assert np.array_equal(pcm.astype(np.int64), samples << ((32 if bps > 16 else 16) - bps)), name
        md5 = hashlib.md5(samples.astype("<i8").reshape(-1).view(np.uint8).reshape(-1, 8)[:, :(bps + 7) // 8].tobytes()).hexdigest()
        assert kv["md5"] == md5 and (kv["stream_md5"] == md5 or name == "md5_zero"), name
        assert kv["verified"] == _table_text(table), name
        assert (kv["slow"] == "1") == (name == flac_craft.FOOLING), name
        # verified mode checks the last frame's CRC-16 too; behind an ID3v1 tag it is not at the end of the data
        assert (kv["last_crc_ok"] == "1") == (name != "trailing_id3v1"), name


def test_standalone_decoder_on_the_fixtures(workdir, fixture_walk):
    for name, (samples, rate, bps, sizes) in fixture_walk.items():
        pcm_path = workdir / "out.pcm"
        out = subprocess.run([str(workdir / "test_flac"), os.path.join(GOLDEN, name), str(pcm_path)], capture_output=True, text=True)
        kv = _kv(out.stdout)
        assert out.returncode == 0 and kv["status"] == "0" and kv["slow"] == "0", (name, out.stdout[-400:])
        assert kv["md5"] == kv["stream_md5"] and int(kv["total"]) == len(samples), name
        assert kv["fast"] == kv["verified"], name
        pcm = np.fromfile(pcm_path, "<i4" if bps > 16 else "<i2").reshape(-1, samples.shape[1])
        assert np.array_equal(pcm.astype(np.int64), samples << ((32 if bps > 16 else 16) - bps)), name


def test_standalone_decoder_refuses_the_malformed_set(workdir):
    for name, _ in flac_craft.malformed_set():
        out = subprocess.run([str(workdir / "test_flac"), str(workdir / f"bad_{name}.flac")], capture_output=True, text=True)
        assert out.returncode == 0 and int(_kv(out.stdout)["status"]) >= 100, (name, out.stdout[-300:])


@pytest.mark.skipif(not os.path.exists(SAN_CXX), reason="needs the ROCm clang for -fsanitize=address,undefined")
def test_frame_decoder_under_address_and_ub_sanitizer(workdir):
    """Where the bounds of the device routine are proven before it runs on a GPU: the same stand-alone program built with
    -fsanitize=address,undefined, over the whole crafted set, the malformed set and 2 000 seeded mutations (byte flips,
    truncations, duplicated ranges) of three crafted streams.  Every buffer is exact-size: the file plus the 16 bytes of padding
    the decoder is promised, the PCM exactly total x channels samples.  Every input ends in a status; exit 0, no report."""
    exe = workdir / "test_flac_san"
    subprocess.check_call([SAN_CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           SRC, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    mutate = [str(workdir / f"good_{n}.flac") for n in ("lpc13_p12_s10", "span70", "escapes")]
    rest = sorted(str(p) for p in workdir.glob("*.flac") if str(p) not in mutate)
    out = subprocess.run([str(exe), "--fuzz", "1", "2000", "3"] + mutate + rest, capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    kv = _kv(out.stdout.replace(" ", "\n"))
    n_files = len(mutate) + len(rest)
    assert int(kv["inputs"]) == n_files + 2000 and int(kv["decoded"]) + int(kv["refused"]) == int(kv["inputs"])
    assert int(kv["decoded"]) >= len(flac_craft.crafted_set()) and int(kv["refused"]) >= len(flac_craft.malformed_set())


def test_flac_symbols_in_header_ffi_and_rust_binding():
    import re

    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "gpu.rs")).read()
    names = ["blissgpu_flac_info", "blissgpu_flac_index", "blissgpu_flac_decode_device", "blissgpu_flac_decode",
             "blissgpu_flac_decode_batch", "blissgpu_analyze_batch_flac", "blissgpu_ctx_flac_slow_songs"]
    lib = _ffi.lib()
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert f"pub fn {name}(" in rust, name
        assert name in _ffi.SIGNATURES and hasattr(lib, name), name
    _vp, u64, u32, u64p, i32p = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    assert _ffi.SIGNATURES["blissgpu_flac_info"] == (C.c_int, [_vp, u64, u64p])
    assert _ffi.SIGNATURES["blissgpu_flac_index"] == (C.c_int, [_vp, u64, C.c_int, u64p, u64p, u64, u64p])
    assert _ffi.SIGNATURES["blissgpu_flac_decode_device"] == (C.c_int, [_vp, _vp, u64, u64p, u64, u64p, _vp, _vp, _vp])
    assert _ffi.SIGNATURES["blissgpu_flac_decode"] == (C.c_int, [_vp, u64, _vp, u64, u64p, i32p])
    assert _ffi.SIGNATURES["blissgpu_analyze_batch_flac"] == (C.c_int, [C.POINTER(_vp), u64p, u32, u32, _vp, i32p])
    assert re.search(r"#define BLISSGPU_SONG_DECODE_ERROR 2\b", header) and "BLISSGPU_SONG_DECODE_ERROR: i32 = 2" in rust
    assert _ffi.SONG_DECODE_ERROR == 2 and _ffi.FLAC_INFO_WORDS == 12 and re.search(r"#define BLISSGPU_FLAC_INFO_WORDS 12u", header)


def test_tags_equal_the_literals_of_the_reference_tag_tests():
    import bliss_rs_amd as bliss

    with open(os.path.join(GOLDEN, "flac_tags.json")) as f:
        lit = json.load(f)
    for name in ("s16_mono_22_5kHz.flac", "no_tags.flac"):
        song = bliss.FlacDecoder.decode(os.path.join(GOLDEN, name))
        for key in ("artist", "album_artist", "title", "album", "track_number", "disc_number", "genre"):
            assert getattr(song, key) == lit[name][key], (name, key)
        assert song.flac == open(os.path.join(GOLDEN, name), "rb").read() and song.sample_array.size == 0   # the COMPRESSED bytes
        if "duration_ms" in lit[name]:
            assert abs(song.duration * 1000.0 - lit[name]["duration_ms"]) < lit[name]["duration_tol_ms"]
    with pytest.raises(bliss.DecodingError):
        bliss.FlacDecoder.decode(os.path.join(GOLDEN, "no_channel.wav"))


def test_track_numbers_parse_like_rusts_i32():
    from bliss_rs_amd.decoder import _vorbis_track

    assert [_vorbis_track(t) for t in ("2", "02/05", "+7", "-1", "06/24")] == [2, 2, 7, -1, 6]
    assert [_vorbis_track(t) for t in ("", "1_0", " 2", "2 ", "02test/05", "٢", "2147483648", "x/3")] == [None] * 8
