"""CPU tests of the FLAC checks (-m "not gpu"): flac_verify.hpp -- the frame CRC-16 as the 64 lanes of flac_crc_kernel compute
it, the MD5 as flac_md5_kernel computes it -- built as a stand-alone host program (tests/cpp/test_flac_verify.cpp), plain and
under AddressSanitizer + UBSan, in exact-size buffers; and the new symbols in the header, the ffi table and the Rust binding.

The streams are tests/flac_craft.py's: its writer computes every CRC-16 with its own table and every MD5 with hashlib."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import flac_craft  # noqa: E402

FIXTURES = ["s32_mono_44_1_kHz.flac", "s32_stereo_44_1_kHz.flac", "testcue.flac", "tone_11080Hz.flac", "s16_mono_22_5kHz.flac", "no_tags.flac"]
SAN_CXX = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "cpp", "test_flac_verify.cpp")
BAD_STREAM, BAD_CRC16, BAD_MD5, MD5_UNCHECKED = 1, 2, 4, 8
RFC1321 = [b"", b"a", b"abc", b"message digest", b"abcdefghijklmnopqrstuvwxyz",
           b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", b"1234567890" * 8]
RFC1321_DIGESTS = ["d41d8cd98f00b204e9800998ecf8427e", "0cc175b9c0f1b6a831c399e269772661", "900150983cd24fb0d6963f7d28e17f72",
                   "f96b697d7cb7938d525a2f31aaf161d0", "c3fcd3d76192e4007dfb496cca67e13b", "d174ab98d277d9f5a5611c2c9f419d9f",
                   "57edf4a22be3c955ac49da2e2107b67a"]


def _message(samples, bps):
    """the bytes FLAC's MD5 covers: interleaved, little-endian, ceil(bps / 8) bytes per sample"""
    return np.asarray(samples, np.int64).astype("<i8").reshape(-1).view(np.uint8).reshape(-1, 8)[:, :(bps + 7) // 8].tobytes()


def _device_pcm(samples, bps):
    """what flac_decode_kernel leaves: int16 = sample << (16 - bps) up to 16 bits, int32 = sample << (32 - bps) above"""
    a = np.asarray(samples, np.int64)
    return (a << (32 - bps)).astype("<i4") if bps > 16 else (a << (16 - bps)).astype("<i2")


def _pcm_cases():
    """(name, samples [n, channels], bps): every depth class, 1 - 3 channels, negative and extreme samples, lengths around the
    block edges of each sample width"""
    rng = np.random.default_rng(1321)
    out = []
    for bps in (8, 12, 16, 20, 24):
        lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
        for ch in (1, 2, 3):
            for n in (0, 1, 5, 21, 22, 43, 64, 97):
                a = rng.integers(lo, hi + 1, size=(n, ch))
                if n >= 5:
                    a[0, 0], a[1, 0], a[2, 0], a[3, 0] = lo, hi, -1, 0
                out.append((f"b{bps}_c{ch}_n{n}", a, bps))
    return out


def _build(exe, sanitize):
    if sanitize:
        subprocess.check_call([SAN_CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               SRC, "-o", str(exe)])
    else:
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", str(exe)])
    return exe


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    """every crafted and malformed stream, the MD5 inputs, and the stand-alone program built with g++"""
    d = tmp_path_factory.mktemp("flac_verify")
    for name, data, *_ in flac_craft.crafted_set():
        (d / f"good_{name}.flac").write_bytes(data)
    for name, data in flac_craft.malformed_set():
        (d / f"bad_{name}.flac").write_bytes(data)
    rng = np.random.default_rng(200)
    (d / "messages.bin").write_bytes(rng.integers(0, 256, size=sum(range(201)), dtype=np.uint8).tobytes())
    for name, a, bps in _pcm_cases():
        (d / f"{name}.pcm").write_bytes(_device_pcm(a, bps).tobytes())
    _build(d / "test_flac_verify", False)
    return d


def _run(exe, args, env=None):
    out = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, (args[:2], out.stdout[-500:], out.stderr[-3000:])
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    return out.stdout


def _frame_rows(name, table):
    rows = [(off, nb) for off, nb, _, _ in table]
    if name == "trailing_id3v1":   # (its last row runs over the 128-byte tag to the end of the data; the frame itself does not)
        rows[-1] = (rows[-1][0], rows[-1][1] - 128)
    return ",".join(f"{o}:{n}" for o, n in rows)


def _check_crc(exe, env=None):
    kv = dict(line.split("=") for line in _run(exe, ["--crc", 7], env).split())
    assert int(kv["crc_cases"]) == 8 * 1100 + 2000 + 301 + 71


def _check_frames(exe, workdir, env=None):
    crafted = flac_craft.crafted_set()
    assert len(crafted) == 64
    for name, data, _, _, table in crafted:
        for off, nb, _, _ in table[:-1]:   # the writer's own CRC, by the writer's own table
            assert flac_craft.crc16(data[off:off + nb]) == 0, name
        kv = dict(line.split("=") for line in _run(exe, ["--frames", workdir / f"good_{name}.flac", _frame_rows(name, table)], env).split())
        assert int(kv["frames"]) == len(table) and int(kv["nonzero"]) == 0, name


def _verdicts(exe, paths, env=None):
    out = {}
    for line in _run(exe, ["--verdict"] + list(paths), env).splitlines():
        name, flags, first_bad, md5 = line.split(" ")
        out[name] = (int(flags), int(first_bad), None if md5 == "-" else md5)
    return out


def _check_verdicts(exe, workdir, env=None):
    crafted = flac_craft.crafted_set()
    got = _verdicts(exe, sorted(workdir.glob("*.flac")), env)
    assert len(got) == len(crafted) + len(flac_craft.malformed_set())
    for name, data, samples, bps, _ in crafted:
        flags, first_bad, md5 = got[f"good_{name}.flac"]
        if name == "md5_zero" or name.startswith("variable_past"):   # no digest to hold / cut out of a longer stream
            assert (flags, first_bad, md5) == (MD5_UNCHECKED, 0xFFFFFFFF, None), name
        else:
            assert (flags, first_bad) == (0, 0xFFFFFFFF) and md5 == hashlib.md5(_message(samples, bps)).hexdigest(), name
    for name, _ in flac_craft.malformed_set():   # a verdict, never a report from the sanitizer
        flags, first_bad, md5 = got[f"bad_{name}.flac"]
        assert flags == BAD_STREAM | MD5_UNCHECKED and md5 is None, name


def _check_md5(exe, workdir, env=None):
    digests = _run(exe, ["--md5-strings"], env).split()
    assert digests == [hashlib.md5(m).hexdigest() for m in RFC1321] == RFC1321_DIGESTS
    blob = (workdir / "messages.bin").read_bytes()
    want, pos = [], 0
    for n in range(201):
        want.append(hashlib.md5(blob[pos:pos + n]).hexdigest())
        pos += n
    assert _run(exe, ["--md5-file", workdir / "messages.bin"], env).split() == want
    cases = _pcm_cases()
    got = _run(exe, ["--md5-pcm"] + [f"{workdir / name}.pcm:{bps}" for name, _, bps in cases], env).split()
    assert len(got) == len(cases)
    for (name, a, bps), digest in zip(cases, got):
        assert digest == hashlib.md5(_message(a, bps)).hexdigest(), name
    assert any((a < 0).any() for _, a, _ in cases)


def test_frame_crc_lane_by_lane_equals_the_byte_serial_crc(workdir):
    _check_crc(workdir / "test_flac_verify")


def test_every_crafted_frame_has_remainder_zero_over_its_crc_field(workdir):
    _check_frames(workdir / "test_flac_verify", workdir)


def test_crafted_streams_verify_and_malformed_streams_end_in_a_verdict(workdir):
    _check_verdicts(workdir / "test_flac_verify", workdir)


def test_fixtures_verify_on_the_host(workdir):
    """the six fixtures were written by other encoders: each holds a nonzero MD5, and the lanes' CRC and the packer's MD5 agree"""
    got = _verdicts(workdir / "test_flac_verify", [os.path.join(GOLDEN, n) for n in FIXTURES])
    for name in FIXTURES:
        data = open(os.path.join(GOLDEN, name), "rb").read()
        p = data.index(b"fLaC") + 8
        assert data[p + 18:p + 34] != bytes(16), name
        assert got[name] == (0, 0xFFFFFFFF, data[p + 18:p + 34].hex()), name


def test_a_flipped_bit_is_a_crc_verdict_on_the_host(workdir, tmp_path):
    """the host twin of the device test: a bit inside a VERBATIM sample of frame 3 moves no boundary and fails frame 3's CRC"""
    data, table = flac_craft.stream(flac_craft._rng_samples(5, 6 * 16, 1, 16), 16, dict(blocksize=16, subframes=dict(type="verbatim")))
    blob = bytearray(data)
    blob[table[3][0] + table[3][1] - 5] ^= 0x10   # the second-to-last sample of the frame
    (tmp_path / "flip.flac").write_bytes(bytes(blob))
    (tmp_path / "sound.flac").write_bytes(data)
    got = _verdicts(workdir / "test_flac_verify", [tmp_path / "flip.flac", tmp_path / "sound.flac"])
    assert got["flip.flac"] == (BAD_CRC16 | MD5_UNCHECKED, 3, None)
    assert got["sound.flac"][:2] == (0, 0xFFFFFFFF)


def test_md5_block_function_and_packer_against_hashlib(workdir):
    _check_md5(workdir / "test_flac_verify", workdir)


@pytest.mark.skipif(not os.path.exists(SAN_CXX), reason="needs the ROCm clang for -fsanitize=address,undefined")
def test_checks_under_address_and_ub_sanitizer(workdir):
    """The same stand-alone program built with -fsanitize=address,undefined, the environment passed through as it is: every load of the lane
    routine and of the packer lies inside the exact-size buffers, for the whole crafted set, the malformed set and every CRC
    and MD5 case above.  Exit 0, no report."""
    exe = _build(workdir / "test_flac_verify_san", True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    _check_crc(exe, env)
    _check_verdicts(exe, workdir, env)
    _check_md5(exe, workdir, env)
    name, data, _, _, table = next(c for c in flac_craft.crafted_set() if c[0] == "bs4608")
    kv = dict(line.split("=") for line in _run(exe, ["--frames", workdir / f"good_{name}.flac", _frame_rows(name, table)], env).split())
    assert int(kv["frames"]) == len(table) and int(kv["nonzero"]) == 0


def test_flac_verify_symbols_in_header_ffi_and_rust_binding():
    from bliss_rs_amd import _ffi

    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "gpu.rs")).read()
    names = ["blissgpu_flac_verify_batch", "blissgpu_analyze_batch_flac_verified", "blissgpu_flac_crc16_device", "blissgpu_flac_md5_device"]
    lib = _ffi.lib()
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert f"pub fn {name}(" in rust, name
        assert name in _ffi.SIGNATURES and hasattr(lib, name), name
    _vp, u64, u32, u64p, u32p, i32p = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    assert _ffi.SIGNATURES["blissgpu_flac_verify_batch"] == (C.c_int, [C.POINTER(_vp), u64p, u32, u32, u32p, u32p, _vp])
    assert _ffi.SIGNATURES["blissgpu_analyze_batch_flac_verified"] == (C.c_int, [C.POINTER(_vp), u64p, u32, u32, u32, _vp, i32p, u32p, u32p])
    assert _ffi.SIGNATURES["blissgpu_flac_crc16_device"] == (C.c_int, [_vp, _vp, u64, u64p, u64, _vp, _vp, _vp])
    assert _ffi.SIGNATURES["blissgpu_flac_md5_device"] == (C.c_int, [_vp, _vp, u64p, _vp])
    consts = {"FLAC_CHECK_CRC16": 1, "FLAC_CHECK_MD5": 2, "FLAC_BAD_STREAM": 1, "FLAC_BAD_CRC16": 2, "FLAC_BAD_MD5": 4, "FLAC_MD5_UNCHECKED": 8}
    for name, value in consts.items():
        assert re.search(r"#define BLISSGPU_%s\s+%du\b" % (name, value), header), name
        assert f"pub const BLISSGPU_{name}: u32 = {value};" in rust, name
        assert getattr(_ffi, name) == value, name
    # the unverified signatures are as they were
    assert _ffi.SIGNATURES["blissgpu_analyze_batch_flac"] == (C.c_int, [C.POINTER(_vp), u64p, u32, u32, _vp, i32p])
    # device-free argument checks: an unknown check bit is refused before anything touches a device
    blob = np.zeros(8, np.uint8)
    files = (C.c_void_p * 1)(blob.ctypes.data)
    sizes = np.array([blob.size], np.uint64)
    flags = np.zeros(1, np.uint32)
    rc = lib.blissgpu_flac_verify_batch(files, sizes.ctypes.data_as(u64p), 1, 4, flags.ctypes.data_as(u32p), None, None)
    assert rc == _ffi.ERR_INVALID and b"unknown check" in lib.blissgpu_last_error()
    rows, status = np.zeros(23, np.float32), np.zeros(1, np.int32)
    rc = lib.blissgpu_analyze_batch_flac_verified(files, sizes.ctypes.data_as(u64p), 1, 2, 8, rows.ctypes.data, status.ctypes.data_as(i32p),
                                                  flags.ctypes.data_as(u32p), None)
    assert rc == _ffi.ERR_INVALID and b"unknown check" in lib.blissgpu_last_error()
    rc = lib.blissgpu_flac_verify_batch(None, None, 1, 1, flags.ctypes.data_as(u32p), None, None)
    assert rc == _ffi.ERR_INVALID and b"NULL argument" in lib.blissgpu_last_error()
