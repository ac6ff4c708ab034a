"""GPU tests of the FLAC path (-m gpu): compressed files in, PCM and feature rows out, with no tolerance anywhere -- FLAC is
lossless, the samples of the crafted streams are known before encoding and the fixtures carry their MD5.

The same crafted and malformed sets have been through the stand-alone host build of the frame decoder, plain and under
AddressSanitizer + UBSan (tests/test_flac_host.py), before they come here; nothing is mutated on the GPU."""
import ctypes as C
import hashlib
import os
import sys
import zlib

import numpy as np
import pytest

from conftest import FEATURE_TOL, GOLDEN, decoded_audio

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_craft  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURES = ["s32_mono_44_1_kHz.flac", "s32_stereo_44_1_kHz.flac", "testcue.flac", "tone_11080Hz.flac", "s16_mono_22_5kHz.flac"]


@pytest.fixture(scope="module")
def bliss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import bliss_rs_amd

    return bliss_rs_amd


@pytest.fixture(scope="module")
def ctx(bliss):
    c = bliss.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fixture_rows(bliss):
    """analyze_flac_batch on the fixtures, ONCE"""
    return bliss.analyze_flac_batch([os.path.join(GOLDEN, n) for n in FIXTURES])


def _adler(x):
    return zlib.adler32(np.ascontiguousarray(x, dtype="<f4").tobytes()) & 0xFFFFFFFF


def _expected_pcm(samples, bps):
    return (samples << ((32 if bps > 16 else 16) - bps)).astype(np.int32 if bps > 16 else np.int16)


def _shape(pcm, samples):
    return pcm.reshape(len(pcm), -1)


def test_whole_crafted_set_in_one_call(bliss, ctx):
    crafted = flac_craft.crafted_set()
    default = bliss.Context.default()
    before = default.flac_slow_songs()
    res = bliss.analyze_flac_batch([data for _, data, *_ in crafted])
    assert [name for (name, *_), r in zip(crafted, res) if isinstance(r, bliss.DecodingError)] == []
    # the slow road was taken once: by the fooling stream
    assert default.flac_slow_songs() - before == 1
    # the PCM of the SAME batch shape -- one upload, one table, one launch for all 64 streams, wavefronts that span songs
    batch = bliss.flac_decode_batch([data for _, data, *_ in crafted])
    assert default.flac_slow_songs() - before == 2
    for (name, _, samples, bps, _), got in zip(crafted, batch):
        assert not isinstance(got, bliss.BlissError), name
        assert got[1:] == (44100, bps) and np.array_equal(got[0], _expected_pcm(samples, bps)), name
    long_enough = [name for (name, _, s, _, _), r in zip(crafted, res) if len(s) // 2 >= 8192 + 64 and isinstance(r, bliss.BlissError)]
    assert long_enough == []
    for name, data, samples, bps, table in crafted:
        pcm, rate, status, end, tab = ctx.flac_decode(data, return_frames=True)
        ctx.synchronize()
        stops = end.cpu().numpy() + 2 - (tab[:, 0] + tab[:, 1]).astype(np.int64)
        sound = bool((status == 0).all()) and (stops[:-1] == 0).all() and stops[-1] == (-128 if name == "trailing_id3v1" else 0)
        assert rate == 44100 and sound == (name != flac_craft.FOOLING), (name, status.cpu().tolist())
        if name == flac_craft.FOOLING:   # ... whose PCM is exact too, through the verified table
            assert tab.tolist() != [list(r) for r in table]
            pcm, rate, status, end, tab = ctx.flac_decode(data, verified=True, return_frames=True)
            assert status.cpu().tolist() == [0] * len(table) and tab.tolist() == [list(r) for r in table]
        assert np.array_equal(_shape(pcm.cpu().numpy(), samples), _expected_pcm(samples, bps)), name
    # the host convenience takes the same road by itself
    fool = next(c for c in crafted if c[0] == flac_craft.FOOLING)
    pcm, rate, bps = bliss.flac_decode(fool[1])
    assert np.array_equal(pcm, _expected_pcm(fool[2], fool[3])) and default.flac_slow_songs() - before == 3
    pcm, rate = ctx.flac_decode(fool[1])
    assert np.array_equal(_shape(pcm.cpu().numpy(), fool[2]), _expected_pcm(fool[2], fool[3]))


def test_fixtures_decode_to_their_md5_and_the_reference_adler32(bliss, ctx, literals):
    from bliss_rs_amd import _ffi

    for name in FIXTURES:
        data = open(os.path.join(GOLDEN, name), "rb").read()
        info = np.zeros(_ffi.FLAC_INFO_WORDS, np.uint64)
        buf = np.frombuffer(data, np.uint8)
        assert _ffi.lib().blissgpu_flac_info(C.c_void_p(buf.ctypes.data), len(data), info.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
        bps = int(info[2])
        pcm, rate, status, end, tab = ctx.flac_decode(data, return_frames=True)
        ctx.synchronize()
        assert status.cpu().tolist() == [0] * len(tab) and rate == int(info[0]) and pcm.shape[0] == int(info[3]), name
        host = pcm.cpu().numpy()
        plain = (host.astype(np.int64) >> ((32 if bps > 16 else 16) - bps)).reshape(-1)
        md5 = hashlib.md5(plain.astype("<i8").view(np.uint8).reshape(-1, 8)[:, :(bps + 7) // 8].tobytes()).digest()
        assert md5 == info[8:10].tobytes(), name
        want, want_rate = decoded_audio(name)
        assert want_rate == rate and host.dtype == want.dtype and np.array_equal(host, want), name
        if name == "s16_mono_22_5kHz.flac":
            assert _adler(host.astype(np.float32) / np.float32(32768.0)) == 0x5E01930B
        if name in ("s32_mono_44_1_kHz.flac", "s32_stereo_44_1_kHz.flac"):
            mono = ctx.pcm_decode(pcm, rate)
            ctx.synchronize()
            assert _adler(mono.cpu().numpy()) == int(literals["resample"]["adler32"][name], 16) == {"s32_mono_44_1_kHz.flac": 0xA0F8B8AF,
                                                                                                "s32_stereo_44_1_kHz.flac": 0xBBCBA1CF}[name]


def test_rows_equal_the_decoded_batch_bit_for_bit(bliss, fixture_rows, literals):
    decoded = [decoded_audio(n) for n in FIXTURES]
    ref = bliss.analyze_decoded_batch([d[0] for d in decoded], [d[1] for d in decoded])
    for name, got, want in zip(FIXTURES, fixture_rows, ref):
        assert not isinstance(got, bliss.BlissError) and not isinstance(want, bliss.BlissError), name
        assert np.array_equal(got.as_arr1().view(np.uint32), want.as_arr1().view(np.uint32)), name
    golden = fixture_rows[FIXTURES.index("s16_mono_22_5kHz.flac")].as_arr1()
    exp = np.array(literals["analysis_v2_s16_mono_22_5kHz"]["values"], np.float32)
    assert np.abs(golden - exp).max() < FEATURE_TOL, golden - exp


def test_cue_tracks_from_the_flac_file(bliss, ctx, literals):
    cue = literals["resample"]["cue"]
    secs = [tuple(msf) for msf in cue["index_mm_ss_ff"]]
    res = bliss.cue.analyze_cue_tracks(ctx, os.path.join(GOLDEN, cue["file"]), 0, secs)
    assert len(res) == 3
    for r, exp in zip(res, cue["tracks"]):
        assert np.abs(r.as_arr1() - np.array(exp, np.float32)).max() < FEATURE_TOL
    samples, rate = decoded_audio(cue["file"])
    same = bliss.cue.analyze_cue_tracks(ctx, samples, rate, secs)
    for a, b in zip(res, same):
        assert np.array_equal(a.as_arr1().view(np.uint32), b.as_arr1().view(np.uint32))


def test_malformed_streams_between_well_formed_songs(bliss, fixture_rows):
    bad = flac_craft.malformed_set()
    good = [os.path.join(GOLDEN, n) for n in ("tone_11080Hz.flac", "s16_mono_22_5kHz.flac")]
    batch = [good[0]] + [data for _, data in bad[:len(bad) // 2]] + [good[1]] + [data for _, data in bad[len(bad) // 2:]] + [good[0]]
    res = bliss.analyze_flac_batch(batch)
    alone = bliss.analyze_flac_batch(good)
    errors = [r for r in res if isinstance(r, bliss.BlissError)]
    assert len(errors) == len(bad) and all(isinstance(e, bliss.DecodingError) for e in errors)
    kept = [r for r in res if not isinstance(r, bliss.BlissError)]
    assert len(kept) == 3
    for got, want in zip(kept, [alone[0], alone[1], alone[0]]):
        assert np.array_equal(got.as_arr1().view(np.uint32), want.as_arr1().view(np.uint32))
    for name, want in zip(("tone_11080Hz.flac", "s16_mono_22_5kHz.flac"), alone):
        assert np.array_equal(want.as_arr1().view(np.uint32), fixture_rows[FIXTURES.index(name)].as_arr1().view(np.uint32))
    for name, data in bad:
        with pytest.raises(bliss.DecodingError):
            bliss.flac_decode(data)
    mixed = bliss.flac_decode_batch([good[0]] + [data for _, data in bad] + [good[1]])
    assert [isinstance(m, bliss.DecodingError) for m in mixed] == [False] + [True] * len(bad) + [False]
    for path, got in zip(good, (mixed[0], mixed[-1])):
        want, rate = decoded_audio(os.path.basename(path))
        assert got[1] == rate and np.array_equal(got[0][:, 0], want)


def test_a_song_that_claims_more_pcm_than_the_workspace_is_refused_alone(bliss, fixture_rows):
    # 40 CONSTANT frames of 65 535 samples x 8 channels at 24 bits: a few hundred bytes that claim 84 MB of PCM
    huge, _ = flac_craft.stream(np.zeros((65535 * 40, 8), np.int64), 24, dict(blocksize=65535, subframes=dict(type="constant")))
    assert len(huge) < 4096
    default = bliss.Context.default()
    limit = default.workspace_limit()
    default.set_workspace_limit(48 << 20)
    try:
        tone = os.path.join(GOLDEN, "tone_11080Hz.flac")
        res = bliss.analyze_flac_batch([tone, huge, tone])
        dec = bliss.flac_decode_batch([tone, huge])
    finally:
        default.set_workspace_limit(limit)
    assert isinstance(res[1], bliss.DecodingError) and isinstance(dec[1], bliss.DecodingError) and not isinstance(dec[0], bliss.BlissError)
    want = fixture_rows[FIXTURES.index("tone_11080Hz.flac")].as_arr1().view(np.uint32)
    assert np.array_equal(res[0].as_arr1().view(np.uint32), want) and np.array_equal(res[2].as_arr1().view(np.uint32), want)


def test_flac_decoder_analyze_paths(bliss, fixture_rows, tmp_path):
    paths = []
    for n in FIXTURES:
        p = tmp_path / n
        p.write_bytes(open(os.path.join(GOLDEN, n), "rb").read())
        paths.append(str(p))
    garbage = tmp_path / "garbage.flac"
    garbage.write_bytes(bytes(range(256)) * 64)
    paths.insert(2, str(garbage))
    missing = str(tmp_path / "missing.flac")
    paths.append(missing)
    out = list(bliss.FlacDecoder.analyze_paths(paths))
    assert sorted(p for p, _ in out) == sorted(paths) and len(out) == len(paths)
    by_path = dict(out)
    assert isinstance(by_path[str(garbage)], bliss.DecodingError) and isinstance(by_path[missing], bliss.DecodingError)
    for n, row in zip(FIXTURES, fixture_rows):
        song = by_path[str(tmp_path / n)]
        assert isinstance(song, bliss.Song) and np.array_equal(song.analysis.as_arr1().view(np.uint32), row.as_arr1().view(np.uint32)), n
    tagged = by_path[str(tmp_path / "s16_mono_22_5kHz.flac")]
    assert (tagged.artist, tagged.title, tagged.track_number, tagged.genre) == ("David TMX", "Renaissance", 2, "Pop")
    one = bliss.FlacDecoder.song_from_path(str(tmp_path / "s16_mono_22_5kHz.flac"))
    assert np.array_equal(one.analysis.as_arr1().view(np.uint32), tagged.analysis.as_arr1().view(np.uint32))
