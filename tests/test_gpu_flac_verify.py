"""GPU tests of the FLAC checks (-m gpu): every frame's CRC-16 (flac_crc_kernel, one wavefront per frame) and the stream's MD5
(flac_md5_kernel, one lane per song), opt-in, a verdict per song.  No tolerance anywhere: the writer of tests/flac_craft.py
computes every CRC-16 with its own table and every MD5 with hashlib, and the fixtures carry the MD5 their encoder wrote.

The arithmetic has been through the stand-alone host build, lane by lane, plain and under AddressSanitizer + UBSan
(tests/test_flac_verify_host.py), before it comes here."""
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_craft  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURES = ["s32_mono_44_1_kHz.flac", "s32_stereo_44_1_kHz.flac", "testcue.flac", "tone_11080Hz.flac", "s16_mono_22_5kHz.flac", "no_tags.flac"]
BAD_STREAM, BAD_CRC16, BAD_MD5, MD5_UNCHECKED = 1, 2, 4, 8
VERBATIM = dict(type="verbatim")


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


def _message(samples, bps):
    return np.asarray(samples, np.int64).astype("<i8").reshape(-1).view(np.uint8).reshape(-1, 8)[:, :(bps + 7) // 8].tobytes()


def _streaminfo_md5_at(data):
    return data.index(b"fLaC") + 8 + 18


def _song(seed):
    """a 16-bit mono VERBATIM stream at 22 050 Hz, long enough to analyse: 47 frames of 192 samples"""
    return flac_craft.stream(flac_craft._rng_samples(seed, 9000, 1, 16, 0.5), 16, dict(blocksize=192, subframes=VERBATIM), rate=22050)


@pytest.fixture(scope="module")
def songs():
    """three analysable songs (bytes, table), built ONCE"""
    return [_song(seed) for seed in (201, 202, 203)]


def _flip_sample_bit(data, table, frame, sample=10, bit=0x04):
    """one bit inside a 16-bit VERBATIM sample of a mono frame: 4 header bytes, the frame number, the CRC-8, the subframe's byte"""
    number_bytes = len(flac_craft.utf8_number(frame))
    blob = bytearray(data)
    blob[table[frame][0] + 4 + number_bytes + 1 + 1 + 2 * sample + 1] ^= bit
    return bytes(blob)


def test_sound_streams_pass(bliss):
    crafted = flac_craft.crafted_set()
    assert len(crafted) == 64
    fixtures = [open(os.path.join(GOLDEN, n), "rb").read() for n in FIXTURES]
    before = bliss.Context.default().flac_slow_songs()
    verdicts = bliss.flac_verify_batch([data for _, data, *_ in crafted] + fixtures, md5=True)
    assert len(verdicts) == len(crafted) + len(fixtures)
    assert bliss.Context.default().flac_slow_songs() - before == 1   # the fooling stream passes after its second pass
    for (name, data, samples, bps, table), v in zip(crafted, verdicts):
        assert v.ok and v.stream_ok and v.crc_ok and v.first_bad_frame is None, (name, v)
        if name == "md5_zero" or name.startswith("variable_past"):   # no digest to hold / cut out of a longer stream
            assert v.md5_state == "unchecked" and v.md5 is None, (name, v)
        else:   # ("total_unknown": STREAMINFO's total is 0, the table's count stands; "trailing_id3v1": the decoder's stop position)
            assert v.md5_state == "match" and v.md5 == hashlib.md5(_message(samples, bps)).hexdigest(), (name, v)
            at = _streaminfo_md5_at(data)
            assert v.md5 == data[at:at + 16].hex(), name
    for name, data, v in zip(FIXTURES, fixtures, verdicts[len(crafted):]):
        at = _streaminfo_md5_at(data)
        assert data[at:at + 16] != bytes(16), name
        assert v.ok and v.md5_state == "match" and v.md5 == data[at:at + 16].hex() and v.flags == 0, (name, v)
    # without the MD5 every song is "unchecked" and no digest comes back
    quick = bliss.flac_verify_batch(fixtures, md5=False)
    assert all(v.ok and v.flags == MD5_UNCHECKED and v.md5 is None for v in quick)


def test_a_flipped_sample_bit_passes_unverified_and_fails_the_crc(bliss, songs):
    """a flipped bit in a VERBATIM sample moves no boundary: the unverified call decodes it (that is the default, pinned here),
    verify="crc" refuses it and names frame 3; its neighbours in the call are untouched"""
    (a, _), (b, table), (c, _) = songs
    assert len(table) >= 5
    damaged = _flip_sample_bit(b, table, 3)
    assert damaged != b and len(damaged) == len(b)
    plain = bliss.analyze_flac_batch([a, damaged, c])
    assert all(isinstance(r, bliss.Analysis) and np.isfinite(r.as_arr1()).all() for r in plain)
    sound = bliss.analyze_flac_batch([a, b, c])
    checked = bliss.analyze_flac_batch([a, damaged, c], verify="crc")
    assert isinstance(checked[1], bliss.DecodingError), checked[1]
    assert checked[1].first_bad_frame == 3 and checked[1].flags & BAD_CRC16 and not checked[1].flags & BAD_STREAM
    assert "CRC-16 mismatch in frame 3" in str(checked[1])
    for k in (0, 2):
        assert isinstance(checked[k], bliss.Analysis)
        assert np.array_equal(checked[k].as_arr1().view(np.uint32), plain[k].as_arr1().view(np.uint32)), k
    # checks = 0 is the unverified call; the sound song is the same row with and without the checks
    for verify in ("crc", "md5"):
        again = bliss.analyze_flac_batch([b], verify=verify)
        assert np.array_equal(again[0].as_arr1().view(np.uint32), sound[1].as_arr1().view(np.uint32)), verify


def _flip_cases():
    """200 seeded single-bit flips across the frame bytes of a VERBATIM, a Rice-coded LPC and a stereo side-channel stream"""
    crafted = {name: (data, table) for name, data, _, _, table in flac_craft.crafted_set()}
    verbatim = flac_craft.stream(flac_craft._rng_samples(5, 6 * 16, 1, 16), 16, dict(blocksize=16, subframes=VERBATIM))
    bases = [verbatim, crafted["lpc8_p15_s14"], crafted["span1"]]   # (span1: one frame of 187 samples, side/right)
    rng = np.random.default_rng(16)
    flips = []
    for k in range(200):
        data, table = bases[k % 3]
        lo, hi = table[0][0], table[-1][0] + table[-1][1]
        assert hi == len(data)
        pos, bit = int(rng.integers(lo, hi)), int(rng.integers(0, 8))
        blob = bytearray(data)
        blob[pos] ^= 1 << bit
        flips.append(bytes(blob))
    return [d for d, _ in bases], flips


def test_every_single_bit_flip_is_caught(bliss):
    bases, flips = _flip_cases()
    assert len(flips) == 200 and len(set(flips)) > 150
    verdicts = bliss.flac_verify_batch(bases + flips, md5=False)
    assert all(v.ok for v in verdicts[:3]), verdicts[:3]
    missed = [k for k, v in enumerate(verdicts[3:]) if v.ok or not v.flags & (BAD_STREAM | BAD_CRC16)]
    assert missed == []
    assert sum(1 for v in verdicts[3:] if v.flags & BAD_CRC16) > 50   # most flips move no boundary: only the CRC sees them


def test_crc_field_and_streaminfo_tampering(bliss, ctx, songs):
    data, table = songs[0]
    # a bit of frame 5's CRC-16 field itself: the audio is what it was
    blob = bytearray(data)
    blob[table[5][0] + table[5][1] - 1] ^= 0x01
    crc_hit = bytes(blob)
    # another digest in STREAMINFO: the frames are what they were
    at = _streaminfo_md5_at(data)
    md5_hit = data[:at] + hashlib.md5(b"another stream").digest() + data[at + 16:]
    v_crc, v_md5, v_ok = bliss.flac_verify_batch([crc_hit, md5_hit, data], md5=True)
    assert v_ok.ok and v_ok.md5 == data[at:at + 16].hex()
    assert v_crc.flags == BAD_CRC16 | MD5_UNCHECKED and v_crc.first_bad_frame == 5 and not v_crc.ok and v_crc.stream_ok and v_crc.md5 is None
    assert v_md5.flags == BAD_MD5 and v_md5.crc_ok and v_md5.md5_state == "mismatch" and v_md5.md5 == data[at:at + 16].hex()
    (pcm_hit, *_), (pcm, *_) = bliss.flac_decode_batch([crc_hit, data])
    assert np.array_equal(pcm_hit, pcm)
    d_pcm, rate = ctx.flac_decode(crc_hit)
    assert ctx.flac_md5(d_pcm, 16) == data[at:at + 16].hex()
    # BAD_MD5 under verify="md5" only
    crc_only = bliss.analyze_flac_batch([md5_hit], verify="crc")
    assert isinstance(crc_only[0], bliss.Analysis)
    both = bliss.analyze_flac_batch([md5_hit, data], verify="md5")
    assert isinstance(both[0], bliss.DecodingError) and both[0].flags == BAD_MD5 and "MD5" in str(both[0])
    assert np.array_equal(both[1].as_arr1().view(np.uint32), crc_only[0].as_arr1().view(np.uint32))   # (the same audio)


def test_md5_padding_and_packing_edges(bliss, ctx):
    """message lengths around the 55 / 56 / 63 / 64-byte edges of MD5's padding for each sample width, in one call and in mixed
    order: the lanes of one wavefront run different lengths, widths and depths"""
    cases = [(8, 1, n) for n in (55, 56, 63, 64, 119)] + [(16, 1, n) for n in (27, 28, 32)] + [(24, 1, n) for n in (19, 21, 22, 40, 64)]
    cases += [(12, 2, 37), (20, 2, 37), (12, 2, 16), (20, 2, 11)]
    order = np.random.default_rng(5).permutation(len(cases))
    streams = []
    for k in order:
        bps, ch, n = cases[k]
        s = flac_craft._rng_samples(300 + int(k), n, ch, bps)
        s[0, :] = -(1 << (bps - 1))
        s[n // 2, :] = -1
        assert (s < 0).any()
        streams.append((s, bps, flac_craft.stream(s, bps, dict(blocksize=16, subframes=VERBATIM))[0]))
    verdicts = bliss.flac_verify_batch([data for _, _, data in streams], md5=True)
    for (s, bps, data), v in zip(streams, verdicts):
        assert v.ok and v.md5_state == "match" and v.md5 == hashlib.md5(_message(s, bps)).hexdigest(), (bps, s.shape, v)
    # the device-to-device form sees the raw digest
    s, bps, data = streams[0]
    d_pcm, _ = ctx.flac_decode(data)
    assert ctx.flac_md5(d_pcm, bps) == hashlib.md5(_message(s, bps)).hexdigest()


def test_crc_kernel_geometry(bliss, ctx):
    """frame offsets of every residue mod 8, frame lengths on both sides of one round of the 64 lanes (512 bytes) and of two
    (1 024), a frame count that is no multiple of the 4 wavefronts of a workgroup -- and one damaged frame among them"""
    sizes = list(range(16, 31)) + list(range(498, 505)) + list(range(1008, 1016))
    samples = flac_craft._rng_samples(77, sum(sizes), 1, 8)
    data, table = flac_craft.stream(samples, 8, [dict(blocksize=b, subframes=VERBATIM) for b in sizes], variable=True)
    lengths = [nb for _, nb, _, _ in table]
    assert {off % 8 for off, *_ in table} == set(range(8))
    assert {511, 512, 513} <= set(lengths) and {1023, 1024, 1025} <= set(lengths), lengths
    assert len(table) % 4 != 0
    blob = bytearray(data)
    hit = lengths.index(1024)
    blob[table[hit][0] + 600] ^= 0x80
    for stream, bad in ((data, None), (bytes(blob), hit)):
        pcm, rate, status, end, tab = ctx.flac_decode(stream, return_frames=True)   # (the fast table: CRC-8 and frame numbers only)
        assert tab.tolist() == [list(r) for r in table] and status.cpu().tolist() == [0] * len(table)
        ok = ctx.flac_crc16(stream, tab, status, end)
        ctx.synchronize()
        assert ok.cpu().tolist() == [0 if k == bad else 1 for k in range(len(table))]
    # a frame that did not decode is not checked
    status[2] = 4
    assert ctx.flac_crc16(data, tab, status, end).cpu().tolist()[:4] == [1, 1, -1, 1]


def test_decoder_interface_reports_the_check_and_the_frame(bliss, songs, tmp_path):
    (a, _), (b, table), _ = songs
    paths = [str(tmp_path / n) for n in ("good.flac", "flipped.flac", "not_flac.flac", "good2.flac")]
    for p, blob in zip(paths, (a, _flip_sample_bit(b, table, 17), b"RIFF" + a[4:], b)):
        with open(p, "wb") as f:
            f.write(blob)
    out = list(bliss.FlacDecoder.analyze_paths_with_options(paths, bliss.AnalysisOptions(), verify="crc"))
    assert [p for p, _ in out] == paths
    assert isinstance(out[0][1], bliss.Song) and isinstance(out[3][1], bliss.Song)
    assert isinstance(out[1][1], bliss.DecodingError) and "CRC-16 mismatch in frame 17" in str(out[1][1]) and paths[1] in str(out[1][1])
    assert out[1][1].first_bad_frame == 17
    assert isinstance(out[2][1], bliss.DecodingError)
    # a file that cannot be decoded reads as before in the default call, and the same under the checks
    for verify in (None, "crc", "md5"):
        res = bliss.analyze_flac_batch([b"RIFF" + a[4:], a[:len(a) // 2]], verify=verify)
        for r in res:
            assert isinstance(r, bliss.DecodingError) and r.message == "the FLAC stream cannot be decoded", (verify, r)
            assert r.flags & 7 == BAD_STREAM and r.first_bad_frame is None
    plain = list(bliss.FlacDecoder.analyze_paths_with_options(paths, bliss.AnalysisOptions()))
    assert dict(plain)[paths[2]].message.endswith("not a FLAC stream") and isinstance(dict(plain)[paths[1]], bliss.Song)
    verdicts = dict(bliss.FlacDecoder.verify_paths(paths))
    assert [verdicts[p].ok for p in paths] == [True, False, False, True] and verdicts[paths[2]].flags & BAD_STREAM
