"""Decoder trait mirror (src/song/decoder.rs:34-333).

Decoding of other codecs (ffmpeg / symphonia, src/song/decoder/*.rs) stays on the CPU and is out of scope
(SURVEY.md section 8): implement `decode` for your container/codec; everything from
PreAnalyzedSong -> Song runs on the GPU.  FLAC is the exception: `FlacDecoder` hands the COMPRESSED file to the device,
which decodes it (one frame per lane), converts it and analyses it.  `analyze_paths` batches the decoded songs into GPU launches
instead of the reference's per-core thread pool (src/song/decoder.rs:282-331).
"""
import abc
import re
import wave
from dataclasses import dataclass, field
from typing import Iterable, Iterator, Optional, Tuple, Union

import numpy as np

from .song import (AnalysisOptions, BlissError, DecodingError, FeaturesVersion, SAMPLE_RATE, Song,
                   analyze_batch, analyze_decoded_batch, analyze_flac_batch, resampled_len)


@dataclass
class PreAnalyzedSong:
    """src/song/decoder.rs:34-65: decoded samples + tags.  The reference's decoders deliver mono 22 050 Hz f32; here a
    decoder may stop earlier and hand over what the codec produced -- [frames, channels] int16 / int32 / float32 at
    `sample_rate` -- and the conversion FFmpegDecoder does on the CPU (libswresample, src/song/decoder/ffmpeg.rs:36-109)
    runs on the device with the analysis."""
    path: str = ""
    artist: Optional[str] = None
    title: Optional[str] = None
    album: Optional[str] = None
    album_artist: Optional[str] = None
    track_number: Optional[int] = None
    disc_number: Optional[int] = None
    genre: Optional[str] = None
    duration: float = 0.0
    sample_array: np.ndarray = field(default_factory=lambda: np.zeros(0, np.float32))
    sample_rate: int = SAMPLE_RATE
    flac: Optional[bytes] = None   # FlacDecoder: the COMPRESSED file; sample_array stays empty, the device decodes

    def _song(self, analysis, version) -> Song:
        return Song(path=self.path, artist=self.artist, title=self.title, album=self.album,
                    album_artist=self.album_artist, track_number=self.track_number, disc_number=self.disc_number,
                    genre=self.genre, duration=self.duration, analysis=analysis, features_version=version)

    def to_song_with_options(self, analysis_options: AnalysisOptions) -> Song:
        """src/song/decoder.rs:85-101"""
        if self.flac is not None:
            analysis = analyze_flac_batch([self.flac], analysis_options)[0]
            if isinstance(analysis, BlissError):
                raise analysis
            return self._song(analysis, FeaturesVersion(analysis_options.features_version))
        if self.sample_rate == SAMPLE_RATE:
            analysis = Song.analyze_with_options(self.sample_array, analysis_options)
        else:
            analysis = Song.analyze_decoded(self.sample_array, self.sample_rate, analysis_options)
        return self._song(analysis, FeaturesVersion(analysis_options.features_version))


class Decoder(abc.ABC):
    """src/song/decoder.rs:115-333"""

    @classmethod
    @abc.abstractmethod
    def decode(cls, path: str) -> PreAnalyzedSong:
        """Required method (src/song/decoder.rs:129): file -> mono 22 050 Hz f32 samples."""

    @classmethod
    def song_from_path(cls, path: str) -> Song:
        return cls.song_from_path_with_options(path, AnalysisOptions())

    @classmethod
    def song_from_path_with_options(cls, path: str, analysis_options: AnalysisOptions) -> Song:
        return cls.decode(path).to_song_with_options(analysis_options)

    @classmethod
    def analyze_paths(cls, paths: Iterable[str]) -> Iterator[Tuple[str, Union[Song, BlissError]]]:
        return cls.analyze_paths_with_options(paths, AnalysisOptions())

    @classmethod
    def analyze_paths_with_options(cls, paths: Iterable[str], analysis_options: AnalysisOptions,
                                   batch_songs: int = 256) -> Iterator[Tuple[str, Union[Song, BlissError]]]:
        """Yields (path, Song | BlissError); a bad file never aborts the run (src/song/decoder.rs:313-325)."""
        version = FeaturesVersion(analysis_options.features_version)
        pending = []

        def flush():
            if all(p.sample_rate == SAMPLE_RATE for p in pending):
                results = analyze_batch([p.sample_array for p in pending], analysis_options)
            else:
                results = analyze_decoded_batch([p.sample_array for p in pending], [p.sample_rate for p in pending],
                                                analysis_options)
            for pre, res in zip(pending, results):
                yield pre.path, (res if isinstance(res, BlissError) else pre._song(res, version))
            pending.clear()

        for path in paths:
            try:
                pending.append(cls.decode(path))
            except BlissError as e:
                yield path, e
                continue
            except Exception as e:  # decoder failures are reported per file
                yield path, DecodingError(str(e))
                continue
            if len(pending) >= batch_songs:
                yield from flush()
        if pending:
            yield from flush()


class RawPcmDecoder(Decoder):
    """Decoder for already-decoded PCM: `.npy` (float32, int16 or int32; 1-D mono or [frames, channels]; 22 050 Hz) and
    16-bit `.wav` (any channel count, ANY sample rate).  Samples are passed on as the file holds them: the widening
    (sample / 32768, FFmpeg's conversion), the mono downmix and the resampling to 22 050 Hz (libswresample's default
    resampler, as FFmpegDecoder uses it: src/song/decoder/ffmpeg.rs:36-109) run on the device."""

    @classmethod
    def decode(cls, path: str) -> PreAnalyzedSong:
        rate = SAMPLE_RATE
        try:
            if path.endswith(".npy"):
                a = np.load(path)
                if a.ndim not in (1, 2) or (a.ndim == 2 and not 1 <= a.shape[1] <= 8):
                    raise DecodingError("expected [frames] or [frames, channels <= 8] samples")
                samples = a if a.dtype in (np.int16, np.int32) else a.astype(np.float32)
            else:
                with wave.open(path, "rb") as w:
                    if w.getsampwidth() != 2 or not 1 <= w.getnchannels() <= 8:
                        raise DecodingError("only s16 wav is supported by RawPcmDecoder")
                    rate = w.getframerate()
                    samples = np.frombuffer(w.readframes(w.getnframes()), "<i2")
                    if w.getnchannels() > 1:
                        samples = samples.reshape(-1, w.getnchannels())
        except BlissError:
            raise
        except Exception as e:
            raise DecodingError(f"while opening format for file '{path}': {e}")
        return PreAnalyzedSong(path=path, sample_array=samples, sample_rate=rate,
                               duration=resampled_len(samples.shape[0], rate) / SAMPLE_RATE)


def _vorbis_track(text: str) -> Optional[int]:
    """`t.parse::<i32>().ok().or_else(|| t.split_once('/')...)` (src/song/decoder/ffmpeg.rs:224-241)"""
    def parse(t):   # Rust's i32::from_str: an optional sign and ASCII digits, nothing else
        if not re.fullmatch(r"[+-]?[0-9]+", t, flags=re.ASCII):
            return None
        return int(t) if -2 ** 31 <= int(t) < 2 ** 31 else None

    if text == "":
        return None
    v = parse(text)
    if v is None and "/" in text:
        v = parse(text.split("/", 1)[0])
    return v


class FlacDecoder(Decoder):
    """.flac files decoded ON THE DEVICE.  `decode` reads the file, STREAMINFO and the VORBIS_COMMENT block -- artist, title,
    album, album_artist, track_number, disc_number and genre as the reference's FFmpeg decoder fills them
    (src/song/decoder/ffmpeg.rs:200-247; FFmpeg names TRACKNUMBER / DISCNUMBER / ALBUMARTIST track / disc / album_artist), the
    duration from STREAMINFO -- and keeps the COMPRESSED bytes in the PreAnalyzedSong.  `analyze_paths_with_options` sends
    batches of compressed files through `analyze_flac_batch`: no residual is ever decoded on the CPU.  `verify_paths` is
    `flac -t` for a library: every frame's CRC-16 and the stream's MD5, checked on the device."""

    _KEYS = {"tracknumber": "track", "discnumber": "disc", "albumartist": "album_artist"}

    @classmethod
    def decode(cls, path: str) -> PreAnalyzedSong:
        try:
            with open(path, "rb") as f:
                data = f.read()
        except OSError as e:
            raise DecodingError(f"while opening format for file '{path}': {e}")
        p = 0
        if data[:3] == b"ID3" and len(data) >= 10:
            p = 10 + ((data[6] & 0x7F) << 21 | (data[7] & 0x7F) << 14 | (data[8] & 0x7F) << 7 | (data[9] & 0x7F)) + (10 if data[5] & 0x10 else 0)
        if data[p:p + 4] != b"fLaC":
            raise DecodingError(f"while opening format for file '{path}': not a FLAC stream")
        p += 4
        rate = total = 0
        tags = {}
        while True:
            if p + 4 > len(data):
                raise DecodingError(f"while opening format for file '{path}': truncated in the metadata")
            kind, length = data[p], int.from_bytes(data[p + 1:p + 4], "big")
            body = data[p + 4:p + 4 + length]
            if len(body) != length:
                raise DecodingError(f"while opening format for file '{path}': truncated in the metadata")
            if kind & 0x7F == 0 and length >= 18:
                v = int.from_bytes(body[10:18], "big")
                rate, total = v >> 44, v & ((1 << 36) - 1)
            elif kind & 0x7F == 4:
                tags = cls._comments(body)
            p += 4 + length
            if kind & 0x80:
                break
        if rate == 0:
            raise DecodingError(f"while opening format for file '{path}': no STREAMINFO")
        text = lambda k: tags.get(k) or None   # ("" => None)
        return PreAnalyzedSong(path=path, artist=text("artist"), title=text("title"), album=text("album"),
                               album_artist=text("album_artist"), genre=text("genre"),
                               track_number=_vorbis_track(tags.get("track", "")), disc_number=_vorbis_track(tags.get("disc", "")),
                               duration=total / rate, sample_rate=rate, flac=data)

    @classmethod
    def _comments(cls, body: bytes) -> dict:
        """VORBIS_COMMENT: little-endian lengths, KEY=value in UTF-8; keys are case-insensitive, a repeated key is joined with
        ';' (FFmpeg's av_dict_set with AV_DICT_APPEND in ff_vorbis_comment)."""
        out = {}
        try:
            p = 4 + int.from_bytes(body[0:4], "little")
            count = int.from_bytes(body[p:p + 4], "little")
            p += 4
            for _ in range(count):
                n = int.from_bytes(body[p:p + 4], "little")
                entry = body[p + 4:p + 4 + n].decode("utf-8", "replace")
                p += 4 + n
                if "=" not in entry:
                    continue
                key, value = entry.split("=", 1)
                key = cls._KEYS.get(key.lower(), key.lower())
                out[key] = out[key] + ";" + value if key in out else value
        except Exception:   # a malformed comment block costs the tags, not the song
            pass
        return out

    @classmethod
    def analyze_paths_with_options(cls, paths: Iterable[str], analysis_options: AnalysisOptions,
                                   batch_songs: int = 256, verify=None) -> Iterator[Tuple[str, Union[Song, BlissError]]]:
        """Yields (path, Song | BlissError), batches of compressed files at a time; a bad file yields its DecodingError and
        never aborts the run (src/song/decoder.rs:313-325).
        verify: None | "crc" | "md5" -- also check every frame's CRC-16 (and the stream's MD5) on the device
        (`analyze_flac_batch`); a song that fails yields a DecodingError that names the file, the check and the frame, e.g.
        "... CRC-16 mismatch in frame 17", and the results keep the order of the paths."""
        version = FeaturesVersion(analysis_options.features_version)
        pending = []   # PreAnalyzedSong, or -- with verify -- the (path, error) of a file that could not be opened

        def flush():
            songs = [p for p in pending if isinstance(p, PreAnalyzedSong)]
            results = iter(analyze_flac_batch([p.flac for p in songs], analysis_options, verify=verify))
            for pre in pending:
                if not isinstance(pre, PreAnalyzedSong):
                    yield pre
                    continue
                res = next(results)
                if isinstance(res, DecodingError) and verify is not None:
                    named = DecodingError(f"while decoding file '{pre.path}': {res.message}")
                    named.flags, named.first_bad_frame = res.flags, res.first_bad_frame
                    res = named
                yield pre.path, (res if isinstance(res, BlissError) else pre._song(res, version))
            pending.clear()

        for path in paths:
            try:
                pending.append(cls.decode(path))
            except Exception as e:
                error = e if isinstance(e, BlissError) else DecodingError(str(e))
                if verify is None:
                    yield path, error
                    continue
                pending.append((path, error))
            if len(pending) >= batch_songs:
                yield from flush()
        if pending:
            yield from flush()

    @classmethod
    def verify_paths(cls, paths: Iterable[str], md5: bool = True, batch_songs: int = 256):
        """Yields (path, FlacVerdict), batches of files at a time (`flac_verify_batch`): no analysis, a verdict per file."""
        from .song import flac_verify_batch

        pending = []
        for path in paths:
            pending.append(path)
            if len(pending) >= batch_songs:
                yield from zip(pending, flac_verify_batch(pending, md5=md5))
                pending = []
        if pending:
            yield from zip(pending, flac_verify_batch(pending, md5=md5))
