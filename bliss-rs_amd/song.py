"""Song / Analysis / FeaturesVersion -- mirror of src/song/mod.rs and src/lib.rs (analysis part)."""
import ctypes as C
import enum
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _ffi

SAMPLE_RATE = 22050  # src/lib.rs:140
CHANNELS = 1         # src/lib.rs:137


class BlissError(Exception):
    """Umbrella error type (src/lib.rs:236-252)."""
    prefix = "error"

    def __init__(self, message):
        super().__init__(message)
        self.message = message

    def __str__(self):
        return f"{self.prefix} - {self.message}"

    def __eq__(self, other):
        return type(self) is type(other) and self.message == other.message

    __hash__ = Exception.__hash__


class DecodingError(BlissError):
    prefix = "error happened while decoding file"


class AnalysisError(BlissError):
    prefix = "error happened while analyzing file"


class ProviderError(BlissError):
    prefix = "error happened with the music library provider"


class FeaturesVersion(enum.IntEnum):
    """src/lib.rs:151-187"""
    Version2 = 2
    Version1 = 1

    def feature_count(self) -> int:
        return 23 if self is FeaturesVersion.Version2 else 20

    def feature_weights(self) -> np.ndarray:
        d = self.feature_count()
        m = np.zeros((d, d), np.float32)
        _ffi.call("blissgpu_feature_weights", int(self), m)
        return m

    def distance_metric(self):
        from .playlist import mahalanobis_distance_builder
        return mahalanobis_distance_builder(self.feature_weights())

    @classmethod
    def try_from(cls, value: int) -> "FeaturesVersion":
        if value in (1, 2):
            return cls(value)
        raise ProviderError(f"This features' version ({value}) does not exist")


FeaturesVersion.LATEST = FeaturesVersion.Version2
NUMBER_FEATURES = FeaturesVersion.LATEST.feature_count()  # src/song/mod.rs:222


class AnalysisIndex(enum.IntEnum):
    """src/song/mod.rs:102-156 (Version2 layout)"""
    Tempo = 0
    Zcr = 1
    MeanSpectralCentroid = 2
    StdDeviationSpectralCentroid = 3
    MeanSpectralRolloff = 4
    StdDeviationSpectralRolloff = 5
    MeanSpectralFlatness = 6
    StdDeviationSpectralFlatness = 7
    MeanLoudness = 8
    StdDeviationLoudness = 9
    Chroma1 = 10
    Chroma2 = 11
    Chroma3 = 12
    Chroma4 = 13
    Chroma5 = 14
    Chroma6 = 15
    Chroma7 = 16
    Chroma8 = 17
    Chroma9 = 18
    Chroma10 = 19
    Chroma11 = 20
    Chroma12 = 21
    Chroma13 = 22


AnalysisIndex.FEATURES_VERSION = FeaturesVersion.LATEST
AnalysisIndexv1 = enum.IntEnum("AnalysisIndexv1", [(m.name, m.value) for m in list(AnalysisIndex)[:20]])
AnalysisIndexv1.FEATURES_VERSION = FeaturesVersion.Version1


@dataclass(frozen=True)
class AnalysisOptions:
    """src/song/mod.rs:248-269.  number_cores is kept for interface parity; the batch is scheduled on
    the GPU, not on a host thread pool."""
    features_version: FeaturesVersion = FeaturesVersion.LATEST
    number_cores: int = field(default_factory=lambda: os.cpu_count() or 1)


class Analysis:
    """src/song/mod.rs:238-371"""

    def __init__(self, analysis: Sequence[float], features_version: FeaturesVersion = FeaturesVersion.LATEST):
        features_version = FeaturesVersion(features_version)
        arr = np.asarray(analysis, dtype=np.float32).copy()
        if arr.ndim != 1 or arr.shape[0] != features_version.feature_count():
            raise ProviderError(
                f"Feature count {arr.size} does not match the expected version feature count "
                f"{features_version.feature_count()}")
        self.internal_analysis = arr
        self.features_version = features_version

    @classmethod
    def new(cls, analysis, features_version):
        return cls(analysis, features_version)

    def as_arr1(self) -> np.ndarray:
        return self.internal_analysis.copy()

    def as_vec(self) -> List[float]:
        return [float(x) for x in self.internal_analysis]

    def __getitem__(self, index):
        want = AnalysisIndex.FEATURES_VERSION if isinstance(index, AnalysisIndex) else AnalysisIndexv1.FEATURES_VERSION
        if self.features_version != want:
            raise RuntimeError("Tried to index features with incompatible indexes")  # the reference panics
        return float(self.internal_analysis[int(index)])

    def __eq__(self, other):
        return (isinstance(other, Analysis) and self.features_version == other.features_version
                and np.array_equal(self.internal_analysis, other.internal_analysis))

    def __repr__(self):
        return f"Analysis (Version {int(self.features_version)}) /* {self.as_vec()} */"

    def distance(self, other: "Analysis") -> float:
        """Default distance for the FeaturesVersion (src/song/mod.rs:364-370)."""
        if self.features_version != other.features_version:
            raise RuntimeError("Mismatched features version between two songs or analysis")  # panic in the reference
        return self.features_version.distance_metric()(self.internal_analysis, other.internal_analysis)


def _as_pcm(sample_array) -> np.ndarray:
    """Decoder output as the library takes it: int16 stays int16 (widened on the device with sample / 32768, FFmpeg's
    s16 -> flt conversion), everything else becomes float32; 1-D = mono, 2-D = [frames, channels] interleaved
    (downmixed on the device like the reference's decoders, src/song/decoder/symphonia.rs:266-300)."""
    a = np.asarray(sample_array)
    if a.dtype not in (np.int16, np.int32):  # int32 = FFmpeg's S32 (24-bit streams left-justified): (float)s / 2^31 on the device
        a = a.astype(np.float32, copy=False)
    if a.ndim == 2 and a.shape[1] == 1:
        a = a[:, 0]
    if a.ndim not in (1, 2):
        raise ProviderError("sample arrays must be 1-D (mono) or 2-D [frames, channels]")
    return np.ascontiguousarray(a)


def _fmt_of(a: np.ndarray) -> int:
    return _ffi.SAMPLE_S16 if a.dtype == np.int16 else (_ffi.SAMPLE_S32 if a.dtype == np.int32 else _ffi.SAMPLE_F32)


def resampled_len(frames: int, sample_rate: int) -> int:
    """Samples at 22 050 Hz that `frames` frames at `sample_rate` become (libswresample's count; device-free)."""
    return int(_ffi.call("blissgpu_resampled_len", int(frames), int(sample_rate)))


def _results(out, status, version):
    results = []
    for i in range(len(status)):
        if status[i] == _ffi.SONG_OK:
            results.append(Analysis(out[i], version))
        elif status[i] == _ffi.SONG_TOO_SHORT:
            results.append(AnalysisError("empty or too short song."))
        else:
            results.append(AnalysisError(f"analysis failed with status {int(status[i])}"))
    return results


def analyze_decoded_batch(sample_arrays: Sequence[np.ndarray], sample_rates, options: Optional[AnalysisOptions] = None):
    """Decoder output at ANY sample rate -> analysis: what FFmpegDecoder::decode + Song::analyze do together
    (src/song/decoder/ffmpeg.rs:36-109, src/song/decoder.rs:85-101), with libswresample's conversion to mono 22 050 Hz
    done on the device (bit for bit at 44 100 Hz, the rate the reference pins).  sample_rates: one rate for all songs or one per song."""
    options = options or AnalysisOptions()
    version = FeaturesVersion(options.features_version)
    arrays = [_as_pcm(a) for a in sample_arrays]
    n = len(arrays)
    if n == 0:
        return []
    rates = [int(sample_rates)] * n if np.isscalar(sample_rates) else [int(r) for r in sample_rates]
    if len(rates) != n:
        raise ProviderError("one sample rate per song")
    d = version.feature_count()
    out = np.empty((n, d), np.float32)
    status = np.zeros(n, np.int32)
    keep = [a if a.size else np.zeros(1, a.dtype) for a in arrays]
    if n == 1:
        a = arrays[0]
        st = C.c_int32(0)
        _ffi.call("blissgpu_analyze_decoded", keep[0], _fmt_of(a), 1 if a.ndim == 1 else a.shape[1], a.shape[0], rates[0],
                  int(version), out, C.byref(st))
        status[0] = st.value
    else:
        songs = (_ffi.DecodedSong * n)()
        for i, a in enumerate(arrays):
            songs[i] = _ffi.DecodedSong(_ffi.address(keep[i]), a.shape[0], rates[i], 1 if a.ndim == 1 else a.shape[1], _fmt_of(a))
        _ffi.call("blissgpu_analyze_batch_decoded", songs, n, int(version), out, status)
    return _results(out, status, version)


def _file_bytes(item) -> np.ndarray:
    if isinstance(item, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(item), np.uint8)
    if isinstance(item, np.ndarray):
        return np.ascontiguousarray(item, np.uint8)
    try:
        with open(item, "rb") as f:
            return np.frombuffer(f.read(), np.uint8)
    except OSError:
        return np.zeros(0, np.uint8)   # an unreadable file is a DecodingError of that song, like any other bad file


_FLAC_CHECKS = {None: 0, "crc": _ffi.FLAC_CHECK_CRC16, "md5": _ffi.FLAC_CHECK_CRC16 | _ffi.FLAC_CHECK_MD5}


def _flac_failure(flags: int, first_bad_frame: int) -> str:
    """the message of a DecodingError that names the check and the frame"""
    if flags & _ffi.FLAC_BAD_STREAM:
        return "the FLAC stream cannot be decoded"
    if flags & _ffi.FLAC_BAD_CRC16:
        return f"the FLAC stream is damaged: CRC-16 mismatch in frame {first_bad_frame}"
    return "the FLAC stream is damaged: the MD5 of the decoded audio is not STREAMINFO's"


def analyze_flac_batch(files, options: Optional[AnalysisOptions] = None, verify: Optional[str] = None):
    """Compressed .flac files (bytes, uint8 arrays or paths) -> one Analysis or BlissError per file.  The host only finds the
    frames; the FLAC decoding, the conversion to mono 22 050 Hz and the analysis all run on the device
    (blissgpu_analyze_batch_flac).  A file that is not FLAC, has an unsupported depth, is truncated or holds a frame that cannot
    be decoded yields DecodingError and leaves every other song of the call untouched.
    verify: None -- the structure only (every frame stops 2 bytes before the next); "crc" -- also every frame's CRC-16, checked
    on the device; "md5" -- the CRC-16 and the MD5 of the decoded audio against STREAMINFO's (one lane per song: slow for long
    songs, a "check my library" mode).  A song that fails a check yields a DecodingError that names the check and the frame
    (its `flags` / `first_bad_frame` attributes hold the verdict); every other row is bit-identical to the unverified call's."""
    if verify not in _FLAC_CHECKS:
        raise ValueError('verify is None, "crc" or "md5"')
    checks = _FLAC_CHECKS[verify]
    options = options or AnalysisOptions()
    version = FeaturesVersion(options.features_version)
    blobs = [_file_bytes(f) for f in files]
    n = len(blobs)
    if n == 0:
        return []
    d = version.feature_count()
    out = np.empty((n, d), np.float32)
    status = np.zeros(n, np.int32)
    keep = [b if b.size else np.zeros(1, np.uint8) for b in blobs]
    ptrs = _ffi.pointer_table(keep)
    sizes = np.array([b.size for b in blobs], np.uint64)
    flags = np.zeros(n, np.uint32)
    first_bad = np.full(n, 0xFFFFFFFF, np.uint32)
    if checks:
        _ffi.call("blissgpu_analyze_batch_flac_verified", ptrs, sizes, n, int(version), checks, out, status, flags, first_bad)
    else:
        _ffi.call("blissgpu_analyze_batch_flac", ptrs, sizes, n, int(version), out, status)
    results = _results(out, status, version)
    for i in range(n):
        if status[i] == _ffi.SONG_DECODE_ERROR:
            # (no check failed -- none was asked for, or the song decoded and the analysis refused it: the stream is what is bad)
            verdict = int(flags[i]) if checks and int(flags[i]) & 7 else int(flags[i]) | _ffi.FLAC_BAD_STREAM
            results[i] = DecodingError(_flac_failure(verdict, int(first_bad[i])))
            results[i].flags = verdict
            results[i].first_bad_frame = int(first_bad[i]) if first_bad[i] != 0xFFFFFFFF else None
    return results


@dataclass
class FlacVerdict:
    """What the device found in one .flac file (flac_verify_batch)."""
    flags: int                      # BLISSGPU_FLAC_BAD_STREAM | _BAD_CRC16 | _BAD_MD5 | _MD5_UNCHECKED
    first_bad_frame: Optional[int]  # the first frame whose CRC-16 failed
    md5: Optional[str]              # the digest of the decoded audio (hex), None when it was not computed

    @property
    def ok(self) -> bool:
        return (self.flags & 7) == 0

    @property
    def stream_ok(self) -> bool:
        return not self.flags & _ffi.FLAC_BAD_STREAM

    @property
    def crc_ok(self) -> bool:
        return self.stream_ok and not self.flags & _ffi.FLAC_BAD_CRC16

    @property
    def md5_state(self) -> str:
        if self.flags & _ffi.FLAC_BAD_MD5:
            return "mismatch"
        return "unchecked" if self.flags & _ffi.FLAC_MD5_UNCHECKED else "match"


def flac_verify_batch(files, md5: bool = True):
    """`flac -t` for a batch of .flac files (bytes, uint8 arrays or paths), on the device: index, upload, decode, the
    end-position check, every frame's CRC-16 and -- md5=True -- the MD5 of the decoded audio against STREAMINFO's; no
    analysis.  One FlacVerdict per file; one bad file never affects another (blissgpu_flac_verify_batch).  The MD5 runs one
    lane per song and is slow for long songs."""
    blobs = [_file_bytes(f) for f in files]
    n = len(blobs)
    if n == 0:
        return []
    keep = [b if b.size else np.zeros(1, np.uint8) for b in blobs]
    ptrs = _ffi.pointer_table(keep)
    sizes = np.array([b.size for b in blobs], np.uint64)
    flags = np.zeros(n, np.uint32)
    first_bad = np.zeros(n, np.uint32)
    digests = np.zeros((n, 16), np.uint8)
    checks = _ffi.FLAC_CHECK_CRC16 | (_ffi.FLAC_CHECK_MD5 if md5 else 0)
    _ffi.call("blissgpu_flac_verify_batch", ptrs, sizes, n, checks, flags, first_bad, digests)
    computed = (flags & (_ffi.FLAC_MD5_UNCHECKED | _ffi.FLAC_BAD_STREAM)) == 0
    return [FlacVerdict(int(f), int(b) if b != 0xFFFFFFFF else None, d.tobytes().hex() if c else None)
            for f, b, d, c in zip(flags, first_bad, digests, computed)]


def flac_decode_batch(files):
    """Several .flac files through ONE upload and ONE decode launch (the decode half of analyze_flac_batch): a list with, per
    file, (samples [frames, channels], sample_rate, bits_per_sample) or DecodingError (blissgpu_flac_decode_batch)."""
    blobs = [_file_bytes(f) for f in files]
    n = len(blobs)
    if n == 0:
        return []
    keep = [b if b.size else np.zeros(1, np.uint8) for b in blobs]
    infos = np.zeros((n, _ffi.FLAC_INFO_WORDS), np.uint64)
    pcm = []
    for b, k, info in zip(blobs, keep, infos):   # sizes first (device-free)
        nf = C.c_uint64(0)
        ok = _ffi.call_unchecked("blissgpu_flac_index", k, b.size, 0, info, None, 0, C.byref(nf)) == _ffi.OK
        ok = ok and 1 <= int(info[1]) <= 8 and 4 <= int(info[2]) <= 24
        pcm.append(np.zeros((int(info[3]) if ok else 0, int(info[1]) if ok else 1), np.int32 if int(info[2]) > 16 else np.int16))
    hold = [p if p.size else np.zeros((1, 1), p.dtype) for p in pcm]
    sizes = np.array([b.size for b in blobs], np.uint64)
    room = np.array([p.nbytes for p in pcm], np.uint64)
    status = np.zeros(n, np.int32)
    _ffi.call("blissgpu_flac_decode_batch", _ffi.pointer_table(keep), sizes, n, _ffi.pointer_table(hold), room, infos, status)
    return [(p[:int(i[3])], int(i[0]), int(i[2])) if st == _ffi.SONG_OK else DecodingError("the FLAC stream cannot be decoded")
            for p, i, st in zip(pcm, infos, status)]


def flac_decode(data):
    """One .flac file (bytes or a path) -> (samples, sample_rate, bits_per_sample), decoded on the device and copied back:
    [frames, channels] int16 (sample << (16 - bps)) up to 16 bits per sample, int32 (sample << (32 - bps)) above
    (blissgpu_flac_decode).  Raises DecodingError."""
    blob = _file_bytes(data)
    info = np.zeros(_ffi.FLAC_INFO_WORDS, np.uint64)
    st = C.c_int32(0)
    src = blob if blob.size else np.zeros(1, np.uint8)
    _ffi.call("blissgpu_flac_decode", src, blob.size, None, 0, info, C.byref(st))
    if st.value != _ffi.SONG_OK:
        raise DecodingError("the FLAC stream cannot be decoded")
    channels, bps = int(info[1]), int(info[2])
    pcm = np.zeros((int(info[3]), channels), np.int32 if bps > 16 else np.int16)
    if pcm.size:
        _ffi.call("blissgpu_flac_decode", src, blob.size, pcm, pcm.nbytes, info, C.byref(st))
        if st.value != _ffi.SONG_OK:
            raise DecodingError("the FLAC stream cannot be decoded")
    return pcm[:int(info[3])], int(info[0]), bps


def analyze_batch(sample_arrays: Sequence[np.ndarray], options: Optional[AnalysisOptions] = None):
    """Bulk Song::analyze_with_options: one GPU batch, per-song result (Analysis or BlissError), like the
    (path, BlissResult<Song>) pairs of analyze_paths_with_options (src/song/decoder.rs:278-332).  A single song goes
    through blissgpu_analyze[_interleaved], whose concurrent callers (threads each analysing one song, as the
    reference's worker pool does, src/song/decoder.rs:299-329) are coalesced into one device batch."""
    options = options or AnalysisOptions()
    version = FeaturesVersion(options.features_version)
    arrays = [_as_pcm(a) for a in sample_arrays]
    n = len(arrays)
    if n == 0:
        return []
    d = version.feature_count()
    out = np.empty((n, d), np.float32)
    status = np.empty(n, np.int32)
    # one device batch per (sample format, channel count) class -- normally there is exactly one
    classes = {}
    for i, a in enumerate(arrays):
        classes.setdefault((_fmt_of(a), 1 if a.ndim == 1 else a.shape[1]), []).append(i)
    for (fmt, channels), idx in classes.items():
        if len(idx) == 1:
            a = arrays[idx[0]]
            buf = a if a.size else np.zeros(1, a.dtype)
            row = np.empty(d, np.float32)
            st = C.c_int32(0)
            _ffi.call("blissgpu_analyze_interleaved", buf, fmt, channels, a.shape[0], int(version), row, C.byref(st))
            out[idx[0]] = row
            status[idx[0]] = st.value
            continue
        lengths = np.array([arrays[i].shape[0] for i in idx], np.uint64)  # frames
        offsets = np.zeros(len(idx), np.uint64)
        offsets[1:] = np.cumsum(lengths)[:-1]
        pcm = np.concatenate([arrays[i].reshape(-1) for i in idx])
        if pcm.size == 0:
            pcm = np.zeros(1, arrays[idx[0]].dtype)
        res = np.empty((len(idx), d), np.float32)
        st = np.empty(len(idx), np.int32)
        _ffi.call("blissgpu_analyze_batch_interleaved", pcm, fmt, channels, offsets, lengths, len(idx), int(version), res, st)
        out[idx] = res
        status[idx] = st
    return _results(out, status, version)


# ---- acoustic fingerprints (blissgpu_fingerprint_batch): opt-in, never part of analyze_* ----
FINGERPRINT_VERSION = 1  # stored beside the words (library.store_fingerprints): another contract, another number


def fingerprint_len(n_samples: int) -> int:
    """Sub-fingerprints of a song of n_samples samples at 22 050 Hz: (n - 8192) // 512, 0 below 8704 (device-free)."""
    return int(_ffi.call("blissgpu_fingerprint_len", int(n_samples)))


def fingerprint_batch(sample_arrays: Sequence[np.ndarray], return_energies: bool = False):
    """The Haitsma-Kalker fingerprint of every song, in one call: sample_arrays are the mono 22 050 Hz float32 samples
    analyze_batch takes (1-D; anything else goes through fingerprint_decoded_batch).  -> a list of np.uint32 arrays, one
    32-bit word per 512-sample hop, empty for a song of fewer than 8704 samples.  The contract -- frames of 8192 samples,
    33 logarithmic bands over 300 .. 2000 Hz, a bit per band and frame pair -- is stated in include/blissgpu.h; two copies of
    one recording differ in few bits once aligned (playlist.fingerprint_match).  return_energies: -> (words, energies), the
    f64 band energies [frames, 33] of every song (the tests' tap)."""
    arrays = []
    for a in sample_arrays:
        a = np.asarray(a)
        if a.ndim == 2 and a.shape[1] == 1:
            a = a[:, 0]
        if a.ndim != 1 or a.dtype.kind != "f":
            raise ProviderError("fingerprint_batch takes mono float samples at 22 050 Hz; decoder output goes through fingerprint_decoded_batch")
        arrays.append(np.ascontiguousarray(a, dtype=np.float32))
    n = len(arrays)
    if n == 0:
        return ([], []) if return_energies else []
    sample_offsets = np.zeros(n + 1, np.uint64)
    sample_offsets[1:] = np.cumsum([a.shape[0] for a in arrays], dtype=np.uint64)
    word_offsets = np.zeros(n + 1, np.uint64)
    word_offsets[1:] = np.cumsum([fingerprint_len(a.shape[0]) for a in arrays], dtype=np.uint64)
    pcm = np.concatenate(arrays) if n > 1 else arrays[0]
    if pcm.size == 0:
        pcm = np.zeros(1, np.float32)
    n_words = int(word_offsets[n])
    words = np.zeros(max(n_words, 1), np.uint32)
    status = np.zeros(n, np.int32)
    energies = np.zeros((n_words + n, 33), np.float64) if return_energies else None
    _ffi.call("blissgpu_fingerprint_batch", pcm, sample_offsets, word_offsets, n, words, status, energies)
    wo = word_offsets.astype(np.int64)
    out = [words[wo[i]:wo[i + 1]].copy() for i in range(n)]
    if not return_energies:
        return out
    # song i owns rows wo[i] + i .. : one per frame = one more than its words; a too-short song has no frame
    return out, [energies[wo[i] + i:wo[i + 1] + i + 1] if wo[i + 1] > wo[i] else np.zeros((0, 33)) for i in range(n)]


def fingerprint_decoded_batch(sample_arrays: Sequence[np.ndarray], sample_rates):
    """fingerprint_batch for decoder output at ANY sample rate (1-D mono or [frames, channels]; float32 / int16 / int32): every
    song goes through the device conversion analyze_decoded_batch uses (blissgpu_pcm_decode_device: downmix, widening,
    libswresample's resampler to mono 22 050 Hz), then through fingerprint_batch.  sample_rates: one rate or one per song."""
    arrays = [_as_pcm(a) for a in sample_arrays]
    n = len(arrays)
    if n == 0:
        return []
    rates = [int(sample_rates)] * n if np.isscalar(sample_rates) else [int(r) for r in sample_rates]
    if len(rates) != n:
        raise ProviderError("one sample rate per song")
    ctx = C.c_void_p()
    _ffi.call("blissgpu_default_ctx", 0, C.byref(ctx))
    mono = []
    for a, rate in zip(arrays, rates):
        n_out = resampled_len(a.shape[0], rate)
        out = np.zeros(n_out, np.float32)
        if n_out:
            d_in, d_out = C.c_void_p(), C.c_void_p()
            _ffi.call("blissgpu_malloc", C.byref(d_in), a.nbytes)
            try:
                _ffi.call("blissgpu_malloc", C.byref(d_out), out.nbytes)
                try:
                    _ffi.call("blissgpu_memcpy_h2d", ctx, d_in, a, a.nbytes)
                    _ffi.call("blissgpu_pcm_decode_device", ctx, d_in, _fmt_of(a), 1 if a.ndim == 1 else a.shape[1], a.shape[0], rate, d_out)
                    _ffi.call("blissgpu_memcpy_d2h", ctx, out, d_out, out.nbytes)  # (on the context's stream, then waits)
                finally:
                    _ffi.call_unchecked("blissgpu_free", d_out)
            finally:
                _ffi.call_unchecked("blissgpu_free", d_in)
        mono.append(out)
    return fingerprint_batch(mono)


# ---- loudness (blissgpu_loudness_batch): EBU R 128 / ReplayGain 2.0, opt-in, never part of analyze_* ----
LOUDNESS_VERSION = 1  # stored beside the figures (library.store_loudness): another contract, another number


@dataclass
class Loudness:
    """The loudness of one song or one album: integrated loudness (LUFS, BS.1770-4 with both gates), loudness range (LU, EBU
    Tech 3342), sample peak and 4x-oversampled true peak (linear, 1.0 = full scale), and `power`, the gated mean square the
    LUFS figure is the logarithm of (the quantity that is defined to the bit)."""
    lufs: float
    range_lu: float
    sample_peak: float
    true_peak: float
    power: float

    def replaygain(self, reference: float = -18.0):
        """(gain_db, peak) of ReplayGain 2.0: the gain that brings the song to `reference` LUFS, and its true peak"""
        return reference - self.lufs, self.true_peak


def _loudness_songs(sample_arrays, sample_rates):
    arrays = [_as_pcm(a) for a in sample_arrays]
    n = len(arrays)
    rates = [int(sample_rates)] * n if np.isscalar(sample_rates) else [int(r) for r in sample_rates]
    if len(rates) != n:
        raise ProviderError("one sample rate per song")
    keep = [a if a.size else np.zeros(1, a.dtype) for a in arrays]
    songs = (_ffi.DecodedSong * max(n, 1))()
    for i, a in enumerate(arrays):
        songs[i] = _ffi.DecodedSong(_ffi.address(keep[i]), a.shape[0], rates[i], 1 if a.ndim == 1 else a.shape[1], _fmt_of(a))
    return arrays, rates, keep, songs


def _album_indices(albums, n):
    """labels of any hashable kind -> (uint32 indices in order of first appearance, the labels in that order)"""
    albums = list(albums)
    if len(albums) != n:
        raise ProviderError("one album label per song")
    order = {}
    idx = np.array([order.setdefault(a, len(order)) for a in albums], np.uint32)
    return idx, list(order)


def loudness_gate(block_powers) -> tuple:
    """(power, lufs) of BS.1770-4's two gates over 400 ms block powers (blissgpu_loudness_gate; device-free)"""
    P = np.ascontiguousarray(block_powers, dtype=np.float64).reshape(-1)
    power, lufs = C.c_double(0.0), C.c_double(0.0)
    _ffi.call("blissgpu_loudness_gate", P if P.size else None, P.size, C.byref(power), C.byref(lufs))
    return power.value, lufs.value


def loudness_range(short_term_powers) -> tuple:
    """(range_lu, lo, hi) of EBU Tech 3342 over 3 s short-term powers (blissgpu_loudness_range; device-free)"""
    ST = np.ascontiguousarray(short_term_powers, dtype=np.float64).reshape(-1)
    r, lo, hi = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    _ffi.call("blissgpu_loudness_range", ST if ST.size else None, ST.size, C.byref(r), C.byref(lo), C.byref(hi))
    return r.value, lo.value, hi.value


def loudness_blocks(z, sample_rate: int) -> tuple:
    """Sub-block energies z [channels, n_sub] -> (P, ST): the 400 ms block powers and the 3 s short-term powers, hop 100 ms
    (blissgpu_loudness_blocks; device-free)"""
    z = np.ascontiguousarray(np.atleast_2d(z), dtype=np.float64)
    channels, n_sub = z.shape
    P = np.zeros(max(n_sub - 3, 0), np.float64)
    ST = np.zeros(max(n_sub - 29, 0), np.float64)
    _ffi.call("blissgpu_loudness_blocks", z if z.size else None, channels, n_sub, int(sample_rate), P if P.size else None,
              ST if ST.size else None)
    return P, ST


def loudness_batch(sample_arrays: Sequence[np.ndarray], sample_rates, albums=None, return_energies: bool = False):
    """EBU R 128 loudness of every song, in one call, at the songs' NATIVE rates: sample_arrays are decoder output (1-D mono or
    [frames, 2]; float32 / int16 / int32), sample_rates one rate or one per song (8 000 .. 768 000 Hz).  -> a list with a
    `Loudness` per song, or AnalysisError for a song of fewer than four 100 ms sub-blocks.  albums: one hashable label per song
    -> (songs, {label: Loudness}), the album figures gated over all blocks of the album's songs (ReplayGain's album gain).
    The K-weighting filter, the energies and both peaks run on the device (blissgpu_loudness_batch); the contract is in
    include/blissgpu.h.  return_energies (the tests' tap): the result is followed by a list of (z [channels, n_sub],
    sample_peak, true_peak) per song, and the gates run through the device-free entry points on those energies -- the same
    arithmetic, the same figures."""
    arrays, rates, keep, songs = _loudness_songs(sample_arrays, sample_rates)
    n = len(arrays)
    labels, names = _album_indices(albums, n) if albums is not None else (None, [])
    status = np.zeros(max(n, 1), np.int32)
    channels = [1 if a.ndim == 1 else a.shape[1] for a in arrays]
    if not return_energies:
        rows = np.zeros((max(n, 1), 5), np.float64)
        album_rows = np.zeros((max(len(names), 1), 5), np.float64)
        _ffi.call("blissgpu_loudness_batch", songs, n, labels, len(names), rows, album_rows if labels is not None else None, status)
        taps = None
    else:
        n_sub = [int(_ffi.call("blissgpu_loudness_subblocks", a.shape[0], r)) for a, r in zip(arrays, rates)]
        zoff = np.zeros(n + 1, np.int64)
        zoff[1:] = np.cumsum([c * u for c, u in zip(channels, n_sub)])
        z = np.zeros(max(int(zoff[n]), 1), np.float64)
        sp, tp = np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.float64)
        _ffi.call("blissgpu_loudness_energies", songs, n, z, sp, tp, status)
        taps = [(z[zoff[i]:zoff[i + 1]].reshape(channels[i], n_sub[i]).copy(), float(sp[i]), float(tp[i])) for i in range(n)]
        rows = np.full((max(n, 1), 5), np.nan)
        blocks = {}
        for i in range(n):
            if status[i] == _ffi.SONG_OK:
                blocks[i] = loudness_blocks(taps[i][0], rates[i])
                rows[i, :2] = loudness_gate(blocks[i][0])
                rows[i, 2] = loudness_range(blocks[i][1])[0]
                rows[i, 3:] = sp[i], tp[i]
        album_rows = np.zeros((max(len(names), 1), 5), np.float64)
        for a in range(len(names)):
            members = [i for i in blocks if labels[i] == a]
            album_rows[a, :2] = loudness_gate(np.concatenate([blocks[i][0] for i in members]) if members else [])
            album_rows[a, 2] = loudness_range(np.concatenate([blocks[i][1] for i in members]) if members else [])[0]
            album_rows[a, 3] = max([sp[i] for i in members], default=0.0)
            album_rows[a, 4] = max([tp[i] for i in members], default=0.0)

    def of(row):
        return Loudness(lufs=float(row[1]), range_lu=float(row[2]), sample_peak=float(row[3]), true_peak=float(row[4]), power=float(row[0]))

    out = [of(rows[i]) if status[i] == _ffi.SONG_OK else AnalysisError("empty or too short song.") for i in range(n)]
    result = (out,) if albums is None else (out, {name: of(album_rows[a]) for a, name in enumerate(names)})
    if return_energies:
        result += (taps,)
    return result[0] if len(result) == 1 else result


def loudness_flac_batch(files, albums=None):
    """loudness_batch for compressed .flac files (bytes, uint8 arrays or paths): flac_decode_batch (decoded on the device, the
    PCM copied back) followed by loudness_batch on that PCM at the files' own rates -- a host round trip of the PCM between the
    two device calls, not a fused path.  A file that cannot be decoded yields its DecodingError and takes no part in its
    album."""
    decoded = flac_decode_batch(files)
    good = [i for i, d in enumerate(decoded) if not isinstance(d, BlissError)]
    if albums is not None:
        albums = list(albums)
        if len(albums) != len(decoded):
            raise ProviderError("one album label per song")
    out = list(decoded)
    res = loudness_batch([decoded[i][0] for i in good], [decoded[i][1] for i in good],
                         albums=None if albums is None else [albums[i] for i in good])
    songs = res if albums is None else res[0]
    for i, r in zip(good, songs):
        out[i] = r
    return out if albums is None else (out, res[1])


@dataclass
class Song:
    """src/song/mod.rs:45-76 (metadata fields kept, filled by decoders)."""
    path: str = ""
    artist: Optional[str] = None
    title: Optional[str] = None
    album: Optional[str] = None
    album_artist: Optional[str] = None
    track_number: Optional[int] = None
    disc_number: Optional[int] = None
    genre: Optional[str] = None
    duration: float = 0.0
    analysis: Optional[Analysis] = None
    features_version: FeaturesVersion = FeaturesVersion.LATEST
    cue_info: Optional[object] = None

    @staticmethod
    def analyze(sample_array) -> Analysis:
        """src/song/mod.rs:403-405"""
        return Song.analyze_with_options(sample_array, AnalysisOptions())

    @staticmethod
    def analyze_with_options(sample_array, analysis_options: AnalysisOptions) -> Analysis:
        """src/song/mod.rs:413-508.  Raises AnalysisError("empty or too short song.") for len < 8192."""
        res = analyze_batch([sample_array], analysis_options)[0]
        if isinstance(res, BlissError):
            raise res
        return res

    @staticmethod
    def analyze_decoded(sample_array, sample_rate: int, analysis_options: Optional[AnalysisOptions] = None) -> Analysis:
        """Decoder output at `sample_rate` Hz (1-D mono or [frames, channels]; float32 / int16 / int32): the conversion
        FFmpegDecoder does on the CPU (src/song/decoder/ffmpeg.rs:36-109) runs on the device, then Song::analyze."""
        res = analyze_decoded_batch([sample_array], sample_rate, analysis_options)[0]
        if isinstance(res, BlissError):
            raise res
        return res

    def distance(self, other: "Song") -> float:
        """src/song/mod.rs:519-521"""
        return self.analysis.distance(other.analysis)
