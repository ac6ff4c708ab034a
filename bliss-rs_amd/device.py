"""Device-resident API: a blissgpu context driven with torch tensors (torch supplies device memory,
streams and torch.distributed; the compute is the HIP library)."""
import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from . import _ffi
from . import playlist as P
from ._ffi import FORMS, GATES, GROUP_MODES, JOURNEY_MODES, METRICS, RADIO_MODES, ROUTES
from .song import DecodingError


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _offsets(offsets, rows):
    """a HOST sequence of G + 1 group offsets over `rows` seed rows -> (uint64 array, G)"""
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1)).astype(np.uint64)
    assert off.shape[0] >= 1 and int(off[-1]) == rows
    return off, off.shape[0] - 1


def _contig(t):
    return None if t is None else t.contiguous()


def _dptr(t):
    """the address of a tensor that _ffi.call must not hold to contiguity: pairwise's `out` comes with its row stride"""
    return C.c_void_p(t.data_ptr())


class Context:
    """blissgpu_ctx wrapper.  Tensors passed in must live on the context's device."""

    def __init__(self, device: int = 0, use_torch_stream: bool = True):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: bliss_rs_amd has no CPU fallback")
        self.torch = torch
        self.device = device
        torch.cuda.set_device(device)
        self._L = _ffi.lib()
        h = C.c_void_p()
        _ffi.call("blissgpu_ctx_create", device, C.byref(h))
        self._h = h
        if use_torch_stream:
            self.bind_current_stream()

    @classmethod
    def default(cls, k: int = 0) -> "Context":
        """The k-th default context of the library -- the one the entry points without a context argument run on
        (blissgpu_default_ctx).  Borrowed: closing this object leaves the context alone."""
        import torch

        self = cls.__new__(cls)
        self.torch = torch
        self._L = _ffi.lib()
        h = C.c_void_p()
        _ffi.call("blissgpu_default_ctx", int(k), C.byref(h))
        self._h = h
        self._borrowed = True
        self.device = _ffi.call("blissgpu_default_device", int(k))
        return self

    def staged_bytes(self) -> int:
        """Bytes of pageable host PCM staged through this context's pinned ring so far (blissgpu_ctx_staged_bytes)."""
        return int(_ffi.call("blissgpu_ctx_staged_bytes", self._h))

    def bind_current_stream(self):
        """Launch on torch's current stream when it is a real stream; the legacy default stream (handle 0) cannot be
        adopted (NULL means "the context's own stream"), so in that case every call below is ordered against it with
        events instead (`_pre` / `_post`)."""
        s = self.torch.cuda.current_stream(self.device).cuda_stream
        _ffi.call("blissgpu_ctx_set_stream", self._h, C.c_void_p(s))

    def _torch_stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _pre(self):
        """the context's stream waits for the inputs torch has queued on its current stream"""
        _ffi.call("blissgpu_ctx_wait_stream", self._h, self._torch_stream())

    def _post(self):
        """torch's current stream waits for the results queued on the context's stream"""
        _ffi.call("blissgpu_ctx_signal_stream", self._h, self._torch_stream())

    def _call(self, name, *args):
        """`name`(this context, *args) between _pre and _post; _post is not run when the call raises"""
        self._pre()
        _ffi.call(name, self._h, *args)
        self._post()

    def _up_f32(self, a):
        """a float32 array uploaded to the context's device; a tensor and None as they are"""
        if a is None or self.torch.is_tensor(a):
            return a
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.torch.device("cuda", self.device))

    def _up_u32(self, a, what):
        """indices (labels, rows, queries) -> a flat int32 tensor on the device holding the uint32 bits; None as it is"""
        torch = self.torch
        if a is None:
            return None
        if torch.is_tensor(a):
            assert a.is_cuda and a.dtype in (torch.int32, torch.int64), what
            return a.to(torch.int32).contiguous().reshape(-1)
        a = np.asarray(a, dtype=np.int64).reshape(-1)
        if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
            raise ValueError(f"{what} must be non-negative indices")
        return torch.from_numpy(a.astype(np.uint32).view(np.int32)).to(torch.device("cuda", self.device))

    def _f32_metric(self, M):
        """the M of the families that also take arrays: uploaded, float32 on the device, contiguous; None as it is"""
        M = self._up_f32(M)
        if M is not None:
            assert M.is_cuda and M.dtype == self.torch.float32
            M = M.contiguous()
        return M

    def _rows(self, X):
        """a float32 [n, d] device tensor, made contiguous"""
        assert X.is_cuda and X.dtype == self.torch.float32 and X.dim() == 2
        return X.contiguous()

    def _rows_pair(self, A, X):
        """two float32 [., d] device tensors over the same d, made contiguous"""
        torch = self.torch
        assert A.is_cuda and X.is_cuda and A.dtype == torch.float32 and X.dtype == torch.float32
        assert A.dim() == 2 and X.dim() == 2 and A.shape[1] == X.shape[1]
        return A.contiguous(), X.contiguous()

    def _i32_per_row(self, t, rows):
        """an int32 device tensor with one entry per row (a skip, the meta keys), made contiguous; None as it is"""
        if t is not None:
            assert t.is_cuda and t.dtype == self.torch.int32 and t.shape[0] == rows
            t = t.contiguous()
        return t

    def _lists(self, q, k, device):
        """the (idx int32 [q, k], dist float32 [q, k]) result pair of a list family, uninitialised"""
        torch = self.torch
        return (torch.empty((q, max(k, 0)), dtype=torch.int32, device=device),
                torch.empty((q, max(k, 0)), dtype=torch.float32, device=device))

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                self._L.blissgpu_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def synchronize(self):
        _ffi.call("blissgpu_ctx_synchronize", self._h)

    OPTIONS = {"serial": _ffi.OPT_SERIAL, "tail_mode": _ffi.OPT_TAIL_MODE, "pipeline_chunks": _ffi.OPT_PIPELINE_CHUNKS,
               "cand_budget": _ffi.OPT_CAND_BUDGET, "rolloff_exact_all": _ffi.OPT_ROLLOFF_EXACT_ALL,
               "debug_chroma": _ffi.OPT_DEBUG_CHROMA, "tail_split": _ffi.OPT_TAIL_SPLIT,
               "stft_shape": _ffi.OPT_STFT_SHAPE, "flux_order": _ffi.OPT_FLUX_ORDER,
               "stage_lanes": _ffi.OPT_STAGE_LANES, "stage_slab_kib": _ffi.OPT_STAGE_SLAB_KIB, "stage_slabs": _ffi.OPT_STAGE_SLABS,
               "stage_numa": _ffi.OPT_STAGE_NUMA, "forest_split": _ffi.OPT_FOREST_SPLIT, "forest_walk": _ffi.OPT_FOREST_WALK,
               "forest_group_nodes": _ffi.OPT_FOREST_GROUP_NODES}

    def set_option(self, name: str, value: int):
        """Scheduling knobs for the measurement tools and the tests (blissgpu_ctx_set_option)."""
        _ffi.call("blissgpu_ctx_set_option", self._h, self.OPTIONS[name], int(value))

    def set_workspace_limit(self, nbytes: int):
        """Scratch bytes of ONE chunk slot; larger batches stream through the two slots in length-bucketed chunks."""
        _ffi.call("blissgpu_ctx_set_workspace_limit", self._h, nbytes)

    def workspace_limit(self) -> int:
        return int(_ffi.call("blissgpu_ctx_get_workspace_limit", self._h))

    def last_chunks(self) -> int:
        """Chunks the last analyze() call was cut into."""
        return int(_ffi.call("blissgpu_debug_last_chunks", self._h))

    # ---- analysis ----
    def analyze(self, pcm, offsets: Sequence[int], lengths: Sequence[int], features_version: int = 2, out=None,
                status=None):
        """pcm: 1-D float32 CUDA tensor holding the songs; returns ([n, d] float32 CUDA tensor, int32 status)."""
        torch = self.torch
        assert pcm.is_cuda and pcm.dtype == torch.float32 and pcm.is_contiguous()
        offsets, lengths = _u64(offsets), _u64(lengths)
        n = len(offsets)
        d = 23 if features_version == 2 else 20
        if out is None:
            out = torch.empty((n, d), dtype=torch.float32, device=pcm.device)
        if status is None:
            status = torch.empty((n,), dtype=torch.int32, device=pcm.device)
        self._call("blissgpu_analyze_batch_device", pcm, offsets, lengths, n, features_version, out, status)
        return out, status

    def synth_white_noise(self, pcm, offsets, lengths, first_song_index: int = 0, song_index=None):
        """Benchmark input: song i gets generator index first_song_index + i, or song_index[i] when given."""
        offsets, lengths = _u64(offsets), _u64(lengths)
        if song_index is None:
            self._call("blissgpu_synth_white_noise_device", pcm, offsets, lengths, len(offsets), first_song_index)
        else:
            idx = np.ascontiguousarray(song_index, np.uint32)
            self._call("blissgpu_synth_white_noise_indexed_device", pcm, offsets, lengths, idx, len(offsets))

    def last_tuning(self, n):
        t = np.empty(n, np.float64)
        b = np.empty(n, np.uint32)
        _ffi.call("blissgpu_debug_last_tuning", self._h, t, b, n)
        return t, b

    TAPS = {"centroid": (0, np.float32), "rolloff": (1, np.float32), "flatness": (2, np.float32),
            "flux": (3, np.float32), "thresholded": (4, np.float32), "run_bpm": (5, np.float32),
            "run_count": (6, np.uint32), "spectrogram": (7, np.float32), "energy256": (8, np.float32),
            "crossings256": (9, np.uint32), "pitch_hist": (10, np.uint32),
            # f64 taps; "chroma" / "interval" need set_option("debug_chroma", 1) before the analysis; for "filter_bank" the
            # `song` argument is the tuning slot (0..99: tuning -0.5 + 0.01 slot, 100: tuning 0.0)
            "chroma": (11, np.float64), "interval": (12, np.float64), "filter_bank": (13, np.float64)}

    def debug_fetch(self, what: str, song: int) -> np.ndarray:
        """Intermediate series of one song of the last chunk (per-stage parity tests)."""
        out = self.debug_fetch_raw(what, song)
        if what == "spectrogram":
            out = out.reshape(-1, 4128)[:, :4097]
        elif what == "filter_bank":
            out = out.reshape(12, 4128)[:, :4097]
        elif what == "chroma":
            out = out.reshape(-1, 12)
        return out

    def debug_fetch_raw(self, what: str, song: int) -> np.ndarray:
        """The tap as the device holds it (flat, padding included)."""
        code, dt = self.TAPS[what]
        n = C.c_uint64()
        probe = np.empty(1, dt)
        _ffi.call("blissgpu_debug_fetch", self._h, code, song, probe, 0, C.byref(n))
        out = np.empty(n.value, dt)
        if n.value:
            _ffi.call("blissgpu_debug_fetch", self._h, code, song, out, n.value, C.byref(n))
        return out

    # ---- distances ----
    def pairwise(self, A, B, metric: str = "euclidean", M=None, out=None):
        torch = self.torch
        assert A.is_cuda and B.is_cuda and A.dtype == torch.float32 and B.dtype == torch.float32
        A, B = A.contiguous(), B.contiguous()
        n, d = A.shape
        m = B.shape[0]
        if out is None:
            out = torch.empty((n, m), dtype=torch.float32, device=A.device)
        M = _contig(M)
        self._call("blissgpu_pairwise_device", A, n, B, m, d, METRICS[metric], M, _dptr(out), out.stride(0))
        return out

    def pcm_s16_to_f32(self, pcm_s16, out=None):
        """On-device s16 -> f32 (sample / 32768): FFmpeg's s16 -> flt conversion (src/song/decoder/ffmpeg.rs:36-109)."""
        torch = self.torch
        assert pcm_s16.is_cuda and pcm_s16.dtype == torch.int16
        pcm_s16 = pcm_s16.contiguous()
        if out is None:
            out = torch.empty(pcm_s16.shape, dtype=torch.float32, device=pcm_s16.device)
        self._call("blissgpu_pcm_s16_to_f32_device", pcm_s16, pcm_s16.numel(), out)
        return out

    def pcm_downmix(self, pcm, out=None):
        """On-device mono downmix of interleaved [frames, channels] decoder output (int16 or float32): stereo ->
        (L + R) * SQRT_2 / 2, more channels -> their mean (src/song/decoder/symphonia.rs:266-300)."""
        torch = self.torch
        assert pcm.is_cuda and pcm.dim() == 2 and pcm.dtype in (torch.int16, torch.float32)
        pcm = pcm.contiguous()
        frames, channels = pcm.shape
        if out is None:
            out = torch.empty((frames,), dtype=torch.float32, device=pcm.device)
        fmt = _ffi.SAMPLE_S16 if pcm.dtype == torch.int16 else _ffi.SAMPLE_F32
        self._call("blissgpu_pcm_downmix_device", pcm, fmt, channels, frames, out)
        return out

    def pcm_decode(self, pcm, sample_rate: int, out=None):
        """On-device conversion of decoder output (1-D mono or [frames, channels]; int16 / int32 / float32) at `sample_rate`
        Hz to the mono 22 050 Hz f32 stream Song::analyze takes: libswresample's default resampler as FFmpegDecoder drives
        it (src/song/decoder/ffmpeg.rs:36-109) -- bit for bit at 44 100 Hz (Adler-32 pins of ffmpeg.rs:433-452, 471-476); other
        rates run the same restatement, held to the oracle only."""
        torch = self.torch
        assert pcm.is_cuda and pcm.dim() in (1, 2) and pcm.dtype in (torch.int16, torch.int32, torch.float32)
        pcm = pcm.contiguous()
        frames = pcm.shape[0]
        channels = 1 if pcm.dim() == 1 else pcm.shape[1]
        n_out = int(_ffi.call("blissgpu_resampled_len", frames, int(sample_rate)))
        if out is None:
            out = torch.empty((n_out,), dtype=torch.float32, device=pcm.device)
        assert out.numel() >= n_out
        fmt = {torch.int16: _ffi.SAMPLE_S16, torch.int32: _ffi.SAMPLE_S32, torch.float32: _ffi.SAMPLE_F32}[pcm.dtype]
        self._call("blissgpu_pcm_decode_device", pcm, fmt, channels, frames, int(sample_rate), out)
        return out[:n_out]

    # ---- FLAC decoded on the device ----
    def flac_slow_songs(self) -> int:
        """Songs of this context whose fast frame table was refused and that went through verified mode."""
        return int(_ffi.call("blissgpu_ctx_flac_slow_songs", self._h))

    def flac_decode(self, data, verified: bool = False, return_frames: bool = False):
        """One .flac file (bytes, a uint8 array, or a path) -> (pcm, sample_rate): the decoder output on the device, interleaved
        [frames, channels] (1-D for mono), int16 = sample << (16 - bps) up to 16 bits per sample, int32 = sample << (32 - bps)
        above -- what the reference's FFmpeg decoder hands to its resampler, and what `pcm_decode` takes.  The host only
        finds the frames (blissgpu_flac_index); every frame is decoded by one lane of flac_decode_kernel.  A frame table of
        the fast mode that the device refuses (a frame that does not stop 2 bytes before the next) is replaced by the
        verified one; what that cannot repair raises DecodingError.
        return_frames: also the per-frame (status, end position) tensors and the table, as they came out of THIS mode."""
        torch = self.torch
        if isinstance(data, (str, os.PathLike)):
            with open(data, "rb") as f:
                data = f.read()
        host = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
        n = int(host.size)
        info = np.zeros(_ffi.FLAC_INFO_WORDS, np.uint64)
        src = host if n else np.zeros(1, np.uint8)
        if _ffi.call_unchecked("blissgpu_flac_info", src, n, info) != _ffi.OK:
            raise DecodingError("not a FLAC stream: " + _ffi.call("blissgpu_last_error").decode())
        channels, bps = int(info[1]), int(info[2])
        if not 4 <= bps <= 24:
            raise DecodingError(f"{bps} bits per sample are not supported")
        nf = C.c_uint64(0)
        _ffi.call_unchecked("blissgpu_flac_index", src, n, int(verified), info, None, 0, C.byref(nf))
        table = np.zeros((max(1, nf.value), 4), np.uint64)
        rc = _ffi.call_unchecked("blissgpu_flac_index", src, n, int(verified), info, table, nf.value, C.byref(nf))
        table = table[:nf.value]
        if rc != _ffi.OK and verified:
            raise DecodingError(_ffi.call("blissgpu_last_error").decode())
        total = int(info[3])
        dev = f"cuda:{self.device}"
        d_bytes = torch.zeros(((n + 16 + 7) // 8) * 8, dtype=torch.uint8, device=dev)
        d_bytes[:n] = torch.from_numpy(host.copy()).to(dev)
        pcm = torch.zeros((total, channels), dtype=torch.int32 if bps > 16 else torch.int16, device=dev)
        status = torch.full((max(1, nf.value),), 8, dtype=torch.int32, device=dev)
        end = torch.zeros((max(1, nf.value),), dtype=torch.int64, device=dev)
        self._call("blissgpu_flac_decode_device", d_bytes, n, table, nf.value, info, pcm, status, end)
        status, end = status[:nf.value], end[:nf.value]
        stops = torch.from_numpy((table[:, 0] + table[:, 1]).astype(np.int64)).to(dev) - 2
        # (the last frame runs to the end of the data in the table and may stop earlier: an ID3v1 tag, padding)
        sound = (rc == _ffi.OK and nf.value > 0 and bool((status == 0).all()) and bool((end[:-1] == stops[:-1]).all())
                 and bool(end[-1] <= stops[-1]))
        out = pcm[:, 0] if channels == 1 else pcm
        if return_frames:
            return out, int(info[0]), status, end, table
        if not sound:
            if verified:
                raise DecodingError("a frame of the stream cannot be decoded")
            return self.flac_decode(host, verified=True)
        return out, int(info[0])

    def flac_crc16(self, data, table, status, end):
        """The CRC-16 of every frame of ONE file on the device (flac_crc_kernel, one wavefront per frame): data -- the file
        (bytes, a uint8 array, or a path); table / status / end as `flac_decode(data, return_frames=True)` returned them.
        -> int32 tensor per frame: 1 = the CRC over [offset, end) equals the two bytes at end, 0 = it does not, -1 = the
        frame's status is not 0 (blissgpu_flac_crc16_device)."""
        torch = self.torch
        if isinstance(data, (str, os.PathLike)):
            with open(data, "rb") as f:
                data = f.read()
        host = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
        nbytes = int(host.size)
        d_bytes = torch.zeros(((nbytes + 16 + 7) // 8) * 8, dtype=torch.uint8, device=status.device)
        d_bytes[:nbytes] = torch.from_numpy(host.copy()).to(status.device)
        table = np.ascontiguousarray(table, np.uint64).reshape(-1, 4)
        nf = int(table.shape[0])
        status = status.contiguous()
        end = end.contiguous()
        assert status.dtype == torch.int32 and end.dtype == torch.int64 and status.numel() >= nf and end.numel() >= nf
        ok = torch.full((max(1, nf),), -2, dtype=torch.int32, device=d_bytes.device)
        self._call("blissgpu_flac_crc16_device", d_bytes, int(nbytes), table, nf, status, end, ok)
        return ok[:nf]

    def flac_md5(self, pcm, bps: int) -> str:
        """The MD5 FLAC defines over the decoded audio, computed on the device by one lane (flac_md5_kernel): pcm -- what
        `flac_decode` returned, [frames, channels] or 1-D, int16 (sample << (16 - bps)) or int32 (sample << (32 - bps)).
        -> the digest as hex, comparable to STREAMINFO's (blissgpu_flac_md5_device)."""
        torch = self.torch
        pcm = pcm.contiguous()
        assert pcm.is_cuda and pcm.dtype == (torch.int32 if bps > 16 else torch.int16) and 4 <= bps <= 24
        frames = int(pcm.shape[0])
        channels = 1 if pcm.dim() == 1 else int(pcm.shape[1])
        info = np.zeros(_ffi.FLAC_INFO_WORDS, np.uint64)
        info[1], info[2], info[3] = channels, bps, frames
        out = torch.zeros(16, dtype=torch.uint8, device=pcm.device)
        self._call("blissgpu_flac_md5_device", pcm if pcm.numel() else None, info, out)  # (no pointer for no samples)
        return bytes(out.cpu().numpy().tobytes()).hex()

    # ---- playlist ordering on device-resident feature matrices (src/playlist.rs:24-59, 256-326) ----
    def _pl_args(self, seeds, cand, M):
        torch = self.torch
        assert seeds.is_cuda and cand.is_cuda and seeds.dtype == torch.float32 and cand.dtype == torch.float32
        seeds, cand = seeds.contiguous(), cand.contiguous()
        if seeds.dim() == 1:
            seeds = seeds[None, :]
        return seeds, cand, _contig(M)

    def set_distance(self, seeds, cand, metric: str = "euclidean", M=None):
        """FunctionDistanceMetric::distance of every candidate row to the seed set."""
        seeds, cand, M = self._pl_args(seeds, cand, M)
        out = self.torch.empty((cand.shape[0],), dtype=self.torch.float32, device=cand.device)
        self._call("blissgpu_set_distance_device", seeds, seeds.shape[0], cand, cand.shape[0], cand.shape[1], METRICS[metric], M,
                   out)
        return out

    def closest_to_songs(self, seeds, cand, metric: str = "euclidean", M=None, return_distances=False):
        """Indices of the candidates sorted (stably) by distance to the seed set (int64 tensor)."""
        torch = self.torch
        seeds, cand, M = self._pl_args(seeds, cand, M)
        n = cand.shape[0]
        order = torch.empty((n,), dtype=torch.int32, device=cand.device)
        dist = torch.empty((n,), dtype=torch.float32, device=cand.device)
        self._call("blissgpu_closest_to_songs_device", seeds, seeds.shape[0], cand, n, cand.shape[1], METRICS[metric], M, order,
                   dist)
        order = order.to(torch.int64)
        return (order, dist) if return_distances else order

    def song_to_song(self, seeds, cand, metric: str = "euclidean", M=None):
        """Greedy nearest-neighbour chain over the candidates (int64 index tensor)."""
        torch = self.torch
        seeds, cand, M = self._pl_args(seeds, cand, M)
        n = cand.shape[0]
        order = torch.empty((n,), dtype=torch.int32, device=cand.device)
        self._call("blissgpu_song_to_song_device", seeds, seeds.shape[0], cand, n, cand.shape[1], METRICS[metric], M, order)
        return order.to(torch.int64)

    def dedup_playlist(self, X, seq=None, meta=None, metric: str = "euclidean", M=None, threshold=None):
        """dedup_playlist_custom_distance over the playlist X[seq] (seq = None: every row): (kept, n_kept) -- kept is an
        int32 tensor of len(seq) slots whose first n_kept (a one-element int64 tensor) hold the kept positions into seq.
        Stays on the device: nothing is copied back.  meta: one int32 key per row of X (playlist.meta_keys) or None.
        Raises BlissGpuError(ERR_NAN) for a NaN distance on the chain of kept songs (synchronises for that check)."""
        torch = self.torch
        assert X.is_cuda and X.dtype == torch.float32 and X.dim() == 2
        X = X.contiguous()
        n, d = X.shape
        length = n if seq is None else seq.shape[0]
        if seq is not None:
            assert seq.is_cuda and seq.dtype == torch.int32
            seq = seq.contiguous()
        meta, M = self._i32_per_row(meta, n), _contig(M)
        kept = torch.empty((max(length, 1),), dtype=torch.int32, device=X.device)
        n_kept = torch.empty((1,), dtype=torch.int64, device=X.device)
        self._call("blissgpu_dedup_playlist_device", X, n, d, seq, length, meta, METRICS[metric], M,
                   float(0.05 if threshold is None else threshold), kept, n_kept)
        return kept[:length], n_kept

    def knn(self, Q, X, k: int, metric: str = "euclidean", M=None, skip=None):
        """The k nearest rows of X for every row of Q without the distance matrix: row i = closest_to_songs(&[Q[i]], X without
        row skip[i], metric) cut after k (src/playlist.rs:256-270, src/library.rs:762-850).  -> (idx int32 [q, k], dist float32
        [q, k]) on the device; equal distances in candidate order; rows with fewer than k eligible candidates end in -1 (the
        library's 0xFFFFFFFF) / inf.  skip: int32 tensor of q candidate indices, -1 = none, or None.  Raises
        BlissGpuError(ERR_NAN) for a NaN among the evaluated distances (synchronises for that check)."""
        Q, X = self._rows_pair(Q, X)
        q, n, k = Q.shape[0], X.shape[0], int(k)
        skip, M = self._i32_per_row(skip, q), _contig(M)
        idx, dist = self._lists(q, k, X.device)
        self._call("blissgpu_knn_device", Q, q, X, n, Q.shape[1], METRICS[metric], M, skip, k, idx, dist)
        return idx, dist

    def scaled_knn(self, Q, qscale, X, cscale, k: int, metric: str = "euclidean", M=None, skip=None):
        """knn under the locally scaled distance dist(i, j) / sqrt(qscale[i] * cscale[j]) (blissgpu_scaled_knn_device, DESIGN.md
        3.27: float32 throughout, the product rounded once, the correctly rounded root, true division).  qscale float32 [q] and
        cscale float32 [n] on the device, every value in [2^-60, 2^60].  -> (idx int32 [q, k], scaled dist float32 [q, k]) on
        the device; equal scaled distances in candidate order; padding -1 / inf and skip as for knn.  Raises BlissGpuError:
        ERR_INVALID for a scale outside the range (NaN included) or a bad skip, ERR_NAN for a NaN among the evaluated distances
        (synchronises for those checks)."""
        torch = self.torch
        Q, X = self._rows_pair(Q, X)
        q, n, k = Q.shape[0], X.shape[0], int(k)
        assert qscale.is_cuda and cscale.is_cuda and qscale.dtype == torch.float32 and cscale.dtype == torch.float32
        qscale, cscale = qscale.contiguous().reshape(-1), cscale.contiguous().reshape(-1)
        if qscale.shape[0] != q or cscale.shape[0] != n:
            raise ValueError("qscale needs one entry per row of Q and cscale one per row of X")
        skip, M = self._i32_per_row(skip, q), _contig(M)
        idx, dist = self._lists(q, k, X.device)
        self._call("blissgpu_scaled_knn_device", Q, q, qscale, X, n, cscale, Q.shape[1], METRICS[metric], M, skip, k, idx, dist)
        return idx, dist

    def knn_occurrence(self, idx, n: int):
        """In how many lists every song is (blissgpu_knn_occurrence_device): idx int32 [q, k] on the device as knn returns it
        (-1 = padding, ignored) -> count int32 [n] on the device, count[j] = the entries equal to j.  Raises
        BlissGpuError(ERR_INVALID) for any other entry outside 0 .. n - 1 (synchronises for that check)."""
        torch = self.torch
        assert idx.is_cuda and idx.dtype == torch.int32 and idx.dim() == 2
        idx = idx.contiguous()
        q, k, n = idx.shape[0], idx.shape[1], int(n)
        count = torch.empty((max(n, 0),), dtype=torch.int32, device=idx.device)
        # (this entry point is given no pointer for an empty tensor)
        self._call("blissgpu_knn_occurrence_device", idx if idx.numel() else None, q, k, n, count if count.numel() else None)
        return count

    def kmeans(self, X, init, max_iter: int = 100, metric: str = "euclidean", M=None):
        """Lloyd's k-means of the rows of X from the centres `init` [k, d], iterated on the device (blissgpu_kmeans_device,
        DESIGN.md 3.21): nearest centre by the all-pairs kernel's distances with ties to the lower centre, sequential f32 means in
        row order, an empty cluster keeps its centre, stop when no label moves or after max_iter updates.  X and init are
        float32 tensors on the device, or numpy arrays (uploaded, results returned as arrays).  -> (labels int32 [n], dist float32
        [n], centroids float32 [k, d], sizes int32 [k], n_iter, converged).  metric: "euclidean" or "mahalanobis" with M.  Raises
        BlissGpuError(ERR_NAN) for a NaN among the evaluated distances; synchronises once per iteration."""
        torch = self.torch
        as_numpy = not torch.is_tensor(X)
        X, init = self._rows_pair(self._up_f32(X), self._up_f32(init))
        M = self._f32_metric(M)
        (n, d), k = X.shape, init.shape[0]
        labels = torch.empty((n,), dtype=torch.int32, device=X.device)
        dist = torch.empty((n,), dtype=torch.float32, device=X.device)
        cent = torch.empty((k, d), dtype=torch.float32, device=X.device)
        sizes = torch.empty((k,), dtype=torch.int32, device=X.device)
        n_iter, conv = C.c_uint32(0), C.c_int32(0)
        self._call("blissgpu_kmeans_device", X, n, d, init, k, METRICS[metric], M, int(max_iter), labels, dist, cent, sizes,
                   C.byref(n_iter), C.byref(conv))
        if as_numpy:
            labels, dist, cent, sizes = (t.cpu().numpy() for t in (labels, dist, cent, sizes))
        return labels, dist, cent, sizes, int(n_iter.value), bool(conv.value)

    def kmeans_stats(self):
        """(device-to-host copies inside the loop, their bytes) of the last kmeans on this context: one pair of flag words per
        assignment."""
        a, b = C.c_uint64(), C.c_uint64()
        _ffi.call("blissgpu_debug_kmeans_stats", self._h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def silhouette(self, X, labels, metric: str = "euclidean", M=None, rows=None, col_groups: int = 0, k: int = None):
        """The silhouette of the labelling `labels` of the rows of X on the device, without the distance matrix
        (blissgpu_silhouette_device): for every scored song a = the mean distance to the other songs of its own
        cluster, b = the smallest mean distance to another non-empty cluster, s = (b - a) / max(a, b), all defined to the bit by
        include/blissgpu.h.  X float32 [n, d] and labels (int32 / int64, every one in 0 .. k - 1) are tensors on the device, or
        numpy arrays (uploaded, results returned as arrays); rows: the songs to score (any order, repeats allowed), None = all;
        k: the number of clusters, None = labels.max() + 1.
        -> (s float32 [q], a float64 [q], b float64 [q], neighbour int32 [q], sizes int32 [k]).  col_groups: 0 = the plan's
        choice; no result bit depends on it.  Raises BlissGpuError: ERR_NAN for a NaN among the evaluated distances, ERR_INVALID
        for a label >= k, fewer than two non-empty clusters or a rows entry past n; synchronises once."""
        torch = self.torch
        as_numpy = not torch.is_tensor(X)
        X = self._up_f32(X)
        labels, rows = self._up_u32(labels, "labels"), self._up_u32(rows, "rows")
        X = self._rows(X)
        n, d = X.shape
        if labels.shape[0] != n:
            raise ValueError("a label per row of X is needed")
        M = self._f32_metric(M)
        if k is None:
            k = int(labels.max().item()) + 1 if n else 1
        q = n if rows is None else rows.shape[0]
        s = torch.zeros((q,), dtype=torch.float32, device=X.device)
        a = torch.zeros((q,), dtype=torch.float64, device=X.device)
        b = torch.zeros((q,), dtype=torch.float64, device=X.device)
        nb = torch.full((q,), -1, dtype=torch.int32, device=X.device)
        sizes = torch.zeros((max(int(k), 0),), dtype=torch.int32, device=X.device)
        self._call("blissgpu_silhouette_device", X, n, d, labels, int(k), METRICS[metric], M, rows, q, int(col_groups), s, a, b, nb,
                   sizes)
        out = (s, a, b, nb, sizes)
        return tuple(t.cpu().numpy() for t in out) if as_numpy else out

    def group_neighbours(self, X, labels, k: int = None, t: int = 1, metric: str = "euclidean", M=None, queries=None,
                         mode: str = "symmetric", slab_groups: int = 0, want_matrix: bool = False):
        """The t nearest groups of every queried group of the labelling `labels` of the rows of X under the average
        nearest-member (Chamfer) distance, on the device without the distance matrix (blissgpu_group_neighbours_device,
        DESIGN.md 3.25), all defined to the bit by include/blissgpu.h.  X float32 [n, d] and labels (int32 / int64, every one in
        0 .. k - 1) are tensors on the device, or numpy arrays (uploaded, results returned as arrays); k: the number of groups,
        None = labels.max() + 1; queries: the groups to answer for (any order, repeats allowed), None = all k in order; mode
        "symmetric" or "directed".
        -> (idx int32 [q, t] with -1 as padding, dist float64 [q, t] with +inf as padding, sizes int32 [k], matrix float64 [k, k]
        or None unless `want_matrix`).  slab_groups: 0 = the plan's choice; no result bit depends on it.  Raises BlissGpuError:
        ERR_NAN for a NaN among the evaluated distances, ERR_INVALID for a label or a query >= k, ERR_OOM when the workspace does
        not fit the context's limit; synchronises once."""
        torch = self.torch
        as_numpy = not torch.is_tensor(X)
        if mode not in GROUP_MODES:
            raise ValueError(f"mode must be one of {tuple(GROUP_MODES)}")
        X = self._up_f32(X)
        labels, queries = self._up_u32(labels, "labels"), self._up_u32(queries, "queries")
        X = self._rows(X)
        n, d = X.shape
        if labels.shape[0] != n:
            raise ValueError("a label per row of X is needed")
        M = self._f32_metric(M)
        if k is None:
            k = int(labels.max().item()) + 1 if n else 1
        k, t = int(k), int(t)
        q = max(k, 0) if queries is None else queries.shape[0]
        idx = torch.full((q, max(t, 0)), -1, dtype=torch.int32, device=X.device)
        dist = torch.full((q, max(t, 0)), float("inf"), dtype=torch.float64, device=X.device)
        sizes = torch.zeros((max(k, 0),), dtype=torch.int32, device=X.device)
        matrix = torch.zeros((max(k, 0), max(k, 0)), dtype=torch.float64, device=X.device) if want_matrix else None
        self._call("blissgpu_group_neighbours_device", X, n, d, labels, k, METRICS[metric], M, queries, q, t, GROUP_MODES[mode],
                   int(slab_groups), idx, dist, sizes, matrix)
        out = (idx, dist, sizes, matrix)
        return tuple(None if a is None else a.cpu().numpy() for a in out) if as_numpy else out

    def mst(self, X, metric: str = "euclidean", M=None, core=None):
        """The minimum spanning tree of the rows of X on the device without the distance matrix (blissgpu_mst_device,
        DESIGN.md 3.26): the unique tree under the edge order (bits of the f32 weight, lower row, higher row) of
        include/blissgpu.h, with weight = the all-pairs distance, or max(distance, core[i], core[j]) when `core` (float32 [n],
        every value >= 0) is given.  X float32 [n, d], M and core are tensors on the device, or numpy arrays (uploaded, results
        returned as arrays).  -> (u int32 [n - 1], v int32 [n - 1], w float32 [n - 1], rounds): the edges in ascending order,
        u < v, and the number of Boruvka rounds run.  metric: "euclidean" or "mahalanobis" with M.  Raises BlissGpuError:
        ERR_INVALID for cosine, a NaN distance or a bad core, ERR_OOM when the workspace does not fit the context's limit;
        synchronises once per round."""
        torch = self.torch
        as_numpy = not torch.is_tensor(X)
        X, M, core = self._rows(self._up_f32(X)), self._f32_metric(M), self._up_f32(core)
        n, d = X.shape
        if core is not None:
            assert core.is_cuda and core.dtype == torch.float32
            core = core.contiguous().reshape(-1)
            if core.shape[0] != n:
                raise ValueError("a core distance per row of X is needed")
        m = max(n - 1, 0)
        u = torch.empty((m,), dtype=torch.int32, device=X.device)
        v = torch.empty((m,), dtype=torch.int32, device=X.device)
        w = torch.empty((m,), dtype=torch.float32, device=X.device)
        rounds = C.c_uint32(0)
        self._call("blissgpu_mst_device", X, n, d, METRICS[metric], M, core, u, v, w, C.byref(rounds))
        if as_numpy:
            u, v, w = (t.cpu().numpy() for t in (u, v, w))
        return u, v, w, int(rounds.value)

    def moments(self, X, labels=None, k: int = None, scatter: bool = True):
        """The first and second moments of the rows of X on the device (blissgpu_moments_device), per group of
        the labelling `labels` and pooled, every sum the blocked sum of include/blissgpu.h.  X float32 [n, d] and labels (int32 /
        int64, every one in 0 .. k - 1; None: one group) are tensors on the device, or numpy arrays (uploaded, results returned as
        arrays); k: the number of groups, None = labels.max() + 1.
        -> (counts int32 [k], mean float64 [k, d], m2 float64 [k, d], min float32 [k, d], max float32 [k, d], S float64 [d, d] or
        None when `scatter` is False).  S is the pooled within-group scatter (without labels: the total scatter).  Raises
        BlissGpuError: ERR_NAN for a NaN or an infinity in X, ERR_INVALID for a label >= k; synchronises once."""
        torch = self.torch
        as_numpy = not torch.is_tensor(X)
        X = self._rows(self._up_f32(X))
        n, d = X.shape
        if labels is not None:
            labels = self._up_u32(labels, "labels")
            if labels.shape[0] != n:
                raise ValueError("a label per row of X is needed")
            if k is None:
                k = int(labels.max().item()) + 1 if n else 1
        elif k is None:
            k = 1
        k = int(k)
        kk = max(k, 0)
        counts = torch.zeros((kk,), dtype=torch.int32, device=X.device)
        mean = torch.zeros((kk, d), dtype=torch.float64, device=X.device)
        m2 = torch.zeros((kk, d), dtype=torch.float64, device=X.device)
        mn = torch.zeros((kk, d), dtype=torch.float32, device=X.device)
        mx = torch.zeros((kk, d), dtype=torch.float32, device=X.device)
        S = torch.zeros((d, d), dtype=torch.float64, device=X.device) if scatter else None
        self._call("blissgpu_moments_device", X, n, d, labels, k, counts, mean, m2, mn, mx, S)
        out = (counts, mean, m2, mn, mx, S)
        return tuple(None if t is None else t.cpu().numpy() for t in out) if as_numpy else out

    def triplet_step(self, X, triplets, M=None, margin: float = 0.0, return_flags: bool = False):
        """One gradient evaluation of triplet metric learning (blissgpu_triplet_step_device) on device tensors:
        X float32 [n, d], triplets int32 [T, 3] as (a, b, o) (int64 is converted), M float32 [d, d] or None for the identity.
        -> (n_active, loss, G float64 numpy [d, d]) and, return_flags, a uint8 tensor [T] on the device.  Synchronises."""
        torch = self.torch
        assert X.is_cuda and X.dtype == torch.float32 and X.dim() == 2
        X = X.contiguous()
        triplets = triplets.to(torch.int32).contiguous() if triplets.dtype != torch.int32 else triplets.contiguous()
        assert triplets.is_cuda and (triplets.numel() == 0 or (triplets.dim() == 2 and triplets.shape[1] == 3))
        (n, d), T = X.shape, triplets.numel() // 3
        if M is not None:
            assert M.is_cuda and M.dtype == torch.float32 and tuple(M.shape) == (d, d)
            M = M.contiguous()
        flags = torch.zeros((T,), dtype=torch.uint8, device=X.device) if return_flags else None
        G = np.zeros((d, d), np.float64)
        n_active, loss = C.c_uint64(0), C.c_double(0.0)
        self._call("blissgpu_triplet_step_device", X, n, d, triplets if T else None, T, M, float(margin), flags if T else None,
                   C.byref(n_active), C.byref(loss), G)
        out = (int(n_active.value), float(loss.value), G)
        return out + (flags,) if return_flags else out

    def learn_metric(self, X, triplets, form: str = "full", init=None, margin: float = None, lr: float = None, reg: float = 0.0,
                     max_iter: int = None):
        """playlist.learn_metric on device tensors (blissgpu_learn_metric_device): X float32 [n, d] and triplets int32 [T, 3]
        stay where they are, an iteration uploads M and downloads the gradient.  init: d host weights or None.
        -> playlist.LearnedMetric (host arrays)."""
        torch = self.torch
        margin = P.LEARN_MARGIN if margin is None else margin
        lr = P.LEARN_LR if lr is None else lr
        max_iter = P.LEARN_MAX_ITER if max_iter is None else max_iter
        assert X.is_cuda and X.dtype == torch.float32 and X.dim() == 2
        X = X.contiguous()
        triplets = triplets.to(torch.int32).contiguous() if triplets.dtype != torch.int32 else triplets.contiguous()
        assert triplets.is_cuda
        (n, d), T = X.shape, triplets.numel() // 3
        init, max_iter = P._learn_args(form, init, d, max_iter)
        M, obj, act = np.zeros((d, d), np.float32), np.zeros(max_iter + 1, np.float64), np.zeros(max_iter + 1, np.uint64)
        n_iter, best_iter, status = C.c_uint32(0), C.c_uint32(0), C.c_int32(0)
        self._call("blissgpu_learn_metric_device", X, n, d, triplets if T else None, T, FORMS[form], init, float(margin), float(lr),
                   float(reg), max_iter, M, obj, act, C.byref(n_iter), C.byref(best_iter), C.byref(status))
        return P._learned(M, obj, act, n_iter, best_iter, status)

    def metric_stats(self):
        """(uploads, downloads, bytes downloaded) inside the loop of the last learn_metric on this context: one M up and one
        result block down per gradient evaluation."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _ffi.call("blissgpu_debug_metric_stats", self._h, C.byref(a), C.byref(b), C.byref(c))
        return int(a.value), int(b.value), int(c.value)

    def group_weights(self, S, offsets):
        """variance_based_weight_matrix (src/playlist.rs:173-221) of every seed group on the device: group g's seeds are the
        rows offsets[g] .. offsets[g + 1] of S (offsets: a HOST sequence of G + 1 integers starting at 0).  -> (weights float32
        [G, d], status int32 [G]) on the device: row g is the DIAGONAL of the reference's matrix; a group of fewer than two
        seeds gets ones and status 1 (BLISSGPU_GROUP_TOO_FEW_SEEDS), every other group status 0."""
        torch = self.torch
        S = self._rows(S)
        off, G = _offsets(offsets, S.shape[0])
        d = S.shape[1]
        weights = torch.empty((G, d), dtype=torch.float32, device=S.device)
        status = torch.empty((G,), dtype=torch.int32, device=S.device)
        self._call("blissgpu_group_weights_device", S, off, G, d, weights, status)
        return weights, status

    def group_knn(self, S, offsets, X, k: int, metric: str = "euclidean", M=None, skip=None, weights=None):
        """The k nearest rows of X for every seed GROUP without a groups x candidates matrix: group g's seeds are the rows
        offsets[g] .. offsets[g + 1] of S (offsets: a HOST sequence of G + 1 integers starting at 0), its row =
        closest_to_songs(those seeds, X without the group's skipped rows, metric) cut after k (src/playlist.rs:36-59, 256-270,
        src/library.rs:762-842); a candidate's score is the sequential f32 sum over the seeds in order.  -> (idx int32 [G, k],
        dist float32 [G, k]) on the device; equal scores in candidate order; rows with fewer than k eligible candidates end in
        -1 (the library's 0xFFFFFFFF) / inf.  skip: int32 tensor with one candidate index per SEED ROW, -1 = none, or None.
        Raises BlissGpuError(ERR_NAN) for a NaN among the scores (synchronises for that check).
        `weights` (metric and M are then not looked at): one DIAGONAL Mahalanobis metric per group, M_g = diag(weights[g]) -- a
        float32 [G, d] tensor, or the string "variance" for the variance-based weights of each group's own seeds, computed on
        the device (group_weights) in the same call.  -> (idx, dist, status int32 [G]): status as group_weights returns it
        (all 0 with given weights)."""
        torch = self.torch
        S, X = self._rows_pair(S, X)
        off, G = _offsets(offsets, S.shape[0])
        n, k = X.shape[0], int(k)
        skip, M = self._i32_per_row(skip, S.shape[0]), _contig(M)
        idx, dist = self._lists(G, k, X.device)
        if weights is not None:
            if isinstance(weights, str):
                if weights != "variance":
                    raise ValueError('weights must be a [G, d] tensor or "variance"')
                weights = None
            else:
                assert weights.is_cuda and weights.dtype == torch.float32 and tuple(weights.shape) == (G, X.shape[1])
                weights = weights.contiguous()
            status = torch.empty((G,), dtype=torch.int32, device=X.device)
            self._call("blissgpu_group_knn_weighted_device", S, off, G, X, n, X.shape[1], weights, skip, k, idx, dist, status)
            return idx, dist, status
        self._call("blissgpu_group_knn_device", S, off, G, X, n, X.shape[1], METRICS[metric], M, skip, k, idx, dist)
        return idx, dist

    def chains(self, S, offsets, X, k: int, metric: str = "euclidean", M=None, skip=None, route: str = "auto"):
        """The first k songs of song_to_song(group, X without the group's skipped rows, metric) (src/playlist.rs:272-326) for
        every seed GROUP in one call: group g's seeds are the rows offsets[g] .. offsets[g + 1] of S (offsets: a HOST sequence of
        G + 1 integers starting at 0).  Song 0 is the candidate closest to the seed set (group_knn's score), song t the candidate
        not yet taken that is closest to song t - 1; equal distances go to the lower index.  -> (idx int32 [G, k], dist float32
        [G, k]) on the device; rows with fewer than k eligible candidates end in -1 (the library's 0xFFFFFFFF) / inf.  skip:
        int32 tensor with one candidate index per SEED ROW, -1 = none, or None.  route: "auto", "steps" (a launch per step) or
        "lists" (the candidates' own k-nearest lists, then one walk); the result does not depend on it.  Raises
        BlissGpuError(ERR_NAN) for a NaN among the distances a chain evaluates (synchronises for that check)."""
        S, X = self._rows_pair(S, X)
        off, G = _offsets(offsets, S.shape[0])
        n, k = X.shape[0], int(k)
        skip, M = self._i32_per_row(skip, S.shape[0]), _contig(M)
        idx, dist = self._lists(G, k, X.device)
        self._call("blissgpu_chains_device", S, off, G, X, n, X.shape[1], METRICS[metric], M, skip, k, ROUTES[route], idx, dist)
        return idx, dist

    def journeys(self, A, B, X, k: int, metric: str = "euclidean", M=None, skip=None, mode: str = "chain", gate: str = None,
                 feature: int = 0):
        """Waypoint and directed song-to-song playlists (blissgpu_journeys_device; the reference only names them, TODO.md "New
        features"), k steps for every journey in one call.  Journey g starts at row g of A.  mode "chain": step 0 picks the
        candidate nearest A[g], step t the candidate nearest the previous pick; `gate` "up" / "down" additionally keeps only
        the candidates whose column `feature` is >= / <= that of the previous pick (of A[g] at step 0; equality passes, a NaN
        on either side does not).  mode "waypoint" (B given, no gate): step t picks the candidate nearest
        A[g] + (B[g] - A[g]) * ((t + 1) / (k + 1)).  A picked candidate is never picked again; skip: int32 tensor [G, 2] of
        candidate indices that are never eligible, -1 = none, or None.  -> (idx int32 [G, k], dist float32 [G, k]) on the
        device; a journey that runs out of eligible candidates ends in -1 (the library's 0xFFFFFFFF) / inf.  Raises
        BlissGpuError(ERR_NAN) for a NaN distance of an eligible candidate (synchronises for that check)."""
        torch = self.torch
        A, X = self._rows_pair(A, X)
        G, n, k = A.shape[0], X.shape[0], int(k)
        if B is not None:
            assert B.is_cuda and B.dtype == torch.float32 and tuple(B.shape) == tuple(A.shape)
            B = B.contiguous()
        if skip is not None:
            assert skip.is_cuda and skip.dtype == torch.int32 and tuple(skip.shape) == (G, 2)
            skip = skip.contiguous()
        M = _contig(M)
        idx, dist = self._lists(G, k, X.device)
        self._call("blissgpu_journeys_device", A, B, G, X, n, X.shape[1], METRICS[metric], M, skip, k, JOURNEY_MODES[mode],
                   GATES[gate], int(feature), idx, dist)
        return idx, dist

    def radio(self, A, X, k: int, labels=None, windows=(), limits=(), from_labels=None, mode: str = "chain",
              metric: str = "euclidean", M=None, skip=None):
        """Radio playlists (blissgpu_radio_device): song-to-song chains (mode "chain") or the k nearest songs
        (mode "nearest") from every row of A under label rules, k steps for every radio in one call.  labels: int32 tensor
        [R, n], one label per rule and candidate (artist id, album id, ...), -1 = no label; from_labels: int32 tensor [G, R],
        the start songs' labels, or None; windows / limits: HOST sequences of R integers -- among the last windows[r] songs of a
        radio (the start song is the one before the first) at most limits[r] carry any one label; windows[r] == 0 switches the
        rule off, windows[r] > k is the whole list.  A picked candidate is never picked again; skip: int32 tensor [G, 2] of
        candidate indices that are never eligible, -1 = none, or None.  -> (idx int32 [G, k], dist float32 [G, k]) on the
        device; a radio that runs out of eligible candidates ends in -1 (the library's 0xFFFFFFFF) / inf.  Raises
        BlissGpuError(ERR_NAN) for a NaN distance of an eligible candidate (synchronises for that check)."""
        torch = self.torch
        A, X = self._rows_pair(A, X)
        G, n, k = A.shape[0], X.shape[0], int(k)
        win = np.ascontiguousarray(np.minimum(np.asarray(windows, np.int64).reshape(-1), 0xFFFFFFFF), dtype=np.uint32)
        lim = np.ascontiguousarray(np.minimum(np.asarray(limits, np.int64).reshape(-1), 0xFFFFFFFF), dtype=np.uint32)
        R = win.shape[0]
        assert lim.shape[0] == R
        if R:
            assert labels is not None and labels.is_cuda and labels.dtype == torch.int32 and tuple(labels.shape) == (R, n)
            labels = labels.contiguous()
        else:
            labels = None
        if from_labels is not None and R:
            assert from_labels.is_cuda and from_labels.dtype == torch.int32 and tuple(from_labels.shape) == (G, R)
            from_labels = from_labels.contiguous()
        else:
            from_labels = None
        if skip is not None:
            assert skip.is_cuda and skip.dtype == torch.int32 and tuple(skip.shape) == (G, 2)
            skip = skip.contiguous()
        M = _contig(M)
        idx, dist = self._lists(G, k, X.device)
        self._call("blissgpu_radio_device", A, G, X, n, X.shape[1], METRICS[metric], M, labels, from_labels, R, win if R else None,
                   lim if R else None, skip, k, RADIO_MODES[mode], idx, dist)
        return idx, dist

    def album_knn(self, S, offsets, X, album_of, n_albums: int, k: int, skip=None):
        """The k nearest ALBUMS of every seed group (blissgpu_album_knn_device): closest_album_to_group (src/playlist.rs:424-485)
        cut after k albums.  Group g's seeds are the rows offsets[g] .. offsets[g + 1] of S (offsets: a HOST sequence of G + 1
        integers starting at 0, no group empty); album_of: int32 tensor [n], the album index 0 .. n_albums of every row of X,
        -1 = no album; skip: int32 tensor with one candidate index per SEED ROW, -1 = none, or None: those rows leave their
        albums before the group's album means are formed.  -> (idx int32 [G, k], dist float32 [G, k], group_means float32
        [G, d], centroids float32 [n_albums, d]) on the device: the albums in ascending (euclidean distance of the album's mean
        to the group's mean, album index), rows with fewer than k existing albums ending in -1 / inf; centroids are the
        full-album means, NaN rows for albums without songs.  Raises BlissGpuError(ERR_NAN) for a NaN distance (album_of and
        skip are read back, which synchronises)."""
        torch = self.torch
        S, X = self._rows_pair(S, X)
        off, G = _offsets(offsets, S.shape[0])
        n, d, k, A = X.shape[0], X.shape[1], int(k), int(n_albums)
        assert album_of.is_cuda and album_of.dtype == torch.int32 and album_of.shape[0] == n
        album_of = album_of.contiguous()
        skip = self._i32_per_row(skip, S.shape[0])
        idx, dist = self._lists(G, k, X.device)
        means = torch.empty((G, d), dtype=torch.float32, device=X.device)
        centroids = torch.empty((max(A, 0), d), dtype=torch.float32, device=X.device)
        self._call("blissgpu_album_knn_device", S, off, G, X, n, d, album_of, A, skip, k, idx, dist, means, centroids)
        return idx, dist, means, centroids

    def duplicate_labels(self, x, meta=None, metric: str = "euclidean", m=None, threshold=0.05, max_pairs: int = 0):
        """Which rows of x are the same song (blissgpu_duplicate_groups_device): the pair i < j is an edge when its distance
        is < threshold or meta[i] != 0 and meta[i] == meta[j] (int32 keys, playlist.meta_keys; None: no such rule).  ->
        (labels, n_pairs): labels an int32 tensor, the smallest row of each row's connected component; n_pairs a one-element
        int64 tensor, the number of edges.  With max_pairs > 0 -> (labels, n_pairs, pairs int32 [max_pairs, 2], dist float32
        [max_pairs]): the first n_pairs entries hold the edges in unspecified order when n_pairs <= max_pairs, otherwise the
        contents are unspecified.  Stays on the device; raises BlissGpuError(ERR_NAN) for a NaN distance (synchronises for
        that check)."""
        torch = self.torch
        x = self._rows(x)
        n, d = x.shape
        meta, m = self._i32_per_row(meta, n), _contig(m)
        max_pairs = int(max_pairs)
        labels = torch.empty((max(n, 1),), dtype=torch.int32, device=x.device)
        n_pairs = torch.empty((1,), dtype=torch.int64, device=x.device)
        pairs = dist = None
        if max_pairs > 0:
            pairs = torch.empty((max_pairs, 2), dtype=torch.int32, device=x.device)
            dist = torch.empty((max_pairs,), dtype=torch.float32, device=x.device)
        self._call("blissgpu_duplicate_groups_device", x, n, d, meta, METRICS[metric], m, float(threshold), labels, n_pairs, pairs,
                   dist, max(max_pairs, 0))
        if max_pairs > 0:
            return labels[:n], n_pairs, pairs, dist
        return labels[:n], n_pairs

    # ---- the isolation-forest metric on device-resident candidates (src/playlist.rs:230-251) ----
    def forest_scores(self, forest, cand, return_path_sum=False):
        """Scores of the candidate rows against a playlist.Forest (float32 tensor; with return_path_sum also the exact
        integer path sums as an int64 tensor).  The forest is uploaded to this device on first use.  Asynchronous."""
        torch = self.torch
        assert cand.is_cuda and cand.dtype == torch.float32 and cand.dim() == 2 and (cand.shape[0] == 0 or cand.shape[1] == forest.d)
        cand = cand.contiguous()
        n = cand.shape[0]
        score = torch.empty((n,), dtype=torch.float32, device=cand.device)
        ps = torch.empty((n,), dtype=torch.int64, device=cand.device) if return_path_sum else None
        self._call("blissgpu_forest_score_device", forest.handle, cand, n, score, ps)
        return (score, ps) if return_path_sum else score

    def forest_closest_to_songs(self, forest, cand, return_scores=False):
        """Indices of the candidates sorted (stably) by their forest score (int64 tensor): closest_to_songs with a
        ForestOptions metric."""
        torch = self.torch
        assert cand.is_cuda and cand.dtype == torch.float32 and cand.dim() == 2 and (cand.shape[0] == 0 or cand.shape[1] == forest.d)
        cand = cand.contiguous()
        n = cand.shape[0]
        order = torch.empty((n,), dtype=torch.int32, device=cand.device)
        score = torch.empty((n,), dtype=torch.float32, device=cand.device)
        self._call("blissgpu_forest_closest_to_songs_device", forest.handle, cand, n, order, score)
        order = order.to(torch.int64)
        return (order, score) if return_scores else order

    def group_forest_knn(self, S, offsets, X, k: int, options, skip=None, seeds_host=None):
        """The k lowest isolation-forest scores of the rows of X for every seed GROUP (blissgpu_group_forest_knn_device): group
        g's forest is playlist.Forest(S[offsets[g]:offsets[g + 1]], options), every group with the same options and seed.
        -> (idx int32 [G, k], score float32 [G, k], status int32 [G]) on the device: row g = the first k of the stable ascending
        order of that forest's scores over X without the group's skipped rows, ending in -1 / inf where fewer are eligible;
        status 1 (BLISSGPU_GROUP_TOO_FEW_SEEDS) and a row of padding for a group with min(sample_size, seeds) < 2.
        skip: int32 tensor with one candidate index per SEED ROW, -1 = none, or None.  The forests are built on the host:
        `seeds_host` (a float32 array equal to S) saves the device-to-host copy of S.  Synchronises before it returns."""
        torch = self.torch
        S, X = self._rows_pair(S, X)
        off, G = _offsets(offsets, S.shape[0])
        n, k = X.shape[0], int(k)
        skip = self._i32_per_row(skip, S.shape[0])
        hs = None
        if seeds_host is not None:
            hs = np.ascontiguousarray(seeds_host, dtype=np.float32)
            assert hs.shape == tuple(S.shape)
        idx, score = self._lists(G, k, X.device)
        status = torch.empty((G,), dtype=torch.int32, device=X.device)
        self._call("blissgpu_group_forest_knn_device", S, hs, off, G, X, n, X.shape[1], options.n_trees, options.sample_size,
                   options.max_tree_depth or 0, options.extension_level, options.seed, skip, k, idx, score, status)
        return idx, score, status

    def group_forest_stats(self):
        """(host ms building forests, host ms waiting for the device, batches) of the last group_forest_knn on this context."""
        a, b, nb = C.c_double(), C.c_double(), C.c_uint64()
        _ffi.call("blissgpu_debug_group_forest_stats", self._h, C.byref(a), C.byref(b), C.byref(nb))
        return a.value, b.value, int(nb.value)

    # ---- profiling ----
    def profile_enable(self, on: bool = True):
        _ffi.call("blissgpu_profile_enable", self._h, int(on))

    def profile_reset(self):
        _ffi.call("blissgpu_profile_reset", self._h)

    def profile(self):
        """{kernel name: (total_ms, launches)} since the last reset."""
        res = {}
        for k in range(_ffi.call("blissgpu_profile_kernel_count")):
            ms, n = C.c_double(), C.c_uint64()
            _ffi.call("blissgpu_profile_get", self._h, k, C.byref(ms), C.byref(n))
            if n.value:
                res[_ffi.call("blissgpu_profile_kernel_name", k).decode()] = (ms.value, n.value)
        return res


class Node:
    """blissgpu_node wrapper: ONE process driving several GPUs (RCCL all-gather of the feature rows inside the
    library).  The one-process-per-GPU form on torch.distributed is bliss_rs_amd.shard."""

    def __init__(self, n_devices: int = 1, devices: Optional[Sequence[int]] = None):
        self._L = _ffi.lib()
        h = C.c_void_p()
        dev = (C.c_int * n_devices)(*devices) if devices is not None else None
        _ffi.call("blissgpu_node_create", n_devices, dev, C.byref(h))
        self._h = h
        self.n_devices = n_devices

    def close(self):
        if getattr(self, "_h", None):
            self._L.blissgpu_node_destroy(self._h)
            self._h = None

    __del__ = close

    def synth_white_noise(self, rank: int, d_pcm_ptr: int, offsets, lengths, song_index):
        """Benchmark input on `rank`'s device: song i (at d_pcm_ptr + offsets[i]) gets generator index song_index[i]."""
        offsets, lengths = _u64(offsets), _u64(lengths)
        idx = np.ascontiguousarray(song_index, np.uint32)
        ctx = _ffi.call("blissgpu_node_ctx", self._h, rank)
        _ffi.call("blissgpu_synth_white_noise_indexed_device", ctx, C.c_void_p(int(d_pcm_ptr)), offsets, lengths, idx, len(offsets))
        _ffi.call("blissgpu_ctx_synchronize", ctx)

    def ctx_set_workspace_limit(self, rank: int, nbytes: int):
        """Scratch bytes of one chunk slot of `rank`'s context (several loopback ranks share one GPU's memory)."""
        _ffi.call("blissgpu_ctx_set_workspace_limit", _ffi.call("blissgpu_node_ctx", self._h, rank), nbytes)

    def shard(self, lengths) -> np.ndarray:
        lengths = _u64(lengths)
        ranks = np.empty(len(lengths), np.uint32)
        _ffi.call("blissgpu_node_shard", self._h, lengths, len(lengths), ranks)
        return ranks

    def row_block(self, n_rows: int, rank: int):
        lo, hi = C.c_uint64(), C.c_uint64()
        _ffi.call("blissgpu_node_row_block", self._h, n_rows, rank, C.byref(lo), C.byref(hi))
        return lo.value, hi.value

    def analyze(self, pcm: np.ndarray, offsets, lengths, features_version: int = 2):
        """Host PCM -> ([n, d] float32, int32 status); the gathered matrix stays on every device for pairwise()."""
        pcm = np.ascontiguousarray(pcm, np.float32)
        offsets, lengths = _u64(offsets), _u64(lengths)
        n = len(offsets)
        d = 23 if features_version == 2 else 20
        out = np.empty((n, d), np.float32)
        status = np.empty(n, np.int32)
        _ffi.call("blissgpu_node_analyze", self._h, pcm, offsets, lengths, n, features_version, out, status)
        _ffi.call("blissgpu_node_synchronize", self._h)
        self._n, self._d = n, d
        return out, status

    def analyze_device(self, d_pcm_ptrs: Sequence[int], offsets, lengths, rank_of_song, features_version: int = 2):
        """Device-resident PCM: song i lives on device rank_of_song[i] at d_pcm_ptrs[rank] + offsets[i] (raw pointers)."""
        offsets, lengths = _u64(offsets), _u64(lengths)
        ranks = np.ascontiguousarray(rank_of_song, np.uint32)
        ptrs = (C.c_void_p * self.n_devices)(*[C.c_void_p(int(p)) for p in d_pcm_ptrs])
        _ffi.call("blissgpu_node_analyze_device", self._h, ptrs, offsets, lengths, ranks, len(offsets), features_version)
        _ffi.call("blissgpu_node_synchronize", self._h)
        self._n, self._d = len(offsets), 23 if features_version == 2 else 20

    def features(self, rank: int = 0) -> np.ndarray:
        """The gathered matrix as held by `rank`'s device."""
        out = np.empty((self._n, self._d), np.float32)
        ctx = _ffi.call("blissgpu_node_ctx", self._h, rank)
        src = _ffi.call("blissgpu_node_features", self._h, rank)
        _ffi.call("blissgpu_memcpy_d2h", ctx, out, src, out.nbytes)
        return out

    def pairwise(self, metric: str = "euclidean", M: Optional[np.ndarray] = None) -> np.ndarray:
        out = np.empty((self._n, self._n), np.float32)
        if M is not None:
            M = np.ascontiguousarray(M, np.float32)
        _ffi.call("blissgpu_node_pairwise", self._h, METRICS[metric], M, out)
        return out
