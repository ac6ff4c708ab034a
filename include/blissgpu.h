/*
 * blissgpu.h -- C ABI of the MI355X-native implementation of bliss-rs's per-song analysis hot path
 * and feature-vector distances.  This is the drop-in boundary: plain pointers and sizes, no C++/torch
 * types, no exceptions across the boundary.  Every entry point cites the reference interface it
 * replaces (file:line into bliss-rs / `bliss-audio` 0.13.0); INTEGRATION.md shows the Rust
 * `extern "C"` binding a bliss-rs maintainer would add.
 *
 * Input contract (same as Song::analyze, src/song/mod.rs:389-392): mono, 22 050 Hz, f32le PCM.
 * Output: one row of 23 (FeaturesVersion::Version2) or 20 (Version1) f32 per song, in the reference's
 * order [tempo, zcr, centroid mean/std, rolloff mean/std, flatness mean/std, loudness mean/std,
 * chroma x13|x10] (src/song/mod.rs:493-498, 102-156).
 *
 * Threading (src/song/decoder.rs:299-329: analyze is called from up to cores + 1 worker threads): EVERY entry point
 * is re-entrant and thread-safe.  Each context carries a mutex; calls on one context are serialised (the host-pointer
 * forms hold it for the whole call, the device forms while they enqueue), calls on different contexts run
 * concurrently.  The entry points without a context argument use process-wide DEFAULT contexts, one per visible HIP
 * device (created on first use; BLISSGPU_DEFAULT_DEVICES="0,2,3" restricts / orders them).
 * Concurrent single-song calls (blissgpu_analyze / blissgpu_analyze_interleaved) are COALESCED: the calls that
 * arrive while a device is busy are analysed together as its next batch, and a batch goes to whichever default device
 * is free -- so N worker threads each calling Song::analyze reach batch throughput on EVERY GPU of the node without
 * changing the caller.  The batch / distance / playlist forms without a context argument run on the first default
 * device (blissgpu_node_* spreads a batch over the node).
 * The library has NO CPU fallback: every compute entry point fails with BLISSGPU_ERR_NO_DEVICE when no
 * gfx950 device / HIP runtime is usable.
 */
#ifndef BLISSGPU_H
#define BLISSGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes (whole-call) ---- */
#define BLISSGPU_OK 0
#define BLISSGPU_ERR_NO_DEVICE 1      /* no usable HIP device: there is no CPU path */
#define BLISSGPU_ERR_INVALID 2        /* bad argument (NULL pointer, unknown features_version/metric, d > 64) */
#define BLISSGPU_ERR_HIP 3            /* a HIP runtime call failed; see blissgpu_last_error() */
#define BLISSGPU_ERR_OOM 4            /* workspace allocation failed */
#define BLISSGPU_ERR_NAN 5            /* a distance is NaN: the reference panics there (n32(), argmin().unwrap()) */
#define BLISSGPU_ERR_RCCL 6           /* librccl could not be loaded or a collective failed (blissgpu_node_* only) */
#define BLISSGPU_ERR_TIMEOUT 7        /* a single-song call was not picked up by any default context within its deadline
                                         (blissgpu_set_single_song_timeout_ms); blissgpu_last_error() names the seats */
#define BLISSGPU_ERR_INTERNAL 8       /* a bounded loop did not end where it must (blissgpu_mst: more than 64 rounds): a defect */

/* ---- per-song status, maps 1:1 onto BlissError (src/lib.rs:236-252) ---- */
#define BLISSGPU_SONG_OK 0
#define BLISSGPU_SONG_TOO_SHORT 1     /* AnalysisError("empty or too short song.") -- len < 8192 (src/song/mod.rs:417-430) */
#define BLISSGPU_SONG_DECODE_ERROR 2  /* DecodingError (blissgpu_analyze_batch_flac): not FLAC, unsupported depth, truncated, or a
                                       * frame error that the verified frame table cannot repair */

/* ---- FeaturesVersion (src/lib.rs:151-187) ---- */
#define BLISSGPU_FEATURES_V1 1u       /* 20 features */
#define BLISSGPU_FEATURES_V2 2u       /* 23 features (LATEST) */

/* ---- sample formats of the PCM feed (decoder output before the mono f32 conversion) ---- */
#define BLISSGPU_SAMPLE_F32 0
#define BLISSGPU_SAMPLE_S16 1         /* sample / 32768 */
#define BLISSGPU_SAMPLE_S32 2         /* (float)sample / 2^31: how FFmpeg delivers 24- and 32-bit streams */
#define BLISSGPU_SAMPLE_RATE 22050u   /* SAMPLE_RATE (src/lib.rs:140): the rate Song::analyze works at */

/* ---- distance metrics (src/playlist.rs:65-79, 129-142) ---- */
#define BLISSGPU_METRIC_EUCLIDEAN 0
#define BLISSGPU_METRIC_COSINE 1
#define BLISSGPU_METRIC_MAHALANOBIS 2

typedef struct blissgpu_ctx blissgpu_ctx;

/* Context = device selection + constant tables (windows, twiddles, the 100 chroma filter banks of
 * chroma_filter(), src/chroma.rs:197-267) + a grow-only HBM workspace + one HIP stream. */
int blissgpu_ctx_create(int device, blissgpu_ctx **ctx);
int blissgpu_ctx_destroy(blissgpu_ctx *ctx);
/* Launch on a caller-owned stream (a hipStream_t passed as void*, e.g. torch's current stream);
 * NULL restores the context's own stream. */
int blissgpu_ctx_set_stream(blissgpu_ctx *ctx, void *hip_stream);
void *blissgpu_ctx_get_stream(blissgpu_ctx *ctx);
/* Ordering against streams the caller owns, without host synchronisation (hipStream_t passed as void*, NULL = the
 * legacy default stream): wait_stream makes the context's stream wait for everything queued on producer_stream
 * (inputs written there), signal_stream makes consumer_stream wait for everything queued on the context's stream
 * (results read there). */
int blissgpu_ctx_wait_stream(blissgpu_ctx *ctx, void *producer_stream);
int blissgpu_ctx_signal_stream(blissgpu_ctx *ctx, void *consumer_stream);
/* Upper bound in bytes for the scratch workspace of ONE chunk (there are two chunk slots; default: a third of the
 * device memory free at creation, at most 64 GiB).  Larger batches are cut into length-bucketed chunks (longest songs
 * first) that stream through the two slots: chunk k + 1's FFT kernels overlap chunk k's per-song tails.  A chunk that
 * does not fit the memory actually free is halved and retried. */
int blissgpu_ctx_set_workspace_limit(blissgpu_ctx *ctx, uint64_t bytes);
uint64_t blissgpu_ctx_get_workspace_limit(blissgpu_ctx *ctx);
int blissgpu_ctx_synchronize(blissgpu_ctx *ctx);
/* Scheduling knobs of ONE context for the measurement tools and the tests (the library reads no environment variable for
 * them; defaults are what production uses).  Synchronises the context's stream. */
#define BLISSGPU_OPT_SERIAL 0           /* 1: every kernel on one stream, nothing overlaps (clean per-kernel timings) */
#define BLISSGPU_OPT_TAIL_MODE 1        /* beat tracker: -1 auto (default), 0 beside / 1 behind the FFT-8192 kernel.  Measurement forms of
                                           round 6 (same rows; none wins, profiles/r06_tail_mask_ab.txt): N >= 2 beside it with the
                                           per-song state machines on a stream confined to N compute units; -2 only the
                                           autocorrelations beside it; -3 the whole tracker beside the chroma contraction */
#define BLISSGPU_OPT_PIPELINE_CHUNKS 2  /* cut big batches into at least this many chunks (default 1) */
#define BLISSGPU_OPT_CAND_BUDGET 3      /* tuning-candidate pool: slots per chroma frame (default 48; 0 starves the pool) */
#define BLISSGPU_OPT_ROLLOFF_EXACT_ALL 4 /* 1: every frame's rolloff bin through the reference-order pass, not only the frames
                                           the FFT-512 kernel cannot prove (tests: both must give the same rows) */
#define BLISSGPU_OPT_TAIL_SPLIT 6       /* one-chunk batches: P >= 2 = the tuning estimate and the contraction run in P pieces of the
                                           songs (at most 8), the contraction of piece k beside the tuning estimate of piece
                                           k + 1; 0 / 1 = unsplit (default: see DESIGN.md section 3b) */
#define BLISSGPU_OPT_FLUX_ORDER 8       /* 1: SpecFlux (src/aubio.rs:455-467) adds its 257 terms one by one in bin order, as the
                                           reference does, instead of 16 per lane + a tree.  The default order deviates from the
                                           reference's by 1.7e-7 rms per value -- inside every tolerance, and the reason the tempo of
                                           white noise sits on the noisier side of the f32-FFT floor; with this option the device's
                                           tempo is as close to the f64-FFT oracle as a plain f32 FFT's.
                                           FFT-512 kernel +19 %, step +6 %.  Default 0 */
#define BLISSGPU_OPT_STFT_SHAPE 7       /* FFT-8192 kernel: 0 = four workgroups per CU, window in registers (default); 1 = the narrow
                                           form (five per CU: window loaded per frame, transposes in two halves); 2 / 3 = one of
                                           the two changes alone.  Same rows bit for bit; 1 is 8 % slower */
#define BLISSGPU_OPT_DEBUG_CHROMA 5     /* 1: the contraction also keeps chroma_stft's matrix and the assembly the interval
                                           means of the chunk for the CHROMA / INTERVAL taps below (96 B per frame); such a
                                           batch must fit ONE chunk (BLISSGPU_ERR_INVALID otherwise) */
/* The host PCM feed's pinned staging ring (pageable sources -- a Rust Vec<f32> out of PreAnalyzedSong,
 * src/song/decoder.rs:34-65, a decoder's frame buffers -- are copied into page-locked slabs by worker threads that run ahead
 * of the link; page-locked / registered sources are handed to the DMA engines as they are).  The ring restarts with the new
 * shape on the next host-pointer call. */
#define BLISSGPU_OPT_STAGE_LANES 9      /* worker threads = copy queues, 1..16; 0 = no ring: leave the staging of pageable memory
                                           to the HIP runtime (one bounce buffer on the calling thread).  Default 4 */
#define BLISSGPU_OPT_STAGE_SLAB_KIB 10  /* size of one page-locked slab, 64 .. 65536 KiB.  Default 4096 */
#define BLISSGPU_OPT_STAGE_SLABS 11     /* slabs each worker rotates through, 1..8.  Default 3 (4 x 3 x 4 MiB = 48 MiB per context) */
#define BLISSGPU_OPT_STAGE_NUMA 12      /* 1: the workers run, and allocate their slabs, on the CPUs next to the device (sysfs
                                           local_cpulist of its PCI function; a no-op on a one-node host); 0 (default): wherever
                                           the scheduler puts them -- near the caller's buffers, which measured better: a worker
                                           reading the caller's memory across the socket link is slower than the DMA engine
                                           reading the slab across it (profiles/r06_stage_numa_ab.txt) */
#define BLISSGPU_OPT_FOREST_SPLIT 13    /* forest scoring: workgroups that share one candidate block's trees; 0 (default) = enough to
                                           fill the device.  path_sum is an integer sum, so every setting gives the same result */
#define BLISSGPU_OPT_FOREST_WALK 14     /* forest scoring: 0 (default) = trees staged in LDS chunk by chunk, 1 = every tree walked
                                           from global memory (measurement form; same result) */
#define BLISSGPU_OPT_FOREST_GROUP_NODES 15 /* blissgpu_group_forest_knn: the node budget of one batch of groups (their forests travel
                                           to the device together); 0 (default) = derived from the workspace limit: what a 64 MiB
                                           image holds, or an eighth of the limit if that is less.  Every setting gives the same
                                           result */
int blissgpu_ctx_set_option(blissgpu_ctx *ctx, int option, int64_t value);
/* Bytes of pageable host PCM this context has staged through its pinned ring since it was created (0: every source so far
 * was page-locked, small, or the ring is switched off). */
uint64_t blissgpu_ctx_staged_bytes(blissgpu_ctx *ctx);

/* The default contexts: how many there are, the HIP ordinal of the k-th, and how many coalesced batches of single-song
 * calls it has served so far (load statistics). */
int blissgpu_default_device_count(void);
int blissgpu_default_device(int k);
uint64_t blissgpu_default_device_batches(int k);
/* The k-th default context itself -- the one the entry points WITHOUT a context argument run on (k = 0 serves the batch,
 * distance and playlist forms; every k a seat of the single-song front) -- created now if it does not exist yet.  Borrowed:
 * the library owns it (never pass it to blissgpu_ctx_destroy); use it for blissgpu_ctx_set_option (e.g. the staging ring's
 * shape), the workspace limit, the profile / debug taps. */
int blissgpu_default_ctx(int k, blissgpu_ctx **ctx);
/* How long a single-song call (blissgpu_analyze / _interleaved) may wait for a default context to pick it up before it
 * fails with BLISSGPU_ERR_TIMEOUT instead of blocking (default 600 000 ms; <= 0 restores the default; clamped to ten
 * years).  A default context
 * whose device cannot give a context is retired -- its traffic goes to the others -- and only when all are retired do the
 * calls fail, with the creation error. */
int blissgpu_set_single_song_timeout_ms(int64_t ms);
/* A default context that could not be created is not retried on every call: a failure that cannot change (no such device,
 * another architecture) is remembered for good, anything else (no memory for the tables while another process holds the
 * device, a HIP error) is tried again after a back-off of 100 ms .. 5 s, and a retired seat of the single-song front is offered
 * traffic again after 1 s .. 64 s.  blissgpu_default_reset() forgets every remembered failure and revives every seat now. */
int blissgpu_default_reset(void);

uint32_t blissgpu_feature_count(uint32_t features_version); /* FeaturesVersion::feature_count, src/lib.rs:181-186 */

/* Replaces Song::analyze / Song::analyze_with_options (src/song/mod.rs:403-508) for ONE song in host
 * memory.  Returns BLISSGPU_OK and writes feature_count floats, or BLISSGPU_OK with *status =
 * BLISSGPU_SONG_TOO_SHORT (out filled with NaN).  status may be NULL.  Uses the process-wide default
 * contexts; safe to call from any number of threads (concurrent calls are coalesced into device batches, one in flight
 * per device). */
int blissgpu_analyze(const float *pcm, uint64_t len, uint32_t features_version, float *out, int32_t *status);
/* Same for raw decoder output: `frames` frames of `channels` interleaved samples (BLISSGPU_SAMPLE_F32 / _S16 / _S32) at
 * 22 050 Hz.  s16 is widened with sample / 32768 and channels are downmixed ON THE DEVICE exactly like the reference's
 * decoders: stereo -> (L + R) * SQRT_2 / 2, more channels -> their mean (src/song/decoder/symphonia.rs:266-300; pinned
 * on data/s16_stereo_22_5kHz.flac by Adler-32 0x1d7b2d6d, src/song/decoder/ffmpeg.rs:448-452).  The caller delivers
 * 22 050 Hz here; blissgpu_analyze_decoded takes any rate. */
int blissgpu_analyze_interleaved(const void *pcm, int sample_format, uint32_t channels, uint64_t frames,
                                 uint32_t features_version, float *out, int32_t *status);

/* Bulk form: the compute half of Decoder::analyze_paths_with_options (src/song/decoder.rs:278-332) once the
 * decoders have produced PCM.  pcm holds the songs back to back (song i = pcm[offsets[i] ..
 * offsets[i] + lengths[i])); out is n_songs x feature_count row-major; status has one entry per
 * song -- one bad song never aborts the batch (src/song/decoder.rs:313-325).  Host pointers. */
int blissgpu_analyze_batch(const float *pcm, const uint64_t *offsets, const uint64_t *lengths, uint32_t n_songs,
                           uint32_t features_version, float *out, int32_t *status);

/* Same, for decoders that deliver signed 16-bit mono 22 050 Hz PCM (what FFmpeg hands to the reference's resampler
 * for the golden files, src/song/decoder/ffmpeg.rs:36-109): the samples cross PCIe as 2 bytes and are widened on the
 * device with sample / 32768, FFmpeg's s16 -> flt conversion (bit-identical to converting on the host first).
 * offsets / lengths are in samples.  Both host forms pipeline the transfer of one group of songs with the analysis
 * of the previous one. */
int blissgpu_analyze_batch_s16(const int16_t *pcm, const uint64_t *offsets, const uint64_t *lengths, uint32_t n_songs,
                               uint32_t features_version, float *out, int32_t *status);
/* Bulk form for interleaved multi-channel decoder output (see blissgpu_analyze_interleaved); offsets / lengths are in
 * FRAMES. */
int blissgpu_analyze_batch_interleaved(const void *pcm, int sample_format, uint32_t channels, const uint64_t *offsets,
                                       const uint64_t *lengths, uint32_t n_songs, uint32_t features_version, float *out,
                                       int32_t *status);
/* ---- decoder output at ANY sample rate (src/song/decoder/ffmpeg.rs:36-109) ----
 * The reference's FFmpegDecoder hands every decoded frame to libswresample with its default options (Kaiser-windowed sinc,
 * filter_size 32, cutoff 0.97, exact rational phases) and asks for mono f32 at 22 050 Hz.  These entry points take what the
 * DECODER delivers -- `frames` frames of `channels` interleaved samples at `sample_rate` Hz -- and do that conversion ON THE
 * DEVICE -- bit for bit at 44 100 Hz, the only rate the reference pins --: widening (s16 / s32), libswresample's resampler with the summation order of its AVX2 + FMA3 kernel,
 * the stream mirrored at both ends, stereo = each channel resampled, then l * sqrt(1/2) + r * sqrt(1/2) (more channels: the
 * sequential mean first, as src/song/decoder/symphonia.rs:291-297, then the resampler).  sample_rate 22 050 is the pass-through
 * of blissgpu_analyze_interleaved.  Pinned by the reference's own Adler-32 decoder tests: 0xa0f8b8af
 * (data/s32_mono_44_1_kHz.flac), 0xbbcba1cf (s32_stereo_44_1_kHz.flac) -- ffmpeg.rs:433-445 -- and 0xd594429c (no_channel.wav,
 * :471-476); with it the three CUE tracks of data/testcue.flac give the 3 x 23 features src/cue.rs:270-415 asserts.
 * Rates other than 44 100 Hz (147 / 441 / 1024 phases, up-sampling) run the same restatement of libswresample's published
 * algorithm; no reference test holds a number for them and no FFmpeg build was available to make one: they are held to the
 * oracle's independent restatement bit for bit and to a sinusoid-reconstruction property, i.e. NOT externally pinned. */
int blissgpu_analyze_decoded(const void *pcm, int sample_format, uint32_t channels, uint64_t frames, uint32_t sample_rate,
                             uint32_t features_version, float *out, int32_t *status);
/* Bulk form: every song with its own buffer, format, channel count and rate (a library is a mix of 44.1 and 48 kHz, mono
 * and stereo files).  The compute half of Decoder::analyze_paths_with_options (src/song/decoder.rs:278-332) for a host that
 * keeps its decoder and drops the resampler. */
typedef struct blissgpu_decoded_song {
    const void *pcm;        /* host memory: frames x channels interleaved samples */
    uint64_t frames;
    uint32_t sample_rate;   /* Hz, 1 .. 768 000 */
    uint16_t channels;      /* 1 .. 8 */
    uint16_t sample_format; /* BLISSGPU_SAMPLE_* */
} blissgpu_decoded_song;
int blissgpu_analyze_batch_decoded(const blissgpu_decoded_song *songs, uint32_t n_songs, uint32_t features_version, float *out,
                                   int32_t *status);
/* Number of 22 050 Hz samples `frames` input frames become (device-free; = frames at 22 050 Hz, 0 when the stream is shorter
 * than the resampler's start-up needs or the rate is out of range). */
uint64_t blissgpu_resampled_len(uint64_t frames, uint32_t sample_rate);
/* The resampler's filter bank for one input rate (device-free; test tap): *taps x *phase_count floats, phase-major; bank
 * may be NULL to query the sizes, at most max_elems floats are written. */
int blissgpu_resample_filter(uint32_t sample_rate, float *bank, uint64_t max_elems, uint32_t *taps, uint32_t *phase_count);

/* The conversions alone, device to device (asynchronous on the context's stream). */
int blissgpu_pcm_s16_to_f32_device(blissgpu_ctx *ctx, const int16_t *d_in, uint64_t n_samples, float *d_out);
int blissgpu_pcm_downmix_device(blissgpu_ctx *ctx, const void *d_in, int sample_format, uint32_t channels, uint64_t frames,
                                float *d_out);
/* decoder output at sample_rate -> mono 22 050 Hz f32; d_out holds blissgpu_resampled_len(frames, sample_rate) samples */
int blissgpu_pcm_decode_device(blissgpu_ctx *ctx, const void *d_in, int sample_format, uint32_t channels, uint64_t frames,
                               uint32_t sample_rate, float *d_out);

/* ---- FLAC decoded ON THE DEVICE: compressed files in, PCM / feature rows out ----
 * The host only finds the frames (it never decodes a residual); flac_decode_kernel decodes one frame per lane into what the
 * reference's FFmpeg decoder hands on: up to 16 bits per sample interleaved int16, sample << (16 - bps); above, interleaved
 * int32, sample << (32 - bps).  Bit for bit -- FLAC is lossless and the stream's MD5 says so.  Handled: CONSTANT / VERBATIM /
 * FIXED 0-4 / LPC 1-32 subframes, wasted bits, both Rice methods, escape partitions, every channel assignment, 1-8 channels,
 * 4-24 bits per sample.  32 bits per sample and Ogg-FLAC are reported as decode errors.
 * The default calls check the structure only (every frame stops 2 bytes before the next).  The frame CRC-16 and the stream
 * MD5 are checked on the device when asked for: blissgpu_flac_verify_batch, blissgpu_analyze_batch_flac_verified (below).
 *
 * info: BLISSGPU_FLAC_INFO_WORDS 64-bit words -- [0] sample rate, [1] channels, [2] bits per sample, [3] total inter-channel
 * samples (0 = unknown in STREAMINFO; blissgpu_flac_index and blissgpu_flac_decode replace it by the count the frame table
 * holds), [4] / [5] min / max block size, [6] min frame size, [7] byte offset of the first frame, [8..9] the MD5 (16 bytes
 * in file order), [10] the stream position the first frame's header codes (set by blissgpu_flac_index / _decode: 0 unless
 * the file was cut out of a longer stream), [11] reserved (0).
 * An ID3v2 tag in front of "fLaC" is skipped.  Device-free. */
#define BLISSGPU_FLAC_INFO_WORDS 12u
int blissgpu_flac_info(const void *file, uint64_t nbytes, uint64_t *info);
/* The frame table: rows of 4 words -- byte offset, byte length (header to CRC-16), first sample, block size.  At most
 * max_frames rows are written (frames may be NULL), *n_frames receives the count.  verified = 0: CRC-8 and the expected frame
 * number only -- fast, and a header-shaped run of bytes inside a frame can fool it (the device notices: that frame does not
 * stop 2 bytes before the next row); verified = 1: CRC-16 over every candidate frame, exact for every frame but the last (it
 * runs to the end of the data; bytes behind the audio are left to the decoder's stop position).  info may be NULL.  Device-free.
 * BLISSGPU_ERR_INVALID for a stream without frames or with fewer samples than STREAMINFO promises (the table is filled). */
int blissgpu_flac_index(const void *file, uint64_t nbytes, int verified, uint64_t *info, uint64_t *frames, uint64_t max_frames,
                        uint64_t *n_frames);
/* Device to device, asynchronous on the context's stream: the frames of ONE file.  d_bytes = the file on the device, 8-byte
 * aligned, with 16 readable bytes behind it; frames / info as blissgpu_flac_index returned them (host memory; info[3] is the
 * size of d_pcm in inter-channel samples: no store goes beyond it).  d_frame_status[i] = 0 or the frame's error
 * (flac_frame.hpp: 1 reserved subframe type, 2 reserved channel assignment, 3 header mismatch, 4 ran past the frame,
 * 5 negative shift, 6 unsupported depth, 7 malformed subframe); d_frame_end[i] = the byte position frame i stopped at --
 * frames[i].offset + frames[i].length - 2 for a frame that is what the table took it for (the last frame may stop earlier). */
int blissgpu_flac_decode_device(blissgpu_ctx *ctx, const void *d_bytes, uint64_t nbytes, const uint64_t *frames, uint64_t n_frames,
                                const uint64_t *info, void *d_pcm, int32_t *d_frame_status, uint64_t *d_frame_end);
/* One file in host memory -> PCM in host memory (default context): fast table, end-position check, verified table and a second
 * launch on a mismatch.  pcm = NULL: info and *status only (nothing runs on the device); otherwise max_bytes >= info[3] x
 * channels x (2 or 4).  *status = BLISSGPU_SONG_OK or BLISSGPU_SONG_DECODE_ERROR (the call itself still returns BLISSGPU_OK). */
int blissgpu_flac_decode(const void *file, uint64_t nbytes, void *pcm, uint64_t max_bytes, uint64_t *info, int32_t *status);
/* Several files through ONE upload and ONE decode launch -- the decode half of blissgpu_analyze_batch_flac, its PCM handed
 * back: pcm[i] (host, max_bytes[i] bytes) receives song i, info + i * BLISSGPU_FLAC_INFO_WORDS its info, status[i] its status.
 * A song whose PCM does not fit max_bytes[i] gets BLISSGPU_SONG_DECODE_ERROR; BLISSGPU_ERR_INVALID when the files do not fit
 * the workspace limit together (this form does not split). */
int blissgpu_flac_decode_batch(const void *const *files, const uint64_t *nbytes, uint32_t n_songs, void *const *pcm,
                               const uint64_t *max_bytes, uint64_t *info, int32_t *status);
/* Bulk form: the bytes of n_songs .flac files -> n_songs feature rows.  Frame tables on the host (at most as many threads as
 * the staging ring has workers), one upload of the compressed bytes, one decode launch for the batch, the end-position
 * check, the device conversion to mono 22 050 Hz per song, the device-resident batch analysis.  The decoded PCM of a
 * sub-batch (with its compressed bytes and mono stream) fits the context's workspace limit; the call is split when it does
 * not, and a song that exceeds the limit by itself is a decode error.  A song's last frame may be followed by other bytes
 * (an ID3v1 tag, padding).  status[i] = BLISSGPU_SONG_OK,
 * _TOO_SHORT or _DECODE_ERROR (row = NaN); one bad file never affects another song of the call.  status may be NULL. */
int blissgpu_analyze_batch_flac(const void *const *files, const uint64_t *nbytes, uint32_t n_songs, uint32_t features_version,
                                float *out, int32_t *status);
/* Songs of this context whose fast frame table the device refused, or could not be closed on the host: they went through
 * verified mode (statistics). */
uint64_t blissgpu_ctx_flac_slow_songs(blissgpu_ctx *ctx);

/* ---- FLAC verified ON THE DEVICE (opt-in): every frame's CRC-16, the stream's MD5, a verdict per song ----
 * checks: what to verify beyond the structure.  CRC16: flac_crc_kernel, one wavefront per frame, over the frame from its first
 * header byte to the decoder's own stop position, against the two bytes there.  MD5: flac_md5_kernel, one lane per song, the
 * digest of the decoded samples (interleaved, little-endian, ceil(bps / 8) bytes each) against STREAMINFO's -- a serial chain
 * per song and slow for long songs (DESIGN.md section 3.19 has the figures): a "check my library" mode. */
#define BLISSGPU_FLAC_CHECK_CRC16 1u
#define BLISSGPU_FLAC_CHECK_MD5   2u
/* verdict flags; a song failed when (flags & 7) != 0 */
#define BLISSGPU_FLAC_BAD_STREAM    1u  /* what is BLISSGPU_SONG_DECODE_ERROR in the unverified calls */
#define BLISSGPU_FLAC_BAD_CRC16     2u
#define BLISSGPU_FLAC_BAD_MD5       4u
#define BLISSGPU_FLAC_MD5_UNCHECKED 8u  /* informational: the MD5 check was not asked for, STREAMINFO's MD5 is all zero, the
                                         * stream was cut out of a longer one (info[10] != 0), the frame table's sample count
                                         * differs from a nonzero STREAMINFO total, or an earlier check of the song failed */
/* Index, upload, decode, the end-position check and the requested checks of n_songs files, no analysis ("flac -t" for a
 * library, in batches); split by the workspace limit like blissgpu_analyze_batch_flac; one bad file never affects another
 * song.  flags[i]: the verdict; first_bad_frame[i] (may be NULL): the first frame of song i whose CRC-16 failed, 0xFFFFFFFF
 * when none; md5 (may be NULL): 16 bytes per song, the computed digest, zeros when it was not computed. */
int blissgpu_flac_verify_batch(const void *const *files, const uint64_t *nbytes, uint32_t n_songs, uint32_t checks,
                               uint32_t *flags, uint32_t *first_bad_frame, void *md5);
/* blissgpu_analyze_batch_flac plus the checks: a song that fails one gets BLISSGPU_SONG_DECODE_ERROR and a NaN row, every
 * other row is bit-identical to the unverified call's.  checks = 0 is the unverified call (flags / first_bad_frame are not
 * written and may be NULL). */
int blissgpu_analyze_batch_flac_verified(const void *const *files, const uint64_t *nbytes, uint32_t n_songs,
                                         uint32_t features_version, uint32_t checks, float *out, int32_t *status,
                                         uint32_t *flags, uint32_t *first_bad_frame);
/* Device to device, asynchronous on the context's stream, ONE file, beside blissgpu_flac_decode_device: d_bytes / frames as
 * there, d_frame_status / d_frame_end as it wrote them.  d_frame_crc_ok[i] = 1 (the CRC-16 over [offset, end) equals the two
 * bytes at end), 0 (it does not, or end does not lie inside the row), -1 (the frame's status is not 0: not checked). */
int blissgpu_flac_crc16_device(blissgpu_ctx *ctx, const void *d_bytes, uint64_t nbytes, const uint64_t *frames, uint64_t n_frames,
                               const int32_t *d_frame_status, const uint64_t *d_frame_end, int32_t *d_frame_crc_ok);
/* d_md5 (16 bytes on the device) = the MD5 of the FLAC message of d_pcm: info[3] inter-channel samples of info[1] channels,
 * int16 (info[2] <= 16 bits per sample) or int32, as blissgpu_flac_decode_device wrote them; d_pcm and d_md5 are 4-byte aligned,
 * info[3] is below 2^36 (what STREAMINFO can code). */
int blissgpu_flac_md5_device(blissgpu_ctx *ctx, const void *d_pcm, const uint64_t *info, void *d_md5);

/* Device-resident form: d_pcm / d_out / d_status are HIP device pointers (d_status may be NULL),
 * offsets / lengths stay on the host (they size the launch).  Asynchronous on the context's
 * stream (d_status is written by the device too: no host synchronisation inside); call blissgpu_ctx_synchronize (or
 * synchronise the stream) before reading d_out.  This is the streaming scheduler of configs like "50 000 songs of
 * 30 s - 10 min": songs are bucketed by length and run as chunks through two workspace slots. */
int blissgpu_analyze_batch_device(blissgpu_ctx *ctx, const float *d_pcm, const uint64_t *offsets,
                                  const uint64_t *lengths, uint32_t n_songs, uint32_t features_version,
                                  float *d_out, int32_t *d_status);

/* Song::distance / Analysis::distance (src/song/mod.rs:364-370, 519-521) and the free functions
 * euclidean_distance / cosine_distance / mahalanobis_distance (src/playlist.rs:65-79, 140-142) for one
 * pair (host pointers; M is d x d row-major, required for MAHALANOBIS, ignored otherwise). */
int blissgpu_distance(const float *a, const float *b, uint32_t d, int metric, const float *M, float *out);

/* All-pairs form: out[i * m + j] = metric(A[i], B[j]).  A is n x d, B is m x d, row-major f32.  This
 * is the batched equivalent of evaluating a DistanceMetric over every candidate
 * (src/playlist.rs:24-59, 256-270).  Host pointers. */
int blissgpu_pairwise(const float *A, uint64_t n, const float *B, uint64_t m, uint32_t d, int metric, const float *M,
                      float *out);
/* Device-resident form; ld_out is the row pitch of d_out in elements (>= m).  Asynchronous. */
int blissgpu_pairwise_device(blissgpu_ctx *ctx, const float *d_A, uint64_t n, const float *d_B, uint64_t m,
                             uint32_t d, int metric, const float *d_M, float *d_out, uint64_t ld_out);

/* ---- playlist ordering (src/playlist.rs:24-59, 256-326) ----
 * A "song" is a row of a feature matrix; results are index permutations into the candidate matrix.
 * The metric built from a set of vectors is FunctionDistanceMetric (src/playlist.rs:36-59): the sequential
 * f32 sum over the set of func(vector_of_the_set, candidate), func = one of the three metrics above.
 * A NaN distance returns BLISSGPU_ERR_NAN (the reference panics: n32() / argmin().unwrap()). */

/* n_seeds may be 0: the sum over an empty set is 0.0 for every candidate, so closest_to_songs returns the candidates
 * in their own order and song_to_song starts from candidate 0. */

/* FunctionDistanceMetric::distance for every candidate: out[j] = sum_i metric(seeds[i], cand[j]). */
int blissgpu_set_distance(const float *seeds, uint32_t n_seeds, const float *cand, uint64_t n, uint32_t d, int metric,
                          const float *M, float *out);
/* closest_to_songs (src/playlist.rs:256-270): order[k] = index of the k-th closest candidate to the seed set
 * (stable: equal distances keep the candidates' order, like sort_by_cached_key); dist (may be NULL) receives
 * the distances in candidate order. */
int blissgpu_closest_to_songs(const float *seeds, uint32_t n_seeds, const float *cand, uint64_t n, uint32_t d,
                              int metric, const float *M, uint32_t *order, float *dist);
/* song_to_song (src/playlist.rs:272-326): greedy nearest-neighbour chain.  order[0] = the candidate closest to the
 * seed set, order[k] = the remaining candidate closest to candidate order[k-1] (first minimum in pool order). */
int blissgpu_song_to_song(const float *seeds, uint32_t n_seeds, const float *cand, uint64_t n, uint32_t d, int metric,
                          const float *M, uint32_t *order);
/* Device-resident forms (all pointers are HIP device pointers; asynchronous except for the NaN check, which
 * synchronises the context's stream before returning). */
int blissgpu_set_distance_device(blissgpu_ctx *ctx, const float *d_seeds, uint32_t n_seeds, const float *d_cand,
                                 uint64_t n, uint32_t d, int metric, const float *d_M, float *d_out);
int blissgpu_closest_to_songs_device(blissgpu_ctx *ctx, const float *d_seeds, uint32_t n_seeds, const float *d_cand,
                                     uint64_t n, uint32_t d, int metric, const float *d_M, uint32_t *d_order,
                                     float *d_dist);
int blissgpu_song_to_song_device(blissgpu_ctx *ctx, const float *d_seeds, uint32_t n_seeds, const float *d_cand,
                                 uint64_t n, uint32_t d, int metric, const float *d_M, uint32_t *d_order);

/* dedup_playlist_custom_distance (src/playlist.rs:343-402) over the playlist seq[0..len) of rows of the n x d matrix x:
 * a song absorbs the songs that follow it while n32(metric(song, next)) < threshold (the reference's default is 0.05f) or
 * both have the same non-empty title and artist; the walk resumes at the first song not absorbed.  seq may be NULL
 * (identity, len == n); every entry must be < n.  meta (may be NULL: no title / artist rule) holds one key per ROW of x:
 * 0 = title or artist is None, equal non-zero keys = equal (title, artist).  kept[0..*n_kept) (room for len entries)
 * receives positions into seq, in order; len == 0 keeps nothing, len == 1 keeps [0].  A NaN distance the reference
 * evaluates (one on the chain of kept songs) returns BLISSGPU_ERR_NAN; the distances it never evaluates do not matter.
 * Two launches whatever the playlist (dedup_next_kernel, dedup_walk_kernel: DESIGN.md 3.9), at most len * 65 distances. */
int blissgpu_dedup_playlist(const float *x, uint64_t n, uint32_t d, const uint32_t *seq, uint64_t len,
                            const uint32_t *meta, int metric, const float *M, float threshold, uint32_t *kept,
                            uint64_t *n_kept);
/* Device-resident form (device pointers, d_n_kept included); asynchronous except for the NaN / seq check, which
 * synchronises the context's stream before returning. */
int blissgpu_dedup_playlist_device(blissgpu_ctx *ctx, const float *d_x, uint64_t n, uint32_t d, const uint32_t *d_seq,
                                   uint64_t len, const uint32_t *d_meta, int metric, const float *d_M, float threshold,
                                   uint32_t *d_kept, uint64_t *d_n_kept);

/* ---- k nearest candidates of every query (src/playlist.rs:256-270, src/library.rs:762-850) ----
 * For query i: the first k entries of closest_to_songs(&[queries[i]], candidates without skip[i], metric), i.e. of the STABLE
 * ascending sort of metric(queries[i], cand[j]) over j != skip[i] -- what Library::playlist_from(&[song]).take(k) asks, for
 * q songs in one call.  idx and dist are q x k row-major; dist may be NULL.  Equal distances come in candidate order (-0.0
 * and +0.0 are equal); every distance is bit for bit what blissgpu_pairwise_device writes for the same pair.
 * skip (may be NULL) holds one candidate index per query that is left out of that query's result and not evaluated (how a song
 * is kept out of its own list when the queries are rows of the candidate matrix); 0xFFFFFFFF skips nothing, any other value
 * >= n is BLISSGPU_ERR_INVALID.  Rows with fewer than k eligible candidates end in idx 0xFFFFFFFF / dist +inf.  A NaN among the
 * evaluated distances returns BLISSGPU_ERR_NAN (the reference's n32() panic); the outputs are then unspecified.
 * 1 <= k <= BLISSGPU_KNN_MAX_K, 1 <= d <= 64, n < 2^32 - 1; q == 0 or n == 0 is BLISSGPU_OK.  Arguments are checked before the
 * device is touched.  No q x n matrix is ever stored: the workspace is O(q k), two launches whatever q and n.
 * queries == cand (the same pointer, q <= n) uploads the matrix once. */
#define BLISSGPU_KNN_MAX_K 1024u
int blissgpu_knn(const float *queries, uint64_t q, const float *cand, uint64_t n, uint32_t d, int metric, const float *M,
                 const uint32_t *skip, uint32_t k, uint32_t *idx, float *dist);
/* Device-resident form (device pointers, d_skip included; d_dist may be NULL); asynchronous except for the NaN / skip check,
 * which synchronises the context's stream before returning. */
int blissgpu_knn_device(blissgpu_ctx *ctx, const float *d_queries, uint64_t q, const float *d_cand, uint64_t n,
                        uint32_t d, int metric, const float *d_M, const uint32_t *d_skip, uint32_t k,
                        uint32_t *d_idx, float *d_dist);

/* ---- Locally scaled k nearest candidates, and how often every song is listed (the reference's TODO.md complains
 * of playlists that "drift" and asks for an objective measure of a similarity) ----
 * A raw nearest-neighbour search in 20 or 23 dimensions has hubs: a few songs are in everyone's list, many in nobody's.  Local
 * scaling (NICDM: Schnitzer, Flexer, Schedl, Widmer, JMLR 2012) ranks by
 *   sdist(i, j) = dist(i, j) / sqrtf(qscale[i] * cscale[j])
 * with dist(i, j) bit for bit what blissgpu_pairwise_device writes for the pair (what blissgpu_knn ranks by), and all three
 * operations in IEEE binary32: the product rounded once, the correctly rounded square root, true division.  A scale is a song's
 * own idea of "near", e.g. the mean distance to its 10 nearest songs from blissgpu_knn.
 * Every scale lies in [2^-60, 2^60], so the product is a normal f32 and its root is not zero; any other value among qscale [q]
 * or cscale [n] -- zero, negative, NaN, infinite -- is BLISSGPU_ERR_INVALID (checked on the device; the outputs are then
 * unspecified).  The selection is exactly blissgpu_knn's with sdist in dist's place: per query the k smallest keys
 * (f32_key(sdist) << 32) | candidate in ascending order, so equal SCALED distances come in candidate order; skip as for
 * blissgpu_knn (0xFFFFFFFF skips nothing, any other value >= n is BLISSGPU_ERR_INVALID); rows with fewer than k eligible
 * candidates end in idx 0xFFFFFFFF / dist +inf; a NaN among the evaluated base distances is BLISSGPU_ERR_NAN.  dist, when not
 * NULL, receives the scaled distances.  Metrics and feature counts as for blissgpu_knn (a diagonal M is detected).
 * 1 <= k <= BLISSGPU_KNN_MAX_K, 1 <= d <= 64, n < 2^32 - 1; q == 0 or n == 0 is BLISSGPU_OK.  Arguments (a NULL qscale or cscale
 * included) are checked before the device is touched.  No q x n matrix is ever stored: the workspace is O(q k) besides the
 * O(n) scales, two launches whatever q and n.  queries == cand with qscale == cscale (the same pointers, q <= n) uploads each
 * once. */
int blissgpu_scaled_knn(const float *queries, uint64_t q, const float *qscale, const float *cand, uint64_t n,
                        const float *cscale, uint32_t d, int metric, const float *M, const uint32_t *skip, uint32_t k,
                        uint32_t *idx, float *dist);
/* Device-resident form (device pointers, d_skip included; d_dist may be NULL); asynchronous except for the NaN / skip / scale
 * check, which synchronises the context's stream before returning. */
int blissgpu_scaled_knn_device(blissgpu_ctx *ctx, const float *d_queries, uint64_t q, const float *d_qscale,
                               const float *d_cand, uint64_t n, const float *d_cscale, uint32_t d, int metric,
                               const float *d_M, const uint32_t *d_skip, uint32_t k, uint32_t *d_idx, float *d_dist);
/* k-occurrence: count [n] receives, for every song j, the number of entries of idx [q][k] equal to j -- in how many lists the
 * song is.  Padding entries (0xFFFFFFFF) are ignored; any other entry >= n is BLISSGPU_ERR_INVALID.  k >= 1, n < 2^32 - 1,
 * q k <= 2^40; q == 0 writes zeros, n == 0 writes nothing.  One launch (integer atomics: the result does not depend on their
 * order).  The skewness of these counts is the hubness of the ranking that produced idx.  BLISSGPU_OCCURRENCE_LDS=1 in the
 * environment, read at every call, counts through a per-workgroup LDS histogram instead (the bench tool's A/B; the same counts). */
int blissgpu_knn_occurrence(const uint32_t *idx, uint64_t q, uint32_t k, uint64_t n, uint32_t *count);
/* Device-resident form (device pointers); synchronises the context's stream before returning. */
int blissgpu_knn_occurrence_device(blissgpu_ctx *ctx, const uint32_t *d_idx, uint64_t q, uint32_t k, uint64_t n,
                                   uint32_t *d_count);

/* ---- k-means clustering of a library (the reference's TODO.md asks for genre clustering, it has no code) ----
 * Lloyd's algorithm over the rows x [n][d] from the initial centres init [k][d], every step defined to the bit.  With
 * dist(i, c) = bit for bit what blissgpu_pairwise_device(x, C_t) writes at [i][c], and L_-1[i] = 0xFFFFFFFF, iteration
 * t = 0, 1, ... is
 *   L_t[i] = the c with the smallest (dist(i, c), c): equal ROUNDED distances (-0.0 and +0.0 are equal) go to the lower c;
 *   D_t[i] = dist(i, L_t[i]);
 *   no label moved (L_t == L_t-1): stop, converged = 1;   t == max_iter: stop, converged = 0;
 *   C_t+1[c] = (0.0f + x[i_0] + x[i_1] + ...) / (float)count_c over the members of c in ASCENDING i, every operation in f32, the
 *              sum never split or restarted (ndarray's mean_axis; blissgpu_album_knn's centroid rule);
 *   C_t+1[c] = C_t[c], the same bits, when c has no member: an empty cluster keeps its centre.
 * Outputs: labels [n] = L_t, dist [n] = D_t (may be NULL), centroids [k][d] = C_t -- the labels are always the nearest-centre
 * labels of the centres returned --, sizes [k] (may be NULL) = members per cluster, *n_iter = t = the number of updates made,
 * *converged.  max_iter = 0 is a pure nearest-centre assignment to init.
 * metric: BLISSGPU_METRIC_EUCLIDEAN, or BLISSGPU_METRIC_MAHALANOBIS with the caller's M (a diagonal M is detected as everywhere
 * else); BLISSGPU_METRIC_COSINE is BLISSGPU_ERR_INVALID (a mean does not minimise it).  A NaN among the evaluated distances
 * returns BLISSGPU_ERR_NAN; the outputs are then unspecified.
 * 1 <= d <= 64, 1 <= k <= BLISSGPU_KMEANS_MAX_K, n < 2^32 - 1; k > n is allowed (the surplus centres stay empty); n == 0 is
 * BLISSGPU_OK with n_iter = 0, converged = 1, centroids = init.  Arguments are checked before the device is touched.
 * Labels, row lists and centres stay on the device between iterations; the host reads one pair of words per iteration (labels
 * that moved, NaN).  Workspace, grow-only in the context: O(n + k d + chunks x k) with chunks x k <= max(k, 2^21) words. */
#define BLISSGPU_KMEANS_MAX_K 65535u
int blissgpu_kmeans(const float *x, uint64_t n, uint32_t d, const float *init, uint32_t k, int metric, const float *M,
                    uint32_t max_iter, uint32_t *labels, float *dist, float *centroids, uint32_t *sizes,
                    uint32_t *n_iter, int32_t *converged);
/* Device-resident form (device pointers, d_dist and d_sizes may be NULL; n_iter and converged are HOST pointers).  It
 * synchronises the context's stream once per iteration and before returning.  d_centroids may be d_init. */
int blissgpu_kmeans_device(blissgpu_ctx *ctx, const float *d_x, uint64_t n, uint32_t d, const float *d_init, uint32_t k,
                           int metric, const float *d_M, uint32_t max_iter, uint32_t *d_labels, float *d_dist,
                           float *d_centroids, uint32_t *d_sizes, uint32_t *n_iter, int32_t *converged);

/* ---- Silhouette of a labelling (the reference's TODO.md asks for "a proper 'objective' way to evaluate" and for
 * the genre clustering / evaluation code, it has no code) ----
 * How well a labelling of the rows x [n][d] separates them under a metric: for every scored song the mean distance to its own
 * cluster against the mean distance to the nearest other cluster, every step defined to the bit.
 * Inputs: x [n][d] f32; labels [n] u32, every one < k; metric: BLISSGPU_METRIC_EUCLIDEAN, or BLISSGPU_METRIC_MAHALANOBIS with the
 * caller's M (a diagonal M is detected as everywhere else); rows [q] u32 (may be NULL) = the songs to score, in any order, repeats
 * allowed: output position p belongs to song rows[p].  rows == NULL scores every song: q is then taken as n, position p = song p.
 * With dist(i, j) = bit for bit what blissgpu_pairwise_device(x, x) writes at [i][j], and size_c = the member count of cluster c:
 *   S(i, c) = 0.0 + (double)dist(i, j_0) + (double)dist(i, j_1) + ... over the members of c in ASCENDING j: one sequential f64
 *             sum, never split or restarted.  The song itself is a member of its own cluster; its term is +0.0;
 *   own = labels[i];   a = S(i, own) / (double)(size_own - 1), and a = 0.0 when size_own == 1;
 *   b = the smallest S(i, c) / (double)size_c over c != own with size_c > 0, neighbour = that c: equal quotients go to the lower c;
 *   s, every operation in f64 rounded on its own, then rounded once to f32:
 *       s = 0 when size_own == 1;   s = 0 when a == b;   s = 1 - a / b when a < b;   s = b / a - 1 when a > b.
 * This form equals (b - a) / max(a, b) and stays defined when one side is 0 or infinite.
 * Outputs, per scored song: s [q] f32; a [q] and b [q] f64 (may be NULL); neighbour [q] u32 (may be NULL); and sizes [k] u32 (may be
 * NULL) = the members per cluster.
 * A NaN among the evaluated distances returns BLISSGPU_ERR_NAN (the k-means rule); the outputs are then unspecified.
 * BLISSGPU_ERR_INVALID: BLISSGPU_METRIC_COSINE (the message names it); a label >= k; fewer than two non-empty clusters; a rows
 * entry >= n; d outside 1 .. 64; k outside 1 .. BLISSGPU_KMEANS_MAX_K; n or q >= 2^32 - 1; NULL x, labels or s.  n == 0 or q == 0 is
 * BLISSGPU_OK: nothing is scored (n == 0 writes zeros to sizes; q == 0 writes nothing).
 * The host form checks all of these before the device is touched; its labels and rows are host memory.
 * col_groups: 0 lets the plan choose into how many column groups the clusters are dealt, anything else forces
 * that many (at most k are used).  No bit of any output depends on it: the argument exists for the tests and the bench tool.
 * No n x n matrix is ever stored.  Workspace, grow-only in the context: the k-means sort's O(n + chunks x k) plus 20 bytes per
 * (scored song, column group). */
int blissgpu_silhouette(const float *x, uint64_t n, uint32_t d, const uint32_t *labels, uint32_t k, int metric, const float *M,
                        const uint32_t *rows, uint64_t q, uint32_t col_groups, float *s, double *a, double *b,
                        uint32_t *neighbour, uint32_t *sizes);
/* Device-resident form (device pointers throughout).  It checks the scalar arguments before it looks at its context, and
 * reports the data-dependent errors (a label >= k, a rows entry >= n, fewer than two non-empty clusters, NaN) after the sort, at
 * its one synchronisation of the context's stream before returning. */
int blissgpu_silhouette_device(blissgpu_ctx *ctx, const float *d_x, uint64_t n, uint32_t d, const uint32_t *d_labels, uint32_t k,
                               int metric, const float *d_M, const uint32_t *d_rows, uint64_t q, uint32_t col_groups, float *d_s,
                               double *d_a, double *d_b, uint32_t *d_neighbour, uint32_t *d_sizes);

/* ---- Group neighbours: which groups of a labelling are like each other (the reference's TODO.md asks: "Have a
 * 'similar artists to the current one' playlist option", it has no code) ----
 * The average nearest-member (Chamfer) distance between the groups of a labelling (artists, albums, genres, clusters) of the rows
 * x [n][d], and per queried group its t nearest groups.  A set-to-set distance, not a distance of means: a group with two styles
 * is near the groups that cover both.  Every step is defined to the bit.
 * Inputs: x [n][d] f32; labels [n] u32, every one < k; k groups; metric: BLISSGPU_METRIC_EUCLIDEAN, or BLISSGPU_METRIC_MAHALANOBIS
 * with the caller's M (a diagonal M is detected as everywhere else); queries [q] u32 (NULL = all k groups in order: q is then taken
 * as k) = the groups to answer for, any order, repeats allowed; t = neighbours per query; mode BLISSGPU_GROUPS_*.
 * With dist(i, j) = bit for bit what blissgpu_pairwise_device(x, x) writes at [i][j], size_c = the member count of group c, and
 * "members in order" = ascending row index:
 *   m(i, c)  = the minimum of dist(i, j) over the members j of c (f32); defined for c != labels[i] with size_c > 0;
 *   T(a, c)  = the f64 sum of (double)m(i, c) over the members i of a in order, u = 0, 1, ..., added in this fixed order: the
 *              terms are cut into blocks of BLISSGPU_MOMENTS_BLOCK = 256, the last block padded with +0.0; within a block, for
 *              h = 128, 64, ..., 1:  v[u] = v[u] + v[u + h] for every u < h, the block's sum is v[0]; the block sums are added
 *              sequentially in ascending block order, starting from 0.0.  Every add is rounded on its own;
 *   D(a->c)  = T(a, c) / (double)size_a;
 *   A(a, c)  = (D(a->c) + D(c->a)) * 0.5 under BLISSGPU_GROUPS_SYMMETRIC;  D(a->c), "how well c covers a", under
 *              BLISSGPU_GROUPS_DIRECTED.
 * Outputs: row g of idx [q][t] u32 and dist [q][t] f64, with a = queries[g]: the t groups c != a with size_c > 0 of smallest
 * A(a, c), ascending; equal values go to the lower c; with fewer than t such groups, or an empty a, the rest of the row is
 * 0xFFFFFFFF / +inf (the k-nearest padding).  sizes [k] u32 (may be NULL).  matrix [k][k] f64 (may be NULL) = A, with 0.0 on
 * the diagonal (of an empty group too) and +inf elsewhere wherever either group is empty.
 * A NaN among the m(i, c) returns BLISSGPU_ERR_NAN; the outputs are then unspecified.  BLISSGPU_ERR_INVALID:
 * BLISSGPU_METRIC_COSINE (the message names it); a label >= k; a query >= k; d outside 1 .. 64; k outside
 * 1 .. BLISSGPU_KMEANS_MAX_K; t outside 1 .. BLISSGPU_KNN_MAX_K; n or q >= 2^32 - 1; NULL x or labels with n > 0, NULL idx or dist with q > 0; an unknown mode.
 * n == 0 is BLISSGPU_OK: rows of padding, zero sizes.  q == 0 is BLISSGPU_OK: no row is written (sizes and matrix still are).
 * Fewer than two non-empty groups is not an error: rows of padding.
 * The host form checks all of these before the device is touched; its labels and queries are host memory.
 * slab_groups: the target groups c are taken in passes of `slab` groups; 0 lets the plan choose, anything else forces that many
 * (at most k).  No bit of any output depends on it: the argument exists for the tests and the bench tool.
 * No n x n matrix is ever stored.  Workspace, grow-only in the context: the k-means sort's O(n + chunks x k), n x slab x 4 bytes of
 * minima, k x k x 8 bytes of D and O(k) per workgroup of the selection.  When that exceeds the context's workspace limit
 * (blissgpu_ctx_get_workspace_limit) with the plan's smallest slab, or with a forced one, the call returns BLISSGPU_ERR_OOM
 * before anything is launched. */
#define BLISSGPU_GROUPS_SYMMETRIC 0
#define BLISSGPU_GROUPS_DIRECTED 1
int blissgpu_group_neighbours(const float *x, uint64_t n, uint32_t d, const uint32_t *labels, uint32_t k, int metric, const float *M,
                              const uint32_t *queries, uint64_t q, uint32_t t, int mode, uint32_t slab_groups, uint32_t *idx,
                              double *dist, uint32_t *sizes, double *matrix);
/* Device-resident form (device pointers throughout).  It checks the scalar arguments before it looks at its context, and
 * reports the data-dependent errors (a label >= k, a query >= k, NaN) after the sort, at its one synchronisation of the
 * context's stream before returning. */
int blissgpu_group_neighbours_device(blissgpu_ctx *ctx, const float *d_x, uint64_t n, uint32_t d, const uint32_t *d_labels,
                                     uint32_t k, int metric, const float *d_M, const uint32_t *d_queries, uint64_t q, uint32_t t,
                                     int mode, uint32_t slab_groups, uint32_t *d_idx, double *d_dist, uint32_t *d_sizes,
                                     double *d_matrix);

/* ---- The minimum spanning tree of a library (the reference's TODO.md complains of playlists that "drift": a
 * walk of this tree is a tour in which every song sounds like one heard before it) ----
 * One object answers "which songs belong together, without a number of clusters", "what are the sub-genres of this genre" and
 * "play everything so that each song follows from the last": cutting the tree's heaviest edges gives the single-linkage clusters
 * at every level, its sorted edges are the dendrogram, a depth-first walk is a tour at most twice the tree's length, and with
 * per-song core distances it is the tree HDBSCAN starts from.  Exact, all pairs, O(n) memory, every bit defined.
 * Inputs: x [n][d] f32, d <= 64; metric: BLISSGPU_METRIC_EUCLIDEAN, or BLISSGPU_METRIC_MAHALANOBIS with the caller's M (a
 * diagonal M is detected as everywhere else); core [n] f32 or NULL.
 *   dist(i, j) = bit for bit what blissgpu_pairwise_device(x, x) writes at [i][j] (the same bits at [j][i]);
 *   w(i, j)    = max(dist(i, j), core[i], core[j]) with core given (every core >= 0; -0.0 counts as +0.0), dist(i, j) without.
 *                With core[i] = the distance from i to its m-th nearest other song this is HDBSCAN's mutual reachability;
 *   key{i, j}  = for i < j the triple (the bits of w(i, j) as a uint32_t, i, j), compared lexicographically.  Weights are >= +0
 *                or +inf, so the integer order is the float order.  The order is strict and total: whatever the ties --
 *                duplicate songs, the plateaus core produces -- there is exactly one minimum spanning tree under it.
 * Outputs: the n - 1 edges of that tree in ascending key: edge_u [n - 1] u32 (the lower song), edge_v [n - 1] u32 (the higher),
 * edge_w [n - 1] f32.  rounds (host memory in both forms, may be NULL) receives the number of Boruvka rounds run: at most
 * ceil(log2 n).  n <= 1: no edge, BLISSGPU_OK, *rounds = 0, and no device is touched.
 * A NaN among the distances -- a NaN feature, a negative sum under an M that is not positive semi-definite -- or a core that
 * is NaN or negative returns BLISSGPU_ERR_INVALID with a message that says so (the first round evaluates every pair); nothing
 * is written to the outputs then.  BLISSGPU_ERR_INVALID too, each with a message that names the argument:
 * BLISSGPU_METRIC_COSINE; an unknown metric; Mahalanobis without M; d outside 1 .. 64; n >= 2^32 - 1; with n >= 2 a NULL x,
 * edge_u, edge_v or edge_w.  The loop over rounds is bounded: after 64 of them the call returns BLISSGPU_ERR_INTERNAL.
 * No n x n matrix is ever stored.  Workspace, grow-only in the context: 4 n bytes each of order, components and picked weights,
 * 8 n of picked edges, and 8 n per column group of the scan (a number the device's size bounds, about 8 192 CUs / n): O(n).
 * When that exceeds the context's workspace limit (blissgpu_ctx_get_workspace_limit) the call returns BLISSGPU_ERR_OOM before
 * anything is launched.  Per round the host receives one pick per component and sends the next order: 8 n bytes.
 * For the tests and the bench tool, read from the environment at every call, and without effect on any bit of the result:
 * BLISSGPU_MST_COL_GROUPS = the scan's column groups (default: the plan's), BLISSGPU_MST_SKIP = 0 turns off the late rounds'
 * skip of pairs inside one component, BLISSGPU_MST_TRACE prints every round's components and times to stderr. */
int blissgpu_mst(const float *x, uint64_t n, uint32_t d, int metric, const float *M, const float *core, uint32_t *edge_u,
                 uint32_t *edge_v, float *edge_w, uint32_t *rounds);
/* Device-resident form (device pointers, except rounds).  It checks the scalar arguments before it looks at its context, and
 * synchronises the context's stream once per round and once more before returning. */
int blissgpu_mst_device(blissgpu_ctx *ctx, const float *d_x, uint64_t n, uint32_t d, int metric, const float *d_M,
                        const float *d_core, uint32_t *d_edge_u, uint32_t *d_edge_v, float *d_edge_w, uint32_t *rounds);

/* ---- Ward clustering of a library: the whole dendrogram ----
 * A nested hierarchy of compact clusters -- a genre that opens into sub-genres that open into scenes: one tree, any K by cutting
 * it, K clusters always a refinement of K - 1.  Ward's minimum-variance linkage needs only the clusters' centroids and sizes,
 *   cost(A, B) = |A| |B| / (|A| + |B|) * ||c_A - c_B||^2   (the growth of the within-cluster sum of squares the merge causes),
 * so it is done like every scan here: all pairs on the device, O(n) memory, no n x n matrix.  Ward is reducible: every pair of
 * clusters that are each other's nearest may merge in the same round, which makes a few dozen rounds of n - 1 merges.
 * Inputs: rows c [m][d] f32, 1 <= d <= 64; sizes size [m] u32, NULL = all 1, every size >= 1, their sum < 2^24 (every size
 * and every sum of two is exact in f32); metric: BLISSGPU_METRIC_EUCLIDEAN, or BLISSGPU_METRIC_MAHALANOBIS with the caller's M
 * (a diagonal M is detected as everywhere else).  All arithmetic is f32, every operation rounded on its own, nothing fused,
 * division correctly rounded.
 * PAIR COST, for positions i != j:
 *   dist(i, j) = bit for bit what blissgpu_pairwise_device(c, c) writes at [i][j] (the same bits at [j][i], see blissgpu_mst);
 *   w(i, j)    = ((float)size[i] * (float)size[j]) / ((float)size[i] + (float)size[j]);
 *   cost(i, j) = (dist(i, j) * dist(i, j)) * w(i, j).
 * Costs are >= +0 or +inf, so the order of their bit patterns as uint32_t is the float order; cost(i, j) and cost(j, i) have
 * the same bits.
 * NEAREST.  nn[i] = the j != i with the smallest 64-bit key (bits(cost(i, j)) << 32) | (i XOR j), cost[i] = that cost.  The XOR
 * tie-break is deliberate: with "ties to the lower index" a block of B identical songs (silent tracks, duplicates) points at
 * one member and merges one pair per round; under the XOR rule the pair of equal-cost positions with the smallest i XOR j is
 * always mutual, so equal rows pair up like the leaves of a binary trie (300 identical rows: 9 rounds, not 299).
 * m == 1: nn[0] = 0xFFFFFFFF, cost[0] = +inf, no device is touched.  m == 0: nothing is touched.
 * THE TREE.  State: m clusters at positions 0 .. m - 1, each with a row, a size and low, its lowest member song.  Start:
 * m = n, the rows are x, all sizes 1, low[p] = p.  Round r = 0, 1, ... while m > 1:
 *   take nn and cost by the rule above; the round's pairs are all (p, q), p < q, with nn[p] == q and nn[q] == p (disjoint by
 *   construction); each pair emits an edge (u = low[p], v = low[q], cost[p], size[p] + size[q], r) and replaces row p by
 *     c_p[k] = (float)(((double)size[p] * (double)c_p[k] + (double)size[q] * (double)c_q[k]) / (double)(size[p] + size[q]))
 *   (the two products, the sum and the quotient each rounded in f64); size[p] += size[q]; position q disappears and the
 *   survivors keep their relative order, so the positions stay ordered by low and u < v always.
 * This procedure is the contract: the tree is what these rounds produce on these roundings, not "the" Ward dendrogram of the
 * exact costs (with which it agrees wherever the costs are apart by more than their rounding).
 * Outputs of blissgpu_ward: the n - 1 edges ascending in (bits(cost), round, u): edge_u, edge_v [n - 1] u32, edge_cost [n - 1]
 * f32, edge_size [n - 1] u32 (may be NULL), edge_round [n - 1] u32 (may be NULL); rounds (host memory, may be NULL) receives
 * the number of rounds.  n <= 1: no edge, BLISSGPU_OK, *rounds = 0, and no device is touched.
 * BLISSGPU_ERR_INVALID with a message, and nothing written, exactly when some cost of some round is NaN -- a NaN feature,
 * inf - inf, a negative sum under an M that is not positive semi-definite (every pair is evaluated in every round).
 * BLISSGPU_ERR_INVALID too, before the device is touched and each with a message that names the argument:
 * BLISSGPU_METRIC_COSINE; an unknown metric; Mahalanobis without M; d outside 1 .. 64; n (m) or the sum of the sizes >= 2^24;
 * a size of 0; a NULL c, x, edge_u, edge_v or edge_cost with n (m) >= 2, a NULL nn or cost with m >= 1.  A round that merges
 * nothing is a defect: BLISSGPU_ERR_INTERNAL.
 * Workspace, grow-only in the context and O(n): the best key of every position (8 n bytes, which the column groups of the scan
 * fold their winners into by 64-bit integer minima: a total order, so no split of the columns changes a bit), and for the tree
 * a copy of the rows (4 n d bytes, rewritten in place by the joins), two sets of sizes and low (16 n) and the join plan (8 n).
 * Beyond the context's workspace limit (blissgpu_ctx_get_workspace_limit) the call returns BLISSGPU_ERR_OOM before anything is
 * launched.  Per round the host receives 16 + 8 m bytes (one copy, one synchronisation) and sends the plan, 8 bytes per
 * surviving position.
 * For the tests and the bench tool, read from the environment at every call, and without effect on any bit of the result:
 * BLISSGPU_WARD_COL_GROUPS = the scan's column groups (default: the plan's), BLISSGPU_WARD_FILTER = 0 takes the root and the
 * weight of every pair, = 1 only of those a one-sided bound lets through (default: the latter in the scans of 12 288 positions
 * or more), BLISSGPU_WARD_TRACE prints every round's clusters, pairs and milliseconds to stderr.
 * Both are host-pointer forms over the context of the default device; there is no device-pointer form. */
int blissgpu_ward_nearest(const float *c, const uint32_t *size, uint64_t m, uint32_t d, int metric, const float *M, uint32_t *nn,
                          float *cost); /* one scan: what a round computes */
int blissgpu_ward(const float *x, uint64_t n, uint32_t d, int metric, const float *M, uint32_t *edge_u, uint32_t *edge_v,
                  float *edge_cost, uint32_t *edge_size, uint32_t *edge_round, uint32_t *rounds);

/* ---- k-medoids (PAM) of a library: K songs that stand for it, under any metric ----
 * k-means, the spanning tree and Ward answer with centroids or tree nodes and refuse the cosine; k-medoids answers with SONGS
 * -- "the 12 songs that summarise this collection" -- and needs only pairwise distances, so every metric of blissgpu_pairwise
 * works.  One objective, TD = the sum over the songs of the distance to the nearest medoid; each round makes the single swap
 * (a medoid out, a non-medoid in) that lowers TD most, found by one all-pairs scan on the device.  O(n + slab k) memory, no
 * n x n matrix.
 * DISTANCE.  dist(i, j) = bit for bit what blissgpu_pairwise_device(x, x) writes at [i][j] (the same bits at [j][i]); metric:
 * BLISSGPU_METRIC_EUCLIDEAN, BLISSGPU_METRIC_COSINE, or BLISSGPU_METRIC_MAHALANOBIS with the caller's M (a diagonal M is
 * detected as everywhere else).  A NaN among the evaluated distances returns BLISSGPU_ERR_NAN (under the cosine a zero row
 * gives one); the outputs are then unspecified.  Nothing is special-cased for a song's distance to itself: under the cosine it
 * need not be +0.
 * STATE.  med [k]: k distinct songs in slot order.  For every song o, idx / dist = what blissgpu_knn returns for the queries
 * x, the candidates x[med[0]], ..., x[med[k - 1]] and min(k, 2) neighbours (equal distances go to the lower slot):
 *   near[o] = idx[0],  d1[o] = dist[0],  d2[o] = dist[1], or +inf when k == 1;
 *   TD = 0.0 + (double)d1[0] + (double)d1[1] + ... + (double)d1[n - 1], one sequential f64 sum in ascending o.
 * ONE SCAN (blissgpu_pam_scan).  Inputs: x [n][d] f32; near [n] u32 (every entry < k), d1, d2 [n] f32 -- any values the caller
 * likes, they need not be a state of any medoids; a NaN in d1 or d2 is refused --; k; rows [q] u32 (every entry < n; any order,
 * repeats allowed), or NULL for every song (q is then ignored and taken as n).  For candidate c = rows[p] and slot m < k, over
 * the songs o with near[o] == m in ascending o, with doc = dist(c, o), every operation rounded on its own and nothing fused:
 *   A(c, m)     = 0.0 + sum of ((double)fminf(doc, d2[o]) - (double)d1[o])      (f32 minimum, two conversions, f64 difference)
 *   B(c, m)     = 0.0 + sum of fmin((double)doc - (double)d1[o], 0.0)           (f64 difference, f64 minimum)
 *   btot(c)     = 0.0 + B(c, 0) + B(c, 1) + ... + B(c, k - 1)                   (ascending m)
 *   delta(c, m) = (btot(c) - B(c, m)) + A(c, m)
 *   best(c), arg(c): start from delta(c, 0) and m = 0; for m = 1, 2, ... a delta(c, m) < best(c) replaces both (a strict
 *                    f64 <: equal values stay with the lower m, a NaN never replaces).
 * A slot without songs has A = B = 0.0.  A(c, m) is the change of TD when slot m's medoid leaves and c joins, B(c, m) the change
 * among slot m's songs when c joins and every medoid stays, so btot(c) is what adding c as a (k + 1)-th medoid would change and
 * delta(c, m) what swapping c into slot m would.  A candidate that is a medoid already is evaluated like any other.
 * Outputs, entry p for rows[p]: btot [q] f64, best [q] f64, arg [q] u32; A, B [q][k] f64 (either may be NULL).  No output bit
 * depends on the scan's column groups, on how the rows are cut into slabs to fit the workspace, or on the order of rows.
 * n == 0 or q == 0: BLISSGPU_OK, nothing is touched.
 * THE CLUSTERING (blissgpu_kmedoids).  init == NULL: the start is BUILD --
 *   slot 0 = the c with the smallest A(c, 0) of a scan with k = 1 under near[o] = 0, d1[o] = 0, d2[o] = +inf (the smallest
 *   sum of distances); slot j = 1, ..., k - 1 = the c that is not yet a medoid with the smallest btot(c) of a scan under the
 *   state of slots 0 .. j - 1; values are compared as f64 (-0.0 == +0.0), equal values go to the lower c, a NaN is never taken
 * -- otherwise init [k] u32, distinct songs < n.  Then rounds t = 0, 1, ...:
 *   1. take the state of med;  2. td_trace[t] = TD;  3. scan every c that is not a medoid;  4. take the smallest
 *   (best(c), c), compared as under BUILD;  5. if there is none, or its best(c) is not < 0, stop with converged = 1;
 *   6. if t == max_swaps, stop with converged = 0;  7. med[arg(c)] = c.
 * Outputs: medoids [k] u32 = med; labels [n] u32 = near and dist [n] f32 = d1 of the last state taken (dist may be NULL), so
 * the labels are always the nearest-medoid labels of the medoids returned; sizes [k] u32 (may be NULL) = the songs per slot;
 * td_trace f64, room for max_swaps + 1 entries, n_swaps + 1 of them written; n_swaps and converged (host memory).
 * 1 <= d <= 64, 1 <= k <= n, k <= BLISSGPU_KMEANS_MAX_K, n < 2^32 - 1; n == 0 is BLISSGPU_OK (*n_swaps = 0, *converged = 1)
 * and touches no device.  BLISSGPU_ERR_INVALID, before the device is touched and each with a message that names the argument:
 * an unknown metric; Mahalanobis without M; d, k, n or q outside those limits; a NULL x, near, d1, d2, btot, best, arg,
 * medoids, labels, td_trace, n_swaps or converged; a near entry >= k; a NaN in d1 or d2; a rows entry >= n; an init entry >= n
 * or one that occurs twice.
 * Workspace, grow-only in the context: O(n) -- the slots' sort, near, d1, d2, the medoids and their rows, the state's search,
 * about 48 n + 4 k d bytes and the sort's histograms -- and 16 k bytes per candidate of a slab for A and B.  The slab is every
 * candidate when that fits the context's workspace limit (blissgpu_ctx_get_workspace_limit); beyond it the slab shrinks; when
 * the O(n) part and ONE candidate's share do not fit, the call returns BLISSGPU_ERR_OOM before anything is launched.  (The
 * state's search keeps its partial lists in the k-nearest search's own buffer.)  Per round the host receives one record of 32
 * bytes -- the winner, its slot, its delta, TD, the NaN word -- with one synchronisation, and sends nothing but the swap.
 * For the tests and the bench tool, read from the environment at every call, and without effect on any bit of the result:
 * BLISSGPU_PAM_COL_GROUPS = the scan's column groups (default: the plan's; at most k are used), BLISSGPU_PAM_TRACE prints every
 * round's TD, winner, delta and milliseconds to stderr.
 * Both are host-pointer forms over the context of the default device; there is no device-pointer form. */
int blissgpu_pam_scan(const float *x, uint64_t n, uint32_t d, const uint32_t *near, const float *d1, const float *d2, uint32_t k,
                      int metric, const float *M, const uint32_t *rows, uint64_t q, double *btot, double *best, uint32_t *arg,
                      double *A, double *B); /* one scan: what a round computes */
int blissgpu_kmedoids(const float *x, uint64_t n, uint32_t d, uint32_t k, int metric, const float *M, const uint32_t *init,
                      uint32_t max_swaps, uint32_t *medoids, uint32_t *labels, float *dist, uint32_t *sizes, double *td_trace,
                      uint32_t *n_swaps, int32_t *converged);
/* The workspace of a call with these sizes under the limit ws_limit, without a device: plan [4] u64 = the bytes, the slab (the
 * candidates scanned at a time; q of them when everything fits), and the words and scan totals reserved for the sort of the
 * slots.  build != 0: blissgpu_kmedoids with init == NULL, which sorts every number of slots from 1 to k and reserves for the
 * largest of them (the sort's table is not monotone in the slots); build == 0: a scan, or a clustering from a given start.  q
 * is the number of candidates (n for a clustering).  BLISSGPU_ERR_OOM exactly when the call itself would return it. */
int blissgpu_pam_plan(uint64_t n, uint32_t d, uint32_t k, uint64_t q, int build, uint64_t ws_limit, uint64_t *plan);

/* ---- Learning the Mahalanobis matrix from training triplets ----
 * The reference has a `training_triplet` table ("song_1 and song_2 are closer together than they are to odd_one_out",
 * src/library.rs:542-556), a TODO.md that asks for "a way to learn a metric with a user survey", and no code that learns.
 *
 * ONE STEP.  x [n][d] f32, 1 <= d <= 64; triplets [T][3] u32 as (a, b, o); M [d][d] f32, NULL = the identity; margin >= 0.
 * All arithmetic is f64, every multiply and every add rounded on its own, sums ascending from 0.0.  For one triplet
 *   u[r] = (double)x[a][r] - (double)x[b][r],  v the same for (a, o),  w for (b, o);
 *   q(t) = sum_r t[r] * s_r  with  s_r = sum_c (double)M[r][c] * t[c];
 *   h1 = (margin + q(u)) - q(v),  h2 = (margin + q(u)) - q(w);  f1 = h1 > 0,  f2 = h2 > 0  (a hinge of exactly 0 is inactive).
 * Outputs: flags [T] u8 (may be NULL) = f1 | f2 << 1;  *n_active = sum(f1 + f2);  *loss = sum(f1 h1 + f2 h2);
 * G [d][d] f64 = sum((f1 + f2) u u' - f1 v v' - f2 w w'), exactly symmetric.  flags and n_active are exact by this contract: a
 * diagonal M (detected as everywhere) and the identity take a shorter route that gives the same bits.  loss and G are f64 sums
 * of those terms (every product of G rounded once) in an order that is a function of (T, d) alone: no floating-point atomics,
 * two calls return identical bits.
 * T == 0: BLISSGPU_OK with zero outputs.  A triplet with an index >= n: BLISSGPU_ERR_INVALID, found on the device, which reads
 * nothing outside x.  A NaN hinge: BLISSGPU_ERR_NAN.  a == b, b == o and the like are legal.  n, T < 2^32 - 1.  The arguments are
 * checked before the device is touched; n_active, loss and G must not be NULL. */
int blissgpu_triplet_step(const float *x, uint64_t n, uint32_t d, const uint32_t *triplets, uint64_t T, const float *M,
                          double margin, uint8_t *flags, uint64_t *n_active, double *loss, double *G);
/* Device-resident form: d_x, d_triplets, d_M and d_flags are device pointers; n_active, loss and G are HOST pointers (one
 * download of d d + 3 words).  Synchronises the context's stream. */
int blissgpu_triplet_step_device(blissgpu_ctx *ctx, const float *d_x, uint64_t n, uint32_t d, const uint32_t *d_triplets,
                                 uint64_t T, const float *d_M, double margin, uint8_t *d_flags, uint64_t *n_active,
                                 double *loss, double *G);

/* THE LOOP: projected gradient descent on  obj(M) = loss(M) / (2 T) + reg * |M - M_0|^2  over M = diag(w), w >= 0 (DIAGONAL) or
 * M = L'L (FULL), so every M it returns is positive semi-definite.  init: d non-negative finite f32 weights or NULL for ones;
 * w_0 = init, L_0 = diag(sqrt(init)), M_0 = diag(init).  Host arithmetic is f64, ascending, uncontracted (metric_learn.hpp).
 * Iteration t = 0, 1, ...:
 *   M_t = diag((float) w), or M_t[i][j] = (float) sum_k L[k][i] L[k][j] (upper half, mirrored);
 *   the step above at M_t gives loss_t, active_t, G_t;   obj_t = loss_t / (2 T) + reg * sum_ij (M_t - M_0)^2, row-major;
 *   M_t or obj_t not finite (or, after iteration 0, a NaN hinge: obj_t = NaN): stop, BLISSGPU_LEARN_DIVERGED;
 *   active_t == 0: stop, BLISSGPU_LEARN_CONVERGED;   t == max_iter: stop, BLISSGPU_LEARN_MAX_ITER;
 *   Gt = G_t / (2 T) + (2 reg) (M_t - M_0);   DIAGONAL: w <- max(0, w - lr Gt[r][r]);
 *   FULL: P[i][j] = sum_k L[i][k] Gt[k][j], L <- L - (2 lr) P.
 * Outputs (HOST pointers in both forms): M [d][d] = the M_t of the finite iteration with the lowest obj, the first such
 * (*best_iter); obj and active (may be NULL; room for max_iter + 1) get *n_iter + 1 entries; *n_iter = the updates made; *status.
 * T == 0 converges at once with M = M_0.  x and the triplets stay on the device; per iteration M is uploaded once and
 * (G, loss, n_active, error bits) downloaded once.  form, init, margin >= 0, reg >= 0, finite lr and the required outputs are
 * checked before the device is touched. */
#define BLISSGPU_METRIC_FORM_DIAGONAL 0
#define BLISSGPU_METRIC_FORM_FULL 1
#define BLISSGPU_LEARN_CONVERGED 0
#define BLISSGPU_LEARN_MAX_ITER 1
#define BLISSGPU_LEARN_DIVERGED 2
int blissgpu_learn_metric(const float *x, uint64_t n, uint32_t d, const uint32_t *triplets, uint64_t T, int form,
                          const float *init, double margin, double lr, double reg, uint32_t max_iter, float *M, double *obj,
                          uint64_t *active, uint32_t *n_iter, uint32_t *best_iter, int32_t *status);
int blissgpu_learn_metric_device(blissgpu_ctx *ctx, const float *d_x, uint64_t n, uint32_t d, const uint32_t *d_triplets,
                                 uint64_t T, int form, const float *init, double margin, double lr, double reg,
                                 uint32_t max_iter, float *M, double *obj, uint64_t *active, uint32_t *n_iter,
                                 uint32_t *best_iter, int32_t *status);

/* ---- Library statistics and covariance-based Mahalanobis metrics (the reference's TODO.md asks for "statistics
 * to the library trait", for "an M that neutralizes feature scaling imbalance" and for the genre clustering "to find an
 * appropriate M matrix", it has no code) ----
 * The first and second moments of the rows x [n][d] f32, per group of a labelling and pooled, every bit defined.
 * Inputs: x [n][d] f32, 1 <= d <= 64, n < 2^32 - 1; labels [n] u32, every one < k, 1 <= k <= BLISSGPU_KMEANS_MAX_K.  labels may
 * be NULL: k must then be 1 and every row is in group 0.
 * THE BLOCKED SUM  B(t_0 ... t_{m-1})  of f64 terms is the one summation order of this section:
 *   m <= BLISSGPU_MOMENTS_BLOCK:  0.0 + t_0 + t_1 + ..., sequential (m == 0: 0.0);
 *   otherwise:  B of the sequence of the sequential sums (each begun at 0.0) of consecutive blocks of BLISSGPU_MOMENTS_BLOCK
 *               terms, the last block may be short.
 * It is a function of m and the order of the terms alone; there are no atomics in it, every multiply and every add is rounded
 * on its own, and no bit of any output depends on how the work is dealt out on the device.
 * Outputs, with "the members of g" = the rows i with labels[i] == g in ASCENDING i, and count_g their number:
 *   counts [k] u32 = count_g;
 *   mean [k][d] f64 = B((double)x[i][r] over the members of g) / (double)count_g; an empty group has mean 0.0;
 *   m2 [k][d] f64 (may be NULL) = B(u * u over the members of g),  u = (double)x[i][r] - mean[g][r]; 0.0 for an empty group;
 *   min, max [k][d] f32 (may be NULL, both or neither) = the least and the greatest x[i][r] of the members; -0.0 orders below
 *       +0.0 here; an empty group gets +inf and -inf;
 *   S [d][d] f64 (may be NULL: the scatter pass is then skipped) = B(u_i[r] * u_i[c] over ALL rows i in ascending i),
 *       u_i[r] = (double)x[i][r] - mean[labels[i]][r].  The upper half (r <= c) is computed and mirrored: S is exactly
 *       symmetric.  With labels S is the pooled within-group scatter, without labels the total scatter.
 * A NaN or an infinity in x returns BLISSGPU_ERR_NAN; a label >= k returns BLISSGPU_ERR_INVALID; the outputs are then
 * unspecified.  BLISSGPU_ERR_INVALID also: d outside 1 .. 64; k outside 1 .. BLISSGPU_KMEANS_MAX_K; NULL labels with k != 1
 * (and n > 0); n >= 2^32 - 1; NULL x (with n > 0), counts or mean; one of min and max NULL and the other not.  n == 0 is BLISSGPU_OK with
 * zero counts, means, m2 and S, and +inf / -inf extrema.
 * The host form checks all of these, its labels included, before the device is touched.
 * Workspace, grow-only in the context: the k-means sort's O(n + chunks x k), 8 (d + d (d + 1) / 2) bytes per block of
 * BLISSGPU_MOMENTS_BLOCK rows, and O(k d). */
#define BLISSGPU_MOMENTS_BLOCK 256
int blissgpu_moments(const float *x, uint64_t n, uint32_t d, const uint32_t *labels, uint32_t k, uint32_t *counts, double *mean,
                     double *m2, float *min, float *max, double *S);
/* Device-resident form (device pointers throughout).  It checks the scalar arguments before it looks at its context, and
 * reports the data-dependent errors (a label >= k, a NaN or an infinity) at its one synchronisation of the context's stream
 * before returning; it reads nothing outside x and labels whatever the labels hold. */
int blissgpu_moments_device(blissgpu_ctx *ctx, const float *d_x, uint64_t n, uint32_t d, const uint32_t *d_labels, uint32_t k,
                            uint32_t *d_counts, double *d_mean, double *d_m2, float *d_min, float *d_max, double *d_S);

/* A scatter matrix turned into a Mahalanobis M.  Pure host code, no device is touched (covariance_metric.hpp); f64, sums
 * ascending from 0.0, every multiply and every add rounded on its own.  S [d][d] f64 (symmetric; the upper half is read),
 * dof > 0 the degrees of freedom (n - the number of non-empty groups), 0 <= shrink <= 1.
 *   C[r][c] = S[r][c] / (double)dof;   T = (0.0 + C[0][0] + C[1][1] + ...) / (double)d;
 *   BLISSGPU_METRIC_FORM_DIAGONAL:  w[r] = 1.0 / ((1.0 - shrink) * C[r][r] + shrink * T);  a w[r] that is not positive and
 *       finite is *status = BLISSGPU_COV_NOT_POSITIVE;
 *   BLISSGPU_METRIC_FORM_FULL:  C'[r][c] = (1.0 - shrink) * C[r][c], and C'[r][r] = (1.0 - shrink) * C[r][r] + shrink * T;
 *       Cholesky-Banachiewicz C' = L L', row i by row i, column j = 0 .. i:  s = 0.0 + L[i][0] L[j][0] + ... (k < j ascending),
 *       j < i: L[i][j] = (C'[i][j] - s) / L[j][j];  j == i: pivot = C'[i][i] - s, L[i][i] = sqrt(pivot); a pivot that is not
 *       positive and finite is BLISSGPU_COV_NOT_POSITIVE;
 *       Linv by forward substitution, column j, row i = j .. d - 1:  Linv[j][j] = 1.0 / L[j][j],
 *       Linv[i][j] = (0.0 - (0.0 + L[i][j] Linv[j][j] + ... + L[i][i-1] Linv[i-1][j])) / L[i][i]  (k = j .. i - 1 ascending);
 *       W[r][c] = 0.0 + Linv[c][r] Linv[c][c] + ... (k = c .. d - 1 ascending) for r <= c, mirrored  (W = Linv' Linv = C'^-1);
 *   both forms: tr = 0.0 + W[0][0] + W[1][1] + ...;  M[r][c] = (float)(W[r][c] * ((double)d / tr)): the trace of M is d, the
 *       convention of variance_based_weight_matrix.  A scale that is not positive and finite is BLISSGPU_COV_NOT_POSITIVE.
 * *status = BLISSGPU_COV_OK and M [d][d] f32 is written; or *status = BLISSGPU_COV_NOT_POSITIVE and M is left untouched.  Both
 * return BLISSGPU_OK.  BLISSGPU_ERR_INVALID: dof == 0, shrink outside [0, 1] (a NaN is), a form that is neither, d outside
 * 1 .. 64, a NULL pointer. */
#define BLISSGPU_COV_OK 0
#define BLISSGPU_COV_NOT_POSITIVE 1
int blissgpu_covariance_metric(const double *S, uint32_t d, uint64_t dof, int form, double shrink, float *M, int32_t *status);

/* The k nearest candidates of every seed GROUP: closest_to_songs(&group, candidates, metric) cut after k, what
 * Library::playlist_from(&[several songs]).take(k) (src/library.rs:762-842) asks per album, artist, genre or saved playlist,
 * for n_groups groups in one call.  seeds is [group_offsets[n_groups]][d] row-major; group g's seeds are the rows
 * group_offsets[g] .. group_offsets[g + 1], in sum order (group_offsets[0] == 0, non-decreasing; a HOST pointer in both forms:
 * the work is dealt out before anything is launched).  A candidate's score is 0.0f + m(seed_0, cand) + m(seed_1, cand) + ...,
 * added sequentially in f32 in seed order: bit for bit what blissgpu_set_distance writes for the same seeds.  An empty group
 * scores +0.0 everywhere (its row is the first k candidates).  Row g of idx / dist ([n_groups][k], dist may be NULL) is the
 * first k entries of the stable ascending order of the group's eligible candidates: equal scores in candidate order, rows with
 * fewer than k eligible candidates end in idx 0xFFFFFFFF / dist +inf.  skip is NULL or one candidate index per SEED ROW: that
 * candidate is left out of the seed's group and none of its distances to the group is looked at (how playlist_from keeps the
 * initial songs out; with one seed per group it is blissgpu_knn's skip); 0xFFFFFFFF skips nothing, any other value >= n is
 * BLISSGPU_ERR_INVALID.  A NaN score of an eligible (group, candidate) pair returns BLISSGPU_ERR_NAN; the outputs are then
 * unspecified.  1 <= k <= BLISSGPU_KNN_MAX_K, 1 <= d <= 64, n < 2^32 - 1, fewer than 2^32 seeds and 2^32 - 1 groups;
 * n_groups == 0 or n == 0 is BLISSGPU_OK (n == 0: every row is padding).  Arguments are checked before the device is touched,
 * the host form's skip on the host.  No seeds x n or n_groups x n array is ever stored: the workspace is O(items x k) keys,
 * two launches whatever n_groups, n and the group sizes. */
int blissgpu_group_knn(const float *seeds, const uint64_t *group_offsets, uint64_t n_groups, const float *cand, uint64_t n,
                       uint32_t d, int metric, const float *M, const uint32_t *skip, uint32_t k, uint32_t *idx, float *dist);
/* Device-resident form (device pointers, d_skip included; group_offsets stays a host pointer); asynchronous except for the
 * NaN / skip check, which synchronises the context's stream before returning. */
int blissgpu_group_knn_device(blissgpu_ctx *ctx, const float *d_seeds, const uint64_t *group_offsets, uint64_t n_groups,
                              const float *d_cand, uint64_t n, uint32_t d, int metric, const float *d_M,
                              const uint32_t *d_skip, uint32_t k, uint32_t *d_idx, float *d_dist);
/* How the two entry points above deal out the work for a device of n_cus compute units (>= 1): device-free.  Items are
 * rectangles, groups [g_lo, g_hi) x candidates [c_lo, c_hi), written as items[i][4] = g_lo, g_hi, c_lo, c_hi; they tile the
 * n_groups x n plane exactly once and c_lo is a multiple of *cand_block (the candidates of one staged block).  *seed_tile is
 * the most seed rows of one group held in LDS at once; a larger group streams through it without restarting its sum.  An
 * item's cost is (seeds of its groups) x (its candidates); no item costs more than
 * max(total cost / n_cus, cand_block x largest group) -- a group's sum cannot be split over workgroups without changing its
 * order, so one block of one group is the smallest unit.  *n_items is always written; nothing is written past max_items. */
int blissgpu_group_knn_plan(const uint64_t *group_offsets, uint64_t n_groups, uint64_t n, uint32_t k, uint32_t n_cus,
                            uint32_t *items, uint64_t max_items, uint64_t *n_items, uint32_t *cand_block,
                            uint32_t *seed_tile);

/* ---- one DIAGONAL metric per seed group ----
 * variance_based_weight_matrix (src/playlist.rs:173-221) is built from a seed set: an album whose songs agree on tempo and timbre
 * but not on key gets a playlist that follows tempo and timbre.  The two pairs of entry points below compute it for every group
 * on the device and search every group's k nearest candidates under its own metric, in one call. */
#define BLISSGPU_GROUP_OK 0
#define BLISSGPU_GROUP_TOO_FEW_SEEDS 1 /* fewer than 2 seeds: the reference's ProviderError("seeds must contain more than one element") */

/* variance_based_weight_matrix of EVERY seed group: weights[g][0 .. d) ([n_groups][d] row-major) is the DIAGONAL of the matrix
 * the reference returns for the rows group_offsets[g] .. group_offsets[g + 1] of seeds (a HOST pointer in both forms, as above).
 * The arithmetic is defined, every operation rounded to f32 on its own: mean = the sequential sum over the seeds in seed order,
 * divided by (float)count; var = var + diff * diff over the seeds in order, divided by the count; w = 1.0f / (var + 1e-6f);
 * total = ndarray's sum() (eight partial sums over k mod 8 for the whole eights, 0 + (p0 + p4) + (p1 + p5) + (p2 + p6) + (p3 + p7),
 * then the tail in order); w *= (float)d / total.  A group of fewer than two seeds (an empty one included) gets a row of 1.0f --
 * the identity, euclidean_distance's own M (src/playlist.rs:69) -- and BLISSGPU_GROUP_TOO_FEW_SEEDS in group_status ([n_groups],
 * may be NULL); every other group BLISSGPU_GROUP_OK.  That is not an error of the call.  Non-finite seeds give whatever this
 * arithmetic gives.  1 <= d <= 64, fewer than 2^32 seeds and 2^32 - 1 groups; n_groups == 0 is BLISSGPU_OK.  Arguments are
 * checked before the device is touched.  One launch whatever the groups (a wavefront per group). */
int blissgpu_group_weights(const float *seeds, const uint64_t *group_offsets, uint64_t n_groups, uint32_t d, float *weights,
                           int32_t *group_status);
/* Device-resident form (device pointers; group_offsets stays a host pointer); synchronises the context's stream before returning. */
int blissgpu_group_weights_device(blissgpu_ctx *ctx, const float *d_seeds, const uint64_t *group_offsets, uint64_t n_groups,
                                  uint32_t d, float *d_weights, int32_t *d_group_status);

/* blissgpu_group_knn with metric = Mahalanobis and ONE DIAGONAL M PER GROUP: M_g = diag(weights[g][0 .. d)), weights
 * [n_groups][d] row-major.  weights == NULL: the variance-based weights of each group's own seeds, computed on the device as
 * above; group_status (may be NULL) is then written as above, and with weights given it is filled with BLISSGPU_GROUP_OK.
 * Everything else is blissgpu_group_knn's contract -- sum order, stable order, skip, padding, the NaN rule (a NaN weight makes
 * its group's scores NaN: BLISSGPU_ERR_NAN when one of them belongs to an eligible candidate), limits, arguments checked before
 * the device is touched, no seeds x n or n_groups x n array -- with group g's metric mahalanobis_distance(., ., diag(weights[g])):
 * a score is bit for bit what blissgpu_set_distance returns for that group's seeds with M = diag(weights[g]).  Three launches
 * with derived weights, two with given ones, whatever n_groups, n and the group sizes; blissgpu_group_knn_plan describes the
 * split unchanged; the workspace grows by n_groups x d floats. */
int blissgpu_group_knn_weighted(const float *seeds, const uint64_t *group_offsets, uint64_t n_groups, const float *cand,
                                uint64_t n, uint32_t d, const float *weights, const uint32_t *skip, uint32_t k,
                                uint32_t *idx, float *dist, int32_t *group_status);
/* Device-resident form (device pointers, d_weights, d_skip and d_group_status included; group_offsets stays a host pointer);
 * asynchronous except for the NaN / skip check, which synchronises the context's stream before returning. */
int blissgpu_group_knn_weighted_device(blissgpu_ctx *ctx, const float *d_seeds, const uint64_t *group_offsets,
                                       uint64_t n_groups, const float *d_cand, uint64_t n, uint32_t d, const float *d_weights,
                                       const uint32_t *d_skip, uint32_t k, uint32_t *d_idx, float *d_dist,
                                       int32_t *d_group_status);

/* ---- the k nearest ALBUMS of every seed group (src/playlist.rs:424-485, src/library.rs:850-893) ----
 * closest_album_to_group cut after k albums -- what Library::album_playlist_from asks per album ("play this album, then the
 * albums most like it") -- for n_groups groups in one call.  seeds, group_offsets (a HOST pointer in both forms), cand and skip
 * are blissgpu_group_knn's; album_of is [n]: the album index (0 .. n_albums) of every candidate, 0xFFFFFFFF = the song has no
 * album.  For group g, every operation rounded to f32 on its own:
 *   group mean     mean_g = (0.0f + seed_0 + seed_1 + ...) / (float)s_g, the sum over the group's seed rows in seed order, per
 *                  feature: ndarray's mean_axis(Axis(0)) of a row-major array;
 *   album rows     R(g, a) = the candidates i with album_of[i] == a, in ascending i, WITHOUT the candidates named by group g's
 *                  skip entries: the reference removes the group's songs from the pool before it forms the album means;
 *   absent albums  an album with R(g, a) empty does not exist for group g (an album that is the whole group is not in the
 *                  reference's pool);
 *   centroid       centroid(g, a) = (0.0f + the rows of R(g, a) in order) / (float)|R(g, a)|; for an album no skip entry of g
 *                  touches this is the group-independent full-album centroid;
 *   distance       dist(g, a) = euclidean_distance(mean_g, centroid(g, a)), bit for bit what blissgpu_distance /
 *                  blissgpu_pairwise return for those two vectors (the reference hard-codes euclidean here).
 * Row g of idx / dist ([n_groups][k], dist may be NULL) holds the first k existing albums in ascending (dist, album index)
 * order: equal distances come in album-index order (-0.0 and +0.0 are equal), infinite distances sort last, rows with fewer
 * than k existing albums end in idx 0xFFFFFFFF / dist +inf.  (The reference leaves ties to HashMap iteration order.)
 * group_means ([n_groups][d], may be NULL) receives mean_g; centroids ([n_albums][d], may be NULL) the FULL-album means, an
 * album without any song a row of NaN (it is absent for every group) -- for callers that cache centroids.
 * A NaN distance of an existing (group, album) pair returns BLISSGPU_ERR_NAN (the reference's n32() panic); the outputs are
 * then unspecified.  An empty group is BLISSGPU_ERR_INVALID (the reference's "Mean of empty slice"), decided from group_offsets.
 * 1 <= k <= BLISSGPU_KNN_MAX_K, 1 <= d <= 64, n < 2^32 - 1, n_albums <= n, fewer than 2^32 seeds and 2^32 - 1 groups; an
 * album_of entry >= n_albums or a skip entry >= n, other than 0xFFFFFFFF, is BLISSGPU_ERR_INVALID.  n_groups == 0 is
 * BLISSGPU_OK; so is n == 0 or n_albums == 0 (every row is padding).  Every check that needs no device data happens before the
 * device is touched, the host form's album_of and skip on the host.  No n_groups x n_albums array is ever stored: the workspace
 * is O(n_albums d + n_groups d + touched (group, album) pairs x d + items x k), at most one touched pair per seed row; three
 * launches whatever n_groups, n_albums and the group sizes. */
int blissgpu_album_knn(const float *seeds, const uint64_t *group_offsets, uint64_t n_groups, const float *cand, uint64_t n,
                       uint32_t d, const uint32_t *album_of, uint64_t n_albums, const uint32_t *skip, uint32_t k,
                       uint32_t *idx, float *dist, float *group_means, float *centroids);
/* Device-resident form (device pointers, d_album_of, d_skip and the outputs included; group_offsets stays a host pointer).  The
 * album row lists are derived on the host: d_album_of and d_skip are read back first, which synchronises the context's stream,
 * as the NaN check at the end does. */
int blissgpu_album_knn_device(blissgpu_ctx *ctx, const float *d_seeds, const uint64_t *group_offsets, uint64_t n_groups,
                              const float *d_cand, uint64_t n, uint32_t d, const uint32_t *d_album_of, uint64_t n_albums,
                              const uint32_t *d_skip, uint32_t k, uint32_t *d_idx, float *d_dist, float *d_group_means,
                              float *d_centroids);

/* ---- song-to-song chains cut after k, one per seed group (src/playlist.rs:272-326) ----
 * Row g of idx / dist ([n_groups][k], dist may be NULL) is the first k songs of song_to_song(&group g, candidates without the
 * group's skipped rows, metric) -- a "journey" playlist starting at every song, album or saved playlist of a library, in one
 * call.  seeds, group_offsets (a HOST pointer in every form) and skip are blissgpu_group_knn's.  For group g:
 *   idx[g][0]  the eligible candidate with the smallest set distance to the group's seeds: the sequential f32 sum in seed
 *              order, bit for bit blissgpu_set_distance (an empty group scores +0.0 everywhere: the first eligible candidate);
 *   idx[g][t]  t >= 1: the eligible candidate not yet taken by this chain with the smallest 0.0f + metric(cand[idx[g][t - 1]],
 *              cand[j]), bit for bit what blissgpu_song_to_song evaluates;
 * dist[g][t] is the winning value.  Among equal values the lowest candidate index wins (-0.0 and +0.0 are equal).  A row with
 * fewer than k eligible candidates ends in idx 0xFFFFFFFF / dist +inf.  BLISSGPU_ERR_NAN is returned exactly when a chain
 * evaluates a NaN within the steps it runs (the reference's argmin().unwrap() panic); the distances FROM the k-th song, and those
 * to skipped or already taken candidates, are never looked at.  Metrics: euclidean, cosine, Mahalanobis with one M.
 * 1 <= k <= BLISSGPU_KNN_MAX_K, 1 <= d <= 64, n < 2^32 - 1, fewer than 2^32 seeds and 2^32 - 1 groups; n_groups == 0 or n == 0
 * is BLISSGPU_OK (n == 0: every row is padding).  Arguments are checked before the device is touched, the host form's skip on
 * the host.
 * route picks how the steps after the first are computed; the result and the error do not depend on it:
 *   BLISSGPU_CHAINS_STEPS  one launch per step over every chain (two when several workgroups share a chain's candidates):
 *                          (k - 1) x n_groups x n pairs, no grid barrier, no workspace beyond O(n_groups);
 *   BLISSGPU_CHAINS_LISTS  the L = k + largest group - 1 nearest candidates of EVERY candidate (blissgpu_knn over the candidates
 *                          themselves, n x n pairs), then one walk over those lists.  Needs L <= BLISSGPU_KNN_MAX_K (else
 *                          BLISSGPU_ERR_INVALID, before the device is touched) and 16 n L + 4 n bytes within the context's
 *                          workspace limit (else BLISSGPU_ERR_INVALID).  A NaN met by the all-pairs search that no chain
 *                          evaluates does not fail the call: it is then answered by steps;
 *   BLISSGPU_CHAINS_AUTO   what blissgpu_chains_plan says for the context's workspace limit. */
#define BLISSGPU_CHAINS_AUTO 0
#define BLISSGPU_CHAINS_STEPS 1
#define BLISSGPU_CHAINS_LISTS 2
int blissgpu_chains(const float *seeds, const uint64_t *group_offsets, uint64_t n_groups, const float *cand, uint64_t n,
                    uint32_t d, int metric, const float *M, const uint32_t *skip, uint32_t k, int route, uint32_t *idx,
                    float *dist);
/* Device-resident form (device pointers, d_skip included; group_offsets stays a host pointer); synchronises the context's
 * stream before returning (the NaN / skip check). */
int blissgpu_chains_device(blissgpu_ctx *ctx, const float *d_seeds, const uint64_t *group_offsets, uint64_t n_groups,
                           const float *d_cand, uint64_t n, uint32_t d, int metric, const float *d_M, const uint32_t *d_skip,
                           uint32_t k, int route, uint32_t *d_idx, float *d_dist);
/* The route BLISSGPU_CHAINS_AUTO takes with a workspace limit of workspace_bytes: a pure function of the sizes, device-free.
 * *list_len (may be NULL) = k + largest group - 1.  *route = BLISSGPU_CHAINS_LISTS when k >= 2, *list_len <=
 * BLISSGPU_KNN_MAX_K, the lists fit workspace_bytes and c x n < (k - 1) x n_groups -- c the measured cost of a pair of the lists
 * route in pairs of a step; BLISSGPU_CHAINS_STEPS otherwise. */
int blissgpu_chains_plan(const uint64_t *group_offsets, uint64_t n_groups, uint64_t n, uint32_t k, uint64_t workspace_bytes,
                         int *route, uint32_t *list_len);

/* ---- journeys: waypoint and directed song-to-song playlists ----
 * The reference has no code for these; its roadmap (TODO.md, "New features") names them: "A waypoint feature: go from song1
 * to song2, both picked by the users, in n songs, without any repetitions" and "A direction feature ('I want the tempo to go
 * down or stay the same')".  Both are the loop of blissgpu_chains -- k steps, each a masked nearest-candidate search over every
 * candidate, one launch per step over every journey -- with another query row or a narrower set of eligible candidates.
 * Journey g has a start row from[g] (d floats), in WAYPOINT mode an end row to[g], and two skip slots skip[g][0 .. 2): candidate
 * indices that are never eligible and never evaluated (normally the rows of the end points when they are candidates
 * themselves), 0xFFFFFFFF = none.  Row g of idx / dist ([n_journeys][k]) is the journey:
 *   BLISSGPU_JOURNEY_CHAIN     the query of step 0 is from[g], the query of step t >= 1 is cand[idx[g][t - 1]];
 *   BLISSGPU_JOURNEY_WAYPOINT  the query of step t is w_t[f] = from[g][f] + (to[g][f] - from[g][f]) * s_t with
 *                              s_t = (float)(t + 1) / (float)(k + 1); difference, product and sum are each rounded to f32.
 * idx[g][t] is the ELIGIBLE candidate j with the smallest 0.0f + metric(query, cand[j]) -- bit for bit what blissgpu_knn /
 * blissgpu_pairwise_device give for that pair -- the lowest index among equal values; dist[g][t] (dist may be NULL) is that
 * value.  Candidate j is eligible at step t when it is not in skip[g], not in idx[g][0 .. t) and, with a gate,
 * cand[j][gate_feature] >= ref (BLISSGPU_GATE_UP) or <= ref (BLISSGPU_GATE_DOWN), ref = from[g][gate_feature] at step 0 and
 * cand[idx[g][t - 1]][gate_feature] afterwards.  Equality passes ("down or stay the same"); a NaN on either side of the
 * comparison makes the candidate ineligible; an ineligible candidate's distance is never looked at.  When no candidate is
 * eligible the journey ends: that step and every later one keep the padding 0xFFFFFFFF / +inf.
 * CHAIN with any gate and WAYPOINT with BLISSGPU_GATE_NONE are allowed; a gate with WAYPOINT is BLISSGPU_ERR_INVALID.  to is
 * NULL unless WAYPOINT and must not be NULL in WAYPOINT mode; skip may be NULL.  Limits as for blissgpu_chains: 1 <= k <=
 * BLISSGPU_KNN_MAX_K, 1 <= d <= 64, n < 2^32 - 1, n_journeys < 2^31, gate_feature < d (looked at only with a gate), metrics and M
 * as for blissgpu_knn (a diagonal M is detected); the host form also refuses a skip entry >= n other than 0xFFFFFFFF.  All of
 * this is BLISSGPU_ERR_INVALID and checked before the device is touched.  n_journeys == 0 or n == 0 is BLISSGPU_OK (n == 0:
 * every row is padding).  BLISSGPU_ERR_NAN exactly when a step that runs evaluates a NaN distance for an eligible candidate
 * (the outputs are then unspecified).  CHAIN with BLISSGPU_GATE_NONE is blissgpu_chains for one-seed groups, WAYPOINT with
 * to == from the first k entries of blissgpu_knn for from, both bit for bit.  min(k, n) launches (twice that when few
 * journeys share the device and several workgroups split a journey's candidates); the workspace is 8 bytes per journey. */
#define BLISSGPU_JOURNEY_CHAIN 0
#define BLISSGPU_JOURNEY_WAYPOINT 1
#define BLISSGPU_GATE_NONE 0
#define BLISSGPU_GATE_UP 1
#define BLISSGPU_GATE_DOWN 2
int blissgpu_journeys(const float *from, const float *to, uint64_t n_journeys, const float *cand, uint64_t n, uint32_t d,
                      int metric, const float *M, const uint32_t *skip, uint32_t k, int mode, int gate, uint32_t gate_feature,
                      uint32_t *idx, float *dist);
/* Device-resident form (device pointers, d_skip included); synchronises the context's stream before returning (the NaN
 * check). */
int blissgpu_journeys_device(blissgpu_ctx *ctx, const float *d_from, const float *d_to, uint64_t n_journeys, const float *d_cand,
                             uint64_t n, uint32_t d, int metric, const float *d_M, const uint32_t *d_skip, uint32_t k, int mode,
                             int gate, uint32_t gate_feature, uint32_t *d_idx, float *d_dist);

/* ---- radio playlists: artist and album separation rules ----
 * Every program built on the reference bolts the same rules onto its playlists on the host: no artist twice within w tracks,
 * no album twice within w tracks, at most c songs per artist in a list.  A greedy chain cannot be filtered afterwards -- a
 * banned pick changes every later step -- so the rules are part of the step here.  Radio g has a start row from[g] (d floats)
 * and two skip slots skip[g][0 .. 2) as for blissgpu_journeys (0xFFFFFFFF = none; skip may be NULL).  Row g of idx / dist
 * ([n_radios][k]; dist may be NULL) is the radio:
 *   BLISSGPU_RADIO_CHAIN    the query of step 0 is from[g], the query of step t >= 1 is cand[idx[g][t - 1]] (song to song);
 *   BLISSGPU_RADIO_NEAREST  the query of every step is from[g] (the k nearest songs under the rules).
 * labels is [n_rules][n]: one label per rule and candidate (artist id, album id, ...); 0xFFFFFFFF = the song has no label and
 * the rule never constrains it.  from_labels is [n_radios][n_rules], the start songs' labels; NULL = the starts carry none.
 * window and limit (HOST arrays of n_rules, in both forms) state rule r: among the last window[r] songs of the radio at most
 * limit[r] may carry any one label.  The history of radio g at step t is position -1 (the start, labelled from_labels[g][r])
 * followed by positions 0 .. t - 1 (its picks).  Candidate j is eligible at step t when it is not in skip[g], not in
 * idx[g][0 .. t), and for every rule r with window[r] >= 1 and L = labels[r][j] != 0xFFFFFFFF the number of history positions
 * p with t - window[r] <= p < t that carry label L is < limit[r].  window[r] == 0 switches rule r off; window[r] > k behaves
 * as k + 1 (the whole list and the start); limit[r] == 0 is BLISSGPU_ERR_INVALID.
 * idx[g][t] is the eligible candidate j with the smallest 0.0f + metric(query, cand[j]) -- bit for bit what
 * blissgpu_pairwise_device writes for the pair -- the lowest index among equal values (-0.0 and +0.0 are equal); dist[g][t] is
 * that value.  When no candidate is eligible the radio ends: that step and every later one keep 0xFFFFFFFF / +inf.  An
 * ineligible candidate's distance is never looked at; BLISSGPU_ERR_NAN exactly when a step that runs evaluates a NaN for an
 * eligible candidate (the outputs are then unspecified).  Limits, metrics and M as for blissgpu_journeys (1 <= k <=
 * BLISSGPU_KNN_MAX_K, 1 <= d <= 64, n < 2^32 - 1, n_radios < 2^31, a diagonal M is detected); n_rules <=
 * BLISSGPU_RADIO_MAX_RULES; labels, window or limit NULL with n_rules > 0 is BLISSGPU_ERR_INVALID; the host form also refuses a
 * skip entry >= n other than 0xFFFFFFFF.  All of this is checked before the device is touched.  n_radios == 0 or n == 0 is
 * BLISSGPU_OK (n == 0: every row is padding).  With n_rules == 0 -- or every label 0xFFFFFFFF, every window 0, or limit[r] >
 * window[r] without from_labels -- CHAIN is blissgpu_journeys(CHAIN, GATE_NONE) and NEAREST the first k entries of
 * blissgpu_knn, bit for bit.  Two launches per step (three when few radios share the device); the workspace is 8 bytes per
 * radio plus 4 (1 + max_r min(window[r], k) / limit[r]) bytes per radio and rule that can ban anything, counted against the
 * context's workspace limit (BLISSGPU_ERR_OOM beyond it).  In the host form from == cand (the same pointer, n_radios <= n: a
 * radio from each of the first n_radios candidates) uploads the rows once. */
#define BLISSGPU_RADIO_MAX_RULES 4u
#define BLISSGPU_RADIO_CHAIN 0
#define BLISSGPU_RADIO_NEAREST 1
int blissgpu_radio(const float *from, uint64_t n_radios, const float *cand, uint64_t n, uint32_t d, int metric, const float *M,
                   const uint32_t *labels, const uint32_t *from_labels, uint32_t n_rules, const uint32_t *window,
                   const uint32_t *limit, const uint32_t *skip, uint32_t k, int mode, uint32_t *idx, float *dist);
/* Device-resident form (device pointers, d_labels, d_from_labels and d_skip included; window and limit stay HOST pointers);
 * synchronises the context's stream before returning (the NaN check). */
int blissgpu_radio_device(blissgpu_ctx *ctx, const float *d_from, uint64_t n_radios, const float *d_cand, uint64_t n, uint32_t d,
                          int metric, const float *d_M, const uint32_t *d_labels, const uint32_t *d_from_labels, uint32_t n_rules,
                          const uint32_t *window, const uint32_t *limit, const uint32_t *d_skip, uint32_t k, int mode,
                          uint32_t *d_idx, float *d_dist);

/* ---- a 2-D map of a library: exact t-SNE, stepped on the device ----
 * Every other library call returns lists; this one returns a picture: a point per song on a plane where sonic neighbours are
 * neighbours.  All pairs are visited in every iteration, no n x n matrix is stored, and every sum has a fixed order, so the
 * result is bit for bit what a sequential loop over the statements below gives.
 *
 * Inputs.  Y is [n][2] f32.  P, the symmetric affinity matrix, is in CSR form: row_offsets uint64[n + 1] (row_offsets[0] = 0,
 * not decreasing, nnz = row_offsets[n]), cols uint32[nnz] (strictly ascending inside a row, never the row itself, < n), vals
 * float[nnz] (finite, >= 0).  Symmetry is the caller's business: the arithmetic below reads rows only.
 *
 * Every operation below is rounded on its own (nothing is fused); f32 division is correctly rounded.
 * Pair quantities, f32, for a row i and any j != i:
 *   dx = Y[i][0] - Y[j][0];  dy = Y[i][1] - Y[j][1];  s = dx * dx + dy * dy  (the two products, then their sum; s may be +inf);
 *   q = 1.0f / (1.0f + s).
 * Repulsion.  The range of j is cut into C = col_groups chunks of w = 256 * ceil(ceil(n / C) / 256) consecutive indices each
 * (chunk c is c w <= j < min(n, (c + 1) w); a chunk that starts at or beyond n is empty).  Per row i and chunk, three f64 sums
 * start at +0.0 and take, for j ascending over the chunk with j != i:
 *   z += (double)q;   rx += (double)((q * q) * dx);   ry += (double)((q * q) * dy)        (the products are f32).
 * z_i, rx_i, ry_i are the chunk sums added in chunk order, each from +0.0.
 * Attraction.  Per row i two f64 sums start at +0.0 and take the row's CSR entries e in stored order, with j = cols[e]:
 *   w = vals[e] * q(i, j)  (f32);   ax += (double)(w * dx);   ay += (double)(w * dy).
 * Normaliser.  Z is the f64 sum of the z_i: rows are taken in blocks of 256 consecutive rows, each block's z_i are added in
 * ascending order from +0.0, and the block sums are added in ascending order from +0.0.
 * Gradient, f64:  grad[i][c] = 4.0 * (E * a_c - r_c / Z)  with E = (double)exaggeration, a = (ax, ay), r = (rx, ry): the
 * product, the quotient, their difference, the product with 4.0.  For n < 2: grad = 0, Z = 0, z_rows = 0, BLISSGPU_OK.
 * Update.  Per element e of [n][2] the f64 state is U[e] (starts at 0) and gain[e] (starts at 1); with g = grad[e]:
 *   gain = (U * g < 0.0) ? gain + 0.2 : gain * 0.8;   gain = max(gain, min_gain);
 *   U = mom * U - (lr * gain) * g;   Y[e] = (float)((double)Y[e] + U).
 * Loop.  Iteration it of [0, n_iter) is a gradient from the current Y, then the update, with (exaggeration, momentum0) while
 * it < exag_iters and (1.0, momentum1) afterwards; z_trace[it] is that iteration's Z.  U and gain start anew in every call.
 *
 * blissgpu_map_step: one gradient evaluation: grad double[n][2], z_rows double[n] (the z_i; may be NULL), *Z.
 * blissgpu_map_layout: the loop from y0; y_out float[n][2] (may be y0), z_trace double[n_iter] (may be NULL).  The iterations
 * are queued without a host synchronisation between them and the call synchronises once.  BLISSGPU_ERR_NAN exactly when
 * n >= 2 and a traced Z is not finite or not > 0 (a NaN or an infinity in y0; every point at infinite distance of every other).
 * n == 0, and n_iter == 0 (y_out = y0), are BLISSGPU_OK; with n == 1 y_out = y0 and every traced Z is 0.
 * col_groups: 1 .. 64, or 0 = what blissgpu_map_plan names for the context's device.  No bit of a result depends on anything
 * but the arguments: two calls with the same col_groups agree on every device.
 * BLISSGPU_ERR_INVALID, checked before the device is touched: a NULL array (z_rows and z_trace excepted), n >= 2^24, nnz >=
 * 2^32, row_offsets that do not start at 0 or that decrease, a row that is unsorted, holds a duplicate or holds itself, an
 * entry of cols >= n, a negative or non-finite entry of vals, col_groups > 64, a parameter that is not finite.  The
 * workspace is 72 + 24 C bytes per row (no partials with one chunk) and 8 bytes per iteration (the trace), counted against the
 * context's workspace limit: BLISSGPU_ERR_OOM beyond it.  Host-pointer forms only, run on the default context. */
int blissgpu_map_step(const float *y, uint64_t n, const uint64_t *row_offsets, const uint32_t *cols, const float *vals,
                      float exaggeration, uint32_t col_groups, double *grad, double *z_rows, double *Z);
int blissgpu_map_layout(const float *y0, uint64_t n, const uint64_t *row_offsets, const uint32_t *cols, const float *vals,
                        uint32_t n_iter, uint32_t exag_iters, float exaggeration, double learning_rate, double momentum0,
                        double momentum1, double min_gain, uint32_t col_groups, float *y_out, double *z_trace);
/* What col_groups == 0 resolves to on a device of n_cus compute units (0: 256); pure, no device is touched.  With
 * B = ceil(n / 256) row blocks: 1 when B <= 1, else min(ceil(4 n_cus / B), B, 64) -- enough 256-row workgroups for four
 * wavefronts on every SIMD, no chunk narrower than one block.  It is 1 once B >= 4 n_cus, the rows alone filling the device,
 * so the partials it asks for never pass 24 * 2 * 256 * 4 * n_cus bytes (12 MiB on 256 compute units).  That is the cap: the
 * function is device-free and does not know a context's workspace limit, whose floor at creation is 256 MiB; on a context
 * whose limit was set below what 72 + 24 col_groups bytes per row need, col_groups = 0 is BLISSGPU_ERR_OOM like any other. */
int blissgpu_map_plan(uint64_t n, uint32_t n_cus, uint32_t *col_groups);

/* ---- duplicate songs of a whole collection ----
 * The duplicate rule of dedup_playlist_custom_distance (src/playlist.rs:381-388) applied to EVERY pair of the n x d matrix x
 * instead of the neighbours of an ordered playlist: the pair (i, j), i < j, is an edge when D[i][j] < threshold (D[i][j] is bit
 * for bit what blissgpu_pairwise_device(x, x) writes at row i, column j; the reference's default threshold is 0.05f) or when
 * meta != NULL && meta[i] != 0 && meta[i] == meta[j] (one title / artist key per row, as for blissgpu_dedup_playlist).
 *   label[i]  the smallest row index of i's connected component of that graph (the closure is transitive)
 *   *n_pairs  the number of edges; always written
 *   pairs     may be NULL; [max_pairs][2], every edge as (i, j) with i < j; pair_dist (may be NULL, only written along with
 *             pairs) holds D[i][j] of the same entry, also for an edge that exists through meta only.  With *n_pairs <=
 *             max_pairs the host form returns the edges in ascending (i, j), the device form the same set in unspecified order;
 *             with *n_pairs > max_pairs the list's contents are unspecified and the call is still BLISSGPU_OK (size the buffer
 *             and call again).  Nothing is written past max_pairs entries; the labels never depend on the pair buffer.
 * label, *n_pairs and the set of pairs are functions of the inputs alone.  A NaN D[i][j] for any i < j returns
 * BLISSGPU_ERR_NAN (the reference's n32() panic); the outputs are then unspecified.  threshold <= 0: no distance edges; a NaN
 * threshold, d outside 1 .. 64, n >= 2^32 - 1, an unknown metric or Mahalanobis without M are BLISSGPU_ERR_INVALID, checked
 * before the device is touched.  n == 0 is BLISSGPU_OK.  No n x n or slab x n array exists: the workspace is the label array
 * and the caller's pair buffer; three launches whatever n. */
int blissgpu_duplicate_groups(const float *x, uint64_t n, uint32_t d, const uint32_t *meta, int metric, const float *M,
                              float threshold, uint32_t *label, uint64_t *n_pairs, uint32_t *pairs, float *pair_dist,
                              uint64_t max_pairs);
/* Device-resident form (device pointers, d_n_pairs included); asynchronous except for the NaN check, which synchronises the
 * context's stream before returning. */
int blissgpu_duplicate_groups_device(blissgpu_ctx *ctx, const float *d_x, uint64_t n, uint32_t d, const uint32_t *d_meta,
                                     int metric, const float *d_M, float threshold, uint32_t *d_label, uint64_t *d_n_pairs,
                                     uint32_t *d_pairs, float *d_pair_dist, uint64_t max_pairs);

/* ---- acoustic fingerprints: the same RECORDING found again ----
 * The reference's TODO.md asks for "better duplicate finding in the playlist module (sometimes songs have different [features]
 * across albums but should have the same fingerprint)"; it has no code for it.  The fingerprint is the one of Haitsma & Kalker,
 * "A Highly Robust Audio Fingerprinting System" (ISMIR 2002), on the 22 050 Hz mono f32 samples blissgpu_analyze_batch takes:
 * its 0.37 s frame is exactly 8192 samples here.  Opt-in: no analyze_* entry point computes it.
 *
 * Frames.  Frame f covers samples [512 f, 512 f + 8192); no padding, no reflection.  A song of n >= 8704 samples has
 * frames = (n - 8192) / 512 + 1 frames and words = frames - 1 = (n - 8192) / 512 sub-fingerprints (integer division); a song of
 * n < 8704 samples has status BLISSGPU_SONG_TOO_SHORT and 0 words.  blissgpu_fingerprint_len returns `words` (device-free).
 *
 * Spectrum.  The window is the periodic Hann window of the analysis STFT (0.5f - 0.5f * cosf(2.0f * n * PI_F / 8192.0f) in f32);
 * the window product is rounded to f32, as the STFT does; the FFT is a real FFT-8192 in f32.
 *
 * Bands.  33 bands over 300 .. 2000 Hz, logarithmically spaced: the bin edges are k_b = rint(300 (2000 / 300)^(b / 33) 8192 /
 * 22050), b = 0 .. 33 -- but the contract is the integer table itself, not the formula:
 *   111 118 125 132 140 149 157 167 177 187 198 210 222 235 249 264 280 296 314 332 352 373 395 418 443 469 497 526 557 590 625
 *   662 702 743
 * (blissgpu_fingerprint_bands returns it, device-free).  Band b is bins [k_b, k_{b+1}), and
 *   E[f][b] = sum over k of ((double)re_k * (double)re_k + (double)im_k * (double)im_k),
 * an f64 sum in ascending bin order taken from the f32 FFT outputs.
 *
 * Bits.  For t = 1 .. frames - 1 and b = 0 .. 31:  m = (E[t][b] - E[t][b+1]) - (E[t-1][b] - E[t-1][b+1]), evaluated in f64 in
 * exactly this association; bit b (LSB = band 0) of word[t-1] is 1 iff m > 0.  Two consecutive frames of digital silence give
 * word 0: a word equal to 0 marks silence, and the match leaves it out.
 *
 * blissgpu_fingerprint_batch (host pointers): song s is pcm[sample_offsets[s] .. sample_offsets[s + 1]) (n_songs + 1 ascending
 * offsets); word_offsets [n_songs + 1] is filled BY THE CALLER from blissgpu_fingerprint_len (word_offsets[0] = 0; anything else
 * is BLISSGPU_ERR_INVALID, as is a song of more than 2^22 words).  words [word_offsets[n_songs]] receives song s's words at
 * word_offsets[s], status [n_songs] BLISSGPU_SONG_OK or BLISSGPU_SONG_TOO_SHORT.  energies (may be NULL; the tests' tap) is f64
 * [word_offsets[n_songs] + n_songs][33]: frame f of song s is row word_offsets[s] + s + f; a too-short song owns one row, all
 * zero.  An all-zero frame has energies exactly 0.0.  Runs on the default context; n_songs == 0 is BLISSGPU_OK. */
uint64_t blissgpu_fingerprint_len(uint64_t n_samples);
int blissgpu_fingerprint_bands(uint32_t *edges); /* edges [34] */
int blissgpu_fingerprint_batch(const float *pcm, const uint64_t *sample_offsets, const uint64_t *word_offsets, uint32_t n_songs,
                               uint32_t *words, int32_t *status, double *energies);
/* The match.  For fingerprints a (length la) and b (length lb) and an offset o in [-max_offset, max_offset]: the positions are
 * those t with 0 <= t < la and 0 <= t + o < lb; a position is valid when a[t] != 0 and b[t + o] != 0;
 *   bits(o) = 32 * #valid,  errors(o) = sum over the valid positions of popcount(a[t] ^ b[t + o]).
 * An offset counts only when #valid >= min_overlap.  The best offset minimises errors / bits, compared exactly
 * (e * bits' < e' * bits in 64-bit integers); ties go to the smaller (|o|, o).  Per pair: offset, errors and bits of the best
 * offset; bits == 0, errors == 0 and offset == 0 when no offset counts.  Pure integer work: the result is defined to the bit.
 * pairs is u32 [n_pairs][2], indices into the n_songs fingerprints words[word_offsets[s] .. word_offsets[s + 1]); a pair (i, i)
 * is allowed.  Limits: at most 2^22 words per song, max_offset <= 4096, min_overlap >= 1, n_pairs < 2^32.  A pair that names a
 * song >= n_songs or a song without words, or a limit exceeded, is BLISSGPU_ERR_INVALID, checked before the device is touched.
 * n_pairs == 0 is BLISSGPU_OK.  Host pointers; runs on the default context. */
int blissgpu_fingerprint_match(const uint32_t *words, const uint64_t *word_offsets, uint32_t n_songs, const uint32_t *pairs,
                               uint64_t n_pairs, uint32_t max_offset, uint32_t min_overlap, int32_t *offset, uint32_t *errors,
                               uint32_t *bits);

/* ---- loudness: EBU R 128 / ReplayGain 2.0 track and album loudness, loudness range, sample and true peak ----
 * What every program around a music library computes per file, measured on the device at the file's NATIVE rate and channel
 * count (ITU-R BS.1770-4, EBU Tech 3341 / 3342).  Opt-in: no analyze_* entry point computes it, no feature row holds it.
 *
 * Input.  blissgpu_decoded_song rows: F32, S16 or S32 interleaved, 8 000 .. 768 000 Hz, 1 or 2 channels, each of weight 1.0
 * (mono is ONE channel, the libebur128 / FFmpeg convention).  More than 2 channels, a rate outside the range or an unknown
 * format is BLISSGPU_ERR_INVALID, checked before the device is touched.  Samples widen to f64 exactly: S16 v / 32768.0, S32
 * (double)v / 2147483648.0 (not the f32 rounding of the analysis path), F32 as it is.  F32 samples must be finite: the results of a
 * song that holds a NaN or an infinity are undefined (no other song of the call is affected).
 *
 * K-weighting.  Two biquads whose coefficients are computed on the host in f64 by the bilinear form.  Stage 1: f0 =
 * 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, K = tan(pi f0 / fs), Vh = 10^(G/20), Vb =
 * Vh^0.4996667741545416, a0 = 1 + K/Q + K^2, b = [(Vh + Vb K/Q + K^2)/a0, 2 (K^2 - Vh)/a0, (Vh - Vb K/Q + K^2)/a0], a1 =
 * 2 (K^2 - 1)/a0, a2 = (1 - K/Q + K^2)/a0.  Stage 2: f0 = 38.13547087602444, Q = 0.5003270373238773, b = [1, -2, 1], the same
 * a1 and a2.  blissgpu_loudness_kweighting returns coef [10] = b0 b1 b2 a1 a2 of stage 1, then of stage 2 (device-free); the
 * TABLE is the contract, a libm may differ from another in the last bit.  At 48 000 Hz it is BS.1770-4's.
 * Per sample and stage, in f64, every operation rounded on its own, in exactly this association:
 *   y = b0 x + s1;   s1 = (b1 x - a1 y) + s2;   s2 = b2 x - a2 y;      stage 2 takes stage 1's y.
 *
 * Sub-blocks.  H = (rate + 5) / 10 samples (integer division: 100 ms), n_sub = frames / H (blissgpu_loudness_subblocks; 0 for a
 * rate out of range).  z[c][u] = the sum of y2^2 over the samples of sub-block u of channel c, sequential in sample order.  The
 * tail beyond n_sub H enters the peaks and no energy.  n_sub < 4: BLISSGPU_SONG_TOO_SHORT.
 *
 * Segments.  Segment g covers sub-blocks [g S, min((g + 1) S, n_sub)); its filter starts from ZERO state at sample
 * max(0, g S - W) H and runs sequentially to the segment's end; outputs before sample g S H are discarded.  The segments that
 * start at sample 0 are the sequential filter; for the others the high-pass poles (radius 0.995 at 48 kHz) have decayed by
 * e^-96 over W = 4 sub-blocks.  S and W are the constants below, the same for every input; because the segmentation is part of
 * the contract, the device's energies are defined to the bit. */
#define BLISSGPU_LOUDNESS_SEGMENT 8
#define BLISSGPU_LOUDNESS_WARMUP 4
/* Peaks.  The sample peak is max |x| over all samples and channels.  The true peak oversamples by F = 4 below 96 000 Hz, 2 below
 * 192 000 Hz, 1 from there on, with the 49-tap Hann-windowed sinc h[i] = sinc((i - 24) / F) 0.5 (1 - cos(2 pi i / 48)), i = 0 ..
 * 48 (blissgpu_true_peak_filter returns F and h, device-free; the table is the contract):
 *   u[k] = sum over i of h[i] xz[k - i + 24], over the taps of that phase (those whose xz is a sample) in ascending i, from 0.0,
 * products and sums in f64; xz is the zero-stuffed channel (xz[F n] = x[n]), zero outside the song.  True peak = max |u[k]| over
 * k < F frames and the channels.
 *
 * Blocks and gates (device-free).  H and the sums in f64:
 *   P[j]  = (sum over c ascending of (((z[c][j] + z[c][j+1]) + z[c][j+2]) + z[c][j+3])) / (double)(4 H),   j = 0 .. n_sub - 4
 *   ST[j] = (sum over c, then u = j .. j + 29, of z[c][u], one sequential sum) / (double)(30 H),           j = 0 .. n_sub - 30
 * (blissgpu_loudness_blocks: z is [channels][n_sub]; P has n_sub - 3 entries, ST n_sub - 29 or none; either may be NULL).
 * Integrated loudness (blissgpu_loudness_gate): of the blocks with P > ABS = 1.1724653045822981e-07 (-70 LUFS; the literal is the
 * contract) Gamma = (sequential sum / count) 0.1; power = sequential sum / count of the blocks with P > ABS and P > Gamma, in
 * ascending order; lufs = -0.691 + 10 log10(power).  No block above ABS: power = 0, lufs = -inf.
 * Loudness range (blissgpu_loudness_range): of the ST > ABS the gate is (sequential sum / count) 0.01; the ST above both, sorted
 * ascending, n of them: lo = sorted[(uint64)((n - 1) 0.10 + 0.5)], hi = sorted[(uint64)((n - 1) 0.95 + 0.5)], range_lu =
 * 10 log10(hi / lo); n = 0: range_lu = lo = hi = 0.
 * An album: the same gates over the concatenation of its OK songs' P (and ST) in song order -- blocks never span songs --, the
 * peaks are the maxima; an album without an OK song has power 0, lufs -inf, range and peaks 0.
 * power, lo, hi, the energies and the peaks are defined to the bit; lufs and range_lu pass through the host's log10.
 *
 * blissgpu_loudness_energies (host pointers, the default context; the device half and the tests' tap): z receives the energies
 * song after song, song s at zoff[s] = sum over the songs before it of channels n_sub, channel-major: z[zoff[s] + c n_sub + u];
 * sample_peak, true_peak and status are [n_songs].  A too-short song never reaches the device: its energies and peaks are 0.
 * blissgpu_loudness_batch: album is NULL or [n_songs] labels < n_albums; song_out is f64 [n_songs][5] = power, lufs, range_lu,
 * sample_peak, true_peak (NaN for a song that is too short); album_out f64 [n_albums][5] (NULL without labels).
 * The PCM is uploaded in its native format; a call whose PCM exceeds half the context's workspace limit (or 8 GiB) runs in
 * groups of consecutive songs, with the same results.  n_songs == 0 is BLISSGPU_OK. */
uint64_t blissgpu_loudness_subblocks(uint64_t frames, uint32_t sample_rate);
int blissgpu_loudness_kweighting(uint32_t sample_rate, double *coef); /* coef [10] */
int blissgpu_true_peak_filter(uint32_t sample_rate, uint32_t *factor, double *h); /* h [49] */
int blissgpu_loudness_blocks(const double *z, uint32_t channels, uint64_t n_sub, uint32_t sample_rate, double *P, double *ST);
int blissgpu_loudness_gate(const double *P, uint64_t n, double *power, double *lufs);
int blissgpu_loudness_range(const double *ST, uint64_t n, double *range_lu, double *lo, double *hi);
int blissgpu_loudness_energies(const blissgpu_decoded_song *songs, uint32_t n_songs, double *z, double *sample_peak,
                               double *true_peak, int32_t *status);
int blissgpu_loudness_batch(const blissgpu_decoded_song *songs, uint32_t n_songs, const uint32_t *album, uint32_t n_albums,
                            double *song_out, double *album_out, int32_t *status);

/* ---- extended isolation forest: the ForestOptions metric of src/playlist.rs:230-251 ----
 * The reference builds extended_isolation_forest::Forest<f32, 23> from the seed songs with the thread RNG and uses its score
 * as the "distance" of closest_to_songs (:247-250): seeds-like songs score low, outliers high.  Here the forest is a pure
 * function of (seed rows, options, 64-bit seed), after Hariri, Carrasco Kind, Brunner, "Extended Isolation Forest" (IEEE TKDE
 * 2019):
 *   psi   = min(sample_size, n_seeds) (src/playlist.rs:237-240); psi < 2 is BLISSGPU_ERR_INVALID (c(psi) = 0: the forest does
 *           not work for a single song).  limit = max_tree_depth (1 .. BLISSGPU_FOREST_MAX_DEPTH; 0 = None) or ceil(log2 psi).
 *   tree t: psi distinct seed rows.  A node with m samples at depth k is a leaf if m <= 1 or k == limit.  Otherwise: a normal
 *           with exactly extension_level + 1 non-zero standard-normal components (the d - extension_level - 1 dropped ones are
 *           drawn uniformly without replacement), an intercept point p uniform in the box of the node's samples,
 *           b = dot(normal, p); samples with dot(normal, x) < b go left, the others right.  A child may be empty.
 *   dot:    DEFINED arithmetic: s = +0.0f; for j ascending with normal[j] != 0: s = s + normal[j] * x[j], product and sum each
 *           rounded to f32.  Dropped components are skipped, not multiplied: a NaN or inf of x in a dimension the node does
 *           not use never reaches s.  A NaN s compares false and goes right.  Builder and kernel use the same test.
 *   leaf:   path length k + c(m), c(m) = 2 (ln(m - 1) + 0.5772156649) - 2 (m - 1) / m for m > 2, c(2) = 1, c(0) = c(1) = 0,
 *           computed in f64 and stored as leaf_q = round(value * 2^24) in a u32.
 *   score:  path_sum = the u64 sum of leaf_q over the trees (order-free, hence exact on the device);
 *           score = (float)exp2(-(path_sum / 2^24 / n_trees) / c(psi)), evaluated in f64.  Always finite: no BLISSGPU_ERR_NAN here.
 *   draws:  draw i of tree t = word (i & 3) of Philox4x32-10(counter = (i / 4 low, i / 4 high, t, 0x45494630), key = (seed low,
 *           seed high)); the forest does not depend on how many threads build it.
 * Limits: 1 <= d <= BLISSGPU_FOREST_MAX_D, 1 <= n_trees <= BLISSGPU_FOREST_MAX_TREES, 0 <= extension_level <= d - 1, psi is capped
 * at BLISSGPU_FOREST_MAX_PSI, fewer than 2^32 - 1 nodes in all, finite seed rows; anything else is BLISSGPU_ERR_INVALID.
 * The forest handle is opaque (void *).  build / info / export / destroy are host-only and work without a GPU. */
#define BLISSGPU_FOREST_MAX_D 32u
#define BLISSGPU_FOREST_MAX_TREES 1048576u
#define BLISSGPU_FOREST_MAX_PSI 65536u
#define BLISSGPU_FOREST_MAX_DEPTH 128u
int blissgpu_forest_build(const float *seeds, uint64_t n_seeds, uint32_t d, uint32_t n_trees, uint32_t sample_size,
                          uint32_t max_tree_depth, uint32_t extension_level, uint64_t seed, void **forest);
int blissgpu_forest_destroy(void *forest); /* also frees the device copies; NULL is fine */
/* Any pointer may be NULL. */
int blissgpu_forest_info(const void *forest, uint32_t *d, uint32_t *n_trees, uint32_t *psi, uint32_t *depth_limit,
                         uint32_t *extension_level, uint64_t *n_nodes);
/* The forest in its canonical dense form (any pointer may be NULL).  With T = n_trees, N = n_nodes:
 *   sample_idx[T * psi]  the seed rows tree t was grown from, sample_idx[t * psi .. (t + 1) * psi)
 *   tree_first[T + 1]    tree t owns the nodes tree_first[t] .. tree_first[t + 1), its root first
 *   normal[N * d]        the node's normal, zeros where dropped (all zero on a leaf)
 *   b[N]                 the node's threshold (0 on a leaf)
 *   left[N], right[N]    node indices of the children, 0xFFFFFFFF on a leaf
 *   leaf_size[N]         samples of the tree that ended in the leaf (0 on an inner node)
 *   leaf_q[N]            the leaf's u32 path length (0 on an inner node) */
int blissgpu_forest_export(const void *forest, uint32_t *sample_idx, uint64_t *tree_first, float *normal, float *b,
                           uint32_t *left, uint32_t *right, uint32_t *leaf_size, uint32_t *leaf_q);
/* score[j] and (path_sum may be NULL) path_sum[j] of the n candidates, rows of d floats, d the forest's.  n == 0 is BLISSGPU_OK;
 * n <= 0xFFFFFF00.  The device copy of the forest is uploaded once per (forest, device) and freed with the forest. */
int blissgpu_forest_score(void *forest, const float *cand, uint64_t n, float *score, uint64_t *path_sum);
/* closest_to_songs with the forest as the metric (src/playlist.rs:256-270): order[k] = the candidate with the k-th lowest score
 * (stable: equal scores keep the candidates' order); score (may be NULL) receives the scores in candidate order. */
int blissgpu_forest_closest_to_songs(void *forest, const float *cand, uint64_t n, uint32_t *order, float *score);
/* Device-resident forms (device pointers); asynchronous on the context's stream but for the first upload of the forest. */
int blissgpu_forest_score_device(blissgpu_ctx *ctx, void *forest, const float *d_cand, uint64_t n, float *d_score,
                                 uint64_t *d_path_sum);
int blissgpu_forest_closest_to_songs_device(blissgpu_ctx *ctx, void *forest, const float *d_cand, uint64_t n,
                                            uint32_t *d_order, float *d_score);

/* ---- one forest per seed GROUP: an isolation-forest playlist for every album in one call ----
 * blissgpu_group_knn with the forest as the metric: seeds, group_offsets (a HOST pointer in every form) and skip are
 * blissgpu_group_knn's.
 * Forest of group g: exactly blissgpu_forest_build(the seed rows of group g, the options, seed).  Every group uses the same
 *   options and the same 64-bit seed; only the seed rows differ.  What is per forest stays per group: psi_g = min(sample_size,
 *   count_g), the depth limit (ceil(log2 psi_g) when max_tree_depth == 0) and c(psi_g).
 * Rows: row g of idx / score ([n_groups][k], score may be NULL) holds the first k entries of the stable ascending order of
 *   blissgpu_forest_score over the group's eligible candidates: equal scores in candidate order, rows with fewer than k eligible
 *   candidates end in idx 0xFFFFFFFF / score +inf.  A score is bit for bit what blissgpu_forest_score writes for that forest and
 *   candidate (the same u64 path sum, the same f64 expression).
 * skip: NULL, or one candidate index per SEED ROW: that candidate is left out of the seed's group; 0xFFFFFFFF skips nothing, any
 *   other value >= n is BLISSGPU_ERR_INVALID.
 * psi_g < 2 ("the forest does not work for a single song"): the group gets BLISSGPU_GROUP_TOO_FEW_SEEDS in group_status
 *   ([n_groups], may be NULL; every other group BLISSGPU_GROUP_OK) and a row of padding.  That is not an error of the call;
 *   sample_size < 2 makes every group such a group.
 * Scores are always finite: there is no BLISSGPU_ERR_NAN.  1 <= k <= BLISSGPU_KNN_MAX_K, 1 <= d <= BLISSGPU_FOREST_MAX_D,
 *   extension_level <= d - 1, the BLISSGPU_FOREST_* limits hold per group, n < 2^32 - 1, fewer than 2^32 seeds and 2^32 - 1
 *   groups; n_groups == 0 or n == 0 is BLISSGPU_OK (n == 0: every row is padding, no forest is built, and the host form does
 *   not touch the device).  Non-finite seed rows are
 *   BLISSGPU_ERR_INVALID.  All arguments, skip and finiteness included, are checked before the device is touched and before any
 *   forest is built.
 * Memory and launches: no n_groups x n and no group x n array is ever stored -- the candidates' path sums live in registers and
 *   the workspace holds partial lists of k keys.  The forests need not fit on the device at once: consecutive groups form a
 *   batch while their planned nodes, n_trees x (2 psi_g - 1) per group (1 for a group without a forest), stay within the node
 *   budget (BLISSGPU_OPT_FOREST_GROUP_NODES); a single group beyond the budget is a batch of its own.  (The plan counts a tree
 *   without empty children; the rare split that leaves a child empty adds nodes, and the image buffers are sized from the built
 *   forests.)  Per batch: the forests are built on up to 16 host threads dealt out over groups, packed into ONE image, uploaded
 *   once, and scored by two launches (scan + merge) whatever the group sizes; batch b + 1 is built while the device scores
 *   batch b.  The result does not depend on the batch split, the thread count or the device. */
int blissgpu_group_forest_knn(const float *seeds, const uint64_t *group_offsets, uint64_t n_groups, const float *cand, uint64_t n,
                              uint32_t d, uint32_t n_trees, uint32_t sample_size, uint32_t max_tree_depth,
                              uint32_t extension_level, uint64_t seed, const uint32_t *skip, uint32_t k, uint32_t *idx,
                              float *score, int32_t *group_status);
/* Device-resident form: d_cand, d_skip, d_idx, d_score, d_group_status are device pointers.  The forests are built on the host,
 * so the seed rows are needed THERE: h_seeds is a host copy of them (then d_seeds is not looked at and may be NULL); with
 * h_seeds == NULL the call makes the one device-to-host copy of d_seeds itself, and their finiteness is checked after that copy.
 * A skip entry >= n is found by the kernel, so it is reported after the kernels have run, and only the rows the kernel reads
 * are looked at: those of the groups that have a forest, and none when n == 0.  Synchronises the context's stream before it returns (the host
 * builds forests while the device works). */
int blissgpu_group_forest_knn_device(blissgpu_ctx *ctx, const float *d_seeds, const float *h_seeds,
                                     const uint64_t *group_offsets, uint64_t n_groups, const float *d_cand, uint64_t n,
                                     uint32_t d, uint32_t n_trees, uint32_t sample_size, uint32_t max_tree_depth,
                                     uint32_t extension_level, uint64_t seed, const uint32_t *d_skip, uint32_t k,
                                     uint32_t *d_idx, float *d_score, int32_t *d_group_status);
/* The batches of the two entry points above for a node budget (0: that of the default 64 MiB image): device-free.  Batch i is
 * the groups batch_first[i] .. batch_first[i + 1] (n_batches + 1 entries: consecutive, every group once).  *n_batches is always
 * written; nothing is written past max_batches entries. */
int blissgpu_group_forest_plan(const uint64_t *group_offsets, uint64_t n_groups, uint32_t d, uint32_t n_trees,
                               uint32_t sample_size, uint32_t max_tree_depth, uint32_t extension_level, uint64_t node_budget,
                               uint64_t *batch_first, uint64_t max_batches, uint64_t *n_batches);
/* The last blissgpu_group_forest_knn call on this context (measurement): host milliseconds spent building and packing forests,
 * host milliseconds spent waiting for the device, and the number of batches.  Any pointer may be NULL. */
int blissgpu_debug_group_forest_stats(blissgpu_ctx *ctx, double *build_ms, double *wait_ms, uint64_t *n_batches);
/* The last blissgpu_kmeans_device call on this context: the device-to-host copies made inside its loop (one per assignment: the
 * pair of flag words) and their bytes.  Either pointer may be NULL. */
int blissgpu_debug_kmeans_stats(blissgpu_ctx *ctx, uint64_t *loop_copies, uint64_t *loop_bytes);
/* The last blissgpu_learn_metric_device call on this context: the uploads (M, one per step) and downloads (the result block,
 * one per step) made inside its loop, and the bytes downloaded.  Any pointer may be NULL. */
int blissgpu_debug_metric_stats(blissgpu_ctx *ctx, uint64_t *loop_uploads, uint64_t *loop_downloads, uint64_t *loop_bytes);

/* FeaturesVersion::feature_weights (src/lib.rs:168-173, 209-234): d x d row-major diagonal matrix. */
int blissgpu_feature_weights(uint32_t features_version, float *M);

/* ---- one process, every GPU of the node ----
 * Songs are independent (Decoder::analyze_paths treats them so, src/song/decoder.rs:299-329), so a library shards by song:
 * greedy longest-first balance of the samples per device, no data-path collective.  After the local batches ONE RCCL
 * all-gather over xGMI (padded to the largest shard) leaves the full n x d feature matrix on every device; the pairwise
 * kernel is then row-block sharded with no further exchange.  RCCL is loaded at run time; without it node creation
 * fails with BLISSGPU_ERR_RCCL.  (bliss_rs_amd/shard.py is the one-process-per-GPU form of the same plan on
 * torch.distributed.) */
typedef struct blissgpu_node blissgpu_node;
/* The plan, device-free (no HIP call, no context): rank_of_song[i] = rank in [0, world) that analyses song i.  Greedy
 * longest-first assignment balancing the samples per rank, ties -> fewest songs -> lowest rank; deterministic, so every
 * host and every process computes the same plan (bliss_rs_amd.shard.shard_songs is the same function). */
int blissgpu_shard_plan(const uint64_t *lengths, uint32_t n_songs, uint32_t world, uint32_t *rank_of_song);
/* Rows [lo, hi) of an n_rows-row distance matrix computed by `rank` of `world` (device-free; rank >= world: empty). */
void blissgpu_row_block(uint64_t n_rows, uint32_t world, uint32_t rank, uint64_t *lo, uint64_t *hi);
/* devices: HIP ordinals (NULL = 0 .. n_devices-1).  Creates one context per rank and the RCCL communicators
 * (ncclCommInitAll).  A list that names an ordinal more than once creates LOOPBACK ranks -- several contexts sharing a
 * GPU: RCCL cannot (and need not) connect them, the gather is done with device-to-device copies; everything else is
 * the same code.  That is how the N > 1 plan / padding / scatter / row-block paths are tested on a one-GPU box. */
int blissgpu_node_create(int n_devices, const int *devices, blissgpu_node **node);
int blissgpu_node_destroy(blissgpu_node *node);
int blissgpu_node_device_count(blissgpu_node *node);
blissgpu_ctx *blissgpu_node_ctx(blissgpu_node *node, int rank); /* the rank's context (device forms, synth, malloc) */
/* The sharding plan: rank_of_song[i] = device rank that analyses song i. */
int blissgpu_node_shard(blissgpu_node *node, const uint64_t *lengths, uint32_t n_songs, uint32_t *rank_of_song);
/* Rows [lo, hi) of an n_rows-row distance matrix computed by `rank`. */
void blissgpu_node_row_block(blissgpu_node *node, uint64_t n_rows, int rank, uint64_t *lo, uint64_t *hi);
/* Bulk analysis of host PCM (the node form of blissgpu_analyze_batch): shards, feeds every device from its own host
 * thread, gathers.  out (host, n_songs x feature_count) and status as in blissgpu_analyze_batch. */
int blissgpu_node_analyze(blissgpu_node *node, const float *pcm, const uint64_t *offsets, const uint64_t *lengths,
                          uint32_t n_songs, uint32_t features_version, float *out, int32_t *status);
/* Device-resident form: song i lives on device rank_of_song[i] at d_pcm[rank_of_song[i]] + offsets[i].  Asynchronous. */
int blissgpu_node_analyze_device(blissgpu_node *node, const float *const *d_pcm, const uint64_t *offsets,
                                 const uint64_t *lengths, const uint32_t *rank_of_song, uint32_t n_songs,
                                 uint32_t features_version);
/* The gathered n_songs x feature_count matrix of the last analysis on `rank`'s device (valid after synchronize). */
const float *blissgpu_node_features(blissgpu_node *node, int rank);
/* All-pairs distances over the gathered matrix, rows sharded across the devices; out is host memory, n x n. */
int blissgpu_node_pairwise(blissgpu_node *node, int metric, const float *M, float *out);
int blissgpu_node_synchronize(blissgpu_node *node);

/* ---- device memory helpers for hosts without their own HIP binding (Rust/C callers) ---- */
int blissgpu_malloc(void **d_ptr, uint64_t bytes);
int blissgpu_free(void *d_ptr);
int blissgpu_memcpy_h2d(blissgpu_ctx *ctx, void *d_dst, const void *h_src, uint64_t bytes);
int blissgpu_memcpy_d2h(blissgpu_ctx *ctx, void *h_dst, const void *d_src, uint64_t bytes);
/* Page-locked host memory for decoder output: H2D copies from it run at full PCIe rate without HIP's staging copy. */
int blissgpu_host_alloc(void **h_ptr, uint64_t bytes);
int blissgpu_host_free(void *h_ptr);

/* ---- benchmark input: synthetic white noise written straight into HBM.  Song i of the call gets
 * uniform [-0.5, 0.5) samples from Philox4x32-10 with key (0x5EED0000 + first_song_index + i, 0) and
 * counter = sample_index / 4 (bit-identical to the oracle's generator).  No reference counterpart. */
int blissgpu_synth_white_noise_device(blissgpu_ctx *ctx, float *d_pcm, const uint64_t *offsets,
                                      const uint64_t *lengths, uint32_t n_songs, uint32_t first_song_index);
/* Same with an explicit generator index per song (a rank's scattered share of a sharded corpus). */
int blissgpu_synth_white_noise_indexed_device(blissgpu_ctx *ctx, float *d_pcm, const uint64_t *offsets,
                                              const uint64_t *lengths, const uint32_t *song_index, uint32_t n_songs);

/* ---- per-kernel timing with HIP events on the context's stream (for bench.py's roofline) ---- */
int blissgpu_profile_enable(blissgpu_ctx *ctx, int enable);
int blissgpu_profile_reset(blissgpu_ctx *ctx);
int blissgpu_profile_kernel_count(void);
const char *blissgpu_profile_kernel_name(int kernel);
/* total_ms / launches accumulated since the last reset (synchronises the stream) */
int blissgpu_profile_get(blissgpu_ctx *ctx, int kernel, double *total_ms, uint64_t *launches);

/* ---- debug taps used by the parity tests: per-song tuning estimate of the last batch ----
 * tuning[i] = estimate_tuning's value for song i of the last analyze_batch_device call on ctx
 * (src/chroma.rs:361-391); n_bpms[i] = number of beats BPMDesc recorded (src/temporal.rs:50-58). */
int blissgpu_debug_last_tuning(blissgpu_ctx *ctx, double *tuning, uint32_t *n_bpms, uint32_t n_songs);

/* Number of chunks the last blissgpu_analyze_batch_device call on ctx was cut into. */
uint64_t blissgpu_debug_last_chunks(blissgpu_ctx *ctx);

/* Intermediate series of song `song` (the caller's index into the last batch; it must belong to the LAST chunk run
 * on ctx) for the per-stage parity tests.  Copies at most max_elems elements (4 bytes; 8 for the f64 taps) to dst,
 * reports the available count in *n_elems. */
#define BLISSGPU_DEBUG_CENTROID 0      /* f32[n_t]  per-frame spectral centroid in Hz (src/timbral.rs:159-173) */
#define BLISSGPU_DEBUG_ROLLOFF 1       /* f32[n_t]  per-frame rolloff in Hz (:175-194) */
#define BLISSGPU_DEBUG_FLATNESS 2      /* f32[n_t]  per-frame flatness (:196-208) */
#define BLISSGPU_DEBUG_FLUX 3          /* f32[n_b]  SpecFlux onset values (src/aubio.rs:455-467) */
#define BLISSGPU_DEBUG_THRESHOLDED 4   /* f32[n_b]  PeakPicker thresholded values (:757) */
#define BLISSGPU_DEBUG_RUN_BPM 5       /* f32[runs] BeatTracking::get_bpm after each run (:1231-1239) */
#define BLISSGPU_DEBUG_RUN_COUNT 6     /* u32[runs] beats BPMDesc recorded while that bpm was current */
#define BLISSGPU_DEBUG_SPECTROGRAM 7   /* f32[n_c][4128] STFT magnitudes, 4097 valid per row (src/utils.rs:26-64) */
#define BLISSGPU_DEBUG_ENERGY256 8     /* f32[ceil(n/256)] sum of squares per 256 samples */
#define BLISSGPU_DEBUG_CROSSINGS256 9  /* u32[ceil(n/256)] zero crossings per 256 samples */
#define BLISSGPU_DEBUG_PITCH_HIST 10   /* u32[100] pitch-residue histogram (peaks above the median's coarse bin) */
/* f64 taps (elements are 8 bytes).  CHROMA and INTERVAL need BLISSGPU_OPT_DEBUG_CHROMA = 1 before the analysis. */
#define BLISSGPU_DEBUG_CHROMA 11       /* f64[n_c][12] chroma_stft's matrix, frame-major, after the column normalisation
                                          (src/chroma.rs:393-412; the reference holds it against data/chroma.npy, :621-639) */
#define BLISSGPU_DEBUG_INTERVAL 12     /* f64[10] chroma_interval_features' time means (src/chroma.rs:137-155) */
#define BLISSGPU_DEBUG_FILTER_BANK 13  /* f64[12][4128] chroma_filter(22050, 8192, 12, tuning) (src/chroma.rs:197-267), 4097
                                          valid per row; `song` is the TUNING SLOT: 0..99 = tuning -0.5 + 0.01 slot, 100 = 0.0 */
int blissgpu_debug_fetch(blissgpu_ctx *ctx, int what, uint32_t song, void *dst, uint64_t max_elems, uint64_t *n_elems);

const char *blissgpu_strerror(int code);
const char *blissgpu_last_error(void); /* thread-local detail of the last failure */
const char *blissgpu_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BLISSGPU_H */
