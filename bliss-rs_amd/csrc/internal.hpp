// internal.hpp -- shared declarations of the MI355X analysis library (not part of the C ABI).
//
// Vocabulary follows the reference (bliss-rs): songs, frames, descriptors, features.
//   timbral frames : PVoc windows, W=512 hop=128   (src/timbral.rs:40-41, src/aubio.rs:182-264)
//   tempo frames   : PVocTempo windows, W=512 hop=256 (src/temporal.rs:40-41, src/aubio.rs:338-425)
//   chroma frames  : STFT windows, W=8192 hop=2205 (src/chroma.rs:39,74, src/utils.rs:26-64)
//   loudness chunks: 1024 samples                  (src/misc.rs:44)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace bg {

constexpr uint32_t SAMPLE_RATE = 22050;   // src/lib.rs:140
constexpr int W512 = 512;                 // SpectralDesc::WINDOW_SIZE / BPMDesc::WINDOW_SIZE
constexpr int HOP_T = 128;                // SpectralDesc::HOP_SIZE
constexpr int HOP_B = 256;                // BPMDesc::HOP_SIZE
constexpr int W8192 = 8192;               // ChromaDesc::WINDOW_SIZE
constexpr int HOP_C = 2205;               // src/chroma.rs:74
constexpr int CBINS = W8192 / 2 + 1;      // 4097
constexpr int CBINS_PAD = 4128;           // row pitch of the stored spectrogram: 129 lines of 128 bytes, so every row starts on a line
constexpr int BANK_PITCH = CBINS_PAD;     // row pitch of the filter bank (zero beyond bin 4096)
constexpr int BANK_ROWS = 12;             // chroma classes
constexpr int LOUD_W = 1024;              // LoudnessDesc::WINDOW_SIZE
constexpr int MIN_SAMPLES = 8192;         // src/song/mod.rs:417-430
constexpr int N_TUNING = 100;             // pitch_tuning histogram bins at resolution 0.01
constexpr int PIP_LO = 57, PIP_HI = 1483; // centre bins visited by pip_track at n_fft=8192 (chroma.rs:302-313)
constexpr int PIP_MAX_PER_FRAME = 714;    // peaks cannot be adjacent: ceil(1427/2)
constexpr int CAND_BUDGET_PER_FRAME = 48; // tuning-candidate pool of a chunk: slots per chroma frame (white noise needs ~8; see tune_select_kernel)
// Coarse magnitude histogram of the tuning estimate: bin = f32 bit pattern >> COARSE_SHIFT, i.e. 2^(23 - COARSE_SHIFT) bins
// per octave.  64 per octave: the peaks that share the median's bins -- the candidates tune_pass2_kernel must evaluate in
// f64 from the spectrogram -- are half as many as with 32 (2.2 % of all peaks), and 14 bits are what a 32-bit peak record
// has left beside the centre bin and the pitch bin.
#ifndef COARSE_SHIFT
#define COARSE_SHIFT 17
#endif
constexpr uint32_t COARSE_LOW_MASK = (1u << COARSE_SHIFT) - 1u;
constexpr int H1_BINS = 1 << (31 - COARSE_SHIFT);   // every positive f32 has a bin
constexpr int BT_WINLEN = 512, BT_STEP = 128, BT_LAGLEN = 128;  // src/aubio.rs:1337-1341, 920-922
constexpr int BT_PRE_STRIDE = 264;  // floats per beat-tracker run written by beat_acf_kernel (kernels_tempo.hip)
constexpr int F512_TILE = 512;            // FFT-512 frames per workgroup (16 lane-groups x 32 consecutive frames + 1 halo frame each)
constexpr int CH_TILE = 64;               // chroma frames per workgroup in the contraction kernel
constexpr int STFT_TILE = 16;             // chroma frames per workgroup in the STFT kernel

// Per-song descriptor, built on the host, read by every kernel.
struct SongDesc {
    uint64_t pcm_off;   // first sample of the song in the batch PCM buffer
    uint64_t n;         // samples
    uint64_t t_off;     // first timbral frame in the batch-wide series arrays
    uint64_t b_off;     // first tempo frame
    uint64_t c_off;     // first chroma frame
    uint64_t e_off;     // first 256-sample energy block
    uint32_t n_t;       // timbral frames   floor((n-512)/128)+1
    uint32_t n_b;       // tempo frames     floor((n-512)/256)+1
    uint32_t n_f;       // FFT-512 frames actually computed = max(n_t, 2*n_b)
    uint32_t n_c;       // chroma frames    ceil_f32(n/2205); frames past the last window (f * 2205 > n) are zero rows
    uint32_t n_e;       // 256-sample blocks ceil(n/256)
    uint32_t n_l;       // loudness chunks  ceil(n/1024)
    uint32_t row;       // output row
    uint32_t ok;        // 1 = analyse, 0 = too short (status already set by the host)
};

// Frames whose rolloff bin the FFT-512 kernel could not prove (see its epilogue) are handed to rolloff_fix_kernel: the
// frame's 256 magnitudes at the entry of its own index, and ROLLOFF_UNPROVEN (no rolloff is negative) in its place of the
// rolloff series, where the exact pass finds it.  The record lives in device memory (filled by the host per chunk); the
// entries borrow the memory of the spectrogram and the peak records, dead until the FFT-8192 kernel starts -- room for every
// frame of the chunk.
struct RollFix {
    float* mags;        // [cap][256]: entry t = the magnitudes of the chunk's timbral frame t (written for unproven frames only)
    uint32_t cap;       // = the chunk's timbral frames
};
constexpr float ROLLOFF_UNPROVEN = -1.0f;

// Per-song scalars produced by the tuning stage.
struct TuningState {
    uint32_t n_peaks;      // total pip_track peaks
    uint32_t b_lo, b_hi;   // coarse bins holding the two middle order statistics
    uint32_t below;        // peaks in coarse bins < b_lo
    uint32_t n_cand;       // candidates appended so far
    int32_t tuning_idx;    // argmax bin (first max); tuning = -0.5 + 0.01*idx ; -1 => tuning 0.0 (no peaks)
    uint32_t cand_off;     // first slot of the song's candidates in the chunk's pool
    uint32_t cand_cap;     // slots granted = peaks inside [b_lo, b_hi]; 0 => the pool was exhausted: tune_final re-scans the records
};

// Beat-tracker result per song
struct TempoState {
    float tempo;        // normalised feature
    uint32_t n_bpms;
};

struct DeviceTables {   // constant tables, built once per context
    const float2* tw8192;     // exp(-2*pi*i*k/8192), k < 8192
    const float2* tw512;      // exp(-2*pi*i*k/512),  k < 512
    const float* hann8192;    // periodic Hann, src/utils.rs:37-39
    const float* hannz512;    // hanningz, src/aubio.rs:151-154
    const double* chroma_bank;// [N_TUNING+1][BANK_ROWS][BANK_PITCH] chroma filters (zero padded); slot N_TUNING = tuning 0.0
    const float* bt_rwv;      // [128] Rayleigh weighting, src/aubio.rs:925-930
    const float* bt_dfwv;     // [512] detection-function weighting, src/aubio.rs:933-936
};

// The profiling table: one entry per kernel, X(id, name).  enum KernelId, K_COUNT and the names blissgpu_profile_kernel_name
// returns are all generated from this list, so a new kernel is one new line.  The ids are positions in the list: a new entry
// goes in front of the last two (tests/test_journeys_host.py holds the table to end in them; tests/test_chains_host.py pins
// the first 29 names by value), and every consumer of the table goes by name
#define BLISSGPU_KERNEL_TABLE(X)                                                                                                  \
    X(K_FFT512, "fft512_kernel")                                                                                                  \
    X(K_ONSET, "onset_kernel")                                                                                                    \
    X(K_BEAT, "beat_kernel")                                                                                                      \
    X(K_STFT8192, "stft8192_kernel")                                                                                              \
    X(K_TUNE_SELECT, "tune_select_kernel")                                                                                        \
    X(K_TUNE_PASS2, "tune_pass2_kernel")                                                                                          \
    X(K_TUNE_FINAL, "tune_final_kernel")                                                                                          \
    X(K_CHROMA, "chroma_kernel")                                                                                                  \
    X(K_SUMMARY, "summary_kernel")                                                                                                \
    X(K_FINALIZE, "assemble_kernel")                                                                                              \
    X(K_PAIRWISE, "pairwise_kernel")                                                                                              \
    X(K_SET_DISTANCE, "set_distance_kernel")                                                                                      \
    X(K_SONG_TO_SONG, "song_to_song_kernel")                                                                                      \
    X(K_SYNTH, "synth_kernel")                                                                                                    \
    X(K_ROLLFIX, "rolloff_fix_kernel")                                                                                            \
    /* playlist deduplication: never launched by the analysis path */                                                             \
    X(K_DEDUP_NEXT, "dedup_next_kernel")                                                                                          \
    X(K_DEDUP_WALK, "dedup_walk_kernel")                                                                                          \
    /* k-nearest search (kernels_knn.hip) */                                                                                      \
    X(K_KNN_SCAN, "knn_scan_kernel")                                                                                              \
    X(K_KNN_MERGE, "knn_merge_kernel")                                                                                            \
    /* isolation-forest scores (kernels_forest.hip) */                                                                            \
    X(K_FOREST_WALK, "forest_walk_kernel")                                                                                        \
    X(K_FOREST_FINISH, "forest_finish_kernel")                                                                                    \
    /* duplicate groups of a collection (kernels_duplicates.hip) */                                                               \
    X(K_DUP_INIT, "dup_init_kernel")                                                                                              \
    X(K_DUP_JOIN, "dup_join_kernel")                                                                                              \
    X(K_DUP_FLATTEN, "dup_flatten_kernel")                                                                                        \
    /* k-nearest search per seed group, the variance-based weights of every seed group (kernels_group_knn.hip) */                 \
    X(K_GROUP_KNN_SCAN, "group_knn_scan_kernel")                                                                                  \
    X(K_GROUP_KNN_MERGE, "group_knn_merge_kernel")                                                                                \
    X(K_GROUP_WEIGHTS, "group_weights_kernel")                                                                                    \
    /* song-to-song chains cut after k (kernels_chains.hip) */                                                                    \
    X(K_CHAIN_STEP, "chain_step_kernel")                                                                                          \
    X(K_CHAIN_WALK, "chain_walk_kernel")                                                                                          \
    /* k-nearest albums per seed group (kernels_albums.hip; its partial lists are merged by knn_merge_kernel) */                  \
    X(KX_SEGMENT_MEAN, "segment_mean_kernel")                                                                                     \
    X(KX_ALBUM_KNN_SCAN, "album_knn_scan_kernel")                                                                                 \
    /* k-means (kernels_kmeans.hip): the nearest centre of every song, the counting sort of the labels, the select */             \
    X(KX_KMEANS_ASSIGN, "kmeans_assign_kernel")                                                                                   \
    X(KX_KMEANS_HIST, "kmeans_hist_kernel")                                                                                       \
    X(KX_KMEANS_SCAN_TILES, "kmeans_scan_tiles_kernel")                                                                           \
    X(KX_KMEANS_SCAN_ADD, "kmeans_scan_add_kernel")                                                                               \
    X(KX_KMEANS_SCATTER, "kmeans_scatter_kernel")                                                                                 \
    X(KX_KMEANS_SELECT, "kmeans_select_kernel")                                                                                   \
    /* one gradient evaluation of triplet metric learning (kernels_metric.hip): the wavefronts' partials, their ascending sum */  \
    X(KX_TRIPLET_STEP, "triplet_step_kernel")                                                                                     \
    X(KX_TRIPLET_REDUCE, "triplet_reduce_kernel")                                                                                 \
    /* the silhouette (kernels_silhouette.hip): the all-pairs sums per (song, cluster), then a, b, neighbour and s */             \
    X(KX_SILHOUETTE_SCAN, "silhouette_scan_kernel")                                                                               \
    X(KX_SILHOUETTE_FINISH, "silhouette_finish_kernel")                                                                           \
    /* the moments (kernels_moments.hip): the levels' offsets, level 0 of the means, of the squared deviations and of the */      \
    /* scatter matrix, every further level of the blocked sum, the extrema */                                                     \
    X(KX_MOMENTS_PLAN, "moments_plan_kernel")                                                                                     \
    X(KX_MOMENTS_SUM, "moments_sum_kernel")                                                                                       \
    X(KX_MOMENTS_M2, "moments_m2_kernel")                                                                                         \
    X(KX_MOMENTS_SCATTER, "moments_scatter_kernel")                                                                               \
    X(KX_MOMENTS_REDUCE, "moments_reduce_kernel")                                                                                 \
    X(KX_MOMENTS_FINISH, "moments_finish_kernel")                                                                                 \
    /* group-to-group set distances (kernels_chamfer.hip): the minima per (song, group), their blocked sums, the selection */     \
    X(KX_CHAMFER_SCAN, "chamfer_scan_kernel")                                                                                     \
    X(KX_CHAMFER_REDUCE, "chamfer_reduce_kernel")                                                                                 \
    X(KX_CHAMFER_SELECT, "chamfer_select_kernel")                                                                                 \
    /* the minimum spanning tree (kernels_mst.hip): every song's smallest edge out of its component, every component's */         \
    X(KX_MST_SCAN, "mst_scan_kernel")                                                                                             \
    X(KX_MST_PICK, "mst_pick_kernel")                                                                                             \
    /* locally scaled k-nearest search and the k-occurrence counts (kernels_scaled_knn.hip; merged by knn_merge_kernel) */        \
    X(KX_SCALED_KNN_SCAN, "scaled_knn_scan_kernel")                                                                               \
    X(KX_KNN_OCCURRENCE, "knn_occurrence_kernel")                                                                                 \
    /* radio playlists (kernels_radio.hip): the banned labels of every (radio, rule), then the step under them */                 \
    X(KX_RADIO_BAN, "radio_ban_kernel")                                                                                           \
    X(KX_RADIO_STEP, "radio_step_kernel")                                                                                         \
    /* the 2-D map (kernels_map.hip): the all-pairs repulsion, the attraction along the CSR rows, the gradient and update */      \
    X(KX_MAP_REPULSE, "map_repulse_kernel")                                                                                       \
    X(KX_MAP_ATTRACT, "map_attract_kernel")                                                                                       \
    X(KX_MAP_UPDATE, "map_update_kernel")                                                                                         \
    /* Ward clustering (kernels_ward.hip): every cluster's nearest other cluster under Ward's cost, the join */                   \
    X(KX_WARD_SCAN, "ward_scan_kernel")                                                                                           \
    X(KX_WARD_JOIN, "ward_join_kernel")                                                                                           \
    /* k-medoids (kernels_pam.hip): the all-pairs swap scan, its fold per candidate, the round's winner, the state's helpers */   \
    X(KX_PAM_SCAN, "pam_scan_kernel")                                                                                             \
    X(KX_PAM_FOLD, "pam_fold_kernel")                                                                                             \
    X(KX_PAM_PICK, "pam_pick_kernel")                                                                                             \
    X(KX_PAM_GATHER, "pam_gather_kernel")                                                                                         \
    X(KX_PAM_STATE, "pam_state_kernel")                                                                                           \
    X(KX_PAM_TD, "pam_td_kernel")                                                                                                 \
    /* acoustic fingerprints (kernels_fingerprint.hip): the frames' band energies, the words, the match per offset block, pick */ \
    X(KX_FP_BANDS, "fp_bands_kernel")                                                                                             \
    X(KX_FP_BITS, "fp_bits_kernel")                                                                                               \
    X(KX_FP_MATCH, "fp_match_kernel")                                                                                             \
    X(KX_FP_PICK, "fp_pick_kernel")                                                                                               \
    /* loudness (kernels_loudness.hip): the K-weighted sub-block energies, the peaks per tile, their fold per song */              \
    X(KX_LOUD_ENERGY, "loud_energy_kernel")                                                                                       \
    X(KX_LOUD_PEAK, "loud_peak_kernel")                                                                                           \
    X(KX_LOUD_FOLD, "loud_fold_kernel")                                                                                           \
    /* the k lowest forest scores per seed group (kernels_forest.hip; merged by group_knn_merge_kernel) */                        \
    X(KX_GROUP_FOREST_SCAN, "group_forest_scan_kernel")                                                                           \
    /* a journey's step (kernels_chains.hip: the chains' scan with a waypoint query or a gate) */                                 \
    X(KX_JOURNEY_STEP, "journey_step_kernel")
enum KernelId : int {
#define X(id, name) id,
    BLISSGPU_KERNEL_TABLE(X)
#undef X
    K_COUNT
};

// lower_bound on a prefix array: largest s with prefix[s] <= x  (prefix has n+1 entries, prefix[0]=0)
__device__ __forceinline__ uint32_t find_segment(const uint32_t* __restrict__ prefix, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (prefix[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- launchers (one per .hip file) ----
struct Workspace {
    // timbral series [total_t]
    float *centroid, *rolloff, *flatness;
    // tempo [total_b]
    float *flux, *thresholded;
    // 256-sample energy blocks [total_e], zero-crossings per block
    float* e256;
    uint32_t* zc256;
    // chroma
    float* spec;            // [total_c][CBINS_PAD] magnitudes (f32, exactly what the reference widens to f64)
    float* frame_max;       // [total_c]
    uint32_t* h1;           // [n_songs][H1_BINS]
    uint32_t* hist100;      // [n_songs][N_TUNING]
    TuningState* tuning;    // [n_songs]
    uint32_t* peak_rec;     // [total_c][PIP_MAX_PER_FRAME] per-peak records written by the STFT kernel (see peak_record())
    uint32_t* peak_cnt;     // [total_c] records per frame
    double* cand_mag;       // [cand_cap] candidate pool of the chunk (slots handed out by tune_select_kernel)
    uint8_t* cand_pb;       // [cand_cap]
    uint32_t* cand_cursor;  // [0] next free pool slot
    uint32_t cand_cap;
    double* chroma_part;    // [total chroma tiles][10] partial sums of interval features
    double* dbg_chroma;     // [total_c][12] chroma_stft's normalised columns, or NULL (BLISSGPU_OPT_DEBUG_CHROMA)
    double* dbg_interval;   // [n_songs][10] interval means before the normalisation, or NULL
    TempoState* tempo;      // [n_songs]
    float* run_bpm;         // [n_songs][runs_pitch] bpm after each beat-tracker run
    uint32_t* run_cnt;      // [n_songs][runs_pitch] beats recorded while that bpm was current
    uint32_t runs_pitch;
    float* bt_pre;          // [total_b / 128 + n_songs][BT_PRE_STRIDE] per-run records; song s starts at run b_off / 128 + s
    float* summary;         // [n_songs][16] features 1..9 (zcr, timbral, loudness summaries)
    RollFix* roll_fix;      // the exact rolloff pass's record (see RollFix)
    size_t roll_fix_bytes;  // the borrowed stretch: spectrogram + peak records
};

struct Batch {
    const float* pcm;
    const SongDesc* songs;    // device
    uint32_t n_songs;
    // tile prefix arrays (device), n_songs+1 entries each
    const uint32_t* pfx_f;    // fft512 tiles
    const uint32_t* pfx_c;    // STFT tiles (STFT_TILE chroma frames each)
    const uint32_t* pfx_ct;   // 64-frame chroma tiles (tuning pass 2 workgroups, chroma_part slots)
    const uint32_t* pfx_cw;   // chroma contraction workgroups (4 tiles of 64 frames each)
    uint32_t tiles_f, tiles_c, tiles_ct, tiles_cw;
    uint64_t total_b;         // tempo frames in the batch
    uint32_t max_nb;          // longest song's tempo-frame count
    uint32_t max_nt;          // longest song's timbral-frame count
};

void launch_fft512(const Batch&, const Workspace&, const DeviceTables&, hipStream_t, bool rolloff_exact_all = false, bool seq_flux = false);
void launch_rolloff_fix(const Batch&, const Workspace&, uint64_t total_t, hipStream_t);
void launch_onset(const Batch&, const Workspace&, hipStream_t);
void launch_beat(const Batch&, const Workspace&, const DeviceTables&, hipStream_t);
// the two halves of launch_beat on streams of their own (the masked tail): autocorrelations (parallel), state machines (a wavefront per song)
void launch_beat_acf(const Batch&, const Workspace&, const DeviceTables&, hipStream_t);
void launch_beat_track(const Batch&, const Workspace&, const DeviceTables&, hipStream_t);
void launch_stft8192(const Batch&, const Workspace&, const DeviceTables&, hipStream_t, int shape = 0);  // shape: BLISSGPU_OPT_STFT_SHAPE
// a contiguous range of a chunk's songs [s0, s1) with the tile / workgroup ranges that belong to it in pfx_ct / pfx_cw
// units (the tuning estimate and the contraction of a one-chunk batch run in two halves; NULL = the whole chunk)
struct SongRange { uint32_t s0, s1, ct0, ct1, cw0, cw1; };
void launch_tune_select(const Batch&, const Workspace&, hipStream_t, const SongRange* r = nullptr);
void launch_tune_pass2(const Batch&, const Workspace&, hipStream_t, const SongRange* r = nullptr);
void launch_tune_final(const Batch&, const Workspace&, hipStream_t, const SongRange* r = nullptr);
void launch_chroma(const Batch&, const Workspace&, const DeviceTables&, hipStream_t, const SongRange* r = nullptr);
void launch_summary(const Batch&, const Workspace&, hipStream_t);
void launch_finalize(const Batch&, const Workspace&, uint32_t features_version, float* d_out, int32_t* d_status,
                     int32_t* dbg_tuning, uint32_t* dbg_nbpms, hipStream_t);
void launch_chroma_bank(double* bank, hipStream_t);
// raw decoder output at 22 050 Hz -> mono f32: sample_format BLISSGPU_SAMPLE_* (s16: sample / 32768, s32: sample / 2^31),
// `channels` interleaved
void launch_pcm_convert(const void* in, int sample_format, uint32_t channels, float* out, uint64_t frames, hipStream_t st);
// raw decoder output at another rate -> mono 22 050 Hz f32 (libswresample's default resampler, resample.hpp)
struct SwrPlan;
hipError_t launch_resample(const void* in, int sample_format, uint32_t channels, uint64_t frames, const SwrPlan& plan,
                           const float* d_bank, float* out, uint64_t n_out, hipStream_t st);
// FLAC frames -> interleaved PCM, one lane per frame (kernels_flac.hip; the decoding itself is flac_frame.hpp)
constexpr int FLAC_LANES = 64;  // one wavefront per workgroup: 16 KiB of LDS for the predictor windows of orders 13..32
struct FlacSong {        // one file of the batch
    uint64_t byte_off;   // its first byte in the batch's compressed bytes (a multiple of 16; 16 bytes of padding follow the file)
    uint64_t nbytes;
    uint64_t pcm_off;    // its first byte in the batch's PCM
    uint64_t total;      // inter-channel samples
    uint64_t base;       // the stream position the file's first frame codes (variable-block-size headers count from it)
    uint32_t channels, bps;
};
struct FlacFrame {       // one row of the frame table (flac_index.hpp)
    uint64_t offset, nbytes, first_sample;  // byte range in the file, header to CRC-16
    uint32_t blocksize, song;               // song: bit 31 = the song's last frame (FLAC_LAST_FRAME)
};
constexpr uint32_t FLAC_LAST_FRAME = 0x80000000u;
void launch_flac_decode(const uint8_t* bytes, const FlacSong* songs, const FlacFrame* frames, uint32_t n_frames, uint8_t* pcm,
                        int32_t* status, uint64_t* end, hipStream_t st);
// song_bad[s] = 1 when a frame of song s failed or did not stop 2 bytes before its successor; a song's last frame may stop
// earlier (an ID3v1 tag or padding behind the audio).  song_bad is zeroed by the caller
void launch_flac_check(const FlacFrame* frames, uint32_t n_frames, const int32_t* status, const uint64_t* end, uint32_t* song_bad,
                       hipStream_t st);
// The opt-in checks (kernels_flac_verify.hip; the arithmetic is flac_verify.hpp).  CRC-16 of every frame with status FRAME_OK
// over [offset, end[i]), one wavefront per frame, against the two bytes at end[i].  A mismatch sets song_crc_bad[s] and takes
// song_first_bad[s] down to the frame's index within its song, i - song_first[s] (song_crc_bad zeroed, song_first_bad set to
// 0xFFFFFFFF by the caller; the three may be NULL together).  frame_ok (may be NULL): 1, 0, or -1 for a frame that was not OK
void launch_flac_crc(const uint8_t* bytes, const FlacSong* songs, const FlacFrame* frames, uint32_t n_frames, const int32_t* status,
                     const uint64_t* end, const uint32_t* song_first, uint32_t* song_crc_bad, uint32_t* song_first_bad, int32_t* frame_ok,
                     hipStream_t st);
struct FlacMd5Job {      // one song of flac_md5_kernel, one lane
    uint64_t pcm_off;    // its first byte in the PCM (a multiple of 4)
    uint64_t n_elems;    // total x channels: int16 up to 16 bits per sample, int32 above
    uint32_t bps, slot;  // digests[16 * slot .. + 16) receives the MD5 of the FLAC message
};
void launch_flac_md5(const uint8_t* pcm, const FlacMd5Job* jobs, uint32_t n_jobs, void* digests, hipStream_t st);
void launch_flac_md5_one(const uint8_t* pcm, const FlacMd5Job& job, void* digests, hipStream_t st);  // the job travels with the launch
// one pair distance with both vectors passed by value (no staging copies); result -> *out (device-visible host word)
void launch_pair_distance(const float* a, const float* b, uint32_t d, int metric, const float* d_M, float* out, hipStream_t st);
// playlist ordering (kernels_playlist.hip)
void launch_set_distance(const float* seeds, uint32_t n_seeds, const float* cand, uint64_t n, uint32_t d, int metric,
                         const float* M, float* dist, uint32_t* keys, uint32_t* idx, uint32_t* nan_flag, hipStream_t st);
// stable radix sort of (key, value) pairs; tmp == NULL reports the scratch bytes; keys_in / vals_in are scratch afterwards
// (sync: one zeroed word -> the single-launch form when the tiles fit max_coresident workgroups; NULL: one launch per step)
hipError_t sort_pairs_u32(void* tmp, size_t* tmp_bytes, uint32_t* keys_in, uint32_t* keys_out, uint32_t* vals_in,
                          uint32_t* vals_out, uint32_t n, hipStream_t st, uint32_t* sync = nullptr, uint32_t max_coresident = 0);
void launch_song_to_song(const float* seeds, uint32_t n_seeds, const float* cand, uint32_t n, uint32_t d, int metric,
                         const float* M, uint32_t* order, unsigned long long* slots, uint32_t* sync, uint32_t grid,
                         hipStream_t st);
// dedup_playlist_custom_distance over the playlist seq[0..len) (NULL: identity) of rows of x: next[p] for every position,
// then the chain walk -> kept[0..*n_kept); a NaN on the chain sets *nan_flag, a seq entry >= n sets *bad
void launch_dedup_next(const float* x, uint64_t n, uint32_t d, const uint32_t* seq, uint32_t len, const uint32_t* meta,
                       int metric, const float* M, float thr, uint32_t* next, uint32_t* bad, hipStream_t st);
void launch_dedup_walk(const float* x, uint64_t n, uint32_t d, const uint32_t* seq, uint32_t len, const uint32_t* meta,
                       int metric, const float* M, float thr, const uint32_t* next, uint32_t* kept, uint64_t* n_kept,
                       uint32_t* nan_flag, uint32_t* bad, hipStream_t st);
// k nearest candidates per query (kernels_knn.hip): the split of the work for (q, n, k), then the two launches.  `part` holds
// part_keys 64-bit keys; a NaN among the evaluated distances sets *nan_flag, a skip entry >= n (other than 0xFFFFFFFF) *bad_flag
struct KnnPlan {
    uint32_t cap;               // keys of a query's threshold buffer: a power of two, >= k + 64
    uint32_t qb;                // queries per workgroup
    uint32_t n_split;           // workgroups that share a query's candidates
    uint32_t blocks_per_split;  // 256-candidate blocks each of them walks
    uint32_t grid_qb;           // query blocks in the grid (the kernel strides over the rest)
    uint64_t part_keys;         // q * n_split * k
};
KnnPlan knn_plan(uint64_t q, uint64_t n, uint32_t k, int n_cus);
void launch_knn_scan(const float* Q, uint64_t q, const float* X, uint32_t n, uint32_t d, int metric, const float* M,
                     int m_is_diag, const uint32_t* skip, uint32_t k, const KnnPlan& p, unsigned long long* part,
                     uint32_t* nan_flag, uint32_t* bad_flag, hipStream_t st);
void launch_knn_merge(const unsigned long long* part, uint64_t q, uint32_t k, const KnnPlan& p, uint32_t* idx, float* dist,
                      hipStream_t st);
// k nearest candidates per query under the locally scaled distance dist / sqrtf(qscale[i] * cscale[j]) (kernels_scaled_knn.hip):
// knn_plan's split, the same partial lists, launch_knn_merge afterwards.  Flags as for knn; a scale outside [2^-60, 2^60] (a NaN
// included) sets *scale_flag
void launch_scaled_knn_scan(const float* Q, uint64_t q, const float* qscale, const float* X, uint32_t n, const float* cscale,
                            uint32_t d, int metric, const float* M, int m_is_diag, const uint32_t* skip, uint32_t k,
                            const KnnPlan& p, unsigned long long* part, uint32_t* nan_flag, uint32_t* bad_flag,
                            uint32_t* scale_flag, hipStream_t st);
// count[idx[e]] += 1 for every entry of idx [entries] that is not 0xFFFFFFFF (count zeroed by the caller); an entry >= n sets
// *bad_flag.  lds: the windowed LDS-histogram form (the A/B of DESIGN.md 3.27), same result
void launch_knn_occurrence(const uint32_t* idx, uint64_t entries, uint32_t n, uint32_t* count, uint32_t* bad_flag, bool lds,
                           int n_cus, hipStream_t st);
// k nearest candidates per seed GROUP (kernels_group_knn.hip): the groups x candidates plane dealt out in items, then the two
// launches.  `part` holds list_off[n_groups] lists of k 64-bit keys; flags as for knn
constexpr int GROUP_KNN_SEED_TILE = 32;  // the most seed rows of one group held in LDS at a time
constexpr int GROUP_KNN_M_PER_GROUP = 2;  // m_is_diag of launch_group_knn_scan: M is [n_groups][d], row g = the diagonal of group g's M
struct GroupKnnItem {
    uint32_t g_lo, g_hi;  // groups [g_lo, g_hi)
    uint32_t c_lo, c_hi;  // candidates [c_lo, c_hi): c_lo a multiple of the candidate block
    uint32_t split;       // which of its groups' partial lists the item writes
};
struct GroupKnnPlan {
    uint32_t cap = 0, qb = 0;               // keys of a group's threshold buffer, groups a workgroup holds at a time
    uint32_t cand_block = 0, seed_tile = 0;
    std::vector<GroupKnnItem> items;
    std::vector<uint32_t> list_off;         // [n_groups + 1]: group g's partial lists are list_off[g] .. list_off[g + 1]
};
GroupKnnPlan group_knn_plan(const uint64_t* off, uint64_t n_groups, uint64_t n, uint32_t k, uint32_t n_cus);
void launch_group_knn_scan(const float* S, const uint32_t* goff, const float* X, uint32_t n, uint32_t d, int metric,
                           const float* M, int m_is_diag, const uint32_t* skip, uint32_t k, const GroupKnnPlan& p,
                           const GroupKnnItem* items, const uint32_t* list_off, unsigned long long* part, uint32_t* nan_flag,
                           uint32_t* bad_flag, hipStream_t st);
void launch_group_knn_merge(const unsigned long long* part, const uint32_t* list_off, uint64_t n_groups, uint32_t k,
                            const GroupKnnPlan& p, uint32_t* idx, float* dist, hipStream_t st);
// W[g][0..d) = the diagonal of variance_based_weight_matrix of group g's seed rows, ones (status 1) under two seeds; status may be NULL
void launch_group_weights(const float* S, const uint32_t* goff, uint64_t n_groups, uint32_t d, float* W, int32_t* status,
                          hipStream_t st);
// k nearest ALBUMS per seed group (kernels_albums.hip).  The tables are built on the host from album_of and skip (device
// pointers here): album a's songs are arow[arow_off[a] .. arow_off[a + 1]) in ascending candidate index; group g's patches --
// the albums its skip entries touch -- are patch_*[patch_off[g] .. patch_off[g + 1]) sorted by album, patch p naming its album,
// the rows the group leaves it (patch_cnt, 0: the album does not exist for the group) and the ascending list
// pskip[pskip_off[p] .. pskip_off[p + 1]) of the rows it loses.
struct AlbumTables {
    const uint32_t *goff, *arow_off, *arow, *patch_off, *patch_album, *patch_cnt, *pskip_off, *pskip;
    uint32_t n_albums, n_groups, n_patches;
};
// the sequential f32 means of every album (-> centroids [n_albums][d], NaN rows for albums without songs), group (-> gmeans
// [n_groups][d]) and patch (-> pcent [n_patches][d]) in one launch
void launch_segment_mean(const float* X, const float* S, uint32_t d, const AlbumTables& t, float* centroids, float* gmeans,
                         float* pcent, hipStream_t st);
// p = knn_plan(n_groups, n_albums, k, n_cus); `part` holds p.part_keys keys for launch_knn_merge; a NaN distance of an existing
// (group, album) pair sets *nan_flag
void launch_album_knn_scan(const float* gmeans, const float* centroids, uint32_t d, const AlbumTables& t, const float* pcent,
                           uint32_t k, const KnnPlan& p, unsigned long long* part, uint32_t* nan_flag, hipStream_t st);
// k-means (kernels_kmeans.hip).  One iteration: assign (labels in place: a song whose label moves counts into *changed; dist may
// be NULL; a NaN among the evaluated distances sets *nan_flag), then the stable counting sort of the labels -- hist [K][W]
// zeroed by the caller, scanned in place into list positions (bsum: scan_tiles words of scratch), arow_off [K + 1] and arow [n]
// in the form AlbumTables wants -- launch_segment_mean over those lists, and the select: next[c] = prev[c] for a cluster
// without rows (next NULL: nothing), sizes[c] (NULL: nothing) = its rows
struct KmeansPlan {
    uint32_t assign_waves, assign_grid;  // wavefronts per workgroup of the assignment (256 songs each), its workgroups
    uint32_t W, chunk;                   // the sort's chunks (one wavefront each) and their songs
    uint64_t hist_words;                 // K * W
    uint32_t scan_tiles;                 // 2048-word tiles of the scan
};
KmeansPlan kmeans_plan(uint64_t n, uint32_t K, int n_cus);
void launch_kmeans_assign(const float* X, uint32_t n, const float* C, uint32_t K, uint32_t d, int metric, const float* M,
                          int m_is_diag, const KmeansPlan& p, uint32_t* labels, float* dist, uint32_t* changed, uint32_t* nan_flag,
                          hipStream_t st);
void launch_kmeans_hist(const uint32_t* labels, uint32_t n, uint32_t K, const KmeansPlan& p, uint32_t* hist, hipStream_t st);
void launch_kmeans_scan_tiles(uint32_t* hist, const KmeansPlan& p, uint32_t* bsum, hipStream_t st);
void launch_kmeans_scan_add(uint32_t* hist, uint32_t n, uint32_t K, const KmeansPlan& p, const uint32_t* bsum, uint32_t* arow_off,
                            hipStream_t st);
void launch_kmeans_scatter(const uint32_t* labels, uint32_t n, uint32_t K, const KmeansPlan& p, uint32_t* pos, uint32_t* arow,
                           hipStream_t st);
void launch_kmeans_select(const float* prev, float* next, const uint32_t* arow_off, uint32_t K, uint32_t d, uint32_t* sizes,
                          hipStream_t st);
// the silhouette of a labelling (kernels_silhouette.hip), after the k-means sort of the labels into arow_off / arow.  The scored
// songs are rows[0 .. q) (NULL: every song, q = n), cut into pieces of 256 per wavefront; the clusters are dealt to Y column
// groups, cluster c to group floor(arow_off[c] Y / n).  The scan writes ws_best_q / ws_best_i [Y][q] (the best other quotient of
// the group's clusters and its cluster, SIL_NONE: none) and ws_own [Y][q] (the own-cluster sum, in the own cluster's group only);
// the finish forms s, a, b, neighbour (a, b, neighbour, sizes may be NULL).  flags[0]: a NaN distance; flags[1]: SIL_ERR_*
constexpr uint32_t SIL_ERR_LABEL = 1u, SIL_ERR_ROW = 2u, SIL_ERR_CLUSTERS = 4u;
struct SilhouetteArgs {
    const float* X;
    const uint32_t *labels, *arow_off, *arow, *rows;
    const float* M;
    uint32_t n, K, q, Y, d;
    int metric;
    double *ws_own, *ws_best_q;
    uint32_t* ws_best_i;
    uint32_t* flags;
    float* s;
    double *a, *b;
    uint32_t *neighbour, *sizes;
};
struct SilhouettePlan {
    uint32_t waves, grid;  // wavefronts per workgroup of the scan (256 scored songs each), its workgroups per column group
    uint32_t Y;            // column groups: col_groups when not 0, else about two workgroups per CU; at most K
};
SilhouettePlan silhouette_plan(uint64_t q, uint32_t K, int n_cus, uint32_t col_groups);
void launch_silhouette_scan(const SilhouetteArgs& a, int m_is_diag, const SilhouettePlan& p, hipStream_t st);
void launch_silhouette_finish(const SilhouetteArgs& a, hipStream_t st);
// the moments of a library (kernels_moments.hip), after the k-means sort of the labels into arow_off / arow (both NULL without
// labels: one group, the rows in place).  Every f64 sum is the blocked sum of include/blissgpu.h, one launch per level: off is
// [levels][K + 1], off[l][g] = where group g's block sums of level l start (moments_plan_kernel); level 0 is the sum / m2 /
// scatter kernel, every further level and the last step (divide, copy, mirror) moments_reduce_kernel.  flags[0]: a NaN or an
// infinity in x; flags[1]: MO_ERR_*
constexpr uint32_t MO_ERR_LABEL = 1u;
constexpr int MO_RED_PART = 0, MO_RED_MEAN = 1, MO_RED_M2 = 2, MO_RED_SCATTER = 3;
struct MomentsArgs {
    const float* X;
    const uint32_t *labels, *arow_off, *arow, *off;
    const double* mean;
    uint32_t n, K, d;
    uint32_t *key_min, *key_max, *flags;
};
struct MomentsPlan {
    uint32_t levels;     // of the blocked sum over n terms: 1 for n <= 256, 2 up to 65 536, at most 4
    uint32_t items[4];   // per level: an upper bound of the groups' block sums, floor(n / 256^(l + 1)) + min(K, n)
    uint32_t blocks[4];  // per level: the block sums over all rows, ceil(n / 256^(l + 1))
};
MomentsPlan moments_plan(uint64_t n, uint32_t K);
void launch_moments_plan(const uint32_t* arow_off, uint32_t n, uint32_t K, const MomentsPlan& p, uint32_t* off, uint32_t* counts,
                         hipStream_t st);
void launch_moments_sum(const MomentsArgs& a, const MomentsPlan& p, double* part, hipStream_t st);
void launch_moments_m2(const MomentsArgs& a, const MomentsPlan& p, double* part, bool extrema, hipStream_t st);
void launch_moments_scatter(const MomentsArgs& a, const MomentsPlan& p, double* part, hipStream_t st);
// out_bound: an upper bound of the block sums this launch forms (the grid); the kernel reads the exact number from out_off / out_n
void launch_moments_reduce(const double* in, const uint32_t* in_off, uint32_t in_n, double* out, const uint32_t* out_off,
                           uint32_t out_n, uint32_t out_bound, uint32_t K, uint32_t w, int mode, const uint32_t* counts, double* dst,
                           uint32_t d, hipStream_t st);
void launch_moments_finish(const uint32_t* counts, const uint32_t* key_min, const uint32_t* key_max, uint32_t K, uint32_t d, float* mn,
                           float* mx, hipStream_t st);
// group-to-group set distances (kernels_chamfer.hip), after the k-means sort of the labels into arow_off / arow.  The target
// groups are taken in slabs [s0, s1): the scan writes minima [s1 - s0][n] (m(i, c) at [c - s0][position of i in the sorted
// order]), the reduce D [K][K] (D(a -> c) for non-empty a != c of the slab; nothing else is written or read).  The select forms
// A per query row (queries NULL: row g = group g) through rowbuf [select_grid][K], writes idx / dist [q][t], sizes and matrix
// (both may be NULL).  flags[0]: a NaN among the minima; flags[1]: CH_ERR_*
constexpr uint32_t CH_ERR_LABEL = 1u, CH_ERR_QUERY = 2u;
constexpr uint64_t CHAMFER_SLAB_BYTES = 512ull << 20;  // the plan's slab holds at most this many bytes of minima
struct ChamferArgs {
    const float* X;
    const uint32_t *labels, *arow_off, *arow, *queries;
    const float* M;
    uint32_t n, K, d, q, t;
    int metric, mode;
    uint32_t s0, s1, Y;
    float* minima;
    double *D, *rowbuf;
    uint32_t* flags;
    uint32_t* idx;
    double* dist;
    uint32_t* sizes;
    double* matrix;
};
struct ChamferPlan {
    uint32_t waves, grid;  // wavefronts per workgroup of the scan (256 positions each), its workgroups per column group
    uint32_t select_grid;  // workgroups of the select, each with a row buffer
    uint32_t slab;         // target groups per pass: slab_groups when not 0, else what CHAMFER_SLAB_BYTES and the limit hold
    uint64_t bytes;        // the whole workspace: fixed_bytes (flags and the sort) + D + row buffers + minima
    bool fits;             // bytes <= ws_limit
};
ChamferPlan chamfer_plan(uint64_t n, uint32_t K, uint64_t q, bool want_matrix, int n_cus, uint32_t slab_groups, uint64_t ws_limit,
                         uint64_t fixed_bytes);
void launch_chamfer_scan(ChamferArgs a, int m_is_diag, const ChamferPlan& p, int n_cus, hipStream_t st);  // (sets a.Y for the slab)
void launch_chamfer_reduce(const ChamferArgs& a, hipStream_t st);
void launch_chamfer_select(const ChamferArgs& a, const ChamferPlan& p, hipStream_t st);
// the minimum spanning tree, one round of Boruvka's algorithm (kernels_mst.hip; mst_merge.hpp is the host half).  order [n] = the
// songs sorted by (component, index), cpos [n] = the component at every position, comps of them.  The scan writes every column
// group's winner per position, part_w / part_j [Y][n] (weight bits, other song; 0xFFFFFFFF: none); the pick merges them into
// [0][.] (phase 0, with the minimum weight per component into comp_w [comps]) and takes the smallest (lower song << 32 | higher
// song) among a component's positions of that weight into comp_uv [comps] (phase 1).  comp_w / comp_uv start as all ones.
// flags[0]: a NaN or negative sum among the evaluated pairs; flags[1]: a core that is NaN or negative
struct MstArgs {
    const float *X, *M, *core;  // core may be NULL
    const uint32_t *order, *cpos;
    uint32_t n, d, comps;
    int metric;
    uint32_t Y, skip, phase;  // skip: wavefronts of one component step over that component's tiles
    uint32_t *part_w, *part_j, *comp_w;
    unsigned long long* comp_uv;
    uint32_t* flags;
};
struct MstPlan {
    uint32_t waves, grid;  // wavefronts per workgroup of the scan (256 positions each), its workgroups per column group
    uint32_t Y;            // column groups: col_groups when not 0, else enough to fill the device
    uint32_t pick_grid;
    uint64_t bytes;        // the whole workspace
    bool fits;             // bytes <= ws_limit
};
MstPlan mst_plan(uint64_t n, int n_cus, uint32_t col_groups, uint64_t ws_limit);
void launch_mst_scan(const MstArgs& a, int m_is_diag, const MstPlan& p, hipStream_t st);
void launch_mst_pick(MstArgs a, uint32_t phase, const MstPlan& p, hipStream_t st);
// Ward clustering, one round (kernels_ward.hip; ward_merge.hpp is the host half).  The m clusters sit at positions 0 .. m - 1;
// position p's row is X[low[p]] (low == NULL: X[p]; every slot below `slots`), its size is size[p] (NULL: 1).  The scan folds
// every position's smallest key (cost bits << 32 | p XOR j) into best [m] by atomic minima (all ones before the launch);
// flags[0]: a NaN cost among the evaluated pairs.  The join reads plan [m_new][2] = (old position, partner or 0xFFFFFFFF),
// rewrites the merged rows in place in the lower position's slot, writes size_out / low_out [m_new] and resets best [m_new]
struct WardArgs {
    const float *X, *M;
    const uint32_t *low, *size;  // either may be NULL
    uint32_t m, d, slots;
    int metric;
    uint32_t Y;
    unsigned long long* best;
    uint32_t* flags;
};
struct WardJoinArgs {
    float* X;
    const uint32_t *plan, *size, *low;
    uint32_t *size_out, *low_out;
    unsigned long long* best;  // [m_new] reset to all ones for the next scan
    uint32_t m_old, m_new, d, slots;
};
struct WardPlan {
    uint32_t waves, grid;  // wavefronts per workgroup of the scan (256 positions each), its workgroups per column group
    uint32_t Y;            // column groups: col_groups when not 0, else enough to fill the device
};
WardPlan ward_plan(uint64_t m, int n_cus, uint32_t col_groups);
void launch_ward_scan(const WardArgs& a, int m_is_diag, bool filter, const WardPlan& p, hipStream_t st);
void launch_ward_join(const WardJoinArgs& a, hipStream_t st);
// k-medoids, one scan of a slab of candidates (kernels_pam.hip), after the k-means sort of near into arow_off / arow.  The slab's
// candidates are rows[0 .. q) (NULL: the songs row0 .. row0 + q), cut into pieces of 256 per wavefront; the slots are dealt to Y
// column groups as the silhouette deals its clusters (silhouette_plan gives the grid).  The scan writes ws_a / ws_b [q][K] for the
// non-empty slots, the fold fills in the empty ones and forms btot, best, arg [q].  flags[0]: a NaN among the evaluated distances
constexpr uint32_t PAM_NONE = 0xFFFFFFFFu;
struct PamArgs {
    const float *X, *M;
    const uint32_t *arow_off, *arow, *rows;
    const float *d1, *d2;
    uint32_t n, K, q, row0, Y, d;
    int metric;
    double *ws_a, *ws_b;
    uint32_t* flags;
    double *btot, *best;
    uint32_t* arg;
};
// what the host reads per round: the winner (c == PAM_NONE: no candidate), its value and slot, TD, the NaN word (and the word the
// k-nearest scan reports a bad skip entry in: never raised here)
struct PamRecord {
    double val, td;
    uint32_t c, arg, nan, bad;
};
void launch_pam_scan(const PamArgs& a, int m_is_diag, const SilhouettePlan& p, hipStream_t st);
void launch_pam_fold(const PamArgs& a, hipStream_t st);
void launch_pam_pick(const double* val, uint32_t stride, const uint32_t* arg, const uint32_t* rows, uint32_t row0, uint32_t q,
                     const uint32_t* ismed, bool fresh, PamRecord* rec, hipStream_t st);
void launch_pam_gather(const float* X, uint32_t* med, uint32_t K, uint32_t d, float* rows_out, uint32_t swap_slot, uint32_t swap_c,
                       bool append, bool mark_all, uint32_t* ismed, hipStream_t st);
void launch_pam_state(const uint32_t* idx, const float* dist, uint32_t n, uint32_t kk, uint32_t* near, float* d1, float* d2,
                      hipStream_t st);
void launch_pam_td(const float* d1, uint32_t n, PamRecord* rec, hipStream_t st);
// acoustic fingerprints (kernels_fingerprint.hip).  Frame f of a song is samples [512 f, 512 f + 8192); a workgroup of the band
// kernel transforms a run of FP_RUN consecutive frames.  A group of songs is described by FpSong [n_songs], run_pfx [n_songs + 1]
// (runs in front of every song) and word_pfx [n_songs + 1]; song s of the group owns the rows word_pfx[s] + s .. of E [rows][33]
// (one row per frame = one more than its words; a too-short song owns one row that nothing writes)
constexpr int FP_FRAME = 8192, FP_HOP = 512, FP_BANDS = 33, FP_RUN = 6;
constexpr uint32_t FP_MAX_WORDS = 1u << 22, FP_MAX_OFFSET = 4096;
// the 34 bin edges of the 33 bands, 300 .. 2000 Hz logarithmically: the contract is this table (include/blissgpu.h)
#define FP_EDGE_LIST                                                                                                             \
    111, 118, 125, 132, 140, 149, 157, 167, 177, 187, 198, 210, 222, 235, 249, 264, 280, 296, 314, 332, 352, 373, 395, 418, 443, \
        469, 497, 526, 557, 590, 625, 662, 702, 743
struct FpSong {
    uint64_t pcm_off;  // first sample in the group's PCM
    uint32_t frames;   // 0: too short
    uint32_t row0;     // first row of E
};
// the best offset of one (pair, block of 256 offsets): count = valid positions (bits = 32 count); valid == 0: no offset counts
struct FpCand {
    uint32_t errors, count;
    int32_t offset;
    uint32_t valid;
};
void launch_fp_bands(const float* pcm, const FpSong* songs, uint32_t n_songs, const uint32_t* run_pfx, uint32_t n_runs,
                     const float* hann, const float2* tw, double* E, hipStream_t st);
void launch_fp_bits(const double* E, const uint32_t* word_pfx, uint32_t n_songs, uint32_t n_words, uint32_t* words, hipStream_t st);
// pairs [n_pairs][2]; cand [n_pairs][n_blocks], n_blocks = ceil((2 max_offset + 1) / 256); n_pairs * n_blocks < 2^31
void launch_fp_match(const uint32_t* words, const uint64_t* word_offsets, uint32_t n_songs, const uint32_t* pairs, uint32_t n_pairs,
                     uint32_t n_blocks, int max_offset, uint32_t min_overlap, FpCand* cand, hipStream_t st);
void launch_fp_pick(const FpCand* cand, uint32_t n_pairs, uint32_t n_blocks, int32_t* offset, uint32_t* errors, uint32_t* bits,
                    hipStream_t st);
// loudness (kernels_loudness.hip).  A group of songs is described by LoudSong [n_songs]; the energy kernel is launched once per
// (sample format, channel count) present in the group, over the songs of that class: song_of [n_class] names them, row_pfx
// [n_class + 1] counts the rows (segments of BLISSGPU_LOUDNESS_SEGMENT sub-blocks) in front of each.  z is the group's energies,
// song s channel c sub-block u at z_off + c n_sub + u.  Every song's PCM starts on a multiple of 256 bytes and is padded to one.
struct LoudSong {
    uint64_t pcm_off;   // bytes into the group's PCM
    uint64_t frames;
    uint64_t z_off;     // doubles into the group's z
    uint32_t hop;       // samples per sub-block
    uint32_t n_sub;     // >= 4
    uint16_t channels, format;
    uint32_t factor;    // the true peak's oversampling: 4, 2 or 1
    double coef[10];    // the K-weighting table (blissgpu_loudness_kweighting)
};
void launch_loud_energy(const uint8_t* pcm, const LoudSong* songs, int format, int channels, const uint32_t* song_of,
                        const uint32_t* row_pfx, uint32_t n_class, uint32_t n_rows, double* z, hipStream_t st);
// tile_pfx [n_songs + 1]: loud_peak_tiles() of every song; htab [3][49]: the interpolators of factor 4, 2, 1; part [n_tiles][2];
// peaks [n_songs][2] = sample peak, true peak
uint32_t loud_peak_tiles(uint64_t frames, uint32_t channels);
void launch_loud_peak(const uint8_t* pcm, const LoudSong* songs, uint32_t n_songs, const uint32_t* tile_pfx, uint32_t n_tiles,
                      const double* htab, double* part, hipStream_t st);
void launch_loud_fold(const double* part, const uint32_t* tile_pfx, uint32_t n_songs, double* peaks, hipStream_t st);
// triplet metric learning, one gradient evaluation (kernels_metric.hip).  The triplets are dealt out in W contiguous chunks, a
// function of T alone; part [W][pairs + 1] f64 and cnt [W][2] u64 are the wavefronts' partials, out = G f64 [d][d] | loss f64 |
// n_active u64 | error bits u64 (TRIPLET_ERR_*).  mode says how M is read; flags (u8 [T]) may be NULL
constexpr int TRIPLET_M_FULL = 0, TRIPLET_M_DIAG = 1, TRIPLET_M_IDENTITY = 2;
constexpr uint32_t TRIPLET_ERR_INDEX = 1u, TRIPLET_ERR_NAN = 2u;
struct TripletPlan {
    uint32_t W, chunk;      // wavefronts (one workgroup each) and the triplets of each, a multiple of 64
    uint32_t pairs;         // d (d + 1) / 2
    uint64_t part_doubles;  // W * (pairs + 1)
};
TripletPlan triplet_plan(uint64_t T, uint32_t d);
void launch_triplet_step(const float* X, uint64_t n, uint32_t d, const uint32_t* trip, uint64_t T, const float* M, int mode,
                         double margin, const TripletPlan& p, uint8_t* flags, double* part, unsigned long long* cnt, hipStream_t st);
void launch_triplet_reduce(const double* part, const unsigned long long* cnt, const TripletPlan& p, uint32_t d, double* out,
                           hipStream_t st);
// song-to-song chains cut after k, one per seed group (kernels_chains.hip).  Step 0 is the group search with k = 1; a later step
// t reads idx[chain][0 .. t) and writes idx / dist [chain][t], directly or -- several workgroups per chain -- through the
// 64-bit minima best[n_chains] (all KNN_NONE before the first step; reset by the step's second launch).  A NaN among the
// distances a chain evaluates sets *nan_flag
struct ChainPlan {
    uint32_t qb;                // chains per workgroup
    uint32_t n_split;           // workgroups that share a chain's candidates
    uint32_t blocks_per_split;  // 256-candidate blocks each of them walks
    uint32_t grid_cb;           // chain blocks in the grid (the kernel strides over the rest)
};
ChainPlan chain_plan(uint64_t n_chains, uint64_t n, int n_cus);
void launch_chain_step(const float* X, uint32_t n, uint32_t d, int metric, const float* M, int m_is_diag, const uint32_t* goff,
                       const uint32_t* skip, uint32_t n_chains, uint32_t k, uint32_t t, const ChainPlan& p, uint32_t* idx,
                       float* dist, unsigned long long* best, uint32_t* nan_flag, hipStream_t st);
// journeys (kernels_chains.hip): chains with a step 0 of their own (the query is the journey's `from` row), two skip slots each
// (skip[n_journeys][2] or NULL) and either a waypoint query -- to != NULL: step t looks around from + (to - from) * s -- or a
// gate on one feature against the previous pick (GATE_*, the values of BLISSGPU_GATE_*).  Step t >= 0 writes idx / dist
// [journey][t] like a chains' step; a journey whose step finds no eligible candidate keeps its padding from there on
constexpr int GATE_NONE = 0, GATE_UP = 1, GATE_DOWN = 2;
struct JourneyStep {
    const float* from;      // [n_journeys][d]
    const float* to;        // [n_journeys][d], NULL: the query is the previous pick
    float s;                // (t + 1) / (k + 1), rounded once on the host
    int gate;               // GATE_*
    uint32_t gate_feature;  // < d
};
void launch_journey_step(const float* X, uint32_t n, uint32_t d, int metric, const float* M, int m_is_diag, const uint32_t* skip,
                         uint32_t n_journeys, uint32_t k, uint32_t t, const ChainPlan& p, const JourneyStep& j, uint32_t* idx,
                         float* dist, unsigned long long* best, uint32_t* nan_flag, hipStream_t st);
// radio playlists (kernels_radio.hip): chains (or, nearest != 0, the k nearest of the start row) under label
// rules.  `rules` holds the ACTIVE rules only (window >= 1 and limit <= window), their windows already cut to k + 1; rule[a] is
// the row of labels ([n_total][n]) and the column of from_labels ([n_radios][n_total] or NULL) that rule a reads.  Step t is
// launch_radio_ban (nothing with no active rule) followed by launch_radio_step: ban[(radio, a)][0 .. cap) / ban_cnt[(radio, a)]
// are the labels banned at that step.  best / nan_flag as for the chains; skip is [n_radios][2] or NULL
constexpr uint32_t RADIO_NONE = 0xFFFFFFFFu;  // no label: never banned
constexpr int RADIO_MAX_RULES = 4;
struct RadioRules {
    uint32_t n, n_total;  // active rules, rules of the call
    uint32_t cap;         // banned labels a (radio, rule) can have: max over the rules of min(window, k) / limit
    uint32_t rule[RADIO_MAX_RULES], window[RADIO_MAX_RULES], limit[RADIO_MAX_RULES];
};
struct RadioArgs {
    const float* X;  // [n][d] candidates
    uint32_t n, d;
    int metric;
    const float* M;
    int m_is_diag;
    const float* from;  // [n_radios][d]
    const uint32_t* skip;
    const uint32_t* labels;
    const uint32_t* from_labels;
    RadioRules rules;
    uint32_t* ban;
    uint32_t* ban_cnt;
    int nearest;
    uint32_t n_radios, k;
    uint32_t* idx;
    float* dist;
    unsigned long long* best;
    uint32_t* nan_flag;
};
void launch_radio_ban(const RadioArgs& a, uint32_t t, hipStream_t st);
void launch_radio_step(const RadioArgs& a, uint32_t t, const ChainPlan& p, hipStream_t st);
// the 2-D map of a library (kernels_map.hip; the arithmetic is stated in include/blissgpu.h).  One gradient
// evaluation is launch_map_repulse (rows x column groups: the sums z, rx, ry of every row over one chunk of j), launch_map_attract
// (the chunk sums added per row, the 256-row block sums of z, and the CSR sums of the rows of at most MAP_LONG_ROW entries; a
// second launch gives every longer row a wavefront), launch_map_update (Z, the gradient, and either grad or the update of Y).
// sums is f64 [3][n] (z | rx | ry), part f64 [chunks][3][n] (unused with one chunk: the scan then writes sums itself), zb f64
// [ceil(n / 256)], att f64 [n][2], U and gain f64 [n][2]; long_rows lists the rows of more than MAP_LONG_ROW entries
constexpr uint32_t MAP_TILE = 256;      // rows of a workgroup, and the points of a staged tile
constexpr uint32_t MAP_LONG_ROW = 256;  // CSR entries a lane walks alone
constexpr uint32_t MAP_MAX_COL_GROUPS = 64;
constexpr int MAP_FEED_SCALAR = 0, MAP_FEED_LDS = 1;  // how the scan is fed y_j: scalar loads, or LDS broadcasts of a staged tile
struct MapPlan {
    uint32_t col_groups;  // C of the contract
    uint32_t width;       // w = 256 ceil(ceil(n / C) / 256)
    uint32_t chunks;      // the chunks that are not empty: ceil(n / w)
    uint32_t blocks;      // ceil(n / 256)
};
uint32_t map_plan_col_groups(uint64_t n, int n_cus);  // what col_groups == 0 resolves to (blissgpu_map_plan)
MapPlan map_plan(uint64_t n, uint32_t col_groups);    // col_groups >= 1
struct MapArgs {
    float* Y;  // [n][2]
    const unsigned long long* row_offsets;
    const uint32_t* cols;
    const float* vals;
    const uint32_t* long_rows;
    uint32_t n, n_long;
    double *sums, *part, *zb, *att, *U, *gain;
    double* grad;   // [n][2]: written instead of the update when not NULL
    double* z_out;  // where Z goes (an entry of the trace, or the step's result)
    double exaggeration, lr, momentum, min_gain;
    uint32_t first;  // the update starts from U = 0, gain = 1 and reads neither
};
void launch_map_repulse(const MapArgs& a, const MapPlan& p, int feed, hipStream_t st);
void launch_map_attract(const MapArgs& a, const MapPlan& p, hipStream_t st);
void launch_map_attract_long(const MapArgs& a, hipStream_t st);
void launch_map_update(const MapArgs& a, const MapPlan& p, hipStream_t st);
// column 0 of idx / dist from step 0's [n_chains] arrays
void launch_chain_first(const uint32_t* idx0, const float* dist0, uint32_t n_chains, uint32_t k, uint32_t* idx, float* dist,
                        hipStream_t st);
// the whole chains from the candidates' own k-nearest lists ([n][L], list c without c): column 0 as above, then the first entry
// of the current song's list that the chain has neither taken nor skipped; *short_flag: a list was too short to tell
void launch_chain_walk(const uint32_t* lists, const float* list_dist, uint32_t L, const uint32_t* goff, const uint32_t* skip,
                       const uint32_t* first, const float* first_dist, uint32_t n_chains, uint32_t k, uint32_t* idx, float* dist,
                       uint32_t* short_flag, hipStream_t st);
// duplicate groups (kernels_duplicates.hip): the split of the triangle of tile pairs for n rows, then the three launches.
// `label` doubles as the union-find's parent array; *n_pairs counts the edges, *cursor hands out pair-list slots (both zeroed
// by the init launch); a NaN distance of a pair i < j sets *nan_flag
struct DupPlan {
    uint32_t nb;         // blocks of 256 rows
    uint32_t row_split;  // workgroups that share a tile's rows (1 unless the triangle is small)
    uint64_t n_work;     // tile pairs I <= J times row_split
    uint32_t grid;
};
DupPlan dup_plan(uint64_t n, int n_cus);
float dup_bound(float threshold);  // sums above it cannot be closer than the threshold after the rounded square root
void launch_dup_init(uint32_t* label, uint32_t n, unsigned long long* n_pairs, unsigned long long* cursor, hipStream_t st);
void launch_dup_join(const float* X, uint32_t n, uint32_t d, int metric, const float* M, int m_is_diag, const uint32_t* meta,
                     float thr, const DupPlan& p, uint32_t* label, unsigned long long* n_pairs, unsigned long long* cursor,
                     uint32_t* pairs, float* pair_dist, uint64_t max_pairs, uint32_t* nan_flag, hipStream_t st);
void launch_dup_flatten(uint32_t* label, uint32_t n, hipStream_t st);
void launch_pairwise(const float* A, uint64_t n, const float* B, uint64_t m, uint32_t d, int metric, const float* M,
                     int m_is_diag, float* out, uint64_t ld_out, hipStream_t);
void launch_synth(float* pcm, const SongDesc* songs, uint32_t n_songs, const uint32_t* pfx_e, uint32_t tiles_e,
                  uint32_t first_song_index, const uint32_t* d_song_index, hipStream_t);

}  // namespace bg
