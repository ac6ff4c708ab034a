// kernels_loudness.hip -- EBU R128 / ReplayGain loudness (include/blissgpu.h): the K-weighted sub-block energies
// and the sample and true peaks of decoder output at its native rate, format and channel count (compiled with -ffp-contract=off:
// every f64 operation of the contract is rounded on its own).
//
//   loud_energy_kernel<FMT, NCH>  a lane owns one (song, channel, segment): it starts the two biquads from zero state
//                    BLISSGPU_LOUDNESS_WARMUP sub-blocks in front of its segment and walks to the segment's end, one sample after
//                    the other; a sub-block's energy is stored when the sub-block ends, the warm-up's are dropped.  A workgroup
//                    of 256 lanes is 256 / NCH rows (a row = one (song, segment); its NCH lanes read the same interleaved
//                    frames).  Neighbouring lanes sit a whole segment apart in memory, so the rows' samples go through LDS:
//                    per step every row's next 128 bytes (32 dwords, from a dword-aligned start) are loaded by 32 consecutive
//                    lanes -- whole cache lines -- and stored in the samples' native format; the lane then reads its own row.
//                    The row pitch is 33 dwords (34 for two channels of 4-byte samples), so the 32 lanes of a half-wave read
//                    32 different banks.  The loop count is the longest row's.
//   loud_peak_kernel a workgroup owns a tile of 2048 interleaved samples of one song, widened to f64 in LDS with a halo of 24
//                    frames on both sides (zero outside the song); a lane owns 8 positions, 256 apart, and evaluates every
//                    phase of the interpolator there in the contract's order.  max |x| and max |u| of the tile go to a
//                    partial record.
//   loud_fold_kernel a wavefront per song: the maxima of its tiles' records.  A maximum has no order, so no atomics are needed
//                    and none are used.
#include <stdint.h>

#include "../../include/blissgpu.h"
#include "device_utils.hpp"
#include "internal.hpp"

namespace bg {

namespace {

constexpr int LD_ROW_DWORDS = 32;    // a row's share of a step: 128 bytes
constexpr int LD_PEAK_TILE = 2048;   // interleaved samples per tile of the peak kernel (a multiple of every channel count)
constexpr int LD_PEAK_HALO = 48;     // 24 frames of at most 2 channels
constexpr int LD_PEAK_TAPS = 49;

template <int FMT>
struct LdSample;
template <>
struct LdSample<BLISSGPU_SAMPLE_S16> {
    using type = int16_t;
    static __device__ __forceinline__ double widen(int16_t v) { return (double)v / 32768.0; }
};
template <>
struct LdSample<BLISSGPU_SAMPLE_S32> {
    using type = int32_t;
    static __device__ __forceinline__ double widen(int32_t v) { return (double)v / 2147483648.0; }
};
template <>
struct LdSample<BLISSGPU_SAMPLE_F32> {
    using type = float;
    static __device__ __forceinline__ double widen(float v) { return (double)v; }
};

}  // namespace

template <int FMT, int NCH>
__global__ __launch_bounds__(256) void loud_energy_kernel(const uint8_t* __restrict__ pcm, const LoudSong* __restrict__ songs,
                                                          const uint32_t* __restrict__ song_of, const uint32_t* __restrict__ row_pfx,
                                                          uint32_t n_class, uint32_t n_rows, double* __restrict__ z) {
    using S = LdSample<FMT>;
    using T = typename S::type;
    constexpr int ESZ = (int)sizeof(T);
    constexpr int ROWS = 256 / NCH;                          // rows of a workgroup
    constexpr int FPC = LD_ROW_DWORDS * 4 / (ESZ * NCH);     // frames of a row per step
    constexpr int PITCH = LD_ROW_DWORDS + (ESZ == 4 && NCH == 2 ? 2 : 1);
    __shared__ uint32_t tile[ROWS * PITCH];
    __shared__ const uint32_t* row_src[ROWS];
    __shared__ uint32_t row_dwords[ROWS];
    __shared__ uint32_t steps_max;
    const int t = threadIdx.x;
    const int rl = t / NCH, c = t % NCH;
    const uint32_t row = blockIdx.x * (uint32_t)ROWS + (uint32_t)rl;
    const bool live = row < n_rows;
    if (t == 0) steps_max = 0;
    __syncthreads();

    // the row's geometry: frames [f0, f1) of its song, sub-blocks from u_out on are kept
    uint32_t hop = 1, u = 0, u_out = 0, skew = 0, n_frames = 0;
    double b10 = 0, b11 = 0, b12 = 0, a11 = 0, a12 = 0, b20 = 0, b21 = 0, b22 = 0, a21 = 0, a22 = 0;
    double* zrow = z;
    if (live) {
        const uint32_t k = find_segment(row_pfx, n_class, row);
        const LoudSong& sd = songs[song_of[k]];
        const uint32_t g = row - row_pfx[k];
        hop = sd.hop;
        u_out = g * (uint32_t)BLISSGPU_LOUDNESS_SEGMENT;
        u = u_out > (uint32_t)BLISSGPU_LOUDNESS_WARMUP ? u_out - (uint32_t)BLISSGPU_LOUDNESS_WARMUP : 0u;
        const uint32_t u_end = min(u_out + (uint32_t)BLISSGPU_LOUDNESS_SEGMENT, sd.n_sub);
        const uint64_t f0 = (uint64_t)u * hop, f1 = (uint64_t)u_end * hop;   // f1 <= frames
        const uint64_t b0 = f0 * (uint64_t)(ESZ * NCH), b_al = b0 & ~(uint64_t)3;
        skew = (uint32_t)((b0 - b_al) / (uint64_t)(ESZ * NCH));              // 1 only for mono 16-bit rows that start on an odd frame
        n_frames = (uint32_t)(f1 - f0);                                      // <= (SEGMENT + WARMUP) * hop < 2^32
        if (c == 0) {
            row_src[rl] = reinterpret_cast<const uint32_t*>(pcm + sd.pcm_off + b_al);   // pcm_off is a multiple of 256
            // (the last dword may reach 2 bytes past the song: every song's PCM is padded to 256 bytes)
            row_dwords[rl] = (uint32_t)((f1 * (uint64_t)(ESZ * NCH) - b_al + 3) >> 2);
            atomicMax(&steps_max, (skew + n_frames + (uint32_t)FPC - 1u) / (uint32_t)FPC);
        }
        b10 = sd.coef[0]; b11 = sd.coef[1]; b12 = sd.coef[2]; a11 = sd.coef[3]; a12 = sd.coef[4];
        b20 = sd.coef[5]; b21 = sd.coef[6]; b22 = sd.coef[7]; a21 = sd.coef[8]; a22 = sd.coef[9];
        zrow = z + sd.z_off + (uint64_t)c * sd.n_sub;
    } else if (c == 0) {
        row_src[rl] = nullptr;
        row_dwords[rl] = 0;
    }
    __syncthreads();
    const uint32_t steps = steps_max;
    const T* mine = reinterpret_cast<const T*>(tile + rl * PITCH) + c;

    double s11 = 0.0, s12 = 0.0, s21 = 0.0, s22 = 0.0, acc = 0.0;
    uint32_t left = hop;                     // samples until the current sub-block ends
    const uint32_t e_end = skew + n_frames;  // the row's frames are [skew, e_end) of its aligned stream
    const int ld = t & 31;
    for (uint32_t step = 0; step < steps; step++) {
        const uint32_t d = step * (uint32_t)LD_ROW_DWORDS + (uint32_t)ld;
#pragma unroll 4
        for (int rr = t >> 5; rr < ROWS; rr += 8) tile[rr * PITCH + ld] = d < row_dwords[rr] ? row_src[rr][d] : 0u;
        __syncthreads();
        const uint32_t lo = max(step * (uint32_t)FPC, skew), hi = min((step + 1u) * (uint32_t)FPC, e_end);
        for (uint32_t e = lo; e < hi; e++) {
            const double x = S::widen(mine[(e - step * (uint32_t)FPC) * NCH]);
            const double y1 = b10 * x + s11;
            s11 = (b11 * x - a11 * y1) + s12;
            s12 = b12 * x - a12 * y1;
            const double y2 = b20 * y1 + s21;
            s21 = (b21 * y1 - a21 * y2) + s22;
            s22 = b22 * y1 - a22 * y2;
            acc = acc + y2 * y2;
            if (--left == 0) {
                if (u >= u_out) zrow[u] = acc;
                u++;
                acc = 0.0;
                left = hop;
            }
        }
        __syncthreads();
    }
}

// tile_pfx [n_songs + 1]: tiles in front of every song; part [tiles][2] = max |x|, max |u|
__global__ __launch_bounds__(256) void loud_peak_kernel(const uint8_t* __restrict__ pcm, const LoudSong* __restrict__ songs,
                                                        uint32_t n_songs, const uint32_t* __restrict__ tile_pfx,
                                                        const double* __restrict__ htab, double* __restrict__ part) {
    __shared__ double xs[LD_PEAK_TILE + 2 * LD_PEAK_HALO];
    __shared__ double red[2][256];
    const int t = threadIdx.x;
    const uint32_t s = find_segment(tile_pfx, n_songs, blockIdx.x);
    const LoudSong& sd = songs[s];
    const int nch = (int)sd.channels, fmt = (int)sd.format;
    const int64_t total = (int64_t)sd.frames * nch;   // interleaved samples of the song
    const int64_t first = (int64_t)(blockIdx.x - tile_pfx[s]) * LD_PEAK_TILE;
    const uint8_t* base = pcm + sd.pcm_off;
    for (int i = t; i < LD_PEAK_TILE + 2 * LD_PEAK_HALO; i += 256) {
        const int64_t e = first - LD_PEAK_HALO + i;
        double v = 0.0;
        if (e >= 0 && e < total) {
            if (fmt == BLISSGPU_SAMPLE_S16) v = LdSample<BLISSGPU_SAMPLE_S16>::widen(reinterpret_cast<const int16_t*>(base)[e]);
            else if (fmt == BLISSGPU_SAMPLE_S32) v = LdSample<BLISSGPU_SAMPLE_S32>::widen(reinterpret_cast<const int32_t*>(base)[e]);
            else v = LdSample<BLISSGPU_SAMPLE_F32>::widen(reinterpret_cast<const float*>(base)[e]);
        }
        xs[i] = v;
    }
    __syncthreads();
    // phase p of position n: u = sum over j of h[p + F j] * x[n + 24 / F - j], ascending j; a neighbouring frame is nch samples away
    const int F = (int)sd.factor, reach = (24 / F) * nch;
    const double* __restrict__ h = htab + (F == 4 ? 0 : F == 2 ? 1 : 2) * LD_PEAK_TAPS;
    double sp = 0.0, tp = 0.0;
    const int count = (int)min((int64_t)LD_PEAK_TILE, total - first);
    for (int n = t; n < count; n += 256) {
        const double* at = xs + LD_PEAK_HALO + n;
        sp = fmax(sp, fabs(at[0]));
        for (int p = 0; p < F; p++) {
            double acc = 0.0;
            const double* q = at + reach;
            for (int i = p; i < LD_PEAK_TAPS; i += F, q -= nch) acc = acc + h[i] * q[0];
            tp = fmax(tp, fabs(acc));
        }
    }
    red[0][t] = sp;
    red[1][t] = tp;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) {
            red[0][t] = fmax(red[0][t], red[0][t + w]);
            red[1][t] = fmax(red[1][t], red[1][t + w]);
        }
        __syncthreads();
    }
    if (t == 0) {
        part[2 * (size_t)blockIdx.x] = red[0][0];
        part[2 * (size_t)blockIdx.x + 1] = red[1][0];
    }
}

// one wavefront per song: peaks [n_songs][2] = the maxima of its tiles' records
__global__ __launch_bounds__(64) void loud_fold_kernel(const double* __restrict__ part, const uint32_t* __restrict__ tile_pfx,
                                                       double* __restrict__ peaks) {
    __shared__ double red[2][64];
    const int t = threadIdx.x;
    const uint32_t s = blockIdx.x, t0 = tile_pfx[s], t1 = tile_pfx[s + 1];
    double sp = 0.0, tp = 0.0;
    for (uint32_t k = t0 + (uint32_t)t; k < t1; k += 64u) {
        sp = fmax(sp, part[2 * (size_t)k]);
        tp = fmax(tp, part[2 * (size_t)k + 1]);
    }
    red[0][t] = sp;
    red[1][t] = tp;
    __syncthreads();
    for (int w = 32; w >= 1; w >>= 1) {
        if (t < w) {
            red[0][t] = fmax(red[0][t], red[0][t + w]);
            red[1][t] = fmax(red[1][t], red[1][t + w]);
        }
        __syncthreads();
    }
    if (t == 0) {
        peaks[2 * (size_t)s] = red[0][0];
        peaks[2 * (size_t)s + 1] = red[1][0];
    }
}

template <int FMT, int NCH>
static void launch_energy_class(const uint8_t* pcm, const LoudSong* songs, const uint32_t* song_of, const uint32_t* row_pfx,
                                uint32_t n_class, uint32_t n_rows, double* z, hipStream_t st) {
    constexpr uint32_t ROWS = 256 / NCH;
    hipLaunchKernelGGL((loud_energy_kernel<FMT, NCH>), dim3((n_rows + ROWS - 1) / ROWS), dim3(256), 0, st, pcm, songs, song_of, row_pfx,
                       n_class, n_rows, z);
}

void launch_loud_energy(const uint8_t* pcm, const LoudSong* songs, int format, int channels, const uint32_t* song_of,
                        const uint32_t* row_pfx, uint32_t n_class, uint32_t n_rows, double* z, hipStream_t st) {
    if (n_rows == 0) return;
    if (channels == 1) {
        if (format == BLISSGPU_SAMPLE_S16) launch_energy_class<BLISSGPU_SAMPLE_S16, 1>(pcm, songs, song_of, row_pfx, n_class, n_rows, z, st);
        else if (format == BLISSGPU_SAMPLE_S32) launch_energy_class<BLISSGPU_SAMPLE_S32, 1>(pcm, songs, song_of, row_pfx, n_class, n_rows, z, st);
        else launch_energy_class<BLISSGPU_SAMPLE_F32, 1>(pcm, songs, song_of, row_pfx, n_class, n_rows, z, st);
    } else {
        if (format == BLISSGPU_SAMPLE_S16) launch_energy_class<BLISSGPU_SAMPLE_S16, 2>(pcm, songs, song_of, row_pfx, n_class, n_rows, z, st);
        else if (format == BLISSGPU_SAMPLE_S32) launch_energy_class<BLISSGPU_SAMPLE_S32, 2>(pcm, songs, song_of, row_pfx, n_class, n_rows, z, st);
        else launch_energy_class<BLISSGPU_SAMPLE_F32, 2>(pcm, songs, song_of, row_pfx, n_class, n_rows, z, st);
    }
}

void launch_loud_peak(const uint8_t* pcm, const LoudSong* songs, uint32_t n_songs, const uint32_t* tile_pfx, uint32_t n_tiles,
                      const double* htab, double* part, hipStream_t st) {
    if (n_tiles == 0) return;
    hipLaunchKernelGGL(loud_peak_kernel, dim3(n_tiles), dim3(256), 0, st, pcm, songs, n_songs, tile_pfx, htab, part);
}

void launch_loud_fold(const double* part, const uint32_t* tile_pfx, uint32_t n_songs, double* peaks, hipStream_t st) {
    if (n_songs == 0) return;
    hipLaunchKernelGGL(loud_fold_kernel, dim3(n_songs), dim3(64), 0, st, part, tile_pfx, peaks);
}

uint32_t loud_peak_tiles(uint64_t frames, uint32_t channels) {
    return (uint32_t)((frames * channels + LD_PEAK_TILE - 1) / LD_PEAK_TILE);
}

}  // namespace bg
