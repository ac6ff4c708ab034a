// kernels_fingerprint.hip -- acoustic fingerprints (include/blissgpu.h): the Haitsma-Kalker sub-fingerprints
// of a song's 22 050 Hz mono PCM, and the alignment search that matches two fingerprints (compiled with -ffp-contract=off).
//
//   fp_bands_kernel  one 256-thread workgroup per run of FP_RUN consecutive frames of one song.  A frame is samples
//                    [512 f, 512 f + 8192): consecutive frames share 15/16 of their samples, so the run's 8192 + 512 (FP_RUN - 1)
//                    samples are staged in LDS once and every frame is windowed out of that copy.  The transform is the
//                    project's FFT-8192: 8192 reals packed as 4096 complex values, three radix16() passes with
//                    two padded LDS transposes, then the real-input split -- for bins 111 .. 742 only: Z[k] and Z[4096 - k] of
//                    those bins live in six of the sixteen output rows, the other ten are never written back.  The window
//                    table holds HALF the Hann window, so A + P of the split is X itself.  Every bin's energy
//                    (double)re^2 + (double)im^2 goes through LDS to the 33 lanes that sum a band each, in ascending bin order.
//                    FP_RUN = 6: 42.0 KiB of samples + 34.0 KiB exchange buffer + 2 KiB twiddles = 78 KiB, two workgroups per CU
//                    (three would leave 17 KiB for the samples: less than one frame; a longer run drops to one workgroup, four
//                    wavefronts that all wait at the same seven barriers per frame: 1.57 times the time at 16).
//   fp_bits_kernel   a lane owns a word: bit b = ((E[t][b] - E[t][b+1]) - (E[t-1][b] - E[t-1][b+1])) > 0, in this association.
//   fp_match_kernel  one workgroup per (pair, block of 256 offsets); a lane owns an offset.  The a words and the b window of
//                    FM_T + 255 words of a chunk are staged in LDS, zero where they leave their song: a zero word is invalid by
//                    the contract, so the padding needs no bounds logic in the loop.  a[t] is a broadcast read, b[t + o] a
//                    consecutive one.  The workgroup's best offset (exact u64 comparison, ties to the smaller (|o|, o): a strict
//                    total order, so the tree's shape does not matter) is its candidate.
//   fp_pick_kernel   a lane owns a pair: the best of its offset blocks' candidates under the same order.
#include <stdint.h>

#include "device_utils.hpp"
#include "fft_r16.hpp"
#include "internal.hpp"

namespace bg {

__device__ constexpr uint16_t FP_EDGE_TABLE[FP_BANDS + 1] = {FP_EDGE_LIST};
constexpr int FP_K0 = 111, FP_K1 = 743;      // bins [FP_K0, FP_K1) carry the 33 bands
constexpr int FP_EX1_PITCH = 257;            // first transpose: k1-major rows of 256 (+1)
constexpr int FP_EX2_PITCH = 272;            // second transpose: j1-major rows of 256 (+16)
constexpr int FP_EX = 16 * FP_EX2_PITCH;     // complex slots of the exchange buffer (34 816 B)
constexpr int FP_SAMPLES = FP_FRAME + FP_HOP * (FP_RUN - 1);
static_assert(FP_K1 - FP_K0 <= 3 * 256, "a thread splits at most three bins");
static_assert((FP_K1 - 1) >> 8 == 2 && (4096 - (FP_K1 - 1)) >> 8 == 13, "the bins and their mirrors lie in rows 0..2 and 13..15");
static_assert((FP_K1 - FP_K0) * sizeof(double) <= FP_EX * sizeof(f2), "the energies fit the exchange buffer");
static_assert(FP_SAMPLES * 4 + FP_EX * 8 + 256 * 8 <= 80 * 1024, "two workgroups per CU");

__global__ __launch_bounds__(256, 2) void fp_bands_kernel(const float* __restrict__ pcm, const FpSong* __restrict__ songs,
                                                          uint32_t n_songs, const uint32_t* __restrict__ run_pfx,
                                                          const float* __restrict__ hann, const float2* __restrict__ tw,
                                                          double* __restrict__ E) {
    __shared__ __attribute__((aligned(16))) float smp[FP_SAMPLES];
    __shared__ __attribute__((aligned(16))) f2 lds[FP_EX];
    __shared__ __attribute__((aligned(16))) f2 tw256[256];  // W_256^(m k) at [16 m + k]
    const int t = threadIdx.x;
    const int lo4 = t & 15, hi4 = t >> 4;
    const uint32_t s = find_segment(run_pfx, n_songs, blockIdx.x);
    const FpSong sd = songs[s];
    const uint32_t f_first = (blockIdx.x - run_pfx[s]) * (uint32_t)FP_RUN;
    const uint32_t nf = min((uint32_t)FP_RUN, sd.frames - f_first);  // >= 1: the song has ceil(frames / FP_RUN) runs
    {
        const float2 a = tw[32 * ((hi4 * lo4) & 255)];
        tw256[t] = mk(a.x, a.y);
    }
    // the run's samples, once: the last frame ends at 512 (f_first + nf - 1) + 8192 <= n, so every index is inside the song
    const float* __restrict__ x = pcm + sd.pcm_off + (uint64_t)f_first * FP_HOP;
    const int count = FP_FRAME + FP_HOP * ((int)nf - 1);
    for (int i = t; i < count; i += 256) smp[i] = x[i];
    // the (halved) window of this thread's 16 complex inputs z[256 n1 + t] = (x[2 (256 n1 + t)], x[2 (256 n1 + t) + 1])
    f2 win[16];
#pragma unroll
    for (int n1 = 0; n1 < 16; n1++) {
        const float2 w = reinterpret_cast<const float2*>(hann)[256 * n1 + t];
        win[n1] = mk(w.x, w.y);
    }
    f2 c_p2;  // W_4096^(m2 k1) of pass 2
    {
        const float2 a = tw[2 * hi4 * lo4];
        c_p2 = mk(a.x, a.y);
    }
    // the bins this thread splits: k = FP_K0 + t + 256 i, and their W_8192^k
    f2 wk[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int k = FP_K0 + t + 256 * i;
        const float2 a = tw[k < FP_K1 ? k : 0];
        wk[i] = mk(a.x, a.y);
    }
    double* const en = reinterpret_cast<double*>(lds);  // the bins' energies, over the dead exchange buffer
    __syncthreads();

#pragma unroll 1
    for (uint32_t fi = 0; fi < nf; fi++) {
        const f2* __restrict__ fr = reinterpret_cast<const f2*>(smp + FP_HOP * fi);
        f2 v[16];
#pragma unroll
        for (int n1 = 0; n1 < 16; n1++) v[n1] = fr[256 * n1 + t] * win[n1];  // the window product, rounded to f32
        // ---- pass 1: DFT over n1 at n2 = t = 16 m1 + m2; twiddle W_256^(m1 k1) ----
        radix16(v);
#pragma unroll
        for (int k1 = 1; k1 < 16; k1++) v[R16(k1)] = cmul_pk(v[R16(k1)], tw256[16 * hi4 + k1]);
#pragma unroll
        for (int k1 = 0; k1 < 16; k1++) lds[k1 * FP_EX1_PITCH + t] = v[R16(k1)];
        __syncthreads();
        // ---- pass 2: thread (k1 = lo4, m2 = hi4): DFT over m1; twiddle W_4096^(m2 k1) W_256^(m2 j1) ----
#pragma unroll
        for (int m1 = 0; m1 < 16; m1++) v[m1] = lds[lo4 * FP_EX1_PITCH + 16 * m1 + hi4];
        radix16(v);
        v[R16(0)] = cmul_pk(v[R16(0)], c_p2);
#pragma unroll
        for (int j1 = 1; j1 < 16; j1++) v[R16(j1)] = cmul_pk(v[R16(j1)], cmul_pk(tw256[16 * hi4 + j1], c_p2));
        __syncthreads();  // every read of the first transpose is done
#pragma unroll
        for (int j1 = 0; j1 < 16; j1++) lds[j1 * FP_EX2_PITCH + t] = v[R16(j1)];
        __syncthreads();
        // ---- pass 3: thread (k1 = lo4, j1 = hi4): DFT over m2 -> Z[t + 256 j2] ----
#pragma unroll
        for (int m2 = 0; m2 < 16; m2++) v[m2] = lds[hi4 * FP_EX2_PITCH + 16 * m2 + lo4];
        radix16(v);
        __syncthreads();  // every read of the second transpose is done
        // rows 0..2 hold bins 0..767, rows 13..15 their mirrors 3328..4095: row j2 goes to slot j2 (< 3) or j2 - 10
#pragma unroll
        for (int j2 = 0; j2 < 3; j2++) {
            lds[t + 256 * j2] = v[R16(j2)];
            lds[t + 256 * (j2 + 3)] = v[R16(j2 + 13)];
        }
        __syncthreads();
        // ---- real-input split: X[k] = A + P, A = zk + conj(zm), P = W_8192^k (-i) (zk - conj(zm)) ----
        double e[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int k = FP_K0 + t + 256 * i;
            e[i] = 0.0;
            if (k < FP_K1) {
                const int km = 4096 - k;
                const f2 zk = lds[k], zm = lds[km - 2560];  // (km >> 8) - 10 rows down
                const float ax = zk.x + zm.x, ay = zk.y - zm.y, bx = zk.x - zm.x, by = zk.y + zm.y;
                const float px = by * wk[i].x + bx * wk[i].y, py = by * wk[i].y - bx * wk[i].x;
                const float re = ax + px, im = ay + py;
                e[i] = (double)re * (double)re + (double)im * (double)im;
            }
        }
        __syncthreads();  // every read of Z is done: the energies take its place
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int k = FP_K0 + t + 256 * i;
            if (k < FP_K1) en[k - FP_K0] = e[i];
        }
        __syncthreads();
        if (t < FP_BANDS) {
            double sum = 0.0;
            for (int k = FP_EDGE_TABLE[t]; k < FP_EDGE_TABLE[t + 1]; k++) sum += en[k - FP_K0];
            E[((uint64_t)sd.row0 + f_first + fi) * FP_BANDS + t] = sum;
        }
        __syncthreads();  // the next frame's first transpose overwrites the energies
    }
}

__global__ __launch_bounds__(256) void fp_bits_kernel(const double* __restrict__ E, const uint32_t* __restrict__ word_pfx,
                                                      uint32_t n_songs, uint32_t n_words, uint32_t* __restrict__ words) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= n_words) return;
    // song s of the group has word_pfx[s + 1] - word_pfx[s] words and one frame more: its rows begin at word_pfx[s] + s
    const uint32_t s = find_segment(word_pfx, n_songs, w);
    const double* __restrict__ e0 = E + ((uint64_t)w + s) * FP_BANDS;  // frame t - 1
    const double* __restrict__ e1 = e0 + FP_BANDS;                      // frame t
    uint32_t bits = 0;
    double p0 = e0[0], p1 = e1[0];
#pragma unroll
    for (int b = 0; b < 32; b++) {
        const double q0 = e0[b + 1], q1 = e1[b + 1];
        const double m = (p1 - q1) - (p0 - q0);
        bits |= (m > 0.0 ? 1u : 0u) << b;
        p0 = q0;
        p1 = q1;
    }
    words[w] = bits;
}

// ---- the match ----
constexpr int FM_T = 1024;  // a words per staged chunk

// (e1, v1, o1) before (e2, v2, o2): the smaller errors / bits (bits = 32 v), then the smaller (|o|, o)
__device__ __forceinline__ bool fp_before(uint32_t e1, uint32_t v1, int o1, uint32_t e2, uint32_t v2, int o2) {
    const uint64_t l = (uint64_t)e1 * v2, r = (uint64_t)e2 * v1;
    if (l != r) return l < r;
    const int a1 = o1 < 0 ? -o1 : o1, a2 = o2 < 0 ? -o2 : o2;
    if (a1 != a2) return a1 < a2;
    return o1 < o2;
}
// the better of two candidates; valid == 0 loses to anything valid
__device__ __forceinline__ FpCand fp_better(const FpCand& a, const FpCand& b) {
    if (!b.valid) return a;
    if (!a.valid) return b;
    return fp_before(b.errors, b.count, b.offset, a.errors, a.count, a.offset) ? b : a;
}

__global__ __launch_bounds__(256) void fp_match_kernel(const uint32_t* __restrict__ words, const uint64_t* __restrict__ word_offsets,
                                                       uint32_t n_songs, const uint32_t* __restrict__ pairs, uint32_t n_blocks,
                                                       int max_offset, uint32_t min_overlap, FpCand* __restrict__ cand) {
    __shared__ uint32_t a_s[FM_T];
    __shared__ uint32_t b_s[FM_T + 256];
    __shared__ FpCand red[256];
    const int t = threadIdx.x;
    const uint32_t pair = blockIdx.x / n_blocks, ob = blockIdx.x % n_blocks;
    const uint32_t ia = pairs[2 * (size_t)pair], ib = pairs[2 * (size_t)pair + 1];
    FpCand mine{0u, 0u, 0, 0u};
    if (ia >= n_songs || ib >= n_songs) {  // (the host form refuses such a pair before the launch)
        if (t == 0) cand[blockIdx.x] = mine;
        return;
    }
    const uint32_t* __restrict__ a = words + word_offsets[ia];
    const uint32_t* __restrict__ b = words + word_offsets[ib];
    const long la = (long)(word_offsets[ia + 1] - word_offsets[ia]), lb = (long)(word_offsets[ib + 1] - word_offsets[ib]);
    const long o_first = -(long)max_offset + 256L * ob;
    const long o = o_first + t;
    // positions any of the block's offsets can use: 0 <= t' < la and 0 <= t' + o' < lb for some o' in [o_first, o_first + 255]
    const long t_lo = max(0L, -(o_first + 255)), t_hi = min(la, lb - o_first);
    uint32_t errors = 0, count = 0;
    for (long t0 = t_lo; t0 < t_hi; t0 += FM_T) {
        const int len = (int)min((long)FM_T, t_hi - t0);
        for (int i = t; i < len; i += 256) a_s[i] = a[t0 + i];  // t0 + i < t_hi <= la
        for (int j = t; j < len + 255; j += 256) {
            const long q = t0 + o_first + j;
            b_s[j] = (q >= 0 && q < lb) ? b[q] : 0u;
        }
        __syncthreads();
#pragma unroll 8
        for (int i = 0; i < len; i++) {
            const uint32_t av = a_s[i], bv = b_s[i + t];
            const bool ok = av != 0u && bv != 0u;
            errors += ok ? (uint32_t)__popc(av ^ bv) : 0u;
            count += ok ? 1u : 0u;
        }
        __syncthreads();
    }
    if (o <= (long)max_offset && count >= min_overlap) mine = FpCand{errors, count, (int)o, 1u};
    red[t] = mine;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) red[t] = fp_better(red[t], red[t + w]);
        __syncthreads();
    }
    if (t == 0) cand[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void fp_pick_kernel(const FpCand* __restrict__ cand, uint32_t n_pairs, uint32_t n_blocks,
                                                      int32_t* __restrict__ offset, uint32_t* __restrict__ errors,
                                                      uint32_t* __restrict__ bits) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n_pairs) return;
    FpCand best{0u, 0u, 0, 0u};
    for (uint32_t k = 0; k < n_blocks; k++) best = fp_better(best, cand[(size_t)p * n_blocks + k]);
    offset[p] = best.valid ? best.offset : 0;
    errors[p] = best.valid ? best.errors : 0u;
    bits[p] = best.valid ? 32u * best.count : 0u;
}

void launch_fp_bands(const float* pcm, const FpSong* songs, uint32_t n_songs, const uint32_t* run_pfx, uint32_t n_runs,
                     const float* hann, const float2* tw, double* E, hipStream_t st) {
    if (n_runs == 0) return;
    hipLaunchKernelGGL(fp_bands_kernel, dim3(n_runs), dim3(256), 0, st, pcm, songs, n_songs, run_pfx, hann, tw, E);
}

void launch_fp_bits(const double* E, const uint32_t* word_pfx, uint32_t n_songs, uint32_t n_words, uint32_t* words, hipStream_t st) {
    if (n_words == 0) return;
    hipLaunchKernelGGL(fp_bits_kernel, dim3((n_words + 255u) / 256u), dim3(256), 0, st, E, word_pfx, n_songs, n_words, words);
}

void launch_fp_match(const uint32_t* words, const uint64_t* word_offsets, uint32_t n_songs, const uint32_t* pairs, uint32_t n_pairs,
                     uint32_t n_blocks, int max_offset, uint32_t min_overlap, FpCand* cand, hipStream_t st) {
    if (n_pairs == 0) return;
    hipLaunchKernelGGL(fp_match_kernel, dim3(n_pairs * n_blocks), dim3(256), 0, st, words, word_offsets, n_songs, pairs, n_blocks,
                       max_offset, min_overlap, cand);
}

void launch_fp_pick(const FpCand* cand, uint32_t n_pairs, uint32_t n_blocks, int32_t* offset, uint32_t* errors, uint32_t* bits,
                    hipStream_t st) {
    if (n_pairs == 0) return;
    hipLaunchKernelGGL(fp_pick_kernel, dim3((n_pairs + 255u) / 256u), dim3(256), 0, st, cand, n_pairs, n_blocks, offset, errors, bits);
}

}  // namespace bg
