// kernels_pairwise.hip -- all-pairs feature-vector distances (compiled with -ffp-contract=off).
//
// Reference (src/playlist.rs):
//   euclidean_distance   :65-71   (a-b).dot(eye).dot(a-b).sqrt()
//   cosine_distance      :76-79   1 - a.b / (sqrt(a.a) * sqrt(b.b))
//   mahalanobis_distance :140-142 (a-b).dot(M).dot(a-b).sqrt()        (default metric: lib.rs:168-178)
// The f32 results are pinned by `assert_eq` literals (playlist.rs:1023,1088,1104; lib.rs:280,289), the
// last of which (3.4999998) depends on ndarray's summation order, so the kernel reproduces it:
//   * Array1.dot(Array2) walks each (strided) column with a plain sequential sum;
//   * Array1.dot(Array1) is `unrolled_dot`: 8 partial sums, combined (p0+p4)+(p1+p5)+(p2+p6)+(p3+p7),
//     then the <8 tail elements sequentially.
// With M = I (or any diagonal M) the vector-matrix product degenerates exactly to an element-wise
// product, which is the fast path.
//
// 4 bytes per pair out, 4*d*(n+m) bytes in.  A workgroup owns 256 columns -- each lane keeps 4 column vectors in
// registers -- and walks PW_RT tiles of 128 rows down them (round 6: the columns are 92 strided loads per lane and used
// to be reloaded for every tile); rows come from LDS as broadcasts, and every wave-store is 64 lanes x 16 B = 1 KiB of
// one output row.  Bound by the vector ALU, not by its stores (profiles/r06_pairwise_staging_ab.txt: the self-distance
// kernel takes 7.6 of its 9.75 ms with every store removed): 136 packed operations + four correctly rounded square
// roots (a quarter-rate instruction each) per four outputs is what the reference's summation order costs.
#include <stdlib.h>

#include <type_traits>

#include "device_utils.hpp"
#include "internal.hpp"
#include "pairwise_math.hpp"

namespace bg {

constexpr int PW_ROWS = 128, PW_COLS = 256, PW_CPT = 4;  // tile rows, tile cols, cols per thread
#ifndef PW_RT
#define PW_RT 8   // 128-row tiles a workgroup walks with its 256 columns in registers (even: the self-distance kernel works in 256 x 256 blocks)
#endif
// an index every lane of the wavefront computed alike, moved to scalar registers: with a 32-bit lane offset on top the store
// takes the `saddr + voffset` form and no lane keeps a 64-bit address (two VGPRs each) across the arithmetic
__device__ __forceinline__ uint64_t wave_uniform(uint64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// Correctly rounded sqrt (what Rust's f32::sqrt / the oracle's sqrtf return) for the two halves of a pair.
// v_sqrt_f32 is within 1 ulp; the exact residuals against the two neighbours (one FMA each) pick the correctly
// rounded value -- the compiler's own sqrtf expansion minus its input scaling for x < 2^-96, which v_sqrt_f32
// needs because it does not take denormal inputs.  The rare tiny inputs (and only those) use sqrtf; 0, inf and
// NaN come out right (NaN residuals fail both comparisons).
__device__ __forceinline__ float sqrt_rn_fast(float x) {
    const float r = __builtin_amdgcn_sqrtf(x);
    const float rd = __uint_as_float(__float_as_uint(r) - 1u), ru = __uint_as_float(__float_as_uint(r) + 1u);
    const float vp = __builtin_fmaf(-rd, r, x), vs = __builtin_fmaf(-ru, r, x);
    float o = (vp <= 0.0f) ? rd : r;
    o = (vs > 0.0f) ? ru : o;
    return o;
}
__device__ __forceinline__ f2 sqrt_rn2(f2 x) {
    f2 r;
    const bool tiny = (x.x < 0x1p-96f && x.x != 0.0f) || (x.y < 0x1p-96f && x.y != 0.0f);
    if (__builtin_expect(__ballot(tiny) != 0ull, 0)) {  // wave-uniform
        r.x = sqrtf(x.x);
        r.y = sqrtf(x.y);
    } else {
        r.x = sqrt_rn_fast(x.x);
        r.y = sqrt_rn_fast(x.y);
    }
    return r;
}


// SYM: A and B are the same matrix.  Every metric here is symmetric bit for bit (negating a - b leaves its squares, the
// quadratic form and the dot products unchanged, and both norm tables come from the same rows), so only the 256 x 256
// blocks on or above the diagonal are computed; an off-diagonal block is also written transposed, 32 rows at a time
// through an LDS tile so that the transposed stores are 128-byte runs.
template <int D, int METRIC, bool DIAG, bool SYM = false>
__global__ __launch_bounds__(256, (METRIC == METRIC_EUCLIDEAN ? 3 : 2)) void pairwise_kernel(const float* __restrict__ A, uint64_t n,
                                                       const float* __restrict__ B, uint64_t m,
                                                       const float* __restrict__ M, float* __restrict__ out,
                                                       uint64_t ld_out) {
    constexpr int DP = (D + 3) & ~3;  // LDS row pitch: 16-byte aligned rows -> ds_read_b128 broadcasts
    __shared__ __attribute__((aligned(16))) float sa[PW_ROWS][DP];
    __shared__ float sna[PW_ROWS];
    __shared__ float sm[(METRIC == METRIC_MAHALANOBIS) ? D * D : 1];
    constexpr int T_ROWS = 32;  // rows staged per transposed write
    // The tile is staged as computed, st[row][column]: a lane's four outputs of a row are 16 consecutive bytes (two 8-byte LDS
    // stores, no four-lanes-to-a-bank conflicts); the transposition happens on the reading side.  Pitch 258 words: row r starts
    // at bank 2 r, so the 8 x 8 lanes of a wavefront that assemble eight 128-byte runs (lane = 8 * column + chunk, words at rows
    // 4 chunk + q) fall on banks 8 chunk + 2 q + column: all different.
    // (Rounds 3 - 5 staged the tile transposed, st[column][row] with an odd pitch: four lanes to a bank on the storing side, 38 %
    // of the kernel's LDS cycles.  Three conflict-free forms of THAT tile lost 10 % each -- every one of them paid for its
    // addresses with vector-ALU instructions, which is what this kernel is short of.  The row-major tile needs none.  A form that
    // pipelines the mirrored stores of one 16-row group into the row loop of the next was built and is slower, 10.3 against
    // 9.8 ms.  Both measured in profiles/r06_pairwise_staging_ab.txt, both kept in tests/tools/probes/lab_switches/.)
    constexpr int ST_PITCH = PW_COLS + 2;
    __shared__ __attribute__((aligned(16))) float st[SYM ? T_ROWS * ST_PITCH : 1];
    auto st_at = [&](int col, int row) -> float& { return st[row * ST_PITCH + col]; };
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const uint32_t bj = blockIdx.x;  // 256-column block
    bool do_t = false;               // this tile's block lies above the diagonal: it is also written transposed
    // A workgroup walks RT row tiles of 128 rows with ITS columns kept in registers (round 6): the columns are 92 strided 4-byte
    // loads per lane, the same in all four wavefronts -- as much traffic through the CU's load path as 40 rows of arithmetic --
    // and were reloaded for every 128 rows.
    constexpr int RT = PW_RT;
    static_assert(RT % (PW_COLS / PW_ROWS) == 0, "a workgroup of the self-distance kernel walks whole 256 x 256 blocks");
    uint64_t i0 = (uint64_t)blockIdx.y * PW_ROWS * RT;
    if (SYM && i0 / PW_COLS > bj) return;  // every block of this workgroup lies below the diagonal: mirrored from above
    const uint64_t j0 = (uint64_t)blockIdx.x * PW_COLS + (uint64_t)lane * PW_CPT;
    uint64_t rows_here = 0;
    if (METRIC == METRIC_MAHALANOBIS) {
        for (int e = tid; e < D * D; e += 256) sm[e] = M[e];
        __syncthreads();
    }

    // the lane's 4 column vectors as two packed pairs: bp[h][k] = (B[j0+2h][k], B[j0+2h+1][k])
    f2 bp[2][D];
    f2 nb[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const uint64_t ja = j0 + 2 * h, jb = ja + 1;
#pragma unroll
        for (int k = 0; k < D; k++) {
            bp[h][k].x = (ja < m) ? B[ja * D + k] : 0.0f;
            bp[h][k].y = (jb < m) ? B[jb * D + k] : 0.0f;
        }
        if (METRIC == METRIC_COSINE) {
            const f2 q = unrolled_dot2<D>([&](int k) { return bp[h][k]; }, [&](int k) { return bp[h][k]; });
            nb[h].x = sqrtf(q.x);
            nb[h].y = sqrtf(q.y);
        }
    }
    float wdiag[D];
#pragma unroll
    for (int k = 0; k < D; k++) wdiag[k] = DIAG ? sm[(k * D + k) % (METRIC == METRIC_MAHALANOBIS ? D * D : 1)] : 0.0f;

    const bool vec_ok = ((ld_out & 3) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0) && (j0 + 3 < m);
    // ---- one row of the tile against the lane's four columns, in pieces so that the loop below can put the tail of one row (the
    // correctly rounded square root: a quarter-rate instruction and two dependent steps behind it) beside the packed arithmetic
    // of the next.  Measured: 0.7 % (profiles/r06_pairwise_two_rows_ab.txt) -- with three wavefronts per SIMD the latencies at
    // the head and the tail of a row were already covered; kept for the A != B Euclidean form, where it costs no registers.
    typedef float f4 __attribute__((ext_vector_type(4)));
    constexpr bool PIPELINED = METRIC == METRIC_EUCLIDEAN && !SYM;  // (the other forms spill at three waves per SIMD)
    auto load_row = [&](f2 (&ap)[DP / 2], int r) __attribute__((always_inline)) {
#pragma unroll
        for (int k4 = 0; k4 < DP / 4; k4++) {  // same address in every lane: LDS broadcast
            const float4 q = *reinterpret_cast<const float4*>(&sa[r][4 * k4]);
            ap[2 * k4].x = q.x; ap[2 * k4].y = q.y; ap[2 * k4 + 1].x = q.z; ap[2 * k4 + 1].y = q.w;
        }
    };
    // the reference's sum for the two columns of pair h (before the square root / the cosine's division)
    auto row_sum = [&](const f2 (&ap)[DP / 2], auto hc) __attribute__((always_inline)) -> f2 {
        return pair_sum<D, METRIC, DIAG>(ap, bp[decltype(hc)::value], wdiag, sm);
    };
    // sum -> distance, the branch-free part (exact unless one of the four sums is a tiny positive number: fix_row)
    auto finish_fast = [&](f2 sum, int h, int r) __attribute__((always_inline)) -> f2 {
        if (METRIC == METRIC_COSINE) return splat(1.0f) - sum / (splat(sna[r]) * nb[h]);
        f2 q;
        q.x = sqrt_rn_fast(sum.x);
        q.y = sqrt_rn_fast(sum.y);
        return q;
    };
    // v_sqrt_f32 does not take denormal inputs: a row with a sum below 2^-96 goes the long way (sqrtf), wave-uniformly.  The test
    // is one unsigned minimum over the four bit patterns -- x in [0, 2^-96) <=> bits(x) < bits(2^-96); inf / NaN / negative sums are
    // large -- and lets ZERO take the long way too (it comes out right there, and a zero distance is a duplicate song: rare).
    // Only the diagonal blocks of a self-distance matrix hold a zero in every row; there (zero_is_common, workgroup-uniform) the
    // test excludes it as rounds 3 - 6 did everywhere: x in (0, 2^-96) <=> bits(x) - 1 < bits(2^-96) - 1, a subtraction per sum.
    bool zero_is_common = false;
    auto is_tiny = [&](f2 a, f2 b) __attribute__((always_inline)) -> bool {
        if (METRIC == METRIC_COSINE) return false;
        if (zero_is_common) {
            const uint32_t lo = min(min(__float_as_uint(a.x) - 1u, __float_as_uint(a.y) - 1u), min(__float_as_uint(b.x) - 1u, __float_as_uint(b.y) - 1u));
            return lo < 0x0F800000u - 1u;
        }
        const uint32_t lo = min(min(__float_as_uint(a.x), __float_as_uint(a.y)), min(__float_as_uint(b.x), __float_as_uint(b.y)));
        return lo < 0x0F800000u;
    };
    auto slow_roots = [&](f2 s) __attribute__((always_inline)) -> f2 { f2 q; q.x = sqrtf(s.x); q.y = sqrtf(s.y); return q; };
    auto emit_row = [&](int r, int R0, f2 q0, f2 q1) __attribute__((always_inline)) {
        // (self-distance form: r is the wavefront's row in a scalar register, the row pointer scalar arithmetic + the lane's 16 bytes)
        float* orow = SYM ? out + wave_uniform((i0 + r) * ld_out + (uint64_t)bj * PW_COLS) + (uint32_t)(lane * PW_CPT)
                          : out + (i0 + r) * ld_out + j0;
        if (vec_ok) {
            f4 q4;
            q4.x = q0.x; q4.y = q0.y; q4.z = q1.x; q4.w = q1.y;
            // written once, never re-read here: non-temporal (plain stores, direct or mirrored, are 2 - 5 % slower:
            // profiles/r06_pairwise_staging_ab.txt, tests/tools/probes/lab_switches/)
            __builtin_nontemporal_store(q4, reinterpret_cast<f4*>(__builtin_assume_aligned(orow, 16)));
        } else {
            const float res[PW_CPT] = {q0.x, q0.y, q1.x, q1.y};
#pragma unroll
            for (int c = 0; c < PW_CPT; c++)
                if (j0 + c < m) orow[c] = res[c];
        }
        if (do_t) {
            f2* d2 = reinterpret_cast<f2*>(__builtin_assume_aligned(&st_at(PW_CPT * lane, r - R0), 8));
            d2[0] = q0;
            d2[1] = q1;
        }
    };
    for (int t = 0; t < RT && i0 < n; t++, i0 += PW_ROWS) {
    if (SYM) {
        const uint32_t bi = (uint32_t)(i0 / PW_COLS);  // block row of this tile
        if (bi > bj) break;                            // mirrored from the block (bj, bi)
        do_t = bj > bi;
        zero_is_common = bi == bj;
    }
    // stage the row tile and, for cosine, the row norms
    if (t) __syncthreads();  // every wavefront has finished with the previous tile's rows
    rows_here = (n - i0 < (uint64_t)PW_ROWS) ? n - i0 : (uint64_t)PW_ROWS;
    {
        // (the thread index made opaque per tile: otherwise the per-lane 64-bit source pointer of this loop is computed once, kept
        // across the arithmetic of all eight tiles -- and spilled, at three wavefronts per SIMD; see the note on the wavefront's index below)
        int t0 = tid;
        if (SYM) asm volatile("" : "+v"(t0));
        for (int e = t0; e < (int)rows_here * D; e += 256) sa[e / D][e % D] = A[i0 * D + e];
    }
    __syncthreads();
    if (METRIC == METRIC_COSINE) {
        if (tid < (int)rows_here) {
            const float* a = sa[tid];
            sna[tid] = sqrtf(unrolled_dot<D>([&](int k) { return a[k]; }, [&](int k) { return a[k]; }));
        }
        __syncthreads();
    }
    // The wavefront's index in a SCALAR register, re-made per tile: everything derived from it (the LDS address of its rows, the
    // row pointer of its direct stores) is then scalar arithmetic per row instead of per-lane 64-bit values computed once and
    // kept -- at three wavefronts per SIMD those were spilled, and the compiler's wait for a reloaded value sat inside the group
    // loop as `s_waitcnt vmcnt(0)`; on gfx950 that counter also holds the wavefront's STORES, so every 32 rows a wavefront stood
    // still until the 16 KiB it had just written were acknowledged by memory.
    int wave_u = wave;
    if (SYM) {
        int w = wave;
        asm volatile("" : "+v"(w));  // (opaque: re-made in this tile, not hoisted to the top of the kernel and carried)
        wave_u = __builtin_amdgcn_readfirstlane(w);
    }
    for (int R0 = 0; R0 < (int)rows_here; R0 += T_ROWS) {
    {
        const int r_end = ((int)rows_here < R0 + T_ROWS) ? (int)rows_here : R0 + T_ROWS;
        int r = R0 + wave_u;
        if (PIPELINED) {
            // two rows per trip, in ONE basic block: the first row's square roots are independent of the second row's 136
            // packed operations (and its LDS reads of the first row's last differences), so the scheduler overlaps them
#pragma unroll 1
            for (; r + 4 < r_end; r += 8) {
                f2 ap[DP / 2];  // the row, two features per register pair
                load_row(ap, r);
                const f2 sa0 = row_sum(ap, std::integral_constant<int, 0>{}), sa1 = row_sum(ap, std::integral_constant<int, 1>{});
                load_row(ap, r + 4);
                f2 qa0 = finish_fast(sa0, 0, r), qa1 = finish_fast(sa1, 1, r);
                const f2 sb0 = row_sum(ap, std::integral_constant<int, 0>{}), sb1 = row_sum(ap, std::integral_constant<int, 1>{});
                f2 qb0 = finish_fast(sb0, 0, r + 4), qb1 = finish_fast(sb1, 1, r + 4);
                const bool tiny = is_tiny(sa0, sa1) || is_tiny(sb0, sb1);
                if (__builtin_expect(__ballot(tiny) != 0ull, 0)) {  // wave-uniform, next to never
                    qa0 = slow_roots(sa0); qa1 = slow_roots(sa1); qb0 = slow_roots(sb0); qb1 = slow_roots(sb1);
                }
                emit_row(r, R0, qa0, qa1);
                emit_row(r + 4, R0, qb0, qb1);
            }
        }
#pragma unroll 1
        for (; r < r_end; r += 4) {   // (the odd row of a ragged tile; every row of the general-M form)
            f2 ap[DP / 2];
            load_row(ap, r);
            const f2 s0 = row_sum(ap, std::integral_constant<int, 0>{}), s1 = row_sum(ap, std::integral_constant<int, 1>{});
            f2 q0 = finish_fast(s0, 0, r), q1 = finish_fast(s1, 1, r);
            if (__builtin_expect(__ballot(is_tiny(s0, s1)) != 0ull, 0)) { q0 = slow_roots(s0); q1 = slow_roots(s1); }  // wave-uniform; ONE test per row
            emit_row(r, R0, q0, q1);
        }
    }
    if (do_t) {  // workgroup-uniform
        __syncthreads();
        // mirrored block: its row bj * 256 + j holds the staged column j, 32 consecutive outputs = one 128-byte run,
        // assembled by 8 consecutive lanes (16 bytes each) so that every store instruction writes whole lines
        const int nvalid = ((int)rows_here - R0 < T_ROWS) ? (int)rows_here - R0 : T_ROWS;
        const bool fast = nvalid == T_ROWS && ((ld_out & 3) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
        constexpr int LPR = T_ROWS / 4, JPP = 256 / LPR;  // lanes per run of T_ROWS floats, runs per pass of the workgroup
        const int chunk = tid % LPR;
        // every run of the pass read from the tile back to back, then stored: one LDS round trip per 32-row group instead
        // of one per run (the loop below waits for each run's words before it stores them)
        if (fast && ((uint64_t)bj + 1) * PW_COLS <= m && ld_out < (1ull << 26)) {  // (32 rows x ld_out floats stay below 2^32 bytes)
            // uniform part in scalar registers, the lane's part (row tid / LPR of the pass, four floats at 4 * chunk) in 32 bits
            int t1 = tid;
            asm volatile("" : "+v"(t1));  // (the lane's offset computed here, not once and held -- spilled -- across the arithmetic)
            const uint32_t lane_off = (uint32_t)(t1 / LPR) * (uint32_t)ld_out + 4u * (uint32_t)(t1 % LPR);
            float* dst = out + wave_uniform((uint64_t)bj * PW_COLS * ld_out + i0 + (uint64_t)R0) + lane_off;
            const uint64_t step = (uint64_t)JPP * ld_out;
            f4 v4[PW_COLS / JPP];
#pragma unroll
            for (int p = 0; p < PW_COLS / JPP; p++) {
                const int j = JPP * p + tid / LPR;
                v4[p].x = st_at(j, 4 * chunk); v4[p].y = st_at(j, 4 * chunk + 1); v4[p].z = st_at(j, 4 * chunk + 2); v4[p].w = st_at(j, 4 * chunk + 3);
            }
#pragma unroll
            for (int p = 0; p < PW_COLS / JPP; p++)
                __builtin_nontemporal_store(v4[p], reinterpret_cast<f4*>(__builtin_assume_aligned(dst + p * step, 16)));
        } else
#pragma unroll 1   // (unrolled, the eight row pointers are hoisted out of the tile loop and held across the arithmetic: 16 registers)
        for (int p = 0; p < PW_COLS / JPP; p++) {
            const int j = JPP * p + tid / LPR;
            const uint64_t jrow = (uint64_t)bj * PW_COLS + (uint64_t)j;
            if (jrow >= m) continue;
            float* dst = out + jrow * ld_out + i0 + (uint64_t)R0 + 4 * chunk;
            if (fast) {
                typedef float f4 __attribute__((ext_vector_type(4)));
                f4 v4;
                v4.x = st_at(j, 4 * chunk); v4.y = st_at(j, 4 * chunk + 1); v4.z = st_at(j, 4 * chunk + 2); v4.w = st_at(j, 4 * chunk + 3);
                __builtin_nontemporal_store(v4, reinterpret_cast<f4*>(__builtin_assume_aligned(dst, 16)));
            } else {
                for (int q = 0; q < 4; q++)
                    if (4 * chunk + q < nvalid) dst[q] = st_at(j, 4 * chunk + q);
            }
        }
        __syncthreads();
    }
    }
    }
}

// generic feature count (d <= 64): one thread per pair, vectors read from global/L2
__global__ __launch_bounds__(256) void pairwise_generic_kernel(const float* __restrict__ A, uint64_t n,
                                                               const float* __restrict__ B, uint64_t m, uint32_t d,
                                                               int metric, const float* __restrict__ M,
                                                               float* __restrict__ out, uint64_t ld_out) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t i = blockIdx.y;
    if (j >= m || i >= n) return;
    const float* a = A + i * d;
    const float* b = B + j * d;
    float v[64], t[64];
    auto udot = [&](const float* xs, const float* ys) {
        float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        uint32_t k = 0;
        for (; k + 8 <= d; k += 8)
            for (int u = 0; u < 8; u++) p[u] = p[u] + xs[k + u] * ys[k + u];
        float sum = 0.0f;
        sum = sum + (p[0] + p[4]);
        sum = sum + (p[1] + p[5]);
        sum = sum + (p[2] + p[6]);
        sum = sum + (p[3] + p[7]);
        for (; k < d; k++) sum = sum + xs[k] * ys[k];
        return sum;
    };
    float res;
    if (metric == METRIC_COSINE) {
        res = 1.0f - udot(a, b) / (sqrtf(udot(a, a)) * sqrtf(udot(b, b)));
    } else {
        for (uint32_t k = 0; k < d; k++) v[k] = a[k] - b[k];
        if (metric == METRIC_EUCLIDEAN) {
            res = sqrtf(udot(v, v));
        } else {
            for (uint32_t jj = 0; jj < d; jj++) {
                float s = 0.0f;
                for (uint32_t ii = 0; ii < d; ii++) s = s + v[ii] * M[ii * d + jj];
                t[jj] = s;
            }
            res = sqrtf(udot(t, v));
        }
    }
    out[i * ld_out + j] = res;
}

void launch_pairwise(const float* A, uint64_t n, const float* B, uint64_t m, uint32_t d, int metric, const float* M,
                     int m_is_diag, float* out, uint64_t ld_out, hipStream_t st) {
    if (n == 0 || m == 0) return;
    with_d(d, [&](auto D) {
        if constexpr (decltype(D)::value == 0) {
            for (uint64_t r0 = 0; r0 < n; r0 += 65535) {  // grid.y <= 65535
                const uint64_t rows = (n - r0 < 65535) ? n - r0 : 65535;
                hipLaunchKernelGGL(pairwise_generic_kernel, dim3((uint32_t)((m + 255) / 256), (uint32_t)rows), dim3(256), 0,
                                   st, A + r0 * d, rows, B, m, d, metric, M, out + r0 * ld_out, ld_out);
            }
        } else {
            // grid.y is limited to 65535 row tiles (8.3 M rows); larger problems are sliced by the caller
            const dim3 grid((uint32_t)((m + PW_COLS - 1) / PW_COLS),
                            (uint32_t)((n + (uint64_t)PW_ROWS * PW_RT - 1) / ((uint64_t)PW_ROWS * PW_RT)));
            const auto launch = [&](auto SELF) {
                with_metric<true>(metric, m_is_diag, [&](auto M_, auto G) {
                    hipLaunchKernelGGL((pairwise_kernel<decltype(D)::value, M_(), G(), decltype(SELF)::value>), grid, dim3(256), 0, st, A,
                                       n, B, m, M, out, ld_out);
                });
            };
            if (A == B && n == m) launch(std::true_type{});  // self-distance matrix: upper block triangle + mirrored stores
            else launch(std::false_type{});
        }
    });
}

}  // namespace bg
