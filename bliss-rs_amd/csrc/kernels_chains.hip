// kernels_chains.hip -- greedy song-to-song chains cut after k, for many seed groups at once (compiled with -ffp-contract=off).
//
// Reference: song_to_song (src/playlist.rs:272-326) followed by take(k): the first song is the candidate closest to the SET of
// seeds (closest_to_songs' score, the sequential f32 sum in seed order); every later song is the remaining candidate closest to
// the song before it, `0.0f + metric(previous, candidate)`, the lowest index among equals.  A chain of k songs takes k steps and
// chains do not talk to each other, so no grid barrier is needed: a step is a launch over every chain.  Step 0 is
// blissgpu_group_knn with k = 1 (kernels_group_knn.hip); this file holds the later steps, in two forms with one result:
//
//   chain_step_kernel   a workgroup owns up to CH_QMAX chains and a range of 256-candidate blocks.  The chains' current rows are
//                       gathered by index into LDS; the scan is knn_scan_kernel's (a block staged in LDS, four candidates per
//                       lane in registers, pair_sum per row, ONE float comparison per candidate against a bound derived from
//                       the chain's running minimum).  Only when some lane passes the bound does the wavefront build the
//                       256-bit mask of the chain's taken and skipped candidates of this block (at most s_g + k entries), the
//                       exact 64-bit keys (f32_key(v) << 32) | j of the others, and their minimum.  Keys are distinct, so the
//                       minimum depends neither on the order in which candidates are met nor on the split: with one workgroup
//                       per chain block the winner goes straight to idx / dist; when several workgroups share the candidates
//                       (few chains), each sends its minimum to best[chain] with a 64-bit atomicMin and chain_put_kernel -- the
//                       second and last launch of the step -- writes it out.
//   journey_step_kernel the same scan for JOURNEYS (blissgpu_journeys): waypoint playlists ("from song1 to song2 in
//                       n songs, without repetitions") and directed ones ("the tempo goes down or stays the same"), which the
//                       reference's TODO.md names and does not ship.  A journey is a chain with a step 0 of its own, two skip
//                       slots, and either a waypoint query or a gate on one feature: see chain_step_body.
//   chain_walk_kernel   many chains: the next song after c is the first entry of c's k-nearest list (blissgpu_knn over the
//                       candidates themselves, c skipped) that the chain has neither taken nor skipped.  Taken and skipped
//                       entries other than c number at most s_g + k - 2, so a list of L = k + max_g s_g - 1 entries always
//                       holds it.  A wavefront per chain: the skipped and taken indices in LDS, 64 list entries at a time, a
//                       ballot for the first free one.  The list's distances are the step's distances bit for bit (pair_sum,
//                       the correctly rounded root, IEEE division) in the same (distance, index) order.
#include <math.h>

#include <algorithm>

#include "device_utils.hpp"
#include "internal.hpp"
#include "knn_list.hpp"
#include "pairwise_math.hpp"
#include "playlist_math.hpp"

namespace bg {

constexpr int CH_QMAX = 32;                // most chains a workgroup of chain_step_kernel owns
constexpr uint32_t CH_NONE = 0xFFFFFFFFu;  // no song: a chain that has run out of candidates, a seed row that skips nothing

__device__ __forceinline__ unsigned long long chain_wave_min(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, WAVE);
        v = o < v ? o : v;
    }
    return v;
}

// D > 0: compile-time feature count (packed arithmetic, candidates in registers).  D == 0: any d <= 64 through pl_distance,
// candidates read from global memory / L2 (slow, exact).  Step t >= 1: reads idx[chain][0 .. t), writes idx / dist [chain][t]
// (n_split == 1) or best[chain] (several workgroups per chain).
// J: the step of a JOURNEY (journey_step_kernel; with J == false nothing below differs from the chains' step).  A journey is a
// chain with two skip slots (skip[2 g], skip[2 g + 1]; goff is not read), a step 0 of its own (t == 0: the query is its `from`
// row), and either
//   a waypoint query (j.to != NULL): step t looks for the candidate nearest from + (to - from) * j.s, computed as the rows are
//   staged -- the previous pick only tells whether the journey has ended; or
//   a gate (j.gate): a candidate is eligible only while cand[gate_feature] >= ref (UP) or <= ref (DOWN), ref the gated feature of
//   the previous pick (of `from` at step 0), one float per chain in LDS.  The candidate's feature comes from the staged block,
//   which stays in LDS through the row loop (D > 0), or from global memory (D == 0); a NaN on either side fails both
//   comparisons.  The gate only narrows `valid`: the bound test stays the cheap rejection it is.
template <int D, int METRIC, bool DIAG, bool J>
__device__ __forceinline__ void chain_step_body(const float* __restrict__ X, uint32_t n, uint32_t d_rt, int metric_rt,
                                                const float* __restrict__ M, const uint32_t* __restrict__ goff,
                                                const uint32_t* __restrict__ skip, uint32_t n_chains, uint32_t k, uint32_t t,
                                                uint32_t qb_rt, uint32_t n_split, uint32_t blocks_per_split, uint32_t* idx,
                                                float* dist, unsigned long long* best, uint32_t* nan_flag, const JourneyStep& j) {
    constexpr bool GENERIC = D == 0;
    constexpr int DQ = GENERIC ? PL_DMAX : ((D + 3) & ~3);  // LDS pitch of a chain's row: 16-byte aligned -> ds_read_b128 broadcasts
    constexpr int XP = GENERIC ? 1 : (D | 1);               // LDS pitch of a staged candidate: odd, lanes l and l + 1 on different banks
    constexpr bool FLAT = XP == D;
    constexpr bool ROOT = !GENERIC && METRIC != METRIC_COSINE;  // the bound is on the sum before the square root
    __shared__ __attribute__((aligned(16))) float s_q[CH_QMAX][DQ];
    __shared__ __attribute__((aligned(16))) float s_x[GENERIC ? 4 : KNN_COLS * XP];
    __shared__ float s_m[(!GENERIC && METRIC == METRIC_MAHALANOBIS) ? D * D : 1];
    __shared__ float s_nq[CH_QMAX];
    __shared__ unsigned long long s_best[CH_QMAX];
    __shared__ float s_bound[CH_QMAX];
    __shared__ uint32_t s_cur[CH_QMAX], s_g0[CH_QMAX], s_gn[CH_QMAX];
    __shared__ uint32_t s_mask[4][8];
    float* s_ref = nullptr;  // the gate's reference value of every chain of the workgroup
    if constexpr (J) {
        __shared__ float ref_lds[CH_QMAX];
        s_ref = ref_lds;
    }
    const bool gated = J && j.gate != GATE_NONE;  // (uniform over the grid)

    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const uint32_t d = GENERIC ? d_rt : (uint32_t)D;
    const uint32_t QB = qb_rt;  // chains per workgroup: at most CH_QMAX
    const uint32_t split = blockIdx.x % n_split;
    const uint32_t cb_step = gridDim.x / n_split;
    const uint32_t n_cb = (n_chains + QB - 1) / QB;
    const uint32_t n_blocks = (uint32_t)(((uint64_t)n + KNN_COLS - 1) / KNN_COLS);
    const uint32_t blk0 = split * blocks_per_split;
    const uint32_t blk1 = (blk0 + blocks_per_split < n_blocks) ? blk0 + blocks_per_split : n_blocks;
    bool saw_nan = false;

    if (!GENERIC && METRIC == METRIC_MAHALANOBIS) {
        for (int e = tid; e < D * D; e += 256) s_m[e] = M[e];
    }
    float wdiag[GENERIC ? 1 : D];
    if constexpr (!GENERIC) {
        if (DIAG) __syncthreads();
#pragma unroll
        for (int kk = 0; kk < D; kk++)  // (the same in every lane: scalar registers)
            wdiag[kk] = DIAG ? __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s_m[(kk * D + kk) % (METRIC == METRIC_MAHALANOBIS ? D * D : 1)]))) : 0.0f;
    }

    for (uint32_t cb = blockIdx.x / n_split; cb < n_cb; cb += cb_step) {
        const uint32_t c0 = cb * QB;
        const uint32_t rows_here = (n_chains - c0 < QB) ? n_chains - c0 : QB;
        __syncthreads();  // every wavefront has finished with the previous chain block
        if ((uint32_t)tid < rows_here) {
            const uint32_t g = c0 + (uint32_t)tid;
            if constexpr (J) {
                s_g0[tid] = 2u * g;
                s_gn[tid] = 2u;
                const uint32_t cur = t ? idx[(uint64_t)g * k + (t - 1u)] : 0u;  // (step 0 has no predecessor: any song will do)
                s_cur[tid] = cur;
                if (gated && cur != CH_NONE)
                    s_ref[tid] = t ? X[(uint64_t)cur * d + j.gate_feature] : j.from[(uint64_t)g * d + j.gate_feature];
            } else {
                const uint32_t a = goff[g];
                s_g0[tid] = a;
                s_gn[tid] = goff[g + 1] - a;
                s_cur[tid] = idx[(uint64_t)g * k + (t - 1u)];  // CH_NONE: the chain has run out of candidates
            }
            s_best[tid] = KNN_NONE;
            s_bound[tid] = INFINITY;
        }
        __syncthreads();
        // the chains' current rows, gathered by index (a journey: its waypoint, or at step 0 its `from` row)
        for (uint32_t e = (uint32_t)tid; e < rows_here * d; e += 256u) {
            const uint32_t r = e / d, cur = s_cur[r];
            float v = 0.0f;
            if (J && cur != CH_NONE && (j.to || t == 0u)) {
                const uint64_t at = (uint64_t)(c0 + r) * d + e % d;
                const float a = j.from[at];
                v = j.to ? a + (j.to[at] - a) * j.s : a;
            } else if (cur != CH_NONE) {
                v = X[(uint64_t)cur * d + e % d];
            }
            s_q[r][e % d] = v;
        }
        __syncthreads();
        if (!GENERIC && METRIC == METRIC_COSINE) {
            if ((uint32_t)tid < rows_here) {
                const float* a = s_q[tid];
                s_nq[tid] = sqrtf(unrolled_dot<(GENERIC ? 1 : D)>([&](int kk) { return a[kk]; }, [&](int kk) { return a[kk]; }));
            }
            __syncthreads();
        }

        for (uint32_t blk = blk0; blk < blk1; blk++) {
            const uint32_t j0 = blk * (uint32_t)KNN_COLS;
            const uint32_t cols_here = (n - j0 < (uint32_t)KNN_COLS) ? n - j0 : (uint32_t)KNN_COLS;
            // the lane's four candidates as two packed pairs: bp[h][kk] = (candidate 2h, candidate 2h + 1), candidate c = row
            // j0 + 64 c + lane
            f2 bp[2][GENERIC ? 1 : D];
            f2 nb[2];
            if constexpr (!GENERIC) {
                if (blk != blk0) __syncthreads();  // every wavefront has taken the previous block into registers
                const float* src = X + (uint64_t)j0 * D;
                const uint32_t floats = cols_here * (uint32_t)D;
                if (FLAT && (reinterpret_cast<uintptr_t>(X) & 15u) == 0) {  // (a block starts 256 * D * 4 bytes after the last: 16-byte aligned too)
                    const float4* src4 = reinterpret_cast<const float4*>(src);
                    float4* dst4 = reinterpret_cast<float4*>(s_x);
                    for (uint32_t e = (uint32_t)tid; e < floats / 4u; e += 256u) dst4[e] = src4[e];
                    if ((uint32_t)tid < (floats & 3u)) s_x[(floats & ~3u) + (uint32_t)tid] = src[(floats & ~3u) + (uint32_t)tid];
                } else if (FLAT) {
                    for (uint32_t e = (uint32_t)tid; e < floats; e += 256u) s_x[e] = src[e];
                } else {
                    for (uint32_t e = (uint32_t)tid; e < floats; e += 256u) s_x[(e / (uint32_t)D) * XP + e % (uint32_t)D] = src[e];
                }
                // a ragged last block: zero rows, so that the lanes beyond it compute on defined values (their results are dropped)
                for (uint32_t e = cols_here * (uint32_t)XP + (uint32_t)tid; e < (uint32_t)(KNN_COLS * XP); e += 256u) s_x[e] = 0.0f;
                __syncthreads();
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const uint32_t la = (uint32_t)(2 * h) * 64u + (uint32_t)lane, lb = la + 64u;
#pragma unroll
                    for (int kk = 0; kk < D; kk++) {
                        bp[h][kk].x = s_x[la * XP + kk];
                        bp[h][kk].y = s_x[lb * XP + kk];
                    }
                    if (METRIC == METRIC_COSINE) {
                        const f2 qq = unrolled_dot2<(GENERIC ? 1 : D)>([&](int kk) { return bp[h][kk]; }, [&](int kk) { return bp[h][kk]; });
                        nb[h].x = sqrtf(qq.x);
                        nb[h].y = sqrtf(qq.y);
                    }
                }
            }
            const uint32_t wave_u = (uint32_t)__builtin_amdgcn_readfirstlane(wave);
#pragma unroll 1
            for (uint32_t r = wave_u; r < rows_here; r += 4u) {
                if (s_cur[r] == CH_NONE) continue;  // (wave-uniform)
                const float ref = gated ? s_ref[r] : 0.0f;
                // pv[c]: what the bound is compared with for candidate c of the lane -- the sum before the root (ROOT) or the distance
                float pv[4];
                if constexpr (GENERIC) {
#pragma unroll 1
                    for (int c = 0; c < 4; c++) {
                        const uint32_t lc = 64u * (uint32_t)c + (uint32_t)lane;
                        pv[c] = (lc < cols_here) ? pl_distance(s_q[r], X + (uint64_t)(j0 + lc) * d, d, metric_rt, M) : INFINITY;
                    }
                } else {
                    f2 ap[DQ / 2];
#pragma unroll
                    for (int k4 = 0; k4 < DQ / 4; k4++) {  // same address in every lane: LDS broadcast
                        const float4 v = *reinterpret_cast<const float4*>(&s_q[r][4 * k4]);
                        ap[2 * k4].x = v.x; ap[2 * k4].y = v.y; ap[2 * k4 + 1].x = v.z; ap[2 * k4 + 1].y = v.w;
                    }
                    f2 s0 = pair_sum<(GENERIC ? 1 : D), METRIC, DIAG>(ap, bp[0], wdiag, s_m);
                    // (general M: one pair's 2 x d differences and products at a time, as in knn_scan_kernel)
                    if (METRIC == METRIC_MAHALANOBIS && !DIAG) asm volatile("" : "+v"(s0));
                    f2 s1 = pair_sum<(GENERIC ? 1 : D), METRIC, DIAG>(ap, bp[1], wdiag, s_m);
                    if (METRIC == METRIC_COSINE) {
                        s0 = splat(1.0f) - s0 / (splat(s_nq[r]) * nb[0]);
                        s1 = splat(1.0f) - s1 / (splat(s_nq[r]) * nb[1]);
                    }
                    pv[0] = s0.x; pv[1] = s0.y; pv[2] = s1.x; pv[3] = s1.y;
                }
                // wave-uniform: can any of the wavefront's 256 candidates beat the chain's minimum?  (`!(v > bound)`: a NaN says yes)
                const float bound = s_bound[r];
                const bool maybe = !(pv[0] > bound) || !(pv[1] > bound) || !(pv[2] > bound) || !(pv[3] > bound);
                if (__ballot(maybe) == 0ull) continue;
                // the chain's taken and skipped candidates of this block as a 256-bit mask
                uint32_t* mask = s_mask[wave_u];
                if (lane < 8) mask[lane] = 0u;
                knn_wave_sync();
                {
                    const uint32_t g0 = s_g0[r], gn = s_gn[r];
                    const uint32_t* taken = idx + (uint64_t)(c0 + r) * k;
                    for (uint32_t e = (uint32_t)lane; e < gn + t; e += 64u) {
                        const uint32_t s = e < gn ? (skip ? skip[g0 + e] : CH_NONE) : taken[e - gn];
                        if (s >= j0 && s - j0 < (uint32_t)KNN_COLS) atomicOr(&mask[(s - j0) >> 5], 1u << ((s - j0) & 31u));
                    }
                    knn_wave_sync();
                }
                // the exact part: distances, keys, the minimum of the eligible ones
                unsigned long long m = KNN_NONE;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const uint32_t lc = 64u * (uint32_t)c + (uint32_t)lane, jc = j0 + lc;  // (jc is only used where lc < cols_here)
                    const bool gone = ((mask[lc >> 5] >> (lc & 31u)) & 1u) != 0u;
                    bool valid = lc < cols_here && !gone;  // a taken or skipped candidate's distance is never looked at
                    if (gated) {                           // ... nor that of one the gate keeps out
                        float f;
                        if constexpr (GENERIC) f = valid ? X[(uint64_t)jc * d + j.gate_feature] : 0.0f;
                        else f = s_x[lc * (uint32_t)XP + j.gate_feature];
                        valid = valid && (j.gate == GATE_UP ? f >= ref : f <= ref);
                    }
                    const float v = 0.0f + (ROOT ? sqrtf(pv[c]) : pv[c]);
                    if (valid && v != v) saw_nan = true;
                    const unsigned long long key = ((unsigned long long)f32_key(v) << 32) | jc;
                    if (valid && key < m) m = key;
                }
                m = chain_wave_min(m);
                if (m < s_best[r]) {  // (wave-uniform)
                    knn_wave_sync();  // every lane has read the old minimum
                    if (lane == 0) {
                        s_best[r] = m;
                        s_bound[r] = knn_bound<ROOT>(m);
                    }
                }
                knn_wave_sync();
            }
        }
        // the winner of this range
        __syncthreads();
        if ((uint32_t)tid < rows_here) {
            const unsigned long long b = s_best[tid];
            const uint64_t g = (uint64_t)c0 + (uint32_t)tid;
            if (b != KNN_NONE) {
                if (n_split == 1u) {
                    idx[g * k + t] = (uint32_t)(b & 0xFFFFFFFFull);
                    if (dist) dist[g * k + t] = knn_key_dist(b);
                } else {
                    atomicMin(&best[g], b);
                }
            }
        }
    }
    if (saw_nan) atomicOr(nan_flag, 1u);
}

template <int D, int METRIC, bool DIAG>
__global__ __launch_bounds__(256, 2) void chain_step_kernel(const float* __restrict__ X, uint32_t n, uint32_t d_rt, int metric_rt,
                                                            const float* __restrict__ M, const uint32_t* __restrict__ goff,
                                                            const uint32_t* __restrict__ skip, uint32_t n_chains, uint32_t k,
                                                            uint32_t t, uint32_t qb_rt, uint32_t n_split,
                                                            uint32_t blocks_per_split, uint32_t* idx, float* dist,
                                                            unsigned long long* best, uint32_t* nan_flag) {
    chain_step_body<D, METRIC, DIAG, false>(X, n, d_rt, metric_rt, M, goff, skip, n_chains, k, t, qb_rt, n_split, blocks_per_split, idx,
                                            dist, best, nan_flag, JourneyStep{});
}

// step t >= 0 of every journey: skip is [n_chains][2] or NULL
template <int D, int METRIC, bool DIAG>
__global__ __launch_bounds__(256, 2) void journey_step_kernel(const float* __restrict__ X, uint32_t n, uint32_t d_rt, int metric_rt,
                                                              const float* __restrict__ M, const uint32_t* __restrict__ skip,
                                                              uint32_t n_chains, uint32_t k, uint32_t t, uint32_t qb_rt,
                                                              uint32_t n_split, uint32_t blocks_per_split, uint32_t* idx,
                                                              float* dist, unsigned long long* best, uint32_t* nan_flag,
                                                              JourneyStep j) {
    chain_step_body<D, METRIC, DIAG, true>(X, n, d_rt, metric_rt, M, nullptr, skip, n_chains, k, t, qb_rt, n_split, blocks_per_split, idx,
                                           dist, best, nan_flag, j);
}

// column t of idx / dist from the chains' minima (best != NULL: a step shared by several workgroups; the minima are reset for
// the next step) or from step 0's [n_chains] arrays (best == NULL, t == 0).  The rest of a row keeps its padding.
__global__ __launch_bounds__(256) void chain_put_kernel(unsigned long long* __restrict__ best, const uint32_t* __restrict__ idx0,
                                                        const float* __restrict__ dist0, uint32_t n_chains, uint32_t k, uint32_t t,
                                                        uint32_t* __restrict__ idx, float* __restrict__ dist) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (g >= n_chains) return;
    if (best) {
        const unsigned long long b = best[g];
        if (b == KNN_NONE) return;
        best[g] = KNN_NONE;
        idx[g * k + t] = (uint32_t)(b & 0xFFFFFFFFull);
        if (dist) dist[g * k + t] = knn_key_dist(b);
    } else {
        idx[g * k + t] = idx0[g];
        if (dist) dist[g * k + t] = dist0[g];
    }
}

// A wavefront per chain over the candidates' k-nearest lists ([n][L], ascending, padded with CH_NONE / +inf; list c leaves c
// out).  first[chain] / first_dist[chain] is step 0.  A chain that finds neither a free entry nor the end of a list within L
// entries sets *short_flag (cannot happen while L >= k + s_g - 1; the entry point then answers by steps).
constexpr int CW_TAKEN = 1088;  // >= s_g + k for every chain the lists route accepts (L = k + max s_g - 1 <= 1024)
__global__ __launch_bounds__(256) void chain_walk_kernel(const uint32_t* __restrict__ lists, const float* __restrict__ list_dist,
                                                         uint32_t L, const uint32_t* __restrict__ goff,
                                                         const uint32_t* __restrict__ skip, const uint32_t* __restrict__ first,
                                                         const float* __restrict__ first_dist, uint32_t n_chains, uint32_t k,
                                                         uint32_t* __restrict__ idx, float* __restrict__ dist,
                                                         uint32_t* short_flag) {
    __shared__ uint32_t s_taken[4][CW_TAKEN];
    const int lane = lane_id(), wave = wave_id();
    uint32_t* taken = s_taken[wave];
    for (uint64_t g = (uint64_t)blockIdx.x * 4 + (uint64_t)wave; g < n_chains; g += (uint64_t)gridDim.x * 4) {
        const uint32_t g0 = goff[g], gn = goff[g + 1] - g0;
        uint32_t cur = first[g];
        uint32_t m = gn + 1u;  // entries of `taken`: the group's skipped candidates, then the chain so far
        if (m + k > (uint32_t)CW_TAKEN + 1u) {  // (wave-uniform; refused by the entry point)
            if (lane == 0) atomicOr(short_flag, 1u);
            continue;
        }
        for (uint32_t e = (uint32_t)lane; e < gn; e += 64u) taken[e] = skip ? skip[g0 + e] : CH_NONE;
        if (lane == 0) {
            taken[gn] = cur;
            idx[g * k] = cur;
            if (dist) dist[g * k] = first_dist[g];
        }
        knn_wave_sync();
        for (uint32_t t = 1; t < k && cur != CH_NONE; t++) {
            const uint32_t* row = lists + (uint64_t)cur * L;
            uint32_t nxt = CH_NONE;
            bool found = false, ended = false;
            for (uint32_t i0 = 0; i0 < L && !found && !ended; i0 += 64u) {
                const uint32_t i = i0 + (uint32_t)lane;
                const uint32_t e = i < L ? row[i] : CH_NONE;
                bool is_free = e != CH_NONE;
                for (uint32_t q = 0; q < m && is_free; q++) is_free = taken[q] != e;  // (the same address in every lane: a broadcast)
                const unsigned long long free_mask = __ballot(is_free), end_mask = __ballot(i < L && e == CH_NONE);
                if (free_mask) {  // (a list is ascending with its padding last: a free entry comes before the end)
                    const int p = __builtin_ctzll(free_mask);
                    nxt = (uint32_t)__shfl((int)e, p, WAVE);
                    if (lane == 0) {
                        idx[g * k + t] = nxt;
                        if (dist) dist[g * k + t] = list_dist[(uint64_t)cur * L + i0 + (uint32_t)p];
                        taken[m] = nxt;
                    }
                    found = true;
                } else if (end_mask) {
                    ended = true;  // every other candidate is taken or skipped: the rest of the row is padding
                }
            }
            if (!found && !ended && lane == 0) atomicOr(short_flag, 1u);
            knn_wave_sync();
            m += found ? 1u : 0u;
            cur = nxt;
        }
        knn_wave_sync();  // the list is read before the wavefront's next chain overwrites it
    }
}

// The split of a step for n_chains chains over n candidates: chains per workgroup (whole rounds of the device, as knn_plan) and,
// when few chains leave the device empty, the workgroups that share a chain's candidates (at least eight blocks each).
ChainPlan chain_plan(uint64_t n_chains, uint64_t n, int n_cus) {
    ChainPlan p{};
    const uint64_t cus = cus_or_default(n_cus);
    p.qb = (uint32_t)CH_QMAX;
    {
        const uint64_t slots = cus * 2;
        const uint64_t rounds = std::max<uint64_t>(1, ((n_chains + p.qb - 1) / p.qb + slots - 1) / slots);
        const uint64_t even = (n_chains + rounds * slots - 1) / (rounds * slots);
        p.qb = (uint32_t)std::min<uint64_t>(p.qb, std::max<uint64_t>(4, (even + 3) / 4 * 4));  // whole rows per wavefront
    }
    const uint64_t n_cb = (n_chains + p.qb - 1) / p.qb;
    const uint64_t n_blocks = (n + KNN_COLS - 1) / KNN_COLS;
    uint64_t split = n_cb ? (4 * cus) / n_cb : 1;
    split = std::min<uint64_t>(split, (n_blocks + 7) / 8);
    split = std::max<uint64_t>(split, 1);
    p.blocks_per_split = (uint32_t)std::max<uint64_t>(1, (n_blocks + split - 1) / split);
    p.n_split = (uint32_t)std::max<uint64_t>(1, (n_blocks + p.blocks_per_split - 1) / p.blocks_per_split);
    p.grid_cb = (uint32_t)std::min<uint64_t>(n_cb, 1u << 20);
    return p;
}

// (j == NULL: a chains' step; otherwise a journeys' step, which reads no goff)
static void step_any(const float* X, uint32_t n, uint32_t d, int metric, const float* M, int m_is_diag, const uint32_t* goff,
                     const uint32_t* skip, uint32_t n_chains, uint32_t k, uint32_t t, const ChainPlan& p, uint32_t* idx, float* dist,
                     unsigned long long* best, uint32_t* nan_flag, const JourneyStep* j, hipStream_t st) {
    if (n_chains == 0 || n == 0) return;
    const dim3 grid(p.grid_cb * p.n_split);
    for_metric_form<true>(d, metric, m_is_diag, [&](auto D, auto M_, auto G) {
        if (j)
            hipLaunchKernelGGL((journey_step_kernel<D(), M_(), G()>), grid, dim3(256), 0, st, X, n, d, metric, M, skip, n_chains, k, t, p.qb,
                               p.n_split, p.blocks_per_split, idx, dist, best, nan_flag, *j);
        else
            hipLaunchKernelGGL((chain_step_kernel<D(), M_(), G()>), grid, dim3(256), 0, st, X, n, d, metric, M, goff, skip, n_chains, k, t,
                               p.qb, p.n_split, p.blocks_per_split, idx, dist, best, nan_flag);
    });
    if (p.n_split > 1)
        hipLaunchKernelGGL(chain_put_kernel, dim3((n_chains + 255u) / 256u), dim3(256), 0, st, best, nullptr, nullptr, n_chains, k, t,
                           idx, dist);
}

void launch_chain_step(const float* X, uint32_t n, uint32_t d, int metric, const float* M, int m_is_diag, const uint32_t* goff,
                       const uint32_t* skip, uint32_t n_chains, uint32_t k, uint32_t t, const ChainPlan& p, uint32_t* idx,
                       float* dist, unsigned long long* best, uint32_t* nan_flag, hipStream_t st) {
    step_any(X, n, d, metric, M, m_is_diag, goff, skip, n_chains, k, t, p, idx, dist, best, nan_flag, nullptr, st);
}

void launch_journey_step(const float* X, uint32_t n, uint32_t d, int metric, const float* M, int m_is_diag, const uint32_t* skip,
                         uint32_t n_journeys, uint32_t k, uint32_t t, const ChainPlan& p, const JourneyStep& j, uint32_t* idx,
                         float* dist, unsigned long long* best, uint32_t* nan_flag, hipStream_t st) {
    step_any(X, n, d, metric, M, m_is_diag, nullptr, skip, n_journeys, k, t, p, idx, dist, best, nan_flag, &j, st);
}

void launch_chain_first(const uint32_t* idx0, const float* dist0, uint32_t n_chains, uint32_t k, uint32_t* idx, float* dist,
                        hipStream_t st) {
    if (n_chains == 0) return;
    hipLaunchKernelGGL(chain_put_kernel, dim3((n_chains + 255u) / 256u), dim3(256), 0, st, nullptr, idx0, dist0, n_chains, k, 0u, idx,
                       dist);
}

void launch_chain_walk(const uint32_t* lists, const float* list_dist, uint32_t L, const uint32_t* goff, const uint32_t* skip,
                       const uint32_t* first, const float* first_dist, uint32_t n_chains, uint32_t k, uint32_t* idx, float* dist,
                       uint32_t* short_flag, hipStream_t st) {
    if (n_chains == 0) return;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)n_chains + 3) / 4, 1u << 20);
    hipLaunchKernelGGL(chain_walk_kernel, dim3(grid), dim3(256), 0, st, lists, list_dist, L, goff, skip, first, first_dist, n_chains,
                       k, idx, dist, short_flag);
}

}  // namespace bg
