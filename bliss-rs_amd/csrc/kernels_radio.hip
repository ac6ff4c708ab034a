// kernels_radio.hip -- radio playlists: greedy song-to-song chains (or the k nearest songs) under LABEL RULES, for many start
// songs at once (blissgpu_radio; compiled with -ffp-contract=off).
//
// Every candidate carries one label per rule (artist id, album id, ...; RADIO_NONE = no label).  Rule r says: among the last
// window[r] songs of a radio -- position -1 is the start song, positions 0 .. t - 1 its picks -- at most limit[r] carry any one
// label.  So at step t a label that already has limit[r] occurrences inside the window is BANNED, and a candidate is eligible
// when it is neither skipped nor taken nor carries a banned label of any rule.  A step is two launches over every radio:
//
//   radio_ban_kernel    a wavefront per (radio, rule): the window's labels in LDS, every label counted against the others, the
//                       banned ones written -- each once, in order of first appearance -- to ban[(radio, rule)][0 .. cap) with
//                       their number in ban_cnt[(radio, rule)].  At most min(window, t + 1) / limit labels can be banned, which
//                       is what the host sizes `cap` from.
//   radio_step_kernel   chain_step_kernel's scan (kernels_chains.hip): a workgroup owns up to RD_QMAX radios and a range of
//                       256-candidate blocks staged in LDS, four candidates per lane in registers, pair_sum per radio, ONE float
//                       comparison per candidate against a bound derived from the radio's running minimum.  Only when some lane
//                       passes the bound does the wavefront go on: rule by rule it loads its candidates' labels (coalesced,
//                       labels[r][j0 + 64 c + lane]) and drops those that equal one of the radio's banned labels (the same
//                       address in every lane: a broadcast out of L2; staging the lists in LDS per radio block was measured
//                       and was no faster); most wavefronts stop there, because the songs nearest a radio are
//                       mostly its last artists'.  The others build the 256-bit mask of taken and skipped candidates, the
//                       exact keys and their minimum as the chains do.  The running minimum is taken over ELIGIBLE candidates
//                       only, so a banned nearer song never tightens the bound: the bound stays a one-sided rejection test
//                       and the result is exact.  mode RADIO_NEAREST keeps the query at from[g]; RADIO_CHAIN gathers the
//                       previous pick's row (step 0: from[g]).
//   radio_put_kernel    the second launch of a step that several workgroups share (few radios): best[radio] -> idx / dist.
#include <math.h>

#include <algorithm>

#include "device_utils.hpp"
#include "internal.hpp"
#include "knn_list.hpp"
#include "pairwise_math.hpp"
#include "playlist_math.hpp"

namespace bg {

constexpr int RD_QMAX = 32;                // most radios a workgroup of radio_step_kernel owns (chain_plan's CH_QMAX)
constexpr uint32_t RD_NONE = RADIO_NONE;   // no song / no label
constexpr int RD_HIST = 1024;              // most history positions a window can hold: min(window, k + 1, t + 1) <= KNN_MAX_K

__device__ __forceinline__ unsigned long long radio_wave_min(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, WAVE);
        v = o < v ? o : v;
    }
    return v;
}

// The banned labels of every (radio, active rule) at step t.  A radio that has ended (its previous pick is RD_NONE) bans nothing:
// its step does not run.
__global__ __launch_bounds__(256) void radio_ban_kernel(const uint32_t* __restrict__ labels, const uint32_t* __restrict__ from_labels,
                                                        const uint32_t* __restrict__ idx, uint32_t n, uint32_t n_radios, uint32_t k,
                                                        uint32_t t, RadioRules rules, uint32_t* __restrict__ ban,
                                                        uint32_t* __restrict__ ban_cnt) {
    __shared__ uint32_t s_hist[4][RD_HIST];
    const int lane = lane_id(), wave = wave_id();
    uint32_t* h = s_hist[wave];
    const uint64_t n_work = (uint64_t)n_radios * rules.n;
    for (uint64_t w = (uint64_t)blockIdx.x * 4 + (uint64_t)wave; w < n_work; w += (uint64_t)gridDim.x * 4) {
        const uint32_t g = (uint32_t)(w / rules.n), a = (uint32_t)(w % rules.n);
        const uint32_t rule = rules.rule[a], win = rules.window[a], lim = rules.limit[a];
        const uint32_t* taken = idx + (uint64_t)g * k;
        uint32_t out = 0;
        if (t == 0u || taken[t - 1u] != RD_NONE) {  // (wave-uniform)
            // history positions p0 .. t - 1, p0 >= -1: entry e is position p0 + e
            const int32_t p0 = (win > t) ? -1 : (int32_t)(t - win);
            uint32_t m = (uint32_t)((int32_t)t - p0);
            if (m > (uint32_t)RD_HIST) m = (uint32_t)RD_HIST;  // (cannot happen: window <= k + 1 and t + 1 <= k <= RD_HIST)
            for (uint32_t e = (uint32_t)lane; e < m; e += 64u) {
                const int32_t p = p0 + (int32_t)e;
                uint32_t L;
                if (p < 0) {
                    L = from_labels ? from_labels[(uint64_t)g * rules.n_total + rule] : RD_NONE;
                } else {
                    const uint32_t s = taken[p];
                    L = s < n ? labels[(uint64_t)rule * n + s] : RD_NONE;
                }
                h[e] = L;
            }
            knn_wave_sync();
            uint32_t* dst = ban + w * rules.cap;
            for (uint32_t e0 = 0; e0 < m; e0 += 64u) {
                const uint32_t e = e0 + (uint32_t)lane;
                const uint32_t L = e < m ? h[e] : RD_NONE;
                uint32_t cnt = 0;
                bool first = true;
                for (uint32_t q = 0; q < m; q++) {  // (the same address in every lane: a broadcast)
                    const bool same = h[q] == L;
                    cnt += same ? 1u : 0u;
                    first = first && !(same && q < e);
                }
                const bool banned = L != RD_NONE && first && cnt >= lim;
                const unsigned long long b = __ballot(banned);
                const uint32_t pos = out + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
                if (banned && pos < rules.cap) dst[pos] = L;
                out += (uint32_t)__popcll(b);
            }
            if (out > rules.cap) out = rules.cap;  // (cannot happen: at most m / limit labels reach the limit)
        }
        if (lane == 0) ban_cnt[w] = out;
        knn_wave_sync();  // the window is read before the wavefront's next item overwrites it
    }
}

// D > 0: compile-time feature count (packed arithmetic, candidates in registers).  D == 0: any d <= 64 through pl_distance,
// candidates read from global memory / L2 (slow, exact).  Step t >= 0: reads idx[radio][0 .. t), writes idx / dist [radio][t]
// (n_split == 1) or best[radio] (several workgroups per radio).  skip is [n_radios][2] or NULL.
template <int D, int METRIC, bool DIAG>
__global__ __launch_bounds__(256, 2) void radio_step_kernel(const float* __restrict__ X, uint32_t n, uint32_t d_rt, int metric_rt,
                                                            const float* __restrict__ M, const float* __restrict__ from,
                                                            const uint32_t* __restrict__ skip, const uint32_t* __restrict__ labels,
                                                            RadioRules rules, const uint32_t* __restrict__ ban,
                                                            const uint32_t* __restrict__ ban_cnt, int nearest, uint32_t n_radios,
                                                            uint32_t k, uint32_t t, uint32_t qb_rt, uint32_t n_split,
                                                            uint32_t blocks_per_split, uint32_t* idx, float* dist,
                                                            unsigned long long* best, uint32_t* nan_flag) {
    constexpr bool GENERIC = D == 0;
    constexpr int DQ = GENERIC ? PL_DMAX : ((D + 3) & ~3);  // LDS pitch of a radio's row: 16-byte aligned -> ds_read_b128 broadcasts
    constexpr int XP = GENERIC ? 1 : (D | 1);               // LDS pitch of a staged candidate: odd, lanes l and l + 1 on different banks
    constexpr bool FLAT = XP == D;
    constexpr bool ROOT = !GENERIC && METRIC != METRIC_COSINE;  // the bound is on the sum before the square root
    __shared__ __attribute__((aligned(16))) float s_q[RD_QMAX][DQ];
    __shared__ __attribute__((aligned(16))) float s_x[GENERIC ? 4 : KNN_COLS * XP];
    __shared__ float s_m[(!GENERIC && METRIC == METRIC_MAHALANOBIS) ? D * D : 1];
    __shared__ float s_nq[RD_QMAX];
    __shared__ unsigned long long s_best[RD_QMAX];
    __shared__ float s_bound[RD_QMAX];
    __shared__ uint32_t s_cur[RD_QMAX];
    __shared__ uint32_t s_mask[4][8];

    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const uint32_t d = GENERIC ? d_rt : (uint32_t)D;
    const uint32_t QB = qb_rt;  // radios per workgroup: at most RD_QMAX
    const uint32_t split = blockIdx.x % n_split;
    const uint32_t cb_step = gridDim.x / n_split;
    const uint32_t n_cb = (n_radios + QB - 1) / QB;
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
        const uint32_t rows_here = (n_radios - c0 < QB) ? n_radios - c0 : QB;
        __syncthreads();  // every wavefront has finished with the previous radio block
        if ((uint32_t)tid < rows_here) {
            const uint32_t g = c0 + (uint32_t)tid;
            s_cur[tid] = t ? idx[(uint64_t)g * k + (t - 1u)] : 0u;  // RD_NONE: the radio has ended (step 0 has no predecessor)
            s_best[tid] = KNN_NONE;
            s_bound[tid] = INFINITY;
        }
        __syncthreads();
        // the radios' query rows: the previous pick gathered by index (CHAIN, t >= 1) or the start row
        for (uint32_t e = (uint32_t)tid; e < rows_here * d; e += 256u) {
            const uint32_t r = e / d, cur = s_cur[r];
            float v = 0.0f;
            if (cur != RD_NONE) v = (nearest || t == 0u) ? from[(uint64_t)(c0 + r) * d + e % d] : X[(uint64_t)cur * d + e % d];
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
                if (s_cur[r] == RD_NONE) continue;  // (wave-uniform)
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
                // wave-uniform: can any of the wavefront's 256 candidates beat the radio's minimum?  (`!(v > bound)`: a NaN says yes)
                const float bound = s_bound[r];
                const bool maybe = !(pv[0] > bound) || !(pv[1] > bound) || !(pv[2] > bound) || !(pv[3] > bound);
                if (__ballot(maybe) == 0ull) continue;
                // the candidates that can still win: inside the block and not above the bound (a value above it cannot beat the
                // radio's minimum, so leaving it out changes nothing)
                bool alive[4];
#pragma unroll
                for (int c = 0; c < 4; c++) alive[c] = 64u * (uint32_t)c + (uint32_t)lane < cols_here && !(pv[c] > bound);
                // the label rules first: a candidate that carries a banned label is out (RD_NONE is never banned).  The nearest
                // songs of a radio are mostly its last artists', so most wavefronts that pass the bound stop here
                for (uint32_t a = 0; a < rules.n; a++) {
                    if (a && __ballot(alive[0] || alive[1] || alive[2] || alive[3]) == 0ull) break;  // (an earlier rule took them all)
                    const uint64_t w = (uint64_t)(c0 + r) * rules.n + a;
                    const uint32_t nban = ban_cnt[w];  // (wave-uniform)
                    if (nban == 0u) continue;
                    const uint32_t* lab = labels + (uint64_t)rules.rule[a] * n + j0;
                    uint32_t L[4];
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const uint32_t lc = 64u * (uint32_t)c + (uint32_t)lane;
                        L[c] = lc < cols_here ? lab[lc] : RD_NONE;
                    }
                    const uint32_t* list = ban + w * rules.cap;
                    for (uint32_t i = 0; i < nban; i++) {
                        const uint32_t b = list[i];  // (the same address in every lane: a broadcast out of L2)
#pragma unroll
                        for (int c = 0; c < 4; c++) alive[c] = alive[c] && L[c] != b;
                    }
                }
                if (rules.n && __ballot(alive[0] || alive[1] || alive[2] || alive[3]) == 0ull) continue;
                // the radio's taken and skipped candidates of this block as a 256-bit mask
                uint32_t* mask = s_mask[wave_u];
                if (lane < 8) mask[lane] = 0u;
                knn_wave_sync();
                {
                    const uint32_t* taken = idx + (uint64_t)(c0 + r) * k;
                    for (uint32_t e = (uint32_t)lane; e < 2u + t; e += 64u) {
                        const uint32_t s = e < 2u ? (skip ? skip[2ull * (c0 + r) + e] : RD_NONE) : taken[e - 2u];
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
                    const bool valid = alive[c] && !gone;  // an ineligible candidate's distance is never looked at
                    const float v = 0.0f + (ROOT ? sqrtf(pv[c]) : pv[c]);
                    if (valid && v != v) saw_nan = true;
                    const unsigned long long key = ((unsigned long long)f32_key(v) << 32) | jc;
                    if (valid && key < m) m = key;
                }
                m = radio_wave_min(m);
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

// column t of idx / dist from the radios' minima (a step shared by several workgroups); the minima are reset for the next step.
// A radio without a winner keeps its padding.
__global__ __launch_bounds__(256) void radio_put_kernel(unsigned long long* __restrict__ best, uint32_t n_radios, uint32_t k, uint32_t t,
                                                        uint32_t* __restrict__ idx, float* __restrict__ dist) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (g >= n_radios) return;
    const unsigned long long b = best[g];
    if (b == KNN_NONE) return;
    best[g] = KNN_NONE;
    idx[g * k + t] = (uint32_t)(b & 0xFFFFFFFFull);
    if (dist) dist[g * k + t] = knn_key_dist(b);
}

void launch_radio_ban(const RadioArgs& a, uint32_t t, hipStream_t st) {
    if (a.n_radios == 0 || a.n == 0 || a.rules.n == 0) return;
    const uint64_t n_work = (uint64_t)a.n_radios * a.rules.n;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n_work + 3) / 4, 1u << 20);
    hipLaunchKernelGGL(radio_ban_kernel, dim3(grid), dim3(256), 0, st, a.labels, a.from_labels, a.idx, a.n, a.n_radios, a.k, t, a.rules,
                       a.ban, a.ban_cnt);
}

void launch_radio_step(const RadioArgs& a, uint32_t t, const ChainPlan& p, hipStream_t st) {
    if (a.n_radios == 0 || a.n == 0) return;
    const dim3 grid(p.grid_cb * p.n_split);
    for_metric_form<true>(a.d, a.metric, a.m_is_diag, [&](auto D, auto M, auto G) {
        hipLaunchKernelGGL((radio_step_kernel<D(), M(), G()>), grid, dim3(256), 0, st, a.X, a.n, a.d, a.metric, a.M, a.from, a.skip, a.labels,
                           a.rules, a.ban, a.ban_cnt, a.nearest, a.n_radios, a.k, t, p.qb, p.n_split, p.blocks_per_split, a.idx, a.dist,
                           a.best, a.nan_flag);
    });
    if (p.n_split > 1)
        hipLaunchKernelGGL(radio_put_kernel, dim3((a.n_radios + 255u) / 256u), dim3(256), 0, st, a.best, a.n_radios, a.k, t, a.idx,
                           a.dist);
}

}  // namespace bg
