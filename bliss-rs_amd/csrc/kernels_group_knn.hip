// kernels_group_knn.hip -- the k nearest candidates of every seed GROUP, without a groups x candidates matrix (compiled with
// -ffp-contract=off).
//
// Reference: closest_to_songs under FunctionDistanceMetric (src/playlist.rs:36-59, 256-270) cut after k -- what
// Library::playlist_from(&[several songs]).take(k) (src/library.rs:762-842) asks per album, artist or saved playlist: a
// candidate's score is the sequential f32 sum, in seed order, of the metric to each seed of the group; the candidates come in
// ascending score, equal scores in candidate order.  Here for G groups at once.  The score is what set_distance_kernel writes
// for the same seeds bit for bit (every pair takes its correctly rounded root / IEEE division before it is added), so the
// selection is a discrete result: the k smallest keys (f32_key(score) << 32) | candidate index, as in kernels_knn.hip.
//
//   group_knn_scan_kernel   a workgroup takes one ITEM of the plan: groups [g_lo, g_hi) x candidates [c_lo, c_hi).  It walks the
//                           groups in chunks of QB (one threshold buffer each, as a query of knn_scan_kernel has); per chunk it
//                           walks the 256-candidate blocks: a block is staged in LDS and each lane takes four candidates into
//                           registers.  Group r of the chunk belongs to wavefront r % 4, which runs the chain over the group's
//                           seeds with the four running scores in registers.  Seeds reach the lanes as LDS broadcasts: the
//                           small groups of a chunk (<= GK_SEED_TILE seeds, GK_RESIDENT in all) stay in LDS for the whole
//                           chunk; any other group streams through a tile of GK_STREAM rows that its wavefront owns, the
//                           next tile already on its way in registers.  A chain never restarts: a group is never split over
//                           wavefronts or workgroups by SEEDS, only by candidates.  After the last seed the scores meet the
//                           group's threshold distance (`!(score > t)`, a NaN passes); only when some lane passes does the
//                           wavefront build the 256-bit mask of the group's skipped candidates in this block, the keys, and
//                           append the survivors to the group's list.  At the end of a chunk the sorted first k keys of every
//                           group go to the list slot (list_off[g] + the item's split index).
//   group_knn_merge_kernel  a wavefront per group: its list_off[g + 1] - list_off[g] partial lists through the same threshold
//                           buffer, then keys -> (index, score) with the 0xFFFFFFFF / +inf padding.
//
//   group_weights_kernel   the per-group metric (blissgpu_group_knn_weighted with weights == NULL): variance_based_weight_matrix
//                           (src/playlist.rs:173-221) of every group's own seeds, a wavefront per group, lane j owning
//                           dimension j.  The scan's PERGROUP form then takes the diagonal of M from row g of that array
//                           (or of the caller's) each time a wavefront turns to its next group.
//
// group_knn_plan deals the groups x candidates plane out in items of bounded cost (seeds x candidates): see there.
#include <math.h>

#include <algorithm>

#include "device_utils.hpp"
#include "internal.hpp"
#include "knn_list.hpp"
#include "pairwise_math.hpp"
#include "playlist_math.hpp"

namespace bg {

constexpr int GK_SEED_TILE = GROUP_KNN_SEED_TILE;  // a group of at most this many seeds may stay in LDS for a whole chunk
constexpr int GK_STREAM = 16;                      // rows of a streamed tile (32 cost 12 registers in flight and, at d = 23, scratch)
constexpr int GK_RESIDENT = 192;                   // seed rows of a chunk's small groups kept in LDS across the candidate blocks
constexpr uint32_t GK_NONE = 0xFFFFFFFFu;

// METRIC: METRIC_MAHALANOBIS means a DIAGONAL M here (general M takes the generic path)
template <int D, int METRIC>
struct GkMath {
    static constexpr int DQ = (D + 3) & ~3;  // LDS pitch of a seed row: 16-byte aligned -> ds_read_b128 broadcasts
    // acc[c] += m(seed_s, candidate c) for the cnt seed rows at `rows` (pitch DQ), in order
    static __device__ __forceinline__ void chain(const float* rows, const float* norms, uint32_t cnt, const f2 (&bp0)[D],
                                                 const f2 (&bp1)[D], const f2 (&nb)[2], const float (&wdiag)[D], float (&acc)[4]) {
        const float none[1] = {0.0f};
#pragma unroll 1
        for (uint32_t s = 0; s < cnt; s++) {
            f2 ap[DQ / 2];
#pragma unroll
            for (int k4 = 0; k4 < DQ / 4; k4++) {  // same address in every lane: LDS broadcast
                const float4 v = *reinterpret_cast<const float4*>(rows + s * DQ + 4 * k4);
                ap[2 * k4].x = v.x; ap[2 * k4].y = v.y; ap[2 * k4 + 1].x = v.z; ap[2 * k4 + 1].y = v.w;
            }
            f2 s0 = pair_sum<D, METRIC, METRIC == METRIC_MAHALANOBIS>(ap, bp0, wdiag, none);
            f2 s1 = pair_sum<D, METRIC, METRIC == METRIC_MAHALANOBIS>(ap, bp1, wdiag, none);
            if (METRIC == METRIC_COSINE) {
                const float na = norms[s];
                s0 = splat(1.0f) - s0 / (splat(na) * nb[0]);
                s1 = splat(1.0f) - s1 / (splat(na) * nb[1]);
            } else {
                s0.x = sqrtf(s0.x); s0.y = sqrtf(s0.y); s1.x = sqrtf(s1.x); s1.y = sqrtf(s1.y);
            }
            acc[0] = acc[0] + s0.x; acc[1] = acc[1] + s0.y; acc[2] = acc[2] + s1.x; acc[3] = acc[3] + s1.y;
        }
    }
};

// pl_distance(a, b, d, PL_MAHALANOBIS, diag(w)) without the d x d matrix.  Column jj of the reference's vector-matrix product
// is 0.0 + ... + diff_jj * w_jj + ... with every other term diff_ii * 0.0: a zero of either sign while every difference is
// finite (the sum starts at +0.0, so the signs never show), a NaN as soon as one is not.  `poison` carries exactly that: it is
// +0.0 or NaN, and reaches the result only when another column exists (d >= 2).
__device__ __forceinline__ float gk_distance_diag(const float* a, const float* b, uint32_t d, const float* __restrict__ w) {
    float poison = 0.0f;
    for (uint32_t kk = 0; kk < d; kk++) poison = poison + (a[kk] - b[kk]) * 0.0f;
    const float q = pl_udot([&](uint32_t kk) { return 0.0f + (a[kk] - b[kk]) * w[kk]; }, [&](uint32_t kk) { return a[kk] - b[kk]; }, d);
    return sqrtf(d >= 2u ? q + poison : q);
}

// D > 0: compile-time feature count, euclidean / cosine / diagonal M.  D == 0: any d <= 64 and any M through pl_distance, seeds
// and candidates read from global memory / L2 (slow, exact).
// PERGROUP (Mahalanobis only): M is not one d x d matrix but [n_groups][d], row g the DIAGONAL of group g's matrix.  The group a
// wavefront works on is wave-uniform, so its row is fetched with scalar loads into the registers the shared diagonal occupies
// in the other form; every other instantiation compiles to what it was.
template <int D, int METRIC, int KEYS, bool PERGROUP = false>
__global__ __launch_bounds__(256, (KEYS == KNN_KEYS_SMALL ? 2 : 1)) void group_knn_scan_kernel(
    const float* __restrict__ S, const uint32_t* __restrict__ goff, const float* __restrict__ X, uint32_t n, uint32_t d_rt,
    int metric_rt, const float* __restrict__ M, const uint32_t* __restrict__ skip, uint32_t k, uint32_t cap, uint32_t qb_rt,
    const GroupKnnItem* __restrict__ items, const uint32_t* __restrict__ list_off, unsigned long long* __restrict__ part,
    uint32_t* nan_flag, uint32_t* bad_flag) {
    constexpr bool GENERIC = D == 0;
    constexpr int DD = GENERIC ? 1 : D;
    constexpr int DQ = GENERIC ? 4 : ((D + 3) & ~3);
    constexpr int XP = GENERIC ? 1 : (D | 1);  // LDS pitch of a staged candidate: odd, lanes l and l + 1 on different banks
    constexpr bool FLAT = XP == D;
    constexpr int PRE = GENERIC ? 1 : (GK_STREAM * D + 63) / 64;  // registers of a tile on its way
    static_assert(GENERIC || 4 * GK_STREAM * DQ <= KNN_COLS * XP, "the four seed tiles live in the staged block's LDS");
    __shared__ __attribute__((aligned(16))) unsigned long long s_buf[KEYS];
    // the staged candidate block; once every wavefront has taken its candidates into registers, the four wavefronts' seed tiles
    __shared__ __attribute__((aligned(16))) float s_x[GENERIC ? 4 : KNN_COLS * XP];
    __shared__ __attribute__((aligned(16))) float s_res[GENERIC ? 4 : GK_RESIDENT * DQ];
    __shared__ float s_rnq[(!GENERIC && METRIC == METRIC_COSINE) ? GK_RESIDENT : 1];
    __shared__ float s_tnq[4][(!GENERIC && METRIC == METRIC_COSINE) ? GK_STREAM : 1];
    __shared__ uint32_t s_rsrc[GK_RESIDENT], s_rskip[GK_RESIDENT];
    __shared__ uint32_t s_mask[4][8];
    __shared__ unsigned long long s_thr[KNN_QMAX];
    __shared__ float s_bound[KNN_QMAX];
    __shared__ uint32_t s_cnt[KNN_QMAX], s_g0[KNN_QMAX], s_gn[KNN_QMAX], s_roff[KNN_QMAX];
    __shared__ uint32_t s_used;

    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const uint32_t d = GENERIC ? d_rt : (uint32_t)D;
    const uint32_t QB = qb_rt;  // groups per chunk: at most KEYS / cap, and at most KNN_QMAX
    const GroupKnnItem it = items[blockIdx.x];
    const uint32_t blk0 = it.c_lo / (uint32_t)KNN_COLS;
    const uint32_t blk1 = (uint32_t)(((uint64_t)it.c_hi + KNN_COLS - 1) / KNN_COLS);
    bool saw_nan = false;

    static_assert(!PERGROUP || METRIC == METRIC_MAHALANOBIS, "a per-group diagonal is a Mahalanobis metric");
    float wdiag[DD];
#pragma unroll
    for (int kk = 0; kk < DD; kk++) wdiag[kk] = (!GENERIC && !PERGROUP && METRIC == METRIC_MAHALANOBIS) ? M[kk * DD + kk] : 0.0f;  // (uniform: scalar registers)

    for (uint32_t gc = it.g_lo; gc < it.g_hi; gc += QB) {
        const uint32_t rows_here = (it.g_hi - gc < QB) ? it.g_hi - gc : QB;
        __syncthreads();  // every wavefront has finished with the previous chunk
        if ((uint32_t)tid < rows_here) {
            const uint32_t a = goff[gc + (uint32_t)tid], b = goff[gc + (uint32_t)tid + 1u];
            s_g0[tid] = a;
            s_gn[tid] = b - a;
            s_cnt[tid] = 0u;
            s_thr[tid] = KNN_NONE;
            s_bound[tid] = INFINITY;
        }
        __syncthreads();
        if (tid == 0) {  // which groups of the chunk keep their seeds in LDS: small ones, first come first served
            uint32_t used = 0;
            for (uint32_t r = 0; r < rows_here; r++) {
                const uint32_t gn = s_gn[r];
                if (!GENERIC && gn <= (uint32_t)GK_SEED_TILE && used + gn <= (uint32_t)GK_RESIDENT) {
                    s_roff[r] = used;
                    for (uint32_t i = 0; i < gn; i++) s_rsrc[used + i] = s_g0[r] + i;
                    used += gn;
                } else {
                    s_roff[r] = GK_NONE;
                }
            }
            s_used = used;
        }
        __syncthreads();
        if constexpr (!GENERIC) {
            const uint32_t used = s_used;
            for (uint32_t e = (uint32_t)tid; e < used * (uint32_t)D; e += 256u)
                s_res[(e / (uint32_t)D) * DQ + e % (uint32_t)D] = S[(uint64_t)s_rsrc[e / (uint32_t)D] * D + e % (uint32_t)D];
            if ((uint32_t)tid < used) s_rskip[tid] = skip ? skip[s_rsrc[tid]] : GK_NONE;
            __syncthreads();
            if (METRIC == METRIC_COSINE && (uint32_t)tid < used) {
                const float* a = s_res + (uint32_t)tid * DQ;
                s_rnq[tid] = sqrtf(unrolled_dot<DD>([&](int kk) { return a[kk]; }, [&](int kk) { return a[kk]; }));
            }
            // (the first block's barriers below order these writes before the wavefronts read them)
        }

        for (uint32_t blk = blk0; blk < blk1; blk++) {
            const uint32_t j0 = blk * (uint32_t)KNN_COLS;
            const uint32_t cols_here = (n - j0 < (uint32_t)KNN_COLS) ? n - j0 : (uint32_t)KNN_COLS;
            // the lane's four candidates as two packed pairs: bp[h][kk] = (candidate 2h, candidate 2h + 1), candidate c = row
            // j0 + 64 c + lane
            f2 bp[2][DD];
            f2 nb[2];
            if constexpr (!GENERIC) {
                __syncthreads();  // every wavefront has finished with the previous block's seed tiles
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
                    for (int kk = 0; kk < DD; kk++) {
                        bp[h][kk].x = s_x[la * XP + kk];
                        bp[h][kk].y = s_x[lb * XP + kk];
                    }
                    if (METRIC == METRIC_COSINE) {
                        const f2 qq = unrolled_dot2<DD>([&](int kk) { return bp[h][kk]; }, [&](int kk) { return bp[h][kk]; });
                        nb[h].x = sqrtf(qq.x);
                        nb[h].y = sqrtf(qq.y);
                    }
                }
                __syncthreads();  // the block is in registers: its LDS now holds the seed tiles
            }
            const uint32_t wave_u = (uint32_t)__builtin_amdgcn_readfirstlane(wave);
#pragma unroll 1
            for (uint32_t r = wave_u; r < rows_here; r += 4u) {
                const uint32_t g0 = s_g0[r], gn = s_gn[r], roff = s_roff[r];
                float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // the running scores of the lane's four candidates
                // the group's own diagonal (gc + r is wave-uniform: scalar loads, scalar registers)
                const float* wrow = PERGROUP ? M + (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(gc + r)) * d : nullptr;
                if constexpr (PERGROUP && !GENERIC) {
#pragma unroll
                    for (int kk = 0; kk < DD; kk++) wdiag[kk] = wrow[kk];
                }
                if constexpr (GENERIC) {
#pragma unroll 1
                    for (int c = 0; c < 4; c++) {
                        const uint32_t lc = 64u * (uint32_t)c + (uint32_t)lane;
                        if (lc < cols_here) {
                            const float* x = X + (uint64_t)(j0 + lc) * d;
                            float a = 0.0f;
                            if constexpr (PERGROUP) {
                                for (uint32_t s = 0; s < gn; s++) a = a + gk_distance_diag(S + (uint64_t)(g0 + s) * d, x, d, wrow);
                            } else {
                                for (uint32_t s = 0; s < gn; s++) a = a + pl_distance(S + (uint64_t)(g0 + s) * d, x, d, metric_rt, M);
                            }
                            acc[c] = a;
                        } else {
                            acc[c] = INFINITY;
                        }
                    }
                } else {
                    using Math = GkMath<DD, METRIC>;
                    if (roff != GK_NONE) {
                        Math::chain(s_res + roff * DQ, s_rnq + (METRIC == METRIC_COSINE ? roff : 0u), gn, bp[0], bp[1], nb, wdiag, acc);
                    } else {
                        // stream the group's rows through the wavefront's tile; the next tile travels while this one is used
                        float* tile = s_x + (uint32_t)wave_u * (uint32_t)(GK_STREAM * DQ);
                        float* tnq = s_tnq[METRIC == METRIC_COSINE ? wave_u : 0u];
                        float pre[PRE];
                        auto fetch = [&](uint32_t t0) __attribute__((always_inline)) {
                            const uint32_t cnt = (gn - t0 < (uint32_t)GK_STREAM) ? gn - t0 : (uint32_t)GK_STREAM;
                            const float* src = S + (uint64_t)(g0 + t0) * D;
#pragma unroll
                            for (int i = 0; i < PRE; i++) {
                                const uint32_t e = (uint32_t)lane + 64u * (uint32_t)i;
                                pre[i] = e < cnt * (uint32_t)D ? src[e] : 0.0f;
                            }
                        };
                        fetch(0u);
#pragma unroll 1
                        for (uint32_t t0 = 0; t0 < gn; t0 += (uint32_t)GK_STREAM) {
                            const uint32_t cnt = (gn - t0 < (uint32_t)GK_STREAM) ? gn - t0 : (uint32_t)GK_STREAM;
                            knn_wave_sync();  // the previous tile has been read
#pragma unroll
                            for (int i = 0; i < PRE; i++) {
                                const uint32_t e = (uint32_t)lane + 64u * (uint32_t)i;
                                if (e < cnt * (uint32_t)D) tile[(e / (uint32_t)D) * DQ + e % (uint32_t)D] = pre[i];
                            }
                            knn_wave_sync();
                            if (METRIC == METRIC_COSINE) {
                                if ((uint32_t)lane < cnt) {
                                    const float* a = tile + (uint32_t)lane * DQ;
                                    tnq[lane] = sqrtf(unrolled_dot<DD>([&](int kk) { return a[kk]; }, [&](int kk) { return a[kk]; }));
                                }
                                knn_wave_sync();
                            }
                            if (t0 + (uint32_t)GK_STREAM < gn) fetch(t0 + (uint32_t)GK_STREAM);
                            Math::chain(tile, tnq, cnt, bp[0], bp[1], nb, wdiag, acc);
                        }
                    }
                }
                // wave-uniform: can any of the wavefront's 256 candidates enter the group's k best?  (`!(v > t)`: a NaN says yes)
                const float bound = s_bound[r];
                const bool maybe = !(acc[0] > bound) || !(acc[1] > bound) || !(acc[2] > bound) || !(acc[3] > bound);
                if (__ballot(maybe) == 0ull) continue;
                // the group's skipped candidates of this block as a 256-bit mask
                uint32_t* mask = s_mask[wave_u];
                if (lane < 8) mask[lane] = 0u;
                knn_wave_sync();
                if (skip) {
                    for (uint32_t e = (uint32_t)lane; e < gn; e += 64u) {
                        const uint32_t s = (roff != GK_NONE) ? s_rskip[roff + e] : skip[g0 + e];
                        if (s == GK_NONE) continue;
                        if (s >= n) atomicOr(bad_flag, 1u);  // reported to the host by the entry point
                        else if (s >= j0 && s - j0 < (uint32_t)KNN_COLS) atomicOr(&mask[(s - j0) >> 5], 1u << ((s - j0) & 31u));
                    }
                    knn_wave_sync();
                }
                // the exact part: keys, the 64-bit comparison with the threshold, survivors into the group's buffer
                KnnList list{s_buf + (size_t)r * cap, s_cnt[r], s_thr[r]};
                const unsigned long long thr_in = list.thr;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const uint32_t lc = 64u * (uint32_t)c + (uint32_t)lane, j = j0 + lc;  // (j is only used where lc < cols_here)
                    const bool skipped = ((mask[lc >> 5] >> (lc & 31u)) & 1u) != 0u;
                    const bool valid = lc < cols_here && !skipped;  // a skipped candidate's score is never looked at
                    const float v = acc[c];
                    if (valid && v != v) saw_nan = true;
                    const unsigned long long key = ((unsigned long long)f32_key(v) << 32) | j;
                    list.push(valid && key < list.thr, key, k, cap, lane);
                }
                if (lane == 0) {
                    s_cnt[r] = list.cnt;
                    if (list.thr != thr_in) {
                        s_thr[r] = list.thr;
                        s_bound[r] = knn_bound<false>(list.thr);
                    }
                }
                knn_wave_sync();
            }
        }
        // the sorted k best of this item's candidates (padded when it held fewer)
        for (uint32_t r = (uint32_t)wave; r < rows_here; r += 4u) {
            unsigned long long* buf = s_buf + (size_t)r * cap;
            knn_sort(buf, s_cnt[r], cap, lane);
            unsigned long long* dst = part + ((uint64_t)list_off[gc + r] + it.split) * (uint64_t)k;
            for (uint32_t i = (uint32_t)lane; i < k; i += 64u) dst[i] = buf[i];
        }
    }
    if (saw_nan) atomicOr(nan_flag, 1u);
}

// the lists list_off[g] .. list_off[g + 1] of part (k keys each, ascending, padded with KNN_NONE) -> idx / dist [group][k]
__global__ __launch_bounds__(256) void group_knn_merge_kernel(const unsigned long long* __restrict__ part,
                                                              const uint32_t* __restrict__ list_off, uint64_t n_groups, uint32_t k,
                                                              uint32_t cap, uint32_t* __restrict__ idx, float* __restrict__ dist) {
    __shared__ __attribute__((aligned(16))) unsigned long long s_buf[4 * 2048];
    const int lane = lane_id(), wave = wave_id();
    for (uint64_t g = (uint64_t)blockIdx.x * 4 + (uint64_t)wave; g < n_groups; g += (uint64_t)gridDim.x * 4) {
        const uint32_t l0 = list_off[g], n_lists = list_off[g + 1] - l0;
        const unsigned long long* src = part + (uint64_t)l0 * k;
        if (n_lists > 1) {
            KnnList list{s_buf + (size_t)wave * cap, 0u, KNN_NONE};
            for (uint32_t s = 0; s < n_lists; s++) {
                for (uint32_t i0 = 0; i0 < k; i0 += 64u) {
                    const uint32_t i = i0 + (uint32_t)lane;
                    const unsigned long long key = i < k ? src[(uint64_t)s * k + i] : KNN_NONE;
                    // (ascending lists: once a whole stretch is rejected the rest of the list is too)
                    const bool take = key != KNN_NONE && key < list.thr;
                    if (__ballot(take) == 0ull) break;
                    list.push(take, key, k, cap, lane);
                }
            }
            knn_sort(list.buf, list.cnt, cap, lane);
            src = list.buf;
        }
        for (uint32_t i = (uint32_t)lane; i < k; i += 64u) {
            const unsigned long long key = n_lists ? src[i] : KNN_NONE;  // (no candidates at all: padding only)
            idx[g * k + i] = (uint32_t)(key & 0xFFFFFFFFull);
            if (dist) dist[g * k + i] = key == KNN_NONE ? INFINITY : knn_key_dist(key);
        }
        knn_wave_sync();  // the list is read before the wavefront's next group overwrites it
    }
}

// variance_based_weight_matrix (src/playlist.rs:173-221) of every seed group: W[g][0..d) is the diagonal of the matrix the
// reference returns for the rows goff[g] .. goff[g + 1] of S.  A wavefront per group, lane j owns dimension j (d <= 64); both
// passes walk the group's rows in seed order -- the adds are a dependent chain, the loads are not, so eight rows travel at a
// time.  Every operation rounds on its own, in the reference's order:
//   mean = (0 + s_0 + s_1 + ...) / (float)count;  var = (0 + diff_0 * diff_0 + ...) / (float)count;  w = 1 / (var + 1e-6);
//   total = ndarray's sum() (unrolled_fold: eight partial sums over k mod 8 for the whole eights, 0 + (p0 + p4) + (p1 + p5) +
//   (p2 + p6) + (p3 + p7), then the tail in order) -- the lanes' weights meet in LDS and every lane adds them in that order;
//   w = w * ((float)d / total).
// A group of fewer than two seeds gets the identity's diagonal (euclidean_distance's own M, src/playlist.rs:69) and status 1.
__global__ __launch_bounds__(256) void group_weights_kernel(const float* __restrict__ S, const uint32_t* __restrict__ goff,
                                                            uint64_t n_groups, uint32_t d, float* __restrict__ W,
                                                            int32_t* __restrict__ status) {
    __shared__ float s_w[4][64];
    const int lane = lane_id(), wave = wave_id();
    const bool mine = (uint32_t)lane < d;
    const uint32_t col = mine ? (uint32_t)lane : 0u;  // (the idle lanes read column 0 and store nothing)
    for (uint64_t g = (uint64_t)blockIdx.x * 4 + (uint64_t)wave; g < n_groups; g += (uint64_t)gridDim.x * 4) {
        const uint32_t a = goff[g], cnt = goff[g + 1] - a;
        float w = 1.0f;
        if (cnt >= 2u) {  // (wave-uniform)
            const float* x = S + (uint64_t)a * d + col;
            const float ns = (float)cnt;
            float mean = 0.0f, var = 0.0f, v[8];
            uint32_t s = 0;
            for (; s + 8u <= cnt; s += 8u) {
#pragma unroll
                for (int i = 0; i < 8; i++) v[i] = x[(uint64_t)(s + (uint32_t)i) * d];
#pragma unroll
                for (int i = 0; i < 8; i++) mean = mean + v[i];
            }
            for (; s < cnt; s++) mean = mean + x[(uint64_t)s * d];
            mean = mean / ns;
            for (s = 0; s + 8u <= cnt; s += 8u) {
#pragma unroll
                for (int i = 0; i < 8; i++) v[i] = x[(uint64_t)(s + (uint32_t)i) * d];
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const float diff = v[i] - mean;
                    var = var + diff * diff;
                }
            }
            for (; s < cnt; s++) {
                const float diff = x[(uint64_t)s * d] - mean;
                var = var + diff * diff;
            }
            var = var / ns;
            w = 1.0f / (var + 1e-6f);
            s_w[wave][lane] = w;
            knn_wave_sync();
            const float* sw = s_w[wave];
            float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            uint32_t kk = 0;
            for (; kk + 8u <= d; kk += 8u)
#pragma unroll
                for (int u = 0; u < 8; u++) p[u] = p[u] + sw[kk + (uint32_t)u];
            float total = 0.0f;
            total = total + (p[0] + p[4]);
            total = total + (p[1] + p[5]);
            total = total + (p[2] + p[6]);
            total = total + (p[3] + p[7]);
            for (; kk < d; kk++) total = total + sw[kk];
            w = w * ((float)d / total);
            knn_wave_sync();  // the weights are read before the wavefront's next group overwrites them
        }
        if (mine) W[g * d + (uint64_t)lane] = w;
        if (status && lane == 0) status[g] = cnt >= 2u ? 0 : 1;
    }
}

// The plan.  An item is a rectangle of the groups x candidates plane; its cost is (seeds of its groups) x (its candidates).
// With total = all seeds x n and T = max(total / (4 n_cus), 256 x largest group):
//   * consecutive groups are gathered into a band while band seeds x n <= T; the band is ONE item over every candidate;
//   * a group that alone exceeds T is a band of its own, cut by candidates into items of whole 256-blocks.  Its chain cannot be
//     split, so one wavefront of the workgroup runs it: such an item gets a quarter of T (but at least eight blocks while
//     that stays within T, and never less than one block).
// Every item costs at most max(T, 256 x its group) <= max(total / n_cus, 256 x largest group).
GroupKnnPlan group_knn_plan(const uint64_t* off, uint64_t n_groups, uint64_t n, uint32_t k, uint32_t n_cus) {
    typedef unsigned __int128 u128;
    GroupKnnPlan p;
    uint32_t p2 = 64;
    while (p2 < k) p2 <<= 1;
    p.cap = 2 * p2;  // a power of two with cap - k >= 64 (see knn_plan)
    p.qb = std::min<uint32_t>((uint32_t)KNN_QMAX, (uint32_t)(p.cap <= 256 ? KNN_KEYS_SMALL : KNN_KEYS_BIG) / p.cap);
    p.cand_block = (uint32_t)KNN_COLS;
    p.seed_tile = (uint32_t)GK_SEED_TILE;
    p.list_off.assign(n_groups + 1, 0u);
    if (n_groups == 0 || n == 0) return p;
    const uint64_t n_blocks = (n + KNN_COLS - 1) / KNN_COLS;
    uint64_t gmax = 0;
    for (uint64_t g = 0; g < n_groups; g++) gmax = std::max(gmax, off[g + 1] - off[g]);
    const u128 total = (u128)off[n_groups] * n;
    const u128 T = std::max<u128>(total / ((u128)4 * std::max<uint32_t>(1u, n_cus)), (u128)KNN_COLS * gmax);
    uint64_t g = 0, lists = 0;
    while (g < n_groups) {
        const uint64_t s = off[g + 1] - off[g];
        if ((u128)s * n > T) {
            const u128 block_cost = (u128)s * KNN_COLS, eight = 8 * block_cost;
            u128 budget = T / 4;
            if (budget < eight) budget = std::min(T, eight);
            const uint64_t bpi = (uint64_t)std::min<u128>(n_blocks, std::max<u128>(1, budget / block_cost));
            uint32_t split = 0;
            for (uint64_t b = 0; b < n_blocks; b += bpi, split++)
                p.items.push_back({(uint32_t)g, (uint32_t)g + 1u, (uint32_t)(b * KNN_COLS),
                                   (uint32_t)std::min<uint64_t>(n, (b + bpi) * KNN_COLS), split});
            p.list_off[g] = (uint32_t)lists;
            lists += split;
            g++;
        } else {
            uint64_t g_hi = g, band = 0;
            while (g_hi < n_groups && (u128)(band + off[g_hi + 1] - off[g_hi]) * n <= T) {
                band += off[g_hi + 1] - off[g_hi];
                p.list_off[g_hi] = (uint32_t)lists++;
                g_hi++;
            }
            p.items.push_back({(uint32_t)g, (uint32_t)g_hi, 0u, (uint32_t)n, 0u});
            g = g_hi;
        }
    }
    p.list_off[n_groups] = (uint32_t)lists;
    return p;
}

void launch_group_knn_scan(const float* S, const uint32_t* goff, const float* X, uint32_t n, uint32_t d, int metric,
                           const float* M, int m_is_diag, const uint32_t* skip, uint32_t k, const GroupKnnPlan& p,
                           const GroupKnnItem* items, const uint32_t* list_off, unsigned long long* part, uint32_t* nan_flag,
                           uint32_t* bad_flag, hipStream_t st) {
    if (p.items.empty()) return;
    const dim3 grid((uint32_t)p.items.size());
    const bool pergroup = m_is_diag == GROUP_KNN_M_PER_GROUP;  // (Mahalanobis; M is [n_groups][d]: one diagonal per group)
    const bool packed = (d == 23 || d == 20) && (metric != METRIC_MAHALANOBIS || m_is_diag);  // general M: pl_distance
    with_d(packed ? d : 0u, [&](auto D_) {
        constexpr int D = decltype(D_)::value;
        const auto scan = [&](auto KEYS) {
            const auto go = [&](auto M_, auto PER) {
                hipLaunchKernelGGL((group_knn_scan_kernel<D, decltype(M_)::value, decltype(KEYS)::value, decltype(PER)::value>), grid,
                                   dim3(256), 0, st, S, goff, X, n, d, metric, M, skip, k, p.cap, p.qb, items, list_off, part, nan_flag,
                                   bad_flag);
            };
            // (the packed kernels' Mahalanobis M is always a diagonal -- see `packed` --, so the ladder's diagonal flag names nothing here)
            if (pergroup) go(std::integral_constant<int, METRIC_MAHALANOBIS>{}, std::true_type{});
            else for_metric_form<true>(D_, metric, m_is_diag, [&](auto, auto M_, auto) { go(M_, std::false_type{}); });
        };
        if (p.cap <= 256) scan(std::integral_constant<int, KNN_KEYS_SMALL>{});
        else scan(std::integral_constant<int, KNN_KEYS_BIG>{});
    });
}

void launch_group_weights(const float* S, const uint32_t* goff, uint64_t n_groups, uint32_t d, float* W, int32_t* status,
                          hipStream_t st) {
    if (n_groups == 0) return;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n_groups + 3) / 4, 1u << 20);
    hipLaunchKernelGGL(group_weights_kernel, dim3(grid), dim3(256), 0, st, S, goff, n_groups, d, W, status);
}

void launch_group_knn_merge(const unsigned long long* part, const uint32_t* list_off, uint64_t n_groups, uint32_t k,
                            const GroupKnnPlan& p, uint32_t* idx, float* dist, hipStream_t st) {
    if (n_groups == 0) return;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n_groups + 3) / 4, 1u << 20);
    hipLaunchKernelGGL(group_knn_merge_kernel, dim3(grid), dim3(256), 0, st, part, list_off, n_groups, k, p.cap, idx, dist);
}

}  // namespace bg
