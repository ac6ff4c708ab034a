// kernels_knn.hip -- the k nearest candidates of every query, without the distance matrix (compiled with -ffp-contract=off).
//
// Reference: closest_to_songs (src/playlist.rs:256-270) for ONE seed, cut after k -- what Library::playlist_from(&[song])
// .take(k) (src/library.rs:762-850) asks per song: the candidates in ascending distance, equal distances in candidate order.
// Here for q seeds at once.  The distances are those of the all-pairs kernel bit for bit (pair_sum of pairwise_math.hpp, the
// correctly rounded square root, IEEE division), so the selection is a discrete result: the k smallest 64-bit keys
//   (f32_key(distance) << 32) | candidate index
// in ascending order.  Keys are distinct, so neither the order in which candidates are met nor the way the work is split
// changes the answer.
//
//   knn_scan_kernel   a workgroup owns up to QB queries (rows in LDS, read as broadcasts) and walks a range of 256-candidate
//                     blocks; a block is staged in LDS with coalesced loads and each lane takes four of its candidates into
//                     registers (as the all-pairs kernel keeps its columns).  Query r belongs to wavefront r % 4, which keeps
//                     its state in LDS: a buffer of `cap` keys, their count, and the rejection threshold = the k-th smallest
//                     key as of the last compaction.  A row against the wavefront's 256 candidates is four packed sums and ONE
//                     float comparison per candidate against a bound derived from the threshold; only when some lane passes it
//                     does the wavefront take the square roots, build the keys, compare them exactly and append the survivors
//                     (ballot + prefix count).  A full buffer is compacted: bitonic sort of the cap keys by the wavefront, the
//                     first k stay.  At the end of the range the sorted first k keys of every query go to `part`.
//   knn_merge_kernel  a wavefront per query: the n_split partial lists through the same threshold buffer, then keys -> (index,
//                     distance) with the 0xFFFFFFFF / +inf padding.  With one split per query it only converts.
//
// The bound (euclidean / Mahalanobis): the square root is taken for survivors only, but ordering by the sum is not ordering by
// the rounded root -- neighbouring sums share a root, and ties go to the lower index.  With t the threshold's distance and
// u = the next float above t, any sum s > u * u (rounded up) has sqrt(s) > u exactly, hence a rounded root >= u > t: rejected
// for certain.  Every other sum -- NaN and negative sums included, the comparison is written `!(s > bound)` -- takes the root and
// the exact 64-bit comparison.  Cosine and the generic-d path compare the distance itself against t.
//
// The keys, the wavefront's bitonic sort and the threshold buffer (KnnList) live in knn_list.hpp, shared with kernels_group_knn.hip.
#include <math.h>

#include <algorithm>

#include "device_utils.hpp"
#include "internal.hpp"
#include "knn_list.hpp"
#include "pairwise_math.hpp"
#include "playlist_math.hpp"

namespace bg {

// D > 0: compile-time feature count (packed arithmetic, candidates in registers).  D == 0: any d <= 64 through pl_distance,
// candidates read from global memory / L2 (slow, exact).
template <int D, int METRIC, bool DIAG, int KEYS>
__global__ __launch_bounds__(256, (KEYS == KNN_KEYS_SMALL ? 2 : 1)) void knn_scan_kernel(
    const float* __restrict__ Q, uint64_t q, const float* __restrict__ X, uint32_t n, uint32_t d_rt, int metric_rt,
    const float* __restrict__ M, const uint32_t* __restrict__ skip, uint32_t k, uint32_t cap, uint32_t qb_rt,
    uint32_t n_split, uint32_t blocks_per_split, unsigned long long* __restrict__ part, uint32_t* nan_flag, uint32_t* bad_flag) {
    constexpr bool GENERIC = D == 0;
    constexpr int DQ = GENERIC ? PL_DMAX : ((D + 3) & ~3);  // LDS pitch of a query row: 16-byte aligned -> ds_read_b128 broadcasts
    constexpr int XP = GENERIC ? 1 : (D | 1);               // LDS pitch of a staged candidate: odd, lanes l and l + 1 on different banks
    constexpr bool FLAT = XP == D;                          // (an odd d: the staged block is a plain copy of its rows)
    constexpr bool ROOT = !GENERIC && METRIC != METRIC_COSINE;  // the bound is on the sum before the square root
    __shared__ __attribute__((aligned(16))) unsigned long long s_buf[KEYS];
    __shared__ __attribute__((aligned(16))) float s_q[KNN_QMAX][DQ];
    __shared__ __attribute__((aligned(16))) float s_x[GENERIC ? 4 : KNN_COLS * XP];
    __shared__ float s_m[(!GENERIC && METRIC == METRIC_MAHALANOBIS) ? D * D : 1];
    __shared__ float s_nq[KNN_QMAX];
    __shared__ unsigned long long s_thr[KNN_QMAX];
    __shared__ float s_bound[KNN_QMAX];
    __shared__ uint32_t s_cnt[KNN_QMAX], s_skip[KNN_QMAX];

    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const uint32_t d = GENERIC ? d_rt : (uint32_t)D;
    const uint32_t QB = qb_rt;  // queries per workgroup: at most KEYS / cap, and at most KNN_QMAX (cap >= 128)
    const uint32_t split = blockIdx.x % n_split;
    const uint64_t qb_step = gridDim.x / n_split;
    const uint64_t n_qb = (q + QB - 1) / QB;
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

    for (uint64_t qb = blockIdx.x / n_split; qb < n_qb; qb += qb_step) {
        const uint64_t q0 = qb * QB;
        const uint32_t rows_here = (q - q0 < (uint64_t)QB) ? (uint32_t)(q - q0) : QB;
        __syncthreads();  // every wavefront has finished with the previous query block
        for (uint32_t e = (uint32_t)tid; e < rows_here * d; e += 256u) s_q[e / d][e % d] = Q[q0 * d + e];
        if ((uint32_t)tid < rows_here) {
            uint32_t s = skip ? skip[q0 + (uint32_t)tid] : 0xFFFFFFFFu;
            if (s != 0xFFFFFFFFu && s >= n) {  // reported to the host by the entry point; the query then skips nothing
                atomicOr(bad_flag, 1u);
                s = 0xFFFFFFFFu;
            }
            s_skip[tid] = s;
            s_cnt[tid] = 0u;
            s_thr[tid] = KNN_NONE;
            s_bound[tid] = INFINITY;
        }
        __syncthreads();
        if (!GENERIC && METRIC == METRIC_COSINE) {
            if ((uint32_t)tid < rows_here) {
                const float* a = s_q[tid];
                s_nq[tid] = sqrtf(unrolled_dot<(GENERIC ? 1 : D)>([&](int kk) { return a[kk]; }, [&](int kk) { return a[kk]; }));
            }
            __syncthreads();
        }

        // (Fetching the next block's rows into registers before the row loop of the current one -- a software pipeline of the
        // candidate stream -- was measured: 24 more registers, 2 % slower at k = 1 and 7 % at k = 32.)
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
            // re-made per block: the row loop's LDS addresses are scalar arithmetic, not per-lane values kept in registers
            const uint32_t wave_u = (uint32_t)__builtin_amdgcn_readfirstlane(wave);
            // (two rows per trip in one basic block, as in the all-pairs kernel's A != B form, was measured: 20.1 against 20.2 ms)
#pragma unroll 1
            for (uint32_t r = wave_u; r < rows_here; r += 4u) {
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
                    // (general M: one pair's 2 x d differences and products at a time -- interleaved by the scheduler, the two
                    // pairs spill 464 B per lane instead of 208)
                    if (METRIC == METRIC_MAHALANOBIS && !DIAG) asm volatile("" : "+v"(s0));
                    f2 s1 = pair_sum<(GENERIC ? 1 : D), METRIC, DIAG>(ap, bp[1], wdiag, s_m);
                    if (METRIC == METRIC_COSINE) {
                        s0 = splat(1.0f) - s0 / (splat(s_nq[r]) * nb[0]);
                        s1 = splat(1.0f) - s1 / (splat(s_nq[r]) * nb[1]);
                    }
                    pv[0] = s0.x; pv[1] = s0.y; pv[2] = s1.x; pv[3] = s1.y;
                }
                // wave-uniform: can any of the wavefront's 256 candidates enter the query's k best?  (`!(v > bound)`: a NaN says yes)
                const float bound = s_bound[r];
                const bool maybe = !(pv[0] > bound) || !(pv[1] > bound) || !(pv[2] > bound) || !(pv[3] > bound);
                if (__ballot(maybe) == 0ull) continue;
                // the exact part: distances, keys, the 64-bit comparison with the threshold, survivors into the query's buffer
                KnnList list{s_buf + (size_t)r * cap, s_cnt[r], s_thr[r]};
                const uint32_t skip_r = s_skip[r];
                const unsigned long long thr_in = list.thr;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const uint32_t lc = 64u * (uint32_t)c + (uint32_t)lane, j = j0 + lc;  // (j is only used where lc < cols_here)
                    const bool valid = lc < cols_here && j != skip_r;  // a skipped pair is not evaluated: its value is never looked at
                    const float v = ROOT ? sqrtf(pv[c]) : pv[c];
                    if (valid && v != v) saw_nan = true;
                    const unsigned long long key = ((unsigned long long)f32_key(v) << 32) | j;
                    list.push(valid && key < list.thr, key, k, cap, lane);
                }
                if (lane == 0) {
                    s_cnt[r] = list.cnt;
                    if (list.thr != thr_in) {
                        s_thr[r] = list.thr;
                        s_bound[r] = knn_bound<ROOT>(list.thr);
                    }
                }
                knn_wave_sync();
            }
        }
        // the sorted k best of this range (padded when it held fewer)
        for (uint32_t r = (uint32_t)wave; r < rows_here; r += 4u) {
            unsigned long long* buf = s_buf + (size_t)r * cap;
            knn_sort(buf, s_cnt[r], cap, lane);
            unsigned long long* dst = part + ((q0 + r) * n_split + split) * (uint64_t)k;
            for (uint32_t i = (uint32_t)lane; i < k; i += 64u) dst[i] = buf[i];
        }
    }
    if (saw_nan) atomicOr(nan_flag, 1u);
}

// part[query][split][k] (each list ascending, padded with KNN_NONE) -> idx / dist [query][k]
__global__ __launch_bounds__(256) void knn_merge_kernel(const unsigned long long* __restrict__ part, uint64_t q, uint32_t k,
                                                        uint32_t cap, uint32_t n_split, uint32_t* __restrict__ idx,
                                                        float* __restrict__ dist) {
    __shared__ __attribute__((aligned(16))) unsigned long long s_buf[4 * 2048];
    const int lane = lane_id(), wave = wave_id();
    for (uint64_t qi = (uint64_t)blockIdx.x * 4 + (uint64_t)wave; qi < q; qi += (uint64_t)gridDim.x * 4) {
        const unsigned long long* src = part + qi * n_split * (uint64_t)k;
        if (n_split > 1) {
            KnnList list{s_buf + (size_t)wave * cap, 0u, KNN_NONE};
            for (uint32_t s = 0; s < n_split; s++) {
                for (uint32_t i0 = 0; i0 < k; i0 += 64u) {
                    const uint32_t i = i0 + (uint32_t)lane;
                    const unsigned long long key = i < k ? src[(uint64_t)s * k + i] : KNN_NONE;
                    // (ascending lists: once a whole group is rejected the rest of the list is too)
                    const bool take = key != KNN_NONE && key < list.thr;
                    if (__ballot(take) == 0ull) break;
                    list.push(take, key, k, cap, lane);
                }
            }
            knn_sort(list.buf, list.cnt, cap, lane);
            src = list.buf;
        }
        for (uint32_t i = (uint32_t)lane; i < k; i += 64u) {
            const unsigned long long key = src[i];
            idx[qi * k + i] = (uint32_t)(key & 0xFFFFFFFFull);
            if (dist) dist[qi * k + i] = key == KNN_NONE ? INFINITY : knn_key_dist(key);
        }
        knn_wave_sync();  // the list is read before the wavefront's next query overwrites it
    }
}

KnnPlan knn_plan(uint64_t q, uint64_t n, uint32_t k, int n_cus) {
    KnnPlan p{};
    uint32_t p2 = 64;
    while (p2 < k) p2 <<= 1;
    p.cap = 2 * p2;  // a power of two with cap - k >= 64: room for one wavefront's survivors right after a compaction
    p.qb = (uint32_t)(p.cap <= 256 ? KNN_KEYS_SMALL : KNN_KEYS_BIG) / p.cap;
    // whole rounds: with `slots` workgroups resident at a time, ceil(n_qb / slots) rounds pass whatever the last one holds, so
    // the queries are spread evenly over that many full rounds (100 000 queries, 32 each: 3125 workgroups = 6.1 rounds of 512
    // take the time of 7; 28 each fill 7 rounds)
    {
        const uint64_t slots = (uint64_t)cus_or_default(n_cus) * (p.cap <= 256 ? 2 : 1);
        const uint64_t rounds = ((q + p.qb - 1) / p.qb + slots - 1) / slots;
        const uint64_t even = (q + rounds * slots - 1) / (rounds * slots);  // queries per workgroup that fill the rounds
        p.qb = (uint32_t)std::min<uint64_t>(p.qb, std::max<uint64_t>(4, (even + 3) / 4 * 4));  // whole rows per wavefront
    }
    const uint64_t n_qb = (q + p.qb - 1) / p.qb;
    const uint64_t n_blocks = (n + KNN_COLS - 1) / KNN_COLS;
    // few queries: several workgroups share a query's candidates (at least eight blocks each) until the device has ~4 per CU
    const uint64_t want = (uint64_t)4 * cus_or_default(n_cus);
    uint64_t split = n_qb ? want / n_qb : 1;
    split = std::min<uint64_t>(split, (n_blocks + 7) / 8);
    split = std::max<uint64_t>(split, 1);
    p.blocks_per_split = (uint32_t)std::max<uint64_t>(1, (n_blocks + split - 1) / split);
    p.n_split = (uint32_t)std::max<uint64_t>(1, (n_blocks + p.blocks_per_split - 1) / p.blocks_per_split);
    p.grid_qb = (uint32_t)std::min<uint64_t>(n_qb, 1u << 20);
    p.part_keys = q * p.n_split * (uint64_t)k;
    return p;
}

void launch_knn_scan(const float* Q, uint64_t q, const float* X, uint32_t n, uint32_t d, int metric, const float* M,
                     int m_is_diag, const uint32_t* skip, uint32_t k, const KnnPlan& p, unsigned long long* part,
                     uint32_t* nan_flag, uint32_t* bad_flag, hipStream_t st) {
    const dim3 grid(p.grid_qb * p.n_split);
    const auto scan = [&](auto D_, auto KEYS) {
        for_metric_form<true>(D_, metric, m_is_diag, [&](auto D, auto M_, auto G) {
            hipLaunchKernelGGL((knn_scan_kernel<D(), M_(), G(), decltype(KEYS)::value>), grid, dim3(256), 0, st, Q, q, X, n, d, metric, M,
                               skip, k, p.cap, p.qb, p.n_split, p.blocks_per_split, part, nan_flag, bad_flag);
        });
    };
    with_d(d, [&](auto D) {
        if (p.cap <= 256) scan(D, std::integral_constant<int, KNN_KEYS_SMALL>{});
        else scan(D, std::integral_constant<int, KNN_KEYS_BIG>{});
    });
}

void launch_knn_merge(const unsigned long long* part, uint64_t q, uint32_t k, const KnnPlan& p, uint32_t* idx, float* dist,
                      hipStream_t st) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((q + 3) / 4, 1u << 20);
    hipLaunchKernelGGL(knn_merge_kernel, dim3(grid), dim3(256), 0, st, part, q, k, p.cap, p.n_split, idx, dist);
}

}  // namespace bg
