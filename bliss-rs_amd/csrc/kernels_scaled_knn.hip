// kernels_scaled_knn.hip -- the k nearest candidates of every query under a LOCALLY SCALED distance, and how often every song is
// listed (compiled with -ffp-contract=off).  DESIGN.md 3.27.
//
// A raw nearest-neighbour search in 20 or 23 dimensions has hubs: a few songs near the middle of the library are in everyone's
// list, many songs in nobody's.  Local scaling (Zelnik-Manor & Perona; NICDM in Schnitzer, Flexer, Schedl & Widmer, "Local and
// global scaling reduce hubs in space", JMLR 2012) divides a distance by the geometric mean of the two songs' own scales:
//   sdist(i, j) = dist(i, j) / sqrtf(qscale[i] * cscale[j])
// with dist the all-pairs kernel's f32 distance bit for bit, the product rounded once, the correctly rounded root and IEEE
// division.  The selection is blissgpu_knn's with sdist in dist's place: the k smallest keys (f32_key(sdist) << 32) | candidate.
//
//   scaled_knn_scan_kernel   knn_scan_kernel's shape (queries in LDS, 256-candidate blocks staged in LDS, four candidates per
//                            lane in registers, the threshold buffer of knn_list.hpp), and with every block its 256 candidate
//                            scales: one coalesced load, four per lane.  The partial lists are knn_scan_kernel's, merged by
//                            knn_merge_kernel.
//   knn_occurrence_kernel    count[j] = the entries of an index matrix equal to j: a grid-stride pass, one integer atomicAdd
//                            per valid entry.  knn_occurrence_lds_kernel is the other side of its A/B.
//
// The bound (euclidean / Mahalanobis).  The k-nearest scan rejects a sum against a bound that depends on the query alone; here
// the candidate's scale enters.  Let t be the threshold's scaled distance, u the next float above t, a = qscale[i],
// b = cscale[j], r = fl(sqrt(fl(a * b))) the divisor, s the sum and dd = fl(sqrt(s)).  Scales lie in [2^-60, 2^60], so fl(a * b)
// and r are normal and r^2 <= a b (1 + 2^-24)^3 (one rounding of the product, one of the root, squared).
//   Claim: s > 0 and s > u^2 a b (1 + 2^-24)^3 (1 + 2^-23)^2  imply  sdist = fl(dd / r) >= u > t.
//   Proof: sqrt(s) > u r (1 + 2^-23).  There is a float p with u r <= p <= sqrt(s): when u r is below the smallest normal, that
//   normal (s > 0 is a float, so sqrt(s) >= 2^-74.5); otherwise floats are spaced at most 2^-23 apart relatively.  Rounding is
//   monotone and p is a float, so dd >= p; then dd / r >= u exactly, and u is a float, so fl(dd / r) >= u.
// The kernel's bound is at least that product: U = up(fl(u * u)) >= u^2, A = up(fl(U * a)) >= u^2 a (`up` = the next float: a
// rounded-to-nearest product is at most half a spacing below the exact one, subnormals included), A' = A moved up 8 floats
// >= A (1 + 2^-24)^8 >= A (1 + 2^-24)^3 (1 + 2^-23)^2 -- per query, when its threshold changes -- and per candidate
// bound = up(fl(A' * b)): one multiplication and one integer addition.  An overflow anywhere gives inf and then a NaN, against
// which `s > bound` is false.  The filter only discards: every sum that is not above its bound -- NaN, negative and zero sums
// included, the comparison is written `!(s > bound)` -- takes the root, the product's root and the division and is compared by
// its finished 64-bit key.  Cosine and the generic-d path compare the finished scaled distance itself against t.
//
// Scales outside [2^-60, 2^60] (zero, negative, NaN, inf) set a flag that the entry point reports; such a scale counts as 1.
#include <math.h>

#include <algorithm>

#include "device_utils.hpp"
#include "internal.hpp"
#include "knn_list.hpp"
#include "pairwise_math.hpp"
#include "playlist_math.hpp"

namespace bg {

constexpr float SCALE_MIN = 0x1p-60f, SCALE_MAX = 0x1p60f;
constexpr uint32_t SCALED_BOUND_ULPS = 8u;  // the widening of A in the file header

__device__ __forceinline__ bool scale_ok(float s) { return s >= SCALE_MIN && s <= SCALE_MAX; }  // (false for a NaN)

// what a candidate's scale is multiplied with to bound its sum (ROOT), or the threshold's distance (!ROOT): see the file header
template <bool ROOT>
__device__ __forceinline__ float scaled_knn_bound(unsigned long long thr, float a) {
    if (thr == KNN_NONE) return INFINITY;
    const float t = knn_key_dist(thr);
    if (!ROOT) return t;
    const uint32_t tb = __float_as_uint(t);
    if (tb >= 0x7F800000u) return INFINITY;  // inf, NaN, -0 and any negative
    const float u = __uint_as_float(tb + 1u);
    const uint32_t ub = __float_as_uint(u * u);
    if (ub >= 0x7F800000u) return INFINITY;
    const uint32_t ab = __float_as_uint(__uint_as_float(ub + 1u) * a);
    if (ab >= 0x7F800000u - (1u + SCALED_BOUND_ULPS)) return INFINITY;
    return __uint_as_float(ab + 1u + SCALED_BOUND_ULPS);
}

// D > 0: compile-time feature count (packed arithmetic, candidates in registers).  D == 0: any d <= 64 through pl_distance,
// candidates read from global memory / L2 (slow, exact).
template <int D, int METRIC, bool DIAG, int KEYS>
__global__ __launch_bounds__(256, (KEYS == KNN_KEYS_SMALL ? 2 : 1)) void scaled_knn_scan_kernel(
    const float* __restrict__ Q, uint64_t q, const float* __restrict__ qscale, const float* __restrict__ X, uint32_t n,
    const float* __restrict__ cscale, uint32_t d_rt, int metric_rt, const float* __restrict__ M, const uint32_t* __restrict__ skip,
    uint32_t k, uint32_t cap, uint32_t qb_rt, uint32_t n_split, uint32_t blocks_per_split, unsigned long long* __restrict__ part,
    uint32_t* nan_flag, uint32_t* bad_flag, uint32_t* scale_flag) {
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
    __shared__ float s_bound[KNN_QMAX], s_qs[KNN_QMAX];
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
    bool saw_nan = false, bad_scale = false;

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
            float a = qscale[q0 + (uint32_t)tid];
            if (!scale_ok(a)) {  // reported likewise; the scale then counts as 1
                bad_scale = true;
                a = 1.0f;
            }
            s_qs[tid] = a;
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

        for (uint32_t blk = blk0; blk < blk1; blk++) {
            const uint32_t j0 = blk * (uint32_t)KNN_COLS;
            const uint32_t cols_here = (n - j0 < (uint32_t)KNN_COLS) ? n - j0 : (uint32_t)KNN_COLS;
            // the lane's four candidates as two packed pairs: bp[h][kk] = (candidate 2h, candidate 2h + 1), candidate c = row
            // j0 + 64 c + lane; cb[c] = that candidate's scale (1 beyond a ragged block: the value is never looked at)
            f2 bp[2][GENERIC ? 1 : D];
            f2 nb[2];
            float cb[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const uint32_t lc = 64u * (uint32_t)c + (uint32_t)lane;
                cb[c] = lc < cols_here ? cscale[j0 + lc] : 1.0f;
                if (!scale_ok(cb[c])) {
                    bad_scale = true;
                    cb[c] = 1.0f;
                }
            }
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
#pragma unroll 1
            for (uint32_t r = wave_u; r < rows_here; r += 4u) {
                const float qs = s_qs[r];
                // pv[c]: the sum before the root (ROOT) or the finished scaled distance of candidate c of the lane
                float pv[4];
                if constexpr (GENERIC) {
#pragma unroll 1
                    for (int c = 0; c < 4; c++) {
                        const uint32_t lc = 64u * (uint32_t)c + (uint32_t)lane;
                        pv[c] = (lc < cols_here) ? pl_distance(s_q[r], X + (uint64_t)(j0 + lc) * d, d, metric_rt, M) / sqrtf(qs * cb[c]) : INFINITY;
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
                        pv[0] = s0.x / sqrtf(qs * cb[0]); pv[1] = s0.y / sqrtf(qs * cb[1]);
                        pv[2] = s1.x / sqrtf(qs * cb[2]); pv[3] = s1.y / sqrtf(qs * cb[3]);
                    } else {
                        pv[0] = s0.x; pv[1] = s0.y; pv[2] = s1.x; pv[3] = s1.y;
                    }
                }
                // wave-uniform: can any of the wavefront's 256 candidates enter the query's k best?  (`!(v > bound)`: a NaN says yes)
                const float bound = s_bound[r];
                bool maybe = false;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    // ROOT: bound = A' of the file header, the candidate's own bound is the next float above A' * b
                    const float bc = ROOT ? __uint_as_float(__float_as_uint(bound * cb[c]) + 1u) : bound;
                    maybe = maybe || !(pv[c] > bc);
                }
                if (__ballot(maybe) == 0ull) continue;
                // the exact part: scaled distances, keys, the 64-bit comparison with the threshold, survivors into the query's buffer
                KnnList list{s_buf + (size_t)r * cap, s_cnt[r], s_thr[r]};
                const uint32_t skip_r = s_skip[r];
                const unsigned long long thr_in = list.thr;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const uint32_t lc = 64u * (uint32_t)c + (uint32_t)lane, j = j0 + lc;  // (j is only used where lc < cols_here)
                    const bool valid = lc < cols_here && j != skip_r;  // a skipped pair is not evaluated: its value is never looked at
                    const float v = ROOT ? sqrtf(pv[c]) / sqrtf(qs * cb[c]) : pv[c];  // (NaN exactly where the base distance is)
                    if (valid && v != v) saw_nan = true;
                    const unsigned long long key = ((unsigned long long)f32_key(v) << 32) | j;
                    list.push(valid && key < list.thr, key, k, cap, lane);
                }
                if (lane == 0) {
                    s_cnt[r] = list.cnt;
                    if (list.thr != thr_in) {
                        s_thr[r] = list.thr;
                        s_bound[r] = scaled_knn_bound<ROOT>(list.thr, qs);
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
    if (bad_scale) atomicOr(scale_flag, 1u);
}

// count[idx[e]] += 1 for the entries that are not padding; integer atomics: the result does not depend on the order
__global__ __launch_bounds__(256) void knn_occurrence_kernel(const uint32_t* __restrict__ idx, uint64_t entries, uint32_t n,
                                                             uint32_t* __restrict__ count, uint32_t* bad_flag) {
    bool bad = false;
    for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < entries; e += (uint64_t)gridDim.x * 256u) {
        const uint32_t j = idx[e];
        if (j == 0xFFFFFFFFu) continue;
        if (j < n) atomicAdd(&count[j], 1u);
        else bad = true;
    }
    if (bad) atomicOr(bad_flag, 1u);
}

// The other side of the A/B: a workgroup owns a contiguous chunk of the entries and walks it once per window of OCC_WINDOW
// songs, counting in LDS; the window's non-zero counters go to `count` with one atomicAdd each.
constexpr uint32_t OCC_WINDOW = 8192;
__global__ __launch_bounds__(256) void knn_occurrence_lds_kernel(const uint32_t* __restrict__ idx, uint64_t entries, uint32_t n,
                                                                 uint32_t* __restrict__ count, uint32_t* bad_flag) {
    __shared__ uint32_t s_hist[OCC_WINDOW];
    const uint64_t per = (entries + gridDim.x - 1) / gridDim.x;
    const uint64_t e0 = std::min<uint64_t>(entries, (uint64_t)blockIdx.x * per), e1 = std::min<uint64_t>(entries, e0 + per);
    bool bad = false;
    for (uint32_t w0 = 0; w0 < n; w0 += OCC_WINDOW) {  // (w0 + OCC_WINDOW may wrap past 2^32: the window test is on j - w0)
        for (uint32_t i = threadIdx.x; i < OCC_WINDOW; i += 256u) s_hist[i] = 0u;
        __syncthreads();
        for (uint64_t e = e0 + threadIdx.x; e < e1; e += 256u) {
            const uint32_t j = idx[e];
            if (j == 0xFFFFFFFFu) continue;
            if (j >= n) bad = true;
            else if (j - w0 < OCC_WINDOW) atomicAdd(&s_hist[j - w0], 1u);  // (j < w0 wraps to a large value)
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < OCC_WINDOW; i += 256u) {
            const uint32_t v = s_hist[i];
            if (v) atomicAdd(&count[w0 + i], v);  // (a counted j is < n, so w0 + i is)
        }
        __syncthreads();
        if (n - w0 <= OCC_WINDOW) break;
    }
    if (bad) atomicOr(bad_flag, 1u);
}

void launch_scaled_knn_scan(const float* Q, uint64_t q, const float* qscale, const float* X, uint32_t n, const float* cscale,
                            uint32_t d, int metric, const float* M, int m_is_diag, const uint32_t* skip, uint32_t k,
                            const KnnPlan& p, unsigned long long* part, uint32_t* nan_flag, uint32_t* bad_flag,
                            uint32_t* scale_flag, hipStream_t st) {
    const dim3 grid(p.grid_qb * p.n_split);
    const auto scan = [&](auto D_, auto KEYS) {
        for_metric_form<true>(D_, metric, m_is_diag, [&](auto D, auto M_, auto G) {
            hipLaunchKernelGGL((scaled_knn_scan_kernel<D(), M_(), G(), decltype(KEYS)::value>), grid, dim3(256), 0, st, Q, q, qscale, X, n,
                               cscale, d, metric, M, skip, k, p.cap, p.qb, p.n_split, p.blocks_per_split, part, nan_flag, bad_flag,
                               scale_flag);
        });
    };
    with_d(d, [&](auto D) {
        if (p.cap <= 256) scan(D, std::integral_constant<int, KNN_KEYS_SMALL>{});
        else scan(D, std::integral_constant<int, KNN_KEYS_BIG>{});
    });
}

void launch_knn_occurrence(const uint32_t* idx, uint64_t entries, uint32_t n, uint32_t* count, uint32_t* bad_flag, bool lds,
                           int n_cus, hipStream_t st) {
    const uint64_t cus = cus_or_default(n_cus);
    if (lds && n) {  // a workgroup per CU and 4 096 entries at least: every workgroup pays n / OCC_WINDOW passes
        const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(cus * 2, (entries + 4095) / 4096));
        hipLaunchKernelGGL(knn_occurrence_lds_kernel, dim3(grid), dim3(256), 0, st, idx, entries, n, count, bad_flag);
    } else {
        const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(cus * 8, (entries + 255) / 256));
        hipLaunchKernelGGL(knn_occurrence_kernel, dim3(grid), dim3(256), 0, st, idx, entries, n, count, bad_flag);
    }
}

}  // namespace bg
