// kernels_ward.hip -- the device half of Ward clustering of a song library (include/blissgpu.h): per round every
// cluster's nearest other cluster under Ward's cost, all pairs of the current centroids and no matrix stored, and the join that
// makes the next round's centroids (compiled with -ffp-contract=off).  ward_merge.hpp is the host half.
//
// The clusters sit at positions 0 .. m - 1; position p's row is X[slot(p)] with slot(p) = low[p], the cluster's lowest member
// song (low == NULL: slot(p) = p), its size is size[p] (NULL: 1).  For positions i != j
//   dist = the all-pairs kernel's distance bit for bit,  w = ((float)size[i] * (float)size[j]) / ((float)size[i] + (float)size[j]),
//   cost = (dist * dist) * w,  key = (bits of cost) << 32 | (i XOR j),
// and best[i] receives the smallest key over j: j = i XOR (the key's low word).
//
//   ward_scan_kernel  mst_scan_kernel's shape: a lane keeps four positions' rows in registers as two packed column pairs, a
//                     wavefront 256 consecutive positions, and the workgroup walks its column group's positions through LDS
//                     tiles read as ds_read_b128 broadcasts; a candidate's size rides as a float in the padding of its LDS row.
//                     Per candidate: pair_sum; then either the root, the weight and the products for every pair (FILTER off),
//                     or first the test  s * P > lim * S  with P = fl(si * sj), S = si + sj (exact below 2^24) and
//                     lim = fl(best * (1 + 2^-16)), which only pairs that cannot win or tie fail to pass (ward_limit below; the
//                     host chooses the form per scan, by m: the filter pays in the large scans).
//                     A NaN or negative sum fails `>` and reaches the full evaluation, which raises flags[0] for a NaN cost.
//                     The generic form (any d <= 64, pl_distance) evaluates every pair in full.  Every column group folds
//                     its winner into best[p] with one unsigned 64-bit atomic minimum: a total order, the same bits however
//                     the columns are split and in whatever order the groups arrive.
//   ward_join_kernel  one lane per (new position t, feature k): plan[t] = (p, q).  With a partner q the row of p becomes
//                     (float)(((double)size[p] * (double)c_p[k] + (double)size[q] * (double)c_q[k]) / (double)(size[p] + size[q]))
//                     IN PLACE in p's slot -- the pairs are disjoint, so no other lane reads or writes that element -- and the
//                     lane with k == 0 writes the new position's size and lowest member into the round's other pair of arrays
//                     and resets the position's best key for the next scan.
#include <math.h>

#include <algorithm>

#include "device_utils.hpp"
#include "internal.hpp"
#include "pairwise_math.hpp"
#include "playlist_math.hpp"
#include "scan_block.hpp"

namespace bg {

constexpr int WD_TILE_FLOATS = 6144;  // 24 KiB of rows per tile: 256 rows at d = 23 or 20 (pitch 24)
constexpr int WD_TILE_ROWS = 256;
constexpr int WD_POS_PER_WAVE = 256;
constexpr uint32_t WD_INF_BITS = 0x7F800000u;

__device__ __forceinline__ float wd_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// The filter's bound.  A pair with sum s >= 1e-30, P = fl(si sj), S = si + sj and  fl(s P) > fl(ward_limit(b) S)  has a cost
// above b.  With u = 2^-24 and every quantity in the normal range (s >= 1e-30, P / S >= 1/2, b >= 1e-30):
//   s P (1 + u) >= fl(s P) (an overflow to +inf included: then s P > FLT_MAX >= the right side, which is finite or the test fails),
//   fl(lim S) >= lim S (1 - u),  lim = fl(b (1 + 2^-16)) >= b (1 + 2^-16) (1 - u),
// so s P / S > b (1 + 2^-16) (1 - u)^2 / (1 + u) > b (1 + 2^-16) (1 - 3 u).  The cost as computed is
//   fl(fl(fl(sqrt s)^2) fl(P / S)) >= s (P / S) (1 - u)^5   (root, square, quotient, product: each rounds once, the square twice
// counted for the root's error), > b (1 + 2^-16) (1 - 8 u) > b.  A cost above b neither wins nor ties.  Below the normal range
// of b (and for b = +inf) the bound says nothing and every pair passes; so does every pair with s < 1e-30.
__device__ __forceinline__ float ward_limit(float b) { return (b >= 1e-30f && b < INFINITY) ? b * 0x1.0001p0f : INFINITY; }

// D > 0: compile-time feature count (packed arithmetic, the lane's rows in registers).  D == 0: any d <= 64 through pl_distance,
// the lane's rows read from global memory / L2 (slow, exact).  blockDim.x = 64 * (wavefronts per workgroup): 1 .. 4.
template <int D, int METRIC, bool DIAG, bool FILTER>
__global__ __launch_bounds__(256) void ward_scan_kernel(const WardArgs a) {
    constexpr bool GENERIC = D == 0;
    constexpr int DD = GENERIC ? 1 : D;
    constexpr int DQ = GENERIC ? 4 : ((D + 4) & ~3);  // LDS pitch of a row: the features, the size, 16-byte aligned
    __shared__ __attribute__((aligned(16))) float s_c[WD_TILE_FLOATS];
    __shared__ float s_m[(!GENERIC && METRIC == METRIC_MAHALANOBIS) ? D * D : 1];

    const float* __restrict__ X = a.X;
    const uint32_t* __restrict__ low = a.low;
    const uint32_t* __restrict__ size = a.size;
    const uint32_t m = a.m, Y = a.Y;
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, lane = (uint32_t)lane_id(), wave = (uint32_t)wave_id();
    const uint32_t d = GENERIC ? a.d : (uint32_t)D;
    const uint32_t pitch = GENERIC ? d + 1u : (uint32_t)DQ;
    const uint32_t tile_rows = std::min<uint32_t>((uint32_t)WD_TILE_ROWS, (uint32_t)WD_TILE_FLOATS / pitch);
    const uint32_t g = blockIdx.y;
    // the wavefront's 256 positions: slot c of the lane is position p0 + 64 c + lane (m < 2^24: 32 bits hold every position)
    const uint32_t p0 = (blockIdx.x * (nthr / 64u) + wave) * (uint32_t)WD_POS_PER_WAVE;

    if (!GENERIC && METRIC == METRIC_MAHALANOBIS) {
        for (uint32_t e = tid; e < (uint32_t)(DD * DD); e += nthr) s_m[e] = a.M[e];
        __syncthreads();
    }
    float wdiag[DD];
    if constexpr (!GENERIC) {
#pragma unroll
        for (int kk = 0; kk < D; kk++)  // (the same in every lane: scalar registers)
            wdiag[kk] = DIAG ? __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s_m[(kk * D + kk) % (METRIC == METRIC_MAHALANOBIS ? D * D : 1)]))) : 0.0f;
    }

    // the lane's four positions, their rows' slots and sizes; a position past m holds nothing
    bool valid[4];
    uint32_t pos[4], slot[4];
    float si[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        pos[c] = p0 + 64u * (uint32_t)c + lane;
        valid[c] = pos[c] < m;
        slot[c] = valid[c] ? (low ? low[pos[c]] : pos[c]) : 0u;
        if (slot[c] >= a.slots) {  // (never with the host's arrays: no read leaves the rows)
            valid[c] = false;
            slot[c] = 0u;
        }
        si[c] = (valid[c] && size) ? (float)size[pos[c]] : 1.0f;
    }
    f2 bp[2][DD];
    if constexpr (!GENERIC) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const float* xa = X + (uint64_t)slot[2 * h] * (uint64_t)D;
            const float* xb = X + (uint64_t)slot[2 * h + 1] * (uint64_t)D;
#pragma unroll
            for (int kk = 0; kk < D; kk++) {
                bp[h][kk].x = valid[2 * h] ? xa[kk] : 0.0f;
                bp[h][kk].y = valid[2 * h + 1] ? xb[kk] : 0.0f;
            }
        }
    }
    const bool wave_empty = p0 >= m;  // a wavefront without a position still stages the tiles with the others

    // this column group's positions
    const uint32_t r_lo = (uint32_t)(((uint64_t)g * m) / Y), r_hi = (uint32_t)(((uint64_t)(g + 1u) * m) / Y);

    uint32_t bw[4], bx[4];  // the best key so far: cost bits, i XOR j
    float lim[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        bw[c] = 0xFFFFFFFFu;
        bx[c] = 0xFFFFFFFFu;
        lim[c] = INFINITY;
    }
    bool saw_nan = false;

    for (uint32_t t0 = r_lo; t0 < r_hi; t0 += tile_rows) {
        const uint32_t rows_here = std::min<uint32_t>(tile_rows, r_hi - t0);
        if (t0 != r_lo) __syncthreads();  // every wavefront has finished with the previous tile
        {
            const uint32_t floats = rows_here * pitch;
#pragma unroll 4
            for (uint32_t e = tid; e < floats; e += nthr) {
                const uint32_t r = e / pitch, kk = e - r * pitch;
                const uint32_t j = t0 + r;
                float v = 0.0f;
                if (kk < d) {
                    const uint32_t sl = low ? low[j] : j;
                    v = sl < a.slots ? X[(uint64_t)sl * d + kk] : 0.0f;
                } else if (kk == d) {
                    v = size ? (float)size[j] : 1.0f;
                }
                s_c[e] = v;
            }
        }
        __syncthreads();
        if (wave_empty) continue;
#pragma unroll 1
        for (uint32_t r = 0; r < rows_here; r++) {
            const uint32_t j = t0 + r;
            if constexpr (GENERIC) {
                const float sj = wd_uniform(s_c[r * pitch + d]);
#pragma unroll 1
                for (int c = 0; c < 4; c++) {
                    if (!valid[c] || pos[c] == j) continue;
                    const float dist = pl_distance(X + (uint64_t)slot[c] * d, s_c + r * pitch, d, a.metric, a.M);
                    const float w = (si[c] * sj) / (si[c] + sj);
                    const uint32_t cb = __float_as_uint((dist * dist) * w);
                    if (cb > WD_INF_BITS) {
                        saw_nan = true;
                        continue;
                    }
                    const uint32_t x = pos[c] ^ j;
                    if (cb < bw[c] || (cb == bw[c] && x < bx[c])) {
                        bw[c] = cb;
                        bx[c] = x;
                    }
                }
            } else {
                f2 ap[DQ / 2];
                scan_query_row<DQ>(&s_c[r * (uint32_t)DQ], ap);
                const float sj = wd_uniform((D & 1) ? ap[D / 2].y : ap[D / 2].x);  // feature slot D: the candidate's size
                f2 sum0 = pair_sum<DD, METRIC, DIAG>(ap, bp[0], wdiag, s_m);
                // (general M: one pair's 2 x d differences and products at a time, as in the k-nearest scan)
                if (METRIC == METRIC_MAHALANOBIS && !DIAG) asm volatile("" : "+v"(sum0));
                const f2 sum1 = pair_sum<DD, METRIC, DIAG>(ap, bp[1], wdiag, s_m);
                const float pv[4] = {sum0.x, sum0.y, sum1.x, sum1.y};
                bool hit[4];
                float P[4], S[4];
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    P[c] = si[c] * sj;
                    S[c] = si[c] + sj;
                    hit[c] = valid[c] && pos[c] != j;
                    // (a NaN or negative sum fails `>`; a sum below 1e-30 fails `>=`: both are evaluated in full)
                    if (FILTER) hit[c] = hit[c] && !(pv[c] * P[c] > lim[c] * S[c] && pv[c] >= 1e-30f);
                }
                if (hit[0] || hit[1] || hit[2] || hit[3]) {
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        if (!hit[c]) continue;
                        const float dist = sqrtf(pv[c]);
                        const float w = P[c] / S[c];
                        const float cost = (dist * dist) * w;
                        const uint32_t cb = __float_as_uint(cost);
                        if (cb > WD_INF_BITS) {
                            saw_nan = true;
                            continue;
                        }
                        const uint32_t x = pos[c] ^ j;
                        if (cb < bw[c] || (cb == bw[c] && x < bx[c])) {
                            bw[c] = cb;
                            bx[c] = x;
                            if (FILTER) lim[c] = ward_limit(cost);
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
        if (pos[c] < m && bw[c] != 0xFFFFFFFFu)
            atomicMin(a.best + pos[c], ((unsigned long long)bw[c] << 32) | (unsigned long long)bx[c]);
    }
    if (saw_nan) atomicOr(a.flags, 1u);
}

__global__ __launch_bounds__(256) void ward_join_kernel(const WardJoinArgs a) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= (uint64_t)a.m_new * a.d) return;
    const uint32_t t = (uint32_t)(e / a.d), k = (uint32_t)(e - (uint64_t)t * a.d);
    const uint32_t p = a.plan[2 * t], q = a.plan[2 * t + 1];
    if (k == 0) a.best[t] = ~0ull;  // the next scan's minima start here
    if (p >= a.m_old) return;  // (never with the host's plan)
    const uint32_t sp = a.size[p], lp = a.low[p];
    if (q == 0xFFFFFFFFu || q >= a.m_old) {
        if (k == 0) {
            a.size_out[t] = sp;
            a.low_out[t] = lp;
        }
        return;
    }
    const uint32_t sq = a.size[q], lq = a.low[q];
    if (lp >= a.slots || lq >= a.slots) return;  // (never with the host's arrays)
    float* cp = a.X + (uint64_t)lp * a.d + k;
    const double num = (double)sp * (double)*cp + (double)sq * (double)a.X[(uint64_t)lq * a.d + k];
    *cp = (float)(num / (double)(sp + sq));
    if (k == 0) {
        a.size_out[t] = sp + sq;
        a.low_out[t] = lp;
    }
}

WardPlan ward_plan(uint64_t m, int n_cus, uint32_t col_groups) {
    WardPlan p{};
    const ScanFill f = scan_fill((m + WD_POS_PER_WAVE - 1) / WD_POS_PER_WAVE, n_cus);  // pieces of 256 positions
    p.waves = f.waves;
    p.grid = std::max<uint32_t>(1u, f.grid);
    // column groups: what fills the device, none with fewer than 64 positions
    const uint64_t in_one = (uint64_t)p.grid * p.waves;
    uint64_t Y = col_groups ? col_groups : std::min<uint64_t>(fill_col_groups(f.cus, in_one), std::max<uint64_t>(1, m / 64));
    Y = std::max<uint64_t>(1, std::min<uint64_t>(Y, std::max<uint64_t>(1, m)));
    p.Y = (uint32_t)std::min<uint64_t>(Y, 65535);
    return p;
}

void launch_ward_scan(const WardArgs& a, int m_is_diag, bool filter, const WardPlan& p, hipStream_t st) {
    if (a.m == 0) return;
    const dim3 grid(p.grid, a.Y), block(64u * p.waves);
    for_metric_form<false>(a.d, a.metric, m_is_diag, [&](auto D, auto M, auto G) {
        if constexpr (D() != 0) {  // (the generic kernel has no filtered form)
            if (filter) {
                hipLaunchKernelGGL((ward_scan_kernel<D(), M(), G(), true>), grid, block, 0, st, a);
                return;
            }
        }
        hipLaunchKernelGGL((ward_scan_kernel<D(), M(), G(), false>), grid, block, 0, st, a);
    });
}

void launch_ward_join(const WardJoinArgs& a, hipStream_t st) {
    const uint64_t lanes = (uint64_t)a.m_new * a.d;
    if (lanes == 0) return;
    hipLaunchKernelGGL(ward_join_kernel, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, st, a);
}

}  // namespace bg
