// kernels_silhouette.hip -- the silhouette of a labelling of a song library, all pairs and nothing stored (compiled with
// -ffp-contract=off).
//
// For every scored song i: S(i, c) = 0.0 + (double)dist(i, j0) + (double)dist(i, j1) + ... over the members of cluster c in
// ascending j, one sequential f64 sum per (song, cluster); a = S(i, own) / (size_own - 1), b = the smallest S(i, c) / size_c over
// the other non-empty clusters (equal quotients go to the lower c), s from a and b (include/blissgpu.h has the contract).  The
// distances are those of the all-pairs kernel bit for bit (pair_sum of pairwise_math.hpp / pl_distance, the correctly rounded
// square root).  Nothing is left to the order in which work arrives: a sum is formed by ONE lane in the contract's order, the
// minima are taken in ascending cluster order with a strict <, and every value reaches memory with a plain store.
//
// The labels are sorted first with the k-means kernels as they are (kmeans_hist / scan_tiles / scan_add / scatter of
// kernels_kmeans.hip): cluster c's members are arow[arow_off[c] .. arow_off[c + 1]) in ascending index.
//
//   silhouette_scan_kernel    kmeans_assign_kernel's shape with the library in the centres' place: a lane keeps four SCORED songs
//                             in registers as two packed column pairs, a wavefront 256, and every wavefront of the workgroup
//                             walks the library in cluster order, staged through arow into LDS tiles of up to 256 rows and read
//                             as ds_read_b128 broadcasts.  Per row: pair_sum, sqrtf, one convert, one f64 add into each of the
//                             lane's four running sums (four independent chains, one add per ~140 packed instructions).  Where a
//                             cluster ends -- uniform across the workgroup: read from arow_off, a scalar branch, runs of empty
//                             clusters skipped -- a song either keeps the sum (its own cluster) or divides it by the size and
//                             takes the quotient as its best when strictly smaller.  The clusters are dealt to Y column groups,
//                             cluster c to group floor(arow_off[c] Y / n): a cluster is never split, so S(i, c) does not depend
//                             on Y.  grid = (pieces of the scored songs, Y); work item (piece, g) writes, per song, its best
//                             other quotient with its cluster (SIL_NONE: the group held no other cluster) and -- when the own
//                             cluster lies in g -- the own-cluster sum, at [g][position].
//   silhouette_finish_kernel  a lane per scored song: the groups' best quotients in ascending g with a strict <, the own sum from
//                             the own cluster's group, then a, b, neighbour and s.  The same launch writes sizes and raises the
//                             error word: a label >= K (every label is looked at, scored or not), a rows entry >= n, fewer than
//                             two non-empty clusters.
#include <math.h>

#include <algorithm>

#include "device_utils.hpp"
#include "internal.hpp"
#include "pairwise_math.hpp"
#include "playlist_math.hpp"
#include "scan_block.hpp"

namespace bg {

constexpr int SIL_TILE_FLOATS = 6144;  // 24 KiB of library rows per tile: 256 rows at d = 23 (pitch 24)
constexpr int SIL_TILE_ROWS = 256;     // at most this many rows per tile
constexpr int SIL_SONGS_PER_WAVE = 256;
constexpr uint32_t SIL_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t sil_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the first cluster c in [0, K] with arow_off[c] >= t (arow_off[0] = 0, arow_off[K] = n >= t)
__device__ __forceinline__ uint32_t sil_first_cluster(const uint32_t* __restrict__ arow_off, uint32_t K, uint64_t t) {
    return t ? find_segment(arow_off, K + 1u, (uint32_t)(t - 1u)) + 1u : 0u;
}

// D > 0: compile-time feature count (packed arithmetic, scored songs in registers).  D == 0: any d <= 64 through pl_distance,
// scored songs read from global memory / L2 (slow, exact).  blockDim.x = 64 * (wavefronts per workgroup): 1 .. 4.
template <int D, int METRIC, bool DIAG>
__global__ __launch_bounds__(256) void silhouette_scan_kernel(const SilhouetteArgs a) {
    constexpr bool GENERIC = D == 0;
    constexpr int DD = GENERIC ? 1 : D;
    constexpr int DQ = GENERIC ? 1 : ((D + 3) & ~3);  // LDS pitch of a row: 16-byte aligned -> ds_read_b128 broadcasts
    __shared__ __attribute__((aligned(16))) float s_c[SIL_TILE_FLOATS];
    __shared__ float s_m[(!GENERIC && METRIC == METRIC_MAHALANOBIS) ? D * D : 1];

    const float* __restrict__ X = a.X;
    const uint32_t* __restrict__ arow_off = a.arow_off;
    const uint32_t* __restrict__ arow = a.arow;
    const uint32_t n = a.n, K = a.K, q = a.q, Y = a.Y;
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, lane = (uint32_t)lane_id(), wave = (uint32_t)wave_id();
    const uint32_t d = GENERIC ? a.d : (uint32_t)D;
    const uint32_t pitch = GENERIC ? d : (uint32_t)DQ;
    const uint32_t tile_rows = std::min<uint32_t>((uint32_t)SIL_TILE_ROWS, (uint32_t)SIL_TILE_FLOATS / pitch);
    const uint32_t g = blockIdx.y;
    // the wavefront's 256 scored positions: slot c of the lane is position p0 + 64 c + lane (64-bit: q may be close to 2^32)
    const uint64_t p0 = ((uint64_t)blockIdx.x * (nthr / 64u) + wave) * (uint64_t)SIL_SONGS_PER_WAVE;

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

    // the lane's four songs: their rows of X and their labels; a position past q or a rows entry past n scores nothing
    bool valid[4];
    uint32_t song[4], own[4];
    bool bad_row = false;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint64_t p = p0 + 64u * (uint32_t)c + lane;
        valid[c] = p < (uint64_t)q;
        song[c] = valid[c] ? (a.rows ? a.rows[p] : (uint32_t)p) : 0u;
        if (valid[c] && song[c] >= n) {
            bad_row = true;
            valid[c] = false;
            song[c] = 0u;
        }
        own[c] = valid[c] ? a.labels[song[c]] : SIL_NONE;
    }
    // ... as two packed pairs: bp[h][kk] = (song 2h, song 2h + 1); the rows of slots that score nothing are zeros
    f2 bp[2][DD];
    if constexpr (!GENERIC) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const float* xa = X + (uint64_t)song[2 * h] * (uint64_t)D;
            const float* xb = X + (uint64_t)song[2 * h + 1] * (uint64_t)D;
#pragma unroll
            for (int kk = 0; kk < D; kk++) {
                bp[h][kk].x = valid[2 * h] ? xa[kk] : 0.0f;
                bp[h][kk].y = valid[2 * h + 1] ? xb[kk] : 0.0f;
            }
        }
    }

    // the group's run of clusters [c_lo, c_hi) = those with floor(arow_off[c] Y / n) == g, and its rows of the sorted order
    const uint32_t c_lo = sil_uniform(sil_first_cluster(arow_off, K, ((uint64_t)g * n + Y - 1u) / Y));
    const uint32_t c_hi = sil_uniform(sil_first_cluster(arow_off, K, ((uint64_t)(g + 1u) * n + Y - 1u) / Y));
    const uint32_t r_lo = sil_uniform(arow_off[c_lo]), r_hi = sil_uniform(arow_off[c_hi]);

    double acc[4], own_sum[4], best_q[4];
    uint32_t best_i[4];
    bool have_own[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        acc[c] = 0.0;
        own_sum[c] = 0.0;
        best_q[c] = 0.0;
        best_i[c] = SIL_NONE;
        have_own[c] = false;
    }
    bool saw_nan = false;

    // cl = the cluster the walk is in, rows [start, end) of the sorted order; runs of empty clusters are stepped over
    uint32_t cl = c_lo, start = r_lo, end = r_lo;
    while (cl < c_hi && (end = sil_uniform(arow_off[cl + 1u])) == start) cl++;

    for (uint32_t t0 = r_lo; t0 < r_hi; t0 += tile_rows) {
        const uint32_t rows_here = std::min<uint32_t>(tile_rows, r_hi - t0);
        if (t0 != r_lo) __syncthreads();  // every wavefront has finished with the previous tile
        {
            // row r of the tile = row arow[t0 + r] of X; the padding of a row travels into registers with it (never into a
            // result): zeros.  (arow holds indices < n whenever every label is < K; otherwise the call fails and the row is zeros)
            const uint32_t floats = rows_here * pitch;
#pragma unroll 4
            for (uint32_t e = tid; e < floats; e += nthr) {
                const uint32_t r = e / pitch, kk = e - r * pitch;
                const uint32_t j = arow[t0 + r];
                s_c[e] = (kk < d && j < n) ? X[(uint64_t)j * d + kk] : 0.0f;
            }
        }
        __syncthreads();
        uint32_t r = 0;
        while (r < rows_here) {
            const uint32_t seg = std::min<uint32_t>(rows_here, end - t0);  // (end > t0 + r: the walk is inside cluster cl)
#pragma unroll 1
            for (; r < seg; r++) {
                if constexpr (GENERIC) {
#pragma unroll 1
                    for (int c = 0; c < 4; c++) {
                        if (!valid[c]) continue;
                        const float v = pl_distance(X + (uint64_t)song[c] * d, s_c + r * pitch, d, a.metric, a.M);
                        acc[c] = acc[c] + (double)v;
                    }
                } else {
                    f2 ap[DQ / 2];
                    scan_query_row<DQ>(&s_c[r * (uint32_t)DQ], ap);
                    f2 s0 = pair_sum<DD, METRIC, DIAG>(ap, bp[0], wdiag, s_m);
                    // (general M: one pair's 2 x d differences and products at a time, as in the k-nearest scan)
                    if (METRIC == METRIC_MAHALANOBIS && !DIAG) asm volatile("" : "+v"(s0));
                    const f2 s1 = pair_sum<DD, METRIC, DIAG>(ap, bp[1], wdiag, s_m);
                    const float pv[4] = {s0.x, s0.y, s1.x, s1.y};
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        acc[c] = acc[c] + (double)sqrtf(pv[c]);
                    }
                }
            }
            if (t0 + r == end) {  // cluster cl ends here (uniform): keep the sum, or divide it and compare
                const double size = (double)(end - start);
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    // a distance is >= 0, +inf or NaN: a sum is NaN exactly when one of its distances was (no inf - inf)
                    if (acc[c] != acc[c] && valid[c]) saw_nan = true;
                    if (own[c] == cl) {
                        own_sum[c] = acc[c];
                        have_own[c] = true;
                    } else {
                        const double quot = acc[c] / size;
                        if (best_i[c] == SIL_NONE || quot < best_q[c]) {  // ascending clusters: a tie keeps the lower one
                            best_q[c] = quot;
                            best_i[c] = cl;
                        }
                    }
                    acc[c] = 0.0;
                }
                cl++;
                start = end;
                while (cl < c_hi && (end = sil_uniform(arow_off[cl + 1u])) == start) cl++;
            }
        }
    }

#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint64_t p = p0 + 64u * (uint32_t)c + lane;
        if (valid[c]) {
            const uint64_t slot = (uint64_t)g * q + p;
            a.ws_best_q[slot] = best_q[c];
            a.ws_best_i[slot] = best_i[c];
            if (have_own[c]) a.ws_own[slot] = own_sum[c];
        }
    }
    if (saw_nan) atomicOr(a.flags, 1u);
    if (bad_row) atomicOr(a.flags + 1, SIL_ERR_ROW);
}

// thread t: scored position t (< q), label t (< n) and cluster t (< K)
__global__ __launch_bounds__(256) void silhouette_finish_kernel(const SilhouetteArgs a) {
    const uint32_t* __restrict__ arow_off = a.arow_off;
    const uint32_t n = a.n, K = a.K, q = a.q, Y = a.Y;
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t < (uint64_t)K) {
        const uint32_t size = arow_off[t + 1u] - arow_off[t];
        if (a.sizes) a.sizes[t] = size;
        if (size == n) atomicOr(a.flags + 1, SIL_ERR_CLUSTERS);  // (labels all < K: one cluster holds every song)
    }
    if (t < (uint64_t)n && a.labels[t] >= K) atomicOr(a.flags + 1, SIL_ERR_LABEL);
    if (t >= (uint64_t)q) return;
    const uint32_t i = a.rows ? a.rows[t] : (uint32_t)t;
    const uint32_t own = i < n ? a.labels[i] : SIL_NONE;
    float s = 0.0f;
    double av = 0.0, bv = INFINITY;
    uint32_t nb = SIL_NONE;
    if (i >= n) {
        atomicOr(a.flags + 1, SIL_ERR_ROW);
    } else if (own < K) {
        const uint32_t size_own = arow_off[own + 1u] - arow_off[own];
        const uint64_t g_own = (uint64_t)arow_off[own] * Y / n;
        const double own_sum = a.ws_own[g_own * q + t];
        for (uint32_t g = 0; g < Y; g++) {
            const uint32_t ci = a.ws_best_i[(uint64_t)g * q + t];
            if (ci == SIL_NONE) continue;
            const double v = a.ws_best_q[(uint64_t)g * q + t];
            if (nb == SIL_NONE || v < bv) {  // ascending groups hold ascending clusters: a tie keeps the lower one
                bv = v;
                nb = ci;
            }
        }
        if (size_own > 1u) {
            av = own_sum / (double)(size_own - 1u);
            double sv = 0.0;
            if (av < bv) sv = 1.0 - av / bv;
            else if (av > bv) sv = bv / av - 1.0;
            s = (float)sv;
        }
    }
    a.s[t] = s;
    if (a.a) a.a[t] = av;
    if (a.b) a.b[t] = bv;
    if (a.neighbour) a.neighbour[t] = nb;
}

SilhouettePlan silhouette_plan(uint64_t q, uint32_t K, int n_cus, uint32_t col_groups) {
    SilhouettePlan p{};
    const ScanFill f = scan_fill((q + SIL_SONGS_PER_WAVE - 1) / SIL_SONGS_PER_WAVE, n_cus);  // pieces of 256 scored songs
    p.waves = f.waves;
    p.grid = f.grid;
    // column groups: what fills the device, at most one group per cluster (a cluster is never split)
    const uint64_t in_one = (uint64_t)std::max<uint32_t>(p.grid, 1u) * p.waves;
    const uint64_t Y = col_groups ? col_groups : fill_col_groups(f.cus, in_one);
    p.Y = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(Y, K));
    return p;
}

void launch_silhouette_scan(const SilhouetteArgs& a, int m_is_diag, const SilhouettePlan& p, hipStream_t st) {
    if (a.q == 0 || a.n == 0) return;
    const dim3 grid(p.grid, p.Y), block(64u * p.waves);
    for_metric_form<false>(a.d, a.metric, m_is_diag, [&](auto D, auto M, auto G) {
        hipLaunchKernelGGL((silhouette_scan_kernel<D(), M(), G()>), grid, block, 0, st, a);
    });
}

void launch_silhouette_finish(const SilhouetteArgs& a, hipStream_t st) {
    const uint64_t threads = std::max<uint64_t>(std::max<uint64_t>(a.q, a.n), a.K);
    hipLaunchKernelGGL(silhouette_finish_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st, a);
}

}  // namespace bg
