// kernels_mst.hip -- the device half of the minimum spanning tree of a song library (include/blissgpu.h): per
// round of Boruvka's algorithm, every song's smallest edge into another component and every component's smallest such edge,
// all pairs and no matrix stored (compiled with -ffp-contract=off).  mst_merge.hpp is the host half.
//
// w(i, j) = max(dist(i, j), core[i], core[j]) with dist the all-pairs kernel's distance bit for bit; edges {u < v} are ordered
// by (bits of w, u, v).  For one song i the candidates j are therefore ordered by (bits of w(i, j), j): with j1 < j2 the pair
// (min(i, j1), max(i, j1)) is below (min(i, j2), max(i, j2)) wherever i lies.
//
// The host uploads, per round, the songs sorted by (component, index) -- order[p] -- and the component at every position --
// cpos[p].  "position" below is a place in that order.
//
//   mst_scan_kernel  chamfer_scan_kernel's shape with an arg-min in the minimum's place: a lane keeps four songs in registers
//                    as two packed column pairs, a wavefront 256 CONSECUTIVE POSITIONS, and the workgroup walks its column
//                    group's rows through LDS tiles read as ds_read_b128 broadcasts; a row's component rides in the padding
//                    of its LDS row.  Per row: pair_sum, and per song one compare of the sum against a LIMIT and one of the
//                    components.  The weight needs the root, and equal roots of unequal sums are ties that the index decides,
//                    so sums cannot stand in for weights; but the root is monotone, so a sum above
//                    limit = best_w^2 (1 + 2^-20), rounded twice, has a root above best_w (mst_limit) and cannot win or tie.
//                    Only what passes that filter takes the root, the maxima with the cores, and the comparison of
//                    (weight bits, j) -- a few candidates per song and tile once the walk has seen a near song.  A NaN or
//                    negative sum fails `sum > limit`, reaches the slow path and raises flags[0] there (candidates of the
//                    song's own component never do: a song against itself may be inf - inf).  The generic form (any d <= 64,
//                    pl_distance) compares the finished weights of every pair.  Each column group writes its winner per
//                    position: part_w / part_j [Y][n].
//                    Late rounds: a wavefront whose 256 positions lie in one component skips every tile whose rows all lie
//                    in that component (both uniform across the wavefront), when a.skip is set.
//   mst_pick_kernel  phase 0: per position the smallest of the Y partial winners under (w, j), kept in part_* [0][p], and an
//                    unsigned atomic minimum of w into comp_w[component].  phase 1: the positions that hold their
//                    component's minimum weight take an unsigned 64-bit atomic minimum of (min(i, j) << 32 | max(i, j)) into
//                    comp_uv[component].  Integer minima have no order: the same bits every run.
#include <math.h>

#include <algorithm>

#include "device_utils.hpp"
#include "internal.hpp"
#include "pairwise_math.hpp"
#include "playlist_math.hpp"
#include "scan_block.hpp"

namespace bg {

constexpr int MS_TILE_FLOATS = 6144;  // 24 KiB of library rows per tile: 256 rows at d = 23 or 20 (pitch 24)
constexpr int MS_TILE_ROWS = 256;
constexpr int MS_SONGS_PER_WAVE = 256;
constexpr uint32_t MS_NONE = 0xFFFFFFFFu;
constexpr uint32_t MS_INF_BITS = 0x7F800000u;

__device__ __forceinline__ uint32_t ms_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// A sum s > mst_limit(w) has sqrtf(s) > w.  With u = 2^-24: fl(w w) >= w^2 (1 - u), times 1 + 2^-20 and rounded again
// >= w^2 (1 - u)^2 (1 + 2^-20) > w^2 (1 + 2^-21), so the exact root of s is above w (1 + 2^-22 - 2^-45), which is above the
// float after w (at most w (1 + 2^-23)); the correctly rounded root is then at least that float.  Below the normal range of
// w w (and for w = +inf) the bound says nothing and every sum passes.
__device__ __forceinline__ float mst_limit(float w) {
    const float q = w * w;
    return q >= 1e-30f ? q * 0x1.00001p0f : INFINITY;
}

// -0.0 counts as +0.0 (the weights' bit patterns must order as integers)
__device__ __forceinline__ float ms_core(float c) { return c == 0.0f ? 0.0f : c; }

// D > 0: compile-time feature count (packed arithmetic, the lane's songs in registers).  D == 0: any d <= 64 through pl_distance,
// the lane's songs read from global memory / L2 (slow, exact).  blockDim.x = 64 * (wavefronts per workgroup): 1 .. 4.
template <int D, int METRIC, bool DIAG>
__global__ __launch_bounds__(256) void mst_scan_kernel(const MstArgs a) {
    constexpr bool GENERIC = D == 0;
    constexpr int DD = GENERIC ? 1 : D;
    constexpr int DQ = GENERIC ? 4 : ((D + 4) & ~3);  // LDS pitch of a row: the features, the component, 16-byte aligned
    __shared__ __attribute__((aligned(16))) float s_c[MS_TILE_FLOATS];
    __shared__ uint32_t s_j[MS_TILE_ROWS];
    __shared__ float s_core[MS_TILE_ROWS];
    __shared__ float s_m[(!GENERIC && METRIC == METRIC_MAHALANOBIS) ? D * D : 1];

    const float* __restrict__ X = a.X;
    const uint32_t* __restrict__ order = a.order;
    const uint32_t* __restrict__ cpos = a.cpos;
    const uint32_t n = a.n, Y = a.Y;
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, lane = (uint32_t)lane_id(), wave = (uint32_t)wave_id();
    const uint32_t d = GENERIC ? a.d : (uint32_t)D;
    const uint32_t pitch = GENERIC ? d + 1u : (uint32_t)DQ;
    const uint32_t tile_rows = std::min<uint32_t>((uint32_t)MS_TILE_ROWS, (uint32_t)MS_TILE_FLOATS / pitch);
    const uint32_t g = blockIdx.y;
    // the wavefront's 256 positions: slot c of the lane is position p0 + 64 c + lane (64-bit: n may be close to 2^32)
    const uint64_t p0 = ((uint64_t)blockIdx.x * (nthr / 64u) + wave) * (uint64_t)MS_SONGS_PER_WAVE;

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

    // the lane's four songs, their components and cores; a position past n holds nothing
    bool valid[4];
    uint32_t song[4], own[4];
    float ci[4];
    bool bad_core = false;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint64_t p = p0 + 64u * (uint32_t)c + lane;
        valid[c] = p < (uint64_t)n;
        song[c] = valid[c] ? order[p] : 0u;
        if (song[c] >= n) {
            valid[c] = false;
            song[c] = 0u;
        }
        own[c] = valid[c] ? cpos[p] : MS_NONE;
        ci[c] = (valid[c] && a.core) ? a.core[song[c]] : 0.0f;
        if (!(ci[c] >= 0.0f)) bad_core = true;  // NaN or negative
        ci[c] = ms_core(ci[c]);
    }
    if (bad_core) atomicOr(a.flags + 1, 1u);
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
    // the component of the whole wavefront, if it has one (positions are sorted by component: first == last); MS_NONE - 1: a
    // wavefront without a song, which has nothing to do in any tile
    uint32_t wave_comp = MS_NONE;
    if (p0 >= (uint64_t)n) {
        wave_comp = MS_NONE - 1u;
    } else if (a.skip) {
        const uint64_t last = std::min<uint64_t>(p0 + (MS_SONGS_PER_WAVE - 1), (uint64_t)n - 1u);
        const uint32_t cf = ms_uniform(cpos[p0]), cl = ms_uniform(cpos[last]);
        if (cf == cl) wave_comp = cf;
    }

    // this column group's rows of the sorted order
    const uint32_t r_lo = (uint32_t)(((uint64_t)g * n) / Y), r_hi = (uint32_t)(((uint64_t)(g + 1u) * n) / Y);

    uint32_t bw[4], bj[4];
    float lim[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        bw[c] = MS_NONE;
        bj[c] = MS_NONE;
        lim[c] = valid[c] ? INFINITY : -1.0f;  // (a slot without a song: every sum >= +0 is above its limit)
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
                const uint32_t j = order[t0 + r];
                float v = 0.0f;
                if (kk < d) v = j < n ? X[(uint64_t)j * d + kk] : 0.0f;
                else if (kk == d) v = __uint_as_float(cpos[t0 + r]);  // (moved as bits, never computed with)
                s_c[e] = v;
            }
            for (uint32_t r = tid; r < rows_here; r += nthr) {
                const uint32_t j = order[t0 + r];
                s_j[r] = j;
                s_core[r] = (a.core && j < n) ? ms_core(a.core[j]) : 0.0f;
            }
        }
        __syncthreads();
        if (wave_comp == MS_NONE - 1u) continue;
        if (wave_comp != MS_NONE) {
            const uint32_t first = ms_uniform(__float_as_uint(s_c[d])), last = ms_uniform(__float_as_uint(s_c[(rows_here - 1u) * pitch + d]));
            if (first == wave_comp && last == wave_comp) continue;  // every pair of this tile is inside one component
        }
#pragma unroll 1
        for (uint32_t r = 0; r < rows_here; r++) {
            if constexpr (GENERIC) {
                const uint32_t rc = ms_uniform(__float_as_uint(s_c[r * pitch + d]));
#pragma unroll 1
                for (int c = 0; c < 4; c++) {
                    if (!valid[c] || own[c] == rc) continue;
                    const float dist = pl_distance(X + (uint64_t)song[c] * d, s_c + r * pitch, d, a.metric, a.M);
                    if (__float_as_uint(dist) > MS_INF_BITS) {
                        saw_nan = true;
                        continue;
                    }
                    const uint32_t wb = __float_as_uint(fmaxf(dist, fmaxf(ci[c], s_core[r])));
                    const uint32_t j = s_j[r];
                    if (wb < bw[c] || (wb == bw[c] && j < bj[c])) {
                        bw[c] = wb;
                        bj[c] = j;
                    }
                }
            } else {
                f2 ap[DQ / 2];
                scan_query_row<DQ>(&s_c[r * (uint32_t)DQ], ap);
                const uint32_t rc = ms_uniform(__float_as_uint((D & 1) ? ap[D / 2].y : ap[D / 2].x));  // feature slot D: the row's component
                f2 sum0 = pair_sum<DD, METRIC, DIAG>(ap, bp[0], wdiag, s_m);
                // (general M: one pair's 2 x d differences and products at a time, as in the k-nearest scan)
                if (METRIC == METRIC_MAHALANOBIS && !DIAG) asm volatile("" : "+v"(sum0));
                const f2 sum1 = pair_sum<DD, METRIC, DIAG>(ap, bp[1], wdiag, s_m);
                const float pv[4] = {sum0.x, sum0.y, sum1.x, sum1.y};
                bool hit[4];
#pragma unroll
                for (int c = 0; c < 4; c++) hit[c] = !(pv[c] > lim[c]) && own[c] != rc;  // (NaN and negative sums pass the first test)
                if (hit[0] || hit[1] || hit[2] || hit[3]) {
                    const uint32_t j = s_j[r];
                    const float cj = s_core[r];
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        if (!hit[c] || !valid[c]) continue;
                        if (__float_as_uint(pv[c]) > MS_INF_BITS) {
                            saw_nan = true;
                            continue;
                        }
                        const float w = fmaxf(sqrtf(pv[c]), fmaxf(ci[c], cj));
                        const uint32_t wb = __float_as_uint(w);
                        if (wb < bw[c] || (wb == bw[c] && j < bj[c])) {
                            bw[c] = wb;
                            bj[c] = j;
                            lim[c] = mst_limit(w);
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint64_t p = p0 + 64u * (uint32_t)c + lane;
        if (p < (uint64_t)n) {
            a.part_w[(uint64_t)g * n + p] = bw[c];
            a.part_j[(uint64_t)g * n + p] = bj[c];
        }
    }
    if (saw_nan) atomicOr(a.flags, 1u);
}

__global__ __launch_bounds__(256) void mst_pick_kernel(const MstArgs a) {
    const uint32_t n = a.n;
    for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < (uint64_t)n; p += (uint64_t)gridDim.x * 256u) {
        const uint32_t c = a.cpos[p];
        if (c >= a.comps) continue;
        if (a.phase == 0u) {
            uint32_t w = a.part_w[p], j = a.part_j[p];
            for (uint32_t g = 1; g < a.Y; g++) {
                const uint32_t ow = a.part_w[(uint64_t)g * n + p], oj = a.part_j[(uint64_t)g * n + p];
                if (ow < w || (ow == w && oj < j)) {
                    w = ow;
                    j = oj;
                }
            }
            a.part_w[p] = w;
            a.part_j[p] = j;
            if (w != MS_NONE && j < n) atomicMin(a.comp_w + c, w);
        } else {
            const uint32_t w = a.part_w[p], j = a.part_j[p], i = a.order[p];
            if (w != MS_NONE && j < n && i < n && w == a.comp_w[c])
                atomicMin(a.comp_uv + c, ((unsigned long long)std::min(i, j) << 32) | (unsigned long long)std::max(i, j));
        }
    }
}

MstPlan mst_plan(uint64_t n, int n_cus, uint32_t col_groups, uint64_t ws_limit) {
    MstPlan p{};
    const ScanFill f = scan_fill((n + MS_SONGS_PER_WAVE - 1) / MS_SONGS_PER_WAVE, n_cus);  // pieces of 256 positions
    p.waves = f.waves;
    p.grid = std::max<uint32_t>(1u, f.grid);
    // column groups: what fills the device, none with fewer than 64 rows
    const uint64_t in_one = (uint64_t)p.grid * p.waves;
    uint64_t Y = col_groups ? col_groups : std::min<uint64_t>(fill_col_groups(f.cus, in_one), std::max<uint64_t>(1, n / 64));
    Y = std::max<uint64_t>(1, std::min<uint64_t>(Y, std::max<uint64_t>(1, n)));
    p.Y = (uint32_t)std::min<uint64_t>(Y, 65535);
    p.pick_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 8ull * f.cus));
    // flags u32[4] | order u32[n] | cpos u32[n] | comp_w u32[n] | part_w u32[Y][n] | part_j u32[Y][n] | comp_uv u64[n]
    p.bytes = 16 + (3 + 2 * (uint64_t)p.Y) * n * 4 + 8 + n * 8;
    p.fits = p.bytes <= ws_limit;
    return p;
}

void launch_mst_scan(const MstArgs& a, int m_is_diag, const MstPlan& p, hipStream_t st) {
    if (a.n == 0) return;
    const dim3 grid(p.grid, a.Y), block(64u * p.waves);
    for_metric_form<false>(a.d, a.metric, m_is_diag, [&](auto D, auto M, auto G) {
        hipLaunchKernelGGL((mst_scan_kernel<D(), M(), G()>), grid, block, 0, st, a);
    });
}

void launch_mst_pick(MstArgs a, uint32_t phase, const MstPlan& p, hipStream_t st) {
    if (a.n == 0) return;
    a.phase = phase;
    hipLaunchKernelGGL(mst_pick_kernel, dim3(p.pick_grid), dim3(256), 0, st, a);
}

}  // namespace bg
