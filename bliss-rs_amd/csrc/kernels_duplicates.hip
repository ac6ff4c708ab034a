// kernels_duplicates.hip -- which rows of a feature matrix are the same song: a self-join under a distance threshold and the
// connected components of its edges, without the distance matrix (compiled with -ffp-contract=off).
//
// Reference: the duplicate rule of dedup_playlist_custom_distance (src/playlist.rs:381-388) -- n32(d) < threshold, or the same
// non-empty title and artist -- applied to EVERY pair of a collection instead of the neighbours of an ordered playlist.  The
// pair (i, j), i < j, is an edge when D[i][j] < threshold (D[i][j] = what the all-pairs kernel writes at row i, column j:
// pair_sum of pairwise_math.hpp, the correctly rounded square root, IEEE division) or meta[i] != 0 && meta[i] == meta[j].
// label[i] = the smallest row index of i's connected component, n_pairs = the number of edges: both discrete functions of the
// input, independent of the order in which the edges are met.
//
//   dup_init_kernel     parent[i] = i (the caller's label array IS the parent array), counters = 0
//   dup_join_kernel     the upper triangle of the n x n pairs in tiles of 256 x 256: a workgroup takes tile t of a linear index
//                       over the tile pairs (I <= J), stages the rows of block I in LDS (read as broadcasts) and the 256 rows of
//                       block J as candidates (each lane takes four into registers as two packed pairs, as the k-nearest scan
//                       does).  Row i is ALWAYS the row operand and j the column operand of pair_sum, so no symmetry of the
//                       arithmetic is assumed; a diagonal tile masks j <= i.  A row against the wavefront's 256 candidates is four
//                       packed sums and one float comparison per candidate; the square root, the exact `<`, the edge count, the
//                       append to the pair list and the union run only when a ballot says some lane may hold an edge.
//   dup_flatten_kernel  label[i] = find(i)
//
// The bound (euclidean / Mahalanobis): with t the threshold, a sum s > B = next_up(fl(t * t)) has s > t^2 exactly (fl is at most
// half an ulp below t^2, B a whole ulp above fl), so sqrt(s) > t and the rounded root -- rounding is monotone, t is a float --
// is >= t: no edge, for certain.  Every other sum, NaN and negative sums included (`!(s > B)`), takes the root and the exact
// comparison.  Cosine and the generic-d path compare the distance itself (`!(v >= t)`).
//
// Components: lock-free union-find on parent[] in global memory.  find() halves the path; a union links the LARGER root under
// the smaller with a compare-and-swap on the larger root's own slot and starts over when the slot has changed.  Only roots are
// ever linked and only non-roots are ever shortened (to an ancestor), so parent[x] <= x always holds, every chain descends
// strictly, and the root of a component is its smallest index whatever the order of the unions.  The loads and stores are
// device-scope atomics: a plain load could be served by a vector L1 that never sees another CU's link.
#include <math.h>

#include <algorithm>

#include "device_utils.hpp"
#include "internal.hpp"
#include "pairwise_math.hpp"
#include "playlist_math.hpp"
#include "scan_block.hpp"

namespace bg {

constexpr int DUP_TILE = 256;  // rows and candidates of a tile: four candidates per lane of a wavefront, lanes l, l + 64, ...

__device__ __forceinline__ uint32_t dup_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void dup_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t dup_find(uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = dup_load(parent + x);
        if (p == x) return x;
        const uint32_t g = dup_load(parent + p);
        if (g == p) return p;
        dup_store(parent + x, g);  // path halving: x is not a root and never becomes one again; g is an ancestor of x
        x = g;
    }
}

__device__ __forceinline__ void dup_unite(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = dup_find(parent, a);
        b = dup_find(parent, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old;  // hi was linked by somebody else meanwhile: go on from where it points now
        b = lo;
    }
}

__global__ __launch_bounds__(256) void dup_init_kernel(uint32_t* __restrict__ parent, uint32_t n, unsigned long long* n_pairs,
                                                       unsigned long long* cursor) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) parent[i] = (uint32_t)i;
    if (i == 0) {
        *n_pairs = 0ull;
        *cursor = 0ull;
    }
}

// in place: a slot holds an ancestor of its row before and the root after, and a root's slot never changes here
__global__ __launch_bounds__(256) void dup_flatten_kernel(uint32_t* label, uint32_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t x = (uint32_t)i, p = dup_load(label + x);
    while (p != x) {
        x = p;
        p = dup_load(label + x);
    }
    dup_store(label + i, x);
}

// tile t of the row-major walk over the tile pairs I <= J of nb blocks: row I starts at I * nb - I (I - 1) / 2
__device__ __forceinline__ void dup_tile_of(uint64_t t, uint64_t nb, uint32_t* I, uint32_t* J) {
    auto start = [&](uint64_t i) { return i * nb - i * (i - 1) / 2; };  // (i = 0: 0 * anything)
    const double b = (double)(2 * nb + 1);
    double est = floor((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
    uint64_t i = est <= 0.0 ? 0 : (uint64_t)est;
    if (i >= nb) i = nb - 1;
    while (i + 1 < nb && start(i + 1) <= t) i++;
    while (i > 0 && start(i) > t) i--;
    *I = (uint32_t)i;
    *J = (uint32_t)(i + (t - start(i)));
}

// D > 0: compile-time feature count (packed arithmetic, candidates in registers).  D == 0: any d <= 64 through pl_distance,
// candidates read from global memory / L2 (slow, exact).
template <int D, int METRIC, bool DIAG>
__global__ __launch_bounds__(256, 2) void dup_join_kernel(const float* __restrict__ X, uint32_t n, uint32_t d_rt, int metric_rt,
                                                          const float* __restrict__ M, const uint32_t* __restrict__ meta,
                                                          float thr, float bound, uint32_t nb, uint32_t row_split,
                                                          uint64_t n_work, uint32_t* parent, unsigned long long* n_pairs,
                                                          unsigned long long* cursor, uint32_t* __restrict__ pairs,
                                                          float* __restrict__ pair_dist, uint64_t max_pairs,
                                                          uint32_t* nan_flag) {
    constexpr bool GENERIC = D == 0;
    static_assert(DUP_TILE == KNN_COLS, "the tile's candidates are one block of scan_block.hpp");
    constexpr int DQ = GENERIC ? PL_DMAX : scan_pitch<D>::DQ;
    constexpr int XP = scan_pitch<D>::XP;
    constexpr bool ROOT = !GENERIC && METRIC != METRIC_COSINE;  // the bound is on the sum before the square root
    __shared__ __attribute__((aligned(16))) float s_q[DUP_TILE][DQ];
    __shared__ __attribute__((aligned(16))) float s_x[GENERIC ? 4 : DUP_TILE * XP];
    __shared__ float s_m[(!GENERIC && METRIC == METRIC_MAHALANOBIS) ? D * D : 1];
    __shared__ float s_nq[DUP_TILE];
    __shared__ uint32_t s_qmeta[DUP_TILE];
    __shared__ unsigned long long s_edges;

    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const uint32_t d = GENERIC ? d_rt : (uint32_t)D;
    const uint32_t rows_per_part = (uint32_t)DUP_TILE / row_split;
    unsigned long long edges = 0ull;  // of this wavefront (the same in every lane)
    bool saw_nan = false;

    if (tid == 0) s_edges = 0ull;
    float wdiag[GENERIC ? 1 : D];
    if constexpr (!GENERIC) scan_load_metric<D, METRIC, DIAG>(M, s_m, wdiag, tid);
    __syncthreads();  // s_edges and M are in place, also for a workgroup whose every work item turns out empty

    for (uint64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
        uint32_t I, J;
        dup_tile_of(w / row_split, nb, &I, &J);
        const bool diag_tile = I == J;
        const uint32_t j0 = J * (uint32_t)DUP_TILE;
        const uint32_t cols_here = (n - j0 < (uint32_t)DUP_TILE) ? n - j0 : (uint32_t)DUP_TILE;
        // the rows of this work item: a slice of block I (the whole block unless the triangle has too few tiles for the device)
        const uint32_t i0 = I * (uint32_t)DUP_TILE + (uint32_t)(w % row_split) * rows_per_part;
        if (i0 >= n) continue;  // (block-uniform: a ragged last block's empty slices)
        const uint32_t rows_here = (n - i0 < rows_per_part) ? n - i0 : rows_per_part;

        __syncthreads();  // every wavefront has finished with the previous tile
        for (uint32_t e = (uint32_t)tid; e < rows_here * d; e += 256u) s_q[e / d][e % d] = X[(uint64_t)i0 * d + e];
        if ((uint32_t)tid < rows_here) s_qmeta[tid] = meta ? meta[i0 + (uint32_t)tid] : 0u;
        if constexpr (GENERIC) __syncthreads();
        else scan_stage_block<D>(s_x, X, j0, cols_here, tid);  // (its closing barrier: the rows and their keys are in place too)
        if (!GENERIC && METRIC == METRIC_COSINE) {
            if ((uint32_t)tid < rows_here) {
                const float* a = s_q[tid];
                s_nq[tid] = sqrtf(unrolled_dot<(GENERIC ? 1 : D)>([&](int kk) { return a[kk]; }, [&](int kk) { return a[kk]; }));
            }
            __syncthreads();
        }

        // the lane's four candidates as two packed pairs: bp[h][kk] = (candidate 2h, candidate 2h + 1), candidate c = row
        // j0 + 64 c + lane; mc[c] its title / artist key
        f2 bp[2][GENERIC ? 1 : D];
        f2 nb2[2];
        uint32_t mc[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const uint32_t lc = 64u * (uint32_t)c + (uint32_t)lane;
            mc[c] = (meta && lc < cols_here) ? meta[j0 + lc] : 0u;
        }
        if constexpr (!GENERIC) {
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
                    nb2[h].x = sqrtf(qq.x);
                    nb2[h].y = sqrtf(qq.y);
                }
            }
        }
        const uint32_t wave_u = (uint32_t)__builtin_amdgcn_readfirstlane(wave);
#pragma unroll 1
        for (uint32_t r = wave_u; r < rows_here; r += 4u) {
            const uint32_t i = i0 + r;
            // pv[c]: what the bound is compared with for candidate c of the lane -- the sum before the root (ROOT) or the distance
            float pv[4];
            if constexpr (GENERIC) {
#pragma unroll 1
                for (int c = 0; c < 4; c++) {
                    const uint32_t lc = 64u * (uint32_t)c + (uint32_t)lane;
                    pv[c] = (lc < cols_here && j0 + lc > i) ? pl_distance(s_q[r], X + (uint64_t)(j0 + lc) * d, d, metric_rt, M) : INFINITY;
                }
            } else {
                f2 ap[DQ / 2];
                scan_query_row<DQ>(s_q[r], ap);
                scan_pair_values<D, METRIC, DIAG>(ap, bp, nb2, s_nq[r], wdiag, s_m, pv);
            }
            // wave-uniform: can any of the wavefront's 256 candidates be an edge of row i?  (a NaN says yes)
            bool maybe;
            if (ROOT) maybe = !(pv[0] > bound) || !(pv[1] > bound) || !(pv[2] > bound) || !(pv[3] > bound);
            else maybe = !(pv[0] >= thr) || !(pv[1] >= thr) || !(pv[2] >= thr) || !(pv[3] >= thr);
            const uint32_t mr = s_qmeta[r];  // 0 (no key, or no title / artist rule at all) joins nothing
            if (mr != 0u) maybe = maybe || mc[0] == mr || mc[1] == mr || mc[2] == mr || mc[3] == mr;
            if (__ballot(maybe) == 0ull) continue;
            // the exact part
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const uint32_t lc = 64u * (uint32_t)c + (uint32_t)lane, j = j0 + lc;  // (j is only used where lc < cols_here)
                const bool valid = lc < cols_here && (!diag_tile || j > i);  // the pairs i < j only: nothing else is looked at
                const float v = ROOT ? sqrtf(pv[c]) : pv[c];
                if (valid && v != v) saw_nan = true;
                const bool edge = valid && (v < thr || (mr != 0u && mc[c] == mr));
                const unsigned long long mask = __ballot(edge);
                if (mask == 0ull) continue;
                const uint32_t cnt = (uint32_t)__popcll(mask);
                edges += cnt;
                if (pairs) {
                    uint32_t lo = 0u, hi = 0u;
                    if (lane == 0) {
                        const unsigned long long base = atomicAdd(cursor, (unsigned long long)cnt);
                        lo = (uint32_t)base;
                        hi = (uint32_t)(base >> 32);
                    }
                    lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
                    hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)hi);
                    const unsigned long long pos = (((unsigned long long)hi << 32) | lo) + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
                    if (edge && pos < max_pairs) {
                        pairs[2 * pos] = i;
                        pairs[2 * pos + 1] = j;
                        if (pair_dist) pair_dist[pos] = v;
                    }
                }
                if (edge) dup_unite(parent, i, j);
            }
        }
    }
    if (lane == 0 && edges) atomicAdd(&s_edges, edges);
    __syncthreads();
    if (tid == 0 && s_edges) atomicAdd(n_pairs, s_edges);
    if (saw_nan) atomicOr(nan_flag, 1u);
}

DupPlan dup_plan(uint64_t n, int n_cus) {
    DupPlan p{};
    p.nb = (uint32_t)((n + DUP_TILE - 1) / DUP_TILE);
    const uint64_t tiles = (uint64_t)p.nb * ((uint64_t)p.nb + 1) / 2;
    // a small triangle: slices of a tile's rows go to workgroups of their own until the device has ~4 per CU
    const uint64_t cus = cus_or_default(n_cus), want = 4 * cus;
    p.row_split = 1;
    while (p.row_split < 8 && tiles * p.row_split < want) p.row_split <<= 1;
    p.n_work = tiles * p.row_split;
    p.grid = (uint32_t)std::min<uint64_t>(p.n_work, 64 * cus);
    return p;
}

float dup_bound(float thr) {
    if (!(thr > 0.0f)) return 0.0f;  // no distance edges; sums <= 0 and NaN still take the root (a negative sum is a NaN distance)
    const float sq = thr * thr;
    if (!(sq < INFINITY)) return INFINITY;
    if (sq < 1.17549435e-38f) return 1.17549435e-38f;  // below the smallest normal float: t^2 < FLT_MIN, whatever the device does with subnormals
    return nextafterf(sq, INFINITY);
}

void launch_dup_init(uint32_t* label, uint32_t n, unsigned long long* n_pairs, unsigned long long* cursor, hipStream_t st) {
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, ((uint64_t)n + 255) / 256);
    hipLaunchKernelGGL(dup_init_kernel, dim3(grid), dim3(256), 0, st, label, n, n_pairs, cursor);
}

void launch_dup_flatten(uint32_t* label, uint32_t n, hipStream_t st) {
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, ((uint64_t)n + 255) / 256);
    hipLaunchKernelGGL(dup_flatten_kernel, dim3(grid), dim3(256), 0, st, label, n);
}

void launch_dup_join(const float* X, uint32_t n, uint32_t d, int metric, const float* M, int m_is_diag, const uint32_t* meta,
                     float thr, const DupPlan& p, uint32_t* label, unsigned long long* n_pairs, unsigned long long* cursor,
                     uint32_t* pairs, float* pair_dist, uint64_t max_pairs, uint32_t* nan_flag, hipStream_t st) {
    const float bound = dup_bound(thr);
    for_metric_form<true>(d, metric, m_is_diag, [&](auto D, auto M_, auto G) {
        hipLaunchKernelGGL((dup_join_kernel<D(), M_(), G()>), dim3(p.grid), dim3(256), 0, st, X, n, d, metric, M, meta, thr, bound, p.nb,
                           p.row_split, p.n_work, label, n_pairs, cursor, pairs, pair_dist, max_pairs, nan_flag);
    });
}

}  // namespace bg
