// kernels_moments.hip -- the first and second moments of a song library, per group of a labelling and pooled (compiled with
// -ffp-contract=off): counts, means, sums of squared deviations, extrema, and the d x d scatter matrix.
//
// Every f64 sum here is THE BLOCKED SUM of include/blissgpu.h: sequential sums (begun at 0.0) of consecutive blocks of 256 terms,
// then the same over the block sums, level by level, until one value is left.  A "level" is one launch: what a work item adds,
// and in which order, is a function of the member counts alone, never of the grid, and nothing is added with atomics.  (A block
// sum is never -0.0, so summing a single block sum once more, 0.0 + v, returns v: a group that needs fewer levels than the
// largest group rides through the surplus ones unchanged.)
//
//   moments_plan_kernel     one workgroup: the member counts (from the k-means sort's arow_off, or n when there are no labels)
//                           and, per level l, the exclusive prefix off[l][g] of ceil(count_g / 256^(l + 1)): where group g's
//                           block sums of that level start.
//   moments_sum_kernel      level 0 of the means: one wavefront per (group, block of 256 members), found by a search in off[0],
//                           so one giant group spreads over the whole GPU.  The members' rows are gathered 64 at a time into
//                           LDS (every lane loads: the row lists are ascending, a group's rows share cache lines), then lane r
//                           adds feature r over the rows in order.  It also looks at every value (NaN, infinity) and, 256
//                           labels per wavefront, at every label (>= k).
//   moments_m2_kernel       the same walk with u = x - mean: the sums of u u, and the extrema as atomic min / max of
//                           order-preserving integer keys (an order-free operation; -0.0 below +0.0), tried only by a wavefront
//                           whose block improves on what is there.
//   moments_scatter_kernel  level 0 of S: one wavefront per block of 256 consecutive rows.  32 rows at a time are centred with
//                           their label's mean (f64) into LDS; a lane owns a 3 x 3 tile of the upper triangle (d = 23: 36
//                           tiles, d = 20: 28; the generic path gives a lane up to four tiles, d = 64: 253), so a row costs it 6
//                           LDS reads for 9 products, all broadcasts or conflict-free (a row is 24 doubles).  Products below
//                           the diagonal in a diagonal tile are computed and dropped.
//   moments_reduce_kernel   every further level, of the per-group sums and of S alike: one thread per (block of 256 partials,
//                           value), 256 sequential adds, coalesced over the values.  Its last launch divides by the count
//                           (mean), copies (m2) or writes the triangle and its mirror (S).
//   moments_finish_kernel   keys -> min / max; +inf / -inf for an empty group.
#include <math.h>

#include <algorithm>

#include "device_utils.hpp"
#include "internal.hpp"
#include "launch_forms.hpp"

namespace bg {

constexpr uint32_t MO_BLOCK = 256;  // = BLISSGPU_MOMENTS_BLOCK
constexpr uint32_t MO_SUB = 64;     // rows per LDS tile of the per-group walk
constexpr uint32_t MO_SSUB = 32;    // rows per LDS tile of the scatter (the generic path: 16, its rows are up to 66 doubles)
constexpr uint32_t MO_TILE = 3;     // a lane's tile of the triangle is MO_TILE x MO_TILE

// LDS traffic between the lanes of ONE wavefront
__device__ __forceinline__ void mo_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the largest g in [0, K) with off[g] <= p  (off[0] == 0 <= p; empty groups repeat their offset, the last of them wins)
__device__ __forceinline__ uint32_t mo_group_of(const uint32_t* __restrict__ off, uint32_t K, uint32_t p) {
    uint32_t lo = 0, hi = K;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (off[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// order-preserving key of a float: -0.0 below +0.0, every finite value between the infinities
__device__ __forceinline__ uint32_t mo_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float mo_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__global__ __launch_bounds__(256) void moments_plan_kernel(const uint32_t* __restrict__ arow_off, uint32_t n, uint32_t K,
                                                           uint32_t levels, uint32_t* __restrict__ off,
                                                           uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_sum[256];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (K + 255u) / 256u;
    const uint32_t g0 = std::min(K, tid * per), g1 = std::min(K, g0 + per);
    uint64_t div = MO_BLOCK;
    for (uint32_t l = 0; l < levels; l++, div *= MO_BLOCK) {
        uint32_t mine = 0;
        for (uint32_t g = g0; g < g1; g++) {
            const uint32_t cnt = arow_off ? arow_off[g + 1] - arow_off[g] : n;
            if (l == 0) counts[g] = cnt;
            mine += (uint32_t)(((uint64_t)cnt + div - 1) / div);
        }
        s_sum[tid] = mine;
        __syncthreads();
        uint32_t before = 0;
        for (uint32_t t = 0; t < tid; t++) before += s_sum[t];
        uint32_t* o = off + (size_t)l * (K + 1);
        for (uint32_t g = g0; g < g1; g++) {
            const uint32_t cnt = arow_off ? arow_off[g + 1] - arow_off[g] : n;
            o[g] = before;
            before += (uint32_t)(((uint64_t)cnt + div - 1) / div);
        }
        if (tid == 255u) o[K] = before;  // (thread 255's range ends at K, or is empty behind it: `before` is the total)
        __syncthreads();
    }
}

// MODE 0: the sums of x (and the checks); MODE 1: the sums of (x - mean)^2 and the extrema.  D == 0: any d <= 64.
template <int D, int MODE>
__device__ __forceinline__ void moments_group_body(const float* __restrict__ X, const uint32_t* __restrict__ arow,
                                                   const uint32_t* __restrict__ arow_off, const uint32_t* __restrict__ off0,
                                                   const uint32_t* __restrict__ labels, const double* __restrict__ mean, uint32_t n,
                                                   uint32_t K, uint32_t d_rt, double* __restrict__ part, uint32_t* key_min,
                                                   uint32_t* key_max, uint32_t* flags) {
    constexpr uint32_t DMAX = D ? D : 64;
    __shared__ float s_x[4][MO_SUB * DMAX];
    const uint32_t d = D ? (uint32_t)D : d_rt;
    const uint32_t lane = (uint32_t)lane_id(), wave = (uint32_t)wave_id();
    const uint32_t p = blockIdx.x * 4u + wave;
    float* tile = s_x[wave];

    if (MODE == 0 && labels) {  // the wavefront's share of the label check: labels [256 p, 256 p + 256)
        bool bad = false;
        for (uint32_t c = 0; c < 4u; c++) {
            const uint64_t i = (uint64_t)p * MO_BLOCK + 64u * c + lane;
            if (i < (uint64_t)n && labels[i] >= K) bad = true;
        }
        if (bad) atomicOr(&flags[1], MO_ERR_LABEL);
    }
    if (p >= off0[K]) return;
    const uint32_t g = mo_group_of(off0, K, p);
    const uint32_t lo = arow_off ? arow_off[g] : 0u, hi = arow_off ? arow_off[g + 1] : n;
    const uint64_t start = (uint64_t)lo + (uint64_t)(p - off0[g]) * MO_BLOCK;
    const uint32_t members = (uint32_t)std::min<uint64_t>(MO_BLOCK, (uint64_t)hi - start);

    double acc = 0.0;
    const double mu = (MODE == 1 && lane < d) ? mean[(size_t)g * d + lane] : 0.0;
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
    bool not_finite = false, bad_row = false;
    for (uint32_t t0 = 0; t0 < members; t0 += MO_SUB) {
        const uint32_t rows = std::min(MO_SUB, members - t0);
        // the row of tile position `lane`
        uint32_t my_row = 0;
        if (lane < rows) {
            const uint64_t pos = start + t0 + lane;
            my_row = arow ? arow[pos] : (uint32_t)pos;
            if (my_row >= n) {  // (only behind a label >= k: the sort left the end of the last list unwritten)
                bad_row = true;
                my_row = 0;
            }
        }
        const uint32_t elems = rows * d;
        for (uint32_t e0 = 0; e0 < elems; e0 += 64u) {  // (every lane takes part in the shuffle: the trip count is uniform)
            const uint32_t e = std::min(e0 + lane, elems - 1u);
            const uint32_t row = e / d, r = e - row * d;
            const uint32_t ri = (uint32_t)__shfl((int)my_row, (int)row, 64);
            if (e0 + lane < elems) tile[e] = X[(uint64_t)ri * d + r];
        }
        mo_wave_sync();
        if (lane < d) {
#pragma unroll 8
            for (uint32_t row = 0; row < rows; row++) {
                const float v = tile[row * d + lane];
                if (MODE == 0) {
                    if (!isfinite(v)) not_finite = true;
                    acc = acc + (double)v;
                } else {
                    const double u = (double)v - mu;
                    const double sq = u * u;
                    acc = acc + sq;
                    const uint32_t key = mo_key(v);
                    kmin = std::min(kmin, key);
                    kmax = std::max(kmax, key);
                }
            }
        }
        mo_wave_sync();
    }
    if (lane < d) {
        part[(size_t)p * d + lane] = acc;
        if (MODE == 1 && key_min) {
            uint32_t* a = key_min + (size_t)g * d + lane;
            uint32_t* b = key_max + (size_t)g * d + lane;
            if (kmin < __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(a, kmin);
            if (kmax > __hip_atomic_load(b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(b, kmax);
        }
    }
    if (not_finite) atomicOr(&flags[0], 1u);
    if (bad_row) atomicOr(&flags[1], MO_ERR_LABEL);
}

template <int D>
__global__ __launch_bounds__(256) void moments_sum_kernel(const float* __restrict__ X, const uint32_t* __restrict__ arow,
                                                          const uint32_t* __restrict__ arow_off, const uint32_t* __restrict__ off0,
                                                          const uint32_t* __restrict__ labels, uint32_t n, uint32_t K, uint32_t d,
                                                          double* __restrict__ part, uint32_t* flags) {
    moments_group_body<D, 0>(X, arow, arow_off, off0, labels, nullptr, n, K, d, part, nullptr, nullptr, flags);
}

template <int D>
__global__ __launch_bounds__(256) void moments_m2_kernel(const float* __restrict__ X, const uint32_t* __restrict__ arow,
                                                         const uint32_t* __restrict__ arow_off, const uint32_t* __restrict__ off0,
                                                         const double* __restrict__ mean, uint32_t n, uint32_t K, uint32_t d,
                                                         double* __restrict__ part, uint32_t* key_min, uint32_t* key_max,
                                                         uint32_t* flags) {
    moments_group_body<D, 1>(X, arow, arow_off, off0, nullptr, mean, n, K, d, part, key_min, key_max, flags);
}

// index of (r, c), r <= c, in the row-major upper triangle
__host__ __device__ __forceinline__ uint32_t mo_tri(uint32_t r, uint32_t c, uint32_t d) { return r * d - r * (r - 1u) / 2u + (c - r); }

template <int D>
__global__ __launch_bounds__(256) void moments_scatter_kernel(const float* __restrict__ X, const uint32_t* __restrict__ labels,
                                                              const double* __restrict__ mean, uint32_t n, uint32_t K, uint32_t d_rt,
                                                              double* __restrict__ part, uint32_t* flags) {
    constexpr uint32_t DMAX = D ? D : 64;
    constexpr uint32_t GMAX = (DMAX + MO_TILE - 1) / MO_TILE, PMAX = GMAX * MO_TILE;
    constexpr uint32_t NT = (GMAX * (GMAX + 1) / 2 + 63) / 64;  // tiles per lane: 1 at d = 20 and 23, 4 at d = 64
    constexpr uint32_t SSUB = D ? MO_SSUB : MO_SSUB / 2;
    __shared__ double s_u[4][SSUB * PMAX];
    const uint32_t d = D ? (uint32_t)D : d_rt;
    const uint32_t G = (d + MO_TILE - 1) / MO_TILE, P = G * MO_TILE, T = G * (G + 1u) / 2u, w = d * (d + 1u) / 2u;
    const uint32_t lane = (uint32_t)lane_id(), wave = (uint32_t)wave_id();
    const uint64_t blk = (uint64_t)blockIdx.x * 4u + wave;
    const uint64_t i0 = blk * MO_BLOCK;
    if (i0 >= (uint64_t)n) return;
    const uint32_t members = (uint32_t)std::min<uint64_t>(MO_BLOCK, (uint64_t)n - i0);
    double* tile = s_u[wave];

    // the lane's tiles: tile q = lane + 64 t is (ti, tj), ti <= tj, counted row by row over the upper triangle of the G x G grid
    uint32_t ta[NT], tb[NT];
    bool live[NT];
#pragma unroll
    for (uint32_t t = 0; t < NT; t++) {
        const uint32_t q = lane + 64u * t;
        live[t] = q < T;
        uint32_t ti = 0, rem = live[t] ? q : 0u;
        while (rem >= G - ti) {
            rem -= G - ti;
            ti++;
        }
        ta[t] = ti * MO_TILE;
        tb[t] = (ti + rem) * MO_TILE;
    }
    double acc[NT][MO_TILE][MO_TILE];
#pragma unroll
    for (uint32_t t = 0; t < NT; t++)
#pragma unroll
        for (uint32_t a = 0; a < MO_TILE; a++)
#pragma unroll
            for (uint32_t b = 0; b < MO_TILE; b++) acc[t][a][b] = 0.0;

    // the padding columns d .. P - 1 are zeros, written once (the staging below never touches them)
    for (uint32_t e = lane; e < SSUB * (P - d); e += 64u) tile[(e / (P - d)) * P + d + e % (P - d)] = 0.0;
    bool bad = false;
    for (uint32_t t0 = 0; t0 < members; t0 += SSUB) {
        const uint32_t rows = std::min<uint32_t>(SSUB, members - t0);
        uint32_t my_label = 0;
        if (labels && lane < rows) {
            my_label = labels[i0 + t0 + lane];
            if (my_label >= K) {
                bad = true;
                my_label = 0;
            }
        }
        const uint32_t elems = rows * d;
        for (uint32_t e0 = 0; e0 < elems; e0 += 64u) {  // (every lane takes part in the shuffle: the trip count is uniform)
            const uint32_t e = std::min(e0 + lane, elems - 1u);
            const uint32_t row = e / d, r = e - row * d;
            const uint32_t l = (uint32_t)__shfl((int)my_label, (int)row, 64);
            if (e0 + lane < elems) tile[row * P + r] = (double)X[(i0 + t0) * d + e] - mean[(size_t)l * d + r];
        }
        mo_wave_sync();
#pragma unroll 2
        for (uint32_t row = 0; row < rows; row++) {
            const double* u = tile + row * P;
#pragma unroll
            for (uint32_t t = 0; t < NT; t++) {
                if (NT > 1 && !live[t]) continue;
                double a[MO_TILE], b[MO_TILE];
#pragma unroll
                for (uint32_t k = 0; k < MO_TILE; k++) {
                    a[k] = u[ta[t] + k];
                    b[k] = u[tb[t] + k];
                }
#pragma unroll
                for (uint32_t x = 0; x < MO_TILE; x++)
#pragma unroll
                    for (uint32_t y = 0; y < MO_TILE; y++) {
                        const double prod = a[x] * b[y];
                        acc[t][x][y] = acc[t][x][y] + prod;
                    }
            }
        }
        mo_wave_sync();
    }
#pragma unroll
    for (uint32_t t = 0; t < NT; t++) {
        if (!live[t]) continue;
#pragma unroll
        for (uint32_t x = 0; x < MO_TILE; x++)
#pragma unroll
            for (uint32_t y = 0; y < MO_TILE; y++) {
                const uint32_t r = ta[t] + x, c = tb[t] + y;
                if (r <= c && c < d) part[blk * w + mo_tri(r, c, d)] = acc[t][x][y];
            }
    }
    if (bad) atomicOr(&flags[1], MO_ERR_LABEL);
}

// out block sum j of group g = 0.0 + in[256 j] + in[256 j + 1] + ... within the group's `in` range; offsets NULL: one group with
// in_n / out_n entries.  mode: MO_RED_PART -> out [.][w]; MO_RED_MEAN -> dst[g][v] = sum / count_g; MO_RED_M2 -> dst[g][v] = sum;
// MO_RED_SCATTER -> dst[r][c] = dst[c][r] = sum, v the triangle index (the last three run when one partial per group is left)
__global__ __launch_bounds__(256) void moments_reduce_kernel(const double* __restrict__ in, const uint32_t* __restrict__ in_off,
                                                             uint32_t in_n, double* __restrict__ out,
                                                             const uint32_t* __restrict__ out_off, uint32_t out_n, uint32_t K,
                                                             uint32_t w, int mode, const uint32_t* __restrict__ counts,
                                                             double* __restrict__ dst, uint32_t d) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t p64 = t / w;
    const uint32_t v = (uint32_t)(t - p64 * w);
    const uint32_t total = out_off ? out_off[K] : out_n;
    if (p64 >= (uint64_t)total) return;
    const uint32_t p = (uint32_t)p64;
    const uint32_t g = out_off ? mo_group_of(out_off, K, p) : 0u;
    const uint32_t j = p - (out_off ? out_off[g] : 0u);
    const uint32_t lo = in_off ? in_off[g] : 0u, hi = in_off ? in_off[g + 1] : in_n;
    const uint64_t i0 = (uint64_t)lo + (uint64_t)j * MO_BLOCK, i1 = std::min<uint64_t>(hi, i0 + MO_BLOCK);
    double acc = 0.0;
#pragma unroll 8
    for (uint64_t i = i0; i < i1; i++) acc = acc + in[i * w + v];
    if (mode == MO_RED_PART) {
        out[(uint64_t)p * w + v] = acc;
    } else if (mode == MO_RED_MEAN) {
        dst[(size_t)g * w + v] = acc / (double)counts[g];
    } else if (mode == MO_RED_M2) {
        dst[(size_t)g * w + v] = acc;
    } else {
        uint32_t r = 0, rem = v;
        while (rem >= d - r) {
            rem -= d - r;
            r++;
        }
        const uint32_t c = r + rem;
        dst[(size_t)r * d + c] = acc;
        dst[(size_t)c * d + r] = acc;
    }
}

__global__ __launch_bounds__(256) void moments_finish_kernel(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ key_min,
                                                             const uint32_t* __restrict__ key_max, uint32_t K, uint32_t d,
                                                             float* __restrict__ mn, float* __restrict__ mx) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= (uint64_t)K * d) return;
    const bool empty = counts[e / d] == 0u;
    mn[e] = empty ? INFINITY : mo_unkey(key_min[e]);
    mx[e] = empty ? -INFINITY : mo_unkey(key_max[e]);
}

MomentsPlan moments_plan(uint64_t n, uint32_t K) {
    MomentsPlan p{};
    const uint64_t groups = std::min<uint64_t>(K, n);  // at most this many groups have members
    uint64_t m = n, div = MO_BLOCK;
    do {
        m = (m + MO_BLOCK - 1) / MO_BLOCK;
        p.items[p.levels] = (uint32_t)(n / div + groups);  // sum_g ceil(count_g / div) <= floor(n / div) + the non-empty groups
        p.blocks[p.levels] = (uint32_t)m;                  // ceil(n / div)
        p.levels++;
        div *= MO_BLOCK;
    } while (m > 1);
    return p;
}

void launch_moments_plan(const uint32_t* arow_off, uint32_t n, uint32_t K, const MomentsPlan& p, uint32_t* off, uint32_t* counts,
                         hipStream_t st) {
    hipLaunchKernelGGL(moments_plan_kernel, dim3(1), dim3(256), 0, st, arow_off, n, K, p.levels, off, counts);
}

void launch_moments_sum(const MomentsArgs& a, const MomentsPlan& p, double* part, hipStream_t st) {
    const dim3 grid((p.items[0] + 3u) / 4u), block(256);
    with_d(a.d, [&](auto D) {
        hipLaunchKernelGGL((moments_sum_kernel<D()>), grid, block, 0, st, a.X, a.arow, a.arow_off, a.off, a.labels, a.n, a.K, a.d, part,
                           a.flags);
    });
}

void launch_moments_m2(const MomentsArgs& a, const MomentsPlan& p, double* part, bool extrema, hipStream_t st) {
    const dim3 grid((p.items[0] + 3u) / 4u), block(256);
    uint32_t *kmin = extrema ? a.key_min : nullptr, *kmax = extrema ? a.key_max : nullptr;
    with_d(a.d, [&](auto D) {
        hipLaunchKernelGGL((moments_m2_kernel<D()>), grid, block, 0, st, a.X, a.arow, a.arow_off, a.off, a.mean, a.n, a.K, a.d, part, kmin,
                           kmax, a.flags);
    });
}

void launch_moments_scatter(const MomentsArgs& a, const MomentsPlan& p, double* part, hipStream_t st) {
    const dim3 grid((p.blocks[0] + 3u) / 4u), block(256);
    with_d(a.d, [&](auto D) {
        hipLaunchKernelGGL((moments_scatter_kernel<D()>), grid, block, 0, st, a.X, a.labels, a.mean, a.n, a.K, a.d, part, a.flags);
    });
}

void launch_moments_reduce(const double* in, const uint32_t* in_off, uint32_t in_n, double* out, const uint32_t* out_off,
                           uint32_t out_n, uint32_t out_bound, uint32_t K, uint32_t w, int mode, const uint32_t* counts, double* dst,
                           uint32_t d, hipStream_t st) {
    const uint64_t threads = (uint64_t)out_bound * w;
    if (threads == 0) return;
    hipLaunchKernelGGL(moments_reduce_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st, in, in_off, in_n, out, out_off,
                       out_n, K, w, mode, counts, dst, d);
}

void launch_moments_finish(const uint32_t* counts, const uint32_t* key_min, const uint32_t* key_max, uint32_t K, uint32_t d, float* mn,
                           float* mx, hipStream_t st) {
    const uint64_t e = (uint64_t)K * d;
    hipLaunchKernelGGL(moments_finish_kernel, dim3((uint32_t)((e + 255) / 256)), dim3(256), 0, st, counts, key_min, key_max, K, d, mn, mx);
}

}  // namespace bg
