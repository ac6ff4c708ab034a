// kernels_chamfer.hip -- group-to-group set distances of a labelled song library (the average nearest-member, or Chamfer,
// distance), all pairs and no matrix stored (compiled with -ffp-contract=off).
//
// m(i, c) = the smallest dist(i, j) over the members j of group c; T(a, c) = the blocked f64 sum of (double)m(i, c) over the
// members i of a in ascending row; D(a -> c) = T(a, c) / size_a; A(a, c) = D(a -> c) or the mean of the two directions
// (include/blissgpu.h has the contract).  The distances are those of the all-pairs kernel bit for bit.
//
// The labels are sorted first with the k-means kernels as they are: group c's members are arow[arow_off[c] .. arow_off[c + 1])
// in ascending index, and "position" below is a place in that sorted order.  The target groups are taken in slabs [s0, s1) of
// at most `slab` groups, one scan and one reduce launch per slab; no output bit depends on the slab.
//
//   chamfer_scan_kernel    silhouette_scan_kernel's shape with a minimum in the f64 sum's place: a lane keeps four songs in
//                          registers as two packed column pairs, a wavefront 256 CONSECUTIVE POSITIONS (so small groups are
//                          packed: a wavefront holds songs of many groups), and the workgroup walks the slab's rows in group
//                          order through LDS tiles read as ds_read_b128 broadcasts.  Per row: pair_sum, one unsigned minimum
//                          and one unsigned maximum of the sum's bit pattern.  Every non-cosine distance of kernels_pairwise.hip
//                          ends in ONE correctly rounded square root of one f32 sum; that root is monotone, so the minimum of
//                          the roots is the root of the minimum and is taken once per (song, group).  A sum is >= +0, +inf, NaN
//                          or negative (an M that is not positive semi-definite; its root is NaN): the first two order as
//                          unsigned integers, the last two lie above 0x7F800000, which is what the maximum is for (a hardware
//                          float minimum would drop a NaN).  The generic form (any d <= 64, pl_distance) takes the same minimum
//                          and maximum of the finished distances.  Where a group ends -- uniform across the workgroup -- every
//                          lane writes its four minima to the slab, laid out [group - s0][position]: consecutive lanes,
//                          consecutive addresses.  The entry of a song's own group is written like any other and never read.
//   chamfer_reduce_kernel  a wavefront per (a, c): the contract's tree over blocks of 256 terms, term u of a block in lane
//                          u % 64, slot u / 64: the levels h = 128 and 64 are adds between a lane's own slots, the levels 32 .. 1
//                          cross-lane shifts.  Block sums are added in ascending order by lane 0, which divides and writes D[a][c].
//                          A group a of at most 32 songs (most albums) needs W <= 32 lanes per tree -- the padding adds +0.0,
//                          which changes no term --, so a wavefront reduces 64 / W target groups at once.
//   chamfer_select_kernel  a workgroup per query row: A(a, .) into a row buffer, then t rounds that each take the smallest
//                          (A, c) above the previous pick -- the (value, index) order of knn_list.hpp's keys, equal values to
//                          the lower c --, the padding, and, when asked, a row of `matrix` per group.  The same launch writes
//                          sizes and raises the error word: a label >= K, a query >= K.
#include <math.h>

#include <algorithm>

#include "device_utils.hpp"
#include "internal.hpp"
#include "pairwise_math.hpp"
#include "playlist_math.hpp"
#include "scan_block.hpp"

namespace bg {

constexpr int CH_TILE_FLOATS = 6144;  // 24 KiB of library rows per tile: 256 rows at d = 23 (pitch 24)
constexpr int CH_TILE_ROWS = 256;
constexpr int CH_SONGS_PER_WAVE = 256;
constexpr uint32_t CH_NONE = 0xFFFFFFFFu;
constexpr uint32_t CH_INF_BITS = 0x7F800000u;

__device__ __forceinline__ uint32_t ch_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the first group c in [lo, K] with arow_off[c] >= t (arow_off[K] >= t)
__device__ __forceinline__ uint32_t ch_first_group(const uint32_t* __restrict__ arow_off, uint32_t K, uint32_t lo, uint64_t t) {
    const uint32_t c = t ? find_segment(arow_off, K + 1u, (uint32_t)(t - 1u)) + 1u : 0u;
    return c < lo ? lo : c;
}

// D > 0: compile-time feature count (packed arithmetic, the lane's songs in registers).  D == 0: any d <= 64 through pl_distance,
// the lane's songs read from global memory / L2 (slow, exact).  blockDim.x = 64 * (wavefronts per workgroup): 1 .. 4.
template <int D, int METRIC, bool DIAG>
__global__ __launch_bounds__(256) void chamfer_scan_kernel(const ChamferArgs a) {
    constexpr bool GENERIC = D == 0;
    constexpr int DD = GENERIC ? 1 : D;
    constexpr int DQ = GENERIC ? 1 : ((D + 3) & ~3);  // LDS pitch of a row: 16-byte aligned -> ds_read_b128 broadcasts
    __shared__ __attribute__((aligned(16))) float s_c[CH_TILE_FLOATS];
    __shared__ float s_m[(!GENERIC && METRIC == METRIC_MAHALANOBIS) ? D * D : 1];

    const float* __restrict__ X = a.X;
    const uint32_t* __restrict__ arow_off = a.arow_off;
    const uint32_t* __restrict__ arow = a.arow;
    const uint32_t n = a.n, K = a.K, Y = a.Y, s0 = a.s0, s1 = a.s1;
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, lane = (uint32_t)lane_id(), wave = (uint32_t)wave_id();
    const uint32_t d = GENERIC ? a.d : (uint32_t)D;
    const uint32_t pitch = GENERIC ? d : (uint32_t)DQ;
    const uint32_t tile_rows = std::min<uint32_t>((uint32_t)CH_TILE_ROWS, (uint32_t)CH_TILE_FLOATS / pitch);
    const uint32_t g = blockIdx.y;
    // the wavefront's 256 positions: slot c of the lane is position p0 + 64 c + lane (64-bit: n may be close to 2^32)
    const uint64_t p0 = ((uint64_t)blockIdx.x * (nthr / 64u) + wave) * (uint64_t)CH_SONGS_PER_WAVE;

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

    // the lane's four songs and their own groups; a position past n holds nothing (and neither does an arow entry past n, which
    // only a label >= K leaves behind: the call fails then)
    bool valid[4];
    uint32_t song[4], own[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint64_t p = p0 + 64u * (uint32_t)c + lane;
        valid[c] = p < (uint64_t)n;
        song[c] = valid[c] ? arow[p] : 0u;
        if (song[c] >= n) {
            valid[c] = false;
            song[c] = 0u;
        }
        own[c] = valid[c] ? a.labels[song[c]] : CH_NONE;
    }
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

    // the slab's rows [R0, R1) of the sorted order, and this column group's run of groups [c_lo, c_hi): those whose first row,
    // counted from R0, falls into [ceil(g rows / Y), ceil((g + 1) rows / Y)) -- a group is never split
    const uint32_t R0 = ch_uniform(arow_off[s0]), R1 = ch_uniform(arow_off[s1]);
    const uint64_t rows = R1 - R0;
    const uint32_t c_lo = ch_uniform(ch_first_group(arow_off, K, s0, (uint64_t)R0 + ((uint64_t)g * rows + Y - 1u) / Y));
    const uint32_t c_hi = ch_uniform(std::min<uint32_t>(s1, ch_first_group(arow_off, K, s0, (uint64_t)R0 + ((uint64_t)(g + 1u) * rows + Y - 1u) / Y)));
    if (c_lo >= c_hi) return;
    const uint32_t r_lo = ch_uniform(arow_off[c_lo]), r_hi = ch_uniform(arow_off[c_hi]);

    uint32_t mn[4], mx[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        mn[c] = CH_NONE;
        mx[c] = 0u;
    }
    bool saw_nan = false;

    // cl = the group the walk is in, rows [start, end) of the sorted order; runs of empty groups are stepped over
    uint32_t cl = c_lo, start = r_lo, end = r_lo;
    while (cl < c_hi && (end = ch_uniform(arow_off[cl + 1u])) == start) cl++;

    for (uint32_t t0 = r_lo; t0 < r_hi; t0 += tile_rows) {
        const uint32_t rows_here = std::min<uint32_t>(tile_rows, r_hi - t0);
        if (t0 != r_lo) __syncthreads();  // every wavefront has finished with the previous tile
        {
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
            const uint32_t seg = std::min<uint32_t>(rows_here, end - t0);  // (end > t0 + r: the walk is inside group cl)
#pragma unroll 1
            for (; r < seg; r++) {
                if constexpr (GENERIC) {
#pragma unroll 1
                    for (int c = 0; c < 4; c++) {
                        if (!valid[c]) continue;
                        const uint32_t vb = __float_as_uint(pl_distance(X + (uint64_t)song[c] * d, s_c + r * pitch, d, a.metric, a.M));
                        mn[c] = min(mn[c], vb);
                        mx[c] = max(mx[c], vb);
                    }
                } else {
                    f2 ap[DQ / 2];
                    scan_query_row<DQ>(&s_c[r * (uint32_t)DQ], ap);
                    f2 sum0 = pair_sum<DD, METRIC, DIAG>(ap, bp[0], wdiag, s_m);
                    // (general M: one pair's 2 x d differences and products at a time, as in the k-nearest scan)
                    if (METRIC == METRIC_MAHALANOBIS && !DIAG) asm volatile("" : "+v"(sum0));
                    const f2 sum1 = pair_sum<DD, METRIC, DIAG>(ap, bp[1], wdiag, s_m);
                    const uint32_t pv[4] = {__float_as_uint(sum0.x), __float_as_uint(sum0.y), __float_as_uint(sum1.x), __float_as_uint(sum1.y)};
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        mn[c] = min(mn[c], pv[c]);
                        mx[c] = max(mx[c], pv[c]);
                    }
                }
            }
            if (t0 + r == end) {  // group cl ends here (uniform): the root of the minimum, one store per song
                float* __restrict__ col = a.minima + (uint64_t)(cl - s0) * n;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    if (valid[c]) {
                        if (mx[c] > CH_INF_BITS && own[c] != cl) saw_nan = true;
                        const float m = __uint_as_float(mn[c]);
                        col[p0 + 64u * (uint32_t)c + lane] = GENERIC ? m : sqrtf(m);
                    }
                    mn[c] = CH_NONE;
                    mx[c] = 0u;
                }
                cl++;
                start = end;
                while (cl < c_hi && (end = ch_uniform(arow_off[cl + 1u])) == start) cl++;
            }
        }
    }
    if (saw_nan) atomicOr(a.flags, 1u);
}

// block (ga, y), wavefront w: group ga against the slab's groups s0 + 4 y + w, + 4 gridDim.y, ...
__global__ __launch_bounds__(256) void chamfer_reduce_kernel(const ChamferArgs a) {
    const uint32_t* __restrict__ arow_off = a.arow_off;
    const uint32_t n = a.n, K = a.K, s0 = a.s0, s1 = a.s1;
    const uint32_t lane = (uint32_t)lane_id(), wave = (uint32_t)wave_id();
    const uint32_t ga = blockIdx.x;
    const uint32_t lo = ch_uniform(arow_off[ga]), hi = ch_uniform(arow_off[ga + 1u]);
    if (hi <= lo || hi > n) return;
    const double size = (double)(hi - lo);
    if (hi - lo <= 32u) {
        // a small group: its terms u >= W (W = the power of two >= its size) are the padding +0.0, and x + 0.0 is x for every
        // x >= +0, so the levels h >= W change nothing and W lanes hold the whole tree.  The wavefront takes 64 / W target groups
        // at a time, lanes [W s, W s + W) group cbase + s: the levels h < W never leave a group's lanes
        uint32_t W = 1u;
        while (W < hi - lo) W <<= 1;
        const uint32_t per = 64u / W, sub = lane / W, u = lane % W;
        for (uint32_t cbase = s0 + (blockIdx.y * 4u + wave) * per; cbase < s1; cbase += 4u * gridDim.y * per) {
            const uint32_t c = cbase + sub;
            const bool live = c < s1 && c != ga && arow_off[c < s1 ? c + 1u : s1] != arow_off[c < s1 ? c : s1];
            double x = (live && u < hi - lo) ? (double)a.minima[(uint64_t)(c - s0) * n + lo + u] : 0.0;
            for (uint32_t h = W >> 1; h > 0; h >>= 1) x = x + __shfl_down(x, h, WAVE);  // (uniform trip count: W is)
            if (live && u == 0) a.D[(uint64_t)ga * K + c] = (0.0 + x) / size;
        }
        return;
    }
    for (uint32_t c = s0 + blockIdx.y * 4u + wave; c < s1; c += 4u * gridDim.y) {
        if (c == ga || ch_uniform(arow_off[c + 1u]) == ch_uniform(arow_off[c])) continue;
        const float* __restrict__ m = a.minima + (uint64_t)(c - s0) * n;
        double total = 0.0;
        for (uint32_t b0 = lo; b0 < hi; b0 += 256u) {
            double v[4];
#pragma unroll
            for (int s = 0; s < 4; s++) {  // term u = 64 s + lane of the block; past the group: the padding +0.0
                const uint32_t p = b0 + 64u * (uint32_t)s + lane;  // (b0 < n < 2^32 - 1 and hi - b0 >= 1: no wrap below hi + 255)
                v[s] = (p < hi && p >= b0) ? (double)m[p] : 0.0;
            }
            v[0] = v[0] + v[2];  // h = 128
            v[1] = v[1] + v[3];
            double x = v[0] + v[1];  // h = 64
#pragma unroll
            for (int h = 32; h > 0; h >>= 1) x = x + __shfl_down(x, h, WAVE);  // lanes < h hold the level's sums
            total = total + x;
        }
        if (lane == 0) a.D[(uint64_t)ga * K + c] = total / size;
    }
}

// the smaller of two (value bits, group) pairs: the key order of the k-nearest lists, equal values to the lower group
__device__ __forceinline__ void ch_take(unsigned long long& kb, uint32_t& kc, unsigned long long ob, uint32_t oc) {
    if (ob < kb || (ob == kb && oc < kc)) {
        kb = ob;
        kc = oc;
    }
}

// block b: jobs b, b + gridDim.x, ...: job < q is query row `job`, job >= q row job - q of `matrix` (only when it is asked for)
__global__ __launch_bounds__(256) void chamfer_select_kernel(const ChamferArgs a) {
    __shared__ unsigned long long s_kb[4];
    __shared__ uint32_t s_kc[4];
    const uint32_t* __restrict__ arow_off = a.arow_off;
    const uint32_t n = a.n, K = a.K, q = a.q, t = a.t;
    const uint32_t tid = threadIdx.x, lane = (uint32_t)lane_id(), wave = (uint32_t)wave_id();
    const bool symmetric = a.mode == 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + tid; i < (uint64_t)n; i += (uint64_t)gridDim.x * 256u)
        if (a.labels[i] >= K) atomicOr(a.flags + 1, CH_ERR_LABEL);
    if (a.sizes)
        for (uint32_t c = blockIdx.x * 256u + tid; c < K; c += gridDim.x * 256u) a.sizes[c] = arow_off[c + 1u] - arow_off[c];
    double* __restrict__ row = a.rowbuf + (uint64_t)blockIdx.x * K;
    const uint64_t jobs = (uint64_t)q + (a.matrix ? K : 0u);
    for (uint64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
        const bool is_matrix = job >= (uint64_t)q;
        uint32_t ga = is_matrix ? (uint32_t)(job - q) : (a.queries ? a.queries[job] : (uint32_t)job);
        bool bad = false;
        if (ga >= K) {  // (a query only)
            if (tid == 0) atomicOr(a.flags + 1, CH_ERR_QUERY);
            bad = true;
            ga = 0;
        }
        const bool a_live = !bad && arow_off[ga + 1u] != arow_off[ga];
        __syncthreads();  // the previous job's rounds have finished with the row buffer
        for (uint32_t c = tid; c < K; c += 256u) {
            const bool live = a_live && c != ga && arow_off[c + 1u] != arow_off[c];
            double v = INFINITY;
            if (live) {
                v = a.D[(uint64_t)ga * K + c];
                if (symmetric) v = (v + a.D[(uint64_t)c * K + ga]) * 0.5;
            }
            if (is_matrix) a.matrix[(uint64_t)ga * K + c] = c == ga ? 0.0 : v;
            else row[c] = live ? v : NAN;  // (NaN: not a candidate; a live value is >= 0 or +inf, or the call fails)
        }
        if (is_matrix) continue;
        __syncthreads();
        unsigned long long last_b = 0ull;
        uint32_t last_c = 0u;
        uint32_t r = 0;
        for (; r < t; r++) {
            unsigned long long kb = ~0ull;
            uint32_t kc = CH_NONE;
            for (uint32_t c = tid; c < K; c += 256u) {
                const double v = row[c];
                if (v != v) continue;
                const unsigned long long vb = (unsigned long long)__double_as_longlong(v);  // v >= +0: the bits order as integers
                if (r && (vb < last_b || (vb == last_b && c <= last_c))) continue;
                ch_take(kb, kc, vb, c);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) ch_take(kb, kc, __shfl_xor(kb, off, WAVE), __shfl_xor(kc, off, WAVE));
            if (lane == 0) {
                s_kb[wave] = kb;
                s_kc[wave] = kc;
            }
            __syncthreads();
            kb = s_kb[0];
            kc = s_kc[0];
#pragma unroll
            for (int w = 1; w < 4; w++) ch_take(kb, kc, s_kb[w], s_kc[w]);
            __syncthreads();  // (the next round writes s_kb again)
            if (kc == CH_NONE) break;
            if (tid == 0) {
                a.idx[job * t + r] = kc;
                a.dist[job * t + r] = __longlong_as_double((long long)kb);
            }
            last_b = kb;
            last_c = kc;
        }
        for (uint32_t e = r + tid; e < t; e += 256u) {  // fewer than t candidates: the k-nearest padding
            a.idx[job * t + e] = CH_NONE;
            a.dist[job * t + e] = INFINITY;
        }
    }
}

ChamferPlan chamfer_plan(uint64_t n, uint32_t K, uint64_t q, bool want_matrix, int n_cus, uint32_t slab_groups, uint64_t ws_limit,
                         uint64_t fixed_bytes) {
    ChamferPlan p{};
    const ScanFill f = scan_fill((n + CH_SONGS_PER_WAVE - 1) / CH_SONGS_PER_WAVE, n_cus);  // pieces of 256 positions
    p.waves = f.waves;
    p.grid = std::max<uint32_t>(1u, f.grid);
    const uint64_t jobs = q + (want_matrix ? K : 0);
    p.select_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::max<uint64_t>(jobs, (n + 255) / 256), 4ull * f.cus));
    // the slab: what CHAMFER_SLAB_BYTES of minima hold, within the workspace limit; a forced slab must fit the limit as it is
    const uint64_t base = fixed_bytes + (uint64_t)K * K * 8 + (uint64_t)p.select_grid * K * 8;
    const uint64_t per_group = std::max<uint64_t>(n, 1) * 4;
    uint64_t slab = slab_groups ? slab_groups : std::max<uint64_t>(1, CHAMFER_SLAB_BYTES / per_group);
    slab = std::min<uint64_t>(slab, K);
    if (!slab_groups && base < ws_limit) slab = std::max<uint64_t>(1, std::min<uint64_t>(slab, (ws_limit - base) / per_group));
    p.slab = (uint32_t)slab;
    p.bytes = base + slab * per_group;
    p.fits = p.bytes <= ws_limit;
    return p;
}

// column groups of one slab's scan: what fills the device, at most one per group of the slab
static uint32_t chamfer_col_groups(const ChamferPlan& p, uint32_t groups, int n_cus) {
    const uint64_t Y = fill_col_groups(cus_or_default(n_cus), (uint64_t)p.grid * p.waves);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(Y, groups));
}

void launch_chamfer_scan(ChamferArgs a, int m_is_diag, const ChamferPlan& p, int n_cus, hipStream_t st) {
    if (a.n == 0 || a.s1 <= a.s0) return;
    a.Y = chamfer_col_groups(p, a.s1 - a.s0, n_cus);
    const dim3 grid(p.grid, a.Y), block(64u * p.waves);
    for_metric_form<false>(a.d, a.metric, m_is_diag, [&](auto D, auto M, auto G) {
        hipLaunchKernelGGL((chamfer_scan_kernel<D(), M(), G()>), grid, block, 0, st, a);
    });
}

void launch_chamfer_reduce(const ChamferArgs& a, hipStream_t st) {
    if (a.n == 0 || a.s1 <= a.s0) return;
    const uint32_t gy = std::max<uint32_t>(1u, std::min<uint32_t>((a.s1 - a.s0 + 3u) / 4u, 64u));
    hipLaunchKernelGGL(chamfer_reduce_kernel, dim3(a.K, gy), dim3(256), 0, st, a);
}

void launch_chamfer_select(const ChamferArgs& a, const ChamferPlan& p, hipStream_t st) {
    hipLaunchKernelGGL(chamfer_select_kernel, dim3(p.select_grid), dim3(256), 0, st, a);
}

}  // namespace bg
