// kernels_pam.hip -- k-medoids (PAM) of a song library: every (candidate song, song) pair per scan and nothing stored (compiled
// with -ffp-contract=off).
//
// The state of a clustering is, per song o, its nearest medoid slot near[o] and the distances d1[o] <= d2[o] to the nearest and
// the second nearest medoid.  One scan answers, for every candidate c and slot m, what the total distance TD would change by
//   A(c, m) = 0.0 + sum over near[o] == m, ascending o, of ((double)fminf(doc, d2[o]) - (double)d1[o])      m leaves, c joins
//   B(c, m) = 0.0 + sum over near[o] == m, ascending o, of fmin((double)doc - (double)d1[o], 0.0)           m stays, c joins
// with doc = dist(c, o), the all-pairs kernel's distance bit for bit (pair_sum of pairwise_math.hpp / pl_distance, the correctly
// rounded square root, IEEE division for the cosine).  include/blissgpu.h has the contract.  Nothing is left to the order in which
// work arrives: a sum is formed by ONE lane in the contract's order, minima are taken in ascending order with a strict <, and
// every value reaches memory with a plain store.
//
// The state's slots are sorted first with the k-means kernels as they are (kmeans_hist / scan_tiles / scan_add / scatter of
// kernels_kmeans.hip): slot m's songs are arow[arow_off[m] .. arow_off[m + 1]) in ascending index.
//
//   pam_scan_kernel    silhouette_scan_kernel's shape: a lane keeps four CANDIDATES in registers as two packed column pairs, a
//                      wavefront 256, and every wavefront of the workgroup walks the library in slot order, staged through arow
//                      into LDS tiles of up to 256 rows; a tile row is read as ds_read_b128 broadcasts together with its (d1, d2,
//                      norm) record.  Per row: pair_sum, the root (or the cosine's division), and two f64 chains per candidate.
//                      Where a slot ends -- uniform across the workgroup: read from arow_off, a scalar branch, runs of empty slots
//                      skipped -- the lane stores A and B of (candidate, slot).  The slots are dealt to Y column groups, slot m to
//                      group floor(arow_off[m] Y / n): a slot is never split, so no sum depends on Y, and every (candidate, slot)
//                      is written by exactly one work item.  fminf and fmin drop a NaN operand, so the sums cannot show a NaN
//                      distance: every doc is compared with itself instead.
//   pam_fold_kernel    a lane per candidate: btot in ascending m, then delta(c, m) = (btot - B) + A, its minimum and the slot.
//   pam_pick_kernel    one workgroup: the smallest (value, song) of a slab of candidates, medoids left out, merged into the
//                      round's record.  Integer and f64 comparisons only, no atomics.
//   pam_gather_kernel  the medoids' rows for the k-nearest search that makes the state (a swap, when there is one, is applied
//                      here), pam_state_kernel unpacks that search's two columns, pam_td_kernel is the one sequential f64 sum.
#include <math.h>

#include <algorithm>

#include "device_utils.hpp"
#include "internal.hpp"
#include "pairwise_math.hpp"
#include "playlist_math.hpp"
#include "scan_block.hpp"

namespace bg {

constexpr int PAM_TILE_FLOATS = 6144;  // 24 KiB of library rows per tile: 256 rows at d = 23 (pitch 24)
constexpr int PAM_TILE_ROWS = 256;     // at most this many rows per tile
constexpr int PAM_SONGS_PER_WAVE = 256;

__device__ __forceinline__ uint32_t pam_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the first slot m in [0, K] with arow_off[m] >= t (arow_off[0] = 0, arow_off[K] = n >= t)
__device__ __forceinline__ uint32_t pam_first_slot(const uint32_t* __restrict__ arow_off, uint32_t K, uint64_t t) {
    return t ? find_segment(arow_off, K + 1u, (uint32_t)(t - 1u)) + 1u : 0u;
}

// D > 0: compile-time feature count (packed arithmetic, candidates in registers).  D == 0: any d <= 64 through pl_distance,
// candidates read from global memory / L2 (slow, exact).  blockDim.x = 64 * (wavefronts per workgroup): 1 .. 4.
template <int D, int METRIC, bool DIAG>
__global__ __launch_bounds__(256) void pam_scan_kernel(const PamArgs a) {
    constexpr bool GENERIC = D == 0;
    constexpr int DD = GENERIC ? 1 : D;
    constexpr int DQ = GENERIC ? 1 : ((D + 3) & ~3);  // LDS pitch of a row: 16-byte aligned -> ds_read_b128 broadcasts
    __shared__ __attribute__((aligned(16))) float s_c[PAM_TILE_FLOATS];
    __shared__ __attribute__((aligned(16))) float4 s_e[PAM_TILE_ROWS];  // per tile row: d1, d2, the row's norm (cosine), unused
    __shared__ float s_m[(!GENERIC && METRIC == METRIC_MAHALANOBIS) ? D * D : 1];

    const float* __restrict__ X = a.X;
    const uint32_t* __restrict__ arow_off = a.arow_off;
    const uint32_t* __restrict__ arow = a.arow;
    const uint32_t n = a.n, K = a.K, q = a.q, Y = a.Y;
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, lane = (uint32_t)lane_id(), wave = (uint32_t)wave_id();
    const uint32_t d = GENERIC ? a.d : (uint32_t)D;
    const uint32_t pitch = GENERIC ? d : (uint32_t)DQ;
    const uint32_t tile_rows = std::min<uint32_t>((uint32_t)PAM_TILE_ROWS, (uint32_t)PAM_TILE_FLOATS / pitch);
    const uint32_t g = blockIdx.y;
    // the wavefront's 256 positions of the slab: slot c of the lane is position p0 + 64 c + lane
    const uint64_t p0 = ((uint64_t)blockIdx.x * (nthr / 64u) + wave) * (uint64_t)PAM_SONGS_PER_WAVE;

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

    // the lane's four candidates; a position past q or a rows entry past n (the entry point refuses those) evaluates nothing
    bool valid[4];
    uint32_t song[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint64_t p = p0 + 64u * (uint32_t)c + lane;
        valid[c] = p < (uint64_t)q;
        song[c] = valid[c] ? (a.rows ? a.rows[p] : a.row0 + (uint32_t)p) : 0u;
        if (song[c] >= n) {
            valid[c] = false;
            song[c] = 0u;
        }
    }
    // ... as two packed pairs: bp[h][kk] = (candidate 2h, candidate 2h + 1); the rows of slots that evaluate nothing are zeros
    f2 bp[2][DD];
    f2 nb[2];
    nb[0] = nb[1] = splat(0.0f);
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
            if (METRIC == METRIC_COSINE) {  // the candidates' norms, as knn_scan_kernel forms them
                const f2 qq = unrolled_dot2<DD>([&](int kk) { return bp[h][kk]; }, [&](int kk) { return bp[h][kk]; });
                nb[h].x = sqrtf(qq.x);
                nb[h].y = sqrtf(qq.y);
            }
        }
    }

    // the group's run of slots [c_lo, c_hi) = those with floor(arow_off[m] Y / n) == g, and its rows of the sorted order
    const uint32_t c_lo = pam_uniform(pam_first_slot(arow_off, K, ((uint64_t)g * n + Y - 1u) / Y));
    const uint32_t c_hi = pam_uniform(pam_first_slot(arow_off, K, ((uint64_t)(g + 1u) * n + Y - 1u) / Y));
    const uint32_t r_lo = pam_uniform(arow_off[c_lo]), r_hi = pam_uniform(arow_off[c_hi]);

    double acc_a[4], acc_b[4];
#pragma unroll
    for (int c = 0; c < 4; c++) acc_a[c] = acc_b[c] = 0.0;
    bool saw_nan = false;

    // cl = the slot the walk is in, rows [start, end) of the sorted order; runs of empty slots are stepped over
    uint32_t cl = c_lo, start = r_lo, end = r_lo;
    while (cl < c_hi && (end = pam_uniform(arow_off[cl + 1u])) == start) cl++;

    for (uint32_t t0 = r_lo; t0 < r_hi; t0 += tile_rows) {
        const uint32_t rows_here = std::min<uint32_t>(tile_rows, r_hi - t0);
        if (t0 != r_lo) __syncthreads();  // every wavefront has finished with the previous tile
        {
            // row r of the tile = row arow[t0 + r] of X; the padding of a row travels into registers with it (never into a
            // result): zeros
            const uint32_t floats = rows_here * pitch;
#pragma unroll 4
            for (uint32_t e = tid; e < floats; e += nthr) {
                const uint32_t r = e / pitch, kk = e - r * pitch;
                const uint32_t j = arow[t0 + r];
                s_c[e] = (kk < d && j < n) ? X[(uint64_t)j * d + kk] : 0.0f;
            }
            for (uint32_t r = tid; r < rows_here; r += nthr) {
                const uint32_t j = arow[t0 + r];
                s_e[r] = j < n ? make_float4(a.d1[j], a.d2[j], 0.0f, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
        __syncthreads();
        if (!GENERIC && METRIC == METRIC_COSINE) {  // the rows' norms, as knn_scan_kernel forms its queries'
            for (uint32_t r = tid; r < rows_here; r += nthr) {
                const float* row = &s_c[r * (uint32_t)DQ];
                s_e[r].z = sqrtf(unrolled_dot<DD>([&](int kk) { return row[kk]; }, [&](int kk) { return row[kk]; }));
            }
            __syncthreads();
        }
        uint32_t r = 0;
        while (r < rows_here) {
            const uint32_t seg = std::min<uint32_t>(rows_here, end - t0);  // (end > t0 + r: the walk is inside slot cl)
#pragma unroll 1
            for (; r < seg; r++) {
                const float4 e = s_e[r];  // the same address in every lane: an LDS broadcast
                const double d1d = (double)e.x;
                float doc[4];
                if constexpr (GENERIC) {
#pragma unroll 1
                    for (int c = 0; c < 4; c++)
                        doc[c] = valid[c] ? pl_distance(X + (uint64_t)song[c] * d, s_c + r * pitch, d, a.metric, a.M) : 0.0f;
                } else {
                    f2 ap[DQ / 2];
                    scan_query_row<DQ>(&s_c[r * (uint32_t)DQ], ap);
                    float pv[4];
                    scan_pair_values<DD, METRIC, DIAG>(ap, bp, nb, e.z, wdiag, s_m, pv);
#pragma unroll
                    for (int c = 0; c < 4; c++) doc[c] = METRIC == METRIC_COSINE ? pv[c] : sqrtf(pv[c]);
                }
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    if (doc[c] != doc[c] && valid[c]) saw_nan = true;
                    acc_a[c] = acc_a[c] + ((double)fminf(doc[c], e.y) - d1d);
                    acc_b[c] = acc_b[c] + fmin((double)doc[c] - d1d, 0.0);
                }
            }
            if (t0 + r == end) {  // slot cl ends here (uniform): its two sums go to memory
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    if (valid[c]) {
                        const uint64_t at = (p0 + 64u * (uint32_t)c + lane) * (uint64_t)K + cl;
                        a.ws_a[at] = acc_a[c];
                        a.ws_b[at] = acc_b[c];
                    }
                    acc_a[c] = acc_b[c] = 0.0;
                }
                cl++;
                start = end;
                while (cl < c_hi && (end = pam_uniform(arow_off[cl + 1u])) == start) cl++;
            }
        }
    }
    if (saw_nan) atomicOr(a.flags, 1u);
}

// thread t: position t (< q) of the slab.  An empty slot has A = B = 0.0 (written here: the scan stores nothing for it)
__global__ __launch_bounds__(256) void pam_fold_kernel(const PamArgs a) {
    const uint32_t* __restrict__ arow_off = a.arow_off;
    const uint32_t K = a.K;
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint64_t)a.q) return;
    double* __restrict__ wa = a.ws_a + t * (uint64_t)K;
    double* __restrict__ wb = a.ws_b + t * (uint64_t)K;
    double btot = 0.0;
    for (uint32_t m = 0; m < K; m++) {
        if (arow_off[m + 1u] == arow_off[m]) {
            wa[m] = 0.0;
            wb[m] = 0.0;
        }
        btot = btot + wb[m];
    }
    double best = 0.0;
    uint32_t arg = 0u;
    for (uint32_t m = 0; m < K; m++) {
        const double delta = (btot - wb[m]) + wa[m];
        if (m == 0u || delta < best) {  // ascending slots: a tie keeps the lower one
            best = delta;
            arg = m;
        }
    }
    a.btot[t] = btot;
    a.best[t] = best;
    a.arg[t] = arg;
}

// one workgroup: the smallest (val[p * stride], song of p) over the slab's positions p < q whose song is no medoid (ismed NULL:
// every song), compared as f64 (so -0.0 == +0.0), equal values to the lower song; a NaN value is never taken.  fresh: the record
// holds nothing yet; otherwise the slab's winner is merged into it
__global__ __launch_bounds__(256) void pam_pick_kernel(const double* __restrict__ val, uint32_t stride, const uint32_t* __restrict__ arg,
                                                       const uint32_t* __restrict__ rows, uint32_t row0, uint32_t q,
                                                       const uint32_t* __restrict__ ismed, int fresh, PamRecord* rec) {
    __shared__ double s_v[256];
    __shared__ uint32_t s_c[256], s_a[256];
    const uint32_t tid = threadIdx.x;
    double bv = 0.0;
    uint32_t bc = PAM_NONE, ba = 0u;
    for (uint32_t p = tid; p < q; p += 256u) {
        const uint32_t c = rows ? rows[p] : row0 + p;
        if (ismed && ismed[c]) continue;
        const double v = val[(uint64_t)p * stride];
        if (v != v) continue;
        if (bc == PAM_NONE || v < bv || (v == bv && c < bc)) {
            bv = v;
            bc = c;
            ba = arg ? arg[p] : 0u;
        }
    }
    s_v[tid] = bv; s_c[tid] = bc; s_a[tid] = ba;
    __syncthreads();
    for (uint32_t w = 128u; w > 0u; w >>= 1) {
        if (tid < w) {
            const double ov = s_v[tid + w];
            const uint32_t oc = s_c[tid + w];
            if (oc != PAM_NONE && (s_c[tid] == PAM_NONE || ov < s_v[tid] || (ov == s_v[tid] && oc < s_c[tid]))) {
                s_v[tid] = ov; s_c[tid] = oc; s_a[tid] = s_a[tid + w];
            }
        }
        __syncthreads();
    }
    if (tid == 0u) {
        const bool have = !fresh && rec->c != PAM_NONE;
        const double rv = rec->val;
        const uint32_t rc = rec->c;
        if (!have || (s_c[0] != PAM_NONE && (s_v[0] < rv || (s_v[0] == rv && s_c[0] < rc)))) {
            rec->val = s_c[0] != PAM_NONE ? s_v[0] : 0.0;
            rec->c = s_c[0];
            rec->arg = s_a[0];
        }
    }
}

// rows_out [K][d] = X[med[s]] for the search that makes the state.  swap_slot != PAM_NONE: med[swap_slot] becomes swap_c first
// (append: the slot held nothing before).  mark_all: every medoid is marked in ismed (a start given by the caller)
__global__ __launch_bounds__(256) void pam_gather_kernel(const float* __restrict__ X, uint32_t* med, uint32_t K, uint32_t d,
                                                         float* __restrict__ rows_out, uint32_t swap_slot, uint32_t swap_c, int append,
                                                         int mark_all, uint32_t* ismed) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= (uint64_t)K * d) return;
    const uint32_t s = (uint32_t)(e / d), kk = (uint32_t)(e - (uint64_t)s * d);
    const bool swapped = s == swap_slot;
    const uint32_t m = swapped ? swap_c : med[s];  // (only the slot's own kk == 0 thread reads and writes med[swap_slot])
    rows_out[e] = X[(uint64_t)m * d + kk];
    if (kk == 0u) {
        if (swapped) {
            if (!append) ismed[med[s]] = 0u;
            med[s] = m;
        }
        if (swapped || mark_all) ismed[m] = 1u;
    }
}

// idx / dist [n][kk] of the k-nearest search over the medoids' rows (kk = 1 or 2) -> near, d1, d2 (+inf when kk == 1)
__global__ __launch_bounds__(256) void pam_state_kernel(const uint32_t* __restrict__ idx, const float* __restrict__ dist, uint32_t n,
                                                        uint32_t kk, uint32_t* __restrict__ near, float* __restrict__ d1,
                                                        float* __restrict__ d2) {
    const uint64_t o = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (o >= (uint64_t)n) return;
    near[o] = idx[o * kk];
    d1[o] = dist[o * kk];
    d2[o] = kk == 2u ? dist[o * kk + 1u] : INFINITY;
}

// TD = 0.0 + (double)d1[0] + (double)d1[1] + ...: ONE sequential f64 sum, formed by one wavefront whose lanes fetch and convert
// 64 values at a time and all add them in order (a value travels through two scalar registers; the chain is the add alone)
__global__ __launch_bounds__(64) void pam_td_kernel(const float* __restrict__ d1, uint32_t n, PamRecord* rec) {
    const uint32_t lane = threadIdx.x;
    double s = 0.0;
    for (uint32_t base = 0; base < n; base += 64u) {
        const uint32_t cnt = std::min<uint32_t>(64u, n - base);
        const double v = lane < cnt ? (double)d1[base + lane] : 0.0;
        const int lo = __double2loint(v), hi = __double2hiint(v);
        if (cnt == 64u) {
#pragma unroll
            for (int i = 0; i < 64; i++) s = s + __hiloint2double(__builtin_amdgcn_readlane(hi, i), __builtin_amdgcn_readlane(lo, i));
        } else {
            for (uint32_t i = 0; i < cnt; i++) s = s + __hiloint2double(__builtin_amdgcn_readlane(hi, (int)i), __builtin_amdgcn_readlane(lo, (int)i));
        }
    }
    if (lane == 0u) rec->td = s;
}

void launch_pam_scan(const PamArgs& a, int m_is_diag, const SilhouettePlan& p, hipStream_t st) {
    if (a.q == 0 || a.n == 0) return;
    const dim3 grid(p.grid, p.Y), block(64u * p.waves);
    for_metric_form<true>(a.d, a.metric, m_is_diag, [&](auto D, auto M, auto G) {
        hipLaunchKernelGGL((pam_scan_kernel<D(), M(), G()>), grid, block, 0, st, a);
    });
}

void launch_pam_fold(const PamArgs& a, hipStream_t st) {
    if (a.q == 0) return;
    hipLaunchKernelGGL(pam_fold_kernel, dim3((uint32_t)(((uint64_t)a.q + 255u) / 256u)), dim3(256), 0, st, a);
}

void launch_pam_pick(const double* val, uint32_t stride, const uint32_t* arg, const uint32_t* rows, uint32_t row0, uint32_t q,
                     const uint32_t* ismed, bool fresh, PamRecord* rec, hipStream_t st) {
    hipLaunchKernelGGL(pam_pick_kernel, dim3(1), dim3(256), 0, st, val, stride, arg, rows, row0, q, ismed, fresh ? 1 : 0, rec);
}

void launch_pam_gather(const float* X, uint32_t* med, uint32_t K, uint32_t d, float* rows_out, uint32_t swap_slot, uint32_t swap_c,
                       bool append, bool mark_all, uint32_t* ismed, hipStream_t st) {
    const uint64_t threads = (uint64_t)K * d;
    hipLaunchKernelGGL(pam_gather_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st, X, med, K, d, rows_out, swap_slot,
                       swap_c, append ? 1 : 0, mark_all ? 1 : 0, ismed);
}

void launch_pam_state(const uint32_t* idx, const float* dist, uint32_t n, uint32_t kk, uint32_t* near, float* d1, float* d2,
                      hipStream_t st) {
    hipLaunchKernelGGL(pam_state_kernel, dim3((uint32_t)(((uint64_t)n + 255u) / 256u)), dim3(256), 0, st, idx, dist, n, kk, near, d1, d2);
}

void launch_pam_td(const float* d1, uint32_t n, PamRecord* rec, hipStream_t st) {
    hipLaunchKernelGGL(pam_td_kernel, dim3(1), dim3(64), 0, st, d1, n, rec);
}

}  // namespace bg
