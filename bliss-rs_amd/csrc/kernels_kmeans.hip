// kernels_kmeans.hip -- Lloyd's k-means over a song library, iterated on the device (compiled with -ffp-contract=off).
//
// One iteration is: the nearest centre of every song, a stable counting sort of the labels into per-cluster row lists, the
// sequential f32 mean of every list (segment_mean_kernel of kernels_albums.hip, unchanged) and a select that keeps the old
// centre of a cluster without members.  Nothing is left to the order in which work arrives: the distances are those of the
// all-pairs kernel bit for bit (pair_sum of pairwise_math.hpp / pl_distance, the correctly rounded square root), equal rounded
// distances go to the lower centre, and the row lists hold ascending song indices whatever the split of the sort.
//
//   kmeans_assign_kernel  lanes own songs, the centres are what is broadcast: a lane keeps four songs in registers as two packed
//                         column pairs (the all-pairs kernel's `bp`), a wavefront 256 songs, and every wavefront of the workgroup
//                         walks the same tile of centres, staged in LDS in ascending index and read as ds_read_b128 broadcasts
//                         (the all-pairs kernel's row `ap`).  K is not bounded by the tile: tiles follow one another.  A song
//                         keeps its running best in registers -- the sum, its rounded root and the index.  The rounded square
//                         root is monotone, so a sum that is not BELOW the best's own sum cannot give a strictly smaller distance
//                         and is rejected without a root (this is tighter than the k-nearest searches' bound, which has to work
//                         from a threshold whose sum is not known: a sum above nextup(fl(u u)) is always also above the best's
//                         sum).  Survivors -- a NaN sum is one, the test is written `!(s >= best)` -- take sqrtf and the strict
//                         comparison; with centres in ascending order a tie keeps the lower index.  No per-song buffer, no key
//                         sort, no cross-lane reduction, no atomics on data: only the counts `changed` and the NaN word.
//   kmeans_hist_kernel    the sort, part 1: the songs are dealt out in W contiguous chunks, one wavefront each; hist[c][w] counts
//                         chunk w's songs with label c (zeroed by the caller; integer adds, their order does not matter).
//   kmeans_scan_*         part 2: ONE exclusive scan over hist in (cluster, chunk) order, in place: hist[c][w] becomes the slot
//                         of the first song of chunk w in cluster c's list, and hist[c][0] the list's start -> arow_off[c].
//   kmeans_scatter_kernel part 3: a wavefront walks its chunk in order, 64 songs at a time: slot = the chunk's running position
//                         of the label + the number of lower lanes with the same label.  arow is fully determined by the labels.
//   kmeans_select_kernel  centres of clusters without rows (segment_mean_kernel wrote NaN rows there) keep the old centre's bits.
#include <math.h>

#include <algorithm>

#include "device_utils.hpp"
#include "internal.hpp"
#include "pairwise_math.hpp"
#include "playlist_math.hpp"
#include "scan_block.hpp"

namespace bg {

constexpr int KM_TILE_FLOATS = 6144;  // 24 KiB of centres per tile: 256 rows at d = 23 (pitch 24)
constexpr int KM_TILE_ROWS = 256;     // at most this many centres per tile
constexpr int KM_SONGS_PER_WAVE = 256;

// D > 0: compile-time feature count (packed arithmetic, songs in registers).  D == 0: any d <= 64 through pl_distance, songs read
// from global memory / L2 (slow, exact).  blockDim.x = 64 * (wavefronts per workgroup): 1 .. 4.
template <int D, int METRIC, bool DIAG>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const float* __restrict__ X, uint32_t n, const float* __restrict__ Cn,
                                                            uint32_t K, uint32_t d_rt, int metric_rt, const float* __restrict__ M,
                                                            uint32_t* __restrict__ labels, float* __restrict__ dist,
                                                            uint32_t* changed, uint32_t* nan_flag) {
    constexpr bool GENERIC = D == 0;
    constexpr int DD = GENERIC ? 1 : D;
    constexpr int DQ = GENERIC ? 1 : ((D + 3) & ~3);  // LDS pitch of a centre: 16-byte aligned -> ds_read_b128 broadcasts
    __shared__ __attribute__((aligned(16))) float s_c[KM_TILE_FLOATS];
    __shared__ float s_m[(!GENERIC && METRIC == METRIC_MAHALANOBIS) ? D * D : 1];

    const uint32_t tid = threadIdx.x, nthr = blockDim.x, lane = (uint32_t)lane_id(), wave = (uint32_t)wave_id();
    const uint32_t d = GENERIC ? d_rt : (uint32_t)D;
    const uint32_t pitch = GENERIC ? d : (uint32_t)DQ;
    const uint32_t tile_rows = std::min<uint32_t>((uint32_t)KM_TILE_ROWS, (uint32_t)KM_TILE_FLOATS / pitch);
    // the wavefront's 256 songs: song c of the lane is row j0 + 64 c + lane (64-bit: n may be close to 2^32)
    const uint64_t j0 = ((uint64_t)blockIdx.x * (nthr / 64u) + wave) * (uint64_t)KM_SONGS_PER_WAVE;

    if (!GENERIC && METRIC == METRIC_MAHALANOBIS) {
        for (uint32_t e = tid; e < (uint32_t)(DD * DD); e += nthr) s_m[e] = M[e];
        __syncthreads();
    }
    float wdiag[DD];
    if constexpr (!GENERIC) {
#pragma unroll
        for (int kk = 0; kk < D; kk++)  // (the same in every lane: scalar registers)
            wdiag[kk] = DIAG ? __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s_m[(kk * D + kk) % (METRIC == METRIC_MAHALANOBIS ? D * D : 1)]))) : 0.0f;
    }

    // the lane's four songs as two packed pairs: bp[h][kk] = (song 2h, song 2h + 1); rows past n are zeros (results dropped)
    f2 bp[2][DD];
    bool valid[4];
#pragma unroll
    for (int c = 0; c < 4; c++) valid[c] = j0 + 64u * (uint32_t)c + lane < (uint64_t)n;
    if constexpr (!GENERIC) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const float* xa = X + (j0 + 64u * (uint32_t)(2 * h) + lane) * (uint64_t)D;
            const float* xb = xa + 64u * (uint32_t)D;
#pragma unroll
            for (int kk = 0; kk < D; kk++) {
                bp[h][kk].x = valid[2 * h] ? xa[kk] : 0.0f;
                bp[h][kk].y = valid[2 * h + 1] ? xb[kk] : 0.0f;
            }
        }
    }

    float best_s[4], best_d[4];  // the best centre's sum (GENERIC: unused), its distance
    uint32_t best_i[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        best_s[c] = INFINITY;
        best_d[c] = INFINITY;
        best_i[c] = 0u;
    }
    bool saw_nan = false;

    for (uint32_t c0 = 0; c0 < K; c0 += tile_rows) {
        const uint32_t rows_here = std::min<uint32_t>(tile_rows, K - c0);
        if (c0) __syncthreads();  // every wavefront has finished with the previous tile
        {
            const float* src = Cn + (uint64_t)c0 * d;
            const uint32_t floats = rows_here * d;
            if (pitch == d) {
                for (uint32_t e = tid; e < floats; e += nthr) s_c[e] = src[e];
            } else {
                for (uint32_t e = tid; e < floats; e += nthr) s_c[(e / d) * pitch + e % d] = src[e];
                // the padding of a row travels into registers with it (never into a result): defined values
                for (uint32_t e = tid; e < rows_here * (pitch - d); e += nthr) s_c[(e / (pitch - d)) * pitch + d + e % (pitch - d)] = 0.0f;
            }
        }
        __syncthreads();
#pragma unroll 1
        for (uint32_t r = 0; r < rows_here; r++) {
            const uint32_t ci = c0 + r;
            if constexpr (GENERIC) {
#pragma unroll 1
                for (int c = 0; c < 4; c++) {
                    if (!valid[c]) continue;
                    const float v = pl_distance(X + (j0 + 64u * (uint32_t)c + lane) * (uint64_t)d, s_c + r * pitch, d, metric_rt, M);
                    if (v != v) saw_nan = true;
                    if (ci == 0u || v < best_d[c]) {
                        best_d[c] = v;
                        best_i[c] = ci;
                    }
                }
            } else {
                f2 ap[DQ / 2];
                scan_query_row<DQ>(&s_c[r * (uint32_t)DQ], ap);
                f2 s0 = pair_sum<DD, METRIC, DIAG>(ap, bp[0], wdiag, s_m);
                // (general M: one pair's 2 x d differences and products at a time, as in the k-nearest scan)
                if (METRIC == METRIC_MAHALANOBIS && !DIAG) asm volatile("" : "+v"(s0));
                const f2 s1 = pair_sum<DD, METRIC, DIAG>(ap, bp[1], wdiag, s_m);
                const float pv[4] = {s0.x, s0.y, s1.x, s1.y};
                // the first centre is taken whatever its distance (the argmin of a row of +inf is index 0)
                const bool maybe = ci == 0u || !(pv[0] >= best_s[0]) || !(pv[1] >= best_s[1]) || !(pv[2] >= best_s[2]) || !(pv[3] >= best_s[3]);
                if (maybe) {
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        if (ci == 0u || !(pv[c] >= best_s[c])) {
                            const float v = sqrtf(pv[c]);
                            if (v != v && valid[c]) saw_nan = true;
                            if (ci == 0u || v < best_d[c]) {
                                best_s[c] = pv[c];
                                best_d[c] = v;
                                best_i[c] = ci;
                            }
                        }
                    }
                }
            }
        }
    }

    uint32_t n_changed = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint64_t j = j0 + 64u * (uint32_t)c + lane;
        bool ch = false;
        if (valid[c]) {
            ch = labels[j] != best_i[c];
            labels[j] = best_i[c];
            if (dist) dist[j] = best_d[c];
        }
        n_changed += (uint32_t)__popcll(__ballot(ch));
    }
    if (lane == 0 && n_changed) atomicAdd(changed, n_changed);
    if (saw_nan) atomicOr(nan_flag, 1u);
}

// LDS / global traffic between the lanes of ONE wavefront: keep the compiler from moving loads and stores across the hand-over
__device__ __forceinline__ void km_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// chunk w = songs [w * chunk, min(n, (w + 1) * chunk)), one wavefront; hist is [K][W]
__global__ __launch_bounds__(256) void kmeans_hist_kernel(const uint32_t* __restrict__ labels, uint32_t n, uint32_t K, uint32_t W,
                                                          uint32_t chunk, uint32_t* __restrict__ hist) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t w = blockIdx.x * 4u + (uint32_t)wave_id();
    if (w >= W) return;
    const uint64_t lo = (uint64_t)w * chunk, hi = std::min<uint64_t>(n, lo + chunk);
    for (uint64_t i = lo + lane; i < hi; i += 64u) {
        const uint32_t l = labels[i];
        if (l < K) atomicAdd(&hist[(uint64_t)l * W + w], 1u);
    }
}

// exclusive scan of a[0 .. len) in tiles of 2048 (256 threads x 8 consecutive elements), in place; bsum[tile] = the tile's total
constexpr uint32_t KM_SCAN_TILE = 2048;
__global__ __launch_bounds__(256) void kmeans_scan_tiles_kernel(uint32_t* __restrict__ a, uint32_t len, uint32_t* __restrict__ bsum) {
    __shared__ uint32_t s_wave[4];
    const uint32_t tid = threadIdx.x, lane = (uint32_t)lane_id(), wave = (uint32_t)wave_id();
    const uint64_t base = (uint64_t)blockIdx.x * KM_SCAN_TILE + (uint64_t)tid * 8u;
    uint32_t v[8], sum = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        v[i] = (base + (uint32_t)i < len) ? a[base + (uint32_t)i] : 0u;
        sum += v[i];
    }
    // inclusive scan of the threads' sums across the wavefront, then across the four wavefronts
    uint32_t inc = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(inc, off, 64);
        if (lane >= (uint32_t)off) inc += up;
    }
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = inc - sum;
    for (uint32_t u = 0; u < wave; u++) before += s_wave[u];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (base + (uint32_t)i < len) a[base + (uint32_t)i] = before;
        before += v[i];
    }
    if (tid == 255u) bsum[blockIdx.x] = before;
}

// adds the totals of the tiles before its own to every element of a tile; then hist[c][0] is where cluster c's list starts
__global__ __launch_bounds__(256) void kmeans_scan_add_kernel(uint32_t* __restrict__ a, uint32_t len, const uint32_t* __restrict__ bsum,
                                                              uint32_t W, uint32_t K, uint32_t n, uint32_t* __restrict__ arow_off) {
    __shared__ uint32_t s_part[256];
    const uint32_t tid = threadIdx.x;
    uint32_t part = 0;
    for (uint32_t b = tid; b < blockIdx.x; b += 256u) part += bsum[b];
    s_part[tid] = part;
    __syncthreads();
    for (uint32_t s = 128u; s > 0u; s >>= 1) {
        if (tid < s) s_part[tid] += s_part[tid + s];
        __syncthreads();
    }
    const uint32_t off = s_part[0];
    const uint64_t base = (uint64_t)blockIdx.x * KM_SCAN_TILE + (uint64_t)tid * 8u;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t e = base + (uint32_t)i;
        if (e < len) {
            const uint32_t v = a[e] + off;
            a[e] = v;
            if (e % W == 0u) arow_off[e / W] = v;
        }
    }
    if (blockIdx.x == 0 && tid == 0) arow_off[K] = n;
}

// pos = the scanned hist: pos[c][w] is the next free slot of cluster c's list for chunk w, advanced as the chunk is walked
__global__ __launch_bounds__(256) void kmeans_scatter_kernel(const uint32_t* __restrict__ labels, uint32_t n, uint32_t K, uint32_t W,
                                                             uint32_t chunk, uint32_t* pos, uint32_t* __restrict__ arow) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t w = blockIdx.x * 4u + (uint32_t)wave_id();
    if (w >= W) return;
    const uint64_t lo = (uint64_t)w * chunk, hi = std::min<uint64_t>(n, lo + chunk);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint64_t i0 = lo; i0 < hi; i0 += 64u) {
        const uint64_t i = i0 + lane;
        const bool live = i < hi;
        const uint32_t l = live ? labels[i] : 0xFFFFFFFFu;
        const bool ok = live && l < K;
        uint32_t* slot = pos + ((uint64_t)(ok ? l : 0u) * W + w);
        const uint32_t first = ok ? *slot : 0u;
        // rank among the lanes with the same label, and their number: one pass per distinct label of the 64
        uint32_t rank = 0, cnt = 0;
        unsigned long long todo = __ballot(ok);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const uint32_t ll = (uint32_t)__builtin_amdgcn_readlane((int)l, leader);
            const unsigned long long same = __ballot(ok && l == ll);
            if (ok && l == ll) {
                rank = (uint32_t)__popcll(same & below);
                cnt = (uint32_t)__popcll(same);
            }
            todo &= ~same;
        }
        if (ok) {
            arow[first + rank] = (uint32_t)i;
            if (rank + 1u == cnt) *slot = first + cnt;
        }
        km_wave_sync();  // the next 64 songs read the positions written here (other lanes of the same wavefront)
    }
}

// next[c] = prev[c] where cluster c has no rows; sizes (may be NULL) = the lists' lengths
__global__ __launch_bounds__(256) void kmeans_select_kernel(const float* __restrict__ prev, float* __restrict__ next,
                                                            const uint32_t* __restrict__ arow_off, uint32_t K, uint32_t d,
                                                            uint32_t* __restrict__ sizes) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= (uint64_t)K * d) return;
    const uint32_t c = (uint32_t)(e / d);
    const uint32_t cnt = arow_off[c + 1] - arow_off[c];
    if (next && cnt == 0u) next[e] = prev[e];
    if (sizes && e % d == 0u) sizes[c] = cnt;
}

KmeansPlan kmeans_plan(uint64_t n, uint32_t K, int n_cus) {
    KmeansPlan p{};
    // assignment: four wavefronts share a tile of centres when there are enough songs to give every CU two such workgroups;
    // a smaller library runs one wavefront per workgroup so that its 256-song pieces spread over the CUs
    const ScanFill f = scan_fill((n + KM_SONGS_PER_WAVE - 1) / KM_SONGS_PER_WAVE, n_cus);
    p.assign_waves = f.waves;
    p.assign_grid = f.grid;
    // the sort: chunks of at least 256 songs, as many as keep the histogram table K x W within 2^21 words
    uint64_t W = std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (1ull << 21) / std::max<uint32_t>(K, 1u)));
    W = std::min<uint64_t>(W, 1u << 20);
    uint64_t chunk = std::max<uint64_t>(1, (n + W - 1) / W);
    chunk = (chunk + 63) / 64 * 64;
    W = std::max<uint64_t>(1, (n + chunk - 1) / chunk);
    p.W = (uint32_t)W;
    p.chunk = (uint32_t)std::min<uint64_t>(chunk, 0xFFFFFFC0ull);
    p.hist_words = (uint64_t)K * W;
    p.scan_tiles = (uint32_t)((p.hist_words + KM_SCAN_TILE - 1) / KM_SCAN_TILE);
    return p;
}

void launch_kmeans_assign(const float* X, uint32_t n, const float* C, uint32_t K, uint32_t d, int metric, const float* M,
                          int m_is_diag, const KmeansPlan& p, uint32_t* labels, float* dist, uint32_t* changed, uint32_t* nan_flag,
                          hipStream_t st) {
    if (n == 0) return;
    const dim3 grid(p.assign_grid), block(64u * p.assign_waves);
    for_metric_form<false>(d, metric, m_is_diag, [&](auto D, auto M_, auto G) {
        hipLaunchKernelGGL((kmeans_assign_kernel<D(), M_(), G()>), grid, block, 0, st, X, n, C, K, d, metric, M, labels, dist, changed,
                           nan_flag);
    });
}

void launch_kmeans_hist(const uint32_t* labels, uint32_t n, uint32_t K, const KmeansPlan& p, uint32_t* hist, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(kmeans_hist_kernel, dim3((p.W + 3u) / 4u), dim3(256), 0, st, labels, n, K, p.W, p.chunk, hist);
}

void launch_kmeans_scan_tiles(uint32_t* hist, const KmeansPlan& p, uint32_t* bsum, hipStream_t st) {
    hipLaunchKernelGGL(kmeans_scan_tiles_kernel, dim3(p.scan_tiles), dim3(256), 0, st, hist, (uint32_t)p.hist_words, bsum);
}

void launch_kmeans_scan_add(uint32_t* hist, uint32_t n, uint32_t K, const KmeansPlan& p, const uint32_t* bsum, uint32_t* arow_off,
                            hipStream_t st) {
    hipLaunchKernelGGL(kmeans_scan_add_kernel, dim3(p.scan_tiles), dim3(256), 0, st, hist, (uint32_t)p.hist_words, bsum, p.W, K, n,
                       arow_off);
}

void launch_kmeans_scatter(const uint32_t* labels, uint32_t n, uint32_t K, const KmeansPlan& p, uint32_t* pos, uint32_t* arow,
                           hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(kmeans_scatter_kernel, dim3((p.W + 3u) / 4u), dim3(256), 0, st, labels, n, K, p.W, p.chunk, pos, arow);
}

void launch_kmeans_select(const float* prev, float* next, const uint32_t* arow_off, uint32_t K, uint32_t d, uint32_t* sizes,
                          hipStream_t st) {
    const uint64_t e = (uint64_t)K * d;
    hipLaunchKernelGGL(kmeans_select_kernel, dim3((uint32_t)((e + 255) / 256)), dim3(256), 0, st, prev, next, arow_off, K, d, sizes);
}

}  // namespace bg
