// kernels_albums.hip -- the k nearest ALBUMS of every seed group, without a groups x albums matrix (compiled with
// -ffp-contract=off).
//
// Reference: closest_album_to_group (src/playlist.rs:424-485) behind Library::album_playlist_from (src/library.rs:850-893),
// cut after k albums: the group's songs leave the pool, every album left in the pool gets the mean of its songs' analyses
// (ndarray's mean_axis(Axis(0)): the sequential f32 sum of the rows, divided by their number), and the albums come in ascending
// euclidean distance of that mean to the group's own mean.  Here for G groups at once.
//
//   segment_mean_kernel     the sequential f32 mean of every SEGMENT, one launch: the A albums (rows gathered from the candidates
//                           through the album's row list, ascending candidate index), the G groups (contiguous seed rows) and
//                           the P patches -- the (group, album) pairs a skip entry touches: the album's row list walked again
//                           beside the sorted list of the rows that group removes from it.  Lanes run across the features, a
//                           segment is walked in order by ONE half (d <= 32: two segments per wavefront) or whole wavefront:
//                           the adds are a dependent chain, the loads are not, so eight rows travel at a time.  A sum is never
//                           restarted or split, however long the segment.  A segment without rows gets a row of NaN.
//   album_knn_scan_kernel   knn_scan_kernel (kernels_knn.hip) with the group means as queries and the album centroids as
//                           candidates, euclidean, and two more rules.  An album without songs is no candidate.  The patches of
//                           a group are a list sorted by album: the wavefront that owns the group keeps a cursor into it, takes
//                           the patches that fall into the current 256-album block, leaves those albums out of the block's own
//                           pass (a 256-bit mask) and pushes the patched centroids' keys instead -- none for a patch without
//                           rows left, the album then does not exist for the group.  The sorted first k keys of every (group,
//                           split) go to `part`; knn_merge_kernel turns them into idx / dist.
//
// Distances are pair_sum / pl_distance of pairwise_math.hpp / playlist_math.hpp: bit for bit the all-pairs kernel's.
#include <math.h>

#include <algorithm>

#include "device_utils.hpp"
#include "internal.hpp"
#include "knn_list.hpp"
#include "pairwise_math.hpp"
#include "playlist_math.hpp"

namespace bg {

constexpr uint32_t AK_NONE = 0xFFFFFFFFu;

// 0.0f + row ids[first] + row ids[first + 1] + ... of column `col` (ids == NULL: rows first, first + 1, ...), in order, without
// the rows named by the ascending list sk[0 .. nsk).  No row index is 0xFFFFFFFF.
__device__ __forceinline__ float segment_sum(const float* __restrict__ base, uint32_t d, uint32_t col,
                                             const uint32_t* __restrict__ ids, uint32_t first, uint32_t cnt,
                                             const uint32_t* __restrict__ sk, uint32_t nsk) {
    float acc = 0.0f;
    uint32_t sp = 0, next = nsk ? sk[0] : AK_NONE;
    uint32_t r = 0;
    for (; r + 8u <= cnt; r += 8u) {
        uint32_t id[8];
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; i++) id[i] = ids ? ids[first + r + (uint32_t)i] : first + r + (uint32_t)i;
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = base[(uint64_t)id[i] * d + col];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (id[i] == next) {
                sp++;
                next = sp < nsk ? sk[sp] : AK_NONE;
            } else {
                acc = acc + v[i];
            }
        }
    }
    for (; r < cnt; r++) {
        const uint32_t id = ids ? ids[first + r] : first + r;
        if (id == next) {
            sp++;
            next = sp < nsk ? sk[sp] : AK_NONE;
        } else {
            acc = acc + base[(uint64_t)id * d + col];
        }
    }
    return acc;
}

// segments 0 .. A: albums -> centroids; A .. A + G: groups -> gmeans; A + G .. A + G + P: patches -> pcent
__global__ __launch_bounds__(256) void segment_mean_kernel(const float* __restrict__ X, const float* __restrict__ S, uint32_t d,
                                                           AlbumTables t, float* __restrict__ centroids,
                                                           float* __restrict__ gmeans, float* __restrict__ pcent) {
    const uint32_t lane = (uint32_t)lane_id(), wave = (uint32_t)wave_id();
    const uint32_t spw = d <= 32u ? 2u : 1u;  // segments per wavefront
    const uint32_t sub = spw == 2u ? lane >> 5 : 0u;
    const uint32_t fl = spw == 2u ? (lane & 31u) : lane;
    const bool mine = fl < d;
    const uint32_t col = mine ? fl : 0u;  // (the idle lanes read column 0 and store nothing)
    const uint64_t n_seg = (uint64_t)t.n_albums + t.n_groups + t.n_patches;
    for (uint64_t w = (uint64_t)blockIdx.x * 4 + wave; w * spw < n_seg; w += (uint64_t)gridDim.x * 4) {
        const uint64_t seg = w * spw + sub;
        if (seg >= n_seg) continue;
        float sum;
        uint32_t left;
        float* out;
        if (seg < t.n_albums) {
            const uint32_t r0 = t.arow_off[seg];
            left = t.arow_off[seg + 1] - r0;
            sum = segment_sum(X, d, col, t.arow, r0, left, nullptr, 0u);
            out = centroids + seg * d;
        } else if (seg < (uint64_t)t.n_albums + t.n_groups) {
            const uint64_t g = seg - t.n_albums;
            const uint32_t r0 = t.goff[g];
            left = t.goff[g + 1] - r0;
            sum = segment_sum(S, d, col, nullptr, r0, left, nullptr, 0u);
            out = gmeans + g * d;
        } else {
            const uint64_t p = seg - t.n_albums - t.n_groups;
            const uint32_t a = t.patch_album[p], r0 = t.arow_off[a], s0 = t.pskip_off[p];
            left = t.patch_cnt[p];
            sum = segment_sum(X, d, col, t.arow, r0, t.arow_off[a + 1] - r0, t.pskip + s0, t.pskip_off[p + 1] - s0);
            out = pcent + p * d;
        }
        const float mean = left ? sum / (float)left : __uint_as_float(0x7FC00000u);
        if (mine) out[fl] = mean;
    }
}

// D > 0: compile-time feature count (packed arithmetic, centroids in registers).  D == 0: any d <= 64 through pl_distance.
template <int D, int KEYS>
__global__ __launch_bounds__(256, (KEYS == KNN_KEYS_SMALL ? 2 : 1)) void album_knn_scan_kernel(
    const float* __restrict__ Q, uint32_t q, const float* __restrict__ X, uint32_t n, uint32_t d_rt, AlbumTables t,
    const float* __restrict__ PC, uint32_t k, uint32_t cap, uint32_t qb_rt, uint32_t n_split, uint32_t blocks_per_split,
    unsigned long long* __restrict__ part, uint32_t* nan_flag) {
    constexpr bool GENERIC = D == 0;
    constexpr int DD = GENERIC ? 1 : D;
    constexpr int DQ = GENERIC ? PL_DMAX : ((D + 3) & ~3);  // LDS pitch of a group mean: 16-byte aligned -> ds_read_b128 broadcasts
    constexpr int XP = GENERIC ? 1 : (D | 1);               // LDS pitch of a staged centroid: odd, lanes l and l + 1 on different banks
    constexpr bool ROOT = !GENERIC;                         // the bound is on the sum before the square root
    __shared__ __attribute__((aligned(16))) unsigned long long s_buf[KEYS];
    __shared__ __attribute__((aligned(16))) float s_q[KNN_QMAX][DQ];
    __shared__ __attribute__((aligned(16))) float s_x[GENERIC ? 4 : KNN_COLS * XP];
    __shared__ unsigned long long s_thr[KNN_QMAX];
    __shared__ float s_bound[KNN_QMAX];
    __shared__ uint32_t s_cnt[KNN_QMAX], s_pcur[KNN_QMAX], s_pend[KNN_QMAX];
    __shared__ uint32_t s_mask[4][8];

    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const uint32_t d = GENERIC ? d_rt : (uint32_t)D;
    const uint32_t QB = qb_rt;  // groups per workgroup: at most KEYS / cap, and at most KNN_QMAX
    const uint32_t split = blockIdx.x % n_split;
    const uint32_t qb_step = gridDim.x / n_split;
    const uint32_t n_qb = (q + QB - 1) / QB;
    const uint32_t n_blocks = (uint32_t)(((uint64_t)n + KNN_COLS - 1) / KNN_COLS);
    const uint32_t blk0 = split * blocks_per_split;
    const uint32_t blk1 = (blk0 + blocks_per_split < n_blocks) ? blk0 + blocks_per_split : n_blocks;
    bool saw_nan = false;
    const float none[1] = {0.0f};
    float wdiag[DD];
#pragma unroll
    for (int kk = 0; kk < DD; kk++) wdiag[kk] = 0.0f;  // (unused by the euclidean sum)

    for (uint32_t qb = blockIdx.x / n_split; qb < n_qb; qb += qb_step) {
        const uint32_t q0 = qb * QB;
        const uint32_t rows_here = (q - q0 < QB) ? q - q0 : QB;
        __syncthreads();  // every wavefront has finished with the previous block of groups
        for (uint32_t e = (uint32_t)tid; e < rows_here * d; e += 256u) s_q[e / d][e % d] = Q[(uint64_t)q0 * d + e];
        if ((uint32_t)tid < rows_here) {
            // the group's patches from the first album of this split on
            uint32_t lo = t.patch_off[q0 + (uint32_t)tid];
            const uint32_t end = t.patch_off[q0 + (uint32_t)tid + 1u];
            const uint64_t first_album = (uint64_t)blk0 * KNN_COLS;
            uint32_t hi = end;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if ((uint64_t)t.patch_album[mid] < first_album) lo = mid + 1u; else hi = mid;
            }
            s_pcur[tid] = lo;
            s_pend[tid] = end;
            s_cnt[tid] = 0u;
            s_thr[tid] = KNN_NONE;
            s_bound[tid] = INFINITY;
        }
        __syncthreads();

        for (uint32_t blk = blk0; blk < blk1; blk++) {
            const uint32_t j0 = blk * (uint32_t)KNN_COLS;
            const uint32_t cols_here = (n - j0 < (uint32_t)KNN_COLS) ? n - j0 : (uint32_t)KNN_COLS;
            // the lane's four albums as two packed pairs: bp[h][kk] = (album 2h, album 2h + 1), album c = row j0 + 64 c + lane
            f2 bp[2][DD];
            if constexpr (!GENERIC) {
                if (blk != blk0) __syncthreads();  // every wavefront has taken the previous block into registers
                const float* src = X + (uint64_t)j0 * D;
                const uint32_t floats = cols_here * (uint32_t)D;
                for (uint32_t e = (uint32_t)tid; e < floats; e += 256u) s_x[(e / (uint32_t)D) * XP + e % (uint32_t)D] = src[e];
                // a ragged last block: zero rows, so that the lanes beyond it compute on defined values (their results are dropped)
                for (uint32_t e = cols_here * (uint32_t)XP + (uint32_t)tid; e < (uint32_t)(KNN_COLS * XP); e += 256u) s_x[e] = 0.0f;
                __syncthreads();
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const uint32_t la = (uint32_t)(2 * h) * 64u + (uint32_t)lane, lb = la + 64u;
#pragma unroll
                    for (int kk = 0; kk < DD; kk++) {
                        bp[h][kk].x = s_x[la * XP + kk];
                        bp[h][kk].y = s_x[lb * XP + kk];
                    }
                }
            }
            // which of the lane's four albums have songs at all (bit c)
            uint32_t present = 0u;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const uint32_t lc = 64u * (uint32_t)c + (uint32_t)lane;
                if (lc < cols_here && t.arow_off[j0 + lc + 1u] != t.arow_off[j0 + lc]) present |= 1u << c;
            }
            const uint32_t wave_u = (uint32_t)__builtin_amdgcn_readfirstlane(wave);
#pragma unroll 1
            for (uint32_t r = wave_u; r < rows_here; r += 4u) {
                // pv[c]: what the bound is compared with for album c of the lane -- the sum before the root (ROOT) or the distance
                float pv[4];
                if constexpr (GENERIC) {
#pragma unroll 1
                    for (int c = 0; c < 4; c++) {
                        const uint32_t lc = 64u * (uint32_t)c + (uint32_t)lane;
                        pv[c] = ((present >> c) & 1u) ? pl_distance(s_q[r], X + (uint64_t)(j0 + lc) * d, d, PL_EUCLIDEAN, nullptr) : INFINITY;
                    }
                } else {
                    f2 ap[DQ / 2];
#pragma unroll
                    for (int k4 = 0; k4 < DQ / 4; k4++) {  // same address in every lane: LDS broadcast
                        const float4 v = *reinterpret_cast<const float4*>(&s_q[r][4 * k4]);
                        ap[2 * k4].x = v.x; ap[2 * k4].y = v.y; ap[2 * k4 + 1].x = v.z; ap[2 * k4 + 1].y = v.w;
                    }
                    const f2 s0 = pair_sum<DD, METRIC_EUCLIDEAN, false>(ap, bp[0], wdiag, none);
                    const f2 s1 = pair_sum<DD, METRIC_EUCLIDEAN, false>(ap, bp[1], wdiag, none);
                    // (an album without songs has a row of NaN: it must not wake the exact part up)
                    pv[0] = (present & 1u) ? s0.x : INFINITY; pv[1] = (present & 2u) ? s0.y : INFINITY;
                    pv[2] = (present & 4u) ? s1.x : INFINITY; pv[3] = (present & 8u) ? s1.y : INFINITY;
                }
                // the group's patches that fall into this block: [pc, pc + np) of its list (sorted by album)
                const uint32_t pc = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_pcur[r]);
                const uint32_t pe = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_pend[r]);
                uint32_t np = 0u;
                if (pc < pe) {
                    const uint32_t jend = j0 + cols_here;
                    for (uint32_t e0 = 0; e0 < (uint32_t)KNN_COLS; e0 += 64u) {
                        const uint32_t p = pc + e0 + (uint32_t)lane;
                        const bool in = p < pe && t.patch_album[p] < jend;
                        const uint32_t got = (uint32_t)__popcll(__ballot(in));
                        np += got;
                        if (got < 64u) break;
                    }
                }
                // wave-uniform: can any of the wavefront's 256 albums enter the group's k best?  (`!(v > bound)`: a NaN says yes)
                const float bound = s_bound[r];
                const bool maybe = !(pv[0] > bound) || !(pv[1] > bound) || !(pv[2] > bound) || !(pv[3] > bound);
                if (np == 0u && __ballot(maybe) == 0ull) continue;
                // the patched albums of this block as a 256-bit mask: their full-album centroids are not looked at
                uint32_t* mask = s_mask[wave_u];
                if (np) {
                    if (lane < 8) mask[lane] = 0u;
                    knn_wave_sync();
                    for (uint32_t e = (uint32_t)lane; e < np; e += 64u) {
                        const uint32_t a = t.patch_album[pc + e] - j0;
                        atomicOr(&mask[a >> 5], 1u << (a & 31u));
                    }
                    knn_wave_sync();
                }
                // the exact part: distances, keys, the 64-bit comparison with the threshold, survivors into the group's buffer
                KnnList list{s_buf + (size_t)r * cap, s_cnt[r], s_thr[r]};
                const unsigned long long thr_in = list.thr;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const uint32_t lc = 64u * (uint32_t)c + (uint32_t)lane, j = j0 + lc;
                    const bool patched = np != 0u && ((mask[lc >> 5] >> (lc & 31u)) & 1u) != 0u;
                    const bool valid = ((present >> c) & 1u) != 0u && !patched;
                    const float v = ROOT ? sqrtf(pv[c]) : pv[c];
                    if (valid && v != v) saw_nan = true;
                    const unsigned long long key = ((unsigned long long)f32_key(v) << 32) | j;
                    list.push(valid && key < list.thr, key, k, cap, lane);
                }
                // the patched centroids, a lane each; a patch without rows left is no album for this group
                for (uint32_t e0 = 0; e0 < np; e0 += 64u) {
                    const uint32_t e = e0 + (uint32_t)lane;
                    const uint32_t p = e < np ? pc + e : pc;
                    const bool exists = e < np && t.patch_cnt[p] != 0u;
                    const float v = exists ? pl_distance(s_q[r], PC + (uint64_t)p * d_rt, d_rt, PL_EUCLIDEAN, nullptr) : INFINITY;
                    if (exists && v != v) saw_nan = true;
                    const unsigned long long key = ((unsigned long long)f32_key(v) << 32) | t.patch_album[p];
                    list.push(exists && key < list.thr, key, k, cap, lane);
                }
                if (lane == 0) {
                    s_cnt[r] = list.cnt;
                    s_pcur[r] = pc + np;
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
            unsigned long long* dst = part + ((uint64_t)(q0 + r) * n_split + split) * (uint64_t)k;
            for (uint32_t i = (uint32_t)lane; i < k; i += 64u) dst[i] = buf[i];
        }
    }
    if (saw_nan) atomicOr(nan_flag, 1u);
}

void launch_segment_mean(const float* X, const float* S, uint32_t d, const AlbumTables& t, float* centroids, float* gmeans,
                         float* pcent, hipStream_t st) {
    const uint64_t n_seg = (uint64_t)t.n_albums + t.n_groups + t.n_patches;
    if (n_seg == 0) return;
    const uint64_t per_wg = 4u * (d <= 32u ? 2u : 1u);
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n_seg + per_wg - 1) / per_wg, 1u << 20);
    hipLaunchKernelGGL(segment_mean_kernel, dim3(grid), dim3(256), 0, st, X, S, d, t, centroids, gmeans, pcent);
}

void launch_album_knn_scan(const float* gmeans, const float* centroids, uint32_t d, const AlbumTables& t, const float* pcent,
                           uint32_t k, const KnnPlan& p, unsigned long long* part, uint32_t* nan_flag, hipStream_t st) {
    if (t.n_groups == 0) return;
    const dim3 grid(p.grid_qb * p.n_split);
#define AK_GO(DD, KK) hipLaunchKernelGGL((album_knn_scan_kernel<DD, KK>), grid, dim3(256), 0, st, gmeans, t.n_groups, centroids, \
                                         t.n_albums, d, t, pcent, k, p.cap, p.qb, p.n_split, p.blocks_per_split, part, nan_flag)
    const bool small = p.cap <= 256;
    if (d == 23 && small) AK_GO(23, KNN_KEYS_SMALL);
    else if (d == 23) AK_GO(23, KNN_KEYS_BIG);
    else if (d == 20 && small) AK_GO(20, KNN_KEYS_SMALL);
    else if (d == 20) AK_GO(20, KNN_KEYS_BIG);
    else if (small) AK_GO(0, KNN_KEYS_SMALL);
    else AK_GO(0, KNN_KEYS_BIG);
#undef AK_GO
}

}  // namespace bg
