// scan_block.hpp -- the front that the scan kernels share: a block of KNN_COLS candidate rows staged in LDS, a query row read as an
// LDS broadcast, and the sums of a lane's four candidates (taken into packed registers by each kernel's own text) against it.  Device-only function
// templates for a compile-time feature count D > 0; the callers' generic-d paths (D == 0) do not come here.  Include only from
// translation units compiled with -ffp-contract=off (pairwise_math.hpp): the arithmetic is the all-pairs kernel's bit for bit.
//
// No helper hides a barrier whose reason is the caller's: the one BEFORE a block is staged (every wavefront has finished with what
// the LDS held) stays at the call site.
#pragma once
#include <stdint.h>

#include "device_utils.hpp"
#include "knn_list.hpp"
#include "pairwise_math.hpp"

namespace bg {

template <int D>
struct scan_pitch {
    static constexpr int DQ = (D + 3) & ~3;   // LDS pitch of a query row: 16-byte aligned -> ds_read_b128 broadcasts
    static constexpr int XP = D | 1;          // LDS pitch of a staged candidate: odd, lanes l and l + 1 on different banks
    static constexpr bool FLAT = XP == D;     // (an odd d: the staged block is a plain copy of its rows)
};

// M into LDS (Mahalanobis) and its diagonal into wdiag (DIAG: the same in every lane, scalar registers; 0 otherwise).  All 256
// threads of the workgroup call it.  A general M is read from s_m after the caller's next barrier.
template <int D, int METRIC, bool DIAG, int NM>
__device__ __forceinline__ void scan_load_metric(const float* __restrict__ M, float (&s_m)[NM], float (&wdiag)[D], int tid) {
    if (METRIC == METRIC_MAHALANOBIS) {
        for (int e = tid; e < D * D; e += 256) s_m[e] = M[e];
    }
    if (DIAG) __syncthreads();
#pragma unroll
    for (int kk = 0; kk < D; kk++)
        wdiag[kk] = DIAG ? __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s_m[(kk * D + kk) % (METRIC == METRIC_MAHALANOBIS ? D * D : 1)]))) : 0.0f;
}

// rows j0 .. j0 + cols_here of X (cols_here <= KNN_COLS) into s_x at pitch XP, coalesced, by all 256 threads; ends with the barrier
// after which every wavefront may read the block.  s_x must be declared __attribute__((aligned(16))): an odd-d block is written
// with 16-byte LDS stores
template <int D>
__device__ __forceinline__ void scan_stage_block(float (&s_x)[KNN_COLS * scan_pitch<D>::XP], const float* __restrict__ X, uint32_t j0,
                                                 uint32_t cols_here, int tid) {
    constexpr int XP = scan_pitch<D>::XP;
    constexpr bool FLAT = scan_pitch<D>::FLAT;
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
}

// a query row (DQ floats in LDS, 16-byte aligned) as register pairs; the same address in every lane: LDS broadcast
template <int DQ>
__device__ __forceinline__ void scan_query_row(const float* row, f2 (&ap)[DQ / 2]) {
#pragma unroll
    for (int k4 = 0; k4 < DQ / 4; k4++) {
        const float4 v = *reinterpret_cast<const float4*>(&row[4 * k4]);
        ap[2 * k4].x = v.x; ap[2 * k4].y = v.y; ap[2 * k4 + 1].x = v.z; ap[2 * k4 + 1].y = v.w;
    }
}

// pv[c]: the row against candidate c of the lane -- the sum before the square root (euclidean, Mahalanobis) or the finished
// cosine distance; nq = the row's norm (cosine)
template <int D, int METRIC, bool DIAG, int AP, int NM>
__device__ __forceinline__ void scan_pair_values(const f2 (&ap)[AP], const f2 (&bp)[2][D], const f2 (&nb)[2], float nq,
                                                 const float (&wdiag)[D], const float (&s_m)[NM], float (&pv)[4]) {
    f2 s0 = pair_sum<D, METRIC, DIAG>(ap, bp[0], wdiag, s_m);
    // (general M: one pair's 2 x d differences and products at a time -- interleaved by the scheduler, the two pairs spill 464 B
    // per lane instead of 208)
    if (METRIC == METRIC_MAHALANOBIS && !DIAG) asm volatile("" : "+v"(s0));
    f2 s1 = pair_sum<D, METRIC, DIAG>(ap, bp[1], wdiag, s_m);
    if (METRIC == METRIC_COSINE) {
        s0 = splat(1.0f) - s0 / (splat(nq) * nb[0]);
        s1 = splat(1.0f) - s1 / (splat(nq) * nb[1]);
    }
    pv[0] = s0.x; pv[1] = s0.y; pv[2] = s1.x; pv[3] = s1.y;
}

}  // namespace bg
