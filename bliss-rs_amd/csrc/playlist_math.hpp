// playlist_math.hpp -- one pair distance for any feature count d <= 64 and the order-preserving sort key of a distance,
// shared by the playlist kernels (kernels_playlist.hip) and the k-nearest search (kernels_knn.hip).  Include only from
// translation units compiled with -ffp-contract=off.
#pragma once
#include "device_utils.hpp"

namespace bg {

enum { PL_EUCLIDEAN = 0, PL_COSINE = 1, PL_MAHALANOBIS = 2 };
constexpr int PL_DMAX = 64;

// ndarray::numeric_util::unrolled_dot (8 partial sums, (p0+p4)+(p1+p5)+(p2+p6)+(p3+p7), tail sequentially)
template <typename FX, typename FY>
__device__ __forceinline__ float pl_udot(FX xs, FY ys, uint32_t d) {
    float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    uint32_t k = 0;
    for (; k + 8 <= d; k += 8)
#pragma unroll
        for (int u = 0; u < 8; u++) p[u] = p[u] + xs(k + u) * ys(k + u);
    float sum = 0.0f;
    sum = sum + (p[0] + p[4]);
    sum = sum + (p[1] + p[5]);
    sum = sum + (p[2] + p[6]);
    sum = sum + (p[3] + p[7]);
    for (; k < d; k++) sum = sum + xs(k) * ys(k);
    return sum;
}

// euclidean / cosine / mahalanobis distance of src/playlist.rs:65-79,140-142 between a (any address space)
// and b; same evaluation order as pairwise_generic_kernel
__device__ __forceinline__ float pl_distance(const float* a, const float* b, uint32_t d, int metric,
                                             const float* __restrict__ M) {
    if (metric == PL_COSINE) {
        const float ab = pl_udot([&](uint32_t k) { return a[k]; }, [&](uint32_t k) { return b[k]; }, d);
        const float aa = pl_udot([&](uint32_t k) { return a[k]; }, [&](uint32_t k) { return a[k]; }, d);
        const float bb = pl_udot([&](uint32_t k) { return b[k]; }, [&](uint32_t k) { return b[k]; }, d);
        return 1.0f - ab / (sqrtf(aa) * sqrtf(bb));
    }
    if (metric == PL_EUCLIDEAN) {
        return sqrtf(pl_udot([&](uint32_t k) { return a[k] - b[k]; }, [&](uint32_t k) { return a[k] - b[k]; }, d));
    }
    float t[PL_DMAX];
    for (uint32_t jj = 0; jj < d; jj++) {
        float s = 0.0f;
        for (uint32_t ii = 0; ii < d; ii++) s = s + (a[ii] - b[ii]) * M[ii * d + jj];
        t[jj] = s;
    }
    return sqrtf(pl_udot([&](uint32_t k) { return t[k]; }, [&](uint32_t k) { return a[k] - b[k]; }, d));
}

// order-preserving u32 image of a non-NaN float; -0.0 and +0.0 compare equal in the reference (partial_cmp /
// n32), so both map to the image of +0.0
__device__ __forceinline__ uint32_t f32_key(float v) {
    if (v == 0.0f) v = 0.0f;
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

}  // namespace bg
