// knn_list.hpp -- the threshold buffer of the k-nearest searches: the 64-bit keys, one wavefront's bitonic sort and the
// append / compact list, shared by kernels_knn.hip and kernels_group_knn.hip.  Include only from translation units compiled
// with -ffp-contract=off (playlist_math.hpp).
#pragma once
#include <math.h>

#include "device_utils.hpp"
#include "playlist_math.hpp"

namespace bg {

constexpr int KNN_COLS = 256;         // candidates per block: four per lane of a wavefront, lanes l, l + 64, l + 128, l + 192
constexpr int KNN_QMAX = 32;          // most queries a workgroup owns (the smallest buffer is 128 keys)
constexpr int KNN_KEYS_SMALL = 4096;  // 32 KiB of keys: two workgroups per CU (cap <= 256)
constexpr int KNN_KEYS_BIG = 14336;   // 112 KiB: one workgroup per CU (cap 512 .. 2048: 28 / 14 / 7 queries)
constexpr unsigned long long KNN_NONE = ~0ull;  // padding key: no distance maps to 0xFFFFFFFF but one NaN, no index is 2^32 - 1

// LDS traffic between the lanes of ONE wavefront (its LDS instructions execute in program order): keep the compiler from
// moving loads and stores across the hand-over
__device__ __forceinline__ void knn_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float knn_key_dist(unsigned long long key) {  // inverse of f32_key
    const uint32_t kb = (uint32_t)(key >> 32);
    return __uint_as_float((kb & 0x80000000u) ? (kb ^ 0x80000000u) : ~kb);
}

// the float a candidate's sum (ROOT) or distance (!ROOT) is compared with: a value ABOVE it cannot beat the threshold key
template <bool ROOT>
__device__ __forceinline__ float knn_bound(unsigned long long thr) {
    if (thr == KNN_NONE) return INFINITY;
    const float t = knn_key_dist(thr);
    if (!ROOT) return t;
    const uint32_t tb = __float_as_uint(t);
    if (tb >= 0x7F800000u) return INFINITY;  // inf, NaN (and any negative: a rounded root is none)
    const float u = __uint_as_float(tb + 1u);
    const uint32_t pb = __float_as_uint(u * u);  // rounded to nearest: at most half an ulp below u^2, one ulp is added
    return pb >= 0x7F800000u ? INFINITY : __uint_as_float(pb + 1u);
}

// One wavefront sorts buf[0 .. cap) ascending (cap a power of two >= 128) after padding buf[cnt .. cap): bitonic network,
// cap / 2 disjoint compare-exchanges per step.
__device__ __forceinline__ void knn_sort(unsigned long long* buf, uint32_t cnt, uint32_t cap, int lane) {
    for (uint32_t i = cnt + (uint32_t)lane; i < cap; i += 64u) buf[i] = KNN_NONE;
    knn_wave_sync();
    for (uint32_t size = 2; size <= cap; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            if (cap < 512u) {  // at most two compare-exchanges per lane
                for (uint32_t t = (uint32_t)lane; t < cap / 2; t += 64u) {
                    const uint32_t i = ((t & ~(stride - 1u)) << 1) | (t & (stride - 1u)), j = i | stride;
                    const unsigned long long a = buf[i], b = buf[j];
                    const bool up = (i & size) == 0u;
                    if ((a > b) == up) {
                        buf[i] = b;
                        buf[j] = a;
                    }
                }
                knn_wave_sync();
                continue;
            }
            // four compare-exchanges per lane and trip, every read ahead of the first write (the pairs of a step are disjoint):
            // the LDS latency is paid once per four
            for (uint32_t t0 = (uint32_t)lane; t0 < cap / 2; t0 += 256u) {
                unsigned long long a[4], b[4];
                uint32_t i[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint32_t t = t0 + 64u * (uint32_t)u;
                    i[u] = ((t & ~(stride - 1u)) << 1) | (t & (stride - 1u));
                    a[u] = buf[i[u]];  // (cap / 2 is a multiple of 256 here)
                    b[u] = buf[i[u] | stride];
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const bool up = (i[u] & size) == 0u;
                    if ((a[u] > b[u]) == up) {
                        buf[i[u]] = b[u];
                        buf[i[u] | stride] = a[u];
                    }
                }
            }
            knn_wave_sync();
        }
    }
}

// The threshold buffer of one query, driven by the wavefront that owns it (every argument but `take` / `key` wave-uniform).
struct KnnList {
    unsigned long long* buf;
    uint32_t cnt;
    unsigned long long thr;
    // keep the k smallest; the threshold becomes the k-th once there are k
    __device__ __forceinline__ void compact(uint32_t k, uint32_t cap, int lane) {
        knn_sort(buf, cnt, cap, lane);
        if (cnt >= k) {
            cnt = k;
            thr = buf[k - 1];
        }
    }
    // append the keys of the lanes with `take` (at most 64; cap - k >= 64 leaves room right after a compaction)
    __device__ __forceinline__ void push(bool take, unsigned long long key, uint32_t k, uint32_t cap, int lane) {
        unsigned long long mask = __ballot(take);
        if (mask == 0ull) return;
        if (cnt + (uint32_t)__popcll(mask) > cap) {
            compact(k, cap, lane);
            take = take && key < thr;
            mask = __ballot(take);
        }
        const uint32_t pos = cnt + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (take) buf[pos] = key;
        cnt += (uint32_t)__popcll(mask);
        knn_wave_sync();
    }
};

}  // namespace bg
