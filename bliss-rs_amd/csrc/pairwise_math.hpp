// pairwise_math.hpp -- the per-pair arithmetic of the feature-vector distances, shared by the all-pairs kernel
// (kernels_pairwise.hip) and the k-nearest search (kernels_knn.hip).  Include only from translation units compiled with
// -ffp-contract=off: every multiply and add below rounds on its own, as in the reference (src/playlist.rs:65-79,140-142;
// ndarray's unrolled_dot order -- see the head of kernels_pairwise.hip).
#pragma once
#include <type_traits>

#include "device_utils.hpp"
#include "launch_forms.hpp"

namespace bg {


typedef float f2 __attribute__((ext_vector_type(2)));

// compile-time loop: f(std::integral_constant<int, 0>{}), ..., f(std::integral_constant<int, N-1>{})
template <int N, typename F, int I = 0>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, F, I + 1>(static_cast<F&&>(f));
    }
}
__device__ __forceinline__ f2 splat(float x) { f2 r; r.x = x; r.y = x; return r; }

// (a, a) - b and (a, a) * b where a is the LO (HI = false) or HI half of a register pair: the broadcast
// is an op_sel modifier of the packed instruction instead of two v_mov per element
template <bool HI>
__device__ __forceinline__ f2 bsub(f2 apair, f2 b) {
    f2 r;
    if (HI) asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(apair), "v"(b));
    else asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(apair), "v"(b));
    return r;
}
template <bool HI>
__device__ __forceinline__ f2 bmul(f2 apair, f2 b) {
    f2 r;
    if (HI) asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(r) : "v"(apair), "v"(b));
    else asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(r) : "v"(apair), "v"(b));
    return r;
}

// ndarray::numeric_util::unrolled_dot over compile-time length D, evaluated for TWO pairs at once in packed
// f32 (v_pk_mul_f32 / v_pk_add_f32: each half rounds exactly like the scalar op; this translation unit is
// compiled with -ffp-contract=off so the multiply and the add stay separate, as in the reference).
template <int D, typename FX, typename FY>
__device__ __forceinline__ f2 unrolled_dot2(FX xs, FY ys) {
    f2 p[8];
#pragma unroll
    for (int u = 0; u < 8; u++) p[u] = splat(0.0f);
    constexpr int BODY = (D / 8) * 8;
#pragma unroll
    for (int k = 0; k < BODY; k++) p[k & 7] = p[k & 7] + xs(k) * ys(k);
    f2 sum = splat(0.0f);
    sum = sum + (p[0] + p[4]);
    sum = sum + (p[1] + p[5]);
    sum = sum + (p[2] + p[6]);
    sum = sum + (p[3] + p[7]);
#pragma unroll
    for (int k = BODY; k < D; k++) sum = sum + xs(k) * ys(k);
    return sum;
}

template <int D, typename FX, typename FY>
__device__ __forceinline__ float unrolled_dot(FX xs, FY ys) {
    float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    constexpr int BODY = (D / 8) * 8;
#pragma unroll
    for (int k = 0; k < BODY; k++) p[k & 7] = p[k & 7] + xs(k) * ys(k);
    float sum = 0.0f;
    sum = sum + (p[0] + p[4]);
    sum = sum + (p[1] + p[5]);
    sum = sum + (p[2] + p[6]);
    sum = sum + (p[3] + p[7]);
#pragma unroll
    for (int k = BODY; k < D; k++) sum = sum + xs(k) * ys(k);
    return sum;
}

// The reference's sum for ONE row against the two columns of a packed pair, before the square root / the cosine's division:
//   ap    the row, two features per register pair (ap[k / 2] holds features k - k % 2 and k - k % 2 + 1)
//   bp    the two columns, feature by feature: bp[k] = (column 0's feature k, column 1's feature k)
//   wdiag the diagonal of M (DIAG), sm the whole of M, row-major (general M); unused otherwise
// euclidean: sum (a - b)^2; cosine: a . b; Mahalanobis: ((a - b) M) . (a - b), the vector-matrix product column by column with a
// plain sequential sum (Array1.dot(Array2)), everything else in unrolled_dot order.
template <int D, int METRIC, bool DIAG, int AP, int NM>
__device__ __forceinline__ f2 pair_sum(const f2 (&ap)[AP], const f2 (&bp)[D], const float (&wdiag)[D], const float (&sm)[NM]) {
    // term k of the unrolled_dot for the two columns
    auto term = [&](auto kc) __attribute__((always_inline)) -> f2 {
        constexpr int k = decltype(kc)::value;
        constexpr bool HI = (k & 1) != 0;
        if (METRIC == METRIC_COSINE) return bmul<HI>(ap[k / 2], bp[k]);
        const f2 v = bsub<HI>(ap[k / 2], bp[k]);
        if (METRIC == METRIC_EUCLIDEAN) return v * v;
        if (DIAG) return (v * splat(wdiag[k])) * v;
        return v;  // (general M: the difference itself)
    };
    if (METRIC == METRIC_MAHALANOBIS && !DIAG) {
        f2 v[D], t[D];
        static_for<D>([&](auto kc) { v[decltype(kc)::value] = term(kc); });
#pragma unroll 1
        for (int jj = 0; jj < D; jj++) {
            f2 acc = splat(0.0f);
#pragma unroll
            for (int ii = 0; ii < D; ii++) acc = acc + v[ii] * splat(sm[ii * D + jj]);
            t[jj] = acc;
        }
        return unrolled_dot2<D>([&](int k) { return t[k]; }, [&](int k) { return v[k]; });
    }
    f2 p[8];
    constexpr int BODY = (D / 8) * 8;
    f2 sum;
    if (METRIC == METRIC_EUCLIDEAN && BODY >= 8) {
        // every term is a square (>= +0), so the reference's `0.0 + term` and `0.0 + (p0 + p4)` are exact
        // identities: start the eight partial sums at their first term (10 of 78 packed instructions less)
        static_for<8>([&](auto kc) { p[decltype(kc)::value] = term(kc); });
        static_for<BODY - 8>([&](auto kc) { constexpr int k = 8 + decltype(kc)::value; p[k & 7] = p[k & 7] + term(std::integral_constant<int, k>{}); });
        sum = p[0] + p[4];
    } else {
#pragma unroll
        for (int u = 0; u < 8; u++) p[u] = splat(0.0f);
        static_for<BODY>([&](auto kc) { constexpr int k = decltype(kc)::value; p[k & 7] = p[k & 7] + term(kc); });
        sum = splat(0.0f);
        sum = sum + (p[0] + p[4]);
    }
    sum = sum + (p[1] + p[5]);
    sum = sum + (p[2] + p[6]);
    sum = sum + (p[3] + p[7]);
    static_for<D - BODY>([&](auto kc) { sum = sum + term(std::integral_constant<int, BODY + decltype(kc)::value>{}); });
    return sum;
}

}  // namespace bg
