// kernels_metric.hip -- one gradient evaluation of triplet metric learning (compiled with -ffp-contract=off).
//
// A training triplet (a, b, o) says "a and b are closer together than either is to o" under the Mahalanobis matrix M being
// learned: two hinges h1 = (margin + q(u)) - q(v), h2 = (margin + q(u)) - q(w) with u = x_a - x_b, v = x_a - x_o, w = x_b - x_o and
// q(t) = t' M t.  One step returns which hinges are active, their sum, and G = sum((f1 + f2) u u' - f1 v v' - f2 w w').
// Everything is f64.  The hinges follow the contract of include/blissgpu.h operation by operation (every product and sum
// rounded on its own, ascending from 0.0), so flags and n_active are exact; loss and G are sums in a fixed order.
//
//   triplet_step_kernel    one wavefront per workgroup owns a contiguous chunk of triplets and walks it 64 at a time.
//                          Phase 1, a lane owns a triplet: it gathers its three rows into LDS as f32 (row pitch d | 1: odd, so the
//                          64 lanes' rows start in different banks), forms the three quadratic forms in one pass over M -- M is
//                          read through wave-uniform addresses, i.e. scalar loads, and one M[r][c] serves u, v and w -- and the
//                          two hinges.  A diagonal M (detected by the host as everywhere else) and the identity take the O(d)
//                          form; it gives the bits of the full form, 0 * inf = NaN included.
//                          Phase 2, a lane owns entries of G: the d (d + 1) / 2 entries of the upper triangle are dealt out 64
//                          at a time, E per lane, and stay in registers across the whole chunk.  The wavefront walks the ACTIVE
//                          triplets of the batch (two ballots; the loop is scalar) in ascending order; every lane reads its
//                          (i, j) columns of the three staged rows and adds three fused products.  The coefficients are 0, 1, 2:
//                          scaling by them is exact, so G[i][j] is one sum of rounded-once products.  A batch without an active
//                          hinge skips phase 2 altogether: late in a learning run most do.
//                          The wavefront writes its partial upper triangle, its partial loss (a fixed xor tree over the lanes'
//                          ascending sums), its count of active hinges and its error bits.  No atomics.
//   triplet_reduce_kernel  adds the W partials in a fixed order (16 contiguous segments of the chunks, each ascending, then the 16
//                          segment sums ascending), mirrors the upper triangle (G is symmetric by construction), sums loss and
//                          n_active and ors the error bits into one block the host downloads in one copy.
//
// The split into chunks is a function of T alone (triplet_plan), never of the device: two calls give the same bits anywhere.
// An index >= n sets the INVALID bit and the triplet is skipped before any row is read.
#include <math.h>

#include <algorithm>

#include "device_utils.hpp"
#include "internal.hpp"

namespace bg {

constexpr uint32_t TRIPLET_MAX_WAVES = 2048;  // partials: at most this many chunks

__device__ __forceinline__ bool f64_finite(double v) { return v - v == 0.0; }

// E: entries of G's upper triangle per lane (64 E >= d (d + 1) / 2).  DC > 0: compile-time d.  blockDim.x = 64.
// mode: TRIPLET_M_FULL / _DIAG / _IDENTITY.  part [W][pairs + 1] (the upper triangle row-major, then the loss), cnt [W][2]
// (active hinges, error bits).  Dynamic LDS: 3 * 64 * (d | 1) floats.
template <int E, int DC>
__global__ __launch_bounds__(64) void triplet_step_kernel(const float* __restrict__ X, uint64_t n, uint32_t d_rt,
                                                          const uint32_t* __restrict__ trip, uint64_t T,
                                                          const float* __restrict__ M, int mode, double margin, uint32_t chunk,
                                                          uint8_t* __restrict__ flags, double* __restrict__ part,
                                                          unsigned long long* __restrict__ cnt) {
    extern __shared__ float s_rows[];  // [3][64][ds]: the rows a, b, o of the batch's triplets
    const uint32_t d = DC ? (uint32_t)DC : d_rt, ds = d | 1u, pairs = d * (d + 1u) / 2u;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t t0 = (uint64_t)blockIdx.x * chunk, t1 = std::min<uint64_t>(T, t0 + chunk);
    float* const my_a = s_rows + (0u * 64u + lane) * ds;
    float* const my_b = s_rows + (1u * 64u + lane) * ds;
    float* const my_o = s_rows + (2u * 64u + lane) * ds;

    // the lane's entries: p = lane + 64 e -> (i, j), i <= j, row-major over the upper triangle
    uint32_t pij[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        uint32_t p = lane + 64u * (uint32_t)e, i = 0u;
        if (p >= pairs) p = 0u;  // (never written back)
        while (p >= d - i) { p -= d - i; i++; }
        pij[e] = i | ((i + p) << 8);
    }
    double acc[E];
#pragma unroll
    for (int e = 0; e < E; e++) acc[e] = 0.0;
    double loss = 0.0;
    unsigned long long n_act = 0ull;
    uint32_t err = 0u;

    for (uint64_t tb = t0; tb < t1; tb += 64u) {
        const uint64_t t = tb + lane;
        const bool in = t < t1;
        uint32_t ia = 0u, ib = 0u, io = 0u;
        if (in) { ia = trip[3u * t]; ib = trip[3u * t + 1u]; io = trip[3u * t + 2u]; }
        const bool ok = in && ia < n && ib < n && io < n;
        if (in && !ok) err |= TRIPLET_ERR_INDEX;
        bool f1 = false, f2 = false;
        if (ok) {
            const float* xa = X + (uint64_t)ia * d;
            const float* xb = X + (uint64_t)ib * d;
            const float* xo = X + (uint64_t)io * d;
            for (uint32_t r = 0; r < d; r++) { my_a[r] = xa[r]; my_b[r] = xb[r]; my_o[r] = xo[r]; }
            double qu = 0.0, qv = 0.0, qw = 0.0;
            if (mode == TRIPLET_M_FULL) {
                for (uint32_t r = 0; r < d; r++) {
                    double su = 0.0, sv = 0.0, sw = 0.0;
                    const float* mrow = M + r * d;
                    for (uint32_t c = 0; c < d; c++) {
                        const double m = (double)mrow[c], a = (double)my_a[c], b = (double)my_b[c], o = (double)my_o[c];
                        su = su + m * (a - b);
                        sv = sv + m * (a - o);
                        sw = sw + m * (b - o);
                    }
                    const double a = (double)my_a[r], b = (double)my_b[r], o = (double)my_o[r];
                    qu = qu + (a - b) * su;
                    qv = qv + (a - o) * sv;
                    qw = qw + (b - o) * sw;
                }
            } else {
                bool fu = true, fv = true, fw = true;
                for (uint32_t r = 0; r < d; r++) {
                    const double m = mode == TRIPLET_M_IDENTITY ? 1.0 : (double)M[r * d + r];
                    const double a = (double)my_a[r], b = (double)my_b[r], o = (double)my_o[r];
                    const double u = a - b, v = a - o, w = b - o;
                    fu = fu && f64_finite(u); fv = fv && f64_finite(v); fw = fw && f64_finite(w);
                    qu = qu + u * (0.0 + m * u);
                    qv = qv + v * (0.0 + m * v);
                    qw = qw + w * (0.0 + m * w);
                }
                if (d > 1u) {  // the full form multiplies an infinite difference by the zeros off the diagonal
                    if (!fu) qu = NAN;
                    if (!fv) qv = NAN;
                    if (!fw) qw = NAN;
                }
            }
            const double base = margin + qu, h1 = base - qv, h2 = base - qw;
            if (h1 != h1 || h2 != h2) err |= TRIPLET_ERR_NAN;
            f1 = h1 > 0.0;
            f2 = h2 > 0.0;
            if (f1) loss = loss + h1;
            if (f2) loss = loss + h2;
            n_act += (f1 ? 1u : 0u) + (f2 ? 1u : 0u);
        }
        if (flags && in) flags[t] = (uint8_t)((f1 ? 1u : 0u) | (f2 ? 2u : 0u));
        const unsigned long long m1 = __ballot(f1), m2 = __ballot(f2);
        __syncthreads();  // (one wavefront: the rows of every lane are in LDS)
        for (unsigned long long mask = m1 | m2; mask; mask &= mask - 1ull) {
            const uint32_t k = (uint32_t)__builtin_ctzll(mask);
            const double c1 = (double)((m1 >> k) & 1ull), c2 = (double)((m2 >> k) & 1ull), c0 = c1 + c2;
            const float* ra = s_rows + (0u * 64u + k) * ds;
            const float* rb = s_rows + (1u * 64u + k) * ds;
            const float* ro = s_rows + (2u * 64u + k) * ds;
#pragma unroll
            for (int e = 0; e < E; e++) {
                if (64u * (uint32_t)e < pairs) {  // (the same in every lane)
                    const uint32_t i = pij[e] & 0xFFu, j = pij[e] >> 8;
                    const double ai = (double)ra[i], bi = (double)rb[i], oi = (double)ro[i];
                    const double aj = (double)ra[j], bj = (double)rb[j], oj = (double)ro[j];
                    double g = acc[e];
                    g = __builtin_fma(c0 * (ai - bi), aj - bj, g);
                    g = __builtin_fma(-c1 * (ai - oi), aj - oj, g);
                    g = __builtin_fma(-c2 * (bi - oi), bj - oj, g);
                    acc[e] = g;
                }
            }
        }
        __syncthreads();  // the next batch overwrites the rows
    }

    const uint32_t ps = pairs + 1u;
    double* out = part + (uint64_t)blockIdx.x * ps;
#pragma unroll
    for (int e = 0; e < E; e++) {
        const uint32_t p = lane + 64u * (uint32_t)e;
        if (p < pairs) out[p] = acc[e];
    }
    loss = wave_sum(loss);
    n_act = wave_sum(n_act);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) err |= (uint32_t)__shfl_xor((int)err, off, WAVE);
    if (lane == 0u) {
        out[pairs] = loss;
        cnt[2ull * blockIdx.x] = n_act;
        cnt[2ull * blockIdx.x + 1ull] = err;
    }
}

// out: G f64 [d][d] | loss f64 | n_active u64 | error bits u64.  A workgroup adds 16 columns of the partials (entries of the
// upper triangle; the loss is column `pairs`): the W chunks are cut into 16 contiguous segments, thread (segment, column) adds
// its segment in ascending order -- eight loads in flight ahead of their adds, 16 lanes on one 128-byte line -- and the first 16
// threads add the 16 segment sums in ascending order: a fixed order, a function of W alone.  The last workgroup sums the counts
// and ors the error bits (integers: any order).
constexpr uint32_t TR_COLS = 16, TR_SEGS = 16;
__global__ __launch_bounds__(256) void triplet_reduce_kernel(const double* __restrict__ part, const unsigned long long* __restrict__ cnt,
                                                             uint32_t W, uint32_t d, double* __restrict__ out) {
    __shared__ double sh[TR_SEGS][TR_COLS];
    __shared__ unsigned long long sh_n[256], sh_e[256];
    const uint32_t pairs = d * (d + 1u) / 2u, ps = pairs + 1u, tid = threadIdx.x;
    if (blockIdx.x == gridDim.x - 1u) {
        unsigned long long a = 0ull, e = 0ull;
        for (uint32_t w = tid; w < W; w += 256u) { a += cnt[2ull * w]; e |= cnt[2ull * w + 1ull]; }
        sh_n[tid] = a;
        sh_e[tid] = e;
        __syncthreads();
        for (uint32_t s = 128u; s > 0u; s >>= 1) {
            if (tid < s) { sh_n[tid] += sh_n[tid + s]; sh_e[tid] |= sh_e[tid + s]; }
            __syncthreads();
        }
        if (tid == 0u) {
            unsigned long long* words = reinterpret_cast<unsigned long long*>(out + d * d + 1u);
            words[0] = sh_n[0];
            words[1] = sh_e[0];
        }
        return;
    }
    const uint32_t col = tid % TR_COLS, seg = tid / TR_COLS, p = blockIdx.x * TR_COLS + col;
    const uint32_t per = (W + TR_SEGS - 1u) / TR_SEGS, w_lo = std::min(W, seg * per), w_hi = std::min(W, w_lo + per);
    double s = 0.0;
    if (p <= pairs) {
        for (uint32_t w0 = w_lo; w0 < w_hi; w0 += 8u) {
            double v[8];
#pragma unroll
            for (uint32_t k = 0; k < 8u; k++) v[k] = w0 + k < w_hi ? part[(uint64_t)(w0 + k) * ps + p] : 0.0;
#pragma unroll
            for (uint32_t k = 0; k < 8u; k++) s = s + v[k];  // (past the segment: s + 0.0 == s)
        }
    }
    sh[seg][col] = s;
    __syncthreads();
    if (seg != 0u || p > pairs) return;
    double t = 0.0;
#pragma unroll
    for (uint32_t k = 0; k < TR_SEGS; k++) t = t + sh[k][col];
    if (p == pairs) {
        out[d * d] = t;
    } else {
        uint32_t q = p, i = 0u;
        while (q >= d - i) { q -= d - i; i++; }
        const uint32_t j = i + q;
        out[i * d + j] = t;
        out[j * d + i] = t;
    }
}

TripletPlan triplet_plan(uint64_t T, uint32_t d) {
    TripletPlan p{};
    uint64_t W = std::max<uint64_t>(1, std::min<uint64_t>((T + 63) / 64, TRIPLET_MAX_WAVES));
    uint64_t chunk = std::max<uint64_t>(1, (T + W - 1) / W);
    chunk = (chunk + 63) / 64 * 64;
    W = std::max<uint64_t>(1, (T + chunk - 1) / chunk);
    p.W = (uint32_t)W;
    p.chunk = (uint32_t)chunk;
    p.pairs = d * (d + 1u) / 2u;
    p.part_doubles = W * (p.pairs + 1u);
    return p;
}

void launch_triplet_step(const float* X, uint64_t n, uint32_t d, const uint32_t* trip, uint64_t T, const float* M, int mode,
                         double margin, const TripletPlan& p, uint8_t* flags, double* part, unsigned long long* cnt, hipStream_t st) {
    const dim3 grid(p.W), block(64);
    const size_t lds = (size_t)3 * 64 * (d | 1u) * sizeof(float);
#define TS_GO(EE, DD) hipLaunchKernelGGL((triplet_step_kernel<EE, DD>), grid, block, lds, st, X, n, d, trip, T, M, mode, margin, \
                                         p.chunk, flags, part, cnt)
    if (d == 23) TS_GO(5, 23);
    else if (d == 20) TS_GO(4, 20);
    else TS_GO(33, 0);  // any d <= 64: 2080 entries at most
#undef TS_GO
}

void launch_triplet_reduce(const double* part, const unsigned long long* cnt, const TripletPlan& p, uint32_t d, double* out,
                           hipStream_t st) {
    hipLaunchKernelGGL(triplet_reduce_kernel, dim3((p.pairs + 1u + TR_COLS - 1u) / TR_COLS + 1u), dim3(256), 0, st, part, cnt, p.W, d, out);
}

}  // namespace bg
