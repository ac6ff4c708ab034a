// kernels_map.hip -- the device half of the 2-D map of a song library (include/blissgpu.h states the arithmetic, DESIGN.md
// 3.31 the shapes tried): exact t-SNE gradients, all pairs and no n x n matrix, every sum in a fixed order (compiled with
// -ffp-contract=off; the f32 division is the compiler's correctly rounded one, which hipcc selects by default).
//
//   map_repulse_kernel  grid = 256-row blocks x column chunks.  A lane owns row i in registers and walks the chunk's j in
//                       ascending order; every lane of a wavefront meets the same j at the same time, so y_j is wave-uniform:
//                       read as LDS broadcasts of a staged tile of 256 points (MAP_FEED_LDS: what runs, by the measurement in
//                       DESIGN.md 3.31) or by scalar loads (MAP_FEED_SCALAR, kept for the bench tool).  The chunk width is a
//                       multiple of 256, so the tiles of j coincide with the row blocks and only the tile that IS the
//                       workgroup's row block holds a j == i: that one tile runs the loop with the test, every other
//                       without.  Three f64 sums per lane, written to sums (one chunk) or to the chunk's plane of part.  No
//                       atomics.
//   map_attract_kernel  <false>: grid = 256-row blocks, a lane per row.  First the row's chunk sums are added in chunk order
//                       (with more than one chunk) and the block's 256 z_i are added by one lane into zb[block] -- the
//                       normaliser Z needs every row before any row's gradient, and this is the launch that sits between the
//                       scan and the update with a workgroup per 256 CONSECUTIVE rows.  Then the lane walks its CSR entries,
//                       unless there are more than MAP_LONG_ROW of them.  <true>: a wavefront per such row (the host lists
//                       them): 64 entries' products at a time in parallel, then added in stored order by every lane alike.
//   map_update_kernel   grid = 256-row blocks.  Lane 0 adds zb in ascending order (Z; block 0 stores it), then every lane forms
//                       its row's two gradient entries and either stores them (a.grad) or applies the update to U, gain, Y.
//                       Every workgroup adds all of zb: ceil(n / 256)^2 additions per iteration against the scan's n^2 pairs
//                       of some 35 instructions each, 1 / 65 536 of the pairs whatever n (DESIGN.md 3.31 has the arithmetic
//                       for the largest n); a fold by one workgroup would cost a launch per iteration instead.
#include <math.h>

#include <algorithm>

#include "internal.hpp"
#include "launch_forms.hpp"

namespace bg {

namespace {

struct MapSums {
    double z, rx, ry;
};

// one pair of the repulsion: the f32 quantities of the contract, each rounded on its own, then the three f64 additions
template <bool SELF_TEST>
__device__ __forceinline__ void map_pair(float xi, float yi, float2 pj, bool self, MapSums& s) {
#pragma clang fp contract(off)
    const float dx = xi - pj.x, dy = yi - pj.y;
    const float sq = dx * dx + dy * dy;
    const float q = 1.0f / (1.0f + sq);
    const float qq = q * q;
    double dz = (double)q, dxr = (double)(qq * dx), dyr = (double)(qq * dy);
    if (SELF_TEST && self) { dz = 0.0; dxr = 0.0; dyr = 0.0; }  // (adding +0.0 leaves a sum that started at +0.0 as it is)
    s.z += dz;
    s.rx += dxr;
    s.ry += dyr;
}

template <int FEED>
__global__ __launch_bounds__(MAP_TILE) void map_repulse_kernel(const float2* __restrict__ Y, uint32_t n, uint32_t width,
                                                                double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ float2 tile[FEED == MAP_FEED_LDS ? MAP_TILE : 1];
    const uint32_t t = threadIdx.x, r0 = blockIdx.x * MAP_TILE, i = r0 + t;
    const uint32_t j0 = blockIdx.y * width, j1 = min(n, j0 + width);  // j0 < n: the grid holds the chunks that are not empty
    const float2 pi = i < n ? Y[i] : make_float2(0.0f, 0.0f);
    MapSums s{0.0, 0.0, 0.0};
    for (uint32_t jt = j0; jt < j1; jt += MAP_TILE) {
        const uint32_t cnt = min(MAP_TILE, j1 - jt);
        const float2* src;
        if (FEED == MAP_FEED_LDS) {
            __syncthreads();  // the tile before this one has been read
            if (t < cnt) tile[t] = Y[jt + t];
            __syncthreads();
            src = tile;
        } else {
            src = Y + jt;  // wave-uniform addresses of memory nothing in this kernel writes: scalar loads
        }
        if (jt == r0) {
            for (uint32_t k = 0; k < cnt; k++) map_pair<true>(pi.x, pi.y, src[k], k == t, s);
        } else if (cnt == MAP_TILE) {
#pragma unroll 8
            for (uint32_t k = 0; k < MAP_TILE; k++) map_pair<false>(pi.x, pi.y, src[k], false, s);
        } else {
            for (uint32_t k = 0; k < cnt; k++) map_pair<false>(pi.x, pi.y, src[k], false, s);
        }
    }
    if (i < n) {
        double* o = out + (size_t)blockIdx.y * 3 * n;
        o[i] = s.z;
        o[(size_t)n + i] = s.rx;
        o[2 * (size_t)n + i] = s.ry;
    }
}

// the attraction of one CSR entry, f32, each operation rounded on its own
__device__ __forceinline__ void map_attract_pair(float2 pi, float2 pj, float v, float* wx, float* wy) {
#pragma clang fp contract(off)
    const float dx = pi.x - pj.x, dy = pi.y - pj.y;
    const float sq = dx * dx + dy * dy;
    const float q = 1.0f / (1.0f + sq);
    const float w = v * q;
    *wx = w * dx;
    *wy = w * dy;
}

template <bool LONG>
__global__ __launch_bounds__(LONG ? 64 : MAP_TILE) void map_attract_kernel(MapArgs a, uint32_t chunks) {
#pragma clang fp contract(off)
    const float2* __restrict__ Y = reinterpret_cast<const float2*>(a.Y);
    const uint32_t t = threadIdx.x, n = a.n;
    if (LONG) {
        __shared__ double px[64], py[64];
        const uint32_t i = a.long_rows[blockIdx.x];
        const unsigned long long e0 = a.row_offsets[i], e1 = a.row_offsets[i + 1];
        const float2 pi = Y[i];
        double ax = 0.0, ay = 0.0;
        for (unsigned long long e = e0; e < e1; e += 64) {
            const uint32_t cnt = (uint32_t)std::min<unsigned long long>(64, e1 - e);
            __syncthreads();  // (one wavefront: the products before these have been added by every lane)
            if (t < cnt) {
                float wx, wy;
                map_attract_pair(pi, Y[a.cols[e + t]], a.vals[e + t], &wx, &wy);
                px[t] = (double)wx;
                py[t] = (double)wy;
            }
            __syncthreads();
            for (uint32_t k = 0; k < cnt; k++) {
                ax += px[k];
                ay += py[k];
            }
        }
        if (t == 0) {
            a.att[2 * (size_t)i] = ax;
            a.att[2 * (size_t)i + 1] = ay;
        }
        return;
    }
    __shared__ double zs[MAP_TILE];
    const uint32_t r0 = blockIdx.x * MAP_TILE, i = r0 + t;
    if (i < n) {
        double z;
        if (chunks > 1) {  // the chunk sums in chunk order, from +0.0
            z = 0.0;
            double rx = 0.0, ry = 0.0;
            for (uint32_t c = 0; c < chunks; c++) {
                const double* p = a.part + (size_t)c * 3 * n;
                z += p[i];
                rx += p[(size_t)n + i];
                ry += p[2 * (size_t)n + i];
            }
            a.sums[i] = z;
            a.sums[(size_t)n + i] = rx;
            a.sums[2 * (size_t)n + i] = ry;
        } else {
            z = a.sums[i];
        }
        zs[t] = z;
    }
    __syncthreads();
    if (t == 0) {  // the block's rows in ascending order
        const uint32_t cnt = min(MAP_TILE, n - r0);
        double zb = 0.0;
        for (uint32_t k = 0; k < cnt; k++) zb += zs[k];
        a.zb[blockIdx.x] = zb;
    }
    if (i >= n) return;
    const unsigned long long e0 = a.row_offsets[i], e1 = a.row_offsets[i + 1];
    if (e1 - e0 > MAP_LONG_ROW) return;  // launch_map_attract_long's
    const float2 pi = Y[i];
    double ax = 0.0, ay = 0.0;
    unsigned long long e = e0;
    for (; e + 8 <= e1; e += 8) {  // eight entries' loads and products in flight, then their additions in stored order
        float wx[8], wy[8];
#pragma unroll
        for (int u = 0; u < 8; u++) map_attract_pair(pi, Y[a.cols[e + u]], a.vals[e + u], &wx[u], &wy[u]);
#pragma unroll
        for (int u = 0; u < 8; u++) {
            ax += (double)wx[u];
            ay += (double)wy[u];
        }
    }
    for (; e < e1; e++) {
        float wx, wy;
        map_attract_pair(pi, Y[a.cols[e]], a.vals[e], &wx, &wy);
        ax += (double)wx;
        ay += (double)wy;
    }
    a.att[2 * (size_t)i] = ax;
    a.att[2 * (size_t)i + 1] = ay;
}

__global__ __launch_bounds__(MAP_TILE) void map_update_kernel(MapArgs a, uint32_t blocks) {
#pragma clang fp contract(off)
    __shared__ double z_all;
    const uint32_t t = threadIdx.x, n = a.n, i = blockIdx.x * MAP_TILE + t;
    if (t == 0) {  // the block sums in ascending order
        double Z = 0.0;
        for (uint32_t b = 0; b < blocks; b++) Z += a.zb[b];
        z_all = Z;
        if (blockIdx.x == 0) *a.z_out = Z;
    }
    __syncthreads();
    if (i >= n) return;
    const double Z = z_all;
#pragma unroll
    for (uint32_t c = 0; c < 2; c++) {
        const size_t e = 2 * (size_t)i + c;
        const double r = a.sums[(size_t)(1 + c) * n + i];
        const double g = 4.0 * (a.exaggeration * a.att[e] - r / Z);
        if (a.grad) {
            a.grad[e] = g;
            continue;
        }
        double U = 0.0, gain = 1.0;
        if (!a.first) { U = a.U[e]; gain = a.gain[e]; }
        gain = (U * g < 0.0) ? gain + 0.2 : gain * 0.8;
        gain = fmax(gain, a.min_gain);
        U = a.momentum * U - (a.lr * gain) * g;
        a.U[e] = U;
        a.gain[e] = gain;
        a.Y[e] = (float)((double)a.Y[e] + U);
    }
}

}  // namespace

// Column groups when the caller names none: enough workgroups for four wavefronts on every SIMD (a workgroup is four), none
// with less than one tile of j, at most MAP_MAX_COL_GROUPS.  Once the rows alone are that many the answer is 1, so the partials
// (24 bytes per row and group) never pass 24 * 2 * 256 * 4 * n_cus bytes: 12 MiB on 256 CUs.
uint32_t map_plan_col_groups(uint64_t n, int n_cus) {
    const uint64_t cus = cus_or_default(n_cus);
    const uint64_t blocks = (n + MAP_TILE - 1) / MAP_TILE;
    if (blocks <= 1) return 1;
    const uint64_t want = (4 * cus + blocks - 1) / blocks;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({want, blocks, (uint64_t)MAP_MAX_COL_GROUPS}));
}

MapPlan map_plan(uint64_t n, uint32_t col_groups) {
    MapPlan p{};
    p.col_groups = std::max(1u, col_groups);
    p.blocks = (uint32_t)((n + MAP_TILE - 1) / MAP_TILE);
    const uint64_t per = (n + p.col_groups - 1) / p.col_groups;
    p.width = (uint32_t)(MAP_TILE * std::max<uint64_t>(1, (per + MAP_TILE - 1) / MAP_TILE));
    p.chunks = (uint32_t)std::max<uint64_t>(1, (n + p.width - 1) / p.width);
    return p;
}

void launch_map_repulse(const MapArgs& a, const MapPlan& p, int feed, hipStream_t st) {
    if (a.n == 0) return;
    const dim3 grid(p.blocks, p.chunks), block(MAP_TILE);
    double* out = p.chunks > 1 ? a.part : a.sums;
    const float2* Y = reinterpret_cast<const float2*>(a.Y);
    if (feed == MAP_FEED_LDS) hipLaunchKernelGGL(map_repulse_kernel<MAP_FEED_LDS>, grid, block, 0, st, Y, a.n, p.width, out);
    else hipLaunchKernelGGL(map_repulse_kernel<MAP_FEED_SCALAR>, grid, block, 0, st, Y, a.n, p.width, out);
}

void launch_map_attract(const MapArgs& a, const MapPlan& p, hipStream_t st) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(map_attract_kernel<false>, dim3(p.blocks), dim3(MAP_TILE), 0, st, a, p.chunks);
}

void launch_map_attract_long(const MapArgs& a, hipStream_t st) {
    if (a.n_long == 0) return;
    hipLaunchKernelGGL(map_attract_kernel<true>, dim3(a.n_long), dim3(64), 0, st, a, 0u);
}

void launch_map_update(const MapArgs& a, const MapPlan& p, hipStream_t st) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(map_update_kernel, dim3(p.blocks), dim3(MAP_TILE), 0, st, a, p.blocks);
}

}  // namespace bg
