// kernels_forest.hip -- the extended isolation forest playlist metric (ForestOptions, src/playlist.rs:230-251):
// the host builder, the canonical export, the device image and the scoring kernels.  Compiled with -ffp-contract=off.
//
// The algorithm is Hariri, Carrasco Kind, Brunner, "Extended Isolation Forest" (IEEE TKDE 2019) in the shape the
// reference's ForestOptions exposes; the contract is written out in include/blissgpu.h.  Two decisions make the device
// result a discrete one:
//   * the split test is defined f32 arithmetic: s = +0; for j ascending with normal[j] != 0: s = s + normal[j] * x[j]
//     (product and sum each rounded); left iff s < b.  The builder partitions its samples with the very same function
//     (forest_split_sum below), and dropped components are skipped, never multiplied.
//   * a leaf's path length depth + c(size) is stored as round(value * 2^24) in a u32 and summed per candidate in a u64, so
//     the sum does not depend on the order of the trees: the kernel splits the trees over workgroups freely.
//
// Device image (internal): node = `stride` u32 words, K = extension_level + 1 components in G = ceil(K / 4) groups,
// stride = (2 + 5 G) | 1 (odd, so that the nodes of a tree spread over the LDS banks):
//     [0] b (f32 bits) on an inner node, leaf_q on a leaf      [1] index of the right child inside the tree, LEAF on a leaf
//     then per group: one word holding four dimensions (a byte each), four components of the normal; ascending dimension,
//     the last group padded with value 0 and dimension d: row d of the LDS feature block is all +0.0, so a padded
//     component adds exactly +0.0 * +0.0 -- no candidate value is ever multiplied by a dropped component
// Trees are stored in preorder, so the left child of node i is node i + 1 and is not stored.
//
// forest_walk_kernel<STAGE, WG, G>: WG candidates per workgroup, one lane each, their features transposed in LDS
// (feat[j * WG + lane]: bank = lane % 32 whatever j, so a lane-varying dimension costs no conflict).  The trees come in
// chunks of consecutive trees whose nodes fit the LDS node buffer; a chunk is copied there once per workgroup and every
// lane walks its trees from LDS.  The walk is latency-bound (node -> test -> next node), so the staged form is instantiated
// per group count G with the group loop unrolled: header and dimension words in one round trip, all components and all
// features in a second, then the chain of adds (G = 0: the loop over the groups, used from global memory).  Two shapes: 256 lanes with a
// 4096-word buffer (four workgroups per CU) when every tree fits it, else 512 lanes with 8192 words (two per CU, the same
// 16 wavefronts).  A tree larger than that is walked from global memory (STAGE = false walks every tree from there: the
// measurement form).  The walk is bounded by the depth limit, not by "until a leaf", and every node index is clamped to
// the tree, so no forest image can spin a wavefront or leave its tree.
// grid.y splits the chunks over workgroups (few candidates, many trees); the partial sums meet in a 64-bit atomic add.
// forest_finish_kernel: score = exp2(-(sum / 2^24 / T) / c(psi)) in f64 -> f32, plus the sort keys of closest_to_songs.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "ctx.hpp"
#include "forest.hpp"
#include "playlist_math.hpp"

namespace bg {

namespace {

constexpr uint32_t LEAF = 0xFFFFFFFFu;

// ---- the defined split test (host and device) ----
__host__ __device__ __forceinline__ float forest_split_sum(const float* vals, const uint8_t* dims, uint32_t K, const float* x) {
    float s = 0.0f;
    for (uint32_t k = 0; k < K; k++) s = s + vals[k] * x[dims[k]];
    return s;
}

// ---- counter-based random draws: word (i & 3) of Philox4x32-10(counter = (i / 4 lo, i / 4 hi, tree, 'EIF0'), key = seed) ----
inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

struct Draws {
    uint32_t k0, k1, tree;
    uint64_t i = 0;
    uint32_t buf[4];
    Draws(uint64_t seed, uint32_t t) : k0((uint32_t)seed), k1((uint32_t)(seed >> 32)), tree(t) {}
    uint32_t next() {
        if ((i & 3) == 0) {
            buf[0] = (uint32_t)(i >> 2); buf[1] = (uint32_t)(i >> 34); buf[2] = tree; buf[3] = 0x45494630u;
            philox4x32_10(buf, k0, k1);
        }
        return buf[i++ & 3];
    }
    uint32_t below(uint32_t n) { return (uint32_t)(((uint64_t)next() * n) >> 32); }  // uniform in [0, n)
    double uniform() { return (double)next() * (1.0 / 4294967296.0); }               // [0, 1)
    float normal() {  // Box-Muller; a component that rounds to 0.0f is redrawn
        for (;;) {
            const double u1 = ((double)next() + 1.0) * (1.0 / 4294967296.0), u2 = uniform();
            const float z = (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
            if (z != 0.0f) return z;
        }
    }
};

struct TreeOut {
    std::vector<uint32_t> sample, right, leaf_size, leaf_q;
    std::vector<float> b, vals;
    std::vector<uint8_t> dims;
};

struct Pending { uint32_t lo, hi, depth, parent; };

// one tree: a pure function of (rows, options, seed, t); `perm` is the caller's identity permutation of the rows (restored)
void build_tree(const float* rows, uint32_t d, uint32_t psi, uint32_t limit, uint32_t K, uint64_t seed, uint32_t t,
                std::vector<uint32_t>& perm, TreeOut& o) {
    Draws rng(seed, t);
    const uint32_t n_rows = (uint32_t)perm.size();
    std::vector<std::pair<uint32_t, uint32_t>> swaps(psi);
    for (uint32_t i = 0; i < psi; i++) {  // psi distinct rows: the head of a Fisher-Yates shuffle
        const uint32_t j = i + rng.below(n_rows - i);
        std::swap(perm[i], perm[j]);
        swaps[i] = {i, j};
    }
    o.sample.assign(perm.begin(), perm.begin() + psi);
    for (uint32_t i = psi; i-- > 0;) std::swap(perm[swaps[i].first], perm[swaps[i].second]);

    std::vector<uint32_t> idx(o.sample), tmp(psi);
    std::vector<Pending> stack;
    stack.push_back({0, psi, 0, LEAF});
    uint8_t pick[64], dims[64];
    float vals[64];
    while (!stack.empty()) {
        const Pending nd = stack.back();
        stack.pop_back();
        const uint32_t me = (uint32_t)o.right.size(), m = nd.hi - nd.lo;
        if (nd.parent != LEAF) o.right[nd.parent] = me;  // a right child learns its index when its turn comes (preorder)
        if (m <= 1 || nd.depth == limit) {
            o.right.push_back(LEAF);
            o.leaf_size.push_back(m);
            o.leaf_q.push_back((uint32_t)llround(((double)nd.depth + forest_c(m)) * 16777216.0));
            o.b.push_back(0.0f);
            o.vals.insert(o.vals.end(), K, 0.0f);
            o.dims.insert(o.dims.end(), K, 0);
            continue;
        }
        // the d - K dropped components: the head of a Fisher-Yates shuffle of the dimensions; the kept ones, ascending
        for (uint32_t j = 0; j < d; j++) pick[j] = (uint8_t)j;
        for (uint32_t i = 0; i < d - K; i++) std::swap(pick[i], pick[i + rng.below(d - i)]);
        std::copy(pick + (d - K), pick + d, dims);
        std::sort(dims, dims + K);
        for (uint32_t k = 0; k < K; k++) vals[k] = rng.normal();
        float p[64];
        for (uint32_t k = 0; k < K; k++) {  // intercept point: uniform in the node's box (only the used dimensions matter)
            float lo = rows[(size_t)idx[nd.lo] * d + dims[k]], hi = lo;
            for (uint32_t s = nd.lo + 1; s < nd.hi; s++) {
                const float v = rows[(size_t)idx[s] * d + dims[k]];
                lo = std::min(lo, v);
                hi = std::max(hi, v);
            }
            const float v = (float)((double)lo + rng.uniform() * ((double)hi - (double)lo));
            p[dims[k]] = std::min(std::max(v, lo), hi);
        }
        const float b = forest_split_sum(vals, dims, K, p);
        uint32_t nl = 0, nr = 0;
        for (uint32_t s = nd.lo; s < nd.hi; s++) {  // stable partition with the defined test
            if (forest_split_sum(vals, dims, K, rows + (size_t)idx[s] * d) < b) idx[nd.lo + nl++] = idx[s];
            else tmp[nr++] = idx[s];
        }
        std::copy(tmp.begin(), tmp.begin() + nr, idx.begin() + nd.lo + nl);
        o.right.push_back(LEAF);  // patched when the right child is numbered
        o.leaf_size.push_back(0);
        o.leaf_q.push_back(0);
        o.b.push_back(b);
        o.vals.insert(o.vals.end(), vals, vals + K);
        o.dims.insert(o.dims.end(), dims, dims + K);
        stack.push_back({nd.lo + nl, nd.hi, nd.depth + 1, me});   // right: after the whole left subtree
        stack.push_back({nd.lo, nd.lo + nl, nd.depth + 1, LEAF});  // left: next, i.e. node me + 1
    }
}

}  // namespace

double forest_c(uint32_t m) {
    if (m <= 1) return 0.0;
    if (m == 2) return 1.0;
    const double x = (double)m;
    return 2.0 * (log(x - 1.0) + 0.5772156649) - 2.0 * (x - 1.0) / x;
}

int forest_build(const float* seeds, uint64_t n_seeds, uint32_t d, uint32_t n_trees, uint32_t sample_size, uint32_t max_tree_depth,
                 uint32_t extension_level, uint64_t seed, Forest** out) {
    const char* who = "blissgpu_forest_build";
    if (!seeds || !out) return fail(BLISSGPU_ERR_INVALID, who, "NULL argument");
    if (d == 0 || d > BLISSGPU_FOREST_MAX_D) return fail(BLISSGPU_ERR_INVALID, who, "d must be 1 .. BLISSGPU_FOREST_MAX_D");
    if (n_trees == 0 || n_trees > BLISSGPU_FOREST_MAX_TREES) return fail(BLISSGPU_ERR_INVALID, who, "n_trees must be 1 .. BLISSGPU_FOREST_MAX_TREES");
    if (extension_level > d - 1) return fail(BLISSGPU_ERR_INVALID, who, "extension_level must be 0 .. d - 1");
    if (max_tree_depth > BLISSGPU_FOREST_MAX_DEPTH) return fail(BLISSGPU_ERR_INVALID, who, "max_tree_depth must be 1 .. 128 (0: none)");
    if (n_seeds > 0xFFFFFFFEull) return fail(BLISSGPU_ERR_INVALID, who, "too many seed rows");
    const uint32_t psi = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(sample_size, n_seeds), BLISSGPU_FOREST_MAX_PSI);
    if (psi < 2)
        return fail(BLISSGPU_ERR_INVALID, who, "min(sample_size, n_seeds) < 2: the forest does not work for a single song (c(psi) = 0)");
    for (uint64_t i = 0; i < n_seeds * d; i++)
        if (!std::isfinite(seeds[i])) return fail(BLISSGPU_ERR_INVALID, who, "seed rows must be finite");
    uint32_t limit = max_tree_depth;
    if (!limit)
        while ((1ull << limit) < psi) limit++;  // ceil(log2 psi)
    const uint32_t K = extension_level + 1;

    std::vector<TreeOut> trees(n_trees);
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const unsigned n_thr = (unsigned)std::min<uint64_t>(hw, std::max<uint64_t>(1, ((uint64_t)n_trees * psi) >> 14));
    auto work = [&](unsigned w) {
        std::vector<uint32_t> perm(n_seeds);
        for (uint32_t i = 0; i < n_seeds; i++) perm[i] = i;
        for (uint32_t t = w; t < n_trees; t += n_thr) build_tree(seeds, d, psi, limit, K, seed, t, perm, trees[t]);
    };
    if (n_thr <= 1) {
        work(0);
    } else {
        std::vector<std::thread> pool;
        for (unsigned w = 0; w < n_thr; w++) pool.emplace_back(work, w);
        for (auto& th : pool) th.join();
    }
    uint64_t total = 0;
    for (auto& t : trees) total += t.right.size();
    if (total >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "the forest has 2^32 - 1 nodes or more");

    Forest* f = new Forest();
    f->d = d; f->n_trees = n_trees; f->psi = psi; f->limit = limit; f->ext = extension_level; f->K = K;
    f->stride = (2 + 5 * ((K + 3) / 4)) | 1;
    f->seed = seed;
    f->c_psi = forest_c(psi);
    f->tree_first.resize((size_t)n_trees + 1);
    f->sample.reserve((size_t)n_trees * psi);
    f->right.reserve(total); f->leaf_size.reserve(total); f->leaf_q.reserve(total); f->b.reserve(total);
    f->vals.reserve(total * K); f->dims.reserve(total * K);
    uint32_t first = 0;
    for (uint32_t t = 0; t < n_trees; t++) {
        TreeOut& o = trees[t];
        f->tree_first[t] = first;
        f->sample.insert(f->sample.end(), o.sample.begin(), o.sample.end());
        f->right.insert(f->right.end(), o.right.begin(), o.right.end());  // tree-local; the export adds tree_first
        f->leaf_size.insert(f->leaf_size.end(), o.leaf_size.begin(), o.leaf_size.end());
        f->leaf_q.insert(f->leaf_q.end(), o.leaf_q.begin(), o.leaf_q.end());
        f->b.insert(f->b.end(), o.b.begin(), o.b.end());
        f->vals.insert(f->vals.end(), o.vals.begin(), o.vals.end());
        f->dims.insert(f->dims.end(), o.dims.begin(), o.dims.end());
        first += (uint32_t)o.right.size();
        o = TreeOut();
    }
    f->tree_first[n_trees] = first;
    // chunks of consecutive trees whose device nodes fit the LDS node buffer; an oversized tree is a chunk of its own
    uint64_t largest = 0;
    for (uint32_t t = 0; t < n_trees; t++) largest = std::max<uint64_t>(largest, (uint64_t)(f->tree_first[t + 1] - f->tree_first[t]) * f->stride);
    f->buf_words = largest > FOREST_LDS_WORDS_SMALL ? FOREST_LDS_WORDS_BIG : FOREST_LDS_WORDS_SMALL;
    f->chunk_tree.push_back(0);
    uint64_t words = 0;
    for (uint32_t t = 0; t < n_trees; t++) {
        const uint64_t w = (uint64_t)(f->tree_first[t + 1] - f->tree_first[t]) * f->stride;
        if (words && words + w > f->buf_words) {
            f->chunk_tree.push_back(t);
            words = 0;
        }
        words += w;
    }
    f->chunk_tree.push_back(n_trees);
    *out = f;
    return BLISSGPU_OK;
}

void forest_export(const Forest* f, uint32_t* sample_idx, uint64_t* tree_first, float* normal, float* b, uint32_t* left,
                   uint32_t* right, uint32_t* leaf_size, uint32_t* leaf_q) {
    const size_t N = f->right.size();
    if (sample_idx) memcpy(sample_idx, f->sample.data(), f->sample.size() * sizeof(uint32_t));
    if (tree_first) for (size_t t = 0; t <= f->n_trees; t++) tree_first[t] = f->tree_first[t];
    if (b) memcpy(b, f->b.data(), N * sizeof(float));
    if (leaf_size) memcpy(leaf_size, f->leaf_size.data(), N * sizeof(uint32_t));
    if (leaf_q) memcpy(leaf_q, f->leaf_q.data(), N * sizeof(uint32_t));
    if (normal) memset(normal, 0, N * f->d * sizeof(float));
    for (uint32_t t = 0; t < f->n_trees; t++) {
        const uint32_t first = f->tree_first[t];
        for (uint32_t i = first; i < f->tree_first[t + 1]; i++) {
            const bool leaf = f->right[i] == LEAF;
            if (left) left[i] = leaf ? LEAF : i + 1;
            if (right) right[i] = leaf ? LEAF : first + f->right[i];
            if (normal && !leaf)
                for (uint32_t k = 0; k < f->K; k++) normal[(size_t)i * f->d + f->dims[(size_t)i * f->K + k]] = f->vals[(size_t)i * f->K + k];
        }
    }
}

// the device image of the forest on `device` (uploaded once, under the forest's lock; freed by forest_destroy)
int forest_device_image(Forest* f, int device, hipStream_t st, const ForestImage** out) {
    std::lock_guard<std::mutex> lk(f->mu);
    auto it = f->images.find(device);
    if (it != f->images.end()) { *out = &it->second; return BLISSGPU_OK; }
    const size_t N = f->right.size(), S = f->stride, K = f->K;
    std::vector<uint32_t> img(N * S, 0u);
    for (size_t i = 0; i < N; i++) {
        uint32_t* p = img.data() + i * S;
        const bool leaf = f->right[i] == LEAF;
        if (leaf) p[0] = f->leaf_q[i]; else memcpy(p, &f->b[i], 4);
        p[1] = f->right[i];
        for (size_t k = K; k < 4 * ((K + 3) / 4); k++) p[2 + 5 * (k >> 2)] |= f->d << (8 * (k & 3));  // padding: the zero row
        for (size_t k = 0; k < K; k++) {
            uint32_t* g = p + 2 + 5 * (k >> 2);
            g[0] |= (uint32_t)f->dims[i * K + k] << (8 * (k & 3));
            memcpy(g + 1 + (k & 3), &f->vals[i * K + k], sizeof(float));
        }
    }
    ForestImage im{};
    const size_t n_first = f->tree_first.size(), n_chunk = f->chunk_tree.size();
    hipError_t e = hipMalloc((void**)&im.nodes, std::max<size_t>(1, img.size()) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&im.tree_first, (n_first + n_chunk) * sizeof(uint32_t));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (im.nodes) (void)hipFree(im.nodes);
        return fail(BLISSGPU_ERR_OOM, "hipMalloc(forest)", hipGetErrorString(e));
    }
    im.chunk_tree = im.tree_first + n_first;
    e = hipMemcpyAsync(im.nodes, img.data(), img.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(im.tree_first, f->tree_first.data(), n_first * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(im.chunk_tree, f->chunk_tree.data(), n_chunk * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // img is a local: the copy must be over before it goes
    if (e != hipSuccess) {
        (void)hipFree(im.nodes); (void)hipFree(im.tree_first);
        return fail(BLISSGPU_ERR_HIP, "upload(forest)", hipGetErrorString(e));
    }
    *out = &(f->images[device] = im);
    return BLISSGPU_OK;
}

void forest_destroy(Forest* f) {
    if (!f) return;
    for (auto& kv : f->images) {
        int cur = 0;
        const bool have = hipGetDevice(&cur) == hipSuccess;
        if (hipSetDevice(kv.first) == hipSuccess) { (void)hipFree(kv.second.nodes); (void)hipFree(kv.second.tree_first); }
        if (have) (void)hipSetDevice(cur);
    }
    delete f;
}

// ---- kernels ----
namespace {

// one tree for one candidate: -> the u32 path length of the leaf reached.  `tree` is LDS or global memory.
// G > 0: the node has exactly G groups and the group loop is unrolled, so every fetch of a node is in flight at once.
template <int WG, int G>
__device__ __forceinline__ uint32_t forest_walk_tree(const uint32_t* tree, uint32_t n_nodes, uint32_t K, uint32_t stride,
                                                     uint32_t limit, const float* feat, uint32_t lane) {
    uint32_t node = 0;
    for (uint32_t step = 0; step < limit; step++) {
        const uint32_t* p = tree + node * stride;
        uint32_t r = p[1];
        uint32_t dw[G ? G : 1];
#pragma unroll
        for (int g = 0; g < G; g++) dw[g] = p[2 + 5 * g];  // with the header, before the leaf test: one round trip less per level
        asm volatile("" : "+v"(r));                        // (the empty statements keep the compiler from sinking these
#pragma unroll
        for (int g = 0; g < G; g++) asm volatile("" : "+v"(dw[g]));  //  fetches behind the test)
        if (r == LEAF) break;
        float s = 0.0f;
        if (G) {  // every fetch of the node in flight at once, then the chain of adds in ascending dimension
            float v[G ? G : 1][4], x[G ? G : 1][4];
#pragma unroll
            for (int g = 0; g < G; g++)
#pragma unroll
                for (int i = 0; i < 4; i++) v[g][i] = __uint_as_float(p[3 + 5 * g + i]);
#pragma unroll
            for (int g = 0; g < G; g++)
#pragma unroll
                for (int i = 0; i < 4; i++) x[g][i] = feat[((dw[g] >> (8 * i)) & 0xFFu) * WG + lane];
#pragma unroll
            for (int g = 0; g < G; g++)
#pragma unroll
                for (int i = 0; i < 4; i++) s = s + v[g][i] * x[g][i];
        } else {
            for (uint32_t k = 0; k < K; k += 4) {
                const uint32_t* q = p + 2 + 5 * (k >> 2);
                const uint32_t dw = q[0];
#pragma unroll
                for (int i = 0; i < 4; i++) s = s + __uint_as_float(q[1 + i]) * feat[((dw >> (8 * i)) & 0xFFu) * WG + lane];
            }
        }
        node = (s < __uint_as_float(p[0])) ? node + 1 : r;
        node = min(node, n_nodes - 1);
    }
    return tree[node * stride];
}

template <bool STAGE, int WG, int G>
__global__ __launch_bounds__(WG) void forest_walk_kernel(
    const float* __restrict__ X, uint32_t n, uint32_t d, const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ tree_first,
    const uint32_t* __restrict__ chunk_tree, uint32_t n_chunks, uint32_t chunks_per_split, uint32_t K, uint32_t stride,
    uint32_t limit, uint32_t buf_words, unsigned long long* __restrict__ sum, int add) {
    extern __shared__ uint32_t forest_lds[];
    float* feat = reinterpret_cast<float*>(forest_lds);  // [d + 1][WG], row d = +0.0 (the padding of a node's last group)
    uint32_t* buf = forest_lds + (d + 1) * WG;           // [buf_words]
    const uint32_t tid = threadIdx.x;
    const uint64_t c0 = (uint64_t)blockIdx.x * WG;
    const uint32_t rows = (uint32_t)min((uint64_t)WG, (uint64_t)n - c0);
    feat[d * WG + tid] = 0.0f;
    for (uint32_t i = tid; i < d * WG; i += WG) {  // coalesced read, transposed write; idle lanes walk zeros
        const uint32_t r = i / d, j = i - r * d;
        feat[j * WG + r] = r < rows ? X[c0 * d + i] : 0.0f;
    }
    __syncthreads();
    unsigned long long acc = 0;
    const uint32_t ch0 = blockIdx.y * chunks_per_split, ch1 = min(n_chunks, ch0 + chunks_per_split);
    for (uint32_t ch = ch0; ch < ch1; ch++) {
        const uint32_t t0 = chunk_tree[ch], t1 = chunk_tree[ch + 1];
        const uint32_t n0 = tree_first[t0];
        const uint64_t words = (uint64_t)(tree_first[t1] - n0) * stride;
        const bool staged = STAGE && words <= buf_words;
        if (staged) {
            __syncthreads();  // the previous chunk's walks are over
            for (uint32_t i = tid; i < (uint32_t)words; i += WG) buf[i] = nodes[(size_t)n0 * stride + i];
            __syncthreads();
        }
        for (uint32_t t = t0; t < t1; t++) {
            const uint32_t first = tree_first[t], cnt = tree_first[t + 1] - first;
            if (cnt == 0) continue;
            if (staged) acc += forest_walk_tree<WG, G>(buf + (first - n0) * stride, cnt, K, stride, limit, feat, tid);
            else acc += forest_walk_tree<WG, G>(nodes + (size_t)first * stride, cnt, K, stride, limit, feat, tid);
        }
    }
    if (tid < rows) {
        if (add) atomicAdd(&sum[c0 + tid], acc);
        else sum[c0 + tid] = acc;
    }
}

__global__ __launch_bounds__(256) void forest_finish_kernel(const unsigned long long* __restrict__ sum, uint32_t n, double n_trees,
                                                            double c_psi, float* __restrict__ score, uint32_t* __restrict__ keys,
                                                            uint32_t* __restrict__ idx) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const double e = (double)sum[j] / 16777216.0 / n_trees;
    const float v = (float)exp2(-e / c_psi);
    if (score) score[j] = v;
    if (keys) {
        keys[j] = f32_key(v);
        idx[j] = j;
    }
}

}  // namespace

static int forest_wg(const Forest* f) { return f->buf_words == FOREST_LDS_WORDS_BIG ? 512 : 256; }

uint32_t forest_split_plan(const Forest* f, uint64_t n, int n_cus, int64_t forced) {
    const uint32_t n_chunks = (uint32_t)f->chunk_tree.size() - 1;
    uint64_t split = 1;
    if (forced > 0) {
        split = (uint64_t)forced;
    } else {  // about sixteen wavefronts per CU before the trees stay whole
        const uint64_t wg = forest_wg(f), blocks = (n + wg - 1) / wg, want = (1024 / wg) * (uint64_t)std::max(1, n_cus);
        if (blocks < want) split = (want + blocks - 1) / blocks;
    }
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(split, n_chunks), 65535));
}

template <bool STAGE, int WG, int G>
static hipError_t forest_launch(const Forest* f, const ForestImage& im, const float* X, uint32_t n, uint32_t n_split,
                                unsigned long long* sum, hipStream_t st) {
    const uint32_t n_chunks = (uint32_t)f->chunk_tree.size() - 1;
    const uint32_t per = (n_chunks + n_split - 1) / n_split;
    const dim3 grid((uint32_t)(((uint64_t)n + WG - 1) / WG), (n_chunks + per - 1) / per);
    const size_t lds = ((size_t)(f->d + 1) * WG + f->buf_words) * sizeof(uint32_t);
    if (lds > 48 * 1024) {  // beyond the default dynamic LDS limit
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&forest_walk_kernel<STAGE, WG, G>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((forest_walk_kernel<STAGE, WG, G>), grid, dim3(WG), lds, st, X, n, f->d, im.nodes, im.tree_first, im.chunk_tree,
                       n_chunks, per, f->K, f->stride, f->limit, f->buf_words, sum, (int)(grid.y > 1));
    return hipGetLastError();
}

// the staged form is instantiated per group count (1 .. 8, i.e. extension_level + 1 <= 32); the global form loops
template <int WG>
static hipError_t forest_launch_wg(const Forest* f, const ForestImage& im, const float* X, uint32_t n, uint32_t n_split, bool stage,
                                   unsigned long long* sum, hipStream_t st) {
    if (!stage) return forest_launch<false, WG, 0>(f, im, X, n, n_split, sum, st);
    switch ((f->K + 3) / 4) {
        case 1: return forest_launch<true, WG, 1>(f, im, X, n, n_split, sum, st);
        case 2: return forest_launch<true, WG, 2>(f, im, X, n, n_split, sum, st);
        case 3: return forest_launch<true, WG, 3>(f, im, X, n, n_split, sum, st);
        case 4: return forest_launch<true, WG, 4>(f, im, X, n, n_split, sum, st);
        case 5: return forest_launch<true, WG, 5>(f, im, X, n, n_split, sum, st);
        case 6: return forest_launch<true, WG, 6>(f, im, X, n, n_split, sum, st);
        case 7: return forest_launch<true, WG, 7>(f, im, X, n, n_split, sum, st);
        default: return forest_launch<true, WG, 8>(f, im, X, n, n_split, sum, st);
    }
}

hipError_t launch_forest_walk(const Forest* f, const ForestImage& im, const float* X, uint32_t n, uint32_t n_split, bool stage,
                              unsigned long long* sum, hipStream_t st) {
    return forest_wg(f) == 512 ? forest_launch_wg<512>(f, im, X, n, n_split, stage, sum, st)
                               : forest_launch_wg<256>(f, im, X, n, n_split, stage, sum, st);
}

void launch_forest_finish(const Forest* f, const unsigned long long* sum, uint32_t n, float* score, uint32_t* keys, uint32_t* idx,
                          hipStream_t st) {
    hipLaunchKernelGGL(forest_finish_kernel, dim3((uint32_t)(((uint64_t)n + 255) / 256)), dim3(256), 0, st, sum, n, (double)f->n_trees, f->c_psi, score,
                       keys, idx);
}

}  // namespace bg
