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
#include <atomic>
#include <chrono>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "ctx.hpp"
#include "forest.hpp"
#include "knn_list.hpp"
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

// first tree of every chunk of consecutive trees whose device nodes fit `buf_words`, and the end
static void forest_chunks(const Forest* f, uint32_t buf_words, std::vector<uint32_t>& chunk_tree) {
    chunk_tree.clear();
    chunk_tree.push_back(0);
    uint64_t words = 0;
    for (uint32_t t = 0; t < f->n_trees; t++) {
        const uint64_t w = (uint64_t)(f->tree_first[t + 1] - f->tree_first[t]) * f->stride;
        if (words && words + w > buf_words) {
            chunk_tree.push_back(t);
            words = 0;
        }
        words += w;
    }
    chunk_tree.push_back(f->n_trees);
}

int forest_build(const float* seeds, uint64_t n_seeds, uint32_t d, uint32_t n_trees, uint32_t sample_size, uint32_t max_tree_depth,
                 uint32_t extension_level, uint64_t seed, Forest** out, unsigned max_threads) {
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
    const unsigned hw = std::max(1u, std::min(std::min(16u, max_threads), std::thread::hardware_concurrency()));
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
    forest_chunks(f, f->buf_words, f->chunk_tree);
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

// the nodes of the forest in the device layout (see the head of this file): right.size() * stride words at dst
static void forest_pack_nodes(const Forest* f, uint32_t* dst) {
    const size_t N = f->right.size(), S = f->stride, K = f->K;
    std::fill(dst, dst + N * S, 0u);
    for (size_t i = 0; i < N; i++) {
        uint32_t* p = dst + i * S;
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
}

// the device image of the forest on `device` (uploaded once, under the forest's lock; freed by forest_destroy)
int forest_device_image(Forest* f, int device, hipStream_t st, const ForestImage** out) {
    std::lock_guard<std::mutex> lk(f->mu);
    auto it = f->images.find(device);
    if (it != f->images.end()) { *out = &it->second; return BLISSGPU_OK; }
    std::vector<uint32_t> img(f->right.size() * (size_t)f->stride);
    forest_pack_nodes(f, img.data());
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

// score = exp2(-(sum / 2^24 / T) / c(psi)) in f64 -> f32: the one expression of every kernel that turns a path sum into a score
__device__ __forceinline__ float forest_score_of(unsigned long long sum, double n_trees, double c_psi) {
    const double e = (double)sum / 16777216.0 / n_trees;
    return (float)exp2(-e / c_psi);
}

__global__ __launch_bounds__(256) void forest_finish_kernel(const unsigned long long* __restrict__ sum, uint32_t n, double n_trees,
                                                            double c_psi, float* __restrict__ score, uint32_t* __restrict__ keys,
                                                            uint32_t* __restrict__ idx) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const float v = forest_score_of(sum[j], n_trees, c_psi);
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


// ---- one forest per seed GROUP: the k lowest scores of every group, no groups x candidates array ----
// A batch of consecutive groups travels as ONE image: descriptors | list offsets | items | tree_first and chunk lists of every
// group | nodes (the layout above; stride and K are the same for every group, because the options are shared).
// group_forest_scan_kernel<G>: a workgroup of 256 lanes takes one ITEM, one group x a range of 256-candidate blocks.  Per block:
// the transposed feature block (feat[j * 256 + lane], zero row d), the 256-bit mask of the group's skipped candidates, then
// every tree of the group through the LDS node buffer chunk by chunk (a chunk beyond the buffer walks from global memory), the
// whole u64 sum in the lane -- one workgroup walks all trees of its group for its candidates, so no atomic is needed.  The sum
// becomes the score (forest_score_of), the score the key (f32_key(score) << 32) | index, and every wavefront pushes its 64 keys
// into a threshold buffer of its own: four partial lists per item, merged with the other items' by group_knn_merge_kernel.
namespace {

constexpr int GF_WG = 256;
constexpr uint32_t GF_SKIP_LDS = 1024;  // skip entries of the group held in LDS (a larger group reads the rest from global memory)
constexpr uint32_t GF_LISTS = GF_WG / 64;

struct GroupForestDesc {
    uint64_t node_word;    // first word of the group's nodes in the batch's node array
    double c_psi;
    uint32_t tree_first;   // the group's tree_first[0 .. n_trees] (node indices inside the group) in the table
    uint32_t chunk_first;  // the group's chunk list [0 .. n_chunks] (tree indices) in the table
    uint32_t n_chunks, n_trees, limit;
    uint32_t seed_first, n_seeds;  // the group's rows of skip
    uint32_t pad;
};
static_assert(sizeof(GroupForestDesc) == 48, "twelve words");

struct GroupForestItem {
    uint32_t group;           // inside the batch
    uint32_t blk_lo, blk_hi;  // 256-candidate blocks [blk_lo, blk_hi)
    uint32_t split;           // the item writes the lists list_off[group] + 4 split .. + 4
};

template <int G>
__global__ __launch_bounds__(GF_WG) void group_forest_scan_kernel(
    const float* __restrict__ X, uint32_t n, uint32_t d, const GroupForestDesc* __restrict__ descs,
    const GroupForestItem* __restrict__ items, const uint32_t* __restrict__ table, const uint32_t* __restrict__ nodes, uint32_t K,
    uint32_t stride, const uint32_t* __restrict__ skip, uint32_t k, uint32_t cap, const uint32_t* __restrict__ list_off,
    unsigned long long* __restrict__ part, uint32_t* bad_flag) {
    constexpr uint32_t WG = GF_WG;
    extern __shared__ __attribute__((aligned(16))) unsigned long long gf_lds[];
    unsigned long long* s_keys = gf_lds;                                        // [4][cap]
    float* feat = reinterpret_cast<float*>(gf_lds + (size_t)GF_LISTS * cap);     // [d + 1][WG], row d = +0.0
    uint32_t* buf = reinterpret_cast<uint32_t*>(feat) + (d + 1) * WG;           // [FOREST_LDS_WORDS_SMALL]
    uint32_t* s_skip = buf + FOREST_LDS_WORDS_SMALL;                            // [GF_SKIP_LDS]
    uint32_t* s_mask = s_skip + GF_SKIP_LDS;                                    // [8]
    const uint32_t tid = threadIdx.x;
    const int lane = lane_id(), wave = wave_id();
    const GroupForestItem it = items[blockIdx.x];
    const GroupForestDesc ds = descs[it.group];
    const uint32_t* tree_first = table + ds.tree_first;
    const uint32_t* chunk_tree = table + ds.chunk_first;
    const uint32_t* gnodes = nodes + ds.node_word;
    const uint32_t n_skip = skip ? ds.n_seeds : 0u;
    for (uint32_t e = tid; e < n_skip && e < GF_SKIP_LDS; e += WG) s_skip[e] = skip[ds.seed_first + e];
    KnnList list{s_keys + (size_t)wave * cap, 0u, KNN_NONE};
    for (uint32_t blk = it.blk_lo; blk < it.blk_hi; blk++) {
        const uint64_t c0 = (uint64_t)blk * WG;
        const uint32_t rows = (uint32_t)min((uint64_t)WG, (uint64_t)n - c0);
        __syncthreads();  // the previous block's walks and mask reads are over (first block: the skip list is in)
        feat[d * WG + tid] = 0.0f;
        for (uint32_t i = tid; i < d * WG; i += WG) {  // coalesced read, transposed write; idle lanes walk zeros
            const uint32_t r = i / d, j = i - r * d;
            feat[j * WG + r] = r < rows ? X[c0 * d + i] : 0.0f;
        }
        if (tid < 8u) s_mask[tid] = 0u;
        __syncthreads();
        for (uint32_t e = tid; e < n_skip; e += WG) {
            const uint32_t s = e < GF_SKIP_LDS ? s_skip[e] : skip[ds.seed_first + e];
            if (s == LEAF) continue;                     // 0xFFFFFFFF skips nothing
            if (s >= n) atomicOr(bad_flag, 1u);          // reported to the host by the entry point
            else if ((uint64_t)s >= c0 && (uint64_t)s - c0 < WG) atomicOr(&s_mask[((uint32_t)(s - c0)) >> 5], 1u << ((s - (uint32_t)c0) & 31u));
        }
        unsigned long long acc = 0;
        for (uint32_t ch = 0; ch < ds.n_chunks; ch++) {
            const uint32_t t0 = chunk_tree[ch], t1 = chunk_tree[ch + 1];
            const uint32_t n0 = tree_first[t0];
            const uint64_t words = (uint64_t)(tree_first[t1] - n0) * stride;
            const bool staged = words <= FOREST_LDS_WORDS_SMALL;
            if (staged) {
                __syncthreads();  // the previous chunk's walks are over
                for (uint32_t i = tid; i < (uint32_t)words; i += WG) buf[i] = gnodes[(size_t)n0 * stride + i];
                __syncthreads();
            }
            for (uint32_t t = t0; t < t1; t++) {
                const uint32_t first = tree_first[t], cnt = tree_first[t + 1] - first;
                if (cnt == 0) continue;
                if (staged) acc += forest_walk_tree<GF_WG, G>(buf + (first - n0) * stride, cnt, K, stride, ds.limit, feat, tid);
                else acc += forest_walk_tree<GF_WG, G>(gnodes + (size_t)first * stride, cnt, K, stride, ds.limit, feat, tid);
            }
        }
        __syncthreads();  // the mask is complete
        const bool skipped = ((s_mask[tid >> 5] >> (tid & 31u)) & 1u) != 0u;
        const bool valid = tid < rows && !skipped;  // a skipped candidate's score is never looked at
        const float v = forest_score_of(acc, (double)ds.n_trees, ds.c_psi);
        const unsigned long long key = ((unsigned long long)f32_key(v) << 32) | (uint32_t)(c0 + tid);
        list.push(valid && key < list.thr, key, k, cap, lane);
    }
    // the sorted k best of this wavefront's candidates (padded when it held fewer)
    knn_sort(list.buf, list.cnt, cap, lane);
    unsigned long long* dst = part + ((uint64_t)list_off[it.group] + (uint64_t)it.split * GF_LISTS + (uint64_t)wave) * (uint64_t)k;
    for (uint32_t i = (uint32_t)lane; i < k; i += 64u) dst[i] = list.buf[i];
}

template <int G>
hipError_t group_forest_launch(uint32_t n_items, size_t lds, hipStream_t st, const float* X, uint32_t n, uint32_t d,
                               const GroupForestDesc* descs, const GroupForestItem* items, const uint32_t* table, const uint32_t* nodes,
                               uint32_t K, uint32_t stride, const uint32_t* skip, uint32_t k, uint32_t cap, const uint32_t* list_off,
                               unsigned long long* part, uint32_t* bad_flag) {
    if (lds > 48 * 1024) {  // beyond the default dynamic LDS limit
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&group_forest_scan_kernel<G>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((group_forest_scan_kernel<G>), dim3(n_items), dim3(GF_WG), lds, st, X, n, d, descs, items, table, nodes, K, stride,
                       skip, k, cap, list_off, part, bad_flag);
    return hipGetLastError();
}

uint32_t group_forest_psi(uint64_t count, uint32_t sample_size) {
    return (uint32_t)std::min<uint64_t>(std::min<uint64_t>(sample_size, count), BLISSGPU_FOREST_MAX_PSI);
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// a batch on the host: built, laid out and packed into the staging buffer
struct GroupForestBatch {
    uint32_t n_groups = 0, n_items = 0;
    size_t list_word = 0, item_word = 0, table_word = 0, node_word = 0, total_words = 0;
    uint64_t n_lists = 0;
};

}  // namespace

uint64_t group_forest_nodes(uint64_t count, uint32_t n_trees, uint32_t sample_size) {
    const uint64_t psi = group_forest_psi(count, sample_size);
    return psi < 2 ? 1 : (uint64_t)n_trees * (2 * psi - 1);
}

uint64_t group_forest_budget(uint64_t workspace_bytes, uint32_t extension_level) {
    const uint64_t stride = (2 + 5 * ((extension_level + 1 + 3) / 4)) | 1;
    return std::max<uint64_t>(1, std::min<uint64_t>(workspace_bytes / 8, 64ull << 20) / (stride * sizeof(uint32_t)));
}

std::vector<uint64_t> group_forest_batches(const uint64_t* off, uint64_t n_groups, uint32_t n_trees, uint32_t sample_size,
                                           uint64_t budget) {
    std::vector<uint64_t> first;
    uint64_t in_batch = 0;
    for (uint64_t g = 0; g < n_groups; g++) {
        const uint64_t nodes = group_forest_nodes(off[g + 1] - off[g], n_trees, sample_size);
        if (g == 0 || in_batch + nodes > budget) {
            first.push_back(g);
            in_batch = 0;
        }
        in_batch += nodes;
    }
    first.push_back(n_groups);
    return first;
}

int group_forest_run(blissgpu_ctx* c, const char* who, const float* h_seeds, const uint64_t* off, uint64_t n_groups,
                     const float* d_cand, uint64_t n, const GroupForestOpts& o, const uint32_t* d_skip, uint32_t k, uint32_t* d_idx,
                     float* d_score, int32_t* d_status, int32_t* h_status) {
    const uint32_t d = o.d, K = o.extension_level + 1, stride = (2 + 5 * ((K + 3) / 4)) | 1;
    std::vector<int32_t> status(n_groups);
    for (uint64_t g = 0; g < n_groups; g++)
        status[g] = group_forest_psi(off[g + 1] - off[g], o.sample_size) < 2 ? BLISSGPU_GROUP_TOO_FEW_SEEDS : BLISSGPU_GROUP_OK;
    if (h_status) std::copy(status.begin(), status.end(), h_status);
    const uint64_t budget = c->forest_group_nodes > 0 ? (uint64_t)c->forest_group_nodes : group_forest_budget(c->ws_limit, o.extension_level);
    const std::vector<uint64_t> batch_first = group_forest_batches(off, n_groups, o.n_trees, o.sample_size, budget);
    const size_t n_batches = batch_first.size() - 1;
    GroupKnnPlan kp;  // (the merge launch reads cap only)
    uint32_t p2 = 64;
    while (p2 < k) p2 <<= 1;
    kp.cap = 2 * p2;  // a power of two with cap - k >= 64 (see knn_plan)
    const uint64_t n_blocks = (n + GF_WG - 1) / GF_WG;
    const size_t lds = (size_t)GF_LISTS * kp.cap * sizeof(unsigned long long) +
                       ((size_t)(d + 1) * GF_WG + FOREST_LDS_WORDS_SMALL + GF_SKIP_LDS + 8) * sizeof(uint32_t);
    for (int s = 0; s < 2; s++)
        if (!c->gf_ev[s]) HIP_TRY(hipEventCreateWithFlags(&c->gf_ev[s], hipEventDisableTiming));
    int rc = c->pl_sync.ensure(4);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->pl_sync.p, 0, 4 * sizeof(uint32_t), c->stream));  // [3]: a skip entry >= n
    if (d_status && n_groups) HIP_TRY(hipMemcpyAsync(d_status, status.data(), n_groups * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    c->gf_build_ms = c->gf_wait_ms = 0.0;
    c->gf_batches = n_batches;
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    bool slot_used[2] = {false, false};
    // the buffers take their planned sizes before the first batch: a buffer that grows later is freed first, and hipFree waits
    // for the device, which would serialise the batches in flight.  (A forest can exceed its planned nodes -- see the plan --
    // so the per-batch ensure() below stays.)
    {
        size_t img_words = 0, part_keys = 0;
        const uint64_t want = 8ull * (uint64_t)std::max(1, c->n_cus);
        for (size_t b = 0; b < n_batches; b++) {
            uint64_t nodes = 0, act = 0;
            for (uint64_t g = batch_first[b]; g < batch_first[b + 1]; g++)
                if (n && status[g] == BLISSGPU_GROUP_OK) {
                    nodes += group_forest_nodes(off[g + 1] - off[g], o.n_trees, o.sample_size);
                    act++;
                }
            const uint64_t bpi = std::max<uint64_t>(1, std::min<uint64_t>(std::max<uint64_t>(1, n_blocks), (act * n_blocks + want - 1) / want));
            const uint64_t splits = (n_blocks + bpi - 1) / bpi, nb = batch_first[b + 1] - batch_first[b];
            img_words = std::max<size_t>(img_words, (size_t)(nodes * stride + nb * (sizeof(GroupForestDesc) / 4 + 1) + act * splits * 4 +
                                                             act * ((uint64_t)o.n_trees + 1) * 2 + 8));
            part_keys = std::max<size_t>(part_keys, (size_t)(act * splits * GF_LISTS * k));
        }
        for (int s = 0; s < 2 && !rc; s++)
            if (s == 0 || n_batches > 1) {
                rc = c->gf_img[s].ensure(std::max<size_t>(1, img_words));
                if (!rc) rc = c->gf_host[s].ensure(std::max<size_t>(1, img_words));
            }
        if (!rc) rc = c->pl_tmp.ensure(std::max<size_t>(8, part_keys * sizeof(unsigned long long)));
        if (rc) return rc;
    }

    // build batch b on the host into staging buffer b & 1: forests on up to 16 threads dealt out over GROUPS
    auto build = [&](size_t b, GroupForestBatch& B) -> int {
        const auto t0 = std::chrono::steady_clock::now();
        const uint64_t g0 = batch_first[b], g1 = batch_first[b + 1];
        const uint32_t nb = (uint32_t)(g1 - g0);
        std::vector<Forest*> fs(nb, nullptr);
        std::vector<std::vector<uint32_t>> chunks(nb);
        std::vector<uint32_t> active;
        for (uint32_t i = 0; i < nb; i++)
            if (n && status[g0 + i] == BLISSGPU_GROUP_OK) active.push_back(i);
        std::atomic<uint32_t> next{0};
        std::atomic<int> first_rc{BLISSGPU_OK};
        std::string first_err;
        std::mutex err_mu;
        auto run_pool = [&](const std::function<void(uint32_t)>& fn) {
            next = 0;
            auto work = [&]() {
                for (uint32_t a; (a = next.fetch_add(1)) < active.size();) fn(active[a]);
            };
            const unsigned n_thr = (unsigned)std::min<size_t>(hw, active.size());
            if (n_thr <= 1) { work(); return; }
            std::vector<std::thread> pool;
            for (unsigned w = 0; w < n_thr; w++) pool.emplace_back(work);
            for (auto& th : pool) th.join();
        };
        run_pool([&](uint32_t i) {
            const uint64_t a = off[g0 + i];
            const int r = forest_build(h_seeds + a * d, off[g0 + i + 1] - a, d, o.n_trees, o.sample_size, o.max_tree_depth,
                                       o.extension_level, o.seed, &fs[i], 1u);
            if (r) {  // (the error text is thread-local: carry it to the caller's thread)
                std::lock_guard<std::mutex> lk(err_mu);
                if (first_rc == BLISSGPU_OK) { first_rc = r; first_err = blissgpu_last_error(); }
                return;
            }
            forest_chunks(fs[i], FOREST_LDS_WORDS_SMALL, chunks[i]);
        });
        auto drop = [&]() { for (Forest* f : fs) delete f; };
        if (first_rc != BLISSGPU_OK) { drop(); return fail(first_rc, who, first_err.c_str()); }
        // the layout: descriptors | list offsets | items | tables | nodes
        const uint64_t want = 8ull * (uint64_t)std::max(1, c->n_cus);
        const uint64_t all_blocks = (uint64_t)active.size() * n_blocks;
        const uint64_t bpi = std::max<uint64_t>(1, std::min<uint64_t>(std::max<uint64_t>(1, n_blocks), (all_blocks + want - 1) / want));
        const uint64_t splits = (n_blocks + bpi - 1) / bpi;
        if ((uint64_t)active.size() * splits > 0x7FFFFFFFull) { drop(); return fail(BLISSGPU_ERR_INVALID, who, "too many work items in a batch"); }
        B = GroupForestBatch();
        B.n_groups = nb;
        B.n_items = (uint32_t)(active.size() * splits);
        B.list_word = (size_t)nb * (sizeof(GroupForestDesc) / 4);
        B.item_word = B.list_word + nb + 1;
        B.table_word = B.item_word + (size_t)B.n_items * (sizeof(GroupForestItem) / 4);
        std::vector<size_t> tf_at(nb, 0), ch_at(nb, 0), node_at(nb, 0);
        size_t at = 0;
        for (uint32_t i : active) {
            tf_at[i] = at; at += fs[i]->tree_first.size();
            ch_at[i] = at; at += chunks[i].size();
        }
        if (at > 0xFFFFFFFFull) { drop(); return fail(BLISSGPU_ERR_INVALID, who, "2^32 trees or more in a batch"); }
        B.node_word = (B.table_word + at + 3) & ~(size_t)3;
        size_t words = 0;
        for (uint32_t i : active) { node_at[i] = words; words += fs[i]->right.size() * (size_t)stride; }
        B.total_words = B.node_word + words;
        int r = c->gf_host[b & 1].ensure(B.total_words);
        if (r) { drop(); return r; }
        uint32_t* h = c->gf_host[b & 1].p;
        GroupForestDesc* descs = reinterpret_cast<GroupForestDesc*>(h);
        uint32_t* list_off = h + B.list_word;
        GroupForestItem* items = reinterpret_cast<GroupForestItem*>(h + B.item_word);
        memset(h, 0, B.node_word * sizeof(uint32_t));
        uint32_t lists = 0, item = 0;
        for (uint32_t i = 0; i < nb; i++) {
            list_off[i] = lists;
            if (!fs[i]) continue;
            GroupForestDesc& ds = descs[i];
            ds.node_word = node_at[i];
            ds.c_psi = fs[i]->c_psi;
            ds.tree_first = (uint32_t)tf_at[i];
            ds.chunk_first = (uint32_t)ch_at[i];
            ds.n_chunks = (uint32_t)chunks[i].size() - 1;
            ds.n_trees = fs[i]->n_trees;
            ds.limit = fs[i]->limit;
            ds.seed_first = (uint32_t)off[g0 + i];
            ds.n_seeds = (uint32_t)(off[g0 + i + 1] - off[g0 + i]);
            std::copy(fs[i]->tree_first.begin(), fs[i]->tree_first.end(), h + B.table_word + tf_at[i]);
            std::copy(chunks[i].begin(), chunks[i].end(), h + B.table_word + ch_at[i]);
            for (uint64_t s = 0; s < splits; s++)
                items[item++] = {i, (uint32_t)(s * bpi), (uint32_t)std::min<uint64_t>(n_blocks, (s + 1) * bpi), (uint32_t)s};
            lists += (uint32_t)(splits * GF_LISTS);
        }
        list_off[nb] = lists;
        B.n_lists = lists;
        run_pool([&](uint32_t i) {
            forest_pack_nodes(fs[i], h + B.node_word + node_at[i]);
            delete fs[i];
            fs[i] = nullptr;
        });
        c->gf_build_ms += ms_since(t0);
        return BLISSGPU_OK;
    };

    // upload + scan + merge of batch b on the context's stream: two launches whatever the group sizes
    auto enqueue = [&](size_t b, const GroupForestBatch& B) -> int {
        int r = c->gf_img[b & 1].ensure(std::max<size_t>(1, B.total_words));
        if (!r) r = c->pl_tmp.ensure(std::max<size_t>(8, (size_t)B.n_lists * k * sizeof(unsigned long long)));
        if (r) return r;
        const uint32_t* img = c->gf_img[b & 1].p;
        HIP_TRY(hipMemcpyAsync(c->gf_img[b & 1].p, c->gf_host[b & 1].p, B.total_words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipEventRecord(c->gf_ev[b & 1], c->stream));
        slot_used[b & 1] = true;
        const GroupForestDesc* descs = reinterpret_cast<const GroupForestDesc*>(img);
        const uint32_t* list_off = img + B.list_word;
        const GroupForestItem* items = reinterpret_cast<const GroupForestItem*>(img + B.item_word);
        unsigned long long* part = reinterpret_cast<unsigned long long*>(c->pl_tmp.p);
        const uint64_t g0 = batch_first[b];
        if (B.n_items) {
            Prof p(c, KX_GROUP_FOREST_SCAN);
            hipError_t e = hipSuccess;
#define GF_GO(GG) e = group_forest_launch<GG>(B.n_items, lds, c->stream, d_cand, (uint32_t)n, d, descs, items, img + B.table_word, \
                                              img + B.node_word, K, stride, d_skip, k, kp.cap, list_off, part, c->pl_sync.p + 3)
            switch ((K + 3) / 4) {
                case 1: GF_GO(1); break;
                case 2: GF_GO(2); break;
                case 3: GF_GO(3); break;
                case 4: GF_GO(4); break;
                case 5: GF_GO(5); break;
                case 6: GF_GO(6); break;
                case 7: GF_GO(7); break;
                default: GF_GO(8); break;
            }
#undef GF_GO
            HIP_TRY(e);
        }
        {
            Prof p(c, K_GROUP_KNN_MERGE);
            launch_group_knn_merge(part, list_off, B.n_groups, k, kp, d_idx + g0 * k, d_score ? d_score + g0 * k : nullptr, c->stream);
        }
        HIP_TRY(hipGetLastError());
        return BLISSGPU_OK;
    };

    // batch b + 1 is built while the device scores batch b; a staging buffer is written again once its copy has left it
    auto build_when_free = [&](size_t b, GroupForestBatch& B) -> int {
        if (slot_used[b & 1]) {
            const auto t0 = std::chrono::steady_clock::now();
            HIP_TRY(hipEventSynchronize(c->gf_ev[b & 1]));
            c->gf_wait_ms += ms_since(t0);
        }
        return build(b, B);
    };
    GroupForestBatch cur, nxt;
    if (n_batches) rc = build_when_free(0, cur);
    for (size_t b = 0; !rc && b < n_batches; b++) {
        rc = enqueue(b, cur);
        if (!rc && b + 1 < n_batches) {
            rc = build_when_free(b + 1, nxt);
            cur = nxt;
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t se = hipStreamSynchronize(c->stream);  // the staging buffers and `status` are the call's
    c->gf_wait_ms += ms_since(t0);
    if (rc) return rc;
    HIP_TRY(se);
    uint32_t flags[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpy(flags, c->pl_sync.p, sizeof(flags), hipMemcpyDeviceToHost));
    if (flags[3]) return fail(BLISSGPU_ERR_INVALID, who, "skip entries must be < n or 0xFFFFFFFF");
    return BLISSGPU_OK;
}

}  // namespace bg
