// forest.hpp -- the extended isolation forest behind the blissgpu_forest_* entry points (kernels_forest.hip builds, exports,
// uploads and scores it; blissgpu.hip holds the C ABI).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <vector>

struct blissgpu_ctx;

namespace bg {

// LDS node buffer of forest_walk_kernel: trees are staged in chunks that fit it.  SMALL goes with 256 candidates per
// workgroup, BIG (chosen when the largest tree does not fit SMALL) with 512
constexpr uint32_t FOREST_LDS_WORDS_SMALL = 4096, FOREST_LDS_WORDS_BIG = 8192;

struct ForestImage {  // the forest on one device
    uint32_t* nodes = nullptr;       // [n_nodes][stride], see kernels_forest.hip
    uint32_t* tree_first = nullptr;  // [n_trees + 1] first node of every tree
    uint32_t* chunk_tree = nullptr;  // [n_chunks + 1] first tree of every chunk (same allocation as tree_first)
};

struct Forest {
    uint32_t d = 0, n_trees = 0, psi = 0, limit = 0, ext = 0, K = 0, stride = 0, buf_words = 0;
    uint64_t seed = 0;
    double c_psi = 0.0;
    std::vector<uint32_t> sample;      // [n_trees][psi] seed rows of every tree
    std::vector<uint32_t> tree_first;  // [n_trees + 1]
    std::vector<uint32_t> chunk_tree;  // [n_chunks + 1]
    // nodes, preorder inside a tree (left child = node + 1)
    std::vector<uint32_t> right;       // tree-local index of the right child, 0xFFFFFFFF on a leaf
    std::vector<uint32_t> leaf_size, leaf_q;
    std::vector<float> b;
    std::vector<float> vals;           // [n_nodes][K] non-zero components of the normal, ascending dimension
    std::vector<uint8_t> dims;         // [n_nodes][K] their dimensions
    std::mutex mu;
    std::map<int, ForestImage> images; // device ordinal -> image
};

double forest_c(uint32_t m);  // average path length of an unsuccessful BST search over m samples
int forest_build(const float* seeds, uint64_t n_seeds, uint32_t d, uint32_t n_trees, uint32_t sample_size, uint32_t max_tree_depth,
                 uint32_t extension_level, uint64_t seed, Forest** out, unsigned max_threads = 16);
void forest_export(const Forest* f, uint32_t* sample_idx, uint64_t* tree_first, float* normal, float* b, uint32_t* left,
                   uint32_t* right, uint32_t* leaf_size, uint32_t* leaf_q);
int forest_device_image(Forest* f, int device, hipStream_t st, const ForestImage** out);
void forest_destroy(Forest* f);
// workgroups that share a candidate block's trees: `forced` > 0 (BLISSGPU_OPT_FOREST_SPLIT) or enough to fill the device
uint32_t forest_split_plan(const Forest* f, uint64_t n, int n_cus, int64_t forced);
hipError_t launch_forest_walk(const Forest* f, const ForestImage& im, const float* X, uint32_t n, uint32_t n_split, bool stage,
                        unsigned long long* sum, hipStream_t st);
void launch_forest_finish(const Forest* f, const unsigned long long* sum, uint32_t n, float* score, uint32_t* keys, uint32_t* idx,
                          hipStream_t st);


// ---- one forest per seed GROUP, the k lowest scores of every group (blissgpu_group_forest_knn) ----
struct GroupForestOpts {
    uint32_t d, n_trees, sample_size, max_tree_depth, extension_level;
    uint64_t seed;
};
// nodes a group of `count` seeds is planned with: n_trees x (2 psi - 1), psi = min(sample_size, count); a group without a
// forest (psi < 2) counts as one node, so that a budget of 1 is one group per batch
uint64_t group_forest_nodes(uint64_t count, uint32_t n_trees, uint32_t sample_size);
// the node budget of a batch when none is forced: what a 64 MiB image (or an eighth of the workspace limit, if less) holds
uint64_t group_forest_budget(uint64_t workspace_bytes, uint32_t extension_level);
// first group of every batch of consecutive groups whose planned nodes stay within the budget (a group beyond it: alone)
std::vector<uint64_t> group_forest_batches(const uint64_t* off, uint64_t n_groups, uint32_t n_trees, uint32_t sample_size,
                                           uint64_t budget);
// both entry points after their argument checks.  h_seeds, off: host; d_cand, d_skip, d_idx, d_score, d_status: device (d_skip,
// d_score, d_status may be NULL); h_status: host or NULL.  Synchronises the context's stream before it returns.
int group_forest_run(blissgpu_ctx* c, const char* who, const float* h_seeds, const uint64_t* off, uint64_t n_groups,
                     const float* d_cand, uint64_t n, const GroupForestOpts& o, const uint32_t* d_skip, uint32_t k,
                     uint32_t* d_idx, float* d_score, int32_t* d_status, int32_t* h_status);

}  // namespace bg
