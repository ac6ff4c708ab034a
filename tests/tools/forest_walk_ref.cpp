// CPU yardstick of tests/tools/forest_bench.py: a plain walk of an EXPORTED forest (include/blissgpu.h, blissgpu_forest_export),
// one candidate at a time through every tree -- what the reference's per-candidate Forest::score loop amounts to -- on
// `threads` threads.  Same defined split test as the library, so its sums double as a check of the device's.
//   c++ -O3 -std=c++17 -shared -fPIC -pthread forest_walk_ref.cpp -o libforest_walk_ref.so
#include <stdint.h>

#include <thread>
#include <vector>

extern "C" void forest_walk_ref(const float* X, uint64_t n, uint32_t d, uint32_t n_trees, const uint64_t* tree_first,
                                const float* normal, const float* b, const uint32_t* left, const uint32_t* right,
                                const uint32_t* leaf_q, uint32_t threads, uint64_t* sum) {
    auto work = [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++) {
            const float* x = X + i * d;
            uint64_t acc = 0;
            for (uint32_t t = 0; t < n_trees; t++) {
                uint64_t node = tree_first[t];
                while (left[node] != 0xFFFFFFFFu) {
                    const float* nv = normal + node * d;
                    float s = 0.0f;
                    for (uint32_t j = 0; j < d; j++)
                        if (nv[j] != 0.0f) s = s + nv[j] * x[j];
                    node = s < b[node] ? left[node] : right[node];
                }
                acc += leaf_q[node];
            }
            sum[i] = acc;
        }
    };
    if (threads <= 1) { work(0, n); return; }
    std::vector<std::thread> pool;
    for (uint32_t w = 0; w < threads; w++) pool.emplace_back(work, n * w / threads, n * (w + 1) / threads);
    for (auto& th : pool) th.join();
}
