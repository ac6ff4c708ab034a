// mst_merge.hpp -- the device-free half of the minimum spanning tree (include/blissgpu.h): everything Boruvka's
// algorithm does between two scans of the device, the bounded loop around them and the final sort of the edges.
//
// The tree is the unique one under the strict total order of the edges {u, v}, u < v: (bits of the f32 weight as u32, u, v),
// compared lexicographically.  Per round every component picks the smallest edge that leaves it (the scan and the pick, on
// the device; a scalar loop in tests/cpp/test_mst_merge.cpp).  Under a strict order those picks never close a cycle, so the
// merge only has to drop the doubles -- two components that picked the same edge --, unite, and renumber.
//
// No HIP, no floating-point arithmetic: weights are carried as their bit patterns.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace bg {

constexpr uint32_t MST_NONE = 0xFFFFFFFFu;  // a component that picked nothing / no song
constexpr uint32_t MST_MAX_ROUNDS = 64;     // ceil(log2 n) <= 32 rounds are ever needed: the loop does not go on past this
enum { MST_OK = 0, MST_BAD_PICK = 1, MST_STALLED = 2, MST_TOO_MANY_ROUNDS = 3 };

struct MstEdge {
    uint32_t w, u, v;  // the key, in its order: weight bits, lower song, higher song
};
inline bool mst_edge_less(const MstEdge& a, const MstEdge& b) {
    if (a.w != b.w) return a.w < b.w;
    if (a.u != b.u) return a.u < b.u;
    return a.v < b.v;
}
inline uint64_t mst_pack(uint32_t u, uint32_t v) { return ((uint64_t)u << 32) | v; }

struct MstState {
    uint32_t n = 0, comps = 0, rounds = 0;
    std::vector<uint32_t> parent;  // union-find over songs
    std::vector<uint32_t> comp;    // [n] the component of every song: 0 .. comps - 1 in order of the lowest member
    std::vector<uint32_t> order;   // [n] the songs sorted by (component, index): what the scan walks
    std::vector<uint32_t> cpos;    // [n] comp[order[p]]: the component at every position
    std::vector<uint32_t> off;     // [comps + 1] component c is order[off[c] .. off[c + 1])
    std::vector<uint32_t> relabel; // scratch: root -> new component
    std::vector<MstEdge> edges;    // the tree so far, in the order found
};

inline uint32_t mst_find(MstState& s, uint32_t x) {
    uint32_t r = x;
    while (s.parent[r] != r) r = s.parent[r];
    while (s.parent[x] != r) {  // path compression
        const uint32_t next = s.parent[x];
        s.parent[x] = r;
        x = next;
    }
    return r;
}

// the (component, index) order and its segments from the union-find: components numbered by their lowest member
inline void mst_renumber(MstState& s) {
    const uint32_t n = s.n;
    std::fill(s.relabel.begin(), s.relabel.end(), MST_NONE);
    uint32_t c = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t r = mst_find(s, i);
        if (s.relabel[r] == MST_NONE) s.relabel[r] = c++;
        s.comp[i] = s.relabel[r];
    }
    s.comps = c;
    s.off.assign((size_t)c + 1, 0u);
    for (uint32_t i = 0; i < n; i++) s.off[s.comp[i] + 1]++;
    for (uint32_t k = 0; k < c; k++) s.off[k + 1] += s.off[k];
    std::vector<uint32_t>& fill = s.relabel;  // (free again: the next free place of every component)
    for (uint32_t k = 0; k < c; k++) fill[k] = s.off[k];
    for (uint32_t i = 0; i < n; i++) {  // ascending i: ascending index inside a component
        const uint32_t p = fill[s.comp[i]]++;
        s.order[p] = i;
        s.cpos[p] = s.comp[i];
    }
}

inline void mst_init(MstState& s, uint32_t n) {
    s.n = n;
    s.rounds = 0;
    s.parent.resize(n);
    s.comp.resize(n);
    s.order.resize(n);
    s.cpos.resize(n);
    s.relabel.resize(n);
    s.edges.clear();
    s.edges.reserve(n ? n - 1 : 0);
    for (uint32_t i = 0; i < n; i++) s.parent[i] = i;
    mst_renumber(s);
}

// one round's picks: pick_w[c] = the weight bits of component c's smallest leaving edge (MST_NONE: none), pick_uv[c] = its
// songs packed (lower << 32 | higher).  A pick must be an edge u < v < n with exactly one end in c.
inline int mst_merge_round(MstState& s, const uint32_t* pick_w, const uint64_t* pick_uv) {
    const uint32_t before = s.comps;
    for (uint32_t c = 0; c < before; c++) {
        if (pick_w[c] == MST_NONE) continue;
        const uint32_t u = (uint32_t)(pick_uv[c] >> 32), v = (uint32_t)pick_uv[c];
        if (!(u < v && v < s.n) || (s.comp[u] == c) == (s.comp[v] == c)) return MST_BAD_PICK;
        const uint32_t ru = mst_find(s, u), rv = mst_find(s, v);
        if (ru == rv) continue;  // the double: the component at the other end picked this edge too (and came first)
        s.parent[std::max(ru, rv)] = std::min(ru, rv);
        s.edges.push_back(MstEdge{pick_w[c], u, v});
    }
    s.rounds++;
    mst_renumber(s);
    return s.comps < before ? MST_OK : MST_STALLED;
}

// Boruvka's loop.  pick(state, pick_w, pick_uv) fills one entry per component of state (comps of them) and returns 0, or an
// error of its own (any value but 0, handed back as it is).  -> MST_OK with the n - 1 edges sorted by key.
template <class Pick>
inline int mst_boruvka(MstState& s, uint32_t n, Pick&& pick) {
    mst_init(s, n);
    std::vector<uint32_t> pw;
    std::vector<uint64_t> puv;
    while (s.comps > 1) {
        if (s.rounds >= MST_MAX_ROUNDS) return MST_TOO_MANY_ROUNDS;
        pw.assign(s.comps, MST_NONE);
        puv.assign(s.comps, ~0ull);
        const int rc = pick(s, pw.data(), puv.data());
        if (rc) return rc;
        const int m = mst_merge_round(s, pw.data(), puv.data());
        if (m == MST_BAD_PICK) return m;
        // (a round without progress is not an error here: the bound on the rounds ends such a loop)
    }
    std::sort(s.edges.begin(), s.edges.end(), mst_edge_less);
    return MST_OK;
}

}  // namespace bg
