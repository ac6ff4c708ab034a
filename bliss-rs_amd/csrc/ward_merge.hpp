// ward_merge.hpp -- the device-free half of Ward clustering (include/blissgpu.h): everything between two scans of
// the device -- the mutual pairs of a round's nearest positions, the edges they emit, the plan the join kernel reads, the next
// round's sizes and lowest members --, the loop around the rounds with its guard, and the final sort of the edges.
//
// The clusters sit at positions 0 .. m - 1 in order of their lowest member song.  A round's pairs are all (p, q), p < q, with
// nn[p] == q and nn[q] == p: disjoint by construction.  Pair (p, q) keeps position p's place and q disappears; the survivors
// keep their relative order, so the positions stay ordered by lowest member and an edge's u = low[p] is below its v = low[q].
//
// No HIP, no floating-point arithmetic: costs are carried as their bit patterns, the rows never come here.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace bg {

constexpr uint32_t WARD_NONE = 0xFFFFFFFFu;  // no partner / no nearest position
enum { WARD_OK = 0, WARD_BAD_NEAREST = 1, WARD_STALLED = 2 };

struct WardEdge {
    uint32_t cost, round, u, v, size;  // the key in its order -- cost bits, round, lower song --, then the higher song and the merged size
};
inline bool ward_edge_less(const WardEdge& a, const WardEdge& b) {
    if (a.cost != b.cost) return a.cost < b.cost;
    if (a.round != b.round) return a.round < b.round;
    return a.u < b.u;
}

struct WardJoin {
    uint32_t p, q;  // the old position that becomes this new one, and the old position merged into it (WARD_NONE: none)
};

struct WardState {
    uint32_t n = 0, m = 0, rounds = 0;
    uint32_t prev_m = 0;               // the positions of the round before: what the plan's entries index
    uint64_t pairs_scanned = 0;       // sum over the rounds of m (m - 1): what the scans evaluated
    std::vector<uint32_t> size, low;   // [m] per position: songs in the cluster, its lowest member
    std::vector<uint32_t> prev_size, prev_low;  // [prev_m] the same of the round before (the next round's while a merge builds them)
    std::vector<WardJoin> plan;        // [m after the round] what the join kernel reads
    std::vector<WardEdge> edges;       // the tree so far, in the order found
};

inline void ward_init(WardState& s, uint32_t n) {
    s.n = s.m = n;
    s.rounds = 0;
    s.prev_m = 0;
    s.pairs_scanned = 0;
    s.size.assign(n, 1u);
    s.low.resize(n);
    for (uint32_t i = 0; i < n; i++) s.low[i] = i;
    s.prev_size.clear();
    s.prev_low.clear();
    s.plan.clear();
    s.edges.clear();
    s.edges.reserve(n ? n - 1 : 0);
}

// one round: nn[p] = the nearest position of p (another position below m), cost[p] = the bits of that pair's cost.  Fills the
// plan, emits the pairs' edges and moves the state to the next round's positions.  -> WARD_OK, WARD_BAD_NEAREST (an nn that is
// no other position: the state is untouched) or WARD_STALLED (no mutual pair: the state is untouched).
inline int ward_merge_round(WardState& s, const uint32_t* nn, const uint32_t* cost) {
    const uint32_t m = s.m;
    for (uint32_t p = 0; p < m; p++)
        if (nn[p] >= m || nn[p] == p) return WARD_BAD_NEAREST;
    uint32_t pairs = 0;
    for (uint32_t p = 0; p < m; p++) pairs += nn[p] > p && nn[nn[p]] == p;
    if (!pairs) return WARD_STALLED;
    s.plan.clear();
    s.prev_size.clear();
    s.prev_low.clear();
    for (uint32_t p = 0; p < m; p++) {
        const uint32_t q = nn[p];
        const bool mutual = nn[q] == p;
        if (mutual && q < p) continue;  // merged into position q: this place disappears
        if (mutual) {
            s.edges.push_back(WardEdge{cost[p], s.rounds, s.low[p], s.low[q], s.size[p] + s.size[q]});
            s.plan.push_back(WardJoin{p, q});
            s.prev_size.push_back(s.size[p] + s.size[q]);
        } else {
            s.plan.push_back(WardJoin{p, WARD_NONE});
            s.prev_size.push_back(s.size[p]);
        }
        s.prev_low.push_back(s.low[p]);
    }
    s.pairs_scanned += (uint64_t)m * (m - 1);
    s.size.swap(s.prev_size);
    s.low.swap(s.prev_low);
    s.prev_m = m;
    s.m = m - pairs;
    s.rounds++;
    return WARD_OK;
}

// The rounds.  nearest(state, nn, cost) fills one entry per position of state (m of them); join(state) applies state.plan to
// the rows (state is already the next round's).  Either returns 0, or an error of its own (any value but 0, handed back as it
// is).  -> WARD_OK with the n - 1 edges sorted by key.  Every round merges at least one pair or the loop ends with
// WARD_STALLED, so it runs at most n - 1 times.
template <class Nearest, class Join>
inline int ward_rounds(WardState& s, uint32_t n, Nearest&& nearest, Join&& join) {
    ward_init(s, n);
    std::vector<uint32_t> nn, cost;
    while (s.m > 1) {
        nn.assign(s.m, WARD_NONE);
        cost.assign(s.m, WARD_NONE);
        int rc = nearest(s, nn.data(), cost.data());
        if (rc) return rc;
        rc = ward_merge_round(s, nn.data(), cost.data());
        if (rc) return rc;
        if (s.m > 1 && (rc = join(s))) return rc;
    }
    std::sort(s.edges.begin(), s.edges.end(), ward_edge_less);
    return WARD_OK;
}

}  // namespace bg
