// test_ward_merge.cpp -- drives bliss-rs_amd/csrc/ward_merge.hpp (the host half of blissgpu_ward: the mutual pairs of a round, the
// edges, the join plan, the loop with its guard, the final sort) without a device, so that tests/test_ward_host.py can compare
// its trees with the contract written out in numpy, and run it under AddressSanitizer / UBSan.  The device's parts -- every
// position's nearest other position and the join of the rows -- are scalar loops here (compile with -ffp-contract=off).
//
//   test_ward_merge <case.in> <case.out>
// case.in  (little endian): u32 n, u32 d, then X f32[n][d]
// case.out: i32 status (WARD_*), u32 rounds, then u, v, cost bits, size, round: u32[n - 1] each
// The distance is sqrtf of the f32 sum of squared differences taken in ascending feature order (the test's numpy dist_fn).
//
//   test_ward_merge --direct
// feeds the merge step the awkward cases by hand; exit status 0 when every one holds.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../bliss-rs_amd/csrc/ward_merge.hpp"

using namespace bg;

static void die(const char* what) {
    fprintf(stderr, "test_ward_merge: %s\n", what);
    exit(2);
}
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            fprintf(stderr, "test_ward_merge: line %d: %s\n", __LINE__, #cond); \
            exit(3);                                                            \
        }                                                                       \
    } while (0)

static uint32_t bits(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}

static int direct() {
    // two positions, each other's nearest: one edge, one position left
    {
        WardState s;
        ward_init(s, 2);
        CHECK(s.m == 2 && s.size[1] == 1 && s.low[1] == 1);
        const uint32_t nn[2] = {1, 0}, cost[2] = {5, 5};
        CHECK(ward_merge_round(s, nn, cost) == WARD_OK);
        CHECK(s.m == 1 && s.prev_m == 2 && s.rounds == 1 && s.edges.size() == 1 && s.plan.size() == 1);
        CHECK(s.edges[0].u == 0 && s.edges[0].v == 1 && s.edges[0].cost == 5 && s.edges[0].size == 2 && s.edges[0].round == 0);
        CHECK(s.plan[0].p == 0 && s.plan[0].q == 1 && s.size[0] == 2 && s.low[0] == 0 && s.pairs_scanned == 2);
    }
    // a chain 0 -> 1 -> 2 <-> 3 and a bystander 4 -> 3: only (2, 3) is mutual; the survivors keep their order
    {
        WardState s;
        ward_init(s, 5);
        const uint32_t nn[5] = {1, 2, 3, 2, 3}, cost[5] = {9, 8, 7, 7, 8};
        CHECK(ward_merge_round(s, nn, cost) == WARD_OK);
        CHECK(s.m == 4 && s.edges.size() == 1 && s.edges[0].u == 2 && s.edges[0].v == 3 && s.edges[0].cost == 7);
        const uint32_t p[4] = {0, 1, 2, 4}, q[4] = {WARD_NONE, WARD_NONE, 3, WARD_NONE}, size[4] = {1, 1, 2, 1}, low[4] = {0, 1, 2, 4};
        for (int t = 0; t < 4; t++) CHECK(s.plan[t].p == p[t] && s.plan[t].q == q[t] && s.size[t] == size[t] && s.low[t] == low[t]);
        // the next round works on positions: (0, 1) and (2, 3) -- the old 2 + 3 and 4 -- merge; u and v are lowest members
        const uint32_t nn2[4] = {1, 0, 3, 2}, cost2[4] = {4, 4, 6, 6};
        CHECK(ward_merge_round(s, nn2, cost2) == WARD_OK);
        CHECK(s.m == 2 && s.rounds == 2 && s.edges.size() == 3);
        CHECK(s.edges[1].u == 0 && s.edges[1].v == 1 && s.edges[1].size == 2 && s.edges[1].round == 1);
        CHECK(s.edges[2].u == 2 && s.edges[2].v == 4 && s.edges[2].size == 3 && s.edges[2].round == 1);
        CHECK(s.size[0] == 2 && s.size[1] == 3 && s.low[0] == 0 && s.low[1] == 2 && s.pairs_scanned == 20 + 12);
    }
    // an nn that is no other position is refused and the state stays; a round without a mutual pair stalls and the state stays
    {
        WardState s;
        ward_init(s, 3);
        const uint32_t cost[3] = {1, 1, 1};
        const uint32_t self[3] = {1, 1, 0}, past[3] = {1, 0, 3}, none[3] = {1, 0, WARD_NONE}, cycle[3] = {1, 2, 0};
        CHECK(ward_merge_round(s, self, cost) == WARD_BAD_NEAREST);
        CHECK(ward_merge_round(s, past, cost) == WARD_BAD_NEAREST);
        CHECK(ward_merge_round(s, none, cost) == WARD_BAD_NEAREST);
        CHECK(ward_merge_round(s, cycle, cost) == WARD_STALLED);
        CHECK(s.m == 3 && s.rounds == 0 && s.edges.empty() && s.size.size() == 3);
    }
    // the loop: the callbacks' own errors come back as they are; no song and one song need no round; a stall ends the loop
    {
        WardState s;
        uint32_t calls = 0;
        auto never = [&](WardState&, uint32_t*, uint32_t*) { calls++; return 0; };
        auto join = [&](WardState&) { return 0; };
        CHECK(ward_rounds(s, 0, never, join) == WARD_OK && s.edges.empty());
        CHECK(ward_rounds(s, 1, never, join) == WARD_OK && s.edges.empty() && calls == 0);
        CHECK(ward_rounds(s, 2, [&](WardState&, uint32_t*, uint32_t*) { return 77; }, join) == 77);
        CHECK(ward_rounds(s, 3, never, join) == WARD_BAD_NEAREST && calls == 1);  // (nn stays WARD_NONE)
        auto cycle = [&](WardState& st, uint32_t* nn, uint32_t* c) {
            for (uint32_t p = 0; p < st.m; p++) { nn[p] = (p + 1) % st.m; c[p] = 1; }
            return 0;
        };
        CHECK(ward_rounds(s, 3, cycle, join) == WARD_STALLED && s.rounds == 0);
        uint32_t joins = 0;
        auto pairs = [&](WardState& st, uint32_t* nn, uint32_t* c) {  // 0 <-> 1, the rest point at 0
            for (uint32_t p = 0; p < st.m; p++) { nn[p] = p ? 0 : 1; c[p] = 10 - st.m; }
            return 0;
        };
        CHECK(ward_rounds(s, 4, pairs, [&](WardState&) { joins++; return 0; }) == WARD_OK);
        CHECK(s.rounds == 3 && joins == 2 && s.edges.size() == 3);  // (no join after the last merge)
        CHECK(ward_rounds(s, 4, pairs, [&](WardState&) { return 55; }) == 55);
        // the sort: ascending (cost, round, u) -- the rounds above ran with costs 6, 7, 8
        CHECK(s.edges.size() == 1);
        ward_rounds(s, 4, pairs, join);
        CHECK(s.edges[0].cost == 6 && s.edges[1].cost == 7 && s.edges[2].cost == 8 && s.edges[2].size == 4);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--direct")) return direct();
    if (argc != 3) die("usage: test_ward_merge <case.in> <case.out> | --direct");
    FILE* f = fopen(argv[1], "rb");
    if (!f) die("cannot open the input");
    uint32_t n = 0, d = 0;
    if (fread(&n, 4, 1, f) != 1 || fread(&d, 4, 1, f) != 1) die("short header");
    if (n > 100000 || d == 0 || d > 64) die("bad header");
    std::vector<float> X((size_t)n * d);
    if (fread(X.data(), 4, X.size(), f) != X.size()) die("short rows");
    fclose(f);

    // rows[low] is the row of the cluster whose lowest member is low, as on the device
    WardState s;
    const int32_t status = ward_rounds(
        s, n,
        [&](WardState& st, uint32_t* nn, uint32_t* cost) {
            for (uint32_t i = 0; i < st.m; i++) {
                uint64_t best = ~0ull;
                const float* a = &X[(size_t)st.low[i] * d];
                for (uint32_t j = 0; j < st.m; j++) {
                    if (j == i) continue;
                    const float* b = &X[(size_t)st.low[j] * d];
                    float sum = 0.0f;
                    for (uint32_t k = 0; k < d; k++) {
                        const float diff = a[k] - b[k];
                        sum = sum + diff * diff;
                    }
                    const float dist = sqrtf(sum);
                    const float si = (float)st.size[i], sj = (float)st.size[j];
                    const float w = (si * sj) / (si + sj);
                    const float c = (dist * dist) * w;
                    const uint64_t key = ((uint64_t)bits(c) << 32) | (uint64_t)(i ^ j);
                    if (key < best) best = key;
                }
                cost[i] = (uint32_t)(best >> 32);
                nn[i] = i ^ (uint32_t)best;
            }
            return 0;
        },
        [&](WardState& st) {
            // (the state is the next round's already; the plan indexes the round before's positions: prev_size, prev_low)
            for (uint32_t t = 0; t < st.m; t++) {
                const WardJoin& e = st.plan[t];
                if (e.p >= st.prev_m || st.prev_low[e.p] != st.low[t]) return 9;
                if (e.q == WARD_NONE) continue;
                if (e.q >= st.prev_m || e.q <= e.p) return 9;
                const uint32_t sp = st.prev_size[e.p], sq = st.prev_size[e.q];
                if (sp + sq != st.size[t]) return 9;
                float* cp = &X[(size_t)st.prev_low[e.p] * d];
                const float* cq = &X[(size_t)st.prev_low[e.q] * d];
                for (uint32_t k = 0; k < d; k++)
                    cp[k] = (float)(((double)sp * (double)cp[k] + (double)sq * (double)cq[k]) / (double)(sp + sq));
            }
            return 0;
        });
    FILE* o = fopen(argv[2], "wb");
    if (!o) die("cannot open the output");
    const uint32_t rounds = s.rounds;
    if (fwrite(&status, 4, 1, o) != 1 || fwrite(&rounds, 4, 1, o) != 1) die("short write");
    if (status == WARD_OK) {
        if (s.edges.size() != (n ? n - 1 : 0)) die("not a whole tree");
        for (int part = 0; part < 5; part++)
            for (const WardEdge& e : s.edges) {
                const uint32_t x = part == 0 ? e.u : part == 1 ? e.v : part == 2 ? e.cost : part == 3 ? e.size : e.round;
                if (fwrite(&x, 4, 1, o) != 1) die("short write");
            }
    }
    fclose(o);
    return 0;
}
