// test_mst_merge.cpp -- drives bliss-rs_amd/csrc/mst_merge.hpp (the host half of blissgpu_mst: Boruvka's loop, the merge between
// two rounds, the final sort) without a device, so that tests/test_mst_host.py can compare its trees with the contract written
// out in numpy, and run it under AddressSanitizer / UBSan.  The device's part -- every component's smallest leaving edge -- is
// a scalar loop over a matrix here.
//
//   test_mst_merge <case.in> <case.out>
// case.in  (little endian): u32 n, u32 has_core, then Dm f32[n][n], then core f32[n] when has_core
// case.out: i32 status (MST_*), u32 rounds, then u u32[n - 1], v u32[n - 1], w u32[n - 1] (the weights' bits)
//
//   test_mst_merge --direct
// feeds the merge step the awkward cases by hand; exit status 0 when every one holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../bliss-rs_amd/csrc/mst_merge.hpp"

using namespace bg;

static void die(const char* what) {
    fprintf(stderr, "test_mst_merge: %s\n", what);
    exit(2);
}
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fprintf(stderr, "test_mst_merge: line %d: %s\n", __LINE__, #cond); \
            exit(3);                                                           \
        }                                                                      \
    } while (0)

static uint32_t bits(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}

static bool key_less(uint32_t w, uint64_t uv, uint32_t ow, uint64_t ouv) { return w != ow ? w < ow : uv < ouv; }

static int direct() {
    // two components picking the same edge: one edge, one union
    {
        MstState s;
        mst_init(s, 2);
        CHECK(s.comps == 2 && s.order[0] == 0 && s.order[1] == 1 && s.cpos[1] == 1 && s.off.size() == 3);
        const uint32_t pw[2] = {5, 5};
        const uint64_t puv[2] = {mst_pack(0, 1), mst_pack(0, 1)};
        CHECK(mst_merge_round(s, pw, puv) == MST_OK);
        CHECK(s.comps == 1 && s.edges.size() == 1 && s.edges[0].u == 0 && s.edges[0].v == 1 && s.edges[0].w == 5 && s.rounds == 1);
    }
    // a chain of picks a -> b -> c -> d (d picks c back): three edges, one component, renumbered by the lowest member
    {
        MstState s;
        mst_init(s, 4);
        const uint32_t pw[4] = {3, 2, 1, 1};
        const uint64_t puv[4] = {mst_pack(0, 1), mst_pack(1, 2), mst_pack(2, 3), mst_pack(2, 3)};
        CHECK(mst_merge_round(s, pw, puv) == MST_OK);
        CHECK(s.comps == 1 && s.edges.size() == 3 && s.off[1] == 4);
        for (uint32_t i = 0; i < 4; i++) CHECK(s.comp[i] == 0 && s.order[i] == i);
    }
    // two pairs: components numbered by their lowest member, the order sorted by (component, index)
    {
        MstState s;
        mst_init(s, 5);
        const uint32_t pw[5] = {1, 1, 1, 1, MST_NONE};
        const uint64_t puv[5] = {mst_pack(0, 3), mst_pack(1, 2), mst_pack(1, 2), mst_pack(0, 3), ~0ull};
        CHECK(mst_merge_round(s, pw, puv) == MST_OK);
        CHECK(s.comps == 3 && s.edges.size() == 2);
        const uint32_t comp[5] = {0, 1, 1, 0, 2}, order[5] = {0, 3, 1, 2, 4}, cpos[5] = {0, 0, 1, 1, 2}, off[4] = {0, 2, 4, 5};
        for (int i = 0; i < 5; i++) CHECK(s.comp[i] == comp[i] && s.order[i] == order[i] && s.cpos[i] == cpos[i]);
        for (int i = 0; i < 4; i++) CHECK(s.off[i] == off[i]);
    }
    // a pick that does not leave its component, or is no edge at all, is refused
    {
        MstState s;
        mst_init(s, 3);
        const uint32_t pw[3] = {1, MST_NONE, MST_NONE};
        uint64_t puv[3] = {mst_pack(1, 2), ~0ull, ~0ull};
        CHECK(mst_merge_round(s, pw, puv) == MST_BAD_PICK);
        mst_init(s, 3);
        puv[0] = mst_pack(0, 3);
        CHECK(mst_merge_round(s, pw, puv) == MST_BAD_PICK);
        mst_init(s, 3);
        puv[0] = mst_pack(1, 0);
        CHECK(mst_merge_round(s, pw, puv) == MST_BAD_PICK);
    }
    // a pick step that never picks: the loop ends after 64 rounds and says so
    {
        MstState s;
        uint32_t calls = 0;
        const int rc = mst_boruvka(s, 3, [&](MstState&, uint32_t*, uint64_t*) { calls++; return 0; });
        CHECK(rc == MST_TOO_MANY_ROUNDS && calls == MST_MAX_ROUNDS && s.rounds == MST_MAX_ROUNDS && s.comps == 3);
        MstState t;
        mst_init(t, 3);
        const uint32_t pw[3] = {MST_NONE, MST_NONE, MST_NONE};
        const uint64_t puv[3] = {0, 0, 0};
        CHECK(mst_merge_round(t, pw, puv) == MST_STALLED && t.comps == 3 && t.edges.empty());
    }
    // the pick's own error comes back as it is; no song and one song need no round
    {
        MstState s;
        CHECK(mst_boruvka(s, 2, [&](MstState&, uint32_t*, uint64_t*) { return 77; }) == 77);
        uint32_t calls = 0;
        CHECK(mst_boruvka(s, 0, [&](MstState&, uint32_t*, uint64_t*) { calls++; return 0; }) == MST_OK && s.edges.empty());
        CHECK(mst_boruvka(s, 1, [&](MstState&, uint32_t*, uint64_t*) { calls++; return 0; }) == MST_OK && s.edges.empty() && calls == 0);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--direct")) return direct();
    if (argc != 3) die("usage: test_mst_merge <case.in> <case.out> | --direct");
    FILE* f = fopen(argv[1], "rb");
    if (!f) die("cannot open the input");
    uint32_t n = 0, has_core = 0;
    if (fread(&n, 4, 1, f) != 1 || fread(&has_core, 4, 1, f) != 1) die("short header");
    if (n > 100000) die("bad header");
    std::vector<float> Dm((size_t)n * n), core(n, 0.0f);
    if (fread(Dm.data(), 4, Dm.size(), f) != Dm.size()) die("short matrix");
    if (has_core && fread(core.data(), 4, n, f) != n) die("short core");
    fclose(f);

    MstState s;
    const int32_t status = mst_boruvka(s, n, [&](MstState& st, uint32_t* pw, uint64_t* puv) {
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t c = st.comp[i];
            for (uint32_t j = 0; j < n; j++) {
                if (st.comp[j] == c) continue;
                float w = Dm[(size_t)i * n + j];
                if (core[i] > w) w = core[i];
                if (core[j] > w) w = core[j];
                const uint64_t uv = i < j ? mst_pack(i, j) : mst_pack(j, i);
                if (pw[c] == MST_NONE || key_less(bits(w), uv, pw[c], puv[c])) {
                    pw[c] = bits(w);
                    puv[c] = uv;
                }
            }
        }
        return 0;
    });
    FILE* o = fopen(argv[2], "wb");
    if (!o) die("cannot open the output");
    const uint32_t rounds = s.rounds;
    if (fwrite(&status, 4, 1, o) != 1 || fwrite(&rounds, 4, 1, o) != 1) die("short write");
    if (status == MST_OK) {
        if (s.edges.size() != (n ? n - 1 : 0)) die("not a spanning tree");
        for (int part = 0; part < 3; part++)
            for (const MstEdge& e : s.edges) {
                const uint32_t x = part == 0 ? e.u : (part == 1 ? e.v : e.w);
                if (fwrite(&x, 4, 1, o) != 1) die("short write");
            }
    }
    fclose(o);
    return 0;
}
