// Stand-alone check of bliss-rs_amd/csrc/launch_forms.hpp (run by tests/test_launch_forms_host.py, plain and under sanitizers):
// the (d, metric, diagonal-M) ladder calls its callback exactly once, with the triple its contract states; the device-fill policy
// gives the values worked out by hand from its three numbers; the label sort's words follow one another as its comment says.
#include <stdio.h>

#include "../../bliss-rs_amd/csrc/launch_forms.hpp"

using namespace bg;

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            failures++;                                                  \
            fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
        }                                                                \
    } while (0)

struct Form {
    int calls = 0, d = -1, metric = -1, diag = -1;
};

// what the ladder is to give, written out as nested ifs
static void want_metric(bool cosine, int metric, int diag, int* m, int* g) {
    if (metric == 0) { *m = METRIC_EUCLIDEAN; *g = 0; }
    else if (cosine && metric == 1) { *m = METRIC_COSINE; *g = 0; }
    else if (diag) { *m = METRIC_MAHALANOBIS; *g = 1; }
    else { *m = METRIC_MAHALANOBIS; *g = 0; }
}

template <bool COSINE>
static void check_ladder() {
    for (uint32_t d = 0; d <= 65; d++) {
        const int want_d = d == 23 ? 23 : d == 20 ? 20 : 0;
        Form one;
        with_d(d, [&](auto D) { one.calls++; one.d = decltype(D)::value; });
        CHECK(one.calls == 1 && one.d == want_d);
        for (int metric = 0; metric <= 2; metric++)
            for (int diag = 0; diag <= 1; diag++) {
                int wm, wg;
                want_metric(COSINE, metric, diag, &wm, &wg);
                Form m;
                with_metric<COSINE>(metric, diag, [&](auto M, auto G) {
                    m.calls++;
                    m.metric = decltype(M)::value;
                    m.diag = decltype(G)::value ? 1 : 0;
                });
                CHECK(m.calls == 1 && m.metric == wm && m.diag == wg);
                if (want_d == 0) { wm = METRIC_EUCLIDEAN; wg = 0; }  // the generic kernel: the metric is a run-time argument
                Form f;
                for_metric_form<COSINE>(d, metric, diag, [&](auto D, auto M, auto G) {
                    f.calls++;
                    f.d = decltype(D)::value;
                    f.metric = decltype(M)::value;
                    f.diag = decltype(G)::value ? 1 : 0;
                });
                CHECK(f.calls == 1 && f.d == want_d && f.metric == wm && f.diag == wg);
                // the form that takes the D with_d gave: the same triple
                Form h;
                with_d(d, [&](auto D_) {
                    for_metric_form<COSINE>(D_, metric, diag, [&](auto D, auto M, auto G) {
                        h.calls++;
                        h.d = decltype(D)::value;
                        h.metric = decltype(M)::value;
                        h.diag = decltype(G)::value ? 1 : 0;
                    });
                });
                CHECK(h.calls == 1 && h.d == want_d && h.metric == wm && h.diag == wg);
            }
    }
}

static void check_fill(uint64_t pieces, int n_cus, uint32_t cus, uint32_t waves, uint32_t grid) {
    const ScanFill f = scan_fill(pieces, n_cus);
    if (f.cus != cus || f.waves != waves || f.grid != grid) {
        failures++;
        fprintf(stderr, "scan_fill(%llu, %d) = (%u, %u, %u), not (%u, %u, %u)\n", (unsigned long long)pieces, n_cus, f.cus, f.waves,
                f.grid, cus, waves, grid);
    }
}

static void check_words(uint64_t hist_words, uint32_t scan_tiles, uint32_t k, uint64_t n) {
    const LabelSortWords o = label_sort_words(hist_words, scan_tiles, k, n);
    CHECK(o.o_hist == 4);
    CHECK(o.o_bsum == 4 + hist_words);
    CHECK(o.o_off == 4 + hist_words + scan_tiles);
    CHECK(o.o_arow == 4 + hist_words + scan_tiles + k + 1);
    CHECK(o.end == 4 + hist_words + scan_tiles + k + 1 + n);
}

int main() {
    check_ladder<true>();
    check_ladder<false>();
    // without cosine kernels a cosine argument takes the Mahalanobis pair: no cosine kernel is named
    {
        Form m;
        with_metric<false>(METRIC_COSINE, 1, [&](auto M, auto G) { m.metric = decltype(M)::value; m.diag = decltype(G)::value; });
        CHECK(m.metric == METRIC_MAHALANOBIS && m.diag == 1);
    }
    // 256 CUs when the context does not know: 8 x 256 = 2048 pieces are the first that take four wavefronts per workgroup
    CHECK(cus_or_default(0) == 256 && cus_or_default(-1) == 256 && cus_or_default(8) == 8 && cus_or_default(304) == 304);
    check_fill(0, 0, 256, 1, 0);
    check_fill(2047, 0, 256, 1, 2047);
    check_fill(2048, 0, 256, 4, 512);
    check_fill(2049, 0, 256, 4, 513);
    check_fill(63, 8, 8, 1, 63);
    check_fill(64, 8, 8, 4, 16);
    // ceil(32 x 256 / in_one)
    CHECK(fill_col_groups(256, 1) == 8192);
    CHECK(fill_col_groups(256, 2048) == 4);
    CHECK(fill_col_groups(256, 8192) == 1);
    CHECK(fill_col_groups(256, 8193) == 1);
    check_words(5, 1, 5, 0);
    check_words(768, 1, 3, 65536);
    check_words(2097152, 1024, 4096, 1);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("launch_forms ok\n");
    return 0;
}
