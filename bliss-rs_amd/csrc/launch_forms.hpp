// launch_forms.hpp -- what every scan family's launcher decides before it launches: which (d, metric, diagonal-M) instantiation
// of its kernel runs, and on how many workgroups.  Host-only and free of HIP, so that a plain C++ compiler
// builds tests/cpp/test_launch_forms.cpp from it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

namespace bg {

enum { METRIC_EUCLIDEAN = 0, METRIC_COSINE = 1, METRIC_MAHALANOBIS = 2 };

// go(std::integral_constant<int, D>{}) with D = d for the two feature counts that have kernels of their own (23: version 2,
// 20: version 1), D = 0 -- the generic kernel, d a run-time argument -- for every other
template <typename F>
inline void with_d(uint32_t d, F&& go) {
    if (d == 23) go(std::integral_constant<int, 23>{});
    else if (d == 20) go(std::integral_constant<int, 20>{});
    else go(std::integral_constant<int, 0>{});
}

// go(M, G) once, with M an integral_constant<int, METRIC_*> and G a bool_constant: is M a diagonal.  A family without a cosine
// kernel passes COSINE = false: its *_args_ok has refused cosine already, and the argument falls through to the Mahalanobis pair
// without naming an instantiation that does not exist
template <bool COSINE, typename F>
inline void with_metric(int metric, int m_is_diag, F&& go) {
    using Mahalanobis = std::integral_constant<int, METRIC_MAHALANOBIS>;
    if (metric == METRIC_EUCLIDEAN) {
        go(std::integral_constant<int, METRIC_EUCLIDEAN>{}, std::false_type{});
        return;
    }
    if constexpr (COSINE) {
        if (metric == METRIC_COSINE) {
            go(std::integral_constant<int, METRIC_COSINE>{}, std::false_type{});
            return;
        }
    }
    if (m_is_diag) go(Mahalanobis{}, std::true_type{});
    else go(Mahalanobis{}, std::false_type{});
}

// The whole ladder, go(D, M, G): d = 23 or 20 under each metric form; every other d the generic <0, EUCLIDEAN, false>, whose
// metric is a run-time argument.  The first form is for a launcher with a choice of its own between with_d and the metric
// (the k-nearest scans' key buffers): it takes the D that with_d gave
template <bool COSINE, int D, typename F>
inline void for_metric_form(std::integral_constant<int, D> d, int metric, int m_is_diag, F&& go) {
    if constexpr (D == 0) go(d, std::integral_constant<int, METRIC_EUCLIDEAN>{}, std::false_type{});
    else with_metric<COSINE>(metric, m_is_diag, [&](auto M, auto G) { go(d, M, G); });
}
template <bool COSINE, typename F>
inline void for_metric_form(uint32_t d, int metric, int m_is_diag, F&& go) {
    with_d(d, [&](auto D) { for_metric_form<COSINE>(D, metric, m_is_diag, go); });
}

// How a scan whose rows come in `pieces` of 256 per wavefront fills the device; the three numbers are one tuning policy, measured
// in DESIGN.md 3.23.  256: the CUs planned for when the context does not know its own.  8: with that many pieces per CU every CU
// gets two workgroups of four wavefronts that share a tile of columns; with fewer, a workgroup is one wavefront, so that the
// pieces spread over the CUs.  32: a scan whose columns are dealt to groups (grid.y) takes as many groups as give about 32
// wavefronts per CU -- four rounds of the eight the registers admit, which evens out the groups' unequal rows -- where in_one is
// the wavefronts of one group.  The caps that differ between the plans stay in the plans
inline uint32_t cus_or_default(int n_cus) { return (uint32_t)(n_cus > 0 ? n_cus : 256); }

struct ScanFill {
    uint32_t cus, waves, grid;  // grid = ceil(pieces / waves): 0 for no pieces
};
inline ScanFill scan_fill(uint64_t pieces, int n_cus) {
    ScanFill f;
    f.cus = cus_or_default(n_cus);
    f.waves = pieces >= 8ull * f.cus ? 4u : 1u;
    f.grid = (uint32_t)((pieces + f.waves - 1) / f.waves);
    return f;
}
inline uint64_t fill_col_groups(uint32_t cus, uint64_t in_one) { return (32ull * cus + in_one - 1) / in_one; }  // in_one >= 1

// Where the k-means sort of a labelling keeps its tables, in 32-bit words from the start of a call's workspace: the call's
// flags u32[4] | hist u32[hist_words] | the scan's totals u32[scan_tiles] | arow_off u32[k + 1] | arow u32[n] | end, the first
// word the caller may use (hist_words and scan_tiles: KmeansPlan)
struct LabelSortWords {
    size_t o_hist, o_bsum, o_off, o_arow, end;
};
inline LabelSortWords label_sort_words(uint64_t hist_words, uint32_t scan_tiles, uint32_t k, uint64_t n) {
    LabelSortWords o;
    o.o_hist = 4;
    o.o_bsum = o.o_hist + (size_t)hist_words;
    o.o_off = o.o_bsum + scan_tiles;
    o.o_arow = o.o_off + k + 1;
    o.end = o.o_arow + (size_t)n;
    return o;
}

}  // namespace bg
