// covariance_metric.hpp -- a scatter matrix turned into a Mahalanobis M (blissgpu_covariance_metric): the inverse of the shrunk
// covariance, diagonal (per-feature standardisation) or full (whitening; with a pooled within-group scatter: relevant component
// analysis), scaled to trace d.  No device code and no HIP header: tests/cpp/test_covariance_metric.cpp drives it, plain and
// under sanitizers.
//
// Every operation is f64, one rounding per multiply and per add, sums ascending from 0.0.  Each product stands in a statement
// of its own, so no compiler contracts it with the add that follows; build with -ffp-contract=off where the compiler would
// contract across statements.  include/blissgpu.h states the formulas; this file is their only implementation.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

namespace bg {
namespace covmetric {

constexpr int FORM_DIAGONAL = 0, FORM_FULL = 1;
constexpr int STATUS_OK = 0, STATUS_NOT_POSITIVE = 1;

inline bool positive_finite(double v) { return v > 0.0 && isfinite(v); }

// S [d][d] (the upper half is read), dof > 0, 0 <= shrink <= 1, form one of the two.  -> STATUS_OK and M [d][d] written, or
// STATUS_NOT_POSITIVE and M untouched.  W (when not NULL) receives the unscaled inverse, [d][d] f64, whenever it was formed.
inline int solve(const double* S, uint32_t d, uint64_t dof, int form, double shrink, float* M, std::vector<double>* W_out = nullptr) {
    const size_t dd = (size_t)d * d;
    const double keep = 1.0 - shrink;
    std::vector<double> C(dd, 0.0), W(dd, 0.0);
    for (uint32_t r = 0; r < d; r++)
        for (uint32_t c = r; c < d; c++) C[(size_t)r * d + c] = C[(size_t)c * d + r] = S[(size_t)r * d + c] / (double)dof;
    double T = 0.0;
    for (uint32_t r = 0; r < d; r++) T = T + C[(size_t)r * d + r];
    T = T / (double)d;
    const double target = shrink * T;

    if (form == FORM_DIAGONAL) {
        for (uint32_t r = 0; r < d; r++) {
            const double kept = keep * C[(size_t)r * d + r];
            const double w = 1.0 / (kept + target);
            if (!positive_finite(w)) return STATUS_NOT_POSITIVE;
            W[(size_t)r * d + r] = w;
        }
    } else {
        // C' in place
        for (uint32_t r = 0; r < d; r++)
            for (uint32_t c = 0; c < d; c++) {
                const double kept = keep * C[(size_t)r * d + c];
                C[(size_t)r * d + c] = r == c ? kept + target : kept;
            }
        std::vector<double> L(dd, 0.0), Li(dd, 0.0);
        for (uint32_t i = 0; i < d; i++)
            for (uint32_t j = 0; j <= i; j++) {
                double s = 0.0;
                for (uint32_t k = 0; k < j; k++) {
                    const double p = L[(size_t)i * d + k] * L[(size_t)j * d + k];
                    s = s + p;
                }
                const double rest = C[(size_t)i * d + j] - s;
                if (j == i) {
                    if (!positive_finite(rest)) return STATUS_NOT_POSITIVE;
                    L[(size_t)i * d + i] = sqrt(rest);
                } else {
                    L[(size_t)i * d + j] = rest / L[(size_t)j * d + j];
                }
            }
        for (uint32_t j = 0; j < d; j++) {
            Li[(size_t)j * d + j] = 1.0 / L[(size_t)j * d + j];
            for (uint32_t i = j + 1; i < d; i++) {
                double s = 0.0;
                for (uint32_t k = j; k < i; k++) {
                    const double p = L[(size_t)i * d + k] * Li[(size_t)k * d + j];
                    s = s + p;
                }
                Li[(size_t)i * d + j] = (0.0 - s) / L[(size_t)i * d + i];
            }
        }
        for (uint32_t r = 0; r < d; r++)
            for (uint32_t c = r; c < d; c++) {
                double s = 0.0;
                for (uint32_t k = c; k < d; k++) {
                    const double p = Li[(size_t)k * d + r] * Li[(size_t)k * d + c];
                    s = s + p;
                }
                W[(size_t)r * d + c] = W[(size_t)c * d + r] = s;
            }
    }
    if (W_out) *W_out = W;
    double tr = 0.0;
    for (uint32_t r = 0; r < d; r++) tr = tr + W[(size_t)r * d + r];
    const double scale = (double)d / tr;
    if (!positive_finite(scale)) return STATUS_NOT_POSITIVE;
    for (size_t e = 0; e < dd; e++) {
        const double v = W[e] * scale;
        M[e] = (float)v;
    }
    return STATUS_OK;
}

}  // namespace covmetric
}  // namespace bg
