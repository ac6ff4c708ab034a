// loudness_gate.hpp -- the device-free half of the loudness measurement (include/blissgpu.h): the K-weighting
// coefficients and the true-peak interpolator for a sample rate, and everything behind the device's sub-block energies -- the
// 400 ms blocks, the 3 s short-term powers, the two gates of ITU-R BS.1770-4 and the loudness range of EBU Tech 3342.
//
// The device delivers z[c][u], the sum of the squared K-weighted samples of channel c over sub-block u (100 ms); everything here
// is a handful of f64 operations per sub-block, each rounded on its own, every sum sequential in the order the header states.
// No HIP: the CPU tests compile this file alone, under AddressSanitizer too.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace bg {

constexpr uint32_t LOUD_MIN_RATE = 8000, LOUD_MAX_RATE = 768000;
constexpr uint32_t LOUD_BLOCK_SUBS = 4, LOUD_SHORT_SUBS = 30;  // 400 ms and 3 s in sub-blocks of 100 ms
constexpr int LOUD_TAPS = 49;                                  // the true-peak interpolator's taps
constexpr double LOUD_ABS_GATE = 1.1724653045822981e-07;       // -70 LUFS as a power: the literal is the contract

inline bool loud_rate_ok(uint32_t rate) { return rate >= LOUD_MIN_RATE && rate <= LOUD_MAX_RATE; }
// samples per sub-block: 100 ms, rounded to the nearest sample
inline uint32_t loud_hop(uint32_t rate) { return (rate + 5) / 10; }
inline uint64_t loud_subblocks(uint64_t frames, uint32_t rate) { return loud_rate_ok(rate) ? frames / loud_hop(rate) : 0; }

// coef [10] = stage 1 (b0 b1 b2 a1 a2), stage 2 (b0 b1 b2 a1 a2): the bilinear form of the two K-weighting biquads
inline void loud_kweighting(uint32_t rate, double* coef) {
    const double pi = 3.14159265358979323846;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = tan(pi * f0 / (double)rate), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        coef[0] = (Vh + Vb * K / Q + K * K) / a0;
        coef[1] = 2.0 * (K * K - Vh) / a0;
        coef[2] = (Vh - Vb * K / Q + K * K) / a0;
        coef[3] = 2.0 * (K * K - 1.0) / a0;
        coef[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = tan(pi * f0 / (double)rate);
        const double a0 = 1.0 + K / Q + K * K;
        coef[5] = 1.0;
        coef[6] = -2.0;
        coef[7] = 1.0;
        coef[8] = 2.0 * (K * K - 1.0) / a0;
        coef[9] = (1.0 - K / Q + K * K) / a0;
    }
}

// the oversampling factor of the true peak at a rate, and the 49-tap Hann-windowed sinc for it
inline uint32_t loud_peak_factor(uint32_t rate) { return rate < 96000 ? 4 : rate < 192000 ? 2 : 1; }
inline void loud_peak_filter(uint32_t factor, double* h) {
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < LOUD_TAPS; i++) {
        const double t = (double)(i - 24) / (double)factor;
        const double sinc = t == 0.0 ? 1.0 : sin(pi * t) / (pi * t);
        h[i] = sinc * (0.5 * (1.0 - cos(2.0 * pi * (double)i / 48.0)));
    }
}

// z [channels][n_sub] -> P [n_sub - 3] (n_sub >= 4) and ST [n_sub - 29] (n_sub >= 30); either output may be NULL
inline void loud_blocks(const double* z, uint32_t channels, uint64_t n_sub, uint32_t hop, double* P, double* ST) {
    if (P && n_sub >= LOUD_BLOCK_SUBS) {
        const double norm = (double)(4ull * hop);
        for (uint64_t j = 0; j + LOUD_BLOCK_SUBS <= n_sub; j++) {
            double sum = 0.0;
            for (uint32_t c = 0; c < channels; c++) {
                const double* zc = z + (uint64_t)c * n_sub + j;
                sum = sum + (((zc[0] + zc[1]) + zc[2]) + zc[3]);
            }
            P[j] = sum / norm;
        }
    }
    if (ST && n_sub >= LOUD_SHORT_SUBS) {
        const double norm = (double)(30ull * hop);
        for (uint64_t j = 0; j + LOUD_SHORT_SUBS <= n_sub; j++) {
            double sum = 0.0;
            for (uint32_t c = 0; c < channels; c++)
                for (uint32_t u = 0; u < LOUD_SHORT_SUBS; u++) sum = sum + z[(uint64_t)c * n_sub + j + u];
            ST[j] = sum / norm;
        }
    }
}

// the mean of the values above `gate`, sequential in their order; *count = how many there are (0: the mean is 0)
inline double loud_mean_above(const double* v, uint64_t n, double gate, uint64_t* count) {
    double sum = 0.0;
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; i++)
        if (v[i] > gate) {
            sum = sum + v[i];
            k++;
        }
    *count = k;
    return k ? sum / (double)k : 0.0;
}

inline double loud_lufs(double power) { return -0.691 + 10.0 * log10(power); }  // power 0: -inf

// BS.1770-4's two gates over block powers: the power of the integrated loudness (0: no block above -70 LUFS)
inline double loud_gate(const double* P, uint64_t n) {
    uint64_t count = 0;
    const double gamma = loud_mean_above(P, n, LOUD_ABS_GATE, &count) * 0.1;
    if (!count) return 0.0;
    double sum = 0.0;
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; i++)
        if (P[i] > LOUD_ABS_GATE && P[i] > gamma) {
            sum = sum + P[i];
            k++;
        }
    return k ? sum / (double)k : 0.0;
}

// EBU Tech 3342 over short-term powers: *lo and *hi are the 10th and 95th percentile powers (0 when nothing passes the gates)
inline double loud_range(const double* ST, uint64_t n, double* lo, double* hi) {
    *lo = *hi = 0.0;
    uint64_t count = 0;
    const double gate = loud_mean_above(ST, n, LOUD_ABS_GATE, &count) * 0.01;
    if (!count) return 0.0;
    std::vector<double> kept;
    kept.reserve(count);
    for (uint64_t i = 0; i < n; i++)
        if (ST[i] > LOUD_ABS_GATE && ST[i] > gate) kept.push_back(ST[i]);
    if (kept.empty()) return 0.0;
    std::sort(kept.begin(), kept.end());
    const uint64_t m = kept.size();
    *lo = kept[(uint64_t)((double)(m - 1) * 0.10 + 0.5)];
    *hi = kept[(uint64_t)((double)(m - 1) * 0.95 + 0.5)];
    return 10.0 * log10(*hi / *lo);
}

}  // namespace bg
