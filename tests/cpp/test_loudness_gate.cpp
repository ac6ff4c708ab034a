// test_loudness_gate.cpp -- bliss-rs_amd/csrc/loudness_gate.hpp as a stand-alone program (tests/test_loudness_host.py builds it
// plainly and with -fsanitize=address,undefined; it is never loaded into another process).
//
//   test_loudness_gate IN OUT     IN and OUT are files of f64.  IN is a sequence of cases:
//     0 n P[n]                      -> power lufs
//     1 n ST[n]                     -> range_lu lo hi
//     2 channels n_sub hop z[..]    -> P[max(n_sub - 3, 0)] ST[max(n_sub - 29, 0)]
//     3 rate                        -> coef[10] factor h[49] hop subblocks(1000000 frames)
#include <stdio.h>

#include <vector>

#include "../../bliss-rs_amd/csrc/loudness_gate.hpp"

static std::vector<double> read_all(const char* path) {
    std::vector<double> v;
    FILE* f = fopen(path, "rb");
    if (!f) return v;
    double x;
    while (fread(&x, sizeof(x), 1, f) == 1) v.push_back(x);
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const std::vector<double> in = read_all(argv[1]);
    std::vector<double> out;
    size_t at = 0;
    while (at < in.size()) {
        const int kind = (int)in[at++];
        if (kind == 0 || kind == 1) {
            const size_t n = (size_t)in[at++];
            if (at + n > in.size()) return 3;
            std::vector<double> v(in.begin() + at, in.begin() + at + n);  // its own allocation: a read past n is a report
            at += n;
            if (kind == 0) {
                const double power = bg::loud_gate(v.data(), v.size());
                out.push_back(power);
                out.push_back(bg::loud_lufs(power));
            } else {
                double lo, hi;
                out.push_back(bg::loud_range(v.data(), v.size(), &lo, &hi));
                out.push_back(lo);
                out.push_back(hi);
            }
        } else if (kind == 2) {
            const uint32_t channels = (uint32_t)in[at++];
            const size_t n_sub = (size_t)in[at++];
            const uint32_t hop = (uint32_t)in[at++];
            if (at + channels * n_sub > in.size()) return 3;
            std::vector<double> z(in.begin() + at, in.begin() + at + channels * n_sub);
            at += channels * n_sub;
            std::vector<double> P(n_sub >= 4 ? n_sub - 3 : 0), ST(n_sub >= 30 ? n_sub - 29 : 0);
            bg::loud_blocks(z.data(), channels, n_sub, hop, P.data(), ST.data());
            out.insert(out.end(), P.begin(), P.end());
            out.insert(out.end(), ST.begin(), ST.end());
        } else if (kind == 3) {
            const uint32_t rate = (uint32_t)in[at++];
            double coef[10], h[bg::LOUD_TAPS];
            bg::loud_kweighting(rate, coef);
            const uint32_t factor = bg::loud_peak_factor(rate);
            bg::loud_peak_filter(factor, h);
            out.insert(out.end(), coef, coef + 10);
            out.push_back((double)factor);
            out.insert(out.end(), h, h + bg::LOUD_TAPS);
            out.push_back((double)bg::loud_hop(rate));
            out.push_back((double)bg::loud_subblocks(1000000, rate));
        } else {
            return 4;
        }
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f) return 5;
    const size_t wrote = fwrite(out.data(), sizeof(double), out.size(), f);
    fclose(f);
    return wrote == out.size() ? 0 : 6;
}
