// test_covariance_metric.cpp -- drives bliss-rs_amd/csrc/covariance_metric.hpp (the host solve of blissgpu_covariance_metric)
// without a device, so that tests/test_moments_host.py can compare it bit for bit with its numpy restatement, and run it under
// AddressSanitizer / UBSan.
//
//   test_covariance_metric <case.in> <case.out>
// case.in  (little endian): u32 d, u32 form, u64 dof, f64 shrink, then S f64[d][d]
// case.out: i32 status, f32 M[d][d] (prefilled with 7.0f: untouched when the status is not OK), f64 W[d][d] (the unscaled inverse)
#include <stdio.h>
#include <stdlib.h>

#include "../../bliss-rs_amd/csrc/covariance_metric.hpp"

static void die(const char* what) {
    fprintf(stderr, "test_covariance_metric: %s\n", what);
    exit(2);
}

int main(int argc, char** argv) {
    if (argc != 3) die("usage: test_covariance_metric <case.in> <case.out>");
    FILE* f = fopen(argv[1], "rb");
    if (!f) die("cannot open the input");
    uint32_t d = 0, form = 0;
    uint64_t dof = 0;
    double shrink = 0.0;
    if (fread(&d, 4, 1, f) != 1 || fread(&form, 4, 1, f) != 1 || fread(&dof, 8, 1, f) != 1 || fread(&shrink, 8, 1, f) != 1) die("short header");
    if (d == 0 || d > 64 || dof == 0) die("bad header");
    const size_t dd = (size_t)d * d;
    std::vector<double> S(dd), W;
    if (fread(S.data(), sizeof(double), dd, f) != dd) die("short matrix");
    fclose(f);
    std::vector<float> M(dd, 7.0f);
    const int32_t status = bg::covmetric::solve(S.data(), d, dof, (int)form, shrink, M.data(), &W);
    W.resize(dd, 0.0);
    FILE* o = fopen(argv[2], "wb");
    if (!o) die("cannot open the output");
    if (fwrite(&status, 4, 1, o) != 1 || fwrite(M.data(), sizeof(float), dd, o) != dd || fwrite(W.data(), sizeof(double), dd, o) != dd)
        die("short write");
    fclose(o);
    return 0;
}
