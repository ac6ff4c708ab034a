// test_metric_learn.cpp -- the host side of blissgpu_learn_metric (bliss-rs_amd/csrc/metric_learn.hpp) without a device: the
// gradient evaluations are replayed from a file, the loop's outputs and every M_t it asked a gradient for go to another.
// tests/test_metric_host.py writes the input, restates the loop in numpy scalars and compares bit for bit; the same source is
// built plain and with -fsanitize=address,undefined.
//
//   test_metric_learn <in> <out>
//   in : i32 form | u32 d | u64 T | f64 lr | f64 reg | u32 max_iter | u32 n_steps | u32 has_init | f32 init[d] (has_init) |
//        n_steps x { i32 rc | u64 active | f64 loss | f64 G[d][d] }
//   out: i32 rc | i32 status | u32 n_iter | u32 best_iter | u32 steps_used | f32 M[d][d] | f64 obj[n_iter + 1] |
//        u64 active[n_iter + 1] | steps_used x f32 M_t[d][d]
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../bliss-rs_amd/csrc/metric_learn.hpp"

namespace {

struct Reader {
    std::vector<unsigned char> b;
    size_t at = 0;
    bool bad = false;
    template <class T>
    T get() {
        T v{};
        if (at + sizeof(T) > b.size()) { bad = true; return v; }
        memcpy(&v, b.data() + at, sizeof(T));
        at += sizeof(T);
        return v;
    }
};

template <class T>
void put(FILE* f, const T* p, size_t n) {
    if (n) fwrite(p, sizeof(T), n, f);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    Reader r;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        unsigned char buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), f)) > 0) r.b.insert(r.b.end(), buf, buf + got);
        fclose(f);
    }
    const int32_t form = r.get<int32_t>();
    const uint32_t d = r.get<uint32_t>();
    const uint64_t T = r.get<uint64_t>();
    const double lr = r.get<double>(), reg = r.get<double>();
    const uint32_t max_iter = r.get<uint32_t>(), n_steps = r.get<uint32_t>(), has_init = r.get<uint32_t>();
    if (r.bad || d == 0 || d > 64 || max_iter > 100000) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<float> init(d);
    if (has_init)
        for (uint32_t k = 0; k < d; k++) init[k] = r.get<float>();
    const size_t dd = (size_t)d * d;
    struct Rec { int32_t rc; uint64_t active; double loss; std::vector<double> G; };
    std::vector<Rec> recs(n_steps);
    for (auto& rec : recs) {
        rec.rc = r.get<int32_t>();
        rec.active = r.get<uint64_t>();
        rec.loss = r.get<double>();
        rec.G.resize(dd);
        for (auto& g : rec.G) g = r.get<double>();
    }
    if (r.bad) { fprintf(stderr, "truncated input\n"); return 2; }

    std::vector<float> seen;  // every M_t a gradient was asked for
    uint32_t used = 0;
    bool ran_out = false;
    auto step = [&](const float* M, double* loss, uint64_t* active, double* G) -> int {
        if (used >= recs.size()) { ran_out = true; return 99; }
        seen.insert(seen.end(), M, M + dd);
        const Rec& rec = recs[used++];
        *loss = rec.loss;
        *active = rec.active;
        memcpy(G, rec.G.data(), dd * sizeof(double));
        return rec.rc;
    };
    std::vector<float> M(dd, -1.0f);
    std::vector<double> obj((size_t)max_iter + 1, -1.0);
    std::vector<uint64_t> active((size_t)max_iter + 1, 77);
    uint32_t n_iter = 0, best_iter = 0;
    int32_t status = -1;
    const int32_t rc = bg::metric::learn(form, d, has_init ? init.data() : nullptr, T, lr, reg, max_iter, step, M.data(), obj.data(),
                                         active.data(), &n_iter, &best_iter, &status);
    if (ran_out) { fprintf(stderr, "the loop asked for more gradients than were recorded\n"); return 3; }
    FILE* f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    put(f, &rc, 1); put(f, &status, 1); put(f, &n_iter, 1); put(f, &best_iter, 1); put(f, &used, 1);
    put(f, M.data(), dd);
    const size_t k = rc ? 0 : (size_t)n_iter + 1;
    put(f, obj.data(), k);
    put(f, active.data(), k);
    put(f, seen.data(), seen.size());
    fclose(f);
    printf("rc=%d status=%d n_iter=%u best_iter=%u steps=%u\n", rc, status, n_iter, best_iter, used);
    return 0;
}
