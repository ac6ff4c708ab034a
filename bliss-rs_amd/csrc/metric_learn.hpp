// metric_learn.hpp -- the host side of triplet metric learning (blissgpu_learn_metric): the state, the matrix M_t it stands for,
// the objective, the projected-gradient update and the loop around a gradient evaluation that the caller supplies.  No device
// code and no HIP header: tests/cpp/test_metric_learn.cpp feeds it recorded gradients, plain and under sanitizers.
//
// Every operation is f64, one rounding per multiply and per add, sums ascending from 0.0.  Each product stands in a statement
// of its own, so no compiler contracts it with the add that follows; build with -ffp-contract=off where the compiler would
// contract across statements.
//
//   DIAGONAL  state w[d], w_0 = init;                M_t = diag((float) w)
//   FULL      state L[d][d], L_0 = diag(sqrt(init)); M_t[i][j] = (float) sum_k L[k][i] L[k][j]  (upper half, mirrored)
//   M_0 = diag(init).  obj_t = loss_t / (2 T) + reg * sum_ij (M_t - M_0)^2, row-major.
//   Gt = G_t / (2 T) + (2 reg) (M_t - M_0);  DIAGONAL: w <- max(0, w - lr Gt[r][r]);  FULL: L <- L - (2 lr) (L Gt).
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

namespace bg {
namespace metric {

constexpr int FORM_DIAGONAL = 0, FORM_FULL = 1;
constexpr int STATUS_CONVERGED = 0, STATUS_MAX_ITER = 1, STATUS_DIVERGED = 2;
constexpr int STEP_NAN = 5;  // = BLISSGPU_ERR_NAN: what a step returns for a NaN hinge

struct Learner {
    int form = FORM_FULL;
    uint32_t d = 0;
    uint64_t T = 0;
    double lr = 0.0, reg = 0.0;
    std::vector<double> w, L, Gt, P;
    std::vector<float> M0, M;

    // init: d non-negative finite weights, or NULL for ones
    void start(int form_, uint32_t d_, const float* init, uint64_t T_, double lr_, double reg_) {
        form = form_; d = d_; T = T_; lr = lr_; reg = reg_;
        const size_t dd = (size_t)d * d;
        w.assign(d, 0.0); L.assign(form == FORM_FULL ? dd : 0, 0.0); Gt.assign(dd, 0.0); P.assign(form == FORM_FULL ? dd : 0, 0.0);
        M0.assign(dd, 0.0f); M.assign(dd, 0.0f);
        for (uint32_t r = 0; r < d; r++) {
            const float v = init ? init[r] : 1.0f;
            M0[(size_t)r * d + r] = v;
            w[r] = (double)v;
            if (form == FORM_FULL) L[(size_t)r * d + r] = sqrt((double)v);
        }
    }

    void build_m() {
        if (form == FORM_DIAGONAL) {
            for (uint32_t r = 0; r < d; r++) M[(size_t)r * d + r] = (float)w[r];
            return;
        }
        for (uint32_t i = 0; i < d; i++)
            for (uint32_t j = i; j < d; j++) {
                double s = 0.0;
                for (uint32_t k = 0; k < d; k++) {
                    const double p = L[(size_t)k * d + i] * L[(size_t)k * d + j];
                    s = s + p;
                }
                M[(size_t)i * d + j] = M[(size_t)j * d + i] = (float)s;
            }
    }

    bool m_finite() const {
        for (float v : M)
            if (!isfinite(v)) return false;
        return true;
    }

    double objective(double loss) const {
        double s = 0.0;
        for (size_t e = 0; e < M.size(); e++) {
            const double diff = (double)M[e] - (double)M0[e];
            const double sq = diff * diff;
            s = s + sq;
        }
        const double fit = T ? loss / (2.0 * (double)T) : 0.0;
        const double pen = reg * s;
        return fit + pen;
    }

    void update(const double* G) {
        const double two_t = 2.0 * (double)T, two_reg = 2.0 * reg;
        for (size_t e = 0; e < M.size(); e++) {
            const double diff = (double)M[e] - (double)M0[e];
            const double pull = two_reg * diff;
            const double fit = T ? G[e] / two_t : 0.0;
            Gt[e] = fit + pull;
        }
        if (form == FORM_DIAGONAL) {
            for (uint32_t r = 0; r < d; r++) {
                const double stepped = lr * Gt[(size_t)r * d + r];
                const double v = w[r] - stepped;
                w[r] = v > 0.0 ? v : 0.0;  // (a NaN is clamped to 0 as well)
            }
            return;
        }
        for (uint32_t i = 0; i < d; i++)
            for (uint32_t j = 0; j < d; j++) {
                double s = 0.0;
                for (uint32_t k = 0; k < d; k++) {
                    const double p = L[(size_t)i * d + k] * Gt[(size_t)k * d + j];
                    s = s + p;
                }
                P[(size_t)i * d + j] = s;
            }
        const double two_lr = 2.0 * lr;
        for (size_t e = 0; e < L.size(); e++) {
            const double stepped = two_lr * P[e];
            L[e] = L[e] - stepped;
        }
    }
};

// step(M, &loss, &active, G) evaluates the gradient at M: 0, STEP_NAN or another error code (returned as it is).
// obj / active (may be NULL): n_iter + 1 entries are written, so max_iter + 1 must fit.  M_out [d][d].
// Iteration t: M_t or obj_t not finite (a step that returns STEP_NAN after the first counts as such, with obj_t = NaN) ->
// DIVERGED; active_t == 0 -> CONVERGED; t == max_iter -> MAX_ITER; else update.  M_out = the M of the finite iteration with the
// lowest obj, the first such (M_0 when there is none).
template <class Step>
int learn(int form, uint32_t d, const float* init, uint64_t T, double lr, double reg, uint32_t max_iter, Step step, float* M_out,
          double* obj, uint64_t* active, uint32_t* n_iter, uint32_t* best_iter, int32_t* status) {
    Learner s;
    s.start(form, d, init, T, lr, reg);
    std::vector<double> G((size_t)d * d);
    std::vector<float> best_m = s.M0;
    double best_obj = 0.0;
    bool have_best = false;
    uint32_t t = 0, best_t = 0;
    int st;
    for (;; t++) {
        s.build_m();
        double loss = 0.0, o = NAN;
        uint64_t act = 0;
        int rc = s.m_finite() ? step(s.M.data(), &loss, &act, G.data()) : STEP_NAN;
        if (rc && !(rc == STEP_NAN && t > 0)) return rc;
        if (!rc) o = s.objective(loss);
        if (obj) obj[t] = o;
        if (active) active[t] = rc ? 0 : act;
        if (!isfinite(o)) { st = STATUS_DIVERGED; break; }
        if (!have_best || o < best_obj) {
            have_best = true;
            best_obj = o;
            best_t = t;
            best_m = s.M;
        }
        if (act == 0) { st = STATUS_CONVERGED; break; }
        if (t == max_iter) { st = STATUS_MAX_ITER; break; }
        s.update(G.data());
    }
    for (size_t e = 0; e < best_m.size(); e++) M_out[e] = best_m[e];
    *n_iter = t;
    *best_iter = best_t;
    *status = st;
    return 0;
}

}  // namespace metric
}  // namespace bg
