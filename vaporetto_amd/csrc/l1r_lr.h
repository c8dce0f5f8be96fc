// liblinear's newGLMNET for L1-regularised logistic regression (linear.cpp: solve_l1r_lr, solver 6), host and device code: the one
// transcript that the device kernels (kernels_train_l1lr.hip), the host driver (capi_train.cpp, solve_l1r_lr) and the native check
// (tests/native/l1r_lr_test.cpp) share.
//
//   min_w  |w|_1 + C sum_i log(1 + exp(-y_i w.x_i)),   the bias a column of ones inside the norm, as liblinear has it.
//
// Per row the solver carries e_i = exp(w.x_i), tau_i = C / (1 + e_i), D_i = C e_i / (1 + e_i)^2 and, inside a Newton iteration,
// xTd_i = x_i.(wpd - w); per column xjneg_sum_j = C sum_{y_i = -1} x_ij (once), Hdiag_j = nu + sum x^2 D, Grad_j = -sum x tau +
// xjneg_sum_j and the trial weights wpd_j.  A Newton iteration: Hdiag, Grad and the violations at w (stop when their sum is <= tol *
// the first one); coordinate descent over wpd on the quadratic model, sweep after sweep until a sweep's violation sum is <= inner_eps
// * the first outer one; a line search over all rows that halves wpd - w until the objective has decreased enough.
//
// A backend B owes the algorithm sums and writes over its own vectors, the same scalar in every thread that steers the loop:
//   setup()              w = wpd = 0, e = 1, tau and D from e, xjneg_sum
//   grad()               Hdiag, Grad and the violations at w (l1lr_grad_term, l1lr_violation); returns the violations' sum
//   qp_start()           xTd = 0
//   cd_group(g)          group g's columns: G = Grad_j + (wpd_j - w_j) nu + sum x D xTd, l1lr_cd_step, wpd_j += z, xTd += z x
//   qp_violation()       the sum of the violations the last sweep's columns reported
//   direction_sums()     {sum Grad_j (wpd_j - w_j), |wpd|_1, C sum_{y = -1} xTd}
//   linesearch_loss()    sum of l1lr_ls_term over the rows
//   accept()             w = wpd; e, tau, D by l1lr_accept_row
//   halve()              wpd = (w + wpd) / 2, xTd /= 2; returns |wpd|_1
//   recompute()          e = exp(Xw) from w, wpd = w
//   ok()                 whether anything failed: ends every loop
// Every decision -- the violation, the soft threshold and its clamp, the three stopping rules, inner_eps, the acceptance test, the
// halvings -- is made here from those scalars alone.
//
// Divergences from liblinear, on purpose: no shrinking at either level (every column is visited by every grad() and every sweep, so
// there is no active-set reactivation either); a column's sum x D xTd is taken on its own and then added to Grad_j + (wpd_j - w_j) nu,
// where liblinear adds the terms onto that start one by one; the line search's row terms are summed and then added to the data-free
// part of cond; |w|_1 sums every entry (liblinear skips exact zeros: the same value); after 20 refused trials wpd is put back to w
// (liblinear keeps the last halved wpd while it zeroes xTd, so its next model starts from a point its xTd does not describe).
//
// Order of a sweep: the groups of l1r.h (capi_train.cpp, l1r_groups), permuted anew for every inner sweep by l1r_shuffle from kL1rSeed,
// the state carried across sweeps and Newton iterations.  The columns of a group share no row, so no column of a launch reads an xTd_i
// that another one writes: a sweep is sequential coordinate descent in the order "by group".
#pragma once
#include <cmath>
#include <cstdint>

#include "l1r.h"
#include "layout.h"

namespace vpt {

constexpr double kL1lrNu = 1e-12;           // nu
constexpr double kL1lrSigma = 0.01;         // sigma
constexpr int kL1lrMaxNewton = 100;         // max_newton_iter
constexpr int kL1lrMaxSweeps = 1000;        // max_iter of the inner loop
constexpr int kL1lrMaxLinesearch = 20;      // max_num_linesearch

// the three-branch rule of l1r_column: how far w_j with loss gradient G is from optimal
VPT_HD double l1lr_violation(double w, double G) {
    const double Gp = G + 1, Gn = G - 1;
    if (w == 0) {
        if (Gp < 0) return -Gp;
        if (Gn > 0) return Gn;
        return 0;
    }
    return w > 0 ? fabs(Gp) : fabs(Gn);
}

// a nonzero's terms of grad(): {x^2 D, x tau}; Hdiag = nu + a, Grad = -b + xjneg_sum
VPT_HD L1rPair l1lr_grad_term(double x, double D, double tau) { return {x * x * D, x * tau}; }
// ... of setup()'s xjneg_sum, in a
VPT_HD L1rPair l1lr_neg_term(double x, double y, double c) { return {y < 0 ? c * x : 0.0, 0.0}; }
// ... of a column's sum in cd_group, in a
VPT_HD L1rPair l1lr_qp_term(double x, double D, double xTd) { return {x * D * xTd, 0.0}; }

struct L1lrStep {
    double z;           // what is added to wpd_j (0: the column is skipped)
    double violation;   // the column's term of the sweep's stopping sum, at the wpd before the step
};
// one column of the inner loop: G the model's gradient at wpd, H = Hdiag_j
VPT_HD L1lrStep l1lr_cd_step(double wpd, double G, double H) {
    const double violation = l1lr_violation(wpd, G);
    const double Gp = G + 1, Gn = G - 1;
    double z;
    if (Gp < H * wpd) z = -Gp / H;
    else if (Gn > H * wpd) z = -Gn / H;
    else z = -wpd;
    if (fabs(z) < 1.0e-12) return {0.0, violation};
    z = fmin(fmax(z, -10.0), 10.0);
    return {z, violation};
}

struct L1lrRow {
    double e, tau, D;
};
// a row's state from its e = exp(w.x)
VPT_HD L1lrRow l1lr_row(double e, double c) {
    const double tau_tmp = 1 / (1 + e);
    return {e, c * tau_tmp, c * e * tau_tmp * tau_tmp};
}
// ... after the step xTd was accepted
VPT_HD L1lrRow l1lr_accept_row(double e, double xTd, double c) { return l1lr_row(e * exp(xTd), c); }
// a row's term of the line search: C log((1 + e') / (exp(xTd) + e')), e' = e exp(xTd)
VPT_HD double l1lr_ls_term(double e, double xTd, double c) {
    const double exp_xTd = exp(xTd);
    const double e_new = e * exp_xTd;
    return c * log((1 + e_new) / (exp_xTd + e_new));
}

struct L1lrSums {
    double delta, wpd_norm1, negsum_xTd;
};
struct L1lrResult {
    uint32_t newton, sweeps, halvings;   // Newton iterations, inner sweeps over all of them, line-search halvings
    double gnorm0, gnorm;                // the first and the last violation sum at w
};

// one training from w = 0; tol: tron_tolerance(eps, pos, l); order[0 .. n_groups): the groups, permuted in place.  The weights are
// left in the backend's w.
template <typename B>
VPT_HD L1lrResult l1r_lr(B& b, double tol, uint32_t* order, uint32_t n_groups) {
    uint64_t rng = kL1rSeed;
    double inner_eps = 1, w_norm = 0, gnorm_init = 0, gnorm_new = 0;
    uint32_t newton = 0, sweeps = 0, halvings = 0;
    b.setup();
    while (newton < uint32_t(kL1lrMaxNewton) && b.ok()) {
        gnorm_new = b.grad();
        if (newton == 0) gnorm_init = gnorm_new;
        if (gnorm_new <= tol * gnorm_init) break;
        b.qp_start();
        int iter = 0;
        while (iter < kL1lrMaxSweeps && b.ok()) {
            l1r_shuffle(order, n_groups, &rng);
            for (uint32_t g = 0; g < n_groups; ++g) b.cd_group(order[g]);
            const double qp_gnorm = b.qp_violation();
            iter++;
            if (qp_gnorm <= inner_eps * gnorm_init) break;
        }
        sweeps += uint32_t(iter);
        const L1lrSums s = b.direction_sums();
        double w_norm_new = s.wpd_norm1;
        double delta = s.delta + (w_norm_new - w_norm);
        double negsum_xTd = s.negsum_xTd;
        int k = 0;
        for (; k < kL1lrMaxLinesearch && b.ok(); ++k) {
            const double cond = w_norm_new - w_norm + negsum_xTd - kL1lrSigma * delta + b.linesearch_loss();
            if (cond <= 0) {
                w_norm = w_norm_new;
                b.accept();
                break;
            }
            w_norm_new = b.halve();
            delta *= 0.5;
            negsum_xTd *= 0.5;
            ++halvings;
        }
        if (k >= kL1lrMaxLinesearch) b.recompute();
        if (iter == 1) inner_eps *= 0.25;
        newton++;
    }
    return {newton, sweeps, halvings, gnorm_init, gnorm_new};
}

}  // namespace vpt
