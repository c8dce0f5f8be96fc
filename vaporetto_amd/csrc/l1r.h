// liblinear's coordinate descent for L1-regularised L2-loss SVC (linear.cpp: solve_l1r_l2_svc, solver 5), one column's step and the
// order of a sweep, host and device code: the one transcript that the device kernels (kernels_train_l1.hip over global memory,
// kernels_train_tags_l1.hip a tag problem in LDS), the host driver (capi_train.cpp, solve_l1r) and the native check
// (tests/native/l1r_test.cpp) share.
//
//   min_w  |w|_1 + C sum_i max(0, b_i)^2,   b_i = 1 - y_i w.x_i,   the bias a column of ones inside the norm, as liblinear has it.
//
// A column j is updated from three sums over its nonzeros, with v = x_ij y_i:
//   G_loss = -2 C sum_{b_i > 0} v b_i     H = max(2 C sum_{b_i > 0} v^2, 1e-12)     (one pass)
//   loss_old = C sum_{b_i > 0} b_i^2      loss_new = C sum_{b_i - d v > 0} (b_i - d v)^2   (a pass per line-search step that needs one)
// A backend B owes the step those sums, the same value in every thread that steers it, and the write of b once a step is accepted:
//   grad_sums()      {sum of l1r_grad_term over the column}: G_loss = -2 a, H = 2 b
//   loss_sums(d)     {loss_old, loss_new} for the trial step d
//   commit(d)        b_i -= d v over the column
// Every decision -- the violation, the Newton direction, the data-free acceptance test, the halvings -- is made here.
//
// Divergences from liblinear, on purpose: no shrinking (every column is visited in every sweep); b is not written during the line
// search (b - d v is computed on the fly and stored once, so the stored b is one rounding of b - d v where liblinear's is the sum of
// its trial updates); a step that is not accepted after 20 halvings is dropped (d = 0, b untouched) where liblinear adds the last
// trial and recomputes b from w.
//
// Order of a sweep: the columns are partitioned into groups (capi_train.cpp, l1r_groups) whose columns share no row, so a group is
// updated in one launch; the groups are permuted anew for every sweep by Fisher-Yates over splitmix64 from kL1rSeed, the state carried
// from sweep to sweep: for i = n - 1 down to 1, swap(order[i], order[next() % (i + 1)]).
#pragma once
#include <cmath>
#include <cstdint>

#include "layout.h"

namespace vpt {

constexpr double kL1rSigma = 0.01;          // sufficient decrease
constexpr int kL1rMaxLinesearch = 20;       // max_num_linesearch
constexpr int kL1rMaxSweeps = 1000;         // max_iter
constexpr uint64_t kL1rSeed = 0x5EED5EED5EED5EEDull;

// splitmix64 (Steele, Lea, Flood 2014)
VPT_HD uint64_t l1r_next(uint64_t* state) {
    uint64_t z = (*state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the order of the next sweep: order[0 .. n) permuted in place
VPT_HD void l1r_shuffle(uint32_t* order, uint32_t n, uint64_t* state) {
    for (uint32_t i = n; i-- > 1;) {
        const uint32_t j = uint32_t(l1r_next(state) % (uint64_t(i) + 1));
        const uint32_t t = order[i];
        order[i] = order[j];
        order[j] = t;
    }
}

struct L1rPair {
    double a, b;
};
VPT_HD L1rPair l1r_add(L1rPair s, L1rPair t) { return {s.a + t.a, s.b + t.b}; }
// a nonzero's terms of the first pass: v = x y, b the row's 1 - y w.x
VPT_HD L1rPair l1r_grad_term(double b, double v, double c) {
    if (!(b > 0)) return {0.0, 0.0};
    const double tmp = c * v;
    return {tmp * b, tmp * v};
}
// ... and of a line-search pass for the trial step d
VPT_HD L1rPair l1r_loss_term(double b, double v, double c, double d) {
    const double b_new = b - d * v;
    return {b > 0 ? c * b * b : 0.0, b_new > 0 ? c * b_new * b_new : 0.0};
}

struct L1rStep {
    double d;           // what was added to w_j (0: skipped or dropped)
    double violation;   // the column's term of the sweep's stopping sum, at the w before the step
    uint32_t halvings;  // line-search halvings: each follows a pass over the column
};

// one column of solve_l1r_l2_svc at weight w; xj_sq = C sum x^2 over the whole column
template <typename B>
VPT_HD L1rStep l1r_column(B& be, double w, double xj_sq) {
    const L1rPair s = be.grad_sums();
    const double G = -2 * s.a;
    const double H = fmax(2 * s.b, 1e-12);
    const double Gp = G + 1, Gn = G - 1;
    double violation = 0;
    if (w == 0) {
        if (Gp < 0) violation = -Gp;
        else if (Gn > 0) violation = Gn;
    } else if (w > 0) violation = fabs(Gp);
    else violation = fabs(Gn);
    double d;
    if (Gp < H * w) d = -Gp / H;
    else if (Gn > H * w) d = -Gn / H;
    else d = -w;
    if (fabs(d) < 1.0e-12) return {0.0, violation, 0};
    double delta = fabs(w + d) - fabs(w) + G * d;
    uint32_t halvings = 0;
    int k = 0;
    for (; k < kL1rMaxLinesearch; ++k) {
        double cond = fabs(w + d) - fabs(w) - kL1rSigma * delta;
        if (xj_sq * d * d + G * d + cond <= 0) break;   // appxcond: no pass over the data
        const L1rPair l = be.loss_sums(d);
        cond = cond + l.b - l.a;
        if (cond <= 0) break;
        d *= 0.5;
        delta *= 0.5;
        ++halvings;
    }
    if (k == kL1rMaxLinesearch) return {0.0, violation, halvings};
    be.commit(d);
    return {d, violation, halvings};
}

}  // namespace vpt
