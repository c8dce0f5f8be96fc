// liblinear's trust-region Newton method (tron.cpp: tron, trcg) for l2r_lr_fun (solver 0) and l2r_l2_svc_fun (solver 2) of linear.cpp,
// as scikit-learn bundles it: CG without a preconditioner, eps_cg = 0.1, from w = 0.  The one transcript the trainer has, host and
// device code: the host driver (capi_train.cpp, Tron: every step a launch, every dot product read back) and the in-kernel solver
// (kernels_train_tags.hip, TagProb: a workgroup over vectors in LDS) are two backends of the template below, and the four kernels
// that evaluate a row's loss or gradient term take it from here.
//
// A backend B owes the algorithm, over its own vectors of n doubles (B::v):
//   fun(x)           the objective at x; leaves what grad needs (z = Xx)
//   grad(x, out)     the gradient at the x of the last fun; leaves what hv needs (D)
//   hv(x, out)       out = x + Xᵀ(D (Xx))
//   dot(a, b)        the same value in every thread that steers the loop
//   zero(x)  copy(x, out)  add(a, b, out)  axpy(a, x, y): y += a x  xpby(x, b, y): y = x + b y
// and the places where the two differ, which are behaviour (a zero's sign, a pass over LDS, a launch) and stay theirs:
//   cg_start()       s = 0, r = d = -g
//   cg_boundary(a)   s += a d, r -= a Hd: the last update of a CG that reached the trust region's boundary
//   cg_more(k)       whether CG may take a step after k of them (a cap; a failed launch)
//   ok()             whether anything failed: ends both loops
// Every decision -- the four radius updates, the boundary step, the three stopping rules -- is made here from those scalars alone.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/vaporetto_hip.h"
#include "layout.h"

namespace vpt {

// ::fun's term of a row with margin yz = y z
VPT_HD double tron_loss(double yz, double c, int solver) {
    if (solver == 0) return yz >= 0 ? c * log(1 + exp(-yz)) : c * (-yz + log(1 + exp(yz)));
    const double d = 1 - yz;
    return d > 0 ? c * d * d : 0.0;
}
// ::grad's terms of a row: gz (the entry of the vector Xᵀ is applied to) and D (Hv's diagonal)
struct TronRow {
    double gz, D;
};
VPT_HD TronRow tron_grad_row(double y, double yz, double c, int solver) {
    if (solver == 0) {
        const double s = 1 / (1 + exp(-yz));
        return {c * (s - 1) * y, c * s * (1 - s)};
    }
    if (yz < 1) return {2 * c * y * (yz - 1), 2 * c};
    return {0, 0};
}
// liblinear's primal tolerance (linear.cpp train_one): eps * max(min(pos, neg), 1) / l
VPT_HD double tron_tolerance(double eps, double pos, double l) { return eps * fmax(fmin(pos, l - pos), 1.0) / l; }

struct TronVectors {   // n doubles each
    double *w, *w_new, *g, *s, *r, *d, *Hd;
};

// trcg: the step s within radius delta and the residual r = -g - Hs; returns the CG steps taken
template <typename B>
VPT_HD int tron_trcg(B& b, double delta) {
    const TronVectors& v = b.v;
    b.cg_start();
    const double cgtol = 0.1 * sqrt(b.dot(v.g, v.g));
    int cg_iter = 0;
    double rTr = b.dot(v.r, v.r);
    while (b.cg_more(cg_iter)) {
        // tron.cpp takes dnrm2(r) anew here although rTr holds the same product: kept, so that the bits are liblinear's
        if (sqrt(b.dot(v.r, v.r)) <= cgtol) break;
        cg_iter++;
        b.hv(v.d, v.Hd);
        double alpha = rTr / b.dot(v.d, v.Hd);
        b.axpy(alpha, v.d, v.s);
        if (sqrt(b.dot(v.s, v.s)) > delta) {
            alpha = -alpha;
            b.axpy(alpha, v.d, v.s);
            const double std_ = b.dot(v.s, v.d), sts = b.dot(v.s, v.s), dtd = b.dot(v.d, v.d), dsq = delta * delta;
            const double rad = sqrt(std_ * std_ + dtd * (dsq - sts));
            alpha = std_ >= 0 ? (dsq - sts) / (std_ + rad) : (rad - std_) / dtd;
            b.cg_boundary(alpha);
            break;
        }
        alpha = -alpha;
        b.axpy(alpha, v.Hd, v.r);
        const double rnew = b.dot(v.r, v.r);
        const double beta = rnew / rTr;
        b.xpby(v.r, beta, v.d);
        rTr = rnew;
    }
    return cg_iter;
}

// tron: one training from w = 0 to |g| <= eps |g0|; the weights are left in b.v.w
template <typename B>
VPT_HD vpt_train_stats tron(B& b, double eps) {
    const double eta0 = 1e-4, eta1 = 0.25, eta2 = 0.75, sigma1 = 0.25, sigma2 = 0.5, sigma3 = 4;
    const int max_iter = 1000;
    const TronVectors& v = b.v;
    b.zero(v.w);
    double f = b.fun(v.w);
    b.grad(v.w, v.g);
    double delta = sqrt(b.dot(v.g, v.g));
    const double gnorm1 = delta;
    double gnorm = gnorm1;
    const bool search = !(gnorm <= eps * gnorm1);
    int iter = 1, cg_total = 0;
    while (iter <= max_iter && search && b.ok()) {
        cg_total += tron_trcg(b, delta);
        b.add(v.w, v.s, v.w_new);
        const double gs = b.dot(v.g, v.s);
        const double prered = -0.5 * (gs - b.dot(v.s, v.r));
        const double fnew = b.fun(v.w_new);
        const double actred = f - fnew;
        const double snorm = sqrt(b.dot(v.s, v.s));
        if (iter == 1) delta = fmin(delta, snorm);
        const double alpha = (fnew - f - gs <= 0) ? sigma3 : fmax(sigma1, -0.5 * (gs / (fnew - f - gs)));
        if (actred < eta0 * prered) delta = fmin(fmax(alpha, sigma1) * snorm, sigma2 * delta);
        else if (actred < eta1 * prered) delta = fmax(sigma1 * delta, fmin(alpha * snorm, sigma2 * delta));
        else if (actred < eta2 * prered) delta = fmax(sigma1 * delta, fmin(alpha * snorm, sigma3 * delta));
        else delta = fmax(delta, fmin(alpha * snorm, sigma3 * delta));
        if (actred > eta0 * prered) {
            iter++;
            b.copy(v.w_new, v.w);
            f = fnew;
            b.grad(v.w, v.g);
            gnorm = sqrt(b.dot(v.g, v.g));
            if (gnorm <= eps * gnorm1) break;
        }
        if (f < -1.0e+32) break;
        if (fabs(actred) <= 0 && prered <= 0) break;
        if (fabs(actred) <= 1.0e-12 * fabs(f) && fabs(prered) <= 1.0e-12 * fabs(f)) break;
    }
    return vpt_train_stats{uint32_t(iter - 1), uint32_t(cg_total), gnorm1, gnorm, f};
}

}  // namespace vpt
