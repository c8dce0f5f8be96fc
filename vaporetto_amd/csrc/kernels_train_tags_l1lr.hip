// Tag-model training with solver 6 (L1-regularised logistic regression, liblinear's newGLMNET): every (surface, slot) problem that
// fits, a workgroup per problem in one launch, one class after another over the same 0/1 matrix (one solve for two classes).
//
// The algorithm is l1r_lr.h's; this file is its in-kernel backend, as kernels_train_l1lr.hip is its backend over global memory.  All
// 256 threads run l1r_lr<B> side by side: every sum the backend returns has the same bits in every thread, so every thread takes the
// header's decisions alike and the barriers inside the backend's steps are met by all.
//
// Where the state lives.  In LDS what a sweep gathers or scatters per nonzero, and the one feature vector a sweep writes: tau, D and
// xTd (rows each) and wpd (features + 1, the bias last).  In global memory what is touched once per column or once per row of a pass:
// w (the output itself), Grad, Hdiag, xjneg_sum and the violations (features + 1 each) and e (rows).  So a problem fits iff
// 3 rows + (features + 1) <= kTagL1LdsDoubles.  The matrix's indices (CSR and CSC) stay in global memory.  A nonzero is 1
// (tag_rows_kernel: a row's columns are distinct) and y comes from the tag id.
//
// A sweep (cd_group): the problem's groups (capi_train.cpp, l1r_groups over the problem's keys: a template's columns share no row, the
// bias alone and last) in a new order, and for each group its columns dealt by length (l1r_team.h, tag_l1_deal); then the workgroup
// meets.  The header would have every thread permute the order; here it is handed one group -- the whole sweep -- which it cannot
// permute and for which it draws nothing, and thread 0 alone runs l1r_shuffle over the real groups in LDS from the backend's own state, kL1rSeed at
// setup and carried across sweeps and Newton iterations: the draws and the orders are those the global-memory driver gets.  grad() and
// setup()'s xjneg_sum deal all columns at once, as the one launch over all columns does: they write nothing that a column reads.
//
// The column team and its summation rule, the LDS behind the problem's vectors and the sums over rows or features are l1r_team.h's: a
// column's sums have the bits the group launches give them, and a sum over a vector has the shape of the host driver's; its terms are
// rounded before they are added, as the driver's term kernels store them.  No atomic on a double.
// A sum that is not finite clears `fine`, and ok() ends every loop of the header.
#include "kernels.hpp"

#include <cmath>

#include "device_common.h"
#include "l1r_lr.h"
#include "l1r_team.h"
#include "tron.h"

namespace vpt {
namespace {

constexpr uint32_t kT = kTrainThreads;

// solver 6's sums over a vector: a term is rounded before it is added, as the host driver's term kernels store it (l1r_team.h)
template <typename F>
__device__ double vec_sum(uint32_t n, F f, double* red) { return tag_l1_vec_sum<true>(n, f, red); }

struct Prob {
    const uint32_t *rp, *cols, *cp, *crow, *y;
    uint32_t nf, l, cls;
    double c;
    double *wpd, *tau, *D, *xTd;                     // LDS
    double *w, *grad, *hdiag, *xjneg, *viol, *e;     // global memory
    __device__ __forceinline__ double target(uint32_t r) const { return y[r] == cls ? 1.0 : -1.0; }
};

// a team of kN threads over one column: nonzeros a .. a + n of the CSC, or rows 0 .. n for the bias
template <uint32_t kN>
struct Team {
    const Prob& P;
    uint32_t a;
    bool bias;
    L1rTeam<kN, uint32_t> tm;

    __device__ __forceinline__ uint32_t row(uint32_t k) const { return bias ? k : P.crow[a + k]; }
    // f(row) over the column's nonzeros
    template <typename F>
    __device__ __forceinline__ L1rPair sums(F f) const {
        return tm.sums([this, f](uint32_t k) { return f(row(k)); });
    }
    // xTd_i += z over the column: its rows are distinct, and no other column of the group has them
    __device__ void add_xTd(double z) const {
        tm.each([this, z](uint32_t k) {
            const uint32_t r = row(k);
            P.xTd[r] = P.xTd[r] + z * 1.0;
        });
    }
};

enum : int { kNeg = 0, kGrad = 1, kCd = 2 };

// kNeg: xjneg_sum[j]; kGrad: Hdiag[j], Grad[j] and the violation at w[j]; kCd: the column's step of the inner loop.  As column() of
// kernels_train_l1lr.hip, with x = 1
template <uint32_t kN, int kMode>
__device__ void column(const Prob& P, uint32_t j, uint32_t t, L1rPair* s0, L1rPair* s1) {
    const bool bias = j == P.nf;
    const uint32_t a = bias ? 0 : P.cp[j], n = bias ? P.l : P.cp[j + 1] - a;
    const Team<kN> be{P, a, bias, {n, t, s0, s1}};
    if constexpr (kMode == kNeg) {
        const L1rPair s = be.sums([&P](uint32_t row) { return l1lr_neg_term(1.0, P.target(row), P.c); });
        if (t == 0) P.xjneg[j] = s.a;
    } else if constexpr (kMode == kGrad) {
        const L1rPair s = be.sums([&P](uint32_t row) { return l1lr_grad_term(1.0, P.D[row], P.tau[row]); });
        if (t != 0) return;
        const double G = -s.b + P.xjneg[j];
        P.hdiag[j] = kL1lrNu + s.a;
        P.grad[j] = G;
        P.viol[j] = l1lr_violation(P.w[j], G);
    } else {
        // every thread of the team reads wpd[j] before the first rendezvous of the sums; thread 0 writes it after the last
        const double w = P.w[j], wpd = P.wpd[j];
        const L1rPair s = be.sums([&P](uint32_t row) { return l1lr_qp_term(1.0, P.D[row], P.xTd[row]); });
        const double G = P.grad[j] + (wpd - w) * kL1lrNu + s.a;
        const L1lrStep step = l1lr_cd_step(wpd, G, P.hdiag[j]);
        if (step.z != 0) be.add_xTd(step.z);
        if (t != 0) return;
        P.viol[j] = step.violation;
        if (step.z != 0) P.wpd[j] = wpd + step.z;
    }
}

// l1r_lr.h's backend
struct Solver {
    Prob P;
    const TagL1Group* gr;      // the problem's groups and their columns
    const uint32_t* gc;
    uint32_t n_groups, n, t;   // n = features + 1
    TagL1Lds L;                // L.order: the groups' order, permuted by thread 0
    uint64_t rng;
    bool fine;

    template <int kMode>
    __device__ __forceinline__ void deal(const TagL1Group& G) {
        tag_l1_deal(G, gc + G.at, L, [this](auto kN, uint32_t j, uint32_t tt, L1rPair* s0, L1rPair* s1) { column<kN, kMode>(P, j, tt, s0, s1); });
    }
    template <int kMode>
    __device__ void all_columns() {
        for (uint32_t g = 0; g < n_groups; ++g) deal<kMode>(gr[g]);
        __syncthreads();
    }
    __device__ __forceinline__ double seen(double s) {
        if (!(fabs(s) <= 1.7976931348623157e308)) fine = false;
        return s;
    }

    __device__ bool ok() const { return fine; }
    __device__ void setup() {
        const L1lrRow r = l1lr_accept_row(1.0, 0.0, P.c);
        for (uint32_t j = t; j < n; j += kT) { P.w[j] = 0; P.wpd[j] = 0; }
        for (uint32_t i = t; i < P.l; i += kT) { P.xTd[i] = 0; P.e[i] = r.e; P.tau[i] = r.tau; P.D[i] = r.D; }
        if (t < n_groups) L.order[t] = t;
        rng = kL1rSeed;
        fine = true;
        __syncthreads();
        all_columns<kNeg>();
    }
    __device__ double grad() {
        all_columns<kGrad>();
        return seen(vec_sum(n, [this](uint32_t j) { return P.viol[j]; }, L.red));
    }
    __device__ void qp_start() {
        for (uint32_t i = t; i < P.l; i += kT) P.xTd[i] = 0;
        __syncthreads();
    }
    // the one group the header knows is the whole sweep
    __device__ void cd_group(uint32_t) {
        if (t == 0) l1r_shuffle(L.order, n_groups, &rng);
        __syncthreads();
        for (uint32_t q = 0; q < n_groups; ++q) {
            deal<kCd>(gr[L.order[q]]);
            __syncthreads();
        }
    }
    __device__ double qp_violation() {
        return seen(vec_sum(n, [this](uint32_t j) { return P.viol[j]; }, L.red));
    }
    __device__ L1lrSums direction_sums() {
        const double delta = vec_sum(n, [this](uint32_t j) { return P.grad[j] * (P.wpd[j] - P.w[j]); }, L.red);
        const double norm1 = vec_sum(n, [this](uint32_t j) { return fabs(P.wpd[j]); }, L.red);
        const double neg = vec_sum(P.l, [this](uint32_t i) { return P.target(i) < 0 ? P.c * P.xTd[i] : 0.0; }, L.red);
        return {seen(delta), seen(norm1), seen(neg)};
    }
    __device__ double linesearch_loss() {
        return seen(vec_sum(P.l, [this](uint32_t i) { return l1lr_ls_term(P.e[i], P.xTd[i], P.c); }, L.red));
    }
    __device__ void accept() {
        for (uint32_t j = t; j < n; j += kT) P.w[j] = P.wpd[j];
        for (uint32_t i = t; i < P.l; i += kT) {
            const L1lrRow r = l1lr_accept_row(P.e[i], P.xTd[i], P.c);
            P.e[i] = r.e; P.tau[i] = r.tau; P.D[i] = r.D;
        }
        __syncthreads();
    }
    __device__ double halve() {
        for (uint32_t j = t; j < n; j += kT) P.wpd[j] = (P.w[j] + P.wpd[j]) * 0.5;
        for (uint32_t i = t; i < P.l; i += kT) P.xTd[i] = P.xTd[i] * 0.5;
        __syncthreads();
        return seen(vec_sum(n, [this](uint32_t j) { return fabs(P.wpd[j]); }, L.red));
    }
    // w.x of row r through the CSR, the bias last: train_xv's order
    __device__ __forceinline__ double wx(uint32_t r) const {
        double z = 0;
        for (uint32_t k = P.rp[r]; k < P.rp[r + 1]; ++k) z += P.w[P.cols[k]];
        return z + P.w[P.nf];
    }
    __device__ void recompute() {
        for (uint32_t i = t; i < P.l; i += kT) P.e[i] = exp(wx(i));
        for (uint32_t j = t; j < n; j += kT) P.wpd[j] = P.w[j];
        __syncthreads();
    }
};

__global__ __launch_bounds__(kT) void tag_l1lr_solve_kernel(const TagSolveDesc* descs, const TagL1Desc* l1descs, const uint32_t* rp, const uint32_t* cols,
                                                            const uint32_t* cp, const uint32_t* crow, const uint32_t* y, const uint32_t* gcols,
                                                            const TagL1Group* groups, double eps, double c, double* scratch, double* w_out,
                                                            vpt_train_stats* stats) {
    __shared__ double lds[kTagL1Doubles];
    const TagSolveDesc D = descs[blockIdx.x];
    const TagL1Desc E = l1descs[blockIdx.x];
    const uint32_t n = D.nf + 1, l = D.l, t = threadIdx.x;
    if (3 * uint64_t(l) + n > kTagL1LdsDoubles || E.n_groups > kTagL1MaxGroups) return;   // the host sends such a problem down the other path
    double* const scr = scratch + E.viol;
    Solver S;
    Prob& P = S.P;
    P.rp = rp + D.rp; P.cols = cols + D.cols; P.cp = cp + D.cp; P.crow = crow + D.cols; P.y = y + D.y;
    P.nf = D.nf; P.l = l; P.c = c;
    P.wpd = lds; P.tau = lds + n; P.D = P.tau + l; P.xTd = P.D + l;
    P.viol = scr; P.grad = scr + n; P.hdiag = scr + 2 * uint64_t(n); P.xjneg = scr + 3 * uint64_t(n); P.e = scr + 4 * uint64_t(n);
    S.gr = groups + E.groups; S.gc = gcols + E.gcols; S.n_groups = E.n_groups; S.n = n; S.t = t;
    S.L = tag_l1_lds(lds);
    double* const red = S.L.red;
    const uint32_t n_solve = D.k == 2 ? 1 : D.k;
    for (uint32_t cls = 0; cls < n_solve; ++cls) {
        P.cls = cls;
        P.w = w_out + D.w + uint64_t(cls) * n;
        const double pos = vec_sum(l, [&](uint32_t i) { return P.y[i] == cls ? 1.0 : 0.0; }, red);
        uint32_t whole_sweep = 0;
        const L1lrResult r = l1r_lr(S, tron_tolerance(eps, pos, double(l)), &whole_sweep, 1);
        // the loss at the weights themselves, not at the e the iterations carried along
        const double loss = vec_sum(l, [&](uint32_t i) { return tron_loss(P.target(i) * S.wx(i), c, 0); }, red);
        const double norm1 = vec_sum(n, [&](uint32_t j) { return fabs(P.w[j]); }, red);
        if (D.k == 2)
            for (uint32_t j = t; j < n; j += kT) w_out[D.w + n + j] = -P.w[j];   // feature_coefficient(f, 1) = -feature_coefficient(f, 0)
        if (t == 0) {
            const vpt_train_stats st{r.newton, r.sweeps, r.gnorm0, r.gnorm, norm1 + loss};
            stats[D.stats + cls] = st;
            if (D.k == 2) stats[D.stats + 1] = st;
        }
        __syncthreads();
    }
}

}  // namespace

bool train_tag_l1lr_fits(uint64_t rows, uint64_t features) { return 3 * rows + (features + 1) <= kTagL1LdsDoubles; }
uint64_t train_tag_l1lr_scratch(uint64_t rows, uint64_t features) { return 4 * (features + 1) + rows; }
hipError_t train_tag_l1lr_solve(const TagSolveDesc* descs, const TagL1Desc* l1descs, uint32_t n_prob, const uint32_t* rp, const uint32_t* cols,
                                const uint32_t* cp, const uint32_t* crow, const uint32_t* y, const uint32_t* gcols, const TagL1Group* groups, double eps,
                                double cost, double* scratch, double* w, vpt_train_stats* stats, hipStream_t st) {
    if (n_prob == 0) return hipSuccess;
    hipLaunchKernelGGL(tag_l1lr_solve_kernel, dim3(n_prob), dim3(kT), 0, st, descs, l1descs, rp, cols, cp, crow, y, gcols, groups, eps, cost, scratch, w,
                       stats);
    return hipGetLastError();
}

}  // namespace vpt
