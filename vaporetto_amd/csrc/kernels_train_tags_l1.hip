// Tag-model training with solver 5 (L1-regularised L2-loss SVC): liblinear's coordinate descent for every (surface, slot) problem that
// fits, a workgroup per problem in one launch, one class after another over the same 0/1 matrix (one solve for two classes).
//
// The step is l1r.h's; this file is its in-kernel backend, as kernels_train_l1.hip is its backend over global memory.  A problem's w
// (features + 1, the bias last) and b (rows) live in LDS; the matrix's indices (CSR and CSC) stay in global memory.  A nonzero is 1
// (tag_rows_kernel: a row's columns are distinct), so v = y_i and xj_sq = C * the column's length.
//
// A sweep: the problem's groups (capi_train.cpp, l1r_groups over the problem's keys: a template's columns share no row, the bias alone
// and last) in a new Fisher-Yates order (thread 0 draws it, LDS hands it on), and for each group its columns dealt by length
// (l1r_team.h, tag_l1_deal); then the workgroup meets.  No column of a group reads a b[i] that another one writes, and there is no
// atomic on a double anywhere.
//
// The column team and its summation rule, the LDS behind w and b and the sums over a vector are l1r_team.h's: a column's sums have the
// bits the group launches give them, and the sweep's violation sum has the shape of the host driver's, so both paths stop at the same
// sweep.
#include "kernels.hpp"

#include <cmath>

#include "device_common.h"
#include "l1r.h"
#include "l1r_team.h"
#include "tron.h"

namespace vpt {
namespace {

constexpr uint32_t kT = kTrainThreads;

// solver 5's sums over a vector: their terms are not rounded first (l1r_team.h)
template <typename F>
__device__ double vec_sum(uint32_t n, F f, double* red) { return tag_l1_vec_sum<false>(n, f, red); }

struct Prob {
    const uint32_t *rp, *cols, *cp, *crow, *y;
    uint32_t nf, l, cls;
    double c;
    double *w, *b;
    __device__ __forceinline__ double target(uint32_t r) const { return y[r] == cls ? 1.0 : -1.0; }
};

// l1r.h's backend for a team of kN threads over one column: nonzeros a .. a + n of the CSC, or rows 0 .. n for the bias
template <uint32_t kN>
struct Team {
    const Prob& P;
    uint32_t a;
    bool bias;
    L1rTeam<kN, uint32_t> tm;

    __device__ __forceinline__ uint32_t row(uint32_t k) const { return bias ? k : P.crow[a + k]; }
    // f(b, v) over the column's nonzeros
    template <typename F>
    __device__ __forceinline__ L1rPair sums(F f) const {
        return tm.sums([this, f](uint32_t k) {
            const uint32_t r = row(k);
            return f(P.b[r], P.target(r));
        });
    }
    __device__ L1rPair grad_sums() const {
        const double c = P.c;
        return sums([c](double b, double v) { return l1r_grad_term(b, v, c); });
    }
    __device__ L1rPair loss_sums(double d) const {
        const double c = P.c;
        return sums([c, d](double b, double v) { return l1r_loss_term(b, v, c, d); });
    }
    __device__ void commit(double d) const {
        tm.each([this, d](uint32_t k) {
            const uint32_t r = row(k);
            P.b[r] = P.b[r] - d * P.target(r);
        });
    }
};

// column j's step by a team: every thread of the team reads w[j] before the first rendezvous of the sums, thread 0 writes it after the last
template <uint32_t kN>
__device__ void column(const Prob& P, uint32_t j, uint32_t t, L1rPair* s0, L1rPair* s1, double* viol, uint32_t* halvings) {
    const bool bias = j == P.nf;
    const uint32_t a = bias ? 0 : P.cp[j], n = bias ? P.l : P.cp[j + 1] - a;
    const Team<kN> be{P, a, bias, {n, t, s0, s1}};
    const double w = P.w[j];
    const L1rStep s = l1r_column(be, w, P.c * double(n));
    if (t != 0) return;
    viol[j] = s.violation;
    if (s.d != 0) P.w[j] = w + s.d;
    if (s.halvings) atomicAdd(halvings, s.halvings);
}

__global__ __launch_bounds__(kT) void tag_l1_solve_kernel(const TagSolveDesc* descs, const TagL1Desc* l1descs, const uint32_t* rp, const uint32_t* cols,
                                                          const uint32_t* cp, const uint32_t* crow, const uint32_t* y, const uint32_t* gcols,
                                                          const TagL1Group* groups, double eps, double c, double* viol_all, double* w_out,
                                                          vpt_train_stats* stats) {
    __shared__ double lds[kTagL1Doubles];
    const TagSolveDesc D = descs[blockIdx.x];
    const TagL1Desc E = l1descs[blockIdx.x];
    const uint32_t n = D.nf + 1, l = D.l, t = threadIdx.x;
    if (uint64_t(n) + l > kTagL1LdsDoubles || E.n_groups > kTagL1MaxGroups) return;   // the host sends such a problem down the other path
    Prob P;
    P.rp = rp + D.rp; P.cols = cols + D.cols; P.cp = cp + D.cp; P.crow = crow + D.cols; P.y = y + D.y;
    P.nf = D.nf; P.l = l; P.c = c; P.w = lds; P.b = lds + n;
    const TagL1Lds L = tag_l1_lds(lds);
    double* const red = L.red;
    uint32_t* const order = L.order;
    uint32_t* const halvings = order + kTagL1MaxGroups;
    const uint32_t* const gc = gcols + E.gcols;
    const TagL1Group* const gr = groups + E.groups;
    double* const viol = viol_all + E.viol;
    const uint32_t n_solve = D.k == 2 ? 1 : D.k;
    for (uint32_t cls = 0; cls < n_solve; ++cls) {
        P.cls = cls;
        for (uint32_t i = t; i < n; i += kT) P.w[i] = 0;
        for (uint32_t i = t; i < l; i += kT) P.b[i] = 1;
        if (t < E.n_groups) order[t] = t;
        if (t == 0) *halvings = 0;
        const double pos = vec_sum(l, [&](uint32_t i) { return P.y[i] == cls ? 1.0 : 0.0; }, red);   // meets: w, b and the order are written
        const double tol = tron_tolerance(eps, pos, double(l));
        uint64_t rng = kL1rSeed;   // thread 0's is the one drawn from
        double v0 = 0, v = 0;
        uint32_t sweeps = 0;
        while (sweeps < uint32_t(kL1rMaxSweeps)) {
            if (t == 0) l1r_shuffle(order, E.n_groups, &rng);
            __syncthreads();
            for (uint32_t q = 0; q < E.n_groups; ++q) {
                const TagL1Group G = gr[order[q]];
                tag_l1_deal(G, gc + G.at, L, [&](auto kN, uint32_t j, uint32_t tt, L1rPair* s0, L1rPair* s1) { column<kN>(P, j, tt, s0, s1, viol, halvings); });
                __syncthreads();
            }
            v = vec_sum(n, [&](uint32_t i) { return viol[i]; }, red);
            if (sweeps++ == 0) v0 = v;
            if (v <= tol * v0) break;
        }
        // the loss at the weights themselves, not at the b the sweeps carried along
        const double loss = vec_sum(l, [&](uint32_t r) {
            double z = 0;
            for (uint32_t k = P.rp[r]; k < P.rp[r + 1]; ++k) z += P.w[P.cols[k]];
            return tron_loss(P.target(r) * (z + P.w[P.nf]), c, 2);
        }, red);
        const double norm1 = vec_sum(n, [&](uint32_t i) { return fabs(P.w[i]); }, red);
        for (uint32_t i = t; i < n; i += kT) {
            w_out[D.w + uint64_t(cls) * n + i] = P.w[i];
            if (D.k == 2) w_out[D.w + n + i] = -P.w[i];   // feature_coefficient(f, 1) = -feature_coefficient(f, 0)
        }
        if (t == 0) {
            const vpt_train_stats st{sweeps, *halvings, v0, v, norm1 + loss};
            stats[D.stats + cls] = st;
            if (D.k == 2) stats[D.stats + 1] = st;
        }
        __syncthreads();
    }
}

}  // namespace

bool train_tag_l1_fits(uint64_t rows, uint64_t features) { return (features + 1) + rows <= kTagL1LdsDoubles; }
hipError_t train_tag_l1_solve(const TagSolveDesc* descs, const TagL1Desc* l1descs, uint32_t n_prob, const uint32_t* rp, const uint32_t* cols,
                              const uint32_t* cp, const uint32_t* crow, const uint32_t* y, const uint32_t* gcols, const TagL1Group* groups, double eps,
                              double cost, double* viol, double* w, vpt_train_stats* stats, hipStream_t st) {
    if (n_prob == 0) return hipSuccess;
    hipLaunchKernelGGL(tag_l1_solve_kernel, dim3(n_prob), dim3(kT), 0, st, descs, l1descs, rp, cols, cp, crow, y, gcols, groups, eps, cost, viol, w, stats);
    return hipGetLastError();
}

}  // namespace vpt
