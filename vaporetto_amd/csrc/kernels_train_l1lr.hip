// Boundary-model training with solver 6 (L1-regularised logistic regression, liblinear's newGLMNET): the device backend of l1r_lr.h.
//
// Three kinds of launch.  l1lr_grad_kernel, one launch over all columns, read-only over the rows' state: Hdiag, Grad and the violation
// at w (and, once, xjneg_sum by the same sums).  l1lr_cd_group_kernel, one launch per group per inner sweep: the columns of a group
// share no row (capi_train.cpp, l1r_groups), so no column reads an xTd[i] that another column of the launch writes, and there is no
// atomic on a double anywhere; a column makes one pass for sum x D xTd, takes l1r_lr.h's step, and a second pass to write xTd if it
// moved.  The l1lr_row_* and l1lr_feat_* kernels, a thread per row or per feature: the line search's terms, the accept step, the
// halvings; their term arrays are summed by the fixed-shape reduction of kernels_train.hip (train_dot).
//
// D and xTd are gathered separately by the sum pass (16 bytes per nonzero) rather than kept as a product D xTd per row: the product
// would halve the sum pass's gather, but every column that moves would read D and write a second row vector in its write pass, and
// the accept and halving steps would have to keep it current.  Which of the two moves fewer bytes depends on the share of columns that
// move in a sweep; nobody has measured it.
//
// Who takes a column, the summation rule of its sums and the dealing of a launch's columns are l1r_team.h's.
#include "kernels.hpp"

#include "device_common.h"
#include "l1r_lr.h"
#include "l1r_team.h"

namespace vpt {
namespace {

// a team of kT threads over one column: its sums and its write of xTd
template <uint32_t kT>
struct Team {
    const L1lrParams& P;
    uint64_t a;         // the column's nonzeros: a .. a + n of the CSC (the bias: rows 0 .. n, value 1)
    bool bias;
    L1rTeam<kT, uint64_t> tm;

    __device__ __forceinline__ uint64_t row(uint64_t k) const { return bias ? k : P.crow[a + k]; }
    __device__ __forceinline__ double x(uint64_t k) const { return bias ? 1.0 : double(P.cval[a + k]); }
    // f(row, x) over the column's nonzeros
    template <typename F>
    __device__ __forceinline__ L1rPair sums(F f) const {
        return tm.sums([this, f](uint64_t k) { return f(row(k), x(k)); });
    }
    // xTd_i += z x_ij over the column: its rows are distinct, and no other column of the launch has them
    __device__ void add_xTd(double z) const {
        tm.each([this, z](uint64_t k) {
            const uint64_t r = row(k);
            P.xTd[r] = P.xTd[r] + z * x(k);
        });
    }
};

enum : int { kNeg = 0, kGrad = 1, kCd = 2 };

// kNeg: xjneg_sum[j]; kGrad: Hdiag[j], Grad[j] and the violation at w[j]; kCd: the column's step of the inner loop
template <uint32_t kT, int kMode>
__device__ void column(const L1lrParams& P, uint32_t j, uint32_t t, L1rPair* s0, L1rPair* s1) {
    const bool bias = j == P.nd;
    const uint64_t a = bias ? 0 : P.cptr[j], n = bias ? P.nr : P.cptr[j + 1] - a;
    const Team<kT> be{P, a, bias, {n, t, s0, s1}};
    if constexpr (kMode == kNeg) {
        const double c = P.c;
        const double* y = P.y;
        const L1rPair s = be.sums([c, y](uint64_t row, double x) { return l1lr_neg_term(x, y[row], c); });
        if (t == 0) P.xjneg[j] = s.a;
    } else if constexpr (kMode == kGrad) {
        const double *D = P.D, *tau = P.tau;
        const L1rPair s = be.sums([D, tau](uint64_t row, double x) { return l1lr_grad_term(x, D[row], tau[row]); });
        if (t != 0) return;
        const double G = -s.b + P.xjneg[j];
        P.hdiag[j] = kL1lrNu + s.a;
        P.grad[j] = G;
        P.viol[j] = l1lr_violation(P.w[j], G);
    } else {
        // every thread of the team reads wpd[j] before the first rendezvous of the sums; thread 0 writes it after the last
        const double w = P.w[j], wpd = P.wpd[j];
        const double *D = P.D, *xTd = P.xTd;
        const L1rPair s = be.sums([D, xTd](uint64_t row, double x) { return l1lr_qp_term(x, D[row], xTd[row]); });
        const double G = P.grad[j] + (wpd - w) * kL1lrNu + s.a;
        const L1lrStep step = l1lr_cd_step(wpd, G, P.hdiag[j]);
        if (step.z != 0) be.add_xTd(step.z);
        if (t != 0) return;
        P.viol[j] = step.violation;
        if (step.z != 0) P.wpd[j] = wpd + step.z;
    }
}

template <int kMode>
__device__ __forceinline__ void columns(const L1lrParams& P, const uint32_t* cols, uint32_t n_lane, uint32_t n_wave, uint32_t n_block,
                                        L1rPair (*lds)[kL1rWaveTiles + 1]) {
    l1r_deal_launch(cols, n_lane, n_wave, n_block, lds, P.nd, P.nnz, P.cptr, P.tile0, P.tile1,
                    [&P](auto kT, uint32_t j, uint32_t t, L1rPair* s0, L1rPair* s1) { column<kT, kMode>(P, j, t, s0, s1); });
}
template <bool kNegSum>
__global__ __launch_bounds__(kTrainThreads) void l1lr_grad_kernel(L1lrParams P, const uint32_t* cols, uint32_t n_lane, uint32_t n_wave, uint32_t n_block) {
    __shared__ L1rPair lds[kL1rWaves][kL1rWaveTiles + 1];
    columns<kNegSum ? kNeg : kGrad>(P, cols, n_lane, n_wave, n_block, lds);
}
__global__ __launch_bounds__(kTrainThreads) void l1lr_cd_group_kernel(L1lrParams P, const uint32_t* cols, uint32_t n_lane, uint32_t n_wave, uint32_t n_block) {
    __shared__ L1rPair lds[kL1rWaves][kL1rWaveTiles + 1];
    columns<kCd>(P, cols, n_lane, n_wave, n_block, lds);
}

// ---- a thread per row
// e, tau, D after the step xTd was accepted (setup: e = 1, xTd = 0)
__global__ __launch_bounds__(kTrainThreads) void l1lr_row_accept_kernel(uint64_t n, double c, const double* xTd, double* e, double* tau, double* D) {
    const uint64_t i = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (i >= n) return;
    const L1lrRow r = l1lr_accept_row(e[i], xTd[i], c);
    e[i] = r.e;
    tau[i] = r.tau;
    D[i] = r.D;
}
__global__ __launch_bounds__(kTrainThreads) void l1lr_row_term_kernel(uint64_t n, double c, const double* e, const double* xTd, double* out) {
    const uint64_t i = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (i < n) out[i] = l1lr_ls_term(e[i], xTd[i], c);
}
// negsum_xTd's terms
__global__ __launch_bounds__(kTrainThreads) void l1lr_row_neg_kernel(uint64_t n, double c, const double* y, const double* xTd, double* out) {
    const uint64_t i = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (i < n) out[i] = y[i] < 0 ? c * xTd[i] : 0.0;
}
__global__ __launch_bounds__(kTrainThreads) void l1lr_row_fill_kernel(uint64_t n, double e0, double* e, double* xTd) {
    const uint64_t i = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (i >= n) return;
    if (e) e[i] = e0;
    xTd[i] = 0.0;
}
// recompute(): e = exp(w.x) from z = Xw
__global__ __launch_bounds__(kTrainThreads) void l1lr_row_exp_kernel(uint64_t n, double* z) {
    const uint64_t i = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (i < n) z[i] = exp(z[i]);
}
// ---- a thread per feature (the bias among them)
// delta's terms and |wpd|_1's
__global__ __launch_bounds__(kTrainThreads) void l1lr_feat_terms_kernel(uint64_t n, const double* w, const double* wpd, const double* grad, double* delta, double* norm1) {
    const uint64_t j = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (j >= n) return;
    if (delta) delta[j] = grad[j] * (wpd[j] - w[j]);
    norm1[j] = fabs(wpd[j]);
}
// halve(): wpd = (w + wpd) / 2 and xTd /= 2, one launch over max(rows, features)
__global__ __launch_bounds__(kTrainThreads) void l1lr_halve_kernel(uint64_t n, uint64_t nr, const double* w, double* wpd, double* xTd) {
    const uint64_t i = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (i < n) wpd[i] = (w[i] + wpd[i]) * 0.5;
    if (i < nr) xTd[i] = xTd[i] * 0.5;
}

hipError_t launch_cols(int mode, const L1lrParams& P, const uint32_t* cols, uint32_t n_lane, uint32_t n_wave, uint32_t n_block, hipStream_t st) {
    const uint32_t blocks = l1r_launch_blocks(n_lane, n_wave, n_block);
    if (blocks == 0) return hipSuccess;
    if (mode == kNeg) hipLaunchKernelGGL(l1lr_grad_kernel<true>, dim3(blocks), dim3(kTrainThreads), 0, st, P, cols, n_lane, n_wave, n_block);
    else if (mode == kGrad) hipLaunchKernelGGL(l1lr_grad_kernel<false>, dim3(blocks), dim3(kTrainThreads), 0, st, P, cols, n_lane, n_wave, n_block);
    else hipLaunchKernelGGL(l1lr_cd_group_kernel, dim3(blocks), dim3(kTrainThreads), 0, st, P, cols, n_lane, n_wave, n_block);
    return hipGetLastError();
}

}  // namespace

hipError_t train_l1lr_grad(const L1lrParams& P, bool neg_sum, const uint32_t* cols, uint32_t n_lane, uint32_t n_wave, uint32_t n_block, hipStream_t st) {
    return launch_cols(neg_sum ? kNeg : kGrad, P, cols, n_lane, n_wave, n_block, st);
}
hipError_t train_l1lr_cd_group(const L1lrParams& P, const uint32_t* cols, uint32_t n_lane, uint32_t n_wave, uint32_t n_block, hipStream_t st) {
    return launch_cols(kCd, P, cols, n_lane, n_wave, n_block, st);
}
hipError_t train_l1lr_start(const L1lrParams& P, bool setup, hipStream_t st) {
    return launch1(l1lr_row_fill_kernel, P.nr, st, P.nr, 1.0, setup ? P.e : nullptr, P.xTd);
}
hipError_t train_l1lr_accept(const L1lrParams& P, hipStream_t st) { return launch1(l1lr_row_accept_kernel, P.nr, st, P.nr, P.c, P.xTd, P.e, P.tau, P.D); }
hipError_t train_l1lr_ls_terms(const L1lrParams& P, double* out, hipStream_t st) { return launch1(l1lr_row_term_kernel, P.nr, st, P.nr, P.c, P.e, P.xTd, out); }
hipError_t train_l1lr_neg_terms(const L1lrParams& P, double* out, hipStream_t st) { return launch1(l1lr_row_neg_kernel, P.nr, st, P.nr, P.c, P.y, P.xTd, out); }
hipError_t train_l1lr_exp(uint64_t n, double* z, hipStream_t st) { return launch1(l1lr_row_exp_kernel, n, st, n, z); }
hipError_t train_l1lr_feat_terms(const L1lrParams& P, double* delta, double* norm1, hipStream_t st) {
    return launch1(l1lr_feat_terms_kernel, P.nd + 1, st, P.nd + 1, P.w, P.wpd, P.grad, delta, norm1);
}
hipError_t train_l1lr_halve(const L1lrParams& P, hipStream_t st) {
    const uint64_t n = P.nd + 1, m = n > P.nr ? n : P.nr;
    return launch1(l1lr_halve_kernel, m, st, n, P.nr, P.w, P.wpd, P.xTd);
}

}  // namespace vpt
