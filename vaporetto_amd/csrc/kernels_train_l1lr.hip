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
// Who takes a column and the summation rule are those of kernels_train_l1.hip: a lane a column of at most kL1rLaneMax nonzeros, a wave
// one of at most kL1rWaveMax, the workgroup a longer one and the bias; a column's sum is taken over tiles of 64 nonzeros, each summed
// in index order by one thread, the tile sums 64 at a time in index order, level by level.  The shape of that tree depends on the
// column's length alone, so every column sum has the same bits on every path and for every launch geometry.
#include "kernels.hpp"

#include "device_common.h"
#include "l1r_lr.h"

namespace vpt {
namespace {

constexpr uint32_t kTileNz = 64;                           // nonzeros (partial sums) a thread adds up in order
constexpr uint32_t kWaveTiles = kL1rWaveMax / kTileNz;     // tile sums a wave keeps in LDS
static_assert(kL1rLaneMax == kTileNz && kWaveTiles >= 1 && kWaveTiles <= 64, "a lane takes one tile, a wave's second level is one sum");

// the lanes of a wave meet: what they wrote to LDS before is what they read after
__device__ __forceinline__ void wave_rendezvous() {
#ifndef VPT_HIPEMU
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#endif
    __builtin_amdgcn_wave_barrier();
}

// a team of kT threads (1: a lane, 64: a wave, 256: the workgroup) over one column: its sums and its write of xTd
template <uint32_t kT>
struct Team {
    const L1lrParams& P;
    uint64_t a, n;      // the column's nonzeros: a .. a + n of the CSC (the bias: rows 0 .. n, value 1)
    bool bias;
    uint32_t t;         // this thread in the team
    L1rPair *s0, *s1;   // the levels' sums, written in turn

    __device__ __forceinline__ void sync() const {
        if constexpr (kT == 64) wave_rendezvous();
        else if constexpr (kT > 64) __syncthreads();
    }
    // the tile that starts at nonzero k0, in index order; f(row, x)
    template <typename F>
    __device__ __forceinline__ L1rPair tile(uint64_t k0, F f) const {
        const uint64_t k1 = k0 + kTileNz < n ? k0 + kTileNz : n;
        L1rPair acc{0.0, 0.0};
        for (uint64_t k = k0; k < k1; ++k) {
            const uint64_t row = bias ? k : P.crow[a + k];
            acc = l1r_add(acc, f(row, bias ? 1.0 : double(P.cval[a + k])));
        }
        return acc;
    }
    template <typename F>
    __device__ L1rPair sums(F f) const {
        if constexpr (kT == 1) return tile(0, f);
        uint64_t m = (n + kTileNz - 1) / kTileNz;
        for (uint64_t i = t; i < m; i += kT) s0[i] = tile(i * kTileNz, f);
        sync();
        L1rPair *src = s0, *dst = s1;
        while (m > 1) {
            const uint64_t g = (m + kTileNz - 1) / kTileNz;
            for (uint64_t i = t; i < g; i += kT) {
                const uint64_t q1 = (i + 1) * kTileNz < m ? (i + 1) * kTileNz : m;
                L1rPair acc{0.0, 0.0};
                for (uint64_t q = i * kTileNz; q < q1; ++q) acc = l1r_add(acc, src[q]);
                dst[i] = acc;
            }
            sync();
            L1rPair* tmp = src; src = dst; dst = tmp;
            m = g;
        }
        const L1rPair r = src[0];
        sync();   // the next pass writes the buffers again
        return r;
    }
    // xTd_i += z x_ij over the column: its rows are distinct, and no other column of the launch has them
    __device__ void add_xTd(double z) const {
        for (uint64_t k = t; k < n; k += kT) {
            const uint64_t row = bias ? k : P.crow[a + k];
            P.xTd[row] = P.xTd[row] + z * (bias ? 1.0 : double(P.cval[a + k]));
        }
    }
};

enum : int { kNeg = 0, kGrad = 1, kCd = 2 };

// kNeg: xjneg_sum[j]; kGrad: Hdiag[j], Grad[j] and the violation at w[j]; kCd: the column's step of the inner loop
template <uint32_t kT, int kMode>
__device__ void column(const L1lrParams& P, uint32_t j, uint32_t t, L1rPair* s0, L1rPair* s1) {
    const bool bias = j == P.nd;
    const uint64_t a = bias ? 0 : P.cptr[j], n = bias ? P.nr : P.cptr[j + 1] - a;
    const Team<kT> be{P, a, n, bias, t, s0, s1};
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

// cols: the launch's columns, those a lane takes first, then a wave's, then a workgroup's
template <int kMode>
__device__ __forceinline__ void columns(const L1lrParams& P, const uint32_t* cols, uint32_t n_lane, uint32_t n_wave, uint32_t n_block,
                                        L1rPair (*lds)[kWaveTiles + 1]) {
    constexpr uint32_t kWaves = kTrainThreads / 64;
    const uint32_t lane_blocks = (n_lane + kTrainThreads - 1) / kTrainThreads, wave_blocks = (n_wave + kWaves - 1) / kWaves;
    uint32_t bx = blockIdx.x;
    if (bx < lane_blocks) {
        const uint32_t i = bx * kTrainThreads + threadIdx.x;
        if (i < n_lane) column<1, kMode>(P, cols[i], 0, nullptr, nullptr);
        return;
    }
    bx -= lane_blocks;
    if (bx < wave_blocks) {
        const uint32_t wave = threadIdx.x >> 6, i = bx * kWaves + wave;
        if (i < n_wave) column<64, kMode>(P, cols[n_lane + i], threadIdx.x & 63u, lds[wave], lds[wave] + kWaveTiles);
        return;
    }
    bx -= wave_blocks;
    if (bx >= n_block) return;
    const uint32_t j = cols[n_lane + n_wave + bx];
    const uint64_t start = j == P.nd ? P.nnz : P.cptr[j];   // the bias behind every column
    column<kTrainThreads, kMode>(P, j, threadIdx.x, P.tile0 + (start >> 6) + j, P.tile1 + (start >> 12) + j);
}

template <bool kNegSum>
__global__ __launch_bounds__(kTrainThreads) void l1lr_grad_kernel(L1lrParams P, const uint32_t* cols, uint32_t n_lane, uint32_t n_wave, uint32_t n_block) {
    __shared__ L1rPair lds[kTrainThreads / 64][kWaveTiles + 1];
    columns<kNegSum ? kNeg : kGrad>(P, cols, n_lane, n_wave, n_block, lds);
}
__global__ __launch_bounds__(kTrainThreads) void l1lr_cd_group_kernel(L1lrParams P, const uint32_t* cols, uint32_t n_lane, uint32_t n_wave, uint32_t n_block) {
    __shared__ L1rPair lds[kTrainThreads / 64][kWaveTiles + 1];
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
    const uint32_t blocks = (n_lane + kTrainThreads - 1) / kTrainThreads + (n_wave + kTrainThreads / 64 - 1) / (kTrainThreads / 64) + n_block;
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
