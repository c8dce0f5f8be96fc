// Boundary-model training with solver 5 (L1-regularised L2-loss SVC): a group of columns of liblinear's coordinate descent in one launch.
//
// The columns of a group share no row (capi_train.cpp, l1r_groups: one template (kind, n-gram length, rel_position) of the char and
// type features, or a single dictionary column, or the bias), so updating them together is coordinate descent over them in any order:
// no column reads a b[i] that another column of the launch writes, and there is no atomic on a double anywhere.  The step itself is
// l1r.h's; this file is its device backend: the sums over a column and the write of b.
//
// Who takes a column, the summation rule of its sums and the dealing of a launch's columns are l1r_team.h's.  A wave keeps its tile
// sums in LDS, a workgroup in global scratch (tile0 / tile1).
#include "kernels.hpp"

#include "device_common.h"
#include "l1r.h"
#include "l1r_team.h"

namespace vpt {
namespace {

// l1r.h's backend for a team of kT threads over one column
template <uint32_t kT>
struct Team {
    const L1rParams& P;
    uint64_t a;         // the column's nonzeros: a .. a + n of the CSC (the bias: rows 0 .. n)
    bool bias;
    L1rTeam<kT, uint64_t> tm;

    __device__ __forceinline__ uint64_t row(uint64_t k) const { return bias ? k : P.crow[a + k]; }
    __device__ __forceinline__ double v(uint64_t k, uint64_t row) const { return bias ? P.y[row] : double(P.cval[a + k]) * P.y[row]; }
    // f(b, v) over the column's nonzeros
    template <typename F>
    __device__ __forceinline__ L1rPair sums(F f) const {
        return tm.sums([this, f](uint64_t k) {
            const uint64_t r = row(k);
            const double x = v(k, r);
            return f(P.b[r], x);
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
        tm.each([this, d](uint64_t k) {
            const uint64_t r = row(k);
            P.b[r] = P.b[r] - d * v(k, r);
        });
    }
};

// kInit: xj_sq[j] = C sum x^2, by the same sums; else the column's step
template <uint32_t kT, bool kInit>
__device__ void column(const L1rParams& P, uint32_t j, uint32_t t, L1rPair* s0, L1rPair* s1) {
    const bool bias = j == P.nd;
    const uint64_t a = bias ? 0 : P.cptr[j], n = bias ? P.nr : P.cptr[j + 1] - a;
    const Team<kT> be{P, a, bias, {n, t, s0, s1}};
    if (kInit) {
        const double c = P.c;
        const L1rPair s = be.sums([c](double, double v) { return L1rPair{c * v * v, 0.0}; });
        if (t == 0) P.xj_sq[j] = s.a;
        return;
    }
    // every thread of the team reads w[j] before the first rendezvous of the sums; thread 0 writes it after the last
    const double w = P.w[j];
    const L1rStep s = l1r_column(be, w, P.xj_sq[j]);
    if (t != 0) return;
    P.viol[j] = s.violation;
    if (s.d != 0) P.w[j] = w + s.d;
    if (s.halvings) atomicAdd(P.halvings, s.halvings);
}

template <bool kInit>
__global__ __launch_bounds__(kTrainThreads) void l1r_group_kernel(L1rParams P, const uint32_t* cols, uint32_t n_lane, uint32_t n_wave, uint32_t n_block) {
    __shared__ L1rPair lds[kL1rWaves][kL1rWaveTiles + 1];
    l1r_deal_launch(cols, n_lane, n_wave, n_block, lds, P.nd, P.nnz, P.cptr, P.tile0, P.tile1,
                    [&P](auto kT, uint32_t j, uint32_t t, L1rPair* s0, L1rPair* s1) { column<kT, kInit>(P, j, t, s0, s1); });
}

}  // namespace

uint64_t train_l1r_scratch(uint64_t nnz, uint64_t nr, uint64_t nd, int level) {
    return ((nnz + nr) >> (level ? 12 : 6)) + nd + 2;
}
hipError_t train_l1r_group(const L1rParams& P, bool init, const uint32_t* cols, uint32_t n_lane, uint32_t n_wave, uint32_t n_block, hipStream_t st) {
    const uint32_t blocks = l1r_launch_blocks(n_lane, n_wave, n_block);
    if (blocks == 0) return hipSuccess;
    if (init) hipLaunchKernelGGL(l1r_group_kernel<true>, dim3(blocks), dim3(kTrainThreads), 0, st, P, cols, n_lane, n_wave, n_block);
    else hipLaunchKernelGGL(l1r_group_kernel<false>, dim3(blocks), dim3(kTrainThreads), 0, st, P, cols, n_lane, n_wave, n_block);
    return hipGetLastError();
}

}  // namespace vpt
