// Boundary-model training with solver 5 (L1-regularised L2-loss SVC): a group of columns of liblinear's coordinate descent in one launch.
//
// The columns of a group share no row (capi_train.cpp, l1r_groups: one template (kind, n-gram length, rel_position) of the char and
// type features, or a single dictionary column, or the bias), so updating them together is coordinate descent over them in any order:
// no column reads a b[i] that another column of the launch writes, and there is no atomic on a double anywhere.  The step itself is
// l1r.h's; this file is its device backend: the sums over a column and the write of b.
//
// Who takes a column, by its nonzeros: a lane one of at most kL1rLaneMax (a wave takes 64 such columns), a wave one of at most
// kL1rWaveMax, a workgroup a longer one (the bias column -- every row, value 1 -- among them).  The two thresholds are the sizes at
// which the next unit has something to do for every member under the summation rule below; they are not measured optima.
//
// Summation rule (the one of the segments of Xᵀv in kernels_train.hip): a column's sum is taken over fixed tiles of 64 nonzeros, each
// summed in index order by one thread; the tile sums are summed 64 at a time in index order, level by level, until one is left.  The
// shape of that tree depends on the column's length alone, so G_loss, H and the losses have the same bits whichever unit took the
// column and whatever the launch geometry.  A wave keeps its tile sums in LDS, a workgroup in global scratch (tile0 / tile1: a
// column's place in them follows from where its nonzeros start, so the columns of a launch do not meet there either).
#include "kernels.hpp"

#include "device_common.h"
#include "l1r.h"

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

// l1r.h's backend for a team of kT threads (1: a lane, 64: a wave, 256: the workgroup) over one column
template <uint32_t kT>
struct Team {
    const L1rParams& P;
    uint64_t a, n;      // the column's nonzeros: a .. a + n of the CSC (the bias: rows 0 .. n)
    bool bias;
    uint32_t t;         // this thread in the team
    L1rPair *s0, *s1;   // the levels' sums, written in turn

    __device__ __forceinline__ void sync() const {
        if constexpr (kT == 64) wave_rendezvous();
        else if constexpr (kT > 64) __syncthreads();
    }
    // the tile that starts at nonzero k0, in index order
    template <typename F>
    __device__ __forceinline__ L1rPair tile(uint64_t k0, F f) const {
        const uint64_t k1 = k0 + kTileNz < n ? k0 + kTileNz : n;
        L1rPair acc{0.0, 0.0};
        for (uint64_t k = k0; k < k1; ++k) {
            const uint64_t row = bias ? k : P.crow[a + k];
            const double v = bias ? P.y[row] : double(P.cval[a + k]) * P.y[row];
            acc = l1r_add(acc, f(P.b[row], v));
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
    __device__ L1rPair grad_sums() const {
        const double c = P.c;
        return sums([c](double b, double v) { return l1r_grad_term(b, v, c); });
    }
    __device__ L1rPair loss_sums(double d) const {
        const double c = P.c;
        return sums([c, d](double b, double v) { return l1r_loss_term(b, v, c, d); });
    }
    __device__ void commit(double d) const {
        for (uint64_t k = t; k < n; k += kT) {
            const uint64_t row = bias ? k : P.crow[a + k];
            const double v = bias ? P.y[row] : double(P.cval[a + k]) * P.y[row];
            P.b[row] = P.b[row] - d * v;
        }
    }
};

// kInit: xj_sq[j] = C sum x^2, by the same sums; else the column's step
template <uint32_t kT, bool kInit>
__device__ void column(const L1rParams& P, uint32_t j, uint32_t t, L1rPair* s0, L1rPair* s1) {
    const bool bias = j == P.nd;
    const uint64_t a = bias ? 0 : P.cptr[j], n = bias ? P.nr : P.cptr[j + 1] - a;
    const Team<kT> be{P, a, n, bias, t, s0, s1};
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

// cols: the group's columns, those a lane takes first, then a wave's, then a workgroup's
template <bool kInit>
__global__ __launch_bounds__(kTrainThreads) void l1r_group_kernel(L1rParams P, const uint32_t* cols, uint32_t n_lane, uint32_t n_wave, uint32_t n_block) {
    constexpr uint32_t kWaves = kTrainThreads / 64;
    __shared__ L1rPair lds[kWaves][kWaveTiles + 1];
    const uint32_t lane_blocks = (n_lane + kTrainThreads - 1) / kTrainThreads, wave_blocks = (n_wave + kWaves - 1) / kWaves;
    uint32_t bx = blockIdx.x;
    if (bx < lane_blocks) {
        const uint32_t i = bx * kTrainThreads + threadIdx.x;
        if (i < n_lane) column<1, kInit>(P, cols[i], 0, nullptr, nullptr);
        return;
    }
    bx -= lane_blocks;
    if (bx < wave_blocks) {
        const uint32_t wave = threadIdx.x >> 6, i = bx * kWaves + wave;
        if (i < n_wave) column<64, kInit>(P, cols[n_lane + i], threadIdx.x & 63u, lds[wave], lds[wave] + kWaveTiles);
        return;
    }
    bx -= wave_blocks;
    if (bx >= n_block) return;
    const uint32_t j = cols[n_lane + n_wave + bx];
    const uint64_t start = j == P.nd ? P.nnz : P.cptr[j];   // the bias behind every column
    column<kTrainThreads, kInit>(P, j, threadIdx.x, P.tile0 + (start >> 6) + j, P.tile1 + (start >> 12) + j);
}

}  // namespace

uint64_t train_l1r_scratch(uint64_t nnz, uint64_t nr, uint64_t nd, int level) {
    return ((nnz + nr) >> (level ? 12 : 6)) + nd + 2;
}
hipError_t train_l1r_group(const L1rParams& P, bool init, const uint32_t* cols, uint32_t n_lane, uint32_t n_wave, uint32_t n_block, hipStream_t st) {
    const uint32_t blocks = (n_lane + kTrainThreads - 1) / kTrainThreads + (n_wave + kTrainThreads / 64 - 1) / (kTrainThreads / 64) + n_block;
    if (blocks == 0) return hipSuccess;
    if (init) hipLaunchKernelGGL(l1r_group_kernel<true>, dim3(blocks), dim3(kTrainThreads), 0, st, P, cols, n_lane, n_wave, n_block);
    else hipLaunchKernelGGL(l1r_group_kernel<false>, dim3(blocks), dim3(kTrainThreads), 0, st, P, cols, n_lane, n_wave, n_block);
    return hipGetLastError();
}

}  // namespace vpt
