// Tag-model training with solver 5 (L1-regularised L2-loss SVC): liblinear's coordinate descent for every (surface, slot) problem that
// fits, a workgroup per problem in one launch, one class after another over the same 0/1 matrix (one solve for two classes).
//
// The step is l1r.h's; this file is its in-kernel backend, as kernels_train_l1.hip is its backend over global memory.  A problem's w
// (features + 1, the bias last) and b (rows) live in LDS; the matrix's indices (CSR and CSC) stay in global memory.  A nonzero is 1
// (tag_rows_kernel: a row's columns are distinct), so v = y_i and xj_sq = C * the column's length.
//
// A sweep: the problem's groups (capi_train.cpp, l1r_groups over the problem's keys: a template's columns share no row, the bias alone
// and last) in a new Fisher-Yates order (thread 0 draws it, LDS hands it on), and for each group its columns dealt by length: a lane
// takes the columns of at most kL1rLaneMax nonzeros, a wave those of at most kL1rWaveMax, the workgroup the longer ones and the bias;
// then the workgroup meets.  No column of a group reads a b[i] that another one writes, and there is no atomic on a double anywhere.
//
// Summation rule: kernels_train_l1.hip's -- tiles of 64 nonzeros in index order, tile sums 64 at a time, level by level -- so a
// column's sums have the bits the group launches give them.  The sweep's violation sum has the shape of the host driver's (dot_kernel
// of kernels_train.hip: tiles of 4096, a thread its sixteen strided values in order, a halving tree over the 256), so both paths stop
// at the same sweep.
#include "kernels.hpp"

#include <cmath>

#include "device_common.h"
#include "l1r.h"
#include "tron.h"

namespace vpt {
namespace {

constexpr uint32_t kT = kTrainThreads;
constexpr uint32_t kWaves = kT / 64;
constexpr uint32_t kTileNz = 64;                            // the summation rule's tile
constexpr uint32_t kWaveTiles = kL1rWaveMax / kTileNz;      // tile sums of a wave's column
// the LDS behind w and b, in doubles: [0, kRedDoubles) the workgroup's level sums (a column has at most kTagL1LdsDoubles rows) or the
// tree of the sums over a vector; then the waves' tile sums; then the groups' order and the halvings
constexpr uint32_t kBlkTiles0 = (kTagL1LdsDoubles + kTileNz - 1) / kTileNz, kBlkTiles1 = (kBlkTiles0 + kTileNz - 1) / kTileNz;
constexpr uint32_t kRedDoubles = 264;
constexpr uint32_t kWaveDoubles = 2 * kWaves * (kWaveTiles + 1);
constexpr uint32_t kOrderDoubles = kTagL1MaxGroups / 2 + 8;
constexpr uint32_t kLdsDoubles = kTagL1LdsDoubles + kRedDoubles + kWaveDoubles + kOrderDoubles;
static_assert(kT == 256 && kL1rLaneMax == kTileNz && kWaveTiles <= 64, "a lane takes one tile, a wave's second level is one sum");
static_assert(2 * (kBlkTiles0 + kBlkTiles1) <= kRedDoubles && kT + 2 <= kRedDoubles && kBlkTiles1 <= kTileNz, "the level sums and the tree share a place");
static_assert(kTagL1LdsDoubles <= 2 * 16 * kT, "a vector is at most two tiles of the tree");
static_assert(kLdsDoubles * 8 <= 61568, "the static LDS array of tag_solve_kernel is the budget");

__device__ __forceinline__ void wave_rendezvous() {
#ifndef VPT_HIPEMU
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#endif
    __builtin_amdgcn_wave_barrier();
}

// the sum of f(0) .. f(n - 1) in the shape of dot_kernel and its second level; the same bits in every thread.  red: kT + 2 doubles
template <typename F>
__device__ double vec_sum(uint32_t n, F f, double* red) {
    const uint32_t t = threadIdx.x, m = (n + 16 * kT - 1) / (16 * kT);
    for (uint32_t tile = 0; tile < m; ++tile) {
        double s = 0;
        for (uint32_t k = 0; k < 16; ++k) {
            const uint32_t i = tile * 16 * kT + k * kT + t;
            if (i < n) s += f(i);
        }
        red[t] = s;
        __syncthreads();
        for (uint32_t h = kT / 2; h > 0; h >>= 1) {
            if (t < h) red[t] += red[t + h];
            __syncthreads();
        }
        if (t == 0) red[kT + tile] = red[0];
        __syncthreads();
    }
    // the partials are a tile of their own: the zeros beside them add nothing
    const double r = m > 1 ? red[kT] + red[kT + 1] : red[kT];
    __syncthreads();   // the next sum writes red again
    return r;
}

struct Prob {
    const uint32_t *rp, *cols, *cp, *crow, *y;
    uint32_t nf, l, cls;
    double c;
    double *w, *b;
    __device__ __forceinline__ double target(uint32_t r) const { return y[r] == cls ? 1.0 : -1.0; }
};

// l1r.h's backend for a team of kN threads (1: a lane, 64: a wave, 256: the workgroup) over one column: nonzeros a .. a + n of the
// CSC, or rows 0 .. n for the bias
template <uint32_t kN>
struct Team {
    const Prob& P;
    uint32_t a, n;
    bool bias;
    uint32_t t;
    L1rPair *s0, *s1;

    __device__ __forceinline__ void sync() const {
        if constexpr (kN == 64) wave_rendezvous();
        else if constexpr (kN > 64) __syncthreads();
    }
    template <typename F>
    __device__ __forceinline__ L1rPair tile(uint32_t k0, F f) const {
        const uint32_t k1 = k0 + kTileNz < n ? k0 + kTileNz : n;
        L1rPair acc{0.0, 0.0};
        for (uint32_t k = k0; k < k1; ++k) {
            const uint32_t row = bias ? k : P.crow[a + k];
            acc = l1r_add(acc, f(P.b[row], P.target(row)));
        }
        return acc;
    }
    template <typename F>
    __device__ L1rPair sums(F f) const {
        if constexpr (kN == 1) return tile(0, f);
        uint32_t m = (n + kTileNz - 1) / kTileNz;
        for (uint32_t i = t; i < m; i += kN) s0[i] = tile(i * kTileNz, f);
        sync();
        L1rPair *src = s0, *dst = s1;
        while (m > 1) {
            const uint32_t g = (m + kTileNz - 1) / kTileNz;
            for (uint32_t i = t; i < g; i += kN) {
                const uint32_t q1 = (i + 1) * kTileNz < m ? (i + 1) * kTileNz : m;
                L1rPair acc{0.0, 0.0};
                for (uint32_t q = i * kTileNz; q < q1; ++q) acc = l1r_add(acc, src[q]);
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
        for (uint32_t k = t; k < n; k += kN) {
            const uint32_t row = bias ? k : P.crow[a + k];
            P.b[row] = P.b[row] - d * P.target(row);
        }
    }
};

// column j's step by a team: every thread of the team reads w[j] before the first rendezvous of the sums, thread 0 writes it after the last
template <uint32_t kN>
__device__ void column(const Prob& P, uint32_t j, uint32_t t, L1rPair* s0, L1rPair* s1, double* viol, uint32_t* halvings) {
    const bool bias = j == P.nf;
    const uint32_t a = bias ? 0 : P.cp[j], n = bias ? P.l : P.cp[j + 1] - a;
    const Team<kN> be{P, a, n, bias, t, s0, s1};
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
    __shared__ double lds[kLdsDoubles];
    const TagSolveDesc D = descs[blockIdx.x];
    const TagL1Desc E = l1descs[blockIdx.x];
    const uint32_t n = D.nf + 1, l = D.l, t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    if (uint64_t(n) + l > kTagL1LdsDoubles || E.n_groups > kTagL1MaxGroups) return;   // the host sends such a problem down the other path
    Prob P;
    P.rp = rp + D.rp; P.cols = cols + D.cols; P.cp = cp + D.cp; P.crow = crow + D.cols; P.y = y + D.y;
    P.nf = D.nf; P.l = l; P.c = c; P.w = lds; P.b = lds + n;
    double* const red = lds + kTagL1LdsDoubles;
    L1rPair* const blk0 = reinterpret_cast<L1rPair*>(red);
    L1rPair* const blk1 = blk0 + kBlkTiles0;
    L1rPair* const wv0 = reinterpret_cast<L1rPair*>(red + kRedDoubles) + wave * (kWaveTiles + 1);
    uint32_t* const order = reinterpret_cast<uint32_t*>(red + kRedDoubles + kWaveDoubles);
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
                const uint32_t* const cj = gc + G.at;
                for (uint32_t i = t; i < G.n_lane; i += kT) column<1>(P, cj[i], 0, nullptr, nullptr, viol, halvings);
                for (uint32_t i = wave; i < G.n_wave; i += kWaves) column<64>(P, cj[G.n_lane + i], lane, wv0, wv0 + kWaveTiles, viol, halvings);
                for (uint32_t i = G.n_lane + G.n_wave; i < G.n; ++i) column<kT>(P, cj[i], t, blk0, blk1, viol, halvings);
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
