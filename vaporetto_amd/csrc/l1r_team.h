// What the device backends of solvers 5 and 6 share (kernels_train_l1.hip and kernels_train_l1lr.hip over global memory,
// kernels_train_tags_l1.hip and kernels_train_tags_l1lr.hip a tag problem in LDS): the team that sums over a column, the dealing of a
// launch's columns, and the in-kernel solvers' LDS plan.  Each is stated here and nowhere else.
//
// Who takes a column, by its nonzeros: a lane one of at most kL1rLaneMax (a wave takes 64 such columns), a wave one of at most
// kL1rWaveMax, a workgroup a longer one (the bias column -- every row, value 1 -- among them).  The two thresholds are the sizes at
// which the next unit has something to do for every member under the summation rule; they are not measured optima.
//
// Summation rule (the one of the segments of Xᵀv in kernels_train.hip): a column's sum is taken over fixed tiles of 64 nonzeros, each
// summed in index order by one thread; the tile sums are summed 64 at a time in index order, level by level, until one is left.  The
// shape of that tree depends on the column's length alone, so a column's sums have the same bits whichever unit took the column,
// whatever the launch geometry, and whether a group launch or an in-kernel solver asked for them: both paths of a tag trainer stop at
// the same sweep.  A wave keeps its tile sums in LDS; a workgroup in global scratch (a group launch) or in LDS (an in-kernel solver).
#pragma once
#include <type_traits>

#include "kernels.hpp"

#include "device_common.h"
#include "l1r.h"

namespace vpt {

// ---- the column team
constexpr uint32_t kL1rTileNz = 64;                              // nonzeros (partial sums) a thread adds up in order
constexpr uint32_t kL1rWaveTiles = kL1rWaveMax / kL1rTileNz;     // tile sums a wave keeps in LDS
static_assert(kL1rLaneMax == kL1rTileNz && kL1rWaveTiles >= 1 && kL1rWaveTiles <= 64, "a lane takes one tile, a wave's second level is one sum");

// the lanes of a wave meet: what they wrote to LDS before is what they read after
__device__ __forceinline__ void wave_rendezvous() {
#ifndef VPT_HIPEMU
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#endif
    __builtin_amdgcn_wave_barrier();
}

// kN threads (1: a lane, 64: a wave, kTrainThreads: the workgroup) over a column of n nonzeros; I: the width of the index arithmetic.
// What nonzero k is -- its row, its value -- is the caller's.
template <uint32_t kN, typename I>
struct L1rTeam {
    I n;
    uint32_t t;         // this thread in the team
    L1rPair *s0, *s1;   // the levels' sums, written in turn

    __device__ __forceinline__ void sync() const {
        if constexpr (kN == 64) wave_rendezvous();
        else if constexpr (kN > 64) __syncthreads();
    }
    // the tile that starts at nonzero k0, in index order
    template <typename F>
    __device__ __forceinline__ L1rPair tile(I k0, F term) const {
        const I k1 = k0 + kL1rTileNz < n ? k0 + kL1rTileNz : n;
        L1rPair acc{0.0, 0.0};
        for (I k = k0; k < k1; ++k) acc = l1r_add(acc, term(k));
        return acc;
    }
    // the sum of term(0) .. term(n - 1) by the summation rule, the same bits in every thread of the team
    template <typename F>
    __device__ L1rPair sums(F term) const {
        if constexpr (kN == 1) return tile(0, term);
        I m = (n + kL1rTileNz - 1) / kL1rTileNz;
        for (I i = t; i < m; i += kN) s0[i] = tile(i * kL1rTileNz, term);
        sync();
        L1rPair *src = s0, *dst = s1;
        while (m > 1) {
            const I g = (m + kL1rTileNz - 1) / kL1rTileNz;
            for (I i = t; i < g; i += kN) {
                const I q1 = (i + 1) * kL1rTileNz < m ? (i + 1) * kL1rTileNz : m;
                L1rPair acc{0.0, 0.0};
                for (I q = i * kL1rTileNz; q < q1; ++q) acc = l1r_add(acc, src[q]);
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
    // the write pass: fn(k) for the nonzeros of this thread
    template <typename F>
    __device__ __forceinline__ void each(F fn) const {
        for (I k = t; k < n; k += kN) fn(k);
    }
};
template <uint32_t kN>
using L1rTeamSize = std::integral_constant<uint32_t, kN>;

// ---- the dealer of a launch
constexpr uint32_t kL1rWaves = kTrainThreads / 64;
// workgroups of a launch over n_lane + n_wave + n_block columns
VPT_HDC uint32_t l1r_launch_blocks(uint32_t n_lane, uint32_t n_wave, uint32_t n_block) {
    return (n_lane + kTrainThreads - 1) / kTrainThreads + (n_wave + kL1rWaves - 1) / kL1rWaves + n_block;
}
// cols: the launch's columns, those a lane takes first, then a wave's, then a workgroup's; fn(team size, column, thread in the team, s0,
// s1).  A workgroup column's place in tile0 / tile1 follows from where its nonzeros start (the bias, column nd, behind every column),
// so the columns of a launch do not meet there.  lds: kL1rWaves rows of the kernel's
template <typename F>
__device__ __forceinline__ void l1r_deal_launch(const uint32_t* cols, uint32_t n_lane, uint32_t n_wave, uint32_t n_block, L1rPair (*lds)[kL1rWaveTiles + 1],
                                                uint64_t nd, uint64_t nnz, const uint64_t* cptr, L1rPair* tile0, L1rPair* tile1, F fn) {
    const uint32_t lane_blocks = l1r_launch_blocks(n_lane, 0, 0), wave_blocks = l1r_launch_blocks(0, n_wave, 0);
    uint32_t bx = blockIdx.x;
    if (bx < lane_blocks) {
        const uint32_t i = bx * kTrainThreads + threadIdx.x;
        if (i < n_lane) fn(L1rTeamSize<1>{}, cols[i], 0u, nullptr, nullptr);
        return;
    }
    bx -= lane_blocks;
    if (bx < wave_blocks) {
        const uint32_t wave = threadIdx.x >> 6, i = bx * kL1rWaves + wave;
        if (i < n_wave) fn(L1rTeamSize<64>{}, cols[n_lane + i], threadIdx.x & 63u, lds[wave], lds[wave] + kL1rWaveTiles);
        return;
    }
    bx -= wave_blocks;
    if (bx >= n_block) return;
    const uint32_t j = cols[n_lane + n_wave + bx];
    const uint64_t start = j == nd ? nnz : cptr[j];
    fn(L1rTeamSize<kTrainThreads>{}, j, threadIdx.x, tile0 + (start >> 6) + j, tile1 + (start >> 12) + j);
}

// ---- the in-kernel plan of the tag solvers: a workgroup per problem, one static LDS array of kTagL1Doubles doubles
// Behind the problem's own vectors (kTagL1LdsDoubles), in doubles: [0, kTagL1RedDoubles) the workgroup's level sums (a column has at
// most kTagL1LdsDoubles rows) or the tree of the sums over a vector; then the waves' tile sums; then the groups' order, and behind the
// order solver 5's halvings.
constexpr uint32_t kTagL1BlkTiles0 = (kTagL1LdsDoubles + kL1rTileNz - 1) / kL1rTileNz, kTagL1BlkTiles1 = (kTagL1BlkTiles0 + kL1rTileNz - 1) / kL1rTileNz;
constexpr uint32_t kTagL1RedDoubles = 264;
constexpr uint32_t kTagL1WaveDoubles = 2 * kL1rWaves * (kL1rWaveTiles + 1);
constexpr uint32_t kTagL1OrderDoubles = kTagL1MaxGroups / 2 + 8;
constexpr uint32_t kTagL1Doubles = kTagL1LdsDoubles + kTagL1RedDoubles + kTagL1WaveDoubles + kTagL1OrderDoubles;
static_assert(kTrainThreads == 256, "vec_sum's tree and its tiles of 16 values a thread");
static_assert(2 * (kTagL1BlkTiles0 + kTagL1BlkTiles1) <= kTagL1RedDoubles && kTrainThreads + 2 <= kTagL1RedDoubles && kTagL1BlkTiles1 <= kL1rTileNz,
              "the level sums and the tree share a place");
static_assert(kTagL1LdsDoubles <= 2 * 16 * kTrainThreads, "a vector is at most two tiles of the tree");
static_assert(kTagL1Doubles * 8 <= 61568, "the static LDS array of tag_solve_kernel is the budget");

struct TagL1Lds {
    double* red;
    L1rPair *blk0, *blk1, *wv0;   // wv0: this thread's wave's
    uint32_t* order;
};
__device__ __forceinline__ TagL1Lds tag_l1_lds(double* lds) {
    double* const red = lds + kTagL1LdsDoubles;
    L1rPair* const blk0 = reinterpret_cast<L1rPair*>(red);
    return {red, blk0, blk0 + kTagL1BlkTiles0, reinterpret_cast<L1rPair*>(red + kTagL1RedDoubles) + (threadIdx.x >> 6) * (kL1rWaveTiles + 1),
            reinterpret_cast<uint32_t*>(red + kTagL1RedDoubles + kTagL1WaveDoubles)};
}

// s + v with v rounded first: never fused with the product that made v
__device__ __forceinline__ double add_rounded(double s, double v) {
#pragma clang fp contract(off)
    return s + v;
}
// the sum of f(0) .. f(n - 1) in the shape of dot_kernel (kernels_train.hip) and its second level: tiles of 4096, a thread its sixteen
// strided values in order, a halving tree over the 256; the same bits in every thread.  red: kTrainThreads + 2 doubles.  The caller
// has met since f's inputs were written.
// kRounded: solver 6 rounds a term before it is added, as the host driver's term kernels store it; solver 5 leaves the device free to
// contract its loss term c d d into the sum, and its objective's last bit rests on that.
template <bool kRounded, typename F>
__device__ double tag_l1_vec_sum(uint32_t n, F f, double* red) {
    constexpr uint32_t kT = kTrainThreads;
    const uint32_t t = threadIdx.x, m = (n + 16 * kT - 1) / (16 * kT);
    for (uint32_t tile = 0; tile < m; ++tile) {
        double s = 0;
        for (uint32_t k = 0; k < 16; ++k) {
            const uint32_t i = tile * 16 * kT + k * kT + t;
            if (i < n) {
                if constexpr (kRounded) s = add_rounded(s, f(i));
                else s += f(i);
            }
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

// a group's columns (cj: the problem's columns from the group's first) by length class; every thread comes through every workgroup
// column.  fn as l1r_deal_launch's
template <typename F>
__device__ __forceinline__ void tag_l1_deal(const TagL1Group& G, const uint32_t* cj, const TagL1Lds& L, F fn) {
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    for (uint32_t i = t; i < G.n_lane; i += kTrainThreads) fn(L1rTeamSize<1>{}, cj[i], 0u, nullptr, nullptr);
    for (uint32_t i = wave; i < G.n_wave; i += kL1rWaves) fn(L1rTeamSize<64>{}, cj[G.n_lane + i], lane, L.wv0, L.wv0 + kL1rWaveTiles);
    for (uint32_t i = G.n_lane + G.n_wave; i < G.n; ++i) fn(L1rTeamSize<kTrainThreads>{}, cj[i], t, L.blk0, L.blk1);
}

}  // namespace vpt
