// Boundary-model training (vaporetto/src/trainer.rs): feature extraction, feature ids, the design matrix and the vector kernels of TRON.
//
// Feature extraction: a thread per boundary enumerates the boundary's features exactly as Trainer::gen_features does (trainer.rs:260-318) --
// char n-grams and type n-grams of the window, dictionary words by Left / Inside / Right -- once to count them and once to write them as
// 128-bit keys (TrainKey below).  Dictionary matches are found per start char by a hash of (code points, length) over a table compiled on
// the host, verified char by char: every occurrence of every word, nested and overlapping ones included (find_overlapping_iter).
//
// Feature ids: the keys go into an open-addressing table (compare-and-swap of an occurrence index); the distinct keys are compacted and
// sorted by a stable LSD radix sort; column j is the j-th distinct key in key order.  Each row's ids are sorted and duplicates merged
// into counts (trainer.rs:321-350: a feature occurring twice at a boundary has value 2).  The CSC copy is the same radix sort of the
// nonzeros by column (stable: rows ascend within a column).
//
// TRON: every reduction has a fixed shape -- a block sums a fixed tile in a fixed order and a fixed tree, columns are cut into segments of
// 64 nonzeros summed in order, level by level -- so that no sum depends on scheduling.  There are no float atomics.
#include "kernels.hpp"

#include <cmath>
#include <utility>

#include "device_common.h"
#include "tron.h"

namespace vpt {
namespace {

constexpr uint32_t kTile = kTrainThreads * 16;   // items per block of the scans, the sort and the reductions
constexpr uint32_t kSeg = 64;                     // nonzeros (partial sums) a column segment of Xᵀv adds up

// word index + 1 of the dictionary word chars[at .. at + len) is, else 0
__device__ __forceinline__ uint32_t dict_find(const TrainFeatParams& P, const uint32_t* chars, uint32_t len, uint64_t h) {
    for (uint64_t s = cps_hash_finish(h, len) & P.dict_mask;; s = (s + 1) & P.dict_mask) {
        const uint32_t e = P.dict_slots[s];
        if (e == 0) return 0;
        const uint64_t w0 = P.dict_off[e - 1], w1 = P.dict_off[e];
        if (w1 - w0 != len) continue;
        bool eq = true;
        for (uint32_t k = 0; k < len && eq; ++k) eq = P.dict_cps[w0 + k] == (chars[k] & kCharMaskTrain);
        if (eq) return e;
    }
}

// Trainer::gen_features for local boundary p of a sentence of n chars (trainer.rs:260-318); kEmit: write the keys from `at` on
template <bool kEmit>
__device__ uint32_t boundary_features(const TrainFeatParams& P, const uint32_t* chars, uint32_t n, uint32_t p, uint64_t at) {
    uint32_t cnt = 0;
    uint32_t tmp[5];
    for (int kind = 0; kind < 2; ++kind) {
        const uint32_t w = kind ? P.typew : P.charw, ng = kind ? P.typen : P.charn;
        for (uint32_t m = 0; m < ng; ++m) {
            const uint32_t lo = p + 1 > w ? p + 1 - w : 0;
            const uint32_t hi0 = p + 1 + w < n ? p + 1 + w : n;
            const uint32_t hi = hi0 > m ? hi0 - m : 0;
            for (uint32_t j = lo; j < hi; ++j) {
                if (kEmit) {
                    for (uint32_t k = 0; k <= m; ++k) tmp[k] = kind ? (chars[j + k] >> 24) : chars[j + k];
                    put_train_key(P.keys, at + cnt, uint32_t(kind), tmp, m + 1, m + 1, int32_t(j) - int32_t(p) - 1);
                }
                ++cnt;
            }
        }
    }
    if (P.dict_mask != 0) {
        // a word chars[s .. s + L) touches boundary p as Left (s = p + 1), Right (s + L - 1 = p) or Inside (s <= p < s + L - 1)
        const uint32_t maxl = P.dict_maxlen;
        for (uint32_t s = p + 1 >= maxl ? p + 1 - maxl : 0; s <= p + 1; ++s) {
            uint64_t h = kCpsHashSeed;
            const uint32_t lmax = n - s < maxl ? n - s : maxl;
            for (uint32_t L = 1; L <= lmax; ++L) {
                h = cps_hash_step(h, chars[s + L - 1]);
                if (s <= p && s + L - 1 < p) continue;   // ends before the boundary
                if (!dict_find(P, chars + s, L, h)) continue;
                if (kEmit) {
                    const uint32_t c[2] = {L < P.dictn ? L : P.dictn, s == p + 1 ? 0u : (s + L - 1 == p ? 2u : 1u)};
                    put_train_key(P.keys, at + cnt, 2, c, 2, 0, -16);
                }
                ++cnt;
            }
        }
    }
    return cnt;
}

template <bool kEmit>
__global__ __launch_bounds__(kTrainThreads) void features_kernel(TrainFeatParams P) {
    const uint64_t b = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (b >= P.total_b) return;
    // the sentence of flat boundary b: the last i with ooff[i] <= b (sentences of one char have no boundary)
    uint64_t lo = 0, hi = P.n_sent;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (P.ooff[mid] <= b) lo = mid; else hi = mid;
    }
    const uint32_t n = uint32_t(P.ooff[lo + 1] - P.ooff[lo] + 1), p = uint32_t(b - P.ooff[lo]);
    const uint32_t* chars = P.cps + P.ooff[lo] + lo;
    if (kEmit) boundary_features<true>(P, chars, n, p, P.row_off[b]);
    else P.counts[b] = boundary_features<false>(P, chars, n, p, 0);
}

// The labels of a device caller, which no host loop has seen: one above 2 (no CharacterBoundary) raises kErrBadLabel.
__global__ __launch_bounds__(kTrainThreads) void check_labels_kernel(const uint8_t* labels, uint64_t n, uint32_t* status) {
    const uint64_t i = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (i < n && labels[i] > 2) atomicOr(status, kErrBadLabel);
}

// ---------------------------------------------------------------------------------------------------- exclusive scan (u32 / u64 -> u64)
__device__ __forceinline__ uint64_t block_exclusive_scan(uint64_t v, uint64_t* lds, uint64_t* total) {
    const uint32_t t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kTrainThreads; d <<= 1) {
        const uint64_t x = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += x;
        __syncthreads();
    }
    const uint64_t incl = lds[t];
    *total = lds[kTrainThreads - 1];
    __syncthreads();
    return incl - v;
}

template <typename T>
__global__ __launch_bounds__(kTrainThreads) void scan_reduce_kernel(const T* in, uint64_t n, uint64_t* sums) {
    __shared__ uint64_t lds[kTrainThreads];
    const uint64_t base = uint64_t(blockIdx.x) * kTile + uint64_t(threadIdx.x) * 16;
    uint64_t s = 0;
    for (uint32_t k = 0; k < 16; ++k)
        if (base + k < n) s += in[base + k];
    uint64_t total;
    block_exclusive_scan(s, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one block: sums[0 .. nb) -> exclusive, out[n] = the total
__global__ __launch_bounds__(kTrainThreads) void scan_top_kernel(uint64_t* sums, uint64_t nb, uint64_t* out, uint64_t n) {
    __shared__ uint64_t lds[kTrainThreads];
    uint64_t carry = 0;
    for (uint64_t c = 0; c < nb; c += kTrainThreads) {
        const uint64_t i = c + threadIdx.x;
        const uint64_t v = i < nb ? sums[i] : 0;
        uint64_t total;
        const uint64_t ex = block_exclusive_scan(v, lds, &total);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) out[n] = carry;
}
template <typename T>
__global__ __launch_bounds__(kTrainThreads) void scan_down_kernel(const T* in, uint64_t n, const uint64_t* sums, uint64_t* out) {
    __shared__ uint64_t lds[kTrainThreads];
    const uint64_t base = uint64_t(blockIdx.x) * kTile + uint64_t(threadIdx.x) * 16;
    uint64_t s = 0;
    for (uint32_t k = 0; k < 16; ++k)
        if (base + k < n) s += in[base + k];
    uint64_t total;
    uint64_t run = sums[blockIdx.x] + block_exclusive_scan(s, lds, &total);
    for (uint32_t k = 0; k < 16; ++k)
        if (base + k < n) { const uint64_t v = in[base + k]; out[base + k] = run; run += v; }
}

// ---------------------------------------------------------------------------------------------------- feature ids
__device__ __forceinline__ bool key_eq(const uint64_t* keys, uint64_t a, uint64_t b) {
    return keys[2 * a] == keys[2 * b] && keys[2 * a + 1] == keys[2 * b + 1];
}
// every occurrence finds (or becomes) the representative of its key: the occurrence whose index the table holds
__global__ __launch_bounds__(kTrainThreads) void insert_kernel(const uint64_t* keys, uint64_t nnz, uint64_t* table, uint64_t mask, uint32_t* rep,
                                                                 uint32_t* flag) {
    const uint64_t i = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (i >= nnz) return;
    uint64_t s = mix64(keys[2 * i] ^ mix64(keys[2 * i + 1])) & mask;
    for (;;) {
        uint64_t e = table[s];
        if (e == 0) {
            e = atomic_cas_u64(table + s, 0, i + 1);
            if (e == 0) e = i + 1;
        }
        if (key_eq(keys, e - 1, i)) { rep[i] = uint32_t(e - 1); flag[i] = e - 1 == i ? 1u : 0u; return; }
        s = (s + 1) & mask;
    }
}
// the distinct keys in first-occurrence order; slot[i] of a representative = its distinct index (read back through rep)
__global__ __launch_bounds__(kTrainThreads) void compact_kernel(const uint64_t* keys, const uint32_t* rep, const uint64_t* pos, uint64_t nnz,
                                                                  uint64_t* dkeys, uint32_t* slot) {
    const uint64_t i = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (i >= nnz || rep[i] != i) return;
    const uint64_t d = pos[i];
    dkeys[2 * d] = keys[2 * i];
    dkeys[2 * d + 1] = keys[2 * i + 1];
    slot[i] = uint32_t(d);
}
__global__ __launch_bounds__(kTrainThreads) void rank_kernel(const uint32_t* order, uint64_t nd, uint32_t* rank) {
    const uint64_t j = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (j < nd) rank[order[j]] = uint32_t(j);
}
__global__ __launch_bounds__(kTrainThreads) void ids_kernel(const uint32_t* rep, const uint32_t* slot, const uint32_t* rank, uint64_t n, uint32_t* ids) {
    const uint64_t i = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (i < n) ids[i] = rank[slot[rep[i]]];
}
__global__ __launch_bounds__(kTrainThreads) void sorted_keys_kernel(const uint64_t* dkeys, const uint32_t* order, uint64_t nd, uint64_t* out) {
    const uint64_t j = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (j >= nd) return;
    out[2 * j] = dkeys[2 * order[j]];
    out[2 * j + 1] = dkeys[2 * order[j] + 1];
}

// a row's ids sorted in place (a row is tens of ids), then the distinct ones counted / written with their counts
__global__ __launch_bounds__(kTrainThreads) void row_sort_kernel(uint32_t* ids, const uint64_t* row_off, uint64_t nrows, uint32_t* merged) {
    const uint64_t r = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (r >= nrows) return;
    const uint64_t a = row_off[r], e = row_off[r + 1];
    for (uint64_t i = a + 1; i < e; ++i) {
        const uint32_t v = ids[i];
        uint64_t j = i;
        while (j > a && ids[j - 1] > v) { ids[j] = ids[j - 1]; --j; }
        ids[j] = v;
    }
    uint32_t m = 0;
    for (uint64_t i = a; i < e; ++i) m += (i == a || ids[i] != ids[i - 1]) ? 1u : 0u;
    merged[r] = m;
}
__global__ __launch_bounds__(kTrainThreads) void row_merge_kernel(const uint32_t* ids, const uint64_t* row_off, const uint64_t* csr_ptr, uint64_t nrows,
                                                                    uint32_t* cols, uint16_t* vals, uint32_t* rows, uint32_t* status) {
    const uint64_t r = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (r >= nrows) return;
    uint64_t o = csr_ptr[r];
    const uint64_t a = row_off[r], e = row_off[r + 1];
    for (uint64_t i = a; i < e;) {
        uint64_t k = i + 1;
        while (k < e && ids[k] == ids[i]) ++k;
        if (k - i > 0xFFFFu) atomicOr(status, 1u);
        cols[o] = ids[i];
        vals[o] = uint16_t(k - i);
        rows[o] = uint32_t(r);
        ++o;
        i = k;
    }
}

// ---------------------------------------------------------------------------------------------------- stable LSD radix sort of indices
// digit of item x: (base[stride * x] >> shift) & 255
__global__ __launch_bounds__(kTrainThreads) void radix_hist_kernel(const uint32_t* base, uint32_t stride, uint32_t shift, const uint32_t* idx, uint64_t n,
                                                                     uint64_t nblk, uint64_t* hist) {
    __shared__ uint32_t cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t t0 = uint64_t(blockIdx.x) * kTile;
    for (uint32_t k = 0; k < 16; ++k) {
        const uint64_t i = t0 + uint64_t(k) * kTrainThreads + threadIdx.x;
        if (i < n) atomicAdd(&cnt[(base[uint64_t(stride) * idx[i]] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[uint64_t(threadIdx.x) * nblk + blockIdx.x] = cnt[threadIdx.x];
}
// the tile in rounds of 256 items, in order: an item's place = the digit's offset for this block + items of that digit in earlier rounds,
// earlier waves of the round, and lower lanes of its wave (eight ballots find the lanes with the same digit)
__global__ __launch_bounds__(kTrainThreads) void radix_scatter_kernel(const uint32_t* base, uint32_t stride, uint32_t shift, const uint32_t* idx_in,
                                                                        uint32_t* idx_out, uint64_t n, uint64_t nblk, const uint64_t* off) {
    constexpr uint32_t kWaves = kTrainThreads / 64;
    __shared__ uint64_t run[256];
    __shared__ uint32_t wcnt[kWaves][256];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    run[t] = off[uint64_t(t) * nblk + blockIdx.x];
    const uint64_t t0 = uint64_t(blockIdx.x) * kTile;
    const uint64_t below = (uint64_t(1) << lane) - 1u;
    for (uint32_t k = 0; k < 16; ++k) {
        for (uint32_t w = 0; w < kWaves; ++w) wcnt[w][t] = 0;
        __syncthreads();
        const uint64_t i = t0 + uint64_t(k) * kTrainThreads + t;
        const bool valid = i < n;
        const uint32_t x = valid ? idx_in[i] : 0u;
        const uint32_t d = valid ? (base[uint64_t(stride) * x] >> shift) & 255u : 0u;
        uint64_t peers = __ballot(valid);
        for (uint32_t bit = 0; bit < 8; ++bit) {
            const uint64_t b = __ballot(((d >> bit) & 1u) != 0);
            peers &= ((d >> bit) & 1u) ? b : ~b;
        }
        const uint32_t rank = uint32_t(__popcll(peers & below));
        if (valid && rank == 0) wcnt[wave][d] = uint32_t(__popcll(peers));
        __syncthreads();
        if (valid) {
            uint64_t o = run[d] + rank;
            for (uint32_t w = 0; w < wave; ++w) o += wcnt[w][d];
            idx_out[o] = x;
        }
        __syncthreads();
        uint32_t add = 0;
        for (uint32_t w = 0; w < kWaves; ++w) add += wcnt[w][t];
        run[t] += add;
        __syncthreads();
    }
}
__global__ __launch_bounds__(kTrainThreads) void iota_kernel(uint32_t* idx, uint64_t n) {
    const uint64_t i = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (i < n) idx[i] = uint32_t(i);
}

// ---------------------------------------------------------------------------------------------------- the CSC copy and its segments
__global__ __launch_bounds__(kTrainThreads) void csc_fill_kernel(const uint32_t* order, const uint32_t* cols, const uint16_t* vals, const uint32_t* rows,
                                                                   uint64_t nnz, uint32_t* crow, uint16_t* cval, uint64_t* cptr) {
    const uint64_t k = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (k >= nnz) return;
    const uint32_t x = order[k];
    crow[k] = rows[x];
    cval[k] = vals[x];
    if (k == 0 || cols[order[k - 1]] != cols[x]) cptr[cols[x]] = k;   // every column has a nonzero
}
// segments of the next level: ceil(len / 64) per column
__global__ __launch_bounds__(kTrainThreads) void seg_count_kernel(const uint64_t* ptr, uint64_t nd, uint64_t* cnt) {
    const uint64_t j = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (j < nd) cnt[j] = (ptr[j + 1] - ptr[j] + kSeg - 1) / kSeg;
}
__global__ __launch_bounds__(kTrainThreads) void seg_col_kernel(const uint64_t* nptr, uint64_t nd, uint32_t* seg_col) {
    const uint64_t j = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (j >= nd) return;
    for (uint64_t s = nptr[j]; s < nptr[j + 1]; ++s) seg_col[s] = uint32_t(j);
}

// ---------------------------------------------------------------------------------------------------- TRON vectors (fp64)
// out[r] = sum over row r of count * v[col] + v[bias]
__global__ __launch_bounds__(kTrainThreads) void xv_kernel(const uint64_t* csr_ptr, const uint32_t* cols, const uint16_t* vals, uint64_t nrows,
                                                             const double* v, uint64_t bias_col, double* out) {
    const uint64_t r = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (r >= nrows) return;
    double s = 0;
    for (uint64_t k = csr_ptr[r]; k < csr_ptr[r + 1]; ++k) s += double(vals[k]) * v[cols[k]];
    out[r] = s + v[bias_col];
}
// a segment of level L + 1: the sum of up to 64 consecutive values of its column at level L (level 0: count * u[row] of the CSC)
__global__ __launch_bounds__(kTrainThreads) void xtv_level_kernel(const uint64_t* ptr, const uint64_t* nptr, const uint32_t* seg_col, uint64_t nseg,
                                                                    const double* in, const uint32_t* crow, const uint16_t* cval, const double* u,
                                                                    double* out) {
    const uint64_t s = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (s >= nseg) return;
    const uint32_t j = seg_col[s];
    const uint64_t a = ptr[j] + kSeg * (s - nptr[j]);
    const uint64_t e = a + kSeg < ptr[j + 1] ? a + kSeg : ptr[j + 1];
    double acc = 0;
    if (crow)
        for (uint64_t k = a; k < e; ++k) acc += double(cval[k]) * u[crow[k]];
    else
        for (uint64_t k = a; k < e; ++k) acc += in[k];
    out[s] = acc;
}
// partial[block] = sum of a[i] * (b ? b[i] : 1) over the block's tile: sixteen strided values per thread in order, then a fixed tree
__global__ __launch_bounds__(kTrainThreads) void dot_kernel(const double* a, const double* b, uint64_t n, double* partial) {
    __shared__ double lds[kTrainThreads];
    const uint64_t t0 = uint64_t(blockIdx.x) * kTile;
    double s = 0;
    for (uint32_t k = 0; k < 16; ++k) {
        const uint64_t i = t0 + uint64_t(k) * kTrainThreads + threadIdx.x;
        if (i < n) s += b ? a[i] * b[i] : a[i];
    }
    lds[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t h = kTrainThreads / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) lds[threadIdx.x] += lds[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = lds[0];
}
// y += alpha * x (alpha read from the host scalar)
__global__ __launch_bounds__(kTrainThreads) void axpy_kernel(uint64_t n, double alpha, const double* x, double* y) {
    const uint64_t i = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (i < n) y[i] += alpha * x[i];
}
// y = beta * y + x
__global__ __launch_bounds__(kTrainThreads) void xpby_kernel(uint64_t n, const double* x, double beta, double* y) {
    const uint64_t i = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (i < n) y[i] = beta * y[i] + x[i];
}
// y = a + b (b's last element: *bias_sum)
__global__ __launch_bounds__(kTrainThreads) void add_kernel(uint64_t n, const double* a, const double* b, const double* bias_sum, double* y) {
    const uint64_t i = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (i < n) y[i] = a[i] + (i + 1 == n ? *bias_sum : b[i]);
}
__global__ __launch_bounds__(kTrainThreads) void scale_rows_kernel(uint64_t n, const double* d, double* t) {
    const uint64_t i = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (i < n) t[i] *= d[i];
}
// the loss terms of l2r_lr_fun / l2r_l2_svc_fun::fun at z = Xw (liblinear linear.cpp)
__global__ __launch_bounds__(kTrainThreads) void loss_kernel(uint64_t n, const double* z, const double* y, double c, int solver, double* loss) {
    const uint64_t i = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (i >= n) return;
    loss[i] = tron_loss(y[i] * z[i], c, solver);
}
// ::grad: gz (the vector Xᵀ is applied to) and D (Hv's diagonal), from the same z
__global__ __launch_bounds__(kTrainThreads) void grad_rows_kernel(uint64_t n, const double* z, const double* y, double c, int solver, double* gz, double* D) {
    const uint64_t i = uint64_t(blockIdx.x) * kTrainThreads + threadIdx.x;
    if (i >= n) return;
    const TronRow t = tron_grad_row(y[i], y[i] * z[i], c, solver);
    D[i] = t.D;
    gz[i] = t.gz;
}

uint64_t tiles(uint64_t n) { return (n + kTile - 1) / kTile; }

}  // namespace

hipError_t train_features(const TrainFeatParams& P, bool emit, hipStream_t st) {
    if (P.total_b == 0) return hipSuccess;
    const dim3 g(uint32_t((P.total_b + kTrainThreads - 1) / kTrainThreads));
    if (emit) hipLaunchKernelGGL(features_kernel<true>, g, dim3(kTrainThreads), 0, st, P);
    else hipLaunchKernelGGL(features_kernel<false>, g, dim3(kTrainThreads), 0, st, P);
    return hipGetLastError();
}
hipError_t train_check_labels(const uint8_t* labels, uint64_t n, uint32_t* status, hipStream_t st) {
    return launch1(check_labels_kernel, n, st, labels, n, status);
}
uint64_t train_scan_scratch(uint64_t n) { return tiles(n) + 1; }
template <typename T>
hipError_t scan(const T* in, uint64_t n, uint64_t* out, uint64_t* scratch, hipStream_t st) {
    const uint64_t nb = tiles(n);
    if (nb) hipLaunchKernelGGL(scan_reduce_kernel<T>, dim3(uint32_t(nb)), dim3(kTrainThreads), 0, st, in, n, scratch);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(kTrainThreads), 0, st, scratch, nb, out, n);
    if (nb) hipLaunchKernelGGL(scan_down_kernel<T>, dim3(uint32_t(nb)), dim3(kTrainThreads), 0, st, in, n, (const uint64_t*)scratch, out);
    return hipGetLastError();
}
hipError_t train_scan(const uint32_t* in, uint64_t n, uint64_t* out, uint64_t* scratch, hipStream_t st) { return scan(in, n, out, scratch, st); }
hipError_t train_scan(const uint64_t* in, uint64_t n, uint64_t* out, uint64_t* scratch, hipStream_t st) { return scan(in, n, out, scratch, st); }
hipError_t train_insert(const uint64_t* keys, uint64_t nnz, uint64_t* table, uint64_t mask, uint32_t* rep, uint32_t* flag, hipStream_t st) {
    return launch1(insert_kernel, nnz, st, keys, nnz, table, mask, rep, flag);
}
hipError_t train_compact(const uint64_t* keys, const uint32_t* rep, const uint64_t* pos, uint64_t nnz, uint64_t* dkeys, uint32_t* slot, hipStream_t st) {
    return launch1(compact_kernel, nnz, st, keys, rep, pos, nnz, dkeys, slot);
}
uint64_t train_radix_scratch(uint64_t n) { return 256 * tiles(n); }
hipError_t train_radix_sort(const uint32_t* base, uint32_t stride, const uint32_t* word_shifts, uint32_t n_passes, uint64_t n, uint32_t* idx,
                            uint32_t* idx_tmp, uint64_t* hist, uint64_t* hist_scan, uint64_t* scan_scratch, hipStream_t st) {
    hipError_t e = launch1(iota_kernel, n, st, idx, n);
    if (e != hipSuccess || n == 0) return e;
    const uint64_t nb = tiles(n);
    for (uint32_t p = 0; p < n_passes; ++p) {
        const uint32_t word = word_shifts[p] >> 8, shift = word_shifts[p] & 255u;
        hipLaunchKernelGGL(radix_hist_kernel, dim3(uint32_t(nb)), dim3(kTrainThreads), 0, st, base + word, stride, shift, (const uint32_t*)idx, n, nb, hist);
        if ((e = train_scan(hist, 256 * nb, hist_scan, scan_scratch, st)) != hipSuccess) return e;
        hipLaunchKernelGGL(radix_scatter_kernel, dim3(uint32_t(nb)), dim3(kTrainThreads), 0, st, base + word, stride, shift, (const uint32_t*)idx,
                           idx_tmp, n, nb, (const uint64_t*)hist_scan);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        std::swap(idx, idx_tmp);
    }
    if (n_passes & 1) return hipMemcpyAsync(idx_tmp, idx, n * 4, hipMemcpyDeviceToDevice, st);   // the result in the caller's idx
    return hipSuccess;
}
hipError_t train_ids(const uint32_t* order, uint64_t nd, uint32_t* rank, const uint32_t* rep, const uint32_t* slot, uint64_t n, uint32_t* ids, hipStream_t st) {
    hipError_t e = launch1(rank_kernel, nd, st, order, nd, rank);
    if (e == hipSuccess) e = launch1(ids_kernel, n, st, rep, slot, (const uint32_t*)rank, n, ids);
    return e;
}
hipError_t train_sorted_keys(const uint64_t* dkeys, const uint32_t* order, uint64_t nd, uint64_t* sorted_keys, hipStream_t st) {
    return launch1(sorted_keys_kernel, nd, st, dkeys, order, nd, sorted_keys);
}
hipError_t train_row_sort(uint32_t* ids, const uint64_t* row_off, uint64_t nrows, uint32_t* merged, hipStream_t st) {
    return launch1(row_sort_kernel, nrows, st, ids, row_off, nrows, merged);
}
hipError_t train_row_merge(const uint32_t* ids, const uint64_t* row_off, const uint64_t* csr_ptr, uint64_t nrows, uint32_t* cols, uint16_t* vals,
                           uint32_t* rows, uint32_t* status, hipStream_t st) {
    return launch1(row_merge_kernel, nrows, st, ids, row_off, csr_ptr, nrows, cols, vals, rows, status);
}
hipError_t train_csc_fill(const uint32_t* order, const uint32_t* cols, const uint16_t* vals, const uint32_t* rows, uint64_t nnz, uint32_t* crow,
                          uint16_t* cval, uint64_t* cptr, hipStream_t st) {
    return launch1(csc_fill_kernel, nnz, st, order, cols, vals, rows, nnz, crow, cval, cptr);
}
hipError_t train_seg_count(const uint64_t* ptr, uint64_t nd, uint64_t* cnt, hipStream_t st) { return launch1(seg_count_kernel, nd, st, ptr, nd, cnt); }
hipError_t train_seg_col(const uint64_t* nptr, uint64_t nd, uint32_t* seg_col, hipStream_t st) { return launch1(seg_col_kernel, nd, st, nptr, nd, seg_col); }
hipError_t train_xv(const uint64_t* csr_ptr, const uint32_t* cols, const uint16_t* vals, uint64_t nrows, const double* v, uint64_t bias_col, double* out,
                    hipStream_t st) {
    return launch1(xv_kernel, nrows, st, csr_ptr, cols, vals, nrows, v, bias_col, out);
}
hipError_t train_xtv_level(const uint64_t* ptr, const uint64_t* nptr, const uint32_t* seg_col, uint64_t nseg, const double* in, const uint32_t* crow,
                           const uint16_t* cval, const double* u, double* out, hipStream_t st) {
    return launch1(xtv_level_kernel, nseg, st, ptr, nptr, seg_col, nseg, in, crow, cval, u, out);
}
uint64_t train_dot_partials(uint64_t n) { return tiles(n); }
hipError_t train_dot(const double* a, const double* b, uint64_t n, double* partial, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(dot_kernel, dim3(uint32_t(tiles(n))), dim3(kTrainThreads), 0, st, a, b, n, partial);
    return hipGetLastError();
}
hipError_t train_axpy(uint64_t n, double alpha, const double* x, double* y, hipStream_t st) { return launch1(axpy_kernel, n, st, n, alpha, x, y); }
hipError_t train_xpby(uint64_t n, const double* x, double beta, double* y, hipStream_t st) { return launch1(xpby_kernel, n, st, n, x, beta, y); }
hipError_t train_add(uint64_t n, const double* a, const double* b, const double* bias_sum, double* y, hipStream_t st) {
    return launch1(add_kernel, n, st, n, a, b, bias_sum, y);
}
hipError_t train_scale_rows(uint64_t n, const double* d, double* t, hipStream_t st) { return launch1(scale_rows_kernel, n, st, n, d, t); }
hipError_t train_loss(uint64_t n, const double* z, const double* y, double c, int solver, double* loss, hipStream_t st) {
    return launch1(loss_kernel, n, st, n, z, y, c, solver, loss);
}
hipError_t train_grad_rows(uint64_t n, const double* z, const double* y, double c, int solver, double* gz, double* D, hipStream_t st) {
    return launch1(grad_rows_kernel, n, st, n, z, y, c, solver, gz, D);
}

}  // namespace vpt
