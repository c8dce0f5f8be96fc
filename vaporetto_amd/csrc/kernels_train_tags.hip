// Tag-model training (vaporetto/src/tag_trainer.rs): the examples and their features, and the batched TRON solver.
//
// Extraction: a thread per char finds out whether a token of Sentence::iter_tokens ends there (the sentence's last char or a WordBoundary
// behind it, no Unknown boundary inside the token) in a sentence with tag slots; such a token is an example.  Its features are the
// n-grams that cover the whole token plus n + 1 more chars (or char types), `rel` of them to the right of the token
// (tag_trainer.rs:79-100); inside one surface's group the token itself is constant, so a feature's key holds the context alone:
//   kind << 120 | c0 << 99 | .. | c4 << 15 | (n + 1) << 5 | (rel + 16)      (kernels_train.hip's TrainKey; left context, then right)
// One pass counts, a scan places, one pass writes the example records (sentence, start, end, features) and the keys.
//
// The solver: a workgroup per (surface, slot) problem runs liblinear's TRON for solvers 0 and 2 entirely inside the kernel, one class
// after another over the same matrix (one solve for two classes).  The algorithm is tron.h's, the same text the host driver of
// capi_train.cpp runs; TagProb below is its backend here.  The fp64 vectors live in LDS; the 0/1 matrix is read as CSR (Xv: a thread
// per row) and CSC (Xᵀv: a thread per column) indices from global memory.  Every sum has a fixed shape: a thread adds its strided
// elements in order, sixteen threads add sixteen partial sums each in order, and every thread adds those sixteen in order -- no float
// atomics, and the scalars that steer the loop are the same bits in every thread.
#include "kernels.hpp"

#include <cmath>

#include "device_common.h"
#include "tron.h"

namespace vpt {
namespace {

constexpr uint32_t kTagThreads = kTrainThreads;

// the features of token [start, end) of a sentence of n chars (tag_trainer.rs:79-100); kEmit: write the keys from `at` on
template <bool kEmit>
__device__ uint32_t token_features(const TagFeatParams& P, const uint32_t* chars, uint32_t n, uint32_t start, uint32_t end, uint64_t at) {
    uint32_t cnt = 0;
    uint32_t tmp[5];
    for (uint32_t kind = 0; kind < 2; ++kind) {
        const uint32_t ng = kind ? P.typen : P.charn;
        for (uint32_t m = 1; m <= ng; ++m) {   // m = n + 1 extra chars
            for (uint32_t left = m < start ? m : start;; --left) {
                const uint32_t right = m - left;
                if (right > n - end) break;   // fewer chars to the left only ask for more to the right
                if (kEmit) {
                    for (uint32_t k = 0; k < left; ++k) tmp[k] = chars[start - left + k];
                    for (uint32_t k = 0; k < right; ++k) tmp[left + k] = chars[end + k];
                    for (uint32_t k = 0; k < m; ++k) tmp[k] = kind ? (tmp[k] >> 24) : (tmp[k] & kCharMaskTrain);
                    put_train_key(P.keys, at + cnt, kind, tmp, m, m, int32_t(right));
                }
                ++cnt;
                if (left == 0) break;
            }
        }
    }
    return cnt;
}

template <bool kEmit>
__global__ __launch_bounds__(kTagThreads) void tag_features_kernel(TagFeatParams P) {
    const uint64_t g = uint64_t(blockIdx.x) * kTagThreads + threadIdx.x;
    if (g >= P.total_chars) return;
    // the sentence of flat char g: the last i with ooff[i] + i <= g
    uint64_t lo = 0, hi = P.n_sent;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (P.ooff[mid] + mid <= g) lo = mid; else hi = mid;
    }
    const uint64_t c0 = P.ooff[lo] + lo;
    const uint32_t n = uint32_t(P.ooff[lo + 1] - P.ooff[lo] + 1), e = uint32_t(g - c0);
    const uint8_t* lab = P.labels + P.ooff[lo];
    bool ex = P.n_tags[lo] != 0 && (e + 1 == n || lab[e] == 1);
    uint32_t start = e;
    while (ex && start > 0 && lab[start - 1] != 1) {
        if (lab[start - 1] != 0) ex = false;   // an Unknown boundary inside: TokenIterator skips the token
        --start;
    }
    if (!kEmit) {
        P.is_ex[g] = ex ? 1u : 0u;
        P.counts[g] = ex ? token_features<false>(P, P.cps + c0, n, start, e + 1, 0) : 0u;
        return;
    }
    if (!ex) return;
    const uint64_t x = P.ex_off[g];
    const uint32_t cnt = token_features<true>(P, P.cps + c0, n, start, e + 1, P.key_off[g]);
    P.recs[4 * x] = uint32_t(lo);
    P.recs[4 * x + 1] = start;
    P.recs[4 * x + 2] = e + 1;
    P.recs[4 * x + 3] = cnt;
}

// the gold tags' CSR (vpt_parse_tokenized_batch's layout) before anything follows its offsets: status |= 1 tag_index, |= 2 span_offsets
__global__ __launch_bounds__(kTagThreads) void tag_validate_kernel(const uint32_t* n_tags, const uint64_t* ooff, uint64_t n_sent, uint64_t total_chars,
                                                                     const uint64_t* tag_index, const uint64_t* span_off, uint64_t n_spans,
                                                                     uint64_t n_tag_bytes, uint32_t* status) {
    const uint64_t g = uint64_t(blockIdx.x) * kTagThreads + threadIdx.x;
    if (g < total_chars) {
        uint64_t lo = 0, hi = n_sent;
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (ooff[mid] + mid <= g) lo = mid; else hi = mid;
        }
        const uint64_t a = tag_index[g], b = tag_index[g + 1];
        if (a > b || b > n_spans || b - a > n_tags[lo]) atomicOr(status, 1u);
    }
    if (g < n_spans) {
        const uint64_t a = span_off[g], b = span_off[g + 1];
        if (a > b || b > n_tag_bytes) atomicOr(status, 2u);
    }
}

// ---------------------------------------------------------------------------------------------------- the batched TRON
// the sum of v over the workgroup, the same bits in every thread
__device__ __forceinline__ double blk_sum(double v, double* red) {
    const uint32_t t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    if (t < 16) {
        double s = 0;
        for (uint32_t k = 0; k < 16; ++k) s += red[16 * t + k];
        red[kTagThreads + t] = s;
    }
    __syncthreads();
    double r = 0;
    for (uint32_t k = 0; k < 16; ++k) r += red[kTagThreads + k];
    return r;
}
__device__ __forceinline__ double blk_dot(const double* a, const double* b, uint32_t n, double* red) {
    double s = 0;
    for (uint32_t i = threadIdx.x; i < n; i += kTagThreads) s += a[i] * b[i];
    return blk_sum(s, red);
}

// the in-kernel backend of tron.h: one class of a problem, the workgroup's threads over vectors in LDS
struct TagProb {
    const uint32_t *rp, *cols, *cp, *crow, *y;
    uint32_t nf, l, n, cls;
    double c;
    int solver;
    double *z, *D, *tmp, *red;
    TronVectors v;

    // out = Xx (the bias column last)
    __device__ __forceinline__ void xv(const double* x, double* out) const {
        for (uint32_t r = threadIdx.x; r < l; r += kTagThreads) {
            double s = 0;
            for (uint32_t k = rp[r]; k < rp[r + 1]; ++k) s += x[cols[k]];
            out[r] = s + x[nf];
        }
        __syncthreads();
    }
    // out = a + Xᵀu
    __device__ __forceinline__ void add_xtv(const double* a, const double* u, double* out) const {
        double b = 0;
        for (uint32_t r = threadIdx.x; r < l; r += kTagThreads) b += u[r];
        b = blk_sum(b, red);
        for (uint32_t j = threadIdx.x; j < nf; j += kTagThreads) {
            double s = 0;
            for (uint32_t k = cp[j]; k < cp[j + 1]; ++k) s += u[crow[k]];
            out[j] = a[j] + s;
        }
        if (threadIdx.x == 0) out[nf] = a[nf] + b;
        __syncthreads();
    }
    __device__ __forceinline__ double target(uint32_t r) const { return y[r] == cls ? 1.0 : -1.0; }
    __device__ double fun(const double* x) const {
        xv(x, z);
        double s = 0;
        for (uint32_t r = threadIdx.x; r < l; r += kTagThreads) s += tron_loss(target(r) * z[r], c, solver);
        const double loss = blk_sum(s, red);
        return blk_dot(x, x, n, red) / 2.0 + loss;
    }
    __device__ void grad(const double* x, double* out) const {
        for (uint32_t r = threadIdx.x; r < l; r += kTagThreads) {
            const double yr = target(r);
            const TronRow t = tron_grad_row(yr, yr * z[r], c, solver);
            D[r] = t.D;
            tmp[r] = t.gz;
        }
        __syncthreads();
        add_xtv(x, tmp, out);
    }
    __device__ void hv(const double* x, double* out) const {
        xv(x, tmp);
        for (uint32_t r = threadIdx.x; r < l; r += kTagThreads) tmp[r] *= D[r];
        __syncthreads();
        add_xtv(x, tmp, out);
    }
    __device__ __forceinline__ double dot(const double* a, const double* b) const { return blk_dot(a, b, n, red); }
    // the vector loops: a thread its strided elements, then the workgroup meets
    template <typename F>
    __device__ __forceinline__ void each(F f) const {
        for (uint32_t i = threadIdx.x; i < n; i += kTagThreads) f(i);
        __syncthreads();
    }
    __device__ __forceinline__ void zero(double* x) const { each([=](uint32_t i) { x[i] = 0; }); }
    __device__ __forceinline__ void copy(const double* x, double* out) const { each([=](uint32_t i) { out[i] = x[i]; }); }
    __device__ __forceinline__ void add(const double* a, const double* b, double* out) const { each([=](uint32_t i) { out[i] = a[i] + b[i]; }); }
    __device__ __forceinline__ void axpy(double a, const double* x, double* y_) const { each([=](uint32_t i) { y_[i] += a * x[i]; }); }
    __device__ __forceinline__ void xpby(const double* x, double b, double* y_) const { each([=](uint32_t i) { y_[i] = b * y_[i] + x[i]; }); }
    __device__ __forceinline__ void cg_start() const { each([=](uint32_t i) { v.s[i] = 0; v.r[i] = -v.g[i]; v.d[i] = -v.g[i]; }); }
    __device__ __forceinline__ void cg_boundary(double a) const { each([=](uint32_t i) { v.s[i] += a * v.d[i]; v.r[i] += -a * v.Hd[i]; }); }
    // exact CG ends within n steps; the cap only keeps a non-finite problem from spinning on the device
    __device__ __forceinline__ bool cg_more(int k) const { return uint32_t(k) < 16 * n + 64; }
    __device__ __forceinline__ bool ok() const { return true; }
};

__global__ __launch_bounds__(kTagThreads) void tag_solve_kernel(const TagSolveDesc* descs, const uint32_t* rp, const uint32_t* cols, const uint32_t* cp,
                                                                  const uint32_t* crow, const uint32_t* y, double eps, double c, int solver,
                                                                  double* w_out, vpt_train_stats* stats) {
    __shared__ double lds[kTagLdsDoubles + kTagThreads + 16];
    const TagSolveDesc P = descs[blockIdx.x];
    const uint32_t n = P.nf + 1, l = P.l, t = threadIdx.x;
    if (7ull * n + 3ull * l > kTagLdsDoubles) return;   // the host sends such a problem down the other path
    TagProb Q;
    Q.rp = rp + P.rp; Q.cols = cols + P.cols; Q.cp = cp + P.cp; Q.crow = crow + P.cols; Q.y = y + P.y;
    Q.nf = P.nf; Q.l = l; Q.n = n; Q.c = c; Q.solver = solver;
    double* const w = lds;
    Q.v = TronVectors{w, w + n, w + 2 * n, w + 3 * n, w + 4 * n, w + 5 * n, w + 6 * n};
    Q.z = w + 7 * n; Q.D = Q.z + l; Q.tmp = Q.D + l; Q.red = lds + kTagLdsDoubles;
    const uint32_t n_solve = P.k == 2 ? 1 : P.k;
    for (uint32_t cls = 0; cls < n_solve; ++cls) {
        Q.cls = cls;
        double pc = 0;
        for (uint32_t i = t; i < l; i += kTagThreads) pc += Q.y[i] == cls ? 1.0 : 0.0;
        const vpt_train_stats st = tron(Q, tron_tolerance(eps, blk_sum(pc, Q.red), double(l)));
        for (uint32_t i = t; i < n; i += kTagThreads) {
            w_out[P.w + uint64_t(cls) * n + i] = w[i];
            if (P.k == 2) w_out[P.w + n + i] = -w[i];   // feature_coefficient(f, 1) = -feature_coefficient(f, 0)
        }
        if (t == 0) {
            stats[P.stats + cls] = st;
            if (P.k == 2) stats[P.stats + 1] = st;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------- surfaces and problem construction
// an example's record in the trainer's own arrays: (first char in the char pool, chars, first key, keys)
__global__ __launch_bounds__(kTagThreads) void tag_rec_finish_kernel(const uint32_t* recs, uint64_t n_ex, const uint64_t* ooff, const uint64_t* key_off,
                                                                       uint32_t cps_base, uint32_t key_base, uint32_t* out) {
    const uint64_t x = uint64_t(blockIdx.x) * kTagThreads + threadIdx.x;
    if (x >= n_ex) return;
    const uint32_t sent = recs[4 * x], start = recs[4 * x + 1], end = recs[4 * x + 2];
    const uint64_t c0 = ooff[sent] + sent;
    out[4 * x] = cps_base + uint32_t(c0 + start);
    out[4 * x + 1] = end - start;
    out[4 * x + 2] = key_base + uint32_t(key_off[c0 + end - 1]);
    out[4 * x + 3] = recs[4 * x + 3];
}
// every example finds (or becomes) the representative of its surface: open addressing by the hash of (code points, length), verified
// char by char
__global__ __launch_bounds__(kTagThreads) void surf_insert_kernel(const uint32_t* ex, uint64_t n_ex, const uint32_t* cps, uint64_t* table, uint64_t mask,
                                                                    uint32_t* rep, uint32_t* flag, uint32_t* maxlen) {
    const uint64_t i = uint64_t(blockIdx.x) * kTagThreads + threadIdx.x;
    if (i >= n_ex) return;
    const uint32_t* c = cps + ex[4 * i];
    const uint32_t len = ex[4 * i + 1];
    uint64_t h = kCpsHashSeed;
    for (uint32_t k = 0; k < len; ++k) h = cps_hash_step(h, c[k]);
    for (uint64_t s = cps_hash_finish(h, len) & mask;; s = (s + 1) & mask) {
        uint64_t e = table[s];
        if (e == 0) {
            e = atomic_cas_u64(table + s, 0, i + 1);
            if (e == 0) { rep[i] = uint32_t(i); flag[i] = 1; atomicMax(maxlen, len); return; }
        }
        const uint32_t* d = cps + ex[4 * (e - 1)];
        bool eq = ex[4 * (e - 1) + 1] == len;
        for (uint32_t k = 0; k < len && eq; ++k) eq = (d[k] & kCharMaskTrain) == (c[k] & kCharMaskTrain);
        if (eq) { rep[i] = uint32_t(e - 1); flag[i] = 0; return; }
    }
}
// the distinct surfaces as rows of maxlen decode_chars words, 0 past the end (so that a prefix sorts first)
__global__ __launch_bounds__(kTagThreads) void surf_matrix_kernel(const uint32_t* ex, uint64_t n_ex, const uint32_t* flag, const uint64_t* pos,
                                                                    const uint32_t* cps, uint32_t maxlen, uint32_t* mat, uint32_t* slot) {
    const uint64_t i = uint64_t(blockIdx.x) * kTagThreads + threadIdx.x;
    if (i >= n_ex || !flag[i]) return;
    const uint64_t d = pos[i];
    const uint32_t len = ex[4 * i + 1];
    for (uint32_t k = 0; k < maxlen; ++k) mat[d * maxlen + k] = k < len ? cps[ex[4 * i] + k] : 0u;
    slot[i] = uint32_t(d);
}
// a row's feature occurrences as (key, problem) records of five words
__global__ __launch_bounds__(kTagThreads) void tag_expand_kernel(const uint32_t* row_ex, const uint32_t* row_prob, uint64_t n_rows, const uint32_t* ex,
                                                                   const uint64_t* occ_off, const uint64_t* keys, uint32_t* nk_or_occ, uint32_t* occ_row) {
    const uint64_t r = uint64_t(blockIdx.x) * kTagThreads + threadIdx.x;
    if (r >= n_rows) return;
    const uint32_t x = row_ex[r];
    if (!occ_off) { nk_or_occ[r] = ex[4 * x + 3]; return; }   // the count pass
    const uint64_t k0 = ex[4 * x + 2];
    uint64_t o = occ_off[r];
    for (uint32_t q = 0; q < ex[4 * x + 3]; ++q, ++o) {
        const uint64_t lo = keys[2 * (k0 + q)], hi = keys[2 * (k0 + q) + 1];
        nk_or_occ[5 * o] = uint32_t(lo); nk_or_occ[5 * o + 1] = uint32_t(lo >> 32);
        nk_or_occ[5 * o + 2] = uint32_t(hi); nk_or_occ[5 * o + 3] = uint32_t(hi >> 32);
        nk_or_occ[5 * o + 4] = row_prob[r];
        occ_row[o] = uint32_t(r);
    }
}
// sorted by (problem, key): 1 where a record differs from the one in front of it
__global__ __launch_bounds__(kTagThreads) void tag_flag_kernel(const uint32_t* occ, const uint32_t* order, uint64_t n, uint32_t* flag) {
    const uint64_t i = uint64_t(blockIdx.x) * kTagThreads + threadIdx.x;
    if (i >= n) return;
    bool diff = i == 0;
    for (uint32_t k = 0; k < 5 && !diff; ++k) diff = occ[5 * uint64_t(order[i]) + k] != occ[5 * uint64_t(order[i - 1]) + k];
    flag[i] = diff ? 1u : 0u;
}
// per problem: where its occurrences and its distinct keys start (the sort keeps a problem's occurrences in its own range), the ends
// of its row and column pointers
__global__ __launch_bounds__(kTagThreads) void tag_prob_kernel(const uint64_t* prob_row_ptr, uint64_t n_prob, const uint64_t* occ_off, const uint64_t* dpos,
                                                                 uint64_t n_occ, uint64_t* prob_occ0, uint64_t* key_ptr) {
    const uint64_t p = uint64_t(blockIdx.x) * kTagThreads + threadIdx.x;
    if (p > n_prob) return;
    const uint64_t o = p < n_prob ? occ_off[prob_row_ptr[p]] : n_occ;
    prob_occ0[p] = o;
    key_ptr[p] = dpos[o];   // dpos[n_occ] = the distinct keys in all
}
// per sorted occurrence: its column inside its problem, the CSC row, and at a key's first occurrence the key and the column pointer
__global__ __launch_bounds__(kTagThreads) void tag_finalize_kernel(const uint32_t* occ, const uint32_t* order, const uint32_t* flag, const uint64_t* dpos,
                                                                     uint64_t n, const uint32_t* occ_row, const uint64_t* prob_row_ptr,
                                                                     const uint64_t* prob_occ0, const uint64_t* key_ptr, uint32_t* occ_col, uint64_t* dkeys,
                                                                     uint32_t* cp, uint32_t* crow) {
    const uint64_t i = uint64_t(blockIdx.x) * kTagThreads + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = order[i];
    const uint32_t p = occ[5 * o + 4];
    const uint64_t gcol = dpos[i] + flag[i] - 1, lcol = gcol - key_ptr[p];
    occ_col[o] = uint32_t(lcol);
    crow[i] = uint32_t(occ_row[o] - prob_row_ptr[p]);
    if (flag[i]) {
        dkeys[2 * gcol] = occ[5 * o] | (uint64_t(occ[5 * o + 1]) << 32);
        dkeys[2 * gcol + 1] = occ[5 * o + 2] | (uint64_t(occ[5 * o + 3]) << 32);
        cp[key_ptr[p] + p + lcol] = uint32_t(i - prob_occ0[p]);
    }
}
// per row: its columns sorted (a row is tens of them, all distinct) and its row pointer; per problem the last pointers
__global__ __launch_bounds__(kTagThreads) void tag_rows_kernel(const uint32_t* row_prob, uint64_t n_rows, const uint64_t* occ_off, const uint64_t* prob_row_ptr,
                                                                 const uint64_t* prob_occ0, const uint64_t* key_ptr, uint32_t* occ_col, uint32_t* rp, uint32_t* cp) {
    const uint64_t r = uint64_t(blockIdx.x) * kTagThreads + threadIdx.x;
    if (r >= n_rows) return;
    const uint64_t a = occ_off[r], e = occ_off[r + 1];
    for (uint64_t i = a + 1; i < e; ++i) {
        const uint32_t v = occ_col[i];
        uint64_t j = i;
        while (j > a && occ_col[j - 1] > v) { occ_col[j] = occ_col[j - 1]; --j; }
        occ_col[j] = v;
    }
    const uint32_t p = row_prob[r];
    rp[prob_row_ptr[p] + p + (r - prob_row_ptr[p])] = uint32_t(a - prob_occ0[p]);
    if (r + 1 == prob_row_ptr[p + 1]) {
        const uint32_t nz = uint32_t(prob_occ0[p + 1] - prob_occ0[p]);
        rp[prob_row_ptr[p + 1] + p] = nz;
        cp[key_ptr[p + 1] + p] = nz;
    }
}

}  // namespace

hipError_t train_tag_features(const TagFeatParams& P, bool emit, hipStream_t st) {
    if (emit) return launch1(tag_features_kernel<true>, P.total_chars, st, P);
    return launch1(tag_features_kernel<false>, P.total_chars, st, P);
}
hipError_t train_tag_validate(const uint32_t* n_tags, const uint64_t* ooff, uint64_t n_sent, uint64_t total_chars, const uint64_t* tag_index,
                              const uint64_t* span_off, uint64_t n_spans, uint64_t n_tag_bytes, uint32_t* status, hipStream_t st) {
    return launch1(tag_validate_kernel, total_chars > n_spans ? total_chars : n_spans, st, n_tags, ooff, n_sent, total_chars, tag_index, span_off,
                        n_spans, n_tag_bytes, status);
}
hipError_t train_tag_rec_finish(const uint32_t* recs, uint64_t n_ex, const uint64_t* ooff, const uint64_t* key_off, uint32_t cps_base, uint32_t key_base,
                                uint32_t* out, hipStream_t st) {
    return launch1(tag_rec_finish_kernel, n_ex, st, recs, n_ex, ooff, key_off, cps_base, key_base, out);
}
hipError_t train_surf_insert(const uint32_t* ex, uint64_t n_ex, const uint32_t* cps, uint64_t* table, uint64_t mask, uint32_t* rep, uint32_t* flag,
                             uint32_t* maxlen, hipStream_t st) {
    return launch1(surf_insert_kernel, n_ex, st, ex, n_ex, cps, table, mask, rep, flag, maxlen);
}
hipError_t train_surf_matrix(const uint32_t* ex, uint64_t n_ex, const uint32_t* flag, const uint64_t* pos, const uint32_t* cps, uint32_t maxlen,
                             uint32_t* mat, uint32_t* slot, hipStream_t st) {
    return launch1(surf_matrix_kernel, n_ex, st, ex, n_ex, flag, pos, cps, maxlen, mat, slot);
}
hipError_t train_tag_expand(const uint32_t* row_ex, const uint32_t* row_prob, uint64_t n_rows, const uint32_t* ex, const uint64_t* occ_off,
                            const uint64_t* keys, uint32_t* nk_or_occ, uint32_t* occ_row, hipStream_t st) {
    return launch1(tag_expand_kernel, n_rows, st, row_ex, row_prob, n_rows, ex, occ_off, keys, nk_or_occ, occ_row);
}
hipError_t train_tag_assemble(const TagBuildParams& B, hipStream_t st) {
    hipError_t e = launch1(tag_prob_kernel, B.n_prob + 1, st, B.prob_row_ptr, B.n_prob, B.occ_off, B.dpos, B.n_occ, B.prob_occ0, B.key_ptr);
    if (e == hipSuccess)
        e = launch1(tag_finalize_kernel, B.n_occ, st, B.occ, B.order, B.flag, B.dpos, B.n_occ, B.occ_row, B.prob_row_ptr, (const uint64_t*)B.prob_occ0,
                         (const uint64_t*)B.key_ptr, B.occ_col, B.dkeys, B.cp, B.crow);
    if (e == hipSuccess)
        e = launch1(tag_rows_kernel, B.n_rows, st, B.row_prob, B.n_rows, B.occ_off, B.prob_row_ptr, (const uint64_t*)B.prob_occ0,
                         (const uint64_t*)B.key_ptr, B.occ_col, B.rp, B.cp);
    return e;
}
hipError_t train_tag_flags(const uint32_t* occ, const uint32_t* order, uint64_t n, uint32_t* flag, hipStream_t st) {
    return launch1(tag_flag_kernel, n, st, occ, order, n, flag);
}
bool train_tag_fits(uint64_t rows, uint64_t features) { return 7 * (features + 1) + 3 * rows <= kTagLdsDoubles; }
hipError_t train_tag_solve(const TagSolveDesc* descs, uint32_t n_prob, const uint32_t* rp, const uint32_t* cols, const uint32_t* cp, const uint32_t* crow,
                           const uint32_t* y, double eps, double cost, int solver, double* w, vpt_train_stats* stats, hipStream_t st) {
    if (n_prob == 0) return hipSuccess;
    hipLaunchKernelGGL(tag_solve_kernel, dim3(n_prob), dim3(kTagThreads), 0, st, descs, rp, cols, cp, crow, y, eps, cost, solver, w, stats);
    return hipGetLastError();
}

}  // namespace vpt
