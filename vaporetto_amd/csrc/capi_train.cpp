// C ABI of libvaporetto_hip.so, boundary-model training: Trainer (vaporetto/src/trainer.rs) with the liblinear TRON solvers 0 and 2 and,
// on a trainer created with VPT_TRAIN_L1R, the coordinate descent of solver 5 by column groups (solve_l1r, l1r.h); with
// VPT_TRAIN_TAGS_L1R beside it solver 5 trains the tag models too (kernels_train_tags_l1.hip in LDS, solve_l1r for what does not fit).
// On a trainer created with VPT_TRAIN_L1R_LR solver 6 trains the boundary model by newGLMNET over the same groups (solve_l1r_lr, l1r_lr.h);
// with VPT_TRAIN_TAGS_L1R_LR beside it and VPT_TRAIN_TAGS solver 6 trains the tag models too (kernels_train_tags_l1lr.hip in LDS,
// solve_l1r_lr for what does not fit).
//
// The vpt_trainer handle keeps every example's feature keys and label on the device (kernels_train.hip); feature ids, the CSR and CSC
// copies of the design matrix are made when they are first needed after an add, and the TRON / CG loop runs here, on the host, over
// device vectors, reading back a scalar per reduction: `Tron` below is the host backend of tron.h, which holds the algorithm (the
// liblinear's that scikit-learn bundles, tron.cpp: CG without a preconditioner, eps_cg = 0.1).  The reference's newer liblinear
// preconditions its CG and reaches the same optimum by another path, so weights agree with it only to the stopping tolerance.
// Quantisation and the model layout are trainer.rs:352-487; the encoder mirrors vaporetto_amd/modelfmt.encode_model (model.rs:99-104).
#include "capi_internal.hpp"
#include "l1r.h"
#include "l1r_lr.h"
#include "tron.h"

#include <chrono>
#include <cmath>
#include <map>
#include <memory>
#include <set>
#include <unordered_map>

namespace {

template <typename T>
struct DBuf {   // a device array; contents are not kept across resize
    T* p = nullptr;
    uint64_t n = 0;
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    ~DBuf() { reset(); }
    void reset() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    hipError_t resize(uint64_t m) {
        reset();
        if (m == 0) m = 1;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), m * sizeof(T));
        if (e == hipSuccess) n = m; else p = nullptr;
        return e;
    }
    // grow to at least m elements keeping the first `keep`
    hipError_t grow(uint64_t m, uint64_t keep, hipStream_t st) {
        if (m <= n) return hipSuccess;
        uint64_t cap = std::max<uint64_t>(m, n + n / 2);
        T* q = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&q), cap * sizeof(T));
        if (e != hipSuccess) return e;
        if (keep) e = hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { (void)hipFree(q); return e; }
        if (p) (void)hipFree(p);
        p = q;
        n = cap;
        return hipSuccess;
    }
};

struct XtvLevel {
    const uint64_t* ptr;   // the level's column pointers (level 0: the CSC's)
    DBuf<uint64_t> nptr;   // the next level's
    DBuf<uint32_t> seg_col;
    DBuf<double> out;
    uint64_t nseg = 0;
};

struct Matrix {   // a design matrix on the device: CSR, CSC and the segments of Xᵀv (csc_levels); the bias column follows column nd - 1
    uint64_t nd = 0, nnz = 0;
    DBuf<uint64_t> csr_ptr, cptr;
    DBuf<uint32_t> cols, crow;
    DBuf<uint16_t> vals, cval;
    std::vector<std::unique_ptr<XtvLevel>> levels;
};

void put_utf8(std::string& s, uint32_t c) {
    if (c < 0x80) s += char(c);
    else if (c < 0x800) { s += char(0xC0 | (c >> 6)); s += char(0x80 | (c & 0x3F)); }
    else if (c < 0x10000) { s += char(0xE0 | (c >> 12)); s += char(0x80 | ((c >> 6) & 0x3F)); s += char(0x80 | (c & 0x3F)); }
    else { s += char(0xF0 | (c >> 18)); s += char(0x80 | ((c >> 12) & 0x3F)); s += char(0x80 | ((c >> 6) & 0x3F)); s += char(0x80 | (c & 0x3F)); }
}
// a symbol of an n-gram of the model: a char as UTF-8, a char type as its byte
void put_sym(std::string& s, uint32_t kind, uint32_t x) { if (kind == 0) put_utf8(s, x); else s += char(x); }

// bincode varint encoding of Model::to_vec (modelfmt._Writer)
struct Enc {
    std::vector<uint8_t> b;
    void u8(uint32_t v) { b.push_back(uint8_t(v)); }
    void uvar(uint64_t v) {
        if (v < 251) { u8(uint32_t(v)); return; }
        int n = v < (1ull << 16) ? 2 : v < (1ull << 32) ? 4 : 8;
        u8(n == 2 ? 0xFB : n == 4 ? 0xFC : 0xFD);
        for (int k = 0; k < n; ++k) u8(uint32_t(v >> (8 * k)) & 0xFF);
    }
    void i32(int32_t v) { uvar(uint32_t((uint32_t(v) << 1) ^ uint32_t(v >> 31))); }
    void raw(const std::string& s) { uvar(s.size()); b.insert(b.end(), s.begin(), s.end()); }
    void weights(const std::vector<int32_t>& w) { uvar(w.size()); for (int32_t x : w) i32(x); }
};

typedef unsigned __int128 u128;

// ---- tag-model training (tag_trainer.rs): what the host keeps of the examples, the problems made of them, and what was trained
struct TagSurface {   // a distinct surface, as build_tags reads it back: index = its id, in byte order
    std::string s;
    std::vector<uint32_t> cps;
    std::vector<uint8_t> types;
};
struct TagProblem {
    uint32_t model, slot, class_offset;
    std::vector<int32_t> cands;           // tag strings in id order
    std::vector<u128> keys;               // the features in key order
    std::vector<uint32_t> y;              // the tag id per row
    uint32_t index = 0;
    uint64_t nnz = 0;
    bool fetched = false;
    std::vector<uint32_t> rp, cols;       // the 0/1 CSR, read back from the device when asked for (fetch_rows)
    uint32_t path = 0;                    // 1 solved inside the kernel, 2 by the global-memory solver (TRON, or solver 5's group launches)
    double seconds_setup = 0, seconds_solve = 0;   // path 2: uploading the matrix and building its CSC; the solves of its classes
    std::vector<double> w;                // [classes][features + 1]
    std::vector<vpt_train_stats> stats;   // per class
};
struct TagModelOut {
    std::string token;
    const TagSurface* surf = nullptr;     // NULL: only the tag dictionary has the surface
    std::vector<std::vector<int32_t>> tags;
    uint32_t n_class = 0;
    std::vector<uint32_t> problems;
};

}  // namespace

struct vpt_trainer {
    int device = 0;
    hipStream_t st = nullptr;
    vpt_train_params prm{};
    std::vector<std::string> dict_words;
    std::vector<uint32_t> dict_len;   // chars per word
    DBuf<uint32_t> d_dict_slots, d_dict_cps, d_cinfo;
    DBuf<uint64_t> d_dict_off;
    uint64_t dict_mask = 0;
    uint32_t dict_maxlen = 0;
    // the examples
    DBuf<uint64_t> keys;      // two words per feature occurrence
    DBuf<uint32_t> row_cnt;   // occurrences per boundary
    DBuf<uint8_t> labels;
    uint64_t nnz_occ = 0, nrows = 0;
    DBuf<uint64_t> scratch;   // of the scans (scan_total, Sorter): grown on demand
    // the design matrix and its columns' keys (valid while `built`)
    bool built = false;
    Matrix m;
    DBuf<uint64_t> sorted_keys;
    // the last training
    std::vector<double> w;        // nd weights + the bias
    std::vector<uint8_t> model;
    vpt_train_stats stats{};
    bool trained = false;
    // tag models (VPT_TRAIN_TAGS)
    std::vector<std::string> tag_strings;
    std::unordered_map<std::string, int32_t> tag_ids;
    // the examples, on the device: the batches' chars, per example (first char, chars, first key, keys), and the keys
    DBuf<uint32_t> d_tag_cps, d_tag_ex;
    DBuf<uint64_t> d_tag_keys;
    uint64_t n_tag_cps = 0, n_tag_ex = 0, n_tag_keys = 0;
    // ... and on the host their tags alone: per example Token::tags().len(), and an interned tag string (-1 None) per slot
    std::vector<uint32_t> ex_ntags;
    std::vector<uint64_t> ex_tag0;
    std::vector<int32_t> ex_tags;
    // the last build: the surfaces by id, the problems' matrices on the device and where each problem's part starts
    std::vector<TagSurface> tag_surfaces;
    DBuf<uint32_t> b_rp, b_cols, b_cp, b_crow, b_y;
    std::vector<uint64_t> h_prob_row_ptr, h_prob_occ0, h_key_ptr;
    double tag_build_host_seconds = 0;
    std::map<std::string, std::vector<int32_t>> tag_defaults;
    bool tags_built = false, tags_trained = false;
    int tag_path_mode = 0;                                    // 0: by size; 1: every problem through the global-memory TRON
    std::vector<TagModelOut> tag_models;
    std::vector<TagProblem> tag_problems;
    vpt_tag_train_summary tag_summary{};
    double tag_build_seconds = 0, tag_add_host_seconds = 0;
    int32_t intern_tag(const std::string& s) {
        auto it = tag_ids.find(s);
        if (it != tag_ids.end()) return it->second;
        const int32_t id = int32_t(tag_strings.size());
        tag_strings.push_back(s);
        tag_ids.emplace(s, id);
        return id;
    }
    ~vpt_trainer() { if (st) (void)hipStreamDestroy(st); }
};

namespace {

vpt_status fail_arg(const std::string& msg) { return fail(VPT_INVALID_ARGUMENT, "InvalidArgumentError: " + msg); }

// the handle of a call that needs a trainer made with VPT_TRAIN_TAGS; args: the call's other pointers are there.  NULL: the error is set
vpt_trainer* tag_trainer(void* th, bool args) {
    vpt_trainer* t = static_cast<vpt_trainer*>(th);
    if (!t || !args) fail_arg("NULL argument");
    else if (!(t->prm.flags & VPT_TRAIN_TAGS)) fail_arg("tags: the trainer was created without VPT_TRAIN_TAGS");
    else return t;
    return nullptr;
}

// the exclusive scan of in[0 .. n) into out[0 .. n] on the trainer's stream; total: out[n] read back (NULL: not needed, nothing waits)
template <typename T>
vpt_status scan_total(vpt_trainer* t, const T* in, uint64_t n, uint64_t* out, uint64_t* total) {
    VPT_HIP(t->scratch.grow(vpt::train_scan_scratch(n) + 1, 0, t->st));
    VPT_HIP(vpt::train_scan(in, n, out, t->scratch.p, t->st));
    if (!total) return VPT_OK;
    VPT_HIP(hipMemcpyAsync(total, out + n, 8, hipMemcpyDeviceToHost, t->st));
    VPT_HIP(hipStreamSynchronize(t->st));
    return VPT_OK;
}

// slots of an open-addressing table for n items: a power of two, at most half full
uint64_t table_slots(uint64_t n) {
    uint64_t slots = 2;
    while (slots < 2 * n) slots <<= 1;
    return slots;
}

// the stable LSD radix sort of item indices: its buffers and its passes; `order` holds the result of run
struct Sorter {
    DBuf<uint32_t> order, tmp;
    DBuf<uint64_t> hist, hist_scan;
    std::vector<uint32_t> passes;   // u32 word of the item << 8 | bit shift, least significant digit first
    void bytes(uint32_t word, uint32_t n_bytes) {
        for (uint32_t k = 0; k < n_bytes; ++k) passes.push_back((word << 8) | (8 * k));
    }
    // as many bytes as the values below n need
    static uint32_t bytes_below(uint64_t n) {
        uint32_t b = 1;
        while (b < 4 && n > (uint64_t(1) << (8 * b))) ++b;
        return b;
    }
    vpt_status run(vpt_trainer* t, const uint32_t* base, uint32_t stride, uint64_t n) {
        const uint64_t nh = vpt::train_radix_scratch(n);
        VPT_HIP(order.resize(n)); VPT_HIP(tmp.resize(n)); VPT_HIP(hist.resize(nh)); VPT_HIP(hist_scan.resize(nh + 1));
        VPT_HIP(t->scratch.grow(vpt::train_scan_scratch(nh) + 1, 0, t->st));
        VPT_HIP(vpt::train_radix_sort(base, stride, passes.data(), uint32_t(passes.size()), n, order.p, tmp.p, hist.p, hist_scan.p, t->scratch.p, t->st));
        return VPT_OK;
    }
};

// M's CSC copy of its CSR's nonzeros (stably sorted by column: rows ascend within a column) and the segments of Xᵀv, level by level,
// until a column is one segment; rows: the row of every nonzero
vpt_status csc_levels(vpt_trainer* t, Matrix& M, const uint32_t* rows, uint64_t nz, uint64_t nd) {
    hipStream_t st = t->st;
    M.levels.clear();
    M.nd = nd;
    M.nnz = nz;
    Sorter S;
    S.bytes(0, Sorter::bytes_below(nd));
    VPT_TRY(S.run(t, M.cols.p, 1, nz));
    VPT_HIP(M.crow.resize(nz)); VPT_HIP(M.cval.resize(nz)); VPT_HIP(M.cptr.resize(nd + 1));
    VPT_HIP(vpt::train_csc_fill(S.order.p, M.cols.p, M.vals.p, rows, nz, M.crow.p, M.cval.p, M.cptr.p, st));
    VPT_HIP(hipMemcpyAsync(M.cptr.p + nd, &nz, 8, hipMemcpyHostToDevice, st));
    VPT_HIP(hipStreamSynchronize(st));   // nz is a local
    DBuf<uint64_t> cnt;
    VPT_HIP(cnt.resize(nd));
    const uint64_t* ptr = M.cptr.p;
    for (;;) {
        M.levels.emplace_back(new XtvLevel());
        XtvLevel& L = *M.levels.back();
        L.ptr = ptr;
        VPT_HIP(L.nptr.resize(nd + 1));
        VPT_HIP(vpt::train_seg_count(ptr, nd, cnt.p, st));
        VPT_TRY(scan_total(t, cnt.p, nd, L.nptr.p, &L.nseg));
        VPT_HIP(L.seg_col.resize(L.nseg)); VPT_HIP(L.out.resize(L.nseg));
        VPT_HIP(vpt::train_seg_col(L.nptr.p, nd, L.seg_col.p, st));
        ptr = L.nptr.p;
        if (L.nseg == nd) break;
    }
    VPT_HIP(hipStreamSynchronize(st));
    return VPT_OK;
}

vpt_status build(vpt_trainer* t) {
    if (t->built) return VPT_OK;
    hipStream_t st = t->st;
    Matrix& M = t->m;
    const uint64_t nnz = t->nnz_occ, nrows = t->nrows;
    if (nnz >= (uint64_t(1) << 32) || nrows >= (uint64_t(1) << 32))
        return fail_arg("examples: at most 2^32 - 1 boundaries and feature occurrences");
    // ---- representatives of the distinct keys
    const uint64_t slots = table_slots(nnz);
    DBuf<uint64_t> table, pos;
    DBuf<uint32_t> rep, slot, flag;
    VPT_HIP(table.resize(slots));
    VPT_HIP(hipMemsetAsync(table.p, 0, slots * 8, st));
    VPT_HIP(rep.resize(nnz)); VPT_HIP(flag.resize(nnz)); VPT_HIP(pos.resize(nnz + 1)); VPT_HIP(slot.resize(nnz));
    VPT_HIP(vpt::train_insert(t->keys.p, nnz, table.p, slots - 1, rep.p, flag.p, st));
    uint64_t nd = 0;
    VPT_TRY(scan_total(t, flag.p, nnz, pos.p, &nd));
    table.reset(); flag.reset();
    DBuf<uint64_t> dkeys;
    VPT_HIP(dkeys.resize(2 * nd));
    VPT_HIP(vpt::train_compact(t->keys.p, rep.p, pos.p, nnz, dkeys.p, slot.p, st));
    // ---- the distinct keys sorted: 16 passes of 8 bits over the four 32-bit words, least significant first
    DBuf<uint32_t> ids;
    {
        Sorter S;
        DBuf<uint32_t> col_of;
        for (uint32_t w = 0; w < 4; ++w) S.bytes(w, 4);
        VPT_TRY(S.run(t, reinterpret_cast<const uint32_t*>(dkeys.p), 4, nd));
        VPT_HIP(col_of.resize(nd)); VPT_HIP(ids.resize(nnz)); VPT_HIP(t->sorted_keys.resize(2 * nd));
        VPT_HIP(vpt::train_ids(S.order.p, nd, col_of.p, rep.p, slot.p, nnz, ids.p, st));
        VPT_HIP(vpt::train_sorted_keys(dkeys.p, S.order.p, nd, t->sorted_keys.p, st));
        VPT_HIP(hipStreamSynchronize(st));
    }
    rep.reset(); slot.reset(); dkeys.reset();
    // ---- CSR: rows in corpus order, ids sorted, duplicates merged into counts
    DBuf<uint64_t> row_off;
    DBuf<uint32_t> merged, rows, status;
    VPT_HIP(row_off.resize(nrows + 1)); VPT_HIP(merged.resize(nrows)); VPT_HIP(M.csr_ptr.resize(nrows + 1));
    VPT_TRY(scan_total(t, t->row_cnt.p, nrows, row_off.p, nullptr));
    VPT_HIP(vpt::train_row_sort(ids.p, row_off.p, nrows, merged.p, st));
    uint64_t nz = 0;
    VPT_TRY(scan_total(t, merged.p, nrows, M.csr_ptr.p, &nz));
    VPT_HIP(status.resize(1));
    VPT_HIP(hipMemsetAsync(status.p, 0, 4, st));
    VPT_HIP(M.cols.resize(nz)); VPT_HIP(M.vals.resize(nz)); VPT_HIP(rows.resize(nz));
    VPT_HIP(vpt::train_row_merge(ids.p, row_off.p, M.csr_ptr.p, nrows, M.cols.p, M.vals.p, rows.p, status.p, st));
    uint32_t bad = 0;
    VPT_HIP(hipMemcpyAsync(&bad, status.p, 4, hipMemcpyDeviceToHost, st));
    VPT_HIP(hipStreamSynchronize(st));
    if (bad) return fail_arg("examples: a feature occurs more than 65535 times at one boundary");
    ids.reset(); row_off.reset(); merged.reset();
    VPT_TRY(csc_levels(t, M, rows.p, nz, nd));
    t->built = true;
    return VPT_OK;
}

// the host backend of tron.h: a step is a launch over device vectors, a dot product is read back
struct Tron {
    const Matrix* m;
    hipStream_t st;
    uint64_t n, nr;
    int solver;
    double c;
    DBuf<double> w, w_new, g, s, r, d, Hd, y, z, zt, gz, D, loss, part0, part1;
    vpt::TronVectors v;
    hipError_t err = hipSuccess;

    // for `rows` examples over M's columns and the bias
    vpt_status init(const Matrix& M, hipStream_t stream, uint64_t rows, int solver_, double cost) {
        m = &M; st = stream; n = M.nd + 1; nr = rows; solver = solver_; c = cost;
        for (DBuf<double>* b : {&w, &w_new, &g, &s, &r, &d, &Hd}) VPT_HIP(b->resize(n));
        for (DBuf<double>* b : {&y, &z, &zt, &gz, &D, &loss}) VPT_HIP(b->resize(nr));
        for (DBuf<double>* b : {&part0, &part1}) VPT_HIP(b->resize(vpt::train_dot_partials(std::max(n, nr))));
        v = vpt::TronVectors{w.p, w_new.p, g.p, s.p, r.p, d.p, Hd.p};
        return VPT_OK;
    }
    // one training from w = 0: the targets (+1 / -1, `pos` of them +1) go up, the weights come back into w_out[0 .. n)
    vpt_status solve(const std::vector<double>& targets, uint64_t pos, double eps, vpt_train_stats* stats, double* w_out) {
        VPT_HIP(hipMemcpy(y.p, targets.data(), nr * 8, hipMemcpyHostToDevice));
        *stats = vpt::tron(*this, vpt::tron_tolerance(eps, double(pos), double(nr)));
        VPT_HIP(err);
        VPT_HIP(hipMemcpy(w_out, w.p, n * 8, hipMemcpyDeviceToHost));
        return VPT_OK;
    }

    // the fixed-shape sum of a[i] * b[i] (b NULL: a[i]), left on the device; returns where
    const double* reduce_dev(const double* a, const double* b, uint64_t len) {
        double* in_out[2] = {part0.p, part1.p};
        uint64_t m = vpt::train_dot_partials(len);
        if (ok()) err = vpt::train_dot(a, b, len, in_out[0], st);
        int k = 0;
        while (m > 1 && ok()) {
            err = vpt::train_dot(in_out[k], nullptr, m, in_out[k ^ 1], st);
            m = vpt::train_dot_partials(m);
            k ^= 1;
        }
        return in_out[k];
    }
    double dot(const double* a, const double* b, uint64_t len) {
        if (len == 0) return 0;
        const double* r_ = reduce_dev(a, b, len);
        double v_ = 0;
        if (ok()) err = hipMemcpyAsync(&v_, r_, 8, hipMemcpyDeviceToHost, st);
        if (ok()) err = hipStreamSynchronize(st);
        return v_;
    }
    double dot(const double* a, const double* b) { return dot(a, b, n); }
    void zero(double* x) { if (ok()) err = hipMemsetAsync(x, 0, n * 8, st); }
    void copy(const double* x, double* out) { if (ok()) err = hipMemcpyAsync(out, x, n * 8, hipMemcpyDeviceToDevice, st); }
    void axpy(double a, const double* x, double* y_) { if (ok()) err = vpt::train_axpy(n, a, x, y_, st); }
    void xpby(const double* x, double b, double* y_) { if (ok()) err = vpt::train_xpby(n, x, b, y_, st); }
    void add(const double* a, const double* b, double* out) { copy(a, out); axpy(1.0, b, out); }
    void cg_start() { zero(v.s); zero(v.r); axpy(-1.0, v.g, v.r); copy(v.r, v.d); }
    void cg_boundary(double a) { axpy(a, v.d, v.s); axpy(-a, v.Hd, v.r); }
    bool ok() const { return err == hipSuccess; }   // a launch failed: every later step is skipped and the loops end
    bool cg_more(int) const { return ok(); }
    // out = a + Xᵀu
    void add_xtv(const double* a, const double* u, double* out) {
        const double* in = nullptr;
        for (auto& Lp : m->levels) {
            XtvLevel& L = *Lp;
            if (ok())
                err = vpt::train_xtv_level(L.ptr, L.nptr.p, L.seg_col.p, L.nseg, in, in ? nullptr : m->crow.p, m->cval.p, u, L.out.p, st);
            in = L.out.p;
        }
        const double* bias = reduce_dev(u, nullptr, nr);
        if (ok()) err = vpt::train_add(n, a, in, bias, out, st);
    }
    double fun(const double* x) {
        if (ok()) err = vpt::train_xv(m->csr_ptr.p, m->cols.p, m->vals.p, nr, x, m->nd, z.p, st);
        if (ok()) err = vpt::train_loss(nr, z.p, y.p, c, solver, loss.p, st);
        const double reg = dot(x, x) / 2.0;
        return reg + dot(loss.p, nullptr, nr);
    }
    void grad(const double* x, double* out) {
        if (ok()) err = vpt::train_grad_rows(nr, z.p, y.p, c, solver, gz.p, D.p, st);
        add_xtv(x, gz.p, out);
    }
    void hv(const double* x, double* out) {
        if (ok()) err = vpt::train_xv(m->csr_ptr.p, m->cols.p, m->vals.p, nr, x, m->nd, zt.p, st);
        if (ok()) err = vpt::train_scale_rows(nr, D.p, zt.p, st);
        add_xtv(x, zt.p, out);
    }
};

// ---------------------------------------------------------------------------------------------------- solver 5 (l1r.h)
// The column groups of a sweep: the char and type columns by template (kind, n-gram length, rel_position) in that order -- a boundary
// has exactly one n-gram of a template, with count 1, so the columns of a template share no row --, then every dictionary column and
// the bias (column nd) alone: those can share rows.  A group's columns stand by length class, as train_l1r_group takes them.
struct L1rGroups {
    std::vector<uint32_t> cols;
    std::vector<uint64_t> ptr{0};
    std::vector<uint32_t> n_lane, n_wave;
    size_t size() const { return n_lane.size(); }
};
template <typename Ptr>
L1rGroups l1r_groups(const std::vector<uint64_t>& keys, const Ptr* cptr, uint64_t nd) {
    std::map<uint32_t, std::vector<uint32_t>> tpl;
    std::vector<uint32_t> alone;
    for (uint64_t j = 0; j < nd; ++j) {
        const vpt::TrainKey k = vpt::train_key(keys[2 * j], keys[2 * j + 1]);
        if (k.kind == 2) alone.push_back(uint32_t(j));
        else tpl[(k.kind << 16) | (k.len << 8) | uint32_t(k.rel + 16)].push_back(uint32_t(j));
    }
    alone.push_back(uint32_t(nd));
    L1rGroups G;
    auto push = [&](const std::vector<uint32_t>& g) {
        auto len = [&](uint32_t j) { return j == nd ? ~uint64_t(0) : uint64_t(cptr[j + 1] - cptr[j]); };
        uint32_t cnt[2] = {0, 0};
        for (int cls = 0; cls < 3; ++cls)
            for (uint32_t j : g) {
                const uint64_t n = len(j);
                if ((n <= vpt::kL1rLaneMax ? 0 : n <= vpt::kL1rWaveMax ? 1 : 2) != cls) continue;
                G.cols.push_back(j);
                if (cls < 2) ++cnt[cls];
            }
        G.ptr.push_back(G.cols.size());
        G.n_lane.push_back(cnt[0]);
        G.n_wave.push_back(cnt[1]);
    };
    for (auto& kv : tpl) push(kv.second);
    for (uint32_t j : alone) push({j});
    return G;
}

// what the launches of a group (and the in-kernel solver's groups) rest on: no row twice in a group.  Checked by the emulated build and
// by -DVPT_DEBUG once per matrix; crow, cptr: the CSC on the host
template <typename Ptr>
vpt_status l1r_check_groups(const L1rGroups& G, const uint32_t* crow, const Ptr* cptr, uint64_t nr, uint64_t nd) {
#if defined(VPT_HIPEMU) || defined(VPT_DEBUG)
    std::vector<uint32_t> seen(nr, ~uint32_t(0));
    for (size_t g = 0; g < G.size(); ++g)
        for (uint64_t q = G.ptr[g]; q < G.ptr[g + 1]; ++q) {
            const uint32_t j = G.cols[q];
            if (j == nd) continue;   // the bias is alone
            for (uint64_t k = cptr[j]; k < cptr[j + 1]; ++k) {
                if (seen[crow[k]] == uint32_t(g)) return fail(VPT_RUNTIME_ERROR, "solver 5: a row occurs twice in a column group");
                seen[crow[k]] = uint32_t(g);
            }
        }
#endif
    return VPT_OK;
}
// the groups of M's columns, whose keys are `keys`, checked as above
vpt_status l1r_matrix_groups(const Matrix& M, uint64_t nr, const std::vector<uint64_t>& keys, L1rGroups& G) {
    const uint64_t nd = M.nd;
    std::vector<uint64_t> cptr(nd + 1);
    VPT_HIP(hipMemcpy(cptr.data(), M.cptr.p, (nd + 1) * 8, hipMemcpyDeviceToHost));
    G = l1r_groups(keys, cptr.data(), nd);
#if defined(VPT_HIPEMU) || defined(VPT_DEBUG)
    std::vector<uint32_t> crow(M.nnz);
    if (M.nnz) VPT_HIP(hipMemcpy(crow.data(), M.crow.p, M.nnz * 4, hipMemcpyDeviceToHost));
    VPT_TRY(l1r_check_groups(G, crow.data(), cptr.data(), nr, nd));
#endif
    return VPT_OK;
}

// solve_l1r_l2_svc from w = 0 by groups over the matrix M of nr rows with the targets y (`pos` of them +1): a launch per group, the
// groups G permuted anew per sweep (l1r.h), the columns' violations summed in a fixed order and read back once per sweep: the only
// readback of a sweep.  The boundary model and a class of a tag problem that does not fit its kernel are solved here.  Out come the
// weights and the stats: sweeps, halvings, the first and last sweep's violation sums, and |w|_1 + C sum max(0, b)^2 with b recomputed
// from w.
vpt_status solve_l1r(vpt_trainer* t, const Matrix& M, uint64_t nr, const std::vector<double>& y, uint64_t pos, const L1rGroups& G, double eps, double cost,
                     double* w_out, vpt_train_stats* stats) {
    hipStream_t st = t->st;
    const uint64_t nd = M.nd, n = nd + 1;
    Tron T;   // its vectors and its reductions: w, y, b (in gz), xj_sq (in s), the violations (in g)
    VPT_TRY(T.init(M, st, nr, 2, cost));
    DBuf<uint32_t> d_cols, d_halv;
    DBuf<vpt::L1rPair> tile0, tile1;
    VPT_HIP(d_cols.resize(G.cols.size())); VPT_HIP(d_halv.resize(1));
    VPT_HIP(tile0.resize(vpt::train_l1r_scratch(M.nnz, nr, nd, 0))); VPT_HIP(tile1.resize(vpt::train_l1r_scratch(M.nnz, nr, nd, 1)));
    const std::vector<double> ones(nr, 1.0);
    VPT_HIP(hipMemcpy(T.y.p, y.data(), nr * 8, hipMemcpyHostToDevice));
    VPT_HIP(hipMemcpy(T.gz.p, ones.data(), nr * 8, hipMemcpyHostToDevice));
    VPT_HIP(hipMemcpy(d_cols.p, G.cols.data(), G.cols.size() * 4, hipMemcpyHostToDevice));
    VPT_HIP(hipMemsetAsync(T.w.p, 0, n * 8, st));
    VPT_HIP(hipMemsetAsync(d_halv.p, 0, 4, st));
    vpt::L1rParams P{};
    P.cptr = M.cptr.p; P.crow = M.crow.p; P.cval = M.cval.p; P.nd = nd; P.nr = nr; P.nnz = M.nnz;
    P.y = T.y.p; P.b = T.gz.p; P.w = T.w.p; P.xj_sq = T.s.p; P.viol = T.g.p; P.halvings = d_halv.p; P.tile0 = tile0.p; P.tile1 = tile1.p; P.c = cost;
    auto launch = [&](size_t g, bool init) {
        const uint32_t total = uint32_t(G.ptr[g + 1] - G.ptr[g]);
        return vpt::train_l1r_group(P, init, d_cols.p + G.ptr[g], G.n_lane[g], G.n_wave[g], total - G.n_lane[g] - G.n_wave[g], st);
    };
    for (size_t g = 0; g < G.size(); ++g) VPT_HIP(launch(g, true));
    const double tol = vpt::tron_tolerance(eps, double(pos), double(nr));
    std::vector<uint32_t> order(G.size());
    for (size_t g = 0; g < G.size(); ++g) order[g] = uint32_t(g);
    uint64_t rng = vpt::kL1rSeed;
    double v0 = 0, v = 0;
    uint32_t sweeps = 0;
    while (sweeps < uint32_t(vpt::kL1rMaxSweeps)) {
        vpt::l1r_shuffle(order.data(), uint32_t(order.size()), &rng);
        for (uint32_t g : order) VPT_HIP(launch(g, false));
        v = T.dot(T.g.p, nullptr, n);
        VPT_HIP(T.err);
        if (sweeps++ == 0) v0 = v;
        if (v <= tol * v0) break;
    }
    uint32_t halvings = 0;
    VPT_HIP(hipMemcpyAsync(&halvings, d_halv.p, 4, hipMemcpyDeviceToHost, st));
    VPT_HIP(hipMemcpyAsync(w_out, T.w.p, n * 8, hipMemcpyDeviceToHost, st));
    // the loss at the weights themselves, not at the b the sweeps carried along
    VPT_HIP(vpt::train_xv(M.csr_ptr.p, M.cols.p, M.vals.p, nr, T.w.p, nd, T.z.p, st));
    VPT_HIP(vpt::train_loss(nr, T.z.p, T.y.p, cost, 2, T.loss.p, st));
    const double loss = T.dot(T.loss.p, nullptr, nr);
    VPT_HIP(T.err);
    double norm1 = 0;
    for (uint64_t j = 0; j < n; ++j) norm1 += std::fabs(w_out[j]);
    *stats = vpt_train_stats{sweeps, halvings, v0, v, norm1 + loss};
    return VPT_OK;
}

// ---------------------------------------------------------------------------------------------------- solver 6 (l1r_lr.h)
// The host backend of l1r_lr.h: a step is a launch, a sum is Tron's fixed-shape reduction read back.  Every vector is one of Tron's:
// per feature w, wpd (w_new), Grad (g), Hdiag (s), xjneg_sum (r), the violations (d) and the terms of a sum (Hd); per row y, e (z),
// tau (zt), D, xTd (gz) and the terms of a sum (loss).
struct L1lr {
    Tron T;
    const L1rGroups* G;
    vpt::L1lrParams P{};
    DBuf<uint32_t> d_cols, d_all;   // the groups' columns; every column by length class, for the launch over all of them
    DBuf<vpt::L1rPair> tile0, tile1;
    DBuf<double> pack;              // three sums, read back in one copy
    uint32_t all_lane = 0, all_wave = 0, all_block = 0;
    hipStream_t st;
    uint64_t n;

    vpt_status init(vpt_trainer* t, const Matrix& M, uint64_t nr, const std::vector<double>& y, const L1rGroups& G_, double cost) {
        st = t->st; G = &G_; n = M.nd + 1;
        VPT_TRY(T.init(M, st, nr, 0, cost));
        std::vector<uint32_t> all;
        for (int cls = 0; cls < 3; ++cls)
            for (size_t g = 0; g < G_.size(); ++g) {
                const uint64_t a = G_.ptr[g], lane = a + G_.n_lane[g], wave = lane + G_.n_wave[g];
                const uint64_t lo = cls == 0 ? a : cls == 1 ? lane : wave, hi = cls == 0 ? lane : cls == 1 ? wave : G_.ptr[g + 1];
                all.insert(all.end(), G_.cols.begin() + lo, G_.cols.begin() + hi);
                (cls == 0 ? all_lane : cls == 1 ? all_wave : all_block) += uint32_t(hi - lo);
            }
        VPT_HIP(d_cols.resize(G_.cols.size())); VPT_HIP(d_all.resize(all.size())); VPT_HIP(pack.resize(3));
        VPT_HIP(tile0.resize(vpt::train_l1r_scratch(M.nnz, nr, M.nd, 0))); VPT_HIP(tile1.resize(vpt::train_l1r_scratch(M.nnz, nr, M.nd, 1)));
        VPT_HIP(hipMemcpy(T.y.p, y.data(), nr * 8, hipMemcpyHostToDevice));
        VPT_HIP(hipMemcpy(d_cols.p, G_.cols.data(), G_.cols.size() * 4, hipMemcpyHostToDevice));
        VPT_HIP(hipMemcpy(d_all.p, all.data(), all.size() * 4, hipMemcpyHostToDevice));
        P.cptr = M.cptr.p; P.crow = M.crow.p; P.cval = M.cval.p; P.nd = M.nd; P.nr = nr; P.nnz = M.nnz;
        P.y = T.y.p; P.e = T.z.p; P.tau = T.zt.p; P.D = T.D.p; P.xTd = T.gz.p;
        P.w = T.w.p; P.wpd = T.w_new.p; P.grad = T.g.p; P.hdiag = T.s.p; P.xjneg = T.r.p; P.viol = T.d.p;
        P.tile0 = tile0.p; P.tile1 = tile1.p; P.c = cost;
        return VPT_OK;
    }
    bool ok() const { return T.ok(); }
    void run(hipError_t e) { if (ok()) T.err = e; }
    void setup() {
        T.zero(P.w); T.zero(P.wpd);
        if (ok()) run(vpt::train_l1lr_start(P, true, st));
        if (ok()) run(vpt::train_l1lr_accept(P, st));   // xTd = 0: e stays 1
        if (ok()) run(vpt::train_l1lr_grad(P, true, d_all.p, all_lane, all_wave, all_block, st));
    }
    double grad() {
        if (ok()) run(vpt::train_l1lr_grad(P, false, d_all.p, all_lane, all_wave, all_block, st));
        return T.dot(P.viol, nullptr, n);
    }
    void qp_start() { if (ok()) run(vpt::train_l1lr_start(P, false, st)); }
    void cd_group(uint32_t g) {
        const uint32_t total = uint32_t(G->ptr[g + 1] - G->ptr[g]);
        if (ok()) run(vpt::train_l1lr_cd_group(P, d_cols.p + G->ptr[g], G->n_lane[g], G->n_wave[g], total - G->n_lane[g] - G->n_wave[g], st));
    }
    double qp_violation() { return T.dot(P.viol, nullptr, n); }
    void keep(const double* sum, int k) { if (ok()) run(hipMemcpyAsync(pack.p + k, sum, 8, hipMemcpyDeviceToDevice, st)); }
    vpt::L1lrSums direction_sums() {
        if (ok()) run(vpt::train_l1lr_feat_terms(P, T.Hd.p, P.viol, st));
        keep(T.reduce_dev(T.Hd.p, nullptr, n), 0);
        keep(T.reduce_dev(P.viol, nullptr, n), 1);
        if (ok()) run(vpt::train_l1lr_neg_terms(P, T.loss.p, st));
        keep(T.reduce_dev(T.loss.p, nullptr, P.nr), 2);
        double s[3] = {0, 0, 0};
        if (ok()) run(hipMemcpyAsync(s, pack.p, sizeof s, hipMemcpyDeviceToHost, st));
        if (ok()) run(hipStreamSynchronize(st));
        return {s[0], s[1], s[2]};
    }
    double linesearch_loss() {
        if (ok()) run(vpt::train_l1lr_ls_terms(P, T.loss.p, st));
        return T.dot(T.loss.p, nullptr, P.nr);
    }
    void accept() {
        T.copy(P.wpd, P.w);
        if (ok()) run(vpt::train_l1lr_accept(P, st));
    }
    double halve() {
        if (ok()) run(vpt::train_l1lr_halve(P, st));
        if (ok()) run(vpt::train_l1lr_feat_terms(P, nullptr, P.viol, st));
        return T.dot(P.viol, nullptr, n);
    }
    void recompute() {
        if (ok()) run(vpt::train_xv(T.m->csr_ptr.p, T.m->cols.p, T.m->vals.p, P.nr, P.w, P.nd, P.e, st));
        if (ok()) run(vpt::train_l1lr_exp(P.nr, P.e, st));
        T.copy(P.w, P.wpd);
    }
};

// solve_l1r_lr from w = 0 over the matrix M of nr rows with the targets y (`pos` of them +1) and the groups G, as solve_l1r takes them.
// Readbacks: one per inner sweep, one per line-search trial, and per Newton iteration the violations' sum and the three sums of the
// direction in one copy.  Out come the weights and the stats: Newton iterations, inner sweeps, the first and last violation sums at w,
// and |w|_1 + C sum log(1 + exp(-y w.x)) recomputed from w by solver 0's loss.
vpt_status solve_l1r_lr(vpt_trainer* t, const Matrix& M, uint64_t nr, const std::vector<double>& y, uint64_t pos, const L1rGroups& G, double eps, double cost,
                        double* w_out, vpt_train_stats* stats) {
    L1lr S;
    VPT_TRY(S.init(t, M, nr, y, G, cost));
    std::vector<uint32_t> order(G.size());
    for (size_t g = 0; g < G.size(); ++g) order[g] = uint32_t(g);
    const vpt::L1lrResult r = vpt::l1r_lr(S, vpt::tron_tolerance(eps, double(pos), double(nr)), order.data(), uint32_t(order.size()));
    VPT_HIP(S.T.err);
    Tron& T = S.T;
    VPT_HIP(hipMemcpyAsync(w_out, T.w.p, S.n * 8, hipMemcpyDeviceToHost, t->st));
    // the loss at the weights themselves, not at the e the iterations carried along
    VPT_HIP(vpt::train_xv(M.csr_ptr.p, M.cols.p, M.vals.p, nr, T.w.p, M.nd, T.z.p, t->st));
    VPT_HIP(vpt::train_loss(nr, T.z.p, T.y.p, cost, 0, T.loss.p, t->st));
    const double loss = T.dot(T.loss.p, nullptr, nr);
    VPT_HIP(T.err);
    double norm1 = 0;
    for (uint64_t j = 0; j < S.n; ++j) norm1 += std::fabs(w_out[j]);
    *stats = vpt_train_stats{r.newton, r.sweeps, r.gnorm0, r.gnorm, norm1 + loss};
    return VPT_OK;
}

void encode_tag_models(vpt_trainer* t, Enc& e);

// trainer.rs:352-487: quantisation and the model's layout, then Model::to_vec
vpt_status make_model(vpt_trainer* t, const std::vector<uint64_t>& keys) {
    const uint64_t nd = t->m.nd;
    const double bias = t->w[nd];
    double wmax = std::fabs(bias);
    for (uint64_t j = 0; j < nd; ++j) wmax = std::max(wmax, std::fabs(t->w[j]));
    const double m = wmax / double((1 << 15) - 1);
    if (m == 0.) return fail(VPT_INVALID_MODEL, "InvalidModelError: all weights are zero");
    const int32_t qbias = int32_t(bias / m);   // to_int_unchecked: truncation toward zero
    const int charw = int(t->prm.charw);
    std::map<std::string, std::vector<int32_t>> cw, tw;
    std::vector<int32_t> dw(3 * size_t(t->prm.dictn), 0);
    for (uint64_t j = 0; j < nd; ++j) {
        const int32_t q = int32_t(t->w[j] / m);
        if (q == 0) continue;
        const vpt::TrainKey k = vpt::train_key(keys[2 * j], keys[2 * j + 1]);
        if (k.kind == 2) {   // c: the class, then Left / Inside / Right
            dw[3 * (k.c[0] - 1) + k.c[1]] = q;
            continue;
        }
        const int len = int(k.len);
        std::string ng;
        for (int i = 0; i < len; ++i) put_sym(ng, k.kind, k.c[i]);
        // the type n-grams use the char window too (trainer.rs:433-440)
        const int posn = charw - len - k.rel;
        auto& mp = k.kind == 0 ? cw : tw;
        auto it = mp.find(ng);
        if (it == mp.end()) it = mp.emplace(ng, std::vector<int32_t>(size_t(2 * charw - len + 1), 0)).first;
        it->second[size_t(posn)] = q;
    }
    Enc e;
    static const char kMagic[] = "VaporettoTokenizer 0.5.0\n";
    e.b.assign(kMagic, kMagic + sizeof(kMagic) - 1);
    for (auto* mp : {&cw, &tw}) {
        e.uvar(mp->size());
        for (auto& kv : *mp) { e.raw(kv.first); e.weights(kv.second); }
    }
    e.uvar(t->dict_words.size());
    for (size_t i = 0; i < t->dict_words.size(); ++i) {
        const uint32_t len = t->dict_len[i];
        const uint32_t idx = std::min(len, t->prm.dictn) - 1;
        std::vector<int32_t> ws(len + 1, dw[3 * idx + 1]);
        ws.front() = dw[3 * idx];
        ws.back() = dw[3 * idx + 2];
        e.raw(t->dict_words[i]);
        e.weights(ws);
        e.uvar(0);   // comment ""
    }
    e.i32(qbias);
    e.u8(t->prm.charw);
    e.u8(t->prm.typew);
    if (t->prm.flags & VPT_TRAIN_TAGS) encode_tag_models(t, e);
    else e.uvar(0);   // no tag models
    t->model = std::move(e.b);
    return VPT_OK;
}

// A device caller's totals, once its stream has been synchronised and before a kernel follows an offset: the features' kernels index
// the boundaries from 0 and run a thread for each of total_b, so both ends of out_offsets are held to exactly that.
vpt_status check_totals(const uint64_t* d_ooff, size_t n, uint64_t total_b) {
    uint64_t first = 0, last = 0;
    VPT_HIP(hipMemcpy(&first, d_ooff, 8, hipMemcpyDeviceToHost));
    VPT_HIP(hipMemcpy(&last, d_ooff + n, 8, hipMemcpyDeviceToHost));
    if (first != 0) return fail_arg("out_offsets: must start at 0");
    if (last != total_b) return fail_arg("total_boundaries: must equal out_offsets[n_sentences]");
    return VPT_OK;
}

// `checked`: the caller has looked at the totals and the labels already (stage_batch on the host, add_tagged_device on the device)
vpt_status add_device(vpt_trainer* t, const uint8_t* d_utf8, const uint64_t* d_boff, const uint64_t* d_ooff, size_t n, uint64_t total_b,
                      const uint8_t* d_labels, unsigned flags, hipStream_t st, bool checked) {
    if ((flags & ~unsigned(VPT_FLAG_KYTEA_FULLWIDTH)) != 0) return fail_arg("flags: only VPT_FLAG_KYTEA_FULLWIDTH");
    if (n == 0) return VPT_OK;
    VPT_HIP(hipSetDevice(t->device));
    // the caller's stream, then ours: the examples are appended in call order
    VPT_HIP(hipStreamSynchronize(st));
    st = t->st;
    if (!checked) VPT_TRY(check_totals(d_ooff, n, total_b));
    const uint64_t total_chars = total_b + n;
    DBuf<uint32_t> cps, status, counts;
    DBuf<uint64_t> off;
    VPT_HIP(cps.resize(total_chars)); VPT_HIP(status.resize(1)); VPT_HIP(counts.resize(total_b)); VPT_HIP(off.resize(total_b + 1));
    VPT_HIP(hipMemsetAsync(status.p, 0, 4, st));
    const bool fw = (flags & VPT_FLAG_KYTEA_FULLWIDTH) != 0;
    VPT_HIP(vpt::launch_decode_chars(d_utf8, d_boff, d_ooff, n, total_chars, fw ? t->d_cinfo.p : nullptr, cps.p, nullptr, status.p, st, fw));
    if (!checked) VPT_HIP(vpt::train_check_labels(d_labels, total_b, status.p, st));
    uint32_t bad = 0;
    VPT_HIP(hipMemcpyAsync(&bad, status.p, 4, hipMemcpyDeviceToHost, st));
    VPT_HIP(hipStreamSynchronize(st));
    if (bad & ~vpt::kErrBadLabel) return fail_arg("out_offsets: do not match the text");
    if (bad) return fail_arg("labels: must be 0, 1 or 2");
    vpt::TrainFeatParams P{};
    P.cps = cps.p; P.ooff = d_ooff; P.n_sent = n; P.total_b = total_b;
    P.charw = t->prm.charw; P.charn = t->prm.charn; P.typew = t->prm.typew; P.typen = t->prm.typen; P.dictn = t->prm.dictn;
    P.dict_maxlen = t->dict_maxlen; P.dict_slots = t->d_dict_slots.p; P.dict_mask = t->dict_mask; P.dict_cps = t->d_dict_cps.p;
    P.dict_off = t->d_dict_off.p;
    P.counts = counts.p;
    VPT_HIP(vpt::train_features(P, false, st));
    uint64_t add = 0;
    VPT_TRY(scan_total(t, counts.p, total_b, off.p, &add));
    VPT_HIP(t->keys.grow(2 * (t->nnz_occ + add), 2 * t->nnz_occ, st));
    VPT_HIP(t->row_cnt.grow(t->nrows + total_b, t->nrows, st));
    VPT_HIP(t->labels.grow(t->nrows + total_b, t->nrows, st));
    P.row_off = off.p;
    P.keys = t->keys.p + 2 * t->nnz_occ;
    VPT_HIP(vpt::train_features(P, true, st));
    VPT_HIP(hipMemcpyAsync(t->row_cnt.p + t->nrows, counts.p, total_b * 4, hipMemcpyDeviceToDevice, st));
    VPT_HIP(hipMemcpyAsync(t->labels.p + t->nrows, d_labels, total_b, hipMemcpyDeviceToDevice, st));
    VPT_HIP(hipStreamSynchronize(st));
    t->nnz_occ += add;
    t->nrows += total_b;
    t->built = false;
    t->trained = false;
    return VPT_OK;
}

// ---------------------------------------------------------------------------------------------------- tag models (tag_trainer.rs)
double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the surface ids of the examples, on the device: representatives by a hash table over (code points, length), the distinct surfaces
// radix-sorted as rows of code points (0 past the end: byte order of UTF-8 is code point order, a prefix first), the examples sorted by
// (surface id, corpus order).  Back come 8 bytes an example and the distinct surfaces' chars.
vpt_status surface_ids(vpt_trainer* t, std::vector<uint32_t>& ex_order, std::vector<uint32_t>& sid) {
    hipStream_t st = t->st;
    const uint64_t n_ex = t->n_tag_ex;
    t->tag_surfaces.clear();
    ex_order.clear(); sid.clear();
    if (n_ex == 0) return VPT_OK;
    const uint64_t slots = table_slots(n_ex);
    DBuf<uint64_t> table, pos;
    DBuf<uint32_t> rep, flag, maxlen, slot, mat, id_of, d_sid;
    VPT_HIP(table.resize(slots)); VPT_HIP(rep.resize(n_ex)); VPT_HIP(flag.resize(n_ex)); VPT_HIP(maxlen.resize(1)); VPT_HIP(pos.resize(n_ex + 1));
    VPT_HIP(slot.resize(n_ex)); VPT_HIP(d_sid.resize(n_ex));
    VPT_HIP(hipMemsetAsync(table.p, 0, slots * 8, st));
    VPT_HIP(hipMemsetAsync(maxlen.p, 0, 4, st));
    VPT_HIP(vpt::train_surf_insert(t->d_tag_ex.p, n_ex, t->d_tag_cps.p, table.p, slots - 1, rep.p, flag.p, maxlen.p, st));
    uint64_t n_surf = 0;
    uint32_t ml = 0;
    VPT_TRY(scan_total(t, flag.p, n_ex, pos.p, &n_surf));
    VPT_HIP(hipMemcpy(&ml, maxlen.p, 4, hipMemcpyDeviceToHost));
    if (3 * uint64_t(ml) >= (1u << 20)) return fail_arg("examples: a tagged token of 349525 chars or more");
    VPT_HIP(mat.resize(n_surf * ml)); VPT_HIP(id_of.resize(n_surf));
    VPT_HIP(vpt::train_surf_matrix(t->d_tag_ex.p, n_ex, flag.p, pos.p, t->d_tag_cps.p, ml, mat.p, slot.p, st));
    Sorter S, E;   // the distinct surfaces by their chars, the examples by surface id
    for (uint32_t w = ml; w-- > 0;) S.bytes(w, 3);   // the type byte above the code point is no part of the order
    VPT_TRY(S.run(t, mat.p, ml, n_surf));
    VPT_HIP(vpt::train_ids(S.order.p, n_surf, id_of.p, rep.p, slot.p, n_ex, d_sid.p, st));
    E.bytes(0, Sorter::bytes_below(n_surf));
    VPT_TRY(E.run(t, d_sid.p, 1, n_ex));
    std::vector<uint32_t> h_mat(n_surf * ml), h_order(n_surf);
    ex_order.resize(n_ex); sid.resize(n_ex);
    VPT_HIP(hipMemcpyAsync(ex_order.data(), E.order.p, n_ex * 4, hipMemcpyDeviceToHost, st));
    VPT_HIP(hipMemcpyAsync(sid.data(), d_sid.p, n_ex * 4, hipMemcpyDeviceToHost, st));
    VPT_HIP(hipMemcpyAsync(h_mat.data(), mat.p, h_mat.size() * 4, hipMemcpyDeviceToHost, st));
    VPT_HIP(hipMemcpyAsync(h_order.data(), S.order.p, n_surf * 4, hipMemcpyDeviceToHost, st));
    VPT_HIP(hipStreamSynchronize(st));
    t->tag_surfaces.resize(n_surf);
    for (uint64_t j = 0; j < n_surf; ++j) {
        TagSurface& S = t->tag_surfaces[j];
        for (uint32_t k = 0; k < ml && h_mat[uint64_t(h_order[j]) * ml + k]; ++k) {
            const uint32_t w = h_mat[uint64_t(h_order[j]) * ml + k];
            S.cps.push_back(w & vpt::kCharMaskTrain);
            S.types.push_back(uint8_t(w >> 24));
            put_utf8(S.s, w & vpt::kCharMaskTrain);
        }
    }
    return VPT_OK;
}

// TagTrainer::train's grouping and train_tag's front half (tag_trainer.rs:148-180, 301-312): the models in surface order, the
// candidates per slot in order of first appearance, and a 0/1 problem per slot with at least two candidates.  The host sees the
// examples' surface ids and tag ids only and picks the rows; the keys are deduplicated and numbered and every problem's CSR and CSC
// written on the device, for all problems at once over concatenated arrays.
vpt_status build_tags(vpt_trainer* t) {
    if (t->tags_built) return VPT_OK;
    const double t_build = now_s();
    hipStream_t st = t->st;
    t->tag_models.clear();
    t->tag_problems.clear();
    t->tags_trained = false;
    std::vector<uint32_t> ex_order, sid;
    VPT_TRY(surface_ids(t, ex_order, sid));
    const double t_host = now_s();
    // a surface's examples: a run of ex_order
    std::vector<uint64_t> run(t->tag_surfaces.size() + 1, 0);
    for (uint32_t x : sid) ++run[x + 1];
    for (size_t j = 0; j < t->tag_surfaces.size(); ++j) run[j + 1] += run[j];
    std::map<std::string, int64_t> all;   // surface -> its id, -1: only the tag dictionary has it
    for (size_t j = 0; j < t->tag_surfaces.size(); ++j) all.emplace(t->tag_surfaces[j].s, int64_t(j));
    for (auto& kv : t->tag_defaults) {
        bool some = false;
        for (int32_t x : kv.second) some = some || x >= 0;
        if (some) all.emplace(kv.first, -1);
    }
    if (all.size() >= (size_t(1) << 24) - 1)
        return fail_arg("examples: at most 2^24 - 2 tag models (distinct token surfaces)");
    std::vector<uint32_t> row_ex, row_prob, row_y;
    std::vector<uint64_t> prob_row_ptr{0};
    for (auto& kv : all) {
        TagModelOut M;
        M.token = kv.first;
        M.surf = kv.second >= 0 ? &t->tag_surfaces[size_t(kv.second)] : nullptr;
        const std::vector<int32_t>* def = M.surf ? nullptr : &t->tag_defaults[kv.first];
        const uint64_t e0 = M.surf ? run[size_t(kv.second)] : 0, n_ex = M.surf ? run[size_t(kv.second) + 1] - e0 : 1;
        auto tags_of = [&](uint64_t i, uint32_t* n) -> const int32_t* {
            if (def) { *n = uint32_t(def->size()); return def->data(); }
            const uint32_t x = ex_order[e0 + i];
            *n = t->ex_ntags[x];
            return t->ex_tags.data() + t->ex_tag0[x];
        };
        uint32_t n_tags = 0;
        for (uint64_t i = 0; i < n_ex; ++i) { uint32_t n; tags_of(i, &n); n_tags = std::max(n_tags, n); }
        M.tags.assign(n_tags, {});
        for (uint64_t i = 0; i < n_ex; ++i) {
            uint32_t n;
            const int32_t* tg = tags_of(i, &n);
            for (uint32_t j = 0; j < n; ++j)
                if (tg[j] >= 0 && std::find(M.tags[j].begin(), M.tags[j].end(), tg[j]) == M.tags[j].end()) M.tags[j].push_back(tg[j]);
        }
        for (uint32_t j = 0; j < n_tags; ++j) {
            if (M.tags[j].size() < 2) continue;   // a fixed tag
            TagProblem Pb;
            Pb.model = uint32_t(t->tag_models.size());
            Pb.slot = j;
            Pb.class_offset = M.n_class;
            Pb.cands = M.tags[j];
            for (uint64_t i = 0; i < n_ex; ++i) {
                uint32_t n;
                const int32_t* tg = tags_of(i, &n);
                if (j >= n || tg[j] < 0) continue;
                row_ex.push_back(ex_order[e0 + i]);
                row_prob.push_back(uint32_t(t->tag_problems.size()));
                Pb.y.push_back(uint32_t(std::find(Pb.cands.begin(), Pb.cands.end(), tg[j]) - Pb.cands.begin()));
            }
            row_y.insert(row_y.end(), Pb.y.begin(), Pb.y.end());
            prob_row_ptr.push_back(row_ex.size());
            M.problems.push_back(uint32_t(t->tag_problems.size()));
            M.n_class += uint32_t(Pb.cands.size());
            t->tag_problems.push_back(std::move(Pb));
        }
        t->tag_models.push_back(std::move(M));
    }
    const double host_s = now_s() - t_host;
    // ---- the matrices, on the device
    const uint64_t n_prob = t->tag_problems.size(), n_rows = row_ex.size();
    t->h_prob_row_ptr = prob_row_ptr;
    t->h_prob_occ0.assign(n_prob + 1, 0);
    t->h_key_ptr.assign(n_prob + 1, 0);
    if (n_rows >= (uint64_t(1) << 32)) return fail_arg("examples: at most 2^32 - 1 rows over the tag problems");
    if (n_prob) {
        DBuf<uint32_t> d_row_ex, d_row_prob, nk, occ, occ_row, flag;
        DBuf<uint64_t> d_prp, occ_off, dpos, prob_occ0, key_ptr, dkeys;
        VPT_HIP(d_row_ex.resize(n_rows)); VPT_HIP(d_row_prob.resize(n_rows)); VPT_HIP(nk.resize(n_rows)); VPT_HIP(d_prp.resize(n_prob + 1));
        VPT_HIP(occ_off.resize(n_rows + 1)); VPT_HIP(t->b_y.resize(n_rows));
        VPT_HIP(hipMemcpyAsync(d_row_ex.p, row_ex.data(), n_rows * 4, hipMemcpyHostToDevice, st));
        VPT_HIP(hipMemcpyAsync(d_row_prob.p, row_prob.data(), n_rows * 4, hipMemcpyHostToDevice, st));
        VPT_HIP(hipMemcpyAsync(t->b_y.p, row_y.data(), n_rows * 4, hipMemcpyHostToDevice, st));
        VPT_HIP(hipMemcpyAsync(d_prp.p, prob_row_ptr.data(), (n_prob + 1) * 8, hipMemcpyHostToDevice, st));
        VPT_HIP(vpt::train_tag_expand(d_row_ex.p, d_row_prob.p, n_rows, t->d_tag_ex.p, nullptr, nullptr, nk.p, nullptr, st));
        uint64_t n_occ = 0;
        VPT_TRY(scan_total(t, nk.p, n_rows, occ_off.p, &n_occ));
        if (n_occ >= (uint64_t(1) << 32)) return fail_arg("examples: at most 2^32 - 1 nonzeros over the tag problems");
        VPT_HIP(occ.resize(5 * n_occ)); VPT_HIP(occ_row.resize(n_occ)); VPT_HIP(flag.resize(n_occ)); VPT_HIP(dpos.resize(n_occ + 1));
        VPT_HIP(vpt::train_tag_expand(d_row_ex.p, d_row_prob.p, n_rows, t->d_tag_ex.p, occ_off.p, t->d_tag_keys.p, occ.p, occ_row.p, st));
        // stably sorted by (problem, key): the key's four words least significant first, then the problem's bytes that can differ
        Sorter S;
        for (uint32_t w = 0; w < 4; ++w) S.bytes(w, 4);
        S.bytes(4, Sorter::bytes_below(n_prob));
        VPT_TRY(S.run(t, occ.p, 5, n_occ));
        VPT_HIP(vpt::train_tag_flags(occ.p, S.order.p, n_occ, flag.p, st));
        uint64_t n_dist = 0;
        VPT_TRY(scan_total(t, flag.p, n_occ, dpos.p, &n_dist));
        VPT_HIP(prob_occ0.resize(n_prob + 1)); VPT_HIP(key_ptr.resize(n_prob + 1)); VPT_HIP(dkeys.resize(2 * n_dist));
        VPT_HIP(t->b_cols.resize(n_occ)); VPT_HIP(t->b_crow.resize(n_occ)); VPT_HIP(t->b_rp.resize(n_rows + n_prob)); VPT_HIP(t->b_cp.resize(n_dist + n_prob));
        vpt::TagBuildParams B{};
        B.n_prob = n_prob; B.n_rows = n_rows; B.n_occ = n_occ; B.prob_row_ptr = d_prp.p; B.row_prob = d_row_prob.p; B.occ_off = occ_off.p; B.occ = occ.p;
        B.occ_row = occ_row.p; B.order = S.order.p; B.flag = flag.p; B.dpos = dpos.p; B.prob_occ0 = prob_occ0.p; B.key_ptr = key_ptr.p;
        B.occ_col = t->b_cols.p; B.dkeys = dkeys.p; B.rp = t->b_rp.p; B.cp = t->b_cp.p; B.crow = t->b_crow.p;
        VPT_HIP(vpt::train_tag_assemble(B, st));
        std::vector<uint64_t> h_dkeys(2 * n_dist);
        VPT_HIP(hipMemcpyAsync(t->h_prob_occ0.data(), prob_occ0.p, (n_prob + 1) * 8, hipMemcpyDeviceToHost, st));
        VPT_HIP(hipMemcpyAsync(t->h_key_ptr.data(), key_ptr.p, (n_prob + 1) * 8, hipMemcpyDeviceToHost, st));
        if (n_dist) VPT_HIP(hipMemcpyAsync(h_dkeys.data(), dkeys.p, n_dist * 16, hipMemcpyDeviceToHost, st));
        VPT_HIP(hipStreamSynchronize(st));
        // the distinct keys alone come back: the model's n-grams are made of them
        for (uint64_t p = 0; p < n_prob; ++p) {
            TagProblem& Pb = t->tag_problems[p];
            Pb.index = uint32_t(p);
            Pb.nnz = t->h_prob_occ0[p + 1] - t->h_prob_occ0[p];
            for (uint64_t c = t->h_key_ptr[p]; c < t->h_key_ptr[p + 1]; ++c) Pb.keys.push_back((u128(h_dkeys[2 * c + 1]) << 64) | h_dkeys[2 * c]);
        }
    }
    t->tags_built = true;
    t->tag_build_seconds = now_s() - t_build;
    t->tag_build_host_seconds = host_s;
    return VPT_OK;
}

// a problem's keys as the two words a key that vpt::train_key and l1r_groups take
std::vector<uint64_t> tag_key_words(const TagProblem& Pb) {
    std::vector<uint64_t> out(2 * Pb.keys.size());
    for (size_t j = 0; j < Pb.keys.size(); ++j) { out[2 * j] = uint64_t(Pb.keys[j]); out[2 * j + 1] = uint64_t(Pb.keys[j] >> 64); }
    return out;
}

// a problem's CSR on the host, for the inspection calls and the global-memory path
vpt_status fetch_rows(vpt_trainer* t, TagProblem& Pb) {
    if (Pb.fetched) return VPT_OK;
    const uint64_t p = Pb.index, l = Pb.y.size();
    Pb.rp.assign(l + 1, 0);
    Pb.cols.assign(Pb.nnz, 0);
    VPT_HIP(hipMemcpy(Pb.rp.data(), t->b_rp.p + t->h_prob_row_ptr[p] + p, (l + 1) * 4, hipMemcpyDeviceToHost));
    if (Pb.nnz) VPT_HIP(hipMemcpy(Pb.cols.data(), t->b_cols.p + t->h_prob_occ0[p], Pb.nnz * 4, hipMemcpyDeviceToHost));
    Pb.fetched = true;
    return VPT_OK;
}

// one problem through the global-memory solver, a class at a time: TRON, or for solvers 5 and 6 the group launches of solve_l1r and
// solve_l1r_lr
vpt_status solve_tag_large(vpt_trainer* t, TagProblem& Pb, double eps, double cost, int solver) {
    hipStream_t st = t->st;
    const double t_setup = now_s();
    VPT_TRY(fetch_rows(t, Pb));
    const uint64_t l = Pb.y.size(), nf = Pb.keys.size(), nz = Pb.cols.size(), k = Pb.cands.size();
    std::vector<uint64_t> ptr(Pb.rp.begin(), Pb.rp.end());
    std::vector<uint32_t> rows(nz);
    for (uint64_t r = 0; r < l; ++r)
        for (uint32_t q = Pb.rp[r]; q < Pb.rp[r + 1]; ++q) rows[q] = uint32_t(r);
    const std::vector<uint16_t> ones(nz, 1);
    Matrix M;
    DBuf<uint32_t> d_rows;
    VPT_HIP(M.csr_ptr.resize(l + 1)); VPT_HIP(M.cols.resize(nz)); VPT_HIP(d_rows.resize(nz)); VPT_HIP(M.vals.resize(nz));
    VPT_HIP(hipMemcpy(M.csr_ptr.p, ptr.data(), (l + 1) * 8, hipMemcpyHostToDevice));
    if (nz) {
        VPT_HIP(hipMemcpy(M.cols.p, Pb.cols.data(), nz * 4, hipMemcpyHostToDevice));
        VPT_HIP(hipMemcpy(d_rows.p, rows.data(), nz * 4, hipMemcpyHostToDevice));
        VPT_HIP(hipMemcpy(M.vals.p, ones.data(), nz * 2, hipMemcpyHostToDevice));
    }
    VPT_TRY(csc_levels(t, M, d_rows.p, nz, nf));
    Tron T;
    L1rGroups G;
    if (solver == 5 || solver == 6) VPT_TRY(l1r_matrix_groups(M, l, tag_key_words(Pb), G));
    else VPT_TRY(T.init(M, st, l, solver, cost));
    std::vector<double> y(l);
    const uint64_t n_solve = k == 2 ? 1 : k, n = nf + 1;
    VPT_HIP(hipStreamSynchronize(st));
    Pb.seconds_setup = now_s() - t_setup;
    Pb.seconds_solve = 0;
    for (uint64_t c = 0; c < n_solve; ++c) {
        uint64_t pos = 0;
        for (uint64_t r = 0; r < l; ++r) { y[r] = Pb.y[r] == c ? 1.0 : -1.0; pos += Pb.y[r] == c; }
        const double t_run = now_s();
        if (solver == 5) VPT_TRY(solve_l1r(t, M, l, y, pos, G, eps, cost, Pb.w.data() + c * n, &Pb.stats[c]));
        else if (solver == 6) VPT_TRY(solve_l1r_lr(t, M, l, y, pos, G, eps, cost, Pb.w.data() + c * n, &Pb.stats[c]));
        else VPT_TRY(T.solve(y, pos, eps, &Pb.stats[c], Pb.w.data() + c * n));
        Pb.seconds_solve += now_s() - t_run;
    }
    if (k == 2) {
        for (uint64_t i = 0; i < n; ++i) Pb.w[n + i] = -Pb.w[i];
        Pb.stats[1] = Pb.stats[0];
    }
    Pb.path = 2;
    return VPT_OK;
}

vpt_status solve_tags(vpt_trainer* t, double eps, double cost, int solver) {
    hipStream_t st = t->st;
    t->tag_summary = vpt_tag_train_summary{};
    std::vector<vpt::TagSolveDesc> descs;
    std::vector<uint32_t> small;
    uint64_t n_w = 0, n_stats = 0;
    // solvers 5 and 6: the in-kernel problems' columns by group (l1r_groups over a problem's keys: a tag example has at most one feature
    // per template, tag_trainer.rs:79-100) beside their descriptors; n_viol counts solver 5's violations or solver 6's scratch
    const bool l1lr = solver == 6, l1 = solver == 5 || l1lr;
    std::vector<vpt::TagL1Desc> l1descs;
    std::vector<vpt::TagL1Group> l1groups;
    std::vector<uint32_t> gcols, h_cp, h_crow;
    uint64_t n_viol = 0;
    if (l1 && t->tag_path_mode == 0 && !t->tag_problems.empty()) {
        h_cp.resize(t->h_key_ptr.back() + t->tag_problems.size());
        VPT_HIP(hipMemcpy(h_cp.data(), t->b_cp.p, h_cp.size() * 4, hipMemcpyDeviceToHost));
#if defined(VPT_HIPEMU) || defined(VPT_DEBUG)
        h_crow.resize(t->h_prob_occ0.back());
        if (!h_crow.empty()) VPT_HIP(hipMemcpy(h_crow.data(), t->b_crow.p, h_crow.size() * 4, hipMemcpyDeviceToHost));
#endif
    }
    for (size_t i = 0; i < t->tag_problems.size(); ++i) {
        TagProblem& Pb = t->tag_problems[i];
        const uint64_t l = Pb.y.size(), nf = Pb.keys.size(), k = Pb.cands.size();
        Pb.w.assign(k * (nf + 1), 0.0);
        Pb.stats.assign(k, vpt_train_stats{});
        Pb.path = (t->tag_path_mode == 0 && (l1lr ? vpt::train_tag_l1lr_fits(l, nf) : l1 ? vpt::train_tag_l1_fits(l, nf) : vpt::train_tag_fits(l, nf))) ? 1 : 2;
        Pb.seconds_setup = Pb.seconds_solve = 0;
        if (Pb.path != 1) continue;
        // the problem where build_tags left it on the device
        vpt::TagSolveDesc D{};
        D.rp = t->h_prob_row_ptr[i] + i; D.cols = t->h_prob_occ0[i]; D.cp = t->h_key_ptr[i] + i; D.y = t->h_prob_row_ptr[i]; D.w = n_w; D.stats = n_stats;
        D.nf = uint32_t(nf); D.l = uint32_t(l); D.k = uint32_t(k);
        n_w += k * (nf + 1);
        n_stats += k;
        descs.push_back(D);
        small.push_back(uint32_t(i));
        if (!l1) continue;
        const uint32_t* cp = h_cp.data() + D.cp;
        const L1rGroups G = l1r_groups(tag_key_words(Pb), cp, nf);
        VPT_TRY(l1r_check_groups(G, h_crow.empty() ? nullptr : h_crow.data() + D.cols, cp, l, nf));
        if (G.size() > vpt::kTagL1MaxGroups) return fail(VPT_RUNTIME_ERROR, "solvers 5 and 6: a tag problem with more column groups than its kernel holds");
        vpt::TagL1Desc E{};
        E.gcols = gcols.size(); E.groups = l1groups.size(); E.viol = n_viol; E.n_groups = uint32_t(G.size());
        for (size_t g = 0; g < G.size(); ++g)
            l1groups.push_back(vpt::TagL1Group{uint32_t(G.ptr[g]), G.n_lane[g], G.n_wave[g], uint32_t(G.ptr[g + 1] - G.ptr[g])});
        gcols.insert(gcols.end(), G.cols.begin(), G.cols.end());
        n_viol += l1lr ? vpt::train_tag_l1lr_scratch(l, nf) : nf + 1;
        l1descs.push_back(E);
    }
    if (!descs.empty()) {
        const double t0 = now_s();
        DBuf<vpt::TagSolveDesc> d_desc;
        DBuf<double> d_w;
        DBuf<vpt_train_stats> d_stats;
        VPT_HIP(d_desc.resize(descs.size())); VPT_HIP(d_w.resize(n_w)); VPT_HIP(d_stats.resize(n_stats));
        VPT_HIP(hipMemcpyAsync(d_desc.p, descs.data(), descs.size() * sizeof(vpt::TagSolveDesc), hipMemcpyHostToDevice, st));
        VPT_HIP(hipMemsetAsync(d_w.p, 0, n_w * 8, st));
        VPT_HIP(hipMemsetAsync(d_stats.p, 0, n_stats * sizeof(vpt_train_stats), st));
        DBuf<vpt::TagL1Desc> d_l1desc;   // solvers 5 and 6
        DBuf<vpt::TagL1Group> d_groups;
        DBuf<uint32_t> d_gcols;
        DBuf<double> d_viol;
        if (l1) {
            VPT_HIP(d_l1desc.resize(l1descs.size())); VPT_HIP(d_groups.resize(l1groups.size())); VPT_HIP(d_gcols.resize(gcols.size())); VPT_HIP(d_viol.resize(n_viol));
            VPT_HIP(hipMemcpyAsync(d_l1desc.p, l1descs.data(), l1descs.size() * sizeof(vpt::TagL1Desc), hipMemcpyHostToDevice, st));
            VPT_HIP(hipMemcpyAsync(d_groups.p, l1groups.data(), l1groups.size() * sizeof(vpt::TagL1Group), hipMemcpyHostToDevice, st));
            VPT_HIP(hipMemcpyAsync(d_gcols.p, gcols.data(), gcols.size() * 4, hipMemcpyHostToDevice, st));
            VPT_HIP(hipMemsetAsync(d_viol.p, 0, n_viol * 8, st));
            VPT_HIP((l1lr ? vpt::train_tag_l1lr_solve : vpt::train_tag_l1_solve)(d_desc.p, d_l1desc.p, uint32_t(descs.size()), t->b_rp.p, t->b_cols.p, t->b_cp.p,
                                                                                 t->b_crow.p, t->b_y.p, d_gcols.p, d_groups.p, eps, cost, d_viol.p, d_w.p,
                                                                                 d_stats.p, st));
        } else {
            VPT_HIP(vpt::train_tag_solve(d_desc.p, uint32_t(descs.size()), t->b_rp.p, t->b_cols.p, t->b_cp.p, t->b_crow.p, t->b_y.p, eps, cost, solver, d_w.p,
                                         d_stats.p, st));
        }
        std::vector<double> w(n_w);
        std::vector<vpt_train_stats> stats(n_stats);
        VPT_HIP(hipMemcpyAsync(w.data(), d_w.p, n_w * 8, hipMemcpyDeviceToHost, st));
        VPT_HIP(hipMemcpyAsync(stats.data(), d_stats.p, n_stats * sizeof(vpt_train_stats), hipMemcpyDeviceToHost, st));
        VPT_HIP(hipStreamSynchronize(st));
        for (size_t q = 0; q < small.size(); ++q) {
            TagProblem& Pb = t->tag_problems[small[q]];
            std::copy(w.begin() + descs[q].w, w.begin() + descs[q].w + Pb.w.size(), Pb.w.begin());
            std::copy(stats.begin() + descs[q].stats, stats.begin() + descs[q].stats + Pb.stats.size(), Pb.stats.begin());
        }
        t->tag_summary.problems_in_kernel = descs.size();
        t->tag_summary.seconds_in_kernel = now_s() - t0;
    }
    const double t1 = now_s();
    for (TagProblem& Pb : t->tag_problems) {
        if (Pb.path != 2) continue;
        VPT_TRY(solve_tag_large(t, Pb, eps, cost, solver));
        ++t->tag_summary.problems_large;
        t->tag_summary.seconds_large_solve += Pb.seconds_solve;
    }
    t->tag_summary.seconds_large = now_s() - t1;
    t->tag_summary.seconds_construction = t->tag_build_seconds;
    t->tag_summary.seconds_construction_host = t->tag_build_host_seconds;
    t->tag_summary.seconds_add_host = t->tag_add_host_seconds;
    t->tags_trained = true;
    return VPT_OK;
}

// train_tag's back half (tag_trainer.rs:195-298) and the tag models of Model::to_vec
void encode_tag_models(vpt_trainer* t, Enc& e) {
    e.uvar(t->tag_models.size());
    for (const TagModelOut& M : t->tag_models) {
        std::map<std::pair<std::string, uint8_t>, std::vector<int32_t>> cw, tw;
        std::vector<int32_t> bias(M.n_class, 0);
        for (uint32_t pi : M.problems) {
            const TagProblem& Pb = t->tag_problems[pi];
            const size_t nf = Pb.keys.size(), k = Pb.cands.size();
            double wmax = 1e-6;
            for (double x : Pb.w) wmax = std::max(wmax, std::fabs(x));
            const double m = wmax / double((1 << 15) - 1);
            for (size_t c = 0; c < k; ++c) bias[Pb.class_offset + c] = int32_t(Pb.w[c * (nf + 1) + nf] / m);
            for (size_t j = 0; j < nf; ++j) {
                std::vector<int32_t>* row = nullptr;
                for (size_t c = 0; c < k; ++c) {
                    const int32_t q = int32_t(Pb.w[c * (nf + 1) + j] / m);
                    if (q == 0) continue;
                    if (!row) {
                        // the n-gram: the left context, the token, the right context
                        const vpt::TrainKey K = vpt::train_key(uint64_t(Pb.keys[j]), uint64_t(Pb.keys[j] >> 64));
                        const uint32_t kind = K.kind, left = K.len - uint32_t(K.rel);
                        std::string ng;
                        for (uint32_t q2 = 0; q2 < left; ++q2) put_sym(ng, kind, K.c[q2]);
                        for (size_t q2 = 0; q2 < M.surf->cps.size(); ++q2) put_sym(ng, kind, kind == 0 ? M.surf->cps[q2] : M.surf->types[q2]);
                        for (uint32_t q2 = left; q2 < K.len; ++q2) put_sym(ng, kind, K.c[q2]);
                        auto& mp = kind == 0 ? cw : tw;
                        row = &mp.emplace(std::make_pair(ng, uint8_t(K.rel)), std::vector<int32_t>(M.n_class, 0)).first->second;
                    }
                    (*row)[Pb.class_offset + c] = q;
                }
            }
        }
        e.raw(M.token);
        e.uvar(M.tags.size());
        for (auto& cands : M.tags) {
            e.uvar(cands.size());
            for (int32_t id : cands) e.raw(t->tag_strings[size_t(id)]);
        }
        for (auto* mp : {&cw, &tw}) {
            size_t n_ng = 0;
            for (auto it = mp->begin(); it != mp->end(); ++it) n_ng += it == mp->begin() || std::prev(it)->first.first != it->first.first;
            e.uvar(n_ng);
            for (auto it = mp->begin(); it != mp->end();) {
                auto last = it;
                size_t n_w = 0;
                while (last != mp->end() && last->first.first == it->first.first) { ++last; ++n_w; }
                e.raw(it->first.first);
                e.uvar(n_w);
                for (; it != last; ++it) { e.u8(it->first.second); e.weights(it->second); }
            }
        }
        e.weights(bias);
    }
}

vpt_status add_tagged_device(vpt_trainer* t, const uint8_t* d_utf8, const uint64_t* d_boff, const uint64_t* d_ooff, size_t n, uint64_t total_b,
                             const uint8_t* d_labels, const uint32_t* d_n_tags, const uint64_t* d_tag_index, const uint64_t* d_span_off,
                             const uint8_t* d_tag_bytes, uint64_t n_spans, uint64_t n_tag_bytes, unsigned flags, hipStream_t caller, bool checked) {
    if ((flags & ~unsigned(VPT_FLAG_KYTEA_FULLWIDTH)) != 0) return fail_arg("flags: only VPT_FLAG_KYTEA_FULLWIDTH");
    if (n == 0) return VPT_OK;
    VPT_HIP(hipSetDevice(t->device));
    VPT_HIP(hipStreamSynchronize(caller));
    hipStream_t st = t->st;
    if (!checked) VPT_TRY(check_totals(d_ooff, n, total_b));
    const uint64_t total_chars = total_b + n;
    if (total_chars >= (uint64_t(1) << 32)) return fail_arg("examples: at most 2^32 - 1 chars in a batch");
    DBuf<uint32_t> cps, status, counts, is_ex;
    VPT_HIP(cps.resize(total_chars)); VPT_HIP(status.resize(2));
    VPT_HIP(hipMemsetAsync(status.p, 0, 8, st));
    const bool fw = (flags & VPT_FLAG_KYTEA_FULLWIDTH) != 0;
    VPT_HIP(vpt::launch_decode_chars(d_utf8, d_boff, d_ooff, n, total_chars, fw ? t->d_cinfo.p : nullptr, cps.p, nullptr, status.p, st, fw));
    if (!checked) VPT_HIP(vpt::train_check_labels(d_labels, total_b, status.p, st));
    uint32_t bad[2] = {0, 0};
    VPT_HIP(hipMemcpyAsync(bad, status.p, 4, hipMemcpyDeviceToHost, st));
    VPT_HIP(hipStreamSynchronize(st));
    if (bad[0] & ~vpt::kErrBadLabel) return fail_arg("out_offsets: do not match the text");
    if (bad[0]) return fail_arg("labels: must be 0, 1 or 2");
    // the tags' CSR is checked on the device before anything follows one of its offsets
    VPT_HIP(vpt::train_tag_validate(d_n_tags, d_ooff, n, total_chars, d_tag_index, d_span_off, n_spans, n_tag_bytes, status.p + 1, st));
    VPT_HIP(hipMemcpyAsync(bad + 1, status.p + 1, 4, hipMemcpyDeviceToHost, st));
    VPT_HIP(hipStreamSynchronize(st));
    if (bad[1] & 1u) return fail_arg("tag_index: must not decrease, pass n_spans or give a char more tags than n_tags");
    if (bad[1] & 2u) return fail_arg("span_offsets: must not decrease or pass tag_bytes");
    std::vector<uint64_t> ooff(n + 1), tindex(total_chars + 1), soff(n_spans + 1);
    std::vector<uint32_t> ntags(n);
    std::vector<uint8_t> tbytes(n_tag_bytes);
    VPT_HIP(hipMemcpy(ooff.data(), d_ooff, (n + 1) * 8, hipMemcpyDeviceToHost));
    VPT_HIP(hipMemcpy(ntags.data(), d_n_tags, n * 4, hipMemcpyDeviceToHost));
    VPT_HIP(hipMemcpy(tindex.data(), d_tag_index, (total_chars + 1) * 8, hipMemcpyDeviceToHost));
    VPT_HIP(hipMemcpy(soff.data(), d_span_off, (n_spans + 1) * 8, hipMemcpyDeviceToHost));
    if (n_tag_bytes) VPT_HIP(hipMemcpy(tbytes.data(), d_tag_bytes, n_tag_bytes, hipMemcpyDeviceToHost));
    // what the model format cannot hold: a NUL, or bytes that are no UTF-8
    {
        std::vector<uint32_t> tmp;
        size_t sent = 0;
        for (uint64_t g = 0; g < total_chars; ++g) {
            while (ooff[sent + 1] + sent + 1 <= g) ++sent;
            for (uint64_t k = tindex[g]; k < tindex[g + 1]; ++k) {
                const uint8_t* b = tbytes.data() + soff[k];
                const size_t len = size_t(soff[k + 1] - soff[k]);
                if (std::find(b, b + len, uint8_t(0)) != b + len)
                    return fail_arg("tags: must not contain NULL (sentence " + std::to_string(sent) + ")");
                if (!vpt::decode_utf8(b, len, tmp))
                    return fail_arg("tags: invalid UTF-8 (sentence " + std::to_string(sent) + ")");
            }
        }
    }
    // the tag examples: count, place, write
    DBuf<uint64_t> ex_off, key_off;
    VPT_HIP(counts.resize(total_chars)); VPT_HIP(is_ex.resize(total_chars)); VPT_HIP(ex_off.resize(total_chars + 1)); VPT_HIP(key_off.resize(total_chars + 1));
    vpt::TagFeatParams P{};
    P.cps = cps.p; P.ooff = d_ooff; P.labels = d_labels; P.n_tags = d_n_tags; P.n_sent = n; P.total_chars = total_chars;
    P.charn = t->prm.charn; P.typen = t->prm.typen; P.is_ex = is_ex.p; P.counts = counts.p;
    VPT_HIP(vpt::train_tag_features(P, false, st));
    uint64_t n_ex = 0, n_keys = 0;
    VPT_TRY(scan_total(t, is_ex.p, total_chars, ex_off.p, &n_ex));
    VPT_TRY(scan_total(t, counts.p, total_chars, key_off.p, &n_keys));
    if (t->n_tag_cps + total_chars >= (uint64_t(1) << 32) || t->n_tag_keys + n_keys >= (uint64_t(1) << 32) || t->n_tag_ex + n_ex >= (uint64_t(1) << 32))
        return fail_arg("examples: at most 2^32 - 1 chars, tagged tokens and tag feature occurrences");
    // the boundary examples, exactly as the untagged call adds them: behind the last refusal, so that a refused batch adds nothing
    VPT_TRY(add_device(t, d_utf8, d_boff, d_ooff, n, total_b, d_labels, flags, st, true));
    // the examples stay on the device: the batch's chars, the records and the keys are appended to the trainer's arrays
    DBuf<uint32_t> recs;
    VPT_HIP(recs.resize(4 * n_ex));
    VPT_HIP(t->d_tag_cps.grow(t->n_tag_cps + total_chars, t->n_tag_cps, st));
    VPT_HIP(t->d_tag_ex.grow(4 * (t->n_tag_ex + n_ex), 4 * t->n_tag_ex, st));
    VPT_HIP(t->d_tag_keys.grow(2 * (t->n_tag_keys + n_keys), 2 * t->n_tag_keys, st));
    P.ex_off = ex_off.p; P.key_off = key_off.p; P.recs = recs.p; P.keys = t->d_tag_keys.p + 2 * t->n_tag_keys;
    VPT_HIP(vpt::train_tag_features(P, true, st));
    VPT_HIP(hipMemcpyAsync(t->d_tag_cps.p + t->n_tag_cps, cps.p, total_chars * 4, hipMemcpyDeviceToDevice, st));
    VPT_HIP(vpt::train_tag_rec_finish(recs.p, n_ex, d_ooff, key_off.p, uint32_t(t->n_tag_cps), uint32_t(t->n_tag_keys), t->d_tag_ex.p + 4 * t->n_tag_ex, st));
    std::vector<uint32_t> h_recs(4 * n_ex);
    if (n_ex) VPT_HIP(hipMemcpyAsync(h_recs.data(), recs.p, n_ex * 16, hipMemcpyDeviceToHost, st));
    VPT_HIP(hipStreamSynchronize(st));
    // the tag strings are interned here, on the host: 16 bytes an example come back, no char and no key
    const double t_host = now_s();
    for (uint64_t x = 0; x < n_ex; ++x) {
        const uint32_t sent = h_recs[4 * x], end = h_recs[4 * x + 2];
        const uint64_t g = ooff[sent] + sent + end - 1;
        t->ex_ntags.push_back(ntags[sent]);
        t->ex_tag0.push_back(t->ex_tags.size());
        for (uint32_t j = 0; j < ntags[sent]; ++j) {
            const uint64_t k = tindex[g] + j;
            if (k >= tindex[g + 1] || soff[k + 1] == soff[k]) { t->ex_tags.push_back(-1); continue; }
            t->ex_tags.push_back(t->intern_tag(std::string(reinterpret_cast<const char*>(tbytes.data()) + soff[k], size_t(soff[k + 1] - soff[k]))));
        }
    }
    t->n_tag_cps += total_chars;
    t->n_tag_ex += n_ex;
    t->n_tag_keys += n_keys;
    t->tag_add_host_seconds += now_s() - t_host;
    t->tags_built = false;
    t->tags_trained = false;
    return VPT_OK;
}

// A host batch on the device, on the trainer's stream: the boundaries counted, the labels checked, the text padded and the offsets
// rebased to its first byte.  The host copies outlive the asynchronous copies (the add that follows ends with a synchronisation).
struct StagedBatch {
    std::vector<uint64_t> boff, ooff;
    uint64_t total_b = 0;
    DBuf<uint8_t> d_text, d_labels;
    DBuf<uint64_t> d_boff, d_ooff;
};
vpt_status stage_batch(vpt_trainer* t, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n, const uint8_t* labels, StagedBatch& B) {
    B.ooff.resize(n + 1);
    VPT_TRY(vpt_count_boundaries(utf8, byte_offsets, n, B.ooff.data()));
    const uint64_t total_b = B.total_b = B.ooff[n];
    if (total_b && !labels) return fail_arg("NULL argument");
    for (uint64_t b = 0; b < total_b; ++b)
        if (labels[b] > 2) return fail_arg("labels: must be 0, 1 or 2");
    VPT_HIP(hipSetDevice(t->device));
    const uint64_t b0 = byte_offsets[0], nbytes = byte_offsets[n] - b0;
    B.boff.assign(byte_offsets, byte_offsets + n + 1);
    for (auto& x : B.boff) x -= b0;
    VPT_HIP(B.d_text.resize(nbytes + 64)); VPT_HIP(B.d_labels.resize(total_b)); VPT_HIP(B.d_boff.resize(n + 1)); VPT_HIP(B.d_ooff.resize(n + 1));
    VPT_HIP(hipMemsetAsync(B.d_text.p, 0, nbytes + 64, t->st));
    VPT_HIP(hipMemcpyAsync(B.d_text.p, utf8 + b0, nbytes, hipMemcpyHostToDevice, t->st));
    if (total_b) VPT_HIP(hipMemcpyAsync(B.d_labels.p, labels, total_b, hipMemcpyHostToDevice, t->st));
    VPT_HIP(hipMemcpyAsync(B.d_boff.p, B.boff.data(), B.boff.size() * 8, hipMemcpyHostToDevice, t->st));
    VPT_HIP(hipMemcpyAsync(B.d_ooff.p, B.ooff.data(), B.ooff.size() * 8, hipMemcpyHostToDevice, t->st));
    return VPT_OK;
}

// the last trained model into the caller's buffer (NULL: its size alone)
vpt_status copy_model(const vpt_trainer* t, uint8_t* model_out, size_t capacity, size_t* needed) {
    *needed = t->model.size();
    if (model_out) {
        if (capacity < t->model.size()) return fail_arg("capacity: smaller than the model");
        std::memcpy(model_out, t->model.data(), t->model.size());
    }
    return VPT_OK;
}

}  // namespace

extern "C" {

vpt_status vpt_trainer_create(const uint32_t* params_words, const uint8_t* dict_utf8, const uint64_t* dict_offsets, size_t n_dict_words,
                              int device_id, void** out) {
    const vpt_train_params* params = reinterpret_cast<const vpt_train_params*>(params_words);
    if (!params || !out || (n_dict_words && (!dict_utf8 || !dict_offsets))) return fail_arg("NULL argument");
    *out = nullptr;
    const vpt_train_params& p = *params;
    if (p.charn < 1 || p.charn > 5) return fail_arg("charn: must be between 1 and 5");
    if (p.typen < 1 || p.typen > 5) return fail_arg("typen: must be between 1 and 5");
    if (p.charw > 16) return fail_arg("charw: must be at most 16");
    if (p.typew > 16) return fail_arg("typew: must be at most 16");
    if (p.typew > p.charw) return fail_arg("typew: must not exceed charw (type weights use the char window)");
    if ((p.flags & ~uint32_t(VPT_TRAIN_TAGS | VPT_TRAIN_L1R | VPT_TRAIN_TAGS_L1R | VPT_TRAIN_L1R_LR | VPT_TRAIN_TAGS_L1R_LR)) != 0)
        return fail_arg((p.flags & VPT_TRAIN_L1R_LR) ? "flags: unknown bit beside VPT_TRAIN_L1R_LR (the others: VPT_TRAIN_TAGS, VPT_TRAIN_L1R, VPT_TRAIN_TAGS_L1R, VPT_TRAIN_TAGS_L1R_LR)"
                                                     : "flags: must be 0 or VPT_TRAIN_TAGS, VPT_TRAIN_L1R or both");
    if ((p.flags & VPT_TRAIN_TAGS_L1R) && (p.flags & (VPT_TRAIN_TAGS | VPT_TRAIN_L1R)) != (VPT_TRAIN_TAGS | VPT_TRAIN_L1R))
        return fail_arg("flags: VPT_TRAIN_TAGS_L1R needs both VPT_TRAIN_TAGS and VPT_TRAIN_L1R");
    if ((p.flags & VPT_TRAIN_TAGS_L1R_LR) && (p.flags & (VPT_TRAIN_TAGS | VPT_TRAIN_L1R_LR)) != (VPT_TRAIN_TAGS | VPT_TRAIN_L1R_LR))
        return fail_arg("flags: VPT_TRAIN_TAGS_L1R_LR needs both VPT_TRAIN_TAGS and VPT_TRAIN_L1R_LR");
    if (n_dict_words && (p.dictn < 1 || p.dictn > 0x1FFFFF)) return fail_arg("dictn: must be at least 1 with a dictionary");
    std::unique_ptr<vpt_trainer> t(new (std::nothrow) vpt_trainer());
    if (!t) return fail(VPT_RUNTIME_ERROR, "out of host memory");
    t->prm = p;
    std::vector<uint32_t> all_cps, cps;
    std::vector<uint64_t> woff{0};
    std::set<std::string> seen;
    for (size_t i = 0; i < n_dict_words; ++i) {
        if (dict_offsets[i + 1] < dict_offsets[i]) return fail_arg("dict_offsets: must be non-decreasing");
        const uint8_t* s = dict_utf8 + dict_offsets[i];
        const size_t len = size_t(dict_offsets[i + 1] - dict_offsets[i]);
        if (len == 0) return fail_arg("dict_words: must not contain an empty word (word " + std::to_string(i) + ")");
        if (!vpt::decode_utf8(s, len, cps)) return fail_arg("dict_words: invalid UTF-8 (word " + std::to_string(i) + ")");
        std::string w(reinterpret_cast<const char*>(s), len);
        if (!seen.insert(w).second) return fail_arg("dict_words: duplicate word (word " + std::to_string(i) + ")");
        t->dict_words.push_back(w);
        t->dict_len.push_back(uint32_t(cps.size()));
        t->dict_maxlen = std::max(t->dict_maxlen, uint32_t(cps.size()));
        all_cps.insert(all_cps.end(), cps.begin(), cps.end());
        woff.push_back(all_cps.size());
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(VPT_RUNTIME_ERROR, "no HIP device available (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= n_dev) return fail_arg("device_id: no such device");
    t->device = device_id;
    VPT_HIP(hipSetDevice(device_id));
    VPT_HIP(hipStreamCreateWithFlags(&t->st, hipStreamNonBlocking));
    // KyteaFullwidthFilter's image of the BMP | its CharacterType << 16 (decode_chars_kernel's table)
    std::vector<uint32_t> cinfo(65536);
    for (uint32_t cp = 0; cp < 65536; ++cp) {
        const uint32_t fw = vpt::kytea_fullwidth_host(cp);
        cinfo[cp] = fw | (uint32_t(vpt::char_type_host(fw)) << 16);
    }
    VPT_HIP(t->d_cinfo.resize(65536));
    VPT_HIP(hipMemcpy(t->d_cinfo.p, cinfo.data(), 65536 * 4, hipMemcpyHostToDevice));
    if (n_dict_words) {
        const uint64_t slots = table_slots(n_dict_words);
        std::vector<uint32_t> tab(slots, 0);
        for (size_t i = 0; i < n_dict_words; ++i) {   // dict_find's probe (kernels_train.hip), through the same hash
            uint64_t h = vpt::kCpsHashSeed;
            for (uint64_t k = woff[i]; k < woff[i + 1]; ++k) h = vpt::cps_hash_step(h, all_cps[k]);
            uint64_t s = vpt::cps_hash_finish(h, woff[i + 1] - woff[i]) & (slots - 1);
            while (tab[s]) s = (s + 1) & (slots - 1);
            tab[s] = uint32_t(i + 1);
        }
        VPT_HIP(t->d_dict_slots.resize(slots)); VPT_HIP(t->d_dict_cps.resize(all_cps.size())); VPT_HIP(t->d_dict_off.resize(woff.size()));
        VPT_HIP(hipMemcpy(t->d_dict_slots.p, tab.data(), slots * 4, hipMemcpyHostToDevice));
        VPT_HIP(hipMemcpy(t->d_dict_cps.p, all_cps.data(), all_cps.size() * 4, hipMemcpyHostToDevice));
        VPT_HIP(hipMemcpy(t->d_dict_off.p, woff.data(), woff.size() * 8, hipMemcpyHostToDevice));
        t->dict_mask = slots - 1;
    }
    *out = t.release();
    return VPT_OK;
}

void vpt_trainer_destroy(void* th) {
    vpt_trainer* t = static_cast<vpt_trainer*>(th);
    if (!t) return;
    (void)hipSetDevice(t->device);
    delete t;
}

vpt_status vpt_trainer_add_batch_device(void* th, const uint8_t* d_utf8, const uint64_t* d_byte_offsets, const uint64_t* d_out_offsets,
                                        size_t n_sentences, uint64_t total_boundaries, const uint8_t* d_labels, unsigned flags, void* hip_stream) {
    vpt_trainer* t = static_cast<vpt_trainer*>(th);
    if (!t || (n_sentences && (!d_utf8 || !d_byte_offsets || !d_out_offsets || (total_boundaries && !d_labels))))
        return fail_arg("NULL argument");
    return add_device(t, d_utf8, d_byte_offsets, d_out_offsets, n_sentences, total_boundaries, d_labels, flags, static_cast<hipStream_t>(hip_stream), false);
}

vpt_status vpt_trainer_add_batch(void* th, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences, const uint8_t* labels,
                                 unsigned flags) {
    vpt_trainer* t = static_cast<vpt_trainer*>(th);
    if (!t || !byte_offsets || (n_sentences && !utf8)) return fail_arg("NULL argument");
    if (n_sentences == 0) return VPT_OK;
    StagedBatch B;
    VPT_TRY(stage_batch(t, utf8, byte_offsets, n_sentences, labels, B));
    return add_device(t, B.d_text.p, B.d_boff.p, B.d_ooff.p, n_sentences, B.total_b, B.d_labels.p, flags, t->st, true);
}

vpt_status vpt_trainer_n_features(void* th, size_t* out) {
    vpt_trainer* t = static_cast<vpt_trainer*>(th);
    if (!t || !out) return fail_arg("NULL argument");
    VPT_HIP(hipSetDevice(t->device));
    VPT_TRY(build(t));
    *out = size_t(t->m.nd);
    return VPT_OK;
}

vpt_status vpt_trainer_csr(void* th, uint64_t* row_ptr_out, uint32_t* cols_out, void* counts_out, size_t capacity, size_t* n_rows,
                           size_t* nnz) {
    vpt_trainer* t = static_cast<vpt_trainer*>(th);
    if (!t || !n_rows || !nnz) return fail_arg("NULL argument");
    VPT_HIP(hipSetDevice(t->device));
    VPT_TRY(build(t));
    const Matrix& M = t->m;
    *n_rows = size_t(t->nrows);
    *nnz = size_t(M.nnz);
    if (!row_ptr_out && !cols_out && !counts_out) return VPT_OK;
    if (!row_ptr_out || !cols_out || !counts_out) return fail_arg("NULL argument");
    if (capacity < M.nnz) return fail_arg("capacity: smaller than the nonzeros");
    VPT_HIP(hipMemcpy(row_ptr_out, M.csr_ptr.p, (t->nrows + 1) * 8, hipMemcpyDeviceToHost));
    if (M.nnz) {
        VPT_HIP(hipMemcpy(cols_out, M.cols.p, M.nnz * 4, hipMemcpyDeviceToHost));
        VPT_HIP(hipMemcpy(counts_out, M.vals.p, M.nnz * 2, hipMemcpyDeviceToHost));
    }
    return VPT_OK;
}

vpt_status vpt_trainer_train(void* th, const void* eps_cost, int solver, uint8_t* model_out, size_t capacity, size_t* needed) {
    vpt_trainer* t = static_cast<vpt_trainer*>(th);
    if (!t || !needed || !eps_cost) return fail_arg("NULL argument");
    double ec[2];
    std::memcpy(ec, eps_cost, sizeof ec);
    const double eps = ec[0], cost = ec[1];
    const bool l1r = (t->prm.flags & VPT_TRAIN_L1R) != 0, l1lr = (t->prm.flags & VPT_TRAIN_L1R_LR) != 0;
    if (solver != 0 && solver != 2 && !(l1r && solver == 5) && !(l1lr && solver == 6))
        return fail_arg(l1lr ? (l1r ? "solver: only 0, 2, 5 and 6 are implemented" : "solver: only 0, 2 and 6 are implemented")
                             : (l1r ? "solver: only 0, 2 and 5 are implemented" : "solver: only 0 and 2 are implemented"));
    if (solver == 5 && (t->prm.flags & VPT_TRAIN_TAGS) && !(t->prm.flags & VPT_TRAIN_TAGS_L1R)) return fail_arg("solver 5: tag models are trained with solvers 0 and 2 only");
    if (solver == 6 && (t->prm.flags & VPT_TRAIN_TAGS) && !(t->prm.flags & VPT_TRAIN_TAGS_L1R_LR)) return fail_arg("solver 6: tag models are trained with solvers 0, 2 and 5 only");
    if (!(eps > 0) || !(cost > 0)) return fail_arg("eps and cost: must be positive");
    VPT_HIP(hipSetDevice(t->device));
    t->trained = false;
    VPT_TRY(build(t));
    const uint64_t nr = t->nrows, nd = t->m.nd;
    std::vector<uint8_t> lab(nr);
    if (nr) VPT_HIP(hipMemcpy(lab.data(), t->labels.p, nr, hipMemcpyDeviceToHost));
    std::vector<double> y(nr);
    uint64_t pos = 0;
    for (uint64_t i = 0; i < nr; ++i) {
        if (lab[i] > 2) return fail_arg("labels: must be 0, 1 or 2");
        y[i] = lab[i] == VPT_WORD_BOUNDARY ? 1.0 : -1.0;
        pos += lab[i] == VPT_WORD_BOUNDARY;
    }
    if (pos == 0 || pos == nr)
        return fail_arg("examples: need both WordBoundary and other boundaries");
    std::vector<uint64_t> keys(2 * nd);
    if (nd) VPT_HIP(hipMemcpy(keys.data(), t->sorted_keys.p, keys.size() * 8, hipMemcpyDeviceToHost));
    if (solver == 5 || solver == 6) {
        L1rGroups G;
        VPT_TRY(l1r_matrix_groups(t->m, nr, keys, G));
        t->w.resize(nd + 1);
        VPT_TRY((solver == 5 ? solve_l1r : solve_l1r_lr)(t, t->m, nr, y, pos, G, eps, cost, t->w.data(), &t->stats));
    } else {
        Tron T;
        VPT_TRY(T.init(t->m, t->st, nr, solver, cost));
        t->w.resize(T.n);
        VPT_TRY(T.solve(y, pos, eps, &t->stats, t->w.data()));
    }
    if (t->prm.flags & VPT_TRAIN_TAGS) {
        VPT_TRY(build_tags(t));
        VPT_TRY(solve_tags(t, eps, cost, solver));
    }
    VPT_TRY(make_model(t, keys));
    t->trained = true;
    return copy_model(t, model_out, capacity, needed);
}

vpt_status vpt_trainer_model(const void* th, uint8_t* model_out, size_t capacity, size_t* needed) {
    const vpt_trainer* t = static_cast<const vpt_trainer*>(th);
    if (!t || !needed) return fail_arg("NULL argument");
    if (!t->trained) return fail_arg("the trainer has no trained model");
    return copy_model(t, model_out, capacity, needed);
}

vpt_status vpt_trainer_weights(void* th, void* weights_out, void* bias_out, uint64_t* keys_out, size_t capacity, size_t* n_features) {
    vpt_trainer* t = static_cast<vpt_trainer*>(th);
    if (!t || !n_features) return fail_arg("NULL argument");
    if (!t->trained) return fail_arg("the trainer has no trained model");
    const uint64_t nd = t->m.nd;
    *n_features = size_t(nd);
    if (!weights_out && !bias_out && !keys_out) return VPT_OK;
    if (capacity < nd) return fail_arg("capacity: smaller than the features");
    if (weights_out) std::memcpy(weights_out, t->w.data(), nd * 8);
    if (bias_out) std::memcpy(bias_out, &t->w[nd], 8);
    if (keys_out && nd) VPT_HIP(hipMemcpy(keys_out, t->sorted_keys.p, nd * 16, hipMemcpyDeviceToHost));
    return VPT_OK;
}

vpt_status vpt_trainer_last_stats(const void* th, void* out) {
    const vpt_trainer* t = static_cast<const vpt_trainer*>(th);
    if (!t || !out) return fail_arg("NULL argument");
    if (!t->trained) return fail_arg("the trainer has no trained model");
    std::memcpy(out, &t->stats, sizeof t->stats);
    return VPT_OK;
}

vpt_status vpt_trainer_add_tagged_batch_device(void* th, const uint8_t* d_utf8, const uint64_t* d_byte_offsets, const uint64_t* d_out_offsets,
                                               size_t n_sentences, uint64_t total_boundaries, const uint8_t* d_labels, const uint32_t* d_n_tags,
                                               const uint64_t* d_tag_index, const uint64_t* d_span_offsets, const uint8_t* d_tag_bytes,
                                               uint64_t n_spans, uint64_t n_tag_bytes, unsigned flags, void* hip_stream) {
    vpt_trainer* t = tag_trainer(th, !n_sentences || (d_utf8 && d_byte_offsets && d_out_offsets && (!total_boundaries || d_labels) && d_n_tags &&
                                                      d_tag_index && d_span_offsets && (!n_tag_bytes || d_tag_bytes)));
    if (!t) return VPT_INVALID_ARGUMENT;
    return add_tagged_device(t, d_utf8, d_byte_offsets, d_out_offsets, n_sentences, total_boundaries, d_labels, d_n_tags, d_tag_index, d_span_offsets,
                             d_tag_bytes, n_spans, n_tag_bytes, flags, static_cast<hipStream_t>(hip_stream), false);
}

vpt_status vpt_trainer_add_tagged_batch(void* th, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences, const uint8_t* labels,
                                        const uint32_t* n_tags, const uint64_t* tag_index, const uint64_t* span_offsets, const uint8_t* tag_bytes,
                                        uint64_t n_spans, uint64_t n_tag_bytes, unsigned flags) {
    vpt_trainer* t = tag_trainer(th, byte_offsets && (!n_sentences || (utf8 && n_tags && tag_index && span_offsets && (!n_tag_bytes || tag_bytes))));
    if (!t) return VPT_INVALID_ARGUMENT;
    if (n_sentences == 0) return VPT_OK;
    StagedBatch B;
    VPT_TRY(stage_batch(t, utf8, byte_offsets, n_sentences, labels, B));
    const uint64_t total_chars = B.total_b + n_sentences;
    DBuf<uint8_t> d_tb;
    DBuf<uint64_t> d_ti, d_so;
    DBuf<uint32_t> d_nt;
    VPT_HIP(d_nt.resize(n_sentences)); VPT_HIP(d_ti.resize(total_chars + 1)); VPT_HIP(d_so.resize(n_spans + 1)); VPT_HIP(d_tb.resize(n_tag_bytes));
    VPT_HIP(hipMemcpyAsync(d_nt.p, n_tags, n_sentences * 4, hipMemcpyHostToDevice, t->st));
    VPT_HIP(hipMemcpyAsync(d_ti.p, tag_index, (total_chars + 1) * 8, hipMemcpyHostToDevice, t->st));
    VPT_HIP(hipMemcpyAsync(d_so.p, span_offsets, (n_spans + 1) * 8, hipMemcpyHostToDevice, t->st));
    if (n_tag_bytes) VPT_HIP(hipMemcpyAsync(d_tb.p, tag_bytes, n_tag_bytes, hipMemcpyHostToDevice, t->st));
    return add_tagged_device(t, B.d_text.p, B.d_boff.p, B.d_ooff.p, n_sentences, B.total_b, B.d_labels.p, d_nt.p, d_ti.p, d_so.p, d_tb.p, n_spans,
                             n_tag_bytes, flags, t->st, true);
}

vpt_status vpt_trainer_set_tag_dictionary(void* th, const uint8_t* surfaces_utf8, const uint64_t* surface_offsets, size_t n_surfaces,
                                          const uint32_t* n_tags, const uint64_t* span_offsets, const uint8_t* tag_bytes) {
    vpt_trainer* t = tag_trainer(th, !n_surfaces || (surfaces_utf8 && surface_offsets && n_tags && span_offsets));
    if (!t) return VPT_INVALID_ARGUMENT;
    std::map<std::string, std::vector<int32_t>> defs;
    std::vector<uint32_t> cps;
    uint64_t k = 0;
    for (size_t i = 0; i < n_surfaces; ++i) {
        const std::string at = " (surface " + std::to_string(i) + ")";
        if (surface_offsets[i + 1] <= surface_offsets[i]) return fail_arg("surface_offsets: must increase" + at);
        const uint8_t* sp = surfaces_utf8 + surface_offsets[i];
        const size_t len = size_t(surface_offsets[i + 1] - surface_offsets[i]);
        if (!vpt::decode_utf8(sp, len, cps)) return fail_arg("surfaces: invalid UTF-8" + at);
        std::vector<int32_t> tags;
        for (uint32_t j = 0; j < n_tags[i]; ++j, ++k) {
            if (span_offsets[k + 1] < span_offsets[k]) return fail_arg("span_offsets: must not decrease" + at);
            const size_t tl = size_t(span_offsets[k + 1] - span_offsets[k]);
            if (tl == 0) { tags.push_back(-1); continue; }
            if (!tag_bytes) return fail_arg("NULL argument");
            const uint8_t* b = tag_bytes + span_offsets[k];
            if (std::find(b, b + tl, uint8_t(0)) != b + tl) return fail_arg("tags: must not contain NULL" + at);
            if (!vpt::decode_utf8(b, tl, cps)) return fail_arg("tags: invalid UTF-8" + at);
            tags.push_back(t->intern_tag(std::string(reinterpret_cast<const char*>(b), tl)));
        }
        defs.emplace(std::string(reinterpret_cast<const char*>(sp), len), std::move(tags));   // the first occurrence wins (trainer.rs:231-238)
    }
    t->tag_defaults = std::move(defs);
    t->tags_built = false;
    t->tags_trained = false;
    t->trained = false;
    return VPT_OK;
}

vpt_status vpt_trainer_set_tag_path(void* th, int mode) {
    vpt_trainer* t = static_cast<vpt_trainer*>(th);
    if (!t) return fail_arg("NULL argument");
    if (mode != 0 && mode != 1) return fail_arg("mode: 0 (by size) or 1 (the global-memory solver)");
    t->tag_path_mode = mode;
    return VPT_OK;
}

vpt_status vpt_trainer_n_tag_problems(void* th, size_t* n_problems, size_t* n_models) {
    vpt_trainer* t = tag_trainer(th, n_problems != nullptr);
    if (!t) return VPT_INVALID_ARGUMENT;
    VPT_TRY(build_tags(t));
    *n_problems = t->tag_problems.size();
    if (n_models) *n_models = t->tag_models.size();
    return VPT_OK;
}

vpt_status vpt_trainer_tag_problem(void* th, size_t i, void* info_out, uint8_t* surface_out, uint8_t* cand_bytes_out, uint64_t* cand_offsets_out,
                                   uint64_t* keys_out, uint64_t* row_ptr_out, uint32_t* cols_out, uint32_t* y_out) {
    vpt_trainer* t = tag_trainer(th, info_out != nullptr);
    if (!t) return VPT_INVALID_ARGUMENT;
    VPT_TRY(build_tags(t));
    if (i >= t->tag_problems.size()) return fail_arg("i: no such tag problem");
    TagProblem& Pb = t->tag_problems[i];
    if (row_ptr_out || cols_out) {
        VPT_HIP(hipSetDevice(t->device));
        VPT_TRY(fetch_rows(t, Pb));
    }
    const std::string& tok = t->tag_models[Pb.model].token;
    vpt_tag_problem_info info{};
    info.slot = Pb.slot; info.n_classes = uint32_t(Pb.cands.size()); info.path = t->tags_trained ? Pb.path : 0; info.model = Pb.model;
    info.seconds_setup = t->tags_trained ? Pb.seconds_setup : 0; info.seconds_solve = t->tags_trained ? Pb.seconds_solve : 0;
    info.n_rows = Pb.y.size(); info.n_features = Pb.keys.size(); info.nnz = Pb.nnz; info.surface_bytes = tok.size();
    for (int32_t id : Pb.cands) info.cand_bytes += t->tag_strings[size_t(id)].size();
    std::memcpy(info_out, &info, sizeof info);
    if (surface_out) std::memcpy(surface_out, tok.data(), tok.size());
    uint64_t at = 0;
    for (size_t c = 0; c < Pb.cands.size(); ++c) {
        const std::string& tg = t->tag_strings[size_t(Pb.cands[c])];
        if (cand_offsets_out) cand_offsets_out[c] = at;
        if (cand_bytes_out) std::memcpy(cand_bytes_out + at, tg.data(), tg.size());
        at += tg.size();
    }
    if (cand_offsets_out) cand_offsets_out[Pb.cands.size()] = at;
    if (keys_out)
        for (size_t j = 0; j < Pb.keys.size(); ++j) { keys_out[2 * j] = uint64_t(Pb.keys[j]); keys_out[2 * j + 1] = uint64_t(Pb.keys[j] >> 64); }
    if (row_ptr_out) for (size_t r = 0; r < Pb.rp.size(); ++r) row_ptr_out[r] = Pb.rp[r];
    if (cols_out && !Pb.cols.empty()) std::memcpy(cols_out, Pb.cols.data(), Pb.cols.size() * 4);
    if (y_out && !Pb.y.empty()) std::memcpy(y_out, Pb.y.data(), Pb.y.size() * 4);
    return VPT_OK;
}

vpt_status vpt_trainer_tag_weights(void* th, size_t i, void* weights_out, size_t capacity, void* stats_out) {
    vpt_trainer* t = static_cast<vpt_trainer*>(th);
    if (!t) return fail_arg("NULL argument");
    if (!t->trained || !t->tags_trained) return fail_arg("the trainer has no trained tag models");
    if (i >= t->tag_problems.size()) return fail_arg("i: no such tag problem");
    const TagProblem& Pb = t->tag_problems[i];
    if (weights_out) {
        if (capacity < Pb.w.size()) return fail_arg("capacity: smaller than classes * (features + 1)");
        std::memcpy(weights_out, Pb.w.data(), Pb.w.size() * 8);
    }
    if (stats_out) std::memcpy(stats_out, Pb.stats.data(), Pb.stats.size() * sizeof(vpt_train_stats));
    return VPT_OK;
}

vpt_status vpt_trainer_tag_summary(const void* th, void* out) {
    const vpt_trainer* t = static_cast<const vpt_trainer*>(th);
    if (!t || !out) return fail_arg("NULL argument");
    if (!t->trained || !t->tags_trained) return fail_arg("the trainer has no trained tag models");
    std::memcpy(out, &t->tag_summary, sizeof t->tag_summary);
    return VPT_OK;
}

}  // extern "C"
