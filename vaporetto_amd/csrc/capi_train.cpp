// C ABI of libvaporetto_hip.so, boundary-model training: Trainer (vaporetto/src/trainer.rs) with the liblinear TRON solvers 0 and 2.
//
// The vpt_trainer handle keeps every example's feature keys and label on the device (kernels_train.hip); feature ids, the CSR and CSC
// copies of the design matrix are made when they are first needed after an add, and the TRON / CG loop runs here, on the host, over
// device vectors, reading back a scalar per reduction.  TRON is the one of the liblinear that scikit-learn bundles (tron.cpp: CG without
// a preconditioner, eps_cg = 0.1); the reference's newer liblinear preconditions its CG and reaches the same optimum by another path, so
// weights agree with it only to the stopping tolerance.  Quantisation and the model layout are trainer.rs:352-487; the encoder mirrors
// vaporetto_amd/modelfmt.encode_model (model.rs:99-104).
#include "capi_internal.hpp"

#include <cmath>
#include <map>
#include <memory>
#include <set>

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

void put_utf8(std::string& s, uint32_t c) {
    if (c < 0x80) s += char(c);
    else if (c < 0x800) { s += char(0xC0 | (c >> 6)); s += char(0x80 | (c & 0x3F)); }
    else if (c < 0x10000) { s += char(0xE0 | (c >> 12)); s += char(0x80 | ((c >> 6) & 0x3F)); s += char(0x80 | (c & 0x3F)); }
    else { s += char(0xF0 | (c >> 18)); s += char(0x80 | ((c >> 12) & 0x3F)); s += char(0x80 | ((c >> 6) & 0x3F)); s += char(0x80 | (c & 0x3F)); }
}
// valid UTF-8 -> scalar values (false if invalid)
bool decode_utf8(const uint8_t* s, size_t len, std::vector<uint32_t>& out) {
    out.clear();
    for (size_t i = 0; i < len;) {
        const uint8_t b = s[i];
        uint32_t c, k;
        if (b < 0x80) { c = b; k = 0; }
        else if ((b & 0xE0) == 0xC0) { c = b & 0x1F; k = 1; }
        else if ((b & 0xF0) == 0xE0) { c = b & 0x0F; k = 2; }
        else if ((b & 0xF8) == 0xF0) { c = b & 0x07; k = 3; }
        else return false;
        for (uint32_t j = 1; j <= k; ++j) {
            if (i + j >= len || (s[i + j] & 0xC0) != 0x80) return false;
            c = (c << 6) | (s[i + j] & 0x3F);
        }
        if (c > 0x10FFFF) return false;
        out.push_back(c);
        i += k + 1;
    }
    return true;
}

uint64_t mix64h(uint64_t x) {   // kernels_train.hip's mix64
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
    return x ^ (x >> 33);
}

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
    // the design matrix (valid while `built`)
    bool built = false;
    uint64_t nd = 0, nnz = 0;
    DBuf<uint64_t> sorted_keys, csr_ptr, cptr;
    DBuf<uint32_t> cols, crow;
    DBuf<uint16_t> vals, cval;
    std::vector<std::unique_ptr<XtvLevel>> levels;
    // the last training
    std::vector<double> w;        // nd weights + the bias
    std::vector<uint8_t> model;
    vpt_train_stats stats{};
    bool trained = false;
    ~vpt_trainer() { if (st) (void)hipStreamDestroy(st); }
};

namespace {

constexpr const char* kIA = "InvalidArgumentError: ";

vpt_status build(vpt_trainer* t) {
    if (t->built) return VPT_OK;
    hipStream_t st = t->st;
    const uint64_t nnz = t->nnz_occ, nrows = t->nrows;
    if (nnz >= (uint64_t(1) << 32) || nrows >= (uint64_t(1) << 32))
        return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "examples: at most 2^32 - 1 boundaries and feature occurrences");
    t->levels.clear();
    // ---- representatives of the distinct keys
    uint64_t slots = 2;
    while (slots < 2 * nnz) slots <<= 1;
    DBuf<uint64_t> table, rep, pos, slot, scratch;
    DBuf<uint32_t> flag;
    VPT_HIP(table.resize(slots));
    VPT_HIP(hipMemsetAsync(table.p, 0, slots * 8, st));
    VPT_HIP(rep.resize(nnz)); VPT_HIP(flag.resize(nnz)); VPT_HIP(pos.resize(nnz + 1)); VPT_HIP(slot.resize(nnz));
    VPT_HIP(scratch.resize(vpt::train_scan_scratch(std::max<uint64_t>({nnz, nrows, vpt::train_radix_scratch(nnz)})) + 1));
    VPT_HIP(vpt::train_insert(t->keys.p, nnz, table.p, slots - 1, rep.p, flag.p, st));
    VPT_HIP(vpt::train_scan_u32(flag.p, nnz, pos.p, scratch.p, st));
    uint64_t nd = 0;
    VPT_HIP(hipMemcpyAsync(&nd, pos.p + nnz, 8, hipMemcpyDeviceToHost, st));
    VPT_HIP(hipStreamSynchronize(st));
    table.reset(); flag.reset();
    DBuf<uint64_t> dkeys;
    VPT_HIP(dkeys.resize(2 * nd));
    VPT_HIP(vpt::train_compact(t->keys.p, rep.p, pos.p, nnz, dkeys.p, slot.p, st));
    // ---- the distinct keys sorted: 16 passes of 8 bits over the four 32-bit words, least significant first
    DBuf<uint32_t> order, tmp;
    DBuf<uint64_t> hist, hist_scan;
    const uint64_t big = std::max(nd, nnz);
    VPT_HIP(order.resize(big)); VPT_HIP(tmp.resize(big));
    VPT_HIP(hist.resize(vpt::train_radix_scratch(big))); VPT_HIP(hist_scan.resize(vpt::train_radix_scratch(big) + 1));
    uint32_t ws[16];
    for (uint32_t k = 0; k < 16; ++k) ws[k] = ((k / 4) << 8) | (8 * (k % 4));
    VPT_HIP(vpt::train_radix_sort(reinterpret_cast<const uint32_t*>(dkeys.p), 4, ws, 16, nd, order.p, tmp.p, hist.p, hist_scan.p, scratch.p, st));
    DBuf<uint32_t> col_of, ids;
    VPT_HIP(col_of.resize(nd)); VPT_HIP(ids.resize(nnz)); VPT_HIP(t->sorted_keys.resize(2 * nd));
    VPT_HIP(vpt::train_ids(order.p, nd, col_of.p, rep.p, slot.p, nnz, ids.p, dkeys.p, t->sorted_keys.p, st));
    VPT_HIP(hipStreamSynchronize(st));
    rep.reset(); slot.reset(); dkeys.reset(); col_of.reset();
    // ---- CSR: rows in corpus order, ids sorted, duplicates merged into counts
    DBuf<uint64_t> row_off;
    DBuf<uint32_t> merged, rows;
    VPT_HIP(row_off.resize(nrows + 1)); VPT_HIP(merged.resize(nrows)); VPT_HIP(t->csr_ptr.resize(nrows + 1));
    VPT_HIP(vpt::train_scan_u32(t->row_cnt.p, nrows, row_off.p, scratch.p, st));
    VPT_HIP(vpt::train_row_sort(ids.p, row_off.p, nrows, merged.p, st));
    VPT_HIP(vpt::train_scan_u32(merged.p, nrows, t->csr_ptr.p, scratch.p, st));
    uint64_t nz = 0;
    VPT_HIP(hipMemcpyAsync(&nz, t->csr_ptr.p + nrows, 8, hipMemcpyDeviceToHost, st));
    VPT_HIP(hipStreamSynchronize(st));
    DBuf<uint32_t> status;
    VPT_HIP(status.resize(1));
    VPT_HIP(hipMemsetAsync(status.p, 0, 4, st));
    VPT_HIP(t->cols.resize(nz)); VPT_HIP(t->vals.resize(nz)); VPT_HIP(rows.resize(nz));
    VPT_HIP(vpt::train_row_merge(ids.p, row_off.p, t->csr_ptr.p, nrows, t->cols.p, t->vals.p, rows.p, status.p, st));
    uint32_t bad = 0;
    VPT_HIP(hipMemcpyAsync(&bad, status.p, 4, hipMemcpyDeviceToHost, st));
    VPT_HIP(hipStreamSynchronize(st));
    if (bad) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "examples: a feature occurs more than 65535 times at one boundary");
    VPT_HIP(hipStreamSynchronize(st));
    ids.reset(); row_off.reset(); merged.reset();
    // ---- CSC: the nonzeros stably sorted by column (rows ascend within a column)
    uint32_t cpasses = 1;
    while (cpasses < 4 && nd > (uint64_t(1) << (8 * cpasses))) ++cpasses;
    for (uint32_t k = 0; k < cpasses; ++k) ws[k] = 8 * k;
    VPT_HIP(vpt::train_radix_sort(t->cols.p, 1, ws, cpasses, nz, order.p, tmp.p, hist.p, hist_scan.p, scratch.p, st));
    VPT_HIP(t->crow.resize(nz)); VPT_HIP(t->cval.resize(nz)); VPT_HIP(t->cptr.resize(nd + 1));
    VPT_HIP(vpt::train_csc_fill(order.p, t->cols.p, t->vals.p, rows.p, nz, t->crow.p, t->cval.p, t->cptr.p, st));
    VPT_HIP(hipMemcpyAsync(t->cptr.p + nd, &nz, 8, hipMemcpyHostToDevice, st));
    // ---- the segments of Xᵀv, level by level, until a column is one segment
    DBuf<uint64_t> cnt;
    VPT_HIP(cnt.resize(nd));
    const uint64_t* ptr = t->cptr.p;
    for (;;) {
        t->levels.emplace_back(new XtvLevel());
        XtvLevel& L = *t->levels.back();
        L.ptr = ptr;
        VPT_HIP(L.nptr.resize(nd + 1));
        VPT_HIP(vpt::train_seg_count(ptr, nd, cnt.p, st));
        VPT_HIP(vpt::train_scan_u64(cnt.p, nd, L.nptr.p, scratch.p, st));
        VPT_HIP(hipMemcpyAsync(&L.nseg, L.nptr.p + nd, 8, hipMemcpyDeviceToHost, st));
        VPT_HIP(hipStreamSynchronize(st));
        VPT_HIP(L.seg_col.resize(L.nseg)); VPT_HIP(L.out.resize(L.nseg));
        VPT_HIP(vpt::train_seg_col(L.nptr.p, nd, L.seg_col.p, st));
        ptr = L.nptr.p;
        if (L.nseg == nd) break;
    }
    VPT_HIP(hipStreamSynchronize(st));
    t->nd = nd;
    t->nnz = nz;
    t->built = true;
    return VPT_OK;
}

// TRON (liblinear tron.cpp as bundled by scikit-learn) for l2r_lr_fun (solver 0) / l2r_l2_svc_fun (solver 2), linear.cpp
struct Tron {
    vpt_trainer* t;
    hipStream_t st;
    uint64_t n, nr;
    int solver;
    double c;
    DBuf<double> w, w_new, g, s, r, d, Hd, y, z, zt, gz, D, loss, part0, part1;
    hipError_t err = hipSuccess;

    // the fixed-shape sum of a[i] * b[i] (b NULL: a[i]), left on the device; returns where
    const double* reduce_dev(const double* a, const double* b, uint64_t len) {
        double* in_out[2] = {part0.p, part1.p};
        uint64_t m = vpt::train_dot_partials(len);
        if (err == hipSuccess) err = vpt::train_dot(a, b, len, in_out[0], st);
        int k = 0;
        while (m > 1 && err == hipSuccess) {
            err = vpt::train_dot(in_out[k], nullptr, m, in_out[k ^ 1], st);
            m = vpt::train_dot_partials(m);
            k ^= 1;
        }
        return in_out[k];
    }
    double dot(const double* a, const double* b, uint64_t len) {
        if (len == 0) return 0;
        const double* r_ = reduce_dev(a, b, len);
        double v = 0;
        if (err == hipSuccess) err = hipMemcpyAsync(&v, r_, 8, hipMemcpyDeviceToHost, st);
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        return v;
    }
    double nrm2(const double* a) { return std::sqrt(dot(a, a, n)); }
    void axpy(double a, const double* x, double* y_) { if (err == hipSuccess) err = vpt::train_axpy(n, a, x, y_, st); }
    // out = a + Xᵀu
    void add_xtv(const double* a, const double* u, double* out) {
        const double* in = nullptr;
        for (auto& Lp : t->levels) {
            XtvLevel& L = *Lp;
            if (err == hipSuccess)
                err = vpt::train_xtv_level(L.ptr, L.nptr.p, L.seg_col.p, L.nseg, in, in ? nullptr : t->crow.p, t->cval.p, u, L.out.p, st);
            in = L.out.p;
        }
        const double* bias = reduce_dev(u, nullptr, nr);
        if (err == hipSuccess) err = vpt::train_add(n, a, in, bias, out, st);
    }
    double fun(const double* x) {
        if (err == hipSuccess) err = vpt::train_xv(t->csr_ptr.p, t->cols.p, t->vals.p, nr, x, t->nd, z.p, st);
        if (err == hipSuccess) err = vpt::train_loss(nr, z.p, y.p, c, solver, loss.p, st);
        const double reg = dot(x, x, n) / 2.0;
        return reg + dot(loss.p, nullptr, nr);
    }
    void grad(const double* x, double* out) {
        if (err == hipSuccess) err = vpt::train_grad_rows(nr, z.p, y.p, c, solver, gz.p, D.p, st);
        add_xtv(x, gz.p, out);
    }
    void hv(const double* v, double* out) {
        if (err == hipSuccess) err = vpt::train_xv(t->csr_ptr.p, t->cols.p, t->vals.p, nr, v, t->nd, zt.p, st);
        if (err == hipSuccess) err = vpt::train_scale_rows(nr, D.p, zt.p, st);
        add_xtv(v, zt.p, out);
    }
    int trcg(double delta) {
        if (err == hipSuccess) err = hipMemsetAsync(s.p, 0, n * 8, st);
        if (err == hipSuccess) err = hipMemsetAsync(r.p, 0, n * 8, st);
        axpy(-1.0, g.p, r.p);
        if (err == hipSuccess) err = hipMemcpyAsync(d.p, r.p, n * 8, hipMemcpyDeviceToDevice, st);
        const double cgtol = 0.1 * nrm2(g.p);
        int cg_iter = 0;
        double rTr = dot(r.p, r.p, n);
        while (err == hipSuccess) {
            if (nrm2(r.p) <= cgtol) break;
            cg_iter++;
            hv(d.p, Hd.p);
            double alpha = rTr / dot(d.p, Hd.p, n);
            axpy(alpha, d.p, s.p);
            if (nrm2(s.p) > delta) {
                alpha = -alpha;
                axpy(alpha, d.p, s.p);
                const double std_ = dot(s.p, d.p, n), sts = dot(s.p, s.p, n), dtd = dot(d.p, d.p, n), dsq = delta * delta;
                const double rad = std::sqrt(std_ * std_ + dtd * (dsq - sts));
                alpha = std_ >= 0 ? (dsq - sts) / (std_ + rad) : (rad - std_) / dtd;
                axpy(alpha, d.p, s.p);
                alpha = -alpha;
                axpy(alpha, Hd.p, r.p);
                break;
            }
            alpha = -alpha;
            axpy(alpha, Hd.p, r.p);
            const double rnew = dot(r.p, r.p, n);
            const double beta = rnew / rTr;
            if (err == hipSuccess) err = vpt::train_xpby(n, r.p, beta, d.p, st);
            rTr = rnew;
        }
        return cg_iter;
    }
    // returns the number of iterations
    void run(double eps, vpt_train_stats* stats) {
        const double eta0 = 1e-4, eta1 = 0.25, eta2 = 0.75, sigma1 = 0.25, sigma2 = 0.5, sigma3 = 4;
        const int max_iter = 1000;
        if (err == hipSuccess) err = hipMemsetAsync(w.p, 0, n * 8, st);
        double f = fun(w.p);
        grad(w.p, g.p);
        double delta = nrm2(g.p);
        const double gnorm1 = delta;
        double gnorm = gnorm1;
        bool search = !(gnorm <= eps * gnorm1);
        int iter = 1, cg_total = 0;
        while (iter <= max_iter && search && err == hipSuccess) {
            const int cg_iter = trcg(delta);
            cg_total += cg_iter;
            if (err == hipSuccess) err = hipMemcpyAsync(w_new.p, w.p, n * 8, hipMemcpyDeviceToDevice, st);
            axpy(1.0, s.p, w_new.p);
            const double gs = dot(g.p, s.p, n);
            const double prered = -0.5 * (gs - dot(s.p, r.p, n));
            const double fnew = fun(w_new.p);
            const double actred = f - fnew;
            const double snorm = nrm2(s.p);
            if (iter == 1) delta = std::min(delta, snorm);
            const double alpha = (fnew - f - gs <= 0) ? sigma3 : std::max(sigma1, -0.5 * (gs / (fnew - f - gs)));
            if (actred < eta0 * prered) delta = std::min(std::max(alpha, sigma1) * snorm, sigma2 * delta);
            else if (actred < eta1 * prered) delta = std::max(sigma1 * delta, std::min(alpha * snorm, sigma2 * delta));
            else if (actred < eta2 * prered) delta = std::max(sigma1 * delta, std::min(alpha * snorm, sigma3 * delta));
            else delta = std::max(delta, std::min(alpha * snorm, sigma3 * delta));
            if (actred > eta0 * prered) {
                iter++;
                if (err == hipSuccess) err = hipMemcpyAsync(w.p, w_new.p, n * 8, hipMemcpyDeviceToDevice, st);
                f = fnew;
                grad(w.p, g.p);
                gnorm = nrm2(g.p);
                if (gnorm <= eps * gnorm1) break;
            }
            if (f < -1.0e+32) break;
            if (std::fabs(actred) <= 0 && prered <= 0) break;
            if (std::fabs(actred) <= 1.0e-12 * std::fabs(f) && std::fabs(prered) <= 1.0e-12 * std::fabs(f)) break;
        }
        stats->iterations = uint32_t(iter - 1);
        stats->cg_steps = uint32_t(cg_total);
        stats->gnorm0 = gnorm1;
        stats->gnorm = gnorm;
        stats->objective = f;
    }
};

// trainer.rs:352-487: quantisation and the model's layout, then Model::to_vec
vpt_status make_model(vpt_trainer* t, const std::vector<uint64_t>& keys) {
    const uint64_t nd = t->nd;
    const double bias = t->w[nd];
    double wmax = std::fabs(bias);
    for (uint64_t j = 0; j < nd; ++j) wmax = std::max(wmax, std::fabs(t->w[j]));
    const double m = wmax / double((1 << 15) - 1);
    if (m == 0.) return fail(VPT_INVALID_MODEL, "InvalidModelError: all weights are zero");
    const int32_t qbias = int32_t(bias / m);   // to_int_unchecked: truncation toward zero
    const int charw = int(t->prm.charw);
    std::map<std::string, std::vector<int32_t>> cw, tw;
    std::vector<int32_t> dw(3 * size_t(t->prm.dictn), 0);
    static const int sh[5] = {99, 78, 57, 36, 15};
    for (uint64_t j = 0; j < nd; ++j) {
        const int32_t q = int32_t(t->w[j] / m);
        if (q == 0) continue;
        const unsigned __int128 v = ((unsigned __int128)keys[2 * j + 1] << 64) | keys[2 * j];
        const uint32_t kind = uint32_t(v >> 120) & 3u;
        if (kind == 2) {
            const uint32_t cls = uint32_t(v >> 99) & 0x1FFFFFu, where = uint32_t(v >> 78) & 0x1FFFFFu;
            dw[3 * (cls - 1) + where] = q;
            continue;
        }
        const int len = int(v >> 5) & 7, rel = int(v & 31u) - 16;
        std::string ng;
        for (int k = 0; k < len; ++k) {
            const uint32_t c = uint32_t(v >> sh[k]) & 0x1FFFFFu;
            if (kind == 0) put_utf8(ng, c); else ng += char(c);
        }
        // the type n-grams use the char window too (trainer.rs:433-440)
        const int posn = charw - len - rel;
        auto& mp = kind == 0 ? cw : tw;
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
    e.uvar(0);   // no tag models
    t->model = std::move(e.b);
    return VPT_OK;
}

vpt_status add_device(vpt_trainer* t, const uint8_t* d_utf8, const uint64_t* d_boff, const uint64_t* d_ooff, size_t n, uint64_t total_b,
                      const uint8_t* d_labels, unsigned flags, hipStream_t st) {
    if ((flags & ~unsigned(VPT_FLAG_KYTEA_FULLWIDTH)) != 0) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "flags: only VPT_FLAG_KYTEA_FULLWIDTH");
    if (n == 0) return VPT_OK;
    VPT_HIP(hipSetDevice(t->device));
    // the caller's stream, then ours: the examples are appended in call order
    VPT_HIP(hipStreamSynchronize(st));
    st = t->st;
    const uint64_t total_chars = total_b + n;
    DBuf<uint32_t> cps, status, counts;
    DBuf<uint64_t> off, scratch;
    VPT_HIP(cps.resize(total_chars)); VPT_HIP(status.resize(1)); VPT_HIP(counts.resize(total_b)); VPT_HIP(off.resize(total_b + 1));
    VPT_HIP(scratch.resize(vpt::train_scan_scratch(total_b) + 1));
    VPT_HIP(hipMemsetAsync(status.p, 0, 4, st));
    const bool fw = (flags & VPT_FLAG_KYTEA_FULLWIDTH) != 0;
    VPT_HIP(vpt::launch_decode_chars(d_utf8, d_boff, d_ooff, n, total_chars, fw ? t->d_cinfo.p : nullptr, cps.p, nullptr, status.p, st, fw));
    uint32_t bad = 0;
    VPT_HIP(hipMemcpyAsync(&bad, status.p, 4, hipMemcpyDeviceToHost, st));
    VPT_HIP(hipStreamSynchronize(st));
    if (bad) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "out_offsets: do not match the text");
    vpt::TrainFeatParams P{};
    P.cps = cps.p; P.ooff = d_ooff; P.n_sent = n; P.total_b = total_b;
    P.charw = t->prm.charw; P.charn = t->prm.charn; P.typew = t->prm.typew; P.typen = t->prm.typen; P.dictn = t->prm.dictn;
    P.dict_maxlen = t->dict_maxlen; P.dict_slots = t->d_dict_slots.p; P.dict_mask = t->dict_mask; P.dict_cps = t->d_dict_cps.p;
    P.dict_off = t->d_dict_off.p;
    P.counts = counts.p;
    VPT_HIP(vpt::train_features(P, false, st));
    VPT_HIP(vpt::train_scan_u32(counts.p, total_b, off.p, scratch.p, st));
    uint64_t add = 0;
    VPT_HIP(hipMemcpyAsync(&add, off.p + total_b, 8, hipMemcpyDeviceToHost, st));
    VPT_HIP(hipStreamSynchronize(st));
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

}  // namespace

extern "C" {

vpt_status vpt_trainer_create(const uint32_t* params_words, const uint8_t* dict_utf8, const uint64_t* dict_offsets, size_t n_dict_words,
                              int device_id, void** out) {
    const vpt_train_params* params = reinterpret_cast<const vpt_train_params*>(params_words);
    if (!params || !out || (n_dict_words && (!dict_utf8 || !dict_offsets))) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "NULL argument");
    *out = nullptr;
    const vpt_train_params& p = *params;
    if (p.charn < 1 || p.charn > 5) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "charn: must be between 1 and 5");
    if (p.typen < 1 || p.typen > 5) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "typen: must be between 1 and 5");
    if (p.charw > 16) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "charw: must be at most 16");
    if (p.typew > 16) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "typew: must be at most 16");
    if (p.typew > p.charw) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "typew: must not exceed charw (type weights use the char window)");
    if (p.flags != 0) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "flags: must be 0");
    if (n_dict_words && (p.dictn < 1 || p.dictn > 0x1FFFFF)) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "dictn: must be at least 1 with a dictionary");
    std::unique_ptr<vpt_trainer> t(new (std::nothrow) vpt_trainer());
    if (!t) return fail(VPT_RUNTIME_ERROR, "out of host memory");
    t->prm = p;
    std::vector<uint32_t> all_cps, cps;
    std::vector<uint64_t> woff{0};
    std::set<std::string> seen;
    for (size_t i = 0; i < n_dict_words; ++i) {
        if (dict_offsets[i + 1] < dict_offsets[i]) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "dict_offsets: must be non-decreasing");
        const uint8_t* s = dict_utf8 + dict_offsets[i];
        const size_t len = size_t(dict_offsets[i + 1] - dict_offsets[i]);
        if (len == 0) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "dict_words: must not contain an empty word (word " + std::to_string(i) + ")");
        if (!decode_utf8(s, len, cps)) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "dict_words: invalid UTF-8 (word " + std::to_string(i) + ")");
        std::string w(reinterpret_cast<const char*>(s), len);
        if (!seen.insert(w).second) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "dict_words: duplicate word (word " + std::to_string(i) + ")");
        t->dict_words.push_back(w);
        t->dict_len.push_back(uint32_t(cps.size()));
        t->dict_maxlen = std::max(t->dict_maxlen, uint32_t(cps.size()));
        all_cps.insert(all_cps.end(), cps.begin(), cps.end());
        woff.push_back(all_cps.size());
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(VPT_RUNTIME_ERROR, "no HIP device available (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= n_dev) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "device_id: no such device");
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
        uint64_t slots = 2;
        while (slots < 2 * n_dict_words) slots <<= 1;
        std::vector<uint32_t> tab(slots, 0);
        for (size_t i = 0; i < n_dict_words; ++i) {
            uint64_t h = 0xCBF29CE484222325ull;
            for (uint64_t k = woff[i]; k < woff[i + 1]; ++k) h = (h ^ all_cps[k]) * 0x100000001B3ull;
            uint64_t s = mix64h(h ^ (woff[i + 1] - woff[i])) & (slots - 1);
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
        return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "NULL argument");
    return add_device(t, d_utf8, d_byte_offsets, d_out_offsets, n_sentences, total_boundaries, d_labels, flags, static_cast<hipStream_t>(hip_stream));
}

vpt_status vpt_trainer_add_batch(void* th, const uint8_t* utf8, const uint64_t* byte_offsets, size_t n_sentences, const uint8_t* labels,
                                 unsigned flags) {
    vpt_trainer* t = static_cast<vpt_trainer*>(th);
    if (!t || !byte_offsets || (n_sentences && !utf8)) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "NULL argument");
    if (n_sentences == 0) return VPT_OK;
    std::vector<uint64_t> ooff(n_sentences + 1);
    vpt_status s = vpt_count_boundaries(utf8, byte_offsets, n_sentences, ooff.data());
    if (s != VPT_OK) return s;
    const uint64_t total_b = ooff[n_sentences];
    if (total_b && !labels) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "NULL argument");
    for (uint64_t b = 0; b < total_b; ++b)
        if (labels[b] > 2) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "labels: must be 0, 1 or 2");
    VPT_HIP(hipSetDevice(t->device));
    const uint64_t b0 = byte_offsets[0], nbytes = byte_offsets[n_sentences] - b0;
    std::vector<uint64_t> boff(byte_offsets, byte_offsets + n_sentences + 1);
    for (auto& x : boff) x -= b0;
    DBuf<uint8_t> d_text, d_labels;
    DBuf<uint64_t> d_boff, d_ooff;
    VPT_HIP(d_text.resize(nbytes + 64)); VPT_HIP(d_labels.resize(total_b)); VPT_HIP(d_boff.resize(n_sentences + 1)); VPT_HIP(d_ooff.resize(n_sentences + 1));
    VPT_HIP(hipMemsetAsync(d_text.p, 0, nbytes + 64, t->st));
    VPT_HIP(hipMemcpyAsync(d_text.p, utf8 + b0, nbytes, hipMemcpyHostToDevice, t->st));
    if (total_b) VPT_HIP(hipMemcpyAsync(d_labels.p, labels, total_b, hipMemcpyHostToDevice, t->st));
    VPT_HIP(hipMemcpyAsync(d_boff.p, boff.data(), boff.size() * 8, hipMemcpyHostToDevice, t->st));
    VPT_HIP(hipMemcpyAsync(d_ooff.p, ooff.data(), ooff.size() * 8, hipMemcpyHostToDevice, t->st));
    return add_device(t, d_text.p, d_boff.p, d_ooff.p, n_sentences, total_b, d_labels.p, flags, t->st);
}

vpt_status vpt_trainer_n_features(void* th, size_t* out) {
    vpt_trainer* t = static_cast<vpt_trainer*>(th);
    if (!t || !out) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "NULL argument");
    VPT_HIP(hipSetDevice(t->device));
    vpt_status s = build(t);
    if (s != VPT_OK) return s;
    *out = size_t(t->nd);
    return VPT_OK;
}

vpt_status vpt_trainer_csr(void* th, uint64_t* row_ptr_out, uint32_t* cols_out, void* counts_out, size_t capacity, size_t* n_rows,
                           size_t* nnz) {
    vpt_trainer* t = static_cast<vpt_trainer*>(th);
    if (!t || !n_rows || !nnz) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "NULL argument");
    VPT_HIP(hipSetDevice(t->device));
    vpt_status s = build(t);
    if (s != VPT_OK) return s;
    *n_rows = size_t(t->nrows);
    *nnz = size_t(t->nnz);
    if (!row_ptr_out && !cols_out && !counts_out) return VPT_OK;
    if (!row_ptr_out || !cols_out || !counts_out) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "NULL argument");
    if (capacity < t->nnz) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "capacity: smaller than the nonzeros");
    VPT_HIP(hipMemcpy(row_ptr_out, t->csr_ptr.p, (t->nrows + 1) * 8, hipMemcpyDeviceToHost));
    if (t->nnz) {
        VPT_HIP(hipMemcpy(cols_out, t->cols.p, t->nnz * 4, hipMemcpyDeviceToHost));
        VPT_HIP(hipMemcpy(counts_out, t->vals.p, t->nnz * 2, hipMemcpyDeviceToHost));
    }
    return VPT_OK;
}

vpt_status vpt_trainer_train(void* th, const void* eps_cost, int solver, uint8_t* model_out, size_t capacity, size_t* needed) {
    vpt_trainer* t = static_cast<vpt_trainer*>(th);
    if (!t || !needed || !eps_cost) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "NULL argument");
    double ec[2];
    std::memcpy(ec, eps_cost, sizeof ec);
    const double eps = ec[0], cost = ec[1];
    if (solver != 0 && solver != 2) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "solver: only 0 and 2 are implemented");
    if (!(eps > 0) || !(cost > 0)) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "eps and cost: must be positive");
    VPT_HIP(hipSetDevice(t->device));
    t->trained = false;
    vpt_status s = build(t);
    if (s != VPT_OK) return s;
    const uint64_t nr = t->nrows;
    std::vector<uint8_t> lab(nr);
    if (nr) VPT_HIP(hipMemcpy(lab.data(), t->labels.p, nr, hipMemcpyDeviceToHost));
    std::vector<double> y(nr);
    uint64_t pos = 0;
    for (uint64_t i = 0; i < nr; ++i) {
        if (lab[i] > 2) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "labels: must be 0, 1 or 2");
        y[i] = lab[i] == VPT_WORD_BOUNDARY ? 1.0 : -1.0;
        pos += lab[i] == VPT_WORD_BOUNDARY;
    }
    if (pos == 0 || pos == nr)
        return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "examples: need both WordBoundary and other boundaries");
    Tron T;
    T.t = t; T.st = t->st; T.n = t->nd + 1; T.nr = nr; T.solver = solver; T.c = cost;
    for (DBuf<double>* b : {&T.w, &T.w_new, &T.g, &T.s, &T.r, &T.d, &T.Hd}) VPT_HIP(b->resize(T.n));
    for (DBuf<double>* b : {&T.y, &T.z, &T.zt, &T.gz, &T.D, &T.loss}) VPT_HIP(b->resize(nr));
    VPT_HIP(T.part0.resize(vpt::train_dot_partials(std::max(T.n, nr)))); VPT_HIP(T.part1.resize(vpt::train_dot_partials(std::max(T.n, nr))));
    VPT_HIP(hipMemcpy(T.y.p, y.data(), nr * 8, hipMemcpyHostToDevice));
    // liblinear's primal tolerance (linear.cpp train_one): eps * max(min(pos, neg), 1) / l
    const double tol = eps * double(std::max<uint64_t>(std::min(pos, nr - pos), 1)) / double(nr);
    T.run(tol, &t->stats);
    VPT_HIP(T.err);
    t->w.resize(T.n);
    VPT_HIP(hipMemcpy(t->w.data(), T.w.p, T.n * 8, hipMemcpyDeviceToHost));
    std::vector<uint64_t> keys(2 * t->nd);
    if (t->nd) VPT_HIP(hipMemcpy(keys.data(), t->sorted_keys.p, keys.size() * 8, hipMemcpyDeviceToHost));
    if ((s = make_model(t, keys)) != VPT_OK) return s;
    t->trained = true;
    *needed = t->model.size();
    if (model_out) {
        if (capacity < t->model.size()) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "capacity: smaller than the model");
        std::memcpy(model_out, t->model.data(), t->model.size());
    }
    return VPT_OK;
}

vpt_status vpt_trainer_model(const void* th, uint8_t* model_out, size_t capacity, size_t* needed) {
    const vpt_trainer* t = static_cast<const vpt_trainer*>(th);
    if (!t || !needed) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "NULL argument");
    if (!t->trained) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "the trainer has no trained model");
    *needed = t->model.size();
    if (model_out) {
        if (capacity < t->model.size()) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "capacity: smaller than the model");
        std::memcpy(model_out, t->model.data(), t->model.size());
    }
    return VPT_OK;
}

vpt_status vpt_trainer_weights(void* th, void* weights_out, void* bias_out, uint64_t* keys_out, size_t capacity, size_t* n_features) {
    vpt_trainer* t = static_cast<vpt_trainer*>(th);
    if (!t || !n_features) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "NULL argument");
    if (!t->trained) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "the trainer has no trained model");
    *n_features = size_t(t->nd);
    if (!weights_out && !bias_out && !keys_out) return VPT_OK;
    if (capacity < t->nd) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "capacity: smaller than the features");
    if (weights_out) std::memcpy(weights_out, t->w.data(), t->nd * 8);
    if (bias_out) std::memcpy(bias_out, &t->w[t->nd], 8);
    if (keys_out && t->nd) VPT_HIP(hipMemcpy(keys_out, t->sorted_keys.p, t->nd * 16, hipMemcpyDeviceToHost));
    return VPT_OK;
}

vpt_status vpt_trainer_last_stats(const void* th, void* out) {
    const vpt_trainer* t = static_cast<const vpt_trainer*>(th);
    if (!t || !out) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "NULL argument");
    if (!t->trained) return fail(VPT_INVALID_ARGUMENT, std::string(kIA) + "the trainer has no trained model");
    std::memcpy(out, &t->stats, sizeof t->stats);
    return VPT_OK;
}

}  // extern "C"
