// TEST INFRASTRUCTURE: vaporetto_amd/csrc/tron.h over a third backend -- a dense fp64 matrix on the host, every sum taken in index
// order -- so that the algorithm is run without either product backend (tests/test_tron_native.py).
//
// stdin: the number of problems, then per problem "rows features solver eps cost" and per row its target (+1 / -1) and its 0/1 features.
// stdout per problem: "stats iterations cg_steps gnorm0 gnorm objective" and "w" with the features' weights and the bias.
#include <cstdio>
#include <vector>

#include "tron.h"

namespace {

struct Dense {
    int l, n, solver;   // n: the features and the bias column
    double c;
    std::vector<double> X, y, z, D, tmp, store;
    vpt::TronVectors v;

    Dense(int rows, int features, int solver_, double cost)
        : l(rows), n(features + 1), solver(solver_), c(cost), X(size_t(rows) * n, 1.0), y(rows), z(rows), D(rows), tmp(rows), store(7 * size_t(n)) {
        double* p = store.data();
        v = vpt::TronVectors{p, p + n, p + 2 * n, p + 3 * n, p + 4 * n, p + 5 * n, p + 6 * n};
    }
    void xv(const double* x, double* out) const {
        for (int r = 0; r < l; ++r) {
            double s = 0;
            for (int j = 0; j < n; ++j) s += X[size_t(r) * n + j] * x[j];
            out[r] = s;
        }
    }
    void add_xtv(const double* a, const double* u, double* out) const {
        for (int j = 0; j < n; ++j) {
            double s = 0;
            for (int r = 0; r < l; ++r) s += X[size_t(r) * n + j] * u[r];
            out[j] = a[j] + s;
        }
    }
    double dot(const double* a, const double* b) const {
        double s = 0;
        for (int i = 0; i < n; ++i) s += a[i] * b[i];
        return s;
    }
    double fun(const double* x) {
        xv(x, z.data());
        double s = 0;
        for (int r = 0; r < l; ++r) s += vpt::tron_loss(y[r] * z[r], c, solver);
        return dot(x, x) / 2.0 + s;
    }
    void grad(const double* x, double* out) {
        for (int r = 0; r < l; ++r) {
            const vpt::TronRow t = vpt::tron_grad_row(y[r], y[r] * z[r], c, solver);
            D[r] = t.D;
            tmp[r] = t.gz;
        }
        add_xtv(x, tmp.data(), out);
    }
    void hv(const double* x, double* out) {
        xv(x, tmp.data());
        for (int r = 0; r < l; ++r) tmp[r] *= D[r];
        add_xtv(x, tmp.data(), out);
    }
    void zero(double* x) const { for (int i = 0; i < n; ++i) x[i] = 0; }
    void copy(const double* x, double* out) const { for (int i = 0; i < n; ++i) out[i] = x[i]; }
    void add(const double* a, const double* b, double* out) const { for (int i = 0; i < n; ++i) out[i] = a[i] + b[i]; }
    void axpy(double a, const double* x, double* y_) const { for (int i = 0; i < n; ++i) y_[i] += a * x[i]; }
    void xpby(const double* x, double b, double* y_) const { for (int i = 0; i < n; ++i) y_[i] = x[i] + b * y_[i]; }
    void cg_start() const { for (int i = 0; i < n; ++i) { v.s[i] = 0; v.r[i] = v.d[i] = -v.g[i]; } }
    void cg_boundary(double a) const { axpy(a, v.d, v.s); axpy(-a, v.Hd, v.r); }
    bool cg_more(int) const { return true; }
    bool ok() const { return true; }
};

}  // namespace

int main() {
    int n_prob = 0;
    if (std::scanf("%d", &n_prob) != 1) return 1;
    for (int p = 0; p < n_prob; ++p) {
        int rows, features, solver;
        double eps, cost;
        if (std::scanf("%d %d %d %lf %lf", &rows, &features, &solver, &eps, &cost) != 5 || rows < 1 || features < 0) return 1;
        Dense B(rows, features, solver, cost);
        int pos = 0;
        for (int r = 0; r < rows; ++r) {
            if (std::scanf("%lf", &B.y[r]) != 1) return 1;
            pos += B.y[r] > 0;
            for (int j = 0; j < features; ++j)
                if (std::scanf("%lf", &B.X[size_t(r) * B.n + j]) != 1) return 1;
        }
        const vpt_train_stats st = vpt::tron(B, vpt::tron_tolerance(eps, double(pos), double(rows)));
        std::printf("stats %u %u %.17g %.17g %.17g\nw", st.iterations, st.cg_steps, st.gnorm0, st.gnorm, st.objective);
        for (int j = 0; j < B.n; ++j) std::printf(" %.17g", B.v.w[j]);
        std::printf("\n");
    }
    return 0;
}
