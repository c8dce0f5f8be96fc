// TEST INFRASTRUCTURE: vaporetto_amd/csrc/l1r.h over a dense, sequential backend -- every sum taken in row order on the host -- so that
// the column step and the sweep order run without the device backend (tests/test_l1r_native.py).  Built with the address and
// undefined-behaviour sanitizers.
//
// stdin: the number of problems, then per problem "rows features eps cost groups", per group its size and its columns (the bias is
// column `features`), and per row its target (+1 / -1) and its feature counts.
// stdout per problem: "stats sweeps halvings violation0 violation" and "w" with the features' weights and the bias.
#include <cstdio>
#include <vector>

#include "l1r.h"

namespace {

struct DenseColumn {
    int l, n, j;   // n: the features and the bias column
    double c;
    const std::vector<double>& X;   // [l][n], the bias column filled with 1
    const std::vector<double>& y;
    std::vector<double>& b;
    template <typename F>
    vpt::L1rPair sums(F f) const {
        vpt::L1rPair acc{0.0, 0.0};
        for (int r = 0; r < l; ++r) {
            const double x = X[size_t(r) * n + j];
            if (x != 0) acc = vpt::l1r_add(acc, f(b[r], x * y[r]));
        }
        return acc;
    }
    vpt::L1rPair grad_sums() const { return sums([this](double bi, double v) { return vpt::l1r_grad_term(bi, v, c); }); }
    vpt::L1rPair loss_sums(double d) const { return sums([this, d](double bi, double v) { return vpt::l1r_loss_term(bi, v, c, d); }); }
    void commit(double d) const {
        for (int r = 0; r < l; ++r) {
            const double x = X[size_t(r) * n + j];
            if (x != 0) b[r] = b[r] - d * (x * y[r]);
        }
    }
};

}  // namespace

int main() {
    int n_prob = 0;
    if (std::scanf("%d", &n_prob) != 1) return 1;
    for (int p = 0; p < n_prob; ++p) {
        int rows, features, n_groups;
        double eps, cost;
        if (std::scanf("%d %d %lf %lf %d", &rows, &features, &eps, &cost, &n_groups) != 5 || rows < 1 || features < 0 || n_groups < 1) return 1;
        const int n = features + 1;
        std::vector<std::vector<int>> groups(n_groups);
        for (auto& g : groups) {
            int size = 0;
            if (std::scanf("%d", &size) != 1 || size < 1) return 1;
            g.resize(size);
            for (int& j : g)
                if (std::scanf("%d", &j) != 1 || j < 0 || j >= n) return 1;
        }
        std::vector<double> X(size_t(rows) * n, 1.0), y(rows), b(rows, 1.0), w(n, 0.0), xj_sq(n, 0.0);
        int pos = 0;
        for (int r = 0; r < rows; ++r) {
            if (std::scanf("%lf", &y[r]) != 1) return 1;
            pos += y[r] > 0;
            for (int j = 0; j < features; ++j)
                if (std::scanf("%lf", &X[size_t(r) * n + j]) != 1) return 1;
        }
        for (int j = 0; j < n; ++j)
            for (int r = 0; r < rows; ++r) xj_sq[j] += cost * X[size_t(r) * n + j] * X[size_t(r) * n + j];
        const double neg = rows - pos, tol = eps * (pos < neg ? (pos > 1 ? pos : 1) : (neg > 1 ? neg : 1)) / rows;
        std::vector<uint32_t> order(n_groups);
        for (int g = 0; g < n_groups; ++g) order[g] = uint32_t(g);
        uint64_t rng = vpt::kL1rSeed;
        double v0 = 0, v = 0;
        unsigned sweeps = 0, halvings = 0;
        while (sweeps < unsigned(vpt::kL1rMaxSweeps)) {
            vpt::l1r_shuffle(order.data(), uint32_t(order.size()), &rng);
            std::vector<double> viol(n, 0.0);
            for (uint32_t g : order)
                for (int j : groups[g]) {
                    DenseColumn col{rows, n, j, cost, X, y, b};
                    const vpt::L1rStep s = vpt::l1r_column(col, w[j], xj_sq[j]);
                    viol[j] = s.violation;
                    w[j] += s.d;
                    halvings += s.halvings;
                }
            v = 0;
            for (double x : viol) v += x;
            if (sweeps++ == 0) v0 = v;
            if (v <= tol * v0) break;
        }
        std::printf("stats %u %u %.17g %.17g\nw", sweeps, halvings, v0, v);
        for (int j = 0; j < n; ++j) std::printf(" %.17g", w[j]);
        std::printf("\n");
    }
    return 0;
}
