// onchip_many_compat_driver.cpp -- MatrixFreeSystem::solveMany reached from a C++ host (tests/test_gpu_onchip_many.py).
// Three systems on an n = m = 12 grid, each with its own right-hand side, shift and guess, solved as one batch; then the same three
// one after another by MSGSolver on a GridSystem of the same grid (mi355cg_set_shift on its handle, setInitialGuess).  One JSON
// object: per system both solutions with 17 digits, the iteration counts and whether every bit agrees.
// Build: g++ -std=c++17 -I iterative_solvers_amd/compat onchip_many_compat_driver.cpp -L... -lmi355cg
#include "dirichlet_solver.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

int main() {
    Kokkos::initialize();
    int rc = 0;
    {
        const int n = 12, nsys = 3;
        const double eps = 1e-9;
        GridSystem grid(n, n, 1.0, 2.0, 1.0, 2.0);
        MatrixFreeSystem sys(n, n, 1.0, 2.0, 1.0, 2.0);
        const size_t U = (size_t)sys.size();
        const std::vector<double> sigma = {0.0, 2.5, 40.0};
        std::vector<std::vector<double>> b(nsys, sys.get_rhs()), x0(nsys, std::vector<double>(U));
        for (int s = 0; s < nsys; ++s)
            for (size_t i = 0; i < U; ++i) {
                b[(size_t)s][i] *= 1.0 + 0.25 * s * std::sin(0.37 * (double)i);
                x0[(size_t)s][i] = 0.01 * s * std::cos(0.11 * (double)i + s);      // system 0: a zero guess
            }
        mi355cg_params p;
        mi355cg_default_params(&p, MI355CG_RULE_MSG_MAXNORM);                       // what MSGSolver::solve sets without a true solution
        p.max_iterations = 10000;
        p.eps_precision = p.eps_residual = p.eps_exact_error = eps;
        p.use_true_solution = 0;
        p.callback_every = 100;
        std::vector<mi355cg_results> res;
        const std::vector<std::vector<double>> xm = sys.solveMany(b, p, &res, sigma, x0);

        std::printf("{\"systems\": [\n");
        for (int s = 0; s < nsys; ++s) {
            mi355cg_compat::check(mi355cg_set_shift(grid.context()->h, sigma[(size_t)s]));
            KokkosVector bv("b", U), gv("x0", U);
            for (size_t i = 0; i < U; ++i) { bv(i) = b[(size_t)s][i]; gv(i) = x0[(size_t)s][i]; }
            MSGSolver solver(grid.get_matrix(), bv, eps, 10000);
            solver.setVerbose(false);
            solver.setInitialGuess(gv);
            const KokkosVector xs = solver.solve(KokkosVector());
            const bool same = std::memcmp(xs.data(), xm[(size_t)s].data(), sizeof(double) * U) == 0;
            if (!same) rc = 1;
            std::printf("{\"sigma\": %.17g, \"iterations_many\": %d, \"iterations_single\": %d, \"converged_many\": %d, \"same_bits\": %s, \"many\": [",
                        sigma[(size_t)s], res[(size_t)s].iterations, solver.getIterations(), res[(size_t)s].converged, same ? "true" : "false");
            for (size_t i = 0; i < U; ++i) std::printf("%s%.17g", i ? ", " : "", xm[(size_t)s][i]);
            std::printf("], \"single\": [");
            for (size_t i = 0; i < U; ++i) std::printf("%s%.17g", i ? ", " : "", xs(i));
            std::printf("]}%s\n", s + 1 < nsys ? "," : "");
        }
        std::printf("]}\n");
    }
    Kokkos::finalize();
    return rc;
}
