// onchip_steps_compat_driver.cpp -- MatrixFreeSystem::timeStepsMany reached from a C++ host (tests/test_gpu_steps_many.py).
// Three members on an n = m = 12 grid, each with its own forcing, start state and time step, integrated over NSTEPS Crank-Nicolson
// steps in one call.  The inputs are plain arithmetic on the system's right-hand side that Python repeats operation by operation;
// the expected states (from mi355cg_time_steps on a second handle) come in on the command line as hex floats: per member its
// steps_done, NSTEPS iteration counts and size() values.  One JSON object: per member whether every bit agrees, and the counts.
// Build: g++ -std=c++17 -I iterative_solvers_amd/compat onchip_steps_compat_driver.cpp -L... -lmi355cg
#include "dirichlet_solver.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char** argv) {
    Kokkos::initialize();
    int rc = 0;
    {
        const int n = 12, nsys = 3, nsteps = 3;
        MatrixFreeSystem sys(n, n, 1.0, 2.0, 1.0, 2.0);
        const size_t U = (size_t)sys.size();
        if ((size_t)argc != 1 + (size_t)nsys * (1 + (size_t)nsteps + U)) { std::fprintf(stderr, "expected %zu arguments\n", (size_t)nsys * (1 + (size_t)nsteps + U)); return 2; }
        const std::vector<double> tau = {0.001, 0.0625, 0.5};
        std::vector<std::vector<double>> g(nsys, sys.get_rhs()), u0(nsys, std::vector<double>(U));
        for (int s = 0; s < nsys; ++s)
            for (size_t i = 0; i < U; ++i) {
                g[(size_t)s][i] *= 1.0 + 0.25 * s * ((double)((i * 37) % 101) / 101.0);
                u0[(size_t)s][i] = 0.01 * s * ((double)((i * 11 + (size_t)s) % 53) / 53.0 - 0.5);       // member 0: from zero
            }
        mi355cg_params p;
        mi355cg_default_params(&p, MI355CG_RULE_REL_2NORM);
        p.max_iterations = 10000;
        p.eps_rel = 1e-9;
        p.use_true_solution = 0;
        p.sync_every = 7;
        std::vector<mi355cg_results> res;
        std::vector<int> done;
        std::vector<std::vector<int>> its;
        const std::vector<std::vector<double>> u = sys.timeStepsMany(u0, tau, 0.5, nsteps, p, &res, &done, &its, g);

        char** arg = argv + 1;
        std::printf("{\"members\": [\n");
        for (int s = 0; s < nsys; ++s) {
            const int want_done = std::atoi(*arg++);
            bool same_counts = done[(size_t)s] == want_done;
            for (int k = 0; k < nsteps; ++k) same_counts = (its[(size_t)s][(size_t)k] == std::atoi(*arg++)) && same_counts;
            std::vector<double> want(U);
            for (size_t i = 0; i < U; ++i) want[i] = std::strtod(*arg++, nullptr);
            const bool same = std::memcmp(want.data(), u[(size_t)s].data(), sizeof(double) * U) == 0;
            if (!same || !same_counts) rc = 1;
            std::printf("{\"steps_done\": %d, \"converged\": %d, \"same_bits\": %s, \"same_counts\": %s, \"iterations\": [", done[(size_t)s],
                        res[(size_t)s].converged, same ? "true" : "false", same_counts ? "true" : "false");
            for (int k = 0; k < nsteps; ++k) std::printf("%s%d", k ? ", " : "", its[(size_t)s][(size_t)k]);
            std::printf("]}%s\n", s + 1 < nsys ? "," : "");
        }
        std::printf("]}\n");
    }
    Kokkos::finalize();
    return rc;
}
