// onchip_wave_compat_driver.cpp -- MatrixFreeSystem::waveStepsMany reached from a C++ host (tests/test_gpu_wave_many.py).
// Three members on an n = m = 12 grid, each with its own forcing, start state, velocity and time step, integrated over NSTEPS steps
// of velocity Verlet (tau = waveCfl() x 1/4, 1/2, 1) and then, from the same start, of Newmark.  The inputs are plain arithmetic on
// the system's right-hand side that Python repeats operation by operation; the expected states come in on the command line as hex
// floats: for Verlet per member size() values of u and of v; for Newmark per member its steps_done, NSTEPS iteration counts, then u
// and v.  One JSON object: per scheme and member whether every bit agrees, and the counts.
// Build: g++ -std=c++17 -I iterative_solvers_amd/compat onchip_wave_compat_driver.cpp -L... -lmi355cg
#include "matrix_free_system.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char** argv) {
    Kokkos::initialize();
    int rc = 0;
    {
        const int n = 12, nsys = 3, nsteps = 3;
        MatrixFreeSystem sys(n, n, 1.0, 2.0, 1.0, 2.0);
        const size_t U = (size_t)sys.size(), expected = (size_t)nsys * (2 * U) + (size_t)nsys * (1 + (size_t)nsteps + 2 * U);
        if ((size_t)argc != 1 + expected) { std::fprintf(stderr, "expected %zu arguments\n", expected); return 2; }
        const double bound = sys.waveCfl();
        const std::vector<double> tau_verlet = {0.25 * bound, 0.5 * bound, bound}, tau_newmark = {0.001, 0.0625, 0.5};
        std::vector<std::vector<double>> g(nsys, sys.get_rhs()), u0(nsys, std::vector<double>(U)), v0(nsys, std::vector<double>(U));
        for (int s = 0; s < nsys; ++s)
            for (size_t i = 0; i < U; ++i) {
                g[(size_t)s][i] *= 1.0 + 0.25 * s * ((double)((i * 37) % 101) / 101.0);
                u0[(size_t)s][i] = 0.01 * s * ((double)((i * 11 + (size_t)s) % 53) / 53.0 - 0.5);       // member 0: from rest at zero
                v0[(size_t)s][i] = 0.5 * s * ((double)((i * 7 + (size_t)s) % 31) / 31.0 - 0.5);
            }
        mi355cg_params p;
        mi355cg_default_params(&p, MI355CG_RULE_REL_2NORM);
        p.max_iterations = 10000;
        p.eps_rel = 1e-9;
        p.use_true_solution = 0;
        p.sync_every = 7;

        char** arg = argv + 1;
        auto same_vector = [&](const std::vector<double>& got) {
            std::vector<double> want(U);
            for (size_t i = 0; i < U; ++i) want[i] = std::strtod(*arg++, nullptr);
            return std::memcmp(want.data(), got.data(), sizeof(double) * U) == 0;
        };
        std::printf("{\"bound\": \"%a\", \"verlet\": [\n", bound);
        {
            std::vector<std::vector<double>> u = u0, v = v0;
            std::vector<mi355cg_results> res;
            std::vector<int> done;
            sys.waveStepsMany(u, v, tau_verlet, nsteps, MI355CG_WAVE_VERLET, p, &res, &done, nullptr, g, 2);
            for (int s = 0; s < nsys; ++s) {
                const bool su = same_vector(u[(size_t)s]), sv = same_vector(v[(size_t)s]);
                if (!su || !sv || done[(size_t)s] != nsteps) rc = 1;
                std::printf("{\"steps_done\": %d, \"converged\": %d, \"iterations\": %d, \"same_u\": %s, \"same_v\": %s}%s\n", done[(size_t)s],
                            res[(size_t)s].converged, res[(size_t)s].iterations, su ? "true" : "false", sv ? "true" : "false", s + 1 < nsys ? "," : "");
            }
        }
        std::printf("], \"newmark\": [\n");
        {
            std::vector<std::vector<double>> u = u0, v = v0;
            std::vector<mi355cg_results> res;
            std::vector<int> done;
            std::vector<std::vector<int>> its;
            sys.waveStepsMany(u, v, tau_newmark, nsteps, MI355CG_WAVE_NEWMARK, p, &res, &done, &its, g);
            for (int s = 0; s < nsys; ++s) {
                const int want_done = std::atoi(*arg++);
                bool same_counts = done[(size_t)s] == want_done;
                for (int k = 0; k < nsteps; ++k) same_counts = (its[(size_t)s][(size_t)k] == std::atoi(*arg++)) && same_counts;
                const bool su = same_vector(u[(size_t)s]), sv = same_vector(v[(size_t)s]);
                if (!su || !sv || !same_counts) rc = 1;
                std::printf("{\"steps_done\": %d, \"converged\": %d, \"same_u\": %s, \"same_v\": %s, \"same_counts\": %s, \"iterations\": [", done[(size_t)s],
                            res[(size_t)s].converged, su ? "true" : "false", sv ? "true" : "false", same_counts ? "true" : "false");
                for (int k = 0; k < nsteps; ++k) std::printf("%s%d", k ? ", " : "", its[(size_t)s][(size_t)k]);
                std::printf("]}%s\n", s + 1 < nsys ? "," : "");
            }
        }
        std::printf("]}\n");
    }
    Kokkos::finalize();
    return rc;
}
