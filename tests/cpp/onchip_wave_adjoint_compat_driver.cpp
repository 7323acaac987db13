// onchip_wave_adjoint_compat_driver.cpp -- MatrixFreeSystem::waveHistoryMany and waveAdjointMany reached from a C++ host
// (tests/test_gpu_wave_adjoint_cpp.py).  Three members on an n = m = 10 grid, each with its own forcing, start state, velocity,
// medium (between 1/4 and 4), time step (waveCfl(its largest c2) x 1/4, 1/2, 1), row of amplitudes and table of adjoint sources,
// NSTEPS = 7 steps with three receivers (unknown 0, the middle one, the last) sampled every second step: the forward run with its
// history, then the backward run from zeros.  The inputs are plain arithmetic on the system's right-hand side that Python repeats
// operation by operation; the expected values come in on the command line as hex floats: per member (NSTEPS + 1) x size() values
// of the history, then per member size() values each of lam, q and sens.  One JSON object: per member whether every bit agrees,
// whether the forward state is waveMediumMany's, and whether a time step above a member's bound is refused.
// Build: g++ -std=c++17 -I iterative_solvers_amd/compat onchip_wave_adjoint_compat_driver.cpp -L... -lmi355cg
#include "matrix_free_system.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char** argv) {
    Kokkos::initialize();
    int rc = 0;
    {
        const int n = 10, nsys = 3, nsteps = 7, every = 2, samples = nsteps / every;
        MatrixFreeSystem sys(n, n, 1.0, 2.0, 1.0, 2.0);
        const size_t U = (size_t)sys.size();
        const std::vector<int> receivers = {0, (int)(U / 2), (int)U - 1};
        const size_t expected = (size_t)nsys * ((size_t)nsteps + 1) * U + (size_t)nsys * 3 * U;
        if ((size_t)argc != 1 + expected) { std::fprintf(stderr, "expected %zu arguments\n", expected); return 2; }
        std::vector<std::vector<double>> g(nsys, sys.get_rhs()), u0(nsys, std::vector<double>(U)), v0(nsys, std::vector<double>(U)), media(nsys, std::vector<double>(U));
        std::vector<std::vector<double>> source(nsys, std::vector<double>((size_t)nsteps + 1));
        std::vector<std::vector<std::vector<double>>> adj(nsys, std::vector<std::vector<double>>((size_t)samples, std::vector<double>(receivers.size())));
        std::vector<double> tau(nsys);
        for (int s = 0; s < nsys; ++s) {
            for (size_t i = 0; i < U; ++i) {
                g[(size_t)s][i] *= 1.0 + 0.25 * s * ((double)((i * 37) % 101) / 101.0);
                u0[(size_t)s][i] = 0.01 * s * ((double)((i * 11 + (size_t)s) % 53) / 53.0 - 0.5);       // member 0: from rest at zero
                v0[(size_t)s][i] = 0.5 * s * ((double)((i * 7 + (size_t)s) % 31) / 31.0 - 0.5);
                media[(size_t)s][i] = 0.25 + 3.75 * ((double)((i * 13 + (size_t)s * 5) % 47) / 46.0);
            }
            for (int k = 0; k <= nsteps; ++k) source[(size_t)s][(size_t)k] = (double)((k * 5 + s * 3) % 11) / 4.0 - 1.0;
            for (int j = 0; j < samples; ++j)
                for (size_t r = 0; r < receivers.size(); ++r) adj[(size_t)s][(size_t)j][r] = (double)((j * 7 + (int)r * 3 + s * 5) % 13) / 8.0 - 0.75;
            const double top = *std::max_element(media[(size_t)s].begin(), media[(size_t)s].end());
            tau[(size_t)s] = sys.waveCfl(top) * (s == 0 ? 0.25 : s == 1 ? 0.5 : 1.0);
        }
        char** arg = argv + 1;
        auto same_values = [&](const double* got, size_t count) {
            std::vector<double> want(count);
            for (size_t i = 0; i < count; ++i) want[i] = std::strtod(*arg++, nullptr);
            return std::memcmp(want.data(), got, sizeof(double) * count) == 0;
        };
        std::vector<std::vector<double>> u = u0, v = v0, um = u0, vm = v0;
        std::vector<std::vector<std::vector<double>>> traces, traces_m, history;
        std::vector<mi355cg_results> res;
        std::vector<int> done;
        sys.waveMediumMany(um, vm, tau, nsteps, media, source, receivers, every, &traces_m, nullptr, nullptr, g, 3);
        sys.waveHistoryMany(u, v, tau, nsteps, media, source, receivers, every, &traces, history, &res, &done, g, 3);
        const bool forward = u == um && v == vm && traces == traces_m;
        if (!forward) rc = 1;
        std::printf("{\"forward_is_the_medium_call\": %s, \"history\": [\n", forward ? "true" : "false");
        for (int s = 0; s < nsys; ++s) {
            bool sh = history.size() == (size_t)nsys && history[(size_t)s].size() == (size_t)nsteps + 1;
            for (int r = 0; r <= nsteps; ++r) {
                if (sh && history[(size_t)s][(size_t)r].size() == U) sh = same_values(history[(size_t)s][(size_t)r].data(), U) && sh;
                else { sh = false; arg += U; }
            }
            if (!sh || done[(size_t)s] != nsteps) rc = 1;
            std::printf("{\"steps_done\": %d, \"converged\": %d, \"same_history\": %s}%s\n", done[(size_t)s], res[(size_t)s].converged, sh ? "true" : "false", s + 1 < nsys ? "," : "");
        }
        std::printf("], \"adjoint\": [\n");
        std::vector<std::vector<double>> lam, q, sens;
        bool refused_tau = false;
        if (history.size() == (size_t)nsys) {
            std::vector<double> big = tau;
            big[2] = sys.waveCfl();
            try { sys.waveAdjointMany(history, big, media, adj, receivers, every, lam, q, sens); } catch (const std::invalid_argument&) { refused_tau = true; }
            if (!lam.empty()) rc = 1;                                  // a refused call writes nothing
            sys.waveAdjointMany(history, tau, media, adj, receivers, every, lam, q, sens, &res, &done, 3);
        }
        for (int s = 0; s < nsys; ++s) {
            const bool have = lam.size() == (size_t)nsys && q.size() == (size_t)nsys && sens.size() == (size_t)nsys;
            bool sl = false, sq = false, ss = false;
            if (have) { sl = same_values(lam[(size_t)s].data(), U); sq = same_values(q[(size_t)s].data(), U); ss = same_values(sens[(size_t)s].data(), U); }
            if (!sl || !sq || !ss || done[(size_t)s] != nsteps) rc = 1;
            std::printf("{\"steps_done\": %d, \"same_lam\": %s, \"same_q\": %s, \"same_sens\": %s}%s\n", done[(size_t)s], sl ? "true" : "false", sq ? "true" : "false",
                        ss ? "true" : "false", s + 1 < nsys ? "," : "");
        }
        if (!refused_tau) rc = 1;
        std::printf("], \"refused_tau\": %s}\n", refused_tau ? "true" : "false");
    }
    Kokkos::finalize();
    return rc;
}
