// onchip_wave_sponge_compat_driver.cpp -- MatrixFreeSystem::waveSpongeMany reached from a C++ host (tests/test_gpu_wave_sponge_cpp.py).
// Three members on an n = m = 12 grid, each with its own forcing, start state, velocity, medium (between 1/4 and 4), time step
// (waveCfl(its largest c2) x 1/4, 1/2, 1), damping field ((tau / 4) d between 0 and 0.9, zero at every 29th unknown) and row of
// amplitudes, integrated over NSTEPS = 7 steps with three receivers (unknown 0, the middle one, the last) sampled every second
// step; then once more with member 2's damping field (the largest time step's), a unit medium and ONE row of amplitudes for all,
// no receivers, every member at the grid's bound x 1/2.  The inputs are plain arithmetic on the system's right-hand side that
// Python repeats operation by operation; the expected values, the results of the Python call, come in on the command line as hex
// floats: per member size() values of u and of v and 3 x 3 samples, then per member u and v of the second run.  One JSON object:
// per run and member whether every bit agrees, and what was refused.
// Build: g++ -std=c++17 -I iterative_solvers_amd/compat onchip_wave_sponge_compat_driver.cpp -L... -lmi355cg
#include "matrix_free_system.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char** argv) {
    Kokkos::initialize();
    int rc = 0;
    {
        const int n = 12, nsys = 3, nsteps = 7, every = 2, samples = nsteps / every;
        MatrixFreeSystem sys(n, n, 1.0, 2.0, 1.0, 2.0);
        const size_t U = (size_t)sys.size();
        const std::vector<int> receivers = {0, (int)(U / 2), (int)U - 1};
        const size_t expected = (size_t)nsys * (2 * U + (size_t)samples * receivers.size()) + (size_t)nsys * 2 * U;
        if ((size_t)argc != 1 + expected) { std::fprintf(stderr, "expected %zu arguments\n", expected); return 2; }
        std::vector<std::vector<double>> g(nsys, sys.get_rhs()), u0(nsys, std::vector<double>(U)), v0(nsys, std::vector<double>(U)), media(nsys, std::vector<double>(U));
        std::vector<std::vector<double>> damping(nsys, std::vector<double>(U)), source(nsys, std::vector<double>((size_t)nsteps + 1));
        std::vector<double> tau(nsys);
        for (int s = 0; s < nsys; ++s) {
            for (size_t i = 0; i < U; ++i) {
                g[(size_t)s][i] *= 1.0 + 0.25 * s * ((double)((i * 37) % 101) / 101.0);
                u0[(size_t)s][i] = 0.01 * s * ((double)((i * 11 + (size_t)s) % 53) / 53.0 - 0.5);       // member 0: from rest at zero
                v0[(size_t)s][i] = 0.5 * s * ((double)((i * 7 + (size_t)s) % 31) / 31.0 - 0.5);
                media[(size_t)s][i] = 0.25 + 3.75 * ((double)((i * 13 + (size_t)s * 5) % 47) / 46.0);
            }
            for (int k = 0; k <= nsteps; ++k) source[(size_t)s][(size_t)k] = (double)((k * 5 + s * 3) % 11) / 4.0 - 1.0;
            const double top = *std::max_element(media[(size_t)s].begin(), media[(size_t)s].end());
            tau[(size_t)s] = sys.waveCfl(top) * (s == 0 ? 0.25 : s == 1 ? 0.5 : 1.0);
            for (size_t i = 0; i < U; ++i) damping[(size_t)s][i] = (double)((i * 17 + (size_t)s * 3) % 29) / 28.0 * 0.9 / (0.25 * tau[(size_t)s]);
        }
        char** arg = argv + 1;
        auto same_values = [&](const double* got, size_t count) {
            std::vector<double> want(count);
            for (size_t i = 0; i < count; ++i) want[i] = std::strtod(*arg++, nullptr);
            return std::memcmp(want.data(), got, sizeof(double) * count) == 0;
        };
        std::printf("{\"damped\": [\n");
        {
            std::vector<std::vector<double>> u = u0, v = v0;
            std::vector<std::vector<std::vector<double>>> traces;
            std::vector<mi355cg_results> res;
            std::vector<int> done;
            sys.waveSpongeMany(u, v, tau, nsteps, media, damping, source, receivers, every, &traces, &res, &done, g, 3);
            for (int s = 0; s < nsys; ++s) {
                const bool su = same_values(u[(size_t)s].data(), U), sv = same_values(v[(size_t)s].data(), U);
                bool st = traces.size() == (size_t)nsys && traces[(size_t)s].size() == (size_t)samples;
                for (int j = 0; j < samples; ++j) {
                    const bool ok = st && traces[(size_t)s][(size_t)j].size() == receivers.size();
                    if (ok) st = same_values(traces[(size_t)s][(size_t)j].data(), receivers.size()) && st;
                    else { st = false; arg += receivers.size(); }
                }
                if (!su || !sv || !st || done[(size_t)s] != nsteps) rc = 1;
                std::printf("{\"steps_done\": %d, \"converged\": %d, \"iterations\": %d, \"same_u\": %s, \"same_v\": %s, \"same_traces\": %s}%s\n", done[(size_t)s],
                            res[(size_t)s].converged, res[(size_t)s].iterations, su ? "true" : "false", sv ? "true" : "false", st ? "true" : "false", s + 1 < nsys ? "," : "");
            }
        }
        std::printf("], \"shared\": [\n");
        {
            std::vector<std::vector<double>> u = u0, v = v0;
            std::vector<std::vector<std::vector<double>>> traces(1);
            std::vector<int> done;
            const std::vector<double> half(nsys, 0.5 * sys.waveCfl());
            sys.waveSpongeMany(u, v, half, nsteps, {std::vector<double>(U, 1.0)}, {damping[2]}, {source[1]}, {}, 1, &traces, nullptr, &done, g);
            for (int s = 0; s < nsys; ++s) {
                const bool su = same_values(u[(size_t)s].data(), U), sv = same_values(v[(size_t)s].data(), U);
                if (!su || !sv || !traces.empty() || done[(size_t)s] != nsteps) rc = 1;
                std::printf("{\"steps_done\": %d, \"same_u\": %s, \"same_v\": %s, \"no_traces\": %s}%s\n", done[(size_t)s], su ? "true" : "false", sv ? "true" : "false",
                            traces.empty() ? "true" : "false", s + 1 < nsys ? "," : "");
            }
        }
        // what the library refuses arrives as std::invalid_argument: a negative damping rate, a NaN, a damping above 4 / tau, a field
        // of the wrong size
        bool refused_negative = false, refused_nan = false, refused_strong = false, refused_size = false;
        {
            std::vector<std::vector<double>> u = u0, v = v0, bad = damping;
            bad[1][5] = -1.0;
            try { sys.waveSpongeMany(u, v, tau, nsteps, media, bad, source, {}, 1, nullptr); } catch (const std::invalid_argument&) { refused_negative = true; }
            bad[1][5] = std::nan("");
            try { sys.waveSpongeMany(u, v, tau, nsteps, media, bad, source, {}, 1, nullptr); } catch (const std::invalid_argument&) { refused_nan = true; }
            bad[1][5] = 4.5 / tau[1];
            try { sys.waveSpongeMany(u, v, tau, nsteps, media, bad, source, {}, 1, nullptr); } catch (const std::invalid_argument&) { refused_strong = true; }
            bad[1][5] = 0.0;
            bad[1].pop_back();
            try { sys.waveSpongeMany(u, v, tau, nsteps, media, bad, source, {}, 1, nullptr); } catch (const std::invalid_argument&) { refused_size = true; }
            if (!refused_negative || !refused_nan || !refused_strong || !refused_size || u != u0 || v != v0) rc = 1;
        }
        std::printf("], \"refused_negative\": %s, \"refused_nan\": %s, \"refused_strong\": %s, \"refused_size\": %s}\n", refused_negative ? "true" : "false",
                    refused_nan ? "true" : "false", refused_strong ? "true" : "false", refused_size ? "true" : "false");
    }
    Kokkos::finalize();
    return rc;
}
