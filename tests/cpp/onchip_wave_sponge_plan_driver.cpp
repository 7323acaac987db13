// onchip_wave_sponge_plan_driver.cpp -- the host arithmetic of the recorded explicit wave stepper with a damping field
// (csrc/onchip_plan.h) on the CPU, under the sanitizers (tests/test_onchip_wave_sponge_cpu.py).
//
// Without arguments: for every even N from 6 to kOnchipMaxN the workspace bytes of several (nsys, nsteps, nrec, record_every) are
// restated from the documented formula -- the medium call's workspace and 16 bytes per member --, and are 0 (refused) for what
// that workspace refuses.  A zero damping is checked to give the factor 1.0 and a damp that changes nothing.  Prints
// "N=<n> unknowns=<u> ws=<nsys>:<nsteps>:<nrec>:<every>:<bytes>,..." per size, "FAIL ..." per violation, "cap <N>" and
// "ok <failures>" at the end.
//
// With <in> <out>: whole steps, written as k_oc_wave_sponge runs them -- launches of at most `launch` steps; at the entry of a
// launch the opening damp and the first half kick with the acceleration formed from (u, g, c2, w[step0]); per step the drift, then
// one pass that forms the acceleration, makes the second kick and the closing damp and, unless the step is the launch's last, the
// next step's opening damp and first kick -- with the functions that kernel calls.  <in> holds doubles: n, tau, nsteps, A0, xk, yk,
// record_every, nrec, launch, then the (n+1)^2 cells of an image of u, per unknown in packed order g, v, c2 and d, the nsteps + 1
// amplitudes, the nrec receivers (packed indices).  <out> receives u and v of every unknown, then (nsteps / record_every) x nrec
// samples.
// With a third argument `factor`: <in> holds count, then count values each of tau, d, v; <out> receives count factors
// onchip_wave_sponge_factor(tau, d), then count values onchip_wave_damp(factor, v).
// Compile with -ffp-contract=off, as the library is.
#include "../../iterative_solvers_amd/csrc/onchip_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace mi355cg;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

static bool read_doubles(std::FILE* f, std::vector<double>& v) { return v.empty() || std::fread(v.data(), sizeof(double), v.size(), f) == v.size(); }
static int write_doubles(const char* path, const std::vector<double>& v) {
    std::FILE* o = std::fopen(path, "wb");
    if (!o) return 2;
    const bool wrote = v.empty() || std::fwrite(v.data(), sizeof(double), v.size(), o) == v.size();
    std::fclose(o);
    return wrote ? 0 : 2;
}

static int factor_file(const char* in, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    double head = 0;
    if (std::fread(&head, sizeof(double), 1, f) != 1 || head < 0 || head > 1e6) { std::fclose(f); return 2; }
    const size_t count = (size_t)head;
    std::vector<double> tau(count), d(count), v(count), res(2 * count);
    const bool read = read_doubles(f, tau) && read_doubles(f, d) && read_doubles(f, v);
    std::fclose(f);
    if (!read) return 2;
    for (size_t i = 0; i < count; ++i) { res[i] = onchip_wave_sponge_factor(tau[i], d[i]); res[count + i] = onchip_wave_damp(res[i], v[i]); }
    return write_doubles(out, res);
}

static int steps_file(const char* in, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    double head[9];
    if (std::fread(head, sizeof(double), 9, f) != 9) { std::fclose(f); return 2; }
    const int n = (int)head[0], nsteps = (int)head[2], every = (int)head[6], nrec = (int)head[7], launch = (int)head[8];
    const OnchipPlan pl = onchip_plan(n);
    if (pl.n != n || nsteps < 0 || nsteps > kOnchipStepsMaxSteps || every < 1 || nrec < 0 || nrec > kOnchipWaveMaxRec || launch < 1) { std::fclose(f); return 3; }
    const double tau = head[1], h = 0.5 * tau;
    const OnchipWaveCoef k{head[3], head[4], head[5]};
    const size_t U = (size_t)pl.unknowns, samples = (size_t)(nsteps / every);
    std::vector<double> img((size_t)pl.cells), g(U), v(U), c2(U), d(U), w((size_t)nsteps + 1), rec((size_t)nrec), res(2 * U + samples * (size_t)nrec);
    const bool read = read_doubles(f, img) && read_doubles(f, g) && read_doubles(f, v) && read_doubles(f, c2) && read_doubles(f, d) && read_doubles(f, w) &&
                      read_doubles(f, rec);
    std::fclose(f);
    if (!read) return 2;
    std::vector<int> cell(U), rcell((size_t)nrec);
    for (int i = 0; i < pl.unknowns; ++i) { int xx, yy; onchip_node(pl, i, &xx, &yy); cell[(size_t)i] = onchip_cell(pl, xx, yy); }
    for (int r = 0; r < nrec; ++r) {
        if (rec[(size_t)r] < 0 || rec[(size_t)r] >= (double)pl.unknowns) return 3;
        rcell[(size_t)r] = cell[(size_t)rec[(size_t)r]];
    }
    auto accel = [&](size_t i, double wn) {
        const size_t c = (size_t)cell[i], p = (size_t)pl.pitch;
        return onchip_wave_medium_accel(k, c2[i], onchip_wave_forcing(wn, g[i]), img[c], img[c - 1], img[c + 1], img[c - p], img[c + p]);
    };
    double* sample = res.data() + 2 * U;
    std::vector<double> sf(U);
    for (int step0 = 0; step0 < nsteps; step0 += launch) {
        const int m = std::min(launch, nsteps - step0);
        for (size_t i = 0; i < U; ++i) {                                            // the entry of a launch: the slot is loaded, the factor formed
            sf[i] = onchip_wave_sponge_factor(tau, d[i]);
            v[i] = onchip_wave_kick(onchip_wave_damp(sf[i], v[i]), h, accel(i, w[(size_t)step0]));
        }
        for (int s = 0; s < m; ++s) {
            for (size_t i = 0; i < U; ++i) img[(size_t)cell[i]] = onchip_wave_drift(img[(size_t)cell[i]], tau, v[i]);      // between the barriers: owned cells only
            for (size_t i = 0; i < U; ++i) {
                const double a = accel(i, w[(size_t)(step0 + s) + 1]);
                v[i] = onchip_wave_damp(sf[i], onchip_wave_kick(v[i], h, a));
                if (s + 1 < m) v[i] = onchip_wave_kick(onchip_wave_damp(sf[i], v[i]), h, a);
            }
            if ((step0 + s + 1) % every == 0) for (int r = 0; r < nrec; ++r) *sample++ = img[(size_t)rcell[(size_t)r]];
        }
    }
    for (size_t i = 0; i < U; ++i) { res[i] = img[(size_t)cell[i]]; res[U + i] = v[i]; }
    return write_doubles(out, res);
}

int main(int argc, char** argv) {
    if (argc == 4 && std::strcmp(argv[3], "factor") == 0) return factor_file(argv[1], argv[2]);
    if (argc == 3) return steps_file(argv[1], argv[2]);
    const int nsys_set[] = {1, 40, kOnchipStepsMaxSys}, nsteps_set[] = {0, 7, kOnchipStepsMaxSteps}, nrec_set[] = {0, 5, kOnchipWaveMaxRec}, every_set[] = {1, 3};
    for (int n = 6; n <= kOnchipMaxN; n += 2) {
        const long long unknowns = (long long)(n / 2 - 1) * (3 * n / 2 - 1);
        std::printf("N=%d unknowns=%lld ws=", n, unknowns);
        bool first = true;
        for (int nsys : nsys_set)
            for (int nsteps : nsteps_set)
                for (int nrec : nrec_set)
                    for (int every : every_set) {
                        const long long got = onchip_wave_sponge_workspace_bytes(n, nsys, nsteps, nrec, every);
                        const long long want = (long long)nsys * (3LL * 8 * unknowns + 456) + 8 + 16LL * nsys + 8 * unknowns + 4 * 64 + 16LL * nsys + 16LL * nsys;
                        CHECK(got == want, "N=%d nsys=%d nsteps=%d nrec=%d every=%d: %lld workspace bytes, not %lld", n, nsys, nsteps, nrec, every, got, want);
                        CHECK(got == onchip_wave_medium_workspace_bytes(n, nsys, nsteps, nrec, every) + 16LL * nsys, "N=%d nsys=%d: not the medium workspace plus the ranges", n, nsys);
                        std::printf("%s%d:%d:%d:%d:%lld", first ? "" : ",", nsys, nsteps, nrec, every, got);
                        first = false;
                    }
        std::printf("\n");
    }
    for (int n : {0, 4, 7, kOnchipMaxN + 1, kOnchipMaxN + 2}) CHECK(onchip_wave_sponge_workspace_bytes(n, 3, 2, 1, 1) == 0, "N=%d has workspace bytes", n);
    CHECK(onchip_wave_sponge_workspace_bytes(10, 0, 1, 1, 1) == 0 && onchip_wave_sponge_workspace_bytes(10, kOnchipStepsMaxSys + 1, 1, 1, 1) == 0, "a member count outside the limits was not refused");
    CHECK(onchip_wave_sponge_workspace_bytes(10, 1, -1, 1, 1) == 0 && onchip_wave_sponge_workspace_bytes(10, 1, kOnchipStepsMaxSteps + 1, 1, 1) == 0, "a step count outside the limits was not refused");
    CHECK(onchip_wave_sponge_workspace_bytes(10, 1, 1, -1, 1) == 0 && onchip_wave_sponge_workspace_bytes(10, 1, 1, kOnchipWaveMaxRec + 1, 1) == 0, "a receiver count outside the limits was not refused");
    CHECK(onchip_wave_sponge_workspace_bytes(10, 1, 1, 1, 0) == 0, "a cadence below 1 was not refused");
    // no damping: the factor is 1.0 and the damp changes no bit, the sign of a zero included; e = 1, the largest allowed, gives 0
    for (double tau : {1.0, 3.7e-3, 0.1, 6.02e5}) {
        const double s = onchip_wave_sponge_factor(tau, 0.0);
        CHECK(s == 1.0, "a zero damping gives the factor %a at tau = %a", s, tau);
        for (double x : {0.0, -0.0, 1.0, -3.5e-3, 7.25e3, 0.1}) {
            const double y = onchip_wave_damp(s, x);
            CHECK(std::memcmp(&x, &y, sizeof x) == 0, "a unit factor changes %a", x);
        }
    }
    CHECK(onchip_wave_sponge_factor(4.0, kOnchipWaveSpongeMaxE) == 0.0 && onchip_wave_sponge_factor(4.0, 0.5) == 1.0 / 3.0 && onchip_wave_sponge_factor(4.0, 3.0) == -0.5,
          "the factor is not (1 - e) / (1 + e)");
    std::printf("cap %d\n", kOnchipMaxN);
    std::printf("ok %d\n", failures);
    return failures ? 1 : 0;
}
