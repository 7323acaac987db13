// onchip_wave_record_plan_driver.cpp -- the host arithmetic of the explicit wave stepper with a source time function and receiver
// traces (csrc/onchip_plan.h) on the CPU, under the sanitizers (tests/test_onchip_wave_record_cpu.py).
//
// Without arguments: for every even N from 6 to kOnchipMaxN the workspace bytes of several (nsys, nsteps, nrec, record_every) are
// restated from the documented formula -- the Verlet workspace and the image cells of kOnchipWaveMaxRec receivers --, and are 0
// (refused) for what the Verlet workspace refuses, for nrec outside 0 .. kOnchipWaveMaxRec and for record_every < 1.  The forcing
// w g is checked to be g itself for w = 1.  Prints "N=<n> unknowns=<u> ws=<nsys>:<nsteps>:<nrec>:<every>:<bytes>,..." per size,
// "FAIL ..." per violation, "cap <N> <receivers>" and "ok <failures>" at the end.
//
// With <in> <out>: whole sourced steps, written as k_oc_wave_record runs them -- the acceleration carried from step to step, formed
// at the entry from (u, g, w[0]) -- with the functions that kernel calls.  <in> holds doubles: n, tau, nsteps, A0, xk, yk,
// record_every, nrec, then the (n+1)^2 cells of an image of u, per unknown in packed order g and v, the nsteps + 1 amplitudes, the
// nrec receivers (packed indices).  <out> receives u and v of every unknown, then (nsteps / record_every) x nrec samples.
// With a third argument `forcing`: <in> holds count, then count amplitudes and count values of g; <out> receives their products.
// Compile with -ffp-contract=off, as the library is.
#include "../../iterative_solvers_amd/csrc/onchip_plan.h"

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

static int forcing_file(const char* in, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    double head = 0;
    if (std::fread(&head, sizeof(double), 1, f) != 1 || head < 0 || head > 1e6) { std::fclose(f); return 2; }
    std::vector<double> w((size_t)head), g((size_t)head), res((size_t)head);
    const bool read = read_doubles(f, w) && read_doubles(f, g);
    std::fclose(f);
    if (!read) return 2;
    for (size_t i = 0; i < res.size(); ++i) res[i] = onchip_wave_forcing(w[i], g[i]);
    return write_doubles(out, res);
}

static int steps_file(const char* in, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    double head[8];
    if (std::fread(head, sizeof(double), 8, f) != 8) { std::fclose(f); return 2; }
    const int n = (int)head[0], nsteps = (int)head[2], every = (int)head[6], nrec = (int)head[7];
    const OnchipPlan pl = onchip_plan(n);
    if (pl.n != n || nsteps < 0 || nsteps > kOnchipStepsMaxSteps || every < 1 || nrec < 0 || nrec > kOnchipWaveMaxRec) { std::fclose(f); return 3; }
    const double tau = head[1], h = 0.5 * tau;
    const OnchipWaveCoef k{head[3], head[4], head[5]};
    const size_t U = (size_t)pl.unknowns, samples = (size_t)(nsteps / every);
    std::vector<double> img((size_t)pl.cells), g(U), v(U), w((size_t)nsteps + 1), rec((size_t)nrec), res(2 * U + samples * (size_t)nrec);
    const bool read = read_doubles(f, img) && read_doubles(f, g) && read_doubles(f, v) && read_doubles(f, w) && read_doubles(f, rec);
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
        return onchip_wave_accel(k, onchip_wave_forcing(wn, g[i]), img[c], img[c - 1], img[c + 1], img[c - p], img[c + p]);
    };
    std::vector<double> a(U);
    for (size_t i = 0; i < U; ++i) a[i] = accel(i, w[0]);
    double* sample = res.data() + 2 * U;
    for (int s = 0; s < nsteps; ++s) {
        for (size_t i = 0; i < U; ++i) {                                            // between the two barriers: owned cells only
            v[i] = onchip_wave_kick(v[i], h, a[i]);
            img[(size_t)cell[i]] = onchip_wave_drift(img[(size_t)cell[i]], tau, v[i]);
        }
        for (size_t i = 0; i < U; ++i) { a[i] = accel(i, w[(size_t)s + 1]); v[i] = onchip_wave_kick(v[i], h, a[i]); }
        if ((s + 1) % every == 0) for (int r = 0; r < nrec; ++r) *sample++ = img[(size_t)rcell[(size_t)r]];
    }
    for (size_t i = 0; i < U; ++i) { res[i] = img[(size_t)cell[i]]; res[U + i] = v[i]; }
    return write_doubles(out, res);
}

int main(int argc, char** argv) {
    if (argc == 4 && std::strcmp(argv[3], "forcing") == 0) return forcing_file(argv[1], argv[2]);
    if (argc == 3) return steps_file(argv[1], argv[2]);
    const int nsys_set[] = {1, 40, kOnchipStepsMaxSys}, nsteps_set[] = {0, 7, kOnchipStepsMaxSteps}, nrec_set[] = {0, 1, 5, kOnchipWaveMaxRec}, every_set[] = {1, 3, 100000};
    for (int n = 6; n <= kOnchipMaxN; n += 2) {
        const long long unknowns = (long long)(n / 2 - 1) * (3 * n / 2 - 1);
        std::printf("N=%d unknowns=%lld ws=", n, unknowns);
        bool first = true;
        for (int nsys : nsys_set)
            for (int nsteps : nsteps_set)
                for (int nrec : nrec_set)
                    for (int every : every_set) {
                        const long long got = onchip_wave_record_workspace_bytes(n, nsys, nsteps, nrec, every);
                        const long long want = (long long)nsys * (3LL * 8 * unknowns + 456) + 8 + 16LL * nsys + 8 * unknowns + 4 * 64;
                        CHECK(got == want, "N=%d nsys=%d nsteps=%d nrec=%d every=%d: %lld workspace bytes, not %lld", n, nsys, nsteps, nrec, every, got, want);
                        CHECK(got == onchip_wave_workspace_bytes(n, nsys, nsteps, kWaveVerlet, 0) + 4LL * kOnchipWaveMaxRec, "N=%d nsys=%d: not the Verlet workspace plus the receiver cells", n, nsys);
                        std::printf("%s%d:%d:%d:%d:%lld", first ? "" : ",", nsys, nsteps, nrec, every, got);
                        first = false;
                    }
        std::printf("\n");
    }
    for (int n : {0, 4, 7, kOnchipMaxN + 1, kOnchipMaxN + 2}) CHECK(onchip_wave_record_workspace_bytes(n, 3, 2, 1, 1) == 0, "N=%d has workspace bytes", n);
    CHECK(onchip_wave_record_workspace_bytes(10, 0, 1, 1, 1) == 0 && onchip_wave_record_workspace_bytes(10, kOnchipStepsMaxSys + 1, 1, 1, 1) == 0, "a member count outside the limits was not refused");
    CHECK(onchip_wave_record_workspace_bytes(10, 1, -1, 1, 1) == 0 && onchip_wave_record_workspace_bytes(10, 1, kOnchipStepsMaxSteps + 1, 1, 1) == 0, "a step count outside the limits was not refused");
    CHECK(onchip_wave_record_workspace_bytes(10, 1, 1, -1, 1) == 0 && onchip_wave_record_workspace_bytes(10, 1, 1, kOnchipWaveMaxRec + 1, 1) == 0, "a receiver count outside the limits was not refused");
    CHECK(onchip_wave_record_workspace_bytes(10, 1, 1, 1, 0) == 0 && onchip_wave_record_workspace_bytes(10, 1, 1, 0, -3) == 0, "a cadence below 1 was not refused");
    CHECK(kOnchipWaveMaxRec == 64 && 2 * 64 * 8 <= kOnchipSideBytes, "the receivers fit in one wave, two blocks of 64 amplitudes in the side data");
    for (double g : {0.0, -0.0, 1.0, -3.5e-300, 7.25e300, 0.1}) {
        const double f = onchip_wave_forcing(1.0, g);
        CHECK(std::memcmp(&f, &g, sizeof f) == 0, "1.0 * %a is not %a", g, g);
    }
    std::printf("cap %d %d\n", kOnchipMaxN, kOnchipWaveMaxRec);
    std::printf("ok %d\n", failures);
    return failures ? 1 : 0;
}
