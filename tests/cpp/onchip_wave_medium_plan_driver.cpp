// onchip_wave_medium_plan_driver.cpp -- the host arithmetic of the recorded explicit wave stepper in a medium (csrc/onchip_plan.h,
// DESIGN section 12.5) on the CPU, under the sanitizers (tests/test_onchip_wave_medium_cpu.py).
//
// Without arguments: for every even N from 6 to kOnchipMaxN the workspace bytes of several (nsys, nsteps, nrec, record_every) are
// restated from the documented formula -- the recorded call's workspace and 16 bytes per member --, and are 0 (refused) for what
// that workspace refuses.  A unit medium is checked to give onchip_wave_accel's bits and c2max = 1 onchip_wave_cfl's.  Prints
// "N=<n> unknowns=<u> ws=<nsys>:<nsteps>:<nrec>:<every>:<bytes>,..." per size, "FAIL ..." per violation, "cap <N>" and
// "ok <failures>" at the end.
//
// With <in> <out>: whole steps in a medium, written as k_oc_wave_medium runs them -- the acceleration carried from step to step,
// formed at the entry from (u, g, c2, w[0]) -- with the functions that kernel calls.  <in> holds doubles: n, tau, nsteps, A0, xk, yk,
// record_every, nrec, then the (n+1)^2 cells of an image of u, per unknown in packed order g, v and c2, the nsteps + 1 amplitudes,
// the nrec receivers (packed indices).  <out> receives u and v of every unknown, then (nsteps / record_every) x nrec samples.
// With a third argument `accel`: <in> holds count, A0, xk, yk, then count values each of c2, f, uc, left, right, down, up; <out>
// receives onchip_wave_medium_accel of them.  With `cfl`: count, then count values each of A0 and c2max; <out> the bounds.
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

static int accel_file(const char* in, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    double head[4];
    if (std::fread(head, sizeof(double), 4, f) != 4 || head[0] < 0 || head[0] > 1e6) { std::fclose(f); return 2; }
    const size_t count = (size_t)head[0];
    const OnchipWaveCoef k{head[1], head[2], head[3]};
    std::vector<double> col[7], res(count);
    bool read = true;
    for (auto& c : col) { c.resize(count); read = read && read_doubles(f, c); }
    std::fclose(f);
    if (!read) return 2;
    for (size_t i = 0; i < count; ++i) res[i] = onchip_wave_medium_accel(k, col[0][i], col[1][i], col[2][i], col[3][i], col[4][i], col[5][i], col[6][i]);
    return write_doubles(out, res);
}

static int cfl_file(const char* in, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    double head = 0;
    if (std::fread(&head, sizeof(double), 1, f) != 1 || head < 0 || head > 1e6) { std::fclose(f); return 2; }
    std::vector<double> A0((size_t)head), top((size_t)head), res((size_t)head);
    const bool read = read_doubles(f, A0) && read_doubles(f, top);
    std::fclose(f);
    if (!read) return 2;
    for (size_t i = 0; i < res.size(); ++i) res[i] = onchip_wave_medium_cfl(A0[i], top[i]);
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
    std::vector<double> img((size_t)pl.cells), g(U), v(U), c2(U), w((size_t)nsteps + 1), rec((size_t)nrec), res(2 * U + samples * (size_t)nrec);
    const bool read = read_doubles(f, img) && read_doubles(f, g) && read_doubles(f, v) && read_doubles(f, c2) && read_doubles(f, w) && read_doubles(f, rec);
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
    if (argc == 4 && std::strcmp(argv[3], "accel") == 0) return accel_file(argv[1], argv[2]);
    if (argc == 4 && std::strcmp(argv[3], "cfl") == 0) return cfl_file(argv[1], argv[2]);
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
                        const long long got = onchip_wave_medium_workspace_bytes(n, nsys, nsteps, nrec, every);
                        const long long want = (long long)nsys * (3LL * 8 * unknowns + 456) + 8 + 16LL * nsys + 8 * unknowns + 4 * 64 + 16LL * nsys;
                        CHECK(got == want, "N=%d nsys=%d nsteps=%d nrec=%d every=%d: %lld workspace bytes, not %lld", n, nsys, nsteps, nrec, every, got, want);
                        CHECK(got == onchip_wave_record_workspace_bytes(n, nsys, nsteps, nrec, every) + 16LL * nsys, "N=%d nsys=%d: not the recorded workspace plus the ranges", n, nsys);
                        std::printf("%s%d:%d:%d:%d:%lld", first ? "" : ",", nsys, nsteps, nrec, every, got);
                        first = false;
                    }
        std::printf("\n");
    }
    for (int n : {0, 4, 7, kOnchipMaxN + 1, kOnchipMaxN + 2}) CHECK(onchip_wave_medium_workspace_bytes(n, 3, 2, 1, 1) == 0, "N=%d has workspace bytes", n);
    CHECK(onchip_wave_medium_workspace_bytes(10, 0, 1, 1, 1) == 0 && onchip_wave_medium_workspace_bytes(10, kOnchipStepsMaxSys + 1, 1, 1, 1) == 0, "a member count outside the limits was not refused");
    CHECK(onchip_wave_medium_workspace_bytes(10, 1, -1, 1, 1) == 0 && onchip_wave_medium_workspace_bytes(10, 1, kOnchipStepsMaxSteps + 1, 1, 1) == 0, "a step count outside the limits was not refused");
    CHECK(onchip_wave_medium_workspace_bytes(10, 1, 1, -1, 1) == 0 && onchip_wave_medium_workspace_bytes(10, 1, 1, kOnchipWaveMaxRec + 1, 1) == 0, "a receiver count outside the limits was not refused");
    CHECK(onchip_wave_medium_workspace_bytes(10, 1, 1, 1, 0) == 0, "a cadence below 1 was not refused");
    // a unit medium: the bits of the homogeneous expression; c2max = 1: the bits of the homogeneous bound
    const OnchipWaveCoef k{-1234.5678, 300.1, 317.1839};
    for (double x : {0.0, 1.0, -3.5e-3, 7.25e3, 0.1}) {
        const double a = onchip_wave_medium_accel(k, 1.0, 0.3 * x, x, 0.7 * x, -x, 1.1 * x, 0.4), b = onchip_wave_accel(k, 0.3 * x, x, 0.7 * x, -x, 1.1 * x, 0.4);
        CHECK(std::memcmp(&a, &b, sizeof a) == 0, "a unit medium changes the acceleration at %a", x);
    }
    for (double A0 : {-1.0, -800.0, -1234.5678, -131072.0, -3.3e7}) {
        const double a = onchip_wave_medium_cfl(A0, 1.0), b = onchip_wave_cfl(A0);
        CHECK(std::memcmp(&a, &b, sizeof a) == 0, "c2max = 1 changes the bound of A0 = %a", A0);
    }
    std::printf("cap %d\n", kOnchipMaxN);
    std::printf("ok %d\n", failures);
    return failures ? 1 : 0;
}
