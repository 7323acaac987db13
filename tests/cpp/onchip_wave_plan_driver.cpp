// onchip_wave_plan_driver.cpp -- the host arithmetic of the on-chip wave steppers (csrc/onchip_plan.h) on the CPU,
// under the sanitizers (tests/test_onchip_wave_cpu.py).
//
// Without arguments: for every even N from 6 to kOnchipMaxN the workspace bytes of several (nsys, nsteps, scheme, with / without
// iteration counts) are restated here from the documented formula -- Verlet: the batch workspace, 16 bytes per member, one packed
// vector; Newmark: the stepping workspace and 16 bytes per member --, and are 0 (refused) above the limits, for sizes the plan
// refuses and for an unknown scheme.  Prints "N=<n> unknowns=<u> ws=<nsys>:<nsteps>:<scheme>:<with>:<bytes>,..." per size, "FAIL ..."
// per violation, "cfl <n> <width> <height> <A_diag> <bound>" (hex floats) for some grids and "ok <failures>" at the end.
//
// With <in> <out>: the per-node expressions of both schemes -- the functions k_onchip_wave_verlet and k_onchip_wave_newmark call --
// over an image.  <in> holds doubles: n, scheme, tau, nsteps, A0, xk, yk, then the (n+1)^2 cells of an image of u, then per unknown
// in packed order g, v and x.  Verlet: nsteps steps of the kernel's loop on the image, the acceleration carried from step to step;
// <out> receives u, then v of every unknown.  Newmark: <out> receives the right-hand side of the step from (u, v), then the new
// velocity hv (x - u) - v.  Every expression is evaluated at the unknown's cell with the neighbours the kernels hand over: cell - 1,
// cell + 1, cell - pitch, cell + pitch.  Compile with -ffp-contract=off, as the library is.
#include "../../iterative_solvers_amd/csrc/onchip_plan.h"

#include <cstdio>
#include <vector>

using namespace mi355cg;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

static int wave_file(const char* in, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    double head[7];
    if (std::fread(head, sizeof(double), 7, f) != 7) { std::fclose(f); return 2; }
    const int n = (int)head[0], scheme = (int)head[1], nsteps = (int)head[3];
    const OnchipPlan pl = onchip_plan(n);
    if (pl.n != n) { std::fclose(f); return 3; }
    const double tau = head[2];
    const OnchipWaveCoef k{head[4], head[5], head[6]};
    const size_t U = (size_t)pl.unknowns;
    std::vector<double> img((size_t)pl.cells), g(U), v(U), x(U), res(2 * U);
    const bool read = std::fread(img.data(), sizeof(double), img.size(), f) == img.size() && std::fread(g.data(), sizeof(double), U, f) == U &&
                      std::fread(v.data(), sizeof(double), U, f) == U && std::fread(x.data(), sizeof(double), U, f) == U;
    std::fclose(f);
    if (!read) return 2;
    std::vector<int> cell(U);
    for (int i = 0; i < pl.unknowns; ++i) { int xx, yy; onchip_node(pl, i, &xx, &yy); cell[(size_t)i] = onchip_cell(pl, xx, yy); }
    auto accel = [&](size_t i) {
        const size_t c = (size_t)cell[i], p = (size_t)pl.pitch;
        return onchip_wave_accel(k, g[i], img[c], img[c - 1], img[c + 1], img[c - p], img[c + p]);
    };
    if (scheme == kWaveVerlet) {
        const double h = 0.5 * tau;
        std::vector<double> a(U);
        for (size_t i = 0; i < U; ++i) a[i] = accel(i);
        for (int s = 0; s < nsteps; ++s) {
            for (size_t i = 0; i < U; ++i) {                                        // between the two barriers: owned cells only
                v[i] = onchip_wave_kick(v[i], h, a[i]);
                img[(size_t)cell[i]] = onchip_wave_drift(img[(size_t)cell[i]], tau, v[i]);
            }
            for (size_t i = 0; i < U; ++i) { a[i] = accel(i); v[i] = onchip_wave_kick(v[i], h, a[i]); }
        }
        for (size_t i = 0; i < U; ++i) { res[i] = img[(size_t)cell[i]]; res[U + i] = v[i]; }
    } else if (scheme == kWaveNewmark) {
        const double sigma = 4.0 / (tau * tau), hv = 2.0 / tau;
        for (size_t i = 0; i < U; ++i) {
            const size_t c = (size_t)cell[i], p = (size_t)pl.pitch;
            res[i] = onchip_newmark_rhs(k, sigma, tau, g[i], v[i], img[c], img[c - 1], img[c + 1], img[c - p], img[c + p]);
            res[U + i] = onchip_newmark_velocity(hv, x[i], img[c], v[i]);
        }
    } else return 3;
    std::FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    const bool wrote = std::fwrite(res.data(), sizeof(double), res.size(), o) == res.size();
    std::fclose(o);
    return wrote ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc == 3) return wave_file(argv[1], argv[2]);
    const int nsys_set[] = {1, 2, 40, 4096, kOnchipStepsMaxSys}, nsteps_set[] = {0, 1, 7, 1024, kOnchipStepsMaxSteps};
    for (int n = 6; n <= kOnchipMaxN; n += 2) {
        const long long unknowns = (long long)(n / 2 - 1) * (3 * n / 2 - 1);
        std::printf("N=%d unknowns=%lld ws=", n, unknowns);
        bool first = true;
        for (int scheme : {kWaveVerlet, kWaveNewmark})
            for (int with = 0; with <= 1; ++with)
                for (int nsys : nsys_set)
                    for (int nsteps : nsteps_set) {
                        const long long counts = with && scheme == kWaveNewmark ? (long long)nsys * nsteps : 0;
                        const long long got = onchip_wave_workspace_bytes(n, nsys, nsteps, scheme, with);
                        if (counts > kOnchipStepsMaxCounts) { CHECK(got == 0, "N=%d nsys=%d nsteps=%d: %lld counts were not refused", n, nsys, nsteps, counts); continue; }
                        const long long batch = (long long)nsys * (3LL * 8 * unknowns + 456) + 8;
                        const long long want = scheme == kWaveVerlet ? batch + 16LL * nsys + 8 * unknowns
                                                                     : batch + 16LL * nsys + 8 * unknowns + 4 * counts + 16LL * nsys;
                        CHECK(got == want, "N=%d nsys=%d nsteps=%d scheme=%d with=%d: %lld workspace bytes, not %lld", n, nsys, nsteps, scheme, with, got, want);
                        CHECK(scheme == kWaveVerlet ? got == onchip_many_workspace_bytes(n, nsys) + 16LL * nsys + 8 * unknowns
                                                    : got == onchip_steps_workspace_bytes(n, nsys, nsteps, with) + 16LL * nsys,
                              "N=%d nsys=%d scheme=%d: not the driver's workspace plus the wave parts", n, nsys, scheme);
                        std::printf("%s%d:%d:%d:%d:%lld", first ? "" : ",", nsys, nsteps, scheme, with, got);
                        first = false;
                    }
        std::printf("\n");
        if (n > 6) CHECK(onchip_wave_workspace_bytes(n, 40, 7, kWaveVerlet, 0) > onchip_wave_workspace_bytes(n - 2, 40, 7, kWaveVerlet, 0), "N=%d: no more bytes than N=%d", n, n - 2);
    }
    for (int scheme : {kWaveVerlet, kWaveNewmark}) {
        for (int n : {0, 4, 7, kOnchipMaxN + 1, kOnchipMaxN + 2}) CHECK(onchip_wave_workspace_bytes(n, 3, 2, scheme, 1) == 0, "N=%d has workspace bytes", n);
        CHECK(onchip_wave_workspace_bytes(10, 0, 1, scheme, 0) == 0 && onchip_wave_workspace_bytes(10, -1, 1, scheme, 0) == 0, "an empty ensemble has workspace bytes");
        CHECK(onchip_wave_workspace_bytes(10, kOnchipStepsMaxSys + 1, 1, scheme, 0) == 0, "more members than the limit were not refused");
        CHECK(onchip_wave_workspace_bytes(10, 1, -1, scheme, 0) == 0 && onchip_wave_workspace_bytes(10, 1, kOnchipStepsMaxSteps + 1, scheme, 0) == 0, "a step count outside the limits was not refused");
    }
    CHECK(onchip_wave_workspace_bytes(10, 3, 2, -1, 0) == 0 && onchip_wave_workspace_bytes(10, 3, 2, 2, 0) == 0, "an unknown scheme has workspace bytes");
    CHECK(onchip_wave_workspace_bytes(10, 1024, 65536, kWaveNewmark, 1) > 0 && onchip_wave_workspace_bytes(10, 1025, 65536, kWaveNewmark, 1) == 0, "the limit of 2^26 counts");
    CHECK(onchip_wave_workspace_bytes(10, 1025, 65536, kWaveVerlet, 1) > 0, "the explicit scheme keeps no counts: their limit does not apply");
    CHECK(kWaveVerlet == 0 && kWaveNewmark == 1 && kOnchipWaveSysBytes == 16 && kOnchipWaveDefaultSteps >= 1, "the constants of the wave steppers");
    const double A0 = -2.0 * (100.0 + 170.0);
    CHECK(onchip_wave_cfl(A0) == 2.0 / std::sqrt(2.0 * 540.0) && onchip_wave_cfl(-A0) == onchip_wave_cfl(A0), "the bound on tau");
    // "cfl <n> <width> <height> <A0> <bound>": the bound of an n x n grid on a width x height domain, the diagonal as grid_setup.cpp forms it
    for (int n : {6, 10, 20, 64})
        for (double height : {1.0, 1.7}) {
            const double hx = 1.0 / n, hy = height / n, diag = -2 * (1 / (hx * hx) + 1 / (hy * hy));
            std::printf("cfl %d %a %a %a %a\n", n, 1.0, height, diag, onchip_wave_cfl(diag));
        }
    std::printf("cap %d\n", kOnchipMaxN);
    std::printf("ok %d\n", failures);
    return failures ? 1 : 0;
}
