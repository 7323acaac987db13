// onchip_steps_plan_driver.cpp -- the host arithmetic of the on-chip ensemble stepper (csrc/onchip_plan.h) on the
// CPU, under the sanitizers (tests/test_onchip_steps_cpu.py).
//
// Without arguments: for every even N from 6 to kOnchipMaxN the workspace bytes of several (nsys, nsteps, with / without iteration
// counts) are restated here from the documented formula -- the batch workspace, 16 bytes per member, one packed vector, 4 bytes per
// count --, must not fall when an argument grows, and are 0 (refused) above the limits and for sizes the plan refuses; the budget
// word must lie in the side data behind the CG state.  Prints "N=<n> unknowns=<u> ws=<nsys>:<nsteps>:<with>:<bytes>,..." per size,
// "FAIL ..." per violation and "ok <failures>" at the end.
//
// With <in> <out>: the per-node right-hand side of a step, onchip_step_rhs -- the function k_onchip_steps calls -- over an image.
// <in> holds doubles: n, theta, sigma, A0, xk, yk, then the (n+1)^2 cells of an image of u, then g for every unknown in packed
// order.  <out> receives b_step of every unknown in packed order, each evaluated at the unknown's cell with the neighbours the
// kernel hands over: cell - 1, cell + 1, cell - pitch, cell + pitch.  Compile with -ffp-contract=off, as the library is.
#include "../../iterative_solvers_amd/csrc/onchip_plan.h"

#include <cstdio>
#include <vector>

using namespace mi355cg;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

static int step_rhs_file(const char* in, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    double head[6];
    if (std::fread(head, sizeof(double), 6, f) != 6) { std::fclose(f); return 2; }
    const int n = (int)head[0];
    const OnchipPlan pl = onchip_plan(n);
    if (pl.n != n) { std::fclose(f); return 3; }
    const double theta = head[1], sigma = head[2];
    const OnchipStepCoef k{head[3], head[4], head[5], theta, (1.0 - theta) / theta, theta < 1.0 ? 1 : 0};
    std::vector<double> img((size_t)pl.cells), g((size_t)pl.unknowns), b((size_t)pl.unknowns);
    const bool read = std::fread(img.data(), sizeof(double), img.size(), f) == img.size() && std::fread(g.data(), sizeof(double), g.size(), f) == g.size();
    std::fclose(f);
    if (!read) return 2;
    for (int i = 0; i < pl.unknowns; ++i) {
        int x, y;
        onchip_node(pl, i, &x, &y);
        const int c = onchip_cell(pl, x, y);
        b[(size_t)i] = onchip_step_rhs(k, sigma, g[(size_t)i], img[(size_t)c], img[(size_t)(c - 1)], img[(size_t)(c + 1)], img[(size_t)(c - pl.pitch)],
                                       img[(size_t)(c + pl.pitch)]);
    }
    std::FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    const bool wrote = std::fwrite(b.data(), sizeof(double), b.size(), o) == b.size();
    std::fclose(o);
    return wrote ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc == 3) return step_rhs_file(argv[1], argv[2]);
    const int nsys_set[] = {1, 2, 40, 4096, kOnchipStepsMaxSys}, nsteps_set[] = {0, 1, 7, 100, 1024, kOnchipStepsMaxSteps};
    for (int n = 6; n <= kOnchipMaxN; n += 2) {
        const long long unknowns = (long long)(n / 2 - 1) * (3 * n / 2 - 1);
        std::printf("N=%d unknowns=%lld ws=", n, unknowns);
        bool first = true;
        for (int with = 0; with <= 1; ++with) {
            long long prev_sys = 0;
            for (int nsys : nsys_set) {
                long long prev_steps = 0, all_steps = 0;
                for (int nsteps : nsteps_set) {
                    const long long counts = with ? (long long)nsys * nsteps : 0, got = onchip_steps_workspace_bytes(n, nsys, nsteps, with);
                    if (counts > kOnchipStepsMaxCounts) { CHECK(got == 0, "N=%d nsys=%d nsteps=%d: %lld counts were not refused", n, nsys, nsteps, counts); continue; }
                    const long long want = (long long)nsys * (3LL * 8 * unknowns + 456) + 8 + 16LL * nsys + 8 * unknowns + 4 * counts;
                    CHECK(got == want, "N=%d nsys=%d nsteps=%d with=%d: %lld workspace bytes, not %lld", n, nsys, nsteps, with, got, want);
                    CHECK(got == onchip_many_workspace_bytes(n, nsys) + 16LL * nsys + 8 * unknowns + 4 * counts, "N=%d nsys=%d: not the batch workspace plus the stepping parts", n, nsys);
                    CHECK(got >= prev_steps && (!with || nsteps == 0 || got > prev_steps), "N=%d nsys=%d with=%d: %lld bytes at %d steps after %lld", n, nsys, with, got, nsteps, prev_steps);
                    CHECK(got >= onchip_steps_workspace_bytes(n, nsys, nsteps, 0), "N=%d nsys=%d nsteps=%d: the counts make the workspace smaller", n, nsys, nsteps);
                    prev_steps = got;
                    if (nsteps == 7) all_steps = got;
                    std::printf("%s%d:%d:%d:%lld", first ? "" : ",", nsys, nsteps, with, got);
                    first = false;
                }
                CHECK(all_steps > prev_sys, "N=%d with=%d: %lld bytes at %d members after %lld", n, with, all_steps, nsys, prev_sys);
                prev_sys = all_steps;
            }
        }
        std::printf("\n");
        if (n > 6) CHECK(onchip_steps_workspace_bytes(n, 40, 7, 1) > onchip_steps_workspace_bytes(n - 2, 40, 7, 1), "N=%d: no more bytes than N=%d", n, n - 2);
    }
    for (int n : {0, 4, 7, kOnchipMaxN + 1, kOnchipMaxN + 2}) CHECK(onchip_steps_workspace_bytes(n, 3, 2, 1) == 0, "N=%d has workspace bytes", n);
    CHECK(onchip_steps_workspace_bytes(10, 0, 1, 0) == 0 && onchip_steps_workspace_bytes(10, -1, 1, 0) == 0, "an empty ensemble has workspace bytes");
    CHECK(onchip_steps_workspace_bytes(10, kOnchipStepsMaxSys + 1, 1, 0) == 0, "more members than the limit were not refused");
    CHECK(onchip_steps_workspace_bytes(10, 1, -1, 0) == 0 && onchip_steps_workspace_bytes(10, 1, kOnchipStepsMaxSteps + 1, 0) == 0, "a step count outside the limits was not refused");
    CHECK(onchip_steps_workspace_bytes(10, 1024, 65536, 1) > 0 && onchip_steps_workspace_bytes(10, 1025, 65536, 1) == 0, "the limit of 2^26 counts");
    CHECK(onchip_steps_workspace_bytes(10, 1025, 65536, 0) > 0, "the limit of the counts applies without counts");
    CHECK(kOnchipStepsMaxSys == 65536 && kOnchipStepsMaxSteps == 65536 && kOnchipStepsMaxCounts == (1LL << 26), "the limits of an ensemble");
    CHECK(kOnchipBudgetOffset >= kOnchipSideBytes - 256 + 184 && kOnchipBudgetOffset + 4 <= kOnchipSideBytes, "the budget word is outside the side data or inside the CG state");
    std::printf("cap %d\n", kOnchipMaxN);
    std::printf("ok %d\n", failures);
    return failures ? 1 : 0;
}
