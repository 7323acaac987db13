// onchip_wave_adjoint_plan_driver.cpp -- the host arithmetic of the adjoint of the recorded explicit wave stepper in a medium
// (csrc/onchip_plan.h) on the CPU, under the sanitizers (tests/test_onchip_wave_adjoint_cpu.py).
//
// Without arguments: for every even N from 6 to kOnchipMaxN the bytes of a history and of the adjoint call's workspace are restated
// from the documented formulas -- 8 nsys (nsteps + 1) unknowns, and the medium call's workspace --, and are 0 (refused) for what
// the calls refuse.  The two halves of the acceleration are checked to give onchip_wave_medium_accel's bits.  Prints
// "N=<n> unknowns=<u> hist=<nsys>:<nsteps>:<bytes>,... ws=<nsys>:<nsteps>:<nrec>:<every>:<bytes>,..." per size, "FAIL ..." per
// violation, "cap <N>" and "ok <failures>" at the end.
//
// With <in> <out>: whole backward steps, written as k_oc_wave_adjoint runs them -- the first half of the first step at the entry,
// then per step the drift, one stencil pass and both kicks from it with the injection between -- with the functions that kernel
// calls.  <in> holds doubles: n, tau, nsteps, A0, xk, yk, record_every, nrec, then the (n+1)^2 cells of an image of q, per
// unknown in packed order lam, S and c2, the (nsteps + 1) x unknowns history, the (nsteps / record_every) x nrec adjoint sources,
// the nrec receivers (packed indices).  <out> receives lam, q and S of every unknown.
// With a third argument `forward`: whole forward steps as k_oc_wave_history runs them.  <in>: onchip_wave_medium_plan_driver's
// (n, tau, nsteps, A0, xk, yk, record_every, nrec, the image of u, g, v, c2, the amplitudes, the receivers); <out> receives u, v,
// the samples, then the (nsteps + 1) x unknowns history.
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

struct Head { int n, nsteps, every, nrec; double tau; OnchipWaveCoef k; OnchipPlan pl; };
static bool read_head(std::FILE* f, Head& hd) {
    double head[8];
    if (std::fread(head, sizeof(double), 8, f) != 8) return false;
    hd.n = (int)head[0]; hd.nsteps = (int)head[2]; hd.every = (int)head[6]; hd.nrec = (int)head[7];
    hd.tau = head[1]; hd.k = OnchipWaveCoef{head[3], head[4], head[5]};
    hd.pl = onchip_plan(hd.n);
    return hd.pl.n == hd.n && hd.nsteps >= 0 && hd.nsteps <= kOnchipStepsMaxSteps && hd.every >= 1 && hd.nrec >= 0 && hd.nrec <= kOnchipWaveMaxRec;
}
static std::vector<int> cells_of(const OnchipPlan& pl) {
    std::vector<int> cell((size_t)pl.unknowns);
    for (int i = 0; i < pl.unknowns; ++i) { int xx, yy; onchip_node(pl, i, &xx, &yy); cell[(size_t)i] = onchip_cell(pl, xx, yy); }
    return cell;
}

static int backward_file(const char* in, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    Head hd;
    if (!read_head(f, hd)) { std::fclose(f); return 3; }
    const OnchipPlan& pl = hd.pl;
    const double tau = hd.tau, h = 0.5 * tau;
    const int nsteps = hd.nsteps, every = hd.every, nrec = hd.nrec;
    const size_t U = (size_t)pl.unknowns, samples = (size_t)(nsteps / every);
    std::vector<double> img((size_t)pl.cells), lam(U), S(U), c2(U), H(((size_t)nsteps + 1) * U), adj(samples * (size_t)nrec), rec((size_t)nrec), res(3 * U);
    const bool read = read_doubles(f, img) && read_doubles(f, lam) && read_doubles(f, S) && read_doubles(f, c2) && read_doubles(f, H) && read_doubles(f, adj) && read_doubles(f, rec);
    std::fclose(f);
    if (!read) return 2;
    const std::vector<int> cell = cells_of(pl);
    for (int r = 0; r < nrec; ++r) if (rec[(size_t)r] < 0 || rec[(size_t)r] >= (double)pl.unknowns) return 3;
    auto stencil = [&](size_t i) {
        const size_t c = (size_t)cell[i], p = (size_t)pl.pitch;
        return onchip_wave_au(hd.k, img[c], img[c - 1], img[c + 1], img[c - p], img[c + p]);
    };
    auto inject = [&](int s) {                                                          // state index s is sampled: its row, ascending
        const double* row = adj.data() + ((size_t)(s / every) - 1) * (size_t)nrec;
        for (int j = 0; j < nrec; ++j) { const size_t i = (size_t)rec[(size_t)j]; lam[i] = onchip_wave_adjoint_inject(lam[i], row[j]); }
    };
    if (nsteps > 0) {
        std::vector<double> aq(U);
        // the entry: the first half of step nsteps
        if (nsteps % every == 0) inject(nsteps);
        for (size_t i = 0; i < U; ++i) aq[i] = stencil(i);
        for (size_t i = 0; i < U; ++i) {
            S[i] = onchip_wave_adjoint_sens(S[i], img[(size_t)cell[i]], H[(size_t)nsteps * U + i]);
            lam[i] = onchip_wave_adjoint_kick(lam[i], h, aq[i]);
        }
        for (int s = nsteps; s > 0; --s) {
            for (size_t i = 0; i < U; ++i) img[(size_t)cell[i]] = onchip_wave_adjoint_drift(img[(size_t)cell[i]], tau, c2[i], lam[i]);   // between the barriers
            for (size_t i = 0; i < U; ++i) aq[i] = stencil(i);
            const bool more = s - 1 > 0;
            for (size_t i = 0; i < U; ++i) {
                S[i] = onchip_wave_adjoint_sens(S[i], img[(size_t)cell[i]], H[(size_t)(s - 1) * U + i]);
                lam[i] = onchip_wave_adjoint_kick(lam[i], h, aq[i]);
            }
            if (!more) break;
            if ((s - 1) % every == 0) inject(s - 1);                                    // the first half of step s - 1, with the same au(q)
            for (size_t i = 0; i < U; ++i) {
                S[i] = onchip_wave_adjoint_sens(S[i], img[(size_t)cell[i]], H[(size_t)(s - 1) * U + i]);
                lam[i] = onchip_wave_adjoint_kick(lam[i], h, aq[i]);
            }
        }
    }
    for (size_t i = 0; i < U; ++i) { res[i] = lam[i]; res[U + i] = img[(size_t)cell[i]]; res[2 * U + i] = S[i]; }
    return write_doubles(out, res);
}

static int forward_file(const char* in, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    Head hd;
    if (!read_head(f, hd)) { std::fclose(f); return 3; }
    const OnchipPlan& pl = hd.pl;
    const double tau = hd.tau, h = 0.5 * tau;
    const int nsteps = hd.nsteps, every = hd.every, nrec = hd.nrec;
    const size_t U = (size_t)pl.unknowns, samples = (size_t)(nsteps / every);
    std::vector<double> img((size_t)pl.cells), g(U), v(U), c2(U), w((size_t)nsteps + 1), rec((size_t)nrec), res(2 * U + samples * (size_t)nrec + ((size_t)nsteps + 1) * U);
    const bool read = read_doubles(f, img) && read_doubles(f, g) && read_doubles(f, v) && read_doubles(f, c2) && read_doubles(f, w) && read_doubles(f, rec);
    std::fclose(f);
    if (!read) return 2;
    const std::vector<int> cell = cells_of(pl);
    for (int r = 0; r < nrec; ++r) if (rec[(size_t)r] < 0 || rec[(size_t)r] >= (double)pl.unknowns) return 3;
    double* sample = res.data() + 2 * U;
    double* hist = res.data() + 2 * U + samples * (size_t)nrec;
    auto pass = [&](int row, double wn, bool second, bool first) {                      // one stencil pass: the row, then the kicks it feeds
        std::vector<double> au(U);
        for (size_t i = 0; i < U; ++i) {
            const size_t c = (size_t)cell[i], p = (size_t)pl.pitch;
            au[i] = onchip_wave_au(hd.k, img[c], img[c - 1], img[c + 1], img[c - p], img[c + p]);
        }
        for (size_t i = 0; i < U; ++i) {
            hist[(size_t)row * U + i] = au[i];
            const double acc = onchip_wave_medium_accel_of(c2[i], au[i], onchip_wave_forcing(wn, g[i]));
            if (second) v[i] = onchip_wave_kick(v[i], h, acc);
            if (first) v[i] = onchip_wave_kick(v[i], h, acc);
        }
    };
    pass(0, w[0], false, nsteps > 0);
    for (int s = 0; s < nsteps; ++s) {
        for (size_t i = 0; i < U; ++i) img[(size_t)cell[i]] = onchip_wave_drift(img[(size_t)cell[i]], tau, v[i]);
        pass(s + 1, w[(size_t)s + 1], true, s + 1 < nsteps);
        if ((s + 1) % every == 0) for (int r = 0; r < nrec; ++r) *sample++ = img[(size_t)cell[(size_t)rec[(size_t)r]]];
    }
    for (size_t i = 0; i < U; ++i) { res[i] = img[(size_t)cell[i]]; res[U + i] = v[i]; }
    return write_doubles(out, res);
}

int main(int argc, char** argv) {
    if (argc == 4 && std::strcmp(argv[3], "forward") == 0) return forward_file(argv[1], argv[2]);
    if (argc == 3) return backward_file(argv[1], argv[2]);
    const int nsys_set[] = {1, 40, kOnchipStepsMaxSys}, nsteps_set[] = {0, 7, kOnchipStepsMaxSteps}, nrec_set[] = {0, 5, kOnchipWaveMaxRec}, every_set[] = {1, 3};
    for (int n = 6; n <= kOnchipMaxN; n += 2) {
        const long long unknowns = (long long)(n / 2 - 1) * (3 * n / 2 - 1);
        std::printf("N=%d unknowns=%lld hist=", n, unknowns);
        bool first = true;
        for (int nsys : nsys_set)
            for (int nsteps : nsteps_set) {
                const long long got = onchip_wave_history_bytes(n, nsys, nsteps), want = 8LL * nsys * ((long long)nsteps + 1) * unknowns;
                CHECK(got == want, "N=%d nsys=%d nsteps=%d: %lld history bytes, not %lld", n, nsys, nsteps, got, want);
                std::printf("%s%d:%d:%lld", first ? "" : ",", nsys, nsteps, got);
                first = false;
            }
        std::printf(" ws=");
        first = true;
        for (int nsys : nsys_set)
            for (int nsteps : nsteps_set)
                for (int nrec : nrec_set)
                    for (int every : every_set) {
                        const long long got = onchip_wave_adjoint_workspace_bytes(n, nsys, nsteps, nrec, every);
                        const long long want = (long long)nsys * (3LL * 8 * unknowns + 456) + 8 + 16LL * nsys + 8 * unknowns + 4 * 64 + 16LL * nsys;
                        CHECK(got == want, "N=%d nsys=%d nsteps=%d nrec=%d every=%d: %lld workspace bytes, not %lld", n, nsys, nsteps, nrec, every, got, want);
                        CHECK(got == onchip_wave_medium_workspace_bytes(n, nsys, nsteps, nrec, every), "N=%d nsys=%d: not the medium call's workspace", n, nsys);
                        std::printf("%s%d:%d:%d:%d:%lld", first ? "" : ",", nsys, nsteps, nrec, every, got);
                        first = false;
                    }
        std::printf("\n");
    }
    for (int n : {0, 4, 7, kOnchipMaxN + 1, kOnchipMaxN + 2}) {
        CHECK(onchip_wave_history_bytes(n, 3, 2) == 0, "N=%d has history bytes", n);
        CHECK(onchip_wave_adjoint_workspace_bytes(n, 3, 2, 1, 1) == 0, "N=%d has workspace bytes", n);
    }
    CHECK(onchip_wave_history_bytes(10, 0, 1) == 0 && onchip_wave_history_bytes(10, kOnchipStepsMaxSys + 1, 1) == 0, "a member count outside the limits has a history");
    CHECK(onchip_wave_history_bytes(10, 1, -1) == 0 && onchip_wave_history_bytes(10, 1, kOnchipStepsMaxSteps + 1) == 0, "a step count outside the limits has a history");
    CHECK(onchip_wave_adjoint_workspace_bytes(10, 0, 1, 1, 1) == 0 && onchip_wave_adjoint_workspace_bytes(10, kOnchipStepsMaxSys + 1, 1, 1, 1) == 0, "a member count outside the limits was not refused");
    CHECK(onchip_wave_adjoint_workspace_bytes(10, 1, -1, 1, 1) == 0 && onchip_wave_adjoint_workspace_bytes(10, 1, kOnchipStepsMaxSteps + 1, 1, 1) == 0, "a step count outside the limits was not refused");
    CHECK(onchip_wave_adjoint_workspace_bytes(10, 1, 1, -1, 1) == 0 && onchip_wave_adjoint_workspace_bytes(10, 1, 1, kOnchipWaveMaxRec + 1, 1) == 0, "a receiver count outside the limits was not refused");
    CHECK(onchip_wave_adjoint_workspace_bytes(10, 1, 1, 1, 0) == 0, "a cadence below 1 was not refused");
    // the acceleration in its two halves: the bits of onchip_wave_medium_accel
    const OnchipWaveCoef k{-1234.5678, 300.1, 317.1839};
    for (double x : {0.0, 1.0, -3.5e-3, 7.25e3, 0.1})
        for (double c : {1.0, 0.25, 3.7}) {
            const double a = onchip_wave_medium_accel(k, c, 0.3 * x, x, 0.7 * x, -x, 1.1 * x, 0.4);
            const double b = onchip_wave_medium_accel_of(c, onchip_wave_au(k, x, 0.7 * x, -x, 1.1 * x, 0.4), 0.3 * x);
            CHECK(std::memcmp(&a, &b, sizeof a) == 0, "the two halves change the acceleration at %a, c2 = %a", x, c);
        }
    std::printf("cap %d\n", kOnchipMaxN);
    std::printf("ok %d\n", failures);
    return failures ? 1 : 0;
}
