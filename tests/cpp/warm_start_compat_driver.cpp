// Warm starts through the C++ drop-in (tests/test_gpu_warm_start.py): MatrixFreeSolver solved cold, capped and continued
// (continueFromSolution), warm-started from a coarse solution (setInitialGuess), and MSGSolver started from a converged solution.
// argv: N cap, then what the Python layer got for the same sequence: the iteration counts of the cold, continued and warm solves,
// the MSG solve's iteration count and stop reason, and the sums (sequential, in index order; hex floats) of the continued, warm
// and MSG solutions.  DirichletSolver's pair is checked on its own (continuation and guess of a converged solve: 0 iterations).  Prints one line of results; exit code 0 when every number matches.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mi355cg_compat.hpp"

static double checksum(const double* x, size_t n) {
    double t = 0.0;
    for (size_t i = 0; i < n; ++i) t += x[i];
    return t;
}

int main(int argc, char** argv) {
    if (argc != 11) { std::fprintf(stderr, "usage: %s N cap cold cont warm msg_its msg_reason sum_cont sum_warm sum_msg\n", argv[0]); return 2; }
    const int N = std::atoi(argv[1]), cap = std::atoi(argv[2]);
    const int want_cold = std::atoi(argv[3]), want_cont = std::atoi(argv[4]), want_warm = std::atoi(argv[5]);
    const int want_msg = std::atoi(argv[6]), want_reason = std::atoi(argv[7]);
    const double want_sum_cont = std::strtod(argv[8], nullptr), want_sum_warm = std::strtod(argv[9], nullptr),
                 want_sum_msg = std::strtod(argv[10], nullptr);
    const std::vector<double> none;

    MatrixFreeSystem s(N, N, 1.0, 2.0, 1.0, 2.0);
    MatrixFreeSolver cold(s, s.get_rhs(), 1e-8, 100000);
    const std::vector<double> x_cold = cold.solve(none);

    MatrixFreeSolver capped(s, s.get_rhs(), 1e-8, cap);
    capped.solve(none);
    MatrixFreeSolver cont(s, s.get_rhs(), 1e-8, 100000);
    cont.continueFromSolution();
    const std::vector<double> x_cont = cont.solve(none);

    MatrixFreeSolver coarse(s, s.get_rhs(), 1e-4, 100000);
    const std::vector<double> x4 = coarse.solve(none);
    MatrixFreeSolver warm(s, s.get_rhs(), 1e-8, 100000);
    warm.setInitialGuess(x4);
    const std::vector<double> x_warm = warm.solve(none);
    const int warm_its = warm.getIterations();
    const std::vector<double> x_again = warm.solve(none);                 // the guess was consumed: cold again
    const bool one_shot = warm.getIterations() == cold.getIterations() && x_again == x_cold;

    GridSystem g(N, N, 1.0, 2.0, 1.0, 2.0);
    MSGSolver msg(g.get_matrix(), g.get_rhs(), 1e-6, 100000);
    msg.setVerbose(false);
    msg.setPrecisionEps(-1.0);
    msg.setExactErrorEps(-1.0);
    KokkosVector guess("x0", x_cold.size());
    for (size_t i = 0; i < x_cold.size(); ++i) guess(i) = x_cold[i];
    msg.setInitialGuess(guess);
    const KokkosVector x_msg = msg.solve(KokkosVector());

    bool refused = false;
    try {
        msg.setInitialGuess(KokkosVector("short", 3));
    } catch (const std::invalid_argument&) {
        refused = true;
    }
    // DirichletSolver forwards both to the MSGSolver of its next solve(): a continuation of a converged solve stops at once,
    // a guess of the wrong size is refused by the setter, and both are one-shot
    DirichletSolver d(N, N, 1.0, 2.0, 1.0, 2.0);
    d.setVerbose(false);
    d.enablePrecisionStopping(false);                                             // the residual test alone: it also runs on a start
    d.setSolverParameters(1e-7, 1e-7, 1e-7, 100000);
    const SolverResults r1 = d.solve();
    d.setSolverParameters(1e-6, 1e-6, 1e-6, 100000);
    d.continueFromSolution();
    const SolverResults r2 = d.solve();
    KokkosVector dg("x0", r1.solution.size());
    for (size_t i = 0; i < r1.solution.size(); ++i) dg(i) = r1.solution[i];
    d.setInitialGuess(dg);
    const SolverResults r3 = d.solve();
    const SolverResults r4 = d.solve();                                           // cold again
    bool d_refused = false;
    try {
        d.setInitialGuess(KokkosVector("short", 3));
    } catch (const std::invalid_argument&) {
        d_refused = true;
    }
    const bool dirichlet = r1.converged && r1.iterations > 1 && r2.converged && r2.iterations == 0 && r2.solution == r1.solution &&
                           r3.converged && r3.iterations == 0 && r3.solution == r1.solution && r4.converged && r4.iterations > 1 &&
                           d_refused;
    const double sum_cont = checksum(x_cont.data(), x_cont.size()), sum_warm = checksum(x_warm.data(), x_warm.size()),
                 sum_msg = checksum(x_msg.data(), x_msg.extent(0));
    std::printf("cold=%d capped=%d cont=%d warm=%d msg=%d reason=%d sum_cont=%a sum_warm=%a sum_msg=%a one_shot=%d refused=%d dirichlet=%d (%d %d %d %d)\n",
                cold.getIterations(), capped.getIterations(), cont.getIterations(), warm_its, msg.getIterations(),
                (int)msg.getStopReason(), sum_cont, sum_warm, sum_msg, (int)one_shot, (int)refused, (int)dirichlet, r1.iterations, r2.iterations,
                r3.iterations, r4.iterations);
    const bool ok = cold.getIterations() == want_cold && capped.getIterations() == cap && cont.getIterations() == want_cont &&
                    warm_its == want_warm && msg.getIterations() == want_msg && (int)msg.getStopReason() == want_reason &&
                    sum_cont == want_sum_cont && sum_warm == want_sum_warm && sum_msg == want_sum_msg && one_shot && refused && dirichlet;
    return ok ? 0 : 1;
}
