// onchip_compat_driver.cpp -- the on-chip solve mode reached from the reference's top-level class (tests/test_gpu_onchip.py).
// A DirichletSolver at the reference's default n = m = 10 on its default domain is solved twice, as it comes and after
// setSolveMode(MI355CG_SOLVE_ONCHIP); one JSON object with both runs and the on-chip launch counts.
// Build: g++ -std=c++17 -I iterative_solvers_amd/compat onchip_compat_driver.cpp -L... -lmi355cg
#include "dirichlet_solver.hpp"

#include <cstdio>

static void run(const char* tag, int mode, bool last) {
    DirichletSolver ds;                                             // n = m = 10, [0, 1] x [0, 1]
    ds.setVerbose(false);
    if (mode != MI355CG_SOLVE_LAUNCHES) ds.setSolveMode(mode);
    const SolverResults r = ds.solve();
    int got_mode = -1;
    long long launches = -1;
    mi355cg_compat::check(mi355cg_get_solve_mode(ds.getGridSystem()->context()->h, &got_mode, &launches));
    std::printf("\"%s\": {\"mode\": %d, \"launches\": %lld, \"iterations\": %d, \"converged\": %d, \"residual_norm\": %.17g, \"error_norm\": %.17g, \"solution\": [",
                tag, got_mode, launches, r.iterations, r.converged ? 1 : 0, r.residual_norm, r.error_norm);
    for (size_t i = 0; i < r.solution.size(); ++i) std::printf("%s%.17g", i ? ", " : "", r.solution[i]);
    std::printf("]}%s\n", last ? "" : ",");
}

int main() {
    Kokkos::initialize();
    std::printf("{\n");
    run("launches", MI355CG_SOLVE_LAUNCHES, false);
    run("onchip", MI355CG_SOLVE_ONCHIP, true);
    std::printf("}\n");
    Kokkos::finalize();
    return 0;
}
