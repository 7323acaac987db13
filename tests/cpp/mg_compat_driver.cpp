// The multigrid extension of the C++ drop-in (tests/test_gpu_mg.py): MatrixFreeSystem::setPreconditioner and
// DirichletSolver::setPreconditioner.  Prints one line of results; exit code 0 when every check holds.
#include <cstdio>
#include <stdexcept>

#include "mi355cg_compat.hpp"

int main() {
    MatrixFreeSystem s(256, 256, 1.0, 2.0, 1.0, 2.0);
    s.setPreconditioner(MI355CG_PRECOND_MG);
    MatrixFreeSolver mf(s, s.get_rhs(), 1e-8, 1000);
    mf.solve(s.get_true_solution_vector());
    const int mf_its = mf.getIterations();

    DirichletSolver d(256, 256, 1.0, 2.0, 1.0, 2.0);
    d.setVerbose(false);
    d.setPreconditioner(MI355CG_PRECOND_MG);
    d.setGridParameters(128, 128, 1.0, 2.0, 1.0, 2.0);              // kept across a new grid
    const SolverResults r = d.solve();

    bool refused = false;
    try {
        MatrixFreeSystem bad(258, 258, 1.0, 2.0, 1.0, 2.0);
        bad.setPreconditioner(MI355CG_PRECOND_MG);
    } catch (const std::invalid_argument&) {
        refused = true;
    }
    std::printf("mf_iterations=%d dirichlet_iterations=%d dirichlet_converged=%d refused=%d\n", mf_its, r.iterations, (int)r.converged, (int)refused);
    return (mf_its >= 1 && mf_its <= 12 && r.converged && r.iterations >= 1 && r.iterations <= 20 && refused) ? 0 : 1;
}
