// MI355CG_PRECOND_MG_ANY through the C++ drop-in (tests/test_gpu_mg_any.py): MatrixFreeSystem::setPreconditioner on a grid
// PRECOND_MG refuses, and DirichletSolver keeping the kind across setGridParameters.  Prints one line of results; exit code 0
// when every check holds.
#include <cstdio>
#include <stdexcept>

#include "mi355cg_compat.hpp"

int main() {
    MatrixFreeSystem s(100, 100, 1.0, 2.0, 1.0, 2.0);
    s.setPreconditioner(MI355CG_PRECOND_MG_ANY);
    MatrixFreeSolver mf(s, s.get_rhs(), 1e-8, 1000);
    mf.solve(s.get_true_solution_vector());
    const int mf_its = mf.getIterations();                           // <= 12 of at most 1000: converged

    DirichletSolver d(100, 100, 1.0, 2.0, 1.0, 2.0);
    d.setVerbose(false);
    d.setPreconditioner(MI355CG_PRECOND_MG_ANY);
    d.setGridParameters(1000, 1000, 1.0, 2.0, 1.0, 2.0);            // kept across a new grid
    const SolverResults r = d.solve();

    bool refused = false;
    try {
        MatrixFreeSystem bad(100, 100, 1.0, 2.0, 1.0, 2.0);
        bad.setPreconditioner(MI355CG_PRECOND_MG);
    } catch (const std::invalid_argument&) {
        refused = true;
    }
    std::printf("mf_iterations=%d dirichlet_iterations=%d dirichlet_converged=%d refused=%d\n", mf_its, r.iterations,
                (int)r.converged, (int)refused);
    return (mf_its >= 1 && mf_its <= 12 && r.converged && r.iterations >= 1 && r.iterations <= 20 && refused) ? 0 : 1;
}
