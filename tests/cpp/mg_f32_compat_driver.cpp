// MI355CG_CYCLE_F32 through the C++ drop-in (tests/test_gpu_mg_f32.py): the fp32 V-cycle set through
// MatrixFreeSystem::setPreconditioner and through DirichletSolver::setPreconditioner (kept across setGridParameters), the same
// iteration count as the fp64 cycle, and the refusal of an unknown precision.  Prints one line of results; exit code 0 when
// every check holds.
#include <cstdio>
#include <stdexcept>

#include "mi355cg_compat.hpp"

int main() {
    MatrixFreeSystem s(258, 258, 1.0, 2.0, 1.0, 2.0);
    s.setPreconditioner(MI355CG_PRECOND_MG_ANY, MI355CG_CYCLE_F32);
    int kind = -1, cycle = -1, levels = -1;
    const int info_rc = mi355cg_preconditioner_info(s.context()->h, &kind, &cycle, &levels);
    MatrixFreeSolver mf(s, s.get_rhs(), 1e-8, 1000);
    mf.solve(s.get_true_solution_vector());
    const int its32 = mf.getIterations();
    s.setPreconditioner(MI355CG_PRECOND_MG_ANY);                      // the default is the fp64 cycle
    int cycle64 = -1;
    mi355cg_preconditioner_info(s.context()->h, nullptr, &cycle64, nullptr);
    MatrixFreeSolver mf64(s, s.get_rhs(), 1e-8, 1000);
    mf64.solve(s.get_true_solution_vector());
    const int its64 = mf64.getIterations();

    DirichletSolver d(100, 100, 1.0, 2.0, 1.0, 2.0);
    d.setVerbose(false);
    d.setPreconditioner(MI355CG_PRECOND_MG_ANY, MI355CG_CYCLE_F32);
    d.setGridParameters(1000, 1000, 1.0, 2.0, 1.0, 2.0);            // kind and precision are kept across a new grid
    const SolverResults r = d.solve();

    bool refused = false;
    try {
        MatrixFreeSystem bad(100, 100, 1.0, 2.0, 1.0, 2.0);
        bad.setPreconditioner(MI355CG_PRECOND_MG_ANY, 5);
    } catch (const std::invalid_argument&) {
        refused = true;
    }
    std::printf("info_rc=%d kind=%d cycle=%d levels=%d cycle64=%d iterations_f32=%d iterations_f64=%d dirichlet_iterations=%d "
                "dirichlet_converged=%d refused=%d\n", info_rc, kind, cycle, levels, cycle64, its32, its64, r.iterations,
                (int)r.converged, (int)refused);
    return (info_rc == 0 && kind == MI355CG_PRECOND_MG_ANY && cycle == MI355CG_CYCLE_F32 && levels == 4 && cycle64 == MI355CG_CYCLE_F64 &&
            its32 >= 1 && its32 <= 12 && its32 == its64 && r.converged && r.iterations >= 1 && r.iterations <= 20 && refused) ? 0 : 1;
}
