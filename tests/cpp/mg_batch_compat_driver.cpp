// Batched multigrid-PCG solves through the C++ drop-in (tests/test_gpu_mg_batch.py): MatrixFreeSystem::solveBatch against one
// MatrixFreeSolver solve per right-hand side on the same system, bit for bit, and its refusals.  Prints one line of results;
// exit code 0 when every check holds.
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "mi355cg_compat.hpp"

int main() {
    MatrixFreeSystem s(130, 130, 1.0, 2.0, 1.0, 2.0);
    mi355cg_params prm;
    mi355cg_default_params(&prm, MI355CG_RULE_REL_2NORM);
    prm.eps_rel = 1e-8;
    prm.max_iterations = 1000;
    prm.use_true_solution = 0;

    std::vector<std::vector<double>> b(3, s.get_rhs());
    for (size_t i = 0; i < b[1].size(); ++i) b[1][i] = 1.0;
    for (size_t i = 0; i < b[2].size(); ++i) b[2][i] = 0.0;

    bool no_precond = false;
    try { s.solveBatch(b, prm); } catch (const std::runtime_error&) { no_precond = true; }

    s.setPreconditioner(MI355CG_PRECOND_MG_ANY);
    std::vector<mi355cg_results> res;
    const std::vector<std::vector<double>> x = s.solveBatch(b, prm, &res);

    bool same = res.size() == b.size() && x.size() == b.size();
    for (size_t k = 0; same && k < b.size(); ++k) {
        MatrixFreeSolver one(s, b[k], 1e-8, 1000);
        const std::vector<double> xs = one.solve(std::vector<double>());
        same = xs == x[k] && one.getIterations() == res[k].iterations;
    }
    const bool counts = same && res[0].iterations >= 1 && res[0].iterations <= 12 && res[2].iterations == 0 && res[0].converged;

    bool refused_size = false, refused_empty = false, refused_u = false;
    try { std::vector<std::vector<double>> bad(2, std::vector<double>(5, 1.0)); s.solveBatch(bad, prm); } catch (const std::invalid_argument&) { refused_size = true; }
    try { s.solveBatch({}, prm); } catch (const std::invalid_argument&) { refused_empty = true; }
    try { mi355cg_params p2 = prm; p2.use_true_solution = 1; s.solveBatch(b, p2); } catch (const std::invalid_argument&) { refused_u = true; }
    s.batchRelease();
    s.batchRelease();

    std::printf("same=%d iterations=%d,%d,%d no_precond=%d refused_size=%d refused_empty=%d refused_u=%d\n", (int)same,
                res.empty() ? -1 : res[0].iterations, res.size() < 2 ? -1 : res[1].iterations, res.size() < 3 ? -1 : res[2].iterations,
                (int)no_precond, (int)refused_size, (int)refused_empty, (int)refused_u);
    return (same && counts && no_precond && refused_size && refused_empty && refused_u) ? 0 : 1;
}
