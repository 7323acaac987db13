// The block eigensolver through the C++ drop-in (tests/test_gpu_eigs.py): MatrixFreeSystem::eigs on the 34 x 34 grid -- residuals
// recomputed with apply(), orthonormality, a second call bit for bit, a converged start block -- and its refusals.  Prints one
// line of results; exit code 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "mi355cg_compat.hpp"

int main() {
    MatrixFreeSystem s(34, 34, 1.0, 2.0, 1.0, 2.0);
    bool no_precond = false;
    try { s.eigs(3); } catch (const std::runtime_error&) { no_precond = true; }
    s.setPreconditioner(MI355CG_PRECOND_MG_ANY);

    const MatrixFreeSystem::EigsResult r = s.eigs(6, 8);
    bool ok = r.info.converged == 1 && r.info.stop_reason == MI355CG_EIG_CONVERGED && r.lambda.size() == 6 && r.vectors.size() == 6 &&
              r.residuals.size() == 8 && r.ritz_values.size() == 8 && r.info.iterations >= 1 && r.info.iterations <= 40;
    double worst_res = 0.0, worst_orth = 0.0;
    for (size_t j = 0; ok && j < 6; ++j) {
        const std::vector<double>& v = r.vectors[j];
        const std::vector<double> av = s * v;
        double rr = 0.0, vv = 0.0;
        for (size_t i = 0; i < v.size(); ++i) { const double d = av[i] + r.lambda[j] * v[i]; rr += d * d; vv += v[i] * v[i]; }
        worst_res = std::fmax(worst_res, std::sqrt(rr) / (r.lambda[j] * std::sqrt(vv)));
        ok = r.lambda[j] > 0.0 && (j == 0 || r.lambda[j] >= r.lambda[j - 1]);
        for (size_t k = 0; k <= j; ++k) {
            double d = 0.0;
            for (size_t i = 0; i < v.size(); ++i) d += v[i] * r.vectors[k][i];
            worst_orth = std::fmax(worst_orth, std::fabs(d - (k == j ? 1.0 : 0.0)));
        }
    }
    ok = ok && worst_res <= 2e-8 && worst_orth <= 1e-12;

    const MatrixFreeSystem::EigsResult again = s.eigs(6, 8);
    const bool same = again.lambda == r.lambda && again.vectors == r.vectors && again.info.iterations == r.info.iterations;
    const MatrixFreeSystem::EigsResult from = s.eigs(6, 6, 1e-7, 200, &r.vectors);        // a converged start block
    const bool locked = from.info.iterations == 0 && from.info.converged == 1;

    bool refused_block = false, refused_nev = false, refused_shape = false, refused_tol = false;
    try { s.eigs(2, 17); } catch (const std::invalid_argument&) { refused_block = true; }
    try { s.eigs(5, 4); } catch (const std::invalid_argument&) { refused_nev = true; }
    try { s.eigs(6, 8, 1e-8, 200, &r.vectors); } catch (const std::invalid_argument&) { refused_shape = true; }
    try { s.eigs(2, 4, 0.0); } catch (const std::invalid_argument&) { refused_tol = true; }
    s.eigsRelease();
    s.eigsRelease();

    std::printf("ok=%d iterations=%d lambda1=%.12g worst_res=%.3g worst_orth=%.3g same=%d locked=%d no_precond=%d refused=%d%d%d%d\n", (int)ok,
                r.info.iterations, r.lambda.empty() ? 0.0 : r.lambda[0], worst_res, worst_orth, (int)same, (int)locked, (int)no_precond,
                (int)refused_block, (int)refused_nev, (int)refused_shape, (int)refused_tol);
    return (ok && same && locked && no_precond && refused_block && refused_nev && refused_shape && refused_tol) ? 0 : 1;
}
