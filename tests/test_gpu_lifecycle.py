"""What a handle keeps in device and pinned memory, replaced and released over and over (csrc/device_buffer.h): the hierarchy in both
precisions, batch and eigensolver workspaces that grow, line tables, the shifted coarse inverse, the warm start's and the stepper's
buffers.  N = 130 with MI355CG_PRECOND_MG_ANY has three levels (130, 64, 32) and its first transfer is non-nested, so every kind of
level vector exists.  No free-memory figure is read: on a shared machine it belongs to everybody."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DOM, CYCLES = 130, (1.0, 2.0, 1.0, 2.0), 6


def _params(isa):
    p = isa.default_params(isa.RULE_REL_2NORM)
    p.eps_rel, p.max_iterations, p.use_true_solution = 1e-8, 10 ** 5, 0
    return p


def test_handle_lifecycle_walks_every_replacement_path():
    import iterative_solvers_amd as isa
    p = _params(isa)
    fresh = isa.MatrixFreeSystem(N, N, *DOM)
    fresh.set_preconditioner(isa.PRECOND_MG_ANY)
    assert fresh.preconditioner_info() == (isa.PRECOND_MG_ANY, isa.CYCLE_F64, 3)
    r = fresh._handle.solve(p)
    assert r.converged
    ref_it, ref_x, b = r.iterations, fresh._handle.solution(), fresh.get_rhs()
    fresh._handle.close()
    rng = np.random.default_rng(20261019)
    batch = np.vstack([b[None, :], rng.standard_normal((4, b.size))])        # system 0 is the handle's own right-hand side
    blocks = {m: rng.standard_normal((m, b.size)) for m in (2, 4)}

    def same_as_fresh(res, x):
        return bool(res.converged) and res.iterations == ref_it and np.array_equal(x, ref_x)

    for cycle in range(CYCLES):
        s = isa.MatrixFreeSystem(N, N, *DOM)
        h = s._handle
        s.set_preconditioner(isa.PRECOND_MG_ANY)                             # 1. the fp64 hierarchy
        assert same_as_fresh(h.solve(p), h.solution())
        for nrhs in (2, 5):                                                  # 2. a batch workspace, then a larger one
            x, res = h.solve_batch(p, batch[:nrhs])
            assert same_as_fresh(res[0], x[0]) and all(q.converged for q in res)
        h.batch_release()
        for m in (2, 4):                                                     # 3. an eigensolver workspace, then a larger one
            lam, _, _, out = h.eigs(1, m, 1e-2, 3, blocks[m])
            assert out.iterations <= 3 and np.all(np.isfinite(lam)) and lam[0] > 0
        s.set_smoother(isa.SMOOTHER_LINE_X)                                  # 4. line tables built and dropped
        assert s.smoother_info() == (isa.SMOOTHER_LINE_X, 1)
        s.set_smoother(isa.SMOOTHER_JACOBI)
        s.set_shift(0.5)                                                     # 5. the coarse inverse rebuilt and swapped, twice
        s.set_shift(0.0)
        s.set_preconditioner(isa.PRECOND_MG_ANY, isa.CYCLE_F32)              # 6. the other precision replaces the hierarchy (and the eigen workspace goes)
        assert s.preconditioner_info() == (isa.PRECOND_MG_ANY, isa.CYCLE_F32, 3)
        assert h.solve(p).converged
        s.set_preconditioner(isa.PRECOND_MG_ANY, isa.CYCLE_F64)
        h.set_initial_guess(0.5 * ref_x)                                     # 7. a warm start (on the hierarchy: the scratch vectors)
        assert h.solve(p).converged
        h.set_initial_guess(ref_x)                                           # 8. one implicit step: step_b in the place of b, a shift
        res, done = h.time_steps(p, 1e-2, 1.0, 1)
        assert done == 1 and res[0].converged
        s.set_shift(0.0)
        assert np.array_equal(s.get_rhs(), b)
        assert same_as_fresh(h.solve(p), h.solution())                       # 9. after all of it: the fresh handle's bits
        s.set_preconditioner(isa.PRECOND_NONE)
        assert s.preconditioner_info() == (isa.PRECOND_NONE, isa.CYCLE_F64, 0)
        h.set_initial_guess(0.5 * ref_x)                                     # the plain path's warm start: its own partials and pinned norms
        plain = h.solve(p)
        assert plain.converged and plain.iterations > 0 and np.all(np.isfinite(h.solution()))
        h.close()
