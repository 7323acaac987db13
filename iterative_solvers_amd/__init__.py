"""iterative_solvers_amd -- MI355X-native matrix-free CG for the 2-D Dirichlet Poisson problem
on the reference's L-shaped grid.  HIP kernels + C ABI in csrc/ (libmi355cg.so); this package
is the host-side mirror of the reference's operator / solver interface."""
from ._capi import (BATCH_MAX, MANY_MAX, STEPS_MANY_MAX_STEPS, WAVE_MAX_RECEIVERS, EIG_BLOCK_MAX, EIG_BREAKDOWN, EIG_CONVERGED, EIG_INTERRUPTED, EIG_ITERATIONS, CYCLE_F32, CYCLE_F64, F64, F32_MIXED, PRECOND_MG, PRECOND_MG_ANY, PRECOND_NONE, RULE_MSG_MAXNORM, RULE_REL_2NORM,
                    SMOOTHER_JACOBI, SMOOTHER_LINE_AUTO, SMOOTHER_LINE_X, SMOOTHER_LINE_Y, SOLVE_LAUNCHES, SOLVE_ONCHIP, WAVE_NEWMARK, WAVE_VERLET, Mi355cgError, lib_path, load)
from .solver import (CrsMatrix, DirichletSolver, GridSystem, MatrixFreeSolver, MatrixFreeSystem, MSGSolver,
                     SolverResults, StopCriterion, default_params, mg_hierarchy, mg_levels, onchip_plan, rayleigh_ritz, sponge_damping, time_steps_many_workspace, wave_medium_many_workspace, wave_record_many_workspace, wave_sponge_many_workspace,
                     wave_steps_many_workspace, wave_adjoint_many_workspace, wave_history_bytes)

__all__ = ["CrsMatrix", "DirichletSolver", "GridSystem", "MatrixFreeSolver", "MatrixFreeSystem", "MSGSolver",
           "SolverResults", "StopCriterion", "default_params", "Mi355cgError", "lib_path", "load",
           "F64", "F32_MIXED", "RULE_MSG_MAXNORM", "RULE_REL_2NORM", "PRECOND_NONE", "PRECOND_MG", "PRECOND_MG_ANY", "CYCLE_F64", "CYCLE_F32", "BATCH_MAX", "MANY_MAX",
           "mg_levels", "mg_hierarchy", "rayleigh_ritz", "EIG_BLOCK_MAX", "EIG_CONVERGED", "EIG_ITERATIONS", "EIG_INTERRUPTED", "EIG_BREAKDOWN",
           "SMOOTHER_JACOBI", "SMOOTHER_LINE_X", "SMOOTHER_LINE_Y", "SMOOTHER_LINE_AUTO",
           "SOLVE_LAUNCHES", "SOLVE_ONCHIP", "onchip_plan", "time_steps_many_workspace", "STEPS_MANY_MAX_STEPS",
           "WAVE_VERLET", "WAVE_NEWMARK", "wave_steps_many_workspace", "wave_record_many_workspace", "WAVE_MAX_RECEIVERS", "wave_medium_many_workspace",
           "wave_sponge_many_workspace", "sponge_damping", "wave_history_bytes", "wave_adjoint_many_workspace"]
