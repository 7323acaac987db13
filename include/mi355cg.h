/*
 * mi355cg.h -- C ABI of libmi355cg.so: the MI355X (gfx950) matrix-free conjugate-gradient
 * path for the 2-D Dirichlet Poisson problem on the reference's L-shaped grid.
 *
 * This is the drop-in boundary underneath the reference's C++ plug-in interfaces.  Each entry
 * point names the reference interface it replaces (paths relative to the reference checkout):
 *
 *   mi355cg_create / _destroy      GridSystem::GridSystem(m,n,a,b,c,d)      solver/grid_system.cpp:301-322
 *                                  MatrixFreeSystem::MatrixFreeSystem       solver/matrix_free_system.cpp:144-159
 *   mi355cg_size                   MatrixFreeSystem::size / matrix.numRows  solver/matrix_free_system.hpp:66
 *   mi355cg_get_rhs                GridSystem::get_rhs / MatrixFreeSystem::get_rhs   grid_system.h:73, matrix_free_system.hpp:49
 *   mi355cg_get_true_solution      get_true_solution_vector                 grid_system.cpp:276-299, matrix_free_system.cpp:162-199
 *   mi355cg_get_node_coords        GridSystem::get_x_coords/get_y_coords    grid_system.cpp:189-190,235-236
 *   mi355cg_set_rhs                Solver(a, b, ...) caller-supplied b      solver/solver.hpp:33-39
 *   mi355cg_apply                  MatrixFreeSystem::apply(x, y)            solver/matrix_free_system.cpp:203-340
 *                                  KokkosSparse::spmv("N",1,A,z,0,A_z)      solver/msg_solver.cpp:93
 *   mi355cg_solve                  MSGSolver::solve(true_solution)          solver/msg_solver.cpp:10-212   (rule MSG_MAXNORM)
 *                                  MatrixFreeSolver::solve(true_solution)   solver/matrix_free_system.cpp:383-482 (rule REL_2NORM)
 *   mi355cg_get_solution/_residual DirichletSolver::getSolution, computeResidual (A x - b)   solver/dirichlet_solver.cpp:147-161,183-191
 *   mi355cg_iter_cb                Solver::setIterationCallback             solver/solver.hpp:46-50
 *   stop_flag                      MSGSolver::requestStop (atomic flag)     solver/msg_solver.hpp:35,76; msg_solver.cpp:82-87
 *
 * Extension without a reference counterpart (the reference has no preconditioner):
 *   mi355cg_set_preconditioner     opt-in geometric multigrid V-cycle M ~ A^-1 for single-GPU fp64 grid handles; while it is
 *                                  set, mi355cg_solve runs preconditioned CG (same stop rules, callbacks, stop flag, results)
 *   mi355cg_set_preconditioner_ex  the same with the precision of the V-cycle: MI355CG_CYCLE_F64 or MI355CG_CYCLE_F32
 *   mi355cg_preconditioner_info    kind, cycle precision and number of levels of what is set
 *   mi355cg_set_smoother / _get_smoother   the smoother of the fp64 V-cycle: damped point Jacobi, or line Jacobi for stretched domains
 *   mi355cg_apply_preconditioner   z = M r on host vectors (packed order)
 *   mi355cg_mg_levels            the hierarchy a grid gets (pure host arithmetic, no GPU needed)
 *   mi355cg_mg_hierarchy           every level's N of either multigrid kind (pure host arithmetic, no GPU needed)
 *   mi355cg_solve_batch            many right-hand sides on one grid by one preconditioned CG loop (host vectors)
 *   mi355cg_solve_batch_device     the same with the vectors in device memory
 *   mi355cg_batch_release          free the workspace the batched solves keep on the handle
 *   mi355cg_set_shift / _get_shift the operator becomes A - sigma I (implicit time steps, screened Poisson, shift-and-invert)
 *   mi355cg_time_steps             theta-scheme steps of u_t = A u - g with the state kept on the device
 *   mi355cg_get_solution_device    the x of the last solve into device memory
 *   mi355cg_eigs / _eigs_device    the lowest eigenpairs by a block iteration preconditioned with the V-cycle
 *   mi355cg_eigs_release           free the workspace the eigen solves keep on the handle
 *   mi355cg_block_gram / _combine  the block kernels of that iteration on host vectors
 *   mi355cg_rayleigh_ritz          its Rayleigh-Ritz step (pure host arithmetic, no GPU needed)
 *   mi355cg_set_solve_mode / _get_solve_mode   opt-in: chunks of a plain fp64 solve as one launch of one workgroup, grids up to N = 128
 *   mi355cg_onchip_plan            the layout of that mode for a grid (pure host arithmetic, no GPU needed)
 *   mi355cg_solve_many / _from / _device / _device_from   many small systems (own b, guess and shift each), one workgroup per system
 *   mi355cg_solve_many_info        LDS per workgroup, resident workgroups per CU and workspace bytes of such a batch
 *   mi355cg_time_steps_many / _device   an ensemble of small time steppers (own state, forcing and tau each), the step loop inside the launch
 *   mi355cg_time_steps_many_workspace   the device workspace bytes of such an ensemble (pure host arithmetic, no GPU needed)
 *   mi355cg_wave_steps_many / _device   an ensemble of small wave-equation steppers u_tt = A u - g: velocity Verlet or Newmark
 *   mi355cg_wave_steps_many_workspace / mi355cg_wave_cfl   its workspace bytes; the explicit scheme's bound on tau (host arithmetic)
 *   mi355cg_wave_record_many / _device / _workspace   the explicit scheme with a source time function and receiver traces
 *   mi355cg_wave_medium_many / _device / _workspace / mi355cg_wave_medium_cfl   that scheme in a medium: a squared wave speed per unknown and member
 *   mi355cg_wave_sponge_many / _device / _workspace   ... with a damping rate per unknown and member: absorbing (sponge) layers
 *   mi355cg_wave_history_many / _device / mi355cg_wave_history_bytes   the scheme in a medium, keeping the history au(u_n) of every step
 *   mi355cg_wave_adjoint_many / _device / _workspace   its exact transpose: adjoint steps and the sensitivity to c2
 *
 * Plain pointers and sizes only; no C++/torch types.  All host vectors are in the reference's
 * PACKED unknown order (bottom-right block row-major, then the upper block row-major;
 * grid_system.cpp:84-111) and are caller-owned.  Every function returns MI355CG_OK (0) or an
 * error code; mi355cg_last_error() gives the text (thread-local).  There is no CPU fallback:
 * without a usable HIP device every compute entry point fails with MI355CG_ERR_HIP.
 */
#ifndef MI355CG_H
#define MI355CG_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355CG_OK            0
#define MI355CG_ERR_INVALID   1   /* bad argument (std::invalid_argument in the C++ wrapper)    */
#define MI355CG_ERR_HIP       2   /* HIP runtime failure / no device (std::runtime_error)       */
#define MI355CG_ERR_STATE     3   /* call order (e.g. get_solution before solve)                */

/* storage / arithmetic type of the CG vectors */
#define MI355CG_F64           0   /* fp64 storage and arithmetic: the parity path               */
#define MI355CG_F32_MIXED     1   /* fp32 inner CG, fp64 residual refinement (no reference twin) */

/* stop rule */
#define MI355CG_RULE_MSG_MAXNORM  0   /* MSGSolver: absolute max-norm criteria, strict <        */
#define MI355CG_RULE_REL_2NORM    1   /* MatrixFreeSolver: ||r||_2 > eps * ||r0||_2             */

/* StopCriterion, solver/msg_solver.hpp:9-15 (same order) */
#define MI355CG_STOP_ITERATIONS   0
#define MI355CG_STOP_PRECISION    1
#define MI355CG_STOP_RESIDUAL     2
#define MI355CG_STOP_EXACT_ERROR  3
#define MI355CG_STOP_INTERRUPTED  4

typedef struct mi355cg_ctx *mi355cg_handle;

/* (iteration, ||x_n - x_{n-1}||, ||residual||, ||x - u||), invoked on the thread that called
 * mi355cg_solve.  MSG rule: max-norms, at it = 0, 1, every callback_every-th and the final one
 * (msg_solver.cpp:75-77,172-183,193-195).  REL_2NORM rule with diagnostics: 2-norms, the TRUE
 * residual b - A x, every iteration, 0-based index (matrix_free_system.cpp:466-468). */
typedef void (*mi355cg_iter_cb)(void *user, int iteration, double precision, double residual, double error);

typedef struct mi355cg_params {
    int    rule;               /* MI355CG_RULE_*                                                 */
    int    max_iterations;     /* Solver::maxIterations                                          */
    double eps_precision;      /* MSG: <= 0 disables (msg_solver.cpp:144)                        */
    double eps_residual;       /* MSG: <= 0 disables (:151)                                      */
    double eps_exact_error;    /* MSG: <= 0 disables (:158)                                      */
    double eps_rel;            /* REL_2NORM: eps of matrix_free_system.cpp:409                   */
    int    use_true_solution;  /* MSG: true_solution.extent(0) > 0 (:64,132,158)                 */
    int    callback_every;     /* MSG cadence (reference: 100); 0 = only it 0/1/final            */
    int    diagnostics;        /* REL_2NORM: reproduce the per-iteration diagnostics + callback  */
    int    sync_every;         /* iterations enqueued between host polls; 0 = automatic          */
    int    fixed_iterations;   /* bench mode: ignore every convergence test, run max_iterations  */
    double inner_eps;          /* F32_MIXED: relative tolerance of each fp32 inner solve (0 = 1e-4) */
} mi355cg_params;

typedef struct mi355cg_results {
    int    iterations;
    int    converged;
    int    stop_reason;           /* MI355CG_STOP_*                                              */
    double final_residual_norm;   /* MSG: max-norm of the recursive residual (msg_solver.cpp:188) */
    double final_precision;       /* MSG: max-norm of x_n - x_{n-1} (:189); DBL_MAX if none      */
    double final_error_norm;      /* MSG: max-norm of x - u (:190); DBL_MAX without u            */
    double r_norm2;               /* Euclidean norm of the recursive residual                    */
    double initial_r_norm2;       /* ||r0||_2                                                    */
    double solve_seconds;         /* wall time of the device loop (init .. last poll)            */
    double refine_true_rel;       /* F32_MIXED: final fp64 ||b-Ax||_2/||b||_2, else 0            */
    int    refine_outer;          /* F32_MIXED: outer refinement steps, else 0                   */
    double loop_seconds;          /* device time of the iterations alone (HIP events on the solve stream: after the
                                     initialisation pass .. after the last launch); 0 where not measured          */
} mi355cg_results;

/* ---- lifetime -------------------------------------------------------------------------------- */
/* Argument order follows DirichletSolver(n, m, a, b, c, d) (dirichlet_solver.cpp:11); only
 * n == m, even, >= 6 is accepted (the reference's index map is only consistent there).         */
int  mi355cg_create(int n, int m, double a, double b, double c, double d,
                    int dtype, int device, mi355cg_handle *out);
/* Generic operator: any caller-supplied CSR matrix (int32 row_map[nrows+1], entries, fp64 values), the contract of
 * Solver(const KokkosCrsMatrix& a, const KokkosVector& b, ...) (solver/solver.hpp:33-39).  Vectors of such a handle are
 * plain length-nrows arrays; set_rhs / set_true_solution / apply / solve / get_solution work as on a grid handle
 * (both stop rules; no per-iteration diagnostics).  A x = KokkosSparse::spmv("N",1,A,x,0,y) (solver/msg_solver.cpp:93),
 * summed per row in entry order. */
int  mi355cg_create_csr(long long nrows, const int *row_map, const int *entries, const double *values,
                        int device, mi355cg_handle *out);
int  mi355cg_set_true_solution(mi355cg_handle h, const double *u);   /* u of the error criterion / norm (MSG rule) */
void mi355cg_destroy(mi355cg_handle h);
const char *mi355cg_last_error(void);
const char *mi355cg_version(void);

/* ---- setup data (host, packed order, length mi355cg_size) ------------------------------------ */
long long mi355cg_size(mi355cg_handle h);
int  mi355cg_get_rhs(mi355cg_handle h, double *out);
int  mi355cg_get_true_solution(mi355cg_handle h, double *out);
int  mi355cg_get_node_coords(mi355cg_handle h, double *xs, double *ys);
int  mi355cg_set_rhs(mi355cg_handle h, const double *b);
/* Opt-in (replaces the host loops of GridSystem::calculate_value / get_true_solution_vector,
 * solver/grid_system.cpp:45-67,276-299): regenerate the right-hand side and the exact solution of the handle's cells on
 * the GPU.  Same expression order; exp() is the device library's (<= 1 ulp from glibc's), so the vectors may differ from
 * the reference's in the last bit, which is why mi355cg_create does NOT do this by default.                              */
int  mi355cg_setup_on_device(mi355cg_handle h);

/* ---- operator -------------------------------------------------------------------------------- */
int  mi355cg_apply(mi355cg_handle h, const double *x, double *y);            /* host buffers   */
int  mi355cg_apply_device(mi355cg_handle h, const double *x_dev, double *y_dev); /* packed, device */

/* ---- solver ---------------------------------------------------------------------------------- */
void mi355cg_default_params(mi355cg_params *p, int rule);
int  mi355cg_solve(mi355cg_handle h, const mi355cg_params *params,
                   mi355cg_iter_cb cb, void *user, const volatile int *stop_flag,
                   mi355cg_results *out);
int  mi355cg_get_solution(mi355cg_handle h, double *x);         /* packed x of the last solve   */
int  mi355cg_get_recursive_residual(mi355cg_handle h, double *r);
int  mi355cg_get_true_residual(mi355cg_handle h, double *ax_minus_b); /* A x - b, one more apply */

/* ---- preconditioner (extension: no reference twin) -------------------------------------------------------------------
 * MI355CG_PRECOND_MG: geometric multigrid.  Level 0 is the handle's grid; level l + 1 has N_l / 2 intervals (steps doubled)
 * and exists while N_l % 4 == 0 and N_l > 32; the coarsest level must have N_L <= 32, so 10, 16, 32 (one level: M = A^-1),
 * 64, 256, 4096 (8 levels) qualify and 258 or 1000 do not.  M = one V-cycle: two damped-Jacobi sweeps (omega 0.8), the
 * residual restricted by full weighting, the coarse correction (recursively; on the coarsest level a dense inverse of A_L
 * computed once on the host) prolonged bilinearly, two more sweeps.  M is symmetric and, like A, negative definite.
 * mi355cg_solve then runs Hestenes-Stiefel PCG from x = 0 (z = M r, p = z + beta p, beta = (r, z) / (r, z)_previous) with the
 * rule, callbacks, stop flag, fixed_iterations and result fields of the plain path; mi355cg_get_solution / _residual report it.
 * MG is refused (MI355CG_ERR_INVALID) on CSR handles, slab / part handles, MI355CG_F32_MIXED handles and grids without a
 * hierarchy.  Memory: level 0 adds five vectors of the handle's size, the coarser levels about one more, the inverse <= 4 MB.
 * set_preconditioner(MI355CG_PRECOND_NONE) frees it: the handle then runs exactly the plain path again.
 *
 * MI355CG_PRECOND_MG_ANY: the same preconditioner for every grid mi355cg_create accepts (even n >= 6).  Its ladder is
 * N_{l+1} = 2 floor(N_l / 4) while N_l > 32, so the coarsest level has 16 <= N_L <= 32 (or N_L = n when n <= 32): 1000 -> 500 ->
 * 250 -> 124 -> 62 -> 30, 258 -> 128 -> 64 -> 32.  A level with N_l % 4 == 0 is nested (N_{l+1} = N_l / 2) and is exactly a
 * PRECOND_MG level; where PRECOND_MG has a hierarchy the two kinds build the same one and give the same bits.  A non-nested
 * level (N_l % 4 == 2) keeps the domain, hx_{l+1} = hx_l N_l / N_{l+1} (same in y), and transfers by the bilinear weights
 * w(x, X) = max(0, 1 - |x N_c - X N_f| / N_f) between the two grids: P interpolates, R = (N_c / N_f)^2 P^T, so M is again
 * symmetric and negative definite.  Refusals as for MG; set_preconditioner(MG) on a grid only MG_ANY covers is refused and
 * leaves the handle as it was; switching kinds where both have a hierarchy keeps it.  Memory: since N_{l+1} <= N_l / 2, at
 * most what PRECOND_MG needs for a grid of the same size.
 * mi355cg_mg_hierarchy: *levels = the number of levels of kind's hierarchy for n, level_n[0 .. min(levels, max_levels) - 1]
 * = N_0 = n, N_1, ...; MI355CG_ERR_INVALID if the kind has none for n (PRECOND_MG: 258, 1000), n is odd or < 6, or the kind
 * is unknown.                                                                                                              */
#define MI355CG_PRECOND_NONE    0
#define MI355CG_PRECOND_MG      1
#define MI355CG_PRECOND_MG_ANY  2
int  mi355cg_set_preconditioner(mi355cg_handle h, int kind);                   /* builds or frees the hierarchy            */
int  mi355cg_apply_preconditioner(mi355cg_handle h, const double *r, double *z); /* host vectors, packed; MI355CG_ERR_STATE if none is set */
int  mi355cg_mg_levels(int n, int *levels, int *coarsest_n);                   /* PRECOND_MG; MI355CG_ERR_INVALID: no hierarchy */
int  mi355cg_mg_hierarchy(int kind, int n, int max_levels, int *levels, int *level_n);   /* no GPU needed               */

/* Precision of the V-cycle of either kind.  MI355CG_CYCLE_F32: z = M32 r runs the same cycle (hierarchy, V(2,2), omega, transfer
 * operators, expression order) with every vector, constant and operation in fp32, on r32 = fl32(r / s), s = 2^e the power of two
 * with 0.5 <= max|r| / s < 1, and returns z = s * (double) z32; max|r| = 0 gives z = 0.  The level constants, the non-nested
 * weights and the coarse inverse are the fp64 values rounded to fp32.  The PCG around it stays fp64: vectors, (r, z), (p, A p),
 * the norms and the stop tests, so the accuracy of the answer is that of the fp64 cycle and the iteration counts are the same
 * (DESIGN section 10.2); the scale makes M32(2^k r) = 2^k M32(r) bit for bit.  One-level grids (n <= 32), where the fp64 cycle
 * is the exact inverse and a solve takes one iteration, take a second one.  Memory: about that of the fp64 hierarchy.
 * mi355cg_set_preconditioner(h, kind) is mi355cg_set_preconditioner_ex(h, kind, MI355CG_CYCLE_F64).  _ex refuses what
 * set_preconditioner refuses, and an unknown cycle (MI355CG_ERR_INVALID); a refused call leaves the handle as it was.  Changing
 * only the precision rebuilds the levels' vectors; MI355CG_PRECOND_NONE frees everything whatever cycle says.
 * mi355cg_preconditioner_info: what is set (kind MI355CG_PRECOND_NONE, cycle MI355CG_CYCLE_F64, levels 0 without a
 * preconditioner); null out-pointers are skipped.                                                                          */
#define MI355CG_CYCLE_F64 0   /* the V-cycle in fp64: what mi355cg_set_preconditioner builds */
#define MI355CG_CYCLE_F32 1   /* the V-cycle in fp32 inside the fp64 PCG */
int  mi355cg_set_preconditioner_ex(mi355cg_handle h, int kind, int cycle);
int  mi355cg_preconditioner_info(mi355cg_handle h, int *kind, int *cycle, int *levels);

/* Smoother of the fp64 V-cycle.  The interface takes n == m, so every domain that is not a square has
 * hx != hy and an operator that is anisotropic by (hx / hy)^2; damped point Jacobi stops smoothing the weakly coupled direction
 * and the iteration count of the preconditioned CG grows with the stretch and with n.  A line smoother replaces the point sweep
 * by  t = u + omega T^-1 (r - A u), omega = 0.8,  T = the level's operator along the lines (its diagonal, shift included, and the
 * two neighbours in the line direction), solved exactly per line.  Lines are the maximal runs of interior nodes of the L-shape.
 * Schedule, transfer operators and coarse inverse are unchanged, T is symmetric, so M stays symmetric negative definite.
 * The default is MI355CG_SMOOTHER_JACOBI: a handle that never calls mi355cg_set_smoother runs the launches it always ran.
 * mi355cg_set_smoother may be called before or after mi355cg_set_preconditioner* and mi355cg_set_shift, with the same result:
 * with a hierarchy present it builds or frees the per-level line tables (2 N_l doubles per level) in place and takes effect at
 * once; without one the value is kept for the next mi355cg_set_preconditioner*.  Everything that runs the fp64 cycle follows it
 * (mi355cg_apply_preconditioner, mi355cg_solve, mi355cg_solve_batch*, mi355cg_time_steps, mi355cg_eigs*); the batch and eigen
 * workspaces, x, r, b, u and a pending guess stay.  MI355CG_SMOOTHER_JACOBI after a line smoother gives the bits of a handle that
 * never had one.  On one-level grids (n <= 32) the cycle is the dense inverse: every smoother gives the same bits.
 * MI355CG_ERR_INVALID, the handle left as it was: a null handle, an unknown value, a CSR, slab / part or MI355CG_F32_MIXED
 * handle, a line smoother while the preconditioner is set with MI355CG_CYCLE_F32 -- and, the other way round,
 * mi355cg_set_preconditioner_ex(.., MI355CG_CYCLE_F32) while a line smoother is set.
 * mi355cg_get_smoother: the value as set, and the direction it means on this handle (0 none, 1 x, 2 y); null out-pointers are skipped. */
#define MI355CG_SMOOTHER_JACOBI    0   /* the default: damped point Jacobi */
#define MI355CG_SMOOTHER_LINE_X    1   /* lines along x (rows)    */
#define MI355CG_SMOOTHER_LINE_Y    2   /* lines along y (columns) */
#define MI355CG_SMOOTHER_LINE_AUTO 3   /* y-lines if level 0 has y_k > x_k, else x-lines; one decision for all levels */
int  mi355cg_set_smoother(mi355cg_handle h, int smoother);
int  mi355cg_get_smoother(mi355cg_handle h, int *smoother, int *direction);

/* Batched solves: nrhs right-hand sides on one handle that has a multigrid preconditioner set (fp64 cycle), solved together by
 * one preconditioned CG loop whose every launch carries all systems that are still iterating, so the launches and the three
 * host waits per iteration of one solve are paid once per batch.
 * b, x: nrhs vectors of mi355cg_size(h) doubles each, packed order, one after the other; out: nrhs entries.
 * System s gets exactly the bits that mi355cg_set_rhs(h, b_s); mi355cg_solve(h, params, NULL, NULL, stop_flag, &res);
 * mi355cg_get_solution(h, x_s) gives on the same handle: all of x_s and iterations, converged, stop_reason,
 * final_residual_norm, final_precision, r_norm2, initial_r_norm2.  Every system follows the stop rule on its own numbers; one
 * that stops is frozen and later launches cover only the others.  stop_flag is read once per iteration: when it is set, every
 * system still iterating ends MI355CG_STOP_INTERRUPTED and the finished ones keep their results.  Both rules and
 * fixed_iterations work.  final_error_norm is DBL_MAX; solve_seconds and loop_seconds are the whole batch's, the same in every
 * entry.  The handle's own state is untouched: its b, its last x and r, what mi355cg_get_solution returns.
 * MI355CG_ERR_INVALID, before anything is allocated or written: a null pointer, nrhs < 1 or > MI355CG_BATCH_MAX, x overlapping
 * b, use_true_solution != 0 or diagnostics != 0 (a batch has no per-system exact solution and no callbacks; note that
 * mi355cg_default_params sets use_true_solution = 1), a preconditioner set with MI355CG_CYCLE_F32.  MI355CG_ERR_STATE: no
 * preconditioner is set (CSR, part and F32_MIXED handles cannot have one).
 * _device: b_dev and x_dev are in device memory of the handle's GPU.  The work runs on the handle's own stream: the caller
 * makes b_dev complete before the call, and the call returns after that stream is idle, x_dev written.
 * Workspace: per system the PCG vectors of level 0 (x, r, z, two directions, A p, the cycle's work vector: seven vectors of the
 * handle's storage size) and the three vectors of every coarser level (about one more), i.e. about 8 level-0 vectors a system
 * -- about 1 GB a system at n = 4096, 50 MB at n = 1000 (computed from the layout) -- plus nrhs packed vectors of staging for
 * the host entry point.  Allocated on first use, kept on the handle, grown when a larger nrhs comes; freed by
 * mi355cg_batch_release (MI355CG_OK if there is none), every mi355cg_set_preconditioner* call that is not refused and
 * mi355cg_destroy.  If it cannot be allocated: MI355CG_ERR_HIP, nothing leaked, the handle usable as before.                                                */
#define MI355CG_BATCH_MAX 64  /* the per-system scalars and the list of active systems travel as kernel arguments */
int  mi355cg_solve_batch(mi355cg_handle h, const mi355cg_params *params, int nrhs, const double *b, double *x,
                         const volatile int *stop_flag, mi355cg_results *out);
int  mi355cg_solve_batch_device(mi355cg_handle h, const mi355cg_params *params, int nrhs, const double *b_dev, double *x_dev,
                                const volatile int *stop_flag, mi355cg_results *out);
int  mi355cg_batch_release(mi355cg_handle h);

/* ---- warm starts (extension: the reference's loops start from x = 0) ---------------------------------------------------
 * A guess x0 (packed order, mi355cg_size(h) doubles) makes the next mi355cg_solve on the handle start from x = x0 and
 * r0 = b - A x0, where A x0 is bit for bit what mi355cg_apply returns and the subtraction is one rounding
 * (matrix_free_system.cpp:389-392); the first direction is built from r0 as the cold start builds it from b, and the loop, the
 * stop flag and the callbacks are those of a cold solve, on the plain and on the preconditioned path.  A guess of zeros is the
 * cold solve bit for bit.  REL_2NORM with a guess stops on ||r||_2 <= eps_rel ||b||_2 (the same thing for x0 = 0), so a warm
 * start or a continuation reaches the cold solve's target with less work; initial_r_norm2 stays ||r0||_2; a start that already
 * meets the rule returns 0 iterations, converged, x = x0.  MSG_MAXNORM with a guess applies the residual test and (where enabled
 * and u is present) the exact-error test to the start state before iteration 1 (r0 may be 0); a cold solve enters iteration 1
 * untested, as the reference does.  The it = 0 callback reports the norms of r0 and x0 - u.
 * The guess is one-shot: the next mi355cg_solve consumes it whatever it returns, later solves are cold.  It is written straight
 * into the handle's x (no extra vector), so from the call to that solve mi355cg_get_solution, _get_recursive_residual and
 * _get_true_residual return MI355CG_ERR_STATE; x0 = NULL withdraws a pending guess and leaves them so until the next solve.
 * mi355cg_set_rhs between the guess and the solve is the normal use (same guess, new b); changing or removing the
 * preconditioner keeps the guess.  _device: x0_dev is in device memory of the handle's GPU, complete before the call.
 * mi355cg_use_solution_as_initial_guess: the x of the last solve is the guess, without a copy -- after a solve that ended
 * MI355CG_STOP_INTERRUPTED or MI355CG_STOP_ITERATIONS this continues it; MI355CG_ERR_STATE if no solve has run.
 * MI355CG_ERR_INVALID, the handle left as it was: a null handle, CSR handles, slab / part handles, MI355CG_F32_MIXED handles.
 * Teams have no warm start.                                                                                                   */
int  mi355cg_set_initial_guess(mi355cg_handle h, const double *x0);            /* host, packed; NULL withdraws a pending guess */
int  mi355cg_set_initial_guess_device(mi355cg_handle h, const double *x0_dev); /* packed, device memory of the handle's GPU   */
int  mi355cg_use_solution_as_initial_guess(mi355cg_handle h);                  /* the x of the last solve, no copy            */
/* mi355cg_solve_batch* with a guess per system: x is in/out, nrhs guesses on entry, the solutions on return.  System s gets
 * exactly the bits of mi355cg_set_rhs(h, b_s); mi355cg_set_initial_guess(h, x0_s); mi355cg_solve; mi355cg_get_solution on the
 * same handle, the 0-iteration case included (such a system never enters a launch of the loop).  Refusals and workspace as for
 * mi355cg_solve_batch*; the host entry point stages 2 nrhs packed vectors.                                                    */
int  mi355cg_solve_batch_from(mi355cg_handle h, const mi355cg_params *params, int nrhs, const double *b, double *x,
                              const volatile int *stop_flag, mi355cg_results *out);
int  mi355cg_solve_batch_device_from(mi355cg_handle h, const mi355cg_params *params, int nrhs, const double *b_dev, double *x_dev,
                                     const volatile int *stop_flag, mi355cg_results *out);

/* ---- diagonal shift and implicit time steps (extension: the reference inverts the Laplacian only) ------------------------
 * mi355cg_set_shift: while sigma is set the handle's operator is A - sigma I.  The stored diagonal is A_diag - sigma (one fp64
 * rounding, on the host); x_k and y_k are unchanged; every multigrid level uses its own -2 (x_k,l + y_k,l) - sigma, the same sigma on
 * every level, and the coarsest level's dense inverse is factored from the shifted matrix; the fp32 cycle rounds the shifted fp64
 * constants to fp32.  Everything that applies the operator follows: mi355cg_apply / _apply_device / _get_true_residual,
 * mi355cg_solve (both rules, diagnostics, fixed_iterations, the deferred x fold, graph replay), r0 = b - (A - sigma I) x0 of a warm
 * start, mi355cg_apply_preconditioner, preconditioned CG of either kind and cycle, and the four mi355cg_solve_batch* entry points.
 * sigma must be finite and >= 0 (the operator stays negative definite); anything else, a CSR handle (the caller owns that matrix), a
 * slab / part handle (hence teams) and an MI355CG_F32_MIXED handle are refused with MI355CG_ERR_INVALID, the handle left as it was.
 * set_shift(h, 0) gives bit for bit the handle that never had a shift.  A change of sigma drops the cached launch graphs of small
 * grids and rebuilds the hierarchy's coefficients and coarse inverse in place (kind, cycle and level count are unchanged; if the
 * rebuild fails, MI355CG_ERR_HIP, the old hierarchy and the old sigma stay).  The batch workspace stays: it holds vectors only.  The
 * last x and r, the handle's b and u and a pending guess stay too; mi355cg_set_preconditioner* after mi355cg_set_shift builds the
 * shifted hierarchy, and the two call orders give the same bits.  mi355cg_get_rhs, mi355cg_get_true_solution and the exact-error test
 * of the MSG rule keep referring to the caller's or the generated vectors: whether u solves the shifted system is the caller's
 * business.
 * mi355cg_time_steps: nsteps steps of the theta scheme for u_t = A u - g, g = the handle's right-hand side at the time of the call
 * (the steady state is the handle's Poisson problem); theta = 1 is implicit Euler, 0.5 Crank-Nicolson.  With sigma = 1 / (theta *
 * tau) a step solves (A - sigma I) u+ = b_step, b_step = -sigma u - ((1 - theta) / theta) A u + g / theta (A unshifted), built by
 * one kernel in one pass over u and g.  The state u is the handle's x: the starting state is the pending guess of
 * mi355cg_set_initial_guess*, or of mi355cg_use_solution_as_initial_guess; without one, MI355CG_ERR_STATE.  Every step warm-starts
 * from u in place through mi355cg_solve's own path, plain or preconditioned, with the warm start's semantics (REL_2NORM relative
 * to ||b_step||_2, a start that meets the rule takes 0 iterations); no packed vector crosses PCIe between steps.  The shift is set
 * to sigma if it is not already exactly sigma and is LEFT SET, so repeated calls with the same (tau, theta) pay the hierarchy
 * rebuild once, and later solves on the handle see A - sigma I until mi355cg_set_shift(h, 0).  out[k] is step k's results.
 * Stepping ends after the first step whose solve does not converge (iteration cap or stop request): *steps_done counts the converged
 * steps, out[steps_done] describes the unfinished one, x holds its last iterate, and the call still returns MI355CG_OK.  One call
 * with nsteps = k and k calls with nsteps = 1, each continued with mi355cg_use_solution_as_initial_guess, give the same bits.
 * nsteps = 0 is MI355CG_OK and does nothing (it needs no starting state and leaves the shift alone).  Memory: one vector of the
 * handle's storage size for b_step, allocated by the first call, freed by mi355cg_destroy; the handle's own b is bit for bit what
 * it was.  MI355CG_ERR_INVALID, before anything is written: a null argument (stop_flag may be null), tau not finite or <= 0, theta
 * outside (0, 1], nsteps < 0, params->diagnostics != 0 or use_true_solution != 0 (no callbacks, no per-step exact solution; note
 * that mi355cg_default_params sets use_true_solution = 1), and the handles that refuse a shift.
 * mi355cg_get_solution_device: mi355cg_get_solution into device memory of the handle's GPU (packed order), complete on return.   */
int  mi355cg_set_shift(mi355cg_handle h, double sigma);
int  mi355cg_get_shift(mi355cg_handle h, double *sigma);
int  mi355cg_time_steps(mi355cg_handle h, const mi355cg_params *params, double tau, double theta, int nsteps,
                        const volatile int *stop_flag, mi355cg_results *out /* nsteps */, int *steps_done);
int  mi355cg_get_solution_device(mi355cg_handle h, double *x_dev);   /* packed, device memory of the handle's GPU */

/* ---- lowest eigenpairs of the operator (extension: the reference solves linear systems only) ------------------------------
 * mi355cg_eigs: the nev lowest eigenpairs of K = -(A - sigma I), sigma the handle's shift, by a locally optimal block
 * preconditioned iteration (LOBPCG) whose preconditioner is one fp64 V-cycle of the handle's multigrid hierarchy: per iteration
 * one V-cycle and one operator apply per active column and no inner solve.  Sign convention: lambda[j] > 0 ascending and
 * (A - sigma I) v_j = -lambda[j] v_j, so with sigma = 0 the lambda are the Laplacian's eigenvalues in the usual positive sense and
 * with a shift they are the unshifted ones + sigma.  x holds `block` packed vectors, nev <= block <= MI355CG_EIG_BLOCK_MAX: the
 * start block on entry (any linearly independent vectors; the columns past nev are guard vectors that speed up the last wanted
 * pairs), the Ritz vectors on return, the first nev of them the eigenvectors, orthonormal in the Euclidean inner product of
 * packed vectors up to rounding.  lambda and resid have `block` entries: the Ritz values and res_j = ||K v_j - lambda_j v_j||_2 /
 * (lambda_j ||v_j||_2) of the returned vectors.  The iteration stops when res_j <= tol for all j < nev (CONVERGED, converged = 1),
 * at max_iterations (ITERATIONS) or when *stop_flag is non-zero (INTERRUPTED; read once per iteration, after the two other
 * tests).  Locking rule: a column, guard columns included, whose res_j <= tol gets no new search direction and no V-cycle in that
 * iteration (soft locking: it stays in the Rayleigh-Ritz basis, so it keeps being rotated with the others); without it a full
 * block of converged directions makes the basis singular.  The Rayleigh-Ritz step (mi355cg_rayleigh_ritz) runs on the host on the
 * <= 48 x 48 Gram matrices the device reduces in a fixed order; a basis [X, W, P] it refuses is retried once as [X, W] (counted in
 * p_drops), and if that is refused too the call ends with stop_reason BREAKDOWN, the last good vectors and MI355CG_OK.  Two calls
 * with the same input give the same bits.  The handle's right-hand side, last solution and residual, a pending guess and the shift
 * are untouched.  MI355CG_ERR_INVALID, before anything is allocated or written: a null argument (stop_flag may be null), nev < 1,
 * block < nev, block > MI355CG_EIG_BLOCK_MAX, block > mi355cg_size(h), tol not finite or <= 0, max_iterations < 1, a preconditioner
 * set with MI355CG_CYCLE_F32.  MI355CG_ERR_STATE: no preconditioner is set (CSR, slab / part and MI355CG_F32_MIXED handles cannot
 * have one).  Workspace: allocated by the first call, kept on the handle, regrown for a larger block, freed by
 * mi355cg_eigs_release, by every mi355cg_set_preconditioner* call that is not refused and by mi355cg_destroy; a failed allocation
 * returns MI355CG_ERR_HIP, leaks nothing and leaves the handle usable.  Memory per column of the block (computed from the layout,
 * not measured): 11 storage vectors (X, A X, P, A P twice, R, Z, A W) plus the V-cycle's vectors of one system (level 0's work
 * vector and three vectors per coarser level: 2.04 storage vectors at n = 1000), rounded up to whole storage vectors: 14 x 8 B x
 * the padded storage length for a hierarchy of two or more levels (11 for one level), 88 MB per column at n = 1000 and 1.4 GB for a
 * block of 16; besides that <= 38 MB of reduction partials.  The host entry point adds `block` packed vectors of staging.
 * mi355cg_eigs_device: the same with x in device memory of the handle's GPU (lambda, resid and out stay host memory).
 * mi355cg_block_gram: c[i * nb + j] = (a_i, b_j) for na and nb <= 48 packed host vectors, each entry summed in a fixed order (two
 * calls give the same bits); mi355cg_block_gram_indexed: the same for the vectors ia[0 .. nia) of a and ib[0 .. nib) of b (c is
 * nia x nib; a null list = all vectors in order) -- the device addresses subsets through such lists, never through copies.
 * mi355cg_block_combine: y_j = sum_i s_i coef[i * m + j], k <= 48 inputs, m <= 16 outputs, i ascending, unfused.  These are the
 * kernels the iteration is built from, on a temporary buffer; they need a whole-grid handle (not CSR, not a slab / part:
 * MI355CG_ERR_INVALID) but no preconditioner.
 * mi355cg_rayleigh_ritz (pure host arithmetic, no GPU needed): for the k x k pair G = S^T S, H = S^T K S (row-major, k <= 48; both
 * are symmetrised) theta ascending and coef (k x k, row-major, column j = Ritz vector j) with coef^T G coef = I, coef^T H coef =
 * diag(theta): D = diag(G)^-1/2, Cholesky D G D = L L^T, a cyclic Jacobi iteration on L^-1 D H D L^-T, coef = D L^-T Y.
 * MI355CG_ERR_STATE for a refused basis: a diagonal entry of G not positive and finite, a failed Cholesky, min diag(L) < 1e-6.  */
#define MI355CG_EIG_BLOCK_MAX 16
#define MI355CG_EIG_CONVERGED   0
#define MI355CG_EIG_ITERATIONS  1
#define MI355CG_EIG_INTERRUPTED 2
#define MI355CG_EIG_BREAKDOWN   3
typedef struct mi355cg_eig_results {
    int iterations;        /* Rayleigh-Ritz steps on [X, W, P] that were taken                                   */
    int converged;         /* 1: res_j <= tol for all j < nev                                                    */
    int stop_reason;       /* MI355CG_EIG_*                                                                      */
    int p_drops;           /* iterations that fell back to the basis [X, W]                                      */
    double solve_seconds;  /* wall time of the call's iteration, transfers of the device entry point included    */
} mi355cg_eig_results;
int  mi355cg_eigs(mi355cg_handle h, int nev, int block, double tol, int max_iterations, double *x, double *lambda, double *resid,
                  const volatile int *stop_flag, mi355cg_eig_results *out);
int  mi355cg_eigs_device(mi355cg_handle h, int nev, int block, double tol, int max_iterations, double *x_dev, double *lambda,
                         double *resid, const volatile int *stop_flag, mi355cg_eig_results *out);
int  mi355cg_eigs_release(mi355cg_handle h);
int  mi355cg_block_gram(mi355cg_handle h, int na, const double *a, int nb, const double *b, double *c);
int  mi355cg_block_gram_indexed(mi355cg_handle h, int na, const double *a, int nia, const int *ia, int nb, const double *b,
                                int nib, const int *ib, double *c);
int  mi355cg_block_combine(mi355cg_handle h, int k, const double *s, int m, const double *coef, double *y);
int  mi355cg_rayleigh_ritz(int k, const double *g, const double *hmat, double *theta, double *coef);

/* ---- measurement hooks (bench.py) ------------------------------------------------------------ */
/* Per-kernel device time of the last mi355cg_solve, measured with HIP events on the solve
 * stream when profiling was enabled.  kernel: 0 = fused stencil (A'), 1 = fused update (B).   */
int  mi355cg_set_profiling(mi355cg_handle h, int enable);
int  mi355cg_get_kernel_time(mi355cg_handle h, int kernel, double *avg_ms, long long *launches);
/* launch geometry: bytes of storage per vector, padded length, grid sizes (for DESIGN/bench)   */
int  mi355cg_get_layout(mi355cg_handle h, long long *padded_len, int *pitch_bottom, int *pitch_upper,
                        int *grid_stencil, int *grid_update, int *rows_per_item);
/* Deferred x fold of single-context fp64 solves (REL_2NORM without diagnostics): instead of touching x in every fourth update
 * launch, a ring of `depth` = 16 or 32 direction buffers is kept and one flat launch applies the last `depth` steps at once --
 * the same roundings in the same order, so the same bits.  Chosen at mi355cg_create: MI355CG_XFOLD=0 off, =16|32 forced, unset =
 * on for handles of 4 Mi owned elements or more whose ring fits in a quarter of the device's memory (32, else 16, else off);
 * an explicit MI355CG_XSTEPS turns it off.  depth: the depth in use, 0 = fused update.  extra_buffers: vectors the ring holds
 * beyond the handle's own, 0 until the first solve that folds (a failed allocation there sets depth to 0 for good).            */
int  mi355cg_get_xfold(mi355cg_handle h, int *depth, int *extra_buffers);

/* ---- on-chip solve mode: small grids in one workgroup (opt-in) --------------
 * The default solve runs two launches per iteration, whose cost is launch-bound and barely falls below N = 256.  For plain fp64
 * grid handles up to N = 128 the direction fits in the LDS of one CU and x, r in the registers of one workgroup: in mode
 * MI355CG_SOLVE_ONCHIP every chunk of iterations (sync_every, the callback schedule and the iteration cap cut them as before) is
 * ONE launch of ONE workgroup, ordered by workgroup barriers alone.  It takes bit-identical steps to the two-launch path: the
 * same x, residual, iteration count, stop reason, norms and callbacks; warm starts, shifts, mi355cg_time_steps and stop requests
 * work unchanged, and a solve may continue in the other mode through mi355cg_use_solution_as_initial_guess.
 *   mi355cg_set_solve_mode   MI355CG_ERR_INVALID (message names the limit) for N above 128, for CSR, F32_MIXED and slab/part
 *                            handles and for handles that have a preconditioner; mi355cg_set_preconditioner* on an on-chip handle
 *                            is refused the same way (MI355CG_PRECOND_NONE is always accepted): go back to
 *                            MI355CG_SOLVE_LAUNCHES first.  Changing the mode drops the cached chunk graphs.
 *   mi355cg_get_solve_mode   the mode, and how many on-chip chunk launches the last mi355cg_solve issued.  A diagnostics solve
 *                            (REL_2NORM with the per-iteration true residual) keeps the two-launch path in either mode and reports 0.
 *                            With mi355cg_set_profiling on, on-chip solves are not per-kernel timed: mi355cg_get_kernel_time
 *                            reports no launches for them.
 *   mi355cg_onchip_plan      pure host arithmetic, no GPU needed: the workgroup size, the LDS bytes in use and the unknowns per
 *                            thread for grid n; MI355CG_ERR_INVALID for odd n, n < 6 and n above the cap.
 * Environment: MI355CG_ONCHIP=1, read by mi355cg_create, selects the mode on eligible handles and is ignored on the others, so
 * an unmodified host of the reference's C++ interface can opt in.                                                              */
#define MI355CG_SOLVE_LAUNCHES 0
#define MI355CG_SOLVE_ONCHIP   1
int  mi355cg_set_solve_mode(mi355cg_handle h, int mode);
int  mi355cg_get_solve_mode(mi355cg_handle h, int *mode, long long *onchip_launches_last_solve);
int  mi355cg_onchip_plan(int n, int *threads, int *lds_bytes, int *elems_per_thread);

/* Batched on-chip solves: nsys independent systems on the grid of one eligible handle (plain fp64, N <= 128, no preconditioner),
 * ONE workgroup per system and one launch per chunk of iterations for all systems still iterating; a workgroup's LDS follows N,
 * so small grids share a CU.  The systems differ in right-hand side, guess and diagonal shift.
 * b, x: nsys vectors of mi355cg_size(h) doubles each, packed order, one after the other; out: nsys entries.
 * sigma: nsys doubles, each finite and >= 0, or NULL = every system has the handle's current shift.  The diagonal of system s is
 * A_diag - sigma_s, rounded once on the host, exactly as mi355cg_set_shift stores it.
 * System s gets exactly the bits that mi355cg_set_shift(h, sigma_s); mi355cg_set_rhs(h, b_s); [_from: mi355cg_set_initial_guess(h,
 * x0_s);] mi355cg_solve(h, params, NULL, NULL, stop_flag, &res); mi355cg_get_solution(h, x_s) gives on the same handle in either
 * solve mode: all of x_s and iterations, converged, stop_reason, final_residual_norm, final_precision, r_norm2, initial_r_norm2.
 * Every system follows the stop rule on its own numbers; one whose state says done costs an early-returning workgroup in later
 * chunks.  Both rules and fixed_iterations work.  _from: x is in/out, a guess per system; a warm MSG_MAXNORM system has the
 * start-state tests of mi355cg_solve applied and may end with 0 iterations, x = x0.  stop_flag is sampled by every workgroup once
 * per iteration: when it is set, every system still iterating ends MI355CG_STOP_INTERRUPTED and the finished ones keep their
 * results; a flag already set at the call interrupts all systems at 0 iterations.  final_error_norm is DBL_MAX; solve_seconds and
 * loop_seconds are the whole batch's, the same in every entry.  The handle's own state is untouched: its b, x, r, shift, solve
 * mode, pending guess and what the getters return; the call works whichever solve mode the handle is in.
 * MI355CG_ERR_INVALID, before anything is allocated or written: a null pointer, nsys < 1 or > MI355CG_MANY_MAX, x overlapping b,
 * an unknown rule, use_true_solution != 0 or diagnostics != 0 (note that mi355cg_default_params sets use_true_solution = 1), a
 * sigma that is negative or not finite, and every handle mi355cg_set_solve_mode(h, MI355CG_SOLVE_ONCHIP) refuses for its kind or
 * size (N > 128, CSR, F32_MIXED, slab / part handles), with that call's message.  MI355CG_ERR_STATE: the handle has a
 * preconditioner (mi355cg_solve_batch is the preconditioned batch).
 * _device: b_dev, x_dev and sigma_dev are in device memory of the handle's GPU.  The work runs on the handle's own stream: the
 * caller makes them complete before the call, and the call returns after that stream is idle, x_dev written.
 * Workspace: per system three packed vectors (x, r, one direction), two CG states, one slot of update partials, the diagonal and
 * ||r0||_2 -- 24 mi355cg_size(h) + 456 bytes -- plus 8 bytes; the host entry points stage b and x on top (2 nsys packed
 * vectors).  Allocated on first use, kept on the handle, grown when a larger nsys comes; freed by mi355cg_batch_release and
 * mi355cg_destroy.  If it cannot be allocated: MI355CG_ERR_HIP, nothing leaked, the handle usable as before.
 * mi355cg_solve_many_info (null out-pointers are skipped): the LDS bytes one workgroup of this grid takes; how many such
 * workgroups the runtime's occupancy query lets reside on one CU (the REL_2NORM kernel); the device workspace bytes for nsys
 * systems without the staging.  Refuses the handles the solves refuse.  Not a pure query when workgroups_per_cu is asked for: for
 * images above 64 KB (N >= 90) it opts the kernel in to that much dynamic LDS (hipFuncSetAttribute), as the first solve would;
 * the occupancy query needs it.                                                                                                 */
#define MI355CG_MANY_MAX 65536
int  mi355cg_solve_many(mi355cg_handle h, const mi355cg_params *params, int nsys, const double *b, double *x, const double *sigma,
                        const volatile int *stop_flag, mi355cg_results *out);
int  mi355cg_solve_many_from(mi355cg_handle h, const mi355cg_params *params, int nsys, const double *b, double *x, const double *sigma,
                             const volatile int *stop_flag, mi355cg_results *out);
int  mi355cg_solve_many_device(mi355cg_handle h, const mi355cg_params *params, int nsys, const double *b_dev, double *x_dev,
                               const double *sigma_dev, const volatile int *stop_flag, mi355cg_results *out);
int  mi355cg_solve_many_device_from(mi355cg_handle h, const mi355cg_params *params, int nsys, const double *b_dev, double *x_dev,
                                    const double *sigma_dev, const volatile int *stop_flag, mi355cg_results *out);
int  mi355cg_solve_many_info(mi355cg_handle h, int nsys, int *lds_bytes_per_workgroup, int *workgroups_per_cu, long long *workspace_bytes);

/* Ensemble time stepping on chip: nsys members on the grid of one eligible handle (exactly the handles mi355cg_solve_many takes),
 * each integrated over nsteps steps of the theta scheme for u_t = A u - g (mi355cg_time_steps), ONE workgroup per member from its
 * first step to its last: the step loop runs inside the launch and the host sees chunks only.  The members
 * differ in state u_s (in/out), forcing g_s and time step tau_s; theta and nsteps are shared.
 * tau: nsys doubles in HOST memory (both entry points).  g: nsys packed vectors, or NULL = the handle's right-hand side for every
 * member.  u: nsys packed vectors of mi355cg_size(h) doubles, the start states in, the states after steps_done[s] steps out (after
 * a step that did not converge: that step's last iterate).  out: nsys entries, the LAST STEP ATTEMPTED of each member.
 * steps_done: nsys ints, the converged steps.  step_iterations: NULL, or nsys x nsteps ints, member-major: the iterations of every
 * step attempted, -1 for steps not taken.
 * Member s gets exactly the bits that mi355cg_set_rhs(h, g_s); mi355cg_set_initial_guess(h, u0_s); mi355cg_time_steps(h, params,
 * tau_s, theta, nsteps, ..) give on a handle of the same grid in either solve mode: all of u_s, steps_done, the iteration count of
 * every step and, for the last step attempted, iterations, converged, stop_reason, r_norm2, initial_r_norm2, final_precision and
 * final_residual_norm.  The shift of member s is sigma_s = 1 / (theta tau_s), its diagonal A_diag - sigma_s rounded once on the
 * host as mi355cg_set_shift stores it; every step starts as a warm solve does (r = b_step - (A - sigma_s) u, reference norm
 * ||b_step||_2; under MSG_MAXNORM the start-state tests apply, so a step may take 0 iterations); max_iterations counts per step.  A
 * member ends after nsteps steps or after its first step that does not converge (the iteration cap or a stop request).
 * A launch gives every member sync_every units (default 200, MSG_MAXNORM 100): a CG iteration costs one, the transition from one
 * step to the next costs one; between two launches the host reads one word.  stop_flag is sampled by every workgroup once per
 * iteration: members still stepping end MI355CG_STOP_INTERRUPTED, finished members keep their results, a flag already set at the
 * call leaves every member at 0 steps with u = u0; a member the host stops between two steps reports the empty state of a step not
 * begun.  final_error_norm is DBL_MAX; solve_seconds and loop_seconds are the whole call's, the same in every entry.  The handle's
 * own state is untouched -- its b, x, r, shift, solve mode, pending guess and what the getters return; unlike mi355cg_time_steps,
 * which leaves the shift set.
 * MI355CG_ERR_INVALID, before anything is allocated or written: a null pointer (stop_flag, g and step_iterations may be null), nsys
 * < 1 or > MI355CG_MANY_MAX, nsteps < 0 or > MI355CG_STEPS_MANY_MAX_STEPS, nsys * nsteps > 2^26 with step_iterations given, theta
 * outside (0, 1], a tau_s that is not finite or <= 0 or whose 1 / (theta tau_s) is not finite, u overlapping g, an unknown rule,
 * use_true_solution != 0 or diagnostics != 0, and every handle mi355cg_solve_many refuses for its kind or size, with its message.
 * MI355CG_ERR_STATE: the handle has a preconditioner.  nsteps = 0 is MI355CG_OK and writes only steps_done = 0.  MI355CG_ERR_HIP
 * if a member still steps after ceil(nsteps (max_iterations + 1) / sync_every) + 1 launches (a guard: it cannot happen).
 * _device: g_dev and u_dev are in device memory of the handle's GPU, everything else in host memory; the work runs on the handle's
 * stream and the call returns after that stream is idle.
 * Workspace: that of mi355cg_solve_many for nsys systems, 16 bytes per member (its shift, its step index and ended flag), one
 * packed vector (the handle's right-hand side) and, with step_iterations, 4 nsys nsteps bytes; the host entry point stages g and u
 * on top (2 nsys packed vectors).  It grows on demand, shares the batch workspace of the handle and is freed by
 * mi355cg_batch_release and mi355cg_destroy.  mi355cg_time_steps_many_workspace: that many bytes for grid n, pure host arithmetic,
 * no GPU needed; MI355CG_ERR_INVALID for a grid, an nsys, an nsteps or a number of counts the calls above refuse.                */
#define MI355CG_STEPS_MANY_MAX_STEPS 65536
int  mi355cg_time_steps_many(mi355cg_handle h, const mi355cg_params *params, int nsys, int nsteps, double theta, const double *tau,
                             const double *g, double *u, const volatile int *stop_flag, mi355cg_results *out, int *steps_done,
                             int *step_iterations);
int  mi355cg_time_steps_many_device(mi355cg_handle h, const mi355cg_params *params, int nsys, int nsteps, double theta, const double *tau,
                                    const double *g_dev, double *u_dev, const volatile int *stop_flag, mi355cg_results *out,
                                    int *steps_done, int *step_iterations);
int  mi355cg_time_steps_many_workspace(int n, int nsys, int nsteps, int with_step_iterations, long long *bytes);

/* Ensemble wave-equation steps on chip: nsys members on the grid of one eligible handle (exactly the handles mi355cg_solve_many
 * takes), each integrated over nsteps steps of u_tt = A u - g_s with its own time step tau_s, ONE workgroup per member (DESIGN
 * section 12.3).  A is the UNSHIFTED operator of the handle.  The state of member s is the pair (u_s, v_s), v = u_t, both in and
 * out; nsteps and the scheme are shared.  One call of k steps gives the bits of k calls of one step: that is how a caller takes
 * snapshots.
 * tau: nsys doubles in HOST memory (both entry points).  g: nsys packed vectors, or NULL = the handle's right-hand side for every
 * member.  u, v: nsys packed vectors of mi355cg_size(h) doubles each.  out: nsys entries.  steps_done: nsys ints.
 * MI355CG_WAVE_VERLET, explicit: with h = 0.5 tau and au(u) = A0 u + xk (left + right) + yk (down + up), one rounding per
 * operation in this order,   a = au(u) - g;  vh = v + h a;  u = u + tau vh;  a = au(u) - g;  v = vh + h a.
 * The step loop runs inside the launch: one stencil pass and two axpys per step, no inner product and no decision; params is not
 * read and may be NULL, step_iterations must be NULL or is left untouched.  All members take the same number of steps; out[s]
 * reports iterations 0, converged 1.  tau_s must not exceed the bound of mi355cg_wave_cfl, beyond which the scheme diverges.
 * steps_per_launch (0: the default, 512; 1024 steps were measured at 15.3 ms per launch for 1024 members
 * of N = 128, the profile has the default's own times) cuts the run into ceil(nsteps / steps_per_launch)
 * launches; before each the host waits for the one before and tests stop_flag: when it is set, steps_done is what has run, every
 * member reports MI355CG_STOP_INTERRUPTED and (u, v) are the state at that step.
 * MI355CG_WAVE_NEWMARK, implicit (beta = 1/4, gamma = 1/2, unconditionally stable): with sigma = 4 / tau^2 and hv = 2 / tau,
 *    w = u + tau v;  b = (g + g) - sigma w;  b = b - au(u);  solve (A - sigma I) x = b from x0 = u;  v = hv (x - u) - v;  u = x,
 * every step the warm-started solve mi355cg_time_steps_many runs, under params as there (both rules, fixed_iterations,
 * max_iterations per step, sync_every units per launch; steps_per_launch is not read), the diagonal A_diag - sigma rounded once
 * as mi355cg_set_shift stores it: member s gets the bits of that solve on a handle of the same grid.  A member ends after its
 * first step that does not converge (the iteration cap or a stop request); its (u, v) are then the state after its last converged
 * step, out[s] and step_iterations report the step attempted, as mi355cg_time_steps_many does.
 * The handle's own state is untouched: its b, x, r, shift, solve mode, pending guess and what the getters return.
 * MI355CG_ERR_INVALID, before anything is allocated or written: a null h, tau, u, v, out or steps_done (Newmark: params), an
 * unknown scheme, any overlap among u, v and g, nsys < 1 or > MI355CG_MANY_MAX, nsteps < 0 or > MI355CG_STEPS_MANY_MAX_STEPS,
 * steps_per_launch < 0, a tau_s that is not finite or <= 0, Verlet: a tau_s above mi355cg_wave_cfl (the message names the bound
 * and the member), Newmark: a tau_s whose 4 / tau_s^2 is not finite, nsys * nsteps > 2^26 with step_iterations given, an unknown
 * rule, use_true_solution != 0 or diagnostics != 0, and every handle mi355cg_solve_many refuses, with its message.
 * MI355CG_ERR_STATE: the handle has a preconditioner.  nsteps = 0 is MI355CG_OK and writes only steps_done = 0.
 * _device: g_dev, u_dev and v_dev are in device memory of the handle's GPU, everything else in host memory; the work runs on the
 * handle's stream and the call returns after that stream is idle.
 * Workspace: Verlet, that of mi355cg_solve_many for nsys systems, 16 bytes per member (tau and 2 / tau) and one packed vector
 * (the handle's right-hand side); Newmark, that of mi355cg_time_steps_many and 16 bytes per member.  The host entry point stages
 * g, u and v on top (3 nsys packed vectors).  It shares the batch workspace of the handle, grows on demand and is freed by
 * mi355cg_batch_release and mi355cg_destroy.  mi355cg_wave_steps_many_workspace: that many bytes, pure host arithmetic.
 * mi355cg_wave_cfl: tau_max = 2 / sqrt(2 |A_diag|) of the UNSHIFTED operator, Gershgorin's bound on the spectrum: sufficient for
 * stability, not sharp; host arithmetic on the handle's geometry, for grid handles of any size.                               */
#define MI355CG_WAVE_VERLET  0     /* explicit: velocity Verlet (= leapfrog), tau limited by the CFL bound */
#define MI355CG_WAVE_NEWMARK 1     /* implicit: Newmark beta = 1/4, gamma = 1/2 (trapezoidal), unconditionally stable */
int  mi355cg_wave_steps_many(mi355cg_handle h, const mi355cg_params *params, int nsys, int nsteps, int scheme, const double *tau,
                             const double *g, double *u, double *v, int steps_per_launch, const volatile int *stop_flag,
                             mi355cg_results *out, int *steps_done, int *step_iterations);
int  mi355cg_wave_steps_many_device(mi355cg_handle h, const mi355cg_params *params, int nsys, int nsteps, int scheme, const double *tau,
                                    const double *g_dev, double *u_dev, double *v_dev, int steps_per_launch,
                                    const volatile int *stop_flag, mi355cg_results *out, int *steps_done, int *step_iterations);
int  mi355cg_wave_steps_many_workspace(int n, int nsys, int nsteps, int scheme, int with_step_iterations, long long *bytes);
int  mi355cg_wave_cfl(mi355cg_handle h, double *tau_max);

/* The explicit scheme with a source time function and receiver traces: mi355cg_wave_steps_many with
 * MI355CG_WAVE_VERLET, its forcing scaled in time and u sampled at a few nodes inside the launch.  tau, g, u, v, steps_per_launch,
 * stop_flag, out and steps_done are that call's; params, scheme and step_iterations have no part in it.
 * w: the amplitudes of the source, nsteps + 1 doubles per member, member s at w + s * w_stride; w_stride = 0: one row for all,
 * otherwise at least nsteps + 1.  w_s[n] is the amplitude at local time n tau_s.  With h = 0.5 tau the step from n to n + 1 is
 *    f = w[n] g;  a = au(u) - f;  vh = v + h a;  u = u + tau vh;  f = w[n + 1] g;  a = au(u) - f;  v = vh + h a,
 * one rounding per operation; the second a of step n is the first of step n + 1.  w = 1 gives the bits of mi355cg_wave_steps_many.
 * rec_nodes: nrec packed unknown indices in [0, mi355cg_size(h)), HOST memory in both entry points, shared by all members; nrec = 0:
 * none, rec_nodes and traces are not read.  After local step n = 1 .. nsteps with n % record_every == 0, sample j = n /
 * record_every - 1 is traces[(s * (nsteps / record_every) + j) * nrec + r] = u_s at receiver r after that step.
 * A call of k * record_every steps with the amplitudes w + k0, ..., then a call from the returned state with the amplitudes from
 * w + k0 + nsteps on give the bits of one long call, the traces one after the other; the cut into launches is as invisible.
 * When stop_flag ends the call, steps_done is what ran, (u, v) the state at that step, and the samples of steps that did not run
 * are left unwritten.
 * MI355CG_ERR_INVALID, before anything is allocated or written: everything mi355cg_wave_steps_many refuses of a Verlet call, a null
 * w, a w_stride that is neither 0 nor >= nsteps + 1, nrec outside 0 .. MI355CG_WAVE_MAX_RECEIVERS, record_every < 1, nrec > 0 with
 * a null rec_nodes or traces, a receiver outside [0, size), w or traces overlapping u, v, g or each other, and (host entry
 * point: the table can be read) an amplitude that is not finite.
 * _device: g_dev, u_dev, v_dev, w_dev and traces_dev are in device memory of the handle's GPU, everything else in host memory.
 * Workspace: that of the Verlet call and the image cells of MI355CG_WAVE_MAX_RECEIVERS receivers (ints); the host entry point
 * stages the tables and the traces on top of g, u and v.  It is the handle's batch workspace, freed by mi355cg_batch_release and
 * mi355cg_destroy.  mi355cg_wave_record_many_workspace: that many bytes, pure host arithmetic.                               */
#define MI355CG_WAVE_MAX_RECEIVERS 64
int  mi355cg_wave_record_many(mi355cg_handle h, int nsys, int nsteps, const double *tau, const double *g, double *u, double *v,
                              const double *w, long long w_stride, int nrec, const int *rec_nodes, int record_every, double *traces,
                              int steps_per_launch, const volatile int *stop_flag, mi355cg_results *out, int *steps_done);
int  mi355cg_wave_record_many_device(mi355cg_handle h, int nsys, int nsteps, const double *tau, const double *g_dev, double *u_dev,
                                     double *v_dev, const double *w_dev, long long w_stride, int nrec, const int *rec_nodes,
                                     int record_every, double *traces_dev, int steps_per_launch, const volatile int *stop_flag,
                                     mi355cg_results *out, int *steps_done);
int  mi355cg_wave_record_many_workspace(int n, int nsys, int nsteps, int nrec, int record_every, long long *bytes);

/* The recorded explicit scheme in a medium (no reference twin): member s integrates
 *    u_tt = c2_s o (A u) - w_s(t) g_s,
 * c2_s > 0 the squared wave speed at every unknown; the source is not scaled by it.  Everything but c2 and c2_stride is
 * mi355cg_wave_record_many's, the semantics of launches, chained calls, steps_done and the traces under a stop flag included.
 * c2: size doubles per member in the packed order, member s at c2 + s * c2_stride; c2_stride = 0: one medium for all members,
 * otherwise at least mi355cg_size(h).  With t = au(u) the acceleration is a = c2 * t - f, f = w g: two roundings after t, and the step is
 *    f = w[n] g;  a = c2 au(u) - f;  vh = v + h a;  u = u + tau vh;  f = w[n + 1] g;  a = c2 au(u) - f;  v = vh + h a.
 * c2 = 1 gives the bits of mi355cg_wave_record_many; every scaling by a power of two is exact, so c2 = 4 with (tau, v, g) gives
 * the u of that call with (2 tau, v / 2, g / 4) and twice its v.
 * The bound of member s is its own: mi355cg_wave_medium_cfl(h, max c2_s) = 2 / sqrt(2 |A_diag| max c2_s), sufficient, not sharp;
 * c2max = 1 gives the bits of mi355cg_wave_cfl.
 * MI355CG_ERR_INVALID, the handle's state, right-hand side, shift and solve mode untouched: everything mi355cg_wave_record_many
 * refuses, with its bound on tau replaced by the member's own; a null c2; a c2_stride that is neither 0 nor >= size; c2
 * overlapping u, v, g, w or the traces; an entry of c2 that is not finite or not > 0 (the message names the member); tau_s above
 * the member's bound (the message names the member and the bound).
 * _device: c2_dev is in device memory like g_dev, u_dev, v_dev, w_dev and traces_dev; one small launch reduces every medium to
 * its least and largest entry, which the host reads back once before the first step launch.  The host entry point finds them on
 * the host.  Workspace: that of mi355cg_wave_record_many and 16 bytes per member for those two numbers; the host entry point
 * stages the media beside g, u and v.  It is the handle's batch workspace, freed by mi355cg_batch_release and mi355cg_destroy.
 * mi355cg_wave_medium_many_workspace: that many bytes, pure host arithmetic.                                                   */
int  mi355cg_wave_medium_many(mi355cg_handle h, int nsys, int nsteps, const double *tau, const double *g, double *u, double *v,
                              const double *c2, long long c2_stride, const double *w, long long w_stride, int nrec, const int *rec_nodes,
                              int record_every, double *traces, int steps_per_launch, const volatile int *stop_flag, mi355cg_results *out,
                              int *steps_done);
int  mi355cg_wave_medium_many_device(mi355cg_handle h, int nsys, int nsteps, const double *tau, const double *g_dev, double *u_dev,
                                     double *v_dev, const double *c2_dev, long long c2_stride, const double *w_dev, long long w_stride,
                                     int nrec, const int *rec_nodes, int record_every, double *traces_dev, int steps_per_launch,
                                     const volatile int *stop_flag, mi355cg_results *out, int *steps_done);
int  mi355cg_wave_medium_many_workspace(int n, int nsys, int nsteps, int nrec, int record_every, long long *bytes);
int  mi355cg_wave_medium_cfl(mi355cg_handle h, double c2max, double *tau_max);

/* ... with a damping field, for absorbing (sponge) layers at the reflecting boundary (no reference twin):
 * member s integrates
 *    u_tt + d_s o u_t = c2_s o (A u) - w_s(t) g_s,
 * d_s >= 0 the damping rate (1 / time) at every unknown.  Everything but d and d_stride is mi355cg_wave_medium_many's, the
 * semantics of launches, chained calls, steps_done and the traces under a stop flag included.
 * d: size doubles per member in the packed order, member s at d + s * d_stride; d_stride = 0: one field for all members,
 * otherwise at least mi355cg_size(h).  The damping enters by a symmetric splitting, v times one factor per unknown at both ends
 * of a step, the factor the Cayley transform of the damping flow over tau / 2 (second order, time-symmetric):
 *    e = (0.25 tau) d;  s = (1 - e) / (1 + e)                      (every operation rounded once, the division IEEE's)
 *    v = s v;  f = w[n] g;  a = c2 au(u) - f;  vh = v + h a;  u = u + tau vh;  f = w[n + 1] g;  a = c2 au(u) - f;  v = vh + h a;  v = s v
 * and the v returned is the one after the closing multiply.  d = 0 gives s = 1 and the bits of mi355cg_wave_medium_many.  Without
 * a forcing the scheme's modified energy never grows.  The bound on tau is the medium's, mi355cg_wave_medium_cfl, unchanged.
 * MI355CG_ERR_INVALID, the handle's state, right-hand side, shift and solve mode untouched: everything
 * mi355cg_wave_medium_many refuses; a null d; a d_stride that is neither 0 nor >= size; d overlapping u, v, g, c2, w or the
 * traces; an entry of d that is negative or not finite (the message names the member); (0.25 tau_s) max d_s > 1, where the factor
 * turns negative and stronger damping would damp less (the message names the member and the bound 4 / tau_s).
 * _device: d_dev is in device memory like c2_dev; a second small launch reduces every damping row to its least and largest
 * entry, read back with the media's.  Workspace: that of mi355cg_wave_medium_many and 16 bytes per member for those two
 * numbers; the host entry point stages the damping rows beside the media.  It is the handle's batch workspace, freed by
 * mi355cg_batch_release and mi355cg_destroy.  mi355cg_wave_sponge_many_workspace: that many bytes, pure host arithmetic.        */
int  mi355cg_wave_sponge_many(mi355cg_handle h, int nsys, int nsteps, const double *tau, const double *g, double *u, double *v,
                              const double *c2, long long c2_stride, const double *d, long long d_stride, const double *w, long long w_stride,
                              int nrec, const int *rec_nodes, int record_every, double *traces, int steps_per_launch,
                              const volatile int *stop_flag, mi355cg_results *out, int *steps_done);
int  mi355cg_wave_sponge_many_device(mi355cg_handle h, int nsys, int nsteps, const double *tau, const double *g_dev, double *u_dev,
                                     double *v_dev, const double *c2_dev, long long c2_stride, const double *d_dev, long long d_stride,
                                     const double *w_dev, long long w_stride, int nrec, const int *rec_nodes, int record_every,
                                     double *traces_dev, int steps_per_launch, const volatile int *stop_flag, mi355cg_results *out,
                                     int *steps_done);
int  mi355cg_wave_sponge_many_workspace(int n, int nsys, int nsteps, int nrec, int record_every, long long *bytes);

/* The adjoint of the scheme in a medium, for the derivative of a trace misfit with respect to c2 (DESIGN section 12.7;
 * no reference twin): one forward run that keeps its history, one backward run.
 * mi355cg_wave_history_many: mi355cg_wave_medium_many's arguments and, behind c2, hist and hist_stride -- the same u, v and
 * traces, bit for bit, and row n of member s's history, size doubles at hist + s * hist_stride + n * size, is
 *    H[n] = au(u_n),  n = 0 .. nsteps,
 * the stencil value of the state after n steps before it is scaled by c2.  hist_stride is at least (nsteps + 1) * size;
 * mi355cg_wave_history_bytes(n, nsys, nsteps) is 8 * nsys * (nsteps + 1) * size, pure host arithmetic.  A call of no steps
 * writes nothing.  Under a stop flag rows 0 .. steps_done are written.  Refused on top of what mi355cg_wave_medium_many refuses:
 * a null hist, a hist_stride below (nsteps + 1) * size, hist overlapping u, v, g, c2, w or the traces.
 * mi355cg_wave_adjoint_many: the exact transpose of the scheme, from state index s = nsteps down to 1, with h = 0.5 tau, lam the
 * adjoint of u, q = c2 o (the adjoint of v) and S the sensitivity accumulator, every operation rounded once:
 *    if s % record_every == 0:  lam[rec_nodes[j]] = lam[rec_nodes[j]] + adj[s / record_every - 1][j],  j = 0 .. nrec - 1 ascending
 *    S = S + q H[s];  lam = lam + h au(q);  q = q + tau (c2 lam);  S = S + q H[s - 1];  lam = lam + h au(q)
 * adj: the adjoint sources, the derivative of the misfit with respect to the traces -- traces - observed for least squares --
 * [nsteps / record_every][nrec] per member at adj + s * adj_stride; adj_stride = 0: one table for all members, otherwise at
 * least (nsteps / record_every) * nrec.  lam, q, S: nsys packed vectors each, in and out.  From lam = q = S = 0:
 *    dJ/dc2 = h S / c2,   dJ/du0 = lam,   dJ/dv0 = q / c2,
 * divisions the caller makes once at the end: no division happens inside a call, so a backward run cut into calls at multiples
 * of record_every -- each with its slice of the history and of adj, from the (lam, q, S) the call before it left -- gives the
 * bits of one call, and a history can be rebuilt segment by segment from checkpoints of (u, v).  steps_per_launch, stop_flag,
 * out and steps_done (steps taken, counted from nsteps down) as in mi355cg_wave_medium_many.
 * MI355CG_ERR_INVALID, the handle's state, right-hand side, shift and solve mode untouched and nothing written: what
 * mi355cg_wave_medium_many refuses of nsys, nsteps, tau, c2, c2_stride, the receivers and steps_per_launch; a member's tau above
 * its own bound mi355cg_wave_medium_cfl(h, max c2_s) (the transpose has the forward scheme's stability); a null hist, lam, q or
 * S; a hist_stride below (nsteps + 1) * size; with receivers a null adj, an adj_stride that is neither 0 nor large enough; any
 * two of c2, hist, adj, lam, q, S overlapping; on the host entry point an adjoint source that is not finite.
 * _device: c2, hist, adj, lam, q, S in device memory, tau and rec_nodes in host memory.  Workspace: that of
 * mi355cg_wave_medium_many (mi355cg_wave_adjoint_many_workspace, pure host arithmetic); the host entry point stages the history,
 * the sources, the media and the three vectors on top.
 * Not built: the transpose of the damped step (mi355cg_wave_sponge_many), derivatives with respect to g or the amplitudes,
 * Newmark, anything but fp64.                                                                                                    */
int  mi355cg_wave_history_many(mi355cg_handle h, int nsys, int nsteps, const double *tau, const double *g, double *u, double *v,
                               const double *c2, long long c2_stride, double *hist, long long hist_stride, const double *w, long long w_stride,
                               int nrec, const int *rec_nodes, int record_every, double *traces, int steps_per_launch,
                               const volatile int *stop_flag, mi355cg_results *out, int *steps_done);
int  mi355cg_wave_history_many_device(mi355cg_handle h, int nsys, int nsteps, const double *tau, const double *g_dev, double *u_dev,
                                      double *v_dev, const double *c2_dev, long long c2_stride, double *hist_dev, long long hist_stride,
                                      const double *w_dev, long long w_stride, int nrec, const int *rec_nodes, int record_every,
                                      double *traces_dev, int steps_per_launch, const volatile int *stop_flag, mi355cg_results *out,
                                      int *steps_done);
int  mi355cg_wave_history_bytes(int n, int nsys, int nsteps, long long *bytes);
int  mi355cg_wave_adjoint_many(mi355cg_handle h, int nsys, int nsteps, const double *tau, const double *c2, long long c2_stride,
                               const double *hist, long long hist_stride, int nrec, const int *rec_nodes, int record_every,
                               const double *adj, long long adj_stride, double *lam, double *q, double *S, int steps_per_launch,
                               const volatile int *stop_flag, mi355cg_results *out, int *steps_done);
int  mi355cg_wave_adjoint_many_device(mi355cg_handle h, int nsys, int nsteps, const double *tau, const double *c2_dev, long long c2_stride,
                                      const double *hist_dev, long long hist_stride, int nrec, const int *rec_nodes, int record_every,
                                      const double *adj_dev, long long adj_stride, double *lam_dev, double *q_dev, double *S_dev,
                                      int steps_per_launch, const volatile int *stop_flag, mi355cg_results *out, int *steps_done);
int  mi355cg_wave_adjoint_many_workspace(int n, int nsys, int nsteps, int nrec, int record_every, long long *bytes);

/* ---- multi-GPU: one context per rank, one contiguous slab of grid rows per context --------------
 * The reference is single-process (no collectives exist in it); this is the scaling
 * surface.  The grid is cut into row slabs balanced by unknown count.  The library runs the
 * kernels; the caller (iterative_solvers_amd/distributed.py over torch.distributed = RCCL)
 * moves what crosses ranks each phase: the per-rank record = reduced partials, optionally followed
 * by the rank's two boundary rows (mi355cg_dist_sums_ptr -> all_gather -> gathered_* arguments,
 * mi355cg_dist_scatter_ghosts), or the boundary rows as point-to-point messages (mi355cg_dist_halo).
 * Every rank reduces the gathered partials in rank order, so all ranks take identical decisions.
 * All dist calls are asynchronous on `stream`, a hipStream_t taken literally (NULL = HIP's default
 * stream, which is torch's default stream too), so they order with the caller's collectives.
 * Host vectors of a slab context (get_rhs, get_solution, ...) cover only its owned packed range. */
int  mi355cg_slab_rows(int n, int world, int rank, int *y_lo, int *y_hi);
/* a part of a 2-D decomposition: rows [y_lo, y_hi] x columns [x_lo, x_hi); x-cuts are multiples of 128 (one wave's strip)   */
int  mi355cg_create_part(int n, int m, double a, double b, double c, double d, int dtype, int device,
                         int y_lo, int y_hi, int x_lo, int x_hi, mi355cg_handle *out);
/* out2[0] = sum of v, out2[1] = sum of v^2 over the handle's own cells, accumulated in double-double on the device (the value
 * does not depend on the decomposition).  which: 0 x, 1 recursive residual, 2 right-hand side, 3 exact solution.             */
int  mi355cg_checksum(mi355cg_handle h, int which, double *out2);
int  mi355cg_create_slab(int n, int m, double a, double b, double c, double d, int dtype, int device,
                         int y_lo, int y_hi, mi355cg_handle *out);
int  mi355cg_owned_range(mi355cg_handle h, long long *packed_begin, long long *packed_len, int *y_lo, int *y_hi);
int  mi355cg_dist_begin(mi355cg_handle h, const mi355cg_params *params, void *stream);
int  mi355cg_dist_reduce(mi355cg_handle h, int which /*0 stencil, 1 update*/, int with_rows, void *stream);
int  mi355cg_dist_sums_ptr(mi355cg_handle h, int which, void **dev_ptr, int *count /*record width*/);
int  mi355cg_dist_record_layout(mi355cg_handle h, int *header, int *row_slot, int *width);   /* doubles */
int  mi355cg_dist_scatter_ghosts(mi355cg_handle h, int vector /*0 r, 1 current direction*/,
                                 const double *gathered_records, int nranks, int rank, void *stream);
int  mi355cg_dist_stencil(mi355cg_handle h, const double *gathered_update_sums, int nranks, int estride,
                          int rows /*0 all, 1 interior, 2 edge rows*/, void *stream);
int  mi355cg_dist_flip(mi355cg_handle h);          /* once per stencil phase: new direction becomes current */
/* rows as in mi355cg_dist_stencil (a full update phase is {0} or {1, 2}).  The default update rebuilds A p from the
 * stored direction, so its first and last owned row read the direction's ghost rows -- which the stencil launch of a
 * slab keeps up to date by itself (it recomputes p_new on its halo anyway and stores it there, bit-identical to the
 * neighbour's rows): the direction never has to cross ranks and mi355cg_dist_update_reads_ghosts() returns 0.        */
int  mi355cg_dist_update(mi355cg_handle h, const double *gathered_stencil_sums, int nranks, int estride,
                         int rows /*0 all, 1 interior, 2 edge rows*/, void *stream);
int  mi355cg_dist_update_reads_ghosts(mi355cg_handle h);   /* non-zero: the caller must deliver the direction halo first (never, see above) */
int  mi355cg_dist_check(mi355cg_handle h, const double *gathered_update_sums, int nranks, int estride, void *stream);
int  mi355cg_dist_summary(mi355cg_handle h, mi355cg_results *out, int *done);   /* after a stream sync */
int  mi355cg_dist_finish(mi355cg_handle h, void *stream);   /* once after the loop: flush the pending x update */
int  mi355cg_dist_history(mi355cg_handle h, int iteration, double *precision, double *residual, double *error);
int  mi355cg_dist_halo(mi355cg_handle h, int vector /*0 r, 1 current direction*/,
                       void **send_lo, void **recv_lo, long long *n_send_lo,
                       void **send_hi, void **recv_hi, long long *n_send_hi);
int  mi355cg_dist_halo_recv_counts(mi355cg_handle h, long long *n_from_lo, long long *n_from_hi);

/* ---- teams: the native multi-GPU loop (csrc/team.h) ---------------------------------------------------------------
 * A team = a decomposition of the grid into `world` parts + a transport.  MI355CG_DECOMP_ROWS: row slabs balanced by
 * unknown count.  MI355CG_DECOMP_2D: (world/2) x 2 blocks -- BASELINE config 4's "2 x 2" for world = 4: y-cuts where the
 * slabs hold equal unknowns, every slab cut in x where ITS unknowns halve, x-cuts on 128-column strip boundaries.
 * Per iteration every part needs every part's 16-double record of partial sums twice, and its neighbours' boundary rows /
 * columns of the residual once.  Default transport: a one-workgroup reducer launch beside every producer launch stores the part's
 * record straight into every other part's mailbox (peer memory over xGMI, IPC-mapped across processes); the consumer launch reduces
 * its own partials and polls its own mailbox for the others; the halo is pushed into the neighbours' ghost cells by one small launch
 * whose last workgroup announces it with a 64-bit store the neighbour's stream waits for.
 * RCCL (ncclAllGather / ncclSend / ncclRecv) carries the bootstrap and is the fallback for both (environment:
 * MI355CG_TEAM_RECORDS = auto | rccl | mailbox | events, MI355CG_TEAM_WAIT = auto | kernel | stream, MI355CG_TEAM_HALO = auto |
 * inline | stream | push, MI355CG_TEAM_TIMEOUT_MS; mi355cg_team_describe says what a team uses).  Results are bit-identical to
 * the single-GPU solve for every decomposition and transport.  The reference has no counterpart (single process,
 * solver/solver.hpp:13 HostSpace only); the entry points mirror mi355cg_create / mi355cg_solve.                          */
#define MI355CG_DECOMP_ROWS 0
#define MI355CG_DECOMP_2D   1
typedef struct mi355cg_team_s *mi355cg_team;
typedef struct mi355cg_halo_msg {
    int id;          /* position in the global message order (every rank enumerates the same list)     */
    int peer;        /* the other part                                                                  */
    int send;        /* 1: this part sends, 0: it receives                                              */
    int kind;        /* 0: cells [x0, x1) of row y0;  1: column x0 over rows y0..y1                     */
    int y0, y1, x0, x1;
    long long count; /* doubles                                                                         */
} mi355cg_halo_msg;
/* pure host arithmetic (no GPU needed): the box of `rank`, and its halo messages per iteration */
int  mi355cg_decompose(int n, int world, int decomp, int rank, int *y_lo, int *y_hi, int *x_lo, int *x_hi);
int  mi355cg_halo_plan(int n, int world, int decomp, int rank, int max_msgs, int *n_msgs, mi355cg_halo_msg *msgs);
/* for tests (host arithmetic only): the work items of a part's launches.  which: 0 whole part, 1 interior, 2 edge.
 * panels: 8 ints per panel {y0, y1, first strip, strips, item rows, chunks, first item, ghost-column flags};
 * cls: [0] = number of XCD classes, [1..9] = their item boundaries                                                    */
int  mi355cg_debug_plan(int n, int world, int decomp, int rank, int which, int *n_panels, int *panels,
                        int *grid, int *n_items, int *cls);
/* LOCAL transport: this process drives all `world` parts; part r runs on devices[r % ndevices] (NULL: device 0).
 * Parts on different GPUs need peer access (xGMI).                                                                   */
int  mi355cg_team_create_local(int n, int m, double a, double b, double c, double d, int world,
                               const int *devices, int ndevices, int decomp, mi355cg_team *out);
/* RCCL transport: one process per part.  Rank 0 obtains a 128-byte id (ncclGetUniqueId) and hands it to the others by
 * any means (MPI, torch.distributed, a file); every rank then creates its side of the team (ncclCommInitRank inside).   */
int  mi355cg_team_unique_id(void *id128);
int  mi355cg_team_create_rccl(int n, int m, double a, double b, double c, double d, int world, int rank, int device,
                              const void *id128, int decomp, mi355cg_team *out);
void mi355cg_team_destroy(mi355cg_team t);
/* as mi355cg_solve (no per-iteration diagnostics).  Collective over the team: every rank calls it with the same params; the
 * callback and the stop flag may differ from rank to rank (the schedule of launches, polls and collectives depends on the
 * parameters only).  A stop request on any rank travels with that rank's next update record and every rank takes the decision
 * INTERRUPTED in the same iteration (msg_solver.cpp:82-87).  A record that does not arrive within MI355CG_TEAM_TIMEOUT_MS
 * (30 s) ends the solve with MI355CG_ERR_STATE on every rank instead of a hang; the team cannot be used after that.        */
int  mi355cg_team_solve(mi355cg_team t, const mi355cg_params *params, mi355cg_iter_cb cb, void *user,
                        const volatile int *stop_flag, mi355cg_results *out);
int  mi355cg_team_info(mi355cg_team t, int *world, int *nlocal, int *decomp, long long *size);
/* "transport=rccl records=mailbox wait=kernel halo=push split=0 ipc=1 shared_device=0 rccl_nranks=8 rccl_lib=...": what the next
 * solve of this team uses (rccl_nranks = what ncclCommCount reports for the team's communicator; 0 for a LOCAL team)        */
int  mi355cg_team_describe(mi355cg_team t, char *buf, int len);
int  mi355cg_team_part(mi355cg_team t, int local_index, mi355cg_handle *part, int *rank);
/* which as in mi355cg_checksum.  get_vector fills the entries of the caller's GLOBAL packed vector (length size) owned by
 * this process's parts; checksum covers this process's parts.                                                           */
int  mi355cg_team_get_vector(mi355cg_team t, int which, double *global_packed);
int  mi355cg_team_checksum(mi355cg_team t, int which, double *out2);
/* which: 2 right-hand side, 3 exact solution: every local part takes its entries of the caller's GLOBAL packed vector -- the b of
 * Solver(a, b, ...) (solver/solver.hpp:33-39) and the true_solution of MSGSolver::solve (msg_solver.cpp:64-72) may be anything.   */
int  mi355cg_team_set_vector(mi355cg_team t, int which, const double *global_packed);
/* MI355CG_F32_MIXED: the team's solves become mi355cg_create(..., MI355CG_F32_MIXED)'s algorithm -- fp64 iterative refinement around
 * an fp32 inner CG (REL_2NORM only) -- across the parts: BASELINE config 3 on more than one GPU.  Row slabs only (the fp32 kernels
 * march 256-column strips).  Collective.  No reference twin: the reference is fp64 only.                                          */
int  mi355cg_team_set_dtype(mi355cg_team t, int dtype);
int  mi355cg_team_setup_on_device(mi355cg_team t);                     /* mi355cg_setup_on_device for every local part */
int  mi355cg_team_set_profiling(mi355cg_team t, int enable);
int  mi355cg_team_phase_times(mi355cg_team t, double *kernel_ms, double *comm_ms, double *wall_ms);   /* per iteration */

#ifdef __cplusplus
}
#endif
#endif /* MI355CG_H */
