// solve_loop.h -- the host side of a CG solve's loop protocol, written once: how many iterations are queued
// between two polls, which iterations a callback sees, when the MSG rule stops, what mi355cg_results reports.  Plain host functions
// over the state the kernels leave behind, no HIP: every solve loop of mi355cg.hip and team.h uses them, tests/cpp/solve_loop_driver.cpp too.
#pragma once
#include "../../include/mi355cg.h"
#include <algorithm>
#include <cfloat>
#include <cmath>

namespace mi355cg {

constexpr int kHist = 512;            // per-iteration norm history ring (>= sync_every)
constexpr int kRing = 8;              // direction buffers of a context (ring; M = xsteps <= kRing of them are in use); also the alpha history depth

// ---- CG state carried on the device ----------------------------------------------------------------
struct CgState {
    double alpha, beta;
    double rr;          // (r, r) of the current residual
    double rr_prev;     // (r, r) one decision earlier (lets a stopped solve resume with the right beta denominator)
    double rz;          // MSG: (r, z) of the current iteration (denominator of the next beta)
    double r0norm;      // ||r0||_2
    double rnorm2;      // ||r||_2
    double rmax, dmax, emax, d2, e2;
    int it, done, reason, converged, first;      // first: no iteration has run yet (no beta); 1 = cold start, 2 = warm start (r0norm is set: ||b||_2)
    int stop;           // a stop request was pending when the last update launch ended (single context: read from the pinned word; msg_solver.cpp:82-87)
    double alpha_hist[kRing];   // step length of iteration k at [k % kRing]: the folded x update (XM >= 2) applies up to kRing - 1 earlier steps at once
};
struct HistEntry { double dmax, rmax, emax, rnorm2, d2, e2, tr2; };   // tr2: ||b - A x||_2^2 (REL_2NORM diagnostics mode, written by k_resid2_hist)

// ---- chunks: the iterations queued between two host polls (the reference polls its stop flag every iteration, msg_solver.cpp:82)
inline int default_sync_every(const mi355cg_params* prm, bool msg) {
    return std::min(prm->sync_every > 0 ? prm->sync_every : (msg ? 100 : 200), kHist);
}
// A chunk ends at the iteration cap and, under MSG, on every callback iteration.  first_chunk: the first iteration on its own, so
// that the it == 1 callback is delivered -- and a stop requested from it honoured -- before more work is queued; the caller says
// when (a watched solve: callback or stop flag; a team: by the parameters alone, so that every rank takes the same schedule).
// Never 0: a chunk at the cap lets the kernels record ITERATIONS.
inline int chunk_len(const mi355cg_params* prm, bool msg, int sync_every, int it_done, bool first_chunk) {
    const int every = prm->callback_every;
    int m = std::min(sync_every, prm->max_iterations - it_done);
    if (msg && every > 0) m = std::min(m, every - it_done % every);
    if (first_chunk) m = 1;
    return std::max(m, 1);
}

// ---- callbacks of the iterations (it_done, it_now] a poll brought back, from the history ring.  fin: the state of that poll.
// MSG: it == 1 and every callback_every-th iteration (msg_solver.cpp:172-183), but not the iteration a criterion stopped on: the
// reference's callback sits after the breaks and that iteration reports through the final callback alone (:193-195).  Hitting the
// iteration cap is no break, and an interruption is noticed at the top of the NEXT iteration (:82-87), after this one's callback.
// diag (REL_2NORM with diagnostics): every iteration, 2-norms, 0-based index (matrix_free_system.cpp:466-468).
inline void replay_callbacks(mi355cg_iter_cb cb, void* user, const mi355cg_params* prm, const CgState& fin, const HistEntry* hist_h,
                             int it_done, int it_now, bool has_u, bool diag) {
    if (!cb || !(diag || prm->rule == MI355CG_RULE_MSG_MAXNORM)) return;
    const int every = prm->callback_every;
    for (int it = it_done + 1; it <= it_now; ++it) {
        const HistEntry& h = hist_h[it % kHist];
        if (diag) { cb(user, it - 1, std::sqrt(h.d2), std::sqrt(h.tr2), std::sqrt(h.e2)); continue; }
        const bool stopped_here = fin.done && fin.reason != MI355CG_STOP_ITERATIONS && fin.reason != MI355CG_STOP_INTERRUPTED && it == it_now;
        if ((it == 1 || (every > 0 && it % every == 0)) && !stopped_here) cb(user, it, h.dmax, h.rmax, has_u ? h.emax : DBL_MAX);
    }
}

// ---- the MSG stop tests on the host (msg_solver.cpp:144-163): precision, then residual, then exact error, strict <, each only
// while its eps > 0.  0 = go on (also under REL_2NORM and with fixed_iterations).  have_precision = false: the state of a warm
// start, which has no step behind it.
inline int msg_stop_reason(const mi355cg_params* prm, bool have_precision, double dmax, double rmax, bool has_u, double emax) {
    if (prm->rule != MI355CG_RULE_MSG_MAXNORM || prm->fixed_iterations) return 0;
    if (have_precision && prm->eps_precision > 0 && dmax < prm->eps_precision) return MI355CG_STOP_PRECISION;
    if (prm->eps_residual > 0 && rmax < prm->eps_residual) return MI355CG_STOP_RESIDUAL;
    if (prm->eps_exact_error > 0 && has_u && emax < prm->eps_exact_error) return MI355CG_STOP_EXACT_ERROR;
    return 0;
}

// ---- mi355cg_results (msg_solver.cpp:187-190): an interrupted solve has not converged whatever its last state says; there is no
// precision before the first step and no error norm without u.  The two times are the caller's to fill in.
inline mi355cg_results make_results(int it, bool interrupted, int converged, int reason, double dmax, double rmax, bool has_u, double emax,
                                    double r_norm2, double initial_r_norm2) {
    mi355cg_results res{};
    res.iterations = it;
    res.converged = interrupted ? 0 : converged;
    res.stop_reason = interrupted ? MI355CG_STOP_INTERRUPTED : reason;
    res.final_residual_norm = rmax;
    res.final_precision = it > 0 ? dmax : DBL_MAX;
    res.final_error_norm = has_u ? emax : DBL_MAX;
    res.r_norm2 = r_norm2; res.initial_r_norm2 = initial_r_norm2;
    return res;
}
inline mi355cg_results make_results(const CgState& fin, bool interrupted, bool has_u, double initial_r_norm2) {
    return make_results(fin.it, interrupted, fin.converged, fin.reason, fin.dmax, fin.rmax, has_u, fin.emax, fin.rnorm2, initial_r_norm2);
}
// F32_MIXED (no reference twin): judged by the fp64 true residual of the returned x, so the max-norms are not reported
inline mi355cg_results make_mixed_results(int it, bool interrupted, bool converged, double rnorm, double bnorm, int outer) {
    mi355cg_results res{};
    res.iterations = it; res.converged = converged ? 1 : 0;
    res.stop_reason = interrupted ? MI355CG_STOP_INTERRUPTED : (converged ? MI355CG_STOP_RESIDUAL : MI355CG_STOP_ITERATIONS);
    res.final_residual_norm = res.final_precision = res.final_error_norm = DBL_MAX;
    res.r_norm2 = rnorm; res.initial_r_norm2 = bnorm;
    res.refine_outer = outer; res.refine_true_rel = bnorm > 0 ? rnorm / bnorm : 0.0;
    return res;
}

}  // namespace mi355cg
