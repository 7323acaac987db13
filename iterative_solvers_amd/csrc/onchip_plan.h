// onchip_plan.h -- the layout of the single-workgroup on-chip CG solve: which thread owns which unknown, where a
// node and its four neighbours sit in the LDS image of the direction, how much LDS that takes.
//
// Free of HIP includes, like item_table.h: the kernel (onchip_kernels.h), mi355cg_onchip_plan and tests/cpp/onchip_plan_driver.cpp
// all read the layout from here.  So do the decisions the host takes about an ensemble of steppers (section 12.2, at the end):
// tests/cpp/onchip_report_driver.cpp prints them without a GPU.
//
//   * Unknowns are numbered row by row, x fastest: first the rows 1 .. N/2 of the bottom-right block (columns N/2+1 .. N-1), then the
//     rows N/2+1 .. N-1 of the upper block (columns 1 .. N-1).
//   * Thread t of T owns the unknowns t, t + T, t + 2T, ... (slot k = unknown k*T + t): the lanes of a wave touch neighbouring
//     cells of the image in every slot.  Its valid slots are a prefix of its `elems` slots.
//   * The image is the whole (N+1) x (N+1) bounding grid, cell(x, y) = y*(N+1) + x.  The neighbours of a cell are cell +- 1 and
//     cell +- (N+1).  Boundary nodes and the cut-out quadrant are cells no thread owns: they are zeroed once and never written, so they
//     are the Dirichlet zeros and the in_j masking of the streaming kernels in one.  Every neighbour of an interior node lies in the image.
#pragma once
#include "item_table.h"               // MI355CG_HD
#include "solve_loop.h"               // CgState, chunk_len, make_results: what the report of an ensemble member is made of

namespace mi355cg {

constexpr int kOnchipMaxN = 128;                      // largest grid the on-chip path takes (DESIGN section 12 says why)
constexpr int kOnchipMaxThreads = 512;                // one workgroup: 8 wave64, two per SIMD, so that a wave may use 256 VGPRs
constexpr int kOnchipMaxElems = 24;                   // unknowns per thread at the cap
constexpr int kOnchipLdsLimit = 160 * 1024;           // LDS of one CU (gfx950)
constexpr int kOnchipMaxCells = (kOnchipMaxN + 1) * (kOnchipMaxN + 1);
// beside the image: the per-wave partials of the two reductions (4 and 10 doubles per wave) and the CG state (256 B at most)
constexpr int kOnchipSideBytes = (kOnchipMaxThreads / 64) * (4 + 10) * 8 + 256;

struct OnchipPlan {
    int n, half;
    int unknowns;                     // (N/2 - 1)(3N/2 - 1)
    int nbottom, wbottom, wupper;     // unknowns of the bottom block; interior columns of a bottom / an upper row
    int threads, elems;               // workgroup size (a multiple of 64); slots per thread (the kernel's unroll class: 1, 2, 4, 8, 16 or 24)
    int pitch, cells;                 // image: N + 1 cells per row, (N + 1)^2 cells
    int lds_bytes;                    // image of this N + the side data
};

MI355CG_HD inline bool onchip_supported(int n) { return n >= 6 && n % 2 == 0 && n <= kOnchipMaxN; }

// Small grids should not pay for 8 waves of reduction: the workgroup grows (64, 128, 256, 512 threads) only as far as it takes
// to keep a thread at four unknowns or fewer; from there the slots per thread grow.
MI355CG_HD inline OnchipPlan onchip_plan(int n) {
    OnchipPlan p{};
    if (!onchip_supported(n)) return p;
    p.n = n; p.half = n / 2;
    p.wbottom = p.half - 1; p.wupper = n - 1;
    p.nbottom = p.half * p.wbottom;
    p.unknowns = p.nbottom + (p.half - 1) * p.wupper;
    int t = 64;
    while (t < kOnchipMaxThreads && 4 * t < p.unknowns) t *= 2;
    p.threads = t;
    const int need = (p.unknowns + t - 1) / t;
    p.elems = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : need <= 16 ? 16 : kOnchipMaxElems;
    p.pitch = n + 1; p.cells = p.pitch * p.pitch;
    p.lds_bytes = p.cells * 8 + kOnchipSideBytes;
    return p;
}

// unknown i in [0, unknowns) -> its node
MI355CG_HD inline void onchip_node(const OnchipPlan& p, int i, int* x, int* y) {
    if (i < p.nbottom) { *y = 1 + i / p.wbottom; *x = p.half + 1 + i % p.wbottom; }
    else { const int j = i - p.nbottom; *y = p.half + 1 + j / p.wupper; *x = 1 + j % p.wupper; }
}
// the unknown in slot `slot` of thread `thread`, -1: the slot is empty
MI355CG_HD inline int onchip_owned(const OnchipPlan& p, int thread, int slot) {
    const int i = slot * p.threads + thread;
    return i < p.unknowns ? i : -1;
}
MI355CG_HD inline int onchip_cell(const OnchipPlan& p, int x, int y) { return y * p.pitch + x; }
// left, right, upper (y + 1) and lower (y - 1) neighbour of a cell
MI355CG_HD inline void onchip_neighbours(const OnchipPlan& p, int cell, int nb[4]) {
    nb[0] = cell - 1; nb[1] = cell + 1; nb[2] = cell + p.pitch; nb[3] = cell - p.pitch;
}

// ---- many systems, one workgroup each (k_onchip_many) ---------------------------------------------------------
// A workgroup's LDS is dynamic and follows N: the side data, then the image of its grid, the total rounded up to 16 bytes.  So small
// grids share a CU: floor(160 KiB / bytes) workgroups, as far as waves and registers allow.
MI355CG_HD inline int onchip_many_image_bytes(int cells) { return (cells * 8 + 15) / 16 * 16; }
MI355CG_HD inline int onchip_many_lds_bytes(int n) { return onchip_supported(n) ? onchip_many_image_bytes((n + 1) * (n + 1)) + kOnchipSideBytes : 0; }
// Device workspace of a batch of nsys systems: per system three packed vectors (x, r, one direction) and kOnchipManySysBytes of
// small data -- two CG states (the iteration boundary's and the host's summary) of 184 bytes, one slot of nine update partials, the
// system's diagonal and ||r0||_2 -- plus one counter of finished systems.  (The host entry points stage b and x on top: 2 nsys
// packed vectors; pinned host mirrors are not counted.)
constexpr int kOnchipManySysBytes = 2 * 184 + (9 + 2) * 8;
constexpr int kOnchipManyFixedBytes = 8;
MI355CG_HD inline long long onchip_many_workspace_bytes(int n, int nsys) {
    if (!onchip_supported(n) || nsys < 1) return 0;
    return (long long)nsys * (3LL * 8 * onchip_plan(n).unknowns + kOnchipManySysBytes) + kOnchipManyFixedBytes;
}

// ---- ensemble time stepping: the step loop inside the launch (k_onchip_steps) --------------------------------
// The right-hand side of one theta-scheme step of u_t = A u - g at ONE node: k_step_rhs's expression (step_kernels.h) in its order,
//   b = (stencil ? g / theta : g) - sigma u;   stencil (theta < 1):  b = b - c1 (A0 u + xk (left + right) + yk (down + up)),
// with the UNSHIFTED diagonal A0 and c1 = (1 - theta) / theta.  Not the summation order of the CG stencil (apply_at).  Plain fp64,
// no contraction: every translation unit that calls it is compiled with -ffp-contract=off.
struct OnchipStepCoef { double A0, xk, yk, theta, c1; int stencil; };
MI355CG_HD inline double onchip_step_rhs(const OnchipStepCoef& k, double sigma, double g, double uc, double left, double right, double down, double up) {
    double b = (k.stencil ? g / k.theta : g) - sigma * uc;
    if (k.stencil) {
        const double au = k.A0 * uc + k.xk * (left + right) + k.yk * (down + up);
        b = b - k.c1 * au;
    }
    return b;
}
// The launch's budget of units (one CG iteration or one step transition each) travels to the chunk body through one word of the
// side data, behind the CG state (184 bytes of the 256 reserved for it).
constexpr int kOnchipBudgetOffset = kOnchipSideBytes - 64;
// Device workspace of nsys members: that of a batch of nsys systems, per member its shift 1 / (theta tau_s) and the step
// bookkeeping (step index, ended flag), one packed vector (the handle's right-hand side, for g = NULL), and the iteration counts
// of nsys x nsteps steps (ints) when the caller asks for them.  (The host entry point stages u and g on top: 2 nsys packed vectors.)
// 0: refused -- a size the plan refuses or an ensemble beyond the limits of mi355cg_time_steps_many.
constexpr int kOnchipStepsMaxSys = 65536, kOnchipStepsMaxSteps = 65536;
constexpr long long kOnchipStepsMaxCounts = 1LL << 26;
constexpr int kOnchipStepsSysBytes = 8 + 2 * 4;
MI355CG_HD inline long long onchip_steps_workspace_bytes(int n, int nsys, int nsteps, int with_step_iterations) {
    if (!onchip_supported(n) || nsys < 1 || nsys > kOnchipStepsMaxSys || nsteps < 0 || nsteps > kOnchipStepsMaxSteps) return 0;
    const long long counts = with_step_iterations ? (long long)nsys * nsteps : 0;
    if (counts > kOnchipStepsMaxCounts) return 0;
    return onchip_many_workspace_bytes(n, nsys) + (long long)nsys * kOnchipStepsSysBytes + 8LL * onchip_plan(n).unknowns + 4 * counts;
}
struct OcStepBook { int step, ended; };       // converged steps so far (the index of the step being solved); the member has ended
static_assert(sizeof(double) + sizeof(OcStepBook) == kOnchipStepsSysBytes, "a member's share of the stepping workspace");

// -- what the host decides about an ensemble (mi355cg_time_steps_many*), free of HIP ------------------------------------------------
// Launches that take every member to its end when each gives a member m units: an iteration costs one, a transition costs one, so
// a member needs at most nsteps * (max_iterations + 1) units; one launch more notices the end.  More than that is an error.
inline long long onchip_steps_launch_cap(int nsteps, int max_iterations, int m) {
    const long long per_member = (long long)nsteps * ((long long)std::max(max_iterations, 0) + 1);
    return (per_member + m - 1) / m + 1;
}
// REL_2NORM reports the max-norm of the residual only where k_check decided, i.e. when the solve ended on a poll of mi355cg_solve's
// chunk schedule; a decision inside a chunk carries 0 (the rule does not reduce that norm).  A member's chunks are cut by its budget,
// not by that schedule, so the host says which of the two a single solve of `it` iterations reports.
inline bool rel_solve_ends_on_a_poll(const mi355cg_params* prm, int sync_every, int it, bool watched) {
    if (it <= 0) return false;                                     // decided by the first launch, before any poll
    int done = 0;
    for (bool first = watched; done < it; first = false) done += chunk_len(prm, false, sync_every, done, first);
    return done == it;
}
// What one member reports after the last launch.  polled: a summary was read at all (otherwise the empty state stands for it);
// interrupted: the host's stop flag ended the call, and only then is `boundary`, the iteration-boundary state, read.  summary: the
// member's state as the host polls it; norm0: ||r0||_2 of its last step; last_rmax: |r| of its last update (REL_2NORM); budget: the
// units of a launch (the sync_every of the single solve); watched: the caller passed a stop flag.
//   ended (after its last step, or a step that did not converge): the steps it converged, the state of the last one;
//   stopped between two steps: the step it finished counts, its iteration count is patched in, the next was not begun: empty state;
//   stopped inside a step: that step does not count and reports its state so far (REL_2NORM: no state is read before its first chunk).
// patch_step >= 0: step_iterations[patch_step] of this member becomes patch_iterations (when the caller asked for the counts).
struct OcStepReport { int steps_done; mi355cg_results res; int patch_step, patch_iterations; };
static inline OcStepReport onchip_step_report(const mi355cg_params* prm, bool msg, bool polled, bool interrupted, const OcStepBook& bk,
                                       const CgState& summary, const CgState& boundary, double norm0, double last_rmax, int budget, bool watched) {
    const CgState fin = polled ? summary : CgState{};
    OcStepReport rep{};
    rep.patch_step = -1;
    if (bk.ended || !interrupted) {
        rep.steps_done = bk.step;
        rep.res = make_results(fin, fin.done && fin.reason == MI355CG_STOP_INTERRUPTED, false, norm0);
        if (!msg) rep.res.final_residual_norm = rel_solve_ends_on_a_poll(prm, budget, fin.it, watched) ? last_rmax : 0.0;
    } else if (boundary.done) {
        rep.steps_done = bk.step + 1;
        rep.patch_step = bk.step; rep.patch_iterations = boundary.it;
        rep.res = make_results(CgState{}, true, false, 0.0);
    } else {
        const bool begun = polled && (msg || boundary.it > 0);
        rep.steps_done = bk.step;
        rep.res = make_results(begun ? fin : CgState{}, true, false, begun ? norm0 : 0.0);
        rep.patch_step = bk.step; rep.patch_iterations = rep.res.iterations;        // attempted: its count so far
    }
    return rep;
}

// ---- ensemble wave-equation steps: u_tt = A u - g (k_onchip_wave_verlet, k_onchip_wave_newmark) ---------------
// The per-node expressions of both schemes, one rounding per operation, no contraction.  au is onchip_step_rhs's stencil: the
// UNSHIFTED diagonal A0, the neighbours in that order.
//   velocity Verlet, h = 0.5 * tau:   a = au(u) - g;   vh = v + h a;   u = u + tau vh;   a = au(u) - g;   v = vh + h a
//   Newmark (beta = 1/4, gamma = 1/2), sigma = 4 / tau^2, hv = 2 / tau:
//       w = u + tau v;   b = (g + g) - sigma w;   b = b - au(u);   (A - sigma I) x = b from x0 = u;   v = hv (x - u) - v;   u = x
constexpr int kWaveVerlet = 0, kWaveNewmark = 1;      // MI355CG_WAVE_VERLET, MI355CG_WAVE_NEWMARK
struct OnchipWaveCoef { double A0, xk, yk; };
MI355CG_HD inline double onchip_wave_au(const OnchipWaveCoef& k, double uc, double left, double right, double down, double up) {
    return k.A0 * uc + k.xk * (left + right) + k.yk * (down + up);
}
MI355CG_HD inline double onchip_wave_accel(const OnchipWaveCoef& k, double g, double uc, double left, double right, double down, double up) {
    return onchip_wave_au(k, uc, left, right, down, up) - g;
}
// A source time function (mi355cg_wave_record_many): the forcing at the time of amplitude w is w g, rounded
// once, and takes g's place in onchip_wave_accel.  1.0 * g == g: an amplitude of one is the constant forcing, bit for bit.
MI355CG_HD inline double onchip_wave_forcing(double w, double g) { return w * g; }
MI355CG_HD inline double onchip_wave_kick(double v, double h, double a) { return v + h * a; }            // both half kicks
MI355CG_HD inline double onchip_wave_drift(double u, double tau, double vh) { return u + tau * vh; }
MI355CG_HD inline double onchip_newmark_rhs(const OnchipWaveCoef& k, double sigma, double tau, double g, double v, double uc, double left,
                                            double right, double down, double up) {
    const double w = uc + tau * v;
    double b = (g + g) - sigma * w;
    b = b - onchip_wave_au(k, uc, left, right, down, up);
    return b;
}
MI355CG_HD inline double onchip_newmark_velocity(double hv, double x, double u, double v) { return hv * (x - u) - v; }
// The Gershgorin bound of the explicit scheme: every eigenvalue of -A lies in [0, 2 |A0|], and velocity Verlet is stable for
// tau^2 * lambda_max <= 4.  Sufficient, not sharp.
inline double onchip_wave_cfl(double A0) { return 2.0 / std::sqrt(2.0 * std::fabs(A0)); }
// Device workspace of nsys members.  Verlet: the batch workspace of nsys systems (the driver's), per member its tau and 2 / tau,
// one packed vector (the handle's right-hand side, for g = NULL).  Newmark: the stepping workspace of nsys members and nsteps
// steps (it has that vector), per member its tau and 2 / tau.  The state (u, v) lives in the caller's vectors.  (The host entry
// point stages g, u and v on top: 3 nsys packed vectors.)  0: refused, as onchip_steps_workspace_bytes refuses.
constexpr int kOnchipWaveSysBytes = 2 * 8;
MI355CG_HD inline long long onchip_wave_workspace_bytes(int n, int nsys, int nsteps, int scheme, int with_step_iterations) {
    if (scheme != kWaveVerlet && scheme != kWaveNewmark) return 0;
    const long long steps = onchip_steps_workspace_bytes(n, nsys, nsteps, scheme == kWaveNewmark && with_step_iterations);
    if (steps == 0) return 0;
    if (scheme == kWaveNewmark) return steps + (long long)nsys * kOnchipWaveSysBytes;
    return onchip_many_workspace_bytes(n, nsys) + (long long)nsys * kOnchipWaveSysBytes + 8LL * onchip_plan(n).unknowns;
}
// With a source and receivers (mi355cg_wave_record_many*): the Verlet workspace and the image cells of kOnchipWaveMaxRec receivers
// (ints).  The amplitude tables and the traces live in the caller's memory.  (The host entry point stages them on top of g, u and
// v: the tables, nsteps + 1 doubles per row, and nsys x (nsteps / record_every) x nrec doubles of traces.)  0: refused -- what the
// Verlet workspace refuses, nrec outside 0 .. kOnchipWaveMaxRec, record_every < 1.
constexpr int kOnchipWaveMaxRec = 64;
MI355CG_HD inline long long onchip_wave_record_workspace_bytes(int n, int nsys, int nsteps, int nrec, int record_every) {
    if (nrec < 0 || nrec > kOnchipWaveMaxRec || record_every < 1) return 0;
    const long long verlet = onchip_wave_workspace_bytes(n, nsys, nsteps, kWaveVerlet, 0);
    return verlet == 0 ? 0 : verlet + 4LL * kOnchipWaveMaxRec;
}
// A medium (mi355cg_wave_medium_many): u_tt = c2 o (A u) - w(t) g with the squared wave speed c2 > 0 of every
// unknown.  The acceleration is the stencil scaled, then the forcing taken off, two roundings after au; the source is not scaled.
// 1.0 * t == t: a unit medium is onchip_wave_accel with the forcing w g, bit for bit.
MI355CG_HD inline double onchip_wave_medium_accel(const OnchipWaveCoef& k, double c2, double f, double uc, double left, double right, double down, double up) {
    const double t = onchip_wave_au(k, uc, left, right, down, up);
    return c2 * t - f;
}
// Its bound: -C A with C = diag(c2) is similar to the symmetric C^(1/2) (-A) C^(1/2), whose eigenvalues lie in [0, 2 |A0| max c2].
// Sufficient, not sharp.  (2 |A0|) * 1.0 is exact: c2max == 1.0 gives the bits of onchip_wave_cfl.
inline double onchip_wave_medium_cfl(double A0, double c2max) { return 2.0 / std::sqrt(2.0 * std::fabs(A0) * c2max); }
// Its workspace: that of the recorded call and two doubles per member, the least and the largest entry of its medium as
// k_oc_medium_range leaves them for the host.  (The host entry point stages the media on top of g, u and v: nsys packed vectors,
// or one.)  0: refused, as onchip_wave_record_workspace_bytes refuses.
constexpr int kOnchipWaveMediumSysBytes = 2 * 8;
MI355CG_HD inline long long onchip_wave_medium_workspace_bytes(int n, int nsys, int nsteps, int nrec, int record_every) {
    const long long record = onchip_wave_record_workspace_bytes(n, nsys, nsteps, nrec, record_every);
    return record == 0 ? 0 : record + (long long)nsys * kOnchipWaveMediumSysBytes;
}
// A damping field (mi355cg_wave_sponge_many): u_tt + d o u_t = c2 o (A u) - w(t) g with the damping rate
// d >= 0 (1 / time) of every unknown, for absorbing (sponge) layers.  The damping flow v' = -d v over tau / 2 enters at both ends
// of the step as its Cayley transform, one factor per unknown formed once per launch; one rounding per operation, the division
// IEEE's.  d = 0 gives s = 1.0 and 1.0 * v == v: the bits of the medium call.
//   e = (0.25 tau) d;  s = (1 - e) / (1 + e);
//   v = s v;  f = w[n] g;  a = c2 au(u) - f;  vh = v + h a;  u = u + tau vh;  f = w[n + 1] g;  a = c2 au(u) - f;  v = vh + h a;  v = s v
// |s| <= 1 for e >= 0, but s < 0 for e > 1 and s -> -1 (no damping at all) as e grows: kOnchipWaveSpongeMaxE is the largest
// (0.25 tau) max d a call takes.  No new restriction on tau: onchip_wave_medium_cfl stays the bound.
constexpr double kOnchipWaveSpongeMaxE = 1.0;
MI355CG_HD inline double onchip_wave_sponge_factor(double tau, double d) {
    const double e = (0.25 * tau) * d;
    return (1.0 - e) / (1.0 + e);
}
MI355CG_HD inline double onchip_wave_damp(double s, double v) { return s * v; }
// Its workspace: that of the medium call and two more doubles per member, the least and the largest entry of its damping row.
// (The host entry point stages the damping rows beside the media: nsys packed vectors, or one.)  0: refused as there.
constexpr int kOnchipWaveSpongeSysBytes = 2 * 8;
MI355CG_HD inline long long onchip_wave_sponge_workspace_bytes(int n, int nsys, int nsteps, int nrec, int record_every) {
    const long long medium = onchip_wave_medium_workspace_bytes(n, nsys, nsteps, nrec, record_every);
    return medium == 0 ? 0 : medium + (long long)nsys * kOnchipWaveSpongeSysBytes;
}
// The adjoint of the scheme in a medium (mi355cg_wave_history_many, mi355cg_wave_adjoint_many).  The forward
// run keeps H[n] = au(u_n), n = 0 .. nsteps: the stencil value t that onchip_wave_medium_accel forms before it scales it.  The
// onchip_wave_au and the function below are that expression in its two halves, so a kernel can store t between them: the same bits.
MI355CG_HD inline double onchip_wave_medium_accel_of(double c2, double t, double f) { return c2 * t - f; }
// The exact transpose of the step, from state index s = nsteps down to 1, h = 0.5 tau; lam is the adjoint of u, q = c2 o (the
// adjoint of v) the field the stencil acts on, S the sensitivity accumulator; one rounding per operation:
//   if s % record_every == 0:  lam[rec[j]] = lam[rec[j]] + r[s / record_every - 1][j],  j ascending
//   S = S + q H[s];  lam = lam + h au(q);  q = q + tau (c2 lam);  S = S + q H[s - 1];  lam = lam + h au(q)
// From lam = q = S = 0:  dJ/dc2 = h S / c2,  dJ/du0 = lam,  dJ/dv0 = q / c2 -- divisions the caller makes, once, at the end.
MI355CG_HD inline double onchip_wave_adjoint_inject(double lam, double r) { return lam + r; }
MI355CG_HD inline double onchip_wave_adjoint_sens(double S, double q, double H) { return S + q * H; }
MI355CG_HD inline double onchip_wave_adjoint_kick(double lam, double h, double aq) { return lam + h * aq; }
MI355CG_HD inline double onchip_wave_adjoint_drift(double q, double tau, double c2, double lam) { return q + tau * (c2 * lam); }
// The history of nsys members over nsteps steps: nsteps + 1 rows of one double per unknown each.  0: refused, as the workspaces.
MI355CG_HD inline long long onchip_wave_history_bytes(int n, int nsys, int nsteps) {
    if (!onchip_supported(n) || nsys < 1 || nsys > kOnchipStepsMaxSys || nsteps < 0 || nsteps > kOnchipStepsMaxSteps) return 0;
    return 8LL * nsys * ((long long)nsteps + 1) * onchip_plan(n).unknowns;
}
// The adjoint call's workspace is the medium call's: the driver's, tau, the receivers (their packed indices here) and the ranges
// of the media.  lam, q, S, the history and the adjoint sources live in the caller's memory.  0: refused as there.
MI355CG_HD inline long long onchip_wave_adjoint_workspace_bytes(int n, int nsys, int nsteps, int nrec, int record_every) {
    return onchip_wave_medium_workspace_bytes(n, nsys, nsteps, nrec, record_every);
}
// Steps of one explicit launch when the caller does not say: the host tests the stop flag between two launches, so the longest
// launch is the latency of a stop request, to stay under 10 ms.  Measured on one MI355X at N = 128, a launch of 1024 steps: 3.7 ms
// for one member, 4.0 ms for 256, 15.3 ms for 1024 members (one workgroup per CU at that size, so four in turn) -- hence half of
// that, 512.  profiles/onchip_wave_time_to_solution.txt ends with the launch times of this default as the timing tool measures them.
constexpr int kOnchipWaveDefaultSteps = 512;

static_assert(kOnchipSideBytes - 256 + 184 <= kOnchipBudgetOffset && kOnchipBudgetOffset % 8 == 0, "the budget word lies behind the CG state");
static_assert(kOnchipMaxCells * 8 + kOnchipSideBytes <= kOnchipLdsLimit, "the image of the largest grid and the side data fit in one CU's LDS");
static_assert((kOnchipMaxCells * 8 + 15) / 16 * 16 + kOnchipSideBytes <= kOnchipLdsLimit, "... with the image rounded up to 16 bytes too");
static_assert(kOnchipMaxThreads * kOnchipMaxElems >= (kOnchipMaxN / 2 - 1) * (3 * kOnchipMaxN / 2 - 1), "every unknown of the largest grid has a slot");

}  // namespace mi355cg
