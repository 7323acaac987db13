// Prints what csrc/onchip_plan.h decides on the host about an ensemble of on-chip steppers: whether a
// REL_2NORM solve of `it` iterations ends on a poll, the launch cap, and what one member reports after the last launch.  No GPU, no
// library: the header is host-only.  tests/test_onchip_report_cpu.py checks the lines against a restatement of the contract.
#include "../../iterative_solvers_amd/csrc/onchip_plan.h"

#include <cstdio>

using namespace mi355cg;

namespace {

mi355cg_params params(int rule, int max_iterations) {
    mi355cg_params p{};
    p.rule = rule; p.max_iterations = max_iterations; p.callback_every = 100;
    return p;
}

void polls() {
    for (int watched = 0; watched < 2; ++watched) for (int sync : {1, 7, 200}) for (int cap : {1, 5, 50}) {
        const mi355cg_params p = params(MI355CG_RULE_REL_2NORM, cap);
        for (int it = 0; it <= cap; ++it) printf("poll %d %d %d %d : %d\n", watched, sync, cap, it, rel_solve_ends_on_a_poll(&p, sync, it, watched != 0) ? 1 : 0);
    }
}

void caps() {
    for (int nsteps : {1, 3, 65536}) for (int cap : {-5, 0, 1, 50, 1000000}) for (int m : {1, 7, 200, 512})
        printf("cap %d %d %d : %lld\n", nsteps, cap, m, onchip_steps_launch_cap(nsteps, cap, m));
}

constexpr int kBudget = 7, kCap = 50;
constexpr double kNorm0 = 8.0, kLastRmax = 0.375;

// the state the host polls of a member whose current step stands at iteration `it`
CgState summary(bool msg, int it, int done, int converged, int reason) {
    CgState s{};
    s.it = it; s.done = done; s.converged = converged; s.reason = reason;
    s.dmax = 0.125; s.rmax = msg ? 0.25 : 0.0; s.emax = 0.5; s.rnorm2 = 2.0; s.r0norm = 4.0;      // REL_2NORM does not reduce |r|: the state carries 0
    return s;
}

void report(const char* tag, int rule, int polled, int watched, bool interrupted, OcStepBook bk, const CgState& sum, const CgState& boundary) {
    const mi355cg_params p = params(rule, kCap);
    const bool msg = rule == MI355CG_RULE_MSG_MAXNORM;
    const OcStepReport rep = onchip_step_report(&p, msg, polled != 0, interrupted, bk, sum, boundary, kNorm0, kLastRmax, kBudget, watched != 0);
    const mi355cg_results& r = rep.res;
    printf("report %s %d %d %d %d : %d %d %d %d %.17g %.17g %.17g %.17g %.17g %d %d\n", tag, rule, polled, watched, sum.it, rep.steps_done, r.iterations,
           r.converged, r.stop_reason, r.final_residual_norm, r.final_precision, r.final_error_norm, r.r_norm2, r.initial_r_norm2, rep.patch_step,
           rep.patch_iterations);
}

void reports() {
    for (int rule : {MI355CG_RULE_MSG_MAXNORM, MI355CG_RULE_REL_2NORM}) for (int watched = 0; watched < 2; ++watched) {
        const bool msg = rule == MI355CG_RULE_MSG_MAXNORM;
        const int hit = msg ? MI355CG_STOP_PRECISION : MI355CG_STOP_RESIDUAL;
        const CgState none{};
        // ended: after its last step (4 of 4, converged), at an iteration on and off the polls of a single solve ...
        for (int it : {0, 12, 14, 15}) report("ended_last", rule, 1, watched, false, OcStepBook{4, 1}, summary(msg, it, 1, 1, hit), none);
        // ... at a step that hit the iteration cap, and at one the device saw the stop request in; `interrupted` or not: an ended member does not ask
        report("ended_cap", rule, 1, watched, false, OcStepBook{2, 1}, summary(msg, kCap, 1, 0, MI355CG_STOP_ITERATIONS), none);
        report("ended_cap", rule, 1, watched, true, OcStepBook{2, 1}, summary(msg, kCap, 1, 0, MI355CG_STOP_ITERATIONS), summary(msg, kCap, 1, 0, MI355CG_STOP_ITERATIONS));
        report("ended_stop", rule, 1, 1, true, OcStepBook{2, 1}, summary(msg, 9, 1, 0, MI355CG_STOP_INTERRUPTED), summary(msg, 9, 1, 0, MI355CG_STOP_INTERRUPTED));
        // stopped by the host between two steps: step 1 converged after 9 iterations, step 2 was not begun
        report("between", rule, 1, 1, true, OcStepBook{1, 0}, summary(msg, 9, 1, 1, hit), summary(msg, 9, 1, 1, hit));
        // stopped by the host inside step 1: after 5 iterations; before its first; before anything was polled at all
        report("inside", rule, 1, 1, true, OcStepBook{1, 0}, summary(msg, 5, 0, 0, 0), summary(msg, 5, 0, 0, 0));
        report("inside", rule, 1, 1, true, OcStepBook{1, 0}, summary(msg, 0, 0, 0, 0), summary(msg, 0, 0, 0, 0));
        report("inside", rule, 0, 1, true, OcStepBook{0, 0}, summary(msg, 33, 1, 1, hit), summary(msg, 0, 0, 0, 0));      // a stale mirror: not read
    }
}

}  // namespace

int main() {
    polls();
    caps();
    reports();
    return 0;
}
