// Prints what csrc/solve_loop.h decides for tables of parameters: chunk schedules, replayed callbacks, MSG stop reasons and
// result fields.  No GPU, no library: the header is host-only.  tests/test_solve_loop_cpu.py checks the lines against a
// restatement of the rules.
#include "../../iterative_solvers_amd/csrc/solve_loop.h"

#include <cstdio>
#include <vector>

using namespace mi355cg;

namespace {

struct Call { int it; double p, r, e; };
std::vector<Call> g_calls;
void record(void*, int it, double p, double r, double e) { g_calls.push_back(Call{it, p, r, e}); }

mi355cg_params params(int rule, int max_iterations, int every, int sync_every) {
    mi355cg_params p{};
    p.rule = rule; p.max_iterations = max_iterations; p.callback_every = every; p.sync_every = sync_every;
    return p;
}

void chunks() {
    const int rules[] = {MI355CG_RULE_MSG_MAXNORM, MI355CG_RULE_REL_2NORM};
    const int caps[] = {1, 7, 100, 699, 1000, 2500};
    const int everys[] = {0, 1, 7, 100, 600};
    const int syncs[] = {0, 1, 5, 64, 500, 512, 4000};
    for (int rule : rules) for (int cap : caps) for (int every : everys) for (int sync : syncs) for (int watched = 0; watched < 2; ++watched) {
        const mi355cg_params p = params(rule, cap, every, sync);
        const bool msg = rule == MI355CG_RULE_MSG_MAXNORM;
        const int se = default_sync_every(&p, msg);
        printf("chunks %d %d %d %d %d %d :", rule, cap, every, sync, watched, se);
        bool first = watched != 0;
        for (int it = 0; it < cap;) { const int m = chunk_len(&p, msg, se, it, first); first = false; printf(" %d", m); it += m; }
        printf(" : %d\n", chunk_len(&p, msg, se, cap, false));       // at the cap: one more iteration for the kernels to refuse
    }
}

// One solve that ends at iteration K with `reason`, polled at the iterations in `polls` (the last one is K).
void replay(int reason, int K, int every, bool has_u, bool diag, const std::vector<int>& polls) {
    std::vector<HistEntry> hist(kHist);
    for (int it = 0; it <= K; ++it) {
        HistEntry& h = hist[it % kHist];
        h.dmax = it + 0.25; h.rmax = it + 0.5; h.emax = it + 0.75; h.rnorm2 = 0; h.d2 = 4.0 * it * it; h.tr2 = 9.0 * it * it; h.e2 = 16.0 * it * it;
    }
    const mi355cg_params p = params(diag ? MI355CG_RULE_REL_2NORM : MI355CG_RULE_MSG_MAXNORM, 1 << 20, every, 0);
    g_calls.clear();
    int it_done = 0;
    for (int now : polls) {
        CgState fin{};
        fin.it = now;
        if (now == K) { fin.done = 1; fin.reason = reason; fin.converged = reason >= MI355CG_STOP_PRECISION && reason <= MI355CG_STOP_EXACT_ERROR; }
        replay_callbacks(record, nullptr, &p, fin, hist.data(), it_done, now, has_u, diag);
        it_done = now;
    }
    printf("replay %d %d %d %d %d %zu :", reason, K, every, has_u ? 1 : 0, diag ? 1 : 0, polls.size());
    for (const Call& c : g_calls) printf(" %d,%.17g,%.17g,%.17g", c.it, c.p, c.r, c.e);
    printf("\n");
}

void replays() {
    for (int reason = MI355CG_STOP_ITERATIONS; reason <= MI355CG_STOP_INTERRUPTED; ++reason)
        for (int K : {21, 23, 1, 7}) {
            std::vector<int> one{K}, many;
            for (int it = 1; it < K; it += 5) many.push_back(it);
            many.push_back(K);
            for (const auto& polls : {one, many}) {
                replay(reason, K, 7, true, false, polls);
                replay(reason, K, 0, false, false, polls);
            }
        }
    replay(MI355CG_STOP_RESIDUAL, 9, 7, true, true, {4, 9});
    g_calls.clear();                                                 // REL_2NORM without diagnostics, and no callback at all: nothing
    const mi355cg_params p = params(MI355CG_RULE_REL_2NORM, 100, 1, 0);
    std::vector<HistEntry> hist(kHist);
    CgState fin{};
    replay_callbacks(record, nullptr, &p, fin, hist.data(), 0, 50, true, false);
    replay_callbacks(nullptr, nullptr, &p, fin, hist.data(), 0, 50, true, true);
    printf("silent %zu\n", g_calls.size());
}

void stops() {
    for (int holds = 0; holds < 8; ++holds) for (int off = 0; off < 8; ++off) for (int have = 0; have < 2; ++have) for (int has_u = 0; has_u < 2; ++has_u) {
        mi355cg_params p = params(MI355CG_RULE_MSG_MAXNORM, 100, 7, 0);
        p.eps_precision = (off & 1) ? 0.0 : 1e-3; p.eps_residual = (off & 2) ? -1.0 : 1e-3; p.eps_exact_error = (off & 4) ? 0.0 : 1e-3;
        const double dmax = (holds & 1) ? 5e-4 : 1e-3, rmax = (holds & 2) ? 5e-4 : 1e-3, emax = (holds & 4) ? 5e-4 : 2e-3;      // equality does not stop
        printf("stop %d %d %d %d : %d\n", holds, off, have, has_u, msg_stop_reason(&p, have != 0, dmax, rmax, has_u != 0, emax));
    }
    mi355cg_params p = params(MI355CG_RULE_MSG_MAXNORM, 100, 7, 0);
    p.eps_precision = p.eps_residual = p.eps_exact_error = 1.0;
    p.fixed_iterations = 1;
    printf("stop_fixed %d\n", msg_stop_reason(&p, true, 0.0, 0.0, true, 0.0));
    p.fixed_iterations = 0; p.rule = MI355CG_RULE_REL_2NORM;
    printf("stop_rel2 %d\n", msg_stop_reason(&p, true, 0.0, 0.0, true, 0.0));
}

void print_results(const char* tag, const mi355cg_results& r) {
    printf("results %s : %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %.17g\n", tag, r.iterations, r.converged, r.stop_reason,
           r.final_residual_norm, r.final_precision, r.final_error_norm, r.r_norm2, r.initial_r_norm2, r.solve_seconds, r.refine_true_rel,
           r.refine_outer, r.loop_seconds);
}

void results() {
    CgState fin{};
    fin.it = 12; fin.done = 1; fin.converged = 1; fin.reason = MI355CG_STOP_RESIDUAL;
    fin.dmax = 0.125; fin.rmax = 0.25; fin.emax = 0.5; fin.rnorm2 = 2.0; fin.r0norm = 8.0;
    print_results("converged", make_results(fin, false, true, fin.r0norm));
    print_results("interrupted", make_results(fin, true, true, fin.r0norm));
    print_results("no_u", make_results(fin, false, false, 16.0));
    fin.it = 0;
    print_results("no_step", make_results(fin, false, true, fin.r0norm));
    print_results("mixed_converged", make_mixed_results(40, false, true, 1.0, 4.0, 3));
    print_results("mixed_interrupted", make_mixed_results(40, true, false, 1.0, 0.0, 1));
}

}  // namespace

int main() {
    chunks();
    replays();
    stops();
    results();
    return 0;
}
