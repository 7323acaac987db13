// mi355cg.hip -- C ABI (include/mi355cg.h) over the HIP kernels in cg_kernels.h.
// One context = one GPU = one part of the grid (the whole grid on a single GPU; a row slab or a 2-D block of a
// decomposed grid).  Teams of parts (native multi-GPU loop, RCCL / in-process transports) live in team.h.
// No CPU fallback: every compute entry point needs a working HIP device.
#include "../../include/mi355cg.h"
#include "cg_kernels.h"
#include "device_buffer.h"
#include "csr_kernels.h"
#include "grid_setup.h"
#include "mg_kernels.h"
#include "mg_batch_kernels.h"
#include "eig_kernels.h"
#include "mg_line_kernels.h"
#include "mg_kernels_f32.h"
#include "step_kernels.h"
#include "onchip_kernels.h"

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

using namespace mi355cg;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCK(expr)                                                                                  \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return fail(MI355CG_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

}  // namespace

// What Buf<T> (device_buffer.h) allocates and frees with: the only hipMalloc / hipHostMalloc / hipFree / hipHostFree of the file.
namespace mi355cg {
int mem_device_alloc(void** out, size_t bytes, bool zero, const char* what) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess && zero && (e = hipMemset(p, 0, bytes)) != hipSuccess) hipFree(p);
    if (e == hipSuccess) { *out = p; return MI355CG_OK; }
    (void)hipGetLastError();                     // a failed allocation leaves no sticky error behind
    return what ? fail(MI355CG_ERR_HIP, "%s", what) : fail(MI355CG_ERR_HIP, "device allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
}
void mem_device_free(void* p) { if (p) hipFree(p); }
int mem_pinned_alloc(void** out, size_t bytes, const char* what) {
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes);
    if (e == hipSuccess) { *out = p; return MI355CG_OK; }
    (void)hipGetLastError();
    return what ? fail(MI355CG_ERR_HIP, "%s", what) : fail(MI355CG_ERR_HIP, "pinned allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
}
void mem_pinned_free(void* p) { if (p) hipHostFree(p); }
}  // namespace mi355cg

namespace {

int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

inline long long round_up(long long v, long long m) { return (v + m - 1) / m * m; }

constexpr int kRecHeader = kRecWords;     // doubles reserved for the sums (hi/lo pairs) and maxes at the head of a part's record
constexpr int kStripCols = 128;    // fp64 strip = 64 lanes x double2: the unit of the x-cuts of a 2-D decomposition

struct EventPool {
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    hipEvent_t get() {
        if (used == ev.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return nullptr; ev.push_back(e); }
        return ev[used++];
    }
    void reset() { used = 0; }
    void destroy() { for (auto e : ev) hipEventDestroy(e); ev.clear(); used = 0; }
};

// Geometric multigrid preconditioner (mi355cg_set_preconditioner; kernels in mg_kernels.h).  Level 0 is the handle's grid; level
// l + 1 has 2 floor(N_l / 4) intervals (mg_shape) and the steps that keep the domain.  Per level: the right-hand side of its cycle
// (level 0: the caller's vector), a work vector and the cycle's result (level 0: the caller's output); the coarsest level keeps
// its dense inverse.
struct MgLevel {
    Geom g{}; long long len = 0; int grid = 0; Buf<double> rhs, a, out;
    Buf<double> tab;                    // line smoother: the level's Thomas factors, 2 N doubles (mg_line_kernels.h); nullptr without one
};
// The same three vectors of a level in fp32 (MI355CG_CYCLE_F32; level 0 too: r32, the work vector, the iterate) with the level's
// constants rounded to fp32; vec: columns per lane of its kernels (mg_kernels_f32.h)
struct MgLevel32 { Buf<float> rhs, a, out; MgCoef32 c{}; float scale = 0.f; int vec = 1; };
struct MgHier {
    int kind = 0;                       // MI355CG_PRECOND_MG or _MG_ANY: the kind last set (where both have a hierarchy it is this one)
    int cycle = MI355CG_CYCLE_F64;      // precision of the V-cycle; F32 keeps lv32 / inv32 instead of the levels' fp64 vectors and inv
    int line_dir = 0;                   // 0: damped point Jacobi; MG_LINE_X / MG_LINE_Y: line Jacobi along it, the levels keep `tab`
    std::vector<MgLevel> lv;
    std::vector<MgLevel32> lv32;
    Buf<float> inv32;                   // A_L^-1 rounded to fp32
    int ncoarse = 0;                    // unknowns of the coarsest level
    Buf<double> inv;                    // A_L^-1, ncoarse x ncoarse, row-major (unknowns in packed order)
    Buf<int> coff;                      // storage offset of every coarsest unknown
    Buf<double> z, p[2], q;             // PCG vectors of level 0 (p: ping-pong)
    Buf<double> part;                   // per-block partials, MG_NFIELDS x kMgMaxGrid
    Buf<double> part_h;                 // pinned copy
};

// Workspace of the batched solves (mi355cg_solve_batch*; kernels in mg_batch_kernels.h): one allocation, system-major.  System s
// keeps its level-0 PCG vectors (x, r, z, p[2], q, the cycle's work vector) and the three vectors of every coarser level at
// base + s * stride + the offsets below.  Built for a hierarchy on first use, kept on the handle, grown for a larger batch.
struct MgBatchLevel { long long rhs = -1, a = -1, out = -1; };
struct MgBatchWs {
    int cap = 0;                        // systems the vectors hold
    long long stride = 0;               // doubles per system, a multiple of 32 (256 B)
    Buf<double> base;                   // (the eigensolver's `cyc` borrows its workspace's)
    long long x = 0, r = 0, z = 0, p[2] = {0, 0}, q = 0;
    std::vector<MgBatchLevel> lv;
    Buf<double> part;                   // [system][field][block], cap x MGBG_NFIELDS (the widest launch) x level 0's grid
    Buf<double> red;                    // [position][field] sums of the last launch
    Buf<double> red_h;                  // pinned copy
    Buf<double> stage;                  // packed vectors of the host entry point, stage_cap x pk_len
    int stage_cap = 0;
};

// Workspace of the block eigensolver (mi355cg_eigs*; kernels in eig_kernels.h): one allocation, column-major
// like the batch workspace.  Column j of the block keeps its vectors in slots of `vlen` doubles at base + (j * slots + slot) * vlen:
// X, A X, P, A P twice (ping-pong: a Rayleigh-Ritz step writes the set it does not read), the residual R (after the cycle: the
// projected W), the cycle's result Z (after the projection: the copy mg_dir_apply keeps of its direction), A W, and from EIG_CYC
// on what mg_vcycle needs per system -- the offsets of `cyc`, an MgBatchWs that owns nothing.
enum { EIG_X = 0, EIG_AX = 2, EIG_P = 4, EIG_AP = 6, EIG_R = 8, EIG_Z = 9, EIG_AW = 10, EIG_CYC = 11 };
struct EigWs {
    int cap = 0;                        // columns the vectors hold
    long long vlen = 0;                 // doubles per slot: the storage length rounded up to 32 (256 B)
    int slots = 0;                      // slots per column
    Buf<double> base;
    MgBatchWs cyc;                      // base, stride and the levels' offsets as mg_vcycle reads them
    Buf<double> part;                   // block partials of the widest launch: a full symmetric gram of 48 vectors
    Buf<double> mat;                    // two reduced matrices (48 x 48), then the coefficients of a combine (48 x 16)
    Buf<double> mat_h;                  // pinned copy
    Buf<double> red;                    // [column][field] sums of k_eig_resid
    Buf<double> stage;                  // packed vectors of the host entry point, cap x pk_len
};

// Workspace of the batched on-chip solves (mi355cg_solve_many*; kernels in onchip_kernels.h).  The device part
// is what onchip_many_workspace_bytes (onchip_plan.h) counts: packed vectors system-major, the small per-system data, one counter.
struct OnchipManyWs {
    int cap = 0;                        // systems it holds
    Buf<double> vec;                    // x of every system, then r, then the direction: 3 x cap x pk_len
    Buf<double> small;                  // update partials (cap x FB_COUNT), diagonals (cap), ||r0||_2 (cap)
    Buf<CgState> s, summary;            // cap each: the iteration-boundary states; what the host reads
    Buf<int> done;                      // systems whose state says done (two words: the copies stay 8-byte)
    Buf<CgState> summary_h;             // pinned copies
    Buf<double> small_h;                // pinned: the layout of `small`
    Buf<int> done_h;
    Buf<double> stage;                  // packed vectors of the host entry points: b, then x (the wave steppers: g, u, v)
    long long stage_cap = 0;            // packed vectors it holds
    // mi355cg_time_steps_many* on top (onchip_steps_workspace_bytes), allocated by the first such call
    int steps_cap = 0;                  // members the next five hold
    Buf<double> step_sigma;             // 1 / (theta tau_s)
    Buf<OcStepBook> book;               // step index and ended flag of every member
    Buf<double> g_one;                  // the handle's right-hand side, packed: the forcing of every member when g = NULL
    Buf<double> step_sigma_h;           // pinned copies; s_h: the iteration-boundary states, read after an interrupted call only
    Buf<OcStepBook> book_h;
    Buf<CgState> s_h;
    Buf<int> step_it;                   // iteration counts, member-major, -1 = step not taken: only when the caller asks for them
    long long step_it_cap = 0;          // counts it holds
    // mi355cg_wave_steps_many* on top (onchip_wave_workspace_bytes): g_one above is shared with the steppers
    int wave_cap = 0;                   // members the next two hold
    Buf<double> wave_tau;               // tau_s of every member, then 2 / tau_s
    Buf<double> wave_tau_h;             // pinned copy
    // mi355cg_wave_record_many* on top (onchip_wave_record_workspace_bytes), allocated by the first such call
    Buf<int> rec_cell;                  // the image cells of kOnchipWaveMaxRec receivers
    Buf<int> rec_cell_h;                // pinned copy
    Buf<double> rec_stage;              // the host entry point: the amplitude tables, then the traces
    long long rec_stage_cap = 0;        // doubles it holds
    // mi355cg_wave_medium_many* on top (onchip_wave_medium_workspace_bytes), allocated by the first such call
    int med_cap = 0;                    // members the next two hold
    Buf<double> med_range;              // the least and the largest entry of every member's medium (k_oc_medium_range)
    Buf<double> med_range_h;            // pinned copy
    // mi355cg_wave_sponge_many* on top (onchip_wave_sponge_workspace_bytes), allocated by the first such call
    int damp_cap = 0;                   // members the next two hold
    Buf<double> damp_range;             // the least and the largest entry of every member's damping row (k_oc_medium_range)
    Buf<double> damp_range_h;           // pinned copy
};

// `small` and its pinned mirror in a call of nsys <= cap systems: nsys x FB_COUNT update partials, then nsys diagonals, then nsys ||r0||_2
struct OnchipSmallView { double* partB; double* diag; double* norm0; };
inline OnchipSmallView onchip_small_view(double* base, int nsys) {
    return OnchipSmallView{base, base + (long long)FB_COUNT * nsys, base + (long long)(FB_COUNT + 1) * nsys};
}

}  // namespace

struct mi355cg_ctx {
    int device = 0;
    int dtype = MI355CG_F64;
    hipStream_t stream = nullptr;
    GridParams gp;
    Geom g{};
    int s_lo = 0, s_hi = 0;             // owned fp64 strips [s_lo, s_hi) (kStripCols columns each); all of them unless 2-D
    long long storage_len = 0;          // elements per vector incl. ghost rows
    long long pk_begin = 0, pk_len = 0; // owned cells in the part's packed order (pk_begin: global packed index of the first; row slabs are contiguous)
    PackGeom pg{};
    // (Plan: item_table.h.  Every plan carries views of its two item tables in device memory: 16 B per item and per wave of its
    // launch.  The handle owns them: plan_items / plan_start below, in the order whole, interior, edge, whole32.)
    Plan whole, interior, edge;         // whole part; rows / strips that need no ghost data; the rest (first + last row, edge strips)
    Plan whole32;                       // fp32 kernels (VEC = 4, 256-column strips): the whole grid, or a row slab of full width
    Buf<ItemDesc> plan_items[4];
    Buf<StartRec> plan_start[4][2];
    int depth = 2;                      // raw rows in flight per wave (env MI355CG_DEPTH: 2 or 3)
    bool has_gc = false;                // 2-D part with a neighbour in x: the stencil launches keep the ghost columns of the direction
    int nB_own = 0;                     // partB slots written by the last update-phase launch(es) of this context
    int strideA = 0, strideB = 0;

    // device vectors in storage layout (fp64 set always; fp32 set for F32_MIXED)
    Buf<double> x, r, p[kRing], ap, b, u;        // (a team part of several: r borrows IPC-pool memory, team.h)
    int xsteps = 4;                     // M: the direction ring has M buffers, x is touched every M-th iteration (env MI355CG_XSTEPS: 2 | 4 | 8)
    Buf<double> scratch[2];             // mi355cg_apply / true residual work space, allocated on first use: never a solver vector
    Buf<float> xf, rf, pf[kRing], apf;  // (a mixed team: rf borrows the memory of r)
    Buf<double> packed;                 // device scratch, pk_len doubles
    Buf<double> partA, partB, partR;
    Buf<double> sumsA, sumsB;           // slab mode: this rank's record = reduced partials [+ its two boundary rows] (feeds the all-gather)
    int rec_width = 0;
    mi355cg_params dist_prm{};                    // slab mode: parameters given to mi355cg_dist_begin
    bool dist_active = false, is_slab = false;
    Buf<CgState> sA, sB, summary;
    Buf<int> qctr;                      // dynamic item queues: kXcds * kQueueSubs counters of the stencil launches, then as many of the update launches (QueueSpec)
    int dyn_rows = 0;                   // > 0: the whole-part launches cut their items this short and deal them through the queues
    Buf<int> stop_h;                    // pinned host word: a stop request, sampled by block 0 of every update launch (msg_solver.cpp:82-87)
    int* stop_dev = nullptr;            // the same word as the device addresses it (nullptr while no solve with a stop flag is running)
    Buf<HistEntry> hist;
    Buf<CgState> summary_h;             // pinned
    Buf<HistEntry> hist_h;              // pinned
    Buf<double> partR_h;                // pinned

    std::vector<double> rhs_h, u_h;     // host copies (owned cells, the part's packed order)
    bool host_rhs_valid = true, host_u_valid = true;     // false after mi355cg_setup_on_device until somebody asks for the host copy
    bool have_u_dev = false, solved = false;
    // Warm start (mi355cg_set_initial_guess*, mi355cg_use_solution_as_initial_guess): the guess lives in x itself.
    bool guess_pending = false;         // the next mi355cg_solve starts from x as it stands (one-shot)
    bool x_is_guess = false;            // x was overwritten by a guess since the last solve: x and r are not a solution and its residual
    Buf<double> guess_part;             // (b, b) partial pairs of k_init_guess (hi, then lo, strideB each), then ||r0||_2 and ||b||_2 (k_guess_state)
    Buf<double> guess_norms_h;          // pinned copy of those two norms
    // Diagonal shift (mi355cg_set_shift): the operator is A - sigma I.  g.A = gp.A - sigma and every multigrid
    // level's diagonal carry it; gp.A stays the Laplacian's.
    double sigma = 0.0;
    int smoother = MI355CG_SMOOTHER_JACOBI;   // as given to mi355cg_set_smoother; kept while there is no hierarchy
    Buf<double> step_b;                 // mi355cg_time_steps: the right-hand side of a step, allocated by the first call
    // generic CSR handle (mi355cg_create_csr): vectors are plain length-n arrays, the operator is this matrix
    bool is_csr = false;
    long long csr_n = 0, csr_nnz = 0;
    Buf<int> csr_row_map, csr_entries; Buf<double> csr_values;
    int grid_csr = 0, grid_update = 0;
    int cur = 0;                        // p[cur] holds the current direction after the last stencil: cur = (iterations done) % xsteps
    int nA_dist = 0;                    // slab mode: stencil partial slots written by the last stencil phase
    // Deferred x fold (k_fold_x; single-context fp64 solves that would otherwise fold x every M-th iteration): a ring of R direction
    // buffers.  Slots 0 .. xsteps-1 are p[], the others are allocated by the first solve that folds (ensure_fold_ring).
    int xfold = 0;                      // R (16 | 32), 0 = the fused update (env MI355CG_XFOLD; unset: by size, see create_impl)
    double* fold_p[kFoldMax] = {};      // the ring's slots: p_k lives in fold_p[k % R]; views of p[] and of fold_own[]
    Buf<double> fold_own[kFoldMax];     // the slots beyond p[] (entries below xsteps stay empty)
    int fold_extra = 0;                 // buffers allocated beyond p[]: 0 until the first solve that folds, then R - xsteps
    Buf<FoldTable> fold_tab;            // device: the slots, and the step lengths of the last R iterations (written by the update launches)
    int fcur = 0;                       // fold mode: (iterations done) % R
    int fold_grid = 0;                  // workgroups of k_fold_x; 0 = one element pair per thread (env MI355CG_XFOLD_GRID)
    bool fold_nt = true;                // nontemporal loads of the once-read directions in k_fold_x (env MI355CG_XFOLD_NT, A/B runs)

    // hipGraph cache for launch-bound (small) grids: one instantiated graph per distinct chunk shape of a solve
    struct ChunkGraph { int m, cur; std::vector<char> flags; hipGraphExec_t exec; };
    std::vector<ChunkGraph> graphs;
    mi355cg_params graph_prm{};          // parameters the cached graphs were captured with
    bool graph_stop = false;            // ... and whether those solves sampled the stop word
    int use_graph = -1;                 // env MI355CG_GRAPH: -1 auto (small grids), 0 off, 1 on
    // On-chip solve mode (mi355cg_set_solve_mode, env MI355CG_ONCHIP): plain fp64 solves without diagnostics run their
    // chunks as one launch of one workgroup (k_onchip) instead of two launches per iteration.
    int solve_mode = MI355CG_SOLVE_LAUNCHES;
    long long onchip_launches = 0;      // on-chip chunk launches of the last mi355cg_solve

    hipEvent_t ev_loop[2] = {nullptr, nullptr};   // brackets the iterations of the last solve (mi355cg_results::loop_seconds)
    std::unique_ptr<MgHier> mg;         // opt-in preconditioner (mi355cg_set_preconditioner): mi355cg_solve runs solve_mg while set
    std::unique_ptr<MgBatchWs> batch;   // workspace of mi355cg_solve_batch*, nullptr until the first batch
    std::unique_ptr<EigWs> eig;         // workspace of mi355cg_eigs*, nullptr until the first eigen solve
    std::unique_ptr<OnchipManyWs> many; // workspace of mi355cg_solve_many*, nullptr until the first such batch
    bool profiling = false;
    EventPool events;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pairs[2];
    double kernel_ms[2] = {0, 0};
    long long kernel_launches[2] = {0, 0};
};

namespace {

// ---- layout ----------------------------------------------------------------------------------------
long long phys_start(const Geom& g, int y) { return row_off(g, y) + (y <= g.half ? g.cb : 0); }
long long phys_end(const Geom& g, int y) { return phys_start(g, y) + (y <= g.half ? g.Pb : g.Pu); }
int strips_total(const GridParams& gp, int vec) { return (gp.n - 1) / (kWave * vec) + 1; }
int first_bottom_strip(const GridParams& gp, int vec) { return (gp.half + 1) / (kWave * vec); }

// first / one-past-last interior column of row y inside the part's strips
void own_cols(const mi355cg_ctx* c, int y, int* xa, int* xb) {
    const int lo = y <= c->gp.half ? c->gp.half + 1 : 1, hi = c->gp.n;       // interior columns [lo, hi)
    *xa = std::max(lo, c->s_lo * kStripCols);
    *xb = std::max(*xa, std::min(hi, c->s_hi * kStripCols));
}

void build_geom(mi355cg_ctx* c, int vec, int y_lo, int y_hi) {
    Geom& g = c->g;
    const GridParams& gp = c->gp;
    g.N = gp.n; g.half = gp.half;
    g.Pu = (int)round_up(g.N + 1, 32);
    g.cb = g.half & ~31;
    g.Pb = g.Pu - g.cb;
    g.xlim = (int)round_up(g.N + 1, vec);
    g.y_lo = y_lo; g.y_hi = y_hi;
    g.base0 = 0;
    g.base0 = phys_start(g, y_lo - 1);
    c->storage_len = phys_end(g, y_hi + 1) - g.base0;
    g.own_begin = phys_start(g, y_lo) - g.base0;
    g.own_len = phys_end(g, y_hi) - phys_start(g, y_lo);
    g.A = gp.A; g.xk = gp.x_k; g.yk = gp.y_k;
    // the part's packed order: its bottom-block rows (each restricted to the own columns), then its upper rows
    PackGeom& pg = c->pg;
    pg.g = g;
    const int yb0 = y_lo, yb1 = std::min(y_hi, gp.half), yu0 = std::max(y_lo, gp.half + 1), yu1 = y_hi;
    int xa = 0, xb = 0;
    pg.nb_rows = std::max(0, yb1 - yb0 + 1); pg.yb0 = yb0;
    own_cols(c, gp.half, &xa, &xb); pg.xb0 = xa; pg.wb = pg.nb_rows ? xb - xa : 0;
    pg.nu_rows = std::max(0, yu1 - yu0 + 1); pg.yu0 = yu0;
    own_cols(c, gp.half + 1, &xa, &xb); pg.xu0 = xa; pg.wu = pg.nu_rows ? xb - xa : 0;
    pg.pk_len = (long long)pg.nb_rows * pg.wb + (long long)pg.nu_rows * pg.wu;
    c->pk_len = pg.pk_len;
    c->pk_begin = packed_row_begin(gp, y_lo);        // meaningful for row slabs (contiguous global range)
}

// Rows [ya, yb] x strips [sa, sb) as up to two rectangles (bottom-right block rows, upper block rows) with their
// ghost-column flags (bit 0: a part to the left, bit 1: a part to the right).
int region_rects(const GridParams& gp, int vec, int ya, int yb, int sa, int sb, Rect out[2]) {
    const int ns_all = strips_total(gp, vec), s0b = first_bottom_strip(gp, vec);
    int nr = 0;
    sb = std::min(sb, ns_all);
    if (ya <= gp.half && yb >= 1) {
        const int s0 = std::max(sa, s0b);
        if (s0 < sb) out[nr++] = Rect{std::max(ya, 1), std::min(yb, gp.half), s0, sb, (sa > s0b ? 1 : 0) | (sb < ns_all ? 2 : 0)};
    }
    if (yb > gp.half && sa < sb)
        out[nr++] = Rect{std::max(ya, gp.half + 1), std::min(yb, gp.n - 1), sa, sb, (sa > 0 ? 1 : 0) | (sb < ns_all ? 2 : 0)};
    return nr;
}

// add_panel, make_plan: item_table.h.  The knobs of a plan as the environment sets them.
PlanKnobs env_knobs() {
    PlanKnobs kn;
    kn.target_waves = env_int("MI355CG_WAVES", 2048); kn.max_blocks = env_int("MI355CG_BLOCKS", 512);
    { const char* v = getenv("MI355CG_ITEM_ROWS"); kn.item_rows = (v && *v) ? std::max(1, atoi(v)) : 0; }
    kn.xcd_classes = env_int("MI355CG_XCD_CLASSES", 1);
    return kn;
}
Plan make_plan(const std::vector<Rect>& rects, int max_rows, int fixed_ty = 0, int dyn_rows = 0) { return make_plan(rects, env_knobs(), max_rows, fixed_ty, dyn_rows); }
constexpr int kMaxRowsF64 = 800, kMaxRowsF32 = 64;

void build_plans(mi355cg_ctx* c) {
    const Geom& g = c->g;
    const GridParams& gp = c->gp;
    Rect rr[2];
    const int nr = region_rects(gp, 2, g.y_lo, g.y_hi, c->s_lo, c->s_hi, rr);
    std::vector<Rect> whole(rr, rr + nr);
    // Static deal (one round of tall items) or run-time item queues (short items, QueueSpec)?  Measured (profiles/r03_tune_notes.md
    // section 5): the queues lose 1.5 % at N = 4096 (49-row items: the balancing gain and the cost of short items cancel) and win
    // +1-3 % at N = 8192, +3-5 % at N = 16384, +5-8 % at N = 32768, where the static items are hundreds of rows tall and the launch
    // tail is whole items.  Default: queues of 16-row items when the static items would be at least 96 rows tall.  MI355CG_DYN_ROWS = 0 | R overrides.
    c->whole = make_plan(whole, kMaxRowsF64);
    c->dyn_rows = std::max(0, env_int("MI355CG_DYN_ROWS", c->whole.ty >= 96 ? 16 : 0));
    if (c->dyn_rows > 0) {
        const Plan dyn = make_plan(whole, kMaxRowsF64, 0, c->dyn_rows);
        if (dyn.wl.ncls == kXcds && dyn.wl.nitems >= 2 * kWaves * dyn.grid) c->whole = dyn; else c->dyn_rows = 0;      // small launches keep the static deal
    }
    c->has_gc = false;
    for (auto& r : whole) if (r.gc) c->has_gc = true;
    // split for halo / compute overlap: `edge` = everything that reads ghost data of r (first and last owned row, the
    // strips beside a ghost column), `interior` = the rest
    std::vector<Rect> inner, rows, cols;
    for (auto& r : whole) {
        const int yi0 = std::max(r.y0, g.y_lo + 1), yi1 = std::min(r.y1, g.y_hi - 1);
        const int si0 = r.s0 + ((r.gc & 1) ? 1 : 0), si1 = r.s1 - ((r.gc & 2) ? 1 : 0);
        if (r.y0 <= g.y_lo && g.y_lo <= r.y1) rows.push_back(Rect{g.y_lo, g.y_lo, r.s0, r.s1, r.gc});
        if (g.y_hi > g.y_lo && r.y0 <= g.y_hi && g.y_hi <= r.y1) rows.push_back(Rect{g.y_hi, g.y_hi, r.s0, r.s1, r.gc});
        if (yi0 > yi1) continue;
        if (si0 < si1) inner.push_back(Rect{yi0, yi1, si0, si1, 0});
        if (si0 >= si1) { cols.push_back(Rect{yi0, yi1, r.s0, r.s1, r.gc}); continue; }     // too narrow to have an interior
        if (r.gc & 1) cols.push_back(Rect{yi0, yi1, r.s0, r.s0 + 1, 1});
        if (r.gc & 2) cols.push_back(Rect{yi0, yi1, r.s1 - 1, r.s1, 2});
    }
    c->interior = make_plan(inner, kMaxRowsF64);
    // edge rows are single-row items; edge strips are cut like the interior
    Plan e_rows = make_plan(rows, kMaxRowsF64, 1), e_cols = make_plan(cols, kMaxRowsF64, c->interior.ty > 0 ? c->interior.ty : 0);
    c->edge = e_rows;
    c->edge.wl.ncls = 1;
    for (int k = 0; k < e_cols.wl.np && c->edge.wl.np < kMaxPanels; ++k) {
        Panel P = e_cols.wl.p[k];
        P.item0 = c->edge.wl.nitems;
        c->edge.wl.p[c->edge.wl.np++] = P;
        c->edge.wl.nitems += P.ns * P.nchunks;
    }
    c->edge.grid = std::max(1, std::min(std::max(1, env_int("MI355CG_BLOCKS", 512)), (c->edge.wl.nitems + kWaves - 1) / kWaves));
    if (c->edge.wl.nitems == 0) c->edge.grid = 0;
    // the fp32 kernels use 256-column strips (float4 per lane) on the same pitches; a 2-D part is cut on 128 columns and has none
    if (c->dtype == MI355CG_F32_MIXED || (c->s_lo == 0 && c->s_hi == strips_total(gp, 2))) {
        Rect r4[2];
        const int n4 = region_rects(gp, 4, g.y_lo, g.y_hi, 0, strips_total(gp, 4), r4);
        c->whole32 = make_plan(std::vector<Rect>(r4, r4 + n4), kMaxRowsF32);
    }
    // rows in flight per wave: 3 measured +1.5 % at N = 4096 and neutral elsewhere (profiles/r02_tune_notes.md section 9); the
    // 12-word update of MI355CG_XSTEPS=8 would need 290 VGPRs at 3 (one wave per SIMD instead of two) and stays at 2
    c->depth = env_int("MI355CG_DEPTH", 3) == 2 ? 2 : 3;
    c->use_graph = env_int("MI355CG_GRAPH", -1);
    c->nB_own = c->whole.grid;
}

// A host array in fresh device memory (blocking copy).  dst is replaced only once the copy is there: a failure leaves it as it was.
template <typename T>
int upload(const std::vector<T>& src, Buf<T>& dst, const char* what = nullptr) {
    Buf<T> fresh;
    if (int rc = Buf<T>::device(fresh, (long long)src.size(), what)) return rc;
    if (hipMemcpy(fresh, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice) != hipSuccess) {
        const hipError_t e = hipGetLastError();
        return what ? fail(MI355CG_ERR_HIP, "%s", what) : fail(MI355CG_ERR_HIP, "upload of %zu bytes failed: %s", sizeof(T) * src.size(), hipGetErrorString(e));
    }
    dst = std::move(fresh);
    return MI355CG_OK;
}

// The item tables of every plan (item_table.h), built and uploaded once, when the handle is created, and owned by the handle.
// No launch and no captured chunk allocates or copies anything for them.
int upload_item_tables(mi355cg_ctx* c) {
    int k = 0;
    for (Plan* pl : {&c->whole, &c->interior, &c->edge, &c->whole32}) {
        const int slot = k++;
        if (pl->wl.nitems == 0 || pl->grid == 0) continue;
        if (int rc = upload(build_item_table(pl->wl), c->plan_items[slot])) return rc;
        pl->d_items = c->plan_items[slot];
        pl->elem = pl == &c->whole32 ? (int)sizeof(float) : (int)sizeof(double);
        for (int rev = 0; rev < 2; ++rev) {      // the start records of the ascending (stencil, apply) and of the reversed descending march (update)
            if (int rc = upload(build_start_table(pl->wl, pl->grid, c->g, pl->elem, rev != 0), c->plan_start[slot][rev])) return rc;
            pl->d_start[rev] = c->plan_start[slot][rev];
        }
    }
    return MI355CG_OK;
}
ItemTab item_tab(const Plan& pl) { return ItemTab{pl.d_items, pl.d_start[0], pl.d_start[1], pl.wl.nitems}; }

int flat_grid(long long n) { return (int)std::max<long long>(1, std::min<long long>(2048, (n + kBlock - 1) / kBlock)); }

// ---- launchers -------------------------------------------------------------------------------------
// Where a consumer kernel finds the partials it reduces in its prologue: the producer kernel's own
// field-major array (estride 1) or partials all-gathered across ranks, rank-major (estride = #fields).
struct PartSrc { const double* ptr; int n, fstride, estride; RecSrc rec; };     // rec.mbox != nullptr (teams): the parts' records instead of partials
// Which items a launch covers, where it runs, and the first partial slot it writes.
struct Where { hipStream_t stream; const Plan* plan; int slot; };

Where whole_part(const mi355cg_ctx* c) { return Where{c->stream, &c->whole, 0}; }
PartSrc own_partB(const mi355cg_ctx* c) { return PartSrc{c->partB, c->nB_own, c->strideB, 1}; }
PartSrc own_partA(const mi355cg_ctx* c) { return PartSrc{c->partA, c->whole.grid, c->strideA, 1}; }

template <typename T, int VEC> Geom kernel_geom(const mi355cg_ctx* c) { Geom g = c->g; g.xlim = (int)round_up(c->g.N + 1, VEC); return g; }

// y = A_h v (plain operator apply on storage-layout vectors)
template <typename T, int VEC>
void launch_apply(const mi355cg_ctx* c, const T* v, T* out, const Where& w) {
    if (w.plan->wl.nitems == 0) return;
    StencilArgs<T> a{};
    a.g = kernel_geom<T, VEC>(c); a.tab = item_tab(*w.plan);
    a.pin = v; a.ap = out; a.partA = nullptr;
    hipLaunchKernelGGL((k_stencil<T, VEC, false, false, 2, false, false, false, false>), dim3(w.plan->grid), dim3(kBlock), 0, w.stream, a);
}

struct IterCfg { RuleParams rp; int want_diag; bool has_u; bool x2 = false; bool fold = false; };     // fold: x2 with the x steps deferred to k_fold_x

// Phase A'.  Does NOT flip c->cur (a part's interior and edge launches share one direction pair).
template <typename T, int VEC>
void launch_iteration_stencil(mi355cg_ctx* c, const IterCfg& cfg, const T* r, const Buf<T> p[kRing], const Where& w, const PartSrc& pb, const FlagSpec* fl = nullptr) {
    if (w.plan->wl.nitems == 0) return;
    StencilArgs<T> a{};
    a.g = kernel_geom<T, VEC>(c); a.tab = item_tab(*w.plan);
    a.r = r; a.pin = p[c->cur]; a.pout = p[(c->cur + 1) % c->xsteps]; a.ap = nullptr;
    a.partB = pb.ptr; a.nB = pb.n; a.strideB = pb.fstride; a.esB = pb.estride; a.src = pb.rec;
    a.partA = c->partA; a.strideA = c->strideA; a.slotA = w.slot;
    a.s_in = c->sB; a.s_out = c->sA; a.hist = c->hist; a.rp = cfg.rp; a.want_diag = cfg.want_diag;
    a.store_ghosts = c->is_slab ? 1 : 0;
    if (fl) a.fl = *fl;
    if (VEC == 2 && c->dyn_rows > 0 && w.plan == &c->whole) a.dq = QueueSpec{c->qctr, c->qctr + kXcds * kQueueSubs * kQueuePitch};
    const dim3 grid(w.plan->grid), block(kBlock);
    const bool msg = cfg.rp.rule == MI355CG_RULE_MSG_MAXNORM, gc = c->has_gc, d3 = c->depth == 3;
    // A team launch (records to gather, flagged partials to store) runs the code with both paths, as ever; a single-context launch
    // gets the instantiation without the team path, and without the queue path unless its items are dealt at run time.
    const bool team = pb.rec.mbox != nullptr || (fl && fl->part), queue = a.dq.mine != nullptr;
#define MI355CG_ST(MSG, D, GC) do { if (team) hipLaunchKernelGGL((k_stencil<T, VEC, true, MSG, D, true, GC, true, VEC == 2>), grid, block, 0, w.stream, a); \
                                    else if (VEC == 2 && queue) hipLaunchKernelGGL((k_stencil<T, VEC, true, MSG, D, true, GC, false, VEC == 2>), grid, block, 0, w.stream, a); \
                                    else hipLaunchKernelGGL((k_stencil<T, VEC, true, MSG, D, true, GC, false, false>), grid, block, 0, w.stream, a); } while (0)
    if constexpr (VEC == 2) {
        if (msg) { if (gc) { if (d3) MI355CG_ST(true, 3, true); else MI355CG_ST(true, 2, true); } else { if (d3) MI355CG_ST(true, 3, false); else MI355CG_ST(true, 2, false); } }
        else     { if (gc) { if (d3) MI355CG_ST(false, 3, true); else MI355CG_ST(false, 2, true); } else { if (d3) MI355CG_ST(false, 3, false); else MI355CG_ST(false, 2, false); } }
    } else {
        if (d3) MI355CG_ST(false, 3, false); else MI355CG_ST(false, 2, false);       // fp32 inner CG: REL_2NORM, single GPU
    }
#undef MI355CG_ST
}

// Phase B on the stencil's work items, marched the other way (it starts on what the stencil launch touched last).
// c->cur was flipped after this iteration's stencil launch: it is the iteration number's parity.
template <typename T, int VEC>
void launch_iteration_update(mi355cg_ctx* c, const IterCfg& cfg, T* x, T* r, const Buf<T> p[kRing], const T* u, const Where& w, const PartSrc& pa, const FlagSpec* fl = nullptr) {
    if (w.plan->wl.nitems == 0) return;
    UpdateStArgs<T> a{};
    a.g = kernel_geom<T, VEC>(c); a.tab = item_tab(*w.plan);
    a.p = p[c->cur]; a.r = r; a.x = x; a.u = u;
    for (int i = 0; i < kRing - 1; ++i) a.pprev[i] = p[(c->cur + 2 * kRing * c->xsteps - 1 - i) % c->xsteps];      // directions of iterations k-1, k-2, ...
    a.partA = pa.ptr; a.nA = pa.n; a.strideA = pa.fstride; a.esA = pa.estride; a.src = pa.rec;
    a.partB = c->partB; a.strideB = c->strideB; a.slotB = w.slot;
    a.s_in = c->sA; a.s_out = c->sB; a.rule = cfg.rp.rule; a.reverse = 1;
    if (fl) a.fl = *fl;
    if (VEC == 2 && c->dyn_rows > 0 && w.plan == &c->whole) a.dq = QueueSpec{c->qctr + kXcds * kQueueSubs * kQueuePitch, c->qctr};
    if (cfg.fold) { a.fold_alpha = reinterpret_cast<double*>(reinterpret_cast<char*>(c->fold_tab.get()) + offsetof(FoldTable, alpha)); a.fold_mask = c->xfold - 1; }
    a.stop_req = w.slot == 0 ? c->stop_dev : nullptr;   // block 0 samples the pinned stop word once per iteration (of a phase in two launches: the one that runs last and owns slot 0)
    const dim3 grid(w.plan->grid), block(kBlock);
    const bool d3 = c->depth == 3 && !(cfg.x2 && c->cur == 0 && c->xsteps == 8);
    const bool team = pa.rec.mbox != nullptr || (fl && fl->part), queue = a.dq.mine != nullptr;      // see launch_iteration_stencil
#define MI355CG_UST_D(XM, HASU, D) do { if (team) hipLaunchKernelGGL((k_update_st<T, VEC, XM, HASU, D, true, true, VEC == 2>), grid, block, 0, w.stream, a); \
                                        else if (VEC == 2 && queue) hipLaunchKernelGGL((k_update_st<T, VEC, XM, HASU, D, true, false, VEC == 2>), grid, block, 0, w.stream, a); \
                                        else hipLaunchKernelGGL((k_update_st<T, VEC, XM, HASU, D, true, false, false>), grid, block, 0, w.stream, a); } while (0)
#define MI355CG_UST(XM, HASU) do { if (d3) MI355CG_UST_D(XM, HASU, 3); else MI355CG_UST_D(XM, HASU, 2); } while (0)
    if (cfg.x2) {                    // iterations k = 0 mod M carry all M x steps (c->cur = k % M)
        if (c->cur != 0 || cfg.fold) MI355CG_UST(0, false); else if (c->xsteps == 8) MI355CG_UST(8, false); else if (c->xsteps == 4) MI355CG_UST(4, false); else MI355CG_UST(2, false);
    }
    else if constexpr (VEC == 2) { if (cfg.has_u) MI355CG_UST(1, true); else MI355CG_UST(1, false); }
#undef MI355CG_UST
#undef MI355CG_UST_D
}

// Flat pass over the owned rows: state initialisation (x = 0, r = b: norms of r0) or the resume step of the mixed path.
template <typename T, int VEC>
void launch_update_flat(mi355cg_ctx* c, const IterCfg& cfg, T* x, T* r, const T* p, const T* ap, const T* u, hipStream_t stream,
                        int grid, double resume_r0norm = -1.0) {
    UpdateArgs<T> a{};
    a.begin = c->g.own_begin / VEC; a.nvec = c->g.own_len / VEC;
    a.x = x; a.r = r; a.p = p; a.ap = ap; a.u = u;
    a.partA = c->partA; a.nA = 0; a.strideA = c->strideA; a.esA = 1;
    a.partB = c->partB; a.strideB = c->strideB;
    a.s_in = c->sA; a.s_out = c->sB; a.rule = cfg.rp.rule; a.init = 1;
    if (resume_r0norm >= 0.0) { a.init = 2; a.r0norm_resume = resume_r0norm; a.s_in = c->sB; }   // measure + re-arm, see k_update
    if (cfg.has_u) hipLaunchKernelGGL((k_update<T, VEC, true>), dim3(grid), dim3(kBlock), 0, stream, a);
    else hipLaunchKernelGGL((k_update<T, VEC, false>), dim3(grid), dim3(kBlock), 0, stream, a);
}

// The x steps of the iterations after the last multiple of M (REL_2NORM folded update), oldest first.
template <typename T, int VEC>
void launch_flush_x(const mi355cg_ctx* c, const Plan& plan, T* x, const Buf<T> p[kRing], const CgState& fin, hipStream_t stream) {
    const int pending = fin.it % c->xsteps;
    if (plan.wl.nitems == 0 || pending == 0) return;
    FlushArgs<T> f{};
    f.n = pending;
    for (int j = 0; j < pending; ++j) { const int k = fin.it - pending + 1 + j; f.p[j] = p[k % c->xsteps]; f.a[j] = (T)fin.alpha_hist[k & (kRing - 1)]; }
    hipLaunchKernelGGL((k_flush_x<T, VEC>), dim3(std::max(1, std::min(1024, (plan.wl.nitems + kWaves - 1) / kWaves))), dim3(kBlock), 0, stream,
                       kernel_geom<T, VEC>(c), item_tab(plan), x, f);
}

// Deferred x fold.  flush_it < 0: after the update launch of an iteration k = 0 mod R, the R steps up to k (unless that launch's
// state says the solve is over); flush_it >= 0: after a loop of flush_it iterations, the flush_it % R steps still pending.
void launch_fold_x(const mi355cg_ctx* c, int flush_it, hipStream_t stream) {
    FoldArgs a{};
    a.begin = c->g.own_begin / 2; a.nvec = c->g.own_len / 2;
    a.x = c->x; a.tab = c->fold_tab; a.s = c->sB; a.mask = c->xfold - 1; a.flush_it = flush_it;
    const long long one_shot = (a.nvec + kBlock - 1) / kBlock;
    const int grid = (int)std::max<long long>(1, c->fold_grid > 0 ? std::min<long long>(c->fold_grid, one_shot) : one_shot);
    if (c->fold_nt) hipLaunchKernelGGL((k_fold_x<true>), dim3(grid), dim3(kBlock), 0, stream, a);
    else hipLaunchKernelGGL((k_fold_x<false>), dim3(grid), dim3(kBlock), 0, stream, a);
}
void free_fold_ring(mi355cg_ctx* c) {
    for (int k = c->xsteps; k < kFoldMax; ++k) { c->fold_own[k].reset(); c->fold_p[k] = nullptr; }
    c->fold_tab.reset();
    c->fold_extra = 0;
}
// The ring of a handle that folds, allocated and zeroed once (pads, boundary and ghost cells of every slot must hold 0, as in p[]).
// If the memory is not there the handle goes back to the fused update for good and stays usable.
bool ensure_fold_ring(mi355cg_ctx* c) {
    if (c->xfold == 0) return false;
    if (c->fold_tab) return true;
    const size_t bytes = sizeof(double) * (size_t)c->storage_len;
    bool ok = true;
    for (int k = 0; k < c->xfold && ok; ++k) {
        if (k < c->xsteps) { c->fold_p[k] = c->p[k]; continue; }
        ok = Buf<double>::device(c->fold_own[k], c->storage_len) == MI355CG_OK && hipMemsetAsync(c->fold_own[k], 0, bytes, c->stream) == hipSuccess;
        c->fold_p[k] = c->fold_own[k];
    }
    FoldTable t{};
    for (int k = 0; k < c->xfold; ++k) t.p[k] = c->fold_p[k];
    ok = ok && Buf<FoldTable>::device(c->fold_tab, 1) == MI355CG_OK &&
         hipMemcpyAsync(c->fold_tab, &t, sizeof t, hipMemcpyHostToDevice, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();                 // the failed allocation is not an error of the solve
        hipStreamSynchronize(c->stream);
        free_fold_ring(c);
        c->xfold = 0;
        return false;
    }
    c->fold_extra = c->xfold - c->xsteps;
    return true;
}

void launch_check(mi355cg_ctx* c, const IterCfg& cfg, hipStream_t stream, const PartSrc& pb) {
    CheckArgs a{};
    a.partB = pb.ptr; a.nB = pb.n; a.strideB = pb.fstride; a.esB = pb.estride; a.src = pb.rec;
    a.s_in = c->sB; a.summary = c->summary; a.hist = c->hist; a.rp = cfg.rp; a.want_diag = cfg.want_diag;
    hipLaunchKernelGGL(k_check, dim3(1), dim3(kBlock), 0, stream, a);
}

// The launch shapes of an iteration: REL_2NORM without diagnostics = x folded every M-th iteration (M = 4: 7.25 words per unknown; on a
// handle with a deferred fold, mi355cg_solve sets cfg.fold: no update launch touches x, k_fold_x does every R-th iteration: 7.0625);
// MSG, and REL_2NORM with the reference's per-iteration diagnostics = x and its norms every iteration (8 words, + u when read).
IterCfg make_cfg(const mi355cg_params* prm) {
    IterCfg cfg{};
    const bool msg = prm->rule == MI355CG_RULE_MSG_MAXNORM;
    cfg.rp.rule = prm->rule; cfg.rp.max_iterations = prm->max_iterations;
    cfg.rp.eps_precision = prm->eps_precision; cfg.rp.eps_residual = prm->eps_residual;
    cfg.rp.eps_exact_error = prm->eps_exact_error; cfg.rp.eps_rel = prm->eps_rel;
    cfg.rp.fixed_iterations = prm->fixed_iterations;
    const bool diag = !msg && prm->diagnostics;
    cfg.has_u = (msg && prm->use_true_solution) || diag;
    cfg.rp.use_u = cfg.has_u ? 1 : 0;
    cfg.want_diag = diag ? 1 : 0;
    cfg.x2 = !msg && !diag;
    return cfg;
}

template <typename T>
int upload_packed(mi355cg_ctx* c, const double* host_packed, T* storage) {
    if (c->is_csr) {                                        // no layout conversion: the caller's order is the storage order
        HIPCK(hipMemcpyAsync(storage, host_packed, sizeof(double) * c->pk_len, hipMemcpyHostToDevice, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        return MI355CG_OK;
    }
    if (c->is_slab) HIPCK(hipDeviceSynchronize());
    if (c->pk_len == 0) return MI355CG_OK;
    HIPCK(hipMemcpyAsync(c->packed, host_packed, sizeof(double) * c->pk_len, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL((k_unpack<T>), dim3(flat_grid(c->pk_len)), dim3(kBlock), 0, c->stream, c->pg, c->packed, storage);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(c->stream));
    return MI355CG_OK;
}
template <typename T>
int download_packed(mi355cg_ctx* c, const T* storage, double* host_packed) {
    if (c->is_csr) {
        HIPCK(hipMemcpyAsync(host_packed, storage, sizeof(double) * c->pk_len, hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        return MI355CG_OK;
    }
    if (c->is_slab) HIPCK(hipDeviceSynchronize());      // part phases run on the caller's / the team's streams
    if (c->pk_len == 0) return MI355CG_OK;
    hipLaunchKernelGGL((k_pack<T>), dim3(flat_grid(c->pk_len)), dim3(kBlock), 0, c->stream, c->pg, storage, c->packed);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(host_packed, c->packed, sizeof(double) * c->pk_len, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return MI355CG_OK;
}

int ensure_host_copies(mi355cg_ctx* c) {        // device-generated problem data: fetch the host copies on first use
    if (!c->host_rhs_valid) { c->rhs_h.resize(c->pk_len); if (int rc = download_packed<double>(c, c->b, c->rhs_h.data())) return rc; c->host_rhs_valid = true; }
    if (!c->host_u_valid) { c->u_h.resize(c->pk_len); if (int rc = download_packed<double>(c, c->u, c->u_h.data())) return rc; c->host_u_valid = true; }
    return MI355CG_OK;
}
// The fp32 vectors of a team's part (mi355cg_team_set_dtype): correction, direction ring and A p.  The fp32 residual is not among
// them: a part keeps it in the memory of its fp64 residual vector (what the neighbours' halo messages are addressed to).
int ensure_f32_vectors(mi355cg_ctx* c) {
    if (c->xsteps > 4) return fail(MI355CG_ERR_INVALID, "MI355CG_XSTEPS=8 is fp64 only");
    if (c->whole32.wl.nitems == 0) return fail(MI355CG_ERR_INVALID, "the fp32 kernels march 256-column strips: a part of a 2-D decomposition (cut on 128 columns) cannot run them; use row slabs");
    if (c->g.own_begin % 4 != 0 || c->g.own_len % 4 != 0) return fail(MI355CG_ERR_STATE, "a part's owned range is not a whole number of float4");
    Buf<float>* fv[] = {&c->xf, &c->apf, &c->pf[0], &c->pf[1], &c->pf[2], &c->pf[3]};
    for (int k = 0; k < 2 + c->xsteps; ++k)
        if (!*fv[k]) if (int rc = Buf<float>::device_zeroed(*fv[k], c->storage_len, "fp32 vector allocation failed")) return rc;
    HIPCK(hipDeviceSynchronize());
    return MI355CG_OK;
}

int ensure_u_on_device(mi355cg_ctx* c) {
    if (c->have_u_dev) return MI355CG_OK;
    if (!c->host_u_valid) return fail(MI355CG_ERR_STATE, "no exact solution on host or device");
    if (int rc = upload_packed<double>(c, c->u_h.data(), c->u)) return rc;
    c->have_u_dev = true;
    return MI355CG_OK;
}
// Work space of mi355cg_apply / mi355cg_get_true_residual.  The reference's apply is const and may be called from an
// iteration callback in the middle of a solve, so it must never borrow a solver vector.
int ensure_scratch(mi355cg_ctx* c) {
    for (auto& s : c->scratch) if (!s) { if (int rc = Buf<double>::device_zeroed(s, c->storage_len)) return rc; }
    HIPCK(hipDeviceSynchronize());      // the zero-fill ran on the NULL stream
    return MI355CG_OK;
}

// Work space of a warm start on the plain path, allocated by the first one: k_init_guess's (b, b) partials and the two norms
// k_guess_state leaves for the host.
int ensure_guess_ws(mi355cg_ctx* c) {
    if (!c->guess_part) if (int rc = Buf<double>::device(c->guess_part, 2 * (long long)c->strideB + 2)) return rc;
    if (!c->guess_norms_h) if (int rc = Buf<double>::pinned(c->guess_norms_h, 2)) return rc;
    return MI355CG_OK;
}

void clear_graphs(mi355cg_ctx* c) {
    for (auto& g : c->graphs) hipGraphExecDestroy(g.exec);
    c->graphs.clear();
}

void prof_begin(mi355cg_ctx* c, hipEvent_t* e0) {
    if (!c->profiling) return;
    *e0 = c->events.get();
    if (*e0) hipEventRecord(*e0, c->stream);
}
void prof_end(mi355cg_ctx* c, int k, hipEvent_t e0) {
    if (!c->profiling || !e0) return;
    hipEvent_t e1 = c->events.get();
    if (!e1) return;
    hipEventRecord(e1, c->stream);
    c->ev_pairs[k].push_back({e0, e1});
}
void prof_collect(mi355cg_ctx* c) {
    for (int k = 0; k < 2; ++k) {
        double tot = 0; long long n = 0;
        for (auto& pr : c->ev_pairs[k]) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { tot += ms; ++n; }
        }
        c->kernel_ms[k] = n ? tot / n : 0.0;
        c->kernel_launches[k] = n;
        c->ev_pairs[k].clear();
    }
    c->events.reset();
}

// The HIP side of solve_loop.h's protocol.  Summary and history ring -> pinned host memory: there once `st` has reached this point.
int fetch_state(mi355cg_ctx* c, hipStream_t st) {
    HIPCK(hipMemcpyAsync(c->summary_h, c->summary, sizeof(CgState), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(c->hist_h, c->hist, sizeof(HistEntry) * kHist, hipMemcpyDeviceToHost, st));
    return MI355CG_OK;
}
// Wait for the context's stream.  With a stop flag the wait polls: the caller's flag lives in ordinary host memory, and while this
// thread waits for a chunk it forwards the flag to the pinned word the kernels sample (mi355cg_solve and mi355cg_solve_many*).
int wait_stream_forwarding_stop(mi355cg_ctx* c, const volatile int* stop_flag) {
    if (!stop_flag) { HIPCK(hipStreamSynchronize(c->stream)); return MI355CG_OK; }
    for (;;) {
        if (*stop_flag) *c->stop_h = 1;
        const hipError_t q = hipStreamQuery(c->stream);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) HIPCK(q);
        std::this_thread::yield();
    }
    return MI355CG_OK;
}
// mi355cg_results::loop_seconds: two events around the iterations.  The caller waits (for the second event or for its stream)
// before it reads the seconds.
int loop_timer_begin(mi355cg_ctx* c, hipStream_t st) {
    if (!c->ev_loop[0]) { HIPCK(hipEventCreate(&c->ev_loop[0])); HIPCK(hipEventCreate(&c->ev_loop[1])); }
    HIPCK(hipEventRecord(c->ev_loop[0], st));
    return MI355CG_OK;
}
int loop_timer_end(mi355cg_ctx* c, hipStream_t st) { HIPCK(hipEventRecord(c->ev_loop[1], st)); return MI355CG_OK; }
double loop_timer_seconds(const mi355cg_ctx* c) {
    float ms = 0;
    return hipEventElapsedTime(&ms, c->ev_loop[0], c->ev_loop[1]) == hipSuccess ? 1e-3 * ms : 0.0;
}

}  // namespace

// ---- generic CSR handles ----------------------------------------------------------------------------------
namespace {

CsrView csr_view(const mi355cg_ctx* c) { return CsrView{c->csr_n, c->csr_row_map, c->csr_entries, c->csr_values}; }

void launch_csr_spmv(mi355cg_ctx* c, const double* x, double* y, const double* r, const CgState* s_in, double* partA) {
    SpmvArgs a{};
    a.A = csr_view(c); a.x = x; a.y = y; a.r = r; a.s_in = s_in; a.partA = partA; a.strideA = c->strideA;
    hipLaunchKernelGGL(k_csr_spmv, dim3(c->grid_csr), dim3(kBlock), 0, c->stream, a);
}

// CG on a caller-supplied matrix: xpay (decision + direction), spmv (+ dots), update.  Same device-side state
// machine, stop rules, callback cadence and result fields as the stencil path.
int solve_csr(mi355cg_ctx* c, const mi355cg_params* prm, mi355cg_iter_cb cb, void* user,
              const volatile int* stop_flag, mi355cg_results* out) {
    if (prm->diagnostics) return fail(MI355CG_ERR_INVALID, "per-iteration diagnostics are not available on CSR handles");
    const bool msg = prm->rule == MI355CG_RULE_MSG_MAXNORM;
    IterCfg cfg = make_cfg(prm);
    if (cfg.has_u && !c->have_u_dev) { cfg.has_u = false; cfg.rp.use_u = 0; }      // no true solution was supplied
    const auto t0 = std::chrono::steady_clock::now();
    const size_t bytes = sizeof(double) * c->storage_len;
    HIPCK(hipMemsetAsync(c->x, 0, bytes, c->stream));
    HIPCK(hipMemsetAsync(c->p[0], 0, bytes, c->stream));
    HIPCK(hipMemsetAsync(c->ap, 0, bytes, c->stream));
    HIPCK(hipMemcpyAsync(c->r, c->b, bytes, hipMemcpyDeviceToDevice, c->stream));
    c->cur = 0;
    const PartSrc pA{c->partA, c->grid_csr, c->strideA, 1};
    auto update = [&](bool init, bool with_u) {
        UpdateArgs<double> a{};
        a.begin = 0; a.nvec = c->csr_n;
        a.x = c->x; a.r = c->r; a.p = c->p[0]; a.ap = c->ap; a.u = c->u;
        a.partA = pA.ptr; a.nA = pA.n; a.strideA = pA.fstride; a.esA = 1;
        a.partB = c->partB; a.strideB = c->strideB;
        a.s_in = c->sA; a.s_out = c->sB; a.rule = cfg.rp.rule; a.init = init ? 1 : 0;
        if (with_u) hipLaunchKernelGGL((k_update<double, 1, true>), dim3(c->grid_update), dim3(kBlock), 0, c->stream, a);
        else hipLaunchKernelGGL((k_update<double, 1, false>), dim3(c->grid_update), dim3(kBlock), 0, c->stream, a);
    };
    update(true, cfg.has_u);
    HIPCK(hipGetLastError());
    auto poll = [&]() -> int {
        launch_check(c, cfg, c->stream, own_partB(c));
        if (int rc = fetch_state(c, c->stream)) return rc;
        HIPCK(hipStreamSynchronize(c->stream));
        return MI355CG_OK;
    };
    if (int rc = poll()) return rc;
    const double initial_rnorm2 = c->summary_h->rnorm2;
    if (msg && cb) cb(user, 0, DBL_MAX, c->summary_h->rmax, cfg.has_u ? c->summary_h->emax : DBL_MAX);
    const int sync_every = default_sync_every(prm, msg);
    int it_done = 0;
    bool first_chunk = (cb != nullptr || stop_flag != nullptr);
    bool interrupted = false;
    while (!c->summary_h->done) {
        if (stop_flag && *stop_flag) { interrupted = true; break; }
        const int m = chunk_len(prm, msg, sync_every, it_done, first_chunk);
        first_chunk = false;
        for (int k = 0; k < m; ++k) {
            XpayArgs xa{};
            xa.n = c->csr_n; xa.r = c->r; xa.p = c->p[0];
            xa.partB = c->partB; xa.nB = c->grid_update; xa.strideB = c->strideB; xa.esB = 1;
            xa.s_in = c->sB; xa.s_out = c->sA; xa.hist = c->hist; xa.rp = cfg.rp; xa.want_diag = 0;
            hipLaunchKernelGGL(k_csr_xpay, dim3(c->grid_update), dim3(kBlock), 0, c->stream, xa);
            launch_csr_spmv(c, c->p[0], c->ap, c->r, c->sA, c->partA);
            update(false, cfg.has_u);
        }
        HIPCK(hipGetLastError());
        if (int rc = poll()) return rc;
        const int it_now = c->summary_h->it;
        replay_callbacks(cb, user, prm, *c->summary_h, c->hist_h, it_done, it_now, cfg.has_u, false);
        it_done = it_now;
    }
    c->solved = true;
    mi355cg_results res = make_results(*c->summary_h, interrupted, cfg.has_u, initial_rnorm2);
    res.solve_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (msg && cb) cb(user, res.iterations, res.final_precision, res.final_residual_norm, res.final_error_norm);
    if (out) *out = res;
    return MI355CG_OK;
}

}  // namespace


// ---- F32_MIXED: fp32 inner CG inside fp64 iterative refinement ------------------------------------
// No reference twin (the reference is fp64 only): the pin is the fp64 TRUE residual of the returned x,
// computed with the bit-exact fp64 operator.  Outer step: d = CG_fp32(A, (float) r) ; x += d ;
// r = b - A x in fp64.  Only the relative 2-norm rule is offered.
namespace {

int poll_summary(mi355cg_ctx* c, const IterCfg& cfg) {
    launch_check(c, cfg, c->stream, own_partB(c));
    HIPCK(hipMemcpyAsync(c->summary_h, c->summary, sizeof(CgState), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return MI355CG_OK;
}

// fp32 CG on (xf, rf): xf = 0 on entry, rf holds the right-hand side and ends as the recursive residual.
// resume_r0norm < 0: fresh start (x = 0, p = 0).  resume_r0norm >= 0: residual replacement -- rf already holds the new true
// residual; keep the direction and the CG scalars, restart only the correction vector xf and the reference norm.
int inner_cg_f32(mi355cg_ctx* c, const IterCfg& cfg, int sync_every, const volatile int* stop_flag, int* its, bool* interrupted,
                 double resume_r0norm = -1.0) {
    const Where w{c->stream, &c->whole32, 0};
    const PartSrc pA{c->partA, c->whole32.grid, c->strideA, 1};
    c->nB_own = c->whole32.grid;
    const size_t bytes = sizeof(float) * c->storage_len;
    HIPCK(hipMemsetAsync(c->xf, 0, bytes, c->stream));
    int done_its = 0;
    if (resume_r0norm < 0.0) {
        for (int k = 0; k < c->xsteps; ++k) HIPCK(hipMemsetAsync(c->pf[k], 0, bytes, c->stream));
        HIPCK(hipMemsetAsync(c->apf, 0, bytes, c->stream));
        c->cur = 0;
        launch_update_flat<float, 4>(c, cfg, c->xf, c->rf, c->pf[0], c->apf, (const float*)nullptr, c->stream, c->whole32.grid);
    } else {
        done_its = c->summary_h->it;
        launch_update_flat<float, 4>(c, cfg, c->xf, c->rf, c->pf[c->cur], c->apf, (const float*)nullptr, c->stream, c->whole32.grid, resume_r0norm);
    }
    HIPCK(hipGetLastError());
    if (int rc = poll_summary(c, cfg)) return rc;
    while (!c->summary_h->done) {
        if (stop_flag && *stop_flag) { *interrupted = true; break; }
        const int m = std::max(1, std::min(sync_every, cfg.rp.max_iterations - done_its));
        for (int k = 0; k < m; ++k) {
            hipEvent_t e0 = nullptr;
            prof_begin(c, &e0);
            launch_iteration_stencil<float, 4>(c, cfg, c->rf, c->pf, w, own_partB(c));
            c->cur = (c->cur + 1) % c->xsteps;
            prof_end(c, 0, e0);
            prof_begin(c, &e0);
            launch_iteration_update<float, 4>(c, cfg, c->xf, c->rf, c->pf, (const float*)nullptr, w, pA);
            prof_end(c, 1, e0);
        }
        HIPCK(hipGetLastError());
        if (int rc = poll_summary(c, cfg)) return rc;
        done_its = c->summary_h->it;
    }
    *its = c->summary_h->it;
    c->cur = *its % c->xsteps;
    launch_flush_x<float, 4>(c, c->whole32, c->xf, c->pf, *c->summary_h, c->stream);      // x steps still pending after the last multiple of M
    HIPCK(hipGetLastError());
    return MI355CG_OK;
}

int solve_mixed(mi355cg_ctx* c, const mi355cg_params* prm, mi355cg_iter_cb cb, void* user,
                const volatile int* stop_flag, mi355cg_results* out) {
    if (prm->rule != MI355CG_RULE_REL_2NORM) return fail(MI355CG_ERR_INVALID, "F32_MIXED offers the REL_2NORM rule only");
    if (c->is_slab) return fail(MI355CG_ERR_INVALID, "F32_MIXED is single-GPU only");
    const auto t0 = std::chrono::steady_clock::now();
    c->events.reset(); c->ev_pairs[0].clear(); c->ev_pairs[1].clear();
    const double inner_eps = prm->inner_eps > 0 ? prm->inner_eps : 1e-4;
    // Restarted refinement is the default.  MI355CG_MIXED_RESTART=0 selects residual replacement (direction and CG scalars
    // kept across outer steps): it saves iterations on small grids but stalled at 2e-5 on N = 8192 in round 1
    // (profiles/r01_tune_notes.md), so it stays experimental and every stage is capped.
    const bool restart = env_int("MI355CG_MIXED_RESTART", 1) != 0;
    int stage_cap = 0;                       // replacement mode: iterations a later stage may spend (3x the first stage)
    const int sync_every = default_sync_every(prm, false);
    const int rgrid = 1024;
    auto residual_pass = [&](double* norm) -> int {      // rf = (float)(b - ap64), *norm = ||b - ap64||_2
        hipLaunchKernelGGL(k_residual_to_f32, dim3(rgrid), dim3(kBlock), 0, c->stream, c->storage_len, c->g.own_begin, c->g.own_len,
                           c->b, c->ap, c->rf, c->partR);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(c->partR_h, c->partR, sizeof(double) * rgrid, hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        double s = 0; for (int i = 0; i < rgrid; ++i) s += c->partR_h[i];
        *norm = std::sqrt(s);
        return MI355CG_OK;
    };
    const size_t bytes64 = sizeof(double) * c->storage_len;
    HIPCK(hipMemsetAsync(c->x, 0, bytes64, c->stream));
    HIPCK(hipMemsetAsync(c->ap, 0, bytes64, c->stream));
    double bnorm = 0, rnorm = 0;
    if (int rc = residual_pass(&bnorm)) return rc;       // x = 0: r = b
    rnorm = bnorm;
    int total = 0, outer = 0;
    bool interrupted = false, converged = bnorm == 0.0;
    while (!converged && total < prm->max_iterations && !interrupted) {
        mi355cg_params ip = *prm;
        ip.eps_rel = inner_eps; ip.diagnostics = 0;
        // restarted refinement: every inner solve starts from scratch with the remaining budget;
        // residual replacement: the iteration counter runs on across outer steps, so the cap is the global one
        ip.max_iterations = restart ? prm->max_iterations - total : prm->max_iterations;
        if (!restart && stage_cap > 0) ip.max_iterations = std::min(ip.max_iterations, total + stage_cap);
        const IterCfg cfg = make_cfg(&ip);
        int its = 0;
        const double resume = (!restart && outer > 0) ? rnorm : -1.0;
        if (int rc = inner_cg_f32(c, cfg, sync_every, stop_flag, &its, &interrupted, resume)) return rc;
        const int its_this = restart ? its : its - total;
        total = restart ? total + its : its; ++outer;
        if (!restart && stage_cap == 0) stage_cap = std::max(2000, 3 * its_this);
        hipLaunchKernelGGL(k_accumulate_f32, dim3(flat_grid(c->g.own_len)), dim3(kBlock), 0, c->stream, c->g.own_begin, c->g.own_len, c->x, c->xf);
        launch_apply<double, 2>(c, c->x, c->ap, whole_part(c));
        const double prev = rnorm;
        if (int rc = residual_pass(&rnorm)) return rc;
        if (cb) cb(user, total, 0.0, rnorm, 0.0);
        converged = !prm->fixed_iterations && rnorm <= prm->eps_rel * bnorm;
        if (prm->fixed_iterations || its_this == 0) break;
        if (!converged && rnorm > 0.5 * prev) break;      // fp32 cannot improve this x any further
    }
    // leave the fp64 residual of the returned x in c->r for mi355cg_get_recursive_residual
    hipLaunchKernelGGL((k_sub<double>), dim3(flat_grid(c->g.own_len)), dim3(kBlock), 0, c->stream, c->g.own_begin, c->g.own_len, c->b, c->ap, c->r);
    HIPCK(hipStreamSynchronize(c->stream));
    c->solved = true; c->cur = 0; c->nB_own = c->whole.grid;
    prof_collect(c);
    mi355cg_results res = make_mixed_results(total, interrupted, converged, rnorm, bnorm, outer);
    res.solve_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (out) *out = res;
    return MI355CG_OK;
}

}  // namespace

// ---- geometric multigrid preconditioner and the preconditioned CG on it (opt-in) -----------------
// Algorithm (fixed; tests/test_mg_cpu.py restates it in NumPy, tests/test_mg_any_cpu.py its non-nested levels):  V(r, l): u = 0,
// two damped-Jacobi sweeps (omega = 0.8), s = r - A_l u restricted, u += P V(R s, l + 1), two more sweeps; the coarsest level
// solves with the dense inverse.  A nested level (N_l = 2 N_{l+1}) uses full weighting and bilinear P, R = P^T / 4; a non-nested
// one the bilinear P between the two grids and R = (N_{l+1} / N_l)^2 P^T.  R proportional to P^T and equal pre- and
// post-smoothers make M symmetric; A is negative definite and so is M, (r, z) < 0.
// PCG (Hestenes-Stiefel, x0 = 0) driven from the host: the scalars of an iteration come back from three short waits (after the
// cycle, after q = A p, after the update), which lets the stop rules, callbacks and stop flag run exactly as in the plain path.
namespace {

constexpr double kMgOmega = 0.8;

// The intervals N_0 = n, N_1, ... of a kind's levels.  MI355CG_PRECOND_MG: N_{l+1} = N_l / 2 while N_l % 4 == 0 and N_l > 32, and
// the coarsest level must have N_L <= 32.  MI355CG_PRECOND_MG_ANY: N_{l+1} = 2 floor(N_l / 4) while N_l > 32, so every even n >= 6
// has one (16 <= N_L <= 32, or N_L = n <= 32); where MG has a hierarchy the two ladders are the same.  Pure host arithmetic.
int mg_shape(int kind, int n, std::vector<int>* ns) {
    if (kind != MI355CG_PRECOND_MG && kind != MI355CG_PRECOND_MG_ANY)
        return fail(MI355CG_ERR_INVALID, "preconditioner kind %d has no multigrid hierarchy (MI355CG_PRECOND_MG = 1, MI355CG_PRECOND_MG_ANY = 2)", kind);
    if (n < 6 || n % 2 != 0) return fail(MI355CG_ERR_INVALID, "grid %d rejected: the L-shaped index map needs an even n >= 6", n);
    ns->assign(1, n);
    int N = n;
    while (N > 32 && (kind == MI355CG_PRECOND_MG_ANY || N % 4 == 0)) { N = 2 * (N / 4); ns->push_back(N); }
    if (N > 32)
        return fail(MI355CG_ERR_INVALID, "grid %d has no multigrid hierarchy: halving stops at N = %d, and the coarsest grid must have "
                    "N <= 32 (a level is halved while N %% 4 == 0 and N > 32)", n, N);
    return MI355CG_OK;
}

// build_geom's storage layout for a whole grid of N intervals (base0 = 0) with the level's 5-point coefficients, the diagonal
// shifted by sigma
Geom mg_geom(int N, double hx, double hy, double sigma, long long* len) {
    Geom g{};
    g.N = N; g.half = N / 2;
    g.Pu = (int)round_up(N + 1, 32); g.cb = g.half & ~31; g.Pb = g.Pu - g.cb;
    g.xlim = (int)round_up(N + 1, 2);
    g.y_lo = 1; g.y_hi = N - 1; g.base0 = 0;
    g.own_begin = phys_start(g, 1); g.own_len = phys_end(g, N - 1) - g.own_begin;
    g.xk = 1 / (hx * hx); g.yk = 1 / (hy * hy);               // grid_system.cpp:316-318 with the level's steps
    g.A = -2 * (g.xk + g.yk) - sigma;                         // the same sigma on every level (mi355cg_set_shift); - 0.0 changes no bit
    *len = phys_end(g, N);
    return g;
}

// Which vectors a level keeps, written once: its right-hand side and its result from level 1 on (level 0's are the caller's), and a
// work vector on every level but the coarsest.  f(level, which, length) allocates one or takes its offset; the first failure ends the walk.
enum MgVecKind { MG_VEC_RHS, MG_VEC_OUT, MG_VEC_A };
template <class F>
int mg_for_level_vectors(const std::vector<MgLevel>& lv, F f) {
    const int nl = (int)lv.size();
    for (int l = 0; l < nl; ++l) {
        if (l > 0) { if (int rc = f(l, MG_VEC_RHS, lv[l].len)) return rc; if (int rc = f(l, MG_VEC_OUT, lv[l].len)) return rc; }
        if (l + 1 < nl) if (int rc = f(l, MG_VEC_A, lv[l].len)) return rc;
    }
    return MI355CG_OK;
}

// A_L^-1 of the coarsest level in its packed unknown order, from the Cholesky factor of -A_L (fp64, host), and the storage
// offset of every unknown.  -A_L = L L^T, T = L^-1 kept transposed (row j = column j of L^-1), -A_L^-1 = T^T T.
void mg_coarse_inverse(const Geom& g, std::vector<double>& inv, std::vector<int>& off) {
    const int N = g.N, W = N + 1;
    std::vector<int> idx((size_t)W * W, -1);
    off.clear();
    for (int y = 1; y <= N - 1; ++y)
        for (int x = (y <= g.half ? g.half + 1 : 1); x <= N - 1; ++x) { idx[(size_t)y * W + x] = (int)off.size(); off.push_back((int)mg_off(g, x, y)); }
    const int n = (int)off.size();
    std::vector<double> S((size_t)n * n, 0.0);
    for (int y = 1; y <= N - 1; ++y)
        for (int x = 1; x <= N - 1; ++x) {
            const int i = idx[(size_t)y * W + x];
            if (i < 0) continue;
            S[(size_t)i * n + i] = -g.A;
            const int nb[4] = {idx[(size_t)y * W + x - 1], idx[(size_t)y * W + x + 1], idx[(size_t)(y - 1) * W + x], idx[(size_t)(y + 1) * W + x]};
            for (int k = 0; k < 4; ++k) if (nb[k] >= 0) S[(size_t)i * n + nb[k]] = k < 2 ? -g.xk : -g.yk;
        }
    for (int j = 0; j < n; ++j) {                              // in place: S's lower triangle becomes L
        double* Sj = &S[(size_t)j * n];
        double d = Sj[j];
        for (int k = 0; k < j; ++k) d -= Sj[k] * Sj[k];
        Sj[j] = std::sqrt(d);
        for (int i = j + 1; i < n; ++i) {
            double* Si = &S[(size_t)i * n];
            double v = Si[j];
            for (int k = 0; k < j; ++k) v -= Si[k] * Sj[k];
            Si[j] = v / Sj[j];
        }
    }
    std::vector<double> T((size_t)n * n, 0.0);               // T[j][i] = (L^-1)[i][j], i >= j
    for (int j = 0; j < n; ++j) {
        double* Tj = &T[(size_t)j * n];
        Tj[j] = 1 / S[(size_t)j * n + j];
        for (int i = j + 1; i < n; ++i) {
            const double* Si = &S[(size_t)i * n];
            double v = 0;
            for (int k = j; k < i; ++k) v += Si[k] * Tj[k];
            Tj[i] = -v / Si[i];
        }
    }
    inv.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {                         // (-A_L)^-1 [i][j] = sum_{k >= i} T[i][k] T[j][k]; exactly symmetric
            const double* Ti = &T[(size_t)i * n];
            const double* Tj = &T[(size_t)j * n];
            double v = 0;
            for (int k = i; k < n; ++k) v += Ti[k] * Tj[k];
            inv[(size_t)i * n + j] = inv[(size_t)j * n + i] = -v;
        }
}

int mg_build32(MgHier* H, const std::vector<double>& inv);

// ---- line smoother (mi355cg_set_smoother; kernels in mg_line_kernels.h) -------------------------------------
// The direction a smoother value means on this handle.  AUTO looks at level 0 alone: the coarser levels keep the ratio of the steps.
int mg_line_direction(const mi355cg_ctx* c, int smoother) {
    if (smoother == MI355CG_SMOOTHER_LINE_X) return MG_LINE_X;
    if (smoother == MI355CG_SMOOTHER_LINE_Y) return MG_LINE_Y;
    if (smoother == MI355CG_SMOOTHER_LINE_AUTO) return c->g.yk > c->g.xk ? MG_LINE_Y : MG_LINE_X;
    return 0;
}

// The Thomas factors of a level's lines (mg_line_kernels.h): tab[i] = inv_i, tab[N + i] = cp_i for 1 <= i <= N - 1
std::vector<double> mg_line_table(const Geom& g, int dir) {
    const double k = dir == MG_LINE_X ? g.xk : g.yk;
    std::vector<double> tab((size_t)2 * g.N, 0.0);
    double cp = 0.0;
    for (int i = 1; i <= g.N - 1; ++i) {
        const double inv = 1.0 / (g.A - k * cp);               // i = 1: A - k * 0 = A
        cp = k * inv;
        tab[i] = inv;
        tab[(size_t)g.N + i] = cp;
    }
    return tab;
}

// The tables of direction dir (dir == 0: none) for every smoothing level of H with the diagonal shifted by sigma, uploaded into
// fresh[level]; H is not touched.
int mg_make_line_tables(const MgHier* H, int dir, double sigma, std::vector<Buf<double>>& fresh) {
    const int nl = (int)H->lv.size();
    fresh = std::vector<Buf<double>>(nl);
    for (int l = 0; dir && l + 1 < nl; ++l) {                      // the coarsest level does not smooth
        Geom g = H->lv[l].g;
        g.A = -2 * (g.xk + g.yk) - sigma;                          // mg_geom's expression
        if (int rc = upload(mg_line_table(g, dir), fresh[l], "line smoother table upload failed")) return rc;
    }
    return MI355CG_OK;
}
// ... and dir becomes H's smoother with them.  The caller has made sure that nothing in flight reads the old tables.
void mg_install_line_tables(MgHier* H, int dir, std::vector<Buf<double>>& fresh) {
    for (size_t l = 0; l < H->lv.size(); ++l) H->lv[l].tab = std::move(fresh[l]);
    H->line_dir = dir;
}
int mg_set_line_tables(MgHier* H, int dir, double sigma) {
    std::vector<Buf<double>> fresh;
    if (int rc = mg_make_line_tables(H, dir, sigma, fresh)) return rc;
    mg_install_line_tables(H, dir, fresh);
    return MI355CG_OK;
}

// The hierarchy is built in a local object: a failure returns and leaves *out as it was, success moves it there.
int mg_build(mi355cg_ctx* c, int kind, std::unique_ptr<MgHier>& out, int cycle = MI355CG_CYCLE_F64) {
    std::vector<int> ns;
    if (int rc = mg_shape(kind, c->gp.n, &ns)) return rc;
    const int nl = (int)ns.size();
    std::unique_ptr<MgHier> H(new MgHier());
    H->kind = kind;
    H->cycle = cycle;
    const bool f64 = cycle == MI355CG_CYCLE_F64;
    H->lv.resize(nl);
    double hx = c->gp.x_step, hy = c->gp.y_step;
    for (int l = 0; l < nl; ++l) {
        MgLevel& L = H->lv[l];
        if (l > 0 && ns[l - 1] == 2 * ns[l]) { hx = std::ldexp(hx, 1); hy = std::ldexp(hy, 1); }   // nested: exactly doubled
        else if (l > 0) { hx = hx * ns[l - 1] / ns[l]; hy = hy * ns[l - 1] / ns[l]; }              // non-nested: same domain
        L.g = mg_geom(ns[l], hx, hy, c->sigma, &L.len);
        L.grid = std::min(L.g.N - 1, kMgMaxGrid);
    }
    if (f64)                                                    // the fp32 cycle has its own vectors (mg_build32)
        if (int rc = mg_for_level_vectors(H->lv, [&](int l, MgVecKind which, long long len) {
                MgLevel& L = H->lv[l];
                return Buf<double>::device_zeroed(which == MG_VEC_RHS ? L.rhs : which == MG_VEC_OUT ? L.out : L.a, len);
            })) return rc;
    const Geom& g0 = H->lv[0].g;
    if (H->lv[0].len != c->storage_len || g0.Pb != c->g.Pb || g0.Pu != c->g.Pu || g0.cb != c->g.cb || c->g.base0 != 0)
        return fail(MI355CG_ERR_STATE, "multigrid level 0 does not match the handle's storage layout");
    for (Buf<double>* v : {&H->z, &H->p[0], &H->p[1], &H->q}) if (int rc = Buf<double>::device_zeroed(*v, c->storage_len)) return rc;
    if (int rc = Buf<double>::device_zeroed(H->part, (long long)MG_NFIELDS * kMgMaxGrid)) return rc;
    if (int rc = Buf<double>::pinned(H->part_h, (long long)MG_NFIELDS * kMgMaxGrid, "pinned partials allocation failed")) return rc;
    std::vector<double> inv;
    std::vector<int> off;
    mg_coarse_inverse(H->lv.back().g, inv, off);
    H->ncoarse = (int)off.size();
    if (H->ncoarse > kMgMaxCoarse) return fail(MI355CG_ERR_STATE, "coarsest grid has %d unknowns (> %d)", H->ncoarse, kMgMaxCoarse);
    if (!f64) { if (int rc = mg_build32(H.get(), inv)) return rc; }
    else if (int rc = upload(inv, H->inv, "coarse inverse upload failed")) return rc;
    if (int rc = upload(off, H->coff, "coarse inverse upload failed")) return rc;
    // the zero-fills ran on the NULL stream; the context's stream does not order with them (see create_state)
    if (hipDeviceSynchronize() != hipSuccess) return fail(MI355CG_ERR_HIP, "hipDeviceSynchronize failed");
    if (f64) if (int rc = mg_set_line_tables(H.get(), mg_line_direction(c, c->smoother), c->sigma)) return rc;   // the smoother set before the hierarchy
    out = std::move(H);
    return MI355CG_OK;
}

// The fp64 V-cycle of a single solve (act == nullptr) or of the active systems of a batch.  The two differ in how a launch goes
// out and in where a level keeps its vectors, and in nothing else:
//   single   k_mg_X on dim3(blocks); the vectors of MgLevel
//   batch    k_mgb_X, whose arguments are k_mg_X's behind act, on dim3(blocks, act->n): a row of blocks per active system; the
//            vectors of system 0 in MgBatchWs (the kernels add a system's stride)
struct MgVecs { double *rhs, *a, *out; };
struct MgCycle {
    mi355cg_ctx* c;
    const MgbAct* act;
    const MgBatchWs* ws = nullptr;      // the systems' vectors if they are not the batch workspace's (the eigensolver's columns)
    template <class... K, class... A>
    void launch(void (*single)(K...), void (*batched)(MgbAct, K...), int blocks, A... args) const {
        if (act) hipLaunchKernelGGL(batched, dim3(blocks, act->n), dim3(kBlock), 0, c->stream, *act, static_cast<K>(args)...);
        else hipLaunchKernelGGL(single, dim3(blocks), dim3(kBlock), 0, c->stream, static_cast<K>(args)...);
    }
    MgVecs vecs(int l) const {                                   // a level has no vector it does not need: nullptr
        if (!act) return {c->mg->lv[l].rhs, c->mg->lv[l].a, c->mg->lv[l].out};
        const MgBatchWs& W = ws ? *ws : *c->batch;
        auto at = [&](long long off) { return off < 0 ? nullptr : W.base + off; };
        return {at(W.lv[l].rhs), at(W.lv[l].a), at(W.lv[l].out)};
    }
};

// One sweep of the hierarchy's smoother on level L: t = S(rhs, u).  first: u = 0.  dot != nullptr: + the partials of (rhs, t), one per
// block of L.grid.  Point Jacobi goes out exactly as before there was a choice.
template <int DIR>
void mg_line_sweep(const MgCycle& cy, const MgLevel& L, bool first, const double* rhs, const double* u, double* t, double* dot) {
    const int blocks = mg_line_blocks(L.g.N);
    const double* tab = L.tab;
    if (dot) cy.launch(k_mg_line<DIR, false, true>, k_mgb_line<DIR, false, true>, L.grid, L.g, kMgOmega, tab, rhs, u, t, dot);
    else if (first) cy.launch(k_mg_line<DIR, true, false>, k_mgb_line<DIR, true, false>, blocks, L.g, kMgOmega, tab, rhs, nullptr, t, nullptr);
    else cy.launch(k_mg_line<DIR, false, false>, k_mgb_line<DIR, false, false>, blocks, L.g, kMgOmega, tab, rhs, u, t, nullptr);
}
void mg_sweep(const MgCycle& cy, const MgLevel& L, bool first, const double* rhs, const double* u, double* t, double* dot) {
    const int dir = cy.c->mg->line_dir;
    if (dir == MG_LINE_X) return mg_line_sweep<MG_LINE_X>(cy, L, first, rhs, u, t, dot);
    if (dir == MG_LINE_Y) return mg_line_sweep<MG_LINE_Y>(cy, L, first, rhs, u, t, dot);
    if (dot) cy.launch(k_mg_smooth<false, true>, k_mgb_smooth<false, true>, L.grid, L.g, kMgOmega, rhs, u, t, dot);
    else if (first) cy.launch(k_mg_smooth<true, false>, k_mgb_smooth<true, false>, L.grid, L.g, kMgOmega, rhs, nullptr, t, nullptr);
    else cy.launch(k_mg_smooth<false, false>, k_mgb_smooth<false, false>, L.grid, L.g, kMgOmega, rhs, u, t, nullptr);
}

// out = V(rhs, l) on level l's vectors.  dot != nullptr (level 0): the last launch also leaves the partials of (rhs, out) there.
void mg_vcycle(const MgCycle& cy, int l, const double* rhs, double* out, double* dot) {
    const MgHier& H = *cy.c->mg;
    const MgLevel& L = H.lv[l];
    if (l + 1 == (int)H.lv.size()) {                             // k_mgb_coarse walks the active list itself: one row of blocks
        const dim3 grid(H.ncoarse), blk(kBlock);
        if (cy.act) hipLaunchKernelGGL(k_mgb_coarse, grid, blk, 0, cy.c->stream, *cy.act, H.ncoarse, (const double*)H.inv, (const int*)H.coff, rhs, out);
        else hipLaunchKernelGGL(k_mg_coarse, grid, blk, 0, cy.c->stream, H.ncoarse, (const double*)H.inv, (const int*)H.coff, rhs, out);
        if (dot) cy.launch(k_mg_dot, k_mgb_dot, L.grid, L.g, rhs, out, dot);
        return;
    }
    const MgLevel& C = H.lv[l + 1];
    double* const a = cy.vecs(l).a;
    const MgVecs cv = cy.vecs(l + 1);
    const bool nested = L.g.N == 2 * C.g.N;
    mg_sweep(cy, L, true, rhs, nullptr, a, nullptr);
    mg_sweep(cy, L, false, rhs, a, out, nullptr);
    if (nested) {
        cy.launch(k_mg_restrict, k_mgb_restrict, C.grid, L.g, C.g, rhs, out, cv.rhs);
    } else {                            // a is free until the first post-sweep: it holds s = rhs - A out for the gather
        const double scale = (double)((long long)C.g.N * C.g.N) / (double)((long long)L.g.N * L.g.N);
        cy.launch(k_mg_residual, k_mgb_residual, L.grid, L.g, rhs, out, a);
        cy.launch(k_mg_restrict_nn, k_mgb_restrict_nn, C.grid, L.g, C.g, scale, a, cv.rhs);
    }
    mg_vcycle(cy, l + 1, cv.rhs, cv.out, nullptr);
    if (nested) cy.launch(k_mg_prolong, k_mgb_prolong, L.grid, L.g, C.g, cv.out, out);
    else cy.launch(k_mg_prolong_nn, k_mgb_prolong_nn, L.grid, L.g, C.g, cv.out, out);
    mg_sweep(cy, L, false, rhs, out, a, nullptr);
    mg_sweep(cy, L, false, rhs, a, out, dot);
}

// ---- the fp32 V-cycle (MI355CG_CYCLE_F32; kernels in mg_kernels_f32.h) -----------------------------------
constexpr int kMg32VecMinN = 256;       // levels with at least this many intervals take 4 columns per lane (a row fills a wave)

// fp32 vectors and constants of every level and the coarse inverse rounded to fp32
int mg_build32(MgHier* H, const std::vector<double>& inv) {
    const int nl = (int)H->lv.size();
    H->lv32.resize(nl);
    for (int l = 0; l < nl; ++l) {
        const MgLevel& L = H->lv[l];
        MgLevel32& F = H->lv32[l];
        F.c = MgCoef32{(float)L.g.A, (float)L.g.xk, (float)L.g.yk, (float)kMgOmega};
        F.vec = L.g.N >= kMg32VecMinN ? 4 : 1;
        if (l + 1 < nl) {
            const Geom& C = H->lv[l + 1].g;
            F.scale = (float)((double)((long long)C.N * C.N) / (double)((long long)L.g.N * L.g.N));
        }
        for (Buf<float>* v : {&F.rhs, &F.out}) if (int rc = Buf<float>::device_zeroed(*v, L.len)) return rc;
        if (l + 1 < nl) if (int rc = Buf<float>::device_zeroed(F.a, L.len)) return rc;
    }
    return upload(std::vector<float>(inv.begin(), inv.end()), H->inv32);
}

// levels l >= 1: out = V(rhs, l) on the level's fp32 vectors
void mg_vcycle32_level(mi355cg_ctx* c, int l);

// the part of a level between its two pre-sweeps and its two post-sweeps: residual, restriction, the coarser cycle, prolongation
template <int V>
void mg_vcycle32_coarse_part(mi355cg_ctx* c, int l) {
    const MgHier& H = *c->mg;
    const MgLevel &L = H.lv[l], &C = H.lv[l + 1];
    const MgLevel32 &F = H.lv32[l], &G = H.lv32[l + 1];
    const hipStream_t st = c->stream;
    const dim3 grid(L.grid), blk(kBlock);
    const bool nested = L.g.N == 2 * C.g.N;
    if (nested) {
        if (G.vec == 4) hipLaunchKernelGGL((k_mg32_restrict<4>), dim3(C.grid), blk, 0, st, L.g, C.g, F.c, (const float*)F.rhs, (const float*)F.out, G.rhs);
        else hipLaunchKernelGGL((k_mg32_restrict<1>), dim3(C.grid), blk, 0, st, L.g, C.g, F.c, (const float*)F.rhs, (const float*)F.out, G.rhs);
    } else {                            // F.a is free until the first post-sweep: it holds s = rhs - A out for the gather
        hipLaunchKernelGGL((k_mg32_residual<V>), grid, blk, 0, st, L.g, F.c, (const float*)F.rhs, (const float*)F.out, F.a);
        hipLaunchKernelGGL(k_mg32_restrict_nn, dim3(C.grid), blk, 0, st, L.g, C.g, F.scale, (const float*)F.a, G.rhs);
    }
    mg_vcycle32_level(c, l + 1);
    if (nested) hipLaunchKernelGGL((k_mg32_prolong<V>), grid, blk, 0, st, L.g, C.g, (const float*)G.out, F.out);
    else hipLaunchKernelGGL(k_mg32_prolong_nn, grid, blk, 0, st, L.g, C.g, (const float*)G.out, F.out);
}

template <int V>
void mg_vcycle32_sweeps(mi355cg_ctx* c, int l, int e, const double* r64, double* z64) {
    const MgHier& H = *c->mg;
    const MgLevel& L = H.lv[l];
    const MgLevel32& F = H.lv32[l];
    const hipStream_t st = c->stream;
    const dim3 grid(L.grid), blk(kBlock);
    const float* nf = nullptr;
    float* nfw = nullptr;
    double* nd = nullptr;
    if (l == 0) hipLaunchKernelGGL((k_mg32_smooth<V, 1>), grid, blk, 0, st, L.g, F.c, e, r64, nf, F.rhs, nf, F.a, nd, nd);
    else hipLaunchKernelGGL((k_mg32_smooth<V, 0>), grid, blk, 0, st, L.g, F.c, 0, (const double*)nd, (const float*)F.rhs, nfw, nf, F.a, nd, nd);
    hipLaunchKernelGGL((k_mg32_smooth<V, 2>), grid, blk, 0, st, L.g, F.c, 0, (const double*)nd, (const float*)F.rhs, nfw, (const float*)F.a, F.out, nd, nd);
    mg_vcycle32_coarse_part<V>(c, l);
    hipLaunchKernelGGL((k_mg32_smooth<V, 2>), grid, blk, 0, st, L.g, F.c, 0, (const double*)nd, (const float*)F.rhs, nfw, (const float*)F.out, F.a, nd, nd);
    if (l == 0) hipLaunchKernelGGL((k_mg32_smooth<V, 3>), grid, blk, 0, st, L.g, F.c, e, r64, nf, nfw, (const float*)F.a, nfw, z64, H.part);
    else hipLaunchKernelGGL((k_mg32_smooth<V, 2>), grid, blk, 0, st, L.g, F.c, 0, (const double*)nd, (const float*)F.rhs, nfw, (const float*)F.a, F.out, nd, nd);
}

void mg_vcycle32_level(mi355cg_ctx* c, int l) {
    const MgHier& H = *c->mg;
    if (l + 1 == (int)H.lv.size()) {
        hipLaunchKernelGGL(k_mg32_coarse, dim3(H.ncoarse), dim3(kBlock), 0, c->stream, H.ncoarse, (const float*)H.inv32, (const int*)H.coff,
                           (const float*)H.lv32[l].rhs, H.lv32[l].out);
        return;
    }
    if (H.lv32[l].vec == 4) mg_vcycle32_sweeps<4>(c, l, 0, nullptr, nullptr);
    else mg_vcycle32_sweeps<1>(c, l, 0, nullptr, nullptr);
}

// z = M32 r on level 0 and the partials of (r, z) in H.part; rmax = max|r| (the scale 2^e is its binary exponent)
int mg_apply32(mi355cg_ctx* c, const double* r, double* z, double rmax) {
    const MgHier& H = *c->mg;
    const MgLevel& L = H.lv[0];
    const hipStream_t st = c->stream;
    const dim3 grid(L.grid), blk(kBlock);
    if (!(rmax > 0)) {                                            // r = 0: z = 0 and (r, z) = 0
        HIPCK(hipMemsetAsync(z, 0, sizeof(double) * L.len, st));
        HIPCK(hipMemsetAsync(H.part, 0, sizeof(double) * L.grid, st));
        return MI355CG_OK;
    }
    int e = 0;
    if (std::isfinite(rmax)) std::frexp(rmax, &e);
    if (H.lv.size() == 1) {
        hipLaunchKernelGGL(k_mg32_cast, grid, blk, 0, st, L.g, e, r, H.lv32[0].rhs);
        mg_vcycle32_level(c, 0);
        hipLaunchKernelGGL(k_mg32_uncast_dot, grid, blk, 0, st, L.g, e, r, (const float*)H.lv32[0].out, z, H.part);
    } else if (H.lv32[0].vec == 4) {
        mg_vcycle32_sweeps<4>(c, 0, e, r, z);
    } else {
        mg_vcycle32_sweeps<1>(c, 0, e, r, z);
    }
    return MI355CG_OK;
}

// PCG with z = M r.  Same stop rules, callback cadence, stop-flag handling and result fields as mi355cg_solve's plain path.
// warm: x holds an initial guess (mi355cg_set_initial_guess*): r0 = b - A x0 with the plain operator's bits, REL_2NORM tests against ||b||_2.
int solve_mg(mi355cg_ctx* c, const mi355cg_params* prm, mi355cg_iter_cb cb, void* user,
             const volatile int* stop_flag, mi355cg_results* out, bool warm) {
    MgHier& H = *c->mg;
    const Geom& g = H.lv[0].g;
    const bool msg = prm->rule == MI355CG_RULE_MSG_MAXNORM;
    const bool diag = !msg && prm->diagnostics;
    const bool has_u = (msg && prm->use_true_solution) || diag;
    if (has_u) if (int rc = ensure_u_on_device(c)) return rc;
    if (warm && !(c->scratch[0] && c->scratch[1])) if (int rc = ensure_scratch(c)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const hipStream_t st = c->stream;
    const int G = H.lv[0].grid;
    const dim3 grid(G), blk(kBlock);
    const size_t bytes = sizeof(double) * c->storage_len;
    // partials of the last launch -> host, summed (maxed) in block order: the fixed reduction order
    auto fetch = [&](int nfields, double* v) -> int {
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(H.part_h, H.part, sizeof(double) * nfields * G, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        for (int f = 0; f < nfields; ++f) {
            double s = 0;
            for (int b = 0; b < G; ++b) s = f < MG_RMAX ? s + H.part_h[f * G + b] : std::max(s, H.part_h[f * G + b]);
            v[f] = s;
        }
        return MI355CG_OK;
    };
    double nm[MG_NFIELDS];
    auto update = [&](double alpha, const double* p, const double* q) -> int {
        hipLaunchKernelGGL(k_mg_update, grid, blk, 0, st, g, alpha, c->x, c->r, p, q, has_u ? (const double*)c->u : (const double*)nullptr, H.part);
        return fetch(MG_NFIELDS, nm);
    };
    // x = 0, r = b (msg_solver.cpp:33-39); a zero step gives the norms of r0 and of x0 - u.  Warm: x stays, r = b - A x with the plain
    // operator (mg_Av groups the neighbours first and is not bit-identical to it), and (b, b) by k_mg_dot, whose sums run in the
    // order of the zero step's (r, r): with x0 = 0 both norms are the cold start's.
    double bb = 0.0;
    HIPCK(hipMemsetAsync(H.q, 0, bytes, st));
    if (warm) {
        launch_apply<double, 2>(c, c->x, c->scratch[0], whole_part(c));
        hipLaunchKernelGGL((k_sub<double>), dim3(flat_grid(c->g.own_len)), blk, 0, st, c->g.own_begin, c->g.own_len, (const double*)c->b, (const double*)c->scratch[0], c->r);
        hipLaunchKernelGGL(k_mg_dot, grid, blk, 0, st, g, (const double*)c->b, (const double*)c->b, H.part);
        if (int rc = fetch(1, &bb)) return rc;
    } else {
        HIPCK(hipMemsetAsync(c->x, 0, bytes, st));
        HIPCK(hipMemcpyAsync(c->r, c->b, bytes, hipMemcpyDeviceToDevice, st));
    }
    if (int rc = update(0.0, H.q, H.q)) return rc;
    const double r0norm = std::sqrt(nm[MG_RR]);
    const double refnorm = warm ? std::sqrt(bb) : r0norm;      // what REL_2NORM is relative to: ||b||_2
    double rnorm = r0norm;
    if (int rc = loop_timer_begin(c, st)) return rc;
    if (msg && cb) cb(user, 0, DBL_MAX, nm[MG_RMAX], has_u ? nm[MG_EMAX] : DBL_MAX);          // msg_solver.cpp:75-77
    const int every = prm->callback_every;
    int it = 0;
    // r0 of a guess may be 0 (alpha = 0 / 0): a warm solve applies the stop tests that have their numbers to the start state
    int reason = warm ? msg_stop_reason(prm, false, 0.0, nm[MG_RMAX], has_u, nm[MG_EMAX]) : 0;
    bool converged = reason != 0, interrupted = false;
    double rho = 0.0;
    for (;;) {
        if (converged) break;                                                                 // a warm start that already meets the rule
        if (!(it < prm->max_iterations)) break;                                               // msg_solver.cpp:80
        if (!msg && !prm->fixed_iterations && !(rnorm > prm->eps_rel * refnorm)) break;       // matrix_free_system.cpp:409
        if (stop_flag && *stop_flag) { interrupted = true; break; }                           // msg_solver.cpp:82-87
        double rz = 0, pq = 0;
        if (H.cycle == MI355CG_CYCLE_F32) { if (int rc = mg_apply32(c, c->r, H.z, nm[MG_RMAX])) return rc; }   // nm: of the last update
        else
        mg_vcycle(MgCycle{c, nullptr}, 0, c->r, H.z, H.part);                                // z = M r, partials of (r, z)
        if (int rc = fetch(1, &rz)) return rc;
        const double beta = it == 0 ? 0.0 : rz / rho;
        rho = rz;
        double* p = H.p[it & 1];
        if (it == 0) hipLaunchKernelGGL((k_mg_dir_apply<true>), grid, blk, 0, st, g, 0.0, (const double*)H.z, (const double*)nullptr, p, H.q, H.part);
        else hipLaunchKernelGGL((k_mg_dir_apply<false>), grid, blk, 0, st, g, beta, (const double*)H.z, (const double*)H.p[(it + 1) & 1], p, H.q, H.part);
        if (int rc = fetch(1, &pq)) return rc;
        if (int rc = update(rho / pq, p, H.q)) return rc;
        ++it;
        rnorm = std::sqrt(nm[MG_RR]);
        reason = msg_stop_reason(prm, true, nm[MG_DMAX], nm[MG_RMAX], has_u, nm[MG_EMAX]);
        if (reason) { converged = true; break; }
        if (diag && cb) {                                                                     // matrix_free_system.cpp:457-468 (0-based index)
            double tr2 = 0;
            hipLaunchKernelGGL(k_mg_resid2, grid, blk, 0, st, g, (const double*)c->b, (const double*)c->x, H.part);
            if (int rc = fetch(1, &tr2)) return rc;
            cb(user, it - 1, std::sqrt(nm[MG_D2]), std::sqrt(tr2), std::sqrt(nm[MG_E2]));
        } else if (msg && cb && (it == 1 || (every > 0 && it % every == 0))) {               // msg_solver.cpp:172-183
            cb(user, it, nm[MG_DMAX], nm[MG_RMAX], has_u ? nm[MG_EMAX] : DBL_MAX);
        }
    }
    if (int rc = loop_timer_end(c, st)) return rc;
    if (!msg) converged = rnorm <= prm->eps_rel * refnorm;                                    // matrix_free_system.cpp:472
    c->solved = true; c->x_is_guess = false;
    c->kernel_ms[0] = c->kernel_ms[1] = 0.0; c->kernel_launches[0] = c->kernel_launches[1] = 0;   // per-kernel times: plain path only
    mi355cg_results res = make_results(it, interrupted, converged ? 1 : 0, reason, nm[MG_DMAX], nm[MG_RMAX], has_u, nm[MG_EMAX], rnorm, r0norm);
    res.solve_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    HIPCK(hipEventSynchronize(c->ev_loop[1]));
    res.loop_seconds = loop_timer_seconds(c);
    if (msg && cb) cb(user, res.iterations, res.final_precision, res.final_residual_norm, res.final_error_norm);   // msg_solver.cpp:193-195
    if (out) *out = res;
    return MI355CG_OK;
}

// ---- batched PCG (mi355cg_solve_batch*; kernels in mg_batch_kernels.h) ------------------------------------
void mg_batch_free(mi355cg_ctx* c) {
    if (!c->batch) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    c->batch.reset();
}
void onchip_many_free(mi355cg_ctx* c) {                            // the workspace of mi355cg_solve_many*
    if (!c->many) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    c->many.reset();
}

// Vectors for nsys systems of the handle's hierarchy (and, stage_sys > 0, the host entry point's packed staging).  A workspace
// that is large enough is kept; a larger one replaces it only once it is complete, so a failure leaves the handle as it was.
int mg_batch_ensure(mi355cg_ctx* c, int nsys, int stage_sys) {
    const MgHier& H = *c->mg;
    if (!c->batch || c->batch->cap < nsys) {
        std::unique_ptr<MgBatchWs> W(new MgBatchWs());
        auto failed = [&](const char* what) { return fail(MI355CG_ERR_HIP, "batch workspace for %d systems: %s allocation failed", nsys, what); };
        long long off = 0;
        auto take = [&](long long len) { const long long o = off; off += round_up(len, 32); return o; };
        const long long len0 = H.lv[0].len;
        W->x = take(len0); W->r = take(len0); W->z = take(len0); W->p[0] = take(len0); W->p[1] = take(len0); W->q = take(len0);
        W->lv.resize(H.lv.size());
        mg_for_level_vectors(H.lv, [&](int l, MgVecKind which, long long len) {
            (which == MG_VEC_RHS ? W->lv[l].rhs : which == MG_VEC_OUT ? W->lv[l].out : W->lv[l].a) = take(len);
            return MI355CG_OK;
        });
        W->stride = off;
        W->cap = nsys;
        const int G = H.lv[0].grid;
        if (Buf<double>::device(W->base, W->stride * nsys)) return failed("vector");
        constexpr int kFields = MGBG_NFIELDS > MGB_NFIELDS ? MGBG_NFIELDS : MGB_NFIELDS;      // the warm start's launch has one field more
        if (Buf<double>::device(W->part, (long long)kFields * G * nsys)) return failed("partials");
        if (Buf<double>::device(W->red, (long long)kFields * kMgBatchMax)) return failed("sums");
        if (Buf<double>::pinned(W->red_h, (long long)kFields * kMgBatchMax)) return failed("pinned sums");
        // boundary nodes and pads hold 0 for good: the kernels write interior nodes only
        if (hipMemsetAsync(W->base, 0, sizeof(double) * W->stride * nsys, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); return failed("zero-filled vector"); }
        if (c->batch) { W->stage = std::move(c->batch->stage); W->stage_cap = c->batch->stage_cap; }
        mg_batch_free(c);
        c->batch = std::move(W);
    }
    MgBatchWs* W = c->batch.get();
    if (stage_sys > W->stage_cap) {
        HIPCK(hipStreamSynchronize(c->stream));                    // nothing in flight reads the buffer that is replaced
        if (Buf<double>::device(W->stage, (long long)c->pk_len * stage_sys))
            return fail(MI355CG_ERR_HIP, "batch staging for %d packed vectors: allocation failed", stage_sys);
        W->stage_cap = stage_sys;
    }
    return MI355CG_OK;
}

// solve_mg for nrhs systems at once.  b_dev, x_dev: packed vectors in device memory (they may be the same buffer: b is consumed
// before x is written).  Every system runs solve_mg's tests on its own numbers in solve_mg's order; one that stops leaves the
// active list and no later launch touches its vectors.  Three host waits per iteration, as there.
// warm (mi355cg_solve_batch*_from): x_dev holds nrhs guesses on entry; system s starts as the single warm solve starts.
int solve_mg_batch(mi355cg_ctx* c, const mi355cg_params* prm, int nrhs, const double* b_dev, double* x_dev,
                   const volatile int* stop_flag, mi355cg_results* out, bool warm = false) {
    const MgHier& H = *c->mg;
    const MgBatchWs& W = *c->batch;
    const Geom& g = H.lv[0].g;
    const bool msg = prm->rule == MI355CG_RULE_MSG_MAXNORM;
    const auto t0 = std::chrono::steady_clock::now();
    const hipStream_t st = c->stream;
    const int G = H.lv[0].grid;
    const dim3 blk(kBlock);
    double* const B = W.base;
    MgbAct act{};
    act.stride = W.stride;
    // the last launch's partials summed on the device in block order, act.n * nfields sums -> host
    auto fetch = [&](int nfields, int first_max) -> int {
        hipLaunchKernelGGL(k_mgb_reduce, dim3(nfields, act.n), dim3(kWave), 0, st, act, nfields, first_max, G, (const double*)W.part, W.red);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(W.red_h, W.red, sizeof(double) * nfields * act.n, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        return MI355CG_OK;
    };
    struct Sys { double rr, rmax, dmax, rho, rnorm, r0norm, refnorm; int it, reason; bool converged, interrupted; };      // refnorm: ||b||_2
    std::vector<Sys> S(nrhs);
    auto take_norms = [&]() {
        for (int k = 0; k < act.n; ++k) {
            Sys& s = S[act.sys[k]];
            s.rr = W.red_h[k * MGB_NFIELDS + MGB_RR]; s.rmax = W.red_h[k * MGB_NFIELDS + MGB_RMAX]; s.dmax = W.red_h[k * MGB_NFIELDS + MGB_DMAX];
        }
    };
    act.n = nrhs;
    for (int s = 0; s < nrhs; ++s) act.sys[s] = s;
    // r = b, x = 0 and the norms of r0 (msg_solver.cpp:33-39)
    hipLaunchKernelGGL(k_mgb_unpack, dim3(flat_grid(c->pk_len), nrhs), blk, 0, st, c->pg, W.stride, b_dev, B + W.r);
    if (warm) {                                                    // x = x0, r = b - A x0, and (b, b) beside the norms of r0
        hipLaunchKernelGGL(k_mgb_unpack, dim3(flat_grid(c->pk_len), nrhs), blk, 0, st, c->pg, W.stride, (const double*)x_dev, B + W.x);
        hipLaunchKernelGGL(k_mgb_init_guess, dim3(G, nrhs), blk, 0, st, act, g, (const double*)(B + W.x), B + W.r, W.part);
        if (int rc = fetch(MGBG_NFIELDS, MGBG_RMAX)) return rc;
        for (int k = 0; k < nrhs; ++k) {
            Sys& s = S[k];
            const double* v = W.red_h + k * MGBG_NFIELDS;
            s.rr = v[MGBG_RR]; s.rmax = v[MGBG_RMAX]; s.dmax = v[MGBG_DMAX]; s.refnorm = std::sqrt(v[MGBG_BB]);
        }
    } else {
        hipLaunchKernelGGL(k_mgb_init, dim3(G, nrhs), blk, 0, st, act, g, B + W.x, (const double*)(B + W.r), W.part);
        if (int rc = fetch(MGB_NFIELDS, MGB_RMAX)) return rc;
        take_norms();
    }
    for (Sys& s : S) {
        s.r0norm = s.rnorm = std::sqrt(s.rr);
        if (!warm) s.refnorm = s.r0norm;
        s.rho = 0.0; s.it = 0; s.reason = MI355CG_STOP_ITERATIONS; s.converged = false; s.interrupted = false;
    }
    if (int rc = loop_timer_begin(c, st)) return rc;
    MgbScal sc{};
    for (int it = 0;; ++it) {
        int n = 0;
        for (int k = 0; k < act.n; ++k) {                          // the tests before an iteration, per system (solve_mg's order)
            Sys& s = S[act.sys[k]];
            if (warm && it == 0) {                                 // solve_mg's test of a warm start state
                s.reason = msg_stop_reason(prm, false, 0.0, s.rmax, false, 0.0);
                if (s.reason) { s.converged = true; continue; }
            }
            if (!(it < prm->max_iterations)) continue;
            if (!msg && !prm->fixed_iterations && !(s.rnorm > prm->eps_rel * s.refnorm)) continue;
            act.sys[n++] = act.sys[k];
        }
        act.n = n;
        if (n == 0) break;
        if (stop_flag && *stop_flag) { for (int k = 0; k < n; ++k) S[act.sys[k]].interrupted = true; break; }
        const dim3 grid(G, n);
        mg_vcycle(MgCycle{c, &act}, 0, B + W.r, B + W.z, W.part); // z = M r, partials of (r, z)
        if (int rc = fetch(1, 1)) return rc;
        for (int k = 0; k < n; ++k) {
            Sys& s = S[act.sys[k]];
            const double rz = W.red_h[k];
            sc.v[k] = it == 0 ? 0.0 : rz / s.rho;
            s.rho = rz;
        }
        const long long p = W.p[it & 1], po = W.p[(it + 1) & 1];
        if (it == 0) hipLaunchKernelGGL((k_mgb_dir_apply<true>), grid, blk, 0, st, act, sc, g, (const double*)(B + W.z), (const double*)nullptr, B + p, B + W.q, W.part);
        else hipLaunchKernelGGL((k_mgb_dir_apply<false>), grid, blk, 0, st, act, sc, g, (const double*)(B + W.z), (const double*)(B + po), B + p, B + W.q, W.part);
        if (int rc = fetch(1, 1)) return rc;
        for (int k = 0; k < n; ++k) sc.v[k] = S[act.sys[k]].rho / W.red_h[k];
        hipLaunchKernelGGL(k_mgb_update, grid, blk, 0, st, act, sc, g, B + W.x, B + W.r, (const double*)(B + p), (const double*)(B + W.q), W.part);
        if (int rc = fetch(MGB_NFIELDS, MGB_RMAX)) return rc;
        take_norms();
        int m = 0;
        for (int k = 0; k < n; ++k) {                              // the tests after an iteration
            Sys& s = S[act.sys[k]];
            s.it = it + 1;
            s.rnorm = std::sqrt(s.rr);
            s.reason = msg_stop_reason(prm, true, s.dmax, s.rmax, false, 0.0);
            if (s.reason) { s.converged = true; continue; }
            act.sys[m++] = act.sys[k];
        }
        act.n = m;
    }
    if (int rc = loop_timer_end(c, st)) return rc;
    hipLaunchKernelGGL(k_mgb_pack, dim3(flat_grid(c->pk_len), nrhs), blk, 0, st, c->pg, W.stride, (const double*)(B + W.x), x_dev);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(st));
    const double loop_s = loop_timer_seconds(c);
    const double solve_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int i = 0; i < nrhs; ++i) {
        const Sys& s = S[i];
        const bool conv = msg ? s.converged : s.rnorm <= prm->eps_rel * s.refnorm;        // matrix_free_system.cpp:472
        mi355cg_results res = make_results(s.it, s.interrupted, conv ? 1 : 0, s.reason, s.dmax, s.rmax, false, 0.0, s.rnorm, s.r0norm);
        res.solve_seconds = solve_s;
        res.loop_seconds = loop_s;
        out[i] = res;
    }
    return MI355CG_OK;
}

// What the on-chip mode refuses (nullptr: the handle is eligible): every handle whose iteration is not the plain fp64 grid CG, and
// grids whose direction does not fit in one CU's LDS.
const char* onchip_refusal(const mi355cg_ctx* c) {
    static char buf[160];
    if (c->is_csr) return "the on-chip solve keeps the grid's direction in LDS: a CSR handle has no grid";
    if (c->is_slab) return "the on-chip solve is one workgroup on one GPU: this handle owns one part of a decomposed grid";
    if (c->dtype != MI355CG_F64) return "the on-chip solve is fp64 only: this handle was created with MI355CG_F32_MIXED";
    if (c->mg) return "the on-chip solve runs plain CG: this handle has a preconditioner (mi355cg_set_preconditioner(h, MI355CG_PRECOND_NONE) first)";
    if (!onchip_supported(c->gp.n)) {
        snprintf(buf, sizeof buf, "the on-chip solve takes grids up to N = %d (the direction must fit in one CU's LDS): this handle has N = %d", kOnchipMaxN, c->gp.n);
        return buf;
    }
    return nullptr;
}

// The refusals the batched entry points share, each written once; what differs is what a kind of batch calls its parts.  Every
// entry point runs the ones it has in its own order (batch_check, many_check, steps_many_check, mi355cg_solve_many_info).
struct BatchKind {
    int most; const char* count_text;                              // "... 1 .. %d <things>, not %d"
    const char* no_exact; const char* no_callbacks;
    const char* plain_cg;                                          // on-chip kinds: what the entry point is, to a handle with a preconditioner
    int count(int n) const { return n < 1 || n > most ? fail(MI355CG_ERR_INVALID, count_text, most, n) : MI355CG_OK; }
    int params(const mi355cg_params* prm) const {
        if (prm->rule != MI355CG_RULE_MSG_MAXNORM && prm->rule != MI355CG_RULE_REL_2NORM) return fail(MI355CG_ERR_INVALID, "unknown rule %d", prm->rule);
        if (prm->use_true_solution) return fail(MI355CG_ERR_INVALID, "%s: use_true_solution must be 0", no_exact);
        if (prm->diagnostics) return fail(MI355CG_ERR_INVALID, "%s has no callbacks: diagnostics must be 0", no_callbacks);
        return MI355CG_OK;
    }
    int onchip(const mi355cg_ctx* c) const {
        if (c->mg) return fail(MI355CG_ERR_STATE, "this handle has a preconditioner: %s", plain_cg);
        if (const char* why = onchip_refusal(c)) return fail(MI355CG_ERR_INVALID, "%s", why);
        return MI355CG_OK;
    }
    // two groups of n full vectors each, `first` the one that is written
    static int apart(const mi355cg_ctx* c, int n, const void* first, const void* second, const char* text) {
        const size_t bytes = sizeof(double) * (size_t)c->gp.size * (size_t)n;
        const uintptr_t fb = (uintptr_t)first, sb = (uintptr_t)second;
        return sb < fb + bytes && fb < sb + bytes ? fail(MI355CG_ERR_INVALID, "%s", text) : MI355CG_OK;
    }
};
const char* const kBatchNoExact = "a batch has no per-system exact solution";
const BatchKind kMgBatch{MI355CG_BATCH_MAX, "a batch has 1 .. %d right-hand sides, not %d", kBatchNoExact, "a batch", nullptr};
const BatchKind kOnchipBatch{MI355CG_MANY_MAX, "a batch of on-chip solves has 1 .. %d systems, not %d", kBatchNoExact, "a batch",
                             "mi355cg_solve_many is plain CG in one workgroup per system (mi355cg_solve_batch is the preconditioned batch)"};
const BatchKind kEnsemble{MI355CG_MANY_MAX, "an ensemble of on-chip steppers has 1 .. %d members, not %d", "a step has no exact solution", "the stepper",
                          "mi355cg_time_steps_many is plain CG in one workgroup per member"};
const BatchKind kWaveEnsemble{MI355CG_MANY_MAX, "an ensemble of on-chip wave steppers has 1 .. %d members, not %d", "a step has no exact solution", "the stepper",
                              "mi355cg_wave_steps_many is one workgroup per member on the plain operator"};

// what both entry points refuse before anything is allocated or written
int batch_check(mi355cg_ctx* c, const mi355cg_params* prm, int nrhs, const void* b, const void* x, const mi355cg_results* out) {
    if (!c || !prm || !b || !x || !out) return fail(MI355CG_ERR_INVALID, "null argument");
    if (int rc = kMgBatch.count(nrhs)) return rc;
    if (int rc = kMgBatch.params(prm)) return rc;
    if (int rc = BatchKind::apart(c, nrhs, x, b, "x overlaps b")) return rc;
    if (!c->mg) return fail(MI355CG_ERR_STATE, "no preconditioner is set on this handle (mi355cg_set_preconditioner): a batch is multigrid-preconditioned CG");
    if (c->mg->cycle != MI355CG_CYCLE_F64) return fail(MI355CG_ERR_INVALID, "a batch runs the fp64 V-cycle: this handle's preconditioner was set with MI355CG_CYCLE_F32");
    return MI355CG_OK;
}

// A host entry point of a batched solve: the packed vectors go up into the staging buffer, the body runs on them in device memory,
// what it wrote comes down.  A group is `count` doubles at stage + at; a null source is not copied up, a null destination not
// copied down.  The caller has ensured the buffer before.
struct StagedGroup { size_t at; const double* up; double* down; };
template <size_t G, class Body>
int run_staged_groups(mi355cg_ctx* c, double* stage, size_t count, const StagedGroup (&groups)[G], Body body) {
    const size_t bytes = sizeof(double) * count;
    for (const StagedGroup& g : groups) if (g.up) HIPCK(hipMemcpyAsync(stage + g.at, g.up, bytes, hipMemcpyHostToDevice, c->stream));
    if (int rc = body()) return rc;
    for (const StagedGroup& g : groups) if (g.down) HIPCK(hipMemcpyAsync(g.down, stage + g.at, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return MI355CG_OK;
}
// Two groups, `body(first, second)`, `second` comes down.  second_at: where the second group starts (count: b or g in the first
// half, x or u in the second; 0: one group that goes up and comes down).
template <class Body>
int run_staged(mi355cg_ctx* c, double* stage, size_t count, size_t second_at, const double* up_first, const double* up_second, double* down, Body body) {
    double* const second = stage + second_at;
    const StagedGroup groups[2] = {{0, up_first, nullptr}, {second_at, up_second, down}};
    return run_staged_groups(c, stage, count, groups, [&]() { return body((const double*)stage, second); });
}

// The unroll classes of onchip_plan (OnchipPlan::elems) and the rule as template arguments, for every on-chip kernel:
// f(std::integral_constant<int, E>, std::bool_constant<MSG>), e.g. to name an instantiation k<decltype(e)::value, decltype(m)::value>.
template <class F>
auto onchip_dispatch(int elems, bool msg, F f) {
    auto with_rule = [&](auto e) { return msg ? f(e, std::true_type{}) : f(e, std::false_type{}); };
    switch (elems) {
        case 1: return with_rule(std::integral_constant<int, 1>{});
        case 2: return with_rule(std::integral_constant<int, 2>{});
        case 4: return with_rule(std::integral_constant<int, 4>{});
        case 8: return with_rule(std::integral_constant<int, 8>{});
        case 16: return with_rule(std::integral_constant<int, 16>{});
        default: return with_rule(std::integral_constant<int, kOnchipMaxElems>{});
    }
}


// ---- block eigensolver (mi355cg_eigs*; kernels in eig_kernels.h) --------------------------------------------
// The Rayleigh-Ritz step on the host (k <= 48): theta ascending and coef (k x k, row-major, column j = Ritz vector j in the basis)
// with coef^T G coef = I and coef^T H coef = diag(theta).  G and H are symmetrised on the way in.  nullptr: done; otherwise why
// the basis is refused.
const char* rr_solve(int k, const double* G, const double* Hm, double* theta, double* coef) {
    const size_t kk = (size_t)k * k;
    std::vector<double> d(k), Gs(kk), Hs(kk), L(kk, 0.0), Y(kk), M(kk), V(kk, 0.0);
    for (int i = 0; i < k; ++i) {
        const double gii = G[(size_t)i * k + i];
        if (!(gii > 0.0) || !std::isfinite(gii)) return "a diagonal entry of the Gram matrix is not positive and finite";
        d[i] = 1.0 / std::sqrt(gii);
    }
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j) {
            Gs[(size_t)i * k + j] = d[i] * (0.5 * (G[(size_t)i * k + j] + G[(size_t)j * k + i])) * d[j];
            Hs[(size_t)i * k + j] = d[i] * (0.5 * (Hm[(size_t)i * k + j] + Hm[(size_t)j * k + i])) * d[j];
            if (!std::isfinite(Gs[(size_t)i * k + j]) || !std::isfinite(Hs[(size_t)i * k + j])) return "an entry of the pair is not finite";
        }
    double lmin = DBL_MAX;
    for (int j = 0; j < k; ++j) {                                  // G^ = L L^T
        double v = Gs[(size_t)j * k + j];
        for (int p = 0; p < j; ++p) v -= L[(size_t)j * k + p] * L[(size_t)j * k + p];
        if (!(v > 0.0)) return "the Cholesky factorisation of the scaled Gram matrix failed";
        const double ljj = std::sqrt(v);
        L[(size_t)j * k + j] = ljj;
        lmin = std::min(lmin, ljj);
        for (int i = j + 1; i < k; ++i) {
            double w = Gs[(size_t)i * k + j];
            for (int p = 0; p < j; ++p) w -= L[(size_t)i * k + p] * L[(size_t)j * k + p];
            L[(size_t)i * k + j] = w / ljj;
        }
    }
    if (lmin < 1e-6) return "the basis is numerically dependent (min diag(L) < 1e-6)";
    for (int c = 0; c < k; ++c)                                    // Y = L^-1 H^
        for (int i = 0; i < k; ++i) {
            double v = Hs[(size_t)i * k + c];
            for (int p = 0; p < i; ++p) v -= L[(size_t)i * k + p] * Y[(size_t)p * k + c];
            Y[(size_t)i * k + c] = v / L[(size_t)i * k + i];
        }
    for (int r = 0; r < k; ++r)                                    // M = Y L^-T, row by row
        for (int i = 0; i < k; ++i) {
            double v = Y[(size_t)r * k + i];
            for (int p = 0; p < i; ++p) v -= L[(size_t)i * k + p] * M[(size_t)r * k + p];
            M[(size_t)r * k + i] = v / L[(size_t)i * k + i];
        }
    for (int i = 0; i < k; ++i)
        for (int j = i + 1; j < k; ++j) M[(size_t)i * k + j] = M[(size_t)j * k + i] = 0.5 * (M[(size_t)i * k + j] + M[(size_t)j * k + i]);
    // cyclic Jacobi: M <- J^T M J until a sweep finds nothing to rotate, V <- V J
    for (int i = 0; i < k; ++i) V[(size_t)i * k + i] = 1.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        int rotations = 0;
        for (int p = 0; p < k - 1; ++p)
            for (int q = p + 1; q < k; ++q) {
                const double apq = M[(size_t)p * k + q];
                const double app = M[(size_t)p * k + p], aqq = M[(size_t)q * k + q];
                if (apq == 0.0 || std::fabs(apq) <= 0.25 * DBL_EPSILON * std::sqrt(std::fabs(app) * std::fabs(aqq))) continue;
                ++rotations;
                const double th = (aqq - app) / (2.0 * apq);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
                const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                for (int r = 0; r < k; ++r) {                      // columns p and q
                    const double arp = M[(size_t)r * k + p], arq = M[(size_t)r * k + q];
                    M[(size_t)r * k + p] = cs * arp - sn * arq;
                    M[(size_t)r * k + q] = sn * arp + cs * arq;
                    const double vrp = V[(size_t)r * k + p], vrq = V[(size_t)r * k + q];
                    V[(size_t)r * k + p] = cs * vrp - sn * vrq;
                    V[(size_t)r * k + q] = sn * vrp + cs * vrq;
                }
                for (int r = 0; r < k; ++r) {                      // rows p and q
                    const double apr = M[(size_t)p * k + r], aqr = M[(size_t)q * k + r];
                    M[(size_t)p * k + r] = cs * apr - sn * aqr;
                    M[(size_t)q * k + r] = sn * apr + cs * aqr;
                }
                M[(size_t)p * k + q] = M[(size_t)q * k + p] = 0.0;
            }
        if (!rotations) break;
    }
    std::vector<int> order(k);
    for (int i = 0; i < k; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return M[(size_t)a * k + a] < M[(size_t)b * k + b]; });
    for (int c = 0; c < k; ++c) {                                  // coef = D L^-T V, columns in ascending order of theta
        const int src = order[c];
        theta[c] = M[(size_t)src * k + src];
        if (!std::isfinite(theta[c])) return "a Ritz value is not finite";
        for (int i = k - 1; i >= 0; --i) {
            double v = V[(size_t)i * k + src];
            for (int p = i + 1; p < k; ++p) v -= L[(size_t)p * k + i] * Y[(size_t)p * k + c];
            Y[(size_t)i * k + c] = v / L[(size_t)i * k + i];      // Y is free: it holds L^-T V now
        }
        for (int i = 0; i < k; ++i) coef[(size_t)i * k + c] = d[i] * Y[(size_t)i * k + c];
    }
    return nullptr;
}

constexpr int kEigMatLen = 2 * kEigBasisMax * kEigBasisMax;       // EigWs::mat: two reduced matrices ...
constexpr int kEigCoefLen = kEigBasisMax * kEigBlockMax;          // ... then the coefficients of a combine
constexpr int kEigGramTilesMax = (kEigBasisMax / kEigTile) * (kEigBasisMax / kEigTile);

void eig_free(mi355cg_ctx* c) {
    if (!c->eig) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    c->eig.reset();
}

// Vectors for a block of m columns on the handle's hierarchy (stage: the host entry point's packed staging too).  A workspace that
// is large enough is kept; a larger one replaces it only once it is complete, so a failure leaves the handle as it was.
int eig_ensure(mi355cg_ctx* c, int m, bool stage) {
    const MgHier& H = *c->mg;
    if (!c->eig || c->eig->cap < m) {
        std::unique_ptr<EigWs> W(new EigWs());
        auto failed = [&](const char* what) { return fail(MI355CG_ERR_HIP, "eigensolver workspace for a block of %d: %s allocation failed", m, what); };
        W->vlen = round_up(H.lv[0].len, 32);
        long long off = (long long)EIG_CYC * W->vlen;
        auto take = [&](long long len) { const long long o = off; off += round_up(len, 32); return o; };
        W->cyc.lv.resize(H.lv.size());
        mg_for_level_vectors(H.lv, [&](int l, MgVecKind which, long long len) {
            (which == MG_VEC_RHS ? W->cyc.lv[l].rhs : which == MG_VEC_OUT ? W->cyc.lv[l].out : W->cyc.lv[l].a) = take(len);
            return MI355CG_OK;
        });
        W->slots = (int)(round_up(off, W->vlen) / W->vlen);
        W->cyc.stride = (long long)W->slots * W->vlen;
        W->cap = m;
        const int G = H.lv[0].grid;
        const long long count = W->cyc.stride * m;
        if (Buf<double>::device(W->base, count)) return failed("vector");
        W->cyc.base.borrow(W->base);
        if (Buf<double>::device(W->part, (long long)kEigGramTilesMax * kEigTileEntries * G)) return failed("partials");
        if (Buf<double>::device(W->mat, kEigMatLen + kEigCoefLen)) return failed("matrix");
        if (Buf<double>::device(W->red, 2 * kEigBlockMax)) return failed("sums");
        if (Buf<double>::pinned(W->mat_h, kEigMatLen + kEigCoefLen + 2 * kEigBlockMax)) return failed("pinned matrix");
        // boundary nodes and pads hold 0 for good: the kernels write interior nodes only
        if (hipMemsetAsync(W->base, 0, sizeof(double) * (size_t)count, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
            (void)hipGetLastError();
            return failed("zero-filled vector");
        }
        eig_free(c);                                               // the staging goes with it: it was sized for the smaller block
        c->eig = std::move(W);
    }
    EigWs* W = c->eig.get();
    if (stage && !W->stage)
        if (Buf<double>::device(W->stage, (long long)c->pk_len * W->cap))
            return fail(MI355CG_ERR_HIP, "eigensolver staging for %d packed vectors: allocation failed", W->cap);
    return MI355CG_OK;
}

// C = A^T B for two lists of vectors of one base: partials, then the ordered sums into c_dev (row-major la.n x lb.n)
template <bool SYM>
void launch_gram(hipStream_t st, const Geom& g, int G, const EigList& la, const EigList& lb, const double* base, double* part, double* c_dev) {
    const int tiles = eig_tiles(la.n) * eig_tiles(lb.n);
    hipLaunchKernelGGL((k_eig_gram<SYM>), dim3(G, tiles), dim3(kBlock), 0, st, g, la, base, lb, base, part);
    hipLaunchKernelGGL((k_eig_reduce<SYM>), dim3(kEigTileEntries, tiles), dim3(kWave), 0, st, la.n, lb.n, G, (const double*)part, c_dev);
}

// The iteration of DESIGN section 10.7 on a block of m columns.  x_dev: m packed vectors in device memory, the start block on
// entry and the Ritz vectors on return.  What the kernels hold is A X, A W, A P and R' = A X + theta X = -(K X - theta X), K = -A:
// H = S^T K S is minus the gram of S and A S, and W = T R = M R' with M the V-cycle.
int solve_eigs(mi355cg_ctx* c, int nev, int m, double tol, int max_iterations, double* x_dev, double* lambda, double* resid,
               const volatile int* stop_flag, mi355cg_eig_results* out) {
    const MgHier& H = *c->mg;
    EigWs& W = *c->eig;
    const Geom& g = H.lv[0].g;
    const int G = H.lv[0].grid;
    const hipStream_t st = c->stream;
    const dim3 blk(kBlock);
    const auto t0 = std::chrono::steady_clock::now();
    const long long cs = W.cyc.stride;
    auto slot = [&](int s) { return W.base + (long long)s * W.vlen; };                    // of column 0
    auto list = [&](EigList& L, int s, const int* cols, int n) { for (int k = 0; k < n; ++k) L.idx[L.n++] = cols[k] * W.slots + s; };
    int all[kEigBlockMax];
    for (int j = 0; j < m; ++j) all[j] = j;
    double* const mat_h = W.mat_h;
    double* const coef_h = W.mat_h + kEigMatLen;
    double* const red_h = coef_h + kEigCoefLen;
    double* const coef_d = W.mat + kEigMatLen;
    MgbAct act{};
    act.stride = cs;
    const MgbScal zero{};
    // q = A v for the listed columns; mg_dir_apply's copy of its direction goes to Z, which is free whenever this runs
    auto apply_A = [&](int src, int dst) {
        hipLaunchKernelGGL((k_mgb_dir_apply<true>), dim3(G, act.n), blk, 0, st, act, zero, g, (const double*)slot(src), (const double*)nullptr,
                           slot(EIG_Z), slot(dst), W.part);
    };
    // G = S^T S and H = -(S^T A S) of the lists -> the host; then the Rayleigh-Ritz step
    std::vector<double> Gm, Hm, th(kEigBasisMax), C((size_t)kEigBasisMax * kEigBasisMax);
    auto fetch_pair = [&](const EigList& ls, const EigList& las) -> int {
        const int k = ls.n;
        launch_gram<true>(st, g, G, ls, ls, W.base, W.part, W.mat);
        launch_gram<true>(st, g, G, ls, las, W.base, W.part, W.mat + (size_t)k * k);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(mat_h, W.mat, sizeof(double) * 2 * k * k, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        Gm.assign(mat_h, mat_h + (size_t)k * k);
        Hm.resize((size_t)k * k);
        for (size_t i = 0; i < (size_t)k * k; ++i) Hm[i] = -mat_h[(size_t)k * k + i];
        return MI355CG_OK;
    };
    // Y_j = sum_i S_i coef[i][j] for the m columns of slot `dst`; coef_h rows [row0, row0 + ls.n) x m are already on the device
    auto combine = [&](const EigList& ls, int row0, int dst) {
        EigList ly{W.vlen, 0, {}};
        list(ly, dst, all, m);
        hipLaunchKernelGGL((k_eig_combine<false>), dim3(G), blk, 0, st, g, ls, (const double*)W.base, (const double*)(coef_d + (size_t)row0 * m), m,
                           ly, W.base, ly, (const double*)W.base);
    };
    auto tail = [&](const EigList& L, int from) { EigList T{L.stride, 0, {}}; for (int i = from; i < L.n; ++i) T.idx[T.n++] = L.idx[i]; return T; };

    std::vector<double> theta(m, 0.0), res(m, HUGE_VAL);
    int it = 0, reason = MI355CG_EIG_ITERATIONS, p_drops = 0, cur = 0, pc = 0;
    bool have_p = false, converged = false;
    // X = the start block, A X, and the first Rayleigh-Ritz step on S = [X]
    hipLaunchKernelGGL(k_mgb_unpack, dim3(flat_grid(c->pk_len), m), blk, 0, st, c->pg, cs, (const double*)x_dev, slot(EIG_X));
    act.n = m;
    for (int j = 0; j < m; ++j) act.sys[j] = j;
    apply_A(EIG_X, EIG_AX);
    {
        EigList ls{W.vlen, 0, {}}, las{W.vlen, 0, {}};
        list(ls, EIG_X, all, m); list(las, EIG_AX, all, m);
        if (int rc = fetch_pair(ls, las)) return rc;
        if (rr_solve(m, Gm.data(), Hm.data(), th.data(), C.data())) {
            reason = MI355CG_EIG_BREAKDOWN;                        // the start block itself is refused: it goes back as it came
            for (int j = 0; j < m; ++j) { const double gj = Gm[(size_t)j * m + j]; theta[j] = gj > 0.0 ? Hm[(size_t)j * m + j] / gj : 0.0; }
        } else {
            for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) coef_h[(size_t)i * m + j] = C[(size_t)i * m + j];
            HIPCK(hipMemcpyAsync(coef_d, coef_h, sizeof(double) * m * m, hipMemcpyHostToDevice, st));
            combine(ls, 0, EIG_X + 1);
            combine(las, 0, EIG_AX + 1);
            cur = 1;
            for (int j = 0; j < m; ++j) theta[j] = th[j];
        }
    }
    while (reason != MI355CG_EIG_BREAKDOWN) {
        // R' = A X + theta X with the norms of R' and X, for all m columns
        MgbScal ths{};
        for (int j = 0; j < m; ++j) ths.v[j] = theta[j];
        hipLaunchKernelGGL(k_eig_resid, dim3(G, m), blk, 0, st, ths, g, cs, (const double*)slot(EIG_X + cur), (const double*)slot(EIG_AX + cur),
                           slot(EIG_R), W.part);
        act.n = m;
        for (int j = 0; j < m; ++j) act.sys[j] = j;
        hipLaunchKernelGGL(k_mgb_reduce, dim3(2, m), dim3(kWave), 0, st, act, 2, 2, G, (const double*)W.part, W.red);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(red_h, W.red, sizeof(double) * 2 * m, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        bool done = true;
        for (int j = 0; j < m; ++j) {
            res[j] = std::sqrt(red_h[2 * j]) / (theta[j] * std::sqrt(red_h[2 * j + 1]));
            if (j < nev && !(res[j] <= tol)) done = false;
        }
        if (done) { converged = true; reason = MI355CG_EIG_CONVERGED; break; }
        if (it >= max_iterations) { reason = MI355CG_EIG_ITERATIONS; break; }
        if (stop_flag && *stop_flag) { reason = MI355CG_EIG_INTERRUPTED; break; }
        int na = 0, cols[kEigBlockMax];                            // soft locking: only columns that have not converged get a W and a P
        for (int j = 0; j < m; ++j) if (!(res[j] <= tol)) cols[na++] = j;
        act.n = na;
        for (int k = 0; k < na; ++k) act.sys[k] = cols[k];
        mg_vcycle(MgCycle{c, &act, &W.cyc}, 0, slot(EIG_R), slot(EIG_Z), nullptr);        // Z = M R' = T R
        // W = Z - X (X^T Z), into R's slots
        EigList lx{W.vlen, 0, {}}, lz{W.vlen, 0, {}}, lw{W.vlen, 0, {}};
        list(lx, EIG_X + cur, all, m); list(lz, EIG_Z, cols, na); list(lw, EIG_R, cols, na);
        launch_gram<false>(st, g, G, lx, lz, W.base, W.part, W.mat);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(mat_h, W.mat, sizeof(double) * m * na, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        for (int i = 0; i < m * na; ++i) coef_h[i] = -mat_h[i];
        HIPCK(hipMemcpyAsync(coef_d, coef_h, sizeof(double) * m * na, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL((k_eig_combine<true>), dim3(G), blk, 0, st, g, lx, (const double*)W.base, (const double*)coef_d, na, lw, W.base, lz,
                           (const double*)W.base);
        apply_A(EIG_R, EIG_AW);
        // S = [X, W, P_act]
        EigList ls = lx, las{W.vlen, 0, {}};
        list(las, EIG_AX + cur, all, m);
        list(ls, EIG_R, cols, na); list(las, EIG_AW, cols, na);
        if (have_p) { list(ls, EIG_P + pc, cols, na); list(las, EIG_AP + pc, cols, na); }
        if (int rc = fetch_pair(ls, las)) return rc;
        int k = ls.n;
        const char* why = rr_solve(k, Gm.data(), Hm.data(), th.data(), C.data());
        if (why && have_p) {                                       // drop P for this iteration: [X, W] is the leading block of the pair
            ++p_drops;
            const int k2 = m + na;
            std::vector<double> G2((size_t)k2 * k2), H2((size_t)k2 * k2);
            for (int i = 0; i < k2; ++i) for (int j = 0; j < k2; ++j) { G2[(size_t)i * k2 + j] = Gm[(size_t)i * k + j]; H2[(size_t)i * k2 + j] = Hm[(size_t)i * k + j]; }
            ls.n = las.n = k = k2;
            why = rr_solve(k, G2.data(), H2.data(), th.data(), C.data());
        }
        if (why) { reason = MI355CG_EIG_BREAKDOWN; break; }
        for (int i = 0; i < k; ++i) for (int j = 0; j < m; ++j) coef_h[(size_t)i * m + j] = C[(size_t)i * k + j];
        HIPCK(hipMemcpyAsync(coef_d, coef_h, sizeof(double) * k * m, hipMemcpyHostToDevice, st));
        combine(ls, 0, EIG_X + (cur ^ 1));
        combine(las, 0, EIG_AX + (cur ^ 1));
        const int pn = have_p ? pc ^ 1 : pc;                       // P+ = S C with the X rows left out
        combine(tail(ls, m), m, EIG_P + pn);
        combine(tail(las, m), m, EIG_AP + pn);
        HIPCK(hipGetLastError());
        cur ^= 1; pc = pn; have_p = true;
        for (int j = 0; j < m; ++j) theta[j] = th[j];
        ++it;
    }
    hipLaunchKernelGGL(k_mgb_pack, dim3(flat_grid(c->pk_len), m), blk, 0, st, c->pg, cs, (const double*)slot(EIG_X + cur), x_dev);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(st));
    for (int j = 0; j < m; ++j) { lambda[j] = theta[j]; resid[j] = res[j]; }
    out->iterations = it;
    out->converged = converged ? 1 : 0;
    out->stop_reason = reason;
    out->p_drops = p_drops;
    out->solve_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return MI355CG_OK;
}

// what both entry points refuse before anything is allocated or written
int eig_check(mi355cg_ctx* c, int nev, int block, double tol, int max_iterations, const void* x, const void* lambda, const void* resid,
              const mi355cg_eig_results* out) {
    if (!c || !x || !lambda || !resid || !out) return fail(MI355CG_ERR_INVALID, "null argument");
    if (nev < 1) return fail(MI355CG_ERR_INVALID, "nev = %d: at least one eigenpair", nev);
    if (block < nev || block > MI355CG_EIG_BLOCK_MAX)
        return fail(MI355CG_ERR_INVALID, "a block has nev .. %d columns, not %d (nev = %d)", MI355CG_EIG_BLOCK_MAX, block, nev);
    if (block > c->gp.size) return fail(MI355CG_ERR_INVALID, "a block of %d is larger than the system (%lld unknowns)", block, (long long)c->gp.size);
    if (!std::isfinite(tol) || !(tol > 0.0)) return fail(MI355CG_ERR_INVALID, "tol must be finite and > 0");
    if (max_iterations < 1) return fail(MI355CG_ERR_INVALID, "max_iterations = %d: at least 1", max_iterations);
    if (!c->mg) return fail(MI355CG_ERR_STATE, "no preconditioner is set on this handle (mi355cg_set_preconditioner): the eigen iteration is multigrid-preconditioned");
    if (c->mg->cycle != MI355CG_CYCLE_F64) return fail(MI355CG_ERR_INVALID, "the eigen iteration runs the fp64 V-cycle: this handle's preconditioner was set with MI355CG_CYCLE_F32");
    return MI355CG_OK;
}

// the block utilities: n packed host vectors -> zero-padded storage vectors of a temporary buffer, vector i at i * vlen
struct BlockTmp { Buf<double> packed, vec, part, mat; };
int block_check(mi355cg_ctx* c) {
    if (c->is_csr) return fail(MI355CG_ERR_INVALID, "the block utilities need the grid operator's storage layout: a CSR handle has no grid");
    if (c->is_slab) return fail(MI355CG_ERR_INVALID, "the block utilities are single-GPU only: this handle owns one part of a decomposed grid");
    return MI355CG_OK;
}
int block_upload(mi355cg_ctx* c, BlockTmp& T, int n, int n_out, const double* const* src, const int* counts, int nsrc, long long vlen) {
    if (Buf<double>::device(T.packed, (long long)c->pk_len * std::max(n, n_out)) || Buf<double>::device(T.vec, vlen * (n + n_out)))
        return fail(MI355CG_ERR_HIP, "block utility: allocation of %d vectors failed", n + n_out);
    HIPCK(hipMemsetAsync(T.vec, 0, sizeof(double) * vlen * (n + n_out), c->stream));
    long long at = 0;
    for (int s = 0; s < nsrc; ++s) {
        HIPCK(hipMemcpyAsync(T.packed + at * c->pk_len, src[s], sizeof(double) * c->pk_len * counts[s], hipMemcpyHostToDevice, c->stream));
        at += counts[s];
    }
    hipLaunchKernelGGL(k_mgb_unpack, dim3(flat_grid(c->pk_len), n), dim3(kBlock), 0, c->stream, c->pg, vlen, (const double*)T.packed, T.vec);
    HIPCK(hipGetLastError());
    return MI355CG_OK;
}

}  // namespace

// ====================================================================================================
extern "C" {

const char* mi355cg_last_error(void) { return g_err.c_str(); }
const char* mi355cg_version(void) { return "mi355cg 0.2 (gfx950)"; }

// What every handle keeps, grid or CSR: the partials of the two phases and of the flat reductions, the device-side CG state with
// its history, and their pinned copies.  The zero-fills run on the NULL stream and are asynchronous to the host; the context's own
// stream is non-blocking and does not order with them.  Without the callers' device-wide wait after it a delayed memset can land
// AFTER the first upload or kernel of the context and wipe it (seen as a right-hand side of zeros -> "converged" at iteration 0).
static int create_state(mi355cg_ctx* c, const char* what) {
    if (int rc = Buf<double>::device_zeroed(c->partA, (long long)FA_COUNT * c->strideA)) return rc;
    if (int rc = Buf<double>::device_zeroed(c->partB, (long long)FB_COUNT * c->strideB)) return rc;
    if (int rc = Buf<double>::device_zeroed(c->partR, 2048)) return rc;
    for (Buf<CgState>* s : {&c->sA, &c->sB, &c->summary}) if (int rc = Buf<CgState>::device_zeroed(*s, 1, what)) return rc;
    if (int rc = Buf<HistEntry>::device_zeroed(c->hist, kHist, what)) return rc;
    if (int rc = Buf<CgState>::pinned(c->summary_h, 1, what)) return rc;
    if (int rc = Buf<HistEntry>::pinned(c->hist_h, kHist, what)) return rc;
    return Buf<double>::pinned(c->partR_h, 2048, what);
}

static int create_impl(int n, int m, double a, double b, double c_, double d, int dtype, int device,
                       int y_lo, int y_hi, int s_lo, int s_hi, bool part, mi355cg_handle* out) {
    if (!out) return fail(MI355CG_ERR_INVALID, "out is null");
    *out = nullptr;
    if (dtype != MI355CG_F64 && dtype != MI355CG_F32_MIXED) return fail(MI355CG_ERR_INVALID, "unknown dtype %d", dtype);
    GridParams gp;
    if (!grid_params_init(&gp, n, m, a, b, c_, d))
        return fail(MI355CG_ERR_INVALID, "grid %dx%d rejected: the L-shaped index map is only consistent for n == m, even, >= 6", n, m);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(MI355CG_ERR_HIP, "no HIP device available (libmi355cg has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(MI355CG_ERR_INVALID, "device %d out of range (0..%d)", device, ndev - 1);
    HIPCK(hipSetDevice(device));

    const int ns_all = strips_total(gp, 2);
    if (!part) { y_lo = 1; y_hi = gp.n - 1; s_lo = 0; s_hi = ns_all; }
    if (y_lo < 1 || y_hi > gp.n - 1 || y_lo > y_hi)
        return fail(MI355CG_ERR_INVALID, "part rows [%d, %d] outside 1..%d", y_lo, y_hi, gp.n - 1);
    if (s_lo < 0 || s_hi > ns_all || s_lo >= s_hi)
        return fail(MI355CG_ERR_INVALID, "part strips [%d, %d) outside 0..%d", s_lo, s_hi, ns_all);
    if (dtype == MI355CG_F32_MIXED && part) return fail(MI355CG_ERR_INVALID, "F32_MIXED is single-GPU only");
    mi355cg_ctx* c = new mi355cg_ctx();
    c->device = device; c->dtype = dtype; c->gp = gp; c->is_slab = part;
    c->s_lo = s_lo; c->s_hi = s_hi;
    build_geom(c, 2, y_lo, y_hi);           // fp64 layout; the fp32 kernels use VEC=4 on the same pitches
    build_plans(c);
    c->strideA = std::max({c->whole.grid, c->interior.grid + c->edge.grid, c->whole32.grid, 1});
    c->strideB = c->strideA;                // the update launches run on the stencil's grids

    int rc = MI355CG_OK;
    auto cleanup = [&]() { mi355cg_destroy(c); return rc; };
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { rc = fail(MI355CG_ERR_HIP, "hipStreamCreate failed"); return cleanup(); }
    if ((rc = upload_item_tables(c))) return cleanup();
    const long long L = c->storage_len;
    // x is folded every M-th iteration: 4 by default.  8 saves another 0.125 words per iteration and measured +0.2-0.7 % for
    // four more vectors (fp64 only: the fp32 8-step launch needs 262 VGPRs and would halve the resident waves)
    { const int m = env_int("MI355CG_XSTEPS", 4); c->xsteps = m == 2 ? 2 : ((m == 8 && dtype == MI355CG_F64) ? 8 : 4); }
    // Deferred x fold (fp64, one context, no explicit MI355CG_XSTEPS): MI355CG_XFOLD = 16 | 32 forces that depth, 0 (or anything else) is
    // the fused update; unset = by size: on from 4 Mi owned elements (the grids that are not graph-replayed), the deepest ring
    // of 32, then 16 buffers that fits in a quarter of the device's memory (N = 16384: 32; N = 32768: fused).
    if (!part && dtype == MI355CG_F64 && !getenv("MI355CG_XSTEPS")) {
        const char* xf = getenv("MI355CG_XFOLD");
        const int want = (xf && *xf) ? atoi(xf) : -1;
        if (want == 16 || want == 32) c->xfold = want;
        else if (want < 0 && c->g.own_len >= (4LL << 20)) {
            size_t mem_free = 0, mem_total = 0;
            if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess)
                for (int R : {32, 16}) if (c->xfold == 0 && sizeof(double) * (size_t)L * (size_t)R <= mem_total / 4) c->xfold = R;
        }
        c->fold_grid = std::max(0, env_int("MI355CG_XFOLD_GRID", 0));
        c->fold_nt = env_int("MI355CG_XFOLD_NT", 1) != 0;
    }
    Buf<double>* vecs[] = {&c->x, &c->r, &c->p[0], &c->p[1], &c->ap, &c->b, &c->u, &c->p[2], &c->p[3], &c->p[4], &c->p[5], &c->p[6], &c->p[7]};
    for (int k = 0; k < 7 + (c->xsteps - 2); ++k) if ((rc = Buf<double>::device_zeroed(*vecs[k], L))) return cleanup();
    if (dtype == MI355CG_F32_MIXED) {
        Buf<float>* fv[] = {&c->xf, &c->rf, &c->pf[0], &c->pf[1], &c->apf, &c->pf[2], &c->pf[3], &c->pf[4], &c->pf[5], &c->pf[6], &c->pf[7]};
        for (int k = 0; k < 5 + (c->xsteps - 2); ++k) if ((rc = Buf<float>::device_zeroed(*fv[k], L, "fp32 vector allocation failed"))) return cleanup();
    }
    if ((rc = Buf<double>::device_zeroed(c->packed, std::max<long long>(c->pk_len, 1)))) return cleanup();
    if ((rc = create_state(c, "state allocation failed"))) return cleanup();
    c->rec_width = kRecHeader + 2 * c->g.Pu;            // [sums | first owned row | last owned row]
    if ((rc = Buf<double>::device_zeroed(c->sumsA, c->rec_width))) return cleanup();
    if ((rc = Buf<double>::device_zeroed(c->sumsB, c->rec_width))) return cleanup();
    if ((rc = Buf<int>::device_zeroed(c->qctr, 2 * kXcds * kQueueSubs * kQueuePitch, "queue counter allocation failed"))) return cleanup();
    if ((rc = Buf<int>::pinned(c->stop_h, 1, "stop word allocation failed"))) return cleanup();
    *c->stop_h = 0;
    if (hipDeviceSynchronize() != hipSuccess) { rc = fail(MI355CG_ERR_HIP, "hipDeviceSynchronize failed"); return cleanup(); }      // the zero-fills: see create_state

    if (env_int("MI355CG_DEVICE_SETUP", 0)) {
        // opt-in: b and u generated on the device, no host pass and no upload; <= 1 ulp from the host values
        c->host_rhs_valid = false; c->host_u_valid = false;
        if ((rc = mi355cg_setup_on_device(c))) return cleanup();
    } else {
        // problem data on the host in the part's packed order (bit-identical to the reference on the same libm), then into
        // storage layout on the device
        c->rhs_h.resize(c->pk_len); c->u_h.resize(c->pk_len);
        grid_fill_box(gp, c->g.y_lo, c->g.y_hi, s_lo * kStripCols, s_hi == ns_all ? gp.n : s_hi * kStripCols, c->rhs_h.data(), c->u_h.data(), nullptr, nullptr);
        if ((rc = upload_packed<double>(c, c->rhs_h.data(), c->b))) return cleanup();
    }
    if (env_int("MI355CG_ONCHIP", 0) == 1 && !onchip_refusal(c)) c->solve_mode = MI355CG_SOLVE_ONCHIP;      // ignored on handles the mode refuses
    *out = c;
    return MI355CG_OK;
}

int mi355cg_create(int n, int m, double a, double b, double c_, double d, int dtype, int device, mi355cg_handle* out) {
    return create_impl(n, m, a, b, c_, d, dtype, device, 0, 0, 0, 0, false, out);
}
int mi355cg_create_slab(int n, int m, double a, double b, double c_, double d, int dtype, int device,
                        int y_lo, int y_hi, mi355cg_handle* out) {
    GridParams gp;
    if (!grid_params_init(&gp, n, m, a, b, c_, d)) return fail(MI355CG_ERR_INVALID, "grid %dx%d rejected: the L-shaped index map is only consistent for n == m, even, >= 6", n, m);
    return create_impl(n, m, a, b, c_, d, dtype, device, y_lo, y_hi, 0, strips_total(gp, 2), true, out);
}
int mi355cg_create_part(int n, int m, double a, double b, double c_, double d, int dtype, int device,
                        int y_lo, int y_hi, int x_lo, int x_hi, mi355cg_handle* out) {
    GridParams gp;
    if (!grid_params_init(&gp, n, m, a, b, c_, d)) return fail(MI355CG_ERR_INVALID, "grid %dx%d rejected: the L-shaped index map is only consistent for n == m, even, >= 6", n, m);
    const int ns_all = strips_total(gp, 2);
    if (x_lo % kStripCols != 0 || (x_hi % kStripCols != 0 && x_hi < gp.n))
        return fail(MI355CG_ERR_INVALID, "part columns [%d, %d): x-cuts must be multiples of %d", x_lo, x_hi, kStripCols);
    return create_impl(n, m, a, b, c_, d, dtype, device, y_lo, y_hi, x_lo / kStripCols, x_hi >= gp.n ? ns_all : x_hi / kStripCols, true, out);
}

int mi355cg_create_csr(long long nrows, const int* row_map, const int* entries, const double* values,
                       int device, mi355cg_handle* out) {
    if (!out) return fail(MI355CG_ERR_INVALID, "out is null");
    *out = nullptr;
    if (nrows <= 0 || !row_map) return fail(MI355CG_ERR_INVALID, "bad CSR arguments");
    if (row_map[0] != 0) return fail(MI355CG_ERR_INVALID, "row_map[0] must be 0");
    const long long nnz = row_map[nrows];
    if (nnz > 0 && (!entries || !values)) return fail(MI355CG_ERR_INVALID, "bad CSR arguments");      // a matrix without entries may come with null arrays
    for (long long i = 0; i < nrows; ++i) if (row_map[i + 1] < row_map[i]) return fail(MI355CG_ERR_INVALID, "row_map is not monotone at row %lld", i);
    for (long long j = 0; j < nnz; ++j) if (entries[j] < 0 || entries[j] >= nrows) return fail(MI355CG_ERR_INVALID, "column index %d out of range at entry %lld", entries[j], j);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MI355CG_ERR_HIP, "no HIP device available (libmi355cg has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(MI355CG_ERR_INVALID, "device %d out of range (0..%d)", device, ndev - 1);
    HIPCK(hipSetDevice(device));
    mi355cg_ctx* c = new mi355cg_ctx();
    c->device = device; c->dtype = MI355CG_F64; c->is_csr = true;
    c->csr_n = nrows; c->csr_nnz = nnz;
    c->gp.size = nrows; c->pk_begin = 0; c->pk_len = nrows; c->storage_len = nrows; c->pg.pk_len = nrows;
    c->g.own_begin = 0; c->g.own_len = nrows;
    const long long nblk = (nrows + kBlock - 1) / kBlock;
    c->grid_csr = (int)std::max<long long>(1, std::min<long long>(2048, nblk));
    c->grid_update = (int)std::max<long long>(1, std::min<long long>(512, nblk));
    c->strideA = c->grid_csr; c->strideB = c->grid_update; c->nB_own = c->grid_update;
    int rc = MI355CG_OK;
    auto cleanup = [&]() { mi355cg_destroy(c); return rc; };
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { rc = fail(MI355CG_ERR_HIP, "hipStreamCreate failed"); return cleanup(); }
    for (Buf<double>* v : {&c->x, &c->r, &c->p[0], &c->p[1], &c->ap, &c->b, &c->u}) if ((rc = Buf<double>::device_zeroed(*v, nrows))) return cleanup();
    if ((rc = create_state(c, "allocation failed"))) return cleanup();
    if ((rc = Buf<int>::device(c->csr_row_map, nrows + 1, "allocation failed")) || (rc = Buf<int>::device(c->csr_entries, std::max<long long>(nnz, 1), "allocation failed")) ||
        (rc = Buf<double>::device(c->csr_values, std::max<long long>(nnz, 1), "allocation failed"))) return cleanup();
    if (hipMemcpy(c->csr_row_map, row_map, sizeof(int) * (nrows + 1), hipMemcpyHostToDevice) != hipSuccess ||
        (nnz > 0 && hipMemcpy(c->csr_entries, entries, sizeof(int) * nnz, hipMemcpyHostToDevice) != hipSuccess) ||
        (nnz > 0 && hipMemcpy(c->csr_values, values, sizeof(double) * nnz, hipMemcpyHostToDevice) != hipSuccess)) {
        rc = fail(MI355CG_ERR_HIP, "CSR upload failed"); return cleanup();
    }
    if (hipDeviceSynchronize() != hipSuccess) { rc = fail(MI355CG_ERR_HIP, "hipDeviceSynchronize failed"); return cleanup(); }      // the zero-fills: see create_state
    c->rhs_h.assign(nrows, 0.0); c->u_h.assign(nrows, 0.0);
    *out = c;
    return MI355CG_OK;
}

int mi355cg_set_true_solution(mi355cg_handle c, const double* u) {
    if (!c || !u) return fail(MI355CG_ERR_INVALID, "null argument");
    HIPCK(hipSetDevice(c->device));
    c->host_u_valid = true;
    c->u_h.resize(c->pk_len);
    std::memcpy(c->u_h.data(), u, sizeof(double) * c->pk_len);
    if (int rc = upload_packed<double>(c, c->u_h.data(), c->u)) return rc;
    c->have_u_dev = true;
    return MI355CG_OK;
}

void mi355cg_destroy(mi355cg_handle c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    clear_graphs(c);
    mg_batch_free(c);
    onchip_many_free(c);
    eig_free(c);
    c->events.destroy();
    for (hipEvent_t e : c->ev_loop) if (e) hipEventDestroy(e);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;                                   // every buffer goes with its member (device_buffer.h)
}

long long mi355cg_size(mi355cg_handle c) { return c ? c->gp.size : -1; }

int mi355cg_get_rhs(mi355cg_handle c, double* out) {
    if (!c || !out) return fail(MI355CG_ERR_INVALID, "null argument");
    if (int rc = ensure_host_copies(c)) return rc;
    std::memcpy(out, c->rhs_h.data(), sizeof(double) * c->pk_len);
    return MI355CG_OK;
}
int mi355cg_get_true_solution(mi355cg_handle c, double* out) {
    if (!c || !out) return fail(MI355CG_ERR_INVALID, "null argument");
    if (int rc = ensure_host_copies(c)) return rc;
    std::memcpy(out, c->u_h.data(), sizeof(double) * c->pk_len);
    return MI355CG_OK;
}
int mi355cg_get_node_coords(mi355cg_handle c, double* xs, double* ys) {
    if (!c || !xs || !ys) return fail(MI355CG_ERR_INVALID, "null argument");
    if (c->is_csr) return fail(MI355CG_ERR_INVALID, "a CSR handle has no grid coordinates");
    const int ns_all = strips_total(c->gp, 2);
    grid_fill_box(c->gp, c->g.y_lo, c->g.y_hi, c->s_lo * kStripCols, c->s_hi == ns_all ? c->gp.n : c->s_hi * kStripCols, nullptr, nullptr, xs, ys);
    return MI355CG_OK;
}
// regenerate b and u of this handle's cells ON THE DEVICE (k_setup).  Opt-in: the device exp() is within
// 1 ulp of glibc's, not identical, so the vectors -- and with them every later number -- may differ from the reference's
// in the last bits.  The host copies are fetched lazily.
int mi355cg_setup_on_device(mi355cg_handle c) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    if (c->is_csr) return fail(MI355CG_ERR_INVALID, "a CSR handle has no grid to set up");
    HIPCK(hipSetDevice(c->device));
    if (c->is_slab) HIPCK(hipDeviceSynchronize());
    SetupArgs s{};
    s.pg = c->pg; s.a = c->gp.a; s.c = c->gp.c; s.x_step = c->gp.x_step; s.y_step = c->gp.y_step; s.xk = c->gp.x_k; s.yk = c->gp.y_k;
    s.n = c->gp.n; s.m = c->gp.m;
    if (c->pk_len > 0) hipLaunchKernelGGL(k_setup, dim3(flat_grid(c->pk_len)), dim3(kBlock), 0, c->stream, s, c->b, c->u);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(c->stream));
    c->have_u_dev = true; c->host_rhs_valid = false; c->host_u_valid = false;
    return MI355CG_OK;
}
int mi355cg_set_rhs(mi355cg_handle c, const double* b) {
    if (!c || !b) return fail(MI355CG_ERR_INVALID, "null argument");
    HIPCK(hipSetDevice(c->device));
    c->host_rhs_valid = true;
    c->rhs_h.resize(c->pk_len);
    std::memcpy(c->rhs_h.data(), b, sizeof(double) * c->pk_len);
    return upload_packed<double>(c, c->rhs_h.data(), c->b);
}

// The reference's apply is const (matrix_free_system.hpp:56) and may be called from an iteration callback in the middle
// of a solve: both entry points work on dedicated scratch vectors, never on a solver vector.
int mi355cg_apply_device(mi355cg_handle c, const double* x_dev, double* y_dev) {
    if (!c || !x_dev || !y_dev) return fail(MI355CG_ERR_INVALID, "null argument");
    if (c->is_slab) return fail(MI355CG_ERR_STATE, "this handle owns one part of a decomposed grid: use the mi355cg_team_* / mi355cg_dist_* entry points");
    HIPCK(hipSetDevice(c->device));
    if (c->is_csr) {
        launch_csr_spmv(c, x_dev, y_dev, nullptr, nullptr, nullptr);
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(c->stream));
        return MI355CG_OK;
    }
    if (int rc = ensure_scratch(c)) return rc;
    hipLaunchKernelGGL((k_unpack<double>), dim3(flat_grid(c->pk_len)), dim3(kBlock), 0, c->stream, c->pg, x_dev, c->scratch[0]);
    launch_apply<double, 2>(c, c->scratch[0], c->scratch[1], whole_part(c));
    hipLaunchKernelGGL((k_pack<double>), dim3(flat_grid(c->pk_len)), dim3(kBlock), 0, c->stream, c->pg, c->scratch[1], y_dev);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(c->stream));
    return MI355CG_OK;
}

int mi355cg_apply(mi355cg_handle c, const double* x, double* y) {
    if (!c || !x || !y) return fail(MI355CG_ERR_INVALID, "null argument");
    if (c->is_slab) return fail(MI355CG_ERR_STATE, "this handle owns one part of a decomposed grid: use the mi355cg_team_* / mi355cg_dist_* entry points");
    HIPCK(hipSetDevice(c->device));
    if (int rc = ensure_scratch(c)) return rc;
    if (int rc = upload_packed<double>(c, x, c->scratch[0])) return rc;
    if (c->is_csr) launch_csr_spmv(c, c->scratch[0], c->scratch[1], nullptr, nullptr, nullptr);
    else launch_apply<double, 2>(c, c->scratch[0], c->scratch[1], whole_part(c));
    HIPCK(hipGetLastError());
    return download_packed<double>(c, c->scratch[1], y);
}

void mi355cg_default_params(mi355cg_params* p, int rule) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->rule = rule;
    p->max_iterations = 10000;                 // solver.hpp:36, matrix_free_system.hpp:101
    p->eps_precision = 1e-6; p->eps_residual = 1e-6; p->eps_exact_error = 1e-6;   // msg_solver.hpp:52-56
    p->eps_rel = 1e-6;                         // matrix_free_system.hpp:100
    p->use_true_solution = 1;
    p->callback_every = rule == MI355CG_RULE_MSG_MAXNORM ? 100 : 1;
    p->diagnostics = 0;
    p->sync_every = 0;
    p->fixed_iterations = 0;
    p->inner_eps = 0.0;
}

// The two ways a solve's state starts, each one pass over the owned range on the part's stream.  (They sit here, at mi355cg_solve,
// because the compiler emits kernels in the order of their first use and the code object keeps the order it was measured in.)
// x = x0 (already in x), r = b - A x0 with A x0 from the plain operator (mi355cg_apply's bits), z = 0.  k_guess_state arms the
// state with ||b||_2 as the reference norm of REL_2NORM.
static int launch_init_guess(mi355cg_ctx* c, bool has_u) {
    launch_apply<double, 2>(c, c->x, c->scratch[0], whole_part(c));
    GuessArgs<double> f{};
    f.begin = c->g.own_begin / 2; f.nvec = c->g.own_len / 2;
    f.b = c->b; f.ax = c->scratch[0]; f.x = c->x; f.r = c->r; f.p0 = c->p[0]; f.u = c->u;
    f.partB = c->partB; f.strideB = c->strideB; f.partG = c->guess_part; f.strideG = c->strideB; f.s_out = c->sB;
    if (has_u) hipLaunchKernelGGL((k_init_guess<double, 2, true>), dim3(c->whole.grid), dim3(kBlock), 0, c->stream, f);
    else hipLaunchKernelGGL((k_init_guess<double, 2, false>), dim3(c->whole.grid), dim3(kBlock), 0, c->stream, f);
    double* norms = c->guess_part + 2 * (size_t)c->strideB;
    hipLaunchKernelGGL(k_guess_state, dim3(1), dim3(kBlock), 0, c->stream, (const double*)c->partB, c->strideB, (const double*)c->guess_part, c->strideB,
                       c->whole.grid, c->sB, norms);
    HIPCK(hipMemcpyAsync(c->guess_norms_h, norms, sizeof(double) * 2, hipMemcpyDeviceToHost, c->stream));     // complete with the first poll
    return MI355CG_OK;
}
// x = 0, r = b, z = 0 (the first stencil makes z = r + 0*z = r; msg_solver.cpp:33-39) and the partial norms of r0.  Everything outside
// the owned range (pitch padding, the rows around the grid) was zeroed when the vectors were allocated and no launch writes anything but
// zeros there; the other directions of the ring are written (iterations 1 .. M-1) before the folded x update first reads them (iteration M).
static void launch_init_fresh(mi355cg_ctx* c, bool has_u) {
    FreshArgs<double> f{};
    f.begin = c->g.own_begin / 2; f.nvec = c->g.own_len / 2;
    f.b = c->b; f.x = c->x; f.r = c->r; f.p0 = c->p[0]; f.u = c->u;
    f.partB = c->partB; f.strideB = c->strideB; f.s_out = c->sB;
    if (has_u) hipLaunchKernelGGL((k_init_fresh<double, 2, true>), dim3(c->whole.grid), dim3(kBlock), 0, c->stream, f);
    else hipLaunchKernelGGL((k_init_fresh<double, 2, false>), dim3(c->whole.grid), dim3(kBlock), 0, c->stream, f);
}

// One chunk of m iterations in one launch of one workgroup, from and to the iteration-boundary state of the two-launch path.
static void launch_onchip_chunk(mi355cg_ctx* c, const IterCfg& cfg, const mi355cg_params* prm, int m) {
    OnchipArgs a{};
    a.g = c->g; a.pl = onchip_plan(c->gp.n);
    a.x = c->x; a.r = c->r; a.u = c->u;
    for (int k = 0; k < c->xsteps; ++k) a.p[k] = c->p[k];
    a.xsteps = c->xsteps;
    a.partB = c->partB; a.nB = c->nB_own; a.strideB = c->strideB;
    a.s = c->sB; a.hist = c->hist; a.rp = cfg.rp;
    a.has_u = cfg.has_u ? 1 : 0; a.u_always = cfg.rp.eps_exact_error > 0 ? 1 : 0; a.every = prm->callback_every;       // need_u of mi355cg_solve
    a.m = m; a.stop_req = c->stop_dev;
    const void* k = onchip_dispatch(a.pl.elems, cfg.rp.rule == MI355CG_RULE_MSG_MAXNORM,
                                    [](auto e, auto m) { return (const void*)&k_onchip<decltype(e)::value, decltype(m)::value>; });
    void* args[] = {&a};
    hipLaunchKernel(k, dim3(1), dim3(a.pl.threads), args, 0, c->stream);
    c->nB_own = 1;                               // the chunk leaves its update partials in one slot
    ++c->onchip_launches;
}

int mi355cg_solve(mi355cg_handle c, const mi355cg_params* prm, mi355cg_iter_cb cb, void* user,
                  const volatile int* stop_flag, mi355cg_results* out) {
    if (!c || !prm) return fail(MI355CG_ERR_INVALID, "null argument");
    if (prm->rule != MI355CG_RULE_MSG_MAXNORM && prm->rule != MI355CG_RULE_REL_2NORM) return fail(MI355CG_ERR_INVALID, "unknown rule %d", prm->rule);
    if (c->is_slab) return fail(MI355CG_ERR_STATE, "this handle owns one part of a decomposed grid: use the mi355cg_team_* / mi355cg_dist_* entry points");
    HIPCK(hipSetDevice(c->device));
    const bool warm = c->guess_pending;          // one-shot: this solve consumes the guess, whatever it returns
    c->guess_pending = false;                    // x_is_guess stays until a solve has completed: a solve that fails before it leaves no solution behind
    c->onchip_launches = 0;
    if (c->is_csr) return solve_csr(c, prm, cb, user, stop_flag, out);
    if (c->dtype == MI355CG_F32_MIXED) return solve_mixed(c, prm, cb, user, stop_flag, out);
    if (c->mg) return solve_mg(c, prm, cb, user, stop_flag, out, warm);               // opt-in preconditioner (fp64 grid handles only)
    const bool msg = prm->rule == MI355CG_RULE_MSG_MAXNORM;
    IterCfg cfg0 = make_cfg(prm);
    // On-chip mode: the chunks below are single launches of k_onchip, which steps x every iteration (nothing folded, nothing to flush).
    // A diagnostics solve needs a true residual per iteration and keeps the two-launch path in either mode.
    const bool onchip = c->solve_mode == MI355CG_SOLVE_ONCHIP && cfg0.want_diag == 0;
    if (onchip) cfg0.x2 = false;
    cfg0.fold = cfg0.x2 && ensure_fold_ring(c);
    const IterCfg cfg = cfg0;
    const bool diag = cfg.want_diag != 0, fold = cfg.fold;
    c->nB_own = c->whole.grid;
    if (cfg.has_u) if (int rc = ensure_u_on_device(c)) return rc;
    if (diag || (warm && !(c->scratch[0] && c->scratch[1]))) if (int rc = ensure_scratch(c)) return rc;      // (a device-wide wait: once per handle for warm starts)
    if (warm) if (int rc = ensure_guess_ws(c)) return rc;

    const auto t0 = std::chrono::steady_clock::now();
    c->events.reset(); c->ev_pairs[0].clear(); c->ev_pairs[1].clear();

    c->cur = 0; c->fcur = 0;
    if (c->qctr && c->dyn_rows > 0) HIPCK(hipMemsetAsync(c->qctr, 0, sizeof(int) * 2 * kXcds * kQueueSubs * kQueuePitch, c->stream));
    if (warm) { if (int rc = launch_init_guess(c, cfg.has_u)) return rc; }      // everything after it is the cold solve's loop
    else launch_init_fresh(c, cfg.has_u);
    HIPCK(hipGetLastError());

    // The stop request: the reference tests its flag at the top of EVERY iteration (msg_solver.cpp:82-87).  Here block 0 of every
    // update launch samples a pinned word and the next stencil prologue turns it into INTERRUPTED, so a request is honoured at the
    // next iteration boundary of the DEVICE, however many iterations the host has already queued.  The caller's flag lives in
    // ordinary host memory; while this thread waits for a chunk it forwards the flag to the pinned word.
    *c->stop_h = 0;
    c->stop_dev = nullptr;
    if (stop_flag) HIPCK(hipHostGetDevicePointer((void**)&c->stop_dev, c->stop_h, 0));
    auto wait_stream = [&]() -> int { return wait_stream_forwarding_stop(c, stop_flag); };
    bool polled = false;
    auto poll = [&]() -> int {
        launch_check(c, cfg, c->stream, own_partB(c));
        if (int rc = fetch_state(c, c->stream)) return rc;
        polled = true;
        return wait_stream();
    };
    // The state of iteration 0 is only fetched when somebody looks at it (the it = 0 callback, msg_solver.cpp:75-77);
    // ||r0|| travels in the state and is read with the last poll.
    *c->summary_h = CgState{};
    if (msg && (cb || warm)) {
        if (int rc = poll()) return rc;
        if (cb) cb(user, 0, DBL_MAX, c->summary_h->rmax, cfg.has_u ? c->summary_h->emax : DBL_MAX);
    }
    // A cold MSG solve enters iteration 1 untested, as the reference does.  The r0 of a guess may be 0 (alpha = 0 / 0), so a warm one
    // first applies the stop tests that have their numbers to the start state (one poll, taken above).
    if (warm)
        if (const int reason = msg_stop_reason(prm, false, 0.0, c->summary_h->rmax, cfg.has_u, c->summary_h->emax)) {
            c->summary_h->done = 1; c->summary_h->converged = 1; c->summary_h->reason = reason;
        }
    if (int rc = loop_timer_begin(c, c->stream)) return rc;

    // The reference recomputes ||x - u|| every iteration (msg_solver.cpp:132-139), but the value is only
    // observable through the exact-error criterion, the periodic callbacks and the final report: read u
    // on exactly those iterations (same values), and once more after the loop if the last one skipped it.
    const int every = prm->callback_every;
    auto need_u = [&](int it) { return diag || cfg.rp.eps_exact_error > 0 || it == 1 || (every > 0 && it % every == 0); };
    const int sync_every = default_sync_every(prm, msg);
    int it_done = 0;
    bool interrupted = false;
    bool first_chunk = cb != nullptr || stop_flag != nullptr;        // a caller that watches the solve
    if (std::memcmp(&c->graph_prm, prm, sizeof *prm) != 0 || c->graph_stop != (stop_flag != nullptr)) {         // kernel arguments embed the solve's parameters
        clear_graphs(c); c->graph_prm = *prm; c->graph_stop = stop_flag != nullptr;                                // (and whether the stop word is sampled): graphs live as long as those do
    }
    const bool graph_ok = !c->profiling && !diag &&
                          (c->use_graph == 1 || (c->use_graph < 0 && c->g.own_len < (4LL << 20) && prm->max_iterations >= 4 * sync_every));
    while (!c->summary_h->done) {
        if (stop_flag && *stop_flag) { interrupted = true; break; }            // msg_solver.cpp:82-87
        const int m = chunk_len(prm, msg, sync_every, it_done, first_chunk);
        first_chunk = false;
        auto enqueue_chunk = [&]() -> int {
            for (int k = 0; k < m; ++k) {
                hipEvent_t e0 = nullptr;
                // Fold mode: the direction pair of this iteration sits in ring slots fcur and fcur + 1.  The launchers address p[] by
                // c->cur, so they are handed a table with those two slots at cur and cur + 1 (the update launch is XM = 0: no pprev).
                Buf<double> pp[kRing];
                if (fold) { pp[c->cur].borrow(c->fold_p[c->fcur]); pp[(c->cur + 1) % c->xsteps].borrow(c->fold_p[(c->fcur + 1) % c->xfold]); }
                const Buf<double>* ring = fold ? pp : c->p;
                prof_begin(c, &e0);
                launch_iteration_stencil<double, 2>(c, cfg, c->r, ring, whole_part(c), own_partB(c));
                c->cur = (c->cur + 1) % c->xsteps;
                if (fold) c->fcur = (c->fcur + 1) % c->xfold;
                prof_end(c, 0, e0);
                prof_begin(c, &e0);
                IterCfg ucfg = cfg;
                ucfg.has_u = cfg.has_u && need_u(it_done + k + 1);      // skip the u stream when nothing reads the error norm
                launch_iteration_update<double, 2>(c, ucfg, c->x, c->r, ring, c->u, whole_part(c), own_partA(c));
                if (fold && c->fcur == 0) launch_fold_x(c, -1, c->stream);      // iteration k = 0 mod R: the last R x steps (update-phase time)
                prof_end(c, 1, e0);
                if (diag) {
                    // MatrixFreeSolver's per-iteration report needs the TRUE residual (matrix_free_system.cpp:457-463): a
                    // second apply and its norm, all in-stream; the value lands in the history entry of this iteration.
                    launch_apply<double, 2>(c, c->x, c->scratch[0], whole_part(c));
                    hipLaunchKernelGGL((k_resid2<double>), dim3(1024), dim3(kBlock), 0, c->stream, c->g.own_begin, c->g.own_len, c->b, c->scratch[0], c->partR);
                    hipLaunchKernelGGL(k_resid2_hist, dim3(1), dim3(kBlock), 0, c->stream, c->partR, 1024, c->sB, c->hist);
                }
            }
            return MI355CG_OK;
        };
        if (onchip) {
            launch_onchip_chunk(c, cfg, prm, m);
        } else if (graph_ok && m >= 8) {
            // Launch-bound grids: replay the chunk as one hipGraph.  The chunk's kernel arguments depend only on
            // (m, direction-buffer parity, which iterations read u), so equal shapes share an instantiated graph.
            std::vector<char> flags(m);
            for (int k = 0; k < m; ++k) flags[k] = cfg.has_u && need_u(it_done + k + 1);
            mi355cg_ctx::ChunkGraph* hit = nullptr;
            const int key = fold ? c->fcur : c->cur;             // the ring position the chunk starts at (fcur % xsteps == cur)
            for (auto& g : c->graphs) if (g.m == m && g.cur == key && g.flags == flags) hit = &g;
            if (!hit) {
                hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
                const int cur0 = c->cur, fcur0 = c->fcur;
                HIPCK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
                const int rc = enqueue_chunk();
                const hipError_t e1 = hipStreamEndCapture(c->stream, &graph);
                c->cur = cur0; c->fcur = fcur0;                  // the capture only recorded; nothing ran
                if (rc) return rc;
                HIPCK(e1);
                HIPCK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
                HIPCK(hipGraphDestroy(graph));
                c->graphs.push_back({m, key, flags, exec});
                hit = &c->graphs.back();
            }
            HIPCK(hipGraphLaunch(hit->exec, c->stream));
            c->cur = (c->cur + m) % c->xsteps;                    // what enqueue_chunk would have left behind
            if (fold) c->fcur = (c->fcur + m) % c->xfold;
        } else {
            if (int rc = enqueue_chunk()) return rc;
        }
        HIPCK(hipGetLastError());
        if (int rc = poll()) return rc;
        const int it_now = c->summary_h->it;
        replay_callbacks(cb, user, prm, *c->summary_h, c->hist_h, it_done, it_now, cfg.has_u, diag);
        it_done = it_now;
    }
    if (int rc = loop_timer_end(c, c->stream)) return rc;
    CgState fin = *c->summary_h;
    c->stop_dev = nullptr;
    if (fin.done && fin.reason == MI355CG_STOP_INTERRUPTED) interrupted = true;      // the device saw the request in the middle of a chunk
    // Launches enqueued after the stop decision return in their prologue but still flipped c->cur on the
    // host: the direction of the last REAL iteration is p[it % M] (the solve starts with cur = 0).
    c->cur = fin.it % c->xsteps;
    if (cfg.x2) {                                   // folded x update: the steps after the last multiple of M (of R) are still pending
        if (fold) { c->fcur = fin.it % c->xfold; if (c->fcur != 0) launch_fold_x(c, fin.it, c->stream); }
        else launch_flush_x<double, 2>(c, c->whole, c->x, c->p, fin, c->stream);
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(c->stream));
    }
    if (cfg.has_u && fin.it > 0 && !need_u(fin.it)) {
        hipLaunchKernelGGL((k_err_maxnorm<double>), dim3(1024), dim3(kBlock), 0, c->stream, c->g.own_begin, c->g.own_len, c->x, c->u, c->partR);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(c->partR_h, c->partR, sizeof(double) * 1024, hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        double m = 0; for (int i = 0; i < 1024; ++i) m = std::max(m, c->partR_h[i]);
        fin.emax = m;
    }
    c->solved = true; c->x_is_guess = false;
    prof_collect(c);
#ifdef MI355CG_WAVE_TIMING
    if (const char* path = getenv("MI355CG_WAVE_TIMING_OUT")) {     // diagnostic build: per-wave timestamps of the last launch of each kernel
        std::vector<unsigned long long> buf(2 * kWtStamps * kWtWaves);
        HIPCK(hipMemcpyFromSymbol(buf.data(), HIP_SYMBOL(g_wave_dbg), buf.size() * sizeof(unsigned long long)));
        if (FILE* f = fopen(path, "wb")) { fwrite(buf.data(), sizeof(unsigned long long), buf.size(), f); fclose(f); }
    }
#endif
    // `polled` is set by the poll that fills summary_h, so every path that has a non-zero state has the two pinned norms as well; a solve
    // that never polled (a stop request set before the call) reports the zeros of the empty state, exactly as a cold solve does
    // warm: the state's reference norm is ||b||_2, this field stays ||r0||_2 (read with the first poll)
    mi355cg_results res = make_results(fin, interrupted, cfg.has_u, warm && polled ? c->guess_norms_h[0] : fin.r0norm);
    res.solve_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    HIPCK(hipEventSynchronize(c->ev_loop[1]));
    res.loop_seconds = loop_timer_seconds(c);
    if (msg && cb) cb(user, res.iterations, res.final_precision, res.final_residual_norm, res.final_error_norm);   // msg_solver.cpp:193-195
    if (out) *out = res;
    return MI355CG_OK;
}

int mi355cg_get_solution(mi355cg_handle c, double* x) {
    if (!c || !x) return fail(MI355CG_ERR_INVALID, "null argument");
    if (c->x_is_guess) return fail(MI355CG_ERR_STATE, "an initial guess was set after the last solve: x holds the guess, not a solution");
    if (!c->solved) return fail(MI355CG_ERR_STATE, "no solve has run on this handle");
    HIPCK(hipSetDevice(c->device));
    return download_packed<double>(c, c->x, x);
}
int mi355cg_get_recursive_residual(mi355cg_handle c, double* r) {
    if (!c || !r) return fail(MI355CG_ERR_INVALID, "null argument");
    if (c->x_is_guess) return fail(MI355CG_ERR_STATE, "an initial guess was set after the last solve: r is not the residual of x");
    if (!c->solved) return fail(MI355CG_ERR_STATE, "no solve has run on this handle");
    HIPCK(hipSetDevice(c->device));
    return download_packed<double>(c, c->r, r);
}
int mi355cg_get_true_residual(mi355cg_handle c, double* out) {
    if (!c || !out) return fail(MI355CG_ERR_INVALID, "null argument");
    if (c->is_slab) return fail(MI355CG_ERR_STATE, "this handle owns one part of a decomposed grid: use the mi355cg_team_* / mi355cg_dist_* entry points");
    if (c->x_is_guess) return fail(MI355CG_ERR_STATE, "an initial guess was set after the last solve: x holds the guess, not a solution");
    if (!c->solved) return fail(MI355CG_ERR_STATE, "no solve has run on this handle");
    HIPCK(hipSetDevice(c->device));
    if (int rc = ensure_scratch(c)) return rc;
    // residual = A x - b   (dirichlet_solver.cpp:147-161)
    if (c->is_csr) launch_csr_spmv(c, c->x, c->scratch[0], nullptr, nullptr, nullptr);
    else launch_apply<double, 2>(c, c->x, c->scratch[0], whole_part(c));
    hipLaunchKernelGGL((k_sub<double>), dim3(flat_grid(c->g.own_len)), dim3(kBlock), 0, c->stream, c->g.own_begin, c->g.own_len, c->scratch[0], c->b, c->scratch[1]);
    HIPCK(hipGetLastError());
    return download_packed<double>(c, c->scratch[1], out);
}

// ---- warm starts ----------------------------------------------------------------------------------------
// The guess is written straight into the handle's x (no extra vector) and consumed by the next mi355cg_solve.  From here to that
// solve x is not a solution and r does not belong to it: the three getters above refuse.
static int guess_check(mi355cg_ctx* c) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    if (c->is_csr) return fail(MI355CG_ERR_INVALID, "an initial guess needs the grid operator's start (r0 = b - A x0): a CSR handle has none");
    if (c->is_slab) return fail(MI355CG_ERR_INVALID, "an initial guess is single-GPU only: this handle owns one part of a decomposed grid");
    if (c->dtype != MI355CG_F64) return fail(MI355CG_ERR_INVALID, "an initial guess is fp64 only: this handle was created with MI355CG_F32_MIXED");
    return MI355CG_OK;
}

int mi355cg_set_initial_guess(mi355cg_handle c, const double* x0) {
    if (int rc = guess_check(c)) return rc;
    if (!x0) { c->guess_pending = false; return MI355CG_OK; }      // withdrawn; if one was set, x stays unusable until the next solve
    HIPCK(hipSetDevice(c->device));
    c->x_is_guess = true;                                          // from the first byte written
    if (int rc = upload_packed<double>(c, x0, c->x)) return rc;
    c->guess_pending = true;
    return MI355CG_OK;
}

int mi355cg_set_initial_guess_device(mi355cg_handle c, const double* x0_dev) {
    if (int rc = guess_check(c)) return rc;
    if (!x0_dev) return fail(MI355CG_ERR_INVALID, "null argument");
    HIPCK(hipSetDevice(c->device));
    c->x_is_guess = true;
    hipLaunchKernelGGL((k_unpack<double>), dim3(flat_grid(c->pk_len)), dim3(kBlock), 0, c->stream, c->pg, x0_dev, c->x);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(c->stream));
    c->guess_pending = true;
    return MI355CG_OK;
}

int mi355cg_use_solution_as_initial_guess(mi355cg_handle c) {
    if (int rc = guess_check(c)) return rc;
    if (!c->solved || c->x_is_guess) return fail(MI355CG_ERR_STATE, "no solve has run on this handle: there is no solution to start from");
    c->x_is_guess = true;                                          // x is complete when a solve returns (k_fold_x / k_flush_x ran): nothing to flush
    c->guess_pending = true;
    return MI355CG_OK;
}

// ---- diagonal shift and implicit time steps ---------------------------------------------------------------
// what a shift, and with it the stepper, refuses: the handles whose operator is not the single-GPU fp64 grid stencil
static int shift_check(mi355cg_ctx* c) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    if (c->is_csr) return fail(MI355CG_ERR_INVALID, "a shift changes the grid operator's diagonal: a CSR handle's matrix is the caller's");
    if (c->is_slab) return fail(MI355CG_ERR_INVALID, "a shift is single-GPU only: this handle owns one part of a decomposed grid");
    if (c->dtype != MI355CG_F64) return fail(MI355CG_ERR_INVALID, "a shift is fp64 only: this handle was created with MI355CG_F32_MIXED");
    return MI355CG_OK;
}

// The operator becomes A - sigma I.  Everything that can fail (the upload of the refactored coarse inverse) happens before the
// handle is touched, so a failure leaves the old hierarchy and the old sigma.
int mi355cg_set_shift(mi355cg_handle c, double sigma) {
    if (int rc = shift_check(c)) return rc;
    if (!std::isfinite(sigma) || sigma < 0.0) return fail(MI355CG_ERR_INVALID, "shift %g rejected: sigma must be finite and >= 0 (A - sigma I stays negative definite)", sigma);
    if (sigma == c->sigma) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->stream));                        // nothing in flight reads the coefficients or the inverse
    if (MgHier* H = c->mg.get()) {
        Geom gc = H->lv.back().g;
        gc.A = -2 * (gc.xk + gc.yk) - sigma;
        std::vector<double> inv;
        std::vector<int> off;
        mg_coarse_inverse(gc, inv, off);                           // off: the layout's, unchanged
        std::vector<Buf<double>> tabs;                             // the lines' factors hold the diagonal too
        if (int rc = mg_make_line_tables(H, H->line_dir, sigma, tabs)) return rc;
        // the last step that can fail: upload replaces the inverse only once the new one is on the device
        if (H->cycle == MI355CG_CYCLE_F32 ? upload(std::vector<float>(inv.begin(), inv.end()), H->inv32) : upload(inv, H->inv))
            return fail(MI355CG_ERR_HIP, "coarse inverse upload failed: the shift stays %g", c->sigma);
        for (size_t l = 0; l < H->lv.size(); ++l) {
            Geom& g = H->lv[l].g;
            g.A = -2 * (g.xk + g.yk) - sigma;                      // mg_geom's expression
            if (l < H->lv32.size()) H->lv32[l].c.A = (float)g.A;
        }
        mg_install_line_tables(H, H->line_dir, tabs);
    }
    c->sigma = sigma;
    c->g.A = c->gp.A - sigma;
    c->pg.g.A = c->g.A;
    clear_graphs(c);                                               // their kernel arguments hold the old Geom
    return MI355CG_OK;
}

int mi355cg_get_shift(mi355cg_handle c, double* sigma) {
    if (!c || !sigma) return fail(MI355CG_ERR_INVALID, "null argument");
    *sigma = c->sigma;
    return MI355CG_OK;
}

int mi355cg_get_solution_device(mi355cg_handle c, double* x_dev) {
    if (!c || !x_dev) return fail(MI355CG_ERR_INVALID, "null argument");
    if (c->x_is_guess) return fail(MI355CG_ERR_STATE, "an initial guess was set after the last solve: x holds the guess, not a solution");
    if (!c->solved) return fail(MI355CG_ERR_STATE, "no solve has run on this handle");
    HIPCK(hipSetDevice(c->device));
    if (c->is_csr) {
        HIPCK(hipMemcpyAsync(x_dev, c->x, sizeof(double) * c->pk_len, hipMemcpyDeviceToDevice, c->stream));
    } else {
        if (c->is_slab) HIPCK(hipDeviceSynchronize());
        if (c->pk_len > 0) hipLaunchKernelGGL((k_pack<double>), dim3(flat_grid(c->pk_len)), dim3(kBlock), 0, c->stream, c->pg, (const double*)c->x, x_dev);
        HIPCK(hipGetLastError());
    }
    HIPCK(hipStreamSynchronize(c->stream));
    return MI355CG_OK;
}

// b_step = g / theta - sigma u - ((1 - theta) / theta) A u from the state u = x and the handle's g = b, into step_b
static void launch_step_rhs(mi355cg_ctx* c, double sigma, double theta) {
    StepRhsArgs a{};
    a.g = c->g;
    a.A0 = c->gp.A; a.xk = c->gp.x_k; a.yk = c->gp.y_k;
    a.sigma = sigma; a.theta = theta; a.c1 = (1.0 - theta) / theta;
    a.u = c->x; a.rhs = c->b; a.out = c->step_b;
    a.tiles_per_row = (c->g.N + kStepTileCols) / kStepTileCols;                    // columns 0 .. N
    a.tiles = (long long)(c->g.N - 1) * a.tiles_per_row;
    const int grid = (int)std::min<long long>(a.tiles, 1 << 20);
    if (theta < 1.0) hipLaunchKernelGGL((k_step_rhs<true>), dim3(grid), dim3(kBlock), 0, c->stream, a);
    else hipLaunchKernelGGL((k_step_rhs<false>), dim3(grid), dim3(kBlock), 0, c->stream, a);
}

// nsteps steps of the theta scheme for u_t = A u - g, the state in x, no packed vector over PCIe.  Each step is mi355cg_solve's warm
// start on the handle with the step's right-hand side in the place of b; the handle's own b is never written.
int mi355cg_time_steps(mi355cg_handle c, const mi355cg_params* prm, double tau, double theta, int nsteps,
                       const volatile int* stop_flag, mi355cg_results* out, int* steps_done) {
    if (!c || !prm || !out || !steps_done) return fail(MI355CG_ERR_INVALID, "null argument");
    if (int rc = shift_check(c)) return rc;
    if (!std::isfinite(tau) || !(tau > 0.0)) return fail(MI355CG_ERR_INVALID, "time step %g rejected: tau must be finite and > 0", tau);
    if (!(theta > 0.0 && theta <= 1.0)) return fail(MI355CG_ERR_INVALID, "theta %g rejected: the scheme needs 0 < theta <= 1", theta);
    if (nsteps < 0) return fail(MI355CG_ERR_INVALID, "nsteps %d rejected: it must be >= 0", nsteps);
    if (prm->rule != MI355CG_RULE_MSG_MAXNORM && prm->rule != MI355CG_RULE_REL_2NORM) return fail(MI355CG_ERR_INVALID, "unknown rule %d", prm->rule);
    if (prm->diagnostics) return fail(MI355CG_ERR_INVALID, "the stepper has no callbacks: diagnostics must be 0");
    if (prm->use_true_solution) return fail(MI355CG_ERR_INVALID, "a step has no exact solution: use_true_solution must be 0");
    const double sigma = 1.0 / (theta * tau);
    if (!std::isfinite(sigma)) return fail(MI355CG_ERR_INVALID, "time step %g rejected: 1 / (theta tau) is not finite", tau);
    if (nsteps == 0) { *steps_done = 0; return MI355CG_OK; }
    if (!c->guess_pending) return fail(MI355CG_ERR_STATE, "no starting state: set it with mi355cg_set_initial_guess* or mi355cg_use_solution_as_initial_guess");
    *steps_done = 0;
    HIPCK(hipSetDevice(c->device));
    if (!c->step_b) {
        if (int rc = Buf<double>::device_zeroed(c->step_b, c->storage_len)) return rc;
        HIPCK(hipDeviceSynchronize());                             // the zero-fill ran on the NULL stream
    }
    if (int rc = mi355cg_set_shift(c, sigma)) return rc;           // a no-op when it is already exactly sigma
    for (int k = 0; k < nsteps; ++k) {
        if (k > 0) { c->x_is_guess = true; c->guess_pending = true; }     // mi355cg_use_solution_as_initial_guess
        launch_step_rhs(c, sigma, theta);
        HIPCK(hipGetLastError());
        std::swap(c->b, c->step_b);                                // the step's right-hand side in the place of b ...
        const int rc = mi355cg_solve(c, prm, nullptr, nullptr, stop_flag, &out[k]);
        std::swap(c->b, c->step_b);                                // ... and back, whatever the solve returned
        if (rc) return rc;
        if (!out[k].converged) break;                              // the iteration cap or a stop request: x holds that step's last iterate
        ++*steps_done;
    }
    return MI355CG_OK;
}

int mi355cg_set_profiling(mi355cg_handle c, int enable) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    c->profiling = enable != 0;
    return MI355CG_OK;
}
int mi355cg_get_kernel_time(mi355cg_handle c, int kernel, double* avg_ms, long long* launches) {
    if (!c || kernel < 0 || kernel > 1) return fail(MI355CG_ERR_INVALID, "bad argument");
    if (avg_ms) *avg_ms = c->kernel_ms[kernel];
    if (launches) *launches = c->kernel_launches[kernel];
    return MI355CG_OK;
}
int mi355cg_get_layout(mi355cg_handle c, long long* padded_len, int* pitch_bottom, int* pitch_upper,
                       int* grid_stencil, int* grid_update, int* rows_per_item) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    if (padded_len) *padded_len = c->g.own_len;
    if (pitch_bottom) *pitch_bottom = c->g.Pb;
    if (pitch_upper) *pitch_upper = c->g.Pu;
    if (grid_stencil) *grid_stencil = c->whole.grid;
    if (grid_update) *grid_update = c->whole.grid;
    if (rows_per_item) *rows_per_item = c->whole.ty;
    return MI355CG_OK;
}

int mi355cg_get_xfold(mi355cg_handle c, int* depth, int* extra_buffers) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    if (depth) *depth = c->xfold;
    if (extra_buffers) *extra_buffers = c->fold_extra;
    return MI355CG_OK;
}

// ---- on-chip solve mode -----------------------------------------------------------------------------
int mi355cg_set_solve_mode(mi355cg_handle c, int mode) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    if (mode != MI355CG_SOLVE_LAUNCHES && mode != MI355CG_SOLVE_ONCHIP)
        return fail(MI355CG_ERR_INVALID, "unknown solve mode %d (MI355CG_SOLVE_LAUNCHES = 0, MI355CG_SOLVE_ONCHIP = 1)", mode);
    if (mode == MI355CG_SOLVE_ONCHIP) if (const char* why = onchip_refusal(c)) return fail(MI355CG_ERR_INVALID, "%s", why);
    if (mode == c->solve_mode) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->stream));
    clear_graphs(c);                                               // chunks of the other mode
    c->solve_mode = mode;
    return MI355CG_OK;
}
int mi355cg_get_solve_mode(mi355cg_handle c, int* mode, long long* onchip_launches_last_solve) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    if (mode) *mode = c->solve_mode;
    if (onchip_launches_last_solve) *onchip_launches_last_solve = c->onchip_launches;
    return MI355CG_OK;
}
int mi355cg_onchip_plan(int n, int* threads, int* lds_bytes, int* elems_per_thread) {
    if (!onchip_supported(n))
        return fail(MI355CG_ERR_INVALID, "grid %d rejected: the on-chip solve takes even n from 6 to %d", n, kOnchipMaxN);
    const OnchipPlan pl = onchip_plan(n);
    if (threads) *threads = pl.threads;
    if (lds_bytes) *lds_bytes = pl.lds_bytes;
    if (elems_per_thread) *elems_per_thread = pl.elems;
    return MI355CG_OK;
}

// ---- geometric multigrid preconditioner (opt-in) ----------------------------------------------------------------------
int mi355cg_mg_levels(int n, int* levels, int* coarsest_n) {
    std::vector<int> ns;
    if (int rc = mg_shape(MI355CG_PRECOND_MG, n, &ns)) return rc;
    if (levels) *levels = (int)ns.size();
    if (coarsest_n) *coarsest_n = ns.back();
    return MI355CG_OK;
}

int mi355cg_mg_hierarchy(int kind, int n, int max_levels, int* levels, int* level_n) {
    if (max_levels < 0 || (max_levels > 0 && !level_n)) return fail(MI355CG_ERR_INVALID, "level_n must hold max_levels >= 0 entries");
    std::vector<int> ns;
    if (int rc = mg_shape(kind, n, &ns)) return rc;
    if (levels) *levels = (int)ns.size();
    for (int l = 0; l < (int)ns.size() && l < max_levels; ++l) level_n[l] = ns[l];
    return MI355CG_OK;
}

int mi355cg_set_preconditioner(mi355cg_handle c, int kind) { return mi355cg_set_preconditioner_ex(c, kind, MI355CG_CYCLE_F64); }

int mi355cg_set_preconditioner_ex(mi355cg_handle c, int kind, int cycle) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    if (kind != MI355CG_PRECOND_NONE && kind != MI355CG_PRECOND_MG && kind != MI355CG_PRECOND_MG_ANY)
        return fail(MI355CG_ERR_INVALID, "unknown preconditioner kind %d (MI355CG_PRECOND_NONE = 0, MI355CG_PRECOND_MG = 1, "
                    "MI355CG_PRECOND_MG_ANY = 2)", kind);
    HIPCK(hipSetDevice(c->device));
    if (kind == MI355CG_PRECOND_NONE) {
        mg_batch_free(c);                                          // the batch workspace belongs to the hierarchy it was built for
        eig_free(c);                                               // and so does the eigensolver's
        if (c->mg) { HIPCK(hipStreamSynchronize(c->stream)); c->mg.reset(); }
        return MI355CG_OK;
    }
    if (c->is_csr) return fail(MI355CG_ERR_INVALID, "the multigrid preconditioner needs the grid operator: a CSR handle has no grid");
    if (c->is_slab) return fail(MI355CG_ERR_INVALID, "the multigrid preconditioner is single-GPU only: this handle owns one part of a decomposed grid");
    if (c->dtype != MI355CG_F64) return fail(MI355CG_ERR_INVALID, "the multigrid preconditioner is fp64 only: this handle was created with MI355CG_F32_MIXED");
    if (c->solve_mode == MI355CG_SOLVE_ONCHIP)
        return fail(MI355CG_ERR_INVALID, "this handle is in the on-chip solve mode, which runs plain CG: mi355cg_set_solve_mode(h, MI355CG_SOLVE_LAUNCHES) first");
    std::vector<int> ns;
    if (int rc = mg_shape(kind, c->gp.n, &ns)) return rc;          // refused: the handle keeps what it had
    if (cycle != MI355CG_CYCLE_F64 && cycle != MI355CG_CYCLE_F32)
        return fail(MI355CG_ERR_INVALID, "unknown V-cycle precision %d (MI355CG_CYCLE_F64 = 0, MI355CG_CYCLE_F32 = 1)", cycle);
    if (cycle == MI355CG_CYCLE_F32 && c->smoother != MI355CG_SMOOTHER_JACOBI)
        return fail(MI355CG_ERR_INVALID, "the fp32 V-cycle smooths with point Jacobi only: this handle has line smoother %d "
                    "(mi355cg_set_smoother(h, MI355CG_SMOOTHER_JACOBI) first)", c->smoother);
    mg_batch_free(c);                                              // accepted: the batch workspace goes, a refused call above keeps it
    eig_free(c);
    if (c->mg && c->mg->cycle == cycle) { c->mg->kind = kind; return MI355CG_OK; }   // both kinds have a hierarchy here: it is the same one
    // another precision: the levels' vectors and the coarse inverse change type.  mg_build replaces the old hierarchy only once
    // the new one is complete, so a failure keeps it.
    if (c->mg) HIPCK(hipStreamSynchronize(c->stream));
    return mg_build(c, kind, c->mg, cycle);
}

// The smoother of the fp64 V-cycle.  With a hierarchy the levels' line tables are built or freed in place;
// without one the value waits for the next mi355cg_set_preconditioner*.  A refusal or a failed upload leaves the handle as it was.
int mi355cg_set_smoother(mi355cg_handle c, int smoother) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    if (smoother != MI355CG_SMOOTHER_JACOBI && smoother != MI355CG_SMOOTHER_LINE_X && smoother != MI355CG_SMOOTHER_LINE_Y &&
        smoother != MI355CG_SMOOTHER_LINE_AUTO)
        return fail(MI355CG_ERR_INVALID, "unknown smoother %d (MI355CG_SMOOTHER_JACOBI = 0, _LINE_X = 1, _LINE_Y = 2, _LINE_AUTO = 3)", smoother);
    if (c->is_csr) return fail(MI355CG_ERR_INVALID, "the smoother belongs to the multigrid preconditioner: a CSR handle has no grid");
    if (c->is_slab) return fail(MI355CG_ERR_INVALID, "the multigrid preconditioner is single-GPU only: this handle owns one part of a decomposed grid");
    if (c->dtype != MI355CG_F64) return fail(MI355CG_ERR_INVALID, "the multigrid preconditioner is fp64 only: this handle was created with MI355CG_F32_MIXED");
    if (smoother != MI355CG_SMOOTHER_JACOBI && c->mg && c->mg->cycle == MI355CG_CYCLE_F32)
        return fail(MI355CG_ERR_INVALID, "the fp32 V-cycle smooths with point Jacobi only: this handle's preconditioner was set with MI355CG_CYCLE_F32");
    if (c->mg && c->mg->cycle == MI355CG_CYCLE_F64) {
        const int dir = mg_line_direction(c, smoother);
        if (dir != c->mg->line_dir) {
            HIPCK(hipSetDevice(c->device));
            HIPCK(hipStreamSynchronize(c->stream));                // nothing in flight reads the tables
            if (int rc = mg_set_line_tables(c->mg.get(), dir, c->sigma)) return rc;
        }
    }
    c->smoother = smoother;
    return MI355CG_OK;
}

int mi355cg_get_smoother(mi355cg_handle c, int* smoother, int* direction) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    if (smoother) *smoother = c->smoother;
    if (direction) *direction = mg_line_direction(c, c->smoother);
    return MI355CG_OK;
}

int mi355cg_preconditioner_info(mi355cg_handle c, int* kind, int* cycle, int* levels) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    if (kind) *kind = c->mg ? c->mg->kind : MI355CG_PRECOND_NONE;
    if (cycle) *cycle = c->mg ? c->mg->cycle : MI355CG_CYCLE_F64;
    if (levels) *levels = c->mg ? (int)c->mg->lv.size() : 0;
    return MI355CG_OK;
}

// z = M r on host vectors (packed order).  Works on the PCG's q (input) and z (output), which hold nothing between iterations,
// so an iteration callback may call it in the middle of a solve.
int mi355cg_apply_preconditioner(mi355cg_handle c, const double* r, double* z) {
    if (!c || !r || !z) return fail(MI355CG_ERR_INVALID, "null argument");
    if (!c->mg) return fail(MI355CG_ERR_STATE, "no preconditioner is set on this handle (mi355cg_set_preconditioner)");
    HIPCK(hipSetDevice(c->device));
    if (int rc = upload_packed<double>(c, r, c->mg->q)) return rc;
    if (c->mg->cycle == MI355CG_CYCLE_F32) {
        double rmax = 0;
        for (long long i = 0; i < c->pk_len; ++i) rmax = std::max(rmax, std::fabs(r[i]));
        if (int rc = mg_apply32(c, c->mg->q, c->mg->z, rmax)) return rc;
    } else
    mg_vcycle(MgCycle{c, nullptr}, 0, c->mg->q, c->mg->z, nullptr);
    HIPCK(hipGetLastError());
    return download_packed<double>(c, c->mg->z, z);
}

// ---- batched solves: nrhs right-hand sides by one multigrid-PCG loop ----------------------------------------
// warm (the _from entry points): a guess per system, x is in/out; system s gets the bits of set_rhs(b_s); set_initial_guess(x0_s); solve; get_solution.
static int solve_batch_device(mi355cg_ctx* c, const mi355cg_params* prm, int nrhs, const double* b_dev, double* x_dev,
                              const volatile int* stop_flag, mi355cg_results* out, bool warm) {
    if (int rc = batch_check(c, prm, nrhs, b_dev, x_dev, out)) return rc;
    HIPCK(hipSetDevice(c->device));
    if (int rc = mg_batch_ensure(c, nrhs, 0)) return rc;
    return solve_mg_batch(c, prm, nrhs, b_dev, x_dev, stop_flag, out, warm);
}
static int solve_batch_host(mi355cg_ctx* c, const mi355cg_params* prm, int nrhs, const double* b, double* x,
                            const volatile int* stop_flag, mi355cg_results* out, bool warm) {
    if (int rc = batch_check(c, prm, nrhs, b, x, out)) return rc;
    HIPCK(hipSetDevice(c->device));
    if (int rc = mg_batch_ensure(c, nrhs, warm ? 2 * nrhs : nrhs)) return rc;
    // cold: b goes up and x comes down through the same buffer; warm: b in the first half, the guesses (then the solutions) in the second
    const size_t count = (size_t)c->pk_len * (size_t)nrhs;
    return run_staged(c, c->batch->stage, count, warm ? count : 0, b, warm ? x : nullptr, x, [&](const double* b_dev, double* x_dev) {
        return solve_mg_batch(c, prm, nrhs, b_dev, x_dev, stop_flag, out, warm);
    });
}

int mi355cg_solve_batch_device(mi355cg_handle c, const mi355cg_params* prm, int nrhs, const double* b_dev, double* x_dev,
                               const volatile int* stop_flag, mi355cg_results* out) {
    return solve_batch_device(c, prm, nrhs, b_dev, x_dev, stop_flag, out, false);
}
int mi355cg_solve_batch(mi355cg_handle c, const mi355cg_params* prm, int nrhs, const double* b, double* x,
                        const volatile int* stop_flag, mi355cg_results* out) {
    return solve_batch_host(c, prm, nrhs, b, x, stop_flag, out, false);
}
int mi355cg_solve_batch_device_from(mi355cg_handle c, const mi355cg_params* prm, int nrhs, const double* b_dev, double* x_dev,
                                    const volatile int* stop_flag, mi355cg_results* out) {
    return solve_batch_device(c, prm, nrhs, b_dev, x_dev, stop_flag, out, true);
}
int mi355cg_solve_batch_from(mi355cg_handle c, const mi355cg_params* prm, int nrhs, const double* b, double* x,
                             const volatile int* stop_flag, mi355cg_results* out) {
    return solve_batch_host(c, prm, nrhs, b, x, stop_flag, out, true);
}

int mi355cg_batch_release(mi355cg_handle c) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    if (!c->batch && !c->many) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    mg_batch_free(c);
    onchip_many_free(c);
    return MI355CG_OK;
}

// ---- batched on-chip solves: many small systems, one workgroup each ---------------------------------------
// what every entry point refuses before anything is allocated or written (sigma: checked by the caller, once it is in host memory)
static int many_check(mi355cg_ctx* c, const mi355cg_params* prm, int nsys, const void* b, const void* x, const mi355cg_results* out) {
    if (!c || !prm || !b || !x || !out) return fail(MI355CG_ERR_INVALID, "null argument");
    if (int rc = kOnchipBatch.count(nsys)) return rc;
    if (int rc = kOnchipBatch.params(prm)) return rc;
    if (int rc = kOnchipBatch.onchip(c)) return rc;
    return BatchKind::apart(c, nsys, x, b, "x overlaps b");
}
static int many_check_sigma(const double* sigma, int nsys) {
    for (int s = 0; sigma && s < nsys; ++s)
        if (!std::isfinite(sigma[s]) || sigma[s] < 0.0)
            return fail(MI355CG_ERR_INVALID, "shift %g of system %d rejected: sigma must be finite and >= 0 (A - sigma I stays negative definite)", sigma[s], s);
    return MI355CG_OK;
}

// A workspace that is large enough is kept; a larger one replaces it only once it is complete, so a failure leaves the handle as it was.
// stage_vecs: packed vectors per system the host entry point stages (0: a device entry point).
static int onchip_many_ensure(mi355cg_ctx* c, int nsys, int stage_vecs) {
    if (!c->many || c->many->cap < nsys) {
        std::unique_ptr<OnchipManyWs> W(new OnchipManyWs());
        auto failed = [&](const char* what) { return fail(MI355CG_ERR_HIP, "on-chip batch workspace for %d systems: %s allocation failed", nsys, what); };
        constexpr int kSmall = FB_COUNT + 2;
        static_assert(2 * sizeof(CgState) + kSmall * sizeof(double) == kOnchipManySysBytes && 2 * sizeof(int) == kOnchipManyFixedBytes, "onchip_plan.h: the workspace formula");
        if (Buf<double>::device(W->vec, 3 * c->pk_len * nsys)) return failed("vector");
        if (Buf<double>::device(W->small, (long long)kSmall * nsys)) return failed("partials");
        if (Buf<CgState>::device(W->s, nsys) || Buf<CgState>::device(W->summary, nsys)) return failed("state");
        if (Buf<int>::device(W->done, 2)) return failed("counter");
        if (Buf<CgState>::pinned(W->summary_h, nsys) || Buf<double>::pinned(W->small_h, (long long)kSmall * nsys) || Buf<int>::pinned(W->done_h, 2)) return failed("pinned copy");
        W->cap = nsys;
        if (c->many) { W->stage = std::move(c->many->stage); W->stage_cap = c->many->stage_cap; }
        onchip_many_free(c);
        c->many = std::move(W);
    }
    OnchipManyWs* W = c->many.get();
    if ((long long)stage_vecs * nsys > W->stage_cap) {
        HIPCK(hipStreamSynchronize(c->stream));                    // nothing in flight reads the buffer that is replaced
        if (Buf<double>::device(W->stage, stage_vecs * c->pk_len * nsys))
            return fail(MI355CG_ERR_HIP, "on-chip batch staging for %d packed vectors: allocation failed", stage_vecs * nsys);
        W->stage_cap = (long long)stage_vecs * nsys;
    }
    return MI355CG_OK;
}

static const void* onchip_many_kernel(int elems, bool msg) {
    return onchip_dispatch(elems, msg, [](auto e, auto m) { return (const void*)&k_onchip_many<decltype(e)::value, decltype(m)::value>; });
}
// Dynamic LDS above 64 KB is opt-in per kernel.
static int onchip_many_allow_lds(const void* kernel, int lds) {
    if (lds > 64 * 1024) HIPCK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    return MI355CG_OK;
}

// One call of mi355cg_solve_many* or mi355cg_time_steps_many* on the handle's OnchipManyWs: everything the two have in common.  A
// caller supplies the diagonals, its start kernel, how long a launch is and what a finished member reports, in this order:
//   open;  host.diag[s] = ...;  upload_diag;  reset_done;  [its own resets];  start(its start kernel);  begin_loop;
//   while (more()) { its cap test;  a.m or its own budget;  launch_and_poll(its chunk kernel) }
//   end_loop;  [its own read-backs];  finish;  out[s] from fin(s) and the mirrors;  stamp_times.
namespace {
struct OnchipManyRun {
    mi355cg_ctx* c; OnchipManyWs* W; const volatile int* stop_flag;
    std::chrono::steady_clock::time_point t0;
    OnchipPlan pl; RuleParams rp; bool msg;
    int nsys, lds;
    long long U, count;                          // ONE stride for the caller's packed vectors and the workspace's; doubles of nsys vectors
    OnchipSmallView dev, host;                   // W->small and its pinned mirror
    double* x; double* r; double* p;             // W->vec
    OnchipManyArgs a;                            // the chunk's arguments, complete but for m (begin_loop)
    bool polled, interrupted;                    // a poll has brought the counter back; the host's stop flag ended the loop

    int open(mi355cg_ctx* c_, const mi355cg_params* prm, int nsys_, const volatile int* stop_flag_, const char* what) {
        t0 = std::chrono::steady_clock::now();
        c = c_; W = c->many.get(); stop_flag = stop_flag_; nsys = nsys_;
        pl = onchip_plan(c->gp.n); rp = make_cfg(prm).rp; msg = prm->rule == MI355CG_RULE_MSG_MAXNORM;
        if (c->pk_len != pl.unknowns) return fail(MI355CG_ERR_STATE, "on-chip %s: the handle packs %lld unknowns, the plan of N = %d has %d", what, c->pk_len, pl.n, pl.unknowns);
        U = pl.unknowns; count = U * nsys; lds = onchip_many_lds_bytes(pl.n);
        dev = onchip_small_view(W->small, nsys); host = onchip_small_view(W->small_h, nsys);
        x = W->vec; r = x + count; p = x + 2 * count;
        polled = interrupted = false;
        return MI355CG_OK;
    }
    int upload_diag() { HIPCK(hipMemcpyAsync(dev.diag, host.diag, sizeof(double) * nsys, hipMemcpyHostToDevice, c->stream)); return MI355CG_OK; }
    int reset_done() { HIPCK(hipMemsetAsync(W->done, 0, sizeof(int) * 2, c->stream)); W->done_h[0] = 0; return MI355CG_OK; }
    int allow_lds(const void* kernel) const { return onchip_many_allow_lds(kernel, lds); }
    int launch(const void* kernel, void** args) { HIPCK(hipLaunchKernel(kernel, dim3(nsys), dim3(pl.threads), args, lds, c->stream)); return MI355CG_OK; }
    int start(const void* kernel, void** args) { if (int rc = allow_lds(kernel)) return rc; return launch(kernel, args); }
    int poll() {                                                   // one word per chunk: how many systems are done
        HIPCK(hipMemcpyAsync(W->done_h, W->done, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        polled = true;
        return wait_stream_forwarding_stop(c, stop_flag);
    }
    // After the start kernel.  The stop request: sampled by every workgroup once per iteration, forwarded by this thread while it
    // waits (as in mi355cg_solve).  start_tested: the start kernel has tested the start states, so they are polled before the loop.
    int begin_loop(bool start_tested) {
        *c->stop_h = 0;
        int* stop_dev = nullptr;
        if (stop_flag) HIPCK(hipHostGetDevicePointer((void**)&stop_dev, c->stop_h, 0));
        a = OnchipManyArgs{};
        a.pl = pl; a.xk = c->g.xk; a.yk = c->g.yk; a.diag = dev.diag;
        a.x = x; a.r = r; a.p = p; a.stride = U;
        a.partB = dev.partB; a.s = W->s; a.summary = W->summary; a.done_count = W->done; a.rp = rp; a.stop_req = stop_dev;
        if (start_tested) if (int rc = poll()) return rc;
        return loop_timer_begin(c, c->stream);
    }
    bool more() {                                                  // false: every system is done, or the host asks to stop
        if (W->done_h[0] >= nsys) return false;
        if (stop_flag && *stop_flag) { interrupted = true; return false; }
        return true;
    }
    int unfinished() const { return nsys - W->done_h[0]; }
    int launch_and_poll(const void* kernel, void** args) { if (int rc = launch(kernel, args)) return rc; return poll(); }
    // a call stopped before anything was polled reports the empty state, as a single solve does; with_norm0: ||r0||_2 is not the state's r0norm
    int end_loop(bool with_norm0) {
        if (int rc = loop_timer_end(c, c->stream)) return rc;
        if (polled) {
            HIPCK(hipMemcpyAsync(W->summary_h, W->summary, sizeof(CgState) * nsys, hipMemcpyDeviceToHost, c->stream));
            if (with_norm0) HIPCK(hipMemcpyAsync(host.norm0, dev.norm0, sizeof(double) * nsys, hipMemcpyDeviceToHost, c->stream));
        }
        return MI355CG_OK;
    }
    int finish(double* x_out) {                                    // the solutions to the caller; every read-back has landed on return
        HIPCK(hipMemcpyAsync(x_out, x, sizeof(double) * count, hipMemcpyDeviceToDevice, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        return MI355CG_OK;
    }
    CgState fin(int s) const { return polled ? W->summary_h[s] : CgState{}; }
    int stamp_times(mi355cg_results* out) {
        HIPCK(hipEventSynchronize(c->ev_loop[1]));
        const double loop_seconds = loop_timer_seconds(c);
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        for (int s = 0; s < nsys; ++s) { out[s].loop_seconds = loop_seconds; out[s].solve_seconds = secs; }
        return MI355CG_OK;
    }
};
}  // namespace

// b_dev, x_dev: nsys packed vectors each in device memory (x_dev: the guesses when warm); sigma: host memory or NULL, checked.
static int solve_many(mi355cg_ctx* c, const mi355cg_params* prm, int nsys, const double* b_dev, double* x_dev, const double* sigma,
                      const volatile int* stop_flag, mi355cg_results* out, bool warm) {
    OnchipManyRun R;
    if (int rc = R.open(c, prm, nsys, stop_flag, "batch")) return rc;
    const OnchipManyWs* W = R.W;
    for (int s = 0; s < nsys; ++s) R.host.diag[s] = sigma ? c->gp.A - sigma[s] : c->g.A;          // mi355cg_set_shift's rounding
    if (int rc = R.upload_diag()) return rc;
    if (int rc = R.reset_done()) return rc;

    OnchipManyInitArgs ia{};
    ia.pl = R.pl; ia.xk = c->g.xk; ia.yk = c->g.yk; ia.diag = R.dev.diag; ia.b = b_dev; ia.x0 = warm ? x_dev : nullptr;
    ia.x = R.x; ia.r = R.r; ia.p = R.p; ia.stride = R.U;
    ia.partB = R.dev.partB; ia.s = W->s; ia.summary = W->summary; ia.norm0 = R.dev.norm0; ia.done_count = W->done; ia.rp = R.rp;
    { void* args[] = {&ia}; if (int rc = R.start(warm ? (const void*)&k_onchip_many_init<true> : (const void*)&k_onchip_many_init<false>, args)) return rc; }
    if (int rc = R.begin_loop(R.msg && warm)) return rc;           // the start states of a warm MSG batch were tested (k_onchip_many_init)

    const void* k_chunk = onchip_many_kernel(R.pl.elems, R.msg);
    if (int rc = R.allow_lds(k_chunk)) return rc;
    const int sync_every = default_sync_every(prm, R.msg);
    void* args[] = {&R.a};
    for (int it_done = 0; R.more(); it_done += R.a.m) {
        if (it_done > prm->max_iterations) return fail(MI355CG_ERR_HIP, "on-chip batch: %d of %d systems still iterate past the iteration cap", R.unfinished(), nsys);
        R.a.m = chunk_len(prm, R.msg, sync_every, it_done, false);
        if (int rc = R.launch_and_poll(k_chunk, args)) return rc;
    }
    if (int rc = R.end_loop(warm)) return rc;
    if (int rc = R.finish(x_dev)) return rc;
    for (int s = 0; s < nsys; ++s) {
        const CgState fin = R.fin(s);
        const bool intr = (R.interrupted && !fin.done) || (fin.done && fin.reason == MI355CG_STOP_INTERRUPTED);
        out[s] = make_results(fin, intr, false, warm && R.polled ? R.host.norm0[s] : fin.r0norm);
    }
    return R.stamp_times(out);
}

static int solve_many_device(mi355cg_ctx* c, const mi355cg_params* prm, int nsys, const double* b_dev, double* x_dev, const double* sigma_dev,
                             const volatile int* stop_flag, mi355cg_results* out, bool warm) {
    if (int rc = many_check(c, prm, nsys, b_dev, x_dev, out)) return rc;
    HIPCK(hipSetDevice(c->device));
    std::vector<double> sigma;
    if (sigma_dev) {
        sigma.resize(nsys);
        HIPCK(hipMemcpy(sigma.data(), sigma_dev, sizeof(double) * nsys, hipMemcpyDeviceToHost));
        if (int rc = many_check_sigma(sigma.data(), nsys)) return rc;
    }
    if (int rc = onchip_many_ensure(c, nsys, 0)) return rc;
    return solve_many(c, prm, nsys, b_dev, x_dev, sigma_dev ? sigma.data() : nullptr, stop_flag, out, warm);
}
static int solve_many_host(mi355cg_ctx* c, const mi355cg_params* prm, int nsys, const double* b, double* x, const double* sigma,
                           const volatile int* stop_flag, mi355cg_results* out, bool warm) {
    if (int rc = many_check(c, prm, nsys, b, x, out)) return rc;
    if (int rc = many_check_sigma(sigma, nsys)) return rc;
    HIPCK(hipSetDevice(c->device));
    if (int rc = onchip_many_ensure(c, nsys, 2)) return rc;
    const size_t count = (size_t)c->pk_len * (size_t)nsys;         // b in the first half, the guesses / the solutions in the second
    return run_staged(c, c->many->stage, count, count, b, warm ? x : nullptr, x, [&](const double* b_dev, double* x_dev) {
        return solve_many(c, prm, nsys, b_dev, x_dev, sigma, stop_flag, out, warm);
    });
}

int mi355cg_solve_many(mi355cg_handle c, const mi355cg_params* prm, int nsys, const double* b, double* x, const double* sigma,
                       const volatile int* stop_flag, mi355cg_results* out) {
    return solve_many_host(c, prm, nsys, b, x, sigma, stop_flag, out, false);
}
int mi355cg_solve_many_from(mi355cg_handle c, const mi355cg_params* prm, int nsys, const double* b, double* x, const double* sigma,
                            const volatile int* stop_flag, mi355cg_results* out) {
    return solve_many_host(c, prm, nsys, b, x, sigma, stop_flag, out, true);
}
int mi355cg_solve_many_device(mi355cg_handle c, const mi355cg_params* prm, int nsys, const double* b_dev, double* x_dev, const double* sigma_dev,
                              const volatile int* stop_flag, mi355cg_results* out) {
    return solve_many_device(c, prm, nsys, b_dev, x_dev, sigma_dev, stop_flag, out, false);
}
int mi355cg_solve_many_device_from(mi355cg_handle c, const mi355cg_params* prm, int nsys, const double* b_dev, double* x_dev, const double* sigma_dev,
                                   const volatile int* stop_flag, mi355cg_results* out) {
    return solve_many_device(c, prm, nsys, b_dev, x_dev, sigma_dev, stop_flag, out, true);
}

int mi355cg_solve_many_info(mi355cg_handle c, int nsys, int* lds_bytes_per_workgroup, int* workgroups_per_cu, long long* workspace_bytes) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    if (int rc = kOnchipBatch.count(nsys)) return rc;
    if (int rc = kOnchipBatch.onchip(c)) return rc;
    const OnchipPlan pl = onchip_plan(c->gp.n);
    const int lds = onchip_many_lds_bytes(pl.n);
    if (lds_bytes_per_workgroup) *lds_bytes_per_workgroup = lds;
    if (workspace_bytes) *workspace_bytes = onchip_many_workspace_bytes(pl.n, nsys);
    if (workgroups_per_cu) {
        HIPCK(hipSetDevice(c->device));
        const void* k = onchip_many_kernel(pl.elems, false);
        if (int rc = onchip_many_allow_lds(k, lds)) return rc;
        int nb = 0;
        HIPCK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, pl.threads, (size_t)lds));
        *workgroups_per_cu = nb;
    }
    return MI355CG_OK;
}

// ---- ensemble time stepping on chip: the step loop inside the launch -----------------------------------------
static_assert(MI355CG_MANY_MAX == kOnchipStepsMaxSys && MI355CG_STEPS_MANY_MAX_STEPS == kOnchipStepsMaxSteps, "onchip_plan.h: the limits of an ensemble");
// The refusals the theta and the wave steppers share, each written once; a check runs them in its own order, among its own.
struct StepChecks {
    static int nsteps(int nsteps) {
        return nsteps < 0 || nsteps > MI355CG_STEPS_MANY_MAX_STEPS ? fail(MI355CG_ERR_INVALID, "nsteps %d rejected: it must be 0 .. %d", nsteps, MI355CG_STEPS_MANY_MAX_STEPS) : MI355CG_OK;
    }
    static int counts(const int* step_iterations, int nsys, int nsteps) {
        if (step_iterations && (long long)nsys * nsteps > kOnchipStepsMaxCounts)
            return fail(MI355CG_ERR_INVALID, "step_iterations for %d members x %d steps rejected: at most %lld counts", nsys, nsteps, kOnchipStepsMaxCounts);
        return MI355CG_OK;
    }
    static int tau(double tau, int s) {
        return !std::isfinite(tau) || !(tau > 0.0) ? fail(MI355CG_ERR_INVALID, "time step %g of member %d rejected: tau must be finite and > 0", tau, s) : MI355CG_OK;
    }
    static int forcing_apart(const mi355cg_ctx* c, int nsys, const void* u, const void* g) { return g ? BatchKind::apart(c, nsys, u, g, "u overlaps g") : MI355CG_OK; }
    // after the check: a call of no steps is over, nothing is selected, allocated or launched
    static bool none(int nsys, int nsteps, int* steps_done) {
        if (nsteps == 0) for (int s = 0; s < nsys; ++s) steps_done[s] = 0;
        return nsteps == 0;
    }
};
// what both entry points refuse before anything is allocated or written (tau is in host memory for both)
static int steps_many_check(mi355cg_ctx* c, const mi355cg_params* prm, int nsys, int nsteps, double theta, const double* tau, const void* g,
                            const void* u, const mi355cg_results* out, const int* steps_done, const int* step_iterations) {
    if (!c || !prm || !tau || !u || !out || !steps_done) return fail(MI355CG_ERR_INVALID, "null argument");
    if (int rc = kEnsemble.count(nsys)) return rc;
    if (int rc = StepChecks::nsteps(nsteps)) return rc;
    if (int rc = StepChecks::counts(step_iterations, nsys, nsteps)) return rc;
    if (!(theta > 0.0 && theta <= 1.0)) return fail(MI355CG_ERR_INVALID, "theta %g rejected: the scheme needs 0 < theta <= 1", theta);
    if (int rc = kEnsemble.params(prm)) return rc;
    if (int rc = kEnsemble.onchip(c)) return rc;
    for (int s = 0; s < nsys; ++s) {
        if (int rc = StepChecks::tau(tau[s], s)) return rc;
        if (!std::isfinite(1.0 / (theta * tau[s]))) return fail(MI355CG_ERR_INVALID, "time step %g of member %d rejected: 1 / (theta tau) is not finite", tau[s], s);
    }
    return StepChecks::forcing_apart(c, nsys, u, g);
}

// The handle's right-hand side, packed, as the forcing of every member when the caller gives none: where it is allocated (false:
// it is there) and the launch that fills it.
static bool g_one_alloc_failed(mi355cg_ctx* c) { return !c->many->g_one && Buf<double>::device(c->many->g_one, c->pk_len); }
static int g_one_pack(mi355cg_ctx* c) {
    hipLaunchKernelGGL((k_pack<double>), dim3(flat_grid(c->pk_len)), dim3(kBlock), 0, c->stream, c->pg, (const double*)c->b, c->many->g_one.get());
    HIPCK(hipGetLastError());
    return MI355CG_OK;
}

// The batch workspace for nsys members, then the stepping parts on top: built complete before they replace what is there.
static int onchip_steps_ensure(mi355cg_ctx* c, int nsys, long long counts, int stage_vecs) {
    if (int rc = onchip_many_ensure(c, nsys, stage_vecs)) return rc;
    OnchipManyWs* W = c->many.get();
    auto failed = [&](const char* what) { return fail(MI355CG_ERR_HIP, "on-chip stepping workspace for %d members: %s allocation failed", nsys, what); };
    if (W->steps_cap < nsys) {
        Buf<double> sigma, sigma_h; Buf<OcStepBook> book, book_h; Buf<CgState> s_h;
        if (Buf<double>::device(sigma, nsys) || Buf<OcStepBook>::device(book, nsys)) return failed("bookkeeping");
        if (g_one_alloc_failed(c)) return failed("vector");
        if (Buf<double>::pinned(sigma_h, nsys) || Buf<OcStepBook>::pinned(book_h, nsys) || Buf<CgState>::pinned(s_h, nsys)) return failed("pinned copy");
        HIPCK(hipStreamSynchronize(c->stream));
        W->step_sigma = std::move(sigma); W->book = std::move(book);
        W->step_sigma_h = std::move(sigma_h); W->book_h = std::move(book_h); W->s_h = std::move(s_h);
        W->steps_cap = nsys;
    }
    if (counts > W->step_it_cap) {
        HIPCK(hipStreamSynchronize(c->stream));
        if (Buf<int>::device(W->step_it, counts)) return failed("iteration count");
        W->step_it_cap = counts;
    }
    return MI355CG_OK;
}

// One call of an implicit stepper -- the theta scheme, or Newmark -- on the handle's OnchipManyWs: the step loop
// inside the launches (oc_step_loop), written once on the host too.  g_dev (or NULL): nsys packed vectors in device memory;
// nsteps >= 1.  Args is the scheme's argument struct; the fields every scheme has are filled here.  A scheme supplies
//   label        what the failure texts call it;
//   sigma(s)     member s's shift; its diagonal is A - sigma as mi355cg_set_shift rounds it;
//   upload()     what else it sends ahead, behind the shifts and in front of the resets;
//   prepare(e)    behind the resets: its own fields of e, and what it still has to put on the stream in front of the start;
//   k_init, chunk_kernel(elems, msg)   its start kernel and its instantiation of the step loop;
//   deliver(R, e)   behind the read-backs: the state to the caller; every read-back has landed on return.
extern "C++" {                                                     // (a template among the C entry points)
template <class Args, class Sigma, class Upload, class Prepare, class Deliver>
static int implicit_steps(mi355cg_ctx* c, const mi355cg_params* prm, int nsys, int nsteps, const double* g_dev, const volatile int* stop_flag,
                          mi355cg_results* out, int* steps_done, int* step_iterations, const char* label, Sigma sigma, Upload upload,
                          Prepare prepare, const void* k_init, const void* (*chunk_kernel)(int, bool), Deliver deliver) {
    OnchipManyRun R;
    if (int rc = R.open(c, prm, nsys, stop_flag, label)) return rc;
    OnchipManyWs* W = R.W;
    const bool msg = R.msg;
    const long long counts = step_iterations ? (long long)nsys * nsteps : 0;
    for (int s = 0; s < nsys; ++s) {
        W->step_sigma_h[s] = sigma(s);
        R.host.diag[s] = c->gp.A - W->step_sigma_h[s];               // mi355cg_set_shift's rounding
    }
    if (int rc = R.upload_diag()) return rc;
    HIPCK(hipMemcpyAsync(W->step_sigma, W->step_sigma_h, sizeof(double) * nsys, hipMemcpyHostToDevice, c->stream));
    if (int rc = upload()) return rc;
    if (int rc = R.reset_done()) return rc;
    HIPCK(hipMemsetAsync(W->book, 0, sizeof(OcStepBook) * nsys, c->stream));
    if (counts) HIPCK(hipMemsetAsync(W->step_it, 0xff, sizeof(int) * counts, c->stream));              // -1: not taken

    Args e{};
    e.pl = R.pl; e.xk = c->g.xk; e.yk = c->g.yk; e.diag = R.dev.diag; e.sigma = W->step_sigma;
    e.g = g_dev ? g_dev : W->g_one.get(); e.g_stride = g_dev ? R.U : 0;
    e.x = R.x; e.r = R.r; e.p = R.p; e.stride = R.U;
    e.partB = R.dev.partB; e.s = W->s; e.summary = W->summary; e.norm0 = R.dev.norm0; e.done_count = W->done;
    e.book = W->book; e.step_it = counts ? W->step_it.get() : nullptr; e.nsteps = nsteps;
    e.rp = R.rp;
    if (int rc = prepare(e)) return rc;
    { void* args[] = {&e}; if (int rc = R.start(k_init, args)) return rc; }
    if (int rc = R.begin_loop(msg)) return rc;                     // the start states were tested, as mi355cg_solve polls a warm MSG start

    const void* k_chunk = chunk_kernel(R.pl.elems, msg);
    if (int rc = R.allow_lds(k_chunk)) return rc;
    e.m = default_sync_every(prm, msg);                            // units per member and launch: an iteration or a transition each
    const long long max_launches = onchip_steps_launch_cap(nsteps, prm->max_iterations, e.m);
    void* args[] = {&R.a, &e};
    for (long long launches = 0; R.more(); ++launches) {
        if (launches >= max_launches) return fail(MI355CG_ERR_HIP, "on-chip %s: %d of %d members still step after %lld launches", label, R.unfinished(), nsys, launches);
        if (int rc = R.launch_and_poll(k_chunk, args)) return rc;
    }
    if (int rc = R.end_loop(true)) return rc;
    HIPCK(hipMemcpyAsync(W->book_h, W->book, sizeof(OcStepBook) * nsys, hipMemcpyDeviceToHost, c->stream));
    if (!msg) HIPCK(hipMemcpyAsync(R.host.partB, R.dev.partB, sizeof(double) * FB_COUNT * nsys, hipMemcpyDeviceToHost, c->stream));     // |r| of the last update
    if (R.interrupted) HIPCK(hipMemcpyAsync(W->s_h, W->s, sizeof(CgState) * nsys, hipMemcpyDeviceToHost, c->stream));
    if (int rc = deliver(R, e)) return rc;
    if (counts) HIPCK(hipMemcpy(step_iterations, W->step_it, sizeof(int) * counts, hipMemcpyDeviceToHost));
    for (int s = 0; s < nsys; ++s) {                               // onchip_plan.h: what a member reports
        const OcStepReport rep = onchip_step_report(prm, msg, R.polled, R.interrupted, W->book_h[s], W->summary_h[s], W->s_h[s], R.host.norm0[s],
                                                    R.host.partB[(long long)s * FB_COUNT + FB_RMAX], e.m, stop_flag != nullptr);
        steps_done[s] = rep.steps_done;
        out[s] = rep.res;
        if (counts && rep.patch_step >= 0) step_iterations[(long long)s * nsteps + rep.patch_step] = rep.patch_iterations;
    }
    return R.stamp_times(out);
}
}  // extern "C++"

// g_dev (or NULL), u_dev: nsys packed vectors each in device memory; tau: host memory, checked; nsteps >= 1.
static int steps_many(mi355cg_ctx* c, const mi355cg_params* prm, int nsys, int nsteps, double theta, const double* tau, const double* g_dev,
                      double* u_dev, const volatile int* stop_flag, mi355cg_results* out, int* steps_done, int* step_iterations) {
    return implicit_steps<OnchipStepsArgs>(
        c, prm, nsys, nsteps, g_dev, stop_flag, out, steps_done, step_iterations, "stepping",
        [&](int s) { return 1.0 / (theta * tau[s]); },            // mi355cg_time_steps's shift, in that form
        [] { return MI355CG_OK; },
        [&](OnchipStepsArgs& e) {
            e.u0 = u_dev;
            e.k = OnchipStepCoef{c->gp.A, c->gp.x_k, c->gp.y_k, theta, (1.0 - theta) / theta, theta < 1.0 ? 1 : 0};       // launch_step_rhs's
            return g_dev ? MI355CG_OK : g_one_pack(c);             // the handle's right-hand side for every member
        },
        (const void*)&k_onchip_steps_init,
        [](int elems, bool msg) { return onchip_dispatch(elems, msg, [](auto el, auto m) { return (const void*)&k_onchip_steps<decltype(el)::value, decltype(m)::value>; }); },
        [&](OnchipManyRun& R, OnchipStepsArgs&) { return R.finish(u_dev); });
}

int mi355cg_time_steps_many_device(mi355cg_handle c, const mi355cg_params* prm, int nsys, int nsteps, double theta, const double* tau,
                                   const double* g_dev, double* u_dev, const volatile int* stop_flag, mi355cg_results* out, int* steps_done,
                                   int* step_iterations) {
    if (int rc = steps_many_check(c, prm, nsys, nsteps, theta, tau, g_dev, u_dev, out, steps_done, step_iterations)) return rc;
    if (StepChecks::none(nsys, nsteps, steps_done)) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    if (int rc = onchip_steps_ensure(c, nsys, step_iterations ? (long long)nsys * nsteps : 0, 0)) return rc;
    return steps_many(c, prm, nsys, nsteps, theta, tau, g_dev, u_dev, stop_flag, out, steps_done, step_iterations);
}
int mi355cg_time_steps_many(mi355cg_handle c, const mi355cg_params* prm, int nsys, int nsteps, double theta, const double* tau, const double* g,
                            double* u, const volatile int* stop_flag, mi355cg_results* out, int* steps_done, int* step_iterations) {
    if (int rc = steps_many_check(c, prm, nsys, nsteps, theta, tau, g, u, out, steps_done, step_iterations)) return rc;
    if (StepChecks::none(nsys, nsteps, steps_done)) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    if (int rc = onchip_steps_ensure(c, nsys, step_iterations ? (long long)nsys * nsteps : 0, 2)) return rc;
    const size_t count = (size_t)c->pk_len * (size_t)nsys;         // g in the first half, the states in the second
    return run_staged(c, c->many->stage, count, count, g, u, u, [&](const double* g_dev, double* u_dev) {
        return steps_many(c, prm, nsys, nsteps, theta, tau, g ? g_dev : nullptr, u_dev, stop_flag, out, steps_done, step_iterations);
    });
}
int mi355cg_time_steps_many_workspace(int n, int nsys, int nsteps, int with_step_iterations, long long* bytes) {
    if (!bytes) return fail(MI355CG_ERR_INVALID, "null argument");
    const long long v = onchip_steps_workspace_bytes(n, nsys, nsteps, with_step_iterations);
    if (v == 0)
        return fail(MI355CG_ERR_INVALID, "ensemble rejected: even n from 6 to %d, 1 .. %d members, 0 .. %d steps, at most %lld iteration counts",
                    kOnchipMaxN, kOnchipStepsMaxSys, kOnchipStepsMaxSteps, kOnchipStepsMaxCounts);
    *bytes = v;
    return MI355CG_OK;
}

// ---- ensemble wave-equation steps on chip: velocity Verlet and Newmark ---------------------------------------
static_assert(MI355CG_WAVE_VERLET == kWaveVerlet && MI355CG_WAVE_NEWMARK == kWaveNewmark && MI355CG_WAVE_MAX_RECEIVERS == kOnchipWaveMaxRec, "onchip_plan.h: the schemes, the receivers");
// what both entry points refuse before anything is allocated or written (tau is in host memory for both)
static int wave_check(mi355cg_ctx* c, const mi355cg_params* prm, int nsys, int nsteps, int scheme, const double* tau, const void* g, const void* u,
                      const void* v, int steps_per_launch, const mi355cg_results* out, const int* steps_done, const int* step_iterations,
                      bool own_bound = false) {                    // a call in a medium tests every member against its own bound (wave_medium_bounds)
    if (!c || !tau || !u || !v || !out || !steps_done) return fail(MI355CG_ERR_INVALID, "null argument");
    if (scheme != MI355CG_WAVE_VERLET && scheme != MI355CG_WAVE_NEWMARK) return fail(MI355CG_ERR_INVALID, "unknown wave scheme %d", scheme);
    const bool newmark = scheme == MI355CG_WAVE_NEWMARK;
    if (newmark && !prm) return fail(MI355CG_ERR_INVALID, "null argument: the Newmark scheme reads params");
    if (int rc = kWaveEnsemble.count(nsys)) return rc;
    if (int rc = StepChecks::nsteps(nsteps)) return rc;
    if (steps_per_launch < 0) return fail(MI355CG_ERR_INVALID, "steps_per_launch %d rejected: 0 (the default) or a positive number of steps", steps_per_launch);
    if (newmark) if (int rc = StepChecks::counts(step_iterations, nsys, nsteps)) return rc;
    if (newmark) if (int rc = kWaveEnsemble.params(prm)) return rc;
    if (int rc = kWaveEnsemble.onchip(c)) return rc;
    const double bound = onchip_wave_cfl(c->gp.A);
    for (int s = 0; s < nsys; ++s) {
        if (int rc = StepChecks::tau(tau[s], s)) return rc;
        if (newmark && !std::isfinite(4.0 / (tau[s] * tau[s]))) return fail(MI355CG_ERR_INVALID, "time step %g of member %d rejected: 4 / tau^2 is not finite", tau[s], s);
        if (!newmark && !own_bound && tau[s] > bound)
            return fail(MI355CG_ERR_INVALID, "time step %.17g of member %d rejected: velocity Verlet needs tau <= %.17g on this grid (mi355cg_wave_cfl); MI355CG_WAVE_NEWMARK has no bound",
                        tau[s], s, bound);
    }
    if (int rc = BatchKind::apart(c, nsys, u, v, "u overlaps v")) return rc;
    if (int rc = StepChecks::forcing_apart(c, nsys, u, g)) return rc;
    return g ? BatchKind::apart(c, nsys, v, g, "v overlaps g") : MI355CG_OK;
}

// The workspace of the scheme's driver, then the wave parts on top: built complete before they replace what is there.
static int onchip_wave_ensure(mi355cg_ctx* c, int nsys, int scheme, long long counts, int stage_vecs) {
    if (int rc = scheme == MI355CG_WAVE_NEWMARK ? onchip_steps_ensure(c, nsys, counts, stage_vecs) : onchip_many_ensure(c, nsys, stage_vecs)) return rc;
    OnchipManyWs* W = c->many.get();
    auto failed = [&](const char* what) { return fail(MI355CG_ERR_HIP, "on-chip wave stepping workspace for %d members: %s allocation failed", nsys, what); };
    if (W->wave_cap < nsys) {
        Buf<double> tau, tau_h;
        if (Buf<double>::device(tau, 2LL * nsys)) return failed("time step");
        if (Buf<double>::pinned(tau_h, 2LL * nsys)) return failed("pinned copy");
        HIPCK(hipStreamSynchronize(c->stream));
        W->wave_tau = std::move(tau); W->wave_tau_h = std::move(tau_h);
        W->wave_cap = nsys;
    }
    if (g_one_alloc_failed(c)) return failed("vector");
    return MI355CG_OK;
}

// tau_s and 2 / tau_s of every member to the device; the handle's right-hand side, packed, when no forcing is given
static int wave_upload(mi355cg_ctx* c, OnchipManyWs* W, int nsys, const double* tau, const double* g_dev) {
    for (int s = 0; s < nsys; ++s) { W->wave_tau_h[s] = tau[s]; W->wave_tau_h[nsys + s] = 2.0 / tau[s]; }
    HIPCK(hipMemcpyAsync(W->wave_tau, W->wave_tau_h, sizeof(double) * 2 * nsys, hipMemcpyHostToDevice, c->stream));
    return g_dev ? MI355CG_OK : g_one_pack(c);
}

// What mi355cg_wave_record_many* adds to an explicit call: w and traces in device memory, nodes (the packed
// indices of the receivers) in host memory; w_stride 0: one row of amplitudes for all members.
// c2 (or NULL: none): the media of mi355cg_wave_medium_many* (section 12.5) in device memory; c2_stride 0: one for all members.
// d (or NULL: none; with c2 only): the damping rows of mi355cg_wave_sponge_many* (section 12.6), likewise.
struct WaveRecord { const double* w; long long w_stride; int nrec; const int* nodes; int every; double* traces; const double* c2 = nullptr; long long c2_stride = 0;
                    const double* d = nullptr; long long d_stride = 0;
                    double* hist = nullptr; long long hist_stride = 0; };     // hist (with c2, without d): the history of mi355cg_wave_history_many* (section 12.7)

// Explicit: ceil(nsteps / m) launches of m steps; before each the host waits for the one before it and tests the caller's flag.
// rec: with a source and receivers; every launch is told where in the call it starts.
static int wave_verlet(mi355cg_ctx* c, int nsys, int nsteps, const double* tau, const double* g_dev, double* u_dev, double* v_dev,
                       int steps_per_launch, const volatile int* stop_flag, mi355cg_results* out, int* steps_done, const WaveRecord* rec = nullptr) {
    mi355cg_params none;                                           // the driver reads a rule; the scheme decides nothing
    mi355cg_default_params(&none, MI355CG_RULE_REL_2NORM);
    OnchipManyRun R;
    if (int rc = R.open(c, &none, nsys, stop_flag, "wave stepping")) return rc;
    OnchipManyWs* W = R.W;
    if (int rc = wave_upload(c, W, nsys, tau, g_dev)) return rc;
    OnchipWaveArgs a{};
    a.pl = R.pl; a.k = OnchipWaveCoef{c->gp.A, c->gp.x_k, c->gp.y_k};
    a.tau = W->wave_tau; a.g = g_dev ? g_dev : W->g_one.get(); a.g_stride = g_dev ? R.U : 0;
    a.u = u_dev; a.v = v_dev; a.stride = R.U;
    OnchipWaveRecArgs x{};
    if (rec) {
        for (int r = 0; r < rec->nrec; ++r) { int xx, yy; onchip_node(R.pl, rec->nodes[r], &xx, &yy); W->rec_cell_h[r] = onchip_cell(R.pl, xx, yy); }
        if (rec->nrec) HIPCK(hipMemcpyAsync(W->rec_cell, W->rec_cell_h, sizeof(int) * rec->nrec, hipMemcpyHostToDevice, c->stream));
        x.w = rec->w; x.w_stride = rec->w_stride; x.rec_cell = W->rec_cell; x.nrec = rec->nrec; x.every = rec->every;
        x.traces = rec->traces; x.tr_stride = (long long)(nsteps / rec->every) * rec->nrec;
    }
    const OnchipWaveMediumArgs md{rec ? rec->c2 : nullptr, rec ? rec->c2_stride : 0};
    const OnchipWaveSpongeArgs sp{rec ? rec->d : nullptr, rec ? rec->d_stride : 0};
    const OnchipWaveHistArgs hs{rec ? rec->hist : nullptr, rec ? rec->hist_stride : 0};
    const void* k_steps = hs.hist ? onchip_dispatch(R.pl.elems, false, [](auto el, auto) { return (const void*)&k_oc_wave_history<decltype(el)::value>; })
                          : sp.d  ? onchip_dispatch(R.pl.elems, false, [](auto el, auto) { return (const void*)&k_oc_wave_sponge<decltype(el)::value>; })
                          : md.c2 ? onchip_dispatch(R.pl.elems, false, [](auto el, auto) { return (const void*)&k_oc_wave_medium<decltype(el)::value>; })
                          : rec ? onchip_dispatch(R.pl.elems, false, [](auto el, auto) { return (const void*)&k_oc_wave_record<decltype(el)::value>; })
                              : onchip_dispatch(R.pl.elems, false, [](auto el, auto) { return (const void*)&k_onchip_wave_verlet<decltype(el)::value>; });
    if (int rc = R.allow_lds(k_steps)) return rc;
    if (int rc = loop_timer_begin(c, c->stream)) return rc;
    const int m = steps_per_launch > 0 ? steps_per_launch : kOnchipWaveDefaultSteps;
    void* args[] = {&a, &x, (void*)&md, hs.hist ? (void*)&hs : (void*)&sp};   // (the plain kernel takes the first alone, the recording one two, the medium's three)
    int done = 0;
    while (done < nsteps) {
        if (done > 0) HIPCK(hipStreamSynchronize(c->stream));
        if (stop_flag && *stop_flag) { R.interrupted = true; break; }
        a.m = std::min(m, nsteps - done);
        if (rec) { x.step0 = done; x.phase = done % rec->every; x.slot = done / rec->every; }
        if (int rc = R.launch(k_steps, args)) return rc;
        done += a.m;
    }
    if (int rc = R.end_loop(false)) return rc;
    HIPCK(hipStreamSynchronize(c->stream));
    CgState fin{};
    fin.done = 1; fin.converged = 1;
    for (int s = 0; s < nsys; ++s) { steps_done[s] = done; out[s] = make_results(fin, R.interrupted, false, 0.0); }
    return R.stamp_times(out);
}

// Implicit: implicit_steps on k_onchip_wave_newmark.  The state moves in u_dev, v_dev themselves.
static int wave_newmark(mi355cg_ctx* c, const mi355cg_params* prm, int nsys, int nsteps, const double* tau, const double* g_dev, double* u_dev,
                        double* v_dev, const volatile int* stop_flag, mi355cg_results* out, int* steps_done, int* step_iterations) {
    return implicit_steps<OnchipNewmarkArgs>(
        c, prm, nsys, nsteps, g_dev, stop_flag, out, steps_done, step_iterations, "wave stepping",
        [&](int s) { return 4.0 / (tau[s] * tau[s]); },
        [&] { return wave_upload(c, c->many.get(), nsys, tau, g_dev); },
        [&](OnchipNewmarkArgs& e) {
            e.tau = c->many->wave_tau; e.u = u_dev; e.v = v_dev; e.nsys = nsys;
            e.k = OnchipWaveCoef{c->gp.A, c->gp.x_k, c->gp.y_k};
            return MI355CG_OK;
        },
        (const void*)&k_onchip_wave_newmark_init,
        [](int elems, bool msg) { return onchip_dispatch(elems, msg, [](auto el, auto m) { return (const void*)&k_onchip_wave_newmark<decltype(el)::value, decltype(m)::value>; }); },
        [&](OnchipManyRun& R, OnchipNewmarkArgs& e) {
            if (R.interrupted) {
                // A member stopped between two steps has a converged step whose transition waited for a launch that never came.  The report
                // counts that step (onchip_step_report), so its state moves on now: the transition's velocity and state update alone.
                void* fargs[] = {&e};
                if (int rc = R.start((const void*)&k_onchip_wave_newmark_finish, fargs)) return rc;
            }
            HIPCK(hipStreamSynchronize(c->stream));
            return MI355CG_OK;
        });
}

static int wave_steps_many(mi355cg_ctx* c, const mi355cg_params* prm, int nsys, int nsteps, int scheme, const double* tau, const double* g_dev,
                           double* u_dev, double* v_dev, int steps_per_launch, const volatile int* stop_flag, mi355cg_results* out,
                           int* steps_done, int* step_iterations) {
    if (scheme == MI355CG_WAVE_NEWMARK) return wave_newmark(c, prm, nsys, nsteps, tau, g_dev, u_dev, v_dev, stop_flag, out, steps_done, step_iterations);
    return wave_verlet(c, nsys, nsteps, tau, g_dev, u_dev, v_dev, steps_per_launch, stop_flag, out, steps_done);
}

int mi355cg_wave_steps_many_device(mi355cg_handle c, const mi355cg_params* prm, int nsys, int nsteps, int scheme, const double* tau,
                                   const double* g_dev, double* u_dev, double* v_dev, int steps_per_launch, const volatile int* stop_flag,
                                   mi355cg_results* out, int* steps_done, int* step_iterations) {
    if (int rc = wave_check(c, prm, nsys, nsteps, scheme, tau, g_dev, u_dev, v_dev, steps_per_launch, out, steps_done, step_iterations)) return rc;
    if (StepChecks::none(nsys, nsteps, steps_done)) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    if (int rc = onchip_wave_ensure(c, nsys, scheme, step_iterations ? (long long)nsys * nsteps : 0, 0)) return rc;
    return wave_steps_many(c, prm, nsys, nsteps, scheme, tau, g_dev, u_dev, v_dev, steps_per_launch, stop_flag, out, steps_done, step_iterations);
}
int mi355cg_wave_steps_many(mi355cg_handle c, const mi355cg_params* prm, int nsys, int nsteps, int scheme, const double* tau, const double* g,
                            double* u, double* v, int steps_per_launch, const volatile int* stop_flag, mi355cg_results* out, int* steps_done,
                            int* step_iterations) {
    if (int rc = wave_check(c, prm, nsys, nsteps, scheme, tau, g, u, v, steps_per_launch, out, steps_done, step_iterations)) return rc;
    if (StepChecks::none(nsys, nsteps, steps_done)) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    if (int rc = onchip_wave_ensure(c, nsys, scheme, step_iterations ? (long long)nsys * nsteps : 0, 3)) return rc;
    const size_t count = (size_t)c->pk_len * (size_t)nsys;         // g, then u, then v; the state comes down
    double* const g_dev = c->many->stage; double* const u_dev = g_dev + count; double* const v_dev = u_dev + count;
    const StagedGroup groups[3] = {{0, g, nullptr}, {count, u, u}, {2 * count, v, v}};
    return run_staged_groups(c, g_dev, count, groups, [&]() {
        return wave_steps_many(c, prm, nsys, nsteps, scheme, tau, g ? g_dev : nullptr, u_dev, v_dev, steps_per_launch, stop_flag, out, steps_done, step_iterations);
    });
}
int mi355cg_wave_steps_many_workspace(int n, int nsys, int nsteps, int scheme, int with_step_iterations, long long* bytes) {
    if (!bytes) return fail(MI355CG_ERR_INVALID, "null argument");
    const long long v = onchip_wave_workspace_bytes(n, nsys, nsteps, scheme, with_step_iterations);
    if (v == 0)
        return fail(MI355CG_ERR_INVALID, "wave ensemble rejected: even n from 6 to %d, 1 .. %d members, 0 .. %d steps, scheme 0 or 1, at most %lld iteration counts",
                    kOnchipMaxN, kOnchipStepsMaxSys, kOnchipStepsMaxSteps, kOnchipStepsMaxCounts);
    *bytes = v;
    return MI355CG_OK;
}
// ---- the explicit scheme with a source time function and receiver traces -----------------------------------
static bool ranges_meet(const void* a, size_t abytes, const void* b, size_t bbytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && abytes && bbytes && pb < pa + abytes && pa < pb + bbytes;
}
// What both entry points refuse before anything is allocated or written: what mi355cg_wave_steps_many refuses of a Verlet call
// (wave_check itself), then what the table, the receivers and the traces add.  host_tables: w can be read here.
static int wave_record_check(mi355cg_ctx* c, int nsys, int nsteps, const double* tau, const void* g, const void* u, const void* v, const double* w,
                             long long w_stride, int nrec, const int* rec_nodes, int record_every, const void* traces, int steps_per_launch,
                             const mi355cg_results* out, const int* steps_done, bool host_tables, bool own_bound = false) {
    if (int rc = wave_check(c, nullptr, nsys, nsteps, MI355CG_WAVE_VERLET, tau, g, u, v, steps_per_launch, out, steps_done, nullptr, own_bound)) return rc;
    if (!w) return fail(MI355CG_ERR_INVALID, "null argument: w, the amplitudes of the source");
    if (w_stride != 0 && w_stride < (long long)nsteps + 1)
        return fail(MI355CG_ERR_INVALID, "w_stride %lld rejected: 0 (one row for all members) or at least nsteps + 1 = %d", w_stride, nsteps + 1);
    if (nrec < 0 || nrec > MI355CG_WAVE_MAX_RECEIVERS) return fail(MI355CG_ERR_INVALID, "nrec %d rejected: a call records 0 .. %d receivers", nrec, MI355CG_WAVE_MAX_RECEIVERS);
    if (record_every < 1) return fail(MI355CG_ERR_INVALID, "record_every %d rejected: it must be >= 1", record_every);
    if (nrec > 0 && (!rec_nodes || !traces)) return fail(MI355CG_ERR_INVALID, "null argument: %d receivers need rec_nodes and traces", nrec);
    for (int r = 0; r < nrec; ++r)
        if (rec_nodes[r] < 0 || rec_nodes[r] >= c->pk_len)
            return fail(MI355CG_ERR_INVALID, "receiver %d is unknown %d: outside [0, %lld)", r, rec_nodes[r], c->pk_len);
    const size_t state = sizeof(double) * (size_t)c->gp.size * (size_t)nsys;
    const size_t wbytes = sizeof(double) * ((size_t)(nsys - 1) * (size_t)w_stride + (size_t)nsteps + 1);
    const size_t tbytes = nrec > 0 ? sizeof(double) * (size_t)nsys * (size_t)(nsteps / record_every) * (size_t)nrec : 0;
    const struct { const void* p; const char* name; } vecs[3] = {{u, "u"}, {v, "v"}, {g, "g"}};
    for (const auto& q : vecs) {
        if (ranges_meet(w, wbytes, q.p, state)) return fail(MI355CG_ERR_INVALID, "w overlaps %s", q.name);
        if (ranges_meet(traces, tbytes, q.p, state)) return fail(MI355CG_ERR_INVALID, "traces overlaps %s", q.name);
    }
    if (ranges_meet(traces, tbytes, w, wbytes)) return fail(MI355CG_ERR_INVALID, "traces overlaps w");
    if (host_tables)
        for (int s = 0; s < (w_stride ? nsys : 1); ++s)
            for (int n = 0; n <= nsteps; ++n)
                if (!std::isfinite(w[(long long)s * w_stride + n]))
                    return fail(MI355CG_ERR_INVALID, "amplitude %g of member %d at step %d rejected: the source must be finite", w[(long long)s * w_stride + n], s, n);
    return MI355CG_OK;
}

// The Verlet workspace, then the receiver cells and (stage_doubles > 0: the host entry point) the staging of the tables and the
// traces on top: built complete before they replace what is there.
static int onchip_wave_record_ensure(mi355cg_ctx* c, int nsys, int stage_vecs, long long stage_doubles) {
    if (int rc = onchip_wave_ensure(c, nsys, MI355CG_WAVE_VERLET, 0, stage_vecs)) return rc;
    OnchipManyWs* W = c->many.get();
    auto failed = [&](const char* what) { return fail(MI355CG_ERR_HIP, "on-chip wave recording workspace for %d members: %s allocation failed", nsys, what); };
    if (!W->rec_cell) {
        Buf<int> cell, cell_h;
        if (Buf<int>::device(cell, kOnchipWaveMaxRec)) return failed("receiver");
        if (Buf<int>::pinned(cell_h, kOnchipWaveMaxRec)) return failed("pinned copy");
        W->rec_cell = std::move(cell); W->rec_cell_h = std::move(cell_h);
    }
    if (stage_doubles > W->rec_stage_cap) {
        Buf<double> stage;
        if (Buf<double>::device(stage, stage_doubles)) return failed("staging");
        HIPCK(hipStreamSynchronize(c->stream));                    // nothing in flight reads the buffer that is replaced
        W->rec_stage = std::move(stage);
        W->rec_stage_cap = stage_doubles;
    }
    return MI355CG_OK;
}

int mi355cg_wave_record_many_device(mi355cg_handle c, int nsys, int nsteps, const double* tau, const double* g_dev, double* u_dev, double* v_dev,
                                    const double* w_dev, long long w_stride, int nrec, const int* rec_nodes, int record_every, double* traces_dev,
                                    int steps_per_launch, const volatile int* stop_flag, mi355cg_results* out, int* steps_done) {
    if (int rc = wave_record_check(c, nsys, nsteps, tau, g_dev, u_dev, v_dev, w_dev, w_stride, nrec, rec_nodes, record_every, traces_dev, steps_per_launch,
                                   out, steps_done, false)) return rc;
    if (StepChecks::none(nsys, nsteps, steps_done)) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    if (int rc = onchip_wave_record_ensure(c, nsys, 0, 0)) return rc;
    const WaveRecord rec{w_dev, w_stride, nrec, rec_nodes, record_every, traces_dev};
    return wave_verlet(c, nsys, nsteps, tau, g_dev, u_dev, v_dev, steps_per_launch, stop_flag, out, steps_done, &rec);
}
int mi355cg_wave_record_many(mi355cg_handle c, int nsys, int nsteps, const double* tau, const double* g, double* u, double* v, const double* w,
                             long long w_stride, int nrec, const int* rec_nodes, int record_every, double* traces, int steps_per_launch,
                             const volatile int* stop_flag, mi355cg_results* out, int* steps_done) {
    if (int rc = wave_record_check(c, nsys, nsteps, tau, g, u, v, w, w_stride, nrec, rec_nodes, record_every, traces, steps_per_launch, out, steps_done, true)) return rc;
    if (StepChecks::none(nsys, nsteps, steps_done)) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    const size_t row = (size_t)nsteps + 1, rows = w_stride ? (size_t)nsys : 1;             // the tables go up packed: row doubles per row
    const size_t sample = (size_t)nrec, samples = (size_t)(nsteps / record_every);          // a member's traces: samples x sample doubles
    if (int rc = onchip_wave_record_ensure(c, nsys, 3, (long long)(rows * row + (size_t)nsys * samples * sample))) return rc;
    const size_t count = (size_t)c->pk_len * (size_t)nsys;         // g, then u, then v; the state comes down
    double* const g_dev = c->many->stage; double* const u_dev = g_dev + count; double* const v_dev = u_dev + count;
    double* const w_dev = c->many->rec_stage; double* const traces_dev = w_dev + rows * row;
    const StagedGroup groups[3] = {{0, g, nullptr}, {count, u, u}, {2 * count, v, v}};
    return run_staged_groups(c, g_dev, count, groups, [&]() {
        HIPCK(hipMemcpy2DAsync(w_dev, sizeof(double) * row, w, sizeof(double) * (w_stride ? (size_t)w_stride : row), sizeof(double) * row, rows, hipMemcpyHostToDevice, c->stream));
        const WaveRecord rec{w_dev, w_stride ? (long long)row : 0, nrec, rec_nodes, record_every, nrec ? traces_dev : nullptr};
        if (int rc = wave_verlet(c, nsys, nsteps, tau, g ? g_dev : nullptr, u_dev, v_dev, steps_per_launch, stop_flag, out, steps_done, &rec)) return rc;
        // the samples of the steps that ran come down; the others stay as the caller left them
        const size_t ran = (size_t)(steps_done[0] / record_every) * sample;
        if (ran) HIPCK(hipMemcpy2DAsync(traces, sizeof(double) * samples * sample, traces_dev, sizeof(double) * samples * sample, sizeof(double) * ran, (size_t)nsys,
                                        hipMemcpyDeviceToHost, c->stream));
        return (int)MI355CG_OK;
    });
}
int mi355cg_wave_record_many_workspace(int n, int nsys, int nsteps, int nrec, int record_every, long long* bytes) {
    if (!bytes) return fail(MI355CG_ERR_INVALID, "null argument");
    const long long v = onchip_wave_record_workspace_bytes(n, nsys, nsteps, nrec, record_every);
    if (v == 0)
        return fail(MI355CG_ERR_INVALID, "recorded wave ensemble rejected: even n from 6 to %d, 1 .. %d members, 0 .. %d steps, 0 .. %d receivers, record_every >= 1",
                    kOnchipMaxN, kOnchipStepsMaxSys, kOnchipStepsMaxSteps, kOnchipWaveMaxRec);
    *bytes = v;
    return MI355CG_OK;
}
// ---- the recorded explicit scheme in a medium: u_tt = c2 o (A u) - w(t) g -----------------------------------
static_assert(kOnchipWaveMediumSysBytes == 2 * sizeof(double), "onchip_plan.h: a member's share of the medium workspace");
// What both entry points refuse on top of wave_record_check (whose homogeneous bound is off: every member has its own).
static int wave_medium_check(mi355cg_ctx* c, int nsys, int nsteps, const double* tau, const void* g, const void* u, const void* v, const double* c2,
                             long long c2_stride, const double* w, long long w_stride, int nrec, const int* rec_nodes, int record_every, const void* traces,
                             int steps_per_launch, const mi355cg_results* out, const int* steps_done, bool host_tables) {
    if (int rc = wave_record_check(c, nsys, nsteps, tau, g, u, v, w, w_stride, nrec, rec_nodes, record_every, traces, steps_per_launch, out, steps_done,
                                   host_tables, true)) return rc;
    if (!c2) return fail(MI355CG_ERR_INVALID, "null argument: c2, the squared wave speed of every unknown");
    if (c2_stride != 0 && c2_stride < c->pk_len)
        return fail(MI355CG_ERR_INVALID, "c2_stride %lld rejected: 0 (one medium for all members) or at least the %lld unknowns of a member", c2_stride, c->pk_len);
    const size_t state = sizeof(double) * (size_t)c->gp.size * (size_t)nsys;
    const size_t cbytes = sizeof(double) * ((c2_stride ? (size_t)(nsys - 1) * (size_t)c2_stride : 0) + (size_t)c->pk_len);
    const size_t wbytes = sizeof(double) * ((size_t)(nsys - 1) * (size_t)w_stride + (size_t)nsteps + 1);
    const size_t tbytes = nrec > 0 ? sizeof(double) * (size_t)nsys * (size_t)(nsteps / record_every) * (size_t)nrec : 0;
    const struct { const void* p; size_t bytes; const char* name; } vecs[5] = {{u, state, "u"}, {v, state, "v"}, {g, state, "g"}, {w, wbytes, "w"}, {traces, tbytes, "traces"}};
    for (const auto& q : vecs)
        if (ranges_meet(c2, cbytes, q.p, q.bytes)) return fail(MI355CG_ERR_INVALID, "c2 overlaps %s", q.name);
    return MI355CG_OK;
}
// range: the least and the largest entry of every row of the media (one row when c2_stride is 0), NaN for a row with an entry
// that is not finite -- what k_oc_medium_range leaves, or the host's own pass.  Every member against its medium and its own bound.
static int wave_medium_bounds(mi355cg_ctx* c, int nsys, const double* tau, const double* range, long long c2_stride) {
    for (int s = 0; s < nsys; ++s) {
        const double lo = range[c2_stride ? 2 * s : 0], hi = range[c2_stride ? 2 * s + 1 : 1];
        if (!std::isfinite(lo) || !std::isfinite(hi))
            return fail(MI355CG_ERR_INVALID, "medium of member %d rejected%s: an entry of c2 is not finite", s, c2_stride ? "" : " (the one medium of all members)");
        if (!(lo > 0.0))
            return fail(MI355CG_ERR_INVALID, "medium of member %d rejected%s: its least entry is %g, and c2, a squared wave speed, must be > 0", s,
                        c2_stride ? "" : " (the one medium of all members)", lo);
        const double bound = onchip_wave_medium_cfl(c->gp.A, hi);
        if (tau[s] > bound)
            return fail(MI355CG_ERR_INVALID, "time step %.17g of member %d rejected: velocity Verlet in its medium (largest c2 %.17g) needs tau <= %.17g (mi355cg_wave_medium_cfl)",
                        tau[s], s, hi, bound);
    }
    return MI355CG_OK;
}
// k_oc_medium_range's result for rows in host memory: `rows` rows of `len` doubles, row s at p + s * stride.
static std::vector<double> host_row_ranges(const double* p, long long stride, size_t rows, size_t len) {
    std::vector<double> range(2 * rows);
    for (size_t s = 0; s < rows; ++s) {
        const double* const row = p + s * (size_t)stride;
        double lo = row[0], hi = row[0];
        bool bad = false;
        for (size_t i = 0; i < len; ++i) { bad = bad || !std::isfinite(row[i]); lo = std::fmin(lo, row[i]); hi = std::fmax(hi, row[i]); }
        range[2 * s] = bad ? NAN : lo; range[2 * s + 1] = bad ? NAN : hi;
    }
    return range;
}
// The recording workspace, then the ranges on top: built complete before they replace what is there.
static int onchip_wave_medium_ensure(mi355cg_ctx* c, int nsys, int stage_vecs, long long stage_doubles) {
    if (int rc = onchip_wave_record_ensure(c, nsys, stage_vecs, stage_doubles)) return rc;
    OnchipManyWs* W = c->many.get();
    if (W->med_cap < nsys) {
        auto failed = [&](const char* what) { return fail(MI355CG_ERR_HIP, "on-chip wave medium workspace for %d members: %s allocation failed", nsys, what); };
        Buf<double> range, range_h;
        if (Buf<double>::device(range, 2LL * nsys)) return failed("range");
        if (Buf<double>::pinned(range_h, 2LL * nsys)) return failed("pinned copy");
        HIPCK(hipStreamSynchronize(c->stream));
        W->med_range = std::move(range); W->med_range_h = std::move(range_h);
        W->med_cap = nsys;
    }
    return MI355CG_OK;
}

int mi355cg_wave_medium_many_device(mi355cg_handle c, int nsys, int nsteps, const double* tau, const double* g_dev, double* u_dev, double* v_dev,
                                    const double* c2_dev, long long c2_stride, const double* w_dev, long long w_stride, int nrec, const int* rec_nodes,
                                    int record_every, double* traces_dev, int steps_per_launch, const volatile int* stop_flag, mi355cg_results* out,
                                    int* steps_done) {
    if (int rc = wave_medium_check(c, nsys, nsteps, tau, g_dev, u_dev, v_dev, c2_dev, c2_stride, w_dev, w_stride, nrec, rec_nodes, record_every, traces_dev,
                                   steps_per_launch, out, steps_done, false)) return rc;
    if (StepChecks::none(nsys, nsteps, steps_done)) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    if (int rc = onchip_wave_medium_ensure(c, nsys, 0, 0)) return rc;
    OnchipManyWs* W = c->many.get();
    const int rows = c2_stride ? nsys : 1;                         // the media are in device memory: one launch reduces them, one read-back
    hipLaunchKernelGGL(k_oc_medium_range, dim3(rows), dim3(kOcRangeThreads), 0, c->stream, c2_dev, c2_stride, (int)c->pk_len, W->med_range.get());
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(W->med_range_h, W->med_range, sizeof(double) * 2 * rows, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    if (int rc = wave_medium_bounds(c, nsys, tau, W->med_range_h, c2_stride)) return rc;
    const WaveRecord rec{w_dev, w_stride, nrec, rec_nodes, record_every, traces_dev, c2_dev, c2_stride};
    return wave_verlet(c, nsys, nsteps, tau, g_dev, u_dev, v_dev, steps_per_launch, stop_flag, out, steps_done, &rec);
}
int mi355cg_wave_medium_many(mi355cg_handle c, int nsys, int nsteps, const double* tau, const double* g, double* u, double* v, const double* c2,
                             long long c2_stride, const double* w, long long w_stride, int nrec, const int* rec_nodes, int record_every, double* traces,
                             int steps_per_launch, const volatile int* stop_flag, mi355cg_results* out, int* steps_done) {
    if (int rc = wave_medium_check(c, nsys, nsteps, tau, g, u, v, c2, c2_stride, w, w_stride, nrec, rec_nodes, record_every, traces, steps_per_launch, out,
                                   steps_done, true)) return rc;
    const size_t len = (size_t)c->pk_len, mrows = c2_stride ? (size_t)nsys : 1;
    // the media can be read here: the two numbers of a row without a launch
    if (int rc = wave_medium_bounds(c, nsys, tau, host_row_ranges(c2, c2_stride, mrows, len).data(), c2_stride)) return rc;
    if (StepChecks::none(nsys, nsteps, steps_done)) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    const size_t row = (size_t)nsteps + 1, rows = w_stride ? (size_t)nsys : 1;             // the tables go up packed: row doubles per row
    const size_t sample = (size_t)nrec, samples = (size_t)(nsteps / record_every);          // a member's traces: samples x sample doubles
    if (int rc = onchip_wave_medium_ensure(c, nsys, 4, (long long)(rows * row + (size_t)nsys * samples * sample))) return rc;
    const size_t count = len * (size_t)nsys;                       // g, then u, then v, then the media (packed: nsys vectors, or one); the state comes down
    double* const g_dev = c->many->stage; double* const u_dev = g_dev + count; double* const v_dev = u_dev + count; double* const c2_dev = v_dev + count;
    double* const w_dev = c->many->rec_stage; double* const traces_dev = w_dev + rows * row;
    const StagedGroup groups[3] = {{0, g, nullptr}, {count, u, u}, {2 * count, v, v}};
    return run_staged_groups(c, g_dev, count, groups, [&]() {
        HIPCK(hipMemcpy2DAsync(c2_dev, sizeof(double) * len, c2, sizeof(double) * (c2_stride ? (size_t)c2_stride : len), sizeof(double) * len, mrows, hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpy2DAsync(w_dev, sizeof(double) * row, w, sizeof(double) * (w_stride ? (size_t)w_stride : row), sizeof(double) * row, rows, hipMemcpyHostToDevice, c->stream));
        const WaveRecord rec{w_dev, w_stride ? (long long)row : 0, nrec, rec_nodes, record_every, nrec ? traces_dev : nullptr, c2_dev, c2_stride ? (long long)len : 0};
        if (int rc = wave_verlet(c, nsys, nsteps, tau, g ? g_dev : nullptr, u_dev, v_dev, steps_per_launch, stop_flag, out, steps_done, &rec)) return rc;
        const size_t ran = (size_t)(steps_done[0] / record_every) * sample;                 // the samples of the steps that ran come down
        if (ran) HIPCK(hipMemcpy2DAsync(traces, sizeof(double) * samples * sample, traces_dev, sizeof(double) * samples * sample, sizeof(double) * ran, (size_t)nsys,
                                        hipMemcpyDeviceToHost, c->stream));
        return (int)MI355CG_OK;
    });
}
int mi355cg_wave_medium_many_workspace(int n, int nsys, int nsteps, int nrec, int record_every, long long* bytes) {
    if (!bytes) return fail(MI355CG_ERR_INVALID, "null argument");
    const long long v = onchip_wave_medium_workspace_bytes(n, nsys, nsteps, nrec, record_every);
    if (v == 0)
        return fail(MI355CG_ERR_INVALID, "recorded wave ensemble in a medium rejected: even n from 6 to %d, 1 .. %d members, 0 .. %d steps, 0 .. %d receivers, record_every >= 1",
                    kOnchipMaxN, kOnchipStepsMaxSys, kOnchipStepsMaxSteps, kOnchipWaveMaxRec);
    *bytes = v;
    return MI355CG_OK;
}
int mi355cg_wave_medium_cfl(mi355cg_handle c, double c2max, double* tau_max) {
    if (!c || !tau_max) return fail(MI355CG_ERR_INVALID, "null argument");
    if (c->is_csr) return fail(MI355CG_ERR_INVALID, "a CSR handle has no grid: the bound is the grid operator's");
    if (!std::isfinite(c2max) || !(c2max > 0.0)) return fail(MI355CG_ERR_INVALID, "c2max %g rejected: the largest squared wave speed is finite and > 0", c2max);
    *tau_max = onchip_wave_medium_cfl(c->gp.A, c2max);
    return MI355CG_OK;
}
// ---- ... with a damping field: u_tt + d o u_t = c2 o (A u) - w(t) g ------------------------------------------
static_assert(kOnchipWaveSpongeSysBytes == 2 * sizeof(double), "onchip_plan.h: a member's share of the sponge workspace");
// What both entry points refuse on top of wave_medium_check.
static int wave_sponge_check(mi355cg_ctx* c, int nsys, int nsteps, const double* tau, const void* g, const void* u, const void* v, const double* c2,
                             long long c2_stride, const double* d, long long d_stride, const double* w, long long w_stride, int nrec, const int* rec_nodes,
                             int record_every, const void* traces, int steps_per_launch, const mi355cg_results* out, const int* steps_done, bool host_tables) {
    if (int rc = wave_medium_check(c, nsys, nsteps, tau, g, u, v, c2, c2_stride, w, w_stride, nrec, rec_nodes, record_every, traces, steps_per_launch, out,
                                   steps_done, host_tables)) return rc;
    if (!d) return fail(MI355CG_ERR_INVALID, "null argument: d, the damping rate of every unknown");
    if (d_stride != 0 && d_stride < c->pk_len)
        return fail(MI355CG_ERR_INVALID, "d_stride %lld rejected: 0 (one damping field for all members) or at least the %lld unknowns of a member", d_stride, c->pk_len);
    const size_t state = sizeof(double) * (size_t)c->gp.size * (size_t)nsys;
    const size_t dbytes = sizeof(double) * ((d_stride ? (size_t)(nsys - 1) * (size_t)d_stride : 0) + (size_t)c->pk_len);
    const size_t cbytes = sizeof(double) * ((c2_stride ? (size_t)(nsys - 1) * (size_t)c2_stride : 0) + (size_t)c->pk_len);
    const size_t wbytes = sizeof(double) * ((size_t)(nsys - 1) * (size_t)w_stride + (size_t)nsteps + 1);
    const size_t tbytes = nrec > 0 ? sizeof(double) * (size_t)nsys * (size_t)(nsteps / record_every) * (size_t)nrec : 0;
    const struct { const void* p; size_t bytes; const char* name; } vecs[6] = {{u, state, "u"}, {v, state, "v"}, {g, state, "g"}, {c2, cbytes, "c2"},
                                                                               {w, wbytes, "w"}, {traces, tbytes, "traces"}};
    for (const auto& q : vecs)
        if (ranges_meet(d, dbytes, q.p, q.bytes)) return fail(MI355CG_ERR_INVALID, "d overlaps %s", q.name);
    return MI355CG_OK;
}
// range: the least and the largest entry of every damping row, as for the media.  Every member against its row: no entry below
// zero, and (0.25 tau_s) max d_s, the e of onchip_wave_sponge_factor, at most kOnchipWaveSpongeMaxE -- beyond it the factor is
// negative and tends to -1, so that stronger damping would damp less.
static int wave_sponge_bounds(int nsys, const double* tau, const double* range, long long d_stride) {
    for (int s = 0; s < nsys; ++s) {
        const double lo = range[d_stride ? 2 * s : 0], hi = range[d_stride ? 2 * s + 1 : 1];
        const char* const shared = d_stride ? "" : " (the one damping field of all members)";
        if (!std::isfinite(lo) || !std::isfinite(hi))
            return fail(MI355CG_ERR_INVALID, "damping of member %d rejected%s: an entry of d is not finite", s, shared);
        if (lo < 0.0)
            return fail(MI355CG_ERR_INVALID, "damping of member %d rejected%s: its least entry is %g, and d, a damping rate, must be >= 0", s, shared, lo);
        if ((0.25 * tau[s]) * hi > kOnchipWaveSpongeMaxE)
            return fail(MI355CG_ERR_INVALID, "damping of member %d rejected%s: its largest entry %.17g with the time step %.17g needs d <= 4 / tau = %.17g; beyond it the "
                        "factor (1 - tau d / 4) / (1 + tau d / 4) turns negative and damps less", s, shared, hi, tau[s], 4.0 / tau[s]);
    }
    return MI355CG_OK;
}
// The medium workspace, then the second pair of ranges on top: built complete before they replace what is there.
static int onchip_wave_sponge_ensure(mi355cg_ctx* c, int nsys, int stage_vecs, long long stage_doubles) {
    if (int rc = onchip_wave_medium_ensure(c, nsys, stage_vecs, stage_doubles)) return rc;
    OnchipManyWs* W = c->many.get();
    if (W->damp_cap < nsys) {
        auto failed = [&](const char* what) { return fail(MI355CG_ERR_HIP, "on-chip wave sponge workspace for %d members: %s allocation failed", nsys, what); };
        Buf<double> range, range_h;
        if (Buf<double>::device(range, 2LL * nsys)) return failed("range");
        if (Buf<double>::pinned(range_h, 2LL * nsys)) return failed("pinned copy");
        HIPCK(hipStreamSynchronize(c->stream));
        W->damp_range = std::move(range); W->damp_range_h = std::move(range_h);
        W->damp_cap = nsys;
    }
    return MI355CG_OK;
}

int mi355cg_wave_sponge_many_device(mi355cg_handle c, int nsys, int nsteps, const double* tau, const double* g_dev, double* u_dev, double* v_dev,
                                    const double* c2_dev, long long c2_stride, const double* d_dev, long long d_stride, const double* w_dev,
                                    long long w_stride, int nrec, const int* rec_nodes, int record_every, double* traces_dev, int steps_per_launch,
                                    const volatile int* stop_flag, mi355cg_results* out, int* steps_done) {
    if (int rc = wave_sponge_check(c, nsys, nsteps, tau, g_dev, u_dev, v_dev, c2_dev, c2_stride, d_dev, d_stride, w_dev, w_stride, nrec, rec_nodes, record_every,
                                   traces_dev, steps_per_launch, out, steps_done, false)) return rc;
    if (StepChecks::none(nsys, nsteps, steps_done)) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    if (int rc = onchip_wave_sponge_ensure(c, nsys, 0, 0)) return rc;
    OnchipManyWs* W = c->many.get();
    const int crows = c2_stride ? nsys : 1, drows = d_stride ? nsys : 1;                   // two launches of the one range kernel, one wait
    hipLaunchKernelGGL(k_oc_medium_range, dim3(crows), dim3(kOcRangeThreads), 0, c->stream, c2_dev, c2_stride, (int)c->pk_len, W->med_range.get());
    HIPCK(hipGetLastError());
    hipLaunchKernelGGL(k_oc_medium_range, dim3(drows), dim3(kOcRangeThreads), 0, c->stream, d_dev, d_stride, (int)c->pk_len, W->damp_range.get());
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(W->med_range_h, W->med_range, sizeof(double) * 2 * crows, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(W->damp_range_h, W->damp_range, sizeof(double) * 2 * drows, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    if (int rc = wave_medium_bounds(c, nsys, tau, W->med_range_h, c2_stride)) return rc;
    if (int rc = wave_sponge_bounds(nsys, tau, W->damp_range_h, d_stride)) return rc;
    const WaveRecord rec{w_dev, w_stride, nrec, rec_nodes, record_every, traces_dev, c2_dev, c2_stride, d_dev, d_stride};
    return wave_verlet(c, nsys, nsteps, tau, g_dev, u_dev, v_dev, steps_per_launch, stop_flag, out, steps_done, &rec);
}
int mi355cg_wave_sponge_many(mi355cg_handle c, int nsys, int nsteps, const double* tau, const double* g, double* u, double* v, const double* c2,
                             long long c2_stride, const double* d, long long d_stride, const double* w, long long w_stride, int nrec, const int* rec_nodes,
                             int record_every, double* traces, int steps_per_launch, const volatile int* stop_flag, mi355cg_results* out, int* steps_done) {
    if (int rc = wave_sponge_check(c, nsys, nsteps, tau, g, u, v, c2, c2_stride, d, d_stride, w, w_stride, nrec, rec_nodes, record_every, traces,
                                   steps_per_launch, out, steps_done, true)) return rc;
    const size_t len = (size_t)c->pk_len, mrows = c2_stride ? (size_t)nsys : 1, drows = d_stride ? (size_t)nsys : 1;
    if (int rc = wave_medium_bounds(c, nsys, tau, host_row_ranges(c2, c2_stride, mrows, len).data(), c2_stride)) return rc;
    if (int rc = wave_sponge_bounds(nsys, tau, host_row_ranges(d, d_stride, drows, len).data(), d_stride)) return rc;
    if (StepChecks::none(nsys, nsteps, steps_done)) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    const size_t row = (size_t)nsteps + 1, rows = w_stride ? (size_t)nsys : 1;             // the tables go up packed: row doubles per row
    const size_t sample = (size_t)nrec, samples = (size_t)(nsteps / record_every);          // a member's traces: samples x sample doubles
    if (int rc = onchip_wave_sponge_ensure(c, nsys, 5, (long long)(rows * row + (size_t)nsys * samples * sample))) return rc;
    const size_t count = len * (size_t)nsys;                       // g, u, v, the media, then the damping rows (packed: nsys vectors, or one)
    double* const g_dev = c->many->stage; double* const u_dev = g_dev + count; double* const v_dev = u_dev + count; double* const c2_dev = v_dev + count;
    double* const d_dev = c2_dev + count;
    double* const w_dev = c->many->rec_stage; double* const traces_dev = w_dev + rows * row;
    const StagedGroup groups[3] = {{0, g, nullptr}, {count, u, u}, {2 * count, v, v}};
    return run_staged_groups(c, g_dev, count, groups, [&]() {
        HIPCK(hipMemcpy2DAsync(c2_dev, sizeof(double) * len, c2, sizeof(double) * (c2_stride ? (size_t)c2_stride : len), sizeof(double) * len, mrows, hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpy2DAsync(d_dev, sizeof(double) * len, d, sizeof(double) * (d_stride ? (size_t)d_stride : len), sizeof(double) * len, drows, hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpy2DAsync(w_dev, sizeof(double) * row, w, sizeof(double) * (w_stride ? (size_t)w_stride : row), sizeof(double) * row, rows, hipMemcpyHostToDevice, c->stream));
        const WaveRecord rec{w_dev, w_stride ? (long long)row : 0, nrec, rec_nodes, record_every, nrec ? traces_dev : nullptr, c2_dev, c2_stride ? (long long)len : 0,
                             d_dev, d_stride ? (long long)len : 0};
        if (int rc = wave_verlet(c, nsys, nsteps, tau, g ? g_dev : nullptr, u_dev, v_dev, steps_per_launch, stop_flag, out, steps_done, &rec)) return rc;
        const size_t ran = (size_t)(steps_done[0] / record_every) * sample;                 // the samples of the steps that ran come down
        if (ran) HIPCK(hipMemcpy2DAsync(traces, sizeof(double) * samples * sample, traces_dev, sizeof(double) * samples * sample, sizeof(double) * ran, (size_t)nsys,
                                        hipMemcpyDeviceToHost, c->stream));
        return (int)MI355CG_OK;
    });
}
int mi355cg_wave_sponge_many_workspace(int n, int nsys, int nsteps, int nrec, int record_every, long long* bytes) {
    if (!bytes) return fail(MI355CG_ERR_INVALID, "null argument");
    const long long v = onchip_wave_sponge_workspace_bytes(n, nsys, nsteps, nrec, record_every);
    if (v == 0)
        return fail(MI355CG_ERR_INVALID, "recorded wave ensemble with a damping field rejected: even n from 6 to %d, 1 .. %d members, 0 .. %d steps, 0 .. %d receivers, record_every >= 1",
                    kOnchipMaxN, kOnchipStepsMaxSys, kOnchipStepsMaxSteps, kOnchipWaveMaxRec);
    *bytes = v;
    return MI355CG_OK;
}
// ---- the adjoint of the scheme in a medium: the forward run with its history, the backward run --------------
// What both history entry points refuse on top of wave_medium_check.
static int wave_history_check(mi355cg_ctx* c, int nsys, int nsteps, const double* tau, const void* g, const void* u, const void* v, const double* c2,
                              long long c2_stride, const double* hist, long long hist_stride, const double* w, long long w_stride, int nrec, const int* rec_nodes,
                              int record_every, const void* traces, int steps_per_launch, const mi355cg_results* out, const int* steps_done, bool host_tables) {
    if (int rc = wave_medium_check(c, nsys, nsteps, tau, g, u, v, c2, c2_stride, w, w_stride, nrec, rec_nodes, record_every, traces, steps_per_launch, out,
                                   steps_done, host_tables)) return rc;
    if (!hist) return fail(MI355CG_ERR_INVALID, "null argument: hist, the history the run writes");
    const long long rows = ((long long)nsteps + 1) * c->pk_len;
    if (hist_stride < rows)
        return fail(MI355CG_ERR_INVALID, "hist_stride %lld rejected: a member's history is (nsteps + 1) x %lld = %lld doubles", hist_stride, c->pk_len, rows);
    const size_t state = sizeof(double) * (size_t)c->gp.size * (size_t)nsys;
    const size_t hbytes = sizeof(double) * ((size_t)(nsys - 1) * (size_t)hist_stride + (size_t)rows);
    const size_t cbytes = sizeof(double) * ((c2_stride ? (size_t)(nsys - 1) * (size_t)c2_stride : 0) + (size_t)c->pk_len);
    const size_t wbytes = sizeof(double) * ((size_t)(nsys - 1) * (size_t)w_stride + (size_t)nsteps + 1);
    const size_t tbytes = nrec > 0 ? sizeof(double) * (size_t)nsys * (size_t)(nsteps / record_every) * (size_t)nrec : 0;
    const struct { const void* p; size_t bytes; const char* name; } vecs[6] = {{u, state, "u"}, {v, state, "v"}, {g, state, "g"}, {c2, cbytes, "c2"},
                                                                               {w, wbytes, "w"}, {traces, tbytes, "traces"}};
    for (const auto& q : vecs)
        if (ranges_meet(hist, hbytes, q.p, q.bytes)) return fail(MI355CG_ERR_INVALID, "hist overlaps %s", q.name);
    return MI355CG_OK;
}
int mi355cg_wave_history_many_device(mi355cg_handle c, int nsys, int nsteps, const double* tau, const double* g_dev, double* u_dev, double* v_dev,
                                     const double* c2_dev, long long c2_stride, double* hist_dev, long long hist_stride, const double* w_dev,
                                     long long w_stride, int nrec, const int* rec_nodes, int record_every, double* traces_dev, int steps_per_launch,
                                     const volatile int* stop_flag, mi355cg_results* out, int* steps_done) {
    if (int rc = wave_history_check(c, nsys, nsteps, tau, g_dev, u_dev, v_dev, c2_dev, c2_stride, hist_dev, hist_stride, w_dev, w_stride, nrec, rec_nodes,
                                    record_every, traces_dev, steps_per_launch, out, steps_done, false)) return rc;
    if (StepChecks::none(nsys, nsteps, steps_done)) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    if (int rc = onchip_wave_medium_ensure(c, nsys, 0, 0)) return rc;
    OnchipManyWs* W = c->many.get();
    const int rows = c2_stride ? nsys : 1;
    hipLaunchKernelGGL(k_oc_medium_range, dim3(rows), dim3(kOcRangeThreads), 0, c->stream, c2_dev, c2_stride, (int)c->pk_len, W->med_range.get());
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(W->med_range_h, W->med_range, sizeof(double) * 2 * rows, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    if (int rc = wave_medium_bounds(c, nsys, tau, W->med_range_h, c2_stride)) return rc;
    WaveRecord rec{w_dev, w_stride, nrec, rec_nodes, record_every, traces_dev, c2_dev, c2_stride};
    rec.hist = hist_dev; rec.hist_stride = hist_stride;
    return wave_verlet(c, nsys, nsteps, tau, g_dev, u_dev, v_dev, steps_per_launch, stop_flag, out, steps_done, &rec);
}
int mi355cg_wave_history_many(mi355cg_handle c, int nsys, int nsteps, const double* tau, const double* g, double* u, double* v, const double* c2,
                              long long c2_stride, double* hist, long long hist_stride, const double* w, long long w_stride, int nrec, const int* rec_nodes,
                              int record_every, double* traces, int steps_per_launch, const volatile int* stop_flag, mi355cg_results* out, int* steps_done) {
    if (int rc = wave_history_check(c, nsys, nsteps, tau, g, u, v, c2, c2_stride, hist, hist_stride, w, w_stride, nrec, rec_nodes, record_every, traces,
                                    steps_per_launch, out, steps_done, true)) return rc;
    const size_t len = (size_t)c->pk_len, mrows = c2_stride ? (size_t)nsys : 1;
    if (int rc = wave_medium_bounds(c, nsys, tau, host_row_ranges(c2, c2_stride, mrows, len).data(), c2_stride)) return rc;
    if (StepChecks::none(nsys, nsteps, steps_done)) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    const size_t row = (size_t)nsteps + 1, rows = w_stride ? (size_t)nsys : 1;             // the tables go up packed: row doubles per row
    const size_t sample = (size_t)nrec, samples = (size_t)(nsteps / record_every);          // a member's traces: samples x sample doubles
    const size_t hrow = row * len;                                                          // a member's history, packed
    if (int rc = onchip_wave_medium_ensure(c, nsys, 4, (long long)(rows * row + (size_t)nsys * samples * sample + (size_t)nsys * hrow))) return rc;
    const size_t count = len * (size_t)nsys;                       // g, then u, then v, then the media; the state comes down
    double* const g_dev = c->many->stage; double* const u_dev = g_dev + count; double* const v_dev = u_dev + count; double* const c2_dev = v_dev + count;
    double* const w_dev = c->many->rec_stage; double* const traces_dev = w_dev + rows * row; double* const hist_dev = traces_dev + (size_t)nsys * samples * sample;
    const StagedGroup groups[3] = {{0, g, nullptr}, {count, u, u}, {2 * count, v, v}};
    return run_staged_groups(c, g_dev, count, groups, [&]() {
        HIPCK(hipMemcpy2DAsync(c2_dev, sizeof(double) * len, c2, sizeof(double) * (c2_stride ? (size_t)c2_stride : len), sizeof(double) * len, mrows, hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpy2DAsync(w_dev, sizeof(double) * row, w, sizeof(double) * (w_stride ? (size_t)w_stride : row), sizeof(double) * row, rows, hipMemcpyHostToDevice, c->stream));
        WaveRecord rec{w_dev, w_stride ? (long long)row : 0, nrec, rec_nodes, record_every, nrec ? traces_dev : nullptr, c2_dev, c2_stride ? (long long)len : 0};
        rec.hist = hist_dev; rec.hist_stride = (long long)hrow;
        if (int rc = wave_verlet(c, nsys, nsteps, tau, g ? g_dev : nullptr, u_dev, v_dev, steps_per_launch, stop_flag, out, steps_done, &rec)) return rc;
        const size_t ran = (size_t)(steps_done[0] / record_every) * sample;                 // the samples and the rows of the steps that ran come down
        if (ran) HIPCK(hipMemcpy2DAsync(traces, sizeof(double) * samples * sample, traces_dev, sizeof(double) * samples * sample, sizeof(double) * ran, (size_t)nsys,
                                        hipMemcpyDeviceToHost, c->stream));
        if (steps_done[0] > 0) HIPCK(hipMemcpy2DAsync(hist, sizeof(double) * (size_t)hist_stride, hist_dev, sizeof(double) * hrow,
                                                      sizeof(double) * ((size_t)steps_done[0] + 1) * len, (size_t)nsys, hipMemcpyDeviceToHost, c->stream));
        return (int)MI355CG_OK;
    });
}
int mi355cg_wave_history_bytes(int n, int nsys, int nsteps, long long* bytes) {
    if (!bytes) return fail(MI355CG_ERR_INVALID, "null argument");
    const long long v = onchip_wave_history_bytes(n, nsys, nsteps);
    if (v == 0)
        return fail(MI355CG_ERR_INVALID, "wave history rejected: even n from 6 to %d, 1 .. %d members, 0 .. %d steps", kOnchipMaxN, kOnchipStepsMaxSys, kOnchipStepsMaxSteps);
    *bytes = v;
    return MI355CG_OK;
}

// What both adjoint entry points refuse before anything is allocated or written.  host_tables: adj can be read here.
static int wave_adjoint_check(mi355cg_ctx* c, int nsys, int nsteps, const double* tau, const double* c2, long long c2_stride, const double* hist,
                              long long hist_stride, int nrec, const int* rec_nodes, int record_every, const double* adj, long long adj_stride,
                              const void* lam, const void* q, const void* S, int steps_per_launch, const mi355cg_results* out, const int* steps_done,
                              bool host_tables) {
    if (!c || !tau || !lam || !q || !S || !out || !steps_done) return fail(MI355CG_ERR_INVALID, "null argument");
    if (int rc = kWaveEnsemble.count(nsys)) return rc;
    if (int rc = StepChecks::nsteps(nsteps)) return rc;
    if (steps_per_launch < 0) return fail(MI355CG_ERR_INVALID, "steps_per_launch %d rejected: 0 (the default) or a positive number of steps", steps_per_launch);
    if (int rc = kWaveEnsemble.onchip(c)) return rc;
    for (int s = 0; s < nsys; ++s) if (int rc = StepChecks::tau(tau[s], s)) return rc;
    if (!c2) return fail(MI355CG_ERR_INVALID, "null argument: c2, the squared wave speed of every unknown");
    if (c2_stride != 0 && c2_stride < c->pk_len)
        return fail(MI355CG_ERR_INVALID, "c2_stride %lld rejected: 0 (one medium for all members) or at least the %lld unknowns of a member", c2_stride, c->pk_len);
    if (!hist) return fail(MI355CG_ERR_INVALID, "null argument: hist, the history of the forward run");
    const long long rows = ((long long)nsteps + 1) * c->pk_len;
    if (hist_stride < rows)
        return fail(MI355CG_ERR_INVALID, "hist_stride %lld rejected: a member's history is (nsteps + 1) x %lld = %lld doubles", hist_stride, c->pk_len, rows);
    if (nrec < 0 || nrec > MI355CG_WAVE_MAX_RECEIVERS) return fail(MI355CG_ERR_INVALID, "nrec %d rejected: a call takes 0 .. %d receivers", nrec, MI355CG_WAVE_MAX_RECEIVERS);
    if (record_every < 1) return fail(MI355CG_ERR_INVALID, "record_every %d rejected: it must be >= 1", record_every);
    const long long table = (long long)(nsteps / record_every) * nrec;                      // a member's adjoint sources
    if (nrec > 0 && (!rec_nodes || !adj)) return fail(MI355CG_ERR_INVALID, "null argument: %d receivers need rec_nodes and adj, the adjoint sources", nrec);
    for (int r = 0; r < nrec; ++r)
        if (rec_nodes[r] < 0 || rec_nodes[r] >= c->pk_len)
            return fail(MI355CG_ERR_INVALID, "receiver %d is unknown %d: outside [0, %lld)", r, rec_nodes[r], c->pk_len);
    if (adj_stride != 0 && adj_stride < table)
        return fail(MI355CG_ERR_INVALID, "adj_stride %lld rejected: 0 (one table for all members) or at least (nsteps / record_every) x nrec = %lld", adj_stride, table);
    if (BatchKind::apart(c, nsys, lam, q, "lam overlaps q") || BatchKind::apart(c, nsys, lam, S, "lam overlaps S") || BatchKind::apart(c, nsys, q, S, "q overlaps S"))
        return MI355CG_ERR_INVALID;
    const size_t state = sizeof(double) * (size_t)c->gp.size * (size_t)nsys;
    const size_t hbytes = sizeof(double) * ((size_t)(nsys - 1) * (size_t)hist_stride + (size_t)rows);
    const size_t cbytes = sizeof(double) * ((c2_stride ? (size_t)(nsys - 1) * (size_t)c2_stride : 0) + (size_t)c->pk_len);
    const size_t abytes = nrec > 0 ? sizeof(double) * ((size_t)(nsys - 1) * (size_t)adj_stride + (size_t)table) : 0;
    const struct { const void* p; size_t bytes; const char* name; } vecs[6] = {{lam, state, "lam"}, {q, state, "q"}, {S, state, "S"}, {c2, cbytes, "c2"},
                                                                               {hist, hbytes, "hist"}, {adj, abytes, "adj"}};
    for (int i = 3; i < 6; ++i)
        for (int j = 0; j < i; ++j)
            if (ranges_meet(vecs[i].p, vecs[i].bytes, vecs[j].p, vecs[j].bytes)) return fail(MI355CG_ERR_INVALID, "%s overlaps %s", vecs[i].name, vecs[j].name);
    if (host_tables && nrec > 0)
        for (int s = 0; s < (adj_stride ? nsys : 1); ++s)
            for (long long i = 0; i < table; ++i)
                if (!std::isfinite(adj[(long long)s * adj_stride + i]))
                    return fail(MI355CG_ERR_INVALID, "adjoint source %g of member %d at sample %lld, receiver %lld rejected: it must be finite", adj[(long long)s * adj_stride + i],
                                s, i / nrec, i % nrec);
    return MI355CG_OK;
}
// Backwards: ceil(nsteps / m) launches of m steps from the state index nsteps down; the host tests the flag between two.
// Everything in device memory but tau and the receivers.
static int wave_adjoint(mi355cg_ctx* c, int nsys, int nsteps, const double* tau, const double* c2_dev, long long c2_stride, const double* hist_dev,
                        long long hist_stride, int nrec, const int* rec_nodes, int record_every, const double* adj_dev, long long adj_stride, double* lam_dev,
                        double* q_dev, double* S_dev, int steps_per_launch, const volatile int* stop_flag, mi355cg_results* out, int* steps_done) {
    mi355cg_params none;                                           // the driver reads a rule; the scheme decides nothing
    mi355cg_default_params(&none, MI355CG_RULE_REL_2NORM);
    OnchipManyRun R;
    if (int rc = R.open(c, &none, nsys, stop_flag, "adjoint wave stepping")) return rc;
    OnchipManyWs* W = R.W;
    for (int s = 0; s < nsys; ++s) { W->wave_tau_h[s] = tau[s]; W->wave_tau_h[nsys + s] = 2.0 / tau[s]; }
    HIPCK(hipMemcpyAsync(W->wave_tau, W->wave_tau_h, sizeof(double) * 2 * nsys, hipMemcpyHostToDevice, c->stream));
    for (int r = 0; r < nrec; ++r) W->rec_cell_h[r] = rec_nodes[r];                         // the kernel wants the packed indices themselves
    if (nrec) HIPCK(hipMemcpyAsync(W->rec_cell, W->rec_cell_h, sizeof(int) * nrec, hipMemcpyHostToDevice, c->stream));
    OnchipWaveAdjArgs a{};
    a.pl = R.pl; a.k = OnchipWaveCoef{c->gp.A, c->gp.x_k, c->gp.y_k};
    a.tau = W->wave_tau; a.c2 = c2_dev; a.c2_stride = c2_stride; a.hist = hist_dev; a.hist_stride = hist_stride;
    a.adj = adj_dev; a.adj_stride = adj_stride; a.rec_node = W->rec_cell; a.nrec = nrec; a.every = record_every;
    a.lam = lam_dev; a.q = q_dev; a.S = S_dev; a.stride = R.U;
    const void* k_steps = onchip_dispatch(R.pl.elems, false, [](auto el, auto) { return (const void*)&k_oc_wave_adjoint<decltype(el)::value>; });
    if (int rc = R.allow_lds(k_steps)) return rc;
    if (int rc = loop_timer_begin(c, c->stream)) return rc;
    const int m = steps_per_launch > 0 ? steps_per_launch : kOnchipWaveDefaultSteps;
    void* args[] = {&a};
    int done = 0;
    while (done < nsteps) {
        if (done > 0) HIPCK(hipStreamSynchronize(c->stream));
        if (stop_flag && *stop_flag) { R.interrupted = true; break; }
        a.m = std::min(m, nsteps - done);
        a.s_top = nsteps - done;
        if (int rc = R.launch(k_steps, args)) return rc;
        done += a.m;
    }
    if (int rc = R.end_loop(false)) return rc;
    HIPCK(hipStreamSynchronize(c->stream));
    CgState fin{};
    fin.done = 1; fin.converged = 1;
    for (int s = 0; s < nsys; ++s) { steps_done[s] = done; out[s] = make_results(fin, R.interrupted, false, 0.0); }
    return R.stamp_times(out);
}
int mi355cg_wave_adjoint_many_device(mi355cg_handle c, int nsys, int nsteps, const double* tau, const double* c2_dev, long long c2_stride,
                                     const double* hist_dev, long long hist_stride, int nrec, const int* rec_nodes, int record_every, const double* adj_dev,
                                     long long adj_stride, double* lam_dev, double* q_dev, double* S_dev, int steps_per_launch, const volatile int* stop_flag,
                                     mi355cg_results* out, int* steps_done) {
    if (int rc = wave_adjoint_check(c, nsys, nsteps, tau, c2_dev, c2_stride, hist_dev, hist_stride, nrec, rec_nodes, record_every, adj_dev, adj_stride, lam_dev,
                                    q_dev, S_dev, steps_per_launch, out, steps_done, false)) return rc;
    if (StepChecks::none(nsys, nsteps, steps_done)) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    if (int rc = onchip_wave_medium_ensure(c, nsys, 0, 0)) return rc;
    OnchipManyWs* W = c->many.get();
    const int rows = c2_stride ? nsys : 1;                         // the transpose has the forward scheme's stability: every member against its own bound
    hipLaunchKernelGGL(k_oc_medium_range, dim3(rows), dim3(kOcRangeThreads), 0, c->stream, c2_dev, c2_stride, (int)c->pk_len, W->med_range.get());
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(W->med_range_h, W->med_range, sizeof(double) * 2 * rows, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    if (int rc = wave_medium_bounds(c, nsys, tau, W->med_range_h, c2_stride)) return rc;
    return wave_adjoint(c, nsys, nsteps, tau, c2_dev, c2_stride, hist_dev, hist_stride, nrec, rec_nodes, record_every, adj_dev, adj_stride, lam_dev, q_dev, S_dev,
                        steps_per_launch, stop_flag, out, steps_done);
}
int mi355cg_wave_adjoint_many(mi355cg_handle c, int nsys, int nsteps, const double* tau, const double* c2, long long c2_stride, const double* hist,
                              long long hist_stride, int nrec, const int* rec_nodes, int record_every, const double* adj, long long adj_stride, double* lam,
                              double* q, double* S, int steps_per_launch, const volatile int* stop_flag, mi355cg_results* out, int* steps_done) {
    if (int rc = wave_adjoint_check(c, nsys, nsteps, tau, c2, c2_stride, hist, hist_stride, nrec, rec_nodes, record_every, adj, adj_stride, lam, q, S,
                                    steps_per_launch, out, steps_done, true)) return rc;
    const size_t len = (size_t)c->pk_len, mrows = c2_stride ? (size_t)nsys : 1;
    if (int rc = wave_medium_bounds(c, nsys, tau, host_row_ranges(c2, c2_stride, mrows, len).data(), c2_stride)) return rc;
    if (StepChecks::none(nsys, nsteps, steps_done)) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    const size_t hrow = ((size_t)nsteps + 1) * len;                                         // a member's history, packed
    const size_t table = (size_t)(nsteps / record_every) * (size_t)nrec, arows = adj_stride ? (size_t)nsys : 1;
    if (int rc = onchip_wave_medium_ensure(c, nsys, 4, (long long)((size_t)nsys * hrow + arows * table))) return rc;
    const size_t count = len * (size_t)nsys;                       // lam, then q, then S (up and down), then the media
    double* const lam_dev = c->many->stage; double* const q_dev = lam_dev + count; double* const S_dev = q_dev + count; double* const c2_dev = S_dev + count;
    double* const hist_dev = c->many->rec_stage; double* const adj_dev = hist_dev + (size_t)nsys * hrow;
    const StagedGroup groups[3] = {{0, lam, lam}, {count, q, q}, {2 * count, S, S}};
    return run_staged_groups(c, lam_dev, count, groups, [&]() {
        HIPCK(hipMemcpy2DAsync(c2_dev, sizeof(double) * len, c2, sizeof(double) * (c2_stride ? (size_t)c2_stride : len), sizeof(double) * len, mrows, hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpy2DAsync(hist_dev, sizeof(double) * hrow, hist, sizeof(double) * (size_t)hist_stride, sizeof(double) * hrow, (size_t)nsys, hipMemcpyHostToDevice, c->stream));
        if (table) HIPCK(hipMemcpy2DAsync(adj_dev, sizeof(double) * table, adj, sizeof(double) * (adj_stride ? (size_t)adj_stride : table), sizeof(double) * table, arows,
                                          hipMemcpyHostToDevice, c->stream));
        return wave_adjoint(c, nsys, nsteps, tau, c2_dev, c2_stride ? (long long)len : 0, hist_dev, (long long)hrow, nrec, rec_nodes, record_every,
                            table ? adj_dev : nullptr, adj_stride ? (long long)table : 0, lam_dev, q_dev, S_dev, steps_per_launch, stop_flag, out, steps_done);
    });
}
int mi355cg_wave_adjoint_many_workspace(int n, int nsys, int nsteps, int nrec, int record_every, long long* bytes) {
    if (!bytes) return fail(MI355CG_ERR_INVALID, "null argument");
    const long long v = onchip_wave_adjoint_workspace_bytes(n, nsys, nsteps, nrec, record_every);
    if (v == 0)
        return fail(MI355CG_ERR_INVALID, "adjoint wave ensemble rejected: even n from 6 to %d, 1 .. %d members, 0 .. %d steps, 0 .. %d receivers, record_every >= 1",
                    kOnchipMaxN, kOnchipStepsMaxSys, kOnchipStepsMaxSteps, kOnchipWaveMaxRec);
    *bytes = v;
    return MI355CG_OK;
}
int mi355cg_wave_cfl(mi355cg_handle c, double* tau_max) {
    if (!c || !tau_max) return fail(MI355CG_ERR_INVALID, "null argument");
    if (c->is_csr) return fail(MI355CG_ERR_INVALID, "a CSR handle has no grid: the bound is the grid operator's");
    *tau_max = onchip_wave_cfl(c->gp.A);
    return MI355CG_OK;
}

// ---- lowest eigenpairs by a block multigrid-preconditioned iteration ------------------------------------------
int mi355cg_eigs_device(mi355cg_handle c, int nev, int block, double tol, int max_iterations, double* x_dev, double* lambda, double* resid,
                        const volatile int* stop_flag, mi355cg_eig_results* out) {
    if (int rc = eig_check(c, nev, block, tol, max_iterations, x_dev, lambda, resid, out)) return rc;
    HIPCK(hipSetDevice(c->device));
    if (int rc = eig_ensure(c, block, false)) return rc;
    return solve_eigs(c, nev, block, tol, max_iterations, x_dev, lambda, resid, stop_flag, out);
}

int mi355cg_eigs(mi355cg_handle c, int nev, int block, double tol, int max_iterations, double* x, double* lambda, double* resid,
                 const volatile int* stop_flag, mi355cg_eig_results* out) {
    if (int rc = eig_check(c, nev, block, tol, max_iterations, x, lambda, resid, out)) return rc;
    HIPCK(hipSetDevice(c->device));
    if (int rc = eig_ensure(c, block, true)) return rc;
    // the start block goes up and the Ritz vectors come down through one buffer
    return run_staged(c, c->eig->stage, (size_t)c->pk_len * (size_t)block, 0, x, nullptr, x, [&](const double*, double* x_dev) {
        return solve_eigs(c, nev, block, tol, max_iterations, x_dev, lambda, resid, stop_flag, out);
    });
}

int mi355cg_eigs_release(mi355cg_handle c) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    if (!c->eig) return MI355CG_OK;
    HIPCK(hipSetDevice(c->device));
    eig_free(c);
    return MI355CG_OK;
}

int mi355cg_rayleigh_ritz(int k, const double* g, const double* hmat, double* theta, double* coef) {
    if (!g || !hmat || !theta || !coef) return fail(MI355CG_ERR_INVALID, "null argument");
    if (k < 1 || k > kEigBasisMax) return fail(MI355CG_ERR_INVALID, "a Rayleigh-Ritz basis has 1 .. %d vectors, not %d", kEigBasisMax, k);
    if (const char* why = rr_solve(k, g, hmat, theta, coef)) return fail(MI355CG_ERR_STATE, "basis refused: %s", why);
    return MI355CG_OK;
}

int mi355cg_block_gram_indexed(mi355cg_handle c, int na, const double* a, int nia, const int* ia, int nb, const double* b, int nib, const int* ib,
                               double* out) {
    if (!c || !a || !b || !out) return fail(MI355CG_ERR_INVALID, "null argument");
    if (na < 1 || na > kEigBasisMax || nb < 1 || nb > kEigBasisMax)
        return fail(MI355CG_ERR_INVALID, "a group has 1 .. %d vectors, not %d and %d", kEigBasisMax, na, nb);
    if ((ia && (nia < 1 || nia > kEigBasisMax)) || (ib && (nib < 1 || nib > kEigBasisMax)))
        return fail(MI355CG_ERR_INVALID, "an index list has 1 .. %d entries, not %d and %d", kEigBasisMax, nia, nib);
    for (int i = 0; ia && i < nia; ++i) if (ia[i] < 0 || ia[i] >= na) return fail(MI355CG_ERR_INVALID, "index %d of the first list is outside 0 .. %d", ia[i], na - 1);
    for (int i = 0; ib && i < nib; ++i) if (ib[i] < 0 || ib[i] >= nb) return fail(MI355CG_ERR_INVALID, "index %d of the second list is outside 0 .. %d", ib[i], nb - 1);
    if (int rc = block_check(c)) return rc;
    HIPCK(hipSetDevice(c->device));
    const long long vlen = round_up(c->storage_len, 32);
    const int G = std::min(c->g.N - 1, kMgMaxGrid);
    EigList la{vlen, 0, {}}, lb{vlen, 0, {}};
    for (int i = 0; i < (ia ? nia : na); ++i) la.idx[la.n++] = ia ? ia[i] : i;
    for (int i = 0; i < (ib ? nib : nb); ++i) lb.idx[lb.n++] = na + (ib ? ib[i] : i);
    BlockTmp T;
    const double* src[2] = {a, b};
    const int counts[2] = {na, nb};
    if (int rc = block_upload(c, T, na + nb, 0, src, counts, 2, vlen)) return rc;
    const int tiles = eig_tiles(la.n) * eig_tiles(lb.n);
    if (Buf<double>::device(T.part, (long long)tiles * kEigTileEntries * G) || Buf<double>::device(T.mat, (long long)la.n * lb.n))
        return fail(MI355CG_ERR_HIP, "block gram: allocation of the partials failed");
    launch_gram<false>(c->stream, c->g, G, la, lb, T.vec, T.part, T.mat);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(out, T.mat, sizeof(double) * la.n * lb.n, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return MI355CG_OK;
}

int mi355cg_block_gram(mi355cg_handle c, int na, const double* a, int nb, const double* b, double* out) {
    return mi355cg_block_gram_indexed(c, na, a, 0, nullptr, nb, b, 0, nullptr, out);
}

int mi355cg_block_combine(mi355cg_handle c, int k, const double* s, int m, const double* coef, double* y) {
    if (!c || !s || !coef || !y) return fail(MI355CG_ERR_INVALID, "null argument");
    if (k < 1 || k > kEigBasisMax) return fail(MI355CG_ERR_INVALID, "a combination has 1 .. %d inputs, not %d", kEigBasisMax, k);
    if (m < 1 || m > kEigBlockMax) return fail(MI355CG_ERR_INVALID, "a combination has 1 .. %d outputs, not %d", kEigBlockMax, m);
    if (int rc = block_check(c)) return rc;
    HIPCK(hipSetDevice(c->device));
    const long long vlen = round_up(c->storage_len, 32);
    const int G = std::min(c->g.N - 1, kMgMaxGrid);
    EigList ls{vlen, 0, {}}, ly{vlen, 0, {}};
    for (int i = 0; i < k; ++i) ls.idx[ls.n++] = i;
    for (int j = 0; j < m; ++j) ly.idx[ly.n++] = k + j;
    BlockTmp T;
    const double* src[1] = {s};
    const int counts[1] = {k};
    if (int rc = block_upload(c, T, k, m, src, counts, 1, vlen)) return rc;
    if (int rc = Buf<double>::device(T.mat, (long long)k * m, "block combine: allocation of the coefficients failed")) return rc;
    HIPCK(hipMemcpyAsync(T.mat, coef, sizeof(double) * k * m, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL((k_eig_combine<false>), dim3(G), dim3(kBlock), 0, c->stream, c->g, ls, (const double*)T.vec, (const double*)T.mat, m, ly, T.vec, ly,
                       (const double*)T.vec);
    hipLaunchKernelGGL(k_mgb_pack, dim3(flat_grid(c->pk_len), m), dim3(kBlock), 0, c->stream, c->pg, vlen, (const double*)(T.vec + (long long)k * vlen), T.packed);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(y, T.packed, sizeof(double) * c->pk_len * m, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return MI355CG_OK;
}

// ---- checksums (tests of large decomposed grids compare these instead of host copies of the vectors) -----------------
namespace {
struct hdd { double hi, lo; };
inline hdd hdd_add(hdd a, hdd b) {                  // same TwoSum-based addition as the device's dd_add (no contraction: -ffp-contract=off)
    const double s = a.hi + b.hi, bb = s - a.hi, e = (a.hi - (s - bb)) + (b.hi - bb);
    const double lo = e + (a.lo + b.lo), hi = s + lo;
    return hdd{hi, lo - (hi - s)};
}
// out[0] += sum of v, out[1] += sum of v^2 over the part's own cells, as double-double pairs.  Synchronises the part's stream.
int ctx_checksum(mi355cg_ctx* c, int which, hdd out[2]) {
    const double* v = which == 0 ? c->x : which == 1 ? c->r : which == 2 ? c->b : which == 3 ? c->u : nullptr;
    if (!v) return fail(MI355CG_ERR_INVALID, "checksum: vector %d (0 x, 1 r, 2 b, 3 u)", which);
    if (c->is_csr) return fail(MI355CG_ERR_INVALID, "checksum: grid handles only");
    HIPCK(hipSetDevice(c->device));
    if (c->is_slab) HIPCK(hipDeviceSynchronize());
    if (which == 3) if (int rc = ensure_u_on_device(c)) return rc;
    const int grid = 512;
    hipLaunchKernelGGL((k_checksum<double, 2>), dim3(grid), dim3(kBlock), 0, c->stream, kernel_geom<double, 2>(c), item_tab(c->whole), v, c->partR);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(c->partR_h, c->partR, sizeof(double) * 4 * grid, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    for (int b = 0; b < grid; ++b) {
        out[0] = hdd_add(out[0], hdd{c->partR_h[b], c->partR_h[grid + b]});
        out[1] = hdd_add(out[1], hdd{c->partR_h[2 * grid + b], c->partR_h[3 * grid + b]});
    }
    return MI355CG_OK;
}
}  // namespace

int mi355cg_checksum(mi355cg_handle c, int which, double* out2) {
    if (!c || !out2) return fail(MI355CG_ERR_INVALID, "null argument");
    hdd s[2] = {{0, 0}, {0, 0}};
    if (int rc = ctx_checksum(c, which, s)) return rc;
    out2[0] = s[0].hi + s[0].lo; out2[1] = s[1].hi + s[1].lo;
    return MI355CG_OK;
}

// ---- slab (one rank of a row-decomposed grid), driven phase by phase by the caller (iterative_solvers_amd/distributed.py) ----
int mi355cg_slab_rows(int n, int world, int rank, int* y_lo, int* y_hi) {
    GridParams gp;
    if (!grid_params_init(&gp, n, n, 0, 1, 0, 1)) return fail(MI355CG_ERR_INVALID, "grid %d rejected", n);
    if (world < 1 || rank < 0 || rank >= world || world > n - 1) return fail(MI355CG_ERR_INVALID, "bad world/rank %d/%d", rank, world);
    // contiguous row slabs balanced by unknown count (bottom rows hold n/2-1 unknowns, upper rows n-1)
    std::vector<int> first(world + 1);
    first[0] = 1; first[world] = n;
    for (int k = 1; k < world; ++k) {                         // smallest y with (unknowns in rows 1..y-1) >= k*U/world
        const long long target = (gp.size * k + world / 2) / world;
        int lo = 1, hi = n;
        while (lo < hi) { const int mid = (lo + hi) / 2; if (packed_row_begin(gp, mid) >= target) hi = mid; else lo = mid + 1; }
        first[k] = lo;
    }
    for (int k = 1; k < world; ++k) first[k] = std::max(first[k], first[k - 1] + 1);        // every rank non-empty
    for (int k = world - 1; k >= 1; --k) first[k] = std::min(first[k], first[k + 1] - 1);
    const int a = first[rank], b = first[rank + 1] - 1;
    if (y_lo) *y_lo = a;
    if (y_hi) *y_hi = b;
    return MI355CG_OK;
}

int mi355cg_owned_range(mi355cg_handle c, long long* packed_begin, long long* packed_len, int* y_lo, int* y_hi) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    if (packed_begin) *packed_begin = c->pk_begin;
    if (packed_len) *packed_len = c->pk_len;
    if (y_lo) *y_lo = c->g.y_lo;
    if (y_hi) *y_hi = c->g.y_hi;
    return MI355CG_OK;
}

// The dist entry points enqueue on the caller's stream, taken literally (NULL = HIP's default stream,
// which is also torch's default stream), so they order with the caller's collectives and copies.
static hipStream_t pick_stream(mi355cg_ctx*, void* stream) { return (hipStream_t)stream; }
// slots of a part's split launches: interior first, then edge
static Where part_where(const mi355cg_ctx* c, hipStream_t st, int rows) {
    if (rows == 1) return Where{st, &c->interior, 0};
    if (rows == 2) return Where{st, &c->edge, c->interior.grid};
    return Where{st, &c->whole, 0};
}
static int part_slots(const mi355cg_ctx* c, int rows) { return rows == 0 ? c->whole.grid : c->interior.grid + c->edge.grid; }

int mi355cg_dist_begin(mi355cg_handle c, const mi355cg_params* prm, void* stream) {
    if (!c || !prm) return fail(MI355CG_ERR_INVALID, "null argument");
    if (c->dtype != MI355CG_F64) return fail(MI355CG_ERR_INVALID, "slab mode is fp64 only");
    if (prm->diagnostics) return fail(MI355CG_ERR_INVALID, "per-iteration diagnostics are not available in slab mode");
    HIPCK(hipSetDevice(c->device));
    c->dist_prm = *prm; c->dist_active = true;
    const IterCfg cfg = make_cfg(prm);
    if (cfg.has_u) if (int rc = ensure_u_on_device(c)) return rc;
    hipStream_t st = pick_stream(c, stream);
    const size_t bytes = sizeof(double) * c->storage_len;
    HIPCK(hipMemsetAsync(c->x, 0, bytes, st));
    for (int k = 0; k < c->xsteps; ++k) HIPCK(hipMemsetAsync(c->p[k], 0, bytes, st));
    HIPCK(hipMemsetAsync(c->ap, 0, bytes, st));
    HIPCK(hipMemcpyAsync(c->r, c->b, bytes, hipMemcpyDeviceToDevice, st));
    c->cur = 0;
    c->nB_own = c->whole.grid;
    launch_update_flat<double, 2>(c, cfg, c->x, c->r, c->p[0], c->ap, c->u, st, c->whole.grid);
    HIPCK(hipGetLastError());
    c->solved = true;
    return MI355CG_OK;
}

// which: 0 = stencil partials (fields FA_*), 1 = update partials (fields FB_*).  Reduces this rank's
// partials into the head of its record (device).  with_rows != 0 also copies the rank's first and
// last owned row of the vector the neighbours need next (which 0: the direction the stencil just
// wrote, call after mi355cg_dist_flip; which 1: the residual) behind the sums, so ONE all-gather
// carries both the scalars and the halo.
int mi355cg_dist_reduce(mi355cg_handle c, int which, int with_rows, void* stream) {
    if (!c || !c->dist_active) return fail(MI355CG_ERR_STATE, "mi355cg_dist_begin has not run");
    hipStream_t st = pick_stream(c, stream);
    const Geom& g = c->g;
    RecordArgs a{};
    a.rec = which == 0 ? c->sumsA : c->sumsB; a.header = kRecHeader; a.row_slot = g.Pu;
    if (which == 0) { a.part = c->partA; a.n = c->nA_dist; a.stride = c->strideA; a.nsum = kNumSumsA; a.lo_off = FA_LO; a.max_first = 0; a.nmax = 0; }
    else { a.part = c->partB; a.n = c->nB_own; a.stride = c->strideB; a.nsum = kNumSumsB; a.lo_off = FB_LO; a.max_first = FB_RMAX; a.nmax = 3; }
    if (with_rows) {
        a.v = which == 0 ? c->p[c->cur] : c->r;
        a.off_lo = phys_start(g, g.y_lo) - g.base0; a.len_lo = g.y_lo <= g.half ? g.Pb : g.Pu;
        a.off_hi = phys_start(g, g.y_hi) - g.base0; a.len_hi = g.y_hi <= g.half ? g.Pb : g.Pu;
    }
    hipLaunchKernelGGL(k_make_record, dim3(with_rows ? 1 + 32 : 1), dim3(kBlock), 0, st, a);
    HIPCK(hipGetLastError());
    return MI355CG_OK;
}
int mi355cg_dist_record_layout(mi355cg_handle c, int* header, int* row_slot, int* width) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    if (header) *header = kRecHeader;
    if (row_slot) *row_slot = c->g.Pu;
    if (width) *width = c->rec_width;
    return MI355CG_OK;
}
int mi355cg_dist_sums_ptr(mi355cg_handle c, int which, void** dev_ptr, int* count) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    if (dev_ptr) *dev_ptr = which == 0 ? (void*)c->sumsA : (void*)c->sumsB;
    if (count) *count = c->rec_width;
    return MI355CG_OK;
}
// After all-gathering full records ([rank][rec_width]): copy the neighbours' boundary rows into this
// rank's ghost rows of `vector` (0 = r from update records, 1 = current direction from stencil records).
int mi355cg_dist_scatter_ghosts(mi355cg_handle c, int vector, const double* gathered, int nranks, int rank, void* stream) {
    if (!c || !gathered) return fail(MI355CG_ERR_INVALID, "null argument");
    if (rank < 0 || rank >= nranks) return fail(MI355CG_ERR_INVALID, "rank %d outside 0..%d", rank, nranks - 1);
    hipStream_t st = pick_stream(c, stream);
    const Geom& g = c->g;
    double* v = vector == 0 ? c->r : c->p[c->cur];
    const size_t W = (size_t)c->rec_width;
    ScatterArgs a{};
    if (rank > 0) {            // ghost row y_lo-1 = the lower neighbour's LAST owned row
        a.src_lo = gathered + W * (rank - 1) + kRecHeader + g.Pu;
        a.dst_lo = v + (phys_start(g, g.y_lo - 1) - g.base0);
        a.len_lo = (g.y_lo - 1) <= g.half ? g.Pb : g.Pu;
    }
    if (rank < nranks - 1) {   // ghost row y_hi+1 = the upper neighbour's FIRST owned row
        a.src_hi = gathered + W * (rank + 1) + kRecHeader;
        a.dst_hi = v + (phys_start(g, g.y_hi + 1) - g.base0);
        a.len_hi = (g.y_hi + 1) <= g.half ? g.Pb : g.Pu;
    }
    if (a.len_lo || a.len_hi) hipLaunchKernelGGL(k_scatter_ghosts, dim3(32), dim3(kBlock), 0, st, a);
    HIPCK(hipGetLastError());
    return MI355CG_OK;
}

// rows: 0 = whole slab, 1 = interior rows only, 2 = the first and last owned row (they read the
// neighbours' ghost rows).  A full stencil phase is either {0} or {1, 2}; call mi355cg_dist_flip once after it.
// `estride` = doubles between consecutive ranks' sums in `gathered_B` (FB_COUNT, or the record width).
int mi355cg_dist_stencil(mi355cg_handle c, const double* gathered_B, int nranks, int estride, int rows, void* stream) {
    if (!c || !c->dist_active || !gathered_B) return fail(MI355CG_ERR_STATE, "mi355cg_dist_begin has not run / null partials");
    const IterCfg cfg = make_cfg(&c->dist_prm);
    const PartSrc pb{gathered_B, nranks, 1, estride};
    launch_iteration_stencil<double, 2>(c, cfg, c->r, c->p, part_where(c, pick_stream(c, stream), rows), pb);
    c->nA_dist = part_slots(c, rows);
    HIPCK(hipGetLastError());
    return MI355CG_OK;
}
int mi355cg_dist_flip(mi355cg_handle c) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    c->cur = (c->cur + 1) % c->xsteps;
    return MI355CG_OK;
}
// rows: as in mi355cg_dist_stencil.  The update rebuilds A p from the stored direction, so its first and last owned row
// read the direction's ghost rows, which the stencil launch keeps up to date itself; a full update phase is {0} or {1, 2}.
int mi355cg_dist_update(mi355cg_handle c, const double* gathered_A, int nranks, int estride, int rows, void* stream) {
    if (!c || !c->dist_active || !gathered_A) return fail(MI355CG_ERR_STATE, "mi355cg_dist_begin has not run / null partials");
    IterCfg cfg = make_cfg(&c->dist_prm);
    const PartSrc pa{gathered_A, nranks, 1, estride};
    c->nB_own = part_slots(c, rows);
    launch_iteration_update<double, 2>(c, cfg, c->x, c->r, c->p, c->u, part_where(c, pick_stream(c, stream), rows), pa);
    HIPCK(hipGetLastError());
    return MI355CG_OK;
}
// Non-zero if the caller has to deliver the direction's ghost rows before the update's edge rows run.  Always 0: the
// stencil launch of a part keeps the new direction in its ghost rows itself (StencilArgs::store_ghosts).
int mi355cg_dist_update_reads_ghosts(mi355cg_handle c) {
    (void)c;
    return 0;
}
// Asynchronous: after the stream reaches this point the summary is in pinned host memory.
int mi355cg_dist_check(mi355cg_handle c, const double* gathered_B, int nranks, int estride, void* stream) {
    if (!c || !c->dist_active || !gathered_B) return fail(MI355CG_ERR_STATE, "mi355cg_dist_begin has not run / null partials");
    const IterCfg cfg = make_cfg(&c->dist_prm);
    hipStream_t st = pick_stream(c, stream);
    launch_check(c, cfg, st, PartSrc{gathered_B, nranks, 1, estride});
    return fetch_state(c, st);
}
// Call once after the loop (after the last mi355cg_dist_check has been synchronised): applies the x update
// that is still pending after an odd iteration count (REL_2NORM).  No-op otherwise.
int mi355cg_dist_finish(mi355cg_handle c, void* stream) {
    if (!c || !c->dist_active) return fail(MI355CG_ERR_STATE, "mi355cg_dist_begin has not run");
    const IterCfg cfg = make_cfg(&c->dist_prm);
    const CgState fin = *c->summary_h;
    c->cur = fin.it % c->xsteps;         // launches after the stop decision were no-ops but advanced the host-side index
    if (cfg.x2) {
        launch_flush_x<double, 2>(c, c->whole, c->x, c->p, fin, pick_stream(c, stream));
        HIPCK(hipGetLastError());
    }
    return MI355CG_OK;
}
int mi355cg_dist_summary(mi355cg_handle c, mi355cg_results* out, int* done) {
    if (!c || !out) return fail(MI355CG_ERR_INVALID, "null argument");
    const CgState fin = *c->summary_h;
    *out = make_results(fin, false, make_cfg(&c->dist_prm).has_u, fin.r0norm);      // the caller's loop decides about interruptions
    if (done) *done = fin.done;
    return MI355CG_OK;
}
int mi355cg_dist_history(mi355cg_handle c, int iteration, double* precision, double* residual, double* error) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    const HistEntry& h = c->hist_h[((iteration % kHist) + kHist) % kHist];
    if (precision) *precision = h.dmax;
    if (residual) *residual = h.rmax;
    if (error) *error = h.emax;
    return MI355CG_OK;
}
// Boundary rows for the halo exchange.  vector: 0 = residual r, 1 = the CURRENT direction (the one
// the last stencil wrote).  *_lo: row y_lo (send) and ghost row y_lo-1 (recv); *_hi: row y_hi and
// ghost row y_hi+1.  Counts are in doubles (the full stored row, pads included).
int mi355cg_dist_halo(mi355cg_handle c, int vector, void** send_lo, void** recv_lo, long long* n_lo,
                      void** send_hi, void** recv_hi, long long* n_hi) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    double* v = vector == 0 ? c->r : c->p[c->cur];
    const Geom& g = c->g;
    auto row_ptr = [&](int y) { return v + (phys_start(g, y) - g.base0); };
    auto row_len = [&](int y) -> long long { return y <= g.half ? g.Pb : g.Pu; };
    if (send_lo) *send_lo = row_ptr(g.y_lo);
    if (recv_lo) *recv_lo = row_ptr(g.y_lo - 1);
    if (send_hi) *send_hi = row_ptr(g.y_hi);
    if (recv_hi) *recv_hi = row_ptr(g.y_hi + 1);
    // a message is the SENDER's row; the receiver's ghost row has the same global index, hence the same length
    if (n_lo) *n_lo = row_len(g.y_lo);          // what this rank sends down; it receives row_len(y_lo-1)
    if (n_hi) *n_hi = row_len(g.y_hi);          // what this rank sends up;   it receives row_len(y_hi+1)
    return MI355CG_OK;
}
int mi355cg_dist_halo_recv_counts(mi355cg_handle c, long long* n_from_lo, long long* n_from_hi) {
    if (!c) return fail(MI355CG_ERR_INVALID, "null handle");
    const Geom& g = c->g;
    if (n_from_lo) *n_from_lo = (g.y_lo - 1) <= g.half ? g.Pb : g.Pu;
    if (n_from_hi) *n_from_hi = (g.y_hi + 1) <= g.half ? g.Pb : g.Pu;
    return MI355CG_OK;
}

}  // extern "C"

#include "team.h"
