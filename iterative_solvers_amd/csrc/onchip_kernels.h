// onchip_kernels.h -- a chunk of CG iterations inside ONE workgroup: plain fp64 grid handles up to N = kOnchipMaxN.
//
// One launch of one workgroup runs up to `m` iterations.  The direction lives in LDS as an (N+1) x (N+1) image with zeros where the
// grid has boundary nodes or no nodes (onchip_plan.h); every thread keeps x, r (and u when the error norm is read) of its unknowns in
// registers.  Nothing but __syncthreads() orders the threads: three barriers per iteration --
//   1  after the new direction z = r + beta*z is in the image (the stencil reads neighbours),
//   2  after the waves' partials of (Az, z) [and (r, z)] are in LDS,
//   3  after the waves' partials of (r, r), |r|, |dx|, |x - u| and the sampled stop word are in LDS
// -- each reduction combining all its fields behind its one barrier.  The three partial areas and the image are distinct, and between
// two uses of any of them lie two other barriers, so no barrier is needed to "protect the previous use".
//
// Entry and exit are the iteration-boundary state of the two-launch path (cg_kernels.h): x, r and the direction of iteration `it` in
// the handle's storage layout (the direction in ring slot it % xsteps), the CgState the update launch leaves in sB, the update
// partials in partB (any number of slots at entry, ONE slot at exit).  Every element-wise expression is that path's, in its order,
// decisions come from decide_after_update and the state is written by write_state_after_decision; the inner products are double-double
// pairs, whose rounded value does not depend on the order of summation.  Hence the same bits as k_stencil + k_update_st, step by step.
//
// The iteration is written once, in oc_chunk.  k_onchip runs it on the handle's own vectors; k_onchip_many on
// system blockIdx.x of a batch of independent systems of one grid -- own right-hand side, guess and diagonal each --, with an LDS
// allocation that follows N, so that small grids share a CU; k_onchip_many_init starts all systems of a batch on the device;
// k_onchip_steps alternates it with the start of the next time step of member blockIdx.x of an ensemble, so
// that a workgroup takes its member through all its steps inside the launches.
#pragma once
#include "cg_kernels.h"
#include "onchip_plan.h"

namespace mi355cg {

struct OnchipArgs {
    Geom g;
    OnchipPlan pl;
    double* x; double* r;
    double* p[kRing]; int xsteps;        // the direction ring: the direction of iteration k is in p[k % xsteps]
    const double* u;
    double* partB; int nB, strideB;      // update partials: nB slots at entry, one at exit
    CgState* s;                          // the state at the iteration boundary (the handle's sB)
    HistEntry* hist;
    RuleParams rp;
    int has_u;                           // the solve reads u at all ...
    int u_always, every;                 // ... on every iteration / on iteration 1 and every `every`-th (mi355cg_solve: need_u)
    int m;                               // iterations of this chunk
    const int* stop_req;                 // pinned host word, sampled once per iteration by one lane; may be null
};

constexpr int kOcWaves = kOnchipMaxThreads / kWave;
constexpr int kOcFieldsA = 4, kOcFieldsB = 10;
static_assert(kOcWaves * (kOcFieldsA + kOcFieldsB) * 8 + (int)sizeof(CgState) <= kOnchipSideBytes, "onchip_plan.h: the side data");

struct OcSumsA { dd pap, rz; };
struct OcSumsB { dd rr, d2, e2; double rmax, dmax, emax, stop; };

// All threads get the workgroup totals: lane tree inside a wave, the waves' partials through LDS behind one barrier, waves in order.
template <bool MSG>
__device__ inline OcSumsA oc_reduce_a(OcSumsA v, double* scr, int nwaves) {
    v.pap = wave_sum_dd(v.pap);
    if (MSG) v.rz = wave_sum_dd(v.rz);
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    if (lane == 0) { double* o = scr + w * kOcFieldsA; o[0] = v.pap.hi; o[1] = v.pap.lo; o[2] = v.rz.hi; o[3] = v.rz.lo; }
    __syncthreads();
    OcSumsA t{dd{scr[0], scr[1]}, dd{scr[2], scr[3]}};
#pragma unroll 1
    for (int k = 1; k < nwaves; ++k) {
        const double* o = scr + k * kOcFieldsA;
        t.pap = dd_add(t.pap, dd{o[0], o[1]});
        if (MSG) t.rz = dd_add(t.rz, dd{o[2], o[3]});
    }
    return t;
}
// FULL: all fields (the MSG rule's update, the partials found at entry); otherwise (r, r) and |r| only -- the others are zero.
// In two halves, so that the totals need not stay in registers: the exit combines the last partials once more.
template <bool FULL>
__device__ inline OcSumsB oc_combine_b(const double* scr, int nwaves) {
    OcSumsB t{dd{scr[0], scr[1]}, dd_zero(), dd_zero(), scr[2], 0.0, 0.0, scr[3]};
    if (FULL) { t.d2 = dd{scr[4], scr[5]}; t.e2 = dd{scr[6], scr[7]}; t.dmax = scr[8]; t.emax = scr[9]; }
#pragma unroll 1
    for (int k = 1; k < nwaves; ++k) {
        const double* o = scr + k * kOcFieldsB;
        t.rr = dd_add(t.rr, dd{o[0], o[1]}); t.rmax = fmax(t.rmax, o[2]);
        if (FULL) {
            t.d2 = dd_add(t.d2, dd{o[4], o[5]}); t.e2 = dd_add(t.e2, dd{o[6], o[7]});
            t.dmax = fmax(t.dmax, o[8]); t.emax = fmax(t.emax, o[9]);
        }
    }
    return t;
}
template <bool FULL>
__device__ inline void oc_publish_b(OcSumsB v, double* scr) {
    v.rr = wave_sum_dd(v.rr); v.rmax = wave_max(v.rmax);
    if (FULL) { v.d2 = wave_sum_dd(v.d2); v.e2 = wave_sum_dd(v.e2); v.dmax = wave_max(v.dmax); v.emax = wave_max(v.emax); }
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    if (lane == 0) {
        double* o = scr + w * kOcFieldsB;
        o[0] = v.rr.hi; o[1] = v.rr.lo; o[2] = v.rmax; o[3] = v.stop;             // stop: thread 0's sample, 0 elsewhere
        if (FULL) { o[4] = v.d2.hi; o[5] = v.d2.lo; o[6] = v.e2.hi; o[7] = v.e2.lo; o[8] = v.dmax; o[9] = v.emax; }
    }
    __syncthreads();
}

// ---- what the chunk body reads of the system it iterates on ---------------------------------------------------------------------
// k_onchip: the handle's vectors in storage layout, its direction ring, its history ring, the diagonal of its Geom.
struct OcLds { double* img; double* scrA; double* scrB; CgState* st; };
struct OcOne {
    static constexpr bool kMany = false;
    // the image of the largest grid, statically: one workgroup per CU whatever N is
    __device__ static __forceinline__ OcLds lds(int /*cells*/) {
        __shared__ double img[kOnchipMaxCells];
        __shared__ double scrA[kOcWaves * kOcFieldsA], scrB[kOcWaves * kOcFieldsB];
        __shared__ CgState st;
        return OcLds{img, scrA, scrB, &st};
    }
    typedef OnchipArgs Args;
    // (accessors over the arguments, not a copy of them in a struct of its own: that cost k_onchip<24, false> five words of scratch)
    __device__ static double* x(const Args& a) { return a.x; }
    __device__ static double* r(const Args& a) { return a.r; }
    __device__ static const double* u(const Args& a) { return a.u; }
    __device__ static double* partB(const Args& a) { return a.partB; }
    __device__ static int nB(const Args& a) { return a.nB; }
    __device__ static int strideB(const Args& a) { return a.strideB; }
    __device__ static CgState* s(const Args& a) { return a.s; }
    __device__ static HistEntry* hist(const Args& a) { return a.hist; }
    __device__ static double cA(const Args& a) { return a.g.A; }
    __device__ static double cxk(const Args& a) { return a.g.xk; }
    __device__ static double cyk(const Args& a) { return a.g.yk; }
    __device__ static int has_u(const OnchipArgs& a) { return a.has_u; }
    __device__ static int u_always(const OnchipArgs& a) { return a.u_always; }
    __device__ static int every(const OnchipArgs& a) { return a.every; }
    __device__ static double* dir(const OnchipArgs& a, int it) { return a.p[it % a.xsteps]; }
    __device__ static long long off(const OnchipArgs& a, int /*i*/, int xx, int yy) { return (long long)(row_off(a.g, yy) + xx - a.g.base0); }
    __device__ static void finished(const Args&) {}
    __device__ static int budget(const Args& a) { return a.m; }                            // iterations of this chunk
    __device__ static int tid() { return threadIdx.x; }
    __device__ static StateLite state(const Args& a) { return load_state_lite(a.s); }
};
// k_onchip_many: system blockIdx.x of a batch.  Vectors in PACKED order (unknown i of onchip_plan.h at i: the
// order of the host interface), one direction buffer, one slot of partials, no history ring, the diagonal from a device array.
struct OnchipManyArgs {
    OnchipPlan pl;
    double xk, yk;
    const double* diag;                  // nsys: A_diag - sigma_s, rounded on the host
    double* x; double* r; double* p;     // nsys vectors of `stride` doubles each
    long long stride;
    double* partB;                       // nsys x FB_COUNT (field-major with stride 1)
    CgState* s;                          // nsys: the states at the iteration boundary
    CgState* summary;                    // nsys: what the end-of-chunk check of a single solve leaves for the host
    int* done_count;                     // systems whose state says done
    RuleParams rp;
    int m;
    const int* stop_req;
};
struct OcMany {
    static constexpr bool kMany = true;
    typedef OnchipManyArgs Args;
    // All LDS is the dynamic region of onchip_many_lds_bytes(n) bytes, so that small grids share a CU: the side data at fixed
    // offsets, then the image of THIS grid.
    __device__ static __forceinline__ OcLds lds(int /*cells*/) {
        extern __shared__ __attribute__((aligned(16))) char oc_dyn_lds[];
        double* side = reinterpret_cast<double*>(oc_dyn_lds);
        return OcLds{reinterpret_cast<double*>(oc_dyn_lds + kOnchipSideBytes), side, side + kOcWaves * kOcFieldsA,
                     reinterpret_cast<CgState*>(side + kOcWaves * (kOcFieldsA + kOcFieldsB))};
    }
    __device__ static long long sys() { return blockIdx.x; }
    __device__ static double* x(const Args& a) { return a.x + sys() * a.stride; }
    __device__ static double* r(const Args& a) { return a.r + sys() * a.stride; }
    __device__ static const double* u(const Args&) { return nullptr; }
    __device__ static double* partB(const Args& a) { return a.partB + sys() * FB_COUNT; }
    __device__ static int nB(const Args&) { return 1; }
    __device__ static int strideB(const Args&) { return 1; }
    __device__ static CgState* s(const Args& a) { return a.s + sys(); }
    __device__ static CgState* summary(const Args& a) { return a.summary + sys(); }
    __device__ static HistEntry* hist(const Args&) { return nullptr; }
    __device__ static double cA(const Args& a) { return a.diag[sys()]; }
    __device__ static double cxk(const Args& a) { return a.xk; }
    __device__ static double cyk(const Args& a) { return a.yk; }
    __device__ static int has_u(const OnchipManyArgs&) { return 0; }
    __device__ static int u_always(const OnchipManyArgs&) { return 0; }
    __device__ static int every(const OnchipManyArgs&) { return 0; }
    __device__ static double* dir(const OnchipManyArgs& a, int) { return a.p + sys() * a.stride; }
    __device__ static long long off(const OnchipManyArgs&, int i, int, int) { return i; }
    __device__ static void finished(const Args& a) { atomicAdd(a.done_count, 1); }       // thread 0, once per system: the launch in which its state turns done
    __device__ static int budget(const Args& a) { return a.m; }
    __device__ static int tid() { return threadIdx.x; }
    __device__ static StateLite state(const Args& a) { return load_state_lite(s(a)); }
};

// The iteration body, written once.  Its LDS is the system type's (Sys::lds): img, pl.cells doubles; scrA, scrB, kOcWaves x
// kOcFieldsA / kOcFieldsB doubles; st, the CG state, in LDS while the chunk runs.  ONE object: write_state_after_decision is handed
// it as source and destination, so its copy is a copy onto itself and only the fields it sets are stored (two objects cost 46
// registers per copy, in mid-loop).
// E: slots per thread (OnchipPlan::elems).  MSG: the max-norm rule -- x and its norms every iteration, (r, z) reduced, u in registers.
// Sys::kMany: the chunk also takes the closing decision a single solve leaves to k_check, per system: the state after the last update
// goes to y.s as it is, the decided state to y.summary, and to y.s as well if it says done (what the next chunk's first decision
// would write: the same numbers decided again).
template <int E, bool MSG, class Sys>
__device__ __forceinline__ void oc_chunk(const typename Sys::Args a) {
    // (The kernel's arguments by value and as a whole, untouched by the kernel itself: the body is optimized before it is inlined.
    // Behind a reference every load of an argument is a load that any store may have changed -- 60 more registers at E = 16, and
    // scratch; and a kernel that reads single fields has its copy cut up, after which the body's copy stays in scratch.)
    const int has_u = Sys::has_u(a), u_always = Sys::u_always(a), every = Sys::every(a);
    const OnchipPlan& pl = a.pl;
    const RuleParams& rp = a.rp;
    const int m = Sys::budget(a);
    const int* const stop_req = a.stop_req;
    const OcLds lds = Sys::lds(pl.cells);
    double* const img = lds.img; double* const scrA = lds.scrA; double* const scrB = lds.scrB; CgState* const st = lds.st;
    static_assert(sizeof(CgState) % sizeof(double) == 0, "the state travels as doubles");
    constexpr int kStateWords = (int)(sizeof(CgState) / sizeof(double));
    const int t = Sys::tid(), T = blockDim.x, nwaves = T / kWave;
    StateLite s = Sys::state(a);
    if (s.done) return;                                // the state already says done: x, r, the state and the partials stay
    const bool use_u = MSG && has_u;

    for (int i = t; i < pl.cells; i += T) img[i] = 0.0;
    if (t < kStateWords) reinterpret_cast<double*>(st)[t] = reinterpret_cast<const double*>(Sys::s(a))[t];      // (thread 0 reads it behind two barriers)
    // the partials the launch before left (the init pass: one slot per workgroup of it; an on-chip chunk: one slot)
    OcSumsB v0{dd_zero(), dd_zero(), dd_zero(), 0.0, 0.0, 0.0, 0.0};
    for (int i = t; i < Sys::nB(a); i += T) {
        const double* q = Sys::partB(a) + i;
        const int sb = Sys::strideB(a);
        v0.rr = dd_add(v0.rr, dd{q[FB_RR * sb], q[(FB_RR + FB_LO) * sb]});
        v0.d2 = dd_add(v0.d2, dd{q[FB_D2 * sb], q[(FB_D2 + FB_LO) * sb]});
        v0.e2 = dd_add(v0.e2, dd{q[FB_E2 * sb], q[(FB_E2 + FB_LO) * sb]});
        v0.rmax = fmax(v0.rmax, q[FB_RMAX * sb]); v0.dmax = fmax(v0.dmax, q[FB_DMAX * sb]); v0.emax = fmax(v0.emax, q[FB_EMAX * sb]);
    }
    __syncthreads();                                   // the image is zero everywhere before the owners fill their cells

    // this thread's unknowns: image cell, x, r [, u] from the system's vectors into registers, the direction into the image
    auto storage_off = [&](int i) { int xx, yy; onchip_node(pl, i, &xx, &yy); return Sys::off(a, i, xx, yy); };
    unsigned cell2[(E + 1) / 2] = {};                   // image cells, two 16-bit indices per register (kOnchipMaxCells < 65536)
    static_assert(kOnchipMaxCells <= 0x10000, "a cell index fits in 16 bits");
    double x[E], r[E], u[MSG ? E : 1];
    int cnt = 0;                                       // valid slots: a prefix
    const double* pin = Sys::dir(a, s.it);
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int i = onchip_owned(pl, t, k);
        x[k] = 0.0; r[k] = 0.0;
        if (MSG) u[k] = 0.0;
        if (i >= 0) {
            int xx, yy;
            onchip_node(pl, i, &xx, &yy);
            const int c = onchip_cell(pl, xx, yy);
            cell2[k / 2] |= (unsigned)c << (16 * (k & 1));
            const long long off = Sys::off(a, i, xx, yy);
            x[k] = Sys::x(a)[off]; r[k] = Sys::r(a)[off]; img[c] = pin[off];
            if (use_u) u[k] = Sys::u(a)[off];
            cnt = k + 1;
        }
    }
    oc_publish_b<true>(v0, scrB);
    // what the next decision needs of the totals: (r, r), and under MSG the three max-norms
    double rr, rmax = 0, dmax = 0, emax = 0;
    { const OcSumsB tot = oc_combine_b<MSG>(scrB, nwaves); rr = dd_value(tot.rr); if (MSG) { rmax = tot.rmax; dmax = tot.dmax; if (rp.use_u) emax = tot.emax; } }

    const double cA = Sys::cA(a), cxk = Sys::cxk(a), cyk = Sys::cyk(a);
    const int pitch = pl.pitch;
    // A z at an owned cell: the stencil launch's formula, verbatim (every owned node is interior: nothing to mask)
    auto apply_at = [&](int c, double cc) {
        double v = cA * cc;
        v = v + cxk * img[c - 1];
        v = v + cxk * img[c + 1];
        v = v + cyk * img[c + pitch];                  // row y+1
        v = v + cyk * img[c - pitch];                  // row y-1
        return v;
    };

    // What a slot's loop body starts from: the cell index, opaque to the optimizer.  Otherwise it keeps the five LDS addresses of
    // every slot (and the storage offsets the exit needs) in registers across the whole iteration loop, and spills them.
    auto own_cell = [&](int k) { unsigned c2 = cell2[k / 2]; asm volatile("" : "+v"(c2)); return (int)((c2 >> (16 * (k & 1))) & 0xffffu); };
    int ran = 0;
    bool decided = false;                              // the loop ended on a decision that says done
    for (int it_k = 0; it_k < m; ++it_k) {
        // the stop request (a pinned HOST word): one lane asks now and hands the answer to the update reduction
        double stop_word = 0.0;
        if (t == 0 && stop_req) stop_word = __hip_atomic_load(stop_req, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0 ? 1.0 : 0.0;

        // ---- the stencil launch's prologue: decide from the update partials (reduce_and_decide without diagnostics)
        const Decision d = decide_after_update(s, rp, rr, rmax, dmax, emax, 0.0, 0.0);
        if (t == 0) write_state_after_decision<true>(st, Sys::hist(a), st, s, d);
        if (d.done) { if constexpr (Sys::kMany) decided = true; break; }
        const double beta = d.beta;

        // ---- phase A': z = r + beta*z, (Az, z) [and (r, z)]
#pragma unroll
        for (int k = 0; k < E; ++k) if (k < cnt) { const int c = own_cell(k); img[c] = r[k] + beta * img[c]; }        // z = r + beta*z
        __syncthreads();                                                                              // barrier 1
        OcSumsA va{dd_zero(), dd_zero()};
#pragma unroll
        for (int k = 0; k < E; ++k) if (k < cnt) {
            const int c = own_cell(k);
            const double cc = img[c];
            const double ap = apply_at(c, cc);
            dd_acc_prod(va.pap, cc, ap);
            if (MSG) dd_acc_prod(va.rz, r[k], cc);
            __builtin_amdgcn_sched_barrier(0);
        }
        const OcSumsA ta = oc_reduce_a<MSG>(va, scrA, nwaves);                                        // barrier 2
        const double pap = dd_value(ta.pap);
        double rz = 0.0, alpha_d;
        if (MSG) { rz = dd_value(ta.rz); alpha_d = rz / pap; }                                        // msg_solver.cpp:102
        else alpha_d = d.rr / pap;                                                                    // matrix_free_system.cpp:419
        const double alpha = alpha_d;

        // ---- phase B: r -= alpha*Az (A z rebuilt from the image: same operands, same order), x += alpha*z, the norms
        const int it_new = s.it + 1;
        const bool u_now = use_u && (u_always || it_new == 1 || (every > 0 && it_new % every == 0));
        OcSumsB vb{dd_zero(), dd_zero(), dd_zero(), 0.0, 0.0, 0.0, stop_word};
#pragma unroll
        for (int k = 0; k < E; ++k) if (k < cnt) {
            const int c = own_cell(k);
            const double cc = img[c];
            const double apj = apply_at(c, cc);
            const double rn = r[k] - alpha * apj;                  // r = r - alpha*A_z      msg_solver.cpp:110-112
            dd_acc_prod(vb.rr, rn, rn);
            vb.rmax = fmax(vb.rmax, fabs(rn));
            const double xn = x[k] + alpha * cc;                   // x = x + alpha*z        msg_solver.cpp:105-107
            if (MSG) {
                const double dx = xn - x[k];                       // diff = x - x_prev      msg_solver.cpp:124-127
                vb.dmax = fmax(vb.dmax, fabs(dx));
                dd_acc_prod(vb.d2, dx, dx);
                if (u_now) {
                    const double ee = xn - u[k];                   // error = x - u          msg_solver.cpp:132-136
                    vb.emax = fmax(vb.emax, fabs(ee));
                    dd_acc_prod(vb.e2, ee, ee);
                }
            }
            r[k] = rn; x[k] = xn;
            __builtin_amdgcn_sched_barrier(0);
        }
        oc_publish_b<MSG>(vb, scrB);                                                                  // barrier 3
        int stop;
        { const OcSumsB tot = oc_combine_b<MSG>(scrB, nwaves); rr = dd_value(tot.rr); stop = tot.stop != 0.0; if (MSG) { rmax = tot.rmax; dmax = tot.dmax; if (rp.use_u) emax = tot.emax; } }
        if (t == 0) {                                              // what the update launch writes
            CgState* o = st;
            o->it = it_new; o->first = 0; o->alpha = alpha_d; o->rz = rz; o->alpha_hist[it_new & (kRing - 1)] = alpha_d;
            o->stop = stop;                                        // the reference tests its flag once per iteration (msg_solver.cpp:82-87)
        }
        s.rr_prev = s.rr; s.rr = d.rr; s.r0norm = d.r0norm;        // what the next decision reads back from that state
        s.alpha = alpha_d; s.rz = rz; s.it = it_new; s.first = 0; s.stop = stop;
        ++ran;
    }

    // ---- exit: the iteration-boundary state, for the host, the next chunk or the two-launch path
    if (ran > 0) {
        double* pout = Sys::dir(a, s.it);
#pragma unroll
        for (int k = 0; k < E; ++k) if (k < cnt) {
            int i = k * T + t;
            asm volatile("" : "+v"(i));                            // recomputed here, not carried through the loop
            const long long off = storage_off(i);
            Sys::x(a)[off] = x[k]; Sys::r(a)[off] = r[k]; pout[off] = img[own_cell(k)];
        }
    }
    __syncthreads();                                               // thread 0's last state stores
    if (t < kStateWords) reinterpret_cast<double*>(Sys::s(a))[t] = reinterpret_cast<const double*>(st)[t];
    if (t == 0) {
        // the partials of the last update (no update ran: of the launch before), all fields, as one slot
        const OcSumsB tot = (MSG || ran == 0) ? oc_combine_b<true>(scrB, nwaves) : oc_combine_b<false>(scrB, nwaves);
        const int sb = Sys::strideB(a);
        Sys::partB(a)[FB_RR * sb] = tot.rr.hi; Sys::partB(a)[(FB_RR + FB_LO) * sb] = tot.rr.lo;
        Sys::partB(a)[FB_D2 * sb] = tot.d2.hi; Sys::partB(a)[(FB_D2 + FB_LO) * sb] = tot.d2.lo;
        Sys::partB(a)[FB_E2 * sb] = tot.e2.hi; Sys::partB(a)[(FB_E2 + FB_LO) * sb] = tot.e2.lo;
        Sys::partB(a)[FB_RMAX * sb] = tot.rmax; Sys::partB(a)[FB_DMAX * sb] = tot.dmax; Sys::partB(a)[FB_EMAX * sb] = tot.emax;
    }
    if constexpr (Sys::kMany) {
        // ---- the closing decision (k_check's: the same numbers the next chunk's first decision would see, without advancing)
        bool done_now = decided;
        if (!decided) {
            // k_check reduces the max-norms and (dx, dx) of the last update's partials under either rule (REL_2NORM: |r| is there, the
            // x norms are zeros); scrB still holds them: m >= 1 iterations ran
            const OcSumsB tot = oc_combine_b<MSG>(scrB, nwaves);
            const Decision d = decide_after_update(s, rp, dd_value(tot.rr), tot.rmax, tot.dmax, 0.0, dd_value(tot.d2), 0.0);
            __syncthreads();                                       // the copy of the undecided state above has read st
            if (t == 0) write_state_after_decision<true>(st, nullptr, st, s, d);
            __syncthreads();
            done_now = d.done != 0;
        }
        if (t < kStateWords) {
            const double w = reinterpret_cast<const double*>(st)[t];
            reinterpret_cast<double*>(Sys::summary(a))[t] = w;
            if (done_now) reinterpret_cast<double*>(Sys::s(a))[t] = w;   // the same lanes that stored the undecided words: in program order
        }
        if (t == 0 && done_now) Sys::finished(a);
    }
}

template <int E, bool MSG>
__global__ __launch_bounds__(kOnchipMaxThreads) void k_onchip(const OnchipArgs a) {
    oc_chunk<E, MSG, OcOne>(a);
}

// ---- many systems, one workgroup each ---------------------------------------------------------------------
static_assert(sizeof(CgState) <= 256 && 2 * (int)sizeof(CgState) + (FB_COUNT + 2) * 8 == kOnchipManySysBytes, "onchip_plan.h: a system's share of the batch workspace");
template <int E, bool MSG>
__global__ __launch_bounds__(kOnchipMaxThreads) void k_onchip_many(const OnchipManyArgs a) {
    oc_chunk<E, MSG, OcMany>(a);
}

// The start of a batch, one workgroup (of the plan's size) per system: what k_init_fresh, or launch_apply + k_init_guess +
// k_guess_state, leave for a single solve.  Cold: x = 0, r = b, z = 0.  WARM: x = x0, r = b - A x0 in one rounding with A x0 by the
// stencil formula from an image of x0, (b, b) beside (r, r), first = 2 with the reference norm ||b||_2, norm0 = ||r0||_2.  The sums
// are double-double pairs, so their rounded values are those of the flat passes although the elements are dealt differently.
// A warm MSG system gets the poll of mi355cg_solve too: the decision on the start state goes to its summary, with the start-state
// tests (msg_stop_reason without a precision) applied; one that is done never iterates.
struct OnchipManyInitArgs {
    OnchipPlan pl;
    double xk, yk;
    const double* diag;
    const double* b; const double* x0;   // nsys packed vectors of `stride` doubles each, like x, r, p (x0: WARM only)
    double* x; double* r; double* p;
    long long stride;
    double* partB; CgState* s; CgState* summary; double* norm0; int* done_count;
    RuleParams rp;
};
// Where the start takes b from.  OcBVector: a packed vector.  OcBStep: the right-hand side of a theta-scheme step, formed in
// registers from the image of the state (which the warm start holds anyway) and the forcing g -- it is never stored, CG needs only
// r and ||b||_2.  The step's expression is onchip_step_rhs (onchip_plan.h), k_step_rhs's: the neighbours in that order.
struct OcBVector {
    const double* b;
    __device__ double at(int i, int, const double*, int) const { return b[i]; }
};
struct OcBStep {
    const double* g; OnchipStepCoef k; double sigma;
    __device__ double at(int i, int c, const double* img, int pitch) const {
        return onchip_step_rhs(k, sigma, g[i], img[c], img[c - 1], img[c + 1], img[c - pitch], img[c + pitch]);
    }
};
// One system's share of the workspace, as the start writes it.  COUNT: a system whose start state says done is counted in
// *done_count (a batch: it is finished; a stepping member is not: its next step follows).
struct OcStartOut { double* x; double* r; double* p; double* partB; CgState* s; CgState* summary; double* norm0; int* done_count; };
template <bool WARM, bool COUNT, class B>
__device__ __forceinline__ void oc_start(const OnchipPlan& pl, const OcLds& l, const RuleParams& rp, double diag, double cxk, double cyk,
                                         const double* x0, const OcStartOut& o, const B& bsrc, int t) {
    const int T = blockDim.x, nwaves = T / kWave;
    if (WARM) {
        for (int i = t; i < pl.cells; i += T) l.img[i] = 0.0;
        __syncthreads();
        for (int i = t; i < pl.unknowns; i += T) { int xx, yy; onchip_node(pl, i, &xx, &yy); l.img[onchip_cell(pl, xx, yy)] = x0[i]; }
        __syncthreads();
    }
    const double cA = WARM ? diag : 0.0;
    const int pitch = pl.pitch;
    OcSumsB v{dd_zero(), dd_zero(), dd_zero(), 0.0, 0.0, 0.0, 0.0};       // d2 carries (b, b)
    for (int i = t; i < pl.unknowns; i += T) {
        int c = 0;
        if (WARM) { int xx, yy; onchip_node(pl, i, &xx, &yy); c = onchip_cell(pl, xx, yy); }
        const double bv = bsrc.at(i, c, l.img, pitch);
        double rv = bv, xv = 0.0;
        if (WARM) {
            xv = l.img[c];
            double ax = cA * xv;                                   // apply_at of the chunk body: k_stencil's formula
            ax = ax + cxk * l.img[c - 1];
            ax = ax + cxk * l.img[c + 1];
            ax = ax + cyk * l.img[c + pitch];
            ax = ax + cyk * l.img[c - pitch];
            rv = bv - ax;                                          // r = b - A*x       matrix_free_system.cpp:389-392
            dd_acc_prod(v.d2, bv, bv);
        }
        dd_acc_prod(v.rr, rv, rv);
        v.rmax = fmax(v.rmax, fabs(rv));
        o.x[i] = xv; o.r[i] = rv; o.p[i] = 0.0;
    }
    oc_publish_b<true>(v, l.scrB);
    if (t != 0) return;
    const OcSumsB tot = oc_combine_b<true>(l.scrB, nwaves);
    double* q = o.partB;
    q[FB_RR] = tot.rr.hi; q[FB_RR + FB_LO] = tot.rr.lo;
    q[FB_D2] = 0.0; q[FB_D2 + FB_LO] = 0.0; q[FB_E2] = 0.0; q[FB_E2 + FB_LO] = 0.0;
    q[FB_RMAX] = tot.rmax; q[FB_DMAX] = 0.0; q[FB_EMAX] = 0.0;
    const double rr = dd_value(tot.rr);
    CgState* sp = o.s;
    *sp = CgState{};
    sp->first = 1;
    *o.norm0 = sqrt(rr);
    if (WARM) {
        sp->r0norm = sqrt(dd_value(tot.d2)); sp->first = 2;
        if (rp.rule == 0 /*MSG_MAXNORM*/) {
            StateLite s{};
            s.r0norm = sp->r0norm; s.first = 2;
            const Decision d = decide_after_update(s, rp, rr, tot.rmax, 0.0, 0.0, 0.0, 0.0);
            const bool met = !rp.fixed_iterations && rp.eps_residual > 0 && tot.rmax < rp.eps_residual;      // msg_stop_reason(prm, false, ..)
            CgState* sm = o.summary;
            write_state_after_decision<true>(sm, nullptr, sp, s, d);
            if (met) { sm->done = 1; sm->converged = 1; sm->reason = 2 /*RESIDUAL*/; }
            if (d.done || met) { *sp = *sm; if (COUNT) atomicAdd(o.done_count, 1); }
        }
    }
}
template <bool WARM>
__global__ __launch_bounds__(kOnchipMaxThreads) void k_onchip_many_init(const OnchipManyInitArgs a) {
    const long long sys = blockIdx.x, base = sys * a.stride;
    const OcStartOut o{a.x + base, a.r + base, a.p + base, a.partB + sys * FB_COUNT, a.s + sys, a.summary + sys, a.norm0 + sys, a.done_count};
    oc_start<WARM, true>(a.pl, OcMany::lds(a.pl.cells), a.rp, WARM ? a.diag[sys] : 0.0, a.xk, a.yk, WARM ? a.x0 + base : nullptr, o,
                         OcBVector{a.b + base}, threadIdx.x);
}

// ---- ensemble time stepping: the step loop inside the launch ----------------------------------------------
// Member blockIdx.x of an ensemble on one grid is integrated over nsteps theta-scheme steps of u_t = A u - g_s with its own step
// tau_s: every step is the warm-started solve of (A - sigma_s I) u' = b_step(u), sigma_s = 1 / (theta tau_s), that
// mi355cg_time_steps runs on a handle, and ONE workgroup takes the member from its first step to its last.  A launch gives each
// member `m` units: a CG iteration costs one, the transition from a converged step to the next costs one, so a launch is bounded by
// m whatever happens (runs of 0-iteration steps included).  The kernel alternates oc_chunk on the member's workspace (x, r, the
// direction, the state: what a batch keeps per system) with the transition: record the step, the new state u = x from the
// workspace into the image, b_step in registers, the warm start of k_onchip_many_init on it (oc_start).  A member ends after its
// last step or after the first step that does not converge (iteration cap, stop request) and is then counted in *done_count, once.
struct OnchipStepsArgs {                 // (its own copies of what it shares with OnchipManyArgs: the chunk's arguments stay whole)
    OnchipPlan pl;
    double xk, yk;
    const double* diag; const double* sigma;         // nsys each: A_diag - sigma_s as mi355cg_set_shift rounds it; sigma_s
    const double* g; long long g_stride;             // forcing: member s reads g + s * g_stride (0: one vector for all)
    const double* u0;                                // k_onchip_steps_init: nsys packed start states of `stride` doubles
    double* x; double* r; double* p;
    long long stride;
    double* partB; CgState* s; CgState* summary; double* norm0; int* done_count;
    OcStepBook* book;                                // nsys
    int* step_it; int nsteps;                        // nsys x nsteps iteration counts, or null
    OnchipStepCoef k;
    RuleParams rp;
    int m;                                           // units of this launch
};
__device__ inline int oc_wg_load(const int* p) {     // what a thread of this workgroup stored before the last barrier; uniform
    return __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}
// The system type of a stepping member: a batch's system, whose chunk length is what is left of the launch's budget (a word of the
// LDS side data, written before the barrier in front of the chunk) and whose state is re-read after stores of this very launch --
// with vector loads: the scalar cache is only invalidated at kernel start.  The step kernel counts finished members itself.
struct OcSteps : OcMany {
    __device__ static int budget(const Args&) {
        extern __shared__ __attribute__((aligned(16))) char oc_dyn_lds[];
        return __builtin_amdgcn_readfirstlane(*reinterpret_cast<const int*>(oc_dyn_lds + kOnchipBudgetOffset));
    }
    __device__ static StateLite state(const Args& a) {
        const CgState* p = s(a);
        auto ld = [](const double* q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
        StateLite L;
        L.alpha = ld(&p->alpha); L.rr = ld(&p->rr); L.rr_prev = ld(&p->rr_prev); L.rz = ld(&p->rz); L.r0norm = ld(&p->r0norm);
        L.it = oc_wg_load(&p->it); L.done = oc_wg_load(&p->done); L.first = oc_wg_load(&p->first); L.stop = oc_wg_load(&p->stop);
        return L;
    }
    __device__ static void finished(const Args&) {}
    // The thread index, opaque to the optimizer, taken anew by every pass of the step loop: what a pass derives from it (the nodes,
    // cells and offsets of its slots) would otherwise be computed once in front of the loop and kept in registers across all of it.
    __device__ static int tid() { int t = threadIdx.x; asm volatile("" : "+v"(t)); return t; }
};
// A scheme of implicit steps is what the step loop below does not know: Args, the kernel's second argument -- its fields pl, xk,
// yk, diag, sigma, g, g_stride, x, r, p, stride, partB, s, summary, norm0, done_count, book, step_it, nsteps, rp and m have one
// meaning in every scheme, and the loop reads none but these --; start(e, lds, t), the warm start of the member's next step from
// its state; kAdvances and advance(e, t), what a CONVERGED step does to a state the member keeps outside the workspace, before the
// book moves on.  OcTheta: the state is the workspace's x itself, nothing to advance.
template <class Args>
__device__ __forceinline__ OcStartOut oc_member_out(const Args& e) {     // member blockIdx.x's share of the workspace; it is not counted when a start says done
    const long long sys = blockIdx.x, base = sys * e.stride;
    return OcStartOut{e.x + base, e.r + base, e.p + base, e.partB + sys * FB_COUNT, e.s + sys, e.summary + sys, e.norm0 + sys, nullptr};
}
struct OcTheta {
    typedef OnchipStepsArgs Args;
    static constexpr bool kAdvances = false;
    __device__ static __forceinline__ void start_from(const Args& e, const OcLds& l, const double* x0, int t) {
        const long long sys = blockIdx.x;
        oc_start<true, false>(e.pl, l, e.rp, e.diag[sys], e.xk, e.yk, x0, oc_member_out(e), OcBStep{e.g + sys * e.g_stride, e.k, e.sigma[sys]}, t);
    }
    __device__ static __forceinline__ void start(const Args& e, const OcLds& l, int t) {
        start_from(e, l, e.x + blockIdx.x * e.stride, t);          // u: the x the chunk (or the start before it) left
    }
    __device__ static __forceinline__ void advance(const Args&, int) {}
};
// the first step's start, from the caller's states (the book is zeroed by the host)
__global__ __launch_bounds__(kOnchipMaxThreads) void k_onchip_steps_init(const OnchipStepsArgs e) {
    OcTheta::start_from(e, OcMany::lds(e.pl.cells), e.u0 + blockIdx.x * e.stride, threadIdx.x);
}
// The step loop, written once for every scheme.  (Both arguments by value and as a whole, as oc_chunk takes its own.)
template <int E, bool MSG, class Scheme>
__device__ __forceinline__ void oc_step_loop(const OnchipManyArgs a, const typename Scheme::Args e) {
    extern __shared__ __attribute__((aligned(16))) char oc_dyn_lds[];
    int* const budget_w = reinterpret_cast<int*>(oc_dyn_lds + kOnchipBudgetOffset);
    const int t = threadIdx.x;
    const long long sys = blockIdx.x;
    OcStepBook* const bk = e.book + sys;
    const CgState* const sp = e.s + sys;
    if (oc_wg_load(&bk->ended)) return;
    int step = oc_wg_load(&bk->step), budget = e.m;
    for (;;) {                                                     // every pass but the last costs a unit or more
        int done = oc_wg_load(&sp->done);
        if (!done) {
            if (budget < 1) break;
            const int it0 = oc_wg_load(&sp->it);
            if (t == 0) *budget_w = budget;
            __syncthreads();
            oc_chunk<E, MSG, OcSteps>(a);
            __syncthreads();                                       // the state the chunk left, for every thread
            budget -= oc_wg_load(&sp->it) - it0;
            done = oc_wg_load(&sp->done);
            if (!done) break;                                      // the budget ran out inside the step
        }
        // the step is over: the member's end, or the transition to its next step
        const int conv = oc_wg_load(&sp->converged);
        const bool last = !conv || step + 1 >= e.nsteps;
        if (!last && budget < 1) break;                            // the transition waits for the next launch
        if (t == 0) {
            if (e.step_it) e.step_it[sys * e.nsteps + step] = oc_wg_load(&sp->it);
            bk->step = step + (conv ? 1 : 0);
            if (last) { bk->ended = 1; atomicAdd(e.done_count, 1); }
        }
        if constexpr (Scheme::kAdvances) if (conv) { Scheme::advance(e, OcSteps::tid()); __syncthreads(); }
        if (last) break;
        budget -= 1; ++step;
        Scheme::start(e, OcMany::lds(e.pl.cells), OcSteps::tid());
        __syncthreads();                                           // thread 0's state, partials and norm
    }
}
template <int E, bool MSG>
__global__ __launch_bounds__(kOnchipMaxThreads) void k_onchip_steps(const OnchipManyArgs a, const OnchipStepsArgs e) {
    oc_step_loop<E, MSG, OcTheta>(a, e);
}

// ---- ensemble wave-equation steps: u_tt = A u - g ---------------------------------------------------------
// Explicit: velocity Verlet.  Member blockIdx.x takes `m` steps with its own tau inside ONE launch: u lives in the image (a thread
// reads its own cells back from it), v, the acceleration a = A u - g and g of its slots in registers.  A step is one stencil pass
// and two axpys between two barriers -- the first before the owned cells are overwritten (every neighbour has read them), the
// second after (every neighbour reads the new ones).  No reduction, no polling, nothing between workgroups.  a is carried from
// one step to the next; at the entry of a launch it is formed anew from (u, g): the same expression, hence the same bits, so k
// launches of one step give what one launch of k steps gives.  The expressions are onchip_plan.h's.
struct OnchipWaveArgs {
    OnchipPlan pl;
    OnchipWaveCoef k;
    const double* tau;                               // nsys
    const double* g; long long g_stride;             // forcing: member s reads g + s * g_stride (0: one vector for all)
    double* u; double* v;                            // nsys packed states of `stride` doubles each, in and out
    long long stride;
    int m;                                           // steps of this launch
};
template <int E>
__global__ __launch_bounds__(kOnchipMaxThreads) void k_onchip_wave_verlet(const OnchipWaveArgs a) {
    const OnchipPlan& pl = a.pl;
    double* const img = OcMany::lds(pl.cells).img;
    const int t = threadIdx.x, T = blockDim.x, pitch = pl.pitch;
    const long long sys = blockIdx.x;
    const double tau = a.tau[sys], h = 0.5 * tau;
    const double* const gin = a.g + sys * a.g_stride;
    double* const uio = a.u + sys * a.stride; double* const vio = a.v + sys * a.stride;

    for (int i = t; i < pl.cells; i += T) img[i] = 0.0;
    __syncthreads();                                               // the image is zero everywhere before the owners fill their cells
    unsigned cell2[(E + 1) / 2] = {};                              // image cells, two 16-bit indices per register (as oc_chunk)
    double v[E], acc[E], g[E];
    int cnt = 0;                                                   // valid slots: a prefix
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int i = onchip_owned(pl, t, k);
        if (i >= 0) {                                              // (slots beyond cnt are never read: nothing to initialise)
            int xx, yy;
            onchip_node(pl, i, &xx, &yy);
            const int c = onchip_cell(pl, xx, yy);
            cell2[k / 2] |= (unsigned)c << (16 * (k & 1));
            img[c] = uio[i]; v[k] = vio[i]; g[k] = gin[i];
            cnt = k + 1;
        }
    }
    __syncthreads();
    auto own_cell = [&](int k) { unsigned c2 = cell2[k / 2]; asm volatile("" : "+v"(c2)); return (int)((c2 >> (16 * (k & 1))) & 0xffffu); };
    auto accel_at = [&](int c, double gk) { return onchip_wave_accel(a.k, gk, img[c], img[c - 1], img[c + 1], img[c - pitch], img[c + pitch]); };
#pragma unroll
    for (int k = 0; k < E; ++k) if (k < cnt) { acc[k] = accel_at(own_cell(k), g[k]); __builtin_amdgcn_sched_barrier(0); }

    for (int s = 0; s < a.m; ++s) {
        __syncthreads();                                           // barrier 1: every neighbour has read the old cells
#pragma unroll
        for (int k = 0; k < E; ++k) if (k < cnt) {
            const int c = own_cell(k);
            v[k] = onchip_wave_kick(v[k], h, acc[k]);              // vh
            img[c] = onchip_wave_drift(img[c], tau, v[k]);
            __builtin_amdgcn_sched_barrier(0);                     // slot by slot: the loads of all slots at once would spill
        }
        __syncthreads();                                           // barrier 2: the new image is complete
#pragma unroll
        for (int k = 0; k < E; ++k) if (k < cnt) {
            acc[k] = accel_at(own_cell(k), g[k]);
            v[k] = onchip_wave_kick(v[k], h, acc[k]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int k = 0; k < E; ++k) if (k < cnt) {
        int i = k * T + t;
        asm volatile("" : "+v"(i));                                // recomputed here, not carried through the loop
        uio[i] = img[own_cell(k)]; vio[i] = v[k];
    }
}

// With a source time function and receivers (mi355cg_wave_record_many*): the forcing of the call's step n is
// w[n] g with the member's amplitude table w, and after every `every`-th step u at nrec nodes goes to the traces.  The step is
// k_onchip_wave_verlet's, still between two barriers, in a kernel of its own: that one stays the code it is (its body moved
// into a function both kernels share is optimized before it meets its launch bounds, and E = 16 comes out another kernel).
//   * The amplitudes reach a step through LDS.  Two blocks of 64 doubles at the head of the side data (the kernel uses the image
//     alone): lane t of wave 0 holds w at the end of the launch's step 64 b + t in block b % 2.  Block 0 is written before the
//     loop; the load of block b + 1 is issued in step 64 b into a register and stored in step 64 b + 32, both behind barrier 2.
//     So the global latency has 32 steps to pass, the block that is overwritten was last read in step 64 b - 1, and the first
//     step that reads the new one lies 32 steps and their barriers ahead.
//   * Thread r < nrec keeps the image cell of receiver r.  Behind barrier 2 the new image is complete and no owner writes before
//     the next barrier 1: in that window it reads its cell and stores it, an ordinary vector store nobody waits for.
// step0, the steps of the call before this launch, places the launch in the table; phase and slot are step0 % every and
// step0 / every, so that the cadence and the sample a step writes do not depend on how the host cuts the call into launches.
// The acceleration at the entry of a launch is formed from (u, g, w[step0]): the expression that left it at the end of step0.
struct OnchipWaveRecArgs {
    const double* w; long long w_stride;             // amplitudes: member s reads w + s * w_stride (0: one row for all), nsteps + 1 each
    int step0;
    const int* rec_cell; int nrec;                   // image cells of the receivers, nrec <= kOnchipWaveMaxRec
    int every, phase, slot;
    double* traces; long long tr_stride;             // member s writes traces + s * tr_stride: its samples, nrec doubles each
};
constexpr int kOcAmpBlock = 64;                      // amplitudes per block: one per lane of wave 0
static_assert(2 * kOcAmpBlock * 8 <= kOnchipSideBytes && kOcAmpBlock <= kWave && kOnchipWaveMaxRec <= kWave, "the amplitude blocks fit in the side data; wave 0 fills them and holds the receivers");
template <int E>
__global__ __launch_bounds__(kOnchipMaxThreads) void k_oc_wave_record(const OnchipWaveArgs a, const OnchipWaveRecArgs x) {
    const OnchipPlan& pl = a.pl;
    extern __shared__ __attribute__((aligned(16))) char oc_dyn_lds[];
    double* const wbuf = reinterpret_cast<double*>(oc_dyn_lds);
    double* const img = OcMany::lds(pl.cells).img;
    const int t = threadIdx.x, T = blockDim.x, pitch = pl.pitch;
    const long long sys = blockIdx.x;
    const double tau = a.tau[sys], h = 0.5 * tau;
    const double* const gin = a.g + sys * a.g_stride;
    double* const uio = a.u + sys * a.stride; double* const vio = a.v + sys * a.stride;
    const double* const wrow = x.w + sys * x.w_stride + x.step0;   // wrow[s]: at the start of the launch's step s, wrow[s + 1]: at its end
    double* trow = x.traces + sys * x.tr_stride + (long long)x.slot * x.nrec;

    for (int i = t; i < pl.cells; i += T) img[i] = 0.0;
    __syncthreads();                                               // the image is zero everywhere before the owners fill their cells
    unsigned cell2[(E + 1) / 2] = {};
    double v[E], acc[E], g[E];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int i = onchip_owned(pl, t, k);
        if (i >= 0) {                                              // (slots beyond cnt are never read: nothing to initialise)
            int xx, yy;
            onchip_node(pl, i, &xx, &yy);
            const int c = onchip_cell(pl, xx, yy);
            cell2[k / 2] |= (unsigned)c << (16 * (k & 1));
            img[c] = uio[i]; v[k] = vio[i]; g[k] = gin[i];
            cnt = k + 1;
        }
    }
    if (t < kOcAmpBlock && t < a.m) wbuf[t] = wrow[t + 1];
    int rcell = 0, phase = x.phase;
    if (t < x.nrec) rcell = x.rec_cell[t];
    double w_now = wrow[0], w_next = 0.0;
    __syncthreads();
    auto own_cell = [&](int k) { unsigned c2 = cell2[k / 2]; asm volatile("" : "+v"(c2)); return (int)((c2 >> (16 * (k & 1))) & 0xffffu); };
    auto accel_at = [&](int c, double f) { return onchip_wave_accel(a.k, f, img[c], img[c - 1], img[c + 1], img[c - pitch], img[c + pitch]); };
#pragma unroll
    for (int k = 0; k < E; ++k) if (k < cnt) { acc[k] = accel_at(own_cell(k), onchip_wave_forcing(w_now, g[k])); __builtin_amdgcn_sched_barrier(0); }

    for (int s = 0; s < a.m; ++s) {
        __syncthreads();                                           // barrier 1: every neighbour has read the old cells
        w_now = wbuf[((s / kOcAmpBlock) & 1) * kOcAmpBlock + s % kOcAmpBlock];        // the amplitude at the END of this step
#pragma unroll
        for (int k = 0; k < E; ++k) if (k < cnt) {
            const int c = own_cell(k);
            v[k] = onchip_wave_kick(v[k], h, acc[k]);              // vh
            img[c] = onchip_wave_drift(img[c], tau, v[k]);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();                                           // barrier 2: the new image is complete
#pragma unroll
        for (int k = 0; k < E; ++k) if (k < cnt) {
            acc[k] = accel_at(own_cell(k), onchip_wave_forcing(w_now, g[k]));
            v[k] = onchip_wave_kick(v[k], h, acc[k]);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (++phase == x.every) {                                  // uniform: this step is sampled
            phase = 0;
            if (t < x.nrec) trow[t] = img[rcell];
            trow += x.nrec;
        }
        const int q = s % kOcAmpBlock, nb = s - q + kOcAmpBlock + t;                  // this lane's step in the next block
        if (t < kOcAmpBlock && nb < a.m) {
            if (q == 0) w_next = wrow[nb + 1];
            if (q == kOcAmpBlock / 2) wbuf[((nb / kOcAmpBlock) & 1) * kOcAmpBlock + t] = w_next;
        }
    }
#pragma unroll
    for (int k = 0; k < E; ++k) if (k < cnt) {
        int i = k * T + t;
        asm volatile("" : "+v"(i));                                // recomputed here, not carried through the loop
        uio[i] = img[own_cell(k)]; vio[i] = v[k];
    }
}

// In a medium (mi355cg_wave_medium_many*): u_tt = c2 o (A u) - w(t) g, the squared wave speed c2 of every
// unknown given per member or once for all.  k_oc_wave_record's step with onchip_wave_medium_accel in both places, c2 of the
// thread's slots in registers beside g (the LDS cannot hold a medium beside the image at the cap), loaded once.  The barriers, the
// amplitude blocks, the receiver window and step0 / phase / slot are that kernel's; it is a kernel of its own for that kernel's
// reason, so the other two stay the code they are.
struct OnchipWaveMediumArgs { const double* c2; long long c2_stride; };      // member s reads c2 + s * c2_stride (0: one vector for all)
template <int E>
__global__ __launch_bounds__(kOnchipMaxThreads) void k_oc_wave_medium(const OnchipWaveArgs a, const OnchipWaveRecArgs x, const OnchipWaveMediumArgs md) {
    const OnchipPlan& pl = a.pl;
    extern __shared__ __attribute__((aligned(16))) char oc_dyn_lds[];
    double* const wbuf = reinterpret_cast<double*>(oc_dyn_lds);
    double* const img = OcMany::lds(pl.cells).img;
    const int t = threadIdx.x, T = blockDim.x, pitch = pl.pitch;
    const long long sys = blockIdx.x;
    const double tau = a.tau[sys], h = 0.5 * tau;
    const double* const gin = a.g + sys * a.g_stride;
    const double* const cin = md.c2 + sys * md.c2_stride;
    double* const uio = a.u + sys * a.stride; double* const vio = a.v + sys * a.stride;
    const double* const wrow = x.w + sys * x.w_stride + x.step0;   // wrow[s]: at the start of the launch's step s, wrow[s + 1]: at its end
    double* trow = x.traces + sys * x.tr_stride + (long long)x.slot * x.nrec;

    for (int i = t; i < pl.cells; i += T) img[i] = 0.0;
    __syncthreads();                                               // the image is zero everywhere before the owners fill their cells
    unsigned cell2[(E + 1) / 2] = {};
    double v[E], acc[E], g[E], c2[E];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int i = onchip_owned(pl, t, k);
        if (i >= 0) {                                              // (slots beyond cnt are never read: nothing to initialise)
            int xx, yy;
            onchip_node(pl, i, &xx, &yy);
            const int c = onchip_cell(pl, xx, yy);
            cell2[k / 2] |= (unsigned)c << (16 * (k & 1));
            img[c] = uio[i]; v[k] = vio[i]; g[k] = gin[i]; c2[k] = cin[i];
            cnt = k + 1;
        }
    }
    if (t < kOcAmpBlock && t < a.m) wbuf[t] = wrow[t + 1];
    int rcell = 0, phase = x.phase;
    if (t < x.nrec) rcell = x.rec_cell[t];
    double w_now = wrow[0], w_next = 0.0;
    __syncthreads();
    auto own_cell = [&](int k) { unsigned cc = cell2[k / 2]; asm volatile("" : "+v"(cc)); return (int)((cc >> (16 * (k & 1))) & 0xffffu); };
    auto accel_at = [&](int c, double ck, double f) { return onchip_wave_medium_accel(a.k, ck, f, img[c], img[c - 1], img[c + 1], img[c - pitch], img[c + pitch]); };
#pragma unroll
    for (int k = 0; k < E; ++k) if (k < cnt) { acc[k] = accel_at(own_cell(k), c2[k], onchip_wave_forcing(w_now, g[k])); __builtin_amdgcn_sched_barrier(0); }

    for (int s = 0; s < a.m; ++s) {
        __syncthreads();                                           // barrier 1: every neighbour has read the old cells
        w_now = wbuf[((s / kOcAmpBlock) & 1) * kOcAmpBlock + s % kOcAmpBlock];        // the amplitude at the END of this step
#pragma unroll
        for (int k = 0; k < E; ++k) if (k < cnt) {
            const int c = own_cell(k);
            v[k] = onchip_wave_kick(v[k], h, acc[k]);              // vh
            img[c] = onchip_wave_drift(img[c], tau, v[k]);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();                                           // barrier 2: the new image is complete
#pragma unroll
        for (int k = 0; k < E; ++k) if (k < cnt) {
            acc[k] = accel_at(own_cell(k), c2[k], onchip_wave_forcing(w_now, g[k]));
            v[k] = onchip_wave_kick(v[k], h, acc[k]);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (++phase == x.every) {                                  // uniform: this step is sampled
            phase = 0;
            if (t < x.nrec) trow[t] = img[rcell];
            trow += x.nrec;
        }
        const int q = s % kOcAmpBlock, nb = s - q + kOcAmpBlock + t;                  // this lane's step in the next block
        if (t < kOcAmpBlock && nb < a.m) {
            if (q == 0) w_next = wrow[nb + 1];
            if (q == kOcAmpBlock / 2) wbuf[((nb / kOcAmpBlock) & 1) * kOcAmpBlock + t] = w_next;
        }
    }
#pragma unroll
    for (int k = 0; k < E; ++k) if (k < cnt) {
        int i = k * T + t;
        asm volatile("" : "+v"(i));                                // recomputed here, not carried through the loop
        uio[i] = img[own_cell(k)]; vio[i] = v[k];
    }
}

// With a damping field (mi355cg_wave_sponge_many*): u_tt + d o u_t = c2 o (A u) - w(t) g, v scaled by
// onchip_wave_sponge_factor at both ends of every step.  A fifth per-slot array does not fit beside v, acc, g and c2 at E = 24,
// so this is k_oc_wave_medium with the loop rotated: acc lives only from the second half kick of a step to the first of the
// next, with nothing but barrier 1 and the back edge between, so both kicks are made in one pass behind barrier 2, the
// acceleration is a temporary, and its registers hold the factors.  At entry: the opening damp and the first half kick.  In the
// loop: barrier 1, the drift, barrier 2, then a, the second kick, the closing damp and -- unless this is the launch's last step
// -- the next step's opening damp and first kick with the same a (damping does not touch u).  The last step of a launch ends
// behind its closing damp, so launches and chained calls stay invisible: the next launch forms the same a from (u, g, c2,
// w[step0]).  The host never launches m = 0 steps.  Everything else is k_oc_wave_medium's; a kernel of its own for its reason.
struct OnchipWaveSpongeArgs { const double* d; long long d_stride; };        // member s reads d + s * d_stride (0: one vector for all)
template <int E>
__global__ __launch_bounds__(kOnchipMaxThreads) void k_oc_wave_sponge(const OnchipWaveArgs a, const OnchipWaveRecArgs x, const OnchipWaveMediumArgs md,
                                                                      const OnchipWaveSpongeArgs sp) {
    const OnchipPlan& pl = a.pl;
    extern __shared__ __attribute__((aligned(16))) char oc_dyn_lds[];
    double* const wbuf = reinterpret_cast<double*>(oc_dyn_lds);
    double* const img = OcMany::lds(pl.cells).img;
    const int t = threadIdx.x, T = blockDim.x, pitch = pl.pitch;
    const long long sys = blockIdx.x;
    const double tau = a.tau[sys], h = 0.5 * tau;
    const double* const gin = a.g + sys * a.g_stride;
    const double* const cin = md.c2 + sys * md.c2_stride;
    const double* const din = sp.d + sys * sp.d_stride;
    double* const uio = a.u + sys * a.stride; double* const vio = a.v + sys * a.stride;
    const double* const wrow = x.w + sys * x.w_stride + x.step0;   // wrow[s]: at the start of the launch's step s, wrow[s + 1]: at its end
    double* trow = x.traces + sys * x.tr_stride + (long long)x.slot * x.nrec;

    for (int i = t; i < pl.cells; i += T) img[i] = 0.0;
    __syncthreads();                                               // the image is zero everywhere before the owners fill their cells
    unsigned cell2[(E + 1) / 2] = {};
    double v[E], g[E], c2[E], sf[E];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int i = onchip_owned(pl, t, k);
        if (i >= 0) {                                              // (slots beyond cnt are never read: nothing to initialise)
            int xx, yy;
            onchip_node(pl, i, &xx, &yy);
            const int c = onchip_cell(pl, xx, yy);
            cell2[k / 2] |= (unsigned)c << (16 * (k & 1));
            img[c] = uio[i]; v[k] = vio[i]; g[k] = gin[i]; c2[k] = cin[i]; sf[k] = onchip_wave_sponge_factor(tau, din[i]);
            cnt = k + 1;
        }
    }
    if (t < kOcAmpBlock && t < a.m) wbuf[t] = wrow[t + 1];
    int rcell = 0, phase = x.phase;
    if (t < x.nrec) rcell = x.rec_cell[t];
    double w_now = wrow[0], w_next = 0.0;
    __syncthreads();
    auto own_cell = [&](int k) { unsigned cc = cell2[k / 2]; asm volatile("" : "+v"(cc)); return (int)((cc >> (16 * (k & 1))) & 0xffffu); };
    auto accel_at = [&](int c, double ck, double f) { return onchip_wave_medium_accel(a.k, ck, f, img[c], img[c - 1], img[c + 1], img[c - pitch], img[c + pitch]); };
#pragma unroll
    for (int k = 0; k < E; ++k) if (k < cnt) {
        const double acc = accel_at(own_cell(k), c2[k], onchip_wave_forcing(w_now, g[k]));
        v[k] = onchip_wave_kick(onchip_wave_damp(sf[k], v[k]), h, acc);        // the opening damp, then vh
        __builtin_amdgcn_sched_barrier(0);
    }

    for (int s = 0; s < a.m; ++s) {
        __syncthreads();                                           // barrier 1: every neighbour has read the old cells
        w_now = wbuf[((s / kOcAmpBlock) & 1) * kOcAmpBlock + s % kOcAmpBlock];        // the amplitude at the END of this step
#pragma unroll
        for (int k = 0; k < E; ++k) if (k < cnt) {
            const int c = own_cell(k);
            img[c] = onchip_wave_drift(img[c], tau, v[k]);         // v holds vh
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();                                           // barrier 2: the new image is complete
        const bool more = s + 1 < a.m;                             // uniform: the next step is this launch's too
#pragma unroll
        for (int k = 0; k < E; ++k) if (k < cnt) {
            const double acc = accel_at(own_cell(k), c2[k], onchip_wave_forcing(w_now, g[k]));
            v[k] = onchip_wave_damp(sf[k], onchip_wave_kick(v[k], h, acc));    // the second kick, the closing damp
            if (more) v[k] = onchip_wave_kick(onchip_wave_damp(sf[k], v[k]), h, acc);  // the next step's opening damp and vh
            __builtin_amdgcn_sched_barrier(0);
        }
        if (++phase == x.every) {                                  // uniform: this step is sampled
            phase = 0;
            if (t < x.nrec) trow[t] = img[rcell];
            trow += x.nrec;
        }
        const int q = s % kOcAmpBlock, nb = s - q + kOcAmpBlock + t;                  // this lane's step in the next block
        if (t < kOcAmpBlock && nb < a.m) {
            if (q == 0) w_next = wrow[nb + 1];
            if (q == kOcAmpBlock / 2) wbuf[((nb / kOcAmpBlock) & 1) * kOcAmpBlock + t] = w_next;
        }
    }
#pragma unroll
    for (int k = 0; k < E; ++k) if (k < cnt) {
        int i = k * T + t;
        asm volatile("" : "+v"(i));                                // recomputed here, not carried through the loop
        uio[i] = img[own_cell(k)]; vio[i] = v[k];
    }
}

// The forward run that keeps its history (mi355cg_wave_history_many*): k_oc_wave_medium's step and bits,
// and the stencil value t = au(u) of every owned slot stored as it is formed, before it is scaled: row step0 + n of the member's
// history is au(u) at the launch's state n, unknown i = k T + t of it at [(step0 + n) size + i], so neighbouring lanes write
// neighbouring doubles -- ordinary vector stores nobody waits for.  Row step0 is written at entry (a later launch rewrites the
// bits the launch before it left there).  The loop is the rotated one of k_oc_wave_sponge, both half kicks from one a behind
// barrier 2 (the same bits: the carried acceleration IS that a), so v, g and c2 are the per-slot arrays and the store has
// registers to spare.  The host never launches m = 0 steps.  A kernel of its own for k_oc_wave_record's reason.
struct OnchipWaveHistArgs { double* hist; long long hist_stride; };          // member s writes hist + s * hist_stride, rows of a.stride doubles
template <int E>
__global__ __launch_bounds__(kOnchipMaxThreads) void k_oc_wave_history(const OnchipWaveArgs a, const OnchipWaveRecArgs x, const OnchipWaveMediumArgs md,
                                                                       const OnchipWaveHistArgs hs) {
    const OnchipPlan& pl = a.pl;
    extern __shared__ __attribute__((aligned(16))) char oc_dyn_lds[];
    double* const wbuf = reinterpret_cast<double*>(oc_dyn_lds);
    double* const img = OcMany::lds(pl.cells).img;
    const int t = threadIdx.x, T = blockDim.x, pitch = pl.pitch;
    const long long sys = blockIdx.x;
    const double tau = a.tau[sys], h = 0.5 * tau;
    const double* const gin = a.g + sys * a.g_stride;
    const double* const cin = md.c2 + sys * md.c2_stride;
    double* const uio = a.u + sys * a.stride; double* const vio = a.v + sys * a.stride;
    const double* const wrow = x.w + sys * x.w_stride + x.step0;   // wrow[s]: at the start of the launch's step s, wrow[s + 1]: at its end
    double* trow = x.traces + sys * x.tr_stride + (long long)x.slot * x.nrec;
    double* hrow = hs.hist + sys * hs.hist_stride + (long long)x.step0 * a.stride + t;     // this lane's column of the row being written

    for (int i = t; i < pl.cells; i += T) img[i] = 0.0;
    __syncthreads();                                               // the image is zero everywhere before the owners fill their cells
    unsigned cell2[(E + 1) / 2] = {};
    double v[E], g[E], c2[E];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int i = onchip_owned(pl, t, k);
        if (i >= 0) {                                              // (slots beyond cnt are never read: nothing to initialise)
            int xx, yy;
            onchip_node(pl, i, &xx, &yy);
            const int c = onchip_cell(pl, xx, yy);
            cell2[k / 2] |= (unsigned)c << (16 * (k & 1));
            img[c] = uio[i]; v[k] = vio[i]; g[k] = gin[i]; c2[k] = cin[i];
            cnt = k + 1;
        }
    }
    if (t < kOcAmpBlock && t < a.m) wbuf[t] = wrow[t + 1];
    int rcell = 0, phase = x.phase;
    if (t < x.nrec) rcell = x.rec_cell[t];
    double w_now = wrow[0], w_next = 0.0;
    __syncthreads();
    auto own_cell = [&](int k) { unsigned cc = cell2[k / 2]; asm volatile("" : "+v"(cc)); return (int)((cc >> (16 * (k & 1))) & 0xffffu); };
    auto stencil_at = [&](int c) { return onchip_wave_au(a.k, img[c], img[c - 1], img[c + 1], img[c - pitch], img[c + pitch]); };
#pragma unroll
    for (int k = 0; k < E; ++k) if (k < cnt) {
        const double au = stencil_at(own_cell(k));
        hrow[k * T] = au;                                          // row step0
        v[k] = onchip_wave_kick(v[k], h, onchip_wave_medium_accel_of(c2[k], au, onchip_wave_forcing(w_now, g[k])));       // vh
        __builtin_amdgcn_sched_barrier(0);
    }

    for (int s = 0; s < a.m; ++s) {
        __syncthreads();                                           // barrier 1: every neighbour has read the old cells
        w_now = wbuf[((s / kOcAmpBlock) & 1) * kOcAmpBlock + s % kOcAmpBlock];        // the amplitude at the END of this step
        hrow += a.stride;
#pragma unroll
        for (int k = 0; k < E; ++k) if (k < cnt) {
            const int c = own_cell(k);
            img[c] = onchip_wave_drift(img[c], tau, v[k]);         // v holds vh
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();                                           // barrier 2: the new image is complete
        const bool more = s + 1 < a.m;                             // uniform: the next step is this launch's too
#pragma unroll
        for (int k = 0; k < E; ++k) if (k < cnt) {
            const double au = stencil_at(own_cell(k));
            hrow[k * T] = au;                                      // row step0 + s + 1
            const double acc = onchip_wave_medium_accel_of(c2[k], au, onchip_wave_forcing(w_now, g[k]));
            v[k] = onchip_wave_kick(v[k], h, acc);                 // the second kick
            if (more) v[k] = onchip_wave_kick(v[k], h, acc);       // the next step's vh
            __builtin_amdgcn_sched_barrier(0);
        }
        if (++phase == x.every) {                                  // uniform: this step is sampled
            phase = 0;
            if (t < x.nrec) trow[t] = img[rcell];
            trow += x.nrec;
        }
        const int q = s % kOcAmpBlock, nb = s - q + kOcAmpBlock + t;                  // this lane's step in the next block
        if (t < kOcAmpBlock && nb < a.m) {
            if (q == 0) w_next = wrow[nb + 1];
            if (q == kOcAmpBlock / 2) wbuf[((nb / kOcAmpBlock) & 1) * kOcAmpBlock + t] = w_next;
        }
    }
#pragma unroll
    for (int k = 0; k < E; ++k) if (k < cnt) {
        int i = k * T + t;
        asm volatile("" : "+v"(i));                                // recomputed here, not carried through the loop
        uio[i] = img[own_cell(k)]; vio[i] = v[k];
    }
}

// The adjoint of that run (mi355cg_wave_adjoint_many*): onchip_plan.h's recurrence from the launch's state
// index s_top down through m steps.  The forward step with the roles swapped: q is the image, lam a register array where the
// forward kernels keep v, and the loop is the rotated one -- au(q) behind the drift of step s is the au(q) the first kick of step
// s - 1 needs, so one stencil pass behind barrier 2 makes both kicks, with only the injection of step s - 1 between them.  The
// per-slot arrays are lam, c2, S and the history row of the NEXT state index, loaded one step before it is used; rows below the
// launch's last state or above s_top are never read.  The last step of a launch ends behind its second kick: the next launch
// forms the same au(q) from the same q, so launches and chained calls are invisible.
//   * Adjoint sources: only a sampled step (s % every == 0, uniform) has a row.  Lane j < nrec of wave 0 loads its entry of the
//     next sampled step's row into a register when the row before it is consumed (`every` steps ahead), stores it to the head of
//     the side data between the barriers of the step above the sampled one, and the injection reads it behind barrier 2.
//   * Injection: a thread finds at load time which of its slots are receivers (a bit per slot) from the table of the receivers'
//     packed indices in the side data; on a sampled step only threads with a bit set walk the receivers, ascending, so
//     duplicates add in that order.
struct OnchipWaveAdjArgs {
    OnchipPlan pl;
    OnchipWaveCoef k;
    const double* tau;                               // nsys
    const double* c2; long long c2_stride;           // member s reads c2 + s * c2_stride (0: one medium for all)
    const double* hist; long long hist_stride;       // member s reads hist + s * hist_stride: rows of `stride` doubles, row n = au(u_n)
    const double* adj; long long adj_stride;         // member s reads adj + s * adj_stride (0: one table for all): row j for step (j + 1) every
    const int* rec_node; int nrec;                   // packed indices of the receivers, nrec <= kOnchipWaveMaxRec
    int every;
    int s_top;                                       // the state index the launch starts from: the call's nsteps - steps done before
    double* lam; double* q; double* S;               // nsys packed vectors of `stride` doubles each, in and out
    long long stride;
    int m;                                           // steps of this launch, 1 <= m <= s_top
};
static_assert(kOnchipWaveMaxRec * (8 + 4) <= kOnchipSideBytes, "a row of adjoint sources and the receiver table fit in the side data");
template <int E>
__global__ __launch_bounds__(kOnchipMaxThreads) void k_oc_wave_adjoint(const OnchipWaveAdjArgs a) {
    const OnchipPlan& pl = a.pl;
    extern __shared__ __attribute__((aligned(16))) char oc_dyn_lds[];
    double* const rbuf = reinterpret_cast<double*>(oc_dyn_lds);                                    // the row of the sampled step
    int* const rnode = reinterpret_cast<int*>(oc_dyn_lds + kOnchipWaveMaxRec * sizeof(double));    // the receivers
    double* const img = OcMany::lds(pl.cells).img;
    const int t = threadIdx.x, T = blockDim.x, pitch = pl.pitch, nrec = a.nrec, every = a.every;
    const long long sys = blockIdx.x;
    const double tau = a.tau[sys], h = 0.5 * tau;
    const double* const cin = a.c2 + sys * a.c2_stride;
    const double* const hcol = a.hist + sys * a.hist_stride + t;   // this lane's column of the history
    double* const lio = a.lam + sys * a.stride; double* const qio = a.q + sys * a.stride; double* const sio = a.S + sys * a.stride;
    int s = a.s_top, ph = s % every;                               // ph == 0: state index s is sampled
    const int lo = s - a.m;                                        // the launch's last state: its steps are s_top .. lo + 1
    // the row of the next sampled step at or below s (never dereferenced when that step is not this launch's)
    const double* arow = a.adj + sys * a.adj_stride + ((long long)((s - ph) / every) - 1) * nrec;
    const bool holder = t < nrec;

    for (int i = t; i < pl.cells; i += T) img[i] = 0.0;
    if (holder) rnode[t] = a.rec_node[t];
    double r_next = 0.0;
    if (ph == 0) {                                                 // uniform: the launch's first step is sampled (s >= 1 > lo)
        if (holder) rbuf[t] = arow[t];
        arow -= nrec;
        if (holder && s - every > lo) r_next = arow[t];
    } else if (holder && s - ph > lo) r_next = arow[t];
    __syncthreads();                                               // the image is zero, the table and the first row are there
    unsigned cell2[(E + 1) / 2] = {};
    double lam[E], c2[E], S[E], hn[E];
    int cnt = 0;
    unsigned mask = 0;
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int i = onchip_owned(pl, t, k);
        if (i >= 0) {                                              // (slots beyond cnt are never read: nothing to initialise)
            int xx, yy;
            onchip_node(pl, i, &xx, &yy);
            const int c = onchip_cell(pl, xx, yy);
            cell2[k / 2] |= (unsigned)c << (16 * (k & 1));
            img[c] = qio[i]; lam[k] = lio[i]; c2[k] = cin[i]; S[k] = sio[i];
            cnt = k + 1;
        }
    }
    const unsigned last = (unsigned)pl.unknowns - 1u;
    const int ucnt = (pl.unknowns + T - 1) / T;                    // uniform: the slots that any thread owns
    const int shift = __builtin_ctz((unsigned)T);                  // T is a power of two: unknown i sits in slot i / T of thread i % T
    for (int j = 0; j < nrec; ++j) {
        const int node = rnode[j];
        if ((node & (T - 1)) == t) mask |= 1u << (node >> shift);
    }
    __syncthreads();
    auto own_cell = [&](int k) { unsigned cc = cell2[k / 2]; asm volatile("" : "+v"(cc)); return (int)((cc >> (16 * (k & 1))) & 0xffffu); };
    auto stencil_at = [&](int c) { return onchip_wave_au(a.k, img[c], img[c - 1], img[c + 1], img[c - pitch], img[c + pitch]); };
    auto inject = [&](int k, double l) {                           // the sampled step's sources at unknown k T + t, ascending
        const int i = k * T + t;
        for (int j = 0; j < nrec; ++j) if (rnode[j] == i) l = onchip_wave_adjoint_inject(l, rbuf[j]);
        return l;
    };
#pragma unroll
    for (int k = 0; k < E; ++k) if (k < cnt) {                     // the first half of step s_top
        const int c = own_cell(k);
        const double qv = img[c], aq = stencil_at(c);
        if (ph == 0 && ((mask >> k) & 1u)) lam[k] = inject(k, lam[k]);
        S[k] = onchip_wave_adjoint_sens(S[k], qv, hcol[(long long)s * a.stride + k * T]);
        lam[k] = onchip_wave_adjoint_kick(lam[k], h, aq);
        hn[k] = hcol[(long long)(s - 1) * a.stride + k * T];       // s - 1 >= lo >= 0
        __builtin_amdgcn_sched_barrier(0);
    }

    for (; s > lo; --s) {
        __syncthreads();                                           // barrier 1: every neighbour has read the old cells, the row is consumed
        const bool more = s - 1 > lo;                              // uniform: step s - 1 is this launch's too
        ph = ph == 0 ? every - 1 : ph - 1;                         // of state index s - 1
        const bool sampled = more && ph == 0;                      // uniform: step s - 1 injects
        if (sampled) {
            if (holder) rbuf[t] = r_next;
            arow -= nrec;
            if (holder && s - 1 - every > lo) r_next = arow[t];
        }
#pragma unroll
        for (int k = 0; k < E; ++k) if (k < cnt) {
            const int c = own_cell(k);
            img[c] = onchip_wave_adjoint_drift(img[c], tau, c2[k], lam[k]);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();                                           // barrier 2: the new image is complete
        // the prefetched row has landed in EVERY slot before the pass, on every lane's path: the pass reads a slot only under the
        // lane's own guard, and without this the compiler must assume a load still in flight when the row's registers are next
        // written, and waits before each of them
#pragma unroll
        for (int k = 0; k < E; ++k) asm volatile("" :: "v"(hn[k]));
#pragma unroll
        for (int k = 0; k < E; ++k) if (k < cnt) {
            const int c = own_cell(k);
            const double qv = img[c], aq = stencil_at(c);
            S[k] = onchip_wave_adjoint_sens(S[k], qv, hn[k]);      // H[s - 1]
            lam[k] = onchip_wave_adjoint_kick(lam[k], h, aq);
            if (more) {                                            // the first half of step s - 1, with the same au(q)
                if (sampled && ((mask >> k) & 1u)) lam[k] = inject(k, lam[k]);
                S[k] = onchip_wave_adjoint_sens(S[k], qv, hn[k]);
                lam[k] = onchip_wave_adjoint_kick(lam[k], h, aq);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // H[s - 2], for the next step: the loads of all slots go out back to back behind the pass.  No lane-dependent branch
        // guards them, not even a uniform one -- a lane reads the row's last unknown for a slot it does not own (one cache line
        // for all such lanes, a value that is never used) -- and the address is the uniform row plus a 32-bit lane index: inside the pass, or
        // behind a per-lane guard, the compiler waits for every load before it issues the next (24 dependent round trips a
        // step at the cap).
        if (more) {
            const double* const hrow = a.hist + sys * a.hist_stride + (long long)(s - 2) * a.stride;
            unsigned idx = (unsigned)t;                            // one index register walks the slots
#pragma unroll
            for (int k = 0; k < E; ++k) if (k < ucnt) {
                hn[k] = hrow[min(idx, last)];
                idx += (unsigned)T;
                __builtin_amdgcn_sched_barrier(0);                 // slot by slot: 24 indices formed ahead would spill
            }
        }
    }
#pragma unroll
    for (int k = 0; k < E; ++k) if (k < cnt) {
        int i = k * T + t;
        asm volatile("" : "+v"(i));                                // recomputed here, not carried through the loop
        qio[i] = img[own_cell(k)]; lio[i] = lam[k]; sio[i] = S[k];
    }
}

// The check launch for media in device memory: workgroup b reduces row b of the media (`rows` of them, `len` doubles each, row b
// at c2 + b * stride) to its least and its largest entry and writes them to out[2 b], out[2 b + 1]; a row with an entry that is
// not finite gets NaN in both.  The host reads them back once and refuses there, so that the message can name the member.
constexpr int kOcRangeThreads = 256;
__global__ __launch_bounds__(kOcRangeThreads) void k_oc_medium_range(const double* c2, long long stride, int len, double* out) {
    __shared__ double part[3][kOcRangeThreads / kWave];
    const double* const row = c2 + (long long)blockIdx.x * stride;
    const int t = threadIdx.x;
    double lo = INFINITY, hi = -INFINITY, bad = 0.0;
    for (int i = t; i < len; i += kOcRangeThreads) {
        const double x = row[i];
        if (!(fabs(x) <= 1.7976931348623157e308)) bad = 1.0;       // NaN or an infinity
        lo = fmin(lo, x); hi = fmax(hi, x);
    }
    for (int d = kWave / 2; d > 0; d >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, d)); hi = fmax(hi, __shfl_xor(hi, d)); bad = fmax(bad, __shfl_xor(bad, d));
    }
    if (t % kWave == 0) { part[0][t / kWave] = lo; part[1][t / kWave] = hi; part[2][t / kWave] = bad; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kOcRangeThreads / kWave; ++w) { lo = fmin(lo, part[0][w]); hi = fmax(hi, part[1][w]); bad = fmax(bad, part[2][w]); }
        const double nan = __builtin_nan("");
        out[2 * (long long)blockIdx.x] = bad != 0.0 ? nan : lo;
        out[2 * (long long)blockIdx.x + 1] = bad != 0.0 ? nan : hi;
    }
}

// Implicit: average-acceleration Newmark.  oc_step_loop with another right-hand side and a velocity: a step is the warm-started
// solve of (A - sigma_s I) x = b_wave(u, v), sigma_s = 4 / tau_s^2, and the transition after a CONVERGED step updates the member's
// state in the caller's vectors -- v = hv (x - u) - v, u = x, with u the state the step started from -- before the next step
// starts from it.  After a step that did not converge (u, v) stay: the state after the last converged step.  Budget of units,
// system type, book and report are the loop's.
struct OcBWave {
    const double* g; const double* v; OnchipWaveCoef k; double sigma, tau;
    __device__ double at(int i, int c, const double* img, int pitch) const {
        return onchip_newmark_rhs(k, sigma, tau, g[i], v[i], img[c], img[c - 1], img[c + 1], img[c - pitch], img[c + pitch]);
    }
};
struct OnchipNewmarkArgs {
    OnchipPlan pl;
    double xk, yk;
    const double* diag; const double* sigma;         // nsys each: A_diag - sigma_s as mi355cg_set_shift rounds it; sigma_s
    const double* tau;                               // nsys tau_s, then nsys 2 / tau_s
    const double* g; long long g_stride;
    double* u; double* v;                            // nsys packed states, in and out: the state after the last converged step
    double* x; double* r; double* p;
    long long stride;
    double* partB; CgState* s; CgState* summary; double* norm0; int* done_count;
    OcStepBook* book;
    int* step_it; int nsteps, nsys;
    OnchipWaveCoef k;
    RuleParams rp;
    int m;
};
// OcNewmark: the scheme of oc_step_loop.  The state moves on after a converged step: v first, it reads the u the step started from.
struct OcNewmark {
    typedef OnchipNewmarkArgs Args;
    static constexpr bool kAdvances = true;
    __device__ static __forceinline__ void start(const Args& e, const OcLds& l, int t) {
        const long long sys = blockIdx.x, base = sys * e.stride;
        oc_start<true, false>(e.pl, l, e.rp, e.diag[sys], e.xk, e.yk, e.u + base, oc_member_out(e),
                              OcBWave{e.g + sys * e.g_stride, e.v + base, e.k, e.sigma[sys], e.tau[sys]}, t);
    }
    __device__ static __forceinline__ void advance(const Args& e, int t) {
        const long long base = (long long)blockIdx.x * e.stride;
        const double hv = e.tau[e.nsys + blockIdx.x];
        for (int i = t; i < e.pl.unknowns; i += (int)blockDim.x) {
            const double xv = e.x[base + i], uo = e.u[base + i];
            e.v[base + i] = onchip_newmark_velocity(hv, xv, uo, e.v[base + i]);
            e.u[base + i] = xv;
        }
    }
};
// After a call the host's stop flag ended: a member that has not ended but whose state says done has converged a step (one that
// did not converge ends the member at once, without budget) and its transition waited for the next launch.  The host counts
// that step, so this launch does the state's part of the transition; the book stays.
__global__ __launch_bounds__(kOnchipMaxThreads) void k_onchip_wave_newmark_finish(const OnchipNewmarkArgs e) {
    const CgState* const sp = e.s + blockIdx.x;
    if (oc_wg_load(&e.book[blockIdx.x].ended) || !oc_wg_load(&sp->done) || !oc_wg_load(&sp->converged)) return;
    OcNewmark::advance(e, threadIdx.x);
}
__global__ __launch_bounds__(kOnchipMaxThreads) void k_onchip_wave_newmark_init(const OnchipNewmarkArgs e) {
    OcNewmark::start(e, OcMany::lds(e.pl.cells), threadIdx.x);
}
template <int E, bool MSG>
__global__ __launch_bounds__(kOnchipMaxThreads) void k_onchip_wave_newmark(const OnchipManyArgs a, const OnchipNewmarkArgs e) {
    oc_step_loop<E, MSG, OcNewmark>(a, e);
}

}  // namespace mi355cg
