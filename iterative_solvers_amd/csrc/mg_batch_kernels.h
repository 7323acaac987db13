// mg_batch_kernels.h -- HIP kernels (gfx950 / CDNA4, wave64) of the batched multigrid-preconditioned CG
// (mi355cg_solve_batch / mi355cg_solve_batch_device): a second grid dimension over the systems of a batch
// that are still iterating.
//
//   blockIdx.x, gridDim.x   exactly as in the single-system launch (MgLevel::grid): the rows a block takes, and with them the
//                           order of every sum, do not depend on the batch
//   blockIdx.y              position in the active list (MgbAct::sys); system s keeps vector v at v + s * MgbAct::stride
//   per-system scalars      (alpha, beta) come by position in MgbScal; the loop is host-driven as in solve_mg
//   partials                [system][field][block]; k_mgb_reduce sums a field's blocks left to right in one wave per
//                           (position, field) -- the sum solve_mg makes on the host -- into [position][field]
//
// k_mgb_smooth, _restrict, _prolong, _residual, _restrict_nn, _prolong_nn, _dir_apply and _dot call the __device__ bodies of
// mg_kernels.h (mg_smooth ... mg_dot) on their system's vectors: there is one expression and one reduction tree, so system s of
// a batch gets the bits a single solve gives it.  The others are kernels of their own: k_mgb_coarse walks the active list,
// k_mgb_update and k_mgb_init[_guess] have their own partial fields, k_mgb_reduce, k_mgb_pack and k_mgb_unpack have no single
// twin.  Systems never meet in a sum.  No kernel here writes a vector of a system that is not in the active list: a finished
// system stays frozen.  Plain fp64 arithmetic (no FMA contraction: -ffp-contract=off), no atomics, no LDS beyond the block
// reduction.
#pragma once
#include "mg_kernels.h"

namespace mi355cg {

constexpr int kMgBatchMax = 64;                    // = MI355CG_BATCH_MAX: the active list and the scalars travel as kernel arguments
enum { MGB_RR = 0, MGB_RMAX = 1, MGB_DMAX = 2, MGB_NFIELDS = 3 };   // k_mgb_update partials; fields >= MGB_RMAX are max-norms

struct MgbAct { long long stride; int n; int sys[kMgBatchMax]; };    // elements between two systems' vectors; active systems
struct MgbScal { double v[kMgBatchMax]; };                           // one scalar per active position

#define MGB_SYS(ACT) ((long long)(ACT).sys[blockIdx.y] * (ACT).stride)
#define MGB_SLOT(ACT) ((long long)(ACT).sys[blockIdx.y] * gridDim.x + blockIdx.x)      // of part[system][0][block]

// The bodies of mg_kernels.h on the vectors of blockIdx.y's system
template <bool FIRST, bool DOT>
__global__ __launch_bounds__(kBlock) void k_mgb_smooth(const MgbAct act, const Geom g, double omega, const double* __restrict__ r_,
                                                       const double* __restrict__ u_, double* __restrict__ t_, double* __restrict__ part) {
    const long long so = MGB_SYS(act);
    mg_smooth<FIRST, DOT>(g, omega, r_ + so, FIRST ? nullptr : u_ + so, t_ + so, DOT ? part + MGB_SLOT(act) : nullptr);
}

__global__ __launch_bounds__(kBlock) void k_mgb_restrict(const MgbAct act, const Geom gf, const Geom gc, const double* __restrict__ r_,
                                                         const double* __restrict__ u_, double* __restrict__ rc_) {
    const long long so = MGB_SYS(act);
    mg_restrict(gf, gc, r_ + so, u_ + so, rc_ + so);
}

__global__ __launch_bounds__(kBlock) void k_mgb_prolong(const MgbAct act, const Geom gf, const Geom gc, const double* __restrict__ e_,
                                                        double* __restrict__ u_) {
    const long long so = MGB_SYS(act);
    mg_prolong(gf, gc, e_ + so, u_ + so);
}

__global__ __launch_bounds__(kBlock) void k_mgb_residual(const MgbAct act, const Geom g, const double* __restrict__ r_,
                                                         const double* __restrict__ u_, double* __restrict__ s_) {
    const long long so = MGB_SYS(act);
    mg_residual(g, r_ + so, u_ + so, s_ + so);
}

__global__ __launch_bounds__(kBlock) void k_mgb_restrict_nn(const MgbAct act, const Geom gf, const Geom gc, double scale,
                                                            const double* __restrict__ s_, double* __restrict__ rc_) {
    const long long so = MGB_SYS(act);
    mg_restrict_nn(gf, gc, scale, s_ + so, rc_ + so);
}

__global__ __launch_bounds__(kBlock) void k_mgb_prolong_nn(const MgbAct act, const Geom gf, const Geom gc, const double* __restrict__ e_,
                                                           double* __restrict__ u_) {
    const long long so = MGB_SYS(act);
    mg_prolong_nn(gf, gc, e_ + so, u_ + so);
}

// Coarsest level, z = A_L^-1 r for every active system in one launch: block i owns row i of the inverse, keeps its lane-strided
// slice (<= kMgbCoarseSlots entries per thread, n <= kMgMaxCoarse) in registers and walks the active list, so the inverse is
// read once per launch and not once per system.  Per system the sum is k_mg_coarse's: lane-strided in ascending j, then the
// block tree.
constexpr int kMgbCoarseSlots = (kMgMaxCoarse + kBlock - 1) / kBlock;
__global__ __launch_bounds__(kBlock) void k_mgb_coarse(const MgbAct act, int n, const double* __restrict__ inv, const int* __restrict__ off,
                                                       const double* __restrict__ r_, double* __restrict__ z_) {
    __shared__ double lds[2 * kWaves];
    for (int i = blockIdx.x; i < n; i += gridDim.x) {                 // uniform per block: every thread reaches the reductions
        double a[kMgbCoarseSlots];
        int oj[kMgbCoarseSlots];
#pragma unroll
        for (int k = 0; k < kMgbCoarseSlots; ++k) {
            const int j = (int)threadIdx.x + k * kBlock;
            a[k] = j < n ? inv[(long long)i * n + j] : 0.0;
            oj[k] = j < n ? off[j] : -1;
        }
        const int oi = off[i];
        for (int pos = 0; pos < act.n; ++pos) {
            const long long so = (long long)act.sys[pos] * act.stride;
            const double* __restrict__ r = r_ + so;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < kMgbCoarseSlots; ++k) if (oj[k] >= 0) s += a[k] * r[oj[k]];
            const double t = block_reduce<false>(s, lds);
            if (threadIdx.x == 0) z_[so + oi] = t;
        }
    }
}

// beta by position; partials of (p, q) into part[system][0][block]
template <bool FIRST>
__global__ __launch_bounds__(kBlock) void k_mgb_dir_apply(const MgbAct act, const MgbScal betas, const Geom g, const double* __restrict__ z_,
                                                          const double* __restrict__ po_, double* __restrict__ p_,
                                                          double* __restrict__ q_, double* __restrict__ part) {
    const long long so = MGB_SYS(act);
    mg_dir_apply<FIRST>(g, betas.v[blockIdx.y], z_ + so, FIRST ? nullptr : po_ + so, p_ + so, q_ + so, part + MGB_SLOT(act));
}

// k_mg_update per active system, alpha by position; partials part[(system * MGB_NFIELDS + field) * gridDim.x + block] of (r, r),
// max |r| and max |dx| (a batch has no exact solution, and (dx, dx) feeds only the callbacks a batch does not have)
__global__ __launch_bounds__(kBlock) void k_mgb_update(const MgbAct act, const MgbScal alphas, const Geom g, double* __restrict__ x_,
                                                       double* __restrict__ r_, const double* __restrict__ p_, const double* __restrict__ q_,
                                                       double* __restrict__ part) {
    __shared__ double lds[2 * kWaves];
    const long long so = MGB_SYS(act);
    const double alpha = alphas.v[blockIdx.y];
    double* __restrict__ x = x_ + so;
    double* __restrict__ r = r_ + so;
    const double* __restrict__ p = p_ + so;
    const double* __restrict__ q = q_ + so;
    double rr = 0, rmax = 0, dmax = 0;
    MG_FOR_INTERIOR(g, xx, y) {
        const long long o = mg_off(g, xx, y);
        const double xo = x[o];
        const double xn = xo + alpha * p[o];
        const double rn = r[o] - alpha * q[o];
        x[o] = xn;
        r[o] = rn;
        const double dx = xn - xo;
        rr += rn * rn;
        rmax = fmax(rmax, fabs(rn)); dmax = fmax(dmax, fabs(dx));
    }
    const long long n = gridDim.x, base = (long long)act.sys[blockIdx.y] * MGB_NFIELDS * n + blockIdx.x;
    double t;
    t = block_reduce<false>(rr, lds); if (threadIdx.x == 0) part[base + MGB_RR * n] = t;
    t = block_reduce<true>(rmax, lds); if (threadIdx.x == 0) part[base + MGB_RMAX * n] = t;
    t = block_reduce<true>(dmax, lds); if (threadIdx.x == 0) part[base + MGB_DMAX * n] = t;
}

// The start of a solve for every system: x = 0 over the interior (r already holds b: k_mgb_unpack wrote it there) with the
// partials solve_mg's zero step gives: (r, r) and max |r| of r = b - 0 * 0, and max |dx| = 0.  Same layout as k_mgb_update.
__global__ __launch_bounds__(kBlock) void k_mgb_init(const MgbAct act, const Geom g, double* __restrict__ x_, const double* __restrict__ r_,
                                                     double* __restrict__ part) {
    __shared__ double lds[2 * kWaves];
    const long long so = MGB_SYS(act);
    double* __restrict__ x = x_ + so;
    const double* __restrict__ r = r_ + so;
    double rr = 0, rmax = 0;
    MG_FOR_INTERIOR(g, xx, y) {
        const long long o = mg_off(g, xx, y);
        const double rn = r[o];
        x[o] = 0.0;
        rr += rn * rn;
        rmax = fmax(rmax, fabs(rn));
    }
    const long long n = gridDim.x, base = (long long)act.sys[blockIdx.y] * MGB_NFIELDS * n + blockIdx.x;
    double t;
    t = block_reduce<false>(rr, lds); if (threadIdx.x == 0) part[base + MGB_RR * n] = t;
    t = block_reduce<true>(rmax, lds); if (threadIdx.x == 0) { part[base + MGB_RMAX * n] = t; part[base + MGB_DMAX * n] = 0.0; }
}

// The warm start of a batch (mi355cg_solve_batch*_from): x holds the guess and r holds b (k_mgb_unpack wrote both).  Per system
// r = b - A x with A x in the operation order of the plain operator (k_stencil: ((((A c + xk l) + xk r) + yk up) + yk down); mg_Av
// groups the neighbours first and differs in the last bit), which is what the single warm solve forms with launch_apply and
// k_sub.  Only r of the node itself is written, so no neighbour's operand changes under a reader.  Partials of this kernel alone,
// part[(system * MGBG_NFIELDS + field) * gridDim.x + block]: (r, r) and (b, b) in k_mgb_init's order, max |r|, and max |dx| = 0.
enum { MGBG_RR = 0, MGBG_BB = 1, MGBG_RMAX = 2, MGBG_DMAX = 3, MGBG_NFIELDS = 4 };   // fields >= MGBG_RMAX are max-norms
__global__ __launch_bounds__(kBlock) void k_mgb_init_guess(const MgbAct act, const Geom g, const double* __restrict__ x_, double* __restrict__ r_,
                                                           double* __restrict__ part) {
    __shared__ double lds[2 * kWaves];
    const long long so = MGB_SYS(act);
    const double* __restrict__ x = x_ + so;
    double* __restrict__ r = r_ + so;
    double rr = 0, bb = 0, rmax = 0;
    MG_FOR_INTERIOR(g, xx, y) {
        const long long o = mg_off(g, xx, y);
        double v = g.A * x[o];
        v = v + g.xk * x[o - 1];
        v = v + g.xk * x[o + 1];
        v = v + g.yk * mg_at(g, x, xx, y + 1);
        v = v + g.yk * mg_at(g, x, xx, y - 1);
        const double bv = r[o];
        const double rn = bv - v;
        r[o] = rn;
        rr += rn * rn; bb += bv * bv;
        rmax = fmax(rmax, fabs(rn));
    }
    const long long n = gridDim.x, base = (long long)act.sys[blockIdx.y] * MGBG_NFIELDS * n + blockIdx.x;
    double t;
    t = block_reduce<false>(rr, lds); if (threadIdx.x == 0) part[base + MGBG_RR * n] = t;
    t = block_reduce<false>(bb, lds); if (threadIdx.x == 0) part[base + MGBG_BB * n] = t;
    t = block_reduce<true>(rmax, lds); if (threadIdx.x == 0) { part[base + MGBG_RMAX * n] = t; part[base + MGBG_DMAX * n] = 0.0; }
}

// the (r, z) of a one-level hierarchy
__global__ __launch_bounds__(kBlock) void k_mgb_dot(const MgbAct act, const Geom g, const double* __restrict__ a_, const double* __restrict__ b_,
                                                    double* __restrict__ part) {
    const long long so = MGB_SYS(act);
    mg_dot(g, a_ + so, b_ + so, part + MGB_SLOT(act));
}

// red[position][field] = the field's nblocks partials of the position's system summed (fields >= first_max: maxed) serially in
// block order from 0 -- what solve_mg's host loop does, hence the same bits -- so that a host wait fetches act.n * nfields
// doubles instead of all partials.  One wave per (field, position): the lanes load 64 consecutive partials at once (the next 64
// are in flight meanwhile), then the wave walks them in order, each read out of its lane into scalar registers (v_readlane), so
// a step of the chain costs the add and not a trip through the LDS crossbar.  The max is the host loop's std::max(s, v) =
// (s < v) ? v : s, not fmax: the two differ on NaN.
__device__ inline double mgb_read_lane(double v, int lane /* uniform */) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}
template <bool IS_MAX>
__device__ inline double mgb_chain(const double* __restrict__ src, int nblocks) {
    const int lane = threadIdx.x;
    double s = 0.0;
    double next = lane < nblocks ? src[lane] : 0.0;
    for (int c = 0; c < nblocks; c += kWave) {
        const double cur = next;
        const int cn = c + kWave;
        next = cn + lane < nblocks ? src[cn + lane] : 0.0;
        const int cnt = nblocks - c < kWave ? nblocks - c : kWave;
        for (int k = 0; k < cnt; ++k) {
            const double v = mgb_read_lane(cur, k);
            s = IS_MAX ? ((s < v) ? v : s) : s + v;
        }
    }
    return s;
}
__global__ __launch_bounds__(kWave) void k_mgb_reduce(const MgbAct act, int nfields, int first_max, int nblocks,
                                                      const double* __restrict__ part, double* __restrict__ red) {
    const int f = blockIdx.x, pos = blockIdx.y;
    const double* __restrict__ src = part + ((long long)act.sys[pos] * nfields + f) * nblocks;
    const double s = f >= first_max ? mgb_chain<true>(src, nblocks) : mgb_chain<false>(src, nblocks);
    if (threadIdx.x == 0) red[pos * nfields + f] = s;
}

// packed (caller's order) <-> storage for every system of a batch: blockIdx.y = system, packed vector s at packed + s * pk_len
__global__ __launch_bounds__(kBlock) void k_mgb_unpack(const PackGeom pg, long long stride, const double* __restrict__ packed,
                                                       double* __restrict__ storage) {
    const double* __restrict__ src = packed + (long long)blockIdx.y * pg.pk_len;
    double* __restrict__ dst = storage + (long long)blockIdx.y * stride;
    const long long step = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < pg.pk_len; i += step) dst[packed_to_storage(pg, i)] = src[i];
}
__global__ __launch_bounds__(kBlock) void k_mgb_pack(const PackGeom pg, long long stride, const double* __restrict__ storage,
                                                     double* __restrict__ packed) {
    const double* __restrict__ src = storage + (long long)blockIdx.y * stride;
    double* __restrict__ dst = packed + (long long)blockIdx.y * pg.pk_len;
    const long long step = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < pg.pk_len; i += step) dst[i] = src[packed_to_storage(pg, i)];
}

#undef MGB_SLOT
#undef MGB_SYS

}  // namespace mi355cg
