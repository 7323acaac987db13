// mg_line_kernels.h -- HIP kernels (gfx950 / CDNA4, wave64) of the opt-in line smoother of the fp64 V-cycle
// (mi355cg_set_smoother).
//
//   k_mg_line<DIR, FIRST, DOT>    one damped line-Jacobi sweep  t = u + omega * T^-1 (r - A u)  [FIRST: u = 0; DOT: + per-block
//                                 partials of (r, t), the (r, z) of the PCG, fused into the last sweep of level 0]
//   k_mgb_line<DIR, FIRST, DOT>   the same on the vectors of blockIdx.y's system of a batch
//
// T is the level's operator along the lines: the diagonal g.A and the coupling k = g.xk (DIR = MG_LINE_X: a line is a row) or
// g.yk (MG_LINE_Y: a column) to the two neighbours in the line.  A line is a maximal run of interior nodes: line l (a row y = l
// or a column x = l, 1 <= l <= N - 1) runs over positions mg_x0(l) .. N - 1 -- the L-shape is symmetric under x <-> y, so the
// first position is the same function of l for both directions.  Every line of a level has the same constant coefficients, so
// the Thomas factors of a line of length n are the first n entries of one sequence (host: mg_line_table):
//     inv_1 = 1 / A,  cp_i = k inv_i,  inv_i = 1 / (A - k cp_{i-1})          tab[i] = inv_i, tab[N + i] = cp_i,  1 <= i <= N - 1
//     forward   d_i = ((r - A u)_i - k d_{i-1}) inv_i   (d_0 = 0)            backward   e_i = d_i - cp_i e_{i+1}   (e_{n+1} = 0)
//
// A block takes kLines = 16 lines and walks them in segments of kSeg = 256 positions through one LDS tile, forward and then back:
//   load    all 256 threads form r - A u for the tile's nodes (16 independent nodes per thread, coalesced along x for both
//           directions: for rows the fast index is the position, for columns it is the line) and put them into the tile
//           (every load at an address that is valid whether or not the slot is a node of the block, so that none waits behind a
//           branch), and every thread puts the factors of its position for the two possible line starts beside it
//   march   16 lanes of wave 0 have a line each and walk its 256 positions in the tile, the carry (d_{i-1}, e_{i+1}) in a register,
//           in batches of 16 positions read from LDS into registers before the chain starts
//   store   all threads write the tile back, coalesced: d into t after the forward march (t is the sweep's own intermediate),
//           t = u + omega e after the backward one
// The tile is stored (slow index) * pitch + (fast index), pitch = the fast extent + 1: the load and store phases touch consecutive
// words, and the march walks a row of the tile (rows) or a column (columns) with the odd pitch keeping the lanes on different
// banks.  So neither direction needs a whole line in LDS, and the chains of a level are spread over ceil((N - 1) / 16)
// workgroups: few lines and long segments, because a sweep is bound by the latency of its load - march - store steps (measured:
// about 6 us each, plus 0.1 us per position marched), of which a line of n nodes needs 2 ceil(n / 256).
// Only interior nodes are written; a node left of the bottom block's storage reads as 0 (mg_at).  The (r, t) partial of a block is
// summed per thread in segment order and then by the fixed block tree: the same inputs give the same bits on every run.  Plain
// fp64 arithmetic (no FMA contraction: -ffp-contract=off).
#pragma once
#include "mg_batch_kernels.h"

namespace mi355cg {

enum { MG_LINE_X = 1, MG_LINE_Y = 2 };            // = the direction mi355cg_get_smoother reports
constexpr int kLines = 16;                        // lines per block = lanes that march
constexpr int kSeg = kBlock;                      // positions per segment
constexpr int kLineSlots = kLines * kSeg / kBlock;             // tile slots per thread
constexpr int kLineTileLen = kSeg * (kLines + 1) > kLines * (kSeg + 1) ? kSeg * (kLines + 1) : kLines * (kSeg + 1);
static_assert(kLines <= kWave && kBlock % kLines == 0 && kSeg == kBlock, "the marching lanes are in wave 0; a thread per position loads the factors");

// blocks a level's line sweep needs (the sweep with DOT is launched on the level's row-marching grid, whose partial slots the
// PCG sums: that grid is never smaller)
__host__ __device__ inline int mg_line_blocks(int N) { return (N - 1 + kLines - 1) / kLines; }

// A tile slot of this thread: slot q is tile (slow0 + q * kSlowStep, fast); the fast index is the one along x, i.e. the position
// for rows (kSeg wide) and the line for columns (kLines wide: 128 B of a row, one cache line), the pitch its extent + 1.
// ok: it is an interior node of the block's lines; if not, (x, y) is the last node of the block's last line l1 (interior, and read and written by this block alone), so that every load
// below can be issued without a branch and a thread has all the loads of its slots in flight together (a load behind a branch
// would wait for the one before it).
struct LineSlot { int x, y, at; bool ok; long long o; };
template <int DIR>
__device__ __forceinline__ LineSlot mg_line_slot(const Geom& g, int l0, int l1, int s0, int q) {
    constexpr int kFast = DIR == MG_LINE_X ? kSeg : kLines, kSlowStep = kBlock / kFast;
    const int fast = (int)threadIdx.x % kFast, slow = (int)threadIdx.x / kFast + q * kSlowStep;
    const int line = l0 + (DIR == MG_LINE_X ? slow : fast), s = s0 + (DIR == MG_LINE_X ? fast : slow), last = g.N - 1;
    LineSlot n;
    n.ok = line <= last && s <= last && s >= mg_x0(g, line);
    n.x = n.ok ? (DIR == MG_LINE_X ? s : line) : (DIR == MG_LINE_X ? last : l1);
    n.y = n.ok ? (DIR == MG_LINE_X ? line : s) : (DIR == MG_LINE_X ? l1 : last);
    n.at = slow * (kFast + 1) + fast;
    n.o = mg_off(g, n.x, n.y);
    return n;
}

template <int DIR, bool FIRST, bool DOT>
__device__ __forceinline__ void mg_line(const Geom g, double omega, const double* __restrict__ tab, const double* __restrict__ r,
                                        const double* __restrict__ u, double* __restrict__ t, double* __restrict__ slot) {
    __shared__ double tile[kLineTileLen];
    __shared__ double ltab[2][kSeg];                  // the segment's factors (inv going forward, cp going back) for the two line starts
    __shared__ double lds[2 * kWaves];
    const double k = DIR == MG_LINE_X ? g.xk : g.yk;
    const int last = g.N - 1;
    const int tid = (int)threadIdx.x;
    constexpr int kPerThread = kLineSlots, kGroup = 8, kMarch = 16;
    static_assert(kPerThread % kGroup == 0 && kSeg % kMarch == 0, "slot groups, march batches");
    auto march_at = [&](int j) { return DIR == MG_LINE_X ? tid * (kSeg + 1) + j : j * (kLines + 1) + tid; };
    double acc = 0.0;
    for (int l0 = 1 + (int)blockIdx.x * kLines; l0 <= last; l0 += (int)gridDim.x * kLines) {    // uniform per block
        const int l1 = l0 + kLines - 1 < last ? l0 + kLines - 1 : last;
        const int sb = mg_x0(g, l1);                             // the first position of the block's longest line
        const int nseg = (last - sb) / kSeg + 1;
        const int ml = l0 + tid, mst = mg_x0(g, ml);             // the marching lane's line and its first position
        const bool marching = tid < kLines && ml <= last;
        for (int pass = 0; pass < 2; ++pass) {                   // 0: forward elimination, 1: back substitution
            double carry = 0.0;
            for (int sg = 0; sg < nseg; ++sg) {
                const int s0 = sb + (pass == 0 ? sg : nseg - 1 - sg) * kSeg;
#pragma unroll
                for (int which = 0; which < 2; ++which) {        // factor i of position s0 + tid of a line that starts at 1 / at N/2 + 1
                    const int i = s0 + tid - (which ? g.half + 1 : 1) + 1;
                    ltab[which][tid] = tab[(pass == 0 ? 0 : g.N) + (i >= 1 && i <= last ? i : 1)];
                }
                if (pass == 1) {
                    double v[kPerThread];
#pragma unroll
                    for (int q = 0; q < kPerThread; ++q) v[q] = t[mg_line_slot<DIR>(g, l0, l1, s0, q).o];
#pragma unroll
                    for (int q = 0; q < kPerThread; ++q) { const LineSlot n = mg_line_slot<DIR>(g, l0, l1, s0, q); if (n.ok) tile[n.at] = v[q]; }
                } else if (FIRST) {
                    double v[kPerThread];
#pragma unroll
                    for (int q = 0; q < kPerThread; ++q) v[q] = r[mg_line_slot<DIR>(g, l0, l1, s0, q).o];
#pragma unroll
                    for (int q = 0; q < kPerThread; ++q) { const LineSlot n = mg_line_slot<DIR>(g, l0, l1, s0, q); if (n.ok) tile[n.at] = v[q]; }
                } else {
#pragma unroll
                    for (int q0 = 0; q0 < kPerThread; q0 += kGroup) {
                        double rv[kGroup], c[kGroup], lf[kGroup], rt[kGroup], dn[kGroup], up[kGroup];
#pragma unroll
                        for (int q = 0; q < kGroup; ++q) {
                            const LineSlot n = mg_line_slot<DIR>(g, l0, l1, s0, q0 + q);
                            const bool no_dn = n.y - 1 <= g.half && n.x < g.cb;      // left of the bottom block's storage: 0 (mg_at)
                            rv[q] = r[n.o]; c[q] = u[n.o]; lf[q] = u[n.o - 1]; rt[q] = u[n.o + 1];
                            up[q] = u[mg_off(g, n.x, n.y + 1)];
                            dn[q] = u[no_dn ? n.o : mg_off(g, n.x, n.y - 1)];
                            dn[q] = no_dn ? 0.0 : dn[q];
                        }
#pragma unroll
                        for (int q = 0; q < kGroup; ++q) {                           // r - A u, mg_Av's expression
                            const LineSlot n = mg_line_slot<DIR>(g, l0, l1, s0, q0 + q);
                            if (n.ok) tile[n.at] = rv[q] - (g.A * c[q] + g.xk * (lf[q] + rt[q]) + g.yk * (dn[q] + up[q]));
                        }
                    }
                }
                __syncthreads();
                if (marching) {
                    const int jlo = mst > s0 ? mst - s0 : 0, jhi = last - s0 < kSeg - 1 ? last - s0 : kSeg - 1;
                    const double* __restrict__ lt = ltab[mst == 1 ? 0 : 1];
#pragma unroll 1
                    for (int b = 0; b < kSeg; b += kMarch) {
                        const int j0 = pass == 0 ? b : kSeg - kMarch - b;
                        if (j0 + kMarch - 1 < jlo || j0 > jhi) continue;             // no position of the lane's line in this batch
                        double v[kMarch], f[kMarch];
#pragma unroll
                        for (int q = 0; q < kMarch; ++q) {
                            const int j = j0 + q;
                            v[q] = tile[march_at(j)];
                            f[q] = lt[j];
                        }
#pragma unroll
                        for (int qq = 0; qq < kMarch; ++qq) {
                            const int q = pass == 0 ? qq : kMarch - 1 - qq, j = j0 + q;
                            const double next = pass == 0 ? (v[q] - k * carry) * f[q] : v[q] - f[q] * carry;
                            carry = j >= jlo && j <= jhi ? next : carry;
                            v[q] = carry;
                        }
#pragma unroll
                        for (int q = 0; q < kMarch; ++q) {
                            const int j = j0 + q;
                            if (j >= jlo && j <= jhi) tile[march_at(j)] = v[q];
                        }
                    }
                }
                __syncthreads();
                if (pass == 0) {
#pragma unroll
                    for (int q = 0; q < kPerThread; ++q) { const LineSlot n = mg_line_slot<DIR>(g, l0, l1, s0, q); if (n.ok) t[n.o] = tile[n.at]; }
                } else {
                    double uv[kPerThread], rv[kPerThread];
#pragma unroll
                    for (int q = 0; q < kPerThread; ++q) {
                        const LineSlot n = mg_line_slot<DIR>(g, l0, l1, s0, q);
                        uv[q] = FIRST ? 0.0 : u[n.o];
                        rv[q] = DOT ? r[n.o] : 0.0;
                    }
#pragma unroll
                    for (int q = 0; q < kPerThread; ++q) {
                        const LineSlot n = mg_line_slot<DIR>(g, l0, l1, s0, q);
                        if (n.ok) {
                            const double e = tile[n.at];
                            const double tv = FIRST ? omega * e : uv[q] + omega * e;
                            t[n.o] = tv;
                            if (DOT) acc += rv[q] * tv;
                        }
                    }
                }
                __syncthreads();                                 // the tile is free, and the d this block wrote are there for its way back
            }
        }
    }
    if (DOT) {
        const double b = block_reduce<false>(acc, lds);
        if (threadIdx.x == 0) *slot = b;
    }
}

template <int DIR, bool FIRST, bool DOT>
__global__ __launch_bounds__(kBlock) void k_mg_line(const Geom g, double omega, const double* __restrict__ tab, const double* __restrict__ r,
                                                    const double* __restrict__ u, double* __restrict__ t, double* __restrict__ part) {
    mg_line<DIR, FIRST, DOT>(g, omega, tab, r, u, t, DOT ? part + blockIdx.x : nullptr);
}

// part[system][0][block], as k_mgb_smooth
template <int DIR, bool FIRST, bool DOT>
__global__ __launch_bounds__(kBlock) void k_mgb_line(const MgbAct act, const Geom g, double omega, const double* __restrict__ tab,
                                                     const double* __restrict__ r_, const double* __restrict__ u_, double* __restrict__ t_,
                                                     double* __restrict__ part) {
    const long long so = (long long)act.sys[blockIdx.y] * act.stride;
    mg_line<DIR, FIRST, DOT>(g, omega, tab, r_ + so, FIRST ? nullptr : u_ + so, t_ + so,
                             DOT ? part + (long long)act.sys[blockIdx.y] * gridDim.x + blockIdx.x : nullptr);
}

}  // namespace mi355cg
