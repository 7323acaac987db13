// mg_kernels.h -- HIP kernels (gfx950 / CDNA4, wave64) of the opt-in geometric multigrid preconditioner and of the
// preconditioned CG loop built on it (mi355cg_set_preconditioner(h, MI355CG_PRECOND_MG)).
//
//   k_mg_smooth     one damped-Jacobi sweep  t = u + omega * ((r - A u) / diag)  [u = 0: the first sweep of a cycle;
//                   + per-block partials of (r, t): the (r, z) of the PCG, fused into the last sweep of level 0]
//   k_mg_restrict   residual s = r - A u on the fine grid fused with full weighting onto the coarse interior
//   k_mg_prolong    bilinear prolongation of the coarse correction fused with u += P e, masked to the fine interior
//   k_mg_residual   s = r - A u at the fine interior nodes (non-nested levels, N_f % 4 == 2; into the level's work vector)
//   k_mg_restrict_nn   R s = (N_c / N_f)^2 P^T s: a gather over the <= 5 x 5 fine nodes of a coarse node's bilinear support
//   k_mg_prolong_nn    u += P e with the bilinear weights of non-nested grids, masked to the fine interior
//   k_mg_coarse     coarsest level: z = A_L^-1 r, one dense mat-vec with the inverse built on the host
//   k_mg_dir_apply  PCG direction p = z + beta p_old (ping-pong buffers) fused with q = A p and partials of (p, q)
//   k_mg_update     x += alpha p, r -= alpha q with partials of (r, r), (dx, dx), (x - u, x - u) and the max-norms
//   k_mg_dot, k_mg_resid2   (r, z) when level 0 is the coarsest; ||b - A x||^2 partials for the REL_2NORM diagnostics
//
// Every level keeps the pitched storage layout of cg_kernels.h (Geom for N_l, the whole grid, base0 = 0).  Boundary nodes and
// pads hold 0 and no kernel here writes anything but interior nodes, so every stencil applies one formula; the only node a
// stencil can name that is not stored is (x, N_l/2) with x < cb (left of the bottom block's storage), which mg_at reads as 0.
// All reductions have a fixed order (a fixed grid, a fixed tree per block, the blocks summed by the host in index order), so
// the same inputs give the same bits on every run.  Plain fp64 arithmetic (no FMA contraction: -ffp-contract=off).
//
// The element-wise loops of smooth, restrict, prolong, residual, restrict_nn, prolong_nn, dir_apply and dot are written once, as
// the __device__ functions mg_smooth ... mg_dot: they take the level geometry, the vectors of one system and the address of the
// block's partial slot.  k_mg_X passes its arguments through; k_mgb_X (mg_batch_kernels.h) offsets every vector to its system.
// They take Geom by value, as the kernels do: by reference the compiler gives mg_restrict_nn's two kernels two VGPRs more.
#pragma once
#include "cg_kernels.h"

namespace mi355cg {

constexpr int kMgMaxGrid = 2048;                  // row-marching grids: at most this many blocks (= partial slots)
constexpr int kMgMaxCoarse = 705;                 // unknowns of the coarsest grid: N_L <= 32 -> (N_L/2 - 1)(3 N_L/2 - 1) <= 705
enum { MG_RR = 0, MG_D2 = 1, MG_E2 = 2, MG_RMAX = 3, MG_DMAX = 4, MG_EMAX = 5, MG_NFIELDS = 6 };   // k_mg_update partials

__host__ __device__ inline long long mg_off(const Geom& g, int x, int y) { return row_off(g, y) - g.base0 + x; }
// value of node (x, y), 0 <= x, y <= N: nodes left of the bottom block's storage are boundary or exterior, i.e. 0
__device__ inline double mg_at(const Geom& g, const double* __restrict__ v, int x, int y) {
    return (y <= g.half && x < g.cb) ? 0.0 : v[mg_off(g, x, y)];
}
// (A v)(x, y) at an interior node: the 5-point formula of the level
__device__ inline double mg_Av(const Geom& g, const double* __restrict__ v, int x, int y) {
    const long long o = mg_off(g, x, y);
    return g.A * v[o] + g.xk * (v[o - 1] + v[o + 1]) + g.yk * (mg_at(g, v, x, y - 1) + mg_at(g, v, x, y + 1));
}
__device__ inline int mg_x0(const Geom& g, int y) { return y <= g.half ? g.half + 1 : 1; }    // first interior column of row y

// The row loops: block b takes interior rows 1 + b, 1 + b + gridDim.x, ...; its threads stride the row's interior columns.
// (mg_batch_kernels.h and eig_kernels.h use the macro too; the last of them undefines it.)
#define MG_FOR_INTERIOR(G, XI, YI)                                                                 \
    for (int YI = 1 + (int)blockIdx.x; YI <= (G).N - 1; YI += (int)gridDim.x)                      \
        for (int XI = mg_x0((G), YI) + (int)threadIdx.x; XI <= (G).N - 1; XI += kBlock)

// slot (DOT): where this block's partial of (r, t) goes
template <bool FIRST, bool DOT>
__device__ __forceinline__ void mg_smooth(const Geom g, double omega, const double* __restrict__ r, const double* __restrict__ u,
                                          double* __restrict__ t, double* __restrict__ slot) {
    __shared__ double lds[2 * kWaves];
    double s = 0.0;
    MG_FOR_INTERIOR(g, x, y) {
        const long long o = mg_off(g, x, y);
        const double rv = r[o];
        double tv;
        if (FIRST) tv = omega * (rv / g.A);                              // u = 0: 0 + omega * ((r - 0) / diag)
        else tv = u[o] + omega * ((rv - mg_Av(g, u, x, y)) / g.A);
        t[o] = tv;
        if (DOT) s += rv * tv;
    }
    if (DOT) {
        const double b = block_reduce<false>(s, lds);
        if (threadIdx.x == 0) *slot = b;
    }
}
template <bool FIRST, bool DOT>
__global__ __launch_bounds__(kBlock) void k_mg_smooth(const Geom g, double omega, const double* __restrict__ r,
                                                      const double* __restrict__ u, double* __restrict__ t, double* __restrict__ part) {
    mg_smooth<FIRST, DOT>(g, omega, r, u, t, DOT ? part + blockIdx.x : nullptr);
}

// coarse interior node (X, Y) <- full weighting of s = r - A u around fine node (2X, 2Y); s = 0 off the fine interior
__device__ inline double mg_fine_residual(const Geom& gf, const double* __restrict__ r, const double* __restrict__ u, int x, int y) {
    return node_interior(gf, x, y) ? r[mg_off(gf, x, y)] - mg_Av(gf, u, x, y) : 0.0;
}
__device__ __forceinline__ void mg_restrict(const Geom gf, const Geom gc, const double* __restrict__ r, const double* __restrict__ u,
                                            double* __restrict__ rc) {
    MG_FOR_INTERIOR(gc, X, Y) {
        const int x = 2 * X, y = 2 * Y;
        const double s00 = mg_fine_residual(gf, r, u, x, y);
        const double sl = mg_fine_residual(gf, r, u, x - 1, y), sr = mg_fine_residual(gf, r, u, x + 1, y);
        const double sd = mg_fine_residual(gf, r, u, x, y - 1), su = mg_fine_residual(gf, r, u, x, y + 1);
        const double sld = mg_fine_residual(gf, r, u, x - 1, y - 1), srd = mg_fine_residual(gf, r, u, x + 1, y - 1);
        const double slu = mg_fine_residual(gf, r, u, x - 1, y + 1), sru = mg_fine_residual(gf, r, u, x + 1, y + 1);
        rc[mg_off(gc, X, Y)] = 0.0625 * (4.0 * s00 + 2.0 * (sl + sr + sd + su) + (sld + srd + slu + sru));
    }
}
__global__ __launch_bounds__(kBlock) void k_mg_restrict(const Geom gf, const Geom gc, const double* __restrict__ r,
                                                        const double* __restrict__ u, double* __restrict__ rc) { mg_restrict(gf, gc, r, u, rc); }

// fine interior node (x, y): u += bilinear interpolation of the coarse correction e (0 on the coarse boundary)
__device__ __forceinline__ void mg_prolong(const Geom gf, const Geom gc, const double* __restrict__ e, double* __restrict__ u) {
    MG_FOR_INTERIOR(gf, x, y) {
        const int cx = x >> 1, cy = y >> 1;
        const double e00 = mg_at(gc, e, cx, cy);
        double corr;
        if ((x & 1) && (y & 1)) corr = 0.25 * (e00 + mg_at(gc, e, cx + 1, cy) + mg_at(gc, e, cx, cy + 1) + mg_at(gc, e, cx + 1, cy + 1));
        else if (x & 1) corr = 0.5 * (e00 + mg_at(gc, e, cx + 1, cy));
        else if (y & 1) corr = 0.5 * (e00 + mg_at(gc, e, cx, cy + 1));
        else corr = e00;
        const long long o = mg_off(gf, x, y);
        u[o] = u[o] + corr;
    }
}
__global__ __launch_bounds__(kBlock) void k_mg_prolong(const Geom gf, const Geom gc, const double* __restrict__ e,
                                                       double* __restrict__ u) { mg_prolong(gf, gc, e, u); }

// ---- non-nested levels (MI355CG_PRECOND_MG_ANY, N_f % 4 == 2, N_c = 2 floor(N_f / 4) = (N_f - 2) / 2) -------------------------
// 1-D bilinear weight of coarse node X at fine node x: the hat of coarse width around X at x's physical place x / N_f, i.e.
// max(0, 1 - |x N_c - X N_f| / N_f).  The numerator is an exact integer, so P and R use the same bits.  At N_f = 2 N_c it gives
// 1 and 1/2: the kernels above.
__host__ __device__ inline double mg_w(int x, int X, int Nf, int Nc) {
    long long d = (long long)x * Nc - (long long)X * Nf;
    if (d < 0) d = -d;
    return d < Nf ? (double)(Nf - d) / (double)Nf : 0.0;
}

// s = r - A u at fine interior nodes; nothing else is written, so s keeps the zero boundary of the level's vectors
__device__ __forceinline__ void mg_residual(const Geom g, const double* __restrict__ r, const double* __restrict__ u, double* __restrict__ s) {
    MG_FOR_INTERIOR(g, x, y) {
        const long long o = mg_off(g, x, y);
        s[o] = r[o] - mg_Av(g, u, x, y);
    }
}
__global__ __launch_bounds__(kBlock) void k_mg_residual(const Geom g, const double* __restrict__ r, const double* __restrict__ u,
                                                        double* __restrict__ s) { mg_residual(g, r, u, s); }

// coarse interior node (X, Y) <- scale * sum over fine nodes y ascending, then x ascending, of w(y, Y) w(x, X) s(x, y), scale =
// (N_c / N_f)^2.  The support |x N_c - X N_f| < N_f is x_lo..x_hi below, <= 5 nodes wide and inside 1..N_f - 1 for 1 <= X <= N_c - 1.
__device__ __forceinline__ void mg_restrict_nn(const Geom gf, const Geom gc, double scale, const double* __restrict__ s,
                                               double* __restrict__ rc) {
    const int Nf = gf.N, Nc = gc.N;
    MG_FOR_INTERIOR(gc, X, Y) {
        const int x_lo = (int)((long long)(X - 1) * Nf / Nc) + 1, x_hi = (int)(((long long)(X + 1) * Nf - 1) / Nc);
        const int y_lo = (int)((long long)(Y - 1) * Nf / Nc) + 1, y_hi = (int)(((long long)(Y + 1) * Nf - 1) / Nc);
        double acc = 0.0;
        for (int y = y_lo; y <= y_hi; ++y) {
            const double wy = mg_w(y, Y, Nf, Nc);
            for (int x = x_lo; x <= x_hi; ++x) acc += (wy * mg_w(x, X, Nf, Nc)) * mg_at(gf, s, x, y);
        }
        rc[mg_off(gc, X, Y)] = scale * acc;
    }
}
__global__ __launch_bounds__(kBlock) void k_mg_restrict_nn(const Geom gf, const Geom gc, double scale, const double* __restrict__ s,
                                                           double* __restrict__ rc) { mg_restrict_nn(gf, gc, scale, s, rc); }

// fine interior node (x, y): u += sum of w(x, X) w(y, Y) e(X, Y) over the coarse nodes X0 = floor(x N_c / N_f), X0 + 1 (same in y)
__device__ __forceinline__ void mg_prolong_nn(const Geom gf, const Geom gc, const double* __restrict__ e, double* __restrict__ u) {
    const int Nf = gf.N, Nc = gc.N;
    MG_FOR_INTERIOR(gf, x, y) {
        const int X0 = (int)((long long)x * Nc / Nf), Y0 = (int)((long long)y * Nc / Nf);
        const double wx0 = mg_w(x, X0, Nf, Nc), wx1 = mg_w(x, X0 + 1, Nf, Nc);
        const double wy0 = mg_w(y, Y0, Nf, Nc), wy1 = mg_w(y, Y0 + 1, Nf, Nc);
        const double corr = wy0 * (wx0 * mg_at(gc, e, X0, Y0) + wx1 * mg_at(gc, e, X0 + 1, Y0)) +
                            wy1 * (wx0 * mg_at(gc, e, X0, Y0 + 1) + wx1 * mg_at(gc, e, X0 + 1, Y0 + 1));
        const long long o = mg_off(gf, x, y);
        u[o] = u[o] + corr;
    }
}
__global__ __launch_bounds__(kBlock) void k_mg_prolong_nn(const Geom gf, const Geom gc, const double* __restrict__ e,
                                                          double* __restrict__ u) { mg_prolong_nn(gf, gc, e, u); }

// z[off[i]] = sum_j inv[i][j] r[off[j]]: block-strided rows, each summed lane-strided and by the fixed block tree
__global__ __launch_bounds__(kBlock) void k_mg_coarse(int n, const double* __restrict__ inv, const int* __restrict__ off,
                                                      const double* __restrict__ r, double* __restrict__ z) {
    __shared__ double lds[2 * kWaves];
    for (int i = blockIdx.x; i < n; i += gridDim.x) {                 // uniform per block: every thread reaches the reduction
        double s = 0.0;
        for (int j = threadIdx.x; j < n; j += kBlock) s += inv[(long long)i * n + j] * r[off[j]];
        const double t = block_reduce<false>(s, lds);
        if (threadIdx.x == 0) z[off[i]] = t;
    }
}

// p = z + beta * p_old (first iteration: p = z) evaluated at the node and its four neighbours, q = A p, partials of (p, q).
// p_old and p are different buffers: a neighbour's p_old must still be there when this node reads it.
template <bool FIRST>
__device__ __forceinline__ void mg_dir_apply(const Geom g, double beta, const double* __restrict__ z, const double* __restrict__ po,
                                             double* __restrict__ p, double* __restrict__ q, double* __restrict__ slot) {
    __shared__ double lds[2 * kWaves];
    double s = 0.0;
    MG_FOR_INTERIOR(g, x, y) {
        const long long o = mg_off(g, x, y);
        auto dir = [&](int xx, int yy) {
            return FIRST ? mg_at(g, z, xx, yy) : mg_at(g, z, xx, yy) + beta * mg_at(g, po, xx, yy);
        };
        const double pc = FIRST ? z[o] : z[o] + beta * po[o];
        const double qv = g.A * pc + g.xk * (dir(x - 1, y) + dir(x + 1, y)) + g.yk * (dir(x, y - 1) + dir(x, y + 1));
        p[o] = pc;
        q[o] = qv;
        s += pc * qv;
    }
    const double b = block_reduce<false>(s, lds);
    if (threadIdx.x == 0) *slot = b;
}
template <bool FIRST>
__global__ __launch_bounds__(kBlock) void k_mg_dir_apply(const Geom g, double beta, const double* __restrict__ z,
                                                         const double* __restrict__ po, double* __restrict__ p,
                                                         double* __restrict__ q, double* __restrict__ part) {
    mg_dir_apply<FIRST>(g, beta, z, po, p, q, part + blockIdx.x);
}

// x += alpha p, r -= alpha q; partials (field-major, part[f * gridDim.x + block]) of the MG_* fields.  u == nullptr: no error norms.
__global__ __launch_bounds__(kBlock) void k_mg_update(const Geom g, double alpha, double* __restrict__ x, double* __restrict__ r,
                                                      const double* __restrict__ p, const double* __restrict__ q,
                                                      const double* __restrict__ u, double* __restrict__ part) {
    __shared__ double lds[2 * kWaves];
    double rr = 0, d2 = 0, e2 = 0, rmax = 0, dmax = 0, emax = 0;
    MG_FOR_INTERIOR(g, xx, y) {
        const long long o = mg_off(g, xx, y);
        const double xo = x[o];
        const double xn = xo + alpha * p[o];                                // msg_solver.cpp:108-110
        const double rn = r[o] - alpha * q[o];                              // :113-115
        x[o] = xn;
        r[o] = rn;
        const double dx = xn - xo;                                          // :127-131
        rr += rn * rn; d2 += dx * dx;
        rmax = fmax(rmax, fabs(rn)); dmax = fmax(dmax, fabs(dx));
        if (u) { const double e = xn - u[o]; e2 += e * e; emax = fmax(emax, fabs(e)); }
    }
    const int n = gridDim.x, b = blockIdx.x;
    double t;
    t = block_reduce<false>(rr, lds); if (threadIdx.x == 0) part[MG_RR * n + b] = t;
    t = block_reduce<false>(d2, lds); if (threadIdx.x == 0) part[MG_D2 * n + b] = t;
    t = block_reduce<false>(e2, lds); if (threadIdx.x == 0) part[MG_E2 * n + b] = t;
    t = block_reduce<true>(rmax, lds); if (threadIdx.x == 0) part[MG_RMAX * n + b] = t;
    t = block_reduce<true>(dmax, lds); if (threadIdx.x == 0) part[MG_DMAX * n + b] = t;
    t = block_reduce<true>(emax, lds); if (threadIdx.x == 0) part[MG_EMAX * n + b] = t;
}

// partials of (a, b) over the interior
__device__ __forceinline__ void mg_dot(const Geom g, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ slot) {
    __shared__ double lds[2 * kWaves];
    double s = 0.0;
    MG_FOR_INTERIOR(g, x, y) { const long long o = mg_off(g, x, y); s += a[o] * b[o]; }
    const double t = block_reduce<false>(s, lds);
    if (threadIdx.x == 0) *slot = t;
}
__global__ __launch_bounds__(kBlock) void k_mg_dot(const Geom g, const double* __restrict__ a, const double* __restrict__ b,
                                                   double* __restrict__ part) { mg_dot(g, a, b, part + blockIdx.x); }

// partials of ||b - A x||^2 (REL_2NORM diagnostics: the true residual, matrix_free_system.cpp:457-463)
__global__ __launch_bounds__(kBlock) void k_mg_resid2(const Geom g, const double* __restrict__ b, const double* __restrict__ x,
                                                      double* __restrict__ part) {
    __shared__ double lds[2 * kWaves];
    double s = 0.0;
    MG_FOR_INTERIOR(g, xx, y) { const double d = b[mg_off(g, xx, y)] - mg_Av(g, x, xx, y); s += d * d; }
    const double t = block_reduce<false>(s, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

}  // namespace mi355cg
