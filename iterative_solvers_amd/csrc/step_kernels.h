// step_kernels.h -- HIP kernel (gfx950 / CDNA4, wave64) of the device-resident theta-scheme stepper (mi355cg_time_steps;
// DESIGN section 10.6).
//
//   k_step_rhs   the right-hand side of one step of u_t = A u - g,
//                    b = g / theta - sigma u - ((1 - theta) / theta) A u,        sigma = 1 / (theta tau),
//                in one pass over u and g in the pitched storage layout of cg_kernels.h.  STENCIL = true (theta < 1) forms the
//                5-point A u of the UNSHIFTED operator itself; STENCIL = false (theta = 1: b = g - sigma u) reads no neighbour:
//                u, g and b once each, 24 B per unknown.
//
// One tile = one row x 512 columns; one thread = one aligned pair of columns (a 16-byte access per stream).  Only interior nodes are
// written, so the pads and the boundary nodes of b keep the zeros they were allocated with.  Rows y <= N/2 store columns from cb
// on (the pitch changes at y = N/2 + 1); the only node a stencil can name that is not stored is (x, N/2) with x < cb, which is
// boundary or exterior: 0.  Plain fp64 arithmetic (no FMA contraction: -ffp-contract=off).
#pragma once
#include "cg_kernels.h"

namespace mi355cg {

constexpr int kStepTileCols = 2 * kBlock;

struct StepRhsArgs {
    Geom g;                     // the handle's layout; its A is not used (it carries the shift)
    double A0, xk, yk;          // the Laplacian's coefficients
    double sigma, theta, c1;            // c1 = (1 - theta) / theta
    const double* u;
    const double* rhs;
    double* out;
    int tiles_per_row;
    long long tiles;
};

template <bool STENCIL>
__global__ __launch_bounds__(kBlock) void k_step_rhs(const StepRhsArgs a) {
    typedef VecOf<double, 2>::type vec_t;
    const Geom& g = a.g;
    for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int y = 1 + (int)(tile / a.tiles_per_row), seg = (int)(tile % a.tiles_per_row);
        const bool bottom = y <= g.half;
        const int x = (bottom ? g.cb : 0) + seg * kStepTileCols + 2 * (int)threadIdx.x;      // even: cb is a multiple of 32
        const int xi = bottom ? g.half + 1 : 1;                                                // first interior column of the row
        const bool in0 = x >= xi && x <= g.N - 1, in1 = x + 1 >= xi && x + 1 <= g.N - 1;
        if (!in0 && !in1) continue;
        const long long o = row_off(g, y) - g.base0 + x;
        const vec_t uc = *reinterpret_cast<const vec_t*>(a.u + o);
        const vec_t gv = *reinterpret_cast<const vec_t*>(a.rhs + o);
        double b0 = (STENCIL ? gv[0] / a.theta : gv[0]) - a.sigma * uc[0];        // theta = 1: g / theta is g
        double b1 = (STENCIL ? gv[1] / a.theta : gv[1]) - a.sigma * uc[1];
        if (STENCIL) {
            vec_t dn = {0.0, 0.0};
            if (!(y - 1 <= g.half && x < g.cb)) dn = *reinterpret_cast<const vec_t*>(a.u + (row_off(g, y - 1) - g.base0 + x));
            const vec_t up = *reinterpret_cast<const vec_t*>(a.u + (row_off(g, y + 1) - g.base0 + x));
            const double left = in0 ? a.u[o - 1] : 0.0, right = in1 ? a.u[o + 2] : 0.0;
            const double au0 = a.A0 * uc[0] + a.xk * (left + uc[1]) + a.yk * (dn[0] + up[0]);
            const double au1 = a.A0 * uc[1] + a.xk * (uc[0] + right) + a.yk * (dn[1] + up[1]);
            b0 = b0 - a.c1 * au0;
            b1 = b1 - a.c1 * au1;
        }
        if (in0 && in1) { vec_t bv = {b0, b1}; *reinterpret_cast<vec_t*>(a.out + o) = bv; }
        else if (in0) a.out[o] = b0;
        else a.out[o + 1] = b1;
    }
}

}  // namespace mi355cg
