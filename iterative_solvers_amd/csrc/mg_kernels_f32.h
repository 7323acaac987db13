// mg_kernels_f32.h -- HIP kernels (gfx950 / CDNA4, wave64) of the fp32 V-cycle inside the fp64 PCG
// (mi355cg_set_preconditioner_ex(h, kind, MI355CG_CYCLE_F32)).  z = M32 r for an fp64 r:
//   s = 2^e with max|r| = m 2^e, 0.5 <= m < 1;  r32 = fl32(r / s);  the V-cycle of mg_kernels.h on r32 with every vector,
//   constant and operation in fp32 (same expression order, no FMA contraction);  z = s * (double) z32.
// The scale makes M32(2^k r) = 2^k M32(r) bit for bit and keeps an fp32 cycle from over- or underflowing where fp64 does not.
//
//   k_mg32_smooth      one damped-Jacobi sweep.  MODE 0: the first of a cycle (u = 0), 1: the first of level 0, which reads the
//                      fp64 r and also writes r32, 2: any other, 3: the last of level 0, which recomputes r32 from the fp64 r,
//                      writes the fp64 z = s * t and the per-block partials of (r, z)
//   k_mg32_restrict    residual fused with full weighting            k_mg32_prolong     bilinear prolongation fused with u += P e
//   k_mg32_residual, k_mg32_restrict_nn, k_mg32_prolong_nn   the non-nested levels; the gather computes the ten 1-D weights of
//                      a coarse node once, outside the 5 x 5 loop
//   k_mg32_coarse      z = fl32(A_L^-1) r, multiplied and summed in fp32
//   k_mg32_cast, k_mg32_uncast_dot   r -> r32 and z32 -> z with the partials of (r, z): grids whose level 0 is the coarsest
//
// Layout and invariants are those of mg_kernels.h (boundary nodes and pads hold 0, only interior nodes get values, fixed
// reduction order).  Every row of a level starts at a multiple of 32 elements (Pb, Pu and cb are multiples of 32), so a run
// of V = 4 columns that starts at a multiple of 4 is a 16-byte aligned float4, and it lies either wholly inside or wholly outside
// a row's storage.  The sweeps, the nested transfers and the residual take V columns per lane: V = 4 on the large levels, V = 1
// (the scalar path, lane for lane the loop of mg_kernels.h) on the small ones.  A run may hang over a row's interior on either
// side; those lanes' columns are boundary nodes or pads, get 0 written back (what they hold) and are left out of every sum.
#pragma once
#include "mg_kernels.h"

namespace mi355cg {

struct MgCoef32 { float A, xk, yk, omega; };      // the level's fp64 constants rounded to fp32

// block b takes interior rows 1 + b, 1 + b + gridDim.x, ...; its lanes stride runs of V columns, the first run aligned down
#define MG32_FOR_RUNS(G, V, X0, YI)                                                                \
    for (int YI = 1 + (int)blockIdx.x; YI <= (G).N - 1; YI += (int)gridDim.x)                      \
        for (int X0 = (mg_x0((G), YI) / (V)) * (V) + (int)threadIdx.x * (V); X0 <= (G).N - 1; X0 += kBlock * (V))

// node (x, y), any x: 0 outside the stored part of the row (left of the bottom block's storage, x < 0, x > N)
__device__ inline float mg32_at(const Geom& g, const float* __restrict__ v, int x, int y) {
    return (x < 0 || x > g.N || (y <= g.half && x < g.cb)) ? 0.0f : v[mg_off(g, x, y)];
}
// V aligned columns x0 .. x0 + V - 1 of row y (x0 >= 0, x0 % V == 0, x0 < Pu): 0 where the row is not stored
template <int V>
__device__ inline void mg32_run(const Geom& g, const float* __restrict__ v, int x0, int y, float* o) {
    const bool stored = !(y <= g.half && x0 < g.cb);
    if (V == 4) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (stored) t = *reinterpret_cast<const float4*>(v + mg_off(g, x0, y));
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else {
        for (int k = 0; k < V; ++k) o[k] = stored ? v[mg_off(g, x0 + k, y)] : 0.0f;
    }
}
template <int V>
__device__ inline void mg32_store(float* __restrict__ p, const float* v) {
    if (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else for (int k = 0; k < V; ++k) p[k] = v[k];
}
// the same for an fp64 vector (the run is always stored: only called on a row's own interior runs)
template <int V>
__device__ inline void mg32_run64(const double* __restrict__ p, double* o) {
    if (V == 4) {
        const double2 a = *reinterpret_cast<const double2*>(p), b = *reinterpret_cast<const double2*>(p + 2);
        o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
    } else {
        for (int k = 0; k < V; ++k) o[k] = p[k];
    }
}
template <int V>
__device__ inline void mg32_store64(double* __restrict__ p, const double* v) {
    if (V == 4) {
        *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]);
        *reinterpret_cast<double2*>(p + 2) = make_double2(v[2], v[3]);
    } else {
        for (int k = 0; k < V; ++k) p[k] = v[k];
    }
}
// (A u) at columns x0 .. x0 + V - 1 of row y: the 5-point formula of mg_Av in fp32
template <int V>
__device__ inline void mg32_Av(const Geom& g, const MgCoef32& c, const float* __restrict__ u, int x0, int y, const float* uc, float* av) {
    float ud[V], uu[V];
    mg32_run<V>(g, u, x0, y - 1, ud);
    mg32_run<V>(g, u, x0, y + 1, uu);
    const float ul = mg32_at(g, u, x0 - 1, y), ur = mg32_at(g, u, x0 + V, y);
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const float l = k == 0 ? ul : uc[k - 1], r = k == V - 1 ? ur : uc[k + 1];
        av[k] = c.A * uc[k] + c.xk * (l + r) + c.yk * (ud[k] + uu[k]);
    }
}

template <int V, int MODE>
__global__ __launch_bounds__(kBlock) void k_mg32_smooth(const Geom g, const MgCoef32 c, int e, const double* __restrict__ r64,
                                                        const float* __restrict__ r32, float* __restrict__ r32_out,
                                                        const float* __restrict__ u, float* __restrict__ t,
                                                        double* __restrict__ z64, double* __restrict__ part) {
    __shared__ double lds[2 * kWaves];
    double s = 0.0;
    MG32_FOR_RUNS(g, V, x0, y) {
        const long long o = mg_off(g, x0, y);
        const int xf = mg_x0(g, y);
        float rv[V], tv[V];
        double rd[V];
        if (MODE == 1 || MODE == 3) {
            mg32_run64<V>(r64 + o, rd);
#pragma unroll
            for (int k = 0; k < V; ++k) {                                // off the interior r32 is 0, whatever r's pads hold
                if (x0 + k < xf || x0 + k > g.N - 1) rd[k] = 0.0;
                rv[k] = (float)ldexp(rd[k], -e);
            }
            if (MODE == 1) mg32_store<V>(r32_out + o, rv);
        } else {
            mg32_run<V>(g, r32, x0, y, rv);
        }
        if (MODE <= 1) {
#pragma unroll
            for (int k = 0; k < V; ++k) tv[k] = c.omega * (rv[k] / c.A);
        } else {
            float uc[V], av[V];
            mg32_run<V>(g, u, x0, y, uc);
            mg32_Av<V>(g, c, u, x0, y, uc, av);
#pragma unroll
            for (int k = 0; k < V; ++k) tv[k] = uc[k] + c.omega * ((rv[k] - av[k]) / c.A);
        }
#pragma unroll
        for (int k = 0; k < V; ++k) if (x0 + k < xf || x0 + k > g.N - 1) tv[k] = 0.0f;
        if (MODE == 3) {
            double zv[V];
#pragma unroll
            for (int k = 0; k < V; ++k) { zv[k] = ldexp((double)tv[k], e); s += rd[k] * zv[k]; }
            mg32_store64<V>(z64 + o, zv);
        } else {
            mg32_store<V>(t + o, tv);
        }
    }
    if (MODE == 3) {
        const double b = block_reduce<false>(s, lds);
        if (threadIdx.x == 0) part[blockIdx.x] = b;
    }
}

// s = r - A u at fine interior nodes (the level's work vector); the other columns of a run get the 0 they hold
template <int V>
__global__ __launch_bounds__(kBlock) void k_mg32_residual(const Geom g, const MgCoef32 c, const float* __restrict__ r,
                                                          const float* __restrict__ u, float* __restrict__ s) {
    MG32_FOR_RUNS(g, V, x0, y) {
        const int xf = mg_x0(g, y);
        float rv[V], uc[V], av[V], sv[V];
        mg32_run<V>(g, r, x0, y, rv);
        mg32_run<V>(g, u, x0, y, uc);
        mg32_Av<V>(g, c, u, x0, y, uc, av);
#pragma unroll
        for (int k = 0; k < V; ++k) sv[k] = (x0 + k < xf || x0 + k > g.N - 1) ? 0.0f : rv[k] - av[k];
        mg32_store<V>(s + mg_off(g, x0, y), sv);
    }
}

// columns xs .. xs + 2 V + 2 of row y, xs = 2 X0 - 2: two scalars, 2 V aligned columns, one scalar
template <int V>
__device__ inline void mg32_seg(const Geom& g, const float* __restrict__ v, int xs, int y, float* o) {
    o[0] = mg32_at(g, v, xs, y);
    o[1] = mg32_at(g, v, xs + 1, y);
    if (V == 4) {
        mg32_run<4>(g, v, xs + 2, y, o + 2);
        mg32_run<4>(g, v, xs + 6, y, o + 6);
    } else {
        for (int k = 0; k < 2 * V; ++k) o[2 + k] = mg32_at(g, v, xs + 2 + k, y);
    }
    o[2 * V + 2] = mg32_at(g, v, xs + 2 * V + 2, y);
}

// coarse interior nodes X0 .. X0 + V - 1 of row Y <- full weighting of s = r - A u around the fine nodes (2 X, 2 Y); s = 0 off
// the fine interior.  A lane holds the five fine rows 2 Y - 2 .. 2 Y + 2 of u over columns 2 X0 - 2 .. 2 X0 + 2 V.
template <int V>
__global__ __launch_bounds__(kBlock) void k_mg32_restrict(const Geom gf, const Geom gc, const MgCoef32 c, const float* __restrict__ r,
                                                          const float* __restrict__ u, float* __restrict__ rc) {
    constexpr int W = 2 * V + 3;
    MG32_FOR_RUNS(gc, V, X0, Y) {
        const int xs = 2 * X0 - 2, Xf = mg_x0(gc, Y);
        float res[3][W];                                   // res[j][i]: s at fine node (xs + i, 2 Y - 1 + j), i = 1 .. 2 V + 1
        float ua[W], ub[W], uc[W];
        mg32_seg<V>(gf, u, xs, 2 * Y - 2, ua);
        mg32_seg<V>(gf, u, xs, 2 * Y - 1, ub);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int y = 2 * Y - 1 + j;
            float rr[W];
            mg32_seg<V>(gf, u, xs, y + 1, uc);
            mg32_seg<V>(gf, r, xs, y, rr);
#pragma unroll
            for (int i = 1; i <= 2 * V + 1; ++i) {
                const float av = c.A * ub[i] + c.xk * (ub[i - 1] + ub[i + 1]) + c.yk * (ua[i] + uc[i]);
                res[j][i] = node_interior(gf, xs + i, y) ? rr[i] - av : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < W; ++i) { ua[i] = ub[i]; ub[i] = uc[i]; }
        }
        float out[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int i = 2 * k + 2;                       // fine column 2 (X0 + k)
            const float s00 = res[1][i], sl = res[1][i - 1], sr = res[1][i + 1], sd = res[0][i], su = res[2][i];
            const float sld = res[0][i - 1], srd = res[0][i + 1], slu = res[2][i - 1], sru = res[2][i + 1];
            const float v = 0.0625f * (4.0f * s00 + 2.0f * (sl + sr + sd + su) + (sld + srd + slu + sru));
            out[k] = (X0 + k < Xf || X0 + k > gc.N - 1) ? 0.0f : v;
        }
        mg32_store<V>(rc + mg_off(gc, X0, Y), out);
    }
}

// fine interior nodes x0 .. x0 + V - 1 of row y: u += bilinear interpolation of the coarse correction e
template <int V>
__global__ __launch_bounds__(kBlock) void k_mg32_prolong(const Geom gf, const Geom gc, const float* __restrict__ e, float* __restrict__ u) {
    constexpr int NC = (V + 1) / 2 + 1;                    // coarse columns x0 / 2 .. x0 / 2 + NC - 1 cover the run
    MG32_FOR_RUNS(gf, V, x0, y) {
        const int xf = mg_x0(gf, y), cx0 = x0 >> 1, cy = y >> 1;
        float e0[NC], e1[NC], uv[V];
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            e0[k] = mg32_at(gc, e, cx0 + k, cy);
            e1[k] = (y & 1) ? mg32_at(gc, e, cx0 + k, cy + 1) : 0.0f;
        }
        const long long o = mg_off(gf, x0, y);
        mg32_run<V>(gf, u, x0, y, uv);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int x = x0 + k, j = k >> 1;                   // = (x >> 1) - cx0: x0 is even when V > 1
            float corr;
            if ((x & 1) && (y & 1)) corr = 0.25f * (e0[j] + e0[j + 1] + e1[j] + e1[j + 1]);
            else if (x & 1) corr = 0.5f * (e0[j] + e0[j + 1]);
            else if (y & 1) corr = 0.5f * (e0[j] + e1[j]);
            else corr = e0[j];
            uv[k] = (x < xf || x > gf.N - 1) ? 0.0f : uv[k] + corr;
        }
        mg32_store<V>(u + o, uv);
    }
}

// ---- non-nested levels --------------------------------------------------------------------------------------------------------
// mg_w in fp32: the exact integer numerator over N_f.  Both are below 2^24 and the quotient is rounded once, which is the fp64
// weight rounded to fp32 (a 53-bit quotient rounded again to 24 bits rounds as the exact quotient does).
__device__ inline float mg32_w(int x, int X, int Nf, int Nc) {
    long long d = (long long)x * Nc - (long long)X * Nf;
    if (d < 0) d = -d;
    return d < Nf ? (float)(int)(Nf - d) / (float)Nf : 0.0f;
}

// k_mg_restrict_nn with the <= 5 + 5 weights of the coarse node computed before the double loop (same products, same order)
__global__ __launch_bounds__(kBlock) void k_mg32_restrict_nn(const Geom gf, const Geom gc, float scale, const float* __restrict__ s,
                                                             float* __restrict__ rc) {
    const int Nf = gf.N, Nc = gc.N;
    for (int Y = 1 + (int)blockIdx.x; Y <= Nc - 1; Y += (int)gridDim.x) {
        const int y_lo = (int)((long long)(Y - 1) * Nf / Nc) + 1, y_hi = (int)(((long long)(Y + 1) * Nf - 1) / Nc);
        float wy[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) wy[j] = mg32_w(y_lo + j, Y, Nf, Nc);
        for (int X = mg_x0(gc, Y) + (int)threadIdx.x; X <= Nc - 1; X += kBlock) {
            const int x_lo = (int)((long long)(X - 1) * Nf / Nc) + 1, x_hi = (int)(((long long)(X + 1) * Nf - 1) / Nc);
            float wx[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) wx[i] = mg32_w(x_lo + i, X, Nf, Nc);
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                if (y_lo + j > y_hi) break;
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    if (x_lo + i > x_hi) break;
                    acc += (wy[j] * wx[i]) * mg32_at(gf, s, x_lo + i, y_lo + j);
                }
            }
            rc[mg_off(gc, X, Y)] = scale * acc;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_mg32_prolong_nn(const Geom gf, const Geom gc, const float* __restrict__ e,
                                                            float* __restrict__ u) {
    const int Nf = gf.N, Nc = gc.N;
    MG32_FOR_RUNS(gf, 1, x, y) {
        const int X0 = (int)((long long)x * Nc / Nf), Y0 = (int)((long long)y * Nc / Nf);
        const float wx0 = mg32_w(x, X0, Nf, Nc), wx1 = mg32_w(x, X0 + 1, Nf, Nc);
        const float wy0 = mg32_w(y, Y0, Nf, Nc), wy1 = mg32_w(y, Y0 + 1, Nf, Nc);
        const float corr = wy0 * (wx0 * mg32_at(gc, e, X0, Y0) + wx1 * mg32_at(gc, e, X0 + 1, Y0)) +
                           wy1 * (wx0 * mg32_at(gc, e, X0, Y0 + 1) + wx1 * mg32_at(gc, e, X0 + 1, Y0 + 1));
        const long long o = mg_off(gf, x, y);
        u[o] = u[o] + corr;
    }
}

// ---- coarsest level -------------------------------------------------------------------------------------------------------------
__device__ inline float block_reduce_f32(float v, float* lds /* >= kWaves floats */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    __syncthreads();
    if (lane == 0) lds[w] = v;
    __syncthreads();
    float t = lds[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) t = t + lds[k];
    return t;
}

__global__ __launch_bounds__(kBlock) void k_mg32_coarse(int n, const float* __restrict__ inv, const int* __restrict__ off,
                                                        const float* __restrict__ r, float* __restrict__ z) {
    __shared__ float lds[kWaves];
    for (int i = blockIdx.x; i < n; i += gridDim.x) {                 // uniform per block: every thread reaches the reduction
        float s = 0.0f;
        for (int j = threadIdx.x; j < n; j += kBlock) s += inv[(long long)i * n + j] * r[off[j]];
        const float t = block_reduce_f32(s, lds);
        if (threadIdx.x == 0) z[off[i]] = t;
    }
}

// one-level grids: r32 = fl32(r / 2^e), and z = 2^e z32 with the partials of (r, z)
__global__ __launch_bounds__(kBlock) void k_mg32_cast(const Geom g, int e, const double* __restrict__ r, float* __restrict__ r32) {
    MG32_FOR_RUNS(g, 1, x, y) { const long long o = mg_off(g, x, y); r32[o] = (float)ldexp(r[o], -e); }
}
__global__ __launch_bounds__(kBlock) void k_mg32_uncast_dot(const Geom g, int e, const double* __restrict__ r, const float* __restrict__ z32,
                                                            double* __restrict__ z, double* __restrict__ part) {
    __shared__ double lds[2 * kWaves];
    double s = 0.0;
    MG32_FOR_RUNS(g, 1, x, y) {
        const long long o = mg_off(g, x, y);
        const double zv = ldexp((double)z32[o], e);
        z[o] = zv;
        s += r[o] * zv;
    }
    const double b = block_reduce<false>(s, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = b;
}

#undef MG32_FOR_RUNS

}  // namespace mi355cg
