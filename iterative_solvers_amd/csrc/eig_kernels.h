// eig_kernels.h -- HIP kernels (gfx950 / CDNA4, wave64) of the block linear algebra between the V-cycles and operator applies of
// the block eigensolver (mi355cg_eigs*, mi355cg_block_gram, mi355cg_block_combine).
//
//   k_eig_gram      C[i][j] = sum over the interior of a_i * b_j for two groups of <= 48 vectors; partials per block
//   k_eig_reduce    the partials of an entry summed in block order (the ordered chain of k_mgb_reduce) into the matrix
//   k_eig_combine   Y_j = [Y0_j +] sum_i S_i * C[i][j], <= 48 inputs, <= 16 outputs, a fixed ascending-i sum
//   k_eig_resid     R_j = A X_j + theta_j X_j (= minus the eigen-residual K X_j - theta_j X_j, K = -A) for every column of the
//                   block in one launch, with the partials of ||R_j||^2 and ||X_j||^2
//
// A group of vectors is an EigList: vector i lives at base + idx[i] * stride in the pitched storage layout of mg_kernels.h, so a
// subset of a workspace (the active columns of a block) is a list and not a copy.  The lists travel as kernel arguments.
// blockIdx.x, gridDim.x are the single-system launch's (MgLevel::grid): the rows a block takes, and with them the order of every
// sum, depend on the grid alone.  Pads and boundary nodes hold 0 and no kernel here writes anything but interior nodes.
//
// k_eig_gram cuts the output into 4 x 4 tiles, one per blockIdx.y: a thread keeps the 16 accumulators of its tile and loads
// 4 + 4 values per node, so a vector of group A is read ceil(nb / 4) times and one of group B ceil(na / 4) times.  Per entry the
// order is mg_dot's: the thread's nodes in ascending order, the block tree, then the blocks left to right -- two launches give the
// same bits.  SYM (a product that is symmetric, S^T S or S^T (A S)): tiles below the diagonal are neither computed nor reduced;
// k_eig_reduce mirrors the tiles above it.
// Plain fp64 arithmetic (no FMA contraction: -ffp-contract=off), no atomics, no LDS beyond the block reduction, no scratch.
#pragma once
#include "mg_batch_kernels.h"

namespace mi355cg {

constexpr int kEigBlockMax = 16;                   // = MI355CG_EIG_BLOCK_MAX: columns of a block
constexpr int kEigBasisMax = 3 * kEigBlockMax;     // vectors of a Rayleigh-Ritz basis [X, W, P], and of a group of k_eig_gram
constexpr int kEigTile = 4;                        // k_eig_gram: the output tile is kEigTile x kEigTile
constexpr int kEigTileEntries = kEigTile * kEigTile;

struct EigList { long long stride; int n; int idx[kEigBasisMax]; };   // vector i at base + idx[i] * stride

__host__ __device__ inline int eig_tiles(int n) { return (n + kEigTile - 1) / kEigTile; }

// part[(tile * 16 + entry) * gridDim.x + block], tile = ti * tiles(nb) + tj, entry = 4 * (row in tile) + (column in tile).  Rows
// and columns past the end of a group read the group's last vector; k_eig_reduce drops what they give.
template <bool SYM>
__global__ __launch_bounds__(kBlock) void k_eig_gram(const Geom g, const EigList la, const double* __restrict__ a_, const EigList lb,
                                                     const double* __restrict__ b_, double* __restrict__ part) {
    __shared__ double lds[2 * kWaves];
    const int tjn = eig_tiles(lb.n);
    const int ti = (int)blockIdx.y / tjn, tj = (int)blockIdx.y % tjn;
    if (SYM && tj < ti) return;                                   // uniform per block
    const double* a[kEigTile];
    const double* b[kEigTile];
#pragma unroll
    for (int k = 0; k < kEigTile; ++k) {
        const int ia = ti * kEigTile + k, ib = tj * kEigTile + k;
        a[k] = a_ + (long long)la.idx[ia < la.n ? ia : la.n - 1] * la.stride;
        b[k] = b_ + (long long)lb.idx[ib < lb.n ? ib : lb.n - 1] * lb.stride;
    }
    double acc[kEigTileEntries];
#pragma unroll
    for (int e = 0; e < kEigTileEntries; ++e) acc[e] = 0.0;
    MG_FOR_INTERIOR(g, x, y) {
        const long long o = mg_off(g, x, y);
        double av[kEigTile], bv[kEigTile];
#pragma unroll
        for (int k = 0; k < kEigTile; ++k) { av[k] = a[k][o]; bv[k] = b[k][o]; }
#pragma unroll
        for (int e = 0; e < kEigTileEntries; ++e) acc[e] += av[e / kEigTile] * bv[e % kEigTile];
    }
    double* __restrict__ dst = part + (long long)blockIdx.y * kEigTileEntries * gridDim.x + blockIdx.x;
#pragma unroll
    for (int e = 0; e < kEigTileEntries; ++e) {
        const double t = block_reduce<false>(acc[e], lds);
        if (threadIdx.x == 0) dst[(long long)e * gridDim.x] = t;
    }
}

// c[i * nb + j] (row-major na x nb) = the nblocks partials of entry (i, j) summed serially in block order from 0; one wave per
// (entry, tile).  SYM (na == nb): a tile above the diagonal also fills its mirror image, tiles below it are not touched.
template <bool SYM>
__global__ __launch_bounds__(kWave) void k_eig_reduce(int na, int nb, int nblocks, const double* __restrict__ part, double* __restrict__ c) {
    const int e = blockIdx.x, tile = blockIdx.y, tjn = eig_tiles(nb);
    const int ti = tile / tjn, tj = tile % tjn;
    if (SYM && tj < ti) return;
    const int i = ti * kEigTile + e / kEigTile, j = tj * kEigTile + e % kEigTile;
    if (i >= na || j >= nb) return;
    const double s = mgb_chain<false>(part + ((long long)tile * kEigTileEntries + e) * nblocks, nblocks);
    if (threadIdx.x == 0) {
        c[(long long)i * nb + j] = s;
        if (SYM && tj > ti) c[(long long)j * nb + i] = s;
    }
}

// Y_j = sum_i S_i * coef[i * ldc + j] over i ascending, each step an unfused multiply and add; INIT: the sum starts from Y0_j
// instead of 0 (the projection W - X (X^T W) with the coefficients negated on the host).  A thread keeps the <= 16 outputs of
// its node in registers and reads every S_i once.  The outputs are buffers of their own: no input is overwritten.
template <bool INIT>
__global__ __launch_bounds__(kBlock) void k_eig_combine(const Geom g, const EigList ls, const double* __restrict__ s_,
                                                        const double* __restrict__ coef, int ldc, const EigList ly, double* __restrict__ y_,
                                                        const EigList l0, const double* __restrict__ y0_) {
    const int m = ly.n;
    MG_FOR_INTERIOR(g, x, y) {
        const long long o = mg_off(g, x, y);
        double acc[kEigBlockMax];
#pragma unroll
        for (int j = 0; j < kEigBlockMax; ++j) acc[j] = (INIT && j < m) ? y0_[(long long)l0.idx[j] * l0.stride + o] : 0.0;
        for (int i = 0; i < ls.n; ++i) {
            const double sv = s_[(long long)ls.idx[i] * ls.stride + o];
            const double* __restrict__ ci = coef + (long long)i * ldc;
#pragma unroll
            for (int j = 0; j < kEigBlockMax; ++j) {
                const double cv = j < m ? ci[j] : 0.0;
                acc[j] = acc[j] + sv * cv;
            }
        }
#pragma unroll
        for (int j = 0; j < kEigBlockMax; ++j) if (j < m) y_[(long long)ly.idx[j] * ly.stride + o] = acc[j];
    }
}

// Column blockIdx.y of the block: r = a x + theta x at the interior nodes; part[(column * 2 + field) * gridDim.x + block], field 0
// = (r, r), field 1 = (x, x) -- k_mgb_reduce's layout with two fields.  theta by column.
__global__ __launch_bounds__(kBlock) void k_eig_resid(const MgbScal theta, const Geom g, long long stride, const double* __restrict__ x_,
                                                      const double* __restrict__ ax_, double* __restrict__ r_, double* __restrict__ part) {
    __shared__ double lds[2 * kWaves];
    const long long so = (long long)blockIdx.y * stride;
    const double th = theta.v[blockIdx.y];
    const double* __restrict__ x = x_ + so;
    const double* __restrict__ ax = ax_ + so;
    double* __restrict__ r = r_ + so;
    double rr = 0, xx = 0;
    MG_FOR_INTERIOR(g, xi, y) {
        const long long o = mg_off(g, xi, y);
        const double xv = x[o];
        const double rv = ax[o] + th * xv;
        r[o] = rv;
        rr += rv * rv; xx += xv * xv;
    }
    const long long n = gridDim.x, base = (long long)blockIdx.y * 2 * n + blockIdx.x;
    double t;
    t = block_reduce<false>(rr, lds); if (threadIdx.x == 0) part[base] = t;
    t = block_reduce<false>(xx, lds); if (threadIdx.x == 0) part[base + n] = t;
}

#undef MG_FOR_INTERIOR

}  // namespace mi355cg
