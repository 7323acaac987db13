// onchip_plan_driver.cpp -- csrc/onchip_plan.h on the host, under the sanitizers (tests/test_onchip_plan_cpu.py).
//
// For every even N from 6 to kOnchipMaxN the ownership of the on-chip solve is restated from node_interior alone -- interior nodes in
// row-major order, dealt to the threads round-robin -- and compared with what the plan's functions say:
//   every interior node is owned by exactly one (thread, slot), no other node is owned; the four neighbours of an owned cell lie in the
//   image; a neighbour that is not interior is a cell no thread owns (the halo stays zero); lds_bytes <= 160 KiB, threads <= 1024 and
//   a multiple of 64, threads x elems >= the unknown count; a thread's valid slots are a prefix.
// Prints "N=<n> threads=<t> lds=<bytes> elems=<e> unknowns=<u>" per size, "FAIL ..." per violation and "ok <failures>" at the end.
#include "../../iterative_solvers_amd/csrc/onchip_plan.h"

#include <cstdio>
#include <vector>

using namespace mi355cg;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

int main() {
    for (int n = 6; n <= kOnchipMaxN; n += 2) {
        CHECK(onchip_supported(n), "N=%d not supported", n);
        const OnchipPlan pl = onchip_plan(n);
        Geom g{};
        g.N = n; g.half = n / 2;                                    // all node_interior reads

        // the restated ownership: interior nodes in row-major order (y, then x), node k to thread k % T, slot k / T
        std::vector<int> want_thread((size_t)(n + 1) * (n + 1), -1), want_slot((size_t)(n + 1) * (n + 1), -1);
        int unknowns = 0;
        for (int y = 0; y <= n; ++y)
            for (int x = 0; x <= n; ++x)
                if (node_interior(g, x, y)) {
                    want_thread[(size_t)y * (n + 1) + x] = unknowns % pl.threads;
                    want_slot[(size_t)y * (n + 1) + x] = unknowns / pl.threads;
                    ++unknowns;
                }
        CHECK(unknowns == (n / 2 - 1) * (3 * n / 2 - 1), "N=%d: %d interior nodes", n, unknowns);
        CHECK(pl.unknowns == unknowns, "N=%d: plan says %d unknowns, the grid has %d", n, pl.unknowns, unknowns);
        CHECK(pl.threads >= 64 && pl.threads <= 1024 && pl.threads % 64 == 0, "N=%d: %d threads", n, pl.threads);
        CHECK(pl.threads <= kOnchipMaxThreads, "N=%d: %d threads above the kernel's launch bound", n, pl.threads);
        CHECK(pl.elems >= 1 && pl.elems <= kOnchipMaxElems, "N=%d: %d slots per thread", n, pl.elems);
        CHECK((long long)pl.threads * pl.elems >= unknowns, "N=%d: %d x %d slots for %d unknowns", n, pl.threads, pl.elems, unknowns);
        CHECK(pl.lds_bytes <= 160 * 1024 && pl.lds_bytes >= pl.cells * 8, "N=%d: %d bytes of LDS", n, pl.lds_bytes);
        CHECK(pl.pitch == n + 1 && pl.cells == (n + 1) * (n + 1) && pl.cells <= kOnchipMaxCells, "N=%d: image %d x %d", n, pl.pitch, pl.cells);

        // what the plan says: who owns which cell
        std::vector<int> owners((size_t)pl.cells, 0);
        for (int t = 0; t < pl.threads; ++t) {
            bool ended = false;
            for (int k = 0; k < pl.elems; ++k) {
                const int i = onchip_owned(pl, t, k);
                if (i < 0) { ended = true; continue; }
                CHECK(!ended, "N=%d thread %d: slot %d is valid behind an empty one", n, t, k);
                CHECK(i < unknowns, "N=%d thread %d slot %d: unknown %d", n, t, k, i);
                int x = -1, y = -1;
                onchip_node(pl, i, &x, &y);
                CHECK(x >= 0 && x <= n && y >= 0 && y <= n, "N=%d thread %d slot %d: node (%d, %d)", n, t, k, x, y);
                if (x < 0 || x > n || y < 0 || y > n) continue;
                CHECK(node_interior(g, x, y), "N=%d thread %d slot %d: owns the exterior node (%d, %d)", n, t, k, x, y);
                const int c = onchip_cell(pl, x, y);
                CHECK(c == y * (n + 1) + x, "N=%d: cell of (%d, %d) is %d", n, x, y, c);
                CHECK(want_thread[(size_t)c] == t && want_slot[(size_t)c] == k, "N=%d node (%d, %d): owned by (%d, %d), restated (%d, %d)", n, x, y,
                      t, k, want_thread[(size_t)c], want_slot[(size_t)c]);
                ++owners[(size_t)c];
            }
        }
        for (int y = 0; y <= n; ++y)
            for (int x = 0; x <= n; ++x) {
                const int c = y * (n + 1) + x;
                CHECK(owners[(size_t)c] == (node_interior(g, x, y) ? 1 : 0), "N=%d node (%d, %d): %d owners", n, x, y, owners[(size_t)c]);
            }
        // neighbours: inside the image; the neighbour cell is the neighbour node; not interior -> owned by nobody
        const int dx[4] = {-1, 1, 0, 0}, dy[4] = {0, 0, 1, -1};
        for (int y = 0; y <= n; ++y)
            for (int x = 0; x <= n; ++x) {
                if (!node_interior(g, x, y)) continue;
                int nb[4];
                onchip_neighbours(pl, onchip_cell(pl, x, y), nb);
                for (int d = 0; d < 4; ++d) {
                    CHECK(nb[d] >= 0 && nb[d] < pl.cells, "N=%d node (%d, %d): neighbour %d at cell %d outside the image", n, x, y, d, nb[d]);
                    if (nb[d] < 0 || nb[d] >= pl.cells) continue;
                    const int xn = x + dx[d], yn = y + dy[d];
                    CHECK(nb[d] == yn * (n + 1) + xn, "N=%d node (%d, %d): neighbour %d is cell %d", n, x, y, d, nb[d]);
                    if (!node_interior(g, xn, yn)) CHECK(owners[(size_t)nb[d]] == 0, "N=%d: halo cell %d has an owner", n, nb[d]);
                }
            }
        std::printf("N=%d threads=%d lds=%d elems=%d unknowns=%d\n", n, pl.threads, pl.lds_bytes, pl.elems, unknowns);
    }
    for (int n : {7, 4, 0, -2, kOnchipMaxN + 1, kOnchipMaxN + 2}) CHECK(!onchip_supported(n), "N=%d supported", n);
    std::printf("cap %d\n", kOnchipMaxN);
    std::printf("ok %d\n", failures);
    return failures ? 1 : 0;
}
