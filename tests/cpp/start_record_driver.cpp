// The start records of csrc/item_table.h without a GPU: for every wave of a plan and both march directions the record must equal,
// field by field, what a wave worked out for itself before the records existed -- item_seq, decode_item and the wave-uniform part
// of item_addr, restated here from the tables' own definitions.  A program of its own, built with the sanitizers by
// tests/test_start_records_cpu.py; prints one line per plan and "FAIL ..." lines for what differs.
#include "../../iterative_solvers_amd/csrc/item_table.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace mi355cg;

// ---- the restatement ---------------------------------------------------------------------------------------------------
static ItemDesc ref_decode(const WorkList& wl, int item) {
    Panel P = wl.p[0];
    for (int k = 1; k < kMaxPanels; ++k) if (k < wl.np && item >= wl.p[k].item0) P = wl.p[k];
    const int local = item - P.item0;
    const int chunk = local / P.ns;
    ItemDesc it;
    it.strip = P.s0 + (local - chunk * P.ns);
    it.ya = P.y0 + chunk * P.ty;
    it.yb = std::min(P.y1, it.ya + P.ty - 1);
    it.gc = (it.strip == P.s0 ? (P.gc & 1) : 0) | (it.strip == P.s0 + P.ns - 1 ? (P.gc & 2) : 0);
    return it;
}
static ItemSeq ref_seq(const WorkList& wl, int block, int grid, int wave) {
    if (wl.ncls == kXcds) {
        const int cls = block % kXcds, nb = (grid - cls + kXcds - 1) / kXcds;
        return ItemSeq{wl.cls0[cls] + (block / kXcds) * kWaves + wave, nb * kWaves, wl.cls0[cls], wl.cls0[cls + 1]};
    }
    return ItemSeq{block * kWaves + wave, grid * kWaves, 0, wl.nitems};
}
// rows y <= half hold the columns from cb on in Pb elements, the rows above hold Pu elements
static long long ref_row_off(const Geom& g, int y) {
    long long off = -g.cb;
    for (int r = 0; r < y; ++r) off += (r < g.half ? g.Pb : (r == g.half ? g.Pb + g.cb : g.Pu));
    return off;
}
struct RefAddr { long long base_el; int so_first, so_c0, nrows, ystart, strip, bot, gc; };
static RefAddr ref_addr(const Geom& g, const ItemDesc& it, int elem, bool desc) {
    RefAddr A;
    const int y0 = it.ya - 1;
    A.nrows = it.yb - it.ya + 1;
    A.ystart = desc ? it.yb : it.ya;
    A.base_el = ref_row_off(g, y0) - g.base0;
    A.bot = it.ya <= g.half;
    A.so_first = desc ? (int)((ref_row_off(g, it.yb + 1) - ref_row_off(g, y0)) * elem) : 0;
    A.so_c0 = desc ? (int)((ref_row_off(g, it.yb) - ref_row_off(g, y0)) * elem) : (int)((ref_row_off(g, it.ya) - ref_row_off(g, y0)) * elem);
    A.strip = it.strip; A.gc = it.gc;
    return A;
}

// build_geom's layout of rows [y_lo, y_hi] of a grid of n intervals
static Geom geom(int n, int y_lo, int y_hi) {
    Geom g{};
    g.N = n; g.half = n / 2;
    g.Pu = (n + 1 + 31) / 32 * 32; g.cb = g.half & ~31; g.Pb = g.Pu - g.cb;
    g.y_lo = y_lo; g.y_hi = y_hi;
    g.base0 = row_off(g, y_lo - 1) + (y_lo - 1 <= g.half ? g.cb : 0);
    return g;
}
// rows [ya, yb] x all strips of `cols` columns (tests/cpp/item_table_driver.cpp: region)
static std::vector<Rect> region(int n, int ya, int yb, int cols) {
    const int half = n / 2, ns_all = (n - 1) / cols + 1, s0b = (half + 1) / cols;
    std::vector<Rect> out;
    if (ya <= half && yb >= 1) out.push_back(Rect{std::max(ya, 1), std::min(yb, half), s0b, ns_all, 0});
    if (yb > half) out.push_back(Rect{std::max(ya, half + 1), std::min(yb, n - 1), 0, ns_all, 0});
    return out;
}

static long long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail++ < 20) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } } while (0)

static void check_plan(const char* what, int n, const Geom& g, const Plan& pl, int elem) {
    const WorkList& wl = pl.wl;
    int idle = 0, several = 0, bottom = 0, upper = 0, corner = 0;
    for (int rev = 0; rev < 2; ++rev) {
        const std::vector<StartRec> t = build_start_table(wl, pl.grid, g, elem, rev != 0);
        CHECK((long long)t.size() == (long long)pl.grid * kWaves, "%s N=%d: %zu records for %d workgroups", what, n, t.size(), pl.grid);
        std::vector<int> first((size_t)std::max(0, wl.nitems), 0);
        for (int b = 0; b < pl.grid; ++b)
            for (int w = 0; w < kWaves; ++w) {
                const StartRec& r = t[(size_t)b * kWaves + w];
                const ItemSeq s = ref_seq(wl, b, pl.grid, w);
                CHECK(r.seq.first == s.first && r.seq.step == s.step && r.seq.begin == s.begin && r.seq.end == s.end, "%s N=%d rev=%d block %d wave %d: sequence differs from item_seq", what, n, rev, b, w);
                const bool have = s.first < s.end;
                CHECK(r.have == (have ? 1 : 0) && r.pad == 0, "%s N=%d rev=%d block %d wave %d: have = %d", what, n, rev, b, w, r.have);
                if (!have) {
                    const ItemUni z{};
                    CHECK(r.u.base_el == z.base_el && r.u.so_first == 0 && r.u.so_c0 == 0 && r.u.nrows == 0 && r.u.ystart == 0 && r.u.strip == 0 && r.u.bot == 0 && r.u.gc == 0,
                          "%s N=%d rev=%d block %d wave %d: a wave without an item has a non-zero record", what, n, rev, b, w);
                    if (!rev) ++idle;
                    continue;
                }
                const int item = rev ? s.end - 1 - (s.first - s.begin) : s.first;
                CHECK(item >= 0 && item < wl.nitems, "%s N=%d rev=%d block %d wave %d: first item %d of %d", what, n, rev, b, w, item, wl.nitems);
                if (item < 0 || item >= wl.nitems) continue;
                ++first[(size_t)item];
                const ItemDesc it = ref_decode(wl, item);
                const RefAddr A = ref_addr(g, it, elem, rev != 0);
                CHECK(r.u.base_el == A.base_el, "%s N=%d rev=%d item %d: base_el %lld, expected %lld", what, n, rev, item, r.u.base_el, A.base_el);
                CHECK(r.u.so_first == A.so_first && r.u.so_c0 == A.so_c0, "%s N=%d rev=%d item %d: so_first %d so_c0 %d, expected %d %d", what, n, rev, item, r.u.so_first, r.u.so_c0, A.so_first, A.so_c0);
                CHECK(r.u.nrows == A.nrows && r.u.ystart == A.ystart, "%s N=%d rev=%d item %d: nrows %d ystart %d, expected %d %d", what, n, rev, item, r.u.nrows, r.u.ystart, A.nrows, A.ystart);
                CHECK(r.u.strip == A.strip && r.u.bot == A.bot && r.u.gc == A.gc, "%s N=%d rev=%d item %d: strip %d bot %d gc %d, expected %d %d %d", what, n, rev, item, r.u.strip, r.u.bot, r.u.gc, A.strip, A.bot, A.gc);
                // the item lies inside the part, and so does the first stored element of its lowest halo row
                CHECK(A.base_el + (it.ya - 1 <= g.half ? g.cb : 0) >= 0 && A.nrows >= 1 && it.ya >= g.y_lo && it.yb <= g.y_hi, "%s N=%d rev=%d item %d: outside the part", what, n, rev, item);
                if (!rev) {
                    if (s.first + s.step < s.end) ++several;
                    if (it.yb <= g.half) ++bottom; else if (it.ya == g.half + 1) ++corner; else if (it.ya > g.half) ++upper;
                }
            }
        // no item is the first item of two waves
        for (int i = 0; i < wl.nitems; ++i) CHECK(first[(size_t)i] <= 1, "%s N=%d rev=%d item %d: first item of %d waves", what, n, rev, i, first[(size_t)i]);
    }
    std::printf("plan %s N=%d grid=%d items=%d ncls=%d ty=%d idle=%d several=%d bottom=%d upper=%d corner=%d\n", what, n, pl.grid, wl.nitems, wl.ncls, pl.ty, idle, several, bottom, upper, corner);
}

int main() {
    struct Case { const char* name; int n, blocks, item_rows, cols, elem, max_rows; };
    const Case cases[] = {
        {"default", 6, 512, 0, 128, 8, 800}, {"blocks1", 6, 1, 0, 128, 8, 800},
        {"default", 66, 512, 0, 128, 8, 800}, {"blocks1", 66, 1, 0, 128, 8, 800},
        {"blocks1rows2", 66, 1, 2, 128, 8, 800},
        {"blocks16", 258, 16, 0, 128, 8, 800},
        {"rows3", 1026, 512, 3, 128, 8, 800},
        {"fp32", 514, 512, 0, 256, 4, 64},
        {"default", 4096, 512, 0, 128, 8, 800},
    };
    for (const Case& c : cases) {
        PlanKnobs kn; kn.max_blocks = c.blocks; kn.item_rows = c.item_rows;
        const Geom g = geom(c.n, 1, c.n - 1);
        check_plan(c.name, c.n, g, make_plan(region(c.n, 1, c.n - 1, c.cols), kn, c.max_rows), c.elem);
    }
    // a row slab: base0 is not 0 (upper half of N = 258, 16 workgroups)
    {
        PlanKnobs kn; kn.max_blocks = 16;
        const int n = 258, ya = 130, yb = 257;
        check_plan("slab", n, geom(n, ya, yb), make_plan(region(n, ya, yb, 128), kn, 800), 8);
    }
    std::printf("%s %lld\n", g_fail ? "failed" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
