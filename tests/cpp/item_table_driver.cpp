// csrc/item_table.h without a GPU: the two tables of every plan against the arithmetic the kernels did for themselves before the
// tables existed (decode_item's panel search and division, item_seq's class ranges), restated here.  A program of its own, built
// with the sanitizers by tests/test_item_table_cpu.py; prints one line per group of cases and "FAIL ..." lines for what differs.
#include "../../iterative_solvers_amd/csrc/item_table.h"

#include <cstdio>
#include <cstdlib>
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
        int begin = wl.cls0[0], end = wl.cls0[1];
        for (int k = 1; k < kXcds; ++k) if (k == cls) { begin = wl.cls0[k]; end = wl.cls0[k + 1]; }
        return ItemSeq{begin + (block / kXcds) * kWaves + wave, nb * kWaves, begin, end};
    }
    return ItemSeq{block * kWaves + wave, grid * kWaves, 0, wl.nitems};
}

// ---- the rectangles of a part: rows [ya, yb] x 128-column strips [sa, sb) of the L-shaped grid (rows <= N/2 only hold the columns
// right of N/2), with the ghost-column flags of a part that has neighbours in x
static int strips_total(int n) { return (n - 1) / 128 + 1; }
static std::vector<Rect> region(int n, int ya, int yb, int sa, int sb) {
    const int half = n / 2, ns_all = strips_total(n), s0b = (half + 1) / 128;
    std::vector<Rect> out;
    sb = std::min(sb, ns_all);
    if (ya <= half && yb >= 1) {
        const int s0 = std::max(sa, s0b);
        if (s0 < sb) out.push_back(Rect{std::max(ya, 1), std::min(yb, half), s0, sb, (sa > s0b ? 1 : 0) | (sb < ns_all ? 2 : 0)});
    }
    if (yb > half && sa < sb) out.push_back(Rect{std::max(ya, half + 1), std::min(yb, n - 1), sa, sb, (sa > 0 ? 1 : 0) | (sb < ns_all ? 2 : 0)});
    return out;
}

static long long g_fail = 0, g_plans = 0, g_items = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail++ < 20) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } } while (0)

static bool same(const ItemDesc& a, const ItemDesc& b) { return a.strip == b.strip && a.ya == b.ya && a.yb == b.yb && a.gc == b.gc; }
static bool same(const ItemSeq& a, const ItemSeq& b) { return a.first == b.first && a.step == b.step && a.begin == b.begin && a.end == b.end; }

static void check_plan(const char* what, int n, const std::vector<Rect>& rects, const Plan& pl) {
    ++g_plans;
    const WorkList& wl = pl.wl;
    long long owned = 0;
    for (auto& r : rects) owned += (long long)std::max(0, r.y1 - r.y0 + 1) * std::max(0, r.s1 - r.s0);
    if (owned == 0) { CHECK(wl.nitems == 0 && pl.grid == 0, "%s N=%d: an empty part has items", what, n); return; }
    CHECK(wl.nitems > 0 && pl.grid > 0, "%s N=%d: no items", what, n);
    const std::vector<ItemDesc> items = build_item_table(wl);
    const std::vector<ItemSeq> seq = build_seq_table(wl, pl.grid);
    CHECK((int)items.size() == wl.nitems, "%s N=%d: %zu entries for %d items", what, n, items.size(), wl.nitems);
    CHECK((long long)seq.size() == (long long)pl.grid * kWaves, "%s N=%d: %zu sequences for %d workgroups", what, n, seq.size(), pl.grid);
    // 1. every entry equals the restatement
    for (int i = 0; i < wl.nitems; ++i) CHECK(same(items[i], ref_decode(wl, i)), "%s N=%d item %d: table differs from decode_item", what, n, i);
    g_items += wl.nitems;
    // 2. every wave's sequence equals the restatement; 3. together they visit every item exactly once
    std::vector<unsigned char> visits((size_t)wl.nitems, 0);
    for (int b = 0; b < pl.grid; ++b)
        for (int w = 0; w < kWaves; ++w) {
            const ItemSeq s = seq[(size_t)b * kWaves + w];
            CHECK(same(s, ref_seq(wl, b, pl.grid, w)), "%s N=%d block %d wave %d: sequence differs from item_seq", what, n, b, w);
            CHECK(s.step > 0 && s.begin >= 0 && s.end <= wl.nitems && s.first >= s.begin, "%s N=%d block %d wave %d: sequence out of range", what, n, b, w);
            if (s.step <= 0 || s.first < 0) continue;
            for (int i = s.first; i < s.end && i < wl.nitems; i += s.step) if (visits[i] < 255) ++visits[i];
        }
    for (int i = 0; i < wl.nitems; ++i) CHECK(visits[i] == 1, "%s N=%d item %d: visited %d times", what, n, i, (int)visits[i]);
    // 4. every owned (row, strip) lies in exactly one item
    const int ns_all = strips_total(n);
    std::vector<unsigned char> cover((size_t)(n + 1) * ns_all, 0);
    long long covered = 0;
    for (const ItemDesc& it : items) {
        CHECK(it.ya >= 1 && it.yb <= n - 1 && it.ya <= it.yb && it.strip >= 0 && it.strip < ns_all, "%s N=%d: item outside the grid", what, n);
        if (it.ya < 0 || it.yb > n || it.strip < 0 || it.strip >= ns_all) continue;
        for (int y = it.ya; y <= it.yb; ++y) { ++cover[(size_t)y * ns_all + it.strip]; ++covered; }
    }
    CHECK(covered == owned, "%s N=%d: items cover %lld (row, strip) pairs, the part owns %lld", what, n, covered, owned);
    for (auto& r : rects)
        for (int y = r.y0; y <= r.y1; ++y)
            for (int s = r.s0; s < r.s1; ++s) CHECK(cover[(size_t)y * ns_all + s] == 1, "%s N=%d: row %d strip %d in %d items", what, n, y, s, (int)cover[(size_t)y * ns_all + s]);
    // the ghost-column flags: only on the first / last strip of a rectangle that has them
    for (const ItemDesc& it : items) {
        int want = 0;
        for (auto& r : rects) if (it.ya >= r.y0 && it.yb <= r.y1 && it.strip >= r.s0 && it.strip < r.s1)
            want = (it.strip == r.s0 ? (r.gc & 1) : 0) | (it.strip == r.s1 - 1 ? (r.gc & 2) : 0);
        CHECK(it.gc == want, "%s N=%d strip %d rows %d..%d: gc %d, expected %d", what, n, it.strip, it.ya, it.yb, it.gc, want);
    }
}

int main() {
    const int sizes[] = {6, 8, 10, 16, 30, 64, 66, 130, 258, 1026, 4096};
    const int waves[] = {4, 64, 2048}, blocks[] = {1, 8, 512}, rows[] = {1, 3, 49};
    for (int n : sizes) {
        // the parts: the whole grid; 2 and 4 row slabs; the 2 x 2 split (rows in two, strips in two: needs two strips)
        struct Part { const char* name; std::vector<Rect> rects; };
        std::vector<Part> parts;
        const int ns_all = strips_total(n);
        parts.push_back(Part{"whole", region(n, 1, n - 1, 0, ns_all)});
        for (int world : {2, 4})
            for (int k = 0; k < world; ++k) {
                const int ya = 1 + (int)((long long)(n - 1) * k / world), yb = (int)((long long)(n - 1) * (k + 1) / world);
                parts.push_back(Part{world == 2 ? "slab/2" : "slab/4", region(n, ya, yb, 0, ns_all)});
            }
        if (ns_all >= 2)
            for (int k = 0; k < 4; ++k) {
                const int ya = k / 2 == 0 ? 1 : n / 2 + 1, yb = k / 2 == 0 ? n / 2 : n - 1, sm = ns_all / 2;
                parts.push_back(Part{"2x2", region(n, ya, yb, k % 2 == 0 ? 0 : sm, k % 2 == 0 ? sm : ns_all)});
            }
        for (auto& part : parts)
            for (int W : waves) for (int B : blocks) for (int R : rows) for (int cls : {0, 1}) {
                PlanKnobs kn; kn.target_waves = W; kn.max_blocks = B; kn.item_rows = R; kn.xcd_classes = cls;
                check_plan(part.name, n, part.rects, make_plan(part.rects, kn, 800));
                if (cls) for (int dyn : {4, 16}) check_plan("queued", n, part.rects, make_plan(part.rects, kn, 800, 0, dyn));
                if (R == 1) check_plan("single rows", n, part.rects, make_plan(part.rects, kn, 800, 1));      // the edge launches' fixed one-row items
            }
        // the knobs as the library leaves them (one tall item per wave up to N = 4096; 64-row items of the fp32 kernels)
        for (auto& part : parts) { check_plan("default", n, part.rects, make_plan(part.rects, PlanKnobs{}, 800)); check_plan("default/64", n, part.rects, make_plan(part.rects, PlanKnobs{}, 64)); }
        std::printf("N=%d plans=%lld items=%lld\n", n, g_plans, g_items);
    }
    std::printf("%s %lld\n", g_fail ? "failed" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
