// item_table.h -- the work items of a launch and who takes them: plan arithmetic, the storage layout and the tables the kernels read.
//
// Free of HIP includes (tests/cpp/item_table_driver.cpp and tests/cpp/start_record_driver.cpp compile it with the host compiler alone).  A launch covers
// a list of panels (rows x column strips, cut into row chunks); one (chunk, strip) pair is one work item.  The kernels used to get
// the panel list by value and searched it in their prologue; now every plan is expanded ONCE, when it is made, into
//   * an ItemDesc per item index, in the enumeration order (panel by panel, chunk-major, strip fastest): 16 bytes, and
//   * a StartRec per wave of the launch and march direction: the item indices that wave takes (its ItemSeq) and the addressing
//     of its FIRST item, ready made: 64 bytes,
// each of which a wave fetches with one scalar load at a wave-uniform index (cg_kernels.h: decode_item, start_rec).
#pragma once
#include <algorithm>
#include <vector>

#ifdef __HIP__
#define MI355CG_HD __attribute__((host)) __attribute__((device))
#else
#define MI355CG_HD
#endif

namespace mi355cg {

// ---- storage layout -------------------------------------------------------------------------------
// Node (x, y) of the (N+1)x(N+1) bounding grid lives at  row_off(y) + x - base0.  Rows y <= N/2
// (bottom-right block + its boundary row 0) only store columns [cb, cb+Pb), cb = N/2 rounded down
// to 32; rows above store columns [0, Pu).  Pb, Pu, cb are multiples of 32 elements so every row
// starts 256-B aligned.  Boundary nodes and pads hold 0 and stay 0; Dirichlet data is in the RHS.
struct Geom {
    int N, half, cb, xlim;            // xlim: columns [0, xlim) are touched by the stencil strips
    int Pb, Pu;                       // row pitches (elements) of bottom / upper rows
    int y_lo, y_hi;                   // owned rows (inclusive); rows y_lo-1 and y_hi+1 are ghosts
    long long base0;                  // physical offset of the first stored element (row y_lo-1)
    long long own_begin, own_len;     // flat [begin, begin+len) of the owned rows, local offsets
    double A, xk, yk;                 // stencil coefficients (grid_system.cpp:316-318)
};

MI355CG_HD inline long long row_off(const Geom& g, int y) {
    return y <= g.half ? (long long)y * g.Pb - g.cb
                       : (long long)(g.half + 1) * g.Pb + (long long)(y - g.half - 1) * g.Pu;
}
MI355CG_HD inline bool node_interior(const Geom& g, int x, int y) {
    return y >= 1 && y <= g.N - 1 && x <= g.N - 1 && x >= (y <= g.half ? g.half + 1 : 1);
}

constexpr int kBlock = 256;           // threads per workgroup = 4 wave64
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
constexpr int kMaxPanels = 8;

// A panel is a rectangle of owned rows x column strips, cut into row chunks; one (chunk, strip)
// pair is one work item = one wave marching `ty` rows of a 64*VEC-column strip.
// gc (2-D decomposition): bit 0 = the column left of the panel's first strip belongs to another part (a ghost
// column of this part), bit 1 = the same on the right of its last strip.
struct Panel { int y0, y1, s0, ns, ty, nchunks, item0, gc; };
// XCD classes: workgroups land on XCD blockIdx % 8, and every XCD has its own L2.  With ncls == 8 the items are cut into
// eight contiguous ranges [cls0[k], cls0[k+1]) -- whole bands of chunk rows -- and range k is served by the workgroups with
// blockIdx % 8 == k only: the strips left and right of a workgroup (whose edge columns it reads) and the chunk rows above and
// below (whose halo rows it reads) are then work of the SAME XCD and those reads hit its L2 instead of going to the fabric
// (PMC: read traffic of the stencil launch 1.10 x -> see profiles/r02_tune_notes.md).  A wrong guess about the placement costs
// those hits, never correctness.
constexpr int kXcds = 8;
struct WorkList { Panel p[kMaxPanels]; int np; int nitems; int ncls; int cls0[kXcds + 1]; };

// One work item: strip, first and last own row, ghost-column flags of this strip (Panel::gc restricted to the panel's end strips)
struct alignas(16) ItemDesc { int strip, ya, yb, gc; };
// the item indices a wave takes: first, first + step, ... < end (begin: first index of the wave's class, for the reversed march and the queues)
struct alignas(16) ItemSeq { int first, step, begin, end; };

// The wave-uniform addressing data of one work item, constant while the item is marched (what the lanes add: cg_kernels.h,
// ItemAddr).  Written once, for both sides: the host expands it into the start records, a wave evaluates it for its later items.
// DESC: the item is marched from its last row down (the update launches).  elem: bytes per element.
struct ItemUni {
    long long base_el;          // element offset of row y0 = ya - 1 (the lowest row the item touches) from the start of a vector
    int so_first, so_c0;        // byte offsets from row y0 of the halo row behind the first own row / of the first own row
    int nrows, ystart;          // rows of the item; its first row in march order
    int strip;
    int bot;                    // 1: all own rows lie in the bottom block of the L
    int gc;
};
template <bool DESC>
MI355CG_HD inline ItemUni item_uniform(const Geom& g, const ItemDesc& it, int elem) {
    ItemUni u;
    const int y0 = it.ya - 1;
    u.nrows = it.yb - it.ya + 1;
    u.ystart = DESC ? it.yb : it.ya;
    u.base_el = row_off(g, y0) - g.base0;
    u.so_first = DESC ? (int)((row_off(g, it.yb + 1) - row_off(g, y0)) * (long long)elem) : 0;
    u.so_c0 = DESC ? (int)((row_off(g, it.yb) - row_off(g, y0)) * (long long)elem) : (y0 + 1 <= g.half ? g.Pb : g.Pu) * elem;
    u.strip = it.strip;
    u.bot = it.ya <= g.half ? 1 : 0;
    u.gc = it.gc;
    return u;
}
// What a wave starts a launch from: its item sequence and the ItemUni of its first item (have == 0: the wave has no item, u is 0).
// Ascending launches (stencil) start on item seq.first, the reversed descending march (update) on seq.end - 1 - (seq.first - seq.begin);
// a launch with run-time queues starts every wave on the same static first item.
struct alignas(64) StartRec { ItemSeq seq; ItemUni u; int have; int pad; };
static_assert(sizeof(StartRec) == 64, "StartRec: one 64-byte scalar load");

// Rows [y0, y1] x strips [s0, s1) with their ghost-column flags
struct Rect { int y0, y1, s0, s1, gc; };

// Append rows [y0, y1] x strips [s0, s1) cut into items of ~ty rows.  Returns the strip-rows added (ty <= 0: only count).
inline long long add_panel(WorkList& wl, int y0, int y1, int s0, int s1, int ty, int gc) {
    const int rows = y1 - y0 + 1, ns = s1 - s0;
    if (rows <= 0 || ns <= 0) return 0;
    if (ty <= 0) return (long long)rows * ns;
    if (wl.np >= kMaxPanels) return 0;
    Panel& P = wl.p[wl.np++];
    P.y0 = y0; P.y1 = y1; P.s0 = s0; P.ns = ns; P.gc = gc;
    P.nchunks = (rows + ty - 1) / ty;
    P.ty = (rows + P.nchunks - 1) / P.nchunks;            // rebalance
    P.nchunks = (rows + P.ty - 1) / P.ty;
    P.item0 = wl.nitems;
    wl.nitems += P.ns * P.nchunks;
    return (long long)rows * ns;
}

// One launch shape: the work items of a set of rows x strips, the persistent grid that marches them, and (device memory, owned by
// the handle: uploaded when the plans are built, freed with it) the two tables of that shape.
struct Plan {
    WorkList wl{}; int grid = 0; int ty = 0;
    int elem = 8;                     // bytes per element of the kernels that march this plan (the start records hold byte offsets)
    ItemDesc* d_items = nullptr;      // wl.nitems entries
    StartRec* d_start[2] = {nullptr, nullptr};     // grid * kWaves entries each: ascending march, reversed descending march
};

// What the environment may override (MI355CG_WAVES, MI355CG_BLOCKS, MI355CG_ITEM_ROWS, MI355CG_XCD_CLASSES)
struct PlanKnobs { int target_waves = 2048, max_blocks = 512, item_rows = 0 /* 0: the caller's max_rows */, xcd_classes = 1; };

// Launch shape for a list of rectangles.  2 048 resident waves (2 workgroups per CU: 8 waves per CU already saturate the
// memory system, round 1) take the items round-robin.  Measured (tools/tune.py, profiles/r02_tune_notes.md): one round of
// items "as tall as it takes" is the best fp64 shape up to ~800 rows per item (N <= 16384 on one GPU); taller items (3 136 rows
// of a 262 KB pitch at N = 32768: every wave sweeps 0.8 GB per stream) lose 14-16 %, so the height is capped and the rest
// becomes further rounds -- which cost nothing since the load pipeline no longer drains between items.  The fp32 kernels
// (256-column strips) like 64 rows.  The height is then nudged so that the items fill a whole number of rounds: a last
// round with a few items would run at a fraction of the chip.
inline Plan make_plan(const std::vector<Rect>& rects, const PlanKnobs& kn, int max_rows, int fixed_ty = 0, int dyn_rows = 0) {
    Plan pl{};
    const int target_waves = std::max(kWaves, kn.target_waves);
    const int max_blocks = std::max(1, kn.max_blocks);
    const int waves = std::min(target_waves, max_blocks * kWaves);
    const long long item_rows = std::max(1, kn.item_rows > 0 ? kn.item_rows : max_rows);
    long long strip_rows = 0;
    WorkList dry{};
    for (auto& r : rects) strip_rows += add_panel(dry, r.y0, r.y1, r.s0, r.s1, 0, 0);
    if (strip_rows == 0) return pl;
    // XCD classes (see WorkList): only for launches that fill the chip, never for the single-row edge launches
    const bool classes = kn.xcd_classes != 0 && fixed_ty == 0 && max_blocks >= kXcds && strip_rows >= 4LL * waves;
    auto build = [&](int ty) {
        WorkList wl{};
        wl.ncls = 1;
        for (auto& r : rects) add_panel(wl, r.y0, r.y1, r.s0, r.s1, ty, r.gc);
        if (classes) {
            wl.ncls = kXcds;
            for (int k = 0; k <= kXcds; ++k) wl.cls0[k] = (int)((long long)wl.nitems * k / kXcds);
        }
        return wl;
    };
    auto fits = [&](const WorkList& wl, long long rounds) {
        if (wl.ncls == kXcds) { for (int k = 0; k < kXcds; ++k) if (wl.cls0[k + 1] - wl.cls0[k] > rounds * (waves / kXcds)) return false; return true; }
        return wl.nitems <= rounds * waves;
    };
    int ty = fixed_ty;
    if (ty <= 0 && dyn_rows > 0 && classes) {
        // dynamic queues: short items, several per wave; no need to fill whole rounds -- whoever is early takes more
        ty = dyn_rows;
        pl.wl = build(ty);
    } else if (ty <= 0) {
        const long long rounds = std::max<long long>(1, (strip_rows + waves * item_rows - 1) / (waves * item_rows));
        ty = (int)std::max<long long>(std::min<long long>(8, item_rows), (strip_rows + rounds * waves - 1) / (rounds * waves));
        for (int tries = 0; tries < 64; ++tries) {
            pl.wl = build(ty);
            if (fits(pl.wl, rounds)) break;
            ++ty;
        }
    } else {
        pl.wl = build(ty);
    }
    pl.ty = ty;
    pl.grid = std::max(1, std::min(max_blocks, (pl.wl.nitems + kWaves - 1) / kWaves));
    if (pl.wl.ncls == kXcds) pl.grid = std::min(max_blocks / kXcds * kXcds, (pl.grid + kXcds - 1) / kXcds * kXcds);      // the classes take turns over the workgroups
    return pl;
}

// ---- the tables ----------------------------------------------------------------------------------------------------
// Items are enumerated panel by panel, chunk-major (strip fastest).
inline std::vector<ItemDesc> build_item_table(const WorkList& wl) {
    std::vector<ItemDesc> t((size_t)std::max(0, wl.nitems));
    for (int k = 0; k < wl.np; ++k) {
        const Panel& P = wl.p[k];
        int i = P.item0;
        for (int chunk = 0; chunk < P.nchunks; ++chunk) {
            const int ya = P.y0 + chunk * P.ty, yb = std::min(P.y1, ya + P.ty - 1);
            for (int s = 0; s < P.ns; ++s, ++i)
                t[(size_t)i] = ItemDesc{P.s0 + s, ya, yb, (s == 0 ? (P.gc & 1) : 0) | (s == P.ns - 1 ? (P.gc & 2) : 0)};
        }
    }
    return t;
}

// Entry b * kWaves + w: wave w of workgroup b of a launch of `grid` workgroups.  Without classes the waves of the launch take
// the items round-robin; with classes workgroup b serves class b % 8 together with the other workgroups of that residue.
inline std::vector<ItemSeq> build_seq_table(const WorkList& wl, int grid) {
    std::vector<ItemSeq> t((size_t)std::max(0, grid) * kWaves);
    for (int b = 0; b < grid; ++b) {
        ItemSeq s{b * kWaves, grid * kWaves, 0, wl.nitems};
        if (wl.ncls == kXcds) {
            const int cls = b % kXcds, nb = (grid - cls + kXcds - 1) / kXcds;      // workgroups of this class
            s = ItemSeq{wl.cls0[cls] + b / kXcds * kWaves, nb * kWaves, wl.cls0[cls], wl.cls0[cls + 1]};
        }
        for (int w = 0; w < kWaves; ++w) { t[(size_t)b * kWaves + w] = s; t[(size_t)b * kWaves + w].first += w; }
    }
    return t;
}

// Entry b * kWaves + w: the start record of wave w of workgroup b.  reversed: for the update launches (see StartRec).
inline std::vector<StartRec> build_start_table(const WorkList& wl, int grid, const Geom& g, int elem, bool reversed) {
    const std::vector<ItemDesc> items = build_item_table(wl);
    const std::vector<ItemSeq> seq = build_seq_table(wl, grid);
    std::vector<StartRec> t(seq.size(), StartRec{});
    for (size_t w = 0; w < seq.size(); ++w) {
        const ItemSeq& s = seq[w];
        t[w].seq = s;
        if (s.first >= s.end) continue;
        t[w].have = 1;
        t[w].u = reversed ? item_uniform<true>(g, items[(size_t)(s.end - 1 - (s.first - s.begin))], elem) : item_uniform<false>(g, items[(size_t)s.first], elem);
    }
    return t;
}

}  // namespace mi355cg
