// attn_plan.hpp — launch plans of the two 256-query-block self-attention kernels (attn_fwd7.hip, attn_fwd8.hip). Host only, no HIP calls.
//
// An XCD owns ceil(H/8) heads x nq query blocks of 256 rows = that many workgroups of equal length on its 32 CUs; a partial
// last round costs a whole round. The last `nq - tail_qb` query blocks of every head can instead be cut into `splits` key ranges
// whose pieces are dispatched behind the whole blocks (same launch) and merged by attn_combine_kernel. The plan minimises the
// makespan of that in-order dispatch under a simple cost model (a piece = 1/splits of a block + a fixed share).
#pragma once
#include <stdint.h>

namespace attn_plan {   // (static: an experiment build of the library loaded next to the product one keeps its own plans and memo)

constexpr int QBLOCK = 256;   // query rows per block of both kernels
constexpr int KTILE = 64;     // keys per tile
constexpr int HDIM = 128;

struct Plan { int64_t tail_qb; int splits; };      // query blocks >= tail_qb are cut into `splits` key ranges; splits == 1: none is

// What one item of the dispatch costs, in whole blocks (per_tile false) or in key tiles (per_tile true: a block's own work is its nt tiles).
struct CostModel {
    bool per_tile;
    double boundary;      // what every item pays on top of its share of the work
    double piece_extra;   // what a piece pays on top of that
    double merge;         // the merge pass behind a split launch
    int min_tiles;        // a piece is at least this many key tiles
    double improve;       // a split has to beat the best plan so far by this fraction of a whole block's cost
    int64_t min_lk;       // shapes the kernel takes: Lk >= min_lk and Lq >= QBLOCK
};

enum Model { V7 = 0, V8 = 1 };
constexpr CostModel MODELS[2] = {
    // attn_fwd7.hip, dispatched in block-id order: a piece carries a fixed prologue share
    {false, 0.0, 0.04, 0.03, 16, 0.02, 1536},
    // attn_fwd8.hip, the persistent kernel: the same item list, drawn by ticket instead of dispatched in block-id order. An item boundary
    // costs ~2.5 tile times there (two bubbles) instead of a whole prologue and epilogue, so shorter pieces pay: down to 8 key tiles (what
    // the GPU tests exercise; the kernel's own protocol needs 5; an item's successor's ticket is drawn while it runs, with room). A piece
    // adds its fp32 partial store.
    {true, 2.5, 1.0, 6.0, 8, 0.01, 8 * KTILE},
};

// shapes the kernel takes (the caller's flags and the counter workspace are checked at the call)
static inline bool applies(Model m, int64_t Lq, int64_t Lk) { return Lk >= MODELS[m].min_lk && Lq >= QBLOCK; }

static inline Plan search(const CostModel& cm, int64_t Lq, int64_t Lk, int64_t H) {
    const int64_t nq = (Lq + QBLOCK - 1) / QBLOCK, hx = (H + 7) / 8, nt = (Lk + KTILE - 1) / KTILE;
    Plan best{nq, 1};
    const double work = cm.per_tile ? (double)nt : 1.0, whole = work + cm.boundary;
    auto makespan = [&](int64_t tail_q, int splits) {
        double cu[32];
        for (double& c : cu) c = 0.0;
        auto put = [&](double cost) {
            int m = 0;
            for (int i = 1; i < 32; ++i) if (cu[i] < cu[m]) m = i;
            cu[m] += cost;
        };
        for (int64_t i = 0; i < hx * (nq - tail_q); ++i) put(whole);
        for (int64_t i = 0; i < hx * tail_q * splits; ++i) put(work / splits + cm.boundary + cm.piece_extra);
        double mx = 0.0;
        for (double c : cu) mx = c > mx ? c : mx;
        return mx + (splits > 1 ? cm.merge : 0.0);
    };
    double bm = makespan(0, 1);
    for (int splits = 2; splits <= 4; ++splits) {
        if (nt / splits < cm.min_tiles) break;
        for (int64_t tail_q = 1; tail_q <= nq && tail_q <= 12; ++tail_q) {
            const double m = makespan(tail_q, splits);
            if (m < bm - cm.improve * whole) { bm = m; best = Plan{nq - tail_q, splits}; }
        }
    }
    return best;
}

// the search (~37 makespan simulations with a 32-way min-scan per workgroup) is a pure function of the launch shape and runs on the host
// inside every yume_attn_fwd_ws call (30-40 times per denoise step): memoised per calling thread, 8 shapes per model
static inline Plan plan(Model m, int64_t Lq, int64_t Lk, int64_t H) {
    struct Entry { int64_t Lq, Lk, H; Plan pl; };
    struct Memo { Entry e[8]; int used, next; };
    static thread_local Memo memos[2] = {};
    Memo& mm = memos[m];
    for (int i = 0; i < mm.used; ++i)
        if (mm.e[i].Lq == Lq && mm.e[i].Lk == Lk && mm.e[i].H == H) return mm.e[i].pl;
    const Plan pl = search(MODELS[m], Lq, Lk, H);
    mm.e[mm.next] = Entry{Lq, Lk, H, pl};
    mm.next = (mm.next + 1) & 7;
    mm.used = mm.used < 8 ? mm.used + 1 : 8;
    return pl;
}

// rows the pieces cover, and the scratch for their partial results: [splits, rows, H*128] fp32 O + [splits, rows, H, 2] fp32 (max, sum)
static inline int64_t split_rows(const Plan& pl, int64_t Lq) { return Lq - pl.tail_qb * QBLOCK; }
static inline int64_t workspace_bytes(const Plan& pl, int64_t Lq, int64_t H) {
    return pl.splits > 1 ? (int64_t)pl.splits * split_rows(pl, Lq) * (H * HDIM + H * 2) * 4 : 0;
}

}  // namespace attn_plan
