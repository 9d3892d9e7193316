// attn_fsink_plan.hpp — the frame window of attn_fband_plan.hpp with an always-visible sink: the first `sink` blocks (frames) of the partition
// are seen by every row (attn_fsink.hpp, yume_attn_fwd_fsink). Plain C++, host and device, no HIP calls: tests/test_attn_fsink_cases_cpu.py
// compiles it into a host program and holds it to a brute-force walk. The Python mirror is tests/attn_fsink_cases.py: change both or neither.
//
// The partition, pos(i), b(p), back and ahead are attn_fband_plan.hpp's; 0 <= sink <= NB. Row i sees
//     0 <= j < Lk   and   ( b(j) < sink   or   attn_fband_plan::visible(i, j) )
// With send = min(start(sink), Lk) (start(NB) = N; the same for every row) a row's visible set is [0, send) ∪ [klo(i), khi(i)], klo / khi
// being attn_fband_plan::key_range's: one interval where klo(i) <= send (also where the band part is empty), two with a hidden gap
// otherwise. The sink changes which keys are seen, not what the rows of the sink frames themselves see beyond that.
//
// A run of rows walks an ascending LIST of 64-key tiles, each once: the sink tiles [0, ceil(send / 64)), then the band tiles
// [max(t_lo, ceil(send / 64)), t_hi] of the run's attn_fband_plan::tile_range — one run, or two with a jump between them.
#pragma once
#include "attn_fband_plan.hpp"

namespace attn_fsink_plan {

using attn_fband_plan::KeyRange;
using attn_fband_plan::KTILE;
using attn_fband_plan::Plan;
using attn_fband_plan::TileRange;

// the tiles [0, n_sink) and [b_lo, b_hi], n_sink <= b_lo. A run without band tiles behind the sink's has b_lo = n_sink, b_hi = n_sink - 1: the
// last tile of the list is b_hi in every case, and the list is empty exactly when b_hi < 0.
struct TileList { int64_t n_sink, b_lo, b_hi; };

// start(sink) cut to Lk: the keys below it are the sink
YUME_FBAND_HD int64_t send(int64_t Lk, const Plan& p, int64_t sink) {
    if (sink <= 0) return 0;
    const int64_t s = sink >= attn_fband_plan::total_blocks(p) ? attn_fband_plan::total_rows(p) : attn_fband_plan::block_start((int32_t)sink, p);
    return s < Lk ? s : Lk;
}

YUME_FBAND_HD bool visible(int64_t i, int64_t j, int64_t Lk, const Plan& p, int64_t sink) {
    if (j < 0 || j >= Lk) return false;
    return j < send(Lk, p, sink) || attn_fband_plan::visible(i, j, Lk, p);
}

// the sink makes no pair visible that the frame window hides: every row's own interval covers [0, send). klo is largest at the last row,
// khi smallest at row 0 (a row whose interval is empty has khi < klo, and fails one of the two).
YUME_FBAND_HD bool adds_nothing(int64_t Lq, int64_t Lk, const Plan& p, int64_t sink) {
    const int64_t se = send(Lk, p, sink);
    return se == 0 || (attn_fband_plan::key_range(Lq - 1, Lq - 1, Lk, p).lo == 0 && attn_fband_plan::key_range(0, 0, Lk, p).hi >= se - 1);
}

// no (row, key) pair of the call is hidden: the sink is the whole key axis, or every row's interval starts inside (or right behind) the
// sink and ends at the last key
YUME_FBAND_HD bool hides_nothing(int64_t Lq, int64_t Lk, const Plan& p, int64_t sink) {
    const int64_t se = send(Lk, p, sink);
    return se >= Lk || (attn_fband_plan::key_range(0, 0, Lk, p).hi == Lk - 1 && attn_fband_plan::key_range(Lq - 1, Lq - 1, Lk, p).lo <= se);
}

// the list of the rows q_first ... q_last (a workgroup's, a wave's): a tile is listed exactly when some row of the run sees one of its keys
YUME_FBAND_HD TileList tile_list(int64_t q_first, int64_t q_last, int64_t Lk, const Plan& p, int64_t sink) {
    const int64_t ns = (send(Lk, p, sink) + KTILE - 1) / KTILE;
    const TileRange r = attn_fband_plan::tile_range(q_first, q_last, Lk, p);      // none: {0, -1}
    return TileList{ns, r.lo > ns ? r.lo : ns, r.hi > ns - 1 ? r.hi : ns - 1};
}

YUME_FBAND_HD int64_t tile_count(const TileList& l) { return l.n_sink + (l.b_hi - l.b_lo + 1); }
YUME_FBAND_HD int64_t first_tile(const TileList& l) { return l.n_sink > 0 ? 0 : l.b_lo; }
// the tile behind t in the list (t a listed tile; the answer lies behind b_hi where t is the last)
YUME_FBAND_HD int64_t next_tile(int64_t t, const TileList& l) { return t + 1 == l.n_sink ? l.b_lo : t + 1; }
YUME_FBAND_HD bool in_list(int64_t t, const TileList& l) { return t >= 0 && (t < l.n_sink || (t >= l.b_lo && t <= l.b_hi)); }

// all 64 keys of tile t lie below Lk and are visible to every row of q_first ... q_last through ONE of the two pieces: the tile takes the
// unmasked body. (A tile that is whole only as the union of the sink's end and a band start takes the masked one.)
YUME_FBAND_HD bool tile_is_interior(int64_t t, int64_t q_first, int64_t q_last, int64_t Lk, const Plan& p, int64_t sink) {
    const int64_t k1 = t * KTILE + KTILE - 1;
    return k1 < Lk && (k1 < send(Lk, p, sink) || attn_fband_plan::tile_is_interior(t, q_first, q_last, Lk, p));
}

}  // namespace attn_fsink_plan
