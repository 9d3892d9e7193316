// attn_fprefix_plan.hpp — frame-window attention over TWO key buffers: a prefix of n_prefix keys that every row sees, in a buffer of its own,
// and a suffix under attn_fband_plan.hpp's frame window (attn_fprefix.hpp, yume_attn_fwd_fprefix). Plain C++, host and device, no HIP calls:
// tests/test_attn_fprefix_cases_cpu.py compiles it into a host program and holds it to a brute-force walk. The Python mirror is
// tests/attn_fprefix_cases.py: change both or neither.
//
// The partition, pos(i), b(p), back, ahead and Lk are the SUFFIX's (attn_fband_plan.hpp), with its own key numbering from 0. Row i sees
//     every prefix key 0 <= j < n_prefix   and   the suffix keys of attn_fband_plan::visible(i, j)
// and O is the softmax over the union, in the logical order prefix then suffix.
//
// The kernel's PADDED coordinate lays both segments on one 64-key tile grid: prefix tile t (0 <= t < np, np = ceil(n_prefix / 64)) holds the
// prefix keys 64 t ..., suffix tile s sits at tile np + s, its keys at P + 64 s ... with P = 64 np. The coordinates n_prefix ... P - 1 are
// the pad of the ragged last prefix tile: no key at all. In that coordinate a row sees [0, n_prefix) ∪ [P + klo(i), P + khi(i)] — r29's two
// intervals with send = n_prefix — and a run of rows walks attn_fsink_plan's ascending TileList: the prefix tiles [0, np), then the suffix's
// band tiles [np + t_lo, np + t_hi] (a jump wherever t_lo > 0, and a change of buffer in every case).
#pragma once
#include "attn_fsink_plan.hpp"

namespace attn_fprefix_plan {

using attn_fband_plan::KeyRange;
using attn_fband_plan::KTILE;
using attn_fband_plan::Plan;
using attn_fband_plan::TileRange;
using attn_fsink_plan::TileList;

YUME_FBAND_HD int64_t prefix_tiles(int64_t n_prefix) { return (n_prefix + KTILE - 1) / KTILE; }
// P: the padded coordinate of suffix key 0
YUME_FBAND_HD int64_t pad(int64_t n_prefix) { return prefix_tiles(n_prefix) * KTILE; }

// seg 0: prefix key j; seg 1: suffix key j
YUME_FBAND_HD bool visible(int64_t i, int seg, int64_t j, int64_t Lk, const Plan& p, int64_t n_prefix) {
    if (seg == 0) return j >= 0 && j < n_prefix;
    return attn_fband_plan::visible(i, j, Lk, p);
}

// the same pair by its padded coordinate c (the pad of the ragged prefix tile is nobody's key)
YUME_FBAND_HD bool visible_padded(int64_t i, int64_t c, int64_t Lk, const Plan& p, int64_t n_prefix) {
    const int64_t P = pad(n_prefix);
    return c < P ? visible(i, 0, c, Lk, p, n_prefix) : visible(i, 1, c - P, Lk, p, n_prefix);
}

// the list of the rows q_first ... q_last in padded tiles: every prefix tile, then the tiles of which some row sees a suffix key. Without
// suffix tiles b_lo = np, b_hi = np - 1; with n_prefix >= 1 the list is never empty.
YUME_FBAND_HD TileList tile_list(int64_t q_first, int64_t q_last, int64_t Lk, const Plan& p, int64_t n_prefix) {
    const int64_t np = prefix_tiles(n_prefix);
    const TileRange r = attn_fband_plan::tile_range(q_first, q_last, Lk, p);      // none: {0, -1}
    if (r.lo > r.hi) return TileList{np, np, np - 1};
    return TileList{np, np + r.lo, np + r.hi};
}

// all 64 coordinates of padded tile t are keys and are visible to every row of q_first ... q_last: the tile takes the unmasked body
YUME_FBAND_HD bool tile_is_interior(int64_t t, int64_t q_first, int64_t q_last, int64_t Lk, const Plan& p, int64_t n_prefix) {
    const int64_t np = prefix_tiles(n_prefix);
    if (t < np) return t * KTILE + KTILE - 1 < n_prefix;
    return attn_fband_plan::tile_is_interior(t - np, q_first, q_last, Lk, p);
}

}  // namespace attn_fprefix_plan
