// attn_band_plan.hpp — which keys a query row of a windowed / causal attention call sees, and which 64-key tiles a run of rows has to walk
// (attn_band.hpp, yume_attn_fwd_band). Plain C++, host and device, no HIP calls: tests/test_attn_band_cases_cpu.py compiles it into a host
// program and holds it to a brute-force walk.
//
// flash-attn 2.7 semantics with an explicit query position: row i of the call sits at pos(i) = q_pos0 + i on the key axis and sees
//     0 <= j < Lk   and   (left < 0 or j >= pos(i) - left)   and   (right < 0 or j <= pos(i) + right)
// left / right = -1: unbounded on that side. causal is right = 0. The 64-key tile grid is the global one (tile t = keys 64 t ... 64 t + 63).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define YUME_BAND_HD __host__ __device__ inline
#else
#define YUME_BAND_HD static inline
#endif

namespace attn_band_plan {

constexpr int KTILE = 64;      // keys per tile (attn_tile.hpp's KT)
constexpr int QBLOCK = 128;    // query rows per workgroup of attn_band_kernel
constexpr int QWAVE = 32;      // query rows per wave

struct Window { int64_t q_pos0, left, right; };
struct KeyRange { int64_t lo, hi; };       // keys lo ... hi inclusive; lo > hi: none
struct TileRange { int64_t lo, hi; };      // tiles lo ... hi inclusive; lo > hi: none

YUME_BAND_HD bool visible(int64_t i, int64_t j, int64_t Lk, Window w) {
    const int64_t pos = w.q_pos0 + i;
    return j >= 0 && j < Lk && (w.left < 0 || j >= pos - w.left) && (w.right < 0 || j <= pos + w.right);
}

// no (row, key) pair of the call is hidden: the call IS the global one. The left edge bites last at the last row, the right edge at row 0.
YUME_BAND_HD bool hides_nothing(int64_t Lq, int64_t Lk, Window w) {
    const bool left_open = w.left < 0 || w.q_pos0 + (Lq - 1) - w.left <= 0;
    const bool right_open = w.right < 0 || w.q_pos0 + w.right >= Lk - 1;
    return left_open && right_open;
}

// the keys some row of q_first ... q_last sees: every row's own interval lies inside, and the range is empty exactly when every row's is
YUME_BAND_HD KeyRange key_range(int64_t q_first, int64_t q_last, int64_t Lk, Window w) {
    int64_t lo = w.left < 0 ? 0 : w.q_pos0 + q_first - w.left;
    int64_t hi = w.right < 0 ? Lk - 1 : w.q_pos0 + q_last + w.right;
    lo = lo > 0 ? lo : 0;
    hi = hi < Lk - 1 ? hi : Lk - 1;
    return KeyRange{lo, hi};
}

YUME_BAND_HD TileRange tile_range(int64_t q_first, int64_t q_last, int64_t Lk, Window w) {
    const KeyRange r = key_range(q_first, q_last, Lk, w);
    if (r.lo > r.hi) return TileRange{0, -1};
    return TileRange{r.lo / KTILE, r.hi / KTILE};
}

// all 64 keys of tile t lie below Lk and are visible to every row of q_first ... q_last: the tile takes the unmasked body
YUME_BAND_HD bool tile_is_interior(int64_t t, int64_t q_first, int64_t q_last, int64_t Lk, Window w) {
    const int64_t k0 = t * KTILE, k1 = k0 + KTILE - 1;
    return k1 < Lk && (w.left < 0 || k0 >= w.q_pos0 + q_last - w.left) && (w.right < 0 || k1 <= w.q_pos0 + q_first + w.right);
}

}  // namespace attn_band_plan
