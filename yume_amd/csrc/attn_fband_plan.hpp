// attn_fband_plan.hpp — which keys a query row of a frame-window / frame-causal attention call sees, and which 64-key tiles a run of rows has
// to walk (attn_fband.hpp, yume_attn_fwd_fband). Plain C++, host and device, no HIP calls: tests/test_attn_fband_cases_cpu.py compiles it into
// a host program and holds it to a brute-force walk. The Python mirror is tests/attn_fband_cases.py: change both or neither.
//
// The key axis is partitioned into blocks (the frames of a video sequence), given as nspan (1 .. 16) uniform spans: span g starts at row
// row0_g (row0_0 = 0, row0_{g+1} = row0_g + rows_g * nblk_g) and holds nblk_g blocks of rows_g rows each; N rows and NB blocks in all, the
// blocks numbered through the spans in order. b(p) is the block of position p, start(b) its first row, end(b) one past its last. Row i of
// the call sits at pos(i) = q_pos0 + i and sees
//     0 <= j < Lk   and   (back < 0 or b(j) >= b(pos(i)) - back)   and   (ahead < 0 or b(j) <= b(pos(i)) + ahead)
// back / ahead = -1: unbounded on that side; (-1, 0) is the frame-causal (block-causal) mask. Every row's visible set is one interval,
//     klo(i) = start(max(b - back, 0)),   khi(i) = min(end(min(b + ahead, NB - 1)), Lk) - 1,
// both ends non-decreasing in i. The caller guarantees 0 <= q_pos0, q_pos0 + Lq <= N, Lk <= N, N < 2^31 (yume_attn_fwd_fband checks them).
// The 64-key tile grid is the global one (tile t = keys 64 t ... 64 t + 63).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define YUME_FBAND_HD __host__ __device__ inline
#else
#define YUME_FBAND_HD static inline
#endif

namespace attn_fband_plan {

constexpr int KTILE = 64;      // keys per tile (attn_tile.hpp's KT)
constexpr int QBLOCK = 128;    // query rows per workgroup of attn_fband_kernel
constexpr int QWAVE = 32;      // query rows per wave
constexpr int MAX_SPANS = 16;

struct Plan {
    int64_t q_pos0, back, ahead;
    int32_t nspan;
    int32_t rows[MAX_SPANS], nblk[MAX_SPANS];
};
struct KeyRange { int64_t lo, hi; };       // keys lo ... hi inclusive; lo > hi: none
struct TileRange { int64_t lo, hi; };      // tiles lo ... hi inclusive; lo > hi: none

YUME_FBAND_HD int64_t total_rows(const Plan& p) {
    int64_t n = 0;
    for (int g = 0; g < p.nspan; ++g) n += (int64_t)p.rows[g] * p.nblk[g];
    return n;
}

YUME_FBAND_HD int64_t total_blocks(const Plan& p) {
    int64_t n = 0;
    for (int g = 0; g < p.nspan; ++g) n += p.nblk[g];
    return n;
}

// b(pos), 0 <= pos < N: the last span that starts at or below pos (nspan compares, the same for every caller: no divergent loop on the
// device), one division inside it
YUME_FBAND_HD int32_t block_of(int32_t pos, const Plan& p) {
    int32_t row0 = 0, blk0 = 0, s_row0 = 0, s_blk0 = 0, s_rows = p.rows[0];
    for (int g = 0; g < p.nspan; ++g) {
        const bool in = pos >= row0;
        s_row0 = in ? row0 : s_row0;
        s_blk0 = in ? blk0 : s_blk0;
        s_rows = in ? p.rows[g] : s_rows;
        row0 += p.rows[g] * p.nblk[g];
        blk0 += p.nblk[g];
    }
    return s_blk0 + (pos - s_row0) / s_rows;
}

// start(b), 0 <= b < NB: the last span whose first block is at or below b (end(b) = start(b) + the rows of b's span: block_end)
YUME_FBAND_HD int32_t block_start(int32_t b, const Plan& p, int32_t* rows_of = nullptr) {
    int32_t row0 = 0, blk0 = 0, s_row0 = 0, s_blk0 = 0, s_rows = p.rows[0];
    for (int g = 0; g < p.nspan; ++g) {
        const bool in = b >= blk0;
        s_row0 = in ? row0 : s_row0;
        s_blk0 = in ? blk0 : s_blk0;
        s_rows = in ? p.rows[g] : s_rows;
        row0 += p.rows[g] * p.nblk[g];
        blk0 += p.nblk[g];
    }
    if (rows_of) *rows_of = s_rows;
    return s_row0 + (b - s_blk0) * s_rows;
}

YUME_FBAND_HD int32_t block_end(int32_t b, const Plan& p) {
    int32_t r;
    const int32_t s = block_start(b, p, &r);
    return s + r;
}

// the keys some row of q_first ... q_last sees: klo of the first row, khi of the last (both ends are non-decreasing in the row, so every row's
// own interval lies inside, and the range is empty exactly when every row's is). q_first == q_last: that row's own interval.
YUME_FBAND_HD KeyRange key_range(int64_t q_first, int64_t q_last, int64_t Lk, const Plan& p) {
    const int64_t nb = total_blocks(p);
    const int64_t b_first = block_of((int32_t)(p.q_pos0 + q_first), p);
    const int64_t b_last = q_last == q_first ? b_first : block_of((int32_t)(p.q_pos0 + q_last), p);
    const int64_t b_lo = (p.back < 0 || b_first - p.back < 0) ? 0 : b_first - p.back;
    const int64_t b_hi = (p.ahead < 0 || p.ahead > nb - 1 - b_last) ? nb - 1 : b_last + p.ahead;
    const int64_t lo = block_start((int32_t)b_lo, p);
    int64_t hi = block_end((int32_t)b_hi, p);
    hi = (hi < Lk ? hi : Lk) - 1;
    return KeyRange{lo, hi};
}

YUME_FBAND_HD bool visible(int64_t i, int64_t j, int64_t Lk, const Plan& p) {
    if (j < 0 || j >= Lk) return false;
    const int64_t b = block_of((int32_t)(p.q_pos0 + i), p), bj = block_of((int32_t)j, p);
    return (p.back < 0 || bj >= b - p.back) && (p.ahead < 0 || bj - b <= p.ahead);
}

// no (row, key) pair of the call is hidden: the call IS the global one. The back edge bites last at the last row, the ahead edge at row 0.
YUME_FBAND_HD bool hides_nothing(int64_t Lq, int64_t Lk, const Plan& p) {
    return key_range(Lq - 1, Lq - 1, Lk, p).lo == 0 && key_range(0, 0, Lk, p).hi == Lk - 1;
}

YUME_FBAND_HD TileRange tile_range(int64_t q_first, int64_t q_last, int64_t Lk, const Plan& p) {
    const KeyRange r = key_range(q_first, q_last, Lk, p);
    if (r.lo > r.hi) return TileRange{0, -1};
    return TileRange{r.lo / KTILE, r.hi / KTILE};
}

// all 64 keys of tile t lie below Lk and are visible to every row of q_first ... q_last: the tile takes the unmasked body. The row whose
// interval starts last is q_last, the one whose interval ends first is q_first.
YUME_FBAND_HD bool tile_is_interior(int64_t t, int64_t q_first, int64_t q_last, int64_t Lk, const Plan& p) {
    const int64_t k0 = t * KTILE, k1 = k0 + KTILE - 1;
    return k1 < Lk && k0 >= key_range(q_last, q_last, Lk, p).lo && k1 <= key_range(q_first, q_first, Lk, p).hi;
}

}  // namespace attn_fband_plan
