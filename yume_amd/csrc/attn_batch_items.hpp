// attn_batch_items.hpp — the item list of the persistent attention kernels (attn8_stream.hpp), as plain integer functions that the host can
// compile too (tests/test_attn_batch_cabi.py walks them): which (head, query block[, key range]) ticket j of XCD y's queue is, and which
// (segment, head) a virtual head of a batch launch stands for. No HIP calls, no device types.
//
// XCD y owns the (virtual) heads y, y + 8, ...; its queue holds the whole query blocks head by head, then the key-range pieces of the blocks
// >= tail_qb. A batch launch (yume_attn_fwd_batch) of nseg segments with H heads each is a launch over nseg * H virtual heads
// hv = s * H + h: the queues, the tickets and the plan see virtual heads only.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ATTN_ITEMS_FN __host__ __device__ __forceinline__
#else
#define ATTN_ITEMS_FN static inline
#endif

namespace attn_items {

struct Decoded { int h, qb, sp, nsp; };        // h: the (virtual) head

// heads of XCD y among H
ATTN_ITEMS_FN int heads_of_xcd(int H, int y) { return (H + 7 - y) >> 3; }
// items of XCD y's queue
ATTN_ITEMS_FN int queue_len(int H, int nqb, int tail_qb, int splits, int y) { return heads_of_xcd(H, y) * (tail_qb + (nqb - tail_qb) * splits); }
// item j (0 <= j < queue_len) of XCD y's queue
ATTN_ITEMS_FN Decoded decode(int H, int nqb, int tail_qb, int splits, int y, int j) {
    Decoded it;
    const int hx = heads_of_xcd(H, y);
    const int nmain = hx * tail_qb, ntq = nqb - tail_qb;
    if (j < nmain) {
        it.h = y + 8 * (j / tail_qb);
        it.qb = j % tail_qb;
        it.sp = 0;
        it.nsp = 1;
    } else {
        const int u = (j - nmain) / splits;
        it.sp = (j - nmain) % splits;
        it.nsp = splits;
        it.h = y + 8 * (u / ntq);
        it.qb = tail_qb + u % ntq;
    }
    return it;
}
// key tiles [t0, t1) of piece sp of nsp over nt tiles
ATTN_ITEMS_FN int piece_begin(int nt, int sp, int nsp) { return (int)((int64_t)nt * sp / nsp); }
// virtual head -> (segment, head) for H heads per segment
ATTN_ITEMS_FN int segment_of(int hv, int H) { return hv / H; }
ATTN_ITEMS_FN int head_in_segment(int hv, int H) { return hv - (hv / H) * H; }

}  // namespace attn_items
