// attn_fwd8.hip — the one-wave-per-SIMD attention of attn_fwd7.hip as PERSISTENT workgroups over ONE CONTINUOUS K / V^T STREAM (r4).
//
// What attn_fwd7 spends outside its steady loop (per 256-query workgroup at the 5B shape, profiles/r3_trace_report.txt: 4.4 us of prologue —
// Q from HBM, the first K tiles —, a first tile at half rate, seven tail tiles on general code at 2.5 instead of 1.5 us, 4.6 us of epilogue,
// 0.9 us of dispatch gap: 8 % of a pass over the keys; for the 512-key cross-attention more than half of it) is the cost of treating every
// (head, query block) as its own launch-let. Here a workgroup is resident for the whole launch (one per CU), draws its items — (head, query
// block[, key range]) — by ticket from its XCD's queue (an XCD owns heads x, x + 8, ...: its 32 CUs sweep the same K / V^T and share them
// in the XCD's L2; an XCD whose queue has run dry steals from the others', so the chip's unequal XCD speeds even out), and NEVER drains its
// pipeline between items:
//   * the K / V^T stream is continuous. The LDS-DMA pieces that the last four tiles of an item used to leave out fetch the FIRST tiles
//     of the next item (of whatever head); the slot of a tile is a global tile counter & 3, so the steady code of attn_fwd7 (compile-time
//     slots, pieces riding in the score MFMAs, one counted wait + one barrier per tile) runs every tile of every item;
//   * the score half of an item's LAST tile already works for the next item: S'(0) = K'(0) Q'^T beside O += V^T(last) P(last). Q' is
//     loaded straight into the AGPRs Q occupied (global_load with an AGPR destination: no VGPRs) in the one gap where they are free —
//     between the last two tiles (bubble 1: one memory latency; the ticket for the item after next is drawn under it);
//   * behind the last tile (bubble 2) the workgroup checks the base-free body's range vote, normalises and stores O^T, zeroes it and
//     goes on: the softmax of the new item's first tile is already half done.
// A key range that ends at the ragged last tile of the sequence is only MASKED (the last two tiles run the masked pieces): the caller
// guarantees (YUME_ATTN_KV_PADDED) that K is readable up to a whole number of 64-key tiles and that V^T's columns up to there hold
// finite values, so a ragged tile is fetched like any other — no clamped sources, no fix-up pass.
// Only the base-free body streams (YUME_ATTN_Q_PRESCALED). A workgroup whose range vote fails reruns that item cold on attn_fwd7's robust
// pieces (run_keys<false, true>) and restarts the stream with the next one: every input has a defined result, as in attn_fwd7.
// Same arithmetic per tile and the same tile order as attn_fwd7: whole query blocks come out bit-identical (tests/test_ops_gpu.py).
// Roofline: MFMA bf16 dense; algorithmic work 4*Lq*Lk*128 flop per head.
// The body lives in attn8_stream.hpp (shared with the batch kernel of attn_batch8.hip); this file instantiates it for one problem.
#define ATTN8_SEG 0
#define ATTN8_KERNEL attn_fwd_kernel_v8
#include "attn8_stream.hpp"

void yume_attn8_launch(const AttnArgs& a, int* counters, int nwg, hipStream_t st) {
    hipLaunchKernelGGL(attn_fwd_kernel_v8, dim3((unsigned)nwg), dim3(256), 0, st, a, counters, nwg);
}
