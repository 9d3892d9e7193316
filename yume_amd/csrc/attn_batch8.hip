// attn_batch8.hip — the persistent self-attention of attn_fwd8.hip over nseg STACKED problems in one launch (r12, yume_attn_fwd_batch): the
// self-attention of a batched forward (DiTEngine.forward_batch), whose samples are stacked rows of one Q / K / V^T / O set.
//
// It is attn_fwd8.hip's kernel with (segment, head) in the place of head — the same source, attn8_stream.hpp with ATTN8_SEG 1, not a copy:
//   * an item is (virtual head hv = s * H + h, query block[, key range]); XCD y owns the virtual heads hv = y (mod 8); the plan is
//     attn_plan's for nseg * H heads; tickets, stealing, the continuous K / V^T stream across item boundaries (also across segments), the
//     bubbles, the range vote and its cold rerun are untouched;
//   * the Q, K, V^T and O bases of an item are its segment's base plus its head's column offset. The kernel addresses with a scalar 64-bit
//     base plus 32-bit per-lane offsets: the segment's offset (s * pitch * ld * 2 bytes, beyond 4 GiB in the product) goes into the scalar
//     base at the item boundary, so the 32-bit limit the dispatcher enforces is ONE segment's extent;
//   * the wave-uniform per-item values (s, h) go back to SGPRs by readfirstlane in decode_item, as the others do;
//   * key-range pieces write their fp32 partial results into their segment's slice of the workspace ([nseg][splits, rows, H*128] and
//     [nseg][splits, rows, H, 2]); attn_combine_kernel is launched once per segment on that slice.
// The arithmetic per tile and the tile order are attn_fwd8.hip's: segment s comes out bit-identical to a variant 8 launch on its views
// whenever both carry the same plan (tests/test_attn_batch_gpu.py).
// Resource usage (-Rpass-analysis=kernel-resource-usage) and the ISA audit (tests/test_attn_batch_isa.py): profiles/r12_forward_batch.md.
#define ATTN8_SEG 1
#define ATTN8_KERNEL attn_batch_kernel_p8
#include "attn8_stream.hpp"

void yume_attn_batch8_launch(const AttnArgs& a, const AttnBatchSeg& sg, int* counters, int nwg, hipStream_t st) {
    hipLaunchKernelGGL(attn_batch_kernel_p8, dim3((unsigned)nwg), dim3(256), 0, st, a, sg, counters, nwg);
}
