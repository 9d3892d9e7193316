// attn_args.hpp — launch arguments shared by the attention kernels (attn_fwd.hip and its kernel headers, attn_fwd7.hip, attn_fwd8.hip,
// attn_batch8.hip).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

struct AttnArgs {
    const unsigned short* Q; int64_t ldq;
    const unsigned short* K; int64_t ldk;
    const unsigned short* Vt; int64_t ldvt;
    unsigned short* O; int64_t ldo;
    int Lq, Lk, H;
    float scale_log2;  // softmax scale * log2(e); exactly 1 when q_prescaled
    int q_prescaled;   // Q already carries softmax scale * log2(e) (YUME_ATTN_Q_PRESCALED): the scores are the exponents
    int accumulate;
    int nqb;           // query blocks per head (of the rows [q_lo, Lq) this launch covers)
    int q_lo;          // first query row of this launch
    // key-range split (the v7 and v8 kernels, planned by attn_plan.hpp): query blocks >= tail_qb are cut into `splits` key ranges inside the
    // same launch (their pieces come after the whole blocks and fill the partial last round of workgroups). Piece s walks key tiles
    // [nt*s/splits, nt*(s+1)/splits) and writes its UNNORMALISED O (fp32) + running max + row sum here; attn_combine_kernel (attn_combine.hpp)
    // merges the pieces. rows = Lq - (q_lo + 256*tail_qb). No launch splits the other kernels: they see tail_qb == nqb, splits == 1 and
    // never touch part_o / part_ml (attn_fwd_kernel_v2 still carries a gridDim.y split that no launch uses).
    float* part_o;     // [splits, rows, H*128]
    float* part_ml;    // [splits, rows, H, 2]
    int tail_qb, splits;
    // yume_attn_fwd_kw: the LAST key (Lk - 1) counts last_w times (its exponential is multiplied by it); exactly 1 on every other call.
    // Read by attn_fwd_kernel_v2<true> and attn_short.hpp only
    float last_w;
};

// attn_fwd7.hip: 4-wave / 64-queries-per-wave kernel (one wave per SIMD, 512 registers); grid = ceil(H/8) * nqb * 8 blocks
void yume_attn7_launch(const AttnArgs& a, hipStream_t st);
// attn_fwd8.hip: the same kernel as `nwg` persistent workgroups over one continuous K / V^T stream; items (the query blocks of a.nqb /
// a.tail_qb / a.splits, as for attn_fwd7) are drawn by ticket from `counters`, one 64-byte set of the caller's counter workspace
// (counters.hpp). Requires a.q_prescaled, K readable and V^T finite up to a whole number of 64-key tiles, every item >= 5 key tiles.
void yume_attn8_launch(const AttnArgs& a, int* counters, int nwg, hipStream_t st);

// A batch launch (yume_attn_fwd_batch): nseg problems of one shape stacked in the same buffers. The AttnArgs beside it describe segment 0 with
// H = nseg * (heads per segment) VIRTUAL heads; segment s lies these many elements further on.
struct AttnBatchSeg {
    int H;                                  // heads per segment: virtual head hv = s * H + h
    int64_t q_step, k_step, o_step;         // q_pitch * ldq, k_pitch * ldk, q_pitch * ldo
    int64_t vt_step;                        // k_pitch (columns of V^T)
    int64_t part_o_step, part_ml_step;      // floats between two segments' slices of part_o / part_ml
};
// attn_batch8.hip: attn_fwd8.hip's kernel over the (segment, head) pairs of a batch launch; a, counters, nwg as for yume_attn8_launch
void yume_attn_batch8_launch(const AttnArgs& a, const AttnBatchSeg& sg, int* counters, int nwg, hipStream_t st);
