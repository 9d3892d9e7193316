// attn_fband.hpp — attn_fband_kernel: frame-window / frame-causal attention over a block partition of the key axis (yume_attn_fwd_fband).
// attn_band_kernel's walk (attn_band.hpp) with the interval source exchanged: its tile body, DMA issue, ragged last tile and O store are the
// ones of that file, called from here; attn_band_kernel itself is not touched.
//
// Row i of the call sits at pos(i) = q_pos0 + i and sees the keys klo(i) ... khi(i) of attn_fband_plan::key_range: every key of the blocks
// (frames) within `back` blocks before and `ahead` blocks after its own. What differs from attn_band_kernel:
//   * in the prologue each lane finds its row's block and from it klo / khi (at most 16 span compares and one integer division, once, the
//     partition read from the kernel arguments); the wave takes its tile range from its first row's klo and its last row's khi (both ends
//     are non-decreasing in the row), the workgroup likewise;
//   * a tile takes the unmasked body when it lies inside [klo(last row of the wave), khi(first row of the wave)] — two wave-uniform tile
//     indices worked out before the loop, two scalar compares in it — and every row of the wave has a base (the per-lane deferred rescale rule
//     of attn_band.hpp, kept for the same reason: the trimmed last block runs the same rows in other waves and has to give the same bits).
// Everything else — the mask before the row maximum, P of a hidden key 0, the empty row, the Q^T fragments named as register operands in
// front of the LDS-DMA issue — is attn_band.hpp's. With one span of one-row blocks the intervals, the tile ranges and the interior tiles are
// attn_band_kernel's for left = back, right = ahead, and so are the bits.
#pragma once
#include "attn_band.hpp"
#include "attn_fband_plan.hpp"

static_assert(attn_fband_plan::KTILE == KT && attn_fband_plan::QBLOCK == QB && attn_fband_plan::QWAVE == QW, "attn_fband_plan.hpp restates the tile constants");

struct AttnFBandArgs {
    AttnArgs a;
    attn_fband_plan::Plan w;
};

namespace {

__global__ __launch_bounds__(NW * 64, 2) void attn_fband_kernel(AttnFBandArgs args) {
    __shared__ __attribute__((aligned(16))) char smem[2 * V2_BUF];
    const AttnArgs& p = args.a;
    const attn_fband_plan::Plan& plan = args.w;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5;
    const int ql = lane & 31;
    YUME_ATTN_BLOCK_HEAD_QB(p, h, qb)
    const int q0 = p.q_lo + qb * QB + wave * QW;
    const int q_end = p.Lq - 1;                                   // rows >= Lq are clamped copies of the last row (load_q_frags) and never stored
    auto cut = [&](int q) { return q < q_end ? q : q_end; };

    // the workgroup's tiles (uniform)
    const attn_fband_plan::TileRange wg = attn_fband_plan::tile_range(p.q_lo + qb * QB, cut(p.q_lo + qb * QB + QB - 1), p.Lk, plan);
    f32x16 oacc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) oacc[i] = zero_acc();
    float m_run = NEG_BIG, l_run = 0.f;
    if (wg.lo > wg.hi) {            // no row of the workgroup sees a key: zeros (before any barrier; uniform)
        store_o_band(p, oacc, l_run, h, q0, ql, hi);
        return;
    }
    const int t0 = (int)wg.lo, t1 = (int)wg.hi + 1;
    // this lane's row (lanes l and l + 32 hold the same row), then the wave's own tiles from its first and its last row
    const attn_fband_plan::KeyRange kr = attn_fband_plan::key_range(cut(q0 + ql), cut(q0 + ql), p.Lk, plan);
    const int klo = (int)kr.lo, khi = (int)kr.hi;
    const int klo_first = __builtin_amdgcn_readfirstlane(klo), khi_first = __builtin_amdgcn_readfirstlane(khi);
    const int klo_last = __builtin_amdgcn_readlane(klo, QW - 1), khi_last = __builtin_amdgcn_readlane(khi, QW - 1);
    const bool wave_sees = klo_first <= khi_last;
    const int wt_lo = wave_sees ? klo_first / KT : 0, wt_hi = wave_sees ? khi_last / KT : -1;
    // the tiles whose 64 keys every row of the wave sees (khi <= Lk - 1: such a tile lies below Lk); none: it_lo > it_hi
    const int it_lo = (klo_last + KT - 1) / KT, it_hi = (khi_first + 1) / KT - 1;

    bf16x8_t qf[8];
    load_q_frags(p, h, q0, ql, hi, qf);
    int koff[8], voff[4];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) koff[ks] = k_frag_offset(ks, ql, hi);
#pragma unroll
    for (int sg = 0; sg < 4; ++sg) voff[sg] = v_frag_offset(sg, ql, hi);
    const int64_t kstep = (int64_t)KT * p.ldk, k_round = 16 * p.ldk, v_round = 32 * p.ldvt;
    DmaBand dp;        // round 0 of dma_init's pointers: K row tid >> 4, V^T row tid >> 3, each with its swizzled chunk
    dp.k = p.K + (int64_t)(tid >> 4) * p.ldk + h * D + (((tid & 15) ^ ((tid >> 4) & 15)) << 3);
    dp.v = p.Vt + (int64_t)(h * D + (tid >> 3)) * p.ldvt + (((tid & 7) ^ ((tid >> 4) & 7)) << 3);
    const int nt = (p.Lk + KT - 1) / KT;
    const bool ragged = (p.Lk % KT) != 0;          // then the LAST tile of the key axis takes the register path
    dp.k += (int64_t)t0 * kstep;
    dp.v += (int64_t)t0 * KT;
    if (t0 == nt - 1 && ragged) {
        Stage st;
        stage_load(st, p, h, t0 * KT, tid);
        stage_store_v2(st, smem, tid);
    } else {
        dma_tile_band(dp, k_round, v_round, kstep, smem, wave);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    int cur = 0;
    for (int t = t0; t < t1; ++t) {
        char* kb = smem + cur * V2_BUF;
        char* nb = smem + (cur ^ 1) * V2_BUF;
        const bool has_next = t + 1 < t1;
        const bool next_reg = has_next && ragged && (t + 2 == nt);
        // the Q^T fragments in registers BEFORE the DMA is issued (attn_band.hpp: a scratch reload behind the issue waits for the whole tile)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) asm volatile("" : "+v"(qf[ks]));
        if (has_next && !next_reg) dma_tile_band(dp, k_round, v_round, kstep, nb, wave);
        if (t >= wt_lo && t <= wt_hi) {
            if (t >= it_lo && t <= it_hi && __all(m_run > NEG_BIG))
                tile_body_v2<false>(kb, p, qf, oacc, m_run, l_run, t * KT, ql, hi, koff, voff);
            else
                tile_body_band(kb, p, qf, oacc, m_run, l_run, t * KT, ql, hi, klo, khi, koff, voff);
        }
        if (next_reg) {
            Stage st;
            stage_load(st, p, h, (t + 1) * KT, tid);
            stage_store_v2(st, nb, tid);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        cur ^= 1;
    }
    store_o_band(p, oacc, l_run, h, q0, ql, hi);
}

}  // namespace

namespace attn_fband {

static inline void launch(const AttnArgs& a, const attn_fband_plan::Plan& w, hipStream_t st) {
    AttnFBandArgs b{whole_blocks(a, QB), w};
    hipLaunchKernelGGL(attn_fband_kernel, xcd_grid(b.a), dim3(NW * 64), 0, st, b);
}

}  // namespace attn_fband
