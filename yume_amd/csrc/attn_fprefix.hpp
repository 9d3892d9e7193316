// attn_fprefix.hpp — attn_fprefix_kernel: frame-window attention over two key buffers (yume_attn_fwd_fprefix): a prefix of n_prefix keys
// that every row sees, read from Kp / Vtp with their own strides, then a suffix under the frame window, read from K / Vt. It is
// attn_fsink_kernel with the sink living in another buffer: the same pieces of attn_band.hpp (dma_tile_band, tile_body_band<true>,
// store_o_band, tile_body_v2<false>) under the same walk over a tile LIST; attn_band_kernel, attn_fband_kernel and attn_fsink_kernel are not
// touched.
//
// The kernel works in the PADDED coordinate of attn_fprefix_plan.hpp: prefix tile t (t < np) holds the prefix keys 64 t ..., suffix tile s
// sits at tile np + s and its keys at P + 64 s ..., P = 64 np. There a row sees [0, n_prefix) ∪ [P + klo(i), P + khi(i)], which is
// tile_body_band<true>'s predicate with send = n_prefix; the pad n_prefix ... P - 1 of a ragged last prefix tile lies in neither interval.
// What differs from attn_fsink_kernel:
//   * the list is the prefix tiles [0, np) then the suffix's band tiles [np + t_lo, np + t_hi]; at the step from np - 1 to the first suffix
//     tile the LDS-DMA prefetch does not advance its pointers but SWITCHES them: base, row strides and tile steps become the suffix's;
//   * each segment may end in a ragged tile (n_prefix % 64, Lk % 64). Either takes the register path (stage_load / stage_store_v2) with its own
//     segment's pointers and key bound, whenever it is the next of the list: rows behind n_prefix of Kp and behind Lk of K are never read,
//     the V^T columns behind them are zeroed in registers, and the mask hides them;
//   * n_prefix >= 1 (the host forwards n_prefix == 0 to yume_attn_fwd_fband), so the list is never empty and every row has a base after
//     tile 0.
// The Q^T fragments and the lane-half index are named as register operands in front of every DMA issue, also the one across the switch.
#pragma once
#include "attn_band.hpp"
#include "attn_fprefix_plan.hpp"

struct AttnFPrefixArgs {
    AttnArgs a;                       // K / Vt / ldk / ldvt / Lk: the suffix
    attn_fband_plan::Plan w;          // the suffix's partition and window
    const unsigned short* Kp; int64_t ldkp;
    const unsigned short* Vtp; int64_t ldvtp;
    int32_t n_prefix;
};

namespace {

__global__ __launch_bounds__(NW * 64, 2) void attn_fprefix_kernel(AttnFPrefixArgs args) {
    __shared__ __attribute__((aligned(16))) char smem[2 * V2_BUF];
    const AttnArgs& p = args.a;
    const attn_fband_plan::Plan& plan = args.w;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int hi = lane >> 5;
    const int ql = lane & 31;
    YUME_ATTN_BLOCK_HEAD_QB(p, h, qb)
    const int q0 = p.q_lo + qb * QB + wave * QW;
    const int q_end = p.Lq - 1;                                   // rows >= Lq are clamped copies of the last row (load_q_frags) and never stored
    auto cut = [&](int q) { return q < q_end ? q : q_end; };

    // the workgroup's tile list in padded tiles (uniform); n_prefix >= 1: never empty
    const int send = args.n_prefix;
    const attn_fsink_plan::TileList wg = attn_fprefix_plan::tile_list(p.q_lo + qb * QB, cut(p.q_lo + qb * QB + QB - 1), p.Lk, plan, send);
    const int np = (int)wg.n_sink, b_lo = (int)wg.b_lo, t_last = (int)wg.b_hi;
    const int P = np * KT;
    f32x16 oacc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) oacc[i] = zero_acc();
    float m_run = NEG_BIG, l_run = 0.f;
    // this lane's row (lanes l and l + 32 hold the same row): its suffix interval, shifted by P; then the wave's own suffix tiles from its
    // first and its last row
    const attn_fband_plan::KeyRange kr = attn_fband_plan::key_range(cut(q0 + ql), cut(q0 + ql), p.Lk, plan);
    const int klo = P + (int)kr.lo, khi = P + (int)kr.hi;
    const int klo_first = __builtin_amdgcn_readfirstlane(klo), khi_first = __builtin_amdgcn_readfirstlane(khi);
    const int klo_last = __builtin_amdgcn_readlane(klo, QW - 1), khi_last = __builtin_amdgcn_readlane(khi, QW - 1);
    const bool wave_sees = klo_first <= khi_last;
    const int wt_lo = wave_sees ? klo_first / KT : 0, wt_hi = wave_sees ? khi_last / KT : -1;
    // the tiles whose 64 coordinates every row of the wave sees: whole prefix tiles, or inside every row's suffix interval (khi <= P + Lk - 1)
    const int is_hi = send / KT - 1;
    const int it_lo = (klo_last + KT - 1) / KT, it_hi = (khi_first + 1) / KT - 1;

    bf16x8_t qf[8];
    load_q_frags(p, h, q0, ql, hi, qf);
    int koff[8], voff[4];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) koff[ks] = k_frag_offset(ks, ql, hi);
#pragma unroll
    for (int sg = 0; sg < 4; ++sg) voff[sg] = v_frag_offset(sg, ql, hi);
    // the ragged last tile of either segment, as a padded tile (-1: none), takes the register path
    const int p_reg = (send % KT) != 0 ? np - 1 : -1;
    const int s_reg = (p.Lk % KT) != 0 ? np + (p.Lk + KT - 1) / KT - 1 : -1;
    // the register path of padded tile t into buf: stage_load with the segment's own pointers, strides and key bound
    auto stage = [&](int t, char* buf) {
        Stage st;
        if (t < np) {
            AttnArgs pp = p;
            pp.K = args.Kp; pp.ldk = args.ldkp; pp.Vt = args.Vtp; pp.ldvt = args.ldvtp; pp.Lk = send;
            stage_load(st, pp, h, t * KT, tid);
        } else {
            stage_load(st, p, h, (t - np) * KT, tid);
        }
        stage_store_v2(st, buf, tid);
    };
    // the DMA state starts on the prefix: round 0 of dma_init's pointers (K row tid >> 4, V^T row tid >> 3, each with its swizzled chunk)
    const int k_lane = h * D + (((tid & 15) ^ ((tid >> 4) & 15)) << 3), v_lane = ((tid & 7) ^ ((tid >> 4) & 7)) << 3;
    int64_t kstep = (int64_t)KT * args.ldkp, k_round = 16 * args.ldkp, v_round = 32 * args.ldvtp;
    DmaBand dp;
    dp.k = args.Kp + (int64_t)(tid >> 4) * args.ldkp + k_lane;
    dp.v = args.Vtp + (int64_t)(h * D + (tid >> 3)) * args.ldvtp + v_lane;
    if (p_reg == 0) stage(0, smem);
    else dma_tile_band(dp, k_round, v_round, kstep, smem, wave);      // (the pointers now stand at prefix tile 1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    int cur = 0;
    for (int t = 0; t <= t_last;) {
        char* kb = smem + cur * V2_BUF;
        char* nb = smem + (cur ^ 1) * V2_BUF;
        const int tn = t + 1 == np ? b_lo : t + 1;          // attn_fsink_plan::next_tile
        const bool has_next = tn <= t_last;
        const bool next_reg = has_next && (tn == p_reg || tn == s_reg);
        // the Q^T fragments in registers BEFORE the DMA is issued (attn_band.hpp: a scratch reload behind the issue waits for the whole tile)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) asm volatile("" : "+v"(qf[ks]));
        asm volatile("" : "+v"(hi));      // and the lane's half, which the masked body's key index starts from
        if (has_next && !next_reg) {
            if (t + 1 == np) {          // the switch: the next tile is suffix tile tn - np, in the other buffer with the other strides
                kstep = (int64_t)KT * p.ldk;
                k_round = 16 * p.ldk;
                v_round = 32 * p.ldvt;
                dp.k = p.K + (int64_t)(tid >> 4) * p.ldk + k_lane + (int64_t)(tn - np) * kstep;
                dp.v = p.Vt + (int64_t)(h * D + (tid >> 3)) * p.ldvt + v_lane + (int64_t)(tn - np) * KT;
            }
            dma_tile_band(dp, k_round, v_round, kstep, nb, wave);
        }
        if (t < np || (t >= wt_lo && t <= wt_hi)) {
            if ((t <= is_hi || (t >= it_lo && t <= it_hi)) && __all(m_run > NEG_BIG))
                tile_body_v2<false>(kb, p, qf, oacc, m_run, l_run, t * KT, ql, hi, koff, voff);
            else
                tile_body_band<true>(kb, p, qf, oacc, m_run, l_run, t * KT, ql, hi, klo, khi, koff, voff, send);
        }
        if (next_reg) stage(tn, nb);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        cur ^= 1;
        t = tn;
    }
    store_o_band(p, oacc, l_run, h, q0, ql, hi);
}

}  // namespace

namespace attn_fprefix {

static inline void launch(const AttnArgs& a, const attn_fband_plan::Plan& w, const void* Kp, int64_t ldkp, const void* Vtp, int64_t ldvtp,
                          int64_t n_prefix, hipStream_t st) {
    AttnFPrefixArgs b{whole_blocks(a, QB), w, (const unsigned short*)Kp, ldkp, (const unsigned short*)Vtp, ldvtp, (int32_t)n_prefix};
    hipLaunchKernelGGL(attn_fprefix_kernel, xcd_grid(b.a), dim3(NW * 64), 0, st, b);
}

}  // namespace attn_fprefix
