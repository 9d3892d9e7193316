// attn_fsink.hpp — attn_fsink_kernel: frame-window attention with an always-visible sink of leading frames (yume_attn_fwd_fsink).
// attn_fband_kernel's prologue and attn_band.hpp's pieces (dma_tile_band, tile_body_band, store_o_band, tile_body_v2<false>) under another
// walk; attn_band_kernel and attn_fband_kernel are not touched.
//
// Row i sees [0, send) ∪ [klo(i), khi(i)] (attn_fsink_plan.hpp: send the end of the sink, the same for every row; klo / khi the frame
// window's). What differs from attn_fband_kernel:
//   * the workgroup walks a LIST of tiles, not a range: the sink tiles [0, n_sink), then the band tiles [b_lo, b_hi] behind them
//     (attn_fsink_plan::tile_list) — one run where the two meet or overlap (no tile loaded or summed twice), two with a jump otherwise. The
//     loop steps with next_tile, and the double-buffered prefetch takes the NEXT TILE OF THE LIST: across the jump the DmaBand pointers
//     advance by the tiles skipped. The ragged last tile of the key axis takes the register path whenever it is the next of the list — also
//     as a sink tile, where Lk cuts the sink;
//   * a wave walks the sink tiles and its own rows' band tiles, and skips the rest (wave-uniform; the barrier is outside the body);
//   * the masked body is tile_body_band<true>: key < send || (klo <= key <= khi) on the scores before the row maximum, P of a hidden key 0,
//     the per-lane deferred rescale as it is;
//   * a tile takes the unmasked body when all of it lies below send, or inside [klo(last row of the wave), khi(first row)], and every row
//     of the wave has a base (attn_band.hpp's rule, for its reason: with a sink every row has one after the first tile).
// The Q^T fragments are named as register operands in front of every DMA issue, also the one across the jump.
#pragma once
#include "attn_band.hpp"
#include "attn_fsink_plan.hpp"

struct AttnFSinkArgs {
    AttnArgs a;
    attn_fband_plan::Plan w;
    int32_t sink;
};

namespace {

__global__ __launch_bounds__(NW * 64, 2) void attn_fsink_kernel(AttnFSinkArgs args) {
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

    // the workgroup's tile list (uniform)
    const attn_fsink_plan::TileList wg = attn_fsink_plan::tile_list(p.q_lo + qb * QB, cut(p.q_lo + qb * QB + QB - 1), p.Lk, plan, args.sink);
    const int send = (int)attn_fsink_plan::send(p.Lk, plan, args.sink);
    f32x16 oacc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) oacc[i] = zero_acc();
    float m_run = NEG_BIG, l_run = 0.f;
    if (wg.b_hi < 0) {              // no row of the workgroup sees a key: zeros (before any barrier; uniform)
        store_o_band(p, oacc, l_run, h, q0, ql, hi);
        return;
    }
    const int n_sink = (int)wg.n_sink, b_lo = (int)wg.b_lo, t_last = (int)wg.b_hi;
    const int t0 = n_sink > 0 ? 0 : b_lo;
    // this lane's row (lanes l and l + 32 hold the same row), then the wave's own band tiles from its first and its last row
    const attn_fband_plan::KeyRange kr = attn_fband_plan::key_range(cut(q0 + ql), cut(q0 + ql), p.Lk, plan);
    const int klo = (int)kr.lo, khi = (int)kr.hi;
    const int klo_first = __builtin_amdgcn_readfirstlane(klo), khi_first = __builtin_amdgcn_readfirstlane(khi);
    const int klo_last = __builtin_amdgcn_readlane(klo, QW - 1), khi_last = __builtin_amdgcn_readlane(khi, QW - 1);
    const bool wave_sees = klo_first <= khi_last;
    const int wt_lo = wave_sees ? klo_first / KT : 0, wt_hi = wave_sees ? khi_last / KT : -1;
    // the tiles whose 64 keys every row of the wave sees: below send (send <= Lk), or inside every row's interval (khi <= Lk - 1)
    const int is_hi = send / KT - 1;
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
    const bool ragged = (p.Lk % KT) != 0;          // then the LAST tile of the key axis takes the register path (the list ascends: it is the list's last)
    dp.k += (int64_t)t0 * kstep;
    dp.v += (int64_t)t0 * KT;
    if (t0 == nt - 1 && ragged) {
        Stage st;
        stage_load(st, p, h, t0 * KT, tid);
        stage_store_v2(st, smem, tid);
    } else {
        dma_tile_band(dp, k_round, v_round, kstep, smem, wave);      // (the pointers now stand at tile t0 + 1)
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    int cur = 0;
    for (int t = t0; t <= t_last;) {
        char* kb = smem + cur * V2_BUF;
        char* nb = smem + (cur ^ 1) * V2_BUF;
        const int tn = t + 1 == n_sink ? b_lo : t + 1;      // attn_fsink_plan::next_tile
        const bool has_next = tn <= t_last;
        const bool next_reg = has_next && ragged && (tn == nt - 1);
        // the Q^T fragments in registers BEFORE the DMA is issued (attn_band.hpp: a scratch reload behind the issue waits for the whole tile)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) asm volatile("" : "+v"(qf[ks]));
        asm volatile("" : "+v"(hi));      // and the lane's half, which the masked body's key index starts from
        if (has_next && !next_reg) {
            if (tn != t + 1) {          // the jump: the pointers stand at t + 1
                dp.k += (int64_t)(tn - t - 1) * kstep;
                dp.v += (int64_t)(tn - t - 1) * KT;
            }
            dma_tile_band(dp, k_round, v_round, kstep, nb, wave);
        }
        if (t < n_sink || (t >= wt_lo && t <= wt_hi)) {
            if ((t <= is_hi || (t >= it_lo && t <= it_hi)) && __all(m_run > NEG_BIG))
                tile_body_v2<false>(kb, p, qf, oacc, m_run, l_run, t * KT, ql, hi, koff, voff);
            else
                tile_body_band<true>(kb, p, qf, oacc, m_run, l_run, t * KT, ql, hi, klo, khi, koff, voff, send);
        }
        if (next_reg) {
            Stage st;
            stage_load(st, p, h, tn * KT, tid);
            stage_store_v2(st, nb, tid);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        cur ^= 1;
        t = tn;
    }
    store_o_band(p, oacc, l_run, h, q0, ql, hi);
}

}  // namespace

namespace attn_fsink {

static inline void launch(const AttnArgs& a, const attn_fband_plan::Plan& w, int64_t sink, hipStream_t st) {
    AttnFSinkArgs b{whole_blocks(a, QB), w, (int32_t)sink};
    hipLaunchKernelGGL(attn_fsink_kernel, xcd_grid(b.a), dim3(NW * 64), 0, st, b);
}

}  // namespace attn_fsink
