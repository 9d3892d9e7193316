// attn_band.hpp — attn_band_kernel: sliding-window / causal attention (yume_attn_fwd_band), the banded form of attn_fwd_kernel_v2.
// 4 waves, 128 queries per workgroup, two workgroups per CU, K / V^T tiles by LDS-DMA into two buffers, one barrier per tile, compiler
// scheduled with v2's sched_barrier ring (formulation and tile layouts: attn_tile.hpp; data movement: attn_fwd_v2.hpp).
//
// Row i of the call sits at pos(i) = q_pos0 + i on the key axis and sees the keys of attn_band_plan::visible. What differs from v2:
//   * a workgroup walks only the tiles t_lo ... t_hi that some row of its 128 sees (attn_band_plan::tile_range; the tile grid stays the global
//     one, so the DMA source alignment and both swizzles are v2's). An empty range stores zeros (nothing under accumulate);
//   * per wave, a tile outside the wave's own range is skipped (wave-uniform; the barrier is outside the body), a tile whose 64 keys are
//     all visible to all 32 rows takes tile_body_v2<false> unchanged, every other tile takes tile_body_band:
//   * there the mask goes onto the SCORES before the row maximum. v2's masked body may take the maximum over unmasked scores because its
//     hidden rows are clamped copies of a visible key; here a hidden key's score can lie arbitrarily far above every visible one, and as the
//     base it would flush the whole visible row to zero. P of a hidden key is set to 0 explicitly: while a row has seen no visible key its
//     m_run is still NEG_BIG and exp2(score - m_run) is not small;
//   * the deferred rescale is decided per lane, and a tile takes the unmasked body only once every row of the wave has seen a key: what a
//     row stores does not depend on the rows that share its wave (short of a score jump of more than 2^8 inside an interior tile, as in v2);
//   * a row that saw no key at all (l == 0) stores 0, never 0 / 0; under accumulate it is not touched (the old O survives bit for bit).
//   * the Q^T fragments are named as register operands in front of the LDS-DMA issue of every tile: where the allocator keeps some of them
//     in scratch (256 VGPRs, 100 bytes of scratch, occupancy 2), the reload is a vector-memory load behind the DMA's, and under the in-order
//     vmcnt the wait for it is a wait for the whole next tile — measured at twice the time per tile (profiles/r26_window_attn.md §3).
// A ragged last tile (Lk % 64 != 0) inside the range is register-staged as in v2. No weighted last key, no key-range split, no workspace.
#pragma once
#include "attn_fwd_v2.hpp"
#include "attn_band_plan.hpp"

static_assert(attn_band_plan::KTILE == KT && attn_band_plan::QBLOCK == QB && attn_band_plan::QWAVE == QW, "attn_band_plan.hpp restates the tile constants");

struct AttnBandArgs {
    AttnArgs a;
    attn_band_plan::Window w;
};

namespace {

// dma_tile with ONE per-thread source pointer per operand instead of v2's four: round rr of the K tile lies 16 rows further on, of the V^T tile
// 32 rows (both swizzles repeat with that period), so the other three are a uniform stride away — twelve registers less across the tile loop
struct DmaBand {
    const unsigned short* k;
    const unsigned short* v;
};
__device__ __forceinline__ void dma_tile_band(DmaBand& dp, int64_t k_round, int64_t v_round, int64_t kstep, char* buf, int wave) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
        __builtin_amdgcn_global_load_lds((gbl_cvoid_t*)(dp.k + rr * k_round), (lds_void_t*)(buf + rr * 4096 + wave * 1024), 16, 0, 0);
    dp.k += kstep;
    char* vb = buf + K_TILE_BYTES;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
        __builtin_amdgcn_global_load_lds((gbl_cvoid_t*)(dp.v + rr * v_round), (lds_void_t*)(vb + rr * 4096 + wave * 1024), 16, 0, 0);
    dp.v += KT;
}

// klo / khi: this lane's row sees the keys klo ... khi (already cut to [0, Lk - 1]; klo > khi: none). SINK (attn_fsink.hpp): and the keys
// below `send` as well, a second interval; without it the instances are the ones they were.
template <bool SINK = false>
__device__ __forceinline__ void tile_body_band(const char* kb, const AttnArgs& p, const bf16x8_t (&qf)[8], f32x16 (&oacc)[4], float& m_run,
                                               float& l_run, int j0, int ql, int hi, int klo, int khi, const int (&koff)[8], const int (&voff)[4],
                                               int send = 0) {
    const char* vb = kb + K_TILE_BYTES;
    f32x16 sacc[2];
    s_tile(kb, qf, sacc, koff);
    // the mask first: a hidden key takes no part in the row maximum
    const int kbase = j0 + 4 * hi;      // element r of half b is key kbase + 32 b + (r & 3) + 8 (r >> 2)
    unsigned vis = 0u;                  // bit 16 b + r: that key is visible to this lane's row
    float mx = NEG_BIG;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kbase + 32 * b + (r & 3) + 8 * (r >> 2);
            const bool v = (SINK && key < send) || (key >= klo && key <= khi);
            vis |= v ? (1u << (16 * b + r)) : 0u;
            mx = fmaxf(mx, v ? sacc[b][r] : NEG_BIG);
        }
    mx = xhalf_max(mx);
    // a row without a visible key so far keeps m_run == NEG_BIG == m_new: the difference is 0 and the deferred rescale does not fire on it
    const float m_new = fmaxf(m_run, mx > NEG_BIG ? mx * p.scale_log2 : NEG_BIG);
    // the deferred rescale PER LANE (v2 moves every lane of the wave when one has to move): the rows of a wave meet their first visible key
    // in different tiles here, and a row's bases must not depend on which rows share its wave — the trimmed last block of the engine runs
    // the same rows in other waves and has to give the same bits. A lane that stays is multiplied by exp2(0) = 1.
    const float m_tgt = (m_new - m_run <= DEFER_LOG2) ? m_run : m_new;
    if (!__all(m_tgt == m_run)) rescale_to(m_tgt, m_run, l_run, oacc);
    float psum = 0.f;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float pv = __builtin_amdgcn_exp2f(fmaf(sacc[b][r], p.scale_log2, -m_run));
            pv = (vis & (1u << (16 * b + r))) ? pv : 0.f;     // explicitly: exp2(score - NEG_BIG) is not small
            sacc[b][r] = pv;
            psum += pv;
        }
    l_run += psum;

    // ---- P^T fragments and O^T += V^T . P^T: as tile_body_v2 ----
    bf16x8_t pf[4];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            u32x4 w;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const unsigned ev = pack_bf16x2(sacc[b][8 * e + 2 * i], sacc[b][8 * e + 2 * i + 1]);
                const unsigned od = pack_bf16x2(sacc[b][8 * e + 4 + 2 * i], sacc[b][8 * e + 4 + 2 * i + 1]);
                const auto r = __builtin_amdgcn_permlane32_swap(ev, od, false, false);
                w[i] = r[0];
                w[2 + i] = r[1];
            }
            pf[2 * b + e] = __builtin_bit_cast(bf16x8_t, w);
        }
    __builtin_amdgcn_sched_barrier(0);
    bf16x8_t vf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) vf[i] = *reinterpret_cast<const bf16x8_t*>(vb + voff[i]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int db = i >> 2, sg = i & 3;
        oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[sg], pf[sg], oacc[db], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (i + 4 < 16) {
            vf[sg] = *reinterpret_cast<const bf16x8_t*>(vb + voff[sg] + (db + 1) * (32 * 128));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// store_o with the empty row: l == 0 stores 0 (the accumulators are 0), and nothing at all under accumulate
__device__ __forceinline__ void store_o_band(const AttnArgs& p, const f32x16 (&oacc)[4], float l_run, int h, int q0, int ql, int hi) {
    const float l_tot = xhalf_sum(l_run);
    const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
    const int q = q0 + ql;
    if (q < p.Lq && !(p.accumulate && !(l_tot > 0.f))) {
        unsigned short* op = p.O + (int64_t)q * p.ldo + h * D + 4 * hi;
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float v0 = oacc[db][4 * g + 0] * inv, v1 = oacc[db][4 * g + 1] * inv;
                float v2 = oacc[db][4 * g + 2] * inv, v3 = oacc[db][4 * g + 3] * inv;
                u32x2* dst = reinterpret_cast<u32x2*>(op + 32 * db + 8 * g);
                if (p.accumulate) {
                    const u32x2 old = *dst;
                    v0 += bf16_to_f32((unsigned short)(old[0] & 0xffffu));
                    v1 += bf16_to_f32((unsigned short)(old[0] >> 16));
                    v2 += bf16_to_f32((unsigned short)(old[1] & 0xffffu));
                    v3 += bf16_to_f32((unsigned short)(old[1] >> 16));
                }
                u32x2 o;
                o[0] = pack_bf16x2(v0, v1);
                o[1] = pack_bf16x2(v2, v3);
                *dst = o;
            }
    }
}

__global__ __launch_bounds__(NW * 64, 2) void attn_band_kernel(AttnBandArgs args) {
    __shared__ __attribute__((aligned(16))) char smem[2 * V2_BUF];
    const AttnArgs& p = args.a;
    const attn_band_plan::Window win = args.w;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5;
    const int ql = lane & 31;
    YUME_ATTN_BLOCK_HEAD_QB(p, h, qb)
    const int q0 = p.q_lo + qb * QB + wave * QW;
    const int q_end = p.Lq - 1;                                   // rows >= Lq are clamped copies of the last row (load_q_frags) and never stored
    auto cut = [&](int q) { return q < q_end ? q : q_end; };

    // the workgroup's tiles (uniform), then this wave's own
    const attn_band_plan::TileRange wg = attn_band_plan::tile_range(p.q_lo + qb * QB, cut(p.q_lo + qb * QB + QB - 1), p.Lk, win);
    f32x16 oacc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) oacc[i] = zero_acc();
    float m_run = NEG_BIG, l_run = 0.f;
    if (wg.lo > wg.hi) {            // no row of the workgroup sees a key: zeros (before any barrier; uniform)
        store_o_band(p, oacc, l_run, h, q0, ql, hi);
        return;
    }
    const int t0 = (int)wg.lo, t1 = (int)wg.hi + 1;
    const int wq0 = cut(q0), wq1 = cut(q0 + QW - 1);
    const attn_band_plan::TileRange wv = attn_band_plan::tile_range(wq0, wq1, p.Lk, win);
    const int wt_lo = __builtin_amdgcn_readfirstlane((int)wv.lo), wt_hi = __builtin_amdgcn_readfirstlane((int)wv.hi);
    // this lane's row
    const attn_band_plan::KeyRange kr = attn_band_plan::key_range(cut(q0 + ql), cut(q0 + ql), p.Lk, win);
    const int klo = (int)kr.lo, khi = (int)kr.hi;

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
        // the Q^T fragments in registers BEFORE the DMA is issued: where the register allocator keeps some of them in scratch, their reload is a
        // vector-memory load like the DMA's, and a wait for it behind the DMA issue is a wait for the whole next tile (measured: twice the
        // time per tile, profiles/r26_window_attn.md)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) asm volatile("" : "+v"(qf[ks]));
        if (has_next && !next_reg) dma_tile_band(dp, k_round, v_round, kstep, nb, wave);
        if (t >= wt_lo && t <= wt_hi) {
            // (the unmasked body only once every row of the wave has a base: its wave-wide rescale would otherwise carry the rows that are
            // under way along with a row that starts here)
            if (attn_band_plan::tile_is_interior(t, wq0, wq1, p.Lk, win) && __all(m_run > NEG_BIG))
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

namespace attn_band {

static inline void launch(const AttnArgs& a, const attn_band_plan::Window& w, hipStream_t st) {
    AttnBandArgs b{whole_blocks(a, QB), w};
    hipLaunchKernelGGL(attn_band_kernel, xcd_grid(b.a), dim3(NW * 64), 0, st, b);
}

}  // namespace attn_band
