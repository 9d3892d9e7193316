// attn_seg.hpp — SEGMENTED cross-attention (r9, yume_attn_fwd_seg): ONE launch serves nseg (2 .. 8) independent segments. Segment s owns the
// query rows [s * seg_pitch, s * seg_pitch + Lq_seg) of Q and O and attends over its own K[s] / Vt[s] with its own key count Lk[s] and its
// own last-key weight. It serves the text cross-attention of a guided (classifier-free guidance) forward whose two legs are stacked rows
// (DiTEngine.forward_pair): the legs share everything but the prompt, and with dedup_pad_keys each prompt has its own n + 1 keys and weight.
// The rows of the pitch gap [s * seg_pitch + Lq_seg, (s + 1) * seg_pitch) are neither read nor written.
//
// Two kernels, both the segmented form of an existing one (the arithmetic per query row is that kernel's, in the same order):
//   attn_short_seg_kernel<NKB>  attn_short.hpp's design (a head's K and V^T resident in ONE wave's registers, exact single-pass softmax, no LDS).
//                               Units are ordered (segment, head, 32-query block); K / V^T are reloaded when the segment OR the head changes (with
//                               H == 1 the head alone never does). NKB = max over the segments of ceil(Lk[s] / 32), so a segment with fewer keys
//                               has WHOLE key blocks masked: every key block is masked against Lk[s], every V^T chunk is zeroed behind
//                               Lk[s], and the weighted key is looked for in every block (attn_short.hpp looks at the last block only).
//   attn_seg_kernel_v2          attn_fwd_kernel_v2<true> (4 waves, 128 queries, K / V^T tiles by LDS-DMA) for any Lk[s]. Query blocks are
//                               counted per segment — a 128-query block never straddles two segments — and the workgroup builds its
//                               segment's AttnArgs once, uniformly, then walks the key tiles with attn_fwd_v2.hpp's own pieces. It is a copy of
//                               that kernel's tile loop (without its unused key-range split), not a shared function: attn_fwd_kernel_v2's
//                               generated code is held fixed, and moving its body behind a call changes it (attn_tile.hpp). The last tile
//                               always takes the masked, weighted body (a weight of 1 multiplies by 1: the same bits).
// The arrays travel BY VALUE in AttnSegArgs (kernel arguments; a captured graph needs no device memory for them). No workspace.
// Resource usage (-Rpass-analysis=kernel-resource-usage): profiles/r9_forward_cfg.md; scratch 0 in every instance.
#pragma once
#include "attn_fwd_v2.hpp"
#include "attn_short.hpp"

constexpr int ATTN_SEG_MAX = 8;

struct AttnSegArgs {
    const unsigned short* Q; int64_t ldq;
    const unsigned short* K[ATTN_SEG_MAX]; int64_t ldk;
    const unsigned short* Vt[ATTN_SEG_MAX]; int64_t ldvt;
    unsigned short* O; int64_t ldo;
    int Lk[ATTN_SEG_MAX];
    float last_w[ATTN_SEG_MAX];      // key Lk[s] - 1 of segment s counts last_w[s] times (1: an ordinary key)
    int nseg, Lq_seg, seg_pitch, H;
    float scale_log2;                // softmax scale * log2(e); exactly 1 when Q is prescaled
    int accumulate;
    int nqb_seg;                     // query blocks per (segment, head)
    int nqb;                         // nseg * nqb_seg: what YUME_ATTN_BLOCK_HEAD_QB spreads over the XCDs
};

namespace attn_seg {

constexpr int HD = attn_short::HD, QB32 = attn_short::QB;

template <int NKB>
__global__ __launch_bounds__(256, 1) void attn_short_seg_kernel(AttnSegArgs p, int nunit) {
    constexpr int NST = 2 * NKB;                                                  // 16-key steps
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ql = lane & 31, hh = lane >> 5;
    // this wave's units [u0, u1) of the (segment, head, query block) order
    const int nwave = (int)gridDim.x * 4, gw = (int)blockIdx.x * 4 + wave;
    const int u0 = (int)(((int64_t)gw * nunit) / nwave), u1 = (int)(((int64_t)(gw + 1) * nunit) / nwave);
    if (u0 >= u1) return;
    const int pm = (ql & 0x13) | ((ql & 4) << 1) | ((ql & 8) >> 1);              // MFMA row ql -> key / feature ql with bits 2 and 3 exchanged
    const int nqb = p.nqb_seg;

    bf16x8_t kf[NKB][8], vf[4][NST];
    int cur = -1;                                                                 // (segment, head) whose K / V^T the registers hold
    int Lk = 0;
    float last_w = 1.f;
    auto load_q = [&](int u, bf16x8_t (&qf)[8]) {
        const int sh = u / nqb, qb = u - sh * nqb;
        const int sg = sh / p.H, h = sh - sg * p.H;
        int q = qb * QB32 + ql;
        q = q < p.Lq_seg ? q : p.Lq_seg - 1;                                      // (a ragged last block stays inside its segment)
        const unsigned short* qp = p.Q + ((int64_t)sg * p.seg_pitch + q) * p.ldq + h * HD + 8 * hh;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const bf16x8_t*>(qp + 16 * ks);
    };
    bf16x8_t qf[8];
    load_q(u0, qf);

    for (int u = u0; u < u1; ++u) {
        const int sh = u / nqb, qb = u - sh * nqb;                                // sh = segment * H + head
        const int sg = sh / p.H, h = sh - sg * p.H;
        if (sh != cur) {                                                          // (uniform) this segment's keys of this head
            cur = sh;
            Lk = p.Lk[sg];
            last_w = p.last_w[sg];
            const unsigned short* Kp = p.K[sg];
            const unsigned short* Vp = p.Vt[sg];
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                int key = 32 * kb + pm;
                key = key < Lk ? key : Lk - 1;                                    // (rows beyond Lk: masked below)
                const unsigned short* kp = Kp + (int64_t)key * p.ldk + h * HD + 8 * hh;
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) kf[kb][ks] = *reinterpret_cast<const bf16x8_t*>(kp + 16 * ks);
            }
            const int kmax = (int)p.ldvt - 8;
#pragma unroll
            for (int st = 0; st < NST; ++st) {
                const int kc = 16 * st + 8 * hh;                                  // first key of this lane's chunk
                const int kload = kc < kmax ? kc : kmax;                          // keep the 16-byte load inside the row
                const int nvalid = (kload == kc) ? max(Lk - kc, 0) : 0;
#pragma unroll
                for (int db = 0; db < 4; ++db) {
                    u32x4 x = *reinterpret_cast<const u32x4*>(Vp + (int64_t)(h * HD + 32 * db + pm) * p.ldvt + kload);
                    if (nvalid < 8) {                                             // (any chunk can lie behind this segment's Lk: exact zeros)
#pragma unroll
                        for (int w = 0; w < 4; ++w) {
                            if (2 * w >= nvalid) x[w] = 0u;
                            else if (2 * w + 1 >= nvalid) x[w] &= 0xffffu;
                        }
                    }
                    vf[db][st] = __builtin_bit_cast(bf16x8_t, x);
                }
            }
        }
        // ---- S^T = K Q^T: NKB key blocks x 8 k-steps (the accumulators alternate)
        f32x16 s[NKB];
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kb][ks], qf[ks], s[kb], 0, 0, 0);
        if (u + 1 < u1) load_q(u + 1, qf);                                       // next unit's Q, one unit ahead
        // ---- the row's maximum over ALL its keys (lane-local + the partner half); every key block is masked against the segment's Lk
        float mx = -3.0e38f;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * kb + 16 * (r >> 3) + 8 * hh + (r & 7);
                const float x = key < Lk ? s[kb][r] * p.scale_log2 : -3.0e38f;
                s[kb][r] = x;
                mx = fmaxf(mx, x);
            }
        mx = attn_short::xhalf_max(mx);
        // ---- exponentials, row sum, P^T fragments: the accumulator's own order (a masked key's exponential is an exact 0)
        float lsum = 0.f;
        bf16x8_t pf[NST];
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                float ex[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float v = __builtin_amdgcn_exp2f(s[kb][8 * e + j] - mx);
                    const int key = 32 * kb + 16 * e + 8 * hh + j;
                    v = key == Lk - 1 ? v * last_w : v;                           // the key that stands for last_w keys
                    ex[j] = v;
                    lsum += v;
                }
                u32x4 w;
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = pack_bf16x2(ex[2 * j], ex[2 * j + 1]);
                pf[2 * kb + e] = __builtin_bit_cast(bf16x8_t, w);
            }
        lsum = attn_short::xhalf_sum(lsum);
        // ---- O^T = V^T P^T: 4 d-blocks x NST key steps, complete in the wave
        f32x16 o[4];
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
#pragma unroll
        for (int st = 0; st < NST; ++st)
#pragma unroll
            for (int db = 0; db < 4; ++db) o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[db][st], pf[st], o[db], 0, 0, 0);
        const float inv = 1.0f / lsum;
        const int q = qb * QB32 + ql;
        if (q < p.Lq_seg) {                                                       // (never the next segment's rows, nor the pitch gap)
            unsigned short* op = p.O + ((int64_t)sg * p.seg_pitch + q) * p.ldo + h * HD + 8 * hh;
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = o[db][8 * e + j] * inv;
                    u32x4* dst = reinterpret_cast<u32x4*>(op + 32 * db + 16 * e);
                    if (p.accumulate) {
                        const u32x4 old = *dst;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            v[2 * j] += bf16_to_f32((unsigned short)(old[j] & 0xffffu));
                            v[2 * j + 1] += bf16_to_f32((unsigned short)(old[j] >> 16));
                        }
                    }
                    u32x4 ov;
#pragma unroll
                    for (int j = 0; j < 4; ++j) ov[j] = pack_bf16x2(v[2 * j], v[2 * j + 1]);
                    *dst = ov;
                }
        }
    }
}

__global__ __launch_bounds__(NW * 64, 2) void attn_seg_kernel_v2(AttnSegArgs p) {
    __shared__ __attribute__((aligned(16))) char smem[2 * V2_BUF];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5;
    const int ql = lane & 31;
    YUME_ATTN_BLOCK_HEAD_QB(p, h, qbs)                                            // qbs = segment * nqb_seg + the segment's query block
    const int sg = qbs / p.nqb_seg, qb = qbs - sg * p.nqb_seg;
    // the segment as a problem of its own (uniform): every piece below is attn_fwd_v2.hpp's, reading these
    AttnArgs a;
    a.Q = p.Q + (int64_t)sg * p.seg_pitch * p.ldq; a.ldq = p.ldq;
    a.K = p.K[sg]; a.ldk = p.ldk;
    a.Vt = p.Vt[sg]; a.ldvt = p.ldvt;
    a.O = p.O + (int64_t)sg * p.seg_pitch * p.ldo; a.ldo = p.ldo;
    a.Lq = p.Lq_seg; a.Lk = p.Lk[sg]; a.H = p.H;
    a.scale_log2 = p.scale_log2;
    a.q_prescaled = 0;
    a.accumulate = p.accumulate;
    a.nqb = p.nqb_seg; a.q_lo = 0;
    a.part_o = nullptr; a.part_ml = nullptr;
    a.tail_qb = p.nqb_seg; a.splits = 1;
    a.last_w = p.last_w[sg];

    const int q0 = qb * QB + wave * QW;
    bf16x8_t qf[8];
    load_q_frags(a, h, q0, ql, hi, qf);
    f32x16 oacc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) oacc[i] = zero_acc();
    float m_run = NEG_BIG, l_run = 0.f;

    int koff[8], voff[4];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) koff[ks] = k_frag_offset(ks, ql, hi);
#pragma unroll
    for (int sgp = 0; sgp < 4; ++sgp) voff[sgp] = v_frag_offset(sgp, ql, hi);
    DmaPtrs dp;
    dma_init(dp, a, h, tid);
    const int64_t kstep = (int64_t)KT * a.ldk;

    const int nt = (a.Lk + KT - 1) / KT;
    const bool ragged = (a.Lk % KT) != 0;          // then the LAST tile takes the register path (keys >= Lk of V^T zeroed)
    if (nt == 1 && ragged) {
        Stage st;
        stage_load(st, a, h, 0, tid);
        stage_store_v2(st, smem, tid);
    } else {
        dma_tile(dp, kstep, smem, wave);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    int cur = 0;
    for (int t = 0; t < nt; ++t) {
        char* kb = smem + cur * V2_BUF;
        char* nb = smem + (cur ^ 1) * V2_BUF;
        const bool has_next = t + 1 < nt;
        const bool next_reg = has_next && ragged && (t + 2 == nt);
        if (has_next && !next_reg) dma_tile(dp, kstep, nb, wave);
        if (t == nt - 1)
            tile_body_v2<true, true>(kb, a, qf, oacc, m_run, l_run, t * KT, ql, hi, koff, voff);
        else
            tile_body_v2<false>(kb, a, qf, oacc, m_run, l_run, t * KT, ql, hi, koff, voff);
        if (next_reg) {
            // (once per workgroup: its address arithmetic is kept HERE — computed ahead of the loop it would be carried through every tile
            // in registers the tile body needs, i.e. spilled)
            int tid_here = tid;
            asm volatile("" : "+v"(tid_here));
            Stage st;
            stage_load(st, a, h, (t + 1) * KT, tid_here);
            stage_store_v2(st, nb, tid_here);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        cur ^= 1;
    }
    store_o(a, oacc, l_run, h, q0, ql, hi);
}

// shapes the short-key kernel takes (host): every segment's Lk <= 128 on top of attn_short::fits' store alignment; the segments' first rows
// must keep that alignment too (seg_pitch * ldo % 8 == 0 follows from ldo % 8 == 0)
inline bool short_fits(const AttnSegArgs& a) {
    for (int s = 0; s < a.nseg; ++s)
        if (a.Lk[s] > attn_short::LKMAX) return false;
    return (a.ldo % 8) == 0 && ((uintptr_t)a.O % 16) == 0;
}

inline void launch_short(const AttnSegArgs& a, int ncu, hipStream_t st) {
    AttnSegArgs b = a;
    b.nqb_seg = (a.Lq_seg + QB32 - 1) / QB32;
    b.nqb = b.nseg * b.nqb_seg;
    const int nunit = b.nqb * b.H;
    const int nwg = (nunit + 3) / 4;
    const dim3 g((unsigned)(nwg < ncu ? nwg : ncu)), blk(256);
    int nkb = 1;
    for (int s = 0; s < a.nseg; ++s) nkb = max(nkb, (a.Lk[s] + 31) / 32);
    if (nkb == 1) hipLaunchKernelGGL(attn_short_seg_kernel<1>, g, blk, 0, st, b, nunit);
    else if (nkb == 2) hipLaunchKernelGGL(attn_short_seg_kernel<2>, g, blk, 0, st, b, nunit);
    else if (nkb == 3) hipLaunchKernelGGL(attn_short_seg_kernel<3>, g, blk, 0, st, b, nunit);
    else hipLaunchKernelGGL(attn_short_seg_kernel<4>, g, blk, 0, st, b, nunit);
}

inline void launch_v2(const AttnSegArgs& a, hipStream_t st) {
    AttnSegArgs b = a;
    b.nqb_seg = (a.Lq_seg + QB - 1) / QB;
    b.nqb = b.nseg * b.nqb_seg;
    hipLaunchKernelGGL(attn_seg_kernel_v2, dim3((unsigned)(((b.H + 7) / 8) * b.nqb * 8)), dim3(NW * 64), 0, st, b);
}

}  // namespace attn_seg
