// attn_fwd_v2.hpp — attn_fwd_kernel_v2<KW>: 4 waves, 128 queries per workgroup, two workgroups per CU, K / V^T tiles by LDS-DMA
// (variant 2; cross-attention and every call with few key tiles or few queries; <true> takes a weighted last key, yume_attn_fwd_kw).
// Formulation and tile layouts: attn_tile.hpp.
// v2: same math and tile shapes as attn_fwd_v1.hpp, different data movement.
//   * K and V^T tiles go HBM -> LDS by LDS-DMA (global_load_lds_dwordx4): no staging VGPRs, no ds_write pass; the
//     bank swizzles are applied on the per-lane SOURCE address (K: chunk ^ (row & 15); V^T: chunk ^ ((row >> 1) & 7))
//     so both tiles are read with conflict-free ds_read_b128.
//   * V^T fragments are 16 contiguous bytes = 8 CONSECUTIVE keys, so the P operand has to hold 8 consecutive keys too:
//     after the exp the packed P words of the two half-waves are exchanged with 8 v_permlane32_swap per tile
//     (lane (q,0) gives its odd 4-key groups, receives the partner's even ones).
//   * only a ragged last tile (Lk % 64 != 0) is register-staged, to zero the keys >= Lk of V^T.
// The DMA of tile t+1 is issued before the compute of tile t and waited for (vmcnt(0)) right before the single
// per-tile barrier, i.e. it has the whole tile of MFMA work to land.
#pragma once
#include "attn_tile.hpp"
#include "trace.hpp"

namespace {

constexpr int V2_BUF = 2 * K_TILE_BYTES;      // K 16 KiB + V^T 16 KiB (128-byte rows, no padding)

// per-thread source pointers of the 8 LDS-DMA pieces of a tile (4 K rounds, 4 V^T rounds), advanced by one tile per use
struct DmaPtrs {
    const unsigned short* k[4];
    const unsigned short* v[4];
};
__device__ __forceinline__ void dma_init(DmaPtrs& dp, const AttnArgs& p, int h, int tid) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = rr * 16 + (tid >> 4);            // K: 64 rows x 16 chunks; full tiles only -> no clamp needed
        dp.k[rr] = p.K + (int64_t)r * p.ldk + h * D + (((tid & 15) ^ (r & 15)) << 3);
        const int d = rr * 32 + (tid >> 3);            // V^T: 128 rows x 8 chunks
        dp.v[rr] = p.Vt + (int64_t)(h * D + d) * p.ldvt + (((tid & 7) ^ ((d >> 1) & 7)) << 3);
    }
}
__device__ __forceinline__ void dma_tile(DmaPtrs& dp, int64_t kstep, char* buf, int wave) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        __builtin_amdgcn_global_load_lds((gbl_cvoid_t*)dp.k[rr], (lds_void_t*)(buf + rr * 4096 + wave * 1024), 16, 0, 0);
        dp.k[rr] += kstep;
    }
    char* vb = buf + K_TILE_BYTES;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        __builtin_amdgcn_global_load_lds((gbl_cvoid_t*)dp.v[rr], (lds_void_t*)(vb + rr * 4096 + wave * 1024), 16, 0, 0);
        dp.v[rr] += KT;
    }
}

// register path for the ragged last tile: same LDS image as dma_tile, keys >= Lk of V^T zeroed (stage_load does it)
__device__ __forceinline__ void stage_store_v2(const Stage& s, char* buf, int tid) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = (tid >> 4) + 16 * rr;
        *reinterpret_cast<u32x4*>(buf + r * 256 + (((tid & 15) ^ (r & 15)) << 4)) = s.k[rr];
    }
    char* vb = buf + K_TILE_BYTES;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int d = (tid >> 3) + 32 * rr;
        *reinterpret_cast<u32x4*>(vb + d * 128 + (((tid & 7) ^ ((d >> 1) & 7)) << 4)) = s.v[rr];
    }
}

template <bool MASK, bool KW = false>
__device__ __forceinline__ void tile_body_v2(const char* kb, const AttnArgs& p, const bf16x8_t (&qf)[8],
                                             f32x16 (&oacc)[4], float& m_run, float& l_run, int j0, int ql, int hi,
                                             const int (&koff)[8], const int (&voff)[4]) {
    const char* vb = kb + K_TILE_BYTES;
    f32x16 sacc[2];
    s_tile(kb, qf, sacc, koff);
    // rows >= Lk of the K tile are clamped copies of key Lk-1, so the row max needs no mask; their P is zeroed below
    float mx = sacc[0][0];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[b][r]);
    mx = xhalf_max(mx);
    const float m_new = fmaxf(m_run, mx * p.scale_log2);
    if (!__all(m_new - m_run <= DEFER_LOG2)) rescale_to(m_new, m_run, l_run, oacc);
    float psum = 0.f;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float pv = __builtin_amdgcn_exp2f(fmaf(sacc[b][r], p.scale_log2, -m_run));
            if (MASK) {
                const int key = j0 + 32 * b + (r & 3) + 8 * (r >> 2) + 4 * hi;
                pv = key < p.Lk ? pv : 0.f;
                if (KW) pv = key == p.Lk - 1 ? pv * p.last_w : pv;      // the weighted last key: the exponential is multiplied, the base logic sees the plain score
            }
            sacc[b][r] = pv;
            psum += pv;
        }
    l_run += psum;

    // ---- P^T fragments of 8 consecutive keys: k-step sg = 2b+e covers keys 16*sg + 8*hi' + j ----
    bf16x8_t pf[4];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            u32x4 w;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const unsigned ev = pack_bf16x2(sacc[b][8 * e + 2 * i], sacc[b][8 * e + 2 * i + 1]);          // group 2e
                const unsigned od = pack_bf16x2(sacc[b][8 * e + 4 + 2 * i], sacc[b][8 * e + 4 + 2 * i + 1]);  // group 2e+1
                const auto r = __builtin_amdgcn_permlane32_swap(ev, od, false, false);
                w[i] = r[0];        // keys j = 0..3 of this lane's half
                w[2 + i] = r[1];    // keys j = 4..7
            }
            pf[2 * b + e] = __builtin_bit_cast(bf16x8_t, w);
        }

    // ---- O^T += V^T . P^T ----
    // The S accumulators are dead once P is packed: their registers hold a 4-deep ring of V^T fragments, pinned with
    // sched_barriers (left alone, the scheduler emits `ds_read ; s_waitcnt lgkmcnt(0) ; v_mfma` sixteen times).
    // row 32db + ql swizzles like row ql ((d >> 1) & 7 is unchanged by + 32db)
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

// KW: the last key carries p.last_w (yume_attn_fwd_kw). The last tile then takes the MASK body also when Lk % 64 == 0 (it still comes by LDS-DMA:
// only a ragged tile is register-staged). KW = false is the kernel as it always was.
template <bool KW>
__global__ __launch_bounds__(NW * 64, 2) void attn_fwd_kernel_v2(AttnArgs p) {
    __shared__ __attribute__((aligned(16))) char smem[2 * V2_BUF];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5;
    const int ql = lane & 31;
    YUME_ATTN_BLOCK_HEAD_QB(p, h, qb)
    TRACE_STAMP(0);
    const int q0 = p.q_lo + qb * QB + wave * QW;
    bf16x8_t qf[8];
    load_q_frags(p, h, q0, ql, hi, qf);
    f32x16 oacc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) oacc[i] = zero_acc();
    float m_run = NEG_BIG, l_run = 0.f;

    int koff[8], voff[4];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) koff[ks] = k_frag_offset(ks, ql, hi);
#pragma unroll
    for (int sg = 0; sg < 4; ++sg) voff[sg] = v_frag_offset(sg, ql, hi);
    DmaPtrs dp;
    dma_init(dp, p, h, tid);
    const int64_t kstep = (int64_t)KT * p.ldk;

    const int nt = (p.Lk + KT - 1) / KT;
    const bool ragged = (p.Lk % KT) != 0;          // then the LAST tile takes the register path
    // (attn_v2::launch never sets gridDim.y > 1: the nsp > 1 paths are dead. They stay until their removal, which changes this kernel's code,
    // is measured on its own.)
    const int nsp = gridDim.y, sp = blockIdx.y;    // key-range split (1 split = the whole range)
    const int t0 = (int)((int64_t)nt * sp / nsp), t1 = (int)((int64_t)nt * (sp + 1) / nsp);
    if (t0 > 0) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            dp.k[rr] += (int64_t)t0 * kstep;
            dp.v[rr] += (int64_t)t0 * KT;
        }
    }
    if (t0 == nt - 1 && ragged) {
        Stage st;
        stage_load(st, p, h, t0 * KT, tid);
        stage_store_v2(st, smem, tid);
    } else {
        dma_tile(dp, kstep, smem, wave);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    TRACE_STAMP(3);

    int cur = 0;
    for (int t = t0; t < t1; ++t) {
        char* kb = smem + cur * V2_BUF;
        char* nb = smem + (cur ^ 1) * V2_BUF;
        const bool has_next = t + 1 < t1;
        const bool next_reg = has_next && ragged && (t + 2 == nt);
        if (has_next && !next_reg) dma_tile(dp, kstep, nb, wave);
        if (t == nt - 1 && (ragged || KW))
            tile_body_v2<true, KW>(kb, p, qf, oacc, m_run, l_run, t * KT, ql, hi, koff, voff);
        else
            tile_body_v2<false>(kb, p, qf, oacc, m_run, l_run, t * KT, ql, hi, koff, voff);
        if (next_reg) {
            Stage st;
            stage_load(st, p, h, (t + 1) * KT, tid);
            stage_store_v2(st, nb, tid);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        cur ^= 1;
    }

    if (nsp > 1) {            // partial result of this key range
        const float l_part = xhalf_sum(l_run);
        const int q = q0 + ql;
        if (q < p.Lq) {
            const int64_t rows = p.Lq - p.q_lo, r = q - p.q_lo;
            float* po = p.part_o + ((int64_t)sp * rows + r) * ((int64_t)p.H * D) + h * D + 4 * hi;
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<f32x4*>(po + 32 * db + 8 * g) =
                        f32x4{oacc[db][4 * g + 0], oacc[db][4 * g + 1], oacc[db][4 * g + 2], oacc[db][4 * g + 3]};
            if (hi == 0) {
                float* pm = p.part_ml + (((int64_t)sp * rows + r) * p.H + h) * 2;
                pm[0] = m_run;
                pm[1] = l_part;
            }
        }
        return;
    }

    TRACE_STAMP(1);
    store_o(p, oacc, l_run, h, q0, ql, hi);
    TRACE_STAMP(2);
}

}  // namespace

namespace attn_v2 {

// all query rows in whole blocks, one key range (gridDim.y = 1); weighted: the last key counts a.last_w times
static inline void launch(const AttnArgs& a, bool weighted, hipStream_t st) {
    const AttnArgs b = whole_blocks(a, QB);
    if (weighted) hipLaunchKernelGGL(attn_fwd_kernel_v2<true>, xcd_grid(b), dim3(NW * 64), 0, st, b);
    else hipLaunchKernelGGL(attn_fwd_kernel_v2<false>, xcd_grid(b), dim3(NW * 64), 0, st, b);
}

}  // namespace attn_v2
