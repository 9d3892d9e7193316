// attn_tile.hpp — what the tile-streaming attention kernels of attn_fwd.hip share (attn_fwd_v1.hpp, attn_fwd_v2.hpp, attn_fwd_v4.hpp and
// the merge pass attn_combine.hpp): tile constants, the half-wave exchanges, the register-staged tile load, and the prologue / epilogue
// pieces every kernel starts and ends with.
// Common to all: each wave owns 32 queries and walks the keys in tiles of 64. Everything is computed TRANSPOSED so that
// the softmax row of a query lives in ONE lane (plus its partner lane^32) and never needs LDS or cross-lane shuffles:
//
//   S^T[key, q] = K[key, :] . Q[q, :]        v_mfma_f32_32x32x16_bf16, A = K tile (LDS), B = Q^T (registers)
//                 C layout: col = lane&31 = q, row = key = (r&3) + 8*(r>>2) + 4*(lane>>5)
//   P^T         = exp2(S^T*c - m)            in registers; packed to bf16 it IS the B operand of
//   O^T[d, q]   = V^T[d, key] . P^T[key, q]  A = V^T tile (LDS, K-major image), B = P^T (registers)
//                 with the SAME key<->k-slot assignment on both operands, so no permutation is needed.
//   O^T accumulators keep col = lane&31 = q, so the online-softmax rescale is lane-local too.
//
// K tile  : LDS [64 keys][128 d] bf16, 16-byte chunk c of row r stored at chunk c ^ (r & 15)  (ds_read_b128 conflict-free)
// V^T tile: LDS [128 d][64 keys] bf16; v1: row stride 136 B (ds_read_b64); v2 / v4: 128-byte rows, chunk c of row d at
//           chunk c ^ ((d >> 1) & 7), the swizzle applied on the SOURCE address of the LDS-DMA
// Roofline: MFMA (bf16 dense). Algorithmic work 4*Lq*Lk*128 flop per head.
#pragma once
#include "common.hpp"
#include "attn_args.hpp"

namespace {

constexpr int QW = 32;          // queries per wave
constexpr int NW = 4;           // waves per workgroup
constexpr int QB = QW * NW;     // 128 queries per workgroup
constexpr int KT = 64;          // keys per tile
constexpr int D = 128;
constexpr int K_TILE_BYTES = KT * D * 2;   // 16384
constexpr float NEG_BIG = -1.0e30f;
constexpr float DEFER_LOG2 = 8.0f;         // deferred-rescale threshold in the log2 domain (P <= 256)

// max / sum across the two 32-lane halves of a wave: one v_permlane32_swap instead of an LDS shuffle
__device__ __forceinline__ float xhalf_max(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xhalf_sum(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_cvoid_t;

struct Stage {
    u32x4 k[4];
    u32x4 v[4];
};

__device__ __forceinline__ void stage_load(Stage& s, const AttnArgs& p, int h, int j0, int tid) {
    // K: 64 rows x 256 B: thread -> chunk c = tid&15, rows tid/16 + 16*rr
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        int key = j0 + (tid >> 4) + 16 * rr;
        key = key < p.Lk ? key : p.Lk - 1;
        s.k[rr] = *reinterpret_cast<const u32x4*>(p.K + (int64_t)key * p.ldk + h * D + (tid & 15) * 8);
    }
    // V^T: 128 rows (d) x 128 B (64 keys): thread -> chunk c = tid&7, rows tid/8 + 32*rr
    int kc = j0 + (tid & 7) * 8;                      // first key of this chunk
    const int kmax = (int)p.ldvt - 8;
    const int kload = kc < kmax ? kc : kmax;          // keep the 16-byte load inside the row
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int d = (tid >> 3) + 32 * rr;
        s.v[rr] = *reinterpret_cast<const u32x4*>(p.Vt + (int64_t)(h * D + d) * p.ldvt + kload);
    }
    if (kc + 8 > p.Lk) {
        // keys >= Lk must contribute exactly 0 (their P is 0, but 0 * NaN-bits would poison O): zero them
        const int nvalid = (kload == kc) ? max(p.Lk - kc, 0) : 0;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                unsigned int x = s.v[rr][w];
                if (2 * w >= nvalid) x = 0u;
                else if (2 * w + 1 >= nvalid) x &= 0xffffu;
                s.v[rr][w] = x;
            }
        }
    }
}

// ---- prologue pieces (every kernel: block id -> work, Q^T fragments, zeroed accumulators; v2 / v4: the swizzle tables) ----

// block -> (head, query block): XCD x (= blockIdx % 8) works on heads x, x+8, ... so one head's
// K/V stay in one XCD's L2 while its query blocks stream through. Declares `int h, qb`; a surplus block id RETURNS FROM THE KERNEL.
// A macro, not a function: with the early exit behind a call the inlined code of attn_fwd_kernel_v2 and attn_fwd_kernel_v4 came out with
// one s_add_i32 whose operands had changed places (every form of a bool- or struct-returning helper tried did that or worse), and those
// kernels' generated code is held fixed. Expanded in place it is the text the kernels always had.
#define YUME_ATTN_BLOCK_HEAD_QB(p, h, qb)                                                 \
    int h, qb;                                                                            \
    {                                                                                     \
        const int bid = blockIdx.x;                                                       \
        const int xcd = bid & 7, idx = bid >> 3;                                          \
        const int hx = (p.H + 7 - xcd) >> 3; /* heads owned by this XCD */                \
        const int per = hx * p.nqb;                                                       \
        if (idx >= per) return;                                                           \
        h = xcd + 8 * (idx / p.nqb);                                                      \
        qb = idx % p.nqb;                                                                 \
    }

// Q^T fragments (B operand) of the wave's 32 queries q0 ..: lane (q = ql, hi) holds Q[q][16*ks + 8*hi .. +7]
__device__ __forceinline__ void load_q_frags(const AttnArgs& p, int h, int q0, int ql, int hi, bf16x8_t (&qf)[8]) {
    int q = q0 + ql;
    q = q < p.Lq ? q : p.Lq - 1;
    const unsigned short* qp = p.Q + (int64_t)q * p.ldq + h * D + 8 * hi;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const bf16x8_t*>(qp + 16 * ks);
}

// a zeroed accumulator block. (By value: a helper that zeroes the kernel's oacc[4] through a reference changed the register allocation of
// attn_fwd_kernel_v2 and attn_fwd_kernel_v4; so did one that fills the koff / voff tables below through references.)
__device__ __forceinline__ f32x16 zero_acc() {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}

// per-lane byte offsets of the K fragment of k-step ks (row ql) and of the V^T fragment of key group sg (row ql) in the swizzled
// 128-byte-row LDS images of v2 / v4
__device__ __forceinline__ int k_frag_offset(int ks, int ql, int hi) { return ql * 256 + (((2 * ks + hi) ^ (ql & 15)) << 4); }
__device__ __forceinline__ int v_frag_offset(int sg, int ql, int hi) { return ql * 128 + (((2 * sg + hi) ^ ((ql >> 1) & 7)) << 4); }

// move the running reference max to m_new: O, l and m together
__device__ __forceinline__ void rescale_to(float m_new, float& m_run, float& l_run, f32x16 (&oacc)[4]) {
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;
    l_run *= alpha;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
}

// S^T = K . Q^T of one 64-key tile (v2 / v4; kb: its swizzled K image in LDS): both 32-key halves per k-step, K fragments KD - 1 k-steps
// ahead (a KD-deep ring, order pinned). Row 32b + ql has the same swizzle as row ql: one per-lane offset per k-step + an immediate
constexpr int KD = 3;
__device__ __forceinline__ void s_tile(const char* kb, const bf16x8_t (&qf)[8], f32x16 (&sacc)[2], const int (&koff)[8]) {
#pragma unroll
    for (int b = 0; b < 2; ++b) sacc[b] = zero_acc();
    bf16x8_t ka[KD], kc[KD];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < KD - 1; ++ks) {
        ka[ks] = *reinterpret_cast<const bf16x8_t*>(kb + koff[ks]);
        kc[ks] = *reinterpret_cast<const bf16x8_t*>(kb + koff[ks] + 32 * 256);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        if (ks + KD - 1 < 8) {
            ka[(ks + KD - 1) % KD] = *reinterpret_cast<const bf16x8_t*>(kb + koff[ks + KD - 1]);
            kc[(ks + KD - 1) % KD] = *reinterpret_cast<const bf16x8_t*>(kb + koff[ks + KD - 1] + 32 * 256);
            __builtin_amdgcn_sched_barrier(0);
        }
        sacc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka[ks % KD], qf[ks], sacc[0], 0, 0, 0);
        sacc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kc[ks % KD], qf[ks], sacc[1], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- epilogue: O[q, d] = O^T[d, q] / l (+ the old O of an accumulating call) ----
__device__ __forceinline__ void store_o(const AttnArgs& p, const f32x16 (&oacc)[4], float l_run, int h, int q0, int ql, int hi) {
    const float l_tot = xhalf_sum(l_run);
    const float inv = 1.0f / l_tot;
    const int q = q0 + ql;
    if (q < p.Lq) {
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

// ---- launch geometry (host): whole query blocks of `qblock` rows over [a.q_lo, a.Lq), no key-range split ----
inline AttnArgs whole_blocks(const AttnArgs& a, int qblock) {
    AttnArgs b = a;
    b.nqb = (a.Lq - a.q_lo + qblock - 1) / qblock;
    b.tail_qb = b.nqb;
    b.splits = 1;
    return b;
}
// every XCD slot gets ceil(H/8)*nqb block ids; surplus ids exit immediately (YUME_ATTN_BLOCK_HEAD_QB)
inline dim3 xcd_grid(const AttnArgs& b) { return dim3((unsigned)(((b.H + 7) / 8) * b.nqb * 8)); }

}  // namespace
