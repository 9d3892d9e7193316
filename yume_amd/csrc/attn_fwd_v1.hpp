// attn_fwd_v1.hpp — attn_fwd_kernel: the first attention kernel (variant 1). 4 waves, 128 queries per workgroup, K / V^T tiles staged
// through registers into a double-buffered LDS image (V^T rows padded to 136 bytes, read with ds_read_b64). Not on the product path: kept as
// an independent cross-check of the LDS-DMA kernels (the tests compare them). Formulation and tile layouts: attn_tile.hpp.
#pragma once
#include "attn_tile.hpp"

namespace {

constexpr int VROW = 136;                  // bytes per V^T row in LDS (128 + 8 pad)
constexpr int V_TILE_BYTES = D * VROW;     // 17408
constexpr int BUF_BYTES = K_TILE_BYTES + V_TILE_BYTES;

__device__ __forceinline__ void stage_store(const Stage& s, char* buf, int tid) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = (tid >> 4) + 16 * rr;
        const int c = tid & 15;
        *reinterpret_cast<u32x4*>(buf + r * 256 + ((c ^ (r & 15)) << 4)) = s.k[rr];
    }
    char* vb = buf + K_TILE_BYTES;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int d = (tid >> 3) + 32 * rr;
        char* dst = vb + d * VROW + (tid & 7) * 16;   // 8-byte aligned only: two b64 writes
        u32x2 lo, hi;
        lo[0] = s.v[rr][0]; lo[1] = s.v[rr][1];
        hi[0] = s.v[rr][2]; hi[1] = s.v[rr][3];
        *reinterpret_cast<u32x2*>(dst) = lo;
        *reinterpret_cast<u32x2*>(dst + 8) = hi;
    }
}

__global__ __launch_bounds__(NW * 64, 2) void attn_fwd_kernel(AttnArgs p) {
    __shared__ __attribute__((aligned(16))) char smem[2 * BUF_BYTES];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5;
    const int ql = lane & 31;

    YUME_ATTN_BLOCK_HEAD_QB(p, h, qb)
    const int q0 = p.q_lo + qb * QB + wave * QW;
    bf16x8_t qf[8];
    load_q_frags(p, h, q0, ql, hi, qf);
    f32x16 oacc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) oacc[i] = zero_acc();
    float m_run = NEG_BIG;   // running max of the SCALED scores (log2 domain)
    float l_run = 0.f;       // this lane's partial row sum (its 32 of every 64 keys)

    const int nt = (p.Lk + KT - 1) / KT;
    Stage st;
    stage_load(st, p, h, 0, tid);
    stage_store(st, smem, tid);
    if (nt > 1) stage_load(st, p, h, KT, tid);
    __syncthreads();

    int cur = 0;
    for (int t = 0; t < nt; ++t) {
        const char* kb = smem + cur * BUF_BYTES;
        const char* vb = kb + K_TILE_BYTES;

        // ---- S^T = K . Q^T : two 32-key blocks x 8 k-steps ----
        f32x16 sacc[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[b][r] = 0.f;
            const int row = 32 * b + ql;
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const int c = 2 * ks + hi;
                const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(kb + row * 256 + ((c ^ (row & 15)) << 4));
                sacc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], sacc[b], 0, 0, 0);
            }
        }

        // ---- online softmax (lane-local + one exchange with lane^32) ----
        const int j0 = t * KT;
        if (j0 + KT > p.Lk) {
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = j0 + 32 * b + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (key >= p.Lk) sacc[b][r] = NEG_BIG;
                }
        }
        float mx = sacc[0][0];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[b][r]);
        mx = xhalf_max(mx);                                   // combine with the partner lane (other 32 keys)
        const float m_new = fmaxf(m_run, mx * p.scale_log2);
        // deferred rescale: keep the old reference max while it is within 2^DEFER of the new one for every
        // query of the wave (P <= 2^DEFER then; O/l is invariant to the reference) — the O-wide multiply is
        // skipped on most tiles. The previous tile's P.V is complete here, so O, l and m move together.
        if (!__all(m_new - m_run <= DEFER_LOG2)) rescale_to(m_new, m_run, l_run, oacc);
        float psum = 0.f;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f(fmaf(sacc[b][r], p.scale_log2, -m_run));
                sacc[b][r] = pv;
                psum += pv;
            }
        l_run += psum;

        // ---- P^T -> bf16 B fragments: k-step s uses block s>>1, regs 8*(s&1) .. +7 ----
        bf16x8_t pf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            u32x4 w;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                w[j] = pack_bf16x2(sacc[s >> 1][8 * (s & 1) + 2 * j], sacc[s >> 1][8 * (s & 1) + 2 * j + 1]);
            pf[s] = __builtin_bit_cast(bf16x8_t, w);
        }

        // ---- O^T += V^T . P^T : 4 d-blocks x 4 k-steps ----
        // A fragment of k-step s for lane (d = 32*db + ql, hi): keys base .. base+3 and base+8 .. base+11,
        // base = 32*(s>>1) + 16*(s&1) + 4*hi  (the keys whose P the same lane group supplies in pf[s]).
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            const char* vrow = vb + (32 * db + ql) * VROW + 8 * hi;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const char* a = vrow + 64 * (s >> 1) + 32 * (s & 1);
                u32x4 w;
                const u32x2 lo = *reinterpret_cast<const u32x2*>(a);
                const u32x2 hi2 = *reinterpret_cast<const u32x2*>(a + 16);
                w[0] = lo[0]; w[1] = lo[1]; w[2] = hi2[0]; w[3] = hi2[1];
                oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, w), pf[s], oacc[db], 0, 0, 0);
            }
        }

        // ---- stage the next tile, prefetch the one after ----
        if (t + 1 < nt) stage_store(st, smem + (cur ^ 1) * BUF_BYTES, tid);
        __syncthreads();
        if (t + 2 < nt) stage_load(st, p, h, (t + 2) * KT, tid);
        cur ^= 1;
    }

    store_o(p, oacc, l_run, h, q0, ql, hi);
}

}  // namespace

namespace attn_v1 {

static inline void launch(const AttnArgs& a, hipStream_t st) {
    const AttnArgs b = whole_blocks(a, QB);
    hipLaunchKernelGGL(attn_fwd_kernel, xcd_grid(b), dim3(NW * 64), 0, st, b);
}

}  // namespace attn_v1
