// attn_short.hpp — attention over a SHORT key sequence (Lk <= 128, head dim 128) with a head's whole K and V^T resident in the registers of
// ONE WAVE (r7). It serves the text cross-attention once the prompt's pad keys are deduplicated (DiTEngine.dedup_pad_keys): the reference
// attends over 512 keys of which 512 - n are copies of one (wan23/modules/model.py:815-821, wan/modules/model.py:931-936); n + 1 keys with a
// weight on the last one are the same softmax (yume_attn_fwd_kw). With 78 keys the call is 14.9 GFLOP against 116 MB of Q read and O written
// on the 5B shape (Lq 9460, H 24).
//
// DESIGNED FOR THE HBM BOUND (Q read + O written, once each; K / V^T are 6 % of the bytes and come from L2), not for the matrix pipe.
//   * a wave is self-sufficient: NKB = ceil(Lk / 32) key blocks; its K fragments (NKB x 8 k-steps of v_mfma_f32_32x32x16_bf16 A operands)
//     and V^T fragments (4 d-blocks x 2 NKB key steps) stay in registers while the head does not change — 128 + 128 registers at NKB = 4,
//     one wave per SIMD (launch bound 256 threads, 1 workgroup per CU: 512 registers per lane);
//   * S^T = K Q^T for 32 queries is 8 NKB MFMAs; every key of the row is present, so the softmax is exact and SINGLE-PASS: one row maximum,
//     no running base, no rescale branch; O^T = V^T P^T is 8 NKB MFMAs and complete in the wave. No LDS, no barrier, no workspace;
//   * P^T needs no exchange: the K rows are loaded in the permuted order of attn_cross_rk.hpp (MFMA row m takes key m with bits 2 and 3
//     exchanged), so a lane's accumulator registers 8 e .. 8 e + 7 of key block kb ARE the B fragment of key step 2 kb + e (keys
//     32 kb + 16 e + 8 half + 0..7), and the V^T fragment is one contiguous 16-byte load;
//   * the V^T ROWS are permuted the same way (MFMA row m takes feature d = m with bits 2 and 3 exchanged): a lane's O^T registers 8 e .. 8 e + 7
//     of d-block db are the eight consecutive features 32 db + 16 e + 8 half + 0..7 of its query — every O store (and the read of an
//     accumulating call) is a full 16 bytes per lane; the eight stores of a lane pair cover the query's whole 256-byte row;
//   * the 4 waves of a workgroup are independent; every wave is persistent over a contiguous range of (head, 32-query block) units in head-major
//     order (static split, no tickets), reloads K / V^T only when the head changes and fetches the next unit's Q fragments straight from
//     global memory one unit ahead, right behind the S products that consumed the current ones;
//   * keys >= Lk: K rows are clamped to row Lk - 1 and their scores masked; V^T chunks are clamped into the row and their columns >= Lk zeroed
//     (0 * garbage must be 0) — with or without YUME_ATTN_KV_PADDED, the loads happen once per head. The last key's exponential is multiplied
//     by p.last_w (1 on an unweighted call). Only the last key block holds masked keys or the last key (NKB = ceil(Lk / 32)).
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): see profiles/r7_dedup_pad_keys.md; scratch 0 in all four
// instances. The compiler schedules the code; nothing here names registers.
#pragma once
#include "common.hpp"
#include "attn_args.hpp"

namespace attn_short {

constexpr int HD = 128;            // head dim
constexpr int QB = 32;             // queries per unit
constexpr int LKMAX = 128;

__device__ __forceinline__ float xhalf_max(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xhalf_sum(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

template <int NKB>
__global__ __launch_bounds__(256, 1) void attn_short_kernel(AttnArgs p, int nqb, int nunit) {
    constexpr int NST = 2 * NKB;                                                  // 16-key steps
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ql = lane & 31, hh = lane >> 5;
    // this wave's units [u0, u1) of the head-major (head, query block) order
    const int nwave = (int)gridDim.x * 4, gw = (int)blockIdx.x * 4 + wave;
    const int u0 = (int)(((int64_t)gw * nunit) / nwave), u1 = (int)(((int64_t)(gw + 1) * nunit) / nwave);
    if (u0 >= u1) return;
    const int pm = (ql & 0x13) | ((ql & 4) << 1) | ((ql & 8) >> 1);              // MFMA row ql -> key / feature ql with bits 2 and 3 exchanged

    bf16x8_t kf[NKB][8], vf[4][NST];
    int head = -1;
    auto load_q = [&](int u, bf16x8_t (&qf)[8]) {
        const int h = u / nqb, qb = u - h * nqb;
        int q = qb * QB + ql;
        q = q < p.Lq ? q : p.Lq - 1;
        const unsigned short* qp = p.Q + (int64_t)q * p.ldq + h * HD + 8 * hh;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const bf16x8_t*>(qp + 16 * ks);
    };
    bf16x8_t qf[8];
    load_q(u0, qf);

    for (int u = u0; u < u1; ++u) {
        const int h = u / nqb, qb = u - h * nqb;
        if (h != head) {                                                          // (uniform) the head's K and V^T fragments
            head = h;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                int key = 32 * kb + pm;
                key = key < p.Lk ? key : p.Lk - 1;                                // (rows beyond Lk: masked below)
                const unsigned short* kp = p.K + (int64_t)key * p.ldk + h * HD + 8 * hh;
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) kf[kb][ks] = *reinterpret_cast<const bf16x8_t*>(kp + 16 * ks);
            }
            const int kmax = (int)p.ldvt - 8;
#pragma unroll
            for (int st = 0; st < NST; ++st) {
                const int kc = 16 * st + 8 * hh;                                  // first key of this lane's chunk
                const int kload = kc < kmax ? kc : kmax;                          // keep the 16-byte load inside the row
                const int nvalid = (kload == kc) ? max(p.Lk - kc, 0) : 0;
#pragma unroll
                for (int db = 0; db < 4; ++db) {
                    u32x4 x = *reinterpret_cast<const u32x4*>(p.Vt + (int64_t)(h * HD + 32 * db + pm) * p.ldvt + kload);
                    if (st >= NST - 2 && nvalid < 8) {                           // (only the last key block can hold keys >= Lk)
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
        // ---- the row's maximum over ALL its keys (lane-local + the partner half)
        float mx = -3.0e38f;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float x = s[kb][r] * p.scale_log2;
                if (kb == NKB - 1) {
                    const int key = 32 * kb + 16 * (r >> 3) + 8 * hh + (r & 7);
                    x = key < p.Lk ? x : -3.0e38f;
                }
                s[kb][r] = x;
                mx = fmaxf(mx, x);
            }
        mx = xhalf_max(mx);
        // ---- exponentials, row sum, P^T fragments: the accumulator's own order
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
                    if (kb == NKB - 1) {
                        const int key = 32 * kb + 16 * e + 8 * hh + j;
                        v = key == p.Lk - 1 ? v * p.last_w : v;                   // the key that stands for last_w keys
                    }
                    ex[j] = v;
                    lsum += v;
                }
                u32x4 w;
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = pack_bf16x2(ex[2 * j], ex[2 * j + 1]);
                pf[2 * kb + e] = __builtin_bit_cast(bf16x8_t, w);
            }
        lsum = xhalf_sum(lsum);
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
        const int q = qb * QB + ql;
        if (q < p.Lq) {
            unsigned short* op = p.O + (int64_t)q * p.ldo + h * HD + 8 * hh;
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

// shapes the kernel takes (host). O is stored 16 bytes at a time: ldo % 8 == 0 and a 16-byte aligned O on top of the common checks
inline bool fits(int64_t Lk, int64_t ldo, const void* O) { return Lk <= LKMAX && (ldo % 8) == 0 && ((uintptr_t)O % 16) == 0; }

inline void launch(const AttnArgs& a, int ncu, hipStream_t st) {
    AttnArgs b = a;
    b.q_lo = 0;
    const int nqb = (int)((b.Lq + QB - 1) / QB);
    const int nunit = nqb * b.H;
    const int nwg = (nunit + 3) / 4;
    const dim3 g((unsigned)(nwg < ncu ? nwg : ncu)), blk(256);
    const int nkb = (b.Lk + 31) / 32;
    if (nkb == 1) hipLaunchKernelGGL(attn_short_kernel<1>, g, blk, 0, st, b, nqb, nunit);
    else if (nkb == 2) hipLaunchKernelGGL(attn_short_kernel<2>, g, blk, 0, st, b, nqb, nunit);
    else if (nkb == 3) hipLaunchKernelGGL(attn_short_kernel<3>, g, blk, 0, st, b, nqb, nunit);
    else hipLaunchKernelGGL(attn_short_kernel<4>, g, blk, 0, st, b, nqb, nunit);
}

}  // namespace attn_short
