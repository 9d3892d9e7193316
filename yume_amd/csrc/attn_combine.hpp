// attn_combine.hpp — attn_combine_kernel: the merge pass behind a launch of attn_fwd7.hip or attn_fwd8.hip that cut its last query blocks
// into key ranges (AttnArgs::tail_qb / splits): one normalised bf16 row of O from the pieces' fp32 partial results.
#pragma once
#include "attn_tile.hpp"

namespace {

constexpr float FAR_BELOW = -100.0f;       // a piece this far under the row's base takes its factor 2^(m_s - m) in two halves

// merge the key-range pieces of the v7 / v8 kernels: O = sum_s O_s 2^(m_s - m) / sum_s l_s 2^(m_s - m), m = max_s m_s (fixed order)
__global__ __launch_bounds__(256) void attn_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml, int splits,
                                                           int64_t rows, int H, unsigned short* __restrict__ O, int64_t ldo, int q_lo,
                                                           int accumulate) {
    const int64_t nq = rows * H * (D / 4);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % (D / 4));
        const int h = (int)((i / (D / 4)) % H);
        const int64_t r = i / ((int64_t)(D / 4) * H);
        float m = NEG_BIG;
        for (int s = 0; s < splits; ++s) m = fmaxf(m, part_ml[((s * rows + r) * H + h) * 2]);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        float l = 0.f;
        for (int s = 0; s < splits; ++s) {
            const float* ml = part_ml + ((s * rows + r) * H + h) * 2;
            const f32x4 o = *reinterpret_cast<const f32x4*>(part_o + (s * rows + r) * ((int64_t)H * D) + h * D + 4 * c4);
            const float d = ml[0] - m;
            if (d < FAR_BELOW) {
                // exp2(d) itself would fall into the denormal range, which v_exp_f32 flushes to 0, and with it a piece that is no small
                // share of the row: an in-range base-free piece comes with the base 0 and a row sum of up to 2^120, beside a sibling that
                // was redone on the robust body with a base above 126 (tests/attn_cases.py, pattern `peak`). The factor in two halves:
                // each is normal down to d = -252, and below that the piece is under 2^-130 of the row.
                const float h2 = __builtin_amdgcn_exp2f(0.5f * d);
                l += (ml[1] * h2) * h2;
                acc += (o * h2) * h2;
            } else {
                const float a = __builtin_amdgcn_exp2f(d);
                l += ml[1] * a;
                acc += o * a;
            }
        }
        const float inv = 1.0f / l;
        float v0 = acc[0] * inv, v1 = acc[1] * inv, v2 = acc[2] * inv, v3 = acc[3] * inv;
        u32x2* dst = reinterpret_cast<u32x2*>(O + (q_lo + r) * ldo + h * D + 4 * c4);
        if (accumulate) {
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

}  // namespace

namespace attn_combine {

// b: the arguments of the split launch (part_o, part_ml, splits, tail_qb set); qblock: its query block (the pieces cover the rows from
// tail_qb * qblock on)
static inline void launch(const AttnArgs& b, int qblock, hipStream_t st) {
    const int q_lo = b.tail_qb * qblock;
    const int64_t rows = b.Lq - q_lo, nq = rows * b.H * (D / 4);
    hipLaunchKernelGGL(attn_combine_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, b.part_o, b.part_ml, b.splits, rows, b.H, b.O,
                       b.ldo, q_lo, b.accumulate);
}

}  // namespace attn_combine
