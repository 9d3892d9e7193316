// mx6.hpp — OCP MXFP6 e2m3 on the device, defined once for the adaLN emitter (norm_e2m3.hip) and the GEMM's MX-out epilogue (gemm_f6.hpp).
//   encoding: 1 sign, 2 exponent bits (bias 1), 3 mantissa bits, no inf / nan: 0 .. 0.875 in steps of 0.125 (subnormal), [1, 2) step 0.125,
//             [2, 4) step 0.25, [4, 7.5] step 0.5.
//   packing:  32 values = 24 bytes, value i at bits [6 i, 6 i + 6) of the group, little-endian (what v_cvt_scalef32_2xpk16_fp6_f32 writes and
//             v_mfma_scale_f32_16x16x128_f8f6f4 reads: tools/ubench/mfma_f6_map.hip).
//   block exponent (the project's one MX rule, tests/conv_f8_cases.py mx_quantise, with 7.5 in place of 448): the smallest integer e with
//             amax <= 7.5 * 2^e, byte e + 127 clamped below at 0, 127 for an all-zero block; q = e2m3_rne(clamp(v * 2^-e, +-7.5)).
#pragma once
#include "common.hpp"

namespace mx6 {

constexpr float E2M3_MAX = 7.5f;

// 7.5 = 1.875 * 2^2: with amax = 1.f * 2^(E - 127) the exponent is E - 127 - 2 where 1.f <= 1.875 (fraction bits <= 0x700000), else one more.
// fp32 has no E > 254: the byte never exceeds 253.
__device__ __forceinline__ int block_byte(float am) {
    const unsigned bits = __float_as_uint(am);                      // am >= 0: no sign bit
    const int byte = (int)(bits >> 23) - 2 + ((bits & 0x7fffffu) > 0x700000u ? 1 : 0);
    return am > 0.f ? max(byte, 0) : 127;
}

// 2^-e = the fp32 with exponent field 254 - byte in [1, 254]: normal, the product v * 2^-e exact
__device__ __forceinline__ float block_mult(int byte) { return __uint_as_float((unsigned)(254 - byte) << 23); }

// the 6-bit code of t, |t| <= 7.5, round to nearest even. a + 2^(20 + E') - 2^(20 + E') rounds a to a multiple of 2^(E' - 3), the step of the
// binade 2^E' (E' = 0 below 2: the subnormals share the first binade's step); a result that reaches the next binade is exact there. The sign
// bit is set for every t < 0, also where |t| rounds to 0.
__device__ __forceinline__ unsigned e2m3_rne(float t) {
    const float a = fabsf(t);
    const int ep = max((int)(__float_as_uint(a) >> 23) - 127, 0);
    const float magic = __uint_as_float((unsigned)(147 + ep) << 23);
    const float r = (a + magic) - magic;
    const unsigned rb = __float_as_uint(r);
    const unsigned code = r < 1.0f ? (unsigned)(r * 8.0f) : ((((rb >> 23) - 126u) << 3) | ((rb >> 20) & 7u));
    return code | (t < 0.f ? 32u : 0u);
}

// four consecutive values of a block -> their 24 bits (value 0 in the low six)
__device__ __forceinline__ unsigned chunk4(float v0, float v1, float v2, float v3, float mult) {
    const float t0 = fminf(fmaxf(v0 * mult, -E2M3_MAX), E2M3_MAX), t1 = fminf(fmaxf(v1 * mult, -E2M3_MAX), E2M3_MAX);
    const float t2 = fminf(fmaxf(v2 * mult, -E2M3_MAX), E2M3_MAX), t3 = fminf(fmaxf(v3 * mult, -E2M3_MAX), E2M3_MAX);
    return e2m3_rne(t0) | (e2m3_rne(t1) << 6) | (e2m3_rne(t2) << 12) | (e2m3_rne(t3) << 18);
}

// dword d (0..5) of a block's 24 bytes from its eight 24-bit chunks: chunks f = d + d / 3 and f + 1, the first shifted down by 8 (d % 3) bits
__device__ __forceinline__ int first_chunk(int d) { return d + d / 3; }
__device__ __forceinline__ unsigned join_chunks(unsigned lo, unsigned hi, int d) {
    const int s = 8 * (d % 3);
    return (lo >> s) | (hi << (24 - s));
}

}  // namespace mx6
