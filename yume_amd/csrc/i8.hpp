// i8.hpp — (r25) the int8 row format of the int8 QKV option, defined once: symmetric int8 with ONE fp32 scale per row.
//
//   amax  = max_k |x[r, k]| over the row's bf16 values;
//   scale = amax / 127.0f (one IEEE fp32 division); 1.0f for an all-zero row;
//   q[k]  = rne(clamp(x[k] / scale, +-127))          clamped BEFORE the rounding: the byte 0x80 (-128) is never emitted.
//
// x / scale is formed as in quant_rows.hip, through the IEEE reciprocal: (x * pre) * inv with inv = 1 / (scale * pre), pre = 2^64 for rows
// whose scale lies below 2^-60 (rows of bf16 subnormals: 1 / scale would overflow), else 1; both products by pre are exact. The reciprocal and
// the product each round once (2^-24 relative), so
//       |q - x / scale| <= 0.5 + 2^-20 |x / scale|.
// Dequantised, x ~ q * scale with |q| <= 127: seven bits of resolution under the row's largest value.
//
// NON-FINITE INPUT (one rule): a row that holds an Inf or a NaN has no amax. Its scale is a quiet NaN and all its bytes are 0 — the GEMM
// behind it then yields NaN for that row's outputs instead of numbers made from a clamped infinity. The other rows are not affected.
// The amax is taken on the bit patterns (|x| as an unsigned integer orders like the value, and every Inf / NaN pattern lies above every
// finite one), so the rule costs nothing per element; i8::row_amax turns "pattern >= Inf" into +Inf before the cross-lane float maximum.
//
// The stand-alone quantiser (quant_rows_i8.hip) and the adaLN emitter (norm_i8.hip) use these functions and nothing else for the format,
// which is what makes the emitter equal its two-call composite bit for bit.
#pragma once
#include "common.hpp"

namespace i8 {

constexpr float I8_MAX = 127.0f;

// running maximum of |x| bit patterns; the two bf16 of a packed dword (element 0 in the low half)
__device__ __forceinline__ unsigned absbits2(unsigned w, unsigned m) {
    m = max(m, (w << 16) & 0x7fffffffu);
    return max(m, w & 0x7fff0000u);
}

// a lane's maximum as a float for the cross-lane maximum: +Inf where the lane saw a non-finite value (fmaxf keeps +Inf against anything)
__device__ __forceinline__ float row_amax(unsigned mbits) {
    return mbits >= 0x7f800000u ? __uint_as_float(0x7f800000u) : __uint_as_float(mbits);
}

struct RowScale {
    float scale;    // what is stored
    float pre, inv; // x / scale = (x * pre) * inv
    bool bad;       // the row held a non-finite value: bytes 0
};

// from the row's reduced amax (>= 0, +Inf for a row with a non-finite value)
__device__ __forceinline__ RowScale row_scale(float amax) {
    RowScale r;
    r.bad = !(amax < __uint_as_float(0x7f800000u));
    const float s = amax > 0.f ? amax / I8_MAX : 1.0f;
    r.pre = s < 0x1p-60f ? 0x1p64f : 1.0f;
    r.inv = 1.0f / (s * r.pre);
    r.scale = r.bad ? __uint_as_float(0x7fc00000u) : s;
    return r;
}

// four bf16 (two packed dwords, element 0 in the low half as pack_bf16x2 leaves them) -> four int8 bytes, byte k = element k
__device__ __forceinline__ unsigned quant4(u32x2 h, const RowScale& r) {
    float f[4];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        f[2 * q] = __uint_as_float(h[q] << 16);
        f[2 * q + 1] = __uint_as_float(h[q] & 0xffff0000u);
    }
    unsigned w = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float t = fminf(fmaxf((f[q] * r.pre) * r.inv, -I8_MAX), I8_MAX);     // clamp BEFORE the rounding: |t| <= 127
        w |= ((unsigned)(int)__builtin_rintf(t) & 0xffu) << (8 * q);                // round to nearest even, then an exact conversion
    }
    return r.bad ? 0u : w;
}

}  // namespace i8
