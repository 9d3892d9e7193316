// quant_rows.hip — per-row absmax quantiser bf16 -> OCP e4m3fn (yume_quant_rows_e4m3): the activation rows [L, K] in front of the fp8 FFN
// GEMMs (gemm_f8.hip) and, once at pack time, their weights [N, K] (one scale per output channel).
//
//   amax = max_k |x[r, k]|;   scale[r] = amax / 448.0f (ONE IEEE fp32 division per row; 1 for an all-zero row);
//   q[r, k] = e4m3_rne(clamp(x[r, k] / scale[r], +-448))
//
// One wave per row, a lane takes 16 elements at a time (two 16-byte loads, one 16-byte store): K = 3072 is 3 rounds of 64 lanes, K = 14336
// is 14, nothing idles at the block's shapes. The row is read twice (amax, then convert); the second read comes from the L2 (a row is at
// most 28 KiB). Per element: two multiplies, one clamp (v_med3), half a v_cvt_pk_fp8_f32 — no division.
//   x / scale is formed as (x * pre) * inv with inv = 1 / (scale * pre), pre = 2^64 for rows whose scale lies below 2^-60 (rows of bf16
//   subnormals: 1 / scale would overflow), else 1. Both products by pre are exact (powers of two, results far from either end of the range).
// Roofline: memory — reads 2 K bytes (+ 2 K from the L2), writes K bytes per row.
#include "common.hpp"

namespace {

constexpr float E4M3_MAX = 448.0f;

__device__ __forceinline__ float absmax8(u32x4 v, float m) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        m = fmaxf(m, fabsf(__uint_as_float(v[q] << 16)));
        m = fmaxf(m, fabsf(__uint_as_float(v[q] & 0xffff0000u)));
    }
    return m;
}

// eight bf16 -> eight e4m3 bytes (two dwords)
__device__ __forceinline__ u32x2 quant8(u32x4 v, float pre, float inv) {
    u32x2 o;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        float f[4];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            f[2 * q] = __uint_as_float(v[2 * h + q] << 16);
            f[2 * q + 1] = __uint_as_float(v[2 * h + q] & 0xffff0000u);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) f[q] = fminf(fmaxf((f[q] * pre) * inv, -E4M3_MAX), E4M3_MAX);      // clamp BEFORE the convert: beyond 448 it gives NaN
        int w = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w, true);
        o[h] = (unsigned)w;
    }
    return o;
}

__global__ __launch_bounds__(256) void quant_rows_e4m3_kernel(const unsigned short* __restrict__ x, int64_t ldx, int64_t R, int K,
                                                              unsigned char* __restrict__ q, int64_t ldq, float* __restrict__ scale) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;                                            // (wave-uniform) rows [0, R) only
    // a lane's 16 elements of round t: columns 16 (64 t + lane) .. + 15 < K (K % 16 == 0), i.e. bytes [32 c, 32 c + 32) of the x row and
    // [16 c, 16 c + 16) of the q row, c < K / 16: inside x[r, 0:K] and q[r, 0:K]
    const unsigned short* xr = x + r * ldx;
    const int nch = K >> 4;
    float m = 0.f;
#pragma unroll 4
    for (int c = lane; c < nch; c += 64) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(xr + 16 * c), b = *reinterpret_cast<const u32x4*>(xr + 16 * c + 8);
        m = absmax8(b, absmax8(a, m));
    }
    m = wave_max(m);
    const float s = m > 0.f ? m / E4M3_MAX : 1.0f;
    const float pre = s < 0x1p-60f ? 0x1p64f : 1.0f;
    const float inv = 1.0f / (s * pre);
    if (lane == 0) scale[r] = s;
    unsigned char* qr = q + r * ldq;
#pragma unroll 4
    for (int c = lane; c < nch; c += 64) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(xr + 16 * c), b = *reinterpret_cast<const u32x4*>(xr + 16 * c + 8);
        const u32x2 lo = quant8(a, pre, inv), hi = quant8(b, pre, inv);
        *reinterpret_cast<u32x4*>(qr + 16 * c) = u32x4{lo[0], lo[1], hi[0], hi[1]};
    }
}

}  // namespace

extern "C" int yume_quant_rows_e4m3(const void* x, int64_t ldx, int64_t R, int64_t K, void* q, int64_t ldq, float* scale, void* stream) {
    YUME_REQUIRE(R >= 0 && K > 0, "quant_rows_e4m3: bad shape R=%lld K=%lld", (long long)R, (long long)K);
    YUME_REQUIRE((K % 16) == 0, "quant_rows_e4m3: K=%lld must be a multiple of 16", (long long)K);
    YUME_REQUIRE(K < (1ll << 31) && R < (1ll << 31) * 4, "quant_rows_e4m3: dimension too large");
    YUME_REQUIRE((ldq % 16) == 0 && ldq >= K, "quant_rows_e4m3: ldq=%lld must be a multiple of 16 and >= K", (long long)ldq);
    YUME_REQUIRE((ldx % 8) == 0 && ldx >= K, "quant_rows_e4m3: ldx=%lld must be a multiple of 8 and >= K", (long long)ldx);
    if (R == 0) return YUME_OK;
    YUME_REQUIRE(x && q && scale, "quant_rows_e4m3: NULL pointer");
    YUME_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)q % 16) == 0 && ((uintptr_t)scale % 4) == 0, "quant_rows_e4m3: x and q must be 16-byte aligned");
    // YUME_NORM_LOG=1 (read once per process): one stderr line per launch, so a log can show that a path makes NO quantiser pass
    static const bool log_on = [] { const char* v = getenv("YUME_NORM_LOG"); return v && atoi(v) != 0; }();
    if (log_on) fprintf(stderr, "[quant] rows_e4m3 R=%lld K=%lld ldx=%lld ldq=%lld\n", (long long)R, (long long)K, (long long)ldx, (long long)ldq);
    hipLaunchKernelGGL(quant_rows_e4m3_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned short*)x, ldx, R, (int)K, (unsigned char*)q, ldq, scale);
    YUME_CHECK_LAUNCH("quant_rows_e4m3");
    return YUME_OK;
}
