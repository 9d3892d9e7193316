// quant_rows_i8.hip — (r25) per-row absmax quantiser bf16 -> symmetric int8 (yume_quant_rows_i8; the format: i8.hpp): the weights [N, K] of
// the int8 QKV option once at pack time (one scale per output channel), and the composite yume_adaln_modulate_i8 (norm_i8.hip) is held to.
//
// quant_rows.hip's structure: one wave per row, a lane takes 16 elements at a time (two 16-byte loads, one 16-byte store); the row is read
// twice (amax, then convert), the second read from the L2. Per element: two multiplies, one clamp, one v_rndne, one convert — no division.
// Roofline: memory — reads 2 K bytes (+ 2 K from the L2), writes K bytes per row.
#include "i8.hpp"

namespace {

__global__ __launch_bounds__(256) void quant_rows_i8_kernel(const unsigned short* __restrict__ x, int64_t ldx, int64_t R, int K,
                                                            unsigned char* __restrict__ q, int64_t ldq, float* __restrict__ scale) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;                                            // (wave-uniform) rows [0, R) only
    // a lane's 16 elements of round t: columns 16 (64 t + lane) .. + 15 < K (K % 16 == 0), i.e. bytes [32 c, 32 c + 32) of the x row and
    // [16 c, 16 c + 16) of the q row, c < K / 16: inside x[r, 0:K] and q[r, 0:K]
    const unsigned short* xr = x + r * ldx;
    const int nch = K >> 4;
    unsigned mb = 0u;
#pragma unroll 4
    for (int c = lane; c < nch; c += 64) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(xr + 16 * c), b = *reinterpret_cast<const u32x4*>(xr + 16 * c + 8);
#pragma unroll
        for (int i = 0; i < 4; ++i) mb = i8::absbits2(b[i], i8::absbits2(a[i], mb));
    }
    const i8::RowScale rs = i8::row_scale(wave_max(i8::row_amax(mb)));
    if (lane == 0) scale[r] = rs.scale;
    unsigned char* qr = q + r * ldq;
#pragma unroll 4
    for (int c = lane; c < nch; c += 64) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(xr + 16 * c), b = *reinterpret_cast<const u32x4*>(xr + 16 * c + 8);
        *reinterpret_cast<u32x4*>(qr + 16 * c) = u32x4{i8::quant4(u32x2{a[0], a[1]}, rs), i8::quant4(u32x2{a[2], a[3]}, rs),
                                                       i8::quant4(u32x2{b[0], b[1]}, rs), i8::quant4(u32x2{b[2], b[3]}, rs)};
    }
}

}  // namespace

extern "C" int yume_quant_rows_i8(const void* x, int64_t ldx, int64_t R, int64_t K, void* q, int64_t ldq, float* scale, void* stream) {
    YUME_REQUIRE(R >= 0 && K > 0, "quant_rows_i8: bad shape R=%lld K=%lld", (long long)R, (long long)K);
    YUME_REQUIRE((K % 16) == 0, "quant_rows_i8: K=%lld must be a multiple of 16", (long long)K);
    YUME_REQUIRE(K < (1ll << 31) && R < (1ll << 31) * 4, "quant_rows_i8: dimension too large");
    YUME_REQUIRE((ldq % 16) == 0 && ldq >= K, "quant_rows_i8: ldq=%lld must be a multiple of 16 and >= K", (long long)ldq);
    YUME_REQUIRE((ldx % 8) == 0 && ldx >= K, "quant_rows_i8: ldx=%lld must be a multiple of 8 and >= K", (long long)ldx);
    if (R == 0) return YUME_OK;
    YUME_REQUIRE(x && q && scale, "quant_rows_i8: NULL pointer");
    YUME_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)q % 16) == 0 && ((uintptr_t)scale % 4) == 0, "quant_rows_i8: x and q must be 16-byte aligned");
    // YUME_NORM_LOG=1 (read once per process): one stderr line per launch, so a log can show that a path makes NO quantiser pass
    static const bool log_on = [] { const char* v = getenv("YUME_NORM_LOG"); return v && atoi(v) != 0; }();
    if (log_on) fprintf(stderr, "[quant] rows_i8 R=%lld K=%lld ldx=%lld ldq=%lld\n", (long long)R, (long long)K, (long long)ldx, (long long)ldq);
    hipLaunchKernelGGL(quant_rows_i8_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned short*)x, ldx, R, (int)K, (unsigned char*)q, ldq, scale);
    YUME_CHECK_LAUNCH("quant_rows_i8");
    return YUME_OK;
}
