// quant_mx.hip — the two stand-alone OCP MX e4m3 quantisers in front of the fp8 self-attention (r22, attn_f8.hpp):
//   yume_quant_rows_mx_e4m3   bf16 rows [R, K] -> e4m3 bytes [R, K] + one E8M0 byte per row and 32 consecutive columns
//   yume_attn_vt_mx_e4m3      the bf16 K-major V^T image [C, Lk] -> the e4m3 V^T image of attn_f8.hpp (tiles of 128 keys in the key order of
//                             the P operand) + one E8M0 byte per channel row and k-block of the instruction
// Exponent rule: the project's one MX rule (gemm_f8.hpp f8_epilogue_mx_gelu, vae_norm_mx.hip mx_store; host mirror
// tests/conv_f8_cases.py mx_quantise): e = the smallest integer with amax <= 448 * 2^e, byte e + 127 clamped below at 0, 127 for an all-zero
// block, q = e4m3_rne(clamp(v * 2^-e, +-448)).
//
// ---- THE V^T8 LAYOUT (the one place it is defined; tests/attn_f8_cases.py vt8_offsets mirrors it) ----
//   Vt8[c * ldvt8 + 128 t + kk] = the byte of key 128 t + key_of(kk), channel row c, for tile t < ceil(Lk / 128), kk < 128:
//       g = (kk >> 4) & 3,  w = 4 (kk >> 6) + ((kk >> 2) & 3),  y = kk & 3          key_of(kk) = 16 w + 4 g + y
//   (kk is the k index of v_mfma_scale_f32_16x16x128_f8f6f4: lane group g holds k = 16 g .. + 15 in registers 0-3 and k = 64 + 16 g .. + 15
//   in registers 4-7. A lane (query n, group g) of the transposed score tile S^T = K Q^T ends a 128-key tile holding keys 16 w + 4 g + y in
//   byte y of the w-th packed P register: exactly its B operand of O^T += V^T P^T in this key order, so P never crosses lanes.)
//   Scale block b < 4 of tile t covers kk = 32 b .. 32 b + 31, i.e. keys { 16 w + 4 g + y : w = 4 (b >> 1) .. + 3, g = 2 (b & 1) .. + 1, y < 4 }:
//       Ev[t * ldev + 4 c + b]                   (tile-major: the 512 scale bytes of one head and tile are contiguous)
//   Keys >= Lk of the last tile are written as byte 0x00 and count as zeros in their block's amax (a block of them alone takes byte 127).
// Roofline: HBM. Algorithmic bytes per element: 2 read + 1 1/32 written.
#include "common.hpp"

namespace {

// the MX scale byte of a block whose largest magnitude is am (>= 0), and the fp32 multiplier 2^-e = 2^(127 - byte)
__device__ __forceinline__ int mx_byte(float am, float& mult) {
    // 448 = 1.75 * 2^8: with amax = 1.f * 2^(E - 127) the exponent is E - 127 - 8 where the significand is <= 1.75, else one more (gemm_f8.hpp)
    const unsigned bits = __float_as_uint(am);
    const int E = (int)(bits >> 23);
    int byte = E - 8 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
    byte = am > 0.f ? max(byte, 0) : 127;
    mult = __uint_as_float((unsigned)(254 - byte) << 23);
    return byte;
}

__device__ __forceinline__ unsigned pack4_e4m3(float a, float b, float c, float d, float mult) {
    const float t0 = fminf(fmaxf(a * mult, -448.0f), 448.0f), t1 = fminf(fmaxf(b * mult, -448.0f), 448.0f);
    const float t2 = fminf(fmaxf(c * mult, -448.0f), 448.0f), t3 = fminf(fmaxf(d * mult, -448.0f), 448.0f);
    const int p = __builtin_amdgcn_cvt_pk_fp8_f32(t0, t1, 0, false);
    return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(t2, t3, p, true);
}

// one thread per (row, block of 32 columns): reads bytes [r * ldx * 2 + 64 b, + 64) of x (32 b + 31 < K <= ldx), writes bytes
// [r * ldq + 32 b, + 32) of q (32 b + 31 < K <= ldq) and byte r * lde + b of e (b < K / 32 <= lde); r < R.
__global__ __launch_bounds__(256) void quant_rows_mx_kernel(const unsigned short* __restrict__ x, int64_t ldx, int64_t R, int nb,
                                                            unsigned char* __restrict__ q, int64_t ldq, unsigned char* __restrict__ e, int64_t lde) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= R * nb) return;
    const int64_t r = idx / nb;
    const int b = (int)(idx - r * nb);
    const u32x4* src = reinterpret_cast<const u32x4*>(x + r * ldx + 32 * b);
    float f[32];
    float am = 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const u32x4 w = src[v];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f[8 * v + 2 * j] = __uint_as_float(w[j] << 16);
            f[8 * v + 2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
            am = fmaxf(am, fmaxf(fabsf(f[8 * v + 2 * j]), fabsf(f[8 * v + 2 * j + 1])));
        }
    }
    float mult;
    const int byte = mx_byte(am, mult);
    u32x4* dst = reinterpret_cast<u32x4*>(q + r * ldq + 32 * b);
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = pack4_e4m3(f[16 * v + 4 * j], f[16 * v + 4 * j + 1], f[16 * v + 4 * j + 2], f[16 * v + 4 * j + 3], mult);
        dst[v] = o;
    }
    e[r * lde + b] = (unsigned char)byte;
}

// one thread per (channel row c = blockIdx.y, tile t, scale block b): the 32 keys of the block are eight runs of four consecutive keys
// 128 t + 16 w + 4 g .. + 3 (header). A run wholly inside Lk is one 8-byte load (ldvt % 4 == 0, key % 4 == 0: aligned, key + 3 < Lk <= ldvt);
// a run across Lk is read key by key below Lk; a run beyond Lk is not read. Writes bytes [c * ldvt8 + 128 t + 32 b, + 32)
// (128 t + 32 b + 31 < 128 ntiles <= ldvt8) and byte t * ldev + 4 c + b (4 c + b < 4 C <= ldev, t < ntiles).
__global__ __launch_bounds__(256) void attn_vt_mx_kernel(const unsigned short* __restrict__ vt, int64_t ldvt, int Lk, int ntiles,
                                                         unsigned char* __restrict__ vt8, int64_t ldvt8, unsigned char* __restrict__ ev, int64_t ldev) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 4 * ntiles) return;
    const int c = blockIdx.y;
    const int t = idx >> 2, b = idx & 3;
    const unsigned short* row = vt + (int64_t)c * ldvt;
    float f[32];
    float am = 0.f;
#pragma unroll
    for (int gh = 0; gh < 2; ++gh)
#pragma unroll
        for (int wl = 0; wl < 4; ++wl) {
            const int key = 128 * t + 16 * (4 * (b >> 1) + wl) + 4 * (2 * (b & 1) + gh);
            float* fo = f + 16 * gh + 4 * wl;
            if (key + 3 < Lk) {
                const u32x2 w = *reinterpret_cast<const u32x2*>(row + key);
                fo[0] = __uint_as_float(w[0] << 16);
                fo[1] = __uint_as_float(w[0] & 0xffff0000u);
                fo[2] = __uint_as_float(w[1] << 16);
                fo[3] = __uint_as_float(w[1] & 0xffff0000u);
            } else {
#pragma unroll
                for (int y = 0; y < 4; ++y) fo[y] = key + y < Lk ? bf16_to_f32(row[key + y]) : 0.f;
            }
#pragma unroll
            for (int y = 0; y < 4; ++y) am = fmaxf(am, fabsf(fo[y]));
        }
    float mult;
    const int byte = mx_byte(am, mult);
    u32x4* dst = reinterpret_cast<u32x4*>(vt8 + (int64_t)c * ldvt8 + 128 * t + 32 * b);
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = pack4_e4m3(f[16 * v + 4 * j], f[16 * v + 4 * j + 1], f[16 * v + 4 * j + 2], f[16 * v + 4 * j + 3], mult);
        dst[v] = o;
    }
    ev[(int64_t)t * ldev + 4 * c + b] = (unsigned char)byte;
}

// YUME_NORM_LOG=1 (read once per process): one stderr line per quantiser launch, as quant_rows.hip
bool quant_log() {
    static const bool on = [] { const char* v = getenv("YUME_NORM_LOG"); return v && atoi(v) != 0; }();
    return on;
}

}  // namespace

extern "C" int yume_quant_rows_mx_e4m3(const void* x, int64_t ldx, int64_t R, int64_t K, void* q, int64_t ldq, void* e, int64_t lde, void* stream) {
    YUME_REQUIRE(R >= 0 && K > 0, "quant_rows_mx_e4m3: bad shape R=%lld K=%lld", (long long)R, (long long)K);
    YUME_REQUIRE((K % 32) == 0, "quant_rows_mx_e4m3: K=%lld must be a multiple of 32 (one scale byte per 32 columns)", (long long)K);
    YUME_REQUIRE(K < (1ll << 31) && R < (1ll << 31), "quant_rows_mx_e4m3: dimension too large");
    YUME_REQUIRE((ldx % 8) == 0 && ldx >= K, "quant_rows_mx_e4m3: ldx=%lld must be a multiple of 8 and >= K", (long long)ldx);
    YUME_REQUIRE((ldq % 16) == 0 && ldq >= K, "quant_rows_mx_e4m3: ldq=%lld must be a multiple of 16 and >= K", (long long)ldq);
    YUME_REQUIRE(lde >= K / 32, "quant_rows_mx_e4m3: lde=%lld must be >= K / 32", (long long)lde);
    YUME_REQUIRE(ldx < (1ll << 31) && ldq < (1ll << 31) && lde < (1ll << 31), "quant_rows_mx_e4m3: row pitch too large");
    if (R == 0) return YUME_OK;
    YUME_REQUIRE(x && q && e, "quant_rows_mx_e4m3: NULL pointer");
    YUME_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)q % 16) == 0, "quant_rows_mx_e4m3: x and q must be 16-byte aligned");
    const int64_t blocks = (R * (K / 32) + 255) / 256;
    YUME_REQUIRE(blocks < (1ll << 31), "quant_rows_mx_e4m3: R * K / 32 = %lld blocks is too large", (long long)(R * (K / 32)));
    if (quant_log())
        fprintf(stderr, "[quant] rows_mx R=%lld K=%lld ldx=%lld ldq=%lld lde=%lld\n", (long long)R, (long long)K, (long long)ldx, (long long)ldq, (long long)lde);
    hipLaunchKernelGGL(quant_rows_mx_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x, ldx, R, (int)(K / 32),
                       (unsigned char*)q, ldq, (unsigned char*)e, lde);
    YUME_CHECK_LAUNCH("quant_rows_mx_e4m3");
    return YUME_OK;
}

extern "C" int yume_attn_vt_mx_e4m3(const void* Vt, int64_t ldvt, int64_t C, int64_t Lk, void* Vt8, int64_t ldvt8, void* Ev, int64_t ldev, void* stream) {
    YUME_REQUIRE(Vt && Vt8 && Ev, "attn_vt_mx_e4m3: NULL pointer");
    YUME_REQUIRE(C >= 1 && Lk >= 1, "attn_vt_mx_e4m3: bad shape C=%lld Lk=%lld", (long long)C, (long long)Lk);
    YUME_REQUIRE((C % 128) == 0 && C < 65536, "attn_vt_mx_e4m3: C=%lld must be a multiple of 128 (whole heads) below 65536", (long long)C);
    YUME_REQUIRE(Lk < (1ll << 28), "attn_vt_mx_e4m3: Lk=%lld is too large", (long long)Lk);
    const int64_t ntiles = (Lk + 127) / 128;
    YUME_REQUIRE((ldvt % 4) == 0 && ldvt >= Lk, "attn_vt_mx_e4m3: ldvt=%lld must be a multiple of 4 and >= Lk", (long long)ldvt);
    YUME_REQUIRE((ldvt8 % 16) == 0 && ldvt8 >= 128 * ntiles, "attn_vt_mx_e4m3: ldvt8=%lld must be a multiple of 16 and >= 128 * ceil(Lk / 128) = %lld",
                 (long long)ldvt8, (long long)(128 * ntiles));
    YUME_REQUIRE((ldev % 4) == 0 && ldev >= 4 * C, "attn_vt_mx_e4m3: ldev=%lld must be a multiple of 4 and >= 4 * C = %lld", (long long)ldev, (long long)(4 * C));
    YUME_REQUIRE(ldvt < (1ll << 31) && ldvt8 < (1ll << 31) && ldev < (1ll << 31), "attn_vt_mx_e4m3: row pitch too large");
    YUME_REQUIRE(((uintptr_t)Vt % 8) == 0 && ((uintptr_t)Vt8 % 16) == 0 && ((uintptr_t)Ev % 4) == 0,
                 "attn_vt_mx_e4m3: Vt must be 8-byte, Vt8 16-byte and Ev 4-byte aligned");
    if (quant_log())
        fprintf(stderr, "[quant] vt_mx C=%lld Lk=%lld tiles=%lld ldvt=%lld ldvt8=%lld ldev=%lld\n", (long long)C, (long long)Lk, (long long)ntiles,
                (long long)ldvt, (long long)ldvt8, (long long)ldev);
    hipLaunchKernelGGL(attn_vt_mx_kernel, dim3((unsigned)((4 * ntiles + 255) / 256), (unsigned)C), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned short*)Vt, ldvt, (int)Lk, (int)ntiles, (unsigned char*)Vt8, ldvt8, (unsigned char*)Ev, ldev);
    YUME_CHECK_LAUNCH("attn_vt_mx_e4m3");
    return YUME_OK;
}
