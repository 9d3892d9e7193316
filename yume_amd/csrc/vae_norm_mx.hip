// vae_norm_mx.hip — RMS_norm (+ SiLU) over channels that leaves OCP MX e4m3 instead of bf16: the producer of the fp8 VAE option (r19).
//
//   yume_vae_rmsnorm_silu_mx(x, ..., q, ldq, e, lde)  ==  yume_vae_rmsnorm_silu(x, ..., y, ldy = C) followed by an MX quantiser of y, bit for bit:
//   the value is computed and rounded to bf16 exactly as vae_ops.hip's kernel of the same shape computes it, then quantised per row and per 32
//   consecutive channels with the exponent rule of YUME_EPI_MX_GELU (gemm_f8.hpp, f8_epilogue_mx_gelu): e = the smallest integer with
//   amax <= 448 * 2^e, byte e + 127 (127 for an all-zero block), q = e4m3_rne(clamp(v * 2^-e, +-448)). No bf16 row, no quantiser pass.
//
// The three kernel forms of vae_ops.hip sum a row's squares in three different orders and evaluate SiLU in two ways, so "the value the norm
// would have written" depends on the form the shape takes there. This file therefore carries the same three forms with the same selection
// (rms<LPR,NV>, rms_g<G,NVL,RI>, rms_flat<NVEC,NVL,RI>; YUME_VAE_NORM_G / YUME_VAE_NORM_FLAT read the same way) and the same arithmetic,
// expression for expression; only the store differs. In every form the four 16-byte vectors of a 32-channel block sit in four ADJACENT lanes
// (lane & ~3 .. + 3) at the same vector slot, since C / 8 and every group width are multiples of 4: the block amax is a lane-local max of 8
// and two xor-shuffles (1, 2). Lanes of rows beyond M carry zeros through the shuffles and store nothing.
// Roofline: HBM. Algorithmic bytes per element: 2 read + 1 1/32 written.
#include "common.hpp"

namespace {

// w = the 8 bf16 values of vector `vi` (channels 8 vi .. 8 vi + 7) of one row, as the norm would have stored them. Called by all 64 lanes.
// live lanes write bytes [8 vi, 8 vi + 8) of the row's q (8 vi + 7 < C <= ldq) and, the first lane of a block, scale byte vi / 4 < C / 32 <= lde.
__device__ __forceinline__ void mx_store(const u32x4& w, bool live, unsigned char* qrow, unsigned char* erow, int vi) {
    float f[8];
    float am = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[2 * j] = __uint_as_float(w[j] << 16);
        f[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
        am = fmaxf(am, fmaxf(fabsf(f[2 * j]), fabsf(f[2 * j + 1])));
    }
    am = fmaxf(am, __shfl_xor(am, 1, 64));
    am = fmaxf(am, __shfl_xor(am, 2, 64));
    // 448 = 1.75 * 2^8: with amax = 1.f * 2^(E - 127) the exponent is E - 127 - 8 where the significand is <= 1.75, else one more (gemm_f8.hpp)
    const unsigned bits = __float_as_uint(am);
    const int E = (int)(bits >> 23);
    int byte = E - 8 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
    byte = am > 0.f ? max(byte, 0) : 127;
    const float mult = __uint_as_float((unsigned)(254 - byte) << 23);
    float t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = fminf(fmaxf(f[j] * mult, -448.0f), 448.0f);
    u32x2 o;
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(t[0], t[1], 0, false);
    o[0] = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(t[2], t[3], p, true);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(t[4], t[5], 0, false);
    o[1] = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(t[6], t[7], p, true);
    if (live) {
        *reinterpret_cast<u32x2*>(qrow + 8 * vi) = o;
        if ((vi & 3) == 0) erow[vi >> 2] = (unsigned char)byte;
    }
}

// ---- vae_ops.hip's rmsnorm_silu_kernel<LPR, NV> ----
template <int LPR, int NV>
__global__ __launch_bounds__(256) void rmsnorm_silu_mx_kernel(const unsigned short* x, int64_t ldx, int64_t M, int C, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, int silu_on, unsigned char* q, int64_t ldq,
                                                              unsigned char* e, int64_t lde) {
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR;
    const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + lane / LPR;
    const bool live = row < M;
    const int nvec = C >> 3;
    u16x8 v[NV];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int vi = sub + i * LPR;
        v[i] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (live && vi < nvec) {
            v[i] = *reinterpret_cast<const u16x8*>(x + row * ldx + 8 * vi);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float f = bf16_to_f32(v[i][j]);
                ss += f * f;
            }
        }
    }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float inv = sqrtf((float)C) / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int vi = sub + i * LPR;
        const bool on = live && vi < nvec;                          // (the four lanes of a block agree: nvec % 4 == 0, LPR % 4 == 0)
        u32x4 w = u32x4{0u, 0u, 0u, 0u};
        if (on) {
            const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + 8 * vi);
            const f32x4 g1 = *reinterpret_cast<const f32x4*>(gamma + 8 * vi + 4);
            f32x4 b0 = f32x4{0.f, 0.f, 0.f, 0.f}, b1 = b0;
            if (beta) {
                b0 = *reinterpret_cast<const f32x4*>(beta + 8 * vi);
                b1 = *reinterpret_cast<const f32x4*>(beta + 8 * vi + 4);
            }
            float o[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = bf16_to_f32(v[i][j]) * inv * g0[j] + b0[j];
                o[4 + j] = bf16_to_f32(v[i][4 + j]) * inv * g1[j] + b1[j];
            }
            if (silu_on) {
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = silu(o[j]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = pack_bf16x2(o[2 * j], o[2 * j + 1]);
        }
        mx_store(w, on, q + row * ldq, e + row * lde, vi);
    }
}

__device__ __forceinline__ f32x2_t silu2_fast(f32x2_t x) {
    const f32x2_t k = {-1.4426950408889634f, -1.4426950408889634f}, one = {1.0f, 1.0f};
    const f32x2_t u = x * k;
    const f32x2_t e = {__builtin_amdgcn_exp2f(u[0]), __builtin_amdgcn_exp2f(u[1])};
    const f32x2_t d = e + one;
    const f32x2_t r = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    return x * r;
}

// ---- vae_ops.hip's rmsnorm_silu_g_kernel<G, NVL, RI> ----
template <int G, int NVL, int RI>
__global__ __launch_bounds__(256) void rmsnorm_silu_g_mx_kernel(const unsigned short* x, int64_t ldx, int64_t M, int C, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, int silu_on, unsigned char* q, int64_t ldq,
                                                                unsigned char* e, int64_t lde) {
    static_assert(G % 4 == 0, "a 32-channel block is four adjacent lanes");
    constexpr int RPW = 64 / G;
    const int lane = threadIdx.x & 63;
    const int sub = lane % G;
    const int64_t row0 = (int64_t)blockIdx.x * (RI * 4 * RPW) + (threadIdx.x >> 6) * RPW + lane / G;
    u32x4 v[RI][NVL];
#pragma unroll
    for (int r = 0; r < RI; ++r) {
        const int64_t row = row0 + (int64_t)r * (4 * RPW);
#pragma unroll
        for (int i = 0; i < NVL; ++i) {
            v[r][i] = u32x4{0u, 0u, 0u, 0u};
            if (row < M) v[r][i] = *reinterpret_cast<const u32x4*>(x + row * ldx + 8 * (sub + i * G));
        }
    }
    float inv[RI];
    const float sqrt_c = sqrtf((float)C);
#pragma unroll
    for (int r = 0; r < RI; ++r) {
        f32x2_t s2 = {0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NVL; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x2_t f = {__uint_as_float(v[r][i][j] << 16), __uint_as_float(v[r][i][j] & 0xffff0000u)};
                s2 += f * f;
            }
        float ss = s2[0] + s2[1];
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
        inv[r] = sqrt_c / fmaxf(sqrtf(ss), 1e-12f);
    }
#pragma unroll
    for (int i = 0; i < NVL; ++i) {
        const int c0 = 8 * (sub + i * G);
        f32x2_t g[4], b[4];
        {
            const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + c0), g1 = *reinterpret_cast<const f32x4*>(gamma + c0 + 4);
            g[0] = f32x2_t{g0[0], g0[1]}; g[1] = f32x2_t{g0[2], g0[3]}; g[2] = f32x2_t{g1[0], g1[1]}; g[3] = f32x2_t{g1[2], g1[3]};
            f32x4 b0 = f32x4{0.f, 0.f, 0.f, 0.f}, b1 = b0;
            if (beta) {
                b0 = *reinterpret_cast<const f32x4*>(beta + c0);
                b1 = *reinterpret_cast<const f32x4*>(beta + c0 + 4);
            }
            b[0] = f32x2_t{b0[0], b0[1]}; b[1] = f32x2_t{b0[2], b0[3]}; b[2] = f32x2_t{b1[0], b1[1]}; b[3] = f32x2_t{b1[2], b1[3]};
        }
#pragma unroll
        for (int r = 0; r < RI; ++r) {
            const int64_t row = row0 + (int64_t)r * (4 * RPW);
            const f32x2_t iv = {inv[r], inv[r]};
            u32x4 w;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x2_t f = {__uint_as_float(v[r][i][j] << 16), __uint_as_float(v[r][i][j] & 0xffff0000u)};
                f32x2_t o = (f * iv) * g[j] + b[j];
                if (silu_on) o = silu2_fast(o);
                w[j] = pack_bf16x2(o[0], o[1]);
            }
            mx_store(w, row < M, q + row * ldq, e + row * lde, sub + i * G);
        }
    }
}

// ---- vae_ops.hip's rmsnorm_silu_flat_kernel<NVEC, NVL, RI, SILU, BETA> (x rows contiguous: ldx == C) ----
template <int NVEC, int NVL, int RI, bool SILU, bool BETA>
__global__ __launch_bounds__(256) void rmsnorm_silu_flat_mx_kernel(const unsigned short* x, int64_t M, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, unsigned char* q, int64_t ldq, unsigned char* e,
                                                                   int64_t lde) {
    constexpr int CH = NVL * 64;                 // vectors per chunk
    constexpr int R = CH / NVEC;                 // rows per chunk
    static_assert(R * NVEC == CH && R <= 64 && (NVEC % 4) == 0, "a chunk is whole rows");
    __shared__ __attribute__((aligned(16))) float part[4][RI][CH];
    __shared__ float scale[4][RI][R];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t total = M * NVEC;
    const int64_t vb0 = ((int64_t)blockIdx.x * 4 + wave) * RI * CH;
    u32x4 v[RI][NVL];
#pragma unroll
    for (int r = 0; r < RI; ++r)
#pragma unroll
        for (int i = 0; i < NVL; ++i) {
            const int64_t f = vb0 + r * CH + i * 64 + lane;
            v[r][i] = u32x4{0u, 0u, 0u, 0u};
            if (f < total) v[r][i] = *reinterpret_cast<const u32x4*>(x + 8 * f);
        }
#pragma unroll
    for (int r = 0; r < RI; ++r)
#pragma unroll
        for (int i = 0; i < NVL; ++i) {
            f32x2_t s2 = {0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x2_t f = {__uint_as_float(v[r][i][j] << 16), __uint_as_float(v[r][i][j] & 0xffff0000u)};
                s2 += f * f;
            }
            part[wave][r][i * 64 + lane] = s2[0] + s2[1];
        }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const float sqrt_c = sqrtf((float)(NVEC * 8));
    if (lane < R) {
#pragma unroll
        for (int r = 0; r < RI; ++r) {
            float ss = 0.f;
#pragma unroll
            for (int k = 0; k < NVEC / 4; ++k) {
                const f32x4 p4 = *reinterpret_cast<const f32x4*>(&part[wave][r][lane * NVEC + 4 * k]);
                ss += (p4[0] + p4[1]) + (p4[2] + p4[3]);
            }
            scale[wave][r][lane] = sqrt_c / fmaxf(sqrtf(ss), 1e-12f);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int i = 0; i < NVL; ++i) {
        const int fl = i * 64 + lane;
        const int rowl = fl / NVEC, vi = fl % NVEC, c0 = 8 * vi;
        f32x2_t g[4], b[4];
        {
            const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + c0), g1 = *reinterpret_cast<const f32x4*>(gamma + c0 + 4);
            g[0] = f32x2_t{g0[0], g0[1]}; g[1] = f32x2_t{g0[2], g0[3]}; g[2] = f32x2_t{g1[0], g1[1]}; g[3] = f32x2_t{g1[2], g1[3]};
            if (BETA) {
                const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + c0), b1 = *reinterpret_cast<const f32x4*>(beta + c0 + 4);
                b[0] = f32x2_t{b0[0], b0[1]}; b[1] = f32x2_t{b0[2], b0[3]}; b[2] = f32x2_t{b1[0], b1[1]}; b[3] = f32x2_t{b1[2], b1[3]};
            }
        }
#pragma unroll
        for (int r = 0; r < RI; ++r) {
            const int64_t f = vb0 + r * CH + fl;
            const float inv = scale[wave][r][rowl];
            const f32x2_t iv = {inv, inv};
            u32x4 w;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x2_t ev = {__uint_as_float(v[r][i][j] << 16), __uint_as_float(v[r][i][j] & 0xffff0000u)};
                f32x2_t o = (ev * iv) * g[j];
                if (BETA) o += b[j];
                if (SILU) o = silu2_fast(o);
                w[j] = pack_bf16x2(o[0], o[1]);
            }
            // vector f of the flat stream = row f / NVEC (< M when f < total), vector vi of it: a chunk starts on a row boundary
            const int64_t row = (vb0 + r * CH) / NVEC + rowl;
            mx_store(w, f < total, q + row * ldq, e + row * lde, vi);
        }
    }
}

bool vae_log() {
    static const bool on = [] { const char* v = getenv("YUME_VAE_LOG"); return v && atoi(v) != 0; }();
    return on;
}

}  // namespace

extern "C" int yume_vae_rmsnorm_silu_mx(const void* x, int64_t ldx, int64_t M, int64_t C, const float* gamma, const float* beta, int silu_on,
                                        void* q, int64_t ldq, void* e, int64_t lde, void* stream) {
    YUME_REQUIRE(x && gamma && q && e, "vae_rmsnorm_silu_mx: NULL pointer");
    YUME_REQUIRE(M > 0 && C > 0 && (C % 32) == 0 && C <= 4096, "vae_rmsnorm_silu_mx: C=%lld must be a multiple of 32 and <= 4096", (long long)C);
    YUME_REQUIRE((ldx % 8) == 0 && ldx >= C, "vae_rmsnorm_silu_mx: ldx=%lld must be a multiple of 8 and >= C", (long long)ldx);
    YUME_REQUIRE((ldq % 8) == 0 && ldq >= C, "vae_rmsnorm_silu_mx: ldq=%lld must be a multiple of 8 and >= C", (long long)ldq);
    YUME_REQUIRE((lde % 4) == 0 && lde >= C / 32, "vae_rmsnorm_silu_mx: lde=%lld must be a multiple of 4 and >= C / 32", (long long)lde);
    YUME_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)q % 16) == 0 && ((uintptr_t)gamma % 16) == 0 && ((uintptr_t)beta % 16) == 0,
                 "vae_rmsnorm_silu_mx: x, q, gamma and beta must be 16-byte aligned");
    YUME_REQUIRE(((uintptr_t)e % 4) == 0, "vae_rmsnorm_silu_mx: e must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const unsigned short* xp = (const unsigned short*)x;
    unsigned char* qp = (unsigned char*)q;
    unsigned char* ep = (unsigned char*)e;
    const int nvec = (int)(C / 8);
    const char* form = "";
    int ta = -1, tb = -1, tc = -1;
#define LAUNCH_RMS(LPR, NV)                                                                                             \
    form = "rms"; ta = LPR; tb = NV;                                                                                    \
    hipLaunchKernelGGL((rmsnorm_silu_mx_kernel<LPR, NV>), dim3((unsigned)((M + 4 * (64 / LPR) - 1) / (4 * (64 / LPR)))), \
                       dim3(256), 0, st, xp, ldx, M, (int)C, gamma, beta, silu_on, qp, ldq, ep, lde)
    // the selection of yume_vae_rmsnorm_silu (vae_ops.hip) for y rows C apart, term for term: the bits follow the form
    static const bool grouped = [] { const char* v = getenv("YUME_VAE_NORM_G"); return !v || atoi(v) != 0; }();
    int G = 1;
    while (G < 64 && (nvec % (2 * G)) == 0) G *= 2;               // nvec % 4 == 0: G >= 4
    const int nvl = nvec / G;
#define LAUNCH_RMS_G(GG, NVL, RI)                                                                                                       \
    form = "rms_g"; ta = GG; tb = NVL; tc = RI;                                                                                         \
    hipLaunchKernelGGL((rmsnorm_silu_g_mx_kernel<GG, NVL, RI>), dim3((unsigned)((M + RI * 4 * (64 / GG) - 1) / (RI * 4 * (64 / GG)))), \
                       dim3(256), 0, st, xp, ldx, M, (int)C, gamma, beta, silu_on, qp, ldq, ep, lde)
#define LAUNCH_RMS_GN(NVL, RI)                                                                              \
    switch (G) {                                                                                            \
        case 4: { LAUNCH_RMS_G(4, NVL, RI); } break;   case 8: { LAUNCH_RMS_G(8, NVL, RI); } break;        \
        case 16: { LAUNCH_RMS_G(16, NVL, RI); } break; case 32: { LAUNCH_RMS_G(32, NVL, RI); } break;      \
        default: { LAUNCH_RMS_G(64, NVL, RI); } break;                                                      \
    }
    static const bool flat = [] { const char* v = getenv("YUME_VAE_NORM_FLAT"); return !v || atoi(v) != 0; }();
#define LAUNCH_RMS_F(NVEC, NVL, RI)                                                                                                         \
    do {                                                                                                                                    \
        const unsigned nb = (unsigned)((M * NVEC + (int64_t)4 * RI * NVL * 64 - 1) / ((int64_t)4 * RI * NVL * 64));                         \
        form = "rms_flat"; ta = NVEC; tb = NVL; tc = RI;                                                                                    \
        if (silu_on && !beta) hipLaunchKernelGGL((rmsnorm_silu_flat_mx_kernel<NVEC, NVL, RI, true, false>), dim3(nb), dim3(256), 0, st, xp, M, gamma, beta, qp, ldq, ep, lde); \
        else if (silu_on) hipLaunchKernelGGL((rmsnorm_silu_flat_mx_kernel<NVEC, NVL, RI, true, true>), dim3(nb), dim3(256), 0, st, xp, M, gamma, beta, qp, ldq, ep, lde);      \
        else if (!beta) hipLaunchKernelGGL((rmsnorm_silu_flat_mx_kernel<NVEC, NVL, RI, false, false>), dim3(nb), dim3(256), 0, st, xp, M, gamma, beta, qp, ldq, ep, lde);      \
        else hipLaunchKernelGGL((rmsnorm_silu_flat_mx_kernel<NVEC, NVL, RI, false, true>), dim3(nb), dim3(256), 0, st, xp, M, gamma, beta, qp, ldq, ep, lde);                  \
    } while (0)
    const bool contiguous = ldx == C;                              // (the norm's own y pitch is C here)
    if (grouped && flat && contiguous && nvec == 12) LAUNCH_RMS_F(12, 3, 2);
    else if (grouped && flat && contiguous && nvec == 24) LAUNCH_RMS_F(24, 3, 2);
    else if (grouped && flat && contiguous && nvec == 48) LAUNCH_RMS_F(48, 3, 2);
    else if (grouped && flat && contiguous && nvec == 20) LAUNCH_RMS_F(20, 5, 1);
    else if (grouped && flat && contiguous && nvec == 40) LAUNCH_RMS_F(40, 5, 1);
    else if (grouped && flat && contiguous && nvec == 80) LAUNCH_RMS_F(80, 5, 1);
    else if (grouped && nvl == 1) { LAUNCH_RMS_GN(1, 4); }
    else if (grouped && nvl == 3) { LAUNCH_RMS_GN(3, 2); }
    else if (grouped && nvl == 5) { LAUNCH_RMS_GN(5, 1); }
    else if (nvec <= 8) { LAUNCH_RMS(8, 1); }
    else if (nvec <= 16) { LAUNCH_RMS(16, 1); }
    else if (nvec <= 32) { LAUNCH_RMS(32, 1); }
    else if (nvec <= 64) { LAUNCH_RMS(64, 1); }
    else if (nvec <= 128) { LAUNCH_RMS(64, 2); }
    else if (nvec <= 256) { LAUNCH_RMS(64, 4); }
    else { LAUNCH_RMS(64, 8); }
#undef LAUNCH_RMS_F
#undef LAUNCH_RMS_GN
#undef LAUNCH_RMS_G
#undef LAUNCH_RMS
    if (vae_log()) {
        char name[48];
        if (tc >= 0) snprintf(name, sizeof(name), "%s<%d,%d,%d>", form, ta, tb, tc);
        else snprintf(name, sizeof(name), "%s<%d,%d>", form, ta, tb);
        fprintf(stderr, "[vae] rms_mx %s M=%lld C=%lld ldx=%lld ldq=%lld lde=%lld silu=%d beta=%d\n", name, (long long)M, (long long)C, (long long)ldx,
                (long long)ldq, (long long)lde, silu_on ? 1 : 0, beta ? 1 : 0);
    }
    YUME_CHECK_LAUNCH("vae_rmsnorm_silu_mx");
    return YUME_OK;
}
