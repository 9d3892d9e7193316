// norm_i8.hip — (r25) adaLN straight to int8 rows: yume_adaln_modulate (norm.hip, bf16 output) followed by yume_quant_rows_i8
// (quant_rows_i8.hip; the format: i8.hpp), in one kernel and without the bf16 row. A translation unit of its own: every kernel of norm.hip
// keeps its code object.
// The statistics and the modulated value mirror norm.hip's adaln_kernel<MAXV> / adaln2_kernel expression for expression (same loads, same
// sums in the same order, the same bf16 pack). The workgroup holds the whole row: the row amax of the bf16-ROUNDED values goes through one
// more block reduction (a maximum: exact, order-free), and scale / pre / inv / clamp / round are i8.hpp's functions, the ones the
// stand-alone quantiser calls — so bytes and scales equal the two-call composite bit for bit in both forms (tests/test_norm_i8_gpu.py).
// Both forms of the call run here: the modulated form (add_one = 1, row_idx) and the norm3 affine form (add_one = 0, tab_stride = 0).
// Roofline: HBM. Algorithmic bytes per token: 4C read + C + 4 write.
#include "i8.hpp"

namespace {

constexpr int NT = 256;

__device__ __forceinline__ float block_sum(float v, float* red /*[8]*/) {
    v = wave_sum(v);
    const int wid = threadIdx.x >> 6;
    __syncthreads();  // protect `red` against the previous use
    if ((threadIdx.x & 63) == 0) red[wid] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) t += red[i];
    return t;
}

__device__ __forceinline__ void block_sum2(float& a, float& b, float* red /*[16]*/) {
    a = wave_sum(a);
    b = wave_sum(b);
    const int wid = threadIdx.x >> 6;
    __syncthreads();  // protect `red` against the previous use
    if ((threadIdx.x & 63) == 0) { red[wid] = a; red[8 + wid] = b; }
    __syncthreads();
    float ta = 0.f, tb = 0.f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) { ta += red[i]; tb += red[8 + i]; }
    a = ta;
    b = tb;
}

__device__ __forceinline__ float block_max(float v, float* red /*[8]*/) {
    v = wave_max(v);
    const int wid = threadIdx.x >> 6;
    __syncthreads();  // protect `red` against the previous use
    if ((threadIdx.x & 63) == 0) red[wid] = v;
    __syncthreads();
    float t = red[0];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) t = fmaxf(t, red[i]);
    return t;
}

__device__ __forceinline__ void block_max2(float& a, float& b, float* red /*[16]*/) {
    a = wave_max(a);
    b = wave_max(b);
    const int wid = threadIdx.x >> 6;
    __syncthreads();  // protect `red` against the previous use
    if ((threadIdx.x & 63) == 0) { red[wid] = a; red[8 + wid] = b; }
    __syncthreads();
    float ta = red[0], tb = red[8];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) { ta = fmaxf(ta, red[i]); tb = fmaxf(tb, red[8 + i]); }
    a = ta;
    b = tb;
}

// adaln_kernel<MAXV> (LayerNorm form) up to the modulated, bf16-rounded row, then the quantiser. A thread's vector vi covers columns
// 4 vi .. 4 vi + 3 < C: bytes [4 vi, 4 vi + 4) of q row t (ldq >= C), one dword store.
template <int MAXV>
__global__ __launch_bounds__(NT) void adaln_i8_kernel(const float* __restrict__ x, int64_t ldx, int C, float eps,
                                                      const float* __restrict__ mul, const float* __restrict__ add,
                                                      int64_t tab_stride, const int32_t* __restrict__ row_idx,
                                                      float add_one, unsigned char* __restrict__ qo, int64_t ldq,
                                                      float* __restrict__ scale) {
    __shared__ float red[8];
    const int64_t t = blockIdx.x;
    const float* xr = x + t * ldx;
    const int nvec = C >> 2;
    f32x4 v[MAXV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int vi = threadIdx.x + i * NT;
        if (vi < nvec) {
            v[i] = *reinterpret_cast<const f32x4*>(xr + 4 * vi);
            s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
        } else {
            v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    constexpr bool HOIST = MAXV <= 3;
    const int64_t row = row_idx ? (int64_t)row_idx[t] : 0;
    const float* mr = mul + row * tab_stride;
    const float* ar = add + row * tab_stride;
    f32x4 m4v[MAXV], a4v[MAXV];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int vi = threadIdx.x + i * NT;
        if (HOIST && vi < nvec) {
            m4v[i] = *reinterpret_cast<const f32x4*>(mr + 4 * vi);
            a4v[i] = *reinterpret_cast<const f32x4*>(ar + 4 * vi);
        }
    }
    const float mean = block_sum(s, red) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int vi = threadIdx.x + i * NT;
        if (vi < nvec) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = v[i][j] - mean;
                q += d * d;
            }
        }
    }
    const float var = block_sum(q, red) / (float)C;
    const float rstd = rsqrtf(var + eps);
    u32x2 hb[MAXV];
    unsigned mb = 0u;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int vi = threadIdx.x + i * NT;
        hb[i] = u32x2{0u, 0u};
        if (vi < nvec) {
            const f32x4 m4 = HOIST ? m4v[i] : *reinterpret_cast<const f32x4*>(mr + 4 * vi);
            const f32x4 a4 = HOIST ? a4v[i] : *reinterpret_cast<const f32x4*>(ar + 4 * vi);
            f32x4 y;
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = (v[i][j] - mean) * rstd * (m4[j] + add_one) + a4[j];
            hb[i][0] = pack_bf16x2(y[0], y[1]);
            hb[i][1] = pack_bf16x2(y[2], y[3]);
            mb = i8::absbits2(hb[i][1], i8::absbits2(hb[i][0], mb));
        }
    }
    const i8::RowScale rs = i8::row_scale(block_max(i8::row_amax(mb), red));
    if (threadIdx.x == 0) scale[t] = rs.scale;
    unsigned char* qr = qo + t * ldq;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int vi = threadIdx.x + i * NT;
        if (vi < nvec) *reinterpret_cast<unsigned*>(qr + 4 * vi) = i8::quant4(hb[i], rs);
    }
}

// adaln2_kernel's two rows per workgroup, then the quantiser on both: per row the arithmetic of adaln_i8_kernel<3> in the same order
__global__ __launch_bounds__(NT) void adaln2_i8_kernel(const float* __restrict__ x, int64_t ldx, int T, int C, float eps,
                                                       const float* __restrict__ mul, const float* __restrict__ add,
                                                       int64_t tab_stride, const int32_t* __restrict__ row_idx,
                                                       float add_one, unsigned char* __restrict__ qo, int64_t ldq,
                                                       float* __restrict__ scale) {
    constexpr int MAXV = 3;
    __shared__ float red[16];
    const int64_t t0 = 2 * (int64_t)blockIdx.x;
    const bool two = t0 + 1 < T;                                   // (uniform) the last block of an odd T holds one row
    const int64_t tr[2] = {t0, two ? t0 + 1 : t0};
    const int nvec = C >> 2;
    f32x4 v[2][MAXV], m4v[2][MAXV], a4v[2][MAXV];
    float s[2] = {0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int vi = threadIdx.x + i * NT;
            if (vi < nvec) {
                v[r][i] = *reinterpret_cast<const f32x4*>(x + tr[r] * ldx + 4 * vi);
            } else {
                v[r][i] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    const int64_t mrow[2] = {row_idx ? (int64_t)row_idx[tr[0]] : 0, row_idx ? (int64_t)row_idx[tr[1]] : 0};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (r == 1 && mrow[1] == mrow[0]) {
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                m4v[1][i] = m4v[0][i];
                a4v[1][i] = a4v[0][i];
            }
            break;
        }
        const float* mr = mul + mrow[r] * tab_stride;
        const float* ar = add + mrow[r] * tab_stride;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int vi = threadIdx.x + i * NT;
            if (vi < nvec) {
                m4v[r][i] = *reinterpret_cast<const f32x4*>(mr + 4 * vi);
                a4v[r][i] = *reinterpret_cast<const f32x4*>(ar + 4 * vi);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < MAXV; ++i) s[r] += (v[r][i][0] + v[r][i][1]) + (v[r][i][2] + v[r][i][3]);
    block_sum2(s[0], s[1], red);
    const float mean[2] = {s[0] / (float)C, s[1] / (float)C};
    float q[2] = {0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int vi = threadIdx.x + i * NT;
            if (vi < nvec) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float d = v[r][i][j] - mean[r];
                    q[r] += d * d;
                }
            }
        }
    block_sum2(q[0], q[1], red);
    u32x2 hb[2][MAXV];
    unsigned mb[2] = {0u, 0u};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const float rstd = rsqrtf(q[r] / (float)C + eps);
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int vi = threadIdx.x + i * NT;
            hb[r][i] = u32x2{0u, 0u};
            if (vi < nvec) {
                f32x4 y;
#pragma unroll
                for (int j = 0; j < 4; ++j) y[j] = (v[r][i][j] - mean[r]) * rstd * (m4v[r][i][j] + add_one) + a4v[r][i][j];
                hb[r][i][0] = pack_bf16x2(y[0], y[1]);
                hb[r][i][1] = pack_bf16x2(y[2], y[3]);
                mb[r] = i8::absbits2(hb[r][i][1], i8::absbits2(hb[r][i][0], mb[r]));
            }
        }
    }
    float am[2] = {i8::row_amax(mb[0]), i8::row_amax(mb[1])};
    block_max2(am[0], am[1], red);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (r == 1 && !two) break;                                  // (uniform)
        const i8::RowScale rs = i8::row_scale(am[r]);
        if (threadIdx.x == 0) scale[tr[r]] = rs.scale;
        unsigned char* qr = qo + tr[r] * ldq;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int vi = threadIdx.x + i * NT;
            if (vi < nvec) *reinterpret_cast<unsigned*>(qr + 4 * vi) = i8::quant4(hb[r][i], rs);
        }
    }
}

// YUME_NORM_LOG=1: one stderr line per launch, in the form of norm.hip's (read once per process)
bool norm_log() {
    static const bool on = [] { const char* v = getenv("YUME_NORM_LOG"); return v && atoi(v) != 0; }();
    return on;
}

}  // namespace

extern "C" int yume_adaln_modulate_i8(const float* x, int64_t ldx, int64_t T, int64_t C, float eps, const float* mul,
                                      const float* add, int64_t tab_stride, const int32_t* row_idx, int add_one,
                                      void* q, int64_t ldq, float* scale, void* stream) {
    YUME_REQUIRE(T >= 0 && C > 0 && C <= 8192, "adaln_modulate_i8: bad shape T=%lld C=%lld (C <= 8192)", (long long)T, (long long)C);
    YUME_REQUIRE((C % 16) == 0, "adaln_modulate_i8: C=%lld must be a multiple of 16", (long long)C);
    YUME_REQUIRE((ldq % 16) == 0 && ldq >= C, "adaln_modulate_i8: ldq=%lld must be a multiple of 16 and >= C", (long long)ldq);
    YUME_REQUIRE((ldx % 4) == 0 && (tab_stride % 4) == 0, "adaln_modulate_i8: strides must be multiples of 4");
    if (T == 0) return YUME_OK;
    YUME_REQUIRE(x && mul && add && q && scale, "adaln_modulate_i8: NULL pointer");
    YUME_REQUIRE(((uintptr_t)q % 16) == 0 && ((uintptr_t)scale % 4) == 0, "adaln_modulate_i8: q must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const float one = add_one ? 1.f : 0.f;
    dim3 grid((unsigned)T), block(NT);
    // the instance choice of yume_adaln_modulate at out_kind = 0, the same environment switch included
    static const bool two_rows = [] { const char* v = getenv("YUME_NORM_TWO_ROWS"); return !v || atoi(v) != 0; }();
    const bool use2 = two_rows && C <= NT * 4 * 3 && T >= 1024 && T < (1ll << 31);
    const int maxv = C <= NT * 4 * 3 ? 3 : C <= NT * 4 * 5 ? 5 : 8;
    if (norm_log()) {
        char name[32];
        if (use2) snprintf(name, sizeof(name), "adaln2_i8");
        else snprintf(name, sizeof(name), "adaln_i8<%d>", maxv);
        fprintf(stderr, "[norm] %s T=%lld C=%lld ldx=%lld ldq=%lld tab_stride=%lld row_idx=%d\n", name, (long long)T, (long long)C, (long long)ldx,
                (long long)ldq, (long long)tab_stride, row_idx ? 1 : 0);
    }
    unsigned char* qo = (unsigned char*)q;
    if (use2)
        hipLaunchKernelGGL(adaln2_i8_kernel, dim3((unsigned)((T + 1) / 2)), block, 0, st, x, ldx, (int)T, (int)C, eps, mul, add, tab_stride, row_idx, one,
                           qo, ldq, scale);
    else if (maxv == 3)
        hipLaunchKernelGGL(adaln_i8_kernel<3>, grid, block, 0, st, x, ldx, (int)C, eps, mul, add, tab_stride, row_idx, one, qo, ldq, scale);
    else if (maxv == 5)
        hipLaunchKernelGGL(adaln_i8_kernel<5>, grid, block, 0, st, x, ldx, (int)C, eps, mul, add, tab_stride, row_idx, one, qo, ldq, scale);
    else
        hipLaunchKernelGGL(adaln_i8_kernel<8>, grid, block, 0, st, x, ldx, (int)C, eps, mul, add, tab_stride, row_idx, one, qo, ldq, scale);
    YUME_CHECK_LAUNCH("adaln_modulate_i8");
    return YUME_OK;
}
