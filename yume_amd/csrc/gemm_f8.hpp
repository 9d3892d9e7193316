// gemm_f8.hpp — the e4m3 x e4m3 GEMM of the fp8 FFN option (r15):   acc[m,n] = sum_k Aq[m,k] * Wq[n,k]  (fp32),
//   y = acc * sa[m] * sw[n] + bias[n],  then the epilogue (BF16 / GELU tanh / F32 / RESID, as gemm_core.hpp defines them).
//
// Structure: gemm_w4.hpp's tile and wave layout, gemm128_kernel's (gemm_core.hpp) loop.
//   * ONE 256 x 256 output tile per workgroup, 4 waves (2 x 2), wave (wr, wc) owns rows wr*128 + [0,128), columns wc*128 + [0,128): 8 x 8
//     accumulator tiles of 16 x 16. No tickets, flags or any other hand-off between workgroups; the grid is tiles_m * tiles_n, walked in
//     the 8-XCD patch order of the bf16 kernels (xcd_chunk + tile_origin).
//   * a K tile is 128 BYTES of every row (one MFMA k-step): each operand tile is a row-major [256][128 B] LDS image = 32 KiB, two buffers of
//     A | W = 128 KiB, staged by LDS-DMA (global_load_lds_dwordx4, 16 B per lane), the bank swizzle of gemm_core.hpp applied on the SOURCE
//     address (16-byte chunk position c of row r holds logical chunk c ^ (r & 7)). Ragged M / N rows are loaded from the CLAMPED row
//     min(row, M - 1) / min(row, N - 1): never past the operand.
//   * v_mfma_scale_f32_16x16x128_f8f6f4 with both formats e4m3 and both E8M0 scale bytes 0x7f (= 1.0): the instruction is used for its rate
//     (2x the bf16 form per clock), the real per-row / per-channel fp32 scales are applied in the epilogue.
//     Operand map (established with the exact-integer pattern rows of tests/gemm_f8_cases.py, profiles/r15_fp8_ffn.md): lane l holds row l & 15
//     and the 32 bytes k = 32 (l >> 4) .. + 31 of both operands, in memory order. The W fragment is the FIRST operand, so a lane ends with
//     C[m = .. + (l & 15)][n = .. + 4 (l >> 4) + 0..3] (the SWAP orientation of gemm_w4.hpp: four consecutive columns per lane).
//   * loop: tile kt+1 is staged into the other buffer while tile kt is multiplied; one `vmcnt(0)` + one barrier per K tile (the barrier says
//     both "tile kt has landed for every wave" and "every wave has read the buffer tile kt+1 goes into"). The schedule inside a K tile is the
//     compiler's (64 MFMAs against 32 ds_read_b128): this kernel is the correctness-first form of the issue's build order with the double
//     buffer added; a hand-placed schedule in the manner of gemm_w4.hpp is the next step once the A/B numbers say where the time goes.
//   * epilogue: bf16 outputs with ldo % 8 == 0 leave through gemm_w4.hpp's LDS image as whole rows (w4_image_offsets / w4_store_image: the
//     same code, ragged M / N included); everything else through gemm_core.hpp's guarded store_row4 (the RESID read-modify-write and GELU
//     arithmetic tests/gemm_cases.py bounds).
// Roofline: MFMA fp8 dense; 2*M*N*K flop per launch.
#pragma once
#include "gemm_w4.hpp"

namespace gemm_f8 {
using namespace gemm_core;

typedef __attribute__((ext_vector_type(8))) int i32x8;

constexpr int F8_BK = 128;                    // bytes = elements of K per tile
constexpr int F8_NTHR = 256;
constexpr int F8_OPER = 256 * F8_BK;          // 32 KiB: one operand of one K tile
constexpr int F8_BUF = 2 * F8_OPER;           // A | W
constexpr int F8_LDS = 2 * F8_BUF;            // 128 KiB (the bf16 output image of the epilogue is 256 x 512 B = 128 KiB too)

struct F8Args {
    const unsigned char* A; int64_t lda; const float* sa;
    const unsigned char* W; int64_t ldw; const float* sw;
};

// the 16 pieces of one K tile of this wave: piece j of an operand = tile rows 32 j + 8 wave + (lane >> 3), chunk position lane & 7.
// ga[j] / gw[j] point at the lane's 16 source bytes of K tile 0; koff = 128 * kt.
//   A: bytes [row * lda + koff + 16 c, + 16) with row = min(m0 + r, M - 1) <= M - 1, c <= 7 and koff + 128 <= K <= lda: inside row `row` of A.
//   W: the same with N, ldw.
__device__ __forceinline__ void f8_stage(const unsigned char* const (&ga)[8], const unsigned char* const (&gw)[8], int koff, char* buf, int wave) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
        __builtin_amdgcn_global_load_lds((gbl_cvoid*)(ga[j] + koff), (lds_void*)(buf + j * 4096 + wave * 1024), 16, 0, 0);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        __builtin_amdgcn_global_load_lds((gbl_cvoid*)(gw[j] + koff), (lds_void*)(buf + F8_OPER + j * 4096 + wave * 1024), 16, 0, 0);
}

// fragment of tile rows row0 + (lane & 15): logical chunks 2 q and 2 q + 1 (q = lane >> 4) sit at positions (2 q) ^ (lane & 7) and that ^ 1
__device__ __forceinline__ i32x8 f8_frag(const char* oper, int row, int lane) {
    const int q = lane >> 4;
    const char* rp = oper + row * F8_BK;
    const u32x4 lo = *reinterpret_cast<const u32x4*>(rp + ((((2 * q) ^ row) & 7) << 4));
    const u32x4 hi = *reinterpret_cast<const u32x4*>(rp + ((((2 * q + 1) ^ row) & 7) << 4));
    return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

template <int EPI>
__device__ __forceinline__ void f8_epilogue(const f32x4 (&acc)[8][8], const Problem& p, const F8Args& f, const Epilogue& e, int m0, int n0, char* smem) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    // the lane's rows m0 + wr*128 + 16 i + l15 and column quads n0 + wc*128 + 16 j + 4 l4 (+ 0..3). Scales and bias are read at the CLAMPED
    // row / for quads inside N only (N % 4 == 0: a quad is inside or outside as a whole); values of rows / quads outside are never stored.
    // (column quad j's scale and bias are loaded inside the j loop: all 16 vectors hoisted in front of it were 64 more live registers beside the
    // 256 accumulators, and the register allocator spilled)
    float sa[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) sa[i] = f.sa[min(m0 + wr * 128 + 16 * i + l15, p.M - 1)];
    auto col = [&](int j, f32x4& sw, f32x4& b) {
        const int n = n0 + wc * 128 + 16 * j + 4 * l4;
        sw = n < p.N ? *reinterpret_cast<const f32x4*>(f.sw + n) : f32x4{1.f, 1.f, 1.f, 1.f};
        b = (e.bias && n < p.N) ? *reinterpret_cast<const f32x4*>(e.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    constexpr bool BF16_OUT = EPI == YUME_EPI_BF16 || EPI == YUME_EPI_BF16_GELU;
    if (BF16_OUT && (e.ldo % 8) == 0) {                            // (workgroup-uniform)
        const gemm_w4::ImageOff io = gemm_w4::w4_image_offsets(wr, wc, l15, l4);
        __syncthreads();                                            // every wave is done with the operand buffers: the image reuses them
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            f32x4 sw, b;
            col(j, sw, b);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const f32x4 v = gemm_w4::w4_act<EPI>((acc[i][j] * sa[i]) * sw + b);
                u32x2 o;
                o[0] = pack_bf16x2(v[0], v[1]);
                o[1] = pack_bf16x2(v[2], v[3]);
                *reinterpret_cast<u32x2*>(smem + ((i & 1) ? io.o[j] : io.e[j]) + i * 8192) = o;
            }
        }
        __syncthreads();
        // stores rows m0 .. m0 + min(256, M - m0) - 1, columns n0 .. n0 + min(256, N - n0) - 1 of out (w4_store_image guards both)
        gemm_w4::w4_store_image(smem, reinterpret_cast<unsigned short*>(e.out), e.ldo, m0, min(256, p.M - m0), n0, min(256, p.N - n0));
        return;
    }
    Epilogue e0 = e;
    e0.bias = nullptr;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        f32x4 sw, b;
        col(j, sw, b);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int m = m0 + wr * 128 + 16 * i + l15, n = n0 + wc * 128 + 16 * j + 4 * l4;
            if (m < p.M && n < p.N) store_row4<EPI>((acc[i][j] * sa[i]) * sw + b, m, n, p, e0);      // out[m, n .. n + 3], n + 3 < N
        }
    }
}

// One instance per epilogue, as gemm_core.hpp's kernels: the K loop is the compiler's and small, four copies of it cost code size only.
template <int EPI>
__global__ __launch_bounds__(F8_NTHR, 1) void gemm_f8_kernel(Problem p, F8Args f, Epilogue e) {
    __shared__ __attribute__((aligned(16))) char smem[F8_LDS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    int start, count, m0, n0;
    xcd_chunk(p.tiles_m * p.tiles_n, blockIdx.x & 7, start, count);
    tile_origin(p, start + (blockIdx.x >> 3), m0, n0);             // m0 < M, n0 < N: the grid is exactly tiles_m * tiles_n

    const unsigned char* ga[8];
    const unsigned char* gw[8];
    {
        const int rl = 8 * wave + (lane >> 3);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = 32 * j + rl;                              // tile row 0..255; r & 7 = lane >> 3 & 7
            const int ch = ((lane & 7) ^ (r & 7)) << 4;             // source byte offset inside the 128-byte K slice: 0..112
            ga[j] = f.A + (int64_t)min(m0 + r, p.M - 1) * f.lda + ch;
            gw[j] = f.W + (int64_t)min(n0 + r, p.N - 1) * f.ldw + ch;
        }
    }
    f32x4 acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = p.K / F8_BK;
    f8_stage(ga, gw, 0, smem, wave);
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's pieces of tile kt have landed ...
        __syncthreads();                                            // ... every wave's have, and every wave is done reading the other buffer
        if (kt + 1 < nk) f8_stage(ga, gw, (kt + 1) * F8_BK, smem + (cur ^ 1) * F8_BUF, wave);
        const char* At = smem + cur * F8_BUF;
        const char* Wt = At + F8_OPER;
        i32x8 a[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = f8_frag(At, wr * 128 + 16 * i + (lane & 15), lane);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const i32x8 w = f8_frag(Wt, wc * 128 + 16 * j + (lane & 15), lane);
#pragma unroll
            for (int i = 0; i < 8; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, a[i], acc[i][j], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
        }
        cur ^= 1;
    }
    f8_epilogue<EPI>(acc, p, f, e, m0, n0, smem);
}

inline int launch_f8(int epi, Problem p, const F8Args& f, const Epilogue& e, hipStream_t st) {
    p.tiles_m = (p.M + 255) / 256;
    p.tiles_n = (p.N + 255) / 256;
    p.group_m = g_group_m;
    const dim3 grid((unsigned)(p.tiles_m * p.tiles_n)), block(F8_NTHR);
    switch (epi) {
        case YUME_EPI_BF16_GELU: hipLaunchKernelGGL(gemm_f8_kernel<YUME_EPI_BF16_GELU>, grid, block, 0, st, p, f, e); break;
        case YUME_EPI_F32: hipLaunchKernelGGL(gemm_f8_kernel<YUME_EPI_F32>, grid, block, 0, st, p, f, e); break;
        case YUME_EPI_RESID: hipLaunchKernelGGL(gemm_f8_kernel<YUME_EPI_RESID>, grid, block, 0, st, p, f, e); break;
        default: hipLaunchKernelGGL(gemm_f8_kernel<YUME_EPI_BF16>, grid, block, 0, st, p, f, e); break;
    }
    YUME_CHECK_LAUNCH("gemm_f8");
    return YUME_OK;
}

}  // namespace gemm_f8
