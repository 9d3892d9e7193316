// gemm_i8.hpp — (r25) the int8 x int8 GEMM of the int8 QKV option:   acc[m,n] = sum_k Aq[m,k] * Wq[n,k]  (int32, EXACT),
//   y = float(acc) * sa[m] * sw[n] + bias[n],  then the epilogue: BF16 / F32, and SPLITT (q | k row-major, V as the K-major V^T image)
//   through yume_gemm_i8_splitt. The operands are the rows of i8.hpp: signed bytes, one fp32 scale per row / per output channel.
//
// Structure: gemm_f8_kernel's (gemm_f8.hpp), unchanged — ONE 256 x 256 output tile per workgroup, 4 waves (2 x 2), 128-byte K tiles, two
// LDS-DMA buffers of A | W (128 KiB), the bank swizzle on the source address, ragged M / N rows loaded from the CLAMPED row, the 8-XCD patch
// order, one `vmcnt(0)` + one barrier per K tile. No tickets, flags or any other hand-off between workgroups. f8_stage and f8_frag are
// called as they are: the bytes, the tile and the LDS access pattern are the e4m3 kernel's.
//   * v_mfma_i32_16x16x64_i8, TWO per 16 x 16 tile and K tile into one i32x4 accumulator: f8_frag's two 16-byte reads (logical chunks 2 q
//     and 2 q + 1 of the 128-byte row, q = lane >> 4) feed one instruction each. Both operands take the same chunk into the same
//     instruction, so whatever k order the instruction gives a lane's 16 bytes, byte k of A meets byte k of W. The rate is the scaled e4m3
//     instruction's: 2x the bf16 form per clock and byte.
//     Operand map (pinned by the exact-integer pattern rows of tests/gemm_i8_cases.py, profiles/r25_int8_qkv.md): lane l holds row l & 15
//     of both operands, bytes SIGNED. The W fragment is the FIRST operand, so a lane ends with C[m = .. + (l & 15)][n = .. + 4 (l >> 4) + 0..3]
//     (the SWAP orientation of gemm_w4.hpp / gemm_f8.hpp: four consecutive columns per lane).
//   * the eight tiles of a column j take their first instruction one behind the other, then their second: a tile's two dependent
//     instructions are eight issues apart.
//   * |acc| <= 127 * 128 * K (the byte 0x80 included): K <= 131072 keeps it below 2^31. The sum is exact — no order, no rounding.
//   * epilogue: the accumulators are converted to fp32 (v_cvt_f32_i32: round to nearest even, exact below 2^24) and handed to
//     gemm_f8::f8_epilogue / f8_epilogue_vt as they are — the stores tests/gemm_f8_cases.py and gemm_f8_splitt_cases.py bound.
// Roofline: MFMA int8 dense; 2*M*N*K integer operations per launch.
#pragma once
#include "gemm_f8.hpp"

namespace gemm_i8 {
using namespace gemm_core;
using gemm_f8::F8Args;
using gemm_f8::F8_BK;
using gemm_f8::F8_BUF;
using gemm_f8::F8_LDS;
using gemm_f8::F8_NTHR;
using gemm_f8::F8_OPER;
using gemm_f8::i32x8;

constexpr int64_t I8_MAX_K = 131072;

template <int EPI>
__global__ __launch_bounds__(F8_NTHR, 1) void gemm_i8_kernel(Problem p, F8Args f, Epilogue e) {
    __shared__ __attribute__((aligned(16))) char smem[F8_LDS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    int start, count, m0, n0;
    xcd_chunk(p.tiles_m * p.tiles_n, blockIdx.x & 7, start, count);
    tile_origin(p, start + (blockIdx.x >> 3), m0, n0);             // m0 < M, n0 < N: the grid is exactly tiles_m * tiles_n

    // the lane's 16 source bytes of each of its 16 pieces of K tile 0 (gemm_f8::f8_stage's contract):
    //   A: bytes [row * lda + 128 kt + 16 c, + 16) with row = min(m0 + r, M - 1) <= M - 1, c <= 7 and 128 kt + 128 <= K <= lda: inside row `row`
    //   W: the same with N, ldw.
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
    i32x4 acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = i32x4{0, 0, 0, 0};

    const int nk = p.K / F8_BK;
    gemm_f8::f8_stage(ga, gw, 0, smem, wave);
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's pieces of tile kt have landed ...
        __syncthreads();                                            // ... every wave's have, and every wave is done reading the other buffer
        if (kt + 1 < nk) gemm_f8::f8_stage(ga, gw, (kt + 1) * F8_BK, smem + (cur ^ 1) * F8_BUF, wave);
        const char* At = smem + cur * F8_BUF;
        const char* Wt = At + F8_OPER;
        i32x8 a[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = gemm_f8::f8_frag(At, wr * 128 + 16 * i + (lane & 15), lane);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const i32x8 w = gemm_f8::f8_frag(Wt, wc * 128 + 16 * j + (lane & 15), lane);
            const i32x4 wlo = {w[0], w[1], w[2], w[3]}, whi = {w[4], w[5], w[6], w[7]};
#pragma unroll
            for (int i = 0; i < 8; ++i)                             // chunk 2 q of both operands
                acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wlo, i32x4{a[i][0], a[i][1], a[i][2], a[i][3]}, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 8; ++i)                             // chunk 2 q + 1 of both operands
                acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(whi, i32x4{a[i][4], a[i][5], a[i][6], a[i][7]}, acc[i][j], 0, 0, 0);
        }
        cur ^= 1;
    }
    f32x4 accf[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) accf[i][j] = f32x4{(float)acc[i][j][0], (float)acc[i][j][1], (float)acc[i][j][2], (float)acc[i][j][3]};
    gemm_f8::f8_epilogue<EPI>(accf, p, f, e, m0, n0, smem);
}

inline int launch_i8(int epi, Problem p, const F8Args& f, const Epilogue& e, hipStream_t st) {
    p.tiles_m = (p.M + 255) / 256;
    p.tiles_n = (p.N + 255) / 256;
    p.group_m = g_group_m;
    const dim3 grid((unsigned)(p.tiles_m * p.tiles_n)), block(F8_NTHR);
    switch (epi) {
        case YUME_EPI_F32: hipLaunchKernelGGL(gemm_i8_kernel<YUME_EPI_F32>, grid, block, 0, st, p, f, e); break;
        case YUME_EPI_BF16_SPLITT: hipLaunchKernelGGL(gemm_i8_kernel<YUME_EPI_BF16_SPLITT>, grid, block, 0, st, p, f, e); break;
        default: hipLaunchKernelGGL(gemm_i8_kernel<YUME_EPI_BF16>, grid, block, 0, st, p, f, e); break;
    }
    YUME_CHECK_LAUNCH("gemm_i8");
    return YUME_OK;
}

}  // namespace gemm_i8
