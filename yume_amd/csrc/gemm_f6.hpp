// gemm_f6.hpp — the OCP MXFP6 e2m3 x e2m3 GEMM of the fp6 FFN option (r23): both operands packed e2m3 (mx6.hpp) with one E8M0 byte per row
// and 32 consecutive k,
//     acc[m, n] = sum_b 2^(ea[m, b] - 127) 2^(ew[n, b] - 127) sum_{k in block b} A[m, k] W[n, k]   (fp32),     y = acc + bias[n],
// then the epilogue: F32 / RESID as gemm_core.hpp defines them (gate, row_idx, gate_stride), or YUME_EPI_MX6_GELU (the producer entry).
//
// Structure: gemm_f8_mx_kernel's (gemm_f8.hpp) tile, wave layout and loop.
//   * ONE 256 x 256 output tile per workgroup, 4 waves (2 x 2), wave (wr, wc) owns rows wr*128 + [0,128), columns wc*128 + [0,128): 8 x 8
//     accumulator tiles of 16 x 16. Nothing is handed between workgroups; the grid is tiles_m * tiles_n in the 8-XCD patch order.
//   * a K tile is 128 values = 96 BYTES of every row: each operand tile is a row-major [256][96 B] LDS image = 24 KiB, two buffers of A | W =
//     96 KiB, staged by LDS-DMA (global_load_lds_dwordx4) in 16-byte pieces: 1536 per operand, six per thread. The LDS destination of one
//     instruction is wave-uniform base + lane * 16, so the image is LINEAR: piece P = 64 (4 j + wave) + lane is bytes [16 P, 16 P + 16) = row
//     P / 6, piece P % 6 of that row. NO bank rotation is applied (six pieces per row is no power of two: gemm_core.hpp's XOR does not carry
//     over; profiles/r23_fp6_ffn.md has what was and was not measured). Ragged M / N rows are loaded from the CLAMPED row min(row, M - 1) /
//     min(row, N - 1): never past the operand.
//   * v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz = blgp = 2 (e2m3), six-register operands. Operand map (tools/ubench/mfma_f6_map.hip,
//     profiles/r23_fp6_ffn.md, pinned by the pattern rows of tests/gemm_f6_cases.py): lane l holds row l & 15 and the 32 values k = 32 (l >> 4)
//     .. + 31 of both operands = the row's bytes [24 (l >> 4), + 24) in memory order; scale selector 0 takes byte 0 of the lane's scale
//     register for row l & 15, k-block l >> 4 of its side. The W fragment is the FIRST operand: a lane ends with C[m = .. + (l & 15)]
//     [n = .. + 4 (l >> 4) + 0..3]. The fragment is read as three 8-byte pieces at 24 q + {0, 8, 16}: none straddles a 16-byte piece.
//   * the scale bytes of BOTH operands travel outside the LDS-DMA stream, as gemm_f8_mx_kernel's activations' do: one 16-byte load per row
//     and four K tiles, issued right after the barrier and before that iteration's stage (A's in K tile 4 g + 1, W's in 4 g + 2), packed one
//     K tile later behind the vmcnt(0) the stage needed anyway — no wait of their own falls between a stage and its vmcnt(0).
//   * loop: tile kt + 1 is staged into the other buffer while tile kt is multiplied; one vmcnt(0) + one barrier per K tile; the schedule
//     inside a K tile is the compiler's.
// Roofline: MFMA fp6 dense; 2*M*N*K flop per launch.
#pragma once
#include "gemm_w4.hpp"
#include "mx6.hpp"

namespace gemm_f6 {
using namespace gemm_core;

typedef __attribute__((ext_vector_type(8))) int i32x8;

constexpr int F6_BK = 128;                    // values of K per tile
constexpr int F6_ROWB = 96;                   // bytes of one row of one K tile
constexpr int F6_NTHR = 256;
constexpr int F6_OPER = 256 * F6_ROWB;        // 24 KiB: one operand of one K tile
constexpr int F6_BUF = 2 * F6_OPER;           // A | W
constexpr int F6_LDS = 2 * F6_BUF;            // 96 KiB

struct F6Args {
    const unsigned char* A; int64_t lda; const unsigned char* ea; int64_t ldea;      // packed rows [M, 3 K / 4] (lda bytes), scale bytes [M, K / 32]
    const unsigned char* W; int64_t ldw; const unsigned char* ew; int64_t ldew;      // the same for the weights [N, ..]
    unsigned char* eo; int64_t ldeo;                                                // MX6_GELU: the scale bytes [M, N / 32] beside the packed output
};

constexpr int EPI_MX6_GELU = YUME_EPI_MX6_GELU;

// the six pieces of one K tile of this thread and operand: piece P = 64 (4 j + wave) + lane < 1536. ga[j] / gw[j] point at the 16 source
// bytes of K tile 0; koff = 96 * kt.
//   A: bytes [row * lda + koff + 16 c, + 16) with row = min(m0 + P / 6, M - 1) <= M - 1, c = P % 6 <= 5, koff + 96 <= 3 K / 4 <= lda: inside row `row`.
//   W: the same with N, ldw.
//   LDS: bytes [1024 (4 j + wave) + 16 lane, + 16) of the operand image, 4 j + wave <= 23: inside its 24 KiB.
__device__ __forceinline__ void f6_stage(const unsigned char* const (&ga)[6], const unsigned char* const (&gw)[6], int koff, char* buf, int wave) {
#pragma unroll
    for (int j = 0; j < 6; ++j)
        __builtin_amdgcn_global_load_lds((gbl_cvoid*)(ga[j] + koff), (lds_void*)(buf + (4 * j + wave) * 1024), 16, 0, 0);
#pragma unroll
    for (int j = 0; j < 6; ++j)
        __builtin_amdgcn_global_load_lds((gbl_cvoid*)(gw[j] + koff), (lds_void*)(buf + F6_OPER + (4 * j + wave) * 1024), 16, 0, 0);
}

// fragment of tile row `row` (< 256): bytes [96 row + 24 q, + 24), q = lane >> 4 <= 3: inside the row's 96 bytes, 8-byte aligned
__device__ __forceinline__ i32x8 f6_frag(const char* oper, int row, int lane) {
    const char* rp = oper + row * F6_ROWB + 24 * (lane >> 4);
    const u32x2 a = *reinterpret_cast<const u32x2*>(rp), b = *reinterpret_cast<const u32x2*>(rp + 8), c = *reinterpret_cast<const u32x2*>(rp + 16);
    return i32x8{(int)a[0], (int)a[1], (int)b[0], (int)b[1], (int)c[0], (int)c[1], 0, 0};
}

// the scale bytes of the lane's eight rows row0 + 16 i + (lane & 15), clamped to rows - 1, for the four K tiles 4 g .. 4 g + 3: one 16-byte
// load per row (bytes [16 g, 16 g + 16) of the row's scales: 16 g + 16 <= round_up(K / 32, 16) <= ld, the row clamped — inside the array;
// bytes beyond K / 32 are read, not used). The addresses are formed here, once per four K tiles: sixteen row pointers kept across the loop
// were 32 registers beside the 256 accumulators, and the register allocator spilled.
// Packed per row into one dword: byte t = the scale of block 4 t + q of the group = the lane's own k-block of K tile 4 g + t.
__device__ __forceinline__ void f6_scales_load(const unsigned char* e, int64_t ld, int row0, int rows, int lane, int g, u32x4 (&raw)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) raw[i] = *reinterpret_cast<const u32x4*>(e + (int64_t)min(row0 + 16 * i + (lane & 15), rows - 1) * ld + 16 * g);
}
__device__ __forceinline__ void f6_scales_pack(const u32x4 (&raw)[8], int lane, unsigned (&pk)[8]) {
    const int sh = 8 * (lane >> 4);
#pragma unroll
    for (int i = 0; i < 8; ++i)
        pk[i] = ((raw[i][0] >> sh) & 0xffu) | (((raw[i][1] >> sh) & 0xffu) << 8) | (((raw[i][2] >> sh) & 0xffu) << 16) | ((raw[i][3] >> sh) << 24 & 0xff000000u);
}

// F32 / RESID: gemm_core.hpp's guarded store_row4. The lane's rows m0 + wr*128 + 16 i + l15 and column quads n0 + wc*128 + 16 j + 4 l4
// (+ 0..3); N % 4 == 0: a quad is inside N or outside as a whole, the bias is read for quads inside N only. (column quad j's bias is loaded
// inside the j loop, as in gemm_f8.hpp: hoisted in front of it the vectors were live beside the 256 accumulators)
template <int EPI>
__device__ __forceinline__ void f6_epilogue(const f32x4 (&acc)[8][8], const Problem& p, const Epilogue& e, int m0, int n0) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    Epilogue e0 = e;
    e0.bias = nullptr;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int n = n0 + wc * 128 + 16 * j + 4 * l4;
        const f32x4 b = (e.bias && n < p.N) ? *reinterpret_cast<const f32x4*>(e.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int m = m0 + wr * 128 + 16 * i + l15;
            if (m < p.M && n < p.N) store_row4<EPI>(acc[i][j] + b, m, n, p, e0);      // out[m, n .. n + 3], n + 3 < N
        }
    }
}

// YUME_EPI_MX6_GELU: v = gelu_tanh(acc + bias[n]) in fp32 leaves as packed e2m3 with one E8M0 byte per row and 32 consecutive columns: no
// bf16 `ff`, no quantiser pass behind it. A block is fragments j = 2 jj and 2 jj + 1 of the wave's columns over the four lanes l15 + 16 {0..3}
// that hold one row: the amax is a lane-local max of 8 and two xor-shuffles (16, 32). A lane's quad of fragment h is chunk 4 h + l4 of the
// block (mx6.hpp); dword d of the block's 24 bytes joins chunks f = d + d / 3 and f + 1, fetched from lanes l15 + 16 (f & 3): lane l4 stores
// dword l4, lanes l4 < 2 also dword 4 + l4. N % 128 == 0: a block lies inside N or outside as a whole; rows >= M and blocks >= N are not
// written (neither bytes nor scale). The shuffles run in every lane, the stores are guarded.
__device__ __forceinline__ void f6_epilogue_mx_gelu(const f32x4 (&acc)[8][8], const Problem& p, const F6Args& f, const Epilogue& e, int m0, int n0) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    unsigned char* const qo = reinterpret_cast<unsigned char*>(e.out);
    const int d0 = l4, d1 = 4 + (l4 & 1);                          // the lane's dwords (d1 stored by l4 < 2 only)
    const int f0 = mx6::first_chunk(d0), f1 = mx6::first_chunk(d1);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int nb = n0 + wc * 128 + 32 * jj;                     // first column of the block; the lane's quads: nb + 4 l4, nb + 16 + 4 l4
        const bool in_n = nb < p.N;                                 // (wave-uniform) then nb + 31 < N
        f32x4 b[2];
#pragma unroll
        for (int h = 0; h < 2; ++h)
            b[h] = (e.bias && in_n) ? *reinterpret_cast<const f32x4*>(e.bias + nb + 16 * h + 4 * l4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int m = m0 + wr * 128 + 16 * i + l15;
            f32x4 v[2];
            float am = 0.f;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                v[h] = gemm_w4::w4_act<YUME_EPI_BF16_GELU>(acc[i][2 * jj + h] + b[h]);
#pragma unroll
                for (int c = 0; c < 4; ++c) am = fmaxf(am, fabsf(v[h][c]));
            }
            am = fmaxf(am, __shfl_xor(am, 16, 64));
            am = fmaxf(am, __shfl_xor(am, 32, 64));
            const int byte = mx6::block_byte(am);
            const float mult = mx6::block_mult(byte);
            const unsigned c0 = mx6::chunk4(v[0][0], v[0][1], v[0][2], v[0][3], mult), c1 = mx6::chunk4(v[1][0], v[1][1], v[1][2], v[1][3], mult);
            auto chunk = [&](int fc) {                               // chunk fc (0..7) of this row's block: quad fc >> 2 of lane l15 + 16 (fc & 3)
                const int src = l15 + 16 * (fc & 3);
                const unsigned x0 = (unsigned)__shfl((int)c0, src, 64), x1 = (unsigned)__shfl((int)c1, src, 64);
                return (fc >> 2) ? x1 : x0;
            };
            const unsigned w0 = mx6::join_chunks(chunk(f0), chunk(f0 + 1), d0);
            const unsigned w1 = mx6::join_chunks(chunk(f1), chunk(f1 + 1), d1);
            if (m < p.M && in_n) {
                // bytes [m * ldo + 24 (nb / 32) + 4 d, + 4), d <= 5: 24 (nb / 32) + 24 <= 3 N / 4 <= ldo, m < M; ldo % 16 == 0: dword-aligned
                unsigned char* const blk = qo + (int64_t)m * e.ldo + 24 * (nb >> 5);
                *reinterpret_cast<unsigned*>(blk + 4 * d0) = w0;
                if (l4 < 2) *reinterpret_cast<unsigned*>(blk + 4 * d1) = w1;
                // byte [m * ldeo + nb / 32]: nb / 32 < N / 32 <= ldeo
                if (l4 == 3) f.eo[(int64_t)m * f.ldeo + (nb >> 5)] = (unsigned char)byte;
            }
        }
    }
}

template <int EPI>
__global__ __launch_bounds__(F6_NTHR, 1) void gemm_f6_mx_kernel(Problem p, F6Args f, Epilogue e) {
    __shared__ __attribute__((aligned(16))) char smem[F6_LDS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    int start, count, m0, n0;
    xcd_chunk(p.tiles_m * p.tiles_n, blockIdx.x & 7, start, count);
    tile_origin(p, start + (blockIdx.x >> 3), m0, n0);             // m0 < M, n0 < N: the grid is exactly tiles_m * tiles_n

    const unsigned char* ga[6];
    const unsigned char* gw[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int P = 64 * (4 * j + wave) + lane;                   // < 1536
        const int r = P / 6, c = P - 6 * r;                         // tile row 0..255, piece 0..5
        ga[j] = f.A + (int64_t)min(m0 + r, p.M - 1) * f.lda + 16 * c;
        gw[j] = f.W + (int64_t)min(n0 + r, p.N - 1) * f.ldw + 16 * c;
    }
    const int ra0 = m0 + wr * 128, rw0 = n0 + wc * 128;            // the wave's first row of each operand's scales
    f32x4 acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = p.K / F6_BK;
    u32x4 raw[8];
    unsigned pka[8], pkan[8], pkw[8], pkwn[8];
    f6_scales_load(f.ea, f.ldea, ra0, p.M, lane, 0, raw);
    f6_scales_pack(raw, lane, pka);
    f6_scales_load(f.ew, f.ldew, rw0, p.N, lane, 0, raw);
    f6_scales_pack(raw, lane, pkw);
    f6_stage(ga, gw, 0, smem, wave);
#pragma unroll
    for (int i = 0; i < 8; ++i) { pkan[i] = pka[i]; pkwn[i] = pkw[i]; }
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's pieces of tile kt have landed (and any scale load before them)
        __syncthreads();                                            // ... every wave's have, and every wave is done reading the other buffer
        // group g + 1 = K tiles kt + 3 .. (t == 1) / kt + 2 .. (t == 2): A's bytes are loaded in t == 1 and packed in t == 2, W's loaded in
        // t == 2 and packed in t == 3, through ONE raw array; each load is issued before this iteration's stage and consumed behind the next
        // iteration's vmcnt(0). Past the last group nothing is loaded and the packs take stale bytes no K tile uses.
        const int t = kt & 3;
        if (t == 2) f6_scales_pack(raw, lane, pkan);
        if (t == 3) f6_scales_pack(raw, lane, pkwn);
        if (t == 1 && kt + 3 < nk) f6_scales_load(f.ea, f.ldea, ra0, p.M, lane, (kt >> 2) + 1, raw);
        if (t == 2 && kt + 2 < nk) f6_scales_load(f.ew, f.ldew, rw0, p.N, lane, (kt >> 2) + 1, raw);
        if (kt + 1 < nk) f6_stage(ga, gw, (kt + 1) * F6_ROWB, smem + (cur ^ 1) * F6_BUF, wave);
        const char* At = smem + cur * F6_BUF;
        const char* Wt = At + F6_OPER;
        i32x8 a[8];
        int sca[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            a[i] = f6_frag(At, wr * 128 + 16 * i + (lane & 15), lane);
            sca[i] = (int)(pka[i] >> (8 * t));
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const i32x8 w = f6_frag(Wt, wc * 128 + 16 * j + (lane & 15), lane);
            const int scw = (int)(pkw[j] >> (8 * t));
#pragma unroll
            for (int i = 0; i < 8; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, a[i], acc[i][j], 2, 2, 0, scw, 0, sca[i]);
        }
        if (t == 3) {
#pragma unroll
            for (int i = 0; i < 8; ++i) { pka[i] = pkan[i]; pkw[i] = pkwn[i]; }
        }
        cur ^= 1;
    }
    if constexpr (EPI == EPI_MX6_GELU) f6_epilogue_mx_gelu(acc, p, f, e, m0, n0);
    else f6_epilogue<EPI>(acc, p, e, m0, n0);
}

inline int launch_f6(int epi, Problem p, const F6Args& f, const Epilogue& e, hipStream_t st) {
    p.tiles_m = (p.M + 255) / 256;
    p.tiles_n = (p.N + 255) / 256;
    p.group_m = g_group_m;
    const dim3 grid((unsigned)(p.tiles_m * p.tiles_n)), block(F6_NTHR);
    if (epi == YUME_EPI_RESID) hipLaunchKernelGGL(gemm_f6_mx_kernel<YUME_EPI_RESID>, grid, block, 0, st, p, f, e);
    else if (epi == EPI_MX6_GELU) hipLaunchKernelGGL(gemm_f6_mx_kernel<EPI_MX6_GELU>, grid, block, 0, st, p, f, e);
    else hipLaunchKernelGGL(gemm_f6_mx_kernel<YUME_EPI_F32>, grid, block, 0, st, p, f, e);
    YUME_CHECK_LAUNCH("gemm_f6");
    return YUME_OK;
}

}  // namespace gemm_f6
