// gemm_f8.hpp — the e4m3 x e4m3 GEMM of the fp8 FFN option (r15):   acc[m,n] = sum_k Aq[m,k] * Wq[n,k]  (fp32),
//   y = acc * sa[m] * sw[n] + bias[n],  then the epilogue (BF16 / GELU tanh / F32 / RESID, as gemm_core.hpp defines them; r18: SPLITT,
//   q | k row-major and V as the K-major V^T image, through yume_gemm_f8_splitt — f8_epilogue_vt below).
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
//     (r16: the pattern rows see only the k order of one operand AGAINST the other. The scale probe, tools/ubench/mfma_f8_scale_map.hip, shows
//     the instruction's own k order is registers 0-3 = k 16 q .. + 15, registers 4-7 = k 64 + 16 q .. + 15 with q = l >> 4; this kernel's chunks
//     2 q, 2 q + 1 are a k-permutation applied to both operands alike — the same sums under unit scales. gemm_f8_mx_kernel below, whose
//     scale bytes cover 32 consecutive k of the instruction's order, loads chunks q and 4 + q.)
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
    // (r16) MX forms: ea = E8M0 scale bytes [M, K / 32] of A (row stride ldea) in place of sa (gemm_f8_mx_kernel); eo = the scale bytes
    // [M, N / 32] (row stride ldeo) the MX_GELU epilogue writes beside its e4m3 output
    const unsigned char* ea; int64_t ldea;
    unsigned char* eo; int64_t ldeo;
};

constexpr int EPI_MX_GELU = YUME_EPI_MX_GELU;

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

// ---- (r18) the transposed side of YUME_EPI_BF16_SPLITT: columns n >= n_split leave as the K-major V^T image outT[n - n_split][m].
// The accumulators keep the SWAP orientation (a lane holds C[m][n .. n + 3]), so the tile's bf16 image is written TRANSPOSED into the LDS
// the operand buffers free — image rows = features n, image columns = tokens m, gemm_w4.hpp's layout ([256][512 B], 16-byte chunk c of row
// r at chunk c ^ (r & 31)) — and leaves through w4_store_image with rows and columns exchanged, as w4_epilogue<SPLITT, !SWAP> does.
// A lane's four values belong to four image rows at one 2-byte column. Lanes l15 and l15 ^ 1 (tokens m, m + 1) exchange one packed pair
// (DPP quad_perm [1, 0, 3, 2]): the even lane then holds (m, m + 1) of columns n, n + 1, the odd lane of columns n + 2, n + 3 — two dword
// writes per lane and tile in place of four 2-byte ones. Banks (ds_write_b32: dword address % 32, conflicts inside a 32-lane half = both values of l4 & 1, all l15): a
// lane's dword is ((l15 >> 1) & 3) of chunk (16 wr + 2 i + (l15 >> 3)) ^ (r & 31) with r & 7 = 4 (l4 & 1) + 2 (l15 & 1) + s: chunk bit 0 =
// l15 >> 3, bit 1 = l15 & 1, bit 2 = l4 & 1 (XORed with constants of the tile) — 32 lanes, 32 different banks, no conflict.
//   image byte of (tile i, j, s = 0 / 1, lane) = r * 512 + ((chunk ^ (r & 31)) << 4) + 4 ((l15 >> 1) & 3),  r = 128 wc + 16 j + 4 l4 + 2 (l15 & 1) + s
//     = vbase + (16 j + s) * 512 + ((wr ^ (j & 1)) << 8) + (lx ^ ((2 i | s) << 4)):  r < 256, chunk < 32 — inside the 128 KiB image.
// Rows m >= M (computed from the clamped row M - 1) and columns n >= N sit in the image and are not stored: w4_store_image takes
// rows_valid = min(256, N - n0) and cols_valid = min(256, M - m0), its last partial chunk element by element.
template <class Col>
__device__ __forceinline__ void f8_epilogue_vt(const f32x4 (&acc)[8][8], const float (&sa)[8], Col col, const Problem& p, const Epilogue& e, int m0,
                                               int n0, char* smem) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    const bool odd = (l15 & 1) != 0;
    const int x0 = 4 * l4 + 2 * (l15 & 1);
    const unsigned vbase = (unsigned)((wc * 128 + x0) * 512 + ((l15 >> 1) & 3) * 4);
    const unsigned lx = (unsigned)((x0 | (l15 >> 3)) << 4);
    __syncthreads();                                                // every wave is done with the operand buffers: the image reuses them
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        f32x4 sw, b;
        col(j, sw, b);
        const unsigned jb = vbase + (unsigned)(16 * j * 512) + (unsigned)((wr ^ (j & 1)) << 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f32x4 v = (acc[i][j] * sa[i]) * sw + b;
            const unsigned p01 = pack_bf16x2(v[0], v[1]), p23 = pack_bf16x2(v[2], v[3]);
            const unsigned got = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(odd ? p01 : p23), 0xB1, 0xf, 0xf, false);   // from lane ^ 1
            const unsigned keep = odd ? p23 : p01;
            const unsigned lo = odd ? got : keep, hi = odd ? keep : got;        // token m (even) / m + 1 of this lane's two columns
            *reinterpret_cast<unsigned*>(smem + jb + (lx ^ (unsigned)((2 * i) << 4))) = (lo & 0xffffu) | (hi << 16);
            *reinterpret_cast<unsigned*>(smem + jb + 512u + (lx ^ (unsigned)((2 * i + 1) << 4))) = (lo >> 16) | (hi & 0xffff0000u);
        }
    }
    __syncthreads();
    // V^T rows n0 - n_split .. + min(256, N - n0) - 1 (< N - n_split), columns m0 .. m0 + min(256, M - m0) - 1 (< M <= ldt)
    gemm_w4::w4_store_image(smem, e.outT + (int64_t)(n0 - e.n_split) * e.ldt, e.ldt, 0, min(256, p.N - n0), m0, min(256, p.M - m0));
}

// MX (gemm_f8_mx_kernel): the row scales were applied inside the instruction, there is no sa (the factor is the literal 1)
template <int EPI, bool MX = false>
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
    for (int i = 0; i < 8; ++i) sa[i] = MX ? 1.0f : f.sa[min(m0 + wr * 128 + 16 * i + l15, p.M - 1)];
    auto col = [&](int j, f32x4& sw, f32x4& b) {
        const int n = n0 + wc * 128 + 16 * j + 4 * l4;
        sw = n < p.N ? *reinterpret_cast<const f32x4*>(f.sw + n) : f32x4{1.f, 1.f, 1.f, 1.f};
        b = (e.bias && n < p.N) ? *reinterpret_cast<const f32x4*>(e.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    if constexpr (EPI == YUME_EPI_BF16_SPLITT) {
        if (n0 >= e.n_split) {                                      // (workgroup-uniform) n_split % 256 == 0: a tile lies wholly on one side
            f8_epilogue_vt(acc, sa, col, p, e, m0, n0, smem);
            return;
        }
    }
    // a SPLITT tile on the row-major side is a BF16 tile: n0 + 256 <= n_split <= N, nothing of it reaches a column >= n_split
    constexpr int EPI_RM = EPI == YUME_EPI_BF16_SPLITT ? YUME_EPI_BF16 : EPI;
    constexpr bool BF16_OUT = EPI_RM == YUME_EPI_BF16 || EPI_RM == YUME_EPI_BF16_GELU;
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
            if (m < p.M && n < p.N) store_row4<EPI_RM>((acc[i][j] * sa[i]) * sw + b, m, n, p, e0);      // out[m, n .. n + 3], n + 3 < N
        }
    }
}

// ---- (r16) the producer's epilogue, YUME_EPI_MX_GELU: v = gelu_tanh(acc sa[m] sw[n] + bias[n]) in fp32 leaves as e4m3 bytes with one E8M0
// scale byte per row and 32 consecutive columns (OCP MX): no bf16 `ff`, no quantiser pass behind it.
//   amax over the block -> e = the smallest integer with amax <= 448 * 2^e, read off the fp32 bits: 448 = 1.75 * 2^8, so with amax =
//   1.f * 2^(E - 127) it is E - 127 - 8 where the significand is <= 1.75 (fraction bits <= 0x600000), else E - 127 - 7. The byte e + 127 =
//   E - 8 (+ 1) is clamped below at 0 (E < 8: amax < 2^-119, e = -127; fp32 has no E > 254, so the byte never exceeds 247); an all-zero
//   block takes e = 0 (byte 127). q = e4m3_rne(clamp(v * 2^-e, +-448)); 2^-e = the fp32 with exponent field 254 - byte in [7, 254]: normal,
//   the product exact.
// A block is fragments j = 2 jj and 2 jj + 1 of the wave's columns (16 columns each, a lane holds 4 of each) over the four lanes
// l15 + 16 {0..3} that hold one row: the amax is a lane-local max of 8 and two xor-shuffles (16, 32) — no LDS, nothing between workgroups.
// N % 32 == 0: a block lies inside N or outside as a whole; rows >= M and blocks >= N are not written (neither bytes nor scale).
__device__ __forceinline__ void f8_epilogue_mx_gelu(const f32x4 (&acc)[8][8], const Problem& p, const F8Args& f, const Epilogue& e, int m0, int n0) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    float sa[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) sa[i] = f.sa[min(m0 + wr * 128 + 16 * i + l15, p.M - 1)];
    unsigned char* const qo = reinterpret_cast<unsigned char*>(e.out);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int nb = n0 + wc * 128 + 32 * jj;                     // first column of the block; the lane's quads: nb + 4 l4, nb + 16 + 4 l4
        const bool in_n = nb < p.N;                                 // (wave-uniform) then nb + 31 < N
        f32x4 sw[2], b[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = nb + 16 * h + 4 * l4;
            sw[h] = in_n ? *reinterpret_cast<const f32x4*>(f.sw + n) : f32x4{1.f, 1.f, 1.f, 1.f};
            b[h] = (e.bias && in_n) ? *reinterpret_cast<const f32x4*>(e.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int m = m0 + wr * 128 + 16 * i + l15;
            f32x4 v[2];
            float am = 0.f;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                v[h] = gemm_w4::w4_act<YUME_EPI_BF16_GELU>((acc[i][2 * jj + h] * sa[i]) * sw[h] + b[h]);
#pragma unroll
                for (int c = 0; c < 4; ++c) am = fmaxf(am, fabsf(v[h][c]));
            }
            am = fmaxf(am, __shfl_xor(am, 16, 64));
            am = fmaxf(am, __shfl_xor(am, 32, 64));
            const unsigned bits = __float_as_uint(am);
            const int E = (int)(bits >> 23);                         // am >= 0: no sign bit
            int byte = E - 8 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
            byte = am > 0.f ? max(byte, 0) : 127;
            const float mult = __uint_as_float((unsigned)(254 - byte) << 23);
            if (m < p.M && in_n) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    float t[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) t[c] = fminf(fmaxf(v[h][c] * mult, -448.0f), 448.0f);
                    int w = __builtin_amdgcn_cvt_pk_fp8_f32(t[0], t[1], 0, false);
                    w = __builtin_amdgcn_cvt_pk_fp8_f32(t[2], t[3], w, true);
                    // bytes [m * ldo + nb + 16 h + 4 l4, + 4): m < M, nb + 16 h + 4 l4 + 3 <= nb + 31 < N <= ldo
                    *reinterpret_cast<int*>(qo + (int64_t)m * e.ldo + nb + 16 * h + 4 * l4) = w;
                }
                // byte [m * ldeo + nb / 32]: nb / 32 < N / 32 <= ldeo
                if (l4 == 0) f.eo[(int64_t)m * f.ldeo + (nb >> 5)] = (unsigned char)byte;
            }
        }
    }
}

// fragment of the MX consumer: the instruction's k order (tools/ubench/mfma_f8_scale_map.hip, profiles/r16_fp8_ffn_fused.md) puts lane group
// q's registers 0-3 at k = 16 q .. + 15 and its registers 4-7 at k = 64 + 16 q .. + 15, and a scale byte covers 32 consecutive k of THAT order.
// So the lane takes logical chunks q and 4 + q of the 128-byte row (positions q ^ (row & 7) and that ^ 4): block b of the instruction is
// bytes 32 b .. 32 b + 31 of memory. (gemm_f8_kernel's chunks 2 q, 2 q + 1 are a k-permutation applied to both operands alike — the same sums
// under unit scales, the wrong blocks under these.)
__device__ __forceinline__ i32x8 f8_frag_mx(const char* oper, int row, int lane) {
    const int q = lane >> 4;
    const char* rp = oper + row * F8_BK;
    const u32x4 lo = *reinterpret_cast<const u32x4*>(rp + (((q ^ row) & 7) << 4));
    const u32x4 hi = *reinterpret_cast<const u32x4*>(rp + ((((4 + q) ^ row) & 7) << 4));
    return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// the scale bytes of this lane's eight rows for the four K tiles 4 g .. 4 g + 3: one 16-byte load per row (bytes [16 g, 16 g + 16) of the
// row's scales: 16 g + 16 <= round_up(K / 32, 16) <= ldea, the row clamped to M - 1 — inside ea; bytes beyond K / 32 are read, not used).
// Packed per row into one dword: byte t = the scale of block 4 t + q of the group = the lane's own k-block of K tile 4 g + t.
__device__ __forceinline__ void f8_mx_scales_load(const unsigned char* const (&ge)[8], int g, u32x4 (&raw)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) raw[i] = *reinterpret_cast<const u32x4*>(ge[i] + 16 * g);
}
__device__ __forceinline__ void f8_mx_scales_pack(const u32x4 (&raw)[8], int lane, unsigned (&pk)[8]) {
    const int sh = 8 * (lane >> 4);
#pragma unroll
    for (int i = 0; i < 8; ++i)
        pk[i] = ((raw[i][0] >> sh) & 0xffu) | (((raw[i][1] >> sh) & 0xffu) << 8) | (((raw[i][2] >> sh) & 0xffu) << 16) | ((raw[i][3] >> sh) << 24 & 0xff000000u);
}

// gemm_f8_kernel with the activations' block scales in the instruction: acc[m, n] = sum_b 2^(ea[m, b] - 127) sum_{k in block b} Aq[m, k] Wq[n, k].
// Same tile, staging and loop. The scale bytes travel OUTSIDE the LDS-DMA stream, as plain global loads into registers, one group of four
// K tiles at a time: the loads of group g + 1 are issued in K tile 4 g + 2, right after the barrier and BEFORE that iteration's stage, so they
// are older than every glds in flight; they are consumed (packed) in K tile 4 g + 3 after the top-of-loop vmcnt(0) that the glds of that
// tile needed anyway — no wait of their own ever falls between a stage and its vmcnt(0). The scale operand uses selector 0 on the byte
// shifted down for the K tile (the three bytes above it are ignored by the instruction).
template <int EPI>
__global__ __launch_bounds__(F8_NTHR, 1) void gemm_f8_mx_kernel(Problem p, F8Args f, Epilogue e) {
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
    const unsigned char* ge[8];
    {
        const int rl = 8 * wave + (lane >> 3);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = 32 * j + rl;                              // tile row 0..255; r & 7 = lane >> 3 & 7
            const int ch = ((lane & 7) ^ (r & 7)) << 4;             // source byte offset inside the 128-byte K slice: 0..112
            ga[j] = f.A + (int64_t)min(m0 + r, p.M - 1) * f.lda + ch;
            gw[j] = f.W + (int64_t)min(n0 + r, p.N - 1) * f.ldw + ch;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) ge[i] = f.ea + (int64_t)min(m0 + wr * 128 + 16 * i + (lane & 15), p.M - 1) * f.ldea;
    }
    f32x4 acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = p.K / F8_BK;
    u32x4 raw[8];
    unsigned pk[8], pkn[8];
    f8_mx_scales_load(ge, 0, raw);
    f8_stage(ga, gw, 0, smem, wave);
    f8_mx_scales_pack(raw, lane, pk);
#pragma unroll
    for (int i = 0; i < 8; ++i) pkn[i] = pk[i];
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's pieces of tile kt have landed (and any scale load before them)
        __syncthreads();                                            // ... every wave's have, and every wave is done reading the other buffer
        const int t = kt & 3;
        if (t == 3) f8_mx_scales_pack(raw, lane, pkn);              // group kt / 4 + 1, loaded one K tile ago (unused garbage past the last group)
        if (t == 2 && kt + 2 < nk) f8_mx_scales_load(ge, (kt >> 2) + 1, raw);
        if (kt + 1 < nk) f8_stage(ga, gw, (kt + 1) * F8_BK, smem + (cur ^ 1) * F8_BUF, wave);
        const char* At = smem + cur * F8_BUF;
        const char* Wt = At + F8_OPER;
        i32x8 a[8];
        int sc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            a[i] = f8_frag_mx(At, wr * 128 + 16 * i + (lane & 15), lane);
            sc[i] = (int)(pk[i] >> (8 * t));
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const i32x8 w = f8_frag_mx(Wt, wc * 128 + 16 * j + (lane & 15), lane);
#pragma unroll
            for (int i = 0; i < 8; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, a[i], acc[i][j], 0, 0, 0, 0x7f7f7f7f, 0, sc[i]);
        }
        if (t == 3) {
#pragma unroll
            for (int i = 0; i < 8; ++i) pk[i] = pkn[i];
        }
        cur ^= 1;
    }
    f8_epilogue<EPI, true>(acc, p, f, e, m0, n0, smem);
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
    if constexpr (EPI == EPI_MX_GELU) f8_epilogue_mx_gelu(acc, p, f, e, m0, n0);
    else f8_epilogue<EPI>(acc, p, f, e, m0, n0, smem);
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
        case EPI_MX_GELU: hipLaunchKernelGGL(gemm_f8_kernel<EPI_MX_GELU>, grid, block, 0, st, p, f, e); break;
        case YUME_EPI_BF16_SPLITT: hipLaunchKernelGGL(gemm_f8_kernel<YUME_EPI_BF16_SPLITT>, grid, block, 0, st, p, f, e); break;
        default: hipLaunchKernelGGL(gemm_f8_kernel<YUME_EPI_BF16>, grid, block, 0, st, p, f, e); break;
    }
    YUME_CHECK_LAUNCH("gemm_f8");
    return YUME_OK;
}

inline int launch_f8_mx(int epi, Problem p, const F8Args& f, const Epilogue& e, hipStream_t st) {
    p.tiles_m = (p.M + 255) / 256;
    p.tiles_n = (p.N + 255) / 256;
    p.group_m = g_group_m;
    const dim3 grid((unsigned)(p.tiles_m * p.tiles_n)), block(F8_NTHR);
    if (epi == YUME_EPI_RESID) hipLaunchKernelGGL(gemm_f8_mx_kernel<YUME_EPI_RESID>, grid, block, 0, st, p, f, e);
    else hipLaunchKernelGGL(gemm_f8_mx_kernel<YUME_EPI_F32>, grid, block, 0, st, p, f, e);
    YUME_CHECK_LAUNCH("gemm_f8_mx");
    return YUME_OK;
}

}  // namespace gemm_f8
