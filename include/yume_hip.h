/*
 * yume_hip.h — C-ABI of libyume_hip.so: the MI355X (gfx950) kernels behind YUME's
 * denoise hot path (WanModel DiT block stack + causal 3D VAE).
 *
 * The reference has no FFI of its own for this path: it is Python calling torch ops and
 * one external native library (flash-attn).  Each entry point below therefore names the
 * reference Python call site(s) it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into memory owned by the caller (torch-allocated);
 *     the library never allocates or frees device memory. The only device memory it keeps a
 *     pointer to between calls is the ticket-counter workspace the caller registers with
 *     yume_counter_workspace_init (below); without one, every kernel runs a ticket-free schedule.
 *   - shapes are element counts, strides/leading dimensions are in ELEMENTS of the buffer type.
 *   - bf16 buffers are passed as `const void*` / `void*` (raw 16-bit brain floats).
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream). No entry point
 *     synchronises; all work is enqueued on `stream`.
 *   - return value: 0 on success, a negative YUME_E* code on failure; the message for the
 *     last failure on the calling thread is returned by yume_last_error(). Nothing throws
 *     across the ABI.
 *   - re-entrant across processes (one process per GPU); no internal threads, no global
 *     mutable device state.
 */
#ifndef YUME_HIP_H
#define YUME_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YUME_OK 0
#define YUME_EINVAL (-1)   /* bad argument (shape/alignment/NULL)          */
#define YUME_ELAUNCH (-2)  /* hipLaunchKernel / runtime error               */
#define YUME_EUNSUP (-3)   /* combination not implemented by this build     */

/* ---- library info ------------------------------------------------------------------- */
const char* yume_last_error(void);
/* ABI version of this header; bumped on any signature change (yume_amd/_lib.py refuses a library that reports another one). */
#define YUME_ABI_VERSION 9
int yume_abi_version(void);
/* name of the gfx target the kernels were compiled for ("gfx950"). */
const char* yume_target_arch(void);

/* ---- caller-owned ticket-counter workspace --------------------------------------------------
 * Kernels that hand out work by ticket (the tails of long convolutions; the persistent attention kernel) draw their counters from a
 * buffer the CALLER owns: yume_counter_workspace_bytes() bytes, 64-byte aligned, registered once per device with
 * yume_counter_workspace_init(ptr, bytes, stream) — the call zeroes it on `stream` — and valid until it is replaced or unregistered
 * (ptr = NULL). Invariant: the buffer holds zeros whenever no launch is using it (the last workgroup of a launch to touch its 64-byte
 * counter set writes the zeros back), so launches need no memset and can be captured into a hipGraph (the set a launch uses is chosen when
 * the launch is enqueued — at capture time for a graph: two replays of ONE captured graph must not run concurrently, as for any graph whose
 * kernels share scratch). Otherwise a set is shared by two launches only if 256 ticketed launches of one device are in flight at once. Without a registered buffer the ticketed kernels keep their static
 * schedules (same results). The registration is per process and per device (the calling thread's current device). */
int64_t yume_counter_workspace_bytes(void);
int yume_counter_workspace_init(void* ptr, int64_t bytes, void* stream);

/* ---- per-box calibration (r5; no reference counterpart — measurement plumbing of bench.py) ----------------
 * Launches `workgroups` x 256 threads (one wave per SIMD), each wave issuing iters * 16 v_mfma_f32_32x32x16_bf16 (32768 flop each, 32
 * matrix-pipe clocks each) on random operands (constant ones draw little power and run at 2.3 GHz) and nothing else. The caller times the launch with events on `stream`: workgroups * 4 * iters * 16 * 32768
 * flop / time = the dense bf16 rate THIS chip sustains under a pure matrix load (nominal 2.5 PFLOP/s assumes 2.4 GHz; the package power
 * limit holds a loaded MI355X near 1.7-1.8 GHz, and by how much differs from box to box). ticks (optional): uint64 [workgroups][2] =
 * {s_memtime delta, s_memrealtime delta (100 MHz)} of each workgroup's first wave; sink: 4 bytes of device memory (never written). */
int yume_calibrate_mfma(int64_t iters, int64_t workgroups, void* ticks, void* sink, void* stream);

/* ---- fused LayerNorm + modulate  ---------------------------------------------------------
 * replaces: wan23/modules/model.py:300-301,309-310 (norm1/norm2 + `*(1+scale)+shift`),
 *           wan23/modules/model.py:140-150 (WanLayerNorm), :308 (norm3, affine),
 *           wan23/modules/model.py:344-347 (Head norm+modulate);  same lines in wan/modules/model.py.
 *
 *   y[t, :] = LN(x[t, :]; eps, no affine) * (mul[row(t), :] + add_one) + add[row(t), :]
 *   row(t) = row_idx ? row_idx[t] : 0
 * x: fp32 [T, C] (row stride ldx).  mul/add: fp32 tables, row stride `tab_stride` elements
 * (for the DiT `mul`=scale chunk, `add`=shift chunk of the [R,6,C] modulation table with
 * add_one=1; for the affine norm3 `mul`=weight, `add`=bias with add_one=0).
 * out_kind: 0 = bf16 [T, C] (ldo), 1 = fp32 [T, C] (ldo),
 *           2 = bf16 3-way split [T, 3C]: [hi | hi | lo] where hi=bf16(y), lo=bf16(y-hi)
 *               (feeds the fp32-accurate head GEMM, see yume_gemm_bf16).
 * C must be a multiple of 8 and <= 8192.
 */
int yume_adaln_modulate(const float* x, int64_t ldx, int64_t T, int64_t C, float eps,
                        const float* mul, const float* add, int64_t tab_stride,
                        const int32_t* row_idx, int add_one,
                        void* out, int64_t ldo, int out_kind, void* stream);

/* ---- bf16 MFMA GEMM with fused epilogues ------------------------------------------------
 * replaces: every nn.Linear on the path — wan23/modules/model.py:171-174,189-195,205-206
 *           (q,k,v,o), :222-231 (cross q,k,v,o), :265-267,309-312 (ffn + gate/residual),
 *           :303-304 (gate + residual), :455-457,815-821 (text_embedding),
 *           :453-454,602-720 (patch embeddings as GEMM over gathered patches), :331,346 (head).
 *
 *   acc[m, n] = sum_k A[m, k] * W[n, k]          (A bf16 [M,K] lda;  W bf16 [N,K] ldw = nn.Linear layout)
 * K must be a multiple of 64; M, N arbitrary (> 0).
 * epilogue `epi`:
 *   YUME_EPI_BF16      out bf16 [M,N] (ldo)      = acc + bias
 *   YUME_EPI_BF16_GELU out bf16 [M,N]            = gelu_tanh(acc + bias)
 *   YUME_EPI_BF16_GELU_ERF  same with the exact erf GELU (img_emb MLPProj, wan/modules/model.py:534-537)
 *   YUME_EPI_F32       out fp32 [M,N]            = acc + bias
 *   YUME_EPI_RESID     out fp32 [M,N] in/out     += (acc + bias) * (gate ? gate[row(m), n] : 1)
 *                      gate fp32 table, row stride gate_stride, row(m) = row_idx ? row_idx[m] : 0
 *   YUME_EPI_BF16_SPLITT  columns n < n_split as YUME_EPI_BF16 into `out`;
 *                      columns n >= n_split written TRANSPOSED as bf16 into outT[(n - n_split), m]
 *                      (row stride ldt >= M) — the K-major V^T image the attention kernel consumes.
 *                      n_split must be a multiple of 128.
 * bias: fp32 [N] or NULL.
 * variant: 0 = automatic — a 256x256-tile kernel once its tiles fill the chip (r3: the one-wave-per-SIMD kernel of csrc/gemm_w4.hpp
 *   where it applies: K >= 192, the six epilogues above; env YUME_GEMM_W4=0 keeps the 8-wave kernel), else the 128x128-tile kernel;
 *   when the 256x256 tiling would leave a last round of tiles at most ~1/3 full, whole rounds of M-tiles go to the 256x256 kernel
 *   and the remaining rows to the 128x128 kernel (two launches inside this call). 1 = 128x128 kernel, 2 = the 8-wave 256x256
 *   kernel, 3 = the one-wave-per-SIMD 256x256 kernel (as 2 where it does not apply). All variants compute the same products in
 *   fp32; they differ in summation order only.
 */
enum {
    YUME_EPI_BF16 = 0,
    YUME_EPI_BF16_GELU = 1,
    YUME_EPI_F32 = 2,
    YUME_EPI_RESID = 3,
    YUME_EPI_BF16_SPLITT = 4,
    YUME_EPI_BF16_GELU_ERF = 5,
    YUME_EPI_BF16_GEGLU = 6,     /* see the T5 section below */
    YUME_EPI_MX_GELU = 7,        /* yume_gemm_f8_mxout only: e4m3 bytes + one E8M0 scale byte per 32 columns (the FP8 FFN section) */
    YUME_EPI_MX6_GELU = 8        /* yume_gemm_f6_mxout only: packed e2m3 + one E8M0 scale byte per 32 columns (the MXFP6 FFN section) */
};
int yume_gemm_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                   int64_t M, int64_t N, int64_t K, int epi,
                   void* out, int64_t ldo,
                   const float* gate, int64_t gate_stride, const int32_t* row_idx,
                   void* outT, int64_t ldt, int64_t n_split,
                   int variant, void* stream);

/* Same call with caller-owned scratch for the STREAM-K TAIL of the one-wave-per-SIMD kernel (r6, ABI 8): a GEMM whose 256 x 256 tiles are
 * not whole rounds of the chip's CUs (the block's N = 3072 projections: 444 tiles = 1.73 rounds) walks the whole rounds one tile per
 * workgroup and cuts the tiles of the last round(s) along K over one more full round of workgroups; partial tiles meet in `workspace`
 * (fp32, summed in a fixed order: results are run-to-run identical). workspace: yume_gemm_workspace_bytes() bytes, 16-byte aligned, ZERO
 * when first handed over (a launch returns every flag word to zero: no memset between launches, capturable into a hipGraph); launches
 * that share one workspace must be ordered on one stream (yume_amd/ops.py keeps one per device and stream). workspace = NULL or too
 * small: the schedules without it (whole tiles; row split + remainder launch), i.e. exactly yume_gemm_bf16. The word behind the last
 * flag (byte offset yume_gemm_workspace_bytes() - 64) is an error word: non-zero after a launch whose finisher timed out on a flag. */
int64_t yume_gemm_workspace_bytes(void);
int yume_gemm_bf16_ws(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                      int64_t M, int64_t N, int64_t K, int epi,
                      void* out, int64_t ldo,
                      const float* gate, int64_t gate_stride, const int32_t* row_idx,
                      void* outT, int64_t ldt, int64_t n_split,
                      int variant, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- FP8 (OCP e4m3fn) FFN linears (r15; functions added, no argument list changed: ABI 9) ---------------------------------
 * replaces (opt-in, DiTEngine.fp8_ffn): the two FFN linears of a block, wan23/modules/model.py:265-267,309-312.
 *
 * yume_quant_rows_e4m3: per-row absmax quantiser. x bf16 [R, K] (row stride ldx elements), q u8 [R, K] (row stride ldq bytes),
 * scale fp32 [R]:
 *     amax = max_k |x[r, k]|;  scale[r] = amax / 448.0f (one IEEE fp32 division; 1.0f for an all-zero row);
 *     q[r, k] = e4m3_rne(clamp(x[r, k] / scale[r], +-448))          (clamped BEFORE the conversion: no byte is 0x7f / 0xff)
 * x / scale is formed with a reciprocal: |q - x / scale| <= half an e4m3 ulp + 2^-20 |x / scale|. Bytes beyond K of a q row and rows
 * beyond R are not written. Checks (YUME_EINVAL): K % 16 == 0, ldq % 16 == 0, ldx % 8 == 0, ldx >= K, ldq >= K, x and q 16-byte
 * aligned. R == 0: YUME_OK, nothing is launched. The same call quantises activations [L, K] and weights [N, K] (one scale per channel).
 *
 * yume_gemm_f8:   acc[m, n] = sum_k Aq[m, k] * Wq[n, k]  (e4m3 x e4m3, fp32 sum);   y = acc * sa[m] * sw[n] + bias[n];  then `epi`:
 *   YUME_EPI_BF16 / YUME_EPI_BF16_GELU (tanh) / YUME_EPI_F32 / YUME_EPI_RESID with out, ldo, gate, gate_stride, row_idx exactly as in
 *   yume_gemm_bf16_ws; any other epilogue: YUME_EUNSUP.
 * Aq u8 [M, K] (row stride lda bytes), Wq u8 [N, K] (ldw), sa fp32 [M], sw fp32 [N], bias fp32 [N] or NULL.
 * Accuracy of the sum: v_mfma_scale_f32_16x16x128_f8f6f4 does not add its 128 products like an fp32 chain; measured on the bare
 * instruction it errs by up to 3.2e-4 * sqrt(sum_k (a_k w_k)^2) per k-step, unbiased (profiles/r15_fp8_ffn.md) — far below the e4m3
 * rounding of the operands, above the bf16 GEMM's fp32 sums. tests/gemm_f8_cases.py holds the call to twice that figure.
 * Checks (YUME_EINVAL): K % 128 == 0, lda % 16 == 0, ldw % 16 == 0, N % 4 == 0, ldo % 4 == 0, Aq / Wq / out / sw / bias / gate 16-byte
 * aligned, gate_stride % 4 == 0. M >= 1, N >= 1 otherwise arbitrary. One 256 x 256 output tile per workgroup, nothing is handed between
 * workgroups; no workspace, no allocation, the caller's stream. */
int yume_quant_rows_e4m3(const void* x, int64_t ldx, int64_t R, int64_t K, void* q, int64_t ldq, float* scale, void* stream);
int yume_gemm_f8(const void* Aq, int64_t lda, const float* sa, const void* Wq, int64_t ldw, const float* sw,
                 const float* bias, int64_t M, int64_t N, int64_t K, int epi, void* out, int64_t ldo,
                 const float* gate, int64_t gate_stride, const int32_t* row_idx, void* stream);
/* yume_gemm_f8_splitt (the QKV form): yume_gemm_f8's operands, sum and scales, y = acc * sa[m] * sw[n] + bias[n], stored as
 * YUME_EPI_BF16_SPLITT of yume_gemm_bf16 stores it: columns n < n_split to out[m, n] (bf16, row-major, row stride ldo elements),
 * columns n >= n_split to outT[n - n_split, m] (bf16, K-major, row stride ldt elements). V^T columns m >= M and rows >= N - n_split
 * are NOT written, out is never written at columns >= n_split. (yume_gemm_f8 itself keeps answering YUME_EUNSUP to that epilogue.)
 * Checks (YUME_EINVAL): those of yume_gemm_f8 on the operands, and 0 <= n_split <= N, n_split % 256 == 0 (a 256 x 256 tile lies
 * wholly on one side); n_split > 0: out non-NULL, 16-byte aligned, ldo % 4 == 0, ldo >= n_split; n_split < N: outT non-NULL,
 * 16-byte aligned, ldt % 8 == 0, ldt >= M. */
int yume_gemm_f8_splitt(const void* Aq, int64_t lda, const float* sa, const void* Wq, int64_t ldw, const float* sw,
                        const float* bias, int64_t M, int64_t N, int64_t K,
                        void* out, int64_t ldo, void* outT, int64_t ldt, int64_t n_split, void* stream);

/* ---- FP8 FFN without quantiser passes (r16; functions added, no argument list changed: ABI 9) ------------------------------
 * yume_adaln_modulate_e4m3: yume_adaln_modulate(..., out_kind = 0) followed by yume_quant_rows_e4m3 on its bf16 output, in one
 * kernel and without the bf16 row: the modulated value is rounded to bf16, the row amax of those values gives scale[t] = amax / 448
 * (1 for a zero row), the bytes are the quantiser's. q u8 [T, C] (row stride ldq bytes) and scale fp32 [T] equal the two-call
 * composite bit for bit. Checks (YUME_EINVAL): C % 16 == 0, C <= 8192, ldq % 16 == 0, ldq >= C, ldx % 4 == 0, tab_stride % 4 == 0,
 * q 16-byte aligned. Bytes beyond C of a q row and rows beyond T are not written. T == 0: YUME_OK, nothing is launched. */
int yume_adaln_modulate_e4m3(const float* x, int64_t ldx, int64_t T, int64_t C, float eps, const float* mul,
                             const float* add, int64_t tab_stride, const int32_t* row_idx, int add_one,
                             void* q, int64_t ldq, float* scale, void* stream);
/* The OCP MX pair between ffn.0 and ffn.2: e4m3 bytes with one E8M0 scale byte (2^(byte - 127)) per row and 32 consecutive columns.
 *
 * yume_gemm_f8_mxout (the producer; epi must be YUME_EPI_MX_GELU, anything else YUME_EUNSUP): yume_gemm_f8's operands and sum;
 *     v = gelu_tanh(acc * sa[m] * sw[n] + bias[n]) in fp32; per row and block of 32 columns amax = max |v|, e = the smallest integer
 *     with amax <= 448 * 2^e clamped to [-127, 127] (taken from the fp32 bits; 0 for an all-zero block), eo[m, n / 32] = e + 127,
 *     out[m, n] = e4m3_rne(clamp(v * 2^-e, +-448)).  out u8 [M, N] (row stride ldo bytes), eo u8 [M, N / 32] (row stride ldeo).
 *     Checks: those of yume_gemm_f8 and N % 32 == 0, ldeo >= N / 32. Rows beyond M, bytes beyond N and scale bytes beyond N / 32 are
 *     not written.
 * yume_gemm_f8_mx (the consumer): acc[m, n] = sum_b 2^(ea[m, b] - 127) * sum_{k in block b} Aq[m, k] * Wq[n, k], the block scales
 *     applied by v_mfma_scale_f32_16x16x128_f8f6f4 itself (scale map: profiles/r16_fp8_ffn_fused.md); y = acc * sw[n] + bias[n]; then
 *     YUME_EPI_F32 or YUME_EPI_RESID as in yume_gemm_f8 (any other epilogue: YUME_EUNSUP). ea u8 [M, K / 32], row stride ldea with
 *     ldea % 16 == 0 and ldea >= K / 32: the kernel reads a row's scale bytes in whole 16-byte groups, so up to 15 bytes behind K / 32
 *     inside the pitch are read (never used). Other checks as yume_gemm_f8. Accuracy of the sum with unequal block scales: measured
 *     3.8e-4 * sqrt(sum_k (2^e a_k w_k)^2) at worst; tests/gemm_f8_mx_cases.py holds the call to twice that. */
int yume_gemm_f8_mxout(const void* Aq, int64_t lda, const float* sa, const void* Wq, int64_t ldw, const float* sw,
                       const float* bias, int64_t M, int64_t N, int64_t K, int epi, void* out, int64_t ldo,
                       void* eo, int64_t ldeo, void* stream);
int yume_gemm_f8_mx(const void* Aq, int64_t lda, const void* ea, int64_t ldea, const void* Wq, int64_t ldw, const float* sw,
                    const float* bias, int64_t M, int64_t N, int64_t K, int epi, void* out, int64_t ldo,
                    const float* gate, int64_t gate_stride, const int32_t* row_idx, void* stream);

/* ---- MXFP6 (OCP e2m3) FFN linears (r23; functions added, no argument list changed: ABI 9) ----------------------------------
 * replaces (opt-in, DiTEngine.fp6_ffn): the FFN adaLN and the two FFN linears of a block, wan23/modules/model.py:265-267,309-312.
 *
 * The format, once: e2m3 = 1 sign, 2 exponent bits (bias 1), 3 mantissa bits, no inf / nan; largest value 7.5, subnormal step 0.125.
 * 32 values pack into 24 bytes, value i at bits [6 i, 6 i + 6) of the group, little-endian: a row of K values is 3 K / 4 bytes. One
 * E8M0 byte per row and 32 consecutive k: e = the smallest integer with amax <= 7.5 * 2^e, byte e + 127 clamped below at 0, 127 for an
 * all-zero block (the project's MX rule with 7.5 in place of 448); q = e2m3_rne(clamp(v * 2^-e, +-7.5)).
 *
 * yume_adaln_modulate_mx_e2m3: yume_adaln_modulate(..., out_kind = 0) followed by that quantiser on its bf16 output, in one kernel and
 *   without the bf16 row: q u8 [T, 3 C / 4] (row stride ldq bytes) and e u8 [T, C / 32] (row stride lde) equal the two-step composite
 *   bit for bit. Checks (YUME_EINVAL): C % 32 == 0, C <= 8192, ldq % 16 == 0, ldq >= 3 C / 4, lde % 16 == 0, lde >= C / 32, ldx % 4 == 0,
 *   tab_stride % 4 == 0, q 16-byte aligned. Bytes beyond 3 C / 4 of a q row, scale bytes beyond C / 32 and rows beyond T are not
 *   written. T == 0: YUME_OK, nothing is launched. YUME_NORM_LOG=1: `[norm] adaln_e2m3<MAXV> ...` / `[norm] adaln2_e2m3 ...`.
 * yume_gemm_f6_mx (the consumer): acc[m, n] = sum_b 2^(ea[m, b] - 127) 2^(ew[n, b] - 127) sum_{k in block b} A[m, k] W[n, k], both block
 *   scales applied by v_mfma_scale_f32_16x16x128_f8f6f4 itself (maps: profiles/r23_fp6_ffn.md); y = acc + bias[n]; then YUME_EPI_F32 or
 *   YUME_EPI_RESID with out, ldo, gate, gate_stride, row_idx as in yume_gemm_bf16_ws (any other epilogue: YUME_EUNSUP).
 *   A6 u8 [M, 3 K / 4] (lda bytes), ea u8 [M, K / 32] (ldea), W6 u8 [N, 3 K / 4] (ldw), ew u8 [N, K / 32] (ldew), bias fp32 [N] or NULL.
 *   Checks (YUME_EINVAL): K % 128 == 0, N % 4 == 0, lda / ldw % 16 == 0 and >= 3 K / 4, ldea / ldew % 16 == 0 and >= K / 32 (a row's
 *   scale bytes are read in whole 16-byte groups: up to 15 bytes behind K / 32 inside the pitch are read, never used), ldo % 4 == 0,
 *   every pointer 16-byte aligned, gate_stride % 4 == 0. M >= 1, N >= 1 otherwise arbitrary. One 256 x 256 tile per workgroup.
 * yume_gemm_f6_mxout (the producer; epi must be YUME_EPI_MX6_GELU, anything else YUME_EUNSUP): the same operands and sum;
 *   v = gelu_tanh(acc + bias[n]) in fp32 leaves quantised by the rule above: out u8 [M, 3 N / 4] (ldo bytes), eo u8 [M, N / 32] (ldeo).
 *   Checks: those of yume_gemm_f6_mx on the operands and N % 128 == 0, ldo % 16 == 0, ldo >= 3 N / 4, ldeo % 16 == 0, ldeo >= N / 32
 *   (the output is the next call's A operand). Rows beyond M, bytes beyond 3 N / 4 and scale bytes beyond N / 32 are not written.
 * Accuracy of the sum: tests/gemm_f6_cases.py bounds every element against fp64 on the very bytes the call receives.
 * YUME_GEMM_LOG=1: `[gemm_f6] mx ...` / `[gemm_f6] mxout ...` per launch. */
int yume_adaln_modulate_mx_e2m3(const float* x, int64_t ldx, int64_t T, int64_t C, float eps, const float* mul,
                                const float* add, int64_t tab_stride, const int32_t* row_idx, int add_one,
                                void* q, int64_t ldq, void* e, int64_t lde, void* stream);
int yume_gemm_f6_mx(const void* A6, int64_t lda, const void* ea, int64_t ldea, const void* W6, int64_t ldw, const void* ew, int64_t ldew,
                    const float* bias, int64_t M, int64_t N, int64_t K, int epi, void* out, int64_t ldo,
                    const float* gate, int64_t gate_stride, const int32_t* row_idx, void* stream);
int yume_gemm_f6_mxout(const void* A6, int64_t lda, const void* ea, int64_t ldea, const void* W6, int64_t ldw, const void* ew, int64_t ldew,
                       const float* bias, int64_t M, int64_t N, int64_t K, int epi, void* out, int64_t ldo,
                       void* eo, int64_t ldeo, void* stream);

/* ---- INT8 QKV / cross-q projections (r25; functions added, no argument list changed: ABI 9) -------------------------------
 * replaces (opt-in, DiTEngine.int8_qkv): the first adaLN + QKV projection and norm3 + cross-attention q projection of a block.
 *
 * The format, once (yume_amd/csrc/i8.hpp): symmetric int8 with one fp32 scale per row.
 *     amax = max_k |x[r, k]| over the row's bf16 values;  scale[r] = amax / 127.0f (one IEEE fp32 division; 1.0f for an all-zero row);
 *     q[r, k] = rne(clamp(x[r, k] / scale[r], +-127))               (clamped BEFORE the rounding: no byte is 0x80)
 * x / scale is formed with a reciprocal, as yume_quant_rows_e4m3 forms it: |q - x / scale| <= 0.5 + 2^-20 |x / scale|.
 * Non-finite input: a row that holds an Inf or a NaN gets scale = NaN and all bytes 0 (its GEMM outputs are then NaN); other rows are
 * not affected.
 *
 * yume_quant_rows_i8: the stand-alone quantiser, x bf16 [R, K] (row stride ldx elements), q i8 [R, K] (row stride ldq bytes), scale fp32
 *   [R]. Checks and untouched bytes as yume_quant_rows_e4m3: K % 16 == 0, ldq % 16 == 0, ldx % 8 == 0, ldx >= K, ldq >= K, x and q 16-byte
 *   aligned; bytes beyond K of a q row and rows beyond R are not written; R == 0: YUME_OK, nothing is launched.
 *   YUME_NORM_LOG=1: `[quant] rows_i8 ...` per launch.
 * yume_adaln_modulate_i8: yume_adaln_modulate(..., out_kind = 0) followed by yume_quant_rows_i8 on its bf16 output, in one kernel and
 *   without the bf16 row; q and scale equal the two-call composite bit for bit. Argument list, checks and untouched bytes are those of
 *   yume_adaln_modulate_e4m3. YUME_NORM_LOG=1: `[norm] adaln_i8<MAXV> ...` / `[norm] adaln2_i8 ...`.
 * yume_gemm_i8:   acc[m, n] = sum_k Aq[m, k] * Wq[n, k]  (signed bytes, int32 sum, EXACT: v_mfma_i32_16x16x64_i8);
 *   y = float(acc) * sa[m] * sw[n] + bias[n] (float(): round to nearest even, exact below 2^24);  then `epi`: YUME_EPI_BF16 or
 *   YUME_EPI_F32 into out (row stride ldo elements); any other epilogue: YUME_EUNSUP. Every byte value is taken, 0x80 = -128 included.
 *   Aq i8 [M, K] (row stride lda bytes), Wq i8 [N, K] (ldw), sa fp32 [M], sw fp32 [N], bias fp32 [N] or NULL.
 *   Checks (YUME_EINVAL): those of yume_gemm_f8 — K % 128 == 0, lda % 16 == 0, ldw % 16 == 0, N % 4 == 0, ldo % 4 == 0, Aq / Wq / out /
 *   sw / bias 16-byte aligned — and K <= 131072 (127 * 128 * K stays below 2^31). One 256 x 256 output tile per workgroup, nothing is
 *   handed between workgroups; no workspace, no allocation, the caller's stream.
 * yume_gemm_i8_splitt (the QKV form): the same sum and scales, stored as yume_gemm_f8_splitt stores them: columns n < n_split to
 *   out[m, n] (bf16 row-major), columns n >= n_split to outT[n - n_split, m] (bf16, K-major); the checks of yume_gemm_f8_splitt
 *   (n_split % 256 == 0, ...) and K <= 131072.
 * YUME_GEMM_LOG=1: `[gemm_i8] i8 M= N= K= epi= ...` per launch (`... ldt= n_split=` for the QKV form, epi = 4). */
int yume_quant_rows_i8(const void* x, int64_t ldx, int64_t R, int64_t K, void* q, int64_t ldq, float* scale, void* stream);
int yume_adaln_modulate_i8(const float* x, int64_t ldx, int64_t T, int64_t C, float eps, const float* mul,
                           const float* add, int64_t tab_stride, const int32_t* row_idx, int add_one,
                           void* q, int64_t ldq, float* scale, void* stream);
int yume_gemm_i8(const void* Aq, int64_t lda, const float* sa, const void* Wq, int64_t ldw, const float* sw,
                 const float* bias, int64_t M, int64_t N, int64_t K, int epi, void* out, int64_t ldo, void* stream);
int yume_gemm_i8_splitt(const void* Aq, int64_t lda, const float* sa, const void* Wq, int64_t ldw, const float* sw,
                        const float* bias, int64_t M, int64_t N, int64_t K,
                        void* out, int64_t ldo, void* outT, int64_t ldt, int64_t n_split, void* stream);

/* ---- RMSNorm over the hidden dim (+ optional 3D RoPE), in place, bf16 -----------------------
 * replaces: wan23/modules/model.py:121-137 (WanRMSNorm on q,k over the FULL hidden dim C),
 *           :38-118 (rope_apply: interleaved-pair complex multiply with the per-token table).
 *
 * buf: bf16 [T, nparts*C] (row stride ld); part p (p < nparts) = columns [p*C, (p+1)*C):
 *   y = x * rsqrt(mean_C(x^2) + eps) * w_p[c]        (fp32 math)
 *   if rope: head-wise (head_dim D, pairs (2j,2j+1)):  (y0,y1) <- (y0*cos - y1*sin, y0*sin + y1*cos)
 *            with rope = fp32 [T, D/2, 2] (cos, sin) per token, shared by all heads.
 * w: fp32 [nparts, C].   C % 512 == 0, D == 128.
 * eps < 0: the rows are NOT normalised — y = x * w_p[c], then RoPE: the reference's nn.Identity in place of WanRMSNorm when a model is
 *   built with qk_norm=False (wan23/modules/model.py:175-176); w then carries ones (times the attention scale on the q side). The same
 *   holds for yume_rmsnorm_rows_periodic.
 */
int yume_rmsnorm_rope(void* buf, int64_t ld, int64_t T, int64_t C, int nparts,
                      const float* w, float eps, const float* rope, int64_t D, void* stream);
/* same RMSNorm (no RoPE) with a per-row weight: row t uses w[(t % wperiod), :]. Normalises the cross-attention K of ALL
 * blocks (wan23/modules/model.py:222-226, one WanRMSNorm per block) in one launch over the buffer [tokens, wperiod*C]
 * viewed as [tokens*wperiod, C]. w: fp32 [wperiod, C]. */
int yume_rmsnorm_rows_periodic(void* buf, int64_t ld, int64_t T, int64_t C, const float* w, int64_t wperiod, float eps,
                               void* stream);
/* env YUME_NORM_LOG=1 (read once per process, like YUME_ATTN_LOG, YUME_GEMM_LOG and YUME_CONV_LOG): every kernel launch of
 * yume_adaln_modulate, yume_rmsnorm_f32 (the T5 section below), yume_rmsnorm_rope and yume_rmsnorm_rows_periodic prints one stderr line
 *   `[norm] <instance> T=.. C=.. nparts=.. out_kind=.. ldx=.. ldo=.. tab_stride=.. wperiod=.. rope=0|1 row_idx=0|1`
 * <instance>: adaln2 (two rows per workgroup: C <= 3072, out_kind 0, T >= 1024), adaln<3|5|8> (C <= 3072 / 5120 / 8192), adaln_rms<3|5|8>
 * (yume_rmsnorm_f32), rope2<2|3> (two rows: nparts*C/8 <= 512 / 768 vectors, wperiod 1, T >= 1024), rope<2|3|5|8> (<= 512 / 768 / 1280 /
 * 2048 vectors). The in-place kernels print their one stride as ldx and ldo. tests/norm_cases.py holds one row per instance. */

/* ---- exact-softmax attention forward (FlashAttention-style, head_dim 128) -----------------
 * replaces: wan23/modules/attention.py:24-130 flash_attention() -> flash_attn_varlen_func
 *           (external flash-attn 2.7.0.post2), call sites wan23/modules/model.py:197-202,227.
 *
 *   O[h, i, :] = softmax_j( scale * <Q[h,i,:], K[h,j,:]> ) V[h, j, :]     j < Lk, no mask, no dropout
 * Q: bf16, token-major: element (i, h, d) at Q[i*ldq + h*128 + d];  K likewise (ldk).
 * Vt: bf16 K-major ("V transposed"): element (j, h, d) at Vt[(h*128 + d)*ldvt + j], ldvt >= Lk,
 *     ldvt % 8 == 0 (the image written by YUME_EPI_BF16_SPLITT / yume_transpose_bf16).
 * O: bf16 token-major (ldo). accumulate != 0: O += result (the 14B image cross-attention sum,
 *    wan/modules/model.py:379-387) using the fp32 accumulator before rounding.
 * variant: 0 = automatic (Lk >= 1536 and Lq >= 256: the one-wave-per-SIMD kernel, 256 queries per workgroup; otherwise
 *    the 4-wave LDS-DMA kernel), 1 = 4-wave register-staged kernel (attn_fwd_v1.hpp), 2 = 4-wave LDS-DMA kernel (attn_fwd_v2.hpp),
 *    4 = 8-wave ping-pong kernel (attn_fwd_v4.hpp), 7 = one-wave-per-SIMD kernel (attn_fwd7.hip), 8 = its persistent form (attn_fwd8.hip; needs the two flags below),
 *    9 = the short-key kernel with K and V^T resident in registers (attn_cross_rk.hpp, r6: 448 < Lk <= 512, Lq >= 1024, ldvt >= 512, and
 *    for Lk < 512 YUME_ATTN_KV_PADDED — the 512-token text cross-attention; measured slower than the 4-wave kernel as built, so variant 0
 *    takes it only with env YUME_ATTN_RK=1). All compute the same function (tests compare them).
 *    | YUME_ATTN_Q_PRESCALED: Q already carries scale * log2(e) — the caller folded that factor into the producer of Q before
 *    its one bf16 rounding (the DiT engine multiplies it into the RMSNorm weight of q, so yume_rmsnorm_rope writes it) — and
 *    `scale` is ignored:  O = sum_j 2^<Q,K_j> V_j / sum_j 2^<Q,K_j>.  The scores then leave the matrix pipe as the exponents
 *    themselves; the one-wave-per-SIMD kernel drops the per-score shift and keeps NO running base (floating point is
 *    scale-invariant: exp2(s - m) and exp2(s) carry the same relative error, m cancels in O / l). Its guard is a range check
 *    of every row sum and output at the end of a workgroup; a workgroup that fails it (scores beyond about +-100 in the log2
 *    domain) is rerun in the same launch on the kernel's rescaling path, so the result is defined for every input.
 */
#define YUME_ATTN_Q_PRESCALED 0x100
/*    | YUME_ATTN_KV_PADDED: the caller guarantees that K has at least ceil(Lk/64)*64 readable rows (whatever they hold) and that Vt has
 *    ldvt >= ceil(Lk/64)*64 with FINITE values in the columns >= Lk (they are multiplied by exact zeros). It opens the persistent
 *    kernel (attn_fwd8.hip: one resident workgroup per CU draws (head, query block) items by ticket and streams K / V^T tiles
 *    continuously across them — the ragged last key tile is fetched like any other and only masked). Which calls take it:
 *      variant 0 (automatic): both flags AND Lk >= 1536 AND Lq >= 256 (where variant 0 would take the one-wave-per-SIMD kernel at all;
 *        the 512-key cross-attention stays on the 4-wave kernel, which measured faster there — also than r6's variant 9) AND a registered counter workspace
 *        (yume_counter_workspace_init) AND Lq * ldq * 2 + 512 < 2^32 (the kernel addresses a query row by a 32-bit byte offset from
 *        its head's base). A call that misses one of these runs variant 7 / 2 as before — silently, it is the same function;
 *        env YUME_ATTN_V8=0 keeps variant 0 off the persistent kernel (A/B runs);
 *      variant 8: insists on it — both flags, Lk >= 512, Lq >= 256, the workspace and the 32-bit limit are then REQUIRED (YUME_EINVAL
 *        by name otherwise). It is the only way to run the persistent kernel for 512 <= Lk < 1536.
 *    Same arithmetic per key tile in the same order as variant 7: whole query blocks are bit-identical. */
#define YUME_ATTN_KV_PADDED 0x200
int yume_attn_fwd(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt,
                  void* O, int64_t ldo, int64_t Lq, int64_t Lk, int64_t H, float scale,
                  int accumulate, int variant, void* stream);
/* Same call with caller-owned scratch (yume_attn_workspace_bytes(Lq, Lk, H) bytes, 0 = none needed; 16-byte aligned): in the
 * automatic mode the query blocks that would form a partial last round of workgroups are then cut into 2-4 key ranges inside
 * the same launch (fp32 partial O, running max and row sum in the scratch) and merged in a fixed order. */
int64_t yume_attn_workspace_bytes(int64_t Lq, int64_t Lk, int64_t H);
int yume_attn_fwd_ws(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt,
                     void* O, int64_t ldo, int64_t Lq, int64_t Lk, int64_t H, float scale,
                     int accumulate, int variant, void* workspace, int64_t workspace_bytes, void* stream);
/* The same call with a WEIGHTED LAST KEY: key Lk-1 stands for `last_key_weight` identical keys,
 *   O[h,i,:] = sum_j w_j e^{scale <Q_i,K_j>} V_j / sum_j w_j e^{scale <Q_i,K_j>},   w_j = 1 for j < Lk-1,  w_{Lk-1} = last_key_weight
 * replaces: the reference's un-masked 512-key cross-attention over a zero-padded prompt (wan23/modules/model.py:815-821 with
 *           context_lens = None, wan/modules/model.py:931-936; wan/modules/t5.py:511-513 trims each prompt to its real length first). A zero
 *           row through text_embedding is a constant vector, so keys n .. 511 of an n-token prompt are copies of one key: softmax over
 *           n real keys and m copies of key p equals softmax over n + 1 keys in which key p counts m times. Nothing is approximated; a run
 *           of repeated keys anywhere else can be folded the same way by putting it last.
 * last_key_weight: by value (a captured graph needs no extra device memory); finite and in [1, 2^20], YUME_EINVAL otherwise. With
 *    YUME_ATTN_Q_PRESCALED the meaning is the same (the weight multiplies 2^s). The kernels multiply the last key's exponential (one bf16
 *    rounding of w e^s before the P V product); the running-base logic sees the plain score.
 * last_key_weight == 1 is exactly yume_attn_fwd_ws: same kernel choice, same bits. A weight != 1 is served by
 *    variant 10 = the short-key kernel (attn_short.hpp, r7: Lk <= 128, a head's K and V^T resident in one wave's registers, exact single-pass
 *                 softmax, no LDS, no workspace; also needs ldo % 8 == 0 and a 16-byte aligned O; selectable at any weight), and
 *    variant 2  = the 4-wave LDS-DMA kernel, any Lk (the last key tile takes the masked body, also when Lk % 64 == 0);
 *    variant 0  = the short-key kernel where it applies (Lk <= 128, ldo % 8 == 0, 16-byte aligned O: measured 1.6-1.9 x faster than variant 2
 *                 on both cross-attention shapes, profiles/r7_dedup_pad_keys.md; env YUME_ATTN_SHORT=0 keeps variant 0 off it for A/B runs),
 *                 otherwise variant 2 — also for Lk >= 1536;
 *    variants 1, 4, 7, 8, 9 return YUME_EUNSUP (the message names the variant).
 * accumulate, ragged Lq, both scale modes and YUME_ATTN_KV_PADDED as above. The workspace is not used by a weighted call. */
int yume_attn_fwd_kw(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt,
                     void* O, int64_t ldo, int64_t Lq, int64_t Lk, int64_t H, float scale,
                     int accumulate, int variant, void* workspace, int64_t workspace_bytes, float last_key_weight, void* stream);
/* SLIDING-WINDOW / CAUSAL form (r26; a function added, no argument list changed: ABI 9). flash-attn 2.7 semantics, bottom-right aligned,
 * with an explicit query position: row i of the call sits at pos(i) = q_pos0 + i on the key axis and
 *   visible(i, j)  <=>  0 <= j < Lk  and  (win_left < 0 or j >= pos(i) - win_left)  and  (win_right < 0 or j <= pos(i) + win_right)
 *   O[h,i,:] = sum_{visible j} e^{scale <Q_i,K_j>} V_j / sum_{visible j} e^{scale <Q_i,K_j>};   O[h,i,:] = 0 where row i sees no key (an
 *   accumulate call then leaves the old O[h,i,:] as it is, bit for bit). Exact softmax over the visible set.
 * replaces: wan23/modules/attention.py:24-130 flash_attention(causal=, window_size=) -> flash_attn_varlen_func(causal, window_size), reached
 *           from WanSelfAttention.forward, wan23/modules/model.py:158-202 (WanModel(window_size=...)). causal is win_right = 0; flash-attn's
 *           alignment of a call with Lq != Lk is q_pos0 = Lk - Lq; a caller that holds a row range of a longer sequence passes the first row's
 *           own index. The reference's FA3 branch ignores the window; that is not reproduced.
 * win_left / win_right: -1 = unbounded on that side. Checks (YUME_EINVAL by name `attn_fwd_band`): everything yume_attn_fwd_ws checks;
 *    win_left, win_right >= -1; q_pos0 in [-2^31, 2^31).
 * A (q_pos0, win_left, win_right) that hides no (i, j) pair of the call IS yume_attn_fwd_ws with the same arguments: same kernel choice, same
 *    log line, same bits. Only a call that hides at least one pair runs the banded kernel (attn_band.hpp: attn_fwd_kernel_v2's tile walk over
 *    the key tiles some row of a 128-query workgroup sees, the mask applied to the scores before the row maximum):
 *    variant 0 and variant 11 = that kernel; any other variant: YUME_EUNSUP (the message names it).
 * accumulate, ragged Lq, both scale modes and YUME_ATTN_KV_PADDED (accepted; it changes nothing here) as for yume_attn_fwd. No weighted last
 *    key, no key-range split; the workspace is handed on to yume_attn_fwd_ws and otherwise unused.
 * env YUME_ATTN_LOG=1: one line per banded call, `[attn_fwd_band] band q_pos0=.. left=.. right=.. tiles_min=.. tiles_max=.. Lq=.. Lk=.. H=..
 *    ...` (the fewest and the most key tiles a workgroup walks). tests/test_attn_band_routes_gpu.py reads it back. */
int yume_attn_fwd_band(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt,
                       void* O, int64_t ldo, int64_t Lq, int64_t Lk, int64_t H, float scale, int accumulate, int variant,
                       int64_t q_pos0, int64_t win_left, int64_t win_right,
                       void* workspace, int64_t workspace_bytes, void* stream);
/* FRAME-WINDOW / FRAME-CAUSAL form (r28; a function added, no argument list changed: ABI 9). The key axis is partitioned into blocks — the
 * frames of a video sequence — by nspan (1 .. 16) uniform spans: span g starts at row row0_g (row0_0 = 0, row0_{g+1} = row0_g + span_rows[g] *
 * span_blocks[g]) and holds span_blocks[g] blocks of span_rows[g] rows each; N rows and NB blocks in all, numbered through the spans in order.
 * b(p) = the block of position p. Row i of the call sits at pos(i) = q_pos0 + i and
 *   visible(i, j)  <=>  0 <= j < Lk  and  (back < 0 or b(j) >= b(pos(i)) - back)  and  (ahead < 0 or b(j) <= b(pos(i)) + ahead)
 *   O[h,i,:] = exact softmax over the visible keys;  O[h,i,:] = 0 where row i sees no key (an accumulate call then leaves the old O[h,i,:] as
 *   it is, bit for bit): yume_attn_fwd_band's rules. A row's visible set is one interval, start(max(b - back, 0)) ... min(end(min(b + ahead,
 *   NB - 1)), Lk) - 1. back / ahead: -1 = unbounded on that side; (-1, 0) is the frame-causal (block-causal) mask.
 * replaces: nothing the reference computes — wan23/modules/model.py runs global self-attention over the FramePack sequence; this is the
 *           frame-aligned form of the window of wan23/modules/attention.py:24-130 flash_attention(window_size=), which counts tokens and so
 *           cuts frames part-way and spans dozens of frames in a coarse history group (yume_amd/framepack.py frame_spans gives the partition).
 * span_rows / span_blocks: HOST arrays of nspan entries, read during the call and handed to the kernel by value (no device memory, nothing a
 *    stream capture could lose), as yume_attn_fwd_seg's arrays.
 * Checks (YUME_EINVAL by name `attn_fwd_fband`): everything yume_attn_fwd_ws checks; nspan in [1, 16]; every span_rows[g], span_blocks[g] >= 1;
 *    N < 2^31; back, ahead >= -1; 0 <= q_pos0; q_pos0 + Lq <= N; Lk <= N.
 * A (partition, back, ahead, q_pos0) that hides no (i, j) pair of the call IS yume_attn_fwd_ws with the same arguments: same kernel choice, same
 *    log line, same bits. One span of one-row blocks computes yume_attn_fwd_band(win_left = back, win_right = ahead), bit for bit. Only a call
 *    that hides at least one pair runs the kernel (attn_fband.hpp: attn_band_kernel's walk, each lane's key interval from its row's block):
 *    variant 0 and variant 12 = that kernel; any other variant: YUME_EUNSUP (the message names it).
 * accumulate, ragged Lq, both scale modes and YUME_ATTN_KV_PADDED (accepted; it changes nothing here) as for yume_attn_fwd. No weighted last
 *    key, no key-range split; the workspace is handed on to yume_attn_fwd_ws and otherwise unused.
 * env YUME_ATTN_LOG=1: one line per banded call, `[attn_fwd_fband] fband q_pos0=.. back=.. ahead=.. nspan=.. nblocks=.. tiles_min=..
 *    tiles_max=.. Lq=.. Lk=.. H=.. ...` (the fewest and the most key tiles a workgroup walks). tests/test_attn_fband_routes_gpu.py reads it. */
int yume_attn_fwd_fband(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt,
                        void* O, int64_t ldo, int64_t Lq, int64_t Lk, int64_t H, float scale, int accumulate, int variant,
                        int64_t q_pos0, int64_t nspan, const int64_t* span_rows, const int64_t* span_blocks, int64_t back, int64_t ahead,
                        void* workspace, int64_t workspace_bytes, void* stream);
/* FRAME-WINDOW form WITH A SINK (r29; a function added, no argument list changed: ABI 9). yume_attn_fwd_fband's partition, pos(i), b(p), back
 * and ahead, and one more integer: the first `sink` blocks (0 <= sink <= NB) are seen by every row —
 *   visible(i, j)  <=>  0 <= j < Lk  and  ( b(j) < sink  or  yume_attn_fwd_fband's visible(i, j) )
 *   With send = min(start(sink), Lk) (start(NB) = N) a row sees [0, send) U [klo(i), khi(i)], klo / khi being yume_attn_fwd_fband's interval:
 *   one interval where klo(i) <= send, two with a hidden gap otherwise. O, the empty row (none with sink >= 1) and accumulate as there.
 * replaces: nothing the reference computes. It is what makes the frame window usable on the sequences of wan23/modules/model.py's FramePack
 *           forward, whose first block is the clip's first frame (yume_amd/framepack.py history_groups: the I2V conditioning image, the anchor
 *           of the long-video loop): the "attention sink" / anchor frames that windowed video attention pairs with a local window.
 * Checks (YUME_EINVAL by name `attn_fwd_fsink`): everything yume_attn_fwd_fband checks; 0 <= sink <= NB.
 * Normalisations: a call that hides no (i, j) pair IS yume_attn_fwd_ws with the same arguments (same kernel choice, log line and bits); sink == 0,
 *    or a sink that shows no pair the window hides, IS yume_attn_fwd_fband with the same arguments (same log line, same bits, its variants).
 *    Only a call whose sink adds a pair runs the kernel (attn_fsink.hpp: a walk over the ascending tile LIST sink tiles + band tiles, the
 *    prefetch following the list across the jump, a two-interval mask): variant 0 and variant 13 = that kernel; any other variant:
 *    YUME_EUNSUP (the message names it).
 * accumulate, ragged Lq, both scale modes, YUME_ATTN_KV_PADDED and the workspace as for yume_attn_fwd_fband.
 * env YUME_ATTN_LOG=1: one line per call that runs the kernel, `[attn_fwd_fsink] fsink q_pos0=.. back=.. ahead=.. sink=.. sink_rows=.. nspan=..
 *    nblocks=.. tiles_min=.. tiles_max=.. Lq=.. Lk=.. H=.. ...` (sink_rows = send; the fewest and the most key tiles a workgroup walks).
 *    tests/test_attn_fsink_routes_gpu.py reads it. */
int yume_attn_fwd_fsink(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt,
                        void* O, int64_t ldo, int64_t Lq, int64_t Lk, int64_t H, float scale, int accumulate, int variant,
                        int64_t q_pos0, int64_t nspan, const int64_t* span_rows, const int64_t* span_blocks, int64_t back, int64_t ahead,
                        int64_t sink, void* workspace, int64_t workspace_bytes, void* stream);
/* FRAME-WINDOW form OVER TWO KEY BUFFERS (r30; a function added, no argument list changed: ABI 9). yume_attn_fwd_fband's arguments describe
 * the SUFFIX (K / Vt / Lk / the spans / back / ahead / q_pos0, with its own key numbering from 0); Kp [n_prefix, H*128] rows ldkp apart and
 * Vtp [H*128, >= n_prefix] rows ldvtp apart are a PREFIX of n_prefix keys in a buffer of their own:
 *   visible(i, j_prefix) for every 0 <= j_prefix < n_prefix;   visible(i, j_suffix)  <=>  yume_attn_fwd_fband's rule on the suffix arguments
 *   O[h,i,:] = exact softmax over the union, in the logical order prefix then suffix. With n_prefix >= 1 no row is empty.
 * replaces: nothing the reference computes. It is what lets a frame-causal FramePack forward keep the K rows / V^T columns of its history
 *           tokens from one denoise step to the next (DiTEngine.cache_history): the history keys are the prefix, the frames being denoised the
 *           suffix, and neither buffer is padded or copied behind the other (n_hist is no multiple of 8, V^T images start 16-byte aligned).
 * Checks (YUME_EINVAL by name `attn_fwd_fprefix`): everything yume_attn_fwd_fband checks on the suffix; n_prefix >= 0; n_prefix + N < 2^31;
 *    with n_prefix > 0: Kp / Vtp non-NULL and 16-byte aligned, ldkp % 8 == 0, ldvtp % 8 == 0, ldvtp >= n_prefix.
 * Normalisation: n_prefix == 0 IS yume_attn_fwd_fband with the same suffix arguments (same log line, same bits, its variants). Every
 *    n_prefix >= 1 runs the kernel (attn_fprefix.hpp: the ceil(n_prefix / 64) prefix tiles, then the suffix's band tiles, the prefetch
 *    switching buffers and strides in between; a ragged last tile of either segment is register-staged with that segment's key bound, so
 *    neither buffer needs padding and no key behind n_prefix or Lk enters a product): variant 0 and variant 14 = that kernel; any other
 *    variant: YUME_EUNSUP (the message names it).
 * accumulate, ragged Lq and both scale modes as for yume_attn_fwd_fband; YUME_ATTN_KV_PADDED is accepted and changes nothing. No key weight, no
 *    key-range split; the workspace is handed on to yume_attn_fwd_fband and otherwise unused.
 * env YUME_ATTN_LOG=1: one line per call that runs the kernel, `[attn_fwd_fprefix] fprefix n_prefix=.. prefix_tiles=.. q_pos0=.. back=..
 *    ahead=.. nspan=.. nblocks=.. tiles_min=.. tiles_max=.. Lq=.. Lk=.. H=.. ...`. tests/test_attn_fprefix_routes_gpu.py reads it. */
int yume_attn_fwd_fprefix(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt,
                          void* O, int64_t ldo, int64_t Lq, int64_t Lk, int64_t H, float scale, int accumulate, int variant,
                          int64_t q_pos0, int64_t nspan, const int64_t* span_rows, const int64_t* span_blocks, int64_t back, int64_t ahead,
                          const void* Kp, int64_t ldkp, const void* Vtp, int64_t ldvtp, int64_t n_prefix,
                          void* workspace, int64_t workspace_bytes, void* stream);
/* SEGMENTED form (r9): ONE launch serves nseg (1 .. 8) independent attention problems that share Q's and O's buffers and every shape but the
 * key count. Segment s owns the query rows [s * seg_pitch, s * seg_pitch + Lq_seg) of Q and O (seg_pitch >= Lq_seg, in rows; the rows of the
 * gap are neither read nor written) and attends over its own K[s] / Vt[s] (Lk[s] keys, key Lk[s] - 1 counting last_key_weight[s] times).
 * replaces: the text cross-attention of the two forwards of a classifier-free-guidance pair (fastvideo/sample/sample.py:774-779 calls the
 *           model twice with everything equal but `context`), run as one pass over the stacked rows of both (DiTEngine.forward_pair).
 * K, Vt: HOST arrays of nseg device pointers; Lk: host array of nseg key counts; last_key_weight: host array of nseg weights, or NULL = all 1.
 *    The arrays are read during the call and travel to the kernel by value (a captured graph needs no device memory for them). No workspace.
 * ldq, ldk, ldvt (>= every Lk[s]), ldo, H, scale, accumulate, YUME_ATTN_Q_PRESCALED / YUME_ATTN_KV_PADDED: as for yume_attn_fwd_kw, common
 *    to all segments. Checks (YUME_EINVAL by name): nseg in [1, 8], seg_pitch >= Lq_seg, every pointer non-NULL and 16-byte aligned, every
 *    Lk[s] >= 1, every weight finite and in [1, 2^20].
 * variant 0  = the segmented short-key kernel when EVERY Lk[s] <= 128 (and ldo % 8 == 0, 16-byte aligned O, env YUME_ATTN_SHORT not 0),
 *              otherwise the segmented 4-wave LDS-DMA kernel;
 * variant 10 = insists on the short-key kernel (YUME_EINVAL when some Lk[s] > 128 or the alignment fails); variant 2 on the 4-wave kernel;
 * any other variant: YUME_EUNSUP (the message names it).
 * nseg == 1 is yume_attn_fwd_kw(Q, .., K[0], .., Vt[0], .., Lq_seg, Lk[0], .., last_key_weight[0]): same kernel choice, same bits.
 * env YUME_ATTN_LOG=1 (read once per process, beside YUME_ATTN_V8, YUME_ATTN_SHORT and YUME_ATTN_RK): every call of the four entry points
 *    prints one line on stderr that names the kernel it runs on (v1, v2, v2w = v2 with the weighted last key, v4, v7, v8, rk, short,
 *    seg_short, seg_v2), for v7 / v8 the plan (tail_qb, splits; v8 also its workgroup count nwg), then the shape, the row strides and the
 *    flags. Host code only: the kernels are the same with the switch on. tests/test_attn_routes_gpu.py reads it back. */
int yume_attn_fwd_seg(const void* Q, int64_t ldq, const void* const* K, int64_t ldk, const void* const* Vt, int64_t ldvt,
                      void* O, int64_t ldo, int64_t nseg, int64_t Lq_seg, int64_t seg_pitch, const int64_t* Lk, int64_t H,
                      float scale, int accumulate, int variant, const float* last_key_weight, void* stream);
/* BATCHED self-attention (r12): ONE launch serves nseg (1 .. 8) attention problems of ONE shape that are stacked in the same buffers. Segment s
 * owns the rows [s * q_pitch, s * q_pitch + Lq_seg) of Q and O, the rows [s * k_pitch, s * k_pitch + Lk_seg) of K and the columns of Vt from
 * s * k_pitch on. Rows and columns in the pitch gaps are neither read for a result nor written.
 * replaces: B separate calls of the model for B samples (the reference's packed path is single-sample by construction,
 *           wan/modules/model.py:474-475,1011), run as one pass over the stacked rows of all of them (DiTEngine.forward_batch).
 * ldq, ldk, ldvt, ldo, H, scale, accumulate, YUME_ATTN_Q_PRESCALED / YUME_ATTN_KV_PADDED (per segment): as for yume_attn_fwd_ws.
 * Checks (YUME_EINVAL by name): nseg in [1, 8]; q_pitch >= Lq_seg; k_pitch a multiple of 64 and >= ceil(Lk_seg/64)*64;
 *    ldvt >= (nseg-1)*k_pitch + ceil(Lk_seg/64)*64; Q, K, Vt, O non-NULL and 16-byte aligned; a workspace that is given is 16-byte aligned and
 *    holds yume_attn_batch_workspace_bytes(nseg, Lq_seg, Lk_seg, H) bytes (NULL: no query block is cut into key ranges).
 * variant 0  = the persistent kernel over (segment, head) pairs (attn_batch8.hip: attn_fwd8.hip's kernel, an item's head being the virtual
 *              head s * H + h; the plan is that of nseg * H heads) when both flags are set, a counter workspace is registered, Lk_seg >= 1536,
 *              Lq_seg >= 256 and Lq_seg * ldq * 2 + 512 < 2^32 — a limit on ONE segment's extent: a segment's base is a 64-bit offset, the stacked
 *              buffers may exceed 4 GiB; otherwise one launch of the segmented 4-wave LDS-DMA kernel (yume_attn_fwd_seg's) over views;
 * variant 8  = insists on the persistent kernel: the conditions are REQUIRED, with Lk_seg >= 512; variant 2 insists on the 4-wave kernel;
 * any other variant: YUME_EUNSUP (the message names it).
 * Same arithmetic per key tile in the same order as yume_attn_fwd's variant 8: segment s is bit-identical to that call on the segment's
 *    views whenever both carry the same plan. nseg == 1 is yume_attn_fwd_ws: same kernel choice, same bits.
 * env YUME_ATTN_LOG=1: one line per call, `[attn_fwd_batch] batch_v8 tail_qb=.. splits=.. nwg=.. nseg=.. ...` or `[attn_fwd_batch] seg_v2 ...`. */
int64_t yume_attn_batch_workspace_bytes(int64_t nseg, int64_t Lq_seg, int64_t Lk_seg, int64_t H);
int yume_attn_fwd_batch(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt,
                        void* O, int64_t ldo, int64_t nseg, int64_t Lq_seg, int64_t q_pitch,
                        int64_t Lk_seg, int64_t k_pitch, int64_t H, float scale, int accumulate, int variant,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* ---- FP8 self-attention, OCP MX e4m3 operands (r22; functions added, no argument list changed: ABI 9) -------------------------
 * replaces (opt-in, DiTEngine.fp8_attn): the self-attention of a block in the single-sample forward, wan23/modules/model.py:139-162.
 *
 * The MX rule of all three (the one of yume_gemm_f8_mxout / yume_vae_rmsnorm_silu_mx): per block of 32 values amax = max |v|, e = the
 * smallest integer with amax <= 448 * 2^e, scale byte e + 127 clamped below at 0, 127 for an all-zero block,
 * q = e4m3_rne(clamp(v * 2^-e, +-448)).
 *
 * yume_quant_rows_mx_e4m3: x bf16 [R, K] (row stride ldx elements) -> q u8 [R, K] (row stride ldq bytes), e u8 [R, K / 32] (row stride
 *   lde bytes), one block per row and 32 consecutive columns. Bytes beyond K / K / 32 of a row and rows beyond R are not written.
 *   Checks (YUME_EINVAL, by name `quant_rows_mx_e4m3`): K % 32 == 0, ldx % 8 == 0, ldx >= K, ldq % 16 == 0, ldq >= K, lde >= K / 32, every
 *   pitch below 2^31, x and q 16-byte aligned, non-NULL. R == 0: YUME_OK, nothing is launched.
 *   One call on qk [L, 2 C] gives q8 | k8 and, per row, the 4 H scale bytes of q followed by the 4 H of k.
 * yume_attn_vt_mx_e4m3: the bf16 K-major V^T image Vt [C, Lk] (row stride ldvt elements) -> the e4m3 image Vt8 [C, 128 * tiles]
 *   (row stride ldvt8 bytes), tiles = ceil(Lk / 128), and Ev u8 [tiles, 4 * C] (row stride ldev bytes):
 *       Vt8[c, 128 t + kk] = key 128 t + key_of(kk),   key_of(kk) = 16 w + 4 g + y with g = (kk >> 4) & 3, w = 4 (kk >> 6) + ((kk >> 2) & 3),
 *       y = kk & 3;     Ev[t, 4 c + b] = the scale byte of bytes kk = 32 b .. 32 b + 31 of that tile row
 *   (the order in which the kernel's P operand holds its keys: yume_amd/csrc/quant_mx.hip). Keys >= Lk of the last tile are written as
 *   byte 0x00 under a valid scale byte: the caller never clears anything. Columns of Vt at or beyond Lk are never read.
 *   Checks (by name `attn_vt_mx_e4m3`): C % 128 == 0, C < 65536, Lk >= 1, ldvt % 4 == 0, ldvt >= Lk, ldvt8 % 16 == 0, ldvt8 >= 128 * tiles,
 *   ldev % 4 == 0, ldev >= 4 * C, every pitch below 2^31, Vt 8-byte, Vt8 16-byte, Ev 4-byte aligned, non-NULL.
 * yume_attn_fwd_f8mx: O[i, 128 h + d] = sum_j 2^<q^_i, k^_j> v^_jd / sum_j 2^<q^_i, k^_j> over j < Lk, the hatted operands the dequantised
 *   bytes (the scale and log2(e) are already in q: yume_rmsnorm_rope's q). Q8 u8 [Lq, 128 H] (ldq bytes), Eq u8 [Lq, 4 H] (ldeq),
 *   K8 u8 [Lk, 128 H] (ldk), Ek u8 [Lk, 4 H] (ldek), Vt8 / Ev as above with C = 128 H, O bf16 [Lq, 128 H] (ldo elements). head_dim 128,
 *   any Lq >= 1 and Lk >= 1. Both products run on v_mfma_scale_f32_16x16x128_f8f6f4; the probabilities are rounded once to e4m3 after
 *   a multiplication by 2^8 (p below 2^-18 of the row's running maximum is dropped), the row sum is taken over the unrounded ones.
 *   No accumulate, weighted key, workspace or key split. Rows of O beyond Lq and columns beyond 128 H are not written.
 *   Checks (by name `attn_fwd_f8mx`): non-NULL; Lq, Lk, H >= 1; ldq / ldk % 16 == 0 and >= 128 H; ldeq / ldek % 4 == 0 and >= 4 H;
 *   ldvt8 % 16 == 0 and >= 128 * tiles; ldev % 4 == 0 and >= 512 H; ldo % 4 == 0 and >= 128 H; every pitch below 2^31 (the kernel's
 *   addressing); Q8, K8, Vt8, O 16-byte, Eq, Ek, Ev 4-byte aligned.
 * env YUME_ATTN_LOG=1: `[attn] f8mx Lq=.. Lk=.. H=.. tiles=..` per launch; YUME_NORM_LOG=1: `[quant] rows_mx ...` / `[quant] vt_mx ...`. */
int yume_quant_rows_mx_e4m3(const void* x, int64_t ldx, int64_t R, int64_t K, void* q, int64_t ldq, void* e, int64_t lde, void* stream);
int yume_attn_vt_mx_e4m3(const void* Vt, int64_t ldvt, int64_t C, int64_t Lk, void* Vt8, int64_t ldvt8, void* Ev, int64_t ldev, void* stream);
int yume_attn_fwd_f8mx(const void* Q8, int64_t ldq, const void* Eq, int64_t ldeq, const void* K8, int64_t ldk, const void* Ek, int64_t ldek,
                       const void* Vt8, int64_t ldvt8, const void* Ev, int64_t ldev, void* O, int64_t ldo,
                       int64_t Lq, int64_t Lk, int64_t H, void* stream);

/* ---- small-M fp32 linear (time embedding MLP) ---------------------------------------------
 * replaces: wan23/modules/model.py:459-461,803-812 (time_embedding, time_projection under
 *           autocast(float32)); only R distinct timesteps are evaluated (R <= 8).
 *   out[r, n] = bias[n] + sum_k act(in[r, k]) * W[n, k] ;  act: 0 = identity, 1 = SiLU
 *   out_act: 0 = none, 1 = SiLU applied to the result.
 * W: fp32 (w_bf16 = 0) or bf16 (w_bf16 = 1), [N, K] row-major. K % 8 == 0.
 * add_table (optional, fp32 [N]): out[r, n] += add_table[n] (folds `modulation + e0`).
 */
int yume_linear_smallm_f32(const float* in, int64_t R, int64_t K, const void* W, int w_bf16,
                           const float* bias, int64_t N, int in_act, int out_act,
                           const float* add_table, float* out, void* stream);

/* ---- sinusoidal timestep embedding ---------------------------------------------------------
 * replaces: wan23/modules/model.py:14-24 sinusoidal_embedding_1d (fp64 math, fp32 result).
 * t: fp64 device array (the reference casts positions to float64); row r uses t[t_index[r]]
 * (t_index: device int32 [R], or NULL for t[r]).  out fp32 [R, dim], dim even.
 */
int yume_sinusoidal_embed(const double* t, const int32_t* t_index, int64_t R, int64_t dim,
                          float* out, void* stream);

/* ---- modulation tables -----------------------------------------------------------------------
 * replaces: wan23/modules/model.py:295-297 `(self.modulation.unsqueeze(0) + e).chunk(6)` for every
 *           block at once, and :344 for the head: out[b, r, :] = tab[b, :] + e0[r, :].
 * tab fp32 [B, W] (stacked block.modulation, W = 6*C), e0 fp32 [R, W], out fp32 [B, R, W]. W % 4 == 0.
 */
int yume_modulation_table(const float* tab, const float* e0, int64_t B, int64_t R, int64_t W,
                          float* out, void* stream);

/* ---- patch gather (im2col for stride==kernel Conv3d) ----------------------------------------
 * replaces: wan23/modules/model.py:602-720 patch_embedding{,_2x,_4x,_8x,_16x}(convpadd(...)):
 *           gathers the (1,kh,kw) patches of `nf` frames into a bf16 matrix the GEMM consumes.
 * x: fp32 or bf16 [Cin, F, H, W] contiguous (in_bf16 selects); frames f0 .. f0+nf-1.
 * out: bf16 [nf*Hp*Wp, Kp] with Hp = ceil(H/kh), Wp = ceil(W/kw), column order (c, dh, dw),
 *      zero for h >= H or w >= W (convpadd :918-931) and for columns >= Cin*kh*kw (K padding to Kp).
 */
int yume_patch_gather(const void* x, int in_bf16, int64_t Cin, int64_t F, int64_t H, int64_t W,
                      int64_t f0, int64_t nf, int64_t kh, int64_t kw,
                      void* out, int64_t Kp, void* stream);

/* ---- unpatchify ------------------------------------------------------------------------------
 * replaces: wan23/modules/model.py:867-890 (einsum 'fhwpqrc->cfphqwr', patch (1,ph,pw)).
 * in: fp32 [F*Hp*Wp, ph*pw*Cout] (ld = ldi) ; out: fp32 [Cout, F, Hp*ph, Wp*pw].
 */
int yume_unpatchify(const float* in, int64_t ldi, int64_t Fr, int64_t Hp, int64_t Wp,
                    int64_t ph, int64_t pw, int64_t Cout, float* out, void* stream);

/* ---- layout / dtype helpers -------------------------------------------------------------------
 * yume_cast_bf16: fp32 [rows, cols] (ldi) -> bf16 (ldo), rows beyond `rows_valid` written as 0
 *   (zero-padding the text context to text_len, wan23/modules/model.py:816-821).
 * yume_transpose_bf16: in [rows, cols] (fp32 or bf16, ldi) -> out bf16 [cols, rows] (ldo); builds the
 *   K-major V^T image for callers that enter at the flash_attention() seam with token-major v.
 */
int yume_cast_bf16(const float* in, int64_t ldi, int64_t rows_valid, int64_t rows, int64_t cols,
                   void* out, int64_t ldo, void* stream);
int yume_transpose_bf16(const void* in, int in_bf16, int64_t ldi, int64_t rows, int64_t cols,
                        void* out, int64_t ldo, void* stream);

/* ======================================================================================================
 * Causal 3D VAE (Wan2.2 z=48 stride 4x16x16 and Wan2.1 z=16 stride 4x8x8).
 * Activations are bf16 CHANNELS-LAST [T, H, W, C] (row = one (t,h,w) position, `ldc` elements apart, C % 8 == 0);
 * the reference layout fp32 [C, T, H, W] only exists at the two ends (yume_vae_pack_input / yume_vae_unpack_output).
 * ====================================================================================================== */

/* ---- implicit-GEMM convolution -------------------------------------------------------------------------
 * replaces: wan23/modules/vae2_2.py:17-44 CausalConv3d (3x3x3, (3,1,1), 1x1x1; the 2-frame feat_cache is the
 *           `cache` operand instead of torch.cat + F.pad), :88-98 Upsample(nearest-exact x2)+Conv2d 3x3 (ups=1),
 *           :101-110 ZeroPad2d((0,1,0,1))+Conv2d 3x3 stride 2 and the stride-(2,1,1) time_conv; same classes in
 *           wan/modules/vae.py.
 *   out[(to,ho,wo), co] = bias[co] + sum_{dt,dh,dw,ci} in(ti,hi,wi)[ci] * W[co, ((dt*kh+dh)*kw+dw)*Cin + ci]
 *   ti = to*st + dt - pt: ti < 0 reads cache frame 2+ti (cache = the last two input frames of the previous
 *   chunk, [2,Hin,Win,ldc]) or zeros when cache is NULL; hi = ho*sh + dh - ph, wi likewise, zero outside the frame;
 *   ups != 0: (hi, wi) index a nearest-2x-upsampled view of the input (hi>>1, wi>>1).
 * W: bf16 [Cout, ldw], ldw >= kt*kh*kw*Cin rounded up to 64, zero padded. zero_page: >= 16 zero bytes on the device.
 * Kernel choice (r3, inside the call; every path computes the same sum in fp32, in its own order): stride-1 convolutions whose frames
 *   are whole 256-position tiles with Cin % 64 == 0 (plain or with the folded upsample) run on the one-wave-per-SIMD pipeline
 *   (csrc/conv_w4.hpp; env YUME_CONV_W4=0: the 8-wave kernel); a causal 3x3x3 conv with Cout <= 16 on frames of >= 64 Ki positions
 *   (the decoder head) on the halo-tile kernel (csrc/conv_halo.hpp; YUME_CONV_HALO=0); the 3x3 (x3) stride-1 convolutions of the 96 / 160-channel
 *   levels on csrc/conv_halo_n.hpp (r6; YUME_CONV_HALO_N=0); the encoders' first convolution (8 -> 96, 16 -> 160 channels) on csrc/conv_in.hpp
 *   (r6: weights resident in registers; YUME_CONV_IN=0); everything else on the GEMM kernels with a
 *   gathering A loader. YUME_CONV_KORDER=0/1/2 selects the K walk of that loader (default 2: dt, channel tile, dh, dw).
 * One-frame forms (r24; no signature changed, ABI 9): a causal 3x3x3 convolution of ONE frame without a cache reads zeros through its taps
 *   dt = 0, 1, so the call kt = 1, pt = 0 with W pointing at element 18*Cin of every 27-tap row (ldw unchanged: ldw is the ROW STRIDE of W,
 *   and only >= the padded K of the call made) computes the same sum. Every kernel above takes that form: the halo-tile kernel and the
 *   encoders' first-convolution kernel through an instance of their own (`conv_halo16_kernel<0, 1>`, `conv_in_kernel<.., KT = 1>`: nine
 *   taps resident in registers instead of 27; YUME_CONV_LOG=1 prints `halo` / `conv_in` with k=1x3x3), under the same shape rules as
 *   their 3x3x3 instances. The call reads W up to K = kh*kw*Cin rounded up to 64 in every row: at Cin = 8 / 16 that leaves a 27-tap row
 *   behind its slice, so there the caller passes a zero-padded copy of the slice (yume_amd.vae.live_view_fits).
 * epi: YUME_EPI_BF16 (bias), YUME_EPI_F32, YUME_CONV_EPI_ADD (out = acc + bias + add[m, co], add bf16 [M, ldadd] —
 *      the ResidualBlock skip, vae2_2.py:239), YUME_CONV_EPI_TSPLIT (upsample3d time_conv, vae2_2.py:145-153:
 *      channel halves of frame t become frames 2t and 2t+1: out[((2t+j)*Ho*Wo + hw), c] for co = j*Cout/2 + c),
 *      YUME_CONV_EPI_RMS_SILU (r6): out = SiLU(RMS_norm(acc + bias) * gamma) — the ResidualBlock's second RMS_norm + SiLU behind its first
 *      convolution (wan/modules/vae.py:75-84 RMS_norm = F.normalize over the channels * sqrt(C) * gamma; :190-207 ResidualBlock; vae2_2.py likewise);
 *      `add` then carries the fp32 gamma[Cout] (ldadd ignored). Fused into the epilogue where one workgroup holds a position's whole channel
 *      row (csrc/conv_halo_n.hpp: Cout 96 / 160; the norm sees the fp32 accumulators); on every other kernel choice the call is the plain
 *      convolution followed by yume_vae_rmsnorm_silu in place (the norm sees the bf16 image): the same function to bf16 rounding.
 *      YUME_CONV_FUSE_NORM=0 forces the second form.
 */
enum { YUME_CONV_EPI_ADD = 16, YUME_CONV_EPI_TSPLIT = 17, YUME_CONV_EPI_RMS_SILU = 18 };
int yume_conv3d_cl(const void* x, const void* cache, int64_t ldc, int64_t Tin, int64_t Hin, int64_t Win, int64_t Cin,
                   const void* W, int64_t ldw, const float* bias, int64_t Cout,
                   int kt, int kh, int kw, int st, int sh, int sw, int pt, int ph, int pw, int ups,
                   int64_t To, int64_t Ho, int64_t Wo, int epi, void* out, int64_t ldo,
                   const void* add, int64_t ldadd, const void* zero_page, void* stream);

/* ---- RMS_norm (+SiLU) over channels ---------------------------------------------------------------------
 * replaces: vae2_2.py:47-61 RMS_norm = F.normalize(x, dim=channel) * sqrt(C) * gamma (+ bias), followed by nn.SiLU
 *           in ResidualBlock (:204-208) and the heads (:560-561,676-677).
 *   y[m, c] = act( x[m, c] / max(||x[m, :]||_2, 1e-12) * sqrt(C) * gamma[c] + beta[c] ),  act = SiLU if silu != 0
 * x, y: bf16 [M, C] (ldx, ldy); gamma fp32 [C]; beta fp32 [C] or NULL. fp32 statistics. C % 8 == 0, C <= 4096.
 * y may be x (in place: every kernel form reads a row whole before it writes it). SiLU is x * rcp(1 + exp2(-x log2 e)) in the r6 forms
 * (1 ulp of fp32, below the bf16 rounding of y).
 */
int yume_vae_rmsnorm_silu(const void* x, int64_t ldx, int64_t M, int64_t C, const float* gamma, const float* beta,
                          int silu, void* y, int64_t ldy, void* stream);

/* ---- DupUp3D shortcut, added in place --------------------------------------------------------------------
 * replaces: vae2_2.py:376-418 DupUp3D + the `x_main + x_shortcut` of Up_ResidualBlock (:499-501).
 *   y[(t', h', w'), oc] += x[(t'+toff)/ft, h'/fs, w'/fs][ (oc*ft*fs*fs + a*fs*fs + b*fs + c) / repeats ]
 *   a = (t'+toff)%ft, b = h'%fs, c = w'%fs, repeats = Cout*ft*fs*fs/Cin; toff = ft-1 on the first chunk (the
 *   reference drops the first ft-1 duplicated frames there), else 0.
 * x bf16 [Tin,Hin,Win,Cin] (ldx); y bf16 [To, Hin*fs, Win*fs, Cout] (ldy), in/out.
 */
int yume_vae_dupup_add(const void* x, int64_t ldx, int64_t Tin, int64_t Hin, int64_t Win, int64_t Cin,
                       void* y, int64_t ldy, int64_t To, int64_t Cout, int ft, int fs, int toff, void* stream);

/* ---- AvgDown3D shortcut, added in place --------------------------------------------------------------------
 * replaces: vae2_2.py:322-373 AvgDown3D + the `x + avg_shortcut(x_copy)` of Down_ResidualBlock (:458).
 *   y[(t,h,w), oc] += mean_{g < G} x'[oc*G + g],  x'[ci*ft*fs*fs + a*fs*fs + b*fs + c] = x[(t*ft + a - padt, h*fs+b, w*fs+c), ci]
 *   G = Cin*ft*fs*fs/Cout; padt = (ft - Tin%ft)%ft zero frames in FRONT (frames with index < 0 contribute 0).
 */
int yume_vae_avgdown_add(const void* x, int64_t ldx, int64_t Tin, int64_t Hin, int64_t Win, int64_t Cin,
                         void* y, int64_t ldy, int64_t Cout, int ft, int fs, void* stream);

/* ---- row softmax for the single-head VAE attention -----------------------------------------------------------
 * replaces: the softmax inside F.scaled_dot_product_attention of AttentionBlock (vae2_2.py:272-276); the two
 *           matmuls around it run on yume_gemm_bf16.  P[r, :n] = softmax(scale * S[r, :n]) (bf16), P[r, n:ldp] = 0.
 */
int yume_softmax_rows(const float* S, int64_t lds, int64_t R, int64_t n, float scale, void* P, int64_t ldp, void* stream);

/* ---- layout conversion at the two ends of the VAE --------------------------------------------------------------
 * yume_vae_pack_input: fp32|bf16 [C, T, H, W] -> bf16 channels-last [T, H/ps, W/ps, Cpad] with
 *   v = x[c] * mul[c] + add[c] (mul/add fp32 [C] or NULL: the `z/scale[1] + scale[0]` of decode, vae2_2.py:833-838)
 *   and, for ps = 2, patchify "b c f (h q) (w r) -> b (c r q) f h w" (vae2_2.py:286-302); channels >= C*ps*ps are 0.
 * yume_vae_unpack_output: bf16 channels-last [T, H, W, ldx] (first Cv channels) -> fp32 [Cv/(ps*ps), T, H*ps, W*ps]
 *   with unpatchify (vae2_2.py:305-319), v = (x - sub[c]) * mul[c] (encode's `(mu - mean) * (1/std)`, :821-826)
 *   and clamp to [lo, hi] when lo < hi (decode's .clamp_(-1, 1), :1066).
 */
int yume_vae_pack_input(const void* x, int in_bf16, int64_t C, int64_t T, int64_t H, int64_t W, int ps,
                        const float* mul, const float* add, void* out, int64_t Cpad, void* stream);
int yume_vae_unpack_output(const void* x, int64_t ldx, int64_t T, int64_t H, int64_t W, int64_t Cv, int ps,
                           const float* sub, const float* mul, float lo, float hi, float* out, void* stream);
/* env YUME_VAE_LOG=1 (read once per process, like YUME_NORM_LOG): every kernel launch of yume_vae_rmsnorm_silu, yume_vae_dupup_add,
 * yume_vae_avgdown_add, yume_softmax_rows, yume_vae_pack_input and yume_vae_unpack_output prints one stderr line `[vae] <instance> k=v ...`:
 *   rms<LPR,NV> | rms_g<G,NVL,RI> | rms_flat<NVEC,NVL,RI,silu,beta>   M= C= ldx= ldy= silu= beta=
 *   dupup | dupup_lines<Q> | avgdown | avgdown_lines<RR>             Tin= Hin= Win= Cin= Cout= ft= fs= toff= ldx= ldy= lines= gx= gy=
 *   softmax_rows | softmax_rows_reg<NV>                              R= n= lds= ldp=
 *   pack<f32|bf16>                                                   C= T= H= W= ps= Cpad= affine= grid=
 *   unpack                                                           T= H= W= Cv= ps= ldx= affine= clamp= grid=
 * (avgdown has no toff: 0; the general shortcut kernels' grid is gx workgroups of a one-dimensional stride loop, gy = 1.) The routes:
 * YUME_VAE_NORM_G / YUME_VAE_NORM_FLAT (read once per process), YUME_VAE_SHORTCUT_LINES / YUME_VAE_SOFTMAX_REG (read per call).
 * tests/vae_op_cases.py holds one row per instance. */

/* ---- FP8 residual convolutions of the VAE (r19; functions added, no argument list changed: ABI 9) ----------------------------
 * The input of every ResidualBlock convolution is the output of an RMS_norm + SiLU launch, so the norm emits OCP MX e4m3 itself (bytes
 * + one E8M0 scale byte 2^(byte - 127) per position and 32 consecutive channels) and the convolution takes the scale bytes into the
 * scale operand of v_mfma_scale_f32_16x16x128_f8f6f4: a per-position scale does not factor out of a convolution, a block scale need not.
 *
 * yume_vae_rmsnorm_silu_mx (the producer): yume_vae_rmsnorm_silu(x, ldx, M, C, gamma, beta, silu, y, ldy = C) followed by an MX quantiser of
 *     the bf16 y, in one kernel and without y, bit for bit: per row and block of 32 channels amax = max |y|, e = the smallest integer with
 *     amax <= 448 * 2^e (the rule of YUME_EPI_MX_GELU; 0 for an all-zero block), e_out[m, c / 32] = e + 127, q[m, c] = e4m3_rne(clamp(y * 2^-e, +-448)).
 *     q u8 [M, C] (row stride ldq bytes), e_out u8 [M, C / 32] (row stride lde). The norm's kernel forms differ in their last bits
 *     (summation order, SiLU form); this call takes the form the norm takes for (C, ldx, ldy = C) and the same route switches.
 *     Checks (YUME_EINVAL): C % 32 == 0, C <= 4096, ldx % 8 == 0, ldx >= C, ldq % 8 == 0, ldq >= C, lde % 4 == 0, lde >= C / 32, x / q / gamma /
 *     beta 16-byte aligned, e_out 4-byte aligned. Bytes beyond C of a q row, scale bytes beyond C / 32 and rows beyond M are not written.
 *     YUME_VAE_LOG=1: one line `[vae] rms_mx <form> M= C= ldx= ldq= lde= silu= beta=`.
 * yume_conv3d_cl_f8mx (the consumer):
 *     out[(to,ho,wo), co] = bias[co] + sw[co] * sum_{dt,dh,dw} sum_b 2^(xe[pos+tap, b] - 127) * sum_{c in block b} xq[pos+tap, c] * Wq[co, tap*Cin + c]
 *     with tap = (dt*kh + dh)*kw + dw and the cache frames and zero padding of yume_conv3d_cl; fp32 sums walked (dt, channel tile of 128, dh, dw).
 *     xq u8 [Tin,Hin,Win,ldc], xe u8 [Tin,Hin,Win,lde]; cacheq / cachee: the last two input frames of the previous chunk in the same layouts,
 *     both NULL or both given; Wq u8 [Cout, ldw] e4m3, sw fp32 [Cout] (the weight's per-output-channel scale), bias fp32 [Cout] or NULL;
 *     zero_page >= 16 zero bytes. epi: YUME_EPI_BF16, YUME_EPI_F32, YUME_CONV_EPI_ADD (add bf16 [M, ldadd]).
 *     Accepted: stride 1, ups = 0, kt / kh / kw in {1, 3} with pt = kt - 1, ph = kh / 2, pw = kw / 2, Cin % 128 == 0 (anything else of these:
 *     YUME_EUNSUP); To = Tin, Ho = Hin, Wo = Win >= 1 (a tile of 256 positions never spans two frames; a frame smaller than a tile is legal),
 *     Cout % 4 == 0, ldc % 16 == 0, ldc >= Cin, lde % 4 == 0, lde >= Cin / 32, ldw % 16 == 0, ldw >= kt*kh*kw*Cin, ldo % 4 == 0, ldo >= Cout,
 *     ADD: add non-NULL, ldadd % 4 == 0, ldadd >= Cout; xq / cacheq / Wq / out / add / zero_page / sw / bias 16-byte aligned, xe / cachee 4-byte
 *     aligned; Hin*Win*ldc < 2^31 (YUME_EINVAL). Nothing is launched when a check fails. YUME_CONV_LOG=1: one line `[conv3d_cl] f8mx M= Cin= ...`.
 *     Accuracy: tests/conv_f8_cases.py bounds every element against fp64 on the very bytes the call receives. */
int yume_vae_rmsnorm_silu_mx(const void* x, int64_t ldx, int64_t M, int64_t C, const float* gamma, const float* beta,
                             int silu, void* q, int64_t ldq, void* e_out, int64_t lde, void* stream);
int yume_conv3d_cl_f8mx(const void* xq, const void* xe, const void* cacheq, const void* cachee, int64_t ldc, int64_t lde,
                        int64_t Tin, int64_t Hin, int64_t Win, int64_t Cin, const void* Wq, int64_t ldw, const float* sw,
                        const float* bias, int64_t Cout, int kt, int kh, int kw, int st, int sh, int sw_, int pt, int ph, int pw,
                        int ups, int64_t To, int64_t Ho, int64_t Wo, int epi, void* out, int64_t ldo,
                        const void* add, int64_t ldadd, const void* zero_page, void* stream);

/* ---- nearest-2x upsample + Conv2d 3x3 folded into four 2x2 convolutions (r21; a function added, no argument list changed: ABI 9) -----
 * replaces: the `nn.Upsample(2x, nearest-exact)` + `Conv2d(3x3, padding 1)` of an upsample Resample (vae2_2.py:73-171), which
 *           yume_conv3d_cl(ups = 1) runs with nine taps per output position. On a nearest-2x image those nine taps read 2 x 2 distinct input
 *           positions; with the taps that share a source summed at pack time the convolution is, per output parity (e_h, e_w), a 2x2 stride-1
 *           convolution on the input-resolution image: 4 taps instead of 9.
 *   out[t, 2a + e_h, 2b + e_w, co] = bias[co] + sum_{th, tw < 2} sum_ci x[t, a + th - (1 - e_h), b + tw - (1 - e_w), ci] * wf[2 e_h + e_w][co][(th*2 + tw)*Cin + ci]
 *   (input positions outside [0, Hin) x [0, Win) contribute 0); all four phases in one launch; fp32 sums walked (channel tile of 64, th, tw).
 * x bf16 [T, Hin, Win, ldc]; wf bf16 [4, Cout, ldw] — phase 2 e_h + e_w, K ordered (th, tw, ci), the sums of the 3x3 taps
 *   wf[e_h, e_w][co][th, tw, ci] = sum_{dh in S(e_h, th)} sum_{dw in S(e_w, tw)} W[co, ci, dh, dw], S(0, .) = ({0}, {1, 2}), S(1, .) = ({0, 1}, {2}),
 *   rounded once to bf16 (yume_amd.vae.fold_upsample_weight); bias fp32 [Cout] or NULL; out bf16 [T, 2 Hin, 2 Win, ldo].
 * Not bit-equal to yume_conv3d_cl(ups = 1) on W: the summed weights are rounded once more (rel-L2 1.6-1.8e-3 per convolution).
 * Any Hin * Win (a tile of 256 input positions never spans two frames or phases; a frame smaller than a tile is legal) and any T.
 * Columns >= Cout of an out row are not written. ldo % 8 == 0: whole 16-byte stores through an LDS image, else guarded 8-byte stores.
 * Checks (YUME_EINVAL, the text names the argument, nothing is launched): x / wf / out non-NULL; T, Hin, Win, Cin, Cout > 0;
 *   Cin % 64 == 0; Cout % 4 == 0; ldc % 8 == 0, ldc >= Cin; ldw % 8 == 0, ldw >= 4 Cin; ldo % 4 == 0, ldo >= Cout; x / wf / out / bias 16-byte
 *   aligned; Hin * Win < 2^28; T * 4 * ceil(Hin Win / 256) * ceil(Cout / 256) < 2^31; one input frame inside a buffer descriptor's range
 *   ((Hin Win + 2 Win + 2) * ldc * 2 < 0x7fffff00); 255 * ldw * 2 + 128 < 2^32.
 * YUME_CONV_LOG=1: one line `[conv3d_cl] w4fold T= Hin= Win= Cin= Cout= tiles=` per launch. YUME_CONV_FOLD_ORDER=1 (read per call,
 *   A/B runs): tiles walk (frame, tile, phase) instead of (frame, phase, tile); the same bits.
 * Accuracy: tests/conv_upfold_cases.py bounds every element against fp64 on the very bytes the call receives. */
int yume_conv_up2_fold(const void* x, int64_t ldc, int64_t T, int64_t Hin, int64_t Win, int64_t Cin,
                       const void* wf, int64_t ldw, const float* bias, int64_t Cout,
                       void* out, int64_t ldo, void* stream);

/* ---- post-decode frame conversion ---------------------------------------------------------------
 * replaces: fastvideo/sample/sample_5b.py:491-500 save_video -> diffusers==0.32.0 VideoProcessor.postprocess_video
 *           (denormalize `(x * 0.5 + 0.5).clamp(0, 1)`, then numpy_to_pil `(x * 255).round().astype("uint8")`) — the
 *           reference does this on the host after a device->host copy of the fp32 video; here it runs on the decoder's
 *           output in HBM and 1 byte per sample crosses PCIe instead of 4.
 * video: fp32 [C, T, H, W] (C <= 4, T*H*W % 4 == 0) -> out: uint8 [T, H, W, C]. Bit-exact (fp32, round half to even).
 */
int yume_frames_u8(const float* video, int64_t C, int64_t T, int64_t H, int64_t W, void* out, void* stream);
/* The web app's own variant of the same step (webapp_single_gpu.py:117-121 `_postprocess_video`, in-tree code):
 *   ((video.clamp(-1, 1) + 1) / 2 * 255).byte()  — the same affine map, but TRUNCATED to uint8 instead of rounded. Same layouts. */
int yume_frames_u8_trunc(const float* video, int64_t C, int64_t T, int64_t H, int64_t W, void* out, void* stream);

/* ======================================================================================================
 * umT5-XXL text encoder (the step before the path; wan/modules/t5.py:440-513 T5EncoderModel,
 * :262-291 T5Encoder, :143-178 T5SelfAttention). It runs on the DiT's GEMM kernels plus four small pieces:
 *   yume_rmsnorm_f32       T5LayerNorm (t5.py:53-67): out bf16 = x * rsqrt(mean(x^2) + eps) * w, x fp32 [T, C]
 *   YUME_EPI_BF16_GEGLU    T5FeedForward's fc1(x) * gelu_tanh(gate(x)) (t5.py:116-141) in ONE GEMM: W = the rows of gate
 *                          and fc1 interleaved (row 2j = gate_j, row 2j+1 = fc1_j), N = 2*dim_ffn, out bf16 [M, N/2]
 *   yume_gemm_bf16_batched the per-head q.k^T and P.v products (t5.py:105-109), `batch` launches per call
 *   yume_softmax_bias_rows P[h,i,:n] = softmax_j(S[h,i,j] + bias[h, j-i+n-1]) (T5 does not scale; bias = the layer's
 *                          relative-position embedding, t5.py:215-259), P[h,i,n:ldp] = 0
 * Padding tokens are not computed at all: their keys are masked to exactly zero weight in the reference (finfo.min bias)
 * and their rows are dropped by T5EncoderModel.__call__ (`u[:v]`), so running on the valid tokens only is identical.
 */
int yume_rmsnorm_f32(const float* x, int64_t ldx, int64_t T, int64_t C, float eps, const float* w, void* out, int64_t ldo,
                     void* stream);
int yume_gemm_bf16_batched(const void* A, int64_t lda, int64_t strideA, const void* W, int64_t ldw, int64_t strideW,
                           int64_t M, int64_t N, int64_t K, int epi, void* out, int64_t ldo, int64_t strideO,
                           int64_t batch, int variant, void* stream);
int yume_softmax_bias_rows(const float* S, int64_t lds, int64_t strideS, int64_t H, int64_t n, const float* bias,
                           int64_t ldb, void* P, int64_t ldp, int64_t strideP, void* stream);
/* split-K for the encoders' small-M GEMMs (M <= 512 tokens against tens of MB of weights — every nn.Linear of t5.py / clip.py):
 * K is cut into `splits` slices computed side by side on the 128x128 kernel (fp32 partials in `workspace`,
 * yume_gemm_splitk_workspace_bytes = splits*M*N*4, caller-owned), then summed in a fixed order with bias + epilogue
 * (YUME_EPI_F32 / RESID without gate / BF16 / BF16_GELU / BF16_GELU_ERF / BF16_GEGLU). K % (splits*64) == 0, N % 8 == 0. */
int64_t yume_gemm_splitk_workspace_bytes(int64_t M, int64_t N, int splits);
int yume_gemm_bf16_splitk(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, int64_t M, int64_t N,
                          int64_t K, int epi, void* out, int64_t ldo, int splits, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YUME_HIP_H */
