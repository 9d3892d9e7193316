"""The case table of the dense GEMM's routes, epilogues and operand layouts, their fp64 reference and the per-element error bound (no test
functions in here).

`yume_gemm_bf16_ws` stands in front of three kernels (gemm128_kernel, the 8-wave gemm256_kernel, the one-wave-per-SIMD gemm_w4_kernel) and
a host-side row split into two launches, each kernel with its own code for every epilogue; `yume_gemm_bf16_batched` and
`yume_gemm_bf16_splitk` (+ splitk_reduce_kernel) stand beside it. tests/test_gemm_routes_gpu.py runs one call per CASES row and holds EVERY
output element to `bound()` against `reference()`, with a guard value around every output; tests/test_gemm_cases_cpu.py proves the table,
the route mirror, the reference and the bound on the host. The split-K tail of gemm_w4_kernel (`w4+sk`) has its own file
(tests/test_gemm_splitk_tail_gpu.py); here it is only asserted to be off.

Operands are bf16-exact (A ~ N(0, 1), W ~ N(0, 1/K)), so a correct kernel errs by the order of its fp32 sum, the fp32 operations of its
epilogue and the one rounding of a bf16 output. With y = acc + bias in fp64, Q = sum_k (a_mk w_nk)^2 and

    e_y = 2^-14 sqrt(Q) + 2^-22 (|y| + |bias|)          (the fp32 sum in any order: conv_cases.py; bias joins in fp32)

    BF16, SPLITT    2^-8 |ref| + e_y                                      ref = y
    F32             e_y
    RESID           |gate| e_y + 2^-22 (|ref| + |x|)                      ref = x + gate * y (gate = 1 without one), all fp32
    GELU, GELU_ERF  2^-8 |ref| + GELU_SLOPE e_y + allowance(y, ref)       ref = gelu(y); |gelu'| <= 1.13 for both forms
    GEGLU           2^-8 |ref| + |v| dg + (|gelu(g)| + dg) e_v + 2^-23 |ref|,  dg = GELU_SLOPE e_g + allowance(g)     ref = v * gelu_tanh(g)

2^-8 |ref| is half a bf16 ulp of the fp64 value of the (activated) output. The activation allowances are derived from the code of
csrc/common.hpp and the stated accuracy of the instructions, not fitted to a kernel (profiles/r13_gemm_routes.md has the derivation):

    gelu_tanh   C_TANH 2^-23 (1 + |x|^3) |ref| + ACT_FLOOR         x * rcp(1 + exp2(x (c1 x^2 + c0))): v_exp_f32 and v_rcp_f32 at 1 ulp
    gelu_erf    2^-23 (C_ERF |x| + 2 |ref|)                         0.5 x (1 + erff(x / sqrt 2)): 1 + erf cancels for x < 0, so the
                                                                    erff error (4 ulp of a value <= 1) is ABSOLUTE in 1 + erf

    python tests/gemm_cases.py --routes        one call per case, `CASE <name>` on stderr before each (YUME_GEMM_LOG=1 names the kernels)
"""
import ctypes
import os
import sys
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_sk_plan as skp  # noqa: E402

EPI_BF16, EPI_GELU, EPI_F32, EPI_RESID, EPI_SPLITT, EPI_GELU_ERF, EPI_GEGLU = 0, 1, 2, 3, 4, 5, 6          # include/yume_hip.h
EPI_NAMES = {0: "bf16", 1: "gelu", 2: "f32", 3: "resid", 4: "splitt", 5: "gelu_erf", 6: "geglu"}
BF16_OUT = (EPI_BF16, EPI_GELU, EPI_SPLITT, EPI_GELU_ERF, EPI_GEGLU)
GUARD = 7.0
BK = 64

# ---- the bound's constants
GELU_SLOPE = 1.13            # max |gelu'|: 1.1290 (erf form, at x = 1.41), 1.1292 (tanh form)
C_TANH = 7.0                 # derived 6.43 (profiles/r13_gemm_routes.md)
C_ERF = 2.0                  # derived 1.74
ACT_FLOOR = 2.0 ** -120      # exp2 overflows for x < -9.6: the kernel stores -0 where the value is below the fp32 normals

# api: "ws" (yume_gemm_bf16_ws), "batched" (yume_gemm_bf16_batched, form = "scores" / "values" / "pattern"), "splitk" (yume_gemm_bf16_splitk)
# route: the kernels the YUME_GEMM_LOG lines of the call must name, in order, at 256 CUs. bias: a bias vector. gate: None (RESID: x += y),
# "one" (one gate row), "inter" (row_idx = m % 3), "seg" (row_idx in segments, boundaries = seg). slices: A and W are the two column
# halves of ONE [rows, 2K] buffer (lda = ldw = 2K, W's pointer K elements in). ldo_x: ldo = stored columns + ldo_x. row0: the call writes
# rows row0.. of a taller buffer. ldt_x: ldt = M rounded up to 8, + ldt_x. pattern: A identity-like, W[n, k] of both indices, bit-exact.
Case = namedtuple("Case", "name api M N K epi variant route bias gate seg slices ldo_x row0 n_split ldt_x splits pattern form",
                  defaults=(False, None, (), False, 0, 0, 0, 0, 0, False, None))


def _c(name, M, N, K, epi, variant, route, **kw):
    return Case(name, kw.pop("api", "ws"), M, N, K, epi, variant, route, **kw)


G128, G256, W4 = "g128", "g256", "w4"
CASES = [
    # ---- gemm128_kernel (variant 1)
    _c("g128_pattern", 256, 256, 256, EPI_F32, 1, G128, pattern=True),
    _c("g128_m1_bf16", 1, 128, 64, EPI_BF16, 1, G128, bias=True),                              # one row, one K tile
    _c("g128_m129_n132_bf16_nobias", 129, 132, 128, EPI_BF16, 1, G128, ldo_x=4),               # two ragged M tiles, N % 8 = 4, ldo = N + 4
    _c("g128_slices_row1_bf16", 129, 132, 128, EPI_BF16, 1, G128, bias=True, slices=True, ldo_x=4, row0=2),      # ldo = 136; rows 2..
    _c("g128_gelu", 129, 260, 64, EPI_GELU, 1, G128, bias=True, ldo_x=8),
    _c("g128_gelu_nobias", 130, 256, 128, EPI_GELU, 1, G128, ldo_x=4),
    _c("g128_gelu_erf", 129, 260, 64, EPI_GELU_ERF, 1, G128, bias=True, ldo_x=4),
    _c("g128_gelu_erf_nobias", 130, 256, 128, EPI_GELU_ERF, 1, G128, slices=True),
    _c("g128_f32", 129, 132, 192, EPI_F32, 1, G128, bias=True, ldo_x=4, row0=1),
    _c("g128_f32_nobias", 1, 132, 64, EPI_F32, 1, G128, ldo_x=8),
    _c("g128_resid_nogate", 129, 132, 128, EPI_RESID, 1, G128, bias=True, ldo_x=4),
    _c("g128_resid_one", 129, 132, 64, EPI_RESID, 1, G128, gate="one", ldo_x=8, row0=1),
    _c("g128_resid_inter", 130, 256, 128, EPI_RESID, 1, G128, bias=True, gate="inter", slices=True),
    _c("g128_resid_seg", 200, 132, 128, EPI_RESID, 1, G128, bias=True, gate="seg", seg=(30, 161), ldo_x=4),   # 30, 161: inside 64-row passes
    _c("g128_splitt", 301, 384, 128, EPI_SPLITT, 1, G128, bias=True, n_split=128, ldt_x=8, ldo_x=8),          # M % 8 = 5, ldt = 312
    _c("g128_splitt_nobias", 129, 256, 64, EPI_SPLITT, 1, G128, n_split=128, ldt_x=8, ldo_x=4, row0=2),
    _c("g128_splitt_v2_falls_back", 301, 640, 128, EPI_SPLITT, 2, G128, bias=True, n_split=384, ldt_x=0),      # n_split % 256 != 0: no 256 kernel
    # ---- gemm256_kernel (variant 2; variant 3 at K = 128, where w4_applies refuses)
    _c("g256_pattern", 256, 256, 256, EPI_F32, 2, G256, pattern=True),
    _c("g256_m1_bf16", 1, 128, 64, EPI_BF16, 2, G256, bias=True),                              # N edge tile: the guarded store_row4 path
    _c("g256_bf16_lds", 257, 512, 128, EPI_BF16, 3, G256, bias=True, ldo_x=8, row0=1),         # variant 3 at K = 128; the LDS image path, ragged M
    _c("g256_bf16_ldo4_nobias", 129, 260, 64, EPI_BF16, 2, G256, ldo_x=4, slices=True),        # ldo % 8 != 0: whole tile from the accumulators
    _c("g256_bf16_full_ldo4", 256, 256, 64, EPI_BF16, 2, G256, bias=True, ldo_x=4),            # epilogue_rows_full with bf16
    _c("g256_gelu", 257, 260, 128, EPI_GELU, 3, G256, bias=True, ldo_x=4),
    _c("g256_gelu_nobias", 256, 256, 64, EPI_GELU, 2, G256, ldo_x=8),
    _c("g256_gelu_erf", 257, 260, 128, EPI_GELU_ERF, 2, G256, bias=True, ldo_x=8),
    _c("g256_gelu_erf_nobias", 256, 256, 64, EPI_GELU_ERF, 3, G256),
    _c("g256_f32", 257, 260, 128, EPI_F32, 2, G256, bias=True, ldo_x=4, row0=1),
    _c("g256_f32_nobias_full", 256, 512, 64, EPI_F32, 2, G256, slices=True),
    _c("g256_resid_nogate", 257, 260, 128, EPI_RESID, 3, G256, bias=True, ldo_x=4),
    _c("g256_resid_one_full", 512, 256, 64, EPI_RESID, 2, G256, gate="one", ldo_x=8),
    _c("g256_resid_inter", 300, 256, 128, EPI_RESID, 2, G256, bias=True, gate="inter", row0=1),
    _c("g256_resid_seg", 512, 260, 64, EPI_RESID, 2, G256, bias=True, gate="seg", seg=(100, 300), ldo_x=4),
    _c("g256_splitt", 301, 768, 128, EPI_SPLITT, 2, G256, bias=True, n_split=256, ldt_x=8, ldo_x=8),           # SWAP and !SWAP tiles, store_col4
    _c("g256_splitt_ldt4", 301, 512, 64, EPI_SPLITT, 2, G256, n_split=256, ldt_x=4),           # ldt % 8 = 4
    _c("g256_geglu", 257, 776, 128, EPI_GEGLU, 2, G256, ldo_x=8),                              # N / 2 = 388: ragged against the tile
    _c("g256_geglu_v0", 256, 512, 64, EPI_GEGLU, 0, G256, ldo_x=4),                            # GEGLU runs the 256 kernel under every variant
    _c("g256_group_tail", 2305, 256, 64, EPI_BF16, 2, G256, bias=True),                        # tiles_m = 10: a short last group, 10 % 8 != 0
    # ---- gemm_w4_kernel (variant 3, K = 192 = exactly three K tiles, and K = 256)
    _c("w4_pattern", 256, 256, 256, EPI_F32, 3, W4, pattern=True),
    _c("w4_bf16", 257, 512, 192, EPI_BF16, 3, W4, bias=True, ldo_x=8, row0=1),                 # one row in the second M tile; the image path
    _c("w4_bf16_ldo4", 257, 256, 192, EPI_BF16, 3, W4, bias=True, ldo_x=4),                    # ldo % 8 != 0: the guarded store_row4 path
    _c("w4_bf16_n260_chunk", 300, 260, 256, EPI_BF16, 3, W4, bias=True, ldo_x=4, slices=True), # N % 8 = 4, ldo = 264: ragged last 16-byte chunk
    _c("w4_bf16_nobias_m1", 1, 256, 192, EPI_BF16, 3, W4),
    _c("w4_gelu", 257, 260, 192, EPI_GELU, 3, W4, bias=True, ldo_x=4),
    _c("w4_gelu_nobias", 256, 256, 256, EPI_GELU, 3, W4, ldo_x=4),
    _c("w4_gelu_erf", 300, 516, 192, EPI_GELU_ERF, 3, W4, bias=True, ldo_x=4),
    _c("w4_gelu_erf_nobias", 257, 256, 256, EPI_GELU_ERF, 3, W4),
    _c("w4_f32", 257, 260, 192, EPI_F32, 3, W4, bias=True, ldo_x=4, row0=1),
    _c("w4_f32_nobias", 256, 256, 256, EPI_F32, 3, W4, slices=True),
    _c("w4_resid_nogate", 257, 256, 192, EPI_RESID, 3, W4, bias=True, ldo_x=4),
    _c("w4_resid_one_n260", 300, 260, 192, EPI_RESID, 3, W4, bias=True, gate="one"),           # N edge tile: RESID leaves the whole-column path
    _c("w4_resid_inter_n516", 257, 516, 256, EPI_RESID, 3, W4, gate="inter", ldo_x=4),
    _c("w4_resid_seg_ragged_last", 300, 256, 192, EPI_RESID, 3, W4, bias=True, gate="seg", seg=(100,)),   # the ragged last M tile shares one gate row
    _c("w4_resid_seg_boundary_in_tile", 600, 512, 192, EPI_RESID, 3, W4, bias=True, gate="seg", seg=(300, 530), row0=1),
    _c("w4_splitt", 300, 768, 192, EPI_SPLITT, 3, W4, bias=True, n_split=256, ldt_x=8, ldo_x=8),           # SWAP and !SWAP tiles; ldt = 312, M % 8 = 4
    _c("w4_splitt_nobias", 257, 512, 256, EPI_SPLITT, 3, W4, n_split=256, ldt_x=0, row0=1),
    _c("w4_splitt_ldt4_falls_back", 301, 512, 192, EPI_SPLITT, 3, G256, bias=True, n_split=256, ldt_x=4),   # ldt % 8 != 0: the 8-wave kernel
    # ---- variant 0, each to the route the mirror names
    _c("v0_below_fill", 300, 256, 192, EPI_BF16, 0, G128, bias=True),
    _c("v0_w4_192_tiles", 2900, 4096, 192, EPI_BF16, 0, W4, bias=True),
    _c("v0_w4_n4004", 2900, 4004, 192, EPI_GELU, 0, W4, bias=True, ldo_x=4),                   # ldo = 4008: the image path's ragged chunk
    _c("v0_g256_k128", 2900, 4096, 128, EPI_BF16, 0, G256, bias=True),
    _c("v0_split_f32", 4231, 4096, 192, EPI_F32, 0, "w4 g128", bias=True),                     # 272 tiles: 4096 rows + a remainder of 135
    _c("v0_split_resid_seg", 4231, 4096, 192, EPI_RESID, 0, "w4 g128", bias=True, gate="seg", seg=(2000, 4150)),
    _c("v0_split_splitt", 4231, 4096, 192, EPI_SPLITT, 0, "w4 g128", bias=True, n_split=2048, ldt_x=8),     # the remainder's outT + M_main
    _c("v0_split_gelu", 4231, 4096, 192, EPI_GELU, 0, "w4 g128", ldo_x=8),
    _c("v0_split_k128", 4231, 4096, 128, EPI_BF16, 0, "g256 g128", bias=True),
    _c("v0_padded_work_refused", 257, 24324, 64, EPI_F32, 0, G128, bias=True),                  # 192 tiles of 256, but 614 > 573 tiles of 128
    # ---- yume_gemm_bf16_batched in the two encoder forms of yume_amd/t5.py (H = 3, n = 77, npad = 128, hd = 64)
    _c("batched_pattern", 128, 128, 128, EPI_F32, 0, "batched", api="batched", form="pattern"),
    _c("batched_scores", 77, 128, 64, EPI_F32, 0, "batched", api="batched", form="scores"),
    _c("batched_values", 77, 64, 128, EPI_BF16, 0, "batched", api="batched", form="values"),
    # ---- yume_gemm_bf16_splitk on the caller's workspace (pre-filled with NaN)
    _c("splitk_pattern", 128, 256, 256, EPI_F32, 0, "batched splitk_reduce", api="splitk", splits=2, pattern=True),
    _c("splitk_s2_f32", 3, 256, 128, EPI_F32, 0, "batched splitk_reduce", api="splitk", splits=2, bias=True, ldo_x=4),
    _c("splitk_s4_bf16", 77, 264, 256, EPI_BF16, 0, "batched splitk_reduce", api="splitk", splits=4, bias=True, ldo_x=8),
    _c("splitk_s16_resid", 77, 256, 1024, EPI_RESID, 0, "batched splitk_reduce", api="splitk", splits=16, bias=True, ldo_x=4),
    _c("splitk_s2_gelu", 77, 264, 128, EPI_GELU, 0, "batched splitk_reduce", api="splitk", splits=2, bias=True, ldo_x=4),
    _c("splitk_s4_gelu_erf", 77, 256, 256, EPI_GELU_ERF, 0, "batched splitk_reduce", api="splitk", splits=4, ldo_x=8),
    _c("splitk_s16_geglu", 77, 264, 1024, EPI_GEGLU, 0, "batched splitk_reduce", api="splitk", splits=16, ldo_x=4),
    _c("splitk_s2_geglu_m3", 3, 256, 128, EPI_GEGLU, 0, "batched splitk_reduce", api="splitk", splits=2, ldo_x=8),
    _c("splitk_s4_resid_m3", 3, 264, 256, EPI_RESID, 0, "batched splitk_reduce", api="splitk", splits=4),
    _c("splitk_s16_bf16_m3", 3, 256, 1024, EPI_BF16, 0, "batched splitk_reduce", api="splitk", splits=16, ldo_x=4),
]
ROUTES = ("g128", "g256", "w4", "w4 g128", "g256 g128", "batched", "batched splitk_reduce")
T5_H, T5_N, T5_NPAD, T5_HD = 3, 77, 128, 64


# ------------------------------------------------------------------------------------------------ geometry of a row
def ceil8(v):
    return (v + 7) // 8 * 8


def out_cols(c):
    """columns of the row-major output the call stores"""
    return c.N // 2 if c.epi == EPI_GEGLU else c.n_split if c.epi == EPI_SPLITT else c.N


def strides(c):
    """(lda, ldw, ldo, ldt) as handed to the call"""
    if c.api == "batched":
        H, hd, npad = T5_H, T5_HD, T5_NPAD
        if c.form == "scores":
            return 2 * H * hd, 2 * H * hd, npad, 0
        if c.form == "values":
            return npad, npad, H * hd, 0
        return c.K, c.K, c.N, 0
    ld = 2 * c.K if c.slices else c.K
    return ld, ld, out_cols(c) + c.ldo_x, (ceil8(c.M) + c.ldt_x) if c.epi == EPI_SPLITT else 0


def out_elem_bytes(c):
    return 4 if c.epi in (EPI_F32, EPI_RESID) else 2


# ------------------------------------------------------------------------------------------------ the dispatcher's mirror
def use_256(M, N, variant, split_ok):
    """gemm_core.hpp use_256 (worth = 1.25)"""
    if variant == 1 or not split_ok:
        return False
    if variant == 2:
        return True
    return skp.use_256(M, N)


def w4_applies(K, lda, ldw, epi):
    """gemm_w4.hpp w4_applies"""
    return skp.w4_applies(K, lda, ldw) and epi in (EPI_BF16, EPI_GELU, EPI_GELU_ERF, EPI_F32, EPI_RESID, EPI_SPLITT)


def row_split(M, N):
    """the host-side row split of variant 0 -> (M_main, remainder rows) or None (gemm_bf16.hip)"""
    tn, tm = (N + 255) // 256, (M + 255) // 256
    T = tm * tn
    R = T % 256
    full = T - R
    m_main = full // tn
    rem = M - m_main * 256
    if R > 0 and R <= 96 and full >= 256 and m_main >= 1 and 0 < rem <= 1024:
        return m_main * 256, rem
    return None


def tail_plan(c, ncu=256, workspace=False):
    """the split-K tail's plan for the call, or None: it needs the automatic variant, a workspace, the w4 route and gemm_sk_plan's consent"""
    lda, ldw, _, ldt = strides(c)
    split_ok = c.epi != EPI_SPLITT or c.n_split % 256 == 0
    if not (c.api == "ws" and c.variant == 0 and workspace and c.epi != EPI_GEGLU and use_256(c.M, c.N, 0, split_ok)
            and w4_applies(c.K, lda, ldw, c.epi) and (c.epi != EPI_SPLITT or ldt % 8 == 0)):
        return None
    return skp.plan(c.M, c.N, c.K, ncu)[0]


def _route_ws(M, N, K, epi, variant, lda, ldw, ldt, n_split, sk):
    split_ok = epi != EPI_SPLITT or n_split % 256 == 0
    if not sk and variant == 0 and epi != EPI_GEGLU and use_256(M, N, 0, split_ok):
        rs = row_split(M, N)
        if rs is not None:
            return (_route_ws(rs[0], N, K, epi, 3, lda, ldw, ldt, n_split, False) +
                    _route_ws(rs[1], N, K, epi, 1, lda, ldw, ldt, n_split, False))
    if epi == EPI_GEGLU:
        return ("g256",)
    big = use_256(M, N, 2 if variant == 3 else variant, split_ok)
    w4 = (variant == 3 or (variant == 0 and big)) and split_ok and w4_applies(K, lda, ldw, epi) and (epi != EPI_SPLITT or ldt % 8 == 0)
    return ("w4+sk" if sk else "w4",) if w4 else ("g256",) if big else ("g128",)


def route(c, ncu=256, workspace=False):
    """the kernels the call launches, in order, as YUME_GEMM_LOG names them (run_case hands over no workspace)"""
    if c.api == "batched":
        return ("batched",)
    if c.api == "splitk":
        return ("batched", "splitk_reduce")
    lda, ldw, _, ldt = strides(c)
    return _route_ws(c.M, c.N, c.K, c.epi, c.variant, lda, ldw, ldt, c.n_split, tail_plan(c, ncu, workspace) is not None)


def w4_branches(c):
    """the branches of w4_epilogue (gemm_w4.hpp) the tiles of a call take, restated from its conditions: {"T" (the K-major V^T image),
    "image", "image_ragged_chunk" (w4_store_image: col_left < 8), "resid_cols" (the whole-column RESID path), "resid_same_row_ragged_m" (...
    where the 128 rows of a wave share a gate row in a tile with ragged M), "row4" (the guarded store_row4 path), "row4_bf16_ldo",
    "row4_resid_n_edge"}"""
    seen = set()
    calls = []
    r = route(c)
    if c.api != "ws":
        return seen
    if r == ("w4",):
        calls.append((0, c.M))
    elif r[0] == "w4":
        calls.append((0, row_split(c.M, c.N)[0]))
    _, _, ldo, ldt = strides(c)
    idx = row_index(c)
    for first, M in calls:
        for m0 in range(0, M, 256):
            for n0 in range(0, c.N, 256):
                if c.epi == EPI_SPLITT and n0 >= c.n_split:
                    seen.add("T")
                    if min(256, M - m0) % 8:
                        seen.add("T_ragged_chunk")
                elif c.epi in (EPI_BF16, EPI_GELU, EPI_GELU_ERF, EPI_SPLITT) and ldo % 8 == 0:
                    seen.add("image")
                    cols = min(256, c.N - n0)
                    if cols < 256 and cols % 8:
                        seen.add("image_ragged_chunk")
                elif c.epi == EPI_RESID and n0 + 256 <= c.N:
                    seen.add("resid_cols")
                    if m0 + 256 > M and idx is not None:
                        for wr in (0, 1):                         # the rows of a wave, clamped to the matrix's last row
                            rows = [min(first + m0 + wr * 128 + i, first + M - 1) for i in range(128)]
                            if len({int(idx[r_]) for r_ in rows}) == 1 and m0 + wr * 128 < M:
                                seen.add("resid_same_row_ragged_m")
                else:
                    seen.add("row4")
                    if c.epi in (EPI_BF16, EPI_GELU, EPI_GELU_ERF, EPI_SPLITT):
                        seen.add("row4_bf16_ldo")
                    if c.epi == EPI_RESID:
                        seen.add("row4_resid_n_edge")
    return seen


# ------------------------------------------------------------------------------------------------ operands
def _bf16_exact(t):
    return t.bfloat16().float()


def row_index(c):
    """int32 [M] gate row of every token, or None"""
    if c.gate == "inter":
        return (torch.arange(c.M) % 3).to(torch.int32)
    if c.gate == "seg":
        idx = torch.zeros(c.M, dtype=torch.int32)
        for b in c.seg:
            idx[b:] += 1
        return idx
    return None


def pattern_w(N, K):
    return _bf16_exact((torch.arange(N).view(N, 1) * 3 + torch.arange(K).view(1, K) % 7).float() / 64)


def make_case(c, device="cpu"):
    """seeded operands, drawn on the CPU generator. Host side (fp32, bf16-exact): "A" [.., M, K], "W" [.., N, K] (a leading batch dim for
    the batched forms), "bias" [N], "x" [M, N] (RESID), "gate" [rows, N], "idx"; "store" = the flat bf16-exact storage A and W are views
    of where they share one (with "a_view" / "w_view" = (offset, strides) into it). Under "dev" what the call takes on `device`."""
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.encode()))
    M, N, K = c.M, c.N, c.K
    ops = {"bias": None, "x": None, "gate": None, "idx": row_index(c), "store": None}
    dev = {}
    if c.api == "batched" and c.form in ("scores", "values"):
        H, n, npad, hd = T5_H, T5_N, T5_NPAD, T5_HD
        if c.form == "scores":
            # qk [npad, 2 * H * hd]: q of head h in columns h * hd .., k of head h in columns H * hd + h * hd ..; rows n.. of q are padding
            store = _bf16_exact(torch.randn(npad, 2 * H * hd, generator=g) * torch.cat([torch.ones(H * hd), torch.full((H * hd,), hd ** -0.5)]))
            ops["a_view"] = (0, (hd, 2 * H * hd, 1), (H, n, hd))
            ops["w_view"] = (H * hd, (hd, 2 * H * hd, 1), (H, npad, hd))
        else:
            # P [H, n, npad] and the K-major V^T [H * hd, npad] behind it in one storage
            store = torch.cat([_bf16_exact(torch.randn(H * n * npad, generator=g)), _bf16_exact(torch.randn(H * hd * npad, generator=g) * npad ** -0.5)])
            ops["a_view"] = (0, (n * npad, npad, 1), (H, n, npad))
            ops["w_view"] = (H * n * npad, (hd * npad, npad, 1), (H, hd, npad))
        store = store.reshape(-1)
        ops["store"] = store
        ops["A"] = torch.as_strided(store, ops["a_view"][2], ops["a_view"][1], ops["a_view"][0])
        ops["W"] = torch.as_strided(store, ops["w_view"][2], ops["w_view"][1], ops["w_view"][0])
        dev["store"] = store.to(torch.bfloat16).to(device)
    else:
        if c.pattern or c.form == "pattern":
            A, W = torch.eye(M, K), pattern_w(N, K)
        else:
            A, W = _bf16_exact(torch.randn(M, K, generator=g)), _bf16_exact(torch.randn(N, K, generator=g) * K ** -0.5)
        if c.slices:
            rows = max(M, N)
            store = _bf16_exact(torch.randn(rows, 2 * K, generator=g))          # what lies beside and below the operands is not zero
            store[:M, :K] = A
            store[:N, K:] = W
            store = store.reshape(-1)
            ops["store"] = store
            ops["a_view"] = (0, (2 * K, 1), (M, K))
            ops["w_view"] = (K, (2 * K, 1), (N, K))
            A = torch.as_strided(store, (M, K), (2 * K, 1), 0)
            W = torch.as_strided(store, (N, K), (2 * K, 1), K)
            dev["store"] = store.to(torch.bfloat16).to(device)
        else:
            dev["A"], dev["W"] = A.to(torch.bfloat16).to(device), W.to(torch.bfloat16).to(device)
        ops["A"], ops["W"] = A, W
    if c.bias:
        ops["bias"] = torch.randn(N, generator=g)
        dev["bias"] = ops["bias"].to(device)
    if c.epi == EPI_RESID:
        ops["x"] = torch.randn(M, N, generator=g)
        dev["x"] = ops["x"].to(device)
        if c.gate is not None:
            rows = 1 if c.gate == "one" else int(ops["idx"].max()) + 1
            tab = torch.randn(rows, 6, N, generator=g)                           # the modulation table of the blocks: the gate is its row 2
            ops["gate"] = tab[:, 2]
            dev["tab"] = tab.to(device)
            if ops["idx"] is not None:
                dev["idx"] = ops["idx"].to(device)
    ops["dev"] = dev
    return ops


def operand_view(ops, which, ld_err=0):
    """the operand read again from the flat storage, its row stride off by ld_err elements (a corruption the bound must flag)"""
    off, st, shape = ops[which + "_view"]
    st = list(st)
    st[-2] += ld_err
    need = off + sum((n - 1) * s for n, s in zip(shape, st)) + 1
    store = ops["store"]
    if need > store.numel():
        store = torch.cat([store, torch.zeros(need - store.numel())])
    return torch.as_strided(store, shape, st, off)


# ------------------------------------------------------------------------------------------------ reference and bound
def gelu(y, epi):
    """torch.nn.GELU (tanh form for EPI_GELU / EPI_GEGLU) in forms without cancellation in the negative tail: 0.5 x (1 + tanh u) =
    x / (1 + exp(-2 u)), 0.5 x (1 + erf(x / sqrt 2)) = 0.5 x erfc(-x / sqrt 2) (torch's own fp64 GELU returns -0 below x = -7.15, where
    the value is -4e-16)"""
    if epi in (EPI_GELU, EPI_GEGLU):
        return y / (1 + torch.exp(-2 * 0.7978845608028654 * (y + 0.044715 * y * y * y)))
    return 0.5 * y * torch.special.erfc(-y * 0.7071067811865476)


def reference(c, ops, device="cpu", dtype=torch.float64, A=None, W=None, idx=None, check_rows=True):
    """the call in `dtype` on `device`: "y" = A W^T + bias, "Q" = sum_k (a_mk w_nk)^2 (one more product, of the squared operands), "ref" =
    behind the epilogue, in the layout of `gather()`: [M, N] ([M, N / 2] GEGLU; [H, M, N] batched; SPLITT: columns n_split.. are what
    outT holds, transposed back). The product runs in row blocks; a handful of rows are recomputed on the host."""
    A = (ops["A"] if A is None else A).to(device, dtype)
    W = (ops["W"] if W is None else W).to(device, dtype)
    Wt = W.transpose(-1, -2).contiguous()
    Wt2 = Wt * Wt
    M = A.shape[-2]
    y = torch.empty(A.shape[:-1] + (W.shape[-2],), dtype=dtype, device=device)
    Q = torch.empty_like(y)
    for r0 in range(0, M, 2048):
        a = A[..., r0:r0 + 2048, :]
        y[..., r0:r0 + 2048, :] = a @ Wt
        Q[..., r0:r0 + 2048, :] = (a * a) @ Wt2
    if check_rows and dtype == torch.float64:
        rows = torch.tensor(sorted({0, M // 3, M // 2, max(0, M - 136), M - 1}))
        host = ops["A"].double()[..., rows, :] @ ops["W"].double().transpose(-1, -2)
        if torch.equal(ops["A"].double(), A.cpu()) and torch.equal(ops["W"].double(), W.cpu()):
            assert (y[..., rows.to(device), :].cpu() - host).abs().max().item() <= 1e-9 * max(1.0, host.abs().max().item()), "device and host fp64 disagree"
    r = {"Q": Q, "bias": torch.zeros((), dtype=dtype, device=device), "x": torch.zeros((), dtype=dtype, device=device), "gate": None}
    if ops["bias"] is not None:
        b = ops["bias"].to(device, dtype)
        y = y + b
        r["bias"] = b.abs().expand_as(y)
    r["y"] = y
    if c.epi in (EPI_GELU, EPI_GELU_ERF):
        r["ref"] = gelu(y, c.epi)
    elif c.epi == EPI_GEGLU:
        r["ref"] = y[..., 1::2] * gelu(y[..., 0::2], c.epi)
    elif c.epi == EPI_RESID:
        x = ops["x"].to(device, dtype)
        r["x"] = x.abs()
        if ops["gate"] is not None:
            idx = ops["idx"] if idx is None else idx
            gt = ops["gate"].to(device, dtype)
            r["gate"] = gt[idx.long().to(device)] if idx is not None else gt[0].expand_as(y)
            r["ref"] = x + y * r["gate"]
        else:
            r["ref"] = x + y
    else:
        r["ref"] = y
    return r


def tanh_allowance(x, ref):
    return C_TANH * 2.0 ** -23 * (1 + x.abs() ** 3) * ref.abs() + ACT_FLOOR


def erf_allowance(x, ref):
    return 2.0 ** -23 * (C_ERF * x.abs() + 2 * ref.abs())


def bound(c, r):
    """the per-element error a correct kernel may show (module docstring)"""
    ref, y = r["ref"].abs(), r["y"]
    ey = 2.0 ** -14 * r["Q"].sqrt() + 2.0 ** -22 * (y.abs() + r["bias"])
    if c.epi in (EPI_BF16, EPI_SPLITT):
        return 2.0 ** -8 * ref + ey
    if c.epi == EPI_F32:
        return ey
    if c.epi == EPI_RESID:
        return (ey * r["gate"].abs() if r["gate"] is not None else ey) + 2.0 ** -22 * (ref + r["x"])
    if c.epi == EPI_GELU:
        return 2.0 ** -8 * ref + GELU_SLOPE * ey + tanh_allowance(y, r["ref"])
    if c.epi == EPI_GELU_ERF:
        return 2.0 ** -8 * ref + GELU_SLOPE * ey + erf_allowance(y, r["ref"])
    assert c.epi == EPI_GEGLU, c
    g, v, eg, ev = y[..., 0::2], y[..., 1::2], ey[..., 0::2], ey[..., 1::2]
    gg = gelu(g, c.epi)
    dg = GELU_SLOPE * eg + tanh_allowance(g, gg)
    return 2.0 ** -8 * ref + v.abs() * dg + (gg.abs() + dg) * ev + 2.0 ** -23 * ref


# ------------------------------------------------------------------------------------------------ the call
def _buffers(c, ops, device):
    """-> {"out": (buffer, mask of the stored elements), "outT": ...}: every buffer GUARD-valued, with guard rows behind (and, row0, in
    front of) the stored rows, guard columns where ldo / ldt exceed the stored ones; RESID: the stored elements hold x"""
    dt = torch.float32 if out_elem_bytes(c) == 4 else torch.bfloat16
    _, _, ldo, ldt = strides(c)
    bufs = {}
    if c.api == "batched" and c.form in ("scores", "pattern"):
        H = T5_H if c.form == "scores" else 2
        buf = torch.full((H * c.M + 1, ldo), GUARD, dtype=dt, device=device)
        mask = torch.zeros(buf.shape, dtype=torch.bool, device=device)
        mask[:H * c.M, :c.N] = True
        bufs["out"] = (buf, mask)
    elif c.api == "batched":
        buf = torch.full((c.M + 1, ldo), GUARD, dtype=dt, device=device)
        mask = torch.zeros(buf.shape, dtype=torch.bool, device=device)
        mask[:c.M] = True
        bufs["out"] = (buf, mask)
    else:
        buf = torch.full((c.row0 + c.M + 1, ldo), GUARD, dtype=dt, device=device)
        mask = torch.zeros(buf.shape, dtype=torch.bool, device=device)
        mask[c.row0:c.row0 + c.M, :out_cols(c)] = True
        if c.epi == EPI_RESID:
            buf[c.row0:c.row0 + c.M, :c.N] = ops["dev"]["x"]
        bufs["out"] = (buf, mask)
        if c.epi == EPI_SPLITT:
            bt = torch.full((c.N - c.n_split + 1, ldt), GUARD, dtype=torch.bfloat16, device=device)
            mt = torch.zeros(bt.shape, dtype=torch.bool, device=device)
            mt[:c.N - c.n_split, :c.M] = True
            bufs["outT"] = (bt, mt)
    return bufs


def _ptr(t, elems=0):
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size()) if t is not None else None


def run_case(c, ops):
    """one call of the raw C-ABI (strided views and the caller's split-K workspace do not pass through yume_amd.ops) -> the buffers of
    `_buffers`, and under "ws" the split-K workspace"""
    from yume_amd import _lib
    lib = _lib.load()
    d = ops["dev"]
    device = (d["store"] if "store" in d else d["A"]).device
    st = torch.cuda.current_stream().cuda_stream
    bufs = _buffers(c, ops, device)
    out = bufs["out"][0]
    lda, ldw, ldo, ldt = strides(c)
    if "store" in d:
        a_p, w_p = _ptr(d["store"], ops["a_view"][0]), _ptr(d["store"], ops["w_view"][0])
    else:
        a_p, w_p = _ptr(d["A"]), _ptr(d["W"])
    if c.api == "batched":
        H, n, npad, hd = T5_H, T5_N, T5_NPAD, T5_HD
        if c.form == "scores":
            args = (a_p, lda, hd, w_p, ldw, hd, n, npad, hd, c.epi, _ptr(out), ldo, n * npad, H)
        elif c.form == "values":
            args = (a_p, lda, n * npad, w_p, ldw, hd * npad, n, hd, npad, c.epi, _ptr(out), ldo, hd, H)
        else:                                   # the same operands for both batches, offset by nothing: both must come out the same
            args = (a_p, lda, 0, w_p, ldw, 0, c.M, c.N, c.K, c.epi, _ptr(out), ldo, c.M * c.N, 2)
        _lib.check(lib.yume_gemm_bf16_batched(*args, 0, st), "yume_gemm_bf16_batched")
    elif c.api == "splitk":
        ws = torch.full((c.splits * c.M * c.N,), float("nan"), dtype=torch.float32, device=device)
        assert ws.numel() * 4 == int(lib.yume_gemm_splitk_workspace_bytes(c.M, c.N, c.splits))
        _lib.check(lib.yume_gemm_bf16_splitk(a_p, lda, w_p, ldw, _ptr(d.get("bias")), c.M, c.N, c.K, c.epi, _ptr(out), ldo, c.splits, _ptr(ws), st),
                   "yume_gemm_bf16_splitk")
        bufs["ws"] = ws
    else:
        tab = d.get("tab")
        outT = bufs["outT"][0] if "outT" in bufs else None
        rc = lib.yume_gemm_bf16_ws(a_p, lda, w_p, ldw, _ptr(d.get("bias")), c.M, c.N, c.K, c.epi, _ptr(out, c.row0 * ldo), ldo,
                                   _ptr(tab, 2 * c.N) if tab is not None else None, 6 * c.N if tab is not None else 0, _ptr(d.get("idx")),
                                   _ptr(outT), ldt, c.n_split, c.variant, None, 0, st)
        _lib.check(rc, "yume_gemm_bf16_ws")
    return bufs


def gather(c, bufs):
    """what the call stored, in the layout of reference()["ref"]"""
    out = bufs["out"][0]
    if c.api == "batched":
        if c.form == "values":
            return out[:c.M].view(c.M, T5_H, T5_HD).permute(1, 0, 2)
        return out[:-1].view(-1, c.M, out.shape[1])[..., :c.N]
    got = out[c.row0:c.row0 + c.M, :out_cols(c)]
    if c.epi == EPI_SPLITT:
        got = torch.cat([got, bufs["outT"][0][:c.N - c.n_split, :c.M].t()], dim=1)
    return got


def guards_damaged(bufs):
    """number of elements outside the stored regions that no longer hold GUARD"""
    return sum(int(((bm[0] != GUARD) & ~bm[1]).sum()) for key, bm in bufs.items() if key != "ws")


def kernel_of(line):
    """`[gemm_bf16] <kernel> M=.. ...` -> <kernel>"""
    return line.split()[1]


def main(argv):
    if argv != ["--routes"]:
        sys.exit(__doc__)
    for c in CASES:
        ops = make_case(c, "cuda")
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {c.name}\n")
        sys.stderr.flush()
        run_case(c, ops)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main(sys.argv[1:])
