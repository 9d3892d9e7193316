"""Case table of yume_adaln_modulate_mx_e2m3 (tests/test_norm_e2m3_cpu.py, tests/test_norm_e2m3_gpu.py).

The call is DEFINED as the host MX6 quantiser (tests/gemm_f6_cases.py mx6_quantise + mx6_pack_bits) applied to what
yume_adaln_modulate(..., out_kind = 0) stores, so the yardstick is that composite on the same device inputs, bit for bit: packed bytes and
scale bytes. Shapes: T in {1, 3, 1023, 1024, 1030} (1024 is the threshold of the two-row instance; 1023 an odd count below it), C in
{128, 384} (one and three blocks per eight-lane group row; 384 / 4 = 96 vectors: the last wave of the first pass is part-filled); with and
without row_idx; and the affine-only form of norm3 (mul = weight, add = bias, tab_stride 0, no row_idx, add_one off). Guard bytes beyond
3 C / 4 and C / 32 and one guard row behind T. The operands come from tests/norm_e4m3_cases.py make_case (outliers, an exactly-zero row).
"""
import torch

import norm_e4m3_cases as nc

GUARD_BYTE = 0xA5
LDQ_X, LDE_X = 16, 16        # bytes a q row / scale row is longer than it must be

# (name, T, C, form): form "idx" / "noidx" (adaLN: table rows, add_one on) / "norm3" (affine only)
CASES = [(f"T{T}_C{C}_{form}", T, C, form) for T in (1, 3, 1023, 1024, 1030) for C in (128, 384) for form in ("noidx", "idx", "norm3")]
IDS = [c[0] for c in CASES]
LOG_SHAPES = [(3, 128), (1023, 384), (1024, 384), (1030, 128)]


def instance(T, C):
    """the log name of the instance a case must run on (YUME_NORM_LOG=1)"""
    return "adaln2_e2m3" if C <= 3072 and T >= 1024 else "adaln_e2m3<%d>" % (3 if C <= 3072 else 5 if C <= 5120 else 8)


def ceil16(v):
    return (v + 15) // 16 * 16


def pitches(C):
    return ceil16(3 * C // 4) + LDQ_X, ceil16(C // 32) + LDE_X


def make_case(T, C, form):
    """-> x fp32 [T, C + 4], mul / add views, tab_stride, row_idx or None, add_one"""
    x, tab, idx = nc.make_case(T, C, form == "idx", True, False)
    if form == "norm3":
        return x, tab[1, 0], tab[1, 1], 0, None, False
    return x, tab[:, 0], tab[:, 1], 2 * C, idx, True
