"""The int8 row format (yume_amd/csrc/i8.hpp) on the host: inputs, an independent mirror of the quantiser in numpy fp32, its checks, and the
case table of yume_adaln_modulate_i8 (no test functions in here; tests/test_norm_i8_cpu.py proves the mirror, tests/test_norm_i8_gpu.py
holds yume_quant_rows_i8 and yume_adaln_modulate_i8 to it bit for bit). Nothing in here touches yume_amd.ops.

    amax = max_k |x[r, k]|;  scale[r] = amax / 127 in fp32 (1 for a zero row);  q = rne(clamp(x / scale, +-127))
    x / scale = (x * pre) * inv,  inv = 1 / (scale * pre),  pre = 2^64 where scale < 2^-60, else 1           (the kernel's form)
    a row with an Inf or a NaN: scale = NaN, every byte 0

Every step is one IEEE fp32 operation (numpy keeps subnormals), so the kernel has to reproduce the mirror bit for bit. Against the real
quotient v = x / scale in fp64 the mirror is held to   |q - v| <= 0.5 + 2^-20 |v|   (check()).

Quantiser inputs (make_input): K in {16, 128, 384, 3072}, R in {1, 5, 301}; for R >= 5 the special rows — all zero; the largest bf16 among
tiny values; bf16 subnormals (the pre-scaled reciprocal); +-amax; and a row of exact .5 ties: amax = 127 * 2^e makes scale = 2^e and
inv = 2^-e exact, the other elements are (j + 0.5) 2^e, which bf16 holds for |j| <= 126 — round-to-nearest-even shows in every one of them.

Emitter cases: C in {512, 3072, 5120}, T in {5, 1023, 1025} (from T = 1024 on, C <= 3072 runs the two-row instance; 1025 leaves it an odd
tail row), the modulated form (add_one, tab_stride = 2 C) and the norm3 affine form (no add_one; without row_idx tab_stride = 0, as the
engine calls it), each with and without row_idx, plus one C = 8192 row for adaln_i8<8>. Inputs are tests/norm_e4m3_cases.make_case's.
"""
import numpy as np
import torch

import norm_e4m3_cases as ec

I8_MAX = 127.0
GUARD_BYTE = 0x5A
GUARD_SCALE = 7.0
QUANT_SHAPES = [(R, K) for R in (1, 5, 301) for K in (16, 128, 384, 3072)]
SPECIAL_ROWS = {"zero": 0, "huge": 1, "subnormal": 2, "plus_minus_amax": 3, "ties": 4}      # rows of the R >= 5 inputs
TIE_EXP = 3                                                                                 # the tie row is scaled by 2^3

ZERO_MOD, N_MOD = ec.ZERO_MOD, ec.N_MOD
zero_row_of = ec.zero_row_of

# (name, T, C, row_idx, add_one)
EMIT_CASES = []
for T in (5, 1023, 1025):
    for C in (512, 3072, 5120):
        for use_idx in (False, True):
            for add_one in (True, False):
                EMIT_CASES.append((f"T{T}_C{C}_{'idx' if use_idx else 'noidx'}_{'modulated' if add_one else 'affine'}", T, C, use_idx, add_one))
EMIT_CASES.append(("T5_C8192_idx_modulated", 5, 8192, True, True))
EMIT_IDS = [c[0] for c in EMIT_CASES]


def instance(T, C):
    """the log name of the instance a shape must run on (YUME_NORM_LOG=1)"""
    if C <= 3072 and T >= 1024:
        return "adaln2_i8"
    return "adaln_i8<%d>" % (3 if C <= 3072 else 5 if C <= 5120 else 8)


def tab_stride(C, use_idx, add_one):
    return 0 if (not use_idx and not add_one) else 2 * C


def make_emit_case(T, C, use_idx, add_one):
    """host tensors: x fp32 [T, C + 4] (ldx > C), table fp32 [N_MOD, 2, C] (mul = table[:, 0], add = table[:, 1]), row_idx int32 [T] or
    None; with row_idx, row zero_row_of(T) comes out exactly zero"""
    return ec.make_case(T, C, use_idx, add_one, False)


def tie_values(K):
    """the tie row before its scale 2^TIE_EXP: 127 first, then (j + 0.5) for j = 0, -1, 1, -2, ... cycling through |j + 0.5| <= 126.5"""
    j = np.arange(K - 1)
    half = np.where(j % 2 == 0, (j // 2) % 127 + 0.5, -((j // 2) % 127) - 0.5)
    return np.concatenate([[127.0], half]).astype(np.float32)


def make_input(R, K, seed=0):
    """bf16 [R, K]: rows of very different magnitude; for R >= 5 the special rows"""
    g = torch.Generator(device="cpu").manual_seed(1000 * R + K + seed)
    x = torch.randn(R, K, generator=g) * 10.0 ** (6 * torch.rand(R, 1, generator=g) - 3)
    if R >= 5:
        x[SPECIAL_ROWS["zero"]] = 0
        x[SPECIAL_ROWS["huge"]] = torch.randn(K, generator=g) * 1e-30              # the largest bf16 among tiny values
        x[SPECIAL_ROWS["huge"], K // 3] = 3.3895313892515355e38                    # 0x7f7f
        x[SPECIAL_ROWS["subnormal"]] = (torch.randint(-127, 128, (K,), generator=g).float() * 2.0 ** -133)     # bf16 subnormals: j 2^-133
        x[SPECIAL_ROWS["subnormal"], 1] = 100 * 2.0 ** -133
        x[SPECIAL_ROWS["plus_minus_amax"], 2] = 5.0 * x[SPECIAL_ROWS["plus_minus_amax"]].abs().max()
        x[SPECIAL_ROWS["plus_minus_amax"], K - 3] = -x[SPECIAL_ROWS["plus_minus_amax"], 2]
        x[SPECIAL_ROWS["ties"]] = torch.from_numpy(tie_values(K)) * 2.0 ** TIE_EXP
    return x.bfloat16()


# ------------------------------------------------------------------------------------------------ the mirror (numpy, fp32, no yume_amd)
def bf16_to_f32(x):
    """torch bf16 [R, K] -> numpy fp32 through the bits"""
    return (x.contiguous().view(torch.int16).numpy().astype(np.uint16).astype(np.uint32) << 16).view(np.float32)


def mirror(x, truncate=False, qmax=I8_MAX):
    """x: torch bf16 [R, K] on the host -> (q int8 [R, K], scale fp32 [R]) as torch tensors. truncate / qmax: the faulty quantisers of
    tests/test_norm_i8_cpu.py."""
    f = bf16_to_f32(x)
    one, F = np.float32(1.0), np.float32
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(f).all(axis=1)
        amax = np.abs(np.where(np.isfinite(f), f, F(0))).max(axis=1).astype(np.float32)
        s = np.where(amax > 0, amax / F(qmax), one).astype(np.float32)           # one IEEE fp32 division per row
        pre = np.where(s < F(2.0 ** -60), F(2.0 ** 64), one).astype(np.float32)
        inv = (one / (s * pre)).astype(np.float32)
        t = ((f * pre[:, None]).astype(np.float32) * inv[:, None]).astype(np.float32)
        t = np.minimum(np.maximum(t, F(-qmax)), F(qmax))                         # clamp BEFORE the rounding
        q = (np.trunc(t) if truncate else np.rint(t))                            # np.rint: round half to even
        q = np.where(bad[:, None], 0, q).astype(np.int8)
        s = np.where(bad, F(np.nan), s).astype(np.float32)
    return torch.from_numpy(q), torch.from_numpy(s)


def ref_scale(x):
    amax = x.float().abs().amax(dim=1)
    return torch.where(amax > 0, amax / torch.tensor(I8_MAX), torch.ones_like(amax))


def check(x, q, scale):
    """x bf16 [R, K] (finite), q int8 [R, K], scale fp32 [R] (all on the host) -> dict of violation counts"""
    want = ref_scale(x)
    v = x.double() / want.double().view(-1, 1)
    err = (q.double() - v).abs()
    amax = x.float().abs().amax(dim=1, keepdim=True)
    at_amax = (x.float().abs() == amax) & (amax > 0)
    return {
        "scale_bits": int((scale.view(torch.int32) != want.view(torch.int32)).sum()),
        "outside_bound": int((~(err <= 0.5 + 2.0 ** -20 * v.abs())).sum()),           # (NaN compares false: counted)
        "amax_not_127": int((q.double()[at_amax] != 127.0 * torch.sign(x.double()[at_amax])).sum()),
        "byte_0x80": int((q == -128).sum()),
    }


CLEAN = {"scale_bits": 0, "outside_bound": 0, "amax_not_127": 0, "byte_0x80": 0}
