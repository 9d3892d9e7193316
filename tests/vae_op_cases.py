"""The case table of the VAE's memory-bound kernels (csrc/vae_ops.hip: the three RMS_norm(+SiLU) forms, the DupUp3D / AvgDown3D shortcut adds in
their general and per-line forms, the row softmax in its three-pass and register-window forms, the NCTHW <-> channels-last packers), their
fp64 reference, the per-element error bound and a host fp32 emulation of the kernels' arithmetic in their own order (no test functions here).

tests/test_vae_op_routes_gpu.py runs one call per CASES row through the raw C-ABI (so that ld > C can be passed) and holds EVERY output
element to `outside()` against `reference()`, with NaN around every output and in every stride gap; tests/test_vae_op_cases_cpu.py proves
the table, the route mirror, the reference, the bound and the faults it flags on the host. profiles/r17_vae_op_routes.md has the derivation
and the figures.

The bound, per element, with u = 2^-24 (fp32) and the family's kappa (KAPPA, fixed against `emulate()` with a factor 2 on top):

    norm            2^-8 |ref| + kappa u A_i,  A_i = (|x_i| rstd |g_i| + |b_i|) L;  L = 1 without SiLU, sup |silu'| with it (SILU_LIP, derived below)
    dupup           2^-8 |ref| + kappa u (|y| + |x|)
    avgdown         2^-8 |ref| + kappa u (|y| + mean_g |x_g|)
    softmax         2^-8 p_i + kappa u p_i (1 + |scale (s_i - max)|) + 2^-126;  P[:, n:ldp] zero in its bits
    pack, affine    2^-8 |ref| + kappa u (|x m| + |a|)                 (one rounding to bf16 of an fp32 value)
    unpack, affine  kappa u (|x| + |sub|) |mul|                        (fp32 output; the clamp moves no two values apart)
    plain movers    the bits of the input (rounded to bf16, nearest even, where the input is fp32); zero fill in its bits

2^-8 |ref| is the one rounding to nearest even of the fp32 value to bf16 (half an ulp of 8 significant bits); kappa u A_i is what the fp32
value itself is off by, A_i the magnitude of what is added and cancelled on the way to element i.

    python tests/vae_op_cases.py --routes              one call per case, `CASE <name>` on stderr before each (YUME_VAE_LOG=1 names the kernels)
    python tests/vae_op_cases.py --norm-bound          the norm rows alone, each held to the bound; exit 1 on any element outside
"""
import ctypes
import math
import os
import sys
import zlib
from collections import namedtuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import vae as ov  # noqa: E402

U = 2.0 ** -24
FLOOR = 2.0 ** -126
NAN = float("nan")
GRID_CAP = 16384 * 256           # elements one trip of grid_for()'s stride loops covers
LINE_LIMIT = 65536
LOG2E = 1.4426950408889634


def _silu_lipschitz():
    """sup |silu'|: silu'(x) = s (1 + x (1 - s)), s = sigmoid(x); silu''(x) = s (1 - s) (2 + x (1 - 2 s)) has one positive root (bisection on
    [2, 3]: 2 + x (1 - 2 s) is 2 - 2 tanh(1) > 0 at 2 and 2 - 3 tanh(1.5) < 0 at 3), the maximum of silu'; silu' -> 1 from above at +inf,
    its minimum (the mirror root, silu'(-x) = 1 - silu'(x)) is 1 - max > -1"""
    s = lambda x: 1.0 / (1.0 + math.exp(-x))
    lo, hi = 2.0, 3.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 2.0 + mid * (1.0 - 2.0 * s(mid)) > 0:
            lo = mid
        else:
            hi = mid
    return s(lo) * (1.0 + lo * (1.0 - s(lo)))


SILU_LIP = _silu_lipschitz()     # 1.0998...
# fixed against emulate() on the table's own inputs: the smallest value that leaves its fp32 values with zero elements outside, times 2,
# rounded up to a whole number (tests/test_vae_op_cases_cpu.py asserts exactly that; the figures: profiles/r17_vae_op_routes.md)
KAPPA = {"norm": 10.0, "dupup": 2.0, "avgdown": 3.0, "softmax": 6.0, "pack": 4.0, "unpack": 4.0}

Case = namedtuple("Case", "name fam route p")
NORM_ORIG = [(8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4), (64, 8)]
NORM_G = [(g, nvl, {1: 4, 3: 2, 5: 1}[nvl]) for nvl in (1, 3, 5) for g in (1, 2, 4, 8, 16, 32, 64)]
NORM_FLAT = [(nvec, nvl, ri) for nvec, nvl, ri in ((12, 3, 2), (24, 3, 2), (48, 3, 2), (20, 5, 1), (40, 5, 1), (80, 5, 1))]
NORM_ROUTES = tuple(["rms<%d,%d>" % t for t in NORM_ORIG] + ["rms_g<%d,%d,%d>" % t for t in NORM_G] +
                    ["rms_flat<%d,%d,%d,%d,%d>" % (t + (s, b)) for t in NORM_FLAT for s in (0, 1) for b in (0, 1)])
ROUTES = NORM_ROUTES + ("dupup", "dupup_lines<1>", "dupup_lines<2>", "dupup_lines<4>", "avgdown", "avgdown_lines<1>", "avgdown_lines<2>",
                        "avgdown_lines<4>", "avgdown_lines<8>", "softmax_rows", "softmax_rows_reg<2>", "softmax_rows_reg<4>", "softmax_rows_reg<8>",
                        "pack<f32>", "pack<bf16>", "unpack")


def _ragged(wg):
    """one whole workgroup of `wg` rows plus one whole wave plus a part of a wave (eight rows at the least: the special rows need them)"""
    m = wg + wg // 4 + wg // 8
    while m < 8:
        m += wg
    return m


def _norm(name, route_, M, C, silu, beta, ldx_x=0, ldy_x=0, inplace=False):
    return Case(name, "norm", route_, dict(M=M, C=C, silu=int(silu), beta=int(beta), ldx_x=ldx_x, ldy_x=ldx_x if inplace else ldy_x, inplace=inplace))


def _norm_rows():
    rows, k = [], 0
    combo = lambda i: ((1, 0), (1, 1), (0, 0), (0, 1))[i % 4]
    # ---- the original form, reachable with no switch: nvl = nvec / G not in {1, 3, 5}
    for C, (lpr, nv), note in ((56, (8, 1), "idle_lane"), (72, (16, 1), ""), (144, (32, 1), ""), (288, (64, 1), ""), (576, (64, 2), "part_vector"),
                               (1024, (64, 2), ""), (2048, (64, 4), ""), (4088, (64, 8), "last_vector_off"), (4096, (64, 8), "abi_max")):
        s, b = combo(k)
        wg = 4 * 64 // lpr
        M = 1 if C == 288 else _ragged(wg)
        rows.append(_norm("rms_c%d%s" % (C, "_" + note if note else "") + ("_m1" if M == 1 else "") + ("_inplace" if C == 576 else ""),
                          "rms<%d,%d>" % (lpr, nv), M, C, s, b, ldx_x=8 if C in (72, 576, 4088) else 0, ldy_x=16 if C in (144, 4088) else 0, inplace=C == 576))
        k += 1
    # ---- the grouped form: NVL = 1 (G = 1 .. 64), NVL = 3 and 5 (contiguous where the flat form does not take the width, strided where it does)
    for nvl, ri, widths in ((1, 4, (8, 16, 32, 64, 128, 256, 512)), (3, 2, (24, 48, 96, 192, 384, 768, 1536)), (5, 1, (40, 80, 160, 320, 640, 1280, 2560))):
        for gi, C in enumerate(widths):
            G = 1 << gi
            s, b = combo(k)
            flat_width = C // 8 in (12, 24, 48, 20, 40, 80)
            wg = ri * 4 * 64 // G
            M = 1 if C in (64, 768, 1280) else _ragged(wg)
            lx, ly = ((8, 0) if C in (96, 640) else (0, 8)) if flat_width else ((8, 8) if C in (16, 1536, 2560) else (0, 0))
            inpl = C in (128, 192, 320)
            if inpl:
                lx = ly = 8 if flat_width else 0
            rows.append(_norm("rmsg_c%d" % C + ("_m1" if M == 1 else "") + ("_ldx" if lx else "") + ("_ldy" if ly and not inpl else "") + ("_inplace" if inpl else ""),
                              "rms_g<%d,%d,%d>" % (G, nvl, ri), M, C, s, b, ldx_x=lx, ldy_x=ly, inplace=inpl))
            k += 1
    # ---- the flat form: every instance; M ragged / part-filled last chunk with a wholly dead last RI-chunk / 1 / in place
    for nvec, nvl, ri in NORM_FLAT:
        R = nvl * 64 // nvec
        wg = 4 * ri * R
        for s, b in ((1, 0), (1, 1), (0, 0), (0, 1)):
            if (s, b) == (1, 1):
                M, tag = wg + R // 2, "_deadchunk"          # the second workgroup's first wave: chunk 0 half filled, chunk 1 (RI = 2) dead
            elif (s, b) == (0, 0) and nvec in (12, 20):
                M, tag = 1, "_m1"
            else:
                M, tag = _ragged(wg), ""
            inpl = (s, b) == (0, 1) and nvec in (24, 40)
            rows.append(_norm("rmsflat_c%d_s%db%d%s%s" % (nvec * 8, s, b, tag, "_inplace" if inpl else ""), "rms_flat<%d,%d,%d,%d,%d>" % (nvec, nvl, ri, s, b),
                              M, nvec * 8, s, b, inplace=inpl))
    return rows


def _dup(name, route_, Tin, Hin, Win, Cin, Cout, ft, fs, toff, ldx_x=0, ldy_x=0):
    return Case(name, "dupup", route_, dict(Tin=Tin, Hin=Hin, Win=Win, Cin=Cin, Cout=Cout, ft=ft, fs=fs, toff=toff, ldx_x=ldx_x, ldy_x=ldy_x))


def _avg(name, route_, Tin, Hin, Win, Cin, Cout, ft, fs, ldx_x=0, ldy_x=0):
    return Case(name, "avgdown", route_, dict(Tin=Tin, Hin=Hin, Win=Win, Cin=Cin, Cout=Cout, ft=ft, fs=fs, ldx_x=ldx_x, ldy_x=ldy_x))


def _sm(name, route_, R, n, lds, ldp, scale=0.25, soff=0):
    return Case(name, "softmax", route_, dict(R=R, n=n, lds=lds, ldp=ldp, scale=scale, soff=soff))


def _pack(name, bf16, C, T, H, W, ps, Cpad, affine):
    return Case(name, "pack", "pack<bf16>" if bf16 else "pack<f32>", dict(bf16=bf16, C=C, T=T, H=H, W=W, ps=ps, Cpad=Cpad, affine=affine))


def _unpack(name, T, H, W, Cv, ps, ldx_x, affine, clamp):
    return Case(name, "unpack", "unpack", dict(T=T, H=H, W=W, Cv=Cv, ps=ps, ldx_x=ldx_x, affine=affine, clamp=clamp))


CASES = _norm_rows() + [
    # ---- yume_vae_dupup_add, the per-line form: Q = Cin / Cout in {1, 2, 4}, repeats = F / Q a power of two
    _dup("dupl_q1_ft2_fs2_first", "dupup_lines<1>", 2, 3, 5, 64, 64, 2, 2, 1),                       # cv = 8, a power of two; toff = ft - 1
    _dup("dupl_q2_ft1_fs2_strided", "dupup_lines<2>", 2, 3, 5, 80, 40, 1, 2, 0, ldx_x=8, ldy_x=8),   # cv = 5
    _dup("dupl_q4_ft2_fs2", "dupup_lines<4>", 1, 2, 3, 384, 96, 2, 2, 0),                            # cv = 12; toff = 0
    _dup("dupl_q4_ft2_fs2_first_strided", "dupup_lines<4>", 2, 2, 3, 160, 40, 2, 2, 1, ldx_x=8, ldy_x=8),
    _dup("dupl_q2_ft2_fs1_first", "dupup_lines<2>", 3, 4, 5, 128, 64, 2, 1, 1),                      # fs = 1 with ft = 2
    _dup("dupl_q1_ft1_fs2_gx2", "dupup_lines<1>", 1, 1, 65, 64, 64, 1, 2, 0),                        # Wo cv = 1040 > 1024: a second, mostly idle workgroup
    # ---- the general form
    _dup("dup_cin_lt_cout", "dupup", 2, 3, 5, 8, 16, 1, 2, 0, ldx_x=8, ldy_x=8),                     # repeats 8 > F = 4
    _dup("dup_q8_first", "dupup", 2, 3, 5, 64, 8, 2, 2, 1),                                          # Q = 8
    _dup("dup_q2_ldx_odd", "dupup", 2, 3, 5, 16, 8, 2, 2, 0, ldx_x=4),                               # ldx % 8 != 0 at a Q the per-line form takes
    # ---- the line limit: To Ho = 255 x 257 and 256 x 256
    _dup("dupl_65535_lines", "dupup_lines<1>", 128, 257, 1, 8, 8, 2, 1, 1),
    _dup("dup_65536_lines", "dupup", 128, 256, 1, 8, 8, 2, 1, 0),
    # ---- beyond grid_for's cap: 1182 x 1186 pixels x 3 vectors = 4 205 556 > 4 194 304, a second trip with a ragged end (67 MB)
    _dup("dup_two_trips", "dupup", 1, 591, 593, 8, 24, 1, 2, 0),
    # ---- yume_vae_avgdown_add, the per-line form: RR = F / G in {1, 2, 4, 8}
    _avg("avgl_rr1_front_pad", "avgdown_lines<1>", 3, 4, 6, 160, 160, 2, 2),                         # Tin % ft != 0; cv = 20
    _avg("avgl_rr2_tin1", "avgdown_lines<2>", 1, 4, 6, 160, 320, 2, 2),                              # Tin = 1 with ft = 2; cv = 40
    _avg("avgl_rr4_strided", "avgdown_lines<4>", 4, 4, 6, 16, 64, 2, 2, ldx_x=8, ldy_x=8),
    _avg("avgl_rr8_front_pad_strided", "avgdown_lines<8>", 3, 4, 6, 8, 64, 2, 2, ldx_x=8, ldy_x=16),
    _avg("avgl_rr2_ft1", "avgdown_lines<2>", 2, 4, 6, 32, 64, 1, 2, ldy_x=8),
    # ---- the general form
    _avg("avg_g3", "avgdown", 2, 4, 6, 24, 32, 1, 2, ldx_x=8, ldy_x=8),                              # G = 3: a division that is not by a power of two
    _avg("avg_g8_gt_f", "avgdown", 2, 4, 6, 64, 32, 1, 2),                                           # G = 8 > F = 4: two input channels per output
    _avg("avg_g3_front_pad", "avgdown", 3, 2, 3, 24, 16, 2, 1),                                      # F = 2, G = 3, a padded first frame
    _avg("avgl_65535_lines", "avgdown_lines<1>", 255, 257, 1, 8, 8, 1, 1),
    _avg("avg_65536_lines", "avgdown", 256, 256, 1, 8, 8, 1, 1),
    _avg("avg_two_trips", "avgdown", 1, 726, 724, 24, 32, 1, 2),                                     # 363 x 362 x 32 = 4 204 992 > 4 194 304 (8.4 MB of y)
    # ---- yume_softmax_rows
    _sm("smax_n1", "softmax_rows_reg<2>", 3, 1, 4, 64),
    _sm("smax_n3", "softmax_rows_reg<2>", 4, 3, 4, 4),
    _sm("smax_n100", "softmax_rows_reg<2>", 5, 100, 100, 100),                                       # ldp = n
    _sm("smax_n101_lds104", "softmax_rows_reg<2>", 3, 101, 104, 128, scale=384 ** -0.5),
    _sm("smax_n2048", "softmax_rows_reg<2>", 4, 2048, 2048, 2048),
    _sm("smax_n2048_ldp_beyond_window", "softmax_rows_reg<2>", 5, 2048, 2048, 2112, scale=1024 ** -0.5),   # the tail loop: 64 columns past 4 x 256 x 2
    _sm("smax_n2049_ldp_inside_window", "softmax_rows_reg<4>", 3, 2049, 2052, 2304),
    _sm("smax_n4096", "softmax_rows_reg<4>", 5, 4096, 4096, 4096, scale=384 ** -0.5),
    _sm("smax_n4097", "softmax_rows_reg<8>", 5, 4097, 4100, 4160),
    _sm("smax_n8163_lds8164", "softmax_rows_reg<8>", 3, 8163, 8164, 8192, scale=1024 ** -0.5),
    _sm("smax_n8192", "softmax_rows_reg<8>", 4, 8192, 8192, 8192),
    _sm("smax_n8193_three_pass", "softmax_rows", 5, 8193, 8196, 8256),
    _sm("smax_n101_lds101_three_pass", "softmax_rows", 3, 101, 101, 104, scale=384 ** -0.5),          # lds % 4 != 0
    _sm("smax_n100_ldp102_three_pass", "softmax_rows", 4, 100, 100, 102),                            # ldp % 4 != 0
    _sm("smax_n100_misaligned_three_pass", "softmax_rows", 5, 100, 100, 100, soff=1),                # S one float off a 16-byte boundary
    _sm("smax_n1_ldp1_three_pass", "softmax_rows", 3, 1, 1, 1),
    # ---- yume_vae_pack_input
    _pack("pack_f32_c3_ps2_t1", False, 3, 1, 6, 10, 2, 16, False),
    _pack("pack_f32_c3_ps2_t3_affine", False, 3, 3, 6, 10, 2, 16, True),
    _pack("pack_bf16_c3_ps2_t3", True, 3, 3, 6, 10, 2, 16, False),
    _pack("pack_f32_c16_ps1_t3_affine", False, 16, 3, 5, 7, 1, 16, True),                            # decode's z / scale + mean
    _pack("pack_bf16_c16_ps1_t1", True, 16, 1, 5, 7, 1, 16, False),
    _pack("pack_f32_c48_ps1_t3", False, 48, 3, 5, 7, 1, 48, False),
    _pack("pack_bf16_c48_ps1_cpad56_t1_affine", True, 48, 1, 5, 7, 1, 56, True),
    _pack("pack_f32_c48_ps1_cpad56_t3", False, 48, 3, 5, 7, 1, 56, False),
    _pack("pack_f32_two_trips", False, 3, 1, 1030, 1022, 2, 16, False),                              # 515 x 511 x 16 = 4 210 640 > 4 194 304
    # ---- yume_vae_unpack_output
    _unpack("unpack_ps1_affine", 3, 5, 7, 16, 1, 0, True, False),                                    # encode's (mu - mean) / std
    _unpack("unpack_ps2_ldx_clamp", 3, 5, 7, 12, 2, 4, False, True),                                 # decode's unpatchify and clamp
    _unpack("unpack_ps2_affine_clamp", 1, 5, 7, 12, 2, 4, True, True),
    _unpack("unpack_ps1_ldx_plain", 1, 5, 7, 48, 1, 8, False, False),
    _unpack("unpack_two_trips", 1, 592, 591, 12, 2, 4, False, True),                                 # 3 x 1184 x 1182 = 4 198 464 > 4 194 304
]
BY_NAME = {c.name: c for c in CASES}
BIG = ("dup_two_trips", "avg_two_trips", "pack_f32_two_trips", "unpack_two_trips")
SOFTMAX_KINDS = ("wide", "equal", "dominant", "offset_plus", "offset_minus", "ordinary")


# ------------------------------------------------------------------------------------------------ the dispatcher's mirror
def _pow2(v):
    return v > 0 and (v & (v - 1)) == 0


def norm_strides(c):
    return c.p["C"] + c.p["ldx_x"], c.p["C"] + c.p["ldy_x"]


def dup_dims(c):
    p = c.p
    To = p["Tin"] * p["ft"] - p["toff"]
    return To, p["Hin"] * p["fs"], p["Win"] * p["fs"]


def avg_dims(c):
    p = c.p
    padt = (p["ft"] - p["Tin"] % p["ft"]) % p["ft"]
    return (p["Tin"] + padt) // p["ft"], p["Hin"] // p["fs"], p["Win"] // p["fs"], padt


def softmax_aligned(c):
    """S starts soff floats and P 64 elements past a 256-byte boundary (run_case)"""
    return (4 * c.p["soff"]) % 16 == 0


def route(c, grouped=True, flat=True, lines=True, reg=True):
    """the kernel instances the call launches, as YUME_VAE_LOG names them: the conditions of the six entry points of csrc/vae_ops.hip,
    restated. grouped / flat / lines / reg: YUME_VAE_NORM_G, YUME_VAE_NORM_FLAT, YUME_VAE_SHORTCUT_LINES, YUME_VAE_SOFTMAX_REG"""
    p = c.p
    if c.fam == "norm":
        C = p["C"]
        ldx, ldy = norm_strides(c)
        nvec = C // 8
        G = 1
        while G < 64 and nvec % (2 * G) == 0:
            G *= 2
        nvl = nvec // G
        if grouped and flat and ldx == C and ldy == C and nvec in (12, 24, 48, 20, 40, 80):
            nvl_f, ri = (3, 2) if nvec in (12, 24, 48) else (5, 1)
            return ("rms_flat<%d,%d,%d,%d,%d>" % (nvec, nvl_f, ri, p["silu"], p["beta"]),)
        if grouped and nvl in (1, 3, 5):
            return ("rms_g<%d,%d,%d>" % (G, nvl, {1: 4, 3: 2, 5: 1}[nvl]),)
        for lim, inst in ((8, (8, 1)), (16, (16, 1)), (32, (32, 1)), (64, (64, 1)), (128, (64, 2)), (256, (64, 4))):
            if nvec <= lim:
                return ("rms<%d,%d>" % inst,)
        return ("rms<64,8>",)
    if c.fam == "dupup":
        To, Ho, Wo = dup_dims(c)
        Fq = p["ft"] * p["fs"] * p["fs"]
        repeats = p["Cout"] * Fq // p["Cin"]
        Q = Fq // repeats if _pow2(repeats) and Fq % repeats == 0 else 0
        ldx = p["Cin"] + p["ldx_x"]
        if lines and Q in (1, 2, 4) and ldx % 8 == 0 and p["Cin"] == p["Cout"] * Q and 0 < To * Ho < LINE_LIMIT and Wo * (p["Cout"] // 8) < 1 << 30:
            return ("dupup_lines<%d>" % Q,)
        return ("dupup",)
    if c.fam == "avgdown":
        To, Ho, Wo, _ = avg_dims(c)
        Fq = p["ft"] * p["fs"] * p["fs"]
        G = p["Cin"] * Fq // p["Cout"]
        RR = Fq // G if G > 0 and Fq % G == 0 else 0
        ldx, ldy = p["Cin"] + p["ldx_x"], p["Cout"] + p["ldy_x"]
        if lines and RR in (1, 2, 4, 8) and p["Cout"] % 8 == 0 and ldy % 8 == 0 and ldx % 8 == 0 and p["Cin"] * RR == p["Cout"] and \
                0 < To * Ho < LINE_LIMIT and Wo * (p["Cout"] // 8) < 1 << 30:
            return ("avgdown_lines<%d>" % RR,)
        return ("avgdown",)
    if c.fam == "softmax":
        n, lds, ldp = p["n"], p["lds"], p["ldp"]
        ok = reg and lds % 4 == 0 and ldp % 4 == 0 and softmax_aligned(c) and lds >= (n + 3) // 4 * 4
        for nv in (2, 4, 8):
            if ok and n <= 1024 * nv:
                return ("softmax_rows_reg<%d>" % nv,)
        return ("softmax_rows",)
    if c.fam == "pack":
        return ("pack<bf16>" if p["bf16"] else "pack<f32>",)
    return ("unpack",)


def grid_for(total):
    return max(1, min((total + 255) // 256, 16384))


def kernel_of(line):
    """`[vae] <instance> k=v ...` -> <instance>"""
    return line.split()[1]


def log_fields(c):
    """what the YUME_VAE_LOG lines of the call carry beside the instance, one dict per launch"""
    p = c.p
    if c.fam == "norm":
        ldx, ldy = norm_strides(c)
        return [dict(M=p["M"], C=p["C"], ldx=ldx, ldy=ldy, silu=p["silu"], beta=p["beta"])]
    if c.fam in ("dupup", "avgdown"):
        if c.fam == "dupup":
            To, Ho, Wo = dup_dims(c)
            total = To * Ho * Wo * (p["Cout"] // 8)
        else:
            To, Ho, Wo, _ = avg_dims(c)
            total = To * Ho * Wo * p["Cout"]
        per_line = "lines" in route(c)[0]
        return [dict(Tin=p["Tin"], Hin=p["Hin"], Win=p["Win"], Cin=p["Cin"], Cout=p["Cout"], ft=p["ft"], fs=p["fs"], toff=p.get("toff", 0),
                     ldx=p["Cin"] + p["ldx_x"], ldy=p["Cout"] + p["ldy_x"], lines=To * Ho,
                     gx=(Wo * (p["Cout"] // 8) + 1023) // 1024 if per_line else grid_for(total), gy=To * Ho if per_line else 1)]
    if c.fam == "softmax":
        return [dict(R=p["R"], n=p["n"], lds=p["lds"], ldp=p["ldp"])]
    if c.fam == "pack":
        return [dict(C=p["C"], T=p["T"], H=p["H"], W=p["W"], ps=p["ps"], Cpad=p["Cpad"], affine=int(p["affine"]),
                     grid=grid_for(p["T"] * (p["H"] // p["ps"]) * (p["W"] // p["ps"]) * p["Cpad"]))]
    return [dict(T=p["T"], H=p["H"], W=p["W"], Cv=p["Cv"], ps=p["ps"], ldx=p["Cv"] + p["ldx_x"], affine=int(p["affine"]), clamp=int(p["clamp"]),
                 grid=grid_for(p["Cv"] * p["T"] * p["H"] * p["W"]))]


def case_bytes(c):
    """bytes of the largest buffer the call touches"""
    p = c.p
    if c.fam == "norm":
        return (p["M"] + 2) * max(norm_strides(c)) * 2
    if c.fam == "dupup":
        To, Ho, Wo = dup_dims(c)
        return max(To * Ho * Wo * (p["Cout"] + p["ldy_x"]), p["Tin"] * p["Hin"] * p["Win"] * (p["Cin"] + p["ldx_x"])) * 2
    if c.fam == "avgdown":
        To, Ho, Wo, _ = avg_dims(c)
        return max(To * Ho * Wo * (p["Cout"] + p["ldy_x"]), p["Tin"] * p["Hin"] * p["Win"] * (p["Cin"] + p["ldx_x"])) * 2
    if c.fam == "softmax":
        return (p["R"] + 2) * p["lds"] * 4
    if c.fam == "pack":
        return max(p["C"] * p["T"] * p["H"] * p["W"] * (2 if p["bf16"] else 4), p["T"] * (p["H"] // p["ps"]) * (p["W"] // p["ps"]) * p["Cpad"] * 2)
    return max(p["T"] * p["H"] * p["W"] * (p["Cv"] + p["ldx_x"]) * 2, p["Cv"] * p["T"] * p["H"] * p["W"] * 4)


# ------------------------------------------------------------------------------------------------ operands
def _gen(c):
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.encode()))


def _bf16_exact(t):
    return t.bfloat16().float()


ZERO_ROW, SPIKE_ROW = 2, 3


def softmax_kind(c, r):
    """which of SOFTMAX_KINDS row r of the case carries: the kinds rotate over the rows of the table"""
    k0 = [d.name for d in CASES if d.fam == "softmax"].index(c.name)
    return SOFTMAX_KINDS[(r + k0) % len(SOFTMAX_KINDS)]


def _cancelling(y, s, g):
    """half of the elements of y (a seeded choice) replaced by -s (1 +- 2^-6), so that y + s cancels to below 2^-4 |y| there"""
    pick = torch.rand(y.shape, generator=g) < 0.5
    sign = torch.where(torch.rand(y.shape, generator=g) < 0.5, -1.0, 1.0)
    return torch.where(pick & (s != 0), _bf16_exact(-s * (1.0 + sign * 2.0 ** -6)), y), pick


def make_case(c):
    """seeded operands, drawn on the CPU generator, fp32 on the host (bf16-exact where the call takes bf16)"""
    g, p = _gen(c), c.p
    o = {}
    if c.fam == "norm":
        M, C = p["M"], p["C"]
        mag = 2.0 ** ((torch.arange(M) % 13) - 6).float()                    # a neighbour's scale is off by a factor 2 at the least
        x = torch.randn(M, C, generator=g).clamp(-6, 6) * mag[:, None]
        if M >= 8:
            x[ZERO_ROW] = 0.0                                                # the 1e-12 clamp: 0, or act(beta)
            x[SPIKE_ROW] = torch.randn(C, generator=g).clamp(-4, 4) * 2.0 ** -10
            x[SPIKE_ROW, (5 * C) // 7] = 2.0 ** 10
        o["x"] = _bf16_exact(x)
        sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
        o["g"] = sign * (0.5 + 1.5 * (torch.randperm(C, generator=g).float() + 0.5) / C)      # mixed sign, 0.5 .. 2, distinct per channel
        o["b"] = torch.randn(C, generator=g) if p["beta"] else None         # the size of the normalised values: some elements cancel
    elif c.fam in ("dupup", "avgdown"):
        if c.fam == "dupup":
            To, Ho, Wo = dup_dims(c)
        else:
            To, Ho, Wo, _ = avg_dims(c)
        x = _bf16_exact(torch.randn(p["Tin"], p["Hin"], p["Win"], p["Cin"], generator=g) * 2.0)
        y = _bf16_exact(torch.randn(To, Ho, Wo, p["Cout"], generator=g) * 2.0)
        o["x"] = x
        o["y"], o["cancel"] = _cancelling(y, _shortcut64(c, x.double()).float(), g)
    elif c.fam == "softmax":
        R, n, sc = p["R"], p["n"], p["scale"]
        S = torch.empty(R, n)
        for r in range(R):
            kind = softmax_kind(c, r)
            z = torch.randn(n, generator=g)
            if kind == "wide":
                S[r] = z * 100.0 / sc                                        # scale (s - max) of hundreds: most columns underflow
            elif kind == "equal":
                S[r] = 3.25                                                  # p = 1 / n
            elif kind == "dominant":
                S[r] = z
                S[r, (2 * n) // 3] += 200.0                                  # one score 200 above the rest
            elif kind == "offset_plus":
                S[r] = 1.0e4 + 5.0 * z                                       # the max subtraction matters
            elif kind == "offset_minus":
                S[r] = -1.0e4 + 5.0 * z
            else:
                S[r] = 5.0 * z
        o["S"] = S
    elif c.fam == "pack":
        x = torch.randn(p["C"], p["T"], p["H"], p["W"], generator=g)
        o["x"] = _bf16_exact(x) if p["bf16"] else x
        o["mul"] = (0.5 + torch.rand(p["C"], generator=g) * 2.5) if p["affine"] else None
        o["add"] = torch.randn(p["C"], generator=g) if p["affine"] else None
    elif c.fam == "unpack":
        x = torch.randn(p["T"], p["H"], p["W"], p["Cv"], generator=g)
        flat = x.view(-1)
        flat[0::7] = 1.0                                                     # exactly on the clamp, and outside it
        flat[1::7] = -1.0
        flat[2::7] = 1.5
        flat[3::7] = -1.0078125
        o["x"] = _bf16_exact(x)
        Co = p["Cv"] // (p["ps"] * p["ps"])
        o["sub"] = torch.randn(Co, generator=g) if p["affine"] else None
        o["mul"] = (0.5 + torch.rand(Co, generator=g) * 2.5) if p["affine"] else None
    else:
        raise AssertionError(c.fam)
    return o


# ------------------------------------------------------------------------------------------------ reference (fp64) and bound
def silu64(x):
    return x / (1 + torch.exp(-x))


def _shortcut64(c, x):
    """the shortcut branch alone, channels-last fp64 [To, Ho, Wo, Cout], from oracle/vae.py's dup_up / avg_down (channels first)"""
    p = c.p
    xc = x.permute(3, 0, 1, 2)
    if c.fam == "dupup":
        s = ov.dup_up(xc, p["Cout"], p["ft"], p["fs"], p["toff"] != 0)       # first chunk: the first ft - 1 duplicated frames dropped
    else:
        s = ov.avg_down(xc, p["Cout"], p["ft"], p["fs"])
    return s.permute(1, 2, 3, 0)


def _to_cl(t):
    return t.permute(1, 2, 3, 0)


def reference(c, o, device="cpu"):
    """the call in fp64 on `device`, on the exact fp32 / bf16 inputs: "ref" in the layout of gather(), "A" the magnitude the fp32 term of the
    bound scales (module docstring); the plain movers: "ref" in the output's own type, compared in its bits"""
    p, f64 = c.p, torch.float64
    D = lambda t: t.to(device, f64)
    if c.fam == "norm":
        x, g = D(o["x"]), D(o["g"])
        b = D(o["b"]) if o["b"] is not None else torch.zeros((), dtype=f64, device=device)
        nrm = x.norm(dim=1, keepdim=True).clamp_min(1e-12)
        v = x / nrm * math.sqrt(p["C"]) * g + b
        ref = silu64(v) if p["silu"] else v
        A = (x.abs() / nrm * math.sqrt(p["C"]) * g.abs() + b.abs()) * (SILU_LIP if p["silu"] else 1.0)
        return {"ref": ref, "A": A}
    if c.fam in ("dupup", "avgdown"):
        x, y = D(o["x"]), D(o["y"])
        s = _shortcut64(c, x)
        m = _shortcut64(c, x.abs())                                          # dupup: |x|; avgdown: mean_g |x_g|
        return {"ref": y + s, "A": y.abs() + m}
    if c.fam == "softmax":
        n, ldp = p["n"], p["ldp"]
        S = D(o["S"])
        mx = S.max(-1, keepdim=True).values
        t = p["scale"] * (S - mx)
        e = torch.exp(t)
        pr = e / e.sum(-1, keepdim=True)
        ref, A = torch.zeros(p["R"], ldp, dtype=f64, device=device), torch.zeros(p["R"], ldp, dtype=f64, device=device)
        ref[:, :n], A[:, :n] = pr, pr * (1 + t.abs())
        return {"ref": ref, "A": A}
    if c.fam == "pack":
        x = o["x"].to(device)
        C, Cv = p["C"], p["C"] * p["ps"] ** 2
        pos = (p["T"], p["H"] // p["ps"], p["W"] // p["ps"])
        if not p["affine"]:
            ref = torch.zeros(*pos, p["Cpad"], dtype=torch.bfloat16, device=device)
            ref[..., :Cv] = _to_cl(ov.patchify(x, p["ps"])).bfloat16()
            return {"ref": ref}
        m, a = D(o["mul"]).view(C, 1, 1, 1), D(o["add"]).view(C, 1, 1, 1)
        ref, A = torch.zeros(*pos, p["Cpad"], dtype=f64, device=device), torch.zeros(*pos, p["Cpad"], dtype=f64, device=device)
        ref[..., :Cv] = _to_cl(ov.patchify(x.double() * m + a, p["ps"]))
        A[..., :Cv] = _to_cl(ov.patchify((x.double() * m).abs() + a.abs(), p["ps"]))
        return {"ref": ref, "A": A}
    if c.fam == "unpack":
        x = o["x"].to(device)
        Co = p["Cv"] // p["ps"] ** 2
        xc = ov.unpatchify(x.permute(3, 0, 1, 2).contiguous(), p["ps"])     # [Co, T, H ps, W ps]
        if not p["affine"]:
            return {"ref": (xc.clamp(-1.0, 1.0) if p["clamp"] else xc).float().contiguous()}
        s, m = D(o["sub"]).view(Co, 1, 1, 1), D(o["mul"]).view(Co, 1, 1, 1)
        ref = (xc.double() - s) * m
        return {"ref": ref.clamp(-1.0, 1.0) if p["clamp"] else ref, "A": (xc.double().abs() + s.abs()) * m.abs()}
    raise AssertionError(c.fam)


def is_plain_mover(c):
    return c.fam in ("pack", "unpack") and not c.p["affine"]


def bf16_out(c):
    return c.fam != "unpack"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def outside(c, r, got, kappa=None):
    """(elements outside the bound — a value that is not finite is outside —, worst error / bound, elements) of a kernel output `got` in the
    layout of gather(); the plain movers: elements whose bits differ; the softmax: a padding element P[:, n:ldp] whose bits are not zero
    is outside too"""
    ref = r["ref"]
    if is_plain_mover(c):
        bad = _bits(got.to(ref.dtype)) != _bits(ref)
        return int(bad.sum()), float(bad.any()), bad.numel()
    k = KAPPA[c.fam] if kappa is None else kappa
    g64 = got.to(ref.dtype)
    err = (g64 - ref).abs()
    bnd = (2.0 ** -8 * ref.abs() if bf16_out(c) else 0.0 * ref) + k * U * r["A"] + (FLOOR if c.fam == "softmax" else 0.0)
    ok = err <= bnd                                                          # NaN: not ok
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    n_out = int((~ok).sum())
    if c.fam == "softmax" and c.p["ldp"] > c.p["n"] and got.dtype == torch.bfloat16:
        n_out += int((_bits(got[:, c.p["n"]:]) != 0).sum())
    if c.fam == "pack" and c.p["Cpad"] > c.p["C"] * c.p["ps"] ** 2 and got.dtype == torch.bfloat16:
        n_out += int((_bits(got[..., c.p["C"] * c.p["ps"] ** 2:]) != 0).sum())
    return n_out, float(ratio.max()), err.numel()


def needed_kappa(c, r, raw):
    """the smallest kappa that leaves the fp32 values `raw` (emulate(raw=True): in front of the one rounding a bf16 output takes, which the
    bound's first term is for) inside kappa u A_i at every element"""
    err = (raw - r["ref"]).abs() - (FLOOR if c.fam == "softmax" else 0.0)
    A = r["A"].expand_as(err)
    return float(torch.where(err > 0, err / (U * A), torch.zeros_like(err)).max())


# ------------------------------------------------------------------------------------------------ host emulation (fp32, the kernels' order)
F32 = np.float32
FAULTS = ("neighbour_scale", "gamma_8_channels_on", "beta_dropped", "silu_skipped", "sumsq_missing_a_part", "last_vector_unwritten",
          "dupup_phase_off_by_one", "dupup_toff_ignored", "avgdown_divides_by_present_frames", "avgdown_last_phase_dropped",
          "softmax_sum_missing_a_wave", "softmax_last_column_dropped", "softmax_junk_column_counted", "softmax_padding_nonzero",
          "pack_q_r_swapped", "unpack_clamp_skipped")


def _np(t):
    return t.detach().cpu().numpy().astype(F32)


def _butterfly(v):
    """[..., L] (L a power of two) -> [...]: the xor butterfly, offsets L / 2 .. 1"""
    L = v.shape[-1]
    lanes = np.arange(L)
    off = L // 2
    while off > 0:
        v = v + v[..., lanes ^ off]
        off //= 2
    return v[..., 0]


def _round_bf16(y):
    return torch.from_numpy(np.ascontiguousarray(y, dtype=F32)).bfloat16()


def emulate(c, o, fault=None, raw=False):
    """what a correct kernel stores, by the kernel's own fp32 steps on the table's inputs (never the code under test), with correctly rounded
    exp2 and reciprocal and no fused multiply-add. `fault` injects one of FAULTS. Returns the output in the layout and the type of gather(),
    or None where the fault does not apply. raw: the fp32 value in front of the rounding to bf16, as fp64, in the layout of the reference"""
    with np.errstate(all="ignore"):
        return {"norm": _emulate_norm, "dupup": _emulate_shortcut, "avgdown": _emulate_shortcut, "softmax": _emulate_softmax, "pack": _emulate_pack,
                "unpack": _emulate_unpack}[c.fam](c, o, fault, raw)


def _out(y, raw):
    return torch.from_numpy(np.ascontiguousarray(y, dtype=F32)).double() if raw else _round_bf16(y)


def _emulate_norm(c, o, fault, raw):
    p = c.p
    M, C = p["M"], p["C"]
    applies = {None: True, "neighbour_scale": M > 1, "gamma_8_channels_on": C > 8, "beta_dropped": bool(p["beta"]), "silu_skipped": bool(p["silu"]),
               "sumsq_missing_a_part": True, "last_vector_unwritten": not raw}
    if not applies.get(fault, False):
        return None
    inst = route(c)[0]
    form, targs = inst.split("<")[0], [int(t) for t in inst.split("<")[1][:-1].split(",")]
    x, g = _np(o["x"]), _np(o["g"])
    b = _np(o["b"]) if o["b"] is not None else None
    nvec = C // 8
    xs = x.copy()
    if fault == "sumsq_missing_a_part":
        xs[:, 8 * (nvec - max(1, nvec // 4)):] = 0                          # a quarter of the row's vectors (one at the least) left out of the sum
    if form == "rms":                                                        # lane sub of LPR: vectors sub + i LPR, eight squares each, in order
        lpr, nv = targs
        xp = np.zeros((M, nv * lpr, 8), F32)
        xp[:, :nvec] = xs.reshape(M, nvec, 8)
        v = xp.reshape(M, nv, lpr, 8)
        ss = np.zeros((M, lpr), F32)
        for i in range(nv):
            for j in range(8):
                ss = ss + v[:, i, :, j] * v[:, i, :, j]
        tot = _butterfly(ss)
    elif form == "rms_g":                                                    # lane sub of G: the even and the odd elements in two sums
        G, nvl, _ = targs
        v = xs.reshape(M, nvl, G, 4, 2)
        s2 = np.zeros((M, G, 2), F32)
        for i in range(nvl):
            for j in range(4):
                s2 = s2 + v[:, i, :, j, :] * v[:, i, :, j, :]
        tot = _butterfly(s2[..., 0] + s2[..., 1])
    else:                                                                    # one partial per vector; a lane adds its row's in fours, in order
        v = xs.reshape(M, nvec, 4, 2)
        s2 = np.zeros((M, nvec, 2), F32)
        for j in range(4):
            s2 = s2 + v[:, :, j, :] * v[:, :, j, :]
        q = (s2[..., 0] + s2[..., 1]).reshape(M, nvec // 4, 4)
        tot = np.zeros((M,), F32)
        for k in range(nvec // 4):
            tot = tot + ((q[:, k, 0] + q[:, k, 1]) + (q[:, k, 2] + q[:, k, 3]))
    inv = (np.sqrt(F32(C)) / np.maximum(np.sqrt(tot), F32(1e-12))).astype(F32)
    if fault == "neighbour_scale":
        inv = np.roll(inv, -1)
    if fault == "gamma_8_channels_on":
        g = np.roll(g, -8)
    y = (x * inv[:, None]) * g[None]
    if b is not None and fault != "beta_dropped":
        y = y + b[None]
    if p["silu"] and fault != "silu_skipped":
        if form == "rms":
            y = y / (F32(1.0) + np.exp(-y).astype(F32))
        else:
            y = y * (F32(1.0) / (np.exp2(y * F32(-LOG2E)).astype(F32) + F32(1.0)))
    out = _out(y.astype(F32), raw)
    if fault == "last_vector_unwritten":
        out[:, C - 8:] = NAN
    return out


def _shortcut_index(c, device="cpu", phase_shift=0, toff=None):
    """DupUp3D: (ti [To,1,1,1], hi [1,Ho,1,1], wi [1,1,Wo,1], channel [To,Ho,Wo,Cout]) of the input element every output element adds, by the
    formula of include/yume_hip.h"""
    p = c.p
    To, Ho, Wo = dup_dims(c)
    ft, fs, Fq = p["ft"], p["fs"], p["ft"] * p["fs"] * p["fs"]
    repeats = p["Cout"] * Fq // p["Cin"]
    tt = torch.arange(To, device=device) + (p["toff"] if toff is None else toff)
    ho, wo, oc = torch.arange(Ho, device=device), torch.arange(Wo, device=device), torch.arange(p["Cout"], device=device)
    phase = ((tt % ft)[:, None, None] * fs + (ho % fs)[None, :, None]) * fs + (wo % fs)[None, None, :]
    phase = (phase + phase_shift) % Fq
    ch = (oc[None, None, None, :] * Fq + phase[..., None]) // repeats
    return (tt // ft)[:, None, None, None], (ho // fs)[None, :, None, None], (wo // fs)[None, None, :, None], ch


def _emulate_shortcut(c, o, fault, raw):
    p = c.p
    x, y = o["x"], o["y"]                                                    # fp32 torch on the host: elementwise fp32 is IEEE, no reduction is used
    if c.fam == "dupup":
        applies = {None: True, "dupup_phase_off_by_one": p["ft"] * p["fs"] ** 2 > 1, "dupup_toff_ignored": p["toff"] > 0}
        if not applies.get(fault, False):
            return None
        ti, hi, wi, ch = _shortcut_index(c, phase_shift=1 if fault == "dupup_phase_off_by_one" else 0, toff=0 if fault == "dupup_toff_ignored" else None)
        v = y + x[ti, hi, wi, ch]
        return v.double() if raw else v.bfloat16()
    To, Ho, Wo, padt = avg_dims(c)
    ft, fs, Fq = p["ft"], p["fs"], p["ft"] * p["fs"] * p["fs"]
    G = p["Cin"] * Fq // p["Cout"]
    applies = {None: True, "avgdown_divides_by_present_frames": padt > 0, "avgdown_last_phase_dropped": Fq > 1}
    if not applies.get(fault, False):
        return None
    to, ho, wo, oc = torch.arange(To), torch.arange(Ho), torch.arange(Wo), torch.arange(p["Cout"])
    s = torch.zeros(To, Ho, Wo, p["Cout"])
    present = torch.zeros(To, 1, 1, p["Cout"])
    for g in range(G):
        idx = oc * G + g
        ci, ph = idx // Fq, idx % Fq
        cc, b, a = ph % fs, (ph // fs) % fs, ph // (fs * fs)
        tsrc = to[:, None] * ft + a[None, :] - padt                          # [To, Cout]
        live = tsrc >= 0
        if fault == "avgdown_last_phase_dropped":
            live = live & (ph != Fq - 1)[None, :]
        val = x[tsrc.clamp_min(0)[:, None, None, :], (ho[:, None] * fs + b[None, :])[None, :, None, :], (wo[:, None] * fs + cc[None, :])[None, None, :, :],
                ci[None, None, None, :]]
        s = torch.where(live[:, None, None, :], s + val, s)
        present = present + live[:, None, None, :].float()
    div = present.clamp_min(1.0) if fault == "avgdown_divides_by_present_frames" else torch.tensor(float(G))
    v = y + s / div
    return v.double() if raw else v.bfloat16()


def _emulate_softmax(c, o, fault, raw):
    p = c.p
    R, n, lds, ldp = p["R"], p["n"], p["lds"], p["ldp"]
    applies = {None: True, "softmax_sum_missing_a_wave": True, "softmax_last_column_dropped": n > 1, "softmax_junk_column_counted": lds > n,
               "softmax_padding_nonzero": ldp > n and not raw}
    if not applies.get(fault, False):
        return None
    S = _np(o["S"])
    inst = route(c)[0]
    nuse = n - 1 if fault == "softmax_last_column_dropped" else n
    mx = S[:, :nuse].max(-1, keepdims=True)
    cc = F32(F32(p["scale"]) * F32(LOG2E))
    e = np.exp2(((S - mx) * cc).astype(F32)).astype(F32)
    e[:, nuse:] = 0
    if inst == "softmax_rows":                                               # thread t: columns t, t + 256, ...
        trips = -(-n // 256)
        ep = np.zeros((R, trips * 256), F32)
        ep[:, :n] = e
        if fault == "softmax_junk_column_counted":
            ep[:, n] = 1.0 if trips * 256 > n else 0.0
        part = np.zeros((R, 256), F32)
        for k in range(trips):
            part = part + ep[:, 256 * k:256 * (k + 1)]
    else:                                                                    # thread t: the four columns of vectors t, t + 256, ..., in order
        nv = int(inst.split("<")[1][0])
        ep = np.zeros((R, nv * 1024), F32)
        ep[:, :n] = e
        if fault == "softmax_junk_column_counted":
            ep[:, n] = 1.0                                                   # a column between n and lds, with the score of the maximum
        v = ep.reshape(R, nv, 256, 4)
        part = np.zeros((R, 256), F32)
        for k in range(nv):
            for j in range(4):
                part = part + v[:, k, :, j]
    red = _butterfly(part.reshape(R, 4, 64))                                 # [R, 4]
    tot = red[:, 0] + red[:, 1] + red[:, 2]
    if fault != "softmax_sum_missing_a_wave":
        tot = tot + red[:, 3]
    inv = (F32(1.0) / tot).astype(F32)
    full = np.zeros((R, ldp), F32)
    full[:, :n] = e * inv[:, None]
    out = _out(full, raw)
    if fault == "softmax_padding_nonzero":
        out[:, n] = 2.0 ** -133                                              # the smallest bf16 subnormal
    return out


def _patch(x, ps, swap=False):
    """[C, T, H, W] -> [T, H / ps, W / ps, C ps ps], channel c ps ps + r ps + q = x[c, t, h ps + q, w ps + r] (swap: q and r exchanged)"""
    C, T, H, W = x.shape
    v = x.reshape(C, T, H // ps, ps, W // ps, ps)
    v = v.permute(1, 2, 4, 0, 3, 5) if swap else v.permute(1, 2, 4, 0, 5, 3)
    return v.reshape(T, H // ps, W // ps, C * ps * ps)


def _emulate_pack(c, o, fault, raw):
    p = c.p
    if fault not in (None, "pack_q_r_swapped") or (fault and p["ps"] == 1) or (raw and not p["affine"]):
        return None
    x = o["x"]
    if p["affine"]:
        x = x * o["mul"].view(-1, 1, 1, 1) + o["add"].view(-1, 1, 1, 1)      # fp32: a product and a sum, each rounded
    Cv = p["C"] * p["ps"] ** 2
    out = torch.zeros(p["T"], p["H"] // p["ps"], p["W"] // p["ps"], p["Cpad"])
    out[..., :Cv] = _patch(x, p["ps"], swap=fault is not None)
    return out.double() if raw else out.bfloat16()


def _emulate_unpack(c, o, fault, raw):
    p = c.p
    if fault not in (None, "unpack_clamp_skipped") or (fault and not p["clamp"]) or (raw and not p["affine"]):
        return None
    ps, Co = p["ps"], p["Cv"] // p["ps"] ** 2
    T, H, W = p["T"], p["H"], p["W"]
    v = o["x"].reshape(T, H, W, Co, ps, ps).permute(3, 0, 1, 5, 2, 4).reshape(Co, T, H * ps, W * ps)      # channel c ps ps + r ps + q -> (h ps + q, w ps + r)
    if p["affine"]:
        v = (v - o["sub"].view(-1, 1, 1, 1)) * o["mul"].view(-1, 1, 1, 1)
    if p["clamp"] and fault is None:
        v = v.clamp(-1.0, 1.0)
    return v.double() if raw else v.contiguous()


# ------------------------------------------------------------------------------------------------ the call
def _guarded(rows, ld, dtype, device, before=1, after=1):
    """a NaN-filled [before + rows + after, ld] buffer and the view of its middle rows"""
    buf = torch.full((before + rows + after, ld), NAN, dtype=dtype, device=device)
    return buf, buf[before:before + rows]


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _mask(buf, rows, cols):
    mask = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    mask[1:1 + rows, :cols] = True
    return mask


def run_case(c, o, device="cuda", inplace=None):
    """one call of the raw C-ABI -> {"out": (buffer, mask of the elements the call stores)}; every buffer NaN outside what the call reads
    and stores: the rows in front and behind, the stride gaps of inputs and outputs, the score columns n .. lds. inplace: override the norm
    row's own choice (the bit-equality test runs both)"""
    from yume_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    p = c.p
    dv = lambda t: t.to(device) if t is not None else None
    if c.fam == "norm":
        M, C = p["M"], p["C"]
        ldx, ldy = norm_strides(c)
        inpl = p["inplace"] if inplace is None else inplace
        xb, xv = _guarded(M, ldx, torch.bfloat16, device)
        xv[:, :C] = dv(o["x"]).bfloat16()
        if inpl:
            yb, yv, ldy = xb, xv, ldx
        else:
            yb, yv = _guarded(M, ldy, torch.bfloat16, device)
        g, b = dv(o["g"]), dv(o["b"])
        _lib.check(lib.yume_vae_rmsnorm_silu(_vp(xv), ldx, M, C, _vp(g), _vp(b), p["silu"], _vp(yv), ldy, st), "yume_vae_rmsnorm_silu")
        return {"out": (yb, _mask(yb, M, C))}
    if c.fam in ("dupup", "avgdown"):
        if c.fam == "dupup":
            To, Ho, Wo = dup_dims(c)
        else:
            To, Ho, Wo, _ = avg_dims(c)
        ldx, ldy = p["Cin"] + p["ldx_x"], p["Cout"] + p["ldy_x"]
        nin, nout = p["Tin"] * p["Hin"] * p["Win"], To * Ho * Wo
        xb, xv = _guarded(nin, ldx, torch.bfloat16, device)
        xv[:, :p["Cin"]] = dv(o["x"]).bfloat16().view(nin, p["Cin"])
        yb, yv = _guarded(nout, ldy, torch.bfloat16, device)
        yv[:, :p["Cout"]] = dv(o["y"]).bfloat16().view(nout, p["Cout"])
        if c.fam == "dupup":
            rc = lib.yume_vae_dupup_add(_vp(xv), ldx, p["Tin"], p["Hin"], p["Win"], p["Cin"], _vp(yv), ldy, To, p["Cout"], p["ft"], p["fs"], p["toff"], st)
        else:
            rc = lib.yume_vae_avgdown_add(_vp(xv), ldx, p["Tin"], p["Hin"], p["Win"], p["Cin"], _vp(yv), ldy, p["Cout"], p["ft"], p["fs"], st)
        _lib.check(rc, "yume_vae_" + c.fam + "_add")
        return {"out": (yb, _mask(yb, nout, p["Cout"]))}
    if c.fam == "softmax":
        R, n, lds, ldp = p["R"], p["n"], p["lds"], p["ldp"]
        s0 = 64 + p["soff"]                                                  # allocations start on 256 bytes: S is 16-byte aligned iff soff % 4 == 0
        Sb = torch.full((s0 + (R + 1) * lds + 8,), NAN, dtype=torch.float32, device=device)
        Sv = torch.as_strided(Sb, (R, lds), (lds, 1), s0)
        Sv[:, :n] = dv(o["S"])                                               # the columns n .. lds stay NaN
        Pb = torch.full((64 + (R + 1) * ldp + 8,), NAN, dtype=torch.bfloat16, device=device)
        Pv = torch.as_strided(Pb, (R, ldp), (ldp, 1), 64)
        mask = torch.zeros(Pb.shape, dtype=torch.bool, device=device)
        mask[64:64 + R * ldp] = True
        assert (Sv.data_ptr() % 16 == 0) == softmax_aligned(c) and Pv.data_ptr() % 8 == 0
        _lib.check(lib.yume_softmax_rows(_vp(Sv), lds, R, n, p["scale"], _vp(Pv), ldp, st), "yume_softmax_rows")
        return {"out": (Pb, mask)}
    if c.fam == "pack":
        x = dv(o["x"]).contiguous()
        if p["bf16"]:
            x = x.bfloat16()
        npos = p["T"] * (p["H"] // p["ps"]) * (p["W"] // p["ps"])
        ob, ov_ = _guarded(npos, p["Cpad"], torch.bfloat16, device)
        mul, add = dv(o["mul"]), dv(o["add"])
        rc = lib.yume_vae_pack_input(_vp(x), int(p["bf16"]), p["C"], p["T"], p["H"], p["W"], p["ps"], _vp(mul), _vp(add), _vp(ov_), p["Cpad"], st)
        _lib.check(rc, "yume_vae_pack_input")
        return {"out": (ob, _mask(ob, npos, p["Cpad"]))}
    if c.fam == "unpack":
        npos, ldx = p["T"] * p["H"] * p["W"], p["Cv"] + p["ldx_x"]
        xb, xv = _guarded(npos, ldx, torch.bfloat16, device)
        xv[:, :p["Cv"]] = dv(o["x"]).bfloat16().view(npos, p["Cv"])
        total = p["Cv"] * npos
        ob = torch.full((total + 128,), NAN, dtype=torch.float32, device=device)
        mask = torch.zeros(ob.shape, dtype=torch.bool, device=device)
        mask[64:64 + total] = True
        sub, mul = dv(o["sub"]), dv(o["mul"])
        lo, hi = (-1.0, 1.0) if p["clamp"] else (0.0, 0.0)
        rc = lib.yume_vae_unpack_output(_vp(xv), ldx, p["T"], p["H"], p["W"], p["Cv"], p["ps"], _vp(sub), _vp(mul), lo, hi, _vp(ob[64:]), st)
        _lib.check(rc, "yume_vae_unpack_output")
        return {"out": (ob, mask)}
    raise AssertionError(c.fam)


def gather(c, bufs, r):
    """what the call stored, in the layout of reference()["ref"]"""
    buf, mask = bufs["out"]
    return buf[mask].view(r["ref"].shape)


def guards_damaged(bufs):
    """number of elements outside the stored region that no longer hold NaN"""
    buf, mask = bufs["out"]
    return int((~torch.isnan(buf) & ~mask).sum())


def main(argv):
    if argv not in (["--routes"], ["--norm-bound"]):
        sys.exit(__doc__)
    bad = 0
    for c in CASES:
        if argv == ["--norm-bound"] and c.fam != "norm":
            continue
        o = make_case(c)
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {c.name}\n")
        sys.stderr.flush()
        bufs = run_case(c, o)
        torch.cuda.synchronize()
        if argv == ["--norm-bound"]:
            r = reference(c, o, "cuda")
            n_out, worst, n = outside(c, r, gather(c, bufs, r))
            print(f"{c.name}: worst error / bound {worst:.3f}; {n_out} of {n} elements outside; guards damaged {guards_damaged(bufs)}")
            bad += n_out + guards_damaged(bufs)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main(sys.argv[1:])
