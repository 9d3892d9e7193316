"""The case table of the norm, RoPE and glue kernels between the GEMMs and the attention of every DiT block and of the T5 encoder
(csrc/norm.hip, csrc/misc.hip, softmax_bias_kernel of csrc/vae_ops.hip), their fp64 reference, the per-element error bound and a host fp32
emulation of the kernels' arithmetic in their own order (no test functions in here).

tests/test_norm_routes_gpu.py runs one call per CASES row and holds EVERY output element to `outside()` against `reference()`, with NaN
around every output and in every stride gap; tests/test_norm_cases_cpu.py proves the table, the route mirror, the reference, the bound and
the faults it flags on the host. profiles/r14_norm_routes.md has the derivation and the figures.

The bound, per element, with u = 2^-24 (fp32) and the family's kappa (KAPPA, fixed against `emulate()` with a factor 2 on top):

    bf16 output     2^-8 |ref| + kappa u A_i                one rounding to nearest even of the fp32 value
    fp32 output     kappa u A_i
    out_kind 2      hi == hi2 in their bits; |hi + lo - ref| <= 2^-16 |ref| + kappa u A_i; hi inside the bf16 bound
    movers          the bits of the input (rounded to bf16, nearest even, where the kernel rounds)

A_i = the sum of the absolute values of what is added and cancelled on the way to element i:

    adaLN           (|x_i - mu| + mean_j |x_j|) rstd |g_i| + |a_i|         g = mul + add_one; mean_j |x_j| carries the error of the fp32 mean
    rmsnorm_f32     |x_i| rstd |w_i|
    RMSNorm(+RoPE)  |y_0 c| + |y_1 s| (resp. |y_0 s| + |y_1 c|), y = x r w; without RoPE |y_i|
    softmax         p_i (1 + |s_i| + |b_i| + |v_i| + |max| + |v_i - max|), v = s + b; + 2^-126 (what underflows is flushed)
    small-M linear  sum_k |act(x_k) w_k| + |b| + |ref - add| + |add| + |ref|
    sinusoidal      2^-24 |ref| + 2^-40 (fp64 on the device, one rounding to fp32; the device's pow and cos are not the host's to the ulp)

    python tests/norm_cases.py --routes        one call per logged case, `CASE <name>` on stderr before each (YUME_NORM_LOG=1 names the kernels)
"""
import ctypes
import os
import sys
import zlib
from collections import namedtuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NT = 256
U = 2.0 ** -24
FLOOR = 2.0 ** -126
NAN = float("nan")
# fixed against emulate() on the table's own inputs: the smallest value that leaves its fp32 values with zero elements outside (adaLN 4.20,
# rmsnorm_f32 4.18, RMSNorm+RoPE 5.64, softmax 0.86, linear 1.13), times 2, rounded up to a whole number (profiles/r14_norm_routes.md)
KAPPA = {"adaln": 9.0, "rms": 9.0, "rope": 12.0, "periodic": 12.0, "softmax": 2.0, "linear": 3.0}

LOGGED = ("adaln", "rms", "rope", "periodic")
MOVERS = ("modtab", "cast", "transpose", "gather", "unpatch")
Case = namedtuple("Case", "name fam route p")
ROUTES = ("adaln2", "adaln<3>", "adaln<5>", "adaln<8>", "adaln_rms<3>", "adaln_rms<5>", "adaln_rms<8>", "rope2<2>", "rope2<3>", "rope<2>",
          "rope<3>", "rope<5>", "rope<8>")


def _adaln(name, route, T, C, kind=0, add_one=1, ridx="none", affine=False, ldx_x=0, ldo_x=0, eps=1e-6):
    return Case(name, "adaln", route, dict(T=T, C=C, kind=kind, add_one=0 if affine else add_one, ridx=ridx, affine=affine, ldx_x=ldx_x, ldo_x=ldo_x,
                                           eps=1e-5 if affine else eps))


def _rms(name, route, T, C, ldx_x=0, ldo_x=0):
    return Case(name, "rms", route, dict(T=T, C=C, ldx_x=ldx_x, ldo_x=ldo_x, eps=1e-6))


def _rope(name, route, T, C, nparts, rope=True, eps=1e-6, ld_x=0, n_rope=None):
    return Case(name, "rope", route, dict(T=T, C=C, nparts=nparts, rope=rope, eps=eps, ld_x=ld_x, n_rope=n_rope, wperiod=1))


def _per(name, route, T, C, wperiod, eps=1e-6, ld_x=0):
    return Case(name, "periodic", route, dict(T=T, C=C, nparts=1, rope=False, eps=eps, ld_x=ld_x, n_rope=None, wperiod=wperiod))


def _smax(name, n, ldp, H, lds_x=0, gap=0):
    return Case(name, "softmax", "softmax_bias", dict(n=n, ldp=ldp, H=H, lds_x=lds_x, gap=gap))


def _lin(name, R, K, N, wbf16=False, in_act=1, out_act=1, bias=True, add=True):
    return Case(name, "linear", "linear_smallm", dict(R=R, K=K, N=N, wbf16=wbf16, in_act=in_act, out_act=out_act, bias=bias, add=add))


def _mv(name, fam, **p):
    return Case(name, fam, fam, p)


CASES = [
    # ---- yume_adaln_modulate: the first and last width of MAXV 3, 5 and 8; T around the two-row threshold
    _adaln("adaln_c8_t1", "adaln<3>", 1, 8),                                             # 254 idle threads
    _adaln("adaln_c8_t1025_idx_odd", "adaln2", 1025, 8, ridx="odd", ldx_x=4, ldo_x=4),
    _adaln("adaln_c1280_t7_idx_nonmono", "adaln<3>", 7, 1280, ridx="nonmono", ldx_x=4, ldo_x=8),
    _adaln("adaln_c1280_t1024_idx_even", "adaln2", 1024, 1280, ridx="even"),
    _adaln("adaln_c3072_t1023_idx_odd", "adaln<3>", 1023, 3072, ridx="odd", ldx_x=8, ldo_x=4),   # the last one-row launch
    _adaln("adaln_c3072_t1024", "adaln2", 1024, 3072, add_one=0, ldx_x=4, ldo_x=4),              # the first two-row launch
    _adaln("adaln_c3072_t1025_idx_odd", "adaln2", 1025, 3072, ridx="odd", ldx_x=4, ldo_x=8),    # odd T, a mixed pair
    _adaln("adaln_c3072_t1025_idx_nonmono", "adaln2", 1025, 3072, ridx="nonmono"),
    _adaln("adaln_c3072_t1025_idx_even", "adaln2", 1025, 3072, ridx="even", ldo_x=4),
    _adaln("adaln_c3072_t1024_f32_stays_one_row", "adaln<3>", 1024, 3072, kind=1, ridx="odd", ldo_x=4),
    _adaln("adaln_c1280_t1025_split3_stays_one_row", "adaln<3>", 1025, 1280, kind=2, ridx="odd", ldx_x=4, ldo_x=8),
    _adaln("adaln_c3072_t7_split3", "adaln<3>", 7, 3072, kind=2, ldo_x=8),
    _adaln("adaln_c3072_t7_affine", "adaln<3>", 7, 3072, affine=True, ldx_x=4),
    _adaln("adaln_c1280_t1025_affine", "adaln2", 1025, 1280, affine=True, ldo_x=4),
    _adaln("adaln_c3080_t7", "adaln<5>", 7, 3080, ridx="nonmono", ldx_x=4, ldo_x=4),            # first width of MAXV 5
    _adaln("adaln_c3080_t1024_one_row", "adaln<5>", 1024, 3080, ridx="odd"),                    # T >= 1024 beyond 3072: one row
    _adaln("adaln_c5120_t7_f32", "adaln<5>", 7, 5120, kind=1, add_one=0, ridx="even", ldo_x=4),
    _adaln("adaln_c5120_t1_split3", "adaln<5>", 1, 5120, kind=2, ldo_x=8),
    _adaln("adaln_c5128_t7", "adaln<8>", 7, 5128, ridx="odd", ldx_x=8, ldo_x=8),                # first width of MAXV 8
    _adaln("adaln_c8192_t7_idx_nonmono", "adaln<8>", 7, 8192, ridx="nonmono", ldx_x=4, ldo_x=4),
    _adaln("adaln_c8192_t1_f32", "adaln<8>", 1, 8192, kind=1),
    _adaln("adaln_c8192_t7_split3_affine", "adaln<8>", 7, 8192, kind=2, affine=True, ldo_x=8),
    # ---- yume_rmsnorm_f32 (adaln_kernel<*, true>)
    _rms("rms_c8_t1", "adaln_rms<3>", 1, 8),
    _rms("rms_c8_t512", "adaln_rms<3>", 512, 8, ldx_x=4, ldo_x=4),
    _rms("rms_c3072_t512", "adaln_rms<3>", 512, 3072, ldx_x=4, ldo_x=8),
    _rms("rms_c4096_t1", "adaln_rms<5>", 1, 4096),
    _rms("rms_c4096_t512", "adaln_rms<5>", 512, 4096, ldx_x=8, ldo_x=4),                        # the umT5-XXL width
    _rms("rms_c8192_t1", "adaln_rms<8>", 1, 8192, ldo_x=4),
    _rms("rms_c8192_t512", "adaln_rms<8>", 512, 8192, ldx_x=4),
    # ---- yume_rmsnorm_rope: nvec = nparts * C / 8 of 64, 512 (NV 2), 640, 768 (NV 3), 896, 1280 (NV 5), 1408, 2048 (NV 8)
    _rope("rope_nv64_t1", "rope<2>", 1, 512, 1),
    _rope("rope_nv64_t1024", "rope2<2>", 1024, 512, 1, ld_x=8),
    _rope("rope_nv512_t1023", "rope<2>", 1023, 2048, 2, ld_x=64),
    _rope("rope_nv512_t1025", "rope2<2>", 1025, 2048, 2, ld_x=8),
    _rope("rope_nv512_p1_t1_norope", "rope<2>", 1, 4096, 1, rope=False),
    _rope("rope_nv640_t1024", "rope2<3>", 1024, 5120, 1, ld_x=8),
    _rope("rope_nv768_t1023", "rope<3>", 1023, 3072, 2),
    _rope("rope_nv768_t1025", "rope2<3>", 1025, 3072, 2, ld_x=3072),                            # the block's own call: q | k of the [T, 3C] projection
    _rope("rope_nv768_t1025_norope", "rope2<3>", 1025, 3072, 2, rope=False),
    _rope("rope_nv768_t1025_noeps", "rope2<3>", 1025, 3072, 2, eps=-1.0, ld_x=8),               # qk_norm=False
    _rope("rope_nv768_split_call", "rope2<3> rope<3>", 1030, 3072, 2, n_rope=1025, ld_x=8),    # qk[:n_rope] with RoPE, qk[n_rope:] without
    _rope("rope_nv896_t1", "rope<5>", 1, 3584, 2),
    _rope("rope_nv896_t1024", "rope<5>", 1024, 3584, 2, ld_x=8),                                # T >= 1024 beyond 768 vectors: one row
    _rope("rope_nv1280_t3_noeps", "rope<5>", 3, 5120, 2, eps=-1.0),
    _rope("rope_nv1408_t1", "rope<8>", 1, 5632, 2, ld_x=8),
    _rope("rope_nv1408_t1024", "rope<8>", 1024, 5632, 2),
    _rope("rope_nv2048_t3", "rope<8>", 3, 8192, 2, ld_x=8),
    _rope("rope_nv1024_p1_t3_norope", "rope<5>", 3, 8192, 1, rope=False),
    # ---- yume_rmsnorm_rows_periodic
    _per("periodic_w1_t1024", "rope2<2>", 1024, 512, 1),                                        # wperiod 1 falls into the two-row kernel
    _per("periodic_w2_t1025", "rope<2>", 1025, 512, 2, ld_x=8),                                 # wperiod > 1 never does
    _per("periodic_w30_t61", "rope<3>", 61, 5120, 30),                                          # 30 blocks' K in one launch; 61 % 30 = 1
    _per("periodic_w30_t61_noeps", "rope<2>", 61, 512, 30, eps=-1.0, ld_x=8),
    # ---- yume_softmax_bias_rows (one wave per row)
    _smax("softmax_n1", 1, 1, 1),
    _smax("softmax_n1_ldp64", 1, 64, 3, gap=8),
    _smax("softmax_n63_ldp64", 63, 64, 3, lds_x=1, gap=64),
    _smax("softmax_n64", 64, 64, 1),
    _smax("softmax_n65_ldp128", 65, 128, 3, lds_x=63),
    _smax("softmax_n65_ldp65", 65, 65, 1, gap=3),
    _smax("softmax_n512_ldp1024", 512, 1024, 3, gap=64),                                        # the encoder's own length
    _smax("softmax_n1000_ldp1024", 1000, 1024, 1, lds_x=24),
    _smax("softmax_n1000_ldp1000", 1000, 1000, 3),
    _smax("softmax_n1024", 1024, 1024, 3, gap=64),
    # ---- yume_linear_smallm_f32
    _lin("linear_r3_k256_n520_all", 3, 256, 520),
    _lin("linear_r3_k256_n520_no_in_act", 3, 256, 520, in_act=0),
    _lin("linear_r3_k256_n520_no_out_act", 3, 256, 520, out_act=0),
    _lin("linear_r3_k256_n520_no_bias", 3, 256, 520, bias=False),
    _lin("linear_r3_k256_n520_no_add", 3, 256, 520, add=False),
    _lin("linear_r1_k8_n1", 1, 8, 1),                                                           # one lane works
    _lin("linear_r8_k520_n3_bf16", 8, 520, 3, wbf16=True),                                      # lane 0 makes a second trip; N % 4 = 3
    _lin("linear_r8_k4096_n3", 8, 4096, 3, out_act=0),
    _lin("linear_r1_k4096_n520_bf16", 1, 4096, 520, wbf16=True, in_act=0, add=False),
    _lin("linear_r3_k8_n520_bf16", 3, 8, 520, wbf16=True, bias=False),
    # ---- yume_sinusoidal_embed
    Case("sinus_dim2", "sinus", "sinus", dict(R=5, dim=2, index=False)),
    Case("sinus_dim256", "sinus", "sinus", dict(R=7, dim=256, index=False)),
    Case("sinus_dim256_index", "sinus", "sinus", dict(R=300, dim=256, index=True)),
    Case("sinus_dim2_index", "sinus", "sinus", dict(R=3, dim=2, index=True)),
    # ---- the bit-exact movers: one row each beyond the block cap x 256 (a second trip of the stride loop), gaps, ragged edges
    _mv("modtab_small", "modtab", B=1, R=1, W=4),
    _mv("modtab_two_trips", "modtab", B=3, R=30, W=48000),                                      # 1 080 000 vectors > 4096 x 256
    _mv("cast_small_rows_valid", "cast", rows=5, rows_valid=3, cols=12, ldi_x=4, ldo_x=8),
    _mv("cast_two_trips_rows_valid", "cast", rows=1030, rows_valid=1000, cols=8192, ldi_x=4, ldo_x=8),   # 2 109 440 vectors > 8192 x 256
    _mv("transpose_f32_ragged", "transpose", rows=77, cols=45, bf16=False, ldi_x=3, ldo_x=5),
    _mv("transpose_bf16_ragged", "transpose", rows=45, cols=77, bf16=True, ldi_x=1, ldo_x=3),
    _mv("transpose_bf16_one", "transpose", rows=1, cols=1, bf16=True, ldi_x=0, ldo_x=0),
    _mv("gather_f32_ragged", "gather", Cin=5, F=4, H=7, W=9, f0=1, nf=2, kh=2, kw=2, Kp=24, bf16=False),
    _mv("gather_bf16_two_trips", "gather", Cin=70, F=3, H=5, W=7, f0=1, nf=2, kh=2, kw=2, Kp=288, bf16=True),   # Kp > 256 columns
    _mv("gather_f32_two_trips", "gather", Cin=33, F=2, H=4, W=6, f0=1, nf=1, kh=2, kw=4, Kp=272, bf16=False),   # W % kw != 0
    _mv("unpatch_small", "unpatch", Fr=1, Hp=2, Wp=3, ph=1, pw=2, Cout=3, ldi_x=2),
    _mv("unpatch_two_trips", "unpatch", Fr=11, Hp=37, Wp=41, ph=2, pw=2, Cout=16, ldi_x=4),     # 1 067 968 elements > 4096 x 256
]
BY_NAME = {c.name: c for c in CASES}


# ------------------------------------------------------------------------------------------------ the dispatcher's mirror
def route(c):
    """the kernel instances the call launches, in order, as YUME_NORM_LOG names them: the conditions of yume_adaln_modulate,
    yume_rmsnorm_f32 and rmsnorm_rope_impl (csrc/norm.hip), restated"""
    p = c.p
    if c.fam == "adaln":
        if p["C"] <= NT * 4 * 3 and p["kind"] == 0 and p["T"] >= 1024:
            return ("adaln2",)
        return ("adaln<%d>" % (3 if p["C"] <= NT * 12 else 5 if p["C"] <= NT * 20 else 8),)
    if c.fam == "rms":
        return ("adaln_rms<%d>" % (3 if p["C"] <= NT * 12 else 5 if p["C"] <= NT * 20 else 8),)
    if c.fam in ("rope", "periodic"):
        nvec = p["C"] // 8 * p["nparts"]

        def one(T):
            if p["wperiod"] == 1 and nvec <= NT * 3 and T >= 1024:
                return "rope2<%d>" % (2 if nvec <= NT * 2 else 3)
            return "rope<%d>" % (2 if nvec <= NT * 2 else 3 if nvec <= NT * 3 else 5 if nvec <= NT * 5 else 8)
        if p["n_rope"] is not None:
            return (one(p["n_rope"]), one(p["T"] - p["n_rope"]))
        return (one(p["T"]),)
    return (c.fam if c.fam in MOVERS or c.fam == "sinus" else c.route,)


def maxv(c):
    return int(route(c)[0].split("<")[1][0]) if "<" in route(c)[0] else 3


def kernel_of(line):
    """`[norm] <instance> T=.. ...` -> <instance>"""
    return line.split()[1]


def log_fields(c):
    """what the YUME_NORM_LOG lines of the call carry beside the instance, one dict per launch"""
    p = c.p
    if c.fam == "adaln":
        ldx, ldo = adaln_strides(c)
        return [dict(T=p["T"], C=p["C"], nparts=1, out_kind=p["kind"], ldx=ldx, ldo=ldo, tab_stride=0 if p["affine"] else 6 * p["C"], wperiod=1, rope=0,
                     row_idx=int(p["ridx"] != "none"))]
    if c.fam == "rms":
        return [dict(T=p["T"], C=p["C"], nparts=1, out_kind=0, ldx=p["C"] + p["ldx_x"], ldo=p["C"] + p["ldo_x"], tab_stride=0, wperiod=1, rope=0, row_idx=0)]
    ld = p["nparts"] * p["C"] + p["ld_x"]
    base = dict(C=p["C"], nparts=p["nparts"], out_kind=0, ldx=ld, ldo=ld, tab_stride=0, wperiod=p["wperiod"], row_idx=0)
    if p["n_rope"] is not None:
        return [dict(base, T=p["n_rope"], rope=1), dict(base, T=p["T"] - p["n_rope"], rope=0)]
    return [dict(base, T=p["T"], rope=int(p["rope"]))]


# ------------------------------------------------------------------------------------------------ operands
def _gen(c):
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.encode()))


def _bf16_exact(t):
    return t.bfloat16().float()


def adaln_strides(c):
    p = c.p
    return p["C"] + p["ldx_x"], (3 * p["C"] if p["kind"] == 2 else p["C"]) + p["ldo_x"]


def row_index(c):
    """int32 [T] modulation row of every token, or None. "even": one boundary on an even row; "odd": boundaries on odd rows (the two rows of
    a workgroup differ there); "nonmono": no order at all"""
    T, kind = c.p["T"], c.p["ridx"]
    t = torch.arange(T)
    if kind == "none":
        return None
    if kind == "even":
        return (t >= (T // 2) // 2 * 2).to(torch.int32)
    if kind == "odd":
        b1, b2 = (T // 3) // 2 * 2 + 1, (2 * T // 3) // 2 * 2 + 1
        return ((t >= b1).int() + (t >= b2).int()).to(torch.int32)
    return ((t * 7 + 3) % 5).to(torch.int32)


def special_rows(x, eps, center=True):
    """rows 1..4 of an input of seven rows or more: a constant row (variance 0: eps decides), a row of variance near eps, a row with
    mean / std = 2^10 (no mean for the RMS forms: |x| = 2^10 times the others'), an all-zero row"""
    if x.shape[0] >= 7:
        x[1] = 3.0 if center else 0.0
        x[2] = (1.0 if center else 0.0) + x[2] * eps ** 0.5
        x[3] = (1024.0 + x[3]) if center else 1024.0 * x[3]
        x[4] = 0.0
        if not center:
            x[1, ::2] = 2.0 ** -3                # a row of one value, sign alternating
            x[1, 1::2] = -2.0 ** -3
    return x


def make_case(c, device="cpu"):
    """seeded operands, drawn on the CPU generator, fp32 on the host (bf16-exact where the call takes bf16); under "dev" what the call takes"""
    g, p = _gen(c), c.p
    o = {}
    if c.fam in ("adaln", "rms"):
        T, C = p["T"], p["C"]
        o["x"] = special_rows(torch.randn(T, C, generator=g), p["eps"], center=c.fam == "adaln")
        if c.fam == "rms":
            o["w"] = torch.randn(C, generator=g)
        elif p["affine"]:
            o["w"], o["b"] = torch.randn(C, generator=g), torch.randn(C, generator=g)
        else:
            o["idx"] = row_index(c)
            R = 1 if o["idx"] is None else int(o["idx"].max()) + 1
            o["tab"] = torch.randn(R, 6, C, generator=g)                     # the blocks' table: shift = chunk 0, scale = chunk 1
    elif c.fam in ("rope", "periodic"):
        T, C, nparts = p["T"], p["C"], p["nparts"]
        x = torch.randn(T, nparts, C, generator=g)
        if nparts == 2:
            x[:, 1] *= 8.0                                                   # a swapped sum of squares shows
        x = special_rows(x.view(T, nparts * C), abs(p["eps"]), center=False)
        o["x"] = _bf16_exact(x)
        o["w"] = torch.randn(p["wperiod"], nparts * C, generator=g)
        nr = p["n_rope"] if p["n_rope"] is not None else T
        if p["rope"]:
            th = (torch.arange(nr * 64, dtype=torch.float64) * 0.0137).view(nr, 64)       # every pair its own angle, in a row and between rows
            o["rope"] = torch.stack([th.cos(), th.sin()], dim=-1).float()    # the fp32 table as stored
    elif c.fam == "softmax":
        H, n = p["H"], p["n"]
        o["S"] = torch.randn(H, n, n, generator=g) * 30.0                    # wide: exp(v - max) underflows for some
        bias = torch.randn(H, 2 * n - 1, generator=g)
        for h in range(H):                                                   # one dominant diagonal j - i = d_h
            bias[h, min(max(n - 1 + (2, -1, 0)[h], 0), 2 * n - 2)] += 40.0
        o["bias"] = bias
    elif c.fam == "linear":
        R, K, N = p["R"], p["K"], p["N"]
        o["x"] = torch.randn(R, K, generator=g) * 2.0
        w = torch.randn(N, K, generator=g) * K ** -0.5
        o["w"] = _bf16_exact(w) if p["wbf16"] else w
        o["bias"] = torch.randn(N, generator=g) if p["bias"] else None
        o["add"] = torch.randn(N, generator=g) if p["add"] else None
    elif c.fam == "sinus":
        o["t"] = torch.cat([torch.tensor([0.0, 1000.0, 999.5]), torch.rand(61, generator=g, dtype=torch.float64) * 1000.0])
        o["idx"] = torch.randint(0, 64, (p["R"],), generator=g).to(torch.int32) if p["index"] else None
    elif c.fam == "modtab":
        o["tab"], o["e0"] = torch.randn(p["B"], p["W"], generator=g), torch.randn(p["R"], p["W"], generator=g)
    elif c.fam == "cast":
        o["x"] = torch.randn(p["rows"], p["cols"], generator=g)
    elif c.fam == "transpose":
        x = torch.randn(p["rows"], p["cols"], generator=g)
        o["x"] = _bf16_exact(x) if p["bf16"] else x
    elif c.fam == "gather":
        x = torch.randn(p["Cin"], p["F"], p["H"], p["W"], generator=g)
        o["x"] = _bf16_exact(x) if p["bf16"] else x
    elif c.fam == "unpatch":
        o["x"] = torch.randn(p["Fr"] * p["Hp"] * p["Wp"], p["ph"] * p["pw"] * p["Cout"], generator=g)
    else:
        raise AssertionError(c.fam)
    o["device"] = device
    return o


def mod_rows(c, o, idx=None):
    """(mul rows, add rows) [T, C] (or [1, C]) fp32 as the call reads them, for the row index `idx` (the case's own by default)"""
    if c.p["affine"]:
        return o["w"][None], o["b"][None]
    idx = o["idx"] if idx is None else idx
    sel = idx.long() if idx is not None else torch.zeros(c.p["T"], dtype=torch.long)
    return o["tab"][sel, 1], o["tab"][sel, 0]


def rope_weight_rows(c, o, div=False):
    T, wp = c.p["T"], c.p["wperiod"]
    t = torch.arange(T)
    return o["w"][torch.clamp(t // wp, max=wp - 1) if div else t % wp]


def rope_table(c, o):
    """[T, 64, 2] (cos, sin); rows past n_rope (and every row without RoPE) are the identity rotation"""
    T = c.p["T"]
    tab = torch.zeros(T, 64, 2)
    tab[..., 0] = 1.0
    if c.p["rope"]:
        tab[:o["rope"].shape[0]] = o["rope"]
    return tab


# ------------------------------------------------------------------------------------------------ reference (fp64) and bound
def silu64(x):
    return x / (1 + torch.exp(-x))


def reference(c, o, device="cpu"):
    """the call in fp64 on `device`, on the exact fp32 / bf16 inputs: "ref" in the layout of gather(), "A" the magnitude the fp32 term of the
    bound scales (module docstring); the movers: "ref" in the output's own type, compared in its bits"""
    p, f64 = c.p, torch.float64
    D = lambda t: t.to(device, f64)
    if c.fam in ("adaln", "rms"):
        x = D(o["x"])
        if c.fam == "adaln":
            mu = x.mean(1, keepdim=True)
            m, a = (D(t) for t in mod_rows(c, o))
            g = m + p["add_one"]
        else:
            mu, g, a = torch.zeros((), dtype=f64, device=device), D(o["w"])[None], torch.zeros((), dtype=f64, device=device)
        d = x - mu
        rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + p["eps"])
        ref = d * rstd * g + a
        A = (d.abs() + (x.abs().mean(1, keepdim=True) if c.fam == "adaln" else 0.0)) * rstd * g.abs() + a.abs()
        return {"ref": ref, "A": A}
    if c.fam in ("rope", "periodic"):
        T, C, nparts = p["T"], p["C"], p["nparts"]
        x = D(o["x"]).view(T, nparts, C)
        r = torch.ones(T, nparts, 1, dtype=f64, device=device) if p["eps"] < 0 else 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + p["eps"])
        y = (x * r * D(rope_weight_rows(c, o)).view(T, nparts, C)).view(T, nparts * C // 128, 64, 2)
        tab = D(rope_table(c, o))[:, None]
        cs, sn = tab[..., 0], tab[..., 1]
        y0, y1 = y[..., 0], y[..., 1]
        ref = torch.stack([y0 * cs - y1 * sn, y0 * sn + y1 * cs], dim=-1)
        A = torch.stack([(y0 * cs).abs() + (y1 * sn).abs(), (y0 * sn).abs() + (y1 * cs).abs()], dim=-1)
        return {"ref": ref.view(T, nparts * C), "A": A.view(T, nparts * C)}
    if c.fam == "softmax":
        H, n, ldp = p["H"], p["n"], p["ldp"]
        S, b = D(o["S"]), D(o["bias"])
        i, j = torch.arange(n, device=device)[:, None], torch.arange(n, device=device)[None]
        B = b[:, j - i + n - 1]                                              # [H, n, n]
        v = S + B
        mx = v.max(-1, keepdim=True).values
        e = torch.exp(v - mx)
        pr = e / e.sum(-1, keepdim=True)
        A = pr * (1 + S.abs() + B.abs() + v.abs() + mx.abs() + (v - mx).abs())
        ref, Af = torch.zeros(H, n, ldp, dtype=f64, device=device), torch.zeros(H, n, ldp, dtype=f64, device=device)
        ref[..., :n], Af[..., :n] = pr, A
        return {"ref": ref, "A": Af}
    if c.fam == "linear":
        x, w = D(o["x"]), D(o["w"])
        xa = silu64(x) if p["in_act"] else x
        acc = xa @ w.t()
        mag = xa.abs() @ w.abs().t()
        b = D(o["bias"]) if o["bias"] is not None else torch.zeros((), dtype=f64, device=device)
        a = D(o["add"]) if o["add"] is not None else torch.zeros((), dtype=f64, device=device)
        v = acc + b
        v2 = silu64(v) if p["out_act"] else v
        ref = v2 + a
        return {"ref": ref, "A": mag + b.abs() + v2.abs() + a.abs() + ref.abs()}
    if c.fam == "sinus":
        R, dim = p["R"], p["dim"]
        half = dim // 2
        t = D(o["t"])
        pos = t[o["idx"].long().to(device)] if o["idx"] is not None else t[:R]
        w = torch.pow(torch.tensor(10000.0, dtype=f64, device=device), -torch.arange(half, dtype=f64, device=device) / half)
        a = pos[:, None] * w[None]
        return {"ref": torch.cat([a.cos(), a.sin()], dim=1), "A": None}
    # ---- the movers
    dv = lambda t: t.to(device)
    if c.fam == "modtab":
        return {"ref": (D(o["tab"])[:, None] + D(o["e0"])[None]).float()}    # one fp32 add = the fp64 sum rounded once
    if c.fam == "cast":
        ref = dv(o["x"]).bfloat16()
        ref[p["rows_valid"]:] = 0
        return {"ref": ref}
    if c.fam == "transpose":
        return {"ref": dv(o["x"]).t().contiguous().bfloat16()}
    if c.fam == "gather":
        kh, kw, f0, nf, Kp = p["kh"], p["kw"], p["f0"], p["nf"], p["Kp"]
        Cin, F, H, W = o["x"].shape
        Hp, Wp = -(-H // kh), -(-W // kw)
        xp = torch.zeros(Cin, nf, Hp * kh, Wp * kw, device=device)
        xp[:, :, :H, :W] = dv(o["x"])[:, f0:f0 + nf]
        t = xp.view(Cin, nf, Hp, kh, Wp, kw).permute(1, 2, 4, 0, 3, 5).reshape(nf * Hp * Wp, Cin * kh * kw)
        ref = torch.zeros(nf * Hp * Wp, Kp, device=device)
        ref[:, :Cin * kh * kw] = t
        return {"ref": ref.bfloat16()}
    if c.fam == "unpatch":
        Fr, Hp, Wp, ph, pw, Co = p["Fr"], p["Hp"], p["Wp"], p["ph"], p["pw"], p["Cout"]
        return {"ref": dv(o["x"]).view(Fr, Hp, Wp, ph, pw, Co).permute(5, 0, 1, 3, 2, 4).reshape(Co, Fr, Hp * ph, Wp * pw).contiguous()}
    raise AssertionError(c.fam)


def bf16_out(c):
    return c.fam in ("rms", "rope", "periodic", "softmax") or (c.fam == "adaln" and c.p["kind"] != 1)


def _terms(c, r, got):
    """[(error, part of the bound without kappa, what kappa u scales)] of every condition on the output; got in the layout of gather()"""
    ref = r["ref"]
    if c.fam == "sinus":
        return [((got - ref).abs(), U * ref.abs() + 2.0 ** -40, torch.zeros_like(ref))]
    A = r["A"].expand_as(ref)
    floor = FLOOR if c.fam == "softmax" else 0.0
    if c.fam == "adaln" and c.p["kind"] == 2:
        C = c.p["C"]
        hi, hi2, lo = got[:, :C], got[:, C:2 * C], got[:, 2 * C:]
        same = torch.where(hi == hi2, 0.0, float("inf")).to(ref.dtype)       # bf16 values: equal values are equal bits (no zero of either sign here)
        return [((hi - ref).abs() + same, 2.0 ** -8 * ref.abs(), A), ((hi + lo - ref).abs(), 2.0 ** -16 * ref.abs(), A)]
    return [((got - ref).abs(), (2.0 ** -8 * ref.abs() if bf16_out(c) else 0.0 * ref) + floor, A)]


def outside(c, r, got, kappa=None):
    """(elements outside the bound — a value that is not finite is outside —, worst error / bound, elements) of a kernel output `got`; the
    movers: elements whose bits differ"""
    if c.fam in MOVERS:
        iv = torch.int16 if r["ref"].dtype == torch.bfloat16 else torch.int32
        bad = got.contiguous().view(iv) != r["ref"].contiguous().view(iv)
        return int(bad.sum()), float(bad.any()), bad.numel()
    k = KAPPA.get(c.fam, 0.0) if kappa is None else kappa
    n_out, worst, n = 0, 0.0, 0
    for err, base, A in _terms(c, r, got.to(r["ref"].dtype)):
        bnd = base + k * U * A
        ok = err <= bnd
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)
        ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
        n_out += int((~ok).sum())
        worst = max(worst, float(ratio.max()))
        n = max(n, err.numel())
    return n_out, worst, n


def needed_kappa(c, r, raw):
    """the smallest kappa that leaves the fp32 values `raw` (emulate(raw=True): in front of the one rounding a bf16 output takes, which the
    bound's first term is for) inside kappa u A_i at every element"""
    err = (raw - r["ref"]).abs() - (FLOOR if c.fam == "softmax" else 0.0)
    A = r["A"].expand_as(err)
    return float(torch.where(err > 0, err / (U * A), torch.zeros_like(err)).max())


# ------------------------------------------------------------------------------------------------ host emulation (fp32, the kernels' order)
F32 = np.float32


def _np(t):
    return t.detach().cpu().numpy().astype(F32)


def _block_sum(part):
    """[T, 256] per-thread partials -> [T]: the xor butterfly of wave_sum inside each wave of 64, then the four waves in wave order"""
    T = part.shape[0]
    v = part.reshape(T, NT // 64, 64)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lanes ^ off]
    t = np.zeros(T, dtype=F32)
    for w in range(NT // 64):
        t = t + v[:, w, 0]
    return t


def _wave_sum(part):
    """[..., 64] -> [...]"""
    lanes = np.arange(64)
    v = part
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ off]
    return v[..., 0]


def _rsqrt(v):
    return (F32(1.0) / np.sqrt(v.astype(F32))).astype(F32)


def _round_bf16(y, trunc=False):
    """fp32 numpy -> the bf16 value as fp64 torch"""
    t = torch.from_numpy(np.ascontiguousarray(y, dtype=F32))
    if trunc:
        return (t.view(torch.int32) & -65536).view(torch.float32).double()
    return t.bfloat16().double()


def emulate(c, o, fault=None, raw=False):
    """what a correct kernel stores, by the kernel's own fp32 steps on the table's inputs (never the code under test): per-thread sums
    sequential over i, the butterfly, the waves' partials in wave order, one rounding to nearest even. `fault` injects one of FAULTS.
    Returns the output in the layout of gather() (fp64; the movers: the output's type), or None where the fault does not apply. raw: the
    fp32 value in front of the rounding to bf16, in the layout of the reference (what needed_kappa() measures the fp32 term on)."""
    p, fam = c.p, c.fam
    with np.errstate(all="ignore"):
        if fam in ("adaln", "rms"):
            return _emulate_adaln(c, o, fault, raw)
        if fam in ("rope", "periodic"):
            return _emulate_rope(c, o, fault, raw)
        if fam == "softmax":
            return _emulate_softmax(c, o, fault, raw)
        if fam == "linear":
            return _emulate_linear(c, o, fault)
    if fam == "sinus":
        return None if fault else reference(c, o)["ref"].float().double()
    return _emulate_mover(c, o, fault)


FAULTS = ("divisor_maxv", "pair_shares_mod_row", "last_odd_unwritten", "last_odd_from_t0", "part1_with_sum0", "rope_offset_from_vi", "sine_sign",
          "weight_row_div", "bf16_trunc", "lo_from_trunc_hi", "eps_dropped", "noeps_normalises", "in_act_row0_only", "k_tail_dropped",
          "bias_index_off_by_one", "padding_unzeroed", "rows_valid_ignored", "one_trip")


def _two_row(c):
    return any(k.startswith(("adaln2", "rope2")) for k in route(c))


def _emulate_adaln(c, o, fault, raw=False):
    p = c.p
    T, C, rms = p["T"], p["C"], c.fam == "rms"
    kind = 0 if rms else p["kind"]
    mv = maxv(c)
    applies = {None: True, "divisor_maxv": True, "pair_shares_mod_row": _two_row(c) and not rms and not p["affine"] and p["ridx"] != "none",
               "last_odd_unwritten": _two_row(c) and T % 2 == 1, "last_odd_from_t0": _two_row(c), "bf16_trunc": kind != 1,
               "lo_from_trunc_hi": kind == 2, "eps_dropped": True}
    if not applies.get(fault, False):
        return None
    x = _np(o["x"])
    if rms:
        m, a, one = _np(o["w"])[None], np.zeros((1, C), F32), F32(0)
    else:
        idx = o.get("idx")
        if fault == "pair_shares_mod_row":
            idx = idx.clone()
            idx[1::2] = idx[0:2 * (T // 2):2]
        m, a = (_np(t) for t in mod_rows(c, o, idx))
        one = F32(p["add_one"])
    eps = F32(0.0 if fault == "eps_dropped" else p["eps"])
    div = F32(mv * NT * 4 if fault == "divisor_maxv" else C)
    xp = np.zeros((T, mv * NT * 4), F32)
    xp[:, :C] = x
    v = xp.reshape(T, mv, NT, 4)
    valid = (np.arange(mv)[:, None] * NT + np.arange(NT)[None]) < C // 4      # [mv, NT]
    if rms:
        mean = np.zeros((T,), F32)
    else:
        s = np.zeros((T, NT), F32)
        for i in range(mv):
            s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
        mean = _block_sum(s) / div
    q = np.zeros((T, NT), F32)
    for i in range(mv):
        for j in range(4):
            d = v[:, i, :, j] - mean[:, None]
            q = q + np.where(valid[i][None], d * d, F32(0))
    rstd = _rsqrt(_block_sum(q) / div + eps)
    y = ((x - mean[:, None]) * rstd[:, None]) * (m + one) + a
    if fault == "last_odd_from_t0":
        t = (T - 1) if (T - 1) % 2 == 1 else T - 2
        y[t] = (((x[t - 1] - mean[t - 1]) * rstd[t - 1]) * ((m[t] if m.shape[0] > 1 else m[0]) + one) + (a[t] if a.shape[0] > 1 else a[0]))
    if kind == 1 or raw:
        out = torch.from_numpy(y.astype(F32)).double()
    else:
        hi = _round_bf16(y, trunc=fault == "bf16_trunc")
        out = hi
        if kind == 2:
            base = _round_bf16(y, trunc=True) if fault == "lo_from_trunc_hi" else hi
            lo = _round_bf16(y - base.float().numpy())
            out = torch.cat([hi, hi, lo], dim=1)
    if fault == "last_odd_unwritten":
        out[T - 1] = NAN
    return out


def _emulate_rope(c, o, fault, raw=False):
    p = c.p
    T, C, nparts, wp = p["T"], p["C"], p["nparts"], p["wperiod"]
    applies = {None: True, "last_odd_unwritten": _two_row(c) and (p["n_rope"] or T) % 2 == 1, "part1_with_sum0": nparts == 2 and p["eps"] >= 0,
               "rope_offset_from_vi": p["rope"], "sine_sign": p["rope"], "weight_row_div": wp > 1, "bf16_trunc": True,
               "eps_dropped": p["eps"] >= 0, "noeps_normalises": p["eps"] < 0}
    if not applies.get(fault, False):
        return None
    nv = int(route(c)[-1].split("<")[1][0])
    nvec, vpp = C // 8 * nparts, C // 8
    x = _np(o["x"])
    xp = np.zeros((T, nv * NT * 8), F32)
    xp[:, :nvec * 8] = x
    v = xp.reshape(T, nv, NT, 8)
    a = np.zeros((T, nv, NT), F32)
    for j in range(8):
        a = a + v[..., j] * v[..., j]
    vi = np.arange(nv)[:, None] * NT + np.arange(NT)[None]
    ss = [np.zeros((T, NT), F32), np.zeros((T, NT), F32)]
    for i in range(nv):
        ss[0] = ss[0] + np.where((vi[i] < vpp)[None], a[:, i], F32(0))
        ss[1] = ss[1] + np.where(((vi[i] >= vpp) & (vi[i] < nvec))[None], a[:, i], F32(0))
    eps = p["eps"]
    if fault == "noeps_normalises":
        eps = 1e-6
    if eps < 0:
        r = [np.ones((T,), F32), np.ones((T,), F32)]
    else:
        e = F32(0.0 if fault == "eps_dropped" else eps)
        r = [_rsqrt(_block_sum(ss[k]) / F32(C) + e) for k in range(2)]
    if fault == "part1_with_sum0":
        r[1] = r[0]
    rr = np.concatenate([np.repeat(r[k][:, None], C, axis=1) for k in range(nparts)], axis=1)
    w = _np(rope_weight_rows(c, o, div=fault == "weight_row_div"))
    y = (x * rr) * w
    tab = _np(rope_table(c, o))                                               # [T, 64, 2]
    col = np.arange(nparts * C)
    pair = (col % 128) // 2
    if fault == "rope_offset_from_vi":
        pair = ((((col // 8) & 127) >> 1) + (col % 8) // 2) % 64
    cs = tab[:, pair[0::2], 0]
    sn = tab[:, pair[0::2], 1]
    if fault == "sine_sign":
        sn = -sn
    y0, y1 = y[:, 0::2], y[:, 1::2]
    out = np.empty_like(y)
    if p["rope"]:
        out[:, 0::2] = y0 * cs - y1 * sn
        out[:, 1::2] = y0 * sn + y1 * cs
        if p["n_rope"] is not None:
            out[p["n_rope"]:] = y[p["n_rope"]:]
    else:
        out = y
    if raw:
        return torch.from_numpy(out.astype(F32)).double()
    res = _round_bf16(out, trunc=fault == "bf16_trunc")
    if fault == "last_odd_unwritten":
        res[(p["n_rope"] or T) - 1] = NAN
    return res


def _emulate_softmax(c, o, fault, raw=False):
    p = c.p
    H, n, ldp = p["H"], p["n"], p["ldp"]
    applies = {None: True, "bf16_trunc": True, "bias_index_off_by_one": n > 1, "padding_unzeroed": ldp > n}
    if not applies.get(fault, False):
        return None
    S, b = _np(o["S"]), _np(o["bias"])
    i, j = np.arange(n)[:, None], np.arange(n)[None]
    sl = j - i + n - 1
    if fault == "bias_index_off_by_one":
        sl = np.clip(sl + 1, 0, 2 * n - 2)
    v = np.full((H, n, 1024), F32(-3.0e38), F32)
    v[..., :n] = S + b[:, sl]
    mx = v.max(-1, keepdims=True)
    e = np.zeros((H, n, 1024), F32)
    e[..., :n] = np.exp((v[..., :n] - mx).astype(F32)).astype(F32)
    ek = e.reshape(H, n, 16, 64)                                              # element j = lane + 64 k
    s = np.zeros((H, n, 64), F32)
    for k in range(16):
        s = s + ek[:, :, k]
    inv = F32(1.0) / _wave_sum(s)
    if raw:
        return torch.from_numpy((e * inv[..., None]).astype(F32)).double()[..., :ldp].clone()
    out = _round_bf16(e * inv[..., None], trunc=fault == "bf16_trunc")[..., :ldp].clone()
    if fault == "padding_unzeroed":
        out[..., n:] = NAN
    return out


def _emulate_linear(c, o, fault):
    p = c.p
    R, K, N = p["R"], p["K"], p["N"]
    applies = {None: True, "in_act_row0_only": bool(p["in_act"]) and R > 1, "k_tail_dropped": K % 512 != 0 and K > 512}
    if not applies.get(fault, False):
        return None
    x, w = _np(o["x"]), _np(o["w"])

    def silu(t):
        return (t / (F32(1.0) + np.exp(-t).astype(F32))).astype(F32)
    xa = silu(x) if p["in_act"] else x.copy()
    if fault == "in_act_row0_only":
        xa[1:] = x[1:]
    Kuse = K // 512 * 512 if fault == "k_tail_dropped" else K
    trips = -(-K // 512)
    xp, wpad = np.zeros((R, trips * 512), F32), np.zeros((N, trips * 512), F32)
    xp[:, :Kuse], wpad[:, :Kuse] = xa[:, :Kuse], w[:, :Kuse]
    xl, wl = xp.reshape(R, trips, 64, 8), wpad.reshape(N, trips, 64, 8)       # k = trip * 512 + lane * 8 + j
    acc = np.zeros((R, N, 64), np.float64)
    for t in range(trips):
        for j in range(8):                                                    # fmaf: the exact product (48 bits) + acc, rounded to fp32
            acc = (xl[:, None, t, :, j].astype(np.float64) * wl[None, :, t, :, j].astype(np.float64) + acc).astype(F32).astype(np.float64)
    tot = _wave_sum(acc.astype(F32))
    vv = tot + (_np(o["bias"])[None] if o["bias"] is not None else F32(0))
    if p["out_act"]:
        vv = silu(vv.astype(F32))
    out = vv + (_np(o["add"])[None] if o["add"] is not None else F32(0))
    return torch.from_numpy(out.astype(F32)).double()


def mover_cap(c):
    """elements (vectors, for the vector movers) one trip of the mover's stride loop covers, in the order the loop walks the output"""
    return {"modtab": 4096 * 256 * 4, "cast": 8192 * 256 * 4, "unpatch": 4096 * 256, "gather": 256}.get(c.fam)


def _emulate_mover(c, o, fault):
    p = c.p
    ref = reference(c, o)["ref"].clone()
    if fault is None:
        return ref
    if fault == "rows_valid_ignored" and c.fam == "cast" and p["rows_valid"] < p["rows"]:
        return o["x"].bfloat16()
    if fault == "bf16_trunc" and ref.dtype == torch.bfloat16 and not p.get("bf16", False):
        src = {"cast": lambda: o["x"], "transpose": lambda: o["x"].t().contiguous()}.get(c.fam)
        if src is None:
            return None
        t = (src().contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()
        if c.fam == "cast":
            t[p["rows_valid"]:] = 0
        return t
    if fault == "one_trip" and mover_cap(c) is not None:
        cap = mover_cap(c)
        if c.fam == "gather":
            if ref.shape[1] <= cap:
                return None
            ref[:, cap:] = NAN
            return ref
        if ref.numel() <= cap:
            return None
        ref.view(-1)[cap:] = NAN
        return ref
    return None


# ------------------------------------------------------------------------------------------------ the call
def _guarded(rows, ld, dtype, device, before=1, after=1):
    """a NaN-filled [before + rows + after, ld] buffer and the view of its middle rows"""
    buf = torch.full((before + rows + after, ld), NAN, dtype=dtype, device=device)
    return buf, buf[before:before + rows]


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def run_case(c, o, device="cuda"):
    """one call (the split row: two) of the raw C-ABI -> {"out": (buffer, mask of the elements the call stores), ...}; every buffer NaN
    outside what the call reads and stores — the rows in front and behind, the stride gaps of inputs and outputs"""
    from yume_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    p = c.p
    dv = lambda t: t.to(device) if t is not None else None

    def masked(buf, view_rows, cols):
        mask = torch.zeros(buf.shape, dtype=torch.bool, device=device)
        mask[view_rows[0]:view_rows[1], :cols] = True
        return mask
    if c.fam in ("adaln", "rms"):
        T, C = p["T"], p["C"]
        if c.fam == "adaln":
            ldx, ldo = adaln_strides(c)
            kind = p["kind"]
        else:
            ldx, ldo, kind = C + p["ldx_x"], C + p["ldo_x"], 0
        xb, xv = _guarded(T, ldx, torch.float32, device)
        xv[:, :C] = dv(o["x"])
        cols = 3 * C if kind == 2 else C
        ob, ov = _guarded(T, ldo, torch.float32 if kind == 1 else torch.bfloat16, device)
        if c.fam == "rms":
            w = dv(o["w"])
            rc = lib.yume_rmsnorm_f32(_vp(xv), ldx, T, C, p["eps"], _vp(w), _vp(ov), ldo, st)
            _lib.check(rc, "yume_rmsnorm_f32")
        else:
            if p["affine"]:
                mul, add, ts, idx = dv(o["w"]), dv(o["b"]), 0, None
                keep = (mul, add)
            else:
                tab, idx = dv(o["tab"]), dv(o["idx"])
                mul, add, ts = tab[0, 1], tab[0, 0], 6 * C
                keep = (tab,)
            rc = lib.yume_adaln_modulate(_vp(xv), ldx, T, C, p["eps"], _vp(mul), _vp(add), ts, _vp(idx), p["add_one"], _vp(ov), ldo, kind, st)
            _lib.check(rc, "yume_adaln_modulate")
        return {"out": (ob, masked(ob, (1, 1 + T), cols))}
    if c.fam in ("rope", "periodic"):
        T, C, nparts = p["T"], p["C"], p["nparts"]
        ld = nparts * C + p["ld_x"]
        bb, bv = _guarded(T, ld, torch.bfloat16, device)
        bv[:, :nparts * C] = dv(o["x"]).bfloat16()
        w = dv(o["w"])
        if c.fam == "periodic":
            rc = lib.yume_rmsnorm_rows_periodic(_vp(bv), ld, T, C, _vp(w), p["wperiod"], p["eps"], st)
            _lib.check(rc, "yume_rmsnorm_rows_periodic")
        else:
            rope = dv(o.get("rope"))
            nr = p["n_rope"] if p["n_rope"] is not None else T
            _lib.check(lib.yume_rmsnorm_rope(_vp(bv), ld, nr, C, nparts, _vp(w), p["eps"], _vp(rope), 128, st), "yume_rmsnorm_rope")
            if nr < T:
                _lib.check(lib.yume_rmsnorm_rope(_vp(bv[nr:]), ld, T - nr, C, nparts, _vp(w), p["eps"], None, 128, st), "yume_rmsnorm_rope")
        return {"out": (bb, masked(bb, (1, 1 + T), nparts * C))}
    if c.fam == "softmax":
        H, n, ldp = p["H"], p["n"], p["ldp"]
        lds, ldb = n + p["lds_x"], 2 * n - 1 + p["gap"]
        strideS, strideP = n * lds + p["gap"], n * ldp + p["gap"]
        Sb = torch.full((H * strideS + 8,), NAN, dtype=torch.float32, device=device)
        Sv = torch.as_strided(Sb, (H, n, n), (strideS, lds, 1), 4)
        Sv.copy_(dv(o["S"]))
        bb = torch.full((H, ldb), NAN, dtype=torch.float32, device=device)
        bb[:, :2 * n - 1] = dv(o["bias"])
        Pb = torch.full((H * strideP + 16,), NAN, dtype=torch.bfloat16, device=device)
        mask = torch.zeros(Pb.shape, dtype=torch.bool, device=device)
        torch.as_strided(mask, (H, n, ldp), (strideP, ldp, 1), 8).fill_(True)
        Pv = torch.as_strided(Pb, (H, n, ldp), (strideP, ldp, 1), 8)
        rc = lib.yume_softmax_bias_rows(_vp(Sv), lds, strideS, H, n, _vp(bb), ldb, _vp(Pv), ldp, strideP, st)
        _lib.check(rc, "yume_softmax_bias_rows")
        return {"out": (Pb, mask), "view": Pv}
    if c.fam == "linear":
        R, K, N = p["R"], p["K"], p["N"]
        x, w = dv(o["x"]).contiguous(), dv(o["w"]).contiguous()
        if p["wbf16"]:
            w = w.bfloat16()
        ob = torch.full((R * N + 128,), NAN, dtype=torch.float32, device=device)
        mask = torch.zeros(ob.shape, dtype=torch.bool, device=device)
        mask[64:64 + R * N] = True
        bias, add = dv(o["bias"]), dv(o["add"])
        rc = lib.yume_linear_smallm_f32(_vp(x), R, K, _vp(w), int(p["wbf16"]), _vp(bias), N, p["in_act"], p["out_act"], _vp(add), _vp(ob[64:]), st)
        _lib.check(rc, "yume_linear_smallm_f32")
        return {"out": (ob, mask)}
    if c.fam == "sinus":
        R, dim = p["R"], p["dim"]
        t, idx = dv(o["t"]), dv(o["idx"])
        ob = torch.full((R * dim + 128,), NAN, dtype=torch.float32, device=device)
        mask = torch.zeros(ob.shape, dtype=torch.bool, device=device)
        mask[64:64 + R * dim] = True
        _lib.check(lib.yume_sinusoidal_embed(_vp(t), _vp(idx), R, dim, _vp(ob[64:]), st), "yume_sinusoidal_embed")
        return {"out": (ob, mask)}
    if c.fam == "modtab":
        B, R, W = p["B"], p["R"], p["W"]
        tab, e0 = dv(o["tab"]), dv(o["e0"])
        ob = torch.full((B * R * W + 128,), NAN, dtype=torch.float32, device=device)
        mask = torch.zeros(ob.shape, dtype=torch.bool, device=device)
        mask[64:64 + B * R * W] = True
        _lib.check(lib.yume_modulation_table(_vp(tab), _vp(e0), B, R, W, _vp(ob[64:]), st), "yume_modulation_table")
        return {"out": (ob, mask)}
    if c.fam == "cast":
        rows, cols = p["rows"], p["cols"]
        ldi, ldo = cols + p["ldi_x"], cols + p["ldo_x"]
        xb, xv = _guarded(rows, ldi, torch.float32, device)
        xv[:, :cols] = dv(o["x"])
        ob, ov = _guarded(rows, ldo, torch.bfloat16, device)
        _lib.check(lib.yume_cast_bf16(_vp(xv), ldi, p["rows_valid"], rows, cols, _vp(ov), ldo, st), "yume_cast_bf16")
        return {"out": (ob, masked(ob, (1, 1 + rows), cols))}
    if c.fam == "transpose":
        rows, cols = p["rows"], p["cols"]
        ldi, ldo = cols + p["ldi_x"], rows + p["ldo_x"]
        xb, xv = _guarded(rows, ldi, torch.bfloat16 if p["bf16"] else torch.float32, device)
        xv[:, :cols] = dv(o["x"]).to(xb.dtype)
        ob, ov = _guarded(cols, ldo, torch.bfloat16, device)
        _lib.check(lib.yume_transpose_bf16(_vp(xv), int(p["bf16"]), ldi, rows, cols, _vp(ov), ldo, st), "yume_transpose_bf16")
        return {"out": (ob, masked(ob, (1, 1 + cols), rows))}
    if c.fam == "gather":
        x = dv(o["x"]).contiguous()
        if p["bf16"]:
            x = x.bfloat16()
        Cin, F, H, W = x.shape
        ntok = p["nf"] * -(-H // p["kh"]) * -(-W // p["kw"])
        ob, ov = _guarded(ntok, p["Kp"], torch.bfloat16, device)
        _lib.check(lib.yume_patch_gather(_vp(x), int(p["bf16"]), Cin, F, H, W, p["f0"], p["nf"], p["kh"], p["kw"], _vp(ov), p["Kp"], st), "yume_patch_gather")
        return {"out": (ob, masked(ob, (1, 1 + ntok), p["Kp"]))}
    if c.fam == "unpatch":
        Fr, Hp, Wp, ph, pw, Co = p["Fr"], p["Hp"], p["Wp"], p["ph"], p["pw"], p["Cout"]
        ntok, width = Fr * Hp * Wp, ph * pw * Co
        ldi = width + p["ldi_x"]
        xb, xv = _guarded(ntok, ldi, torch.float32, device)
        xv[:, :width] = dv(o["x"])
        total = Co * Fr * Hp * ph * Wp * pw
        ob = torch.full((total + 128,), NAN, dtype=torch.float32, device=device)
        mask = torch.zeros(ob.shape, dtype=torch.bool, device=device)
        mask[64:64 + total] = True
        _lib.check(lib.yume_unpatchify(_vp(xv), ldi, Fr, Hp, Wp, ph, pw, Co, _vp(ob[64:]), st), "yume_unpatchify")
        return {"out": (ob, mask)}
    raise AssertionError(c.fam)


def gather(c, bufs, r):
    """what the call stored, in the layout of reference()["ref"]"""
    buf, mask = bufs["out"]
    if c.fam == "softmax":
        return bufs["view"]
    return buf[mask].view(*r["ref"].shape[:-1], -1)                              # (out_kind 2: three times the reference's columns)


def guards_damaged(bufs):
    """number of elements outside the stored region that no longer hold NaN"""
    buf, mask = bufs["out"]
    return int((~torch.isnan(buf) & ~mask).sum())


def main(argv):
    if argv != ["--routes"]:
        sys.exit(__doc__)
    for c in CASES:
        if c.fam not in LOGGED:
            continue
        o = make_case(c)
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {c.name}\n")
        sys.stderr.flush()
        run_case(c, o)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main(sys.argv[1:])
