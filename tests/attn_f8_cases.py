"""The case table of the MX e4m3 self-attention (yume_attn_fwd_f8mx, yume_amd/csrc/attn_f8.hpp) and of its two quantisers
(yume_quant_rows_mx_e4m3, yume_attn_vt_mx_e4m3, yume_amd/csrc/quant_mx.hip): operands, the fp64 reference on the very bytes the device is
given, the per-element bound, a host emulation that rounds where the kernel rounds, ten injectable faults (no test functions in here;
the patterns and helpers are tests/attn_cases.py's, the host MX quantiser is tests/conv_f8_cases.py's).

    O[i, h, :] = sum_j 2^<q^_i, k^_j> v^_j / sum_j 2^<q^_i, k^_j>,  j < Lk            hatted = the dequantised bytes (q carries scale * log2(e))

Reference: exact softmax in fp64 on the dequantised operands. The quantisation error of q, k and v is not the kernel's to answer for; the
quantisers are held bit for bit to the host MX quantiser by their own rows (QCASES, VCASES).

Bound, per element — attn_cases.bound's form with the P rounding at e4m3's half ulp (a_ij = the exact softmax weight, A = sum_j a_ij |v^_jd|,
Q = sum_j (a_ij v^_jd)^2):

    |got - ref| <= 2^-8 |ref|  +  KAPPA8 * 2^-5 sqrt(Q)  +  flush  +  score  +  2^-20 A

  * 2^-8 |ref|: half a bf16 ulp of what is stored.
  * KAPPA8 * 2^-5 sqrt(Q): P is rounded ONCE to e4m3 (three fraction bits): each rounding is at most 2^-4 of its P (half an ulp at the
    bottom of a binade, 2^-5 at the top), independent from key to key: their sum walks about 0.8 * 2^-5 sqrt(Q) away. The P that is rounded is
    the one against the RUNNING maximum; the later rescales by 2^(m_old - m_new) are exact in effect (a common fp32 factor of numerator and
    denominator), so the relative size of a P's rounding error is what it was when it was made. KAPPA8 = attn_cases.KAPPA = 4.5; it is settled
    by the host emulation at the table's own sizes (`--emulate`: no element outside on any row) and by the injected faults
    (tests/test_attn_f8_cases_cpu.py), never by a device. Figures: profiles/r22_fp8_attn.md.
  * flush: 256 p below 2^-6 is an e4m3 subnormal (spacing 2^-9), below 2^-10 it is dropped: the absolute error of such a P is at most 2^-18
    in units of the row's running maximum, hence at most 2^-18 in units of the final one. Only keys whose FINAL p is under 2^-14 can have
    been subnormal when rounded (p against a running maximum is never smaller than against the final one; a key at or above 2^-14 was normal
    and sits in the KAPPA8 term). These errors are uniform in +-2^-18 or, for a dropped p, the p itself in [0, 2^-18): rms 2^-18 / sqrt(3)
    either way, signs following v^: a random walk over the row's v^,
        flush = FLUSH_K * 2^-18 sqrt(sum_{j: p_j < 2^-14} v^_jd^2) / l,       l = sum_j p_j (the row sum in units of the maximum),
    FLUSH_K = 3.25 = 5.6 deviations (the same 5.6 KAPPA stands for in attn_cases.py).
  * score: the scaled instruction sums the 128 products of a score in registers, NOT as an fp32 chain (profiles/r15_fp8_ffn.md §4):
    |ds_ij| <= C_SUM_MX sigma_ij, sigma_ij = sqrt(sum_k (q^_ik k^_jk)^2), C_SUM_MX = 7.62e-4 (tests/gemm_f8_mx_cases.py). Through 2^x a score
    error moves p_ij by ln 2 * ds_ij of itself, in the numerator and in the denominator: dO_d = ln 2 sum_j a_ij ds_ij (v^_jd - O_d), so
        score = ln 2 * C_SUM_MX * (sum_j a_ij sigma_ij |v^_jd| + |ref_d| sum_j a_ij sigma_ij)            (no cancellation assumed).
  * 2^-20 A: fp32 scores under the exponential, the fp32 exp2, the fp32 sums (the row sum is taken over the UNROUNDED p, attn_f8.hpp).

Patterns: attn_cases.make_case's `probe`, `stairs`, `levels`, `random` (pre-scaled q), quantised on the host; `stairs` carries a score
offset per 64 keys, so the running maximum of a row moves at every 128-key tile (up or down by turns); `levels` puts a large constant offset
on every score of a row (it must cancel). Two `pattern` rows are exact integers (make_pattern): the kernel's result is held bit for bit to
`emulate()`, whose every fp32 step is exact on them.

    python tests/attn_f8_cases.py --routes      one call per row, `CASE <name>` on stderr before each (YUME_ATTN_LOG=1 / YUME_NORM_LOG=1 name the launches)
    python tests/attn_f8_cases.py --emulate     the host emulation's worst error / bound of every row at its full size (no GPU)
"""
import math
import os
import sys
import zlib
from collections import namedtuple

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_cases as ac  # noqa: E402
import conv_f8_cases as cc  # noqa: E402
import gemm_f8_mx_cases as mc  # noqa: E402

D = ac.D
KEYS = 128                   # keys per tile (attn_f8.hpp)
QBLOCK = 256                 # queries per workgroup
SENTINEL = ac.SENTINEL
GUARD_ROWS, GUARD_COLS = ac.GUARD_ROWS, ac.GUARD_COLS
KAPPA8 = ac.KAPPA
FLUSH_K = 3.25
C_SUM_MX = mc.C_SUM_MX
NAN_BYTE = 0x7F              # e4m3 NaN: every operand byte a kernel must not use
NAN_SCALE = 0xFF             # E8M0 NaN: every scale byte a kernel must not use
GUARD_BYTE = mc.GUARD_BYTE   # what the quantisers must leave untouched
P_SHIFT = 8                  # P = e4m3(2^P_SHIFT p), the second product's scale byte is 127 - P_SHIFT
EINVAL = -1

# ldq_x / ldk_x: bytes a row of Q8 / K8 is longer than 128 H (multiples of 16); lde_x: of Eq / Ek (multiples of 4); ldvt8_x: of Vt8
# (multiples of 16); ldev_x: of Ev (multiples of 4); ldo_x: elements of O (multiples of 4)
Case = namedtuple("Case", "name Lq Lk H pattern ldq_x ldk_x lde_x ldvt8_x ldev_x ldo_x", defaults=(0, 0, 0, 0, 0, 0))

LQS = (1, 255, 256, 257, 301)
LKS = (1, 127, 128, 129, 257, 640)


def _table():
    rows = []
    # ---- Lq = 301 (a whole block and a ragged one) against every Lk: probe; the patterns that need more than one tile where there is one
    for n, Lk in enumerate(LKS):
        pitched = dict(ldq_x=16, ldk_x=32, lde_x=4, ldvt8_x=16, ldev_x=8, ldo_x=4 + GUARD_COLS) if n % 2 == 0 else {}
        rows.append(Case(f"probe_q301_k{Lk}", 301, Lk, 3, "probe", **pitched))
        if Lk > KEYS:
            rows.append(Case(f"stairs_q301_k{Lk}", 301, Lk, 3 if n % 2 else 1, "stairs", **({} if pitched else dict(ldvt8_x=48, ldo_x=8))))
    rows.append(Case("levels_q301_k257", 301, 257, 3, "levels", ldq_x=16, ldo_x=12))
    rows.append(Case("levels_q257_k640", 257, 640, 1, "levels"))
    rows.append(Case("random_q301_k257", 301, 257, 3, "random"))
    rows.append(Case("random_q256_k640", 256, 640, 1, "random", ldvt8_x=16, ldev_x=4))
    # ---- the other Lq against Lk, thinned as attn_cases._table thins (every second pair, patterns and head counts by turns)
    for n, Lq in enumerate(LQS[:-1]):
        for m, Lk in enumerate(LKS):
            if (n + m) % 2:
                continue
            pattern = ("probe", "random")[(n + m) // 2 % 2]
            rows.append(Case(f"{pattern}_q{Lq}_k{Lk}", Lq, Lk, (1, 3)[(n + m // 2) % 2], pattern, ldo_x=(0, 4)[m % 2 == 0 and n % 2 == 0]))
    # ---- exact integers
    rows.append(Case("pattern_q301_k640", 301, 640, 3, "pattern", ldq_x=16, lde_x=4, ldvt8_x=16, ldev_x=4, ldo_x=8))
    rows.append(Case("pattern_q257_k129", 257, 129, 1, "pattern"))
    return rows


CASES = _table()
assert len({c.name for c in CASES}) == len(CASES)


def tiles(Lk):
    return (Lk + KEYS - 1) // KEYS


def shrink(c):
    """the same key structure with at most 2 heads and 157 queries (a ragged last fragment of 16)"""
    return c._replace(name=c.name + "_small", Lq=min(c.Lq, 157), H=min(c.H, 2))


# ---- the V^T8 layout (yume_amd/csrc/quant_mx.hip) ------------------------------------------------------------------------------------------
def vt8_offsets(Lk):
    """key index held by byte column 128 t + kk of a Vt8 row, for every column of the image (long [128 * tiles]; an index >= Lk is padding):
    g = (kk >> 4) & 3, w = 4 (kk >> 6) + ((kk >> 2) & 3), y = kk & 3 -> key 128 t + 16 w + 4 g + y. Scale block b of a tile = columns 32 b .. + 31."""
    kk = torch.arange(KEYS)
    key = 16 * (4 * (kk >> 6) + ((kk >> 2) & 3)) + 4 * ((kk >> 4) & 3) + (kk & 3)
    return (torch.arange(tiles(Lk)).view(-1, 1) * KEYS + key.view(1, -1)).reshape(-1)


def vt_mx_quantise(vt, Lk):
    """host mirror of yume_attn_vt_mx_e4m3: vt [C, >= Lk] (values a bf16 holds) -> (vt8 u8 [C, 128 tiles], ev u8 [tiles, 4 C])"""
    C, T = vt.shape[0], tiles(Lk)
    pad = torch.zeros(C, KEYS * T)
    pad[:, :Lk] = vt[:, :Lk].float()
    q, e = cc.mx_quantise(pad[:, vt8_offsets(Lk)])                 # e [C, 4 T]
    return q, e.view(C, T, 4).permute(1, 0, 2).reshape(T, 4 * C).contiguous()


def vt_mx_dequantise(vt8, ev, Lk):
    """(vt8 [C, 128 tiles], ev [tiles, 4 C]) -> v^ fp32 [Lk, C]"""
    C, T = vt8.shape[0], tiles(Lk)
    e = ev.view(T, C, 4).permute(1, 0, 2).reshape(C, 4 * T)
    img = cc.mx_dequantise(vt8, e)
    out = torch.zeros(C, KEYS * T)
    out[:, vt8_offsets(Lk)] = img
    return out[:, :Lk].t().contiguous()


# ---- operands ------------------------------------------------------------------------------------------------------------------------------
def make_pattern(c):
    """exact integers, seeded. With scale exponents E drawn from {-1, 0, 1} per (row, block) — per (channel, tile, block) for V^T — and every
    byte = target / 2^E (0.5 .. 12, exact in e4m3):
      q^_i is 1 at ONE feature of each 32-feature block (drawn per row, block and head) and 0 elsewhere;
      k^_j[f] is 1 or 2 (drawn per key, feature and head), plus the key's tile index j // 128 on the features below 32;
      v^_j[d] is 1 .. 4 (drawn per key, channel and head).
    A score is the sum of four K values, 4 .. 8 plus the key's tile index: integers, every p a power of two from 2^-4 up inside a tile, the
    running maximum one higher at every tile (every old sum is halved there); 256 p, the products of both instructions (at most 7 bits under
    the largest of one sum) and every fp32 sum (under 21 bits) are exact. A byte or a scale byte taken from another row, key, feature,
    channel, block, tile or head changes the integers."""
    Lq, Lk, H, T = c.Lq, c.Lk, c.H, tiles(c.Lk)
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.split("_small")[0].encode()))
    rnd = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g)
    f = torch.arange(D)
    hot = rnd(0, 31, Lq, H, 4) + 32 * torch.arange(4)                                                  # the feature of (row, head, block)
    qt = (f.view(1, 1, 1, D) == hot.unsqueeze(-1)).any(dim=2).float()                               # [Lq, H, D]
    kt = (rnd(1, 2, Lk, H, D) + (f < 32).view(1, 1, D) * (torch.arange(Lk) // KEYS).view(Lk, 1, 1)).float()
    eq, ek = rnd(-1, 1, Lq, H, 4), rnd(-1, 1, Lk, H, 4)
    key = vt8_offsets(Lk)                                                                            # image column -> key
    vk = rnd(1, 4, KEYS * T, H, D).float()                                                           # drawn per key (padding keys: unused)
    vimg = (vk[key] * (key < Lk).view(-1, 1, 1)).permute(1, 2, 0).reshape(H * D, KEYS * T)          # [H D, 128 T] in image order
    ev = rnd(-1, 1, H * D, T, 4)
    tob = lambda t: t.to(torch.float8_e4m3fn).view(torch.uint8)
    q8 = tob((qt * torch.pow(2.0, -eq.float()).repeat_interleave(32, dim=2)).reshape(Lq, H * D))
    k8 = tob((kt * torch.pow(2.0, -ek.float()).repeat_interleave(32, dim=2)).reshape(Lk, H * D))
    vt8 = tob(vimg * torch.pow(2.0, -ev.float()).reshape(H * D, 4 * T).repeat_interleave(32, dim=1))
    as_bytes = lambda e: (e + 127).to(torch.uint8)
    return (q8, as_bytes(eq).reshape(Lq, 4 * H), k8, as_bytes(ek).reshape(Lk, 4 * H), vt8,
            as_bytes(ev).permute(1, 0, 2).reshape(T, 4 * H * D).contiguous())


def make_case(c):
    """seeded operands on the CPU: the bytes and scale bytes the call gets ("q8" [Lq, 128 H], "eq" [Lq, 4 H], "k8", "ek", "vt8" [128 H, 128 tiles],
    "ev" [tiles, 512 H]) and their dequantised values "q", "k", "v" fp32 [L, H, 128]"""
    if c.pattern == "pattern":
        q8, eq, k8, ek, vt8, ev = make_pattern(c)
    else:
        base = ac._fwd(c.name.split("_small")[0], 0, c.Lq, c.Lk, c.H, c.pattern, "tight", "f8mx", prescaled=True, padded=True)
        sg = ac.make_case(base)["segs"][0]
        q8, eq = cc.mx_quantise(sg["q"].reshape(c.Lq, c.H * D))
        k8, ek = cc.mx_quantise(sg["k"].reshape(c.Lk, c.H * D))
        vt8, ev = vt_mx_quantise(sg["v"].reshape(c.Lk, c.H * D).t().contiguous(), c.Lk)
    ops = {"q8": q8, "eq": eq, "k8": k8, "ek": ek, "vt8": vt8, "ev": ev}
    ops["q"] = cc.mx_dequantise(q8, eq).view(c.Lq, c.H, D)
    ops["k"] = cc.mx_dequantise(k8, ek).view(c.Lk, c.H, D)
    ops["v"] = vt_mx_dequantise(vt8, ev, c.Lk).view(c.Lk, c.H, D)
    return ops


# ---- reference and bound -------------------------------------------------------------------------------------------------------------------
def reference(c, ops, device="cpu"):
    """exact softmax attention in fp64 on the dequantised operands -> "ref", "A", "Q", "flush" (sqrt(sum_{p_j < 2^-14} v^2) / l), "score"
    (sum_j a_ij sigma_ij |v_jd| + |ref_d| sum_j a_ij sigma_ij), each fp64 [Lq, H, 128] on `device`"""
    q, k, v = (ops[n].to(device, torch.float64) for n in ("q", "k", "v"))
    out = {n: torch.empty(c.Lq, c.H, D, dtype=torch.float64, device=device) for n in ("ref", "A", "Q", "flush", "score")}
    for h in range(c.H):
        qh, kh, vh = q[:, h], k[:, h], v[:, h]
        x = qh @ kh.T
        p = torch.exp2(x - x.max(dim=1, keepdim=True).values)
        l = p.sum(dim=1, keepdim=True)
        a = p / l
        out["ref"][:, h] = a @ vh
        out["A"][:, h] = a @ vh.abs()
        out["Q"][:, h] = (a * a) @ (vh * vh)
        out["flush"][:, h] = ((p < 2.0 ** -14).double() @ (vh * vh)).sqrt() / l
        asig = a * ((qh * qh) @ (kh * kh).T).sqrt()
        out["score"][:, h] = asig @ vh.abs() + out["ref"][:, h].abs() * asig.sum(dim=1, keepdim=True)
    return out


def bound(r, kappa=KAPPA8):
    """the per-element error a correct kernel may show against r["ref"] (module docstring)"""
    return (2.0 ** -8 * r["ref"].abs() + kappa * 2.0 ** -5 * r["Q"].sqrt() + FLUSH_K * 2.0 ** -18 * r["flush"] + math.log(2) * C_SUM_MX * r["score"]
            + 2.0 ** -20 * r["A"])


# ---- host emulation ------------------------------------------------------------------------------------------------------------------------
FAULTS = ("vt_scale_neighbour", "q_scale_rotated", "unmasked", "tile_skipped", "no_rescale", "p_scale_off", "p_truncated", "no_divide",
          "ragged_wrong_row", "vt_head_off")


def fault_applies(c, fault):
    """is the corruption one the bound has to flag on this row? Where it changes what the kernel computes by more than a correct one's roundings:
      * a neighbouring V^T scale byte differs by one binade or more on most blocks of every row with real data (not where the neighbour is the
        same byte: never true of a whole row here);
      * rotated q scale bytes change the scores wherever a row of q has blocks of different size: not `levels` / `stairs`, whose feature 0
        dominates block 0 and makes every row's own maximum key decide, only where there is more than one key to weigh (Lk >= 2) and more
        than a row or two of q (Lq >= 16: the four blocks of ONE row may well carry the same byte);
      * unmasked keys are copies of key Lk - 1 with zero V rows: they take weight from the row (ragged Lk only; not `levels` and `stairs` rows,
        where the last key may lie far under the row's maximum);
      * a skipped tile, a dropped rescale need two tiles (a dropped rescale shows where the maximum moves UP by a whole binade or more between
        tiles: `stairs` and `pattern`; the second tile of a `pattern` row holds the same integers as every other: without it the row's mean
        barely moves, and those rows are held bit for bit anyway);
      * a P scale one off doubles O; an undivided O differs wherever the row sum is not 1 (Lk >= 2);
      * truncated P is a whole e4m3 ulp off, always downwards: a bias of 2^-4.4 A on average against a bound that walks as sqrt(Q): it shows on
        flat rows with many keys (random, Lk >= 257), not beside a probe key's own rounding and not under the score term of a `levels`
        row (its offsets of up to 160 make sigma large);
      * the wrong row in a ragged block needs a ragged block with two rows and two keys (with one key every row is that key's V row);
        the neighbouring head's V^T needs two heads."""
    T = tiles(c.Lk)
    return {"vt_scale_neighbour": True,
            "q_scale_rotated": c.Lk >= 2 and c.Lq >= 16 and c.pattern in ("probe", "random", "pattern"),
            "unmasked": c.Lk % KEYS != 0 and c.Lk >= 2 and c.pattern in ("probe", "random", "pattern"),
            "tile_skipped": T >= 2 and c.pattern != "pattern",
            "no_rescale": T >= 2 and c.pattern in ("stairs", "pattern"),
            "p_scale_off": True,
            "p_truncated": c.pattern == "random" and c.Lk >= 257,
            "no_divide": c.Lk >= 2,
            "ragged_wrong_row": c.Lq % 16 != 0 and c.Lq >= 2 and c.Lk >= 2,
            "vt_head_off": c.H >= 2}[fault]


def _e4m3(t, truncate=False):
    """fp32 -> the value of its e4m3 rounding (nearest even; `truncate`: towards zero), subnormals kept, below half the smallest one 0"""
    r = t.to(torch.float8_e4m3fn).float()
    if truncate:
        ulp = torch.where(t.abs() >= 2.0 ** -6, torch.exp2(torch.floor(torch.log2(t.abs().clamp(min=2.0 ** -6))) - 3), torch.full_like(t, 2.0 ** -9))
        r = torch.where(r.abs() > t.abs(), r - ulp * torch.sign(t), r)
    return r


def emulate(c, ops, fault=None):
    """what attn_f8mx_kernel stores, on the CPU in fp32: fp32 scores of the dequantised operands, per 128-key tile the running maximum
    m, alpha = 2^(m_old - m_new), P = e4m3_rne(2^(s - (m - 8))), l = l alpha + sum of the UNROUNDED 256 p, O = O alpha + 2^-8 (P @ v^);
    then bf16(O * (256 / l)). -> fp64 [Lq, H, 128]"""
    Lq, Lk, H, T = c.Lq, c.Lk, c.H, tiles(c.Lk)
    q, k, v = ops["q"], ops["k"], ops["v"]
    if fault == "q_scale_rotated":
        q = cc.mx_dequantise(ops["q8"], ops["eq"].view(Lq, H, 4).roll(1, dims=2).reshape(Lq, 4 * H)).view(Lq, H, D)
    if fault == "vt_scale_neighbour":
        ev = ops["ev"].view(T, H * D, 4)[:, :, [1, 0, 3, 2]].reshape(T, 4 * H * D)
        v = vt_mx_dequantise(ops["vt8"], ev, Lk).view(Lk, H, D)
    if fault == "vt_head_off":
        v = v.roll(-1, dims=1)
    out = torch.empty(Lq, H, D, dtype=torch.float32)
    for h in range(H):
        kh, vh = k[:, h], v[:, h]
        if fault == "unmasked" and Lk % KEYS:                     # the clamped K row Lk - 1 against zero V^T bytes
            pad = T * KEYS - Lk
            kh = torch.cat([kh, kh[-1:].expand(pad, D)])
            vh = torch.cat([vh, torch.zeros(pad, D)])
        x = q[:, h] @ kh.T
        m = torch.full((Lq, 1), -float("inf"))
        l = torch.zeros(Lq, 1)
        o = torch.zeros(Lq, D)
        for t in range(T):
            if fault == "tile_skipped" and t == 1:
                continue
            xs = x[:, t * KEYS:(t + 1) * KEYS]
            mnew = torch.maximum(m, xs.max(dim=1, keepdim=True).values)
            alpha = torch.exp2(m - mnew)
            m = mnew
            p = torch.exp2(xs - (mnew - P_SHIFT))
            l = l * alpha + p.sum(dim=1, keepdim=True)
            P = _e4m3(p, truncate=fault == "p_truncated")
            if fault != "no_rescale":
                o = o * alpha
            o = o + (P @ vh[t * KEYS:(t + 1) * KEYS]) * 2.0 ** -(P_SHIFT - (1 if fault == "p_scale_off" else 0))
        out[:, h] = o if fault == "no_divide" else o * (2.0 ** P_SHIFT / l)
    if fault == "ragged_wrong_row":
        out[Lq - 1] = out[Lq - 2]
    return out.to(torch.bfloat16).double()


# ---- the call on the device ----------------------------------------------------------------------------------------------------------------
def _padded(body, rows, ld, fill, row0=0):
    buf = torch.full((rows, ld), fill, dtype=torch.uint8)
    buf[row0:row0 + body.shape[0], :body.shape[1]] = body
    return buf


def device_operands(c, ops, device="cuda"):
    """the operands in the row's pitches; every byte a kernel must not use is an e4m3 / E8M0 NaN (guard rows, pitch gaps, K rows >= Lk, V^T
    rows of the heads above and below, V^T columns beyond the last tile), O is NaN where it must be written and SENTINEL everywhere else"""
    H, HC, T = c.H, c.H * D, tiles(c.Lk)
    dv = {}
    qb = _padded(ops["q8"], GUARD_ROWS + c.Lq + GUARD_ROWS, HC + c.ldq_x, NAN_BYTE, GUARD_ROWS).to(device)
    eqb = _padded(ops["eq"], GUARD_ROWS + c.Lq + GUARD_ROWS, 4 * H + c.lde_x, NAN_SCALE, GUARD_ROWS).to(device)
    kb = _padded(ops["k8"], c.Lk + GUARD_ROWS, HC + c.ldk_x, NAN_BYTE).to(device)
    ekb = _padded(ops["ek"], c.Lk + GUARD_ROWS, 4 * H + c.lde_x, NAN_SCALE).to(device)
    vb = _padded(ops["vt8"], D + HC + D, KEYS * T + c.ldvt8_x, NAN_BYTE, D).to(device)
    evb = _padded(ops["ev"], T + 1, 4 * HC + c.ldev_x, NAN_SCALE).to(device)
    dv.update(q8=qb[GUARD_ROWS:GUARD_ROWS + c.Lq, :HC], eq=eqb[GUARD_ROWS:GUARD_ROWS + c.Lq, :4 * H], k8=kb[:c.Lk, :HC], ek=ekb[:c.Lk, :4 * H],
              vt8=vb[D:D + HC, :KEYS * T], ev=evb[:T, :4 * HC])
    obuf = torch.full((GUARD_ROWS + c.Lq + GUARD_ROWS, HC + c.ldo_x), SENTINEL, dtype=torch.bfloat16)
    obuf[GUARD_ROWS:GUARD_ROWS + c.Lq, :HC] = float("nan")
    dv["obuf"] = obuf.to(device)
    dv["o"] = dv["obuf"][GUARD_ROWS:GUARD_ROWS + c.Lq, :HC]
    return dv


def run_case(c, ops, dv=None):
    """one call into fresh operands (or `dv`) -> the device operands; the result is in ["obuf"]"""
    from yume_amd import ops as yops
    dv = dv or device_operands(c, ops)
    yops.attn_fwd_f8mx(dv["q8"], dv["eq"], dv["k8"], dv["ek"], dv["vt8"], dv["ev"], dv["o"], c.Lq, c.Lk, c.H)
    return dv


def written(c, dv):
    """(the result [Lq, H, 128] fp64, everything else of obuf as one flat tensor: guard rows, guard columns)"""
    obuf = dv["obuf"]
    mask = torch.ones_like(obuf, dtype=torch.bool)
    mask[GUARD_ROWS:GUARD_ROWS + c.Lq, :c.H * D] = False
    return obuf[GUARD_ROWS:GUARD_ROWS + c.Lq, :c.H * D].double().view(c.Lq, c.H, D), obuf[mask]


# ---- the quantisers' rows ------------------------------------------------------------------------------------------------------------------
QCase = namedtuple("QCase", "name R K ldx_x ldq_x lde_x", defaults=(0, 0, 0))
QCASES = [QCase("r1_k32", 1, 32), QCase("r257_k128", 257, 128, ldx_x=8, ldq_x=16, lde_x=3), QCase("r301_k384", 301, 384),
          QCase("r77_k384_pitches", 77, 384, ldx_x=16, ldq_x=32, lde_x=5), QCase("r513_k32_pitches", 513, 32, ldx_x=8, ldq_x=16, lde_x=1)]
VCase = namedtuple("VCase", "name H Lk ldvt_x ldvt8_x ldev_x", defaults=(0, 0, 0))
VCASES = [VCase("h1_k1", 1, 1, ldvt_x=3), VCase("h2_k127", 2, 127, ldvt_x=1, ldvt8_x=16, ldev_x=4), VCase("h1_k128", 1, 128),
          VCase("h3_k129", 3, 129, ldvt_x=7, ldvt8_x=32), VCase("h2_k300", 2, 300, ldev_x=8)]
BF16_MAX = 3.3895313892515355e38


def _quant_input(rows, cols, g):
    """rows of very different size, a zero block, a zero row, a block holding the largest bf16 and one holding its negative"""
    x = torch.randn(rows, cols, generator=g) * torch.pow(2.0, torch.randint(-20, 21, (rows, 1), generator=g).float())
    if cols >= 32:
        x[:, :32] *= 2.0 ** -9
    if rows > 2:
        x[2] = 0
    x[rows // 2, :min(cols, 32)] = 0
    x[0, cols - 1] = BF16_MAX
    x[rows - 1, 0] = -BF16_MAX
    return x.bfloat16()


def run_qcase(c, device="cuda"):
    """-> (x bf16 [R, K] on the CPU, q [R + 1, ldq], e [R + 1, lde] from the device, GUARD_BYTE where nothing may be stored)"""
    from yume_amd import ops as yops
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.encode()))
    xb = _quant_input(c.R, c.K + c.ldx_x, g)
    q = torch.full((c.R + 1, c.K + c.ldq_x), GUARD_BYTE, dtype=torch.uint8, device=device)
    e = torch.full((c.R + 1, c.K // 32 + c.lde_x), GUARD_BYTE, dtype=torch.uint8, device=device)
    yops.quant_rows_mx_e4m3(xb.to(device)[:, :c.K], q[:c.R, :c.K], e[:c.R, :c.K // 32])
    return xb[:, :c.K], q.cpu(), e.cpu()


def run_vcase(c, device="cuda"):
    """-> (vt bf16 [128 H, Lk] on the CPU, vt8 [128 H + 1, ldvt8], ev [tiles + 1, ldev] from the device; V^T columns >= Lk hold NaN)"""
    from yume_amd import ops as yops
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.encode()))
    C, T = c.H * D, tiles(c.Lk)
    ldvt = (c.Lk + c.ldvt_x + 3) // 4 * 4
    vb = torch.full((C, ldvt), float("nan"), dtype=torch.bfloat16)
    vb[:, :c.Lk] = _quant_input(C, c.Lk, g)
    vt8 = torch.full((C + 1, KEYS * T + c.ldvt8_x), GUARD_BYTE, dtype=torch.uint8, device=device)
    ev = torch.full((T + 1, 4 * C + c.ldev_x), GUARD_BYTE, dtype=torch.uint8, device=device)
    yops.attn_vt_mx_e4m3(vb.to(device), c.Lk, vt8[:C, :KEYS * T], ev[:T, :4 * C])
    return vb[:, :c.Lk], vt8.cpu(), ev.cpu()


# calls that must be refused before any launch: (name, entry, what differs from a valid call, a word of the message). The valid calls:
# rows R = 5, K = 128; vt C = 256, Lk = 300; fwd Lq = 300, Lk = 300, H = 2; every pitch minimal.
REFUSALS = [
    ("rows_x_null", "rows", dict(x=0), "NULL"), ("rows_e_null", "rows", dict(e=0), "NULL"), ("rows_k_48", "rows", dict(K=48, ldx=48, ldq=48), "K=48"),
    ("rows_lde_short", "rows", dict(lde=3), "lde=3"), ("rows_ldq_odd", "rows", dict(ldq=136), "ldq=136"), ("rows_ldx_short", "rows", dict(ldx=120), "ldx=120"),
    ("rows_pitch_2g", "rows", dict(ldq=1 << 31), "pitch"),
    ("vt_null", "vt", dict(Vt8=0), "NULL"), ("vt_c_130", "vt", dict(C=130), "C=130"), ("vt_lk_0", "vt", dict(Lk=0), "Lk=0"),
    ("vt_ldvt8_8", "vt", dict(ldvt8=384 + 8), "ldvt8=392"), ("vt_ldvt8_short", "vt", dict(ldvt8=256), "ldvt8=256"),
    ("vt_ldev_short", "vt", dict(ldev=1020), "ldev=1020"), ("vt_pitch_2g", "vt", dict(ldvt=1 << 31), "pitch"),
    ("fwd_q_null", "fwd", dict(Q8=0), "NULL"), ("fwd_ev_null", "fwd", dict(Ev=0), "NULL"), ("fwd_o_null", "fwd", dict(O=0), "NULL"),
    ("fwd_ldvt8_8", "fwd", dict(ldvt8=384 + 8), "ldvt8=392"), ("fwd_ldvt8_short", "fwd", dict(ldvt8=256), "ldvt8=256"),
    ("fwd_ldeq_short", "fwd", dict(ldeq=4), "ldeq=4"), ("fwd_ldek_odd", "fwd", dict(ldek=10), "ldek=10"), ("fwd_ldev_short", "fwd", dict(ldev=1020), "ldev=1020"),
    ("fwd_lq_0", "fwd", dict(Lq=0), "Lq=0"), ("fwd_lk_0", "fwd", dict(Lk=0), "Lk=0"), ("fwd_h_0", "fwd", dict(H=0), "H=0"),
    ("fwd_ldq_short", "fwd", dict(ldq=240), "ldq=240"), ("fwd_ldo_odd", "fwd", dict(ldo=258), "ldo=258"),
    ("fwd_q_misaligned", "fwd", dict(Q8=4096 + 8), "aligned"), ("fwd_ek_misaligned", "fwd", dict(Ek=4096 + 2), "aligned"),
    ("fwd_ldk_2g", "fwd", dict(ldk=1 << 31), "overflows the kernel's addressing"), ("fwd_ldo_2g", "fwd", dict(ldo=1 << 31), "overflows the kernel's addressing"),
]


def refusal_call(lib, entry, kw, ptr=4096):
    """a refusal row through the raw C-ABI with pointers that are never dereferenced -> the return code"""
    import ctypes
    P = lambda v: ctypes.c_void_p(v) if v else None
    g = lambda k, dflt: kw.get(k, dflt)
    if entry == "rows":
        K = g("K", 128)
        return lib.yume_quant_rows_mx_e4m3(P(g("x", ptr)), g("ldx", K), g("R", 5), K, P(g("q", ptr)), g("ldq", K), P(g("e", ptr)), g("lde", K // 32), None)
    if entry == "vt":
        C, Lk = g("C", 256), g("Lk", 300)
        return lib.yume_attn_vt_mx_e4m3(P(g("Vt", ptr)), g("ldvt", 300), C, Lk, P(g("Vt8", ptr)), g("ldvt8", 384), P(g("Ev", ptr)), g("ldev", 4 * C), None)
    H = g("H", 2)
    return lib.yume_attn_fwd_f8mx(P(g("Q8", ptr)), g("ldq", 256), P(g("Eq", ptr)), g("ldeq", 8), P(g("K8", ptr)), g("ldk", 256), P(g("Ek", ptr)),
                                  g("ldek", 8), P(g("Vt8", ptr)), g("ldvt8", 384), P(g("Ev", ptr)), g("ldev", 1024), P(g("O", ptr)), g("ldo", 256),
                                  g("Lq", 300), g("Lk", 300), H, None)


def emulation_ratios(cases, kappa=KAPPA8, out=sys.stdout):
    """the emulation's worst error / bound of every row at its own size, on the host (what KAPPA8 is settled from)"""
    for c in cases:
        ops = make_case(c)
        r = reference(c, ops)
        ratio = (emulate(c, ops) - r["ref"]).abs() / bound(r, kappa)
        out.write(f"{c.name}: worst error / bound {ratio.max().item():.3f}, {int((ratio > 1).sum())} of {ratio.numel()} elements outside\n")
        out.flush()


def main(argv):
    if argv == ["--emulate"]:
        return emulation_ratios(CASES)
    if argv != ["--routes"]:
        sys.exit(__doc__)
    for c in CASES:
        ops = make_case(c)
        dv = device_operands(c, ops)
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {c.name}\n")
        sys.stderr.flush()
        run_case(c, ops, dv)
        torch.cuda.synchronize()
    for c in QCASES:
        sys.stderr.write(f"CASE {c.name}\n")
        sys.stderr.flush()
        run_qcase(c)
        torch.cuda.synchronize()
    for c in VCASES:
        sys.stderr.write(f"CASE {c.name}\n")
        sys.stderr.flush()
        run_vcase(c)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main(sys.argv[1:])
