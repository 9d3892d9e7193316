"""The case table of the attention kernel routes, their fp64 reference, the per-element error bound and a host emulation of the kernels'
arithmetic (no test functions in here).

yume_attn_fwd / _ws / _kw / _seg are one entry point in front of seven kernels, their two segmented forms and a merge pass; the shape,
the flags, the variant, the weight, the scratch, three environment switches and the counter workspace pick among them.
tests/test_attn_routes_gpu.py runs one call per CASES row and holds EVERY output element to `bound()` against `reference()`;
tests/test_attn_cases_cpu.py proves the reference and the bound on the host at a shrunken copy of every row and checks that the bound
flags ten injected faults.

Operands are bf16. A correct kernel makes fp32 scores, rounds each P (w P for a weighted last key) to bf16 ONCE, accumulates P V and the
row sum in fp32 and rounds O / l (+ the old O of an accumulate call) to bf16 once:

    |got - ref| <= 2^-8 |ref + base|  +  KAPPA * 2^-9 sqrt(Q)  +  2^-20 (A + |base|)      A = sum_j a_ij |v_jd|,  Q = sum_j (a_ij v_jd)^2

  * 2^-8 |ref + base|: half a bf16 ulp of what is stored;
  * the roundings of the P of one row are independent, each at most 2^-8 of its P (half a bf16 ulp at the bottom of a binade, 2^-9 at
    the top; about 0.8 * 2^-9 rms): their sum walks about 0.8 * 2^-9 sqrt(Q) away, and KAPPA = 4.5 is 5.6 of these deviations. KAPPA is
    settled by the host emulation at the table's own sizes (`--emulate` below: no element outside on any row, which 4 misses on two
    rows of 4.3e6 elements) and by the injected faults (5 no longer flags a truncated output on four shrunken rows); the figures are in
    profiles/r11_attn_routes.md. It is never fitted to a kernel. The row sum is taken over the unrounded P;
  * 2^-20 (A + |base|): fp32 scores under the exponential, the fp32 sums, the product of the scale and log2(e) in fp32.
For a weighted last key a_ij is the key's whole weight (w times one copy's), since w P is rounded once.

Input patterns (Case.pattern) and operand forms (Case.form): `make_case` and `device_operands`.

    python tests/attn_cases.py --routes        one call per case, `CASE <name>` on stderr before each (YUME_ATTN_LOG=1 names the kernels)
    python tests/attn_cases.py --emulate       the host emulation's worst error / bound of every row at its full size (no GPU; minutes)
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

D = 128
KT = 64                      # keys per tile (attn_tile.hpp)
QBLOCK = 256                 # query rows per block of the v7 / v8 kernels (attn_plan.hpp)
SCALE = 1 / math.sqrt(D)
LOG2E = 1.4426950408889634
SENTINEL = 77.0              # guard rows, guard columns and pitch gaps of O
PAD_VALUE = 37.5             # V^T columns >= Lk under YUME_ATTN_KV_PADDED (finite junk)
GUARD_ROWS, GUARD_COLS = 8, 64
KAPPA = 4.5

# entry: "fwd" (ops.attn_fwd) or "seg" (ops.attn_fwd_seg: Lk and weight are tuples, one per segment; pitch = rows between segments).
# route: the kernel the YUME_ATTN_LOG line of the call must name; plan: (tail_qb, splits) it must carry (v7 / v8).
# workspace: the call hands over the scratch of the key-range split. acc: O += result.
Case = namedtuple("Case", "name entry variant Lq Lk H pattern form prescaled padded weight acc route plan pitch workspace",
                  defaults=(None, None, True))

STAIR_STEPS = (1, 7, 8, 9, 12, 13, 14, 20)
LEVELS = sorted(set(range(-160, -59, 4)) | set(range(-112, -87)) | set(range(60, 161, 4)) | set(range(100, 133)))
PEAK_SUM_LOG2 = 119
PEAK_DELTAS = tuple(range(8, 24))
HALVES = [(lv, dl) for lv in range(100, 128) for dl in range(13)]


def _fwd(name, variant, Lq, Lk, H, pattern, form, route, prescaled=False, padded=False, weight=1.0, acc=False, plan=None, workspace=True):
    return Case(name, "fwd", variant, Lq, Lk, H, pattern, form, prescaled, padded, weight, acc, route, plan, None, workspace)


def _table():
    rows = []
    # ---- v1 / v2 / v4 (variants 1, 2, 4): ragged and whole Lk around one and several key tiles, ragged Lq (two blocks and a tail)
    for kern, variant in (("v1", 1), ("v2", 2), ("v4", 4)):
        for n, Lk in enumerate((1, 63, 64, 65, 257, 640)):
            forms = ("tight", "engine_cross") if (n + variant) % 2 == 0 else ("engine_cross", "tight")
            rows.append(_fwd(f"{kern}_probe_k{Lk}", variant, 301, Lk, 3, "probe", forms[0], kern))
            if Lk > KT:            # (stairs need more than one key tile)
                rows.append(_fwd(f"{kern}_stairs_k{Lk}", variant, 301, Lk, 3, "stairs", forms[1], kern))
        rows.append(_fwd(f"{kern}_acc_k257", variant, 301, 257, 3, "probe", "engine_cross", kern, acc=True))
        rows.append(_fwd(f"{kern}_random_k257", variant, 301, 257, 3, "random", "tight", kern))
    # the engine's text cross-attention: automatic, both flags, 512 keys -> the 4-wave LDS-DMA kernel
    rows.append(_fwd("auto_cross_k512", 0, 301, 512, 3, "probe", "engine_cross", "v2", prescaled=True, padded=True))
    # ---- a weighted last key: the 4-wave kernel (2), the short-key kernel (10) and the automatic choice (0); both scale modes
    for n, Lk in enumerate((1, 2, 64, 65, 78, 128)):
        for m, (variant, route) in enumerate(((2, "v2w"), (10, "short"), (0, "short"))):
            pre = (n + m) % 2 == 1
            rows.append(_fwd(f"kw{variant}_k{Lk}", variant, 301, Lk, 3, "probe", "engine_cross", route, prescaled=pre, padded=pre, weight=435.0))
    rows.append(_fwd("kw10_k1_w1", 10, 301, 1, 3, "probe", "engine_cross", "short", weight=1.0))
    rows.append(_fwd("kw10_k128_w1", 10, 301, 128, 3, "probe", "engine_cross", "short", prescaled=True, padded=True, weight=1.0))
    rows.append(_fwd("kw10_random_k78", 10, 301, 78, 3, "random", "engine_cross", "short", weight=435.0))
    rows.append(_fwd("kw0_k300", 0, 301, 300, 3, "probe", "engine_cross", "v2w", weight=212.0))
    # ---- segments: two and three, different Lk and weights, a pitch gap (130 rows at a pitch of 192)
    seg = lambda name, variant, Lks, ws, route, pre=False, acc=False: Case(name, "seg", variant, 130, Lks, 3, "probe", "engine_cross", pre, pre,
                                                                           ws, acc, route, None, 192, False)
    rows.append(seg("seg_short_auto_3", 0, (78, 5, 128), (434.0, 507.0, 1.0), "seg_short", pre=True))
    rows.append(seg("seg_short_v10_2", 10, (78, 5), (434.0, 507.0), "seg_short", acc=True))
    rows.append(seg("seg_v2_v2_2", 2, (78, 300), (434.0, 212.0), "seg_v2"))
    rows.append(seg("seg_v2_auto_3", 0, (64, 513, 78), (1.0, 1.0, 434.0), "seg_v2", pre=True))
    # ---- rk (variant 9): K and V^T resident in registers, 448 < Lk <= 512
    rows.append(_fwd("rk_k449", 9, 1061, 449, 2, "probe", "engine_cross", "rk", prescaled=True, padded=True))
    rows.append(_fwd("rk_k512", 9, 1061, 512, 2, "probe", "engine_cross", "rk"))
    rows.append(_fwd("rk_random_k512", 9, 1061, 512, 2, "random", "tight", "rk"))
    # ---- v7: variant 7 (whole blocks only) and the automatic route without both flags. The v7 model plans every splits value 2, 3, 4
    # beside whole blocks from 33 query blocks per XCD slot on (tests/test_attn_cases_cpu.py holds the plans to attn_plan::search)
    rows.append(_fwd("v7_whole_probe", 7, 300, 1600, 2, "probe", "engine_self", "v7", plan=(2, 1)))
    rows.append(_fwd("v7_whole_stairs", 7, 300, 1600, 2, "stairs", "engine_self", "v7", plan=(2, 1)))
    rows.append(_fwd("v7_whole_random", 7, 300, 1600, 2, "random", "engine_self", "v7", plan=(2, 1)))
    rows.append(_fwd("v7_nows_probe", 0, 300, 2100, 2, "probe", "engine_self", "v7", plan=(2, 1), workspace=False))
    rows.append(_fwd("v7_s2_probe", 0, 8442, 2100, 1, "probe", "engine_self", "v7", plan=(32, 2)))
    rows.append(_fwd("v7_s2_stairs", 0, 8442, 2100, 1, "stairs", "engine_self", "v7", plan=(32, 2)))
    rows.append(_fwd("v7_s3_probe", 0, 8442, 3100, 1, "probe", "engine_self", "v7", plan=(32, 3)))
    rows.append(_fwd("v7_s4_stairs", 0, 8442, 4160, 1, "stairs", "engine_self", "v7", plan=(32, 4)))
    rows.append(_fwd("v7_s2_pre_acc", 0, 8442, 2100, 1, "probe", "engine_self", "v7", plan=(32, 2), prescaled=True, acc=True))
    rows.append(_fwd("v7_s2_pre_levels", 0, 8442, 2100, 4, "levels", "engine_self", "v7", plan=(32, 2), prescaled=True))
    rows.append(_fwd("v7_s2_pre_halves", 0, 8442, 2100, 4, "halves", "engine_self", "v7", plan=(32, 2), prescaled=True))
    rows.append(_fwd("v7_s2_pre_peak", 0, 8442, 2100, 2, "peak", "engine_self", "v7", plan=(32, 2), prescaled=True))
    rows.append(_fwd("v7_s3_pre_halves", 0, 8442, 3100, 4, "halves", "engine_self", "v7", plan=(32, 3), prescaled=True))
    # ---- v8: variant 8 and the automatic route with both flags and a counter workspace (Lk >= 1536)
    v8 = lambda name, variant, Lq, Lk, H, pattern, plan, acc=False: _fwd(name, variant, Lq, Lk, H, pattern, "engine_self", "v8", plan=plan,
                                                                          prescaled=True, padded=True, acc=acc)
    rows.append(v8("v8_whole_probe", 8, 300, 520, 1, "probe", (2, 1)))
    rows.append(v8("v8_whole_random", 8, 300, 520, 1, "random", (2, 1)))
    rows.append(v8("v8_s2_probe", 8, 8442, 1030, 1, "probe", (32, 2)))                 # fewer heads than XCDs
    rows.append(v8("v8_s2_h9_probe", 8, 4346, 1030, 9, "probe", (16, 2)))              # more than 8 heads: two heads on XCD 0
    rows.append(v8("v8_s3_auto_stairs", 0, 8442, 1600, 1, "stairs", (32, 3)))
    rows.append(v8("v8_s4_auto_probe", 0, 8442, 2100, 1, "probe", (32, 4), acc=True))
    rows.append(v8("v8_s2_levels", 8, 8442, 1030, 4, "levels", (32, 2)))
    rows.append(v8("v8_s2_halves", 8, 8442, 1030, 4, "halves", (32, 2)))
    rows.append(v8("v8_s2_peak", 8, 8442, 1030, 2, "peak", (32, 2)))
    rows.append(v8("v8_s4_auto_halves", 0, 8442, 2100, 4, "halves", (32, 4)))
    return rows


CASES = _table()
ROUTES = ("v1", "v2", "v2w", "v4", "v7", "v8", "rk", "short", "seg_short", "seg_v2")
MAX_WORK = 8500 * 2100 * 8


def segments(c):
    """[(Lk, weight)] of the call's segments (one for entry "fwd")"""
    return list(zip(c.Lk, c.weight)) if c.entry == "seg" else [(c.Lk, c.weight)]


def split_rows(c):
    """(first query row cut into key ranges, splits); (Lq, 1) where the row's plan does not split"""
    if c.plan is None or c.plan[1] == 1:
        return c.Lq, 1
    return c.plan[0] * QBLOCK, c.plan[1]


def shrink(c):
    """the same key structure (Lk, tiles, weights, pattern, scale mode, splits) with at most 2 heads and 160 queries; a split row keeps
    96 whole-block rows in front of 64 rows cut into key ranges"""
    Lq = min(c.Lq, 160)
    plan = c.plan
    if plan is not None and plan[1] > 1:
        plan = (96 / QBLOCK, plan[1])
    return c._replace(name=c.name + "_small", Lq=Lq, H=min(c.H, 2), plan=plan, pitch=None if c.pitch is None else Lq + 30)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16)


def probe_walk(Lq, Lk):
    """j(i): the key query i is pulled toward — the last 66 keys first, then the first 66, then the keys within 2 of every multiple of 64,
    then all keys, spread evenly over the rows that are left"""
    order, seen = [], set()
    special = list(range(Lk - 1, max(Lk - 67, -1), -1)) + list(range(min(66, Lk)))
    special += [m + o for m in range(KT, Lk + 3, KT) for o in (-2, -1, 0, 1, 2)]
    for j in special:
        if 0 <= j < Lk and j not in seen:
            seen.add(j)
            order.append(j)
    j = torch.tensor(order, dtype=torch.long)
    if Lq <= len(order):
        return j[:Lq]
    rest = Lq - len(order)
    spread = (torch.arange(rest, dtype=torch.long) * Lk) // rest
    return torch.cat([j, spread])


def _slot_values(values, Lq, H, lo, hi):
    """values[idx] for the slots (head-major) of the query rows [lo, hi): contiguous bands in the order of `values` when there are more
    slots than values, an even sample of them otherwise -> index tensor [hi - lo, H]"""
    R = hi - lo
    slot = torch.arange(H).view(1, H) * R + torch.arange(R).view(R, 1)
    return (slot * len(values)) // (R * H)


def make_case(c):
    """seeded operands on the CPU: {"segs": [{"q", "k", "v" bf16 [L, H, 128], "w" last-key weight}], "base": the old O of an accumulate
    call, bf16 [rows of the call, H * 128], or None, "scale_log2": what multiplies q.k in the exponent of 2 (fp32)}.
    Patterns:
      random  q, k, v ~ N(0, 1)
      probe   q_i = 0.5 r_i + g k_j(i), j(i) = probe_walk: key j(i) holds about half the weight of row i
      levels  (pre-scaled q) feature 0 of q is level / 8 against k[:, :, 0] = 8: a constant score offset per row, LEVELS in ascending bands
              over the whole-block rows and again over the rows cut into key ranges, heads first
      halves  as levels over the HALVES grid (level, delta): feature 1 of q is delta / 8 against k[j, :, 1] = 8 for the keys of the upper
              half of the key tiles (0 below): the pieces of one row land on different sides of the base-free body's range check
      peak    (pre-scaled q, two key ranges; beyond the grid of `halves`, which cannot reach this) every row carries the level that puts
              the row sum of the FIRST piece just under 2^PEAK_SUM_LOG2, inside the base-free range, and ONE key of the second piece
              (in its second tile) lies PEAK_DELTAS above the level: that piece overflows, is redone on the robust body and comes back
              with a base of 118 ... 132, so the merge scales the first piece — up to 2^-7 of the row — by 2^-118 ... 2^-132, down into
              the denormal range of the hardware's exp2
      stairs  (plain scale; pre-scaled on v8, where it sends every item through the rerun on the robust body) feature 0 of k is the key's tile index t, feature 0 of q is +-step / scale_log2: key tile t carries the offset
              step * t in the log2 domain, ascending and descending by turns in groups of 16 rows, step walking STAIR_STEPS every 32 rows"""
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.split("_small")[0].encode()))
    scale_log2 = 1.0 if c.prescaled else float(torch.tensor(SCALE, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    H, Lq = c.H, c.Lq
    segs = []
    for Lk, w in segments(c):
        r = torch.randn(Lq, H, D, generator=g)
        k = _bf16(torch.randn(Lk, H, D, generator=g)).float()
        v = _bf16(torch.randn(Lk, H, D, generator=g))
        q = r
        if c.pattern == "probe":
            gain = (math.log(Lk) + 0.3) / (SCALE * D) if Lk > 1 else 0.5
            q = 0.5 * r + gain * k[probe_walk(Lq, Lk)]
        if c.pattern == "stairs":
            assert Lk > KT
            k[:, :, 0] = (torch.arange(Lk) // KT).view(Lk, 1).float()
        if c.prescaled:
            q = q * (SCALE * LOG2E)
        q = _bf16(q).float()
        if c.pattern == "stairs":
            grp = torch.arange(Lq) // 16
            step = torch.tensor(STAIR_STEPS, dtype=torch.float32)[(grp // 2) % len(STAIR_STEPS)]
            q[:, :, 0] = _bf16((1 - 2 * (grp % 2)).float() * step / scale_log2).float().view(Lq, 1)
        if c.pattern in ("levels", "halves"):
            assert c.prescaled
            values = LEVELS if c.pattern == "levels" else HALVES
            lo, _ = split_rows(c)
            lo = int(lo)
            idx = torch.cat([_slot_values(values, Lq, H, a, b) for a, b in ((0, lo), (lo, Lq)) if b > a])
            tab = torch.tensor([(x, 0) if c.pattern == "levels" else x for x in values], dtype=torch.float32)
            k[:, :, 0] = 8.0
            q[:, :, 0] = tab[idx, 0] / 8
            if c.pattern == "halves":
                upper = (torch.arange(Lk) // KT) >= ((Lk + KT - 1) // KT) // 2
                k[:, :, 1] = upper.float().view(Lk, 1) * 8.0
                q[:, :, 1] = tab[idx, 1] / 8
        if c.pattern == "peak":
            assert c.prescaled and split_rows(c)[1] == 2
            lower = ((Lk + KT - 1) // KT) // 2 * KT                         # keys of the first piece
            k[:, :, 0] = 8.0
            q[:, :, 0] = float(PEAK_SUM_LOG2 - math.ceil(math.log2(lower) + 1)) / 8
            k[:, :, 1] = 0.0
            k[lower + KT + 6, :, 1] = 8.0
            q[:, :, 1] = torch.tensor(PEAK_DELTAS, dtype=torch.float32)[torch.arange(Lq) % len(PEAK_DELTAS)].view(Lq, 1) / 8
        assert torch.equal(_bf16(q).float(), q) and torch.equal(_bf16(k).float(), k)
        segs.append({"q": _bf16(q), "k": _bf16(k), "v": v, "w": float(w)})
    base = _bf16(torch.randn(call_rows(c), H * D, generator=g)) if c.acc else None
    return {"segs": segs, "base": base, "scale_log2": scale_log2}


def call_rows(c):
    """query rows the call spans (the pitch gaps of a segmented call included)"""
    return c.Lq if c.entry == "fwd" else (len(c.Lk) - 1) * c.pitch + c.Lq


def seg_base(c, ops, s):
    """the old O of segment s as [Lq, H, 128] (None without accumulate)"""
    if ops["base"] is None:
        return None
    r0 = s * (c.pitch or 0)
    return ops["base"][r0:r0 + c.Lq].view(c.Lq, c.H, D)


# ---- reference ---------------------------------------------------------------------------------------------------------------------------
CHUNK_BYTES = 256 << 20


def reference_one(q, k, v, w, scale_log2, device="cpu", chunk_bytes=CHUNK_BYTES):
    """exact softmax attention of one segment in fp64, head by head, in chunks of queries whose score matrix stays under chunk_bytes:
    q [Lq, H, 128], k, v [Lk, H, 128], the last key counting w times -> "ref", "A" = sum_j a_ij |v_jd|, "Q" = sum_j (a_ij v_jd)^2, each
    [Lq, H, 128] fp64 on `device` (a_ij: the whole weight of key j in row i)."""
    Lq, H, _ = q.shape
    Lk = k.shape[0]
    out = {n: torch.empty(Lq, H, D, dtype=torch.float64, device=device) for n in ("ref", "A", "Q")}
    rows = max(1, chunk_bytes // (8 * Lk))
    lw = torch.zeros(Lk, dtype=torch.float64, device=device)
    lw[-1] = math.log2(w)
    for h in range(H):
        kh = k[:, h].to(device, torch.float64)
        vh = v[:, h].to(device, torch.float64)
        for r0 in range(0, Lq, rows):
            x = (q[r0:r0 + rows, h].to(device, torch.float64) @ kh.T) * scale_log2 + lw
            a = torch.exp2(x - x.max(dim=1, keepdim=True).values)
            a /= a.sum(dim=1, keepdim=True)
            out["ref"][r0:r0 + rows, h] = a @ vh
            out["A"][r0:r0 + rows, h] = a @ vh.abs()
            out["Q"][r0:r0 + rows, h] = (a * a) @ (vh * vh)
    return out


def reference(c, ops, device="cpu", chunk_bytes=CHUNK_BYTES):
    """one reference per segment: [{"ref", "A", "Q", "base" (fp64 [Lq, H, 128], zeros without accumulate)}]"""
    res = []
    for s, sg in enumerate(ops["segs"]):
        r = reference_one(sg["q"], sg["k"], sg["v"], sg["w"], ops["scale_log2"], device, chunk_bytes)
        b = seg_base(c, ops, s)
        r["base"] = b.to(device, torch.float64) if b is not None else torch.zeros((), dtype=torch.float64, device=device)
        res.append(r)
    return res


def bound(r, kappa=KAPPA):
    """the per-element error a correct kernel may show against r["ref"] + r["base"] (module docstring)"""
    return 2.0 ** -8 * (r["ref"] + r["base"]).abs() + kappa * 2.0 ** -9 * r["Q"].sqrt() + 2.0 ** -20 * (r["A"] + r["base"].abs())


# ---- host emulation of the kernels' arithmetic -----------------------------------------------------------------------------------------------
FAULTS = ("lost_last_key", "last_key_twice", "pad_column", "v_rows_swapped", "scale_bf16", "small_exp_flushed", "truncated", "merge_no_factor",
          "merge_flushed", "weight_one")


def fault_applies(c, fault):
    """is the corruption one the bound has to flag on this row? Where it changes what a kernel of the row computes by more than the
    roundings of a correct one:
      * one key (Lk == 1) is a copy of its V row whatever the scores, the scale and the weight are;
      * the pad column's score 0 lies 100 and more below every score of a `halves` or `peak` row: its weight is under 2^-100;
      * a rounded scale (0.2 % off) moves the weights of a row with a spread of scores: not where one weighted key holds all but 2^-8;
      * flushed small exponentials show on rows that are not flat (probe) with enough keys below 2^-12 of the base to matter (Lk >= 128);
      * a truncated output is a whole bf16 ulp off at worst: it shows where the roundings of P are small beside the output, on flat rows
        (random, levels, halves, stairs) and under the old O of an accumulate call, not beside a probe key's own rounding;
      * in-range base-free pieces all carry the base 0 (factor 1): the merge factor matters where a robust body ran, and it reaches
        the denormal range on `peak` rows only."""
    lks = [lk for lk, _ in segments(c)]
    lk_min, lk_max = min(lks), max(lks)
    weighted = any(w != 1.0 for _, w in segments(c))
    return {"lost_last_key": lk_min >= 2, "last_key_twice": lk_min >= 2,
            "pad_column": any(lk % KT for lk in lks) and c.pattern not in ("halves", "peak"),
            "v_rows_swapped": lk_min >= 2,
            "scale_bf16": not c.prescaled and lk_max >= 2 and not (weighted and lk_max <= 2),
            "small_exp_flushed": c.pattern == "probe" and lk_max >= 128,
            "truncated": c.pattern not in ("probe", "peak") or c.acc,
            "merge_no_factor": split_rows(c)[1] > 1 and (not c.prescaled or c.pattern in ("levels", "halves", "stairs", "peak")),
            "merge_flushed": c.pattern == "peak",
            "weight_one": weighted and lk_max >= 2}[fault]


def _round_bf16(t, truncate=False):
    if truncate:
        return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)
    return t.to(torch.bfloat16).float()


def emulate_one(q, k, v, w, scale_log2, prescaled, base=None, split=(None, 1), fault=None):
    """what a correct kernel stores for one segment, on the CPU in fp32: scores from the bf16 operands, exp2 against the row's base (plain
    scale) or base-free (pre-scaled q: exp2 of the score itself, results under 2^-126 flushed; a piece outside 2^-100 < l < 2^120,
    |O| < 2^120 is redone against its base), ONE bf16 rounding of w P, fp32 row sum and accumulation, the pieces of a split row merged as
    attn_combine.hpp does, one bf16 rounding of O / l (+ base). -> fp64 [Lq, H, 128]"""
    Lq, H, _ = q.shape
    Lk = k.shape[0]
    qf, kf, vf = q.float(), k.float(), v.float()
    W = torch.ones(Lq, Lk)
    W[:, -1] = 1.0 if fault == "weight_one" else w
    if fault == "lost_last_key":
        W[-32:, -1] = 0.0
    if fault == "last_key_twice":
        W[:, -1] *= 2
    if fault == "v_rows_swapped":
        vf = vf.clone()
        vf[[Lk - 1, Lk - 2]] = vf[[Lk - 2, Lk - 1]]
    if fault == "pad_column":          # a key of score 0 whose V row is the finite junk of the padding
        kf = torch.cat([kf, torch.zeros(1, H, D)])
        vf = torch.cat([vf, torch.full((1, H, D), PAD_VALUE)])
        W = torch.cat([W, torch.ones(Lq, 1)], dim=1)
    c2 = torch.tensor(scale_log2, dtype=torch.float32)
    if fault == "scale_bf16":
        c2 = _round_bf16(c2)
    lo, splits = split
    lo = Lq if lo is None or splits == 1 else int(lo)
    nt = (Lk + KT - 1) // KT
    out = torch.empty(Lq, H, D, dtype=torch.float32)

    def piece(x, Wp, vp, basefree):
        """-> (m, l, O): the base, the fp32 row sum and the unnormalised fp32 O of the keys given"""
        live = Wp > 0
        m = torch.where(live, x, torch.full_like(x, -float("inf"))).max(dim=1, keepdim=True).values
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))

        def body(mm):
            e = x - mm
            p = torch.where(e < -126.0, torch.zeros_like(e), torch.exp2(e))
            if fault == "small_exp_flushed":
                p = torch.where(e - (m - mm) < -12.0, torch.zeros_like(p), p)
            p = p * Wp
            return p.sum(dim=1, keepdim=True), _round_bf16(p) @ vp

        if basefree:
            zero = torch.zeros_like(m)
            l0, o0 = body(zero)
            ok = torch.isfinite(l0) & (l0 > 2.0 ** -100) & (l0 < 2.0 ** 120) & (o0.abs().amax(dim=1, keepdim=True) < 2.0 ** 120)
            l1, o1 = body(m)
            return torch.where(ok, zero, m), torch.where(ok, l0, l1), torch.where(ok, o0, o1)
        l1, o1 = body(m)
        return m, l1, o1

    for h in range(H):
        x = (qf[:, h] @ kf[:, h].T) * c2
        vh = vf[:, h]
        if lo > 0:
            _, l, o = piece(x[:lo], W[:lo], vh, prescaled)
            out[:lo, h] = o / l
        if lo < Lq:
            parts = []
            for s in range(splits):
                j0, j1 = nt * s // splits * KT, min(nt * (s + 1) // splits * KT, x.shape[1])
                if s == splits - 1:
                    j1 = x.shape[1]
                parts.append(piece(x[lo:, j0:j1], W[lo:, j0:j1], vh[j0:j1], prescaled))
            m = torch.stack([p[0] for p in parts]).max(dim=0).values
            l = torch.zeros_like(m)
            acc = torch.zeros(Lq - lo, D)
            for ms, ls, os_ in parts:
                a = torch.ones_like(m) if fault == "merge_no_factor" else torch.exp2(ms - m)
                if fault == "merge_flushed":       # what an exp2 that flushes denormal results makes of a factor under 2^-126
                    a = torch.where(ms - m < -126.0, torch.zeros_like(a), a)
                l = l + ls * a
                acc = acc + os_ * a
            out[lo:, h] = acc * (1.0 / l)
    if base is not None:
        out = out + base.float()
    return _round_bf16(out, truncate=fault == "truncated").double()


def emulate(c, ops, fault=None):
    """[fp64 [Lq, H, 128]] per segment"""
    return [emulate_one(sg["q"], sg["k"], sg["v"], sg["w"], ops["scale_log2"], c.prescaled, seg_base(c, ops, s), split_rows(c), fault)
            for s, sg in enumerate(ops["segs"])]


# ---- the call on the device ------------------------------------------------------------------------------------------------------------------
def device_operands(c, ops, device="cuda"):
    """the operands in the row's form; everything a kernel must not use holds NaN (q rows outside the call's, pitch gaps, k rows >= Lk, the
    neighbours' columns and rows, V^T columns >= Lk — PAD_VALUE there under YUME_ATTN_KV_PADDED), everything it must not write SENTINEL.
      tight         q [rows, HC], k [Lk, HC], V^T [HC, Lk up to 8], O [rows, HC]                        (HC = H * 128)
      engine_self   q = the left column half of one [.., 2 HC] buffer from row GUARD_ROWS on, k = its right half from row 0;
                    V^T a row slice of a taller buffer; O a row-offset view of a buffer with GUARD_ROWS rows around and GUARD_COLS columns behind
      engine_cross  k = the middle column block of [Lk up to 64, 3 HC], V^T the matching row slice of [3 HC, ..]; q with NaN rows behind; O guarded
    -> {"q", "ks", "vts", "o", "obuf", "o_rows": (first row, rows) of o in obuf}"""
    nan = float("nan")
    H, HC, rows = c.H, c.H * D, call_rows(c)
    segs = ops["segs"]
    lk_max = max(sg["k"].shape[0] for sg in segs)
    q2 = torch.full((rows, HC), nan, dtype=torch.bfloat16)
    for s, sg in enumerate(segs):
        r0 = s * (c.pitch or 0)
        q2[r0:r0 + c.Lq] = sg["q"].reshape(c.Lq, HC)
    ldvt = (lk_max + KT - 1) // KT * KT if c.padded else (lk_max + 7) // 8 * 8
    ks, vts = [], []
    if c.form == "engine_self":
        assert len(segs) == 1
        Lk = lk_max
        alloc = max(GUARD_ROWS + rows + GUARD_ROWS, (Lk + KT - 1) // KT * KT)
        qk = torch.full((alloc, 2 * HC), nan, dtype=torch.bfloat16)
        qk[GUARD_ROWS:GUARD_ROWS + rows, :HC] = q2
        qk[:Lk, HC:] = segs[0]["k"].reshape(Lk, HC)
        qk = qk.to(device)
        q = qk[GUARD_ROWS:GUARD_ROWS + rows, :HC]
        ks.append(qk[:Lk, HC:])
    else:
        qb = torch.full((rows + GUARD_ROWS, HC), nan, dtype=torch.bfloat16)
        qb[:rows] = q2
        q = qb.to(device)[:rows]
    for sg in segs:
        Lk = sg["k"].shape[0]
        if c.form == "engine_cross":
            kb = torch.full(((Lk + KT - 1) // KT * KT, 3 * HC), nan, dtype=torch.bfloat16)
            kb[:Lk, HC:2 * HC] = sg["k"].reshape(Lk, HC)
            ks.append(kb.to(device)[:Lk, HC:2 * HC])
        elif c.form == "tight":
            ks.append(sg["k"].reshape(Lk, HC).to(device))
        above = {"tight": 0, "engine_self": D, "engine_cross": HC}[c.form]
        vb = torch.full((above + HC + above, ldvt), nan, dtype=torch.bfloat16)
        vb[above:above + HC, :Lk] = sg["v"].reshape(Lk, HC).T
        if c.padded:
            vb[above:above + HC, Lk:] = PAD_VALUE
        vts.append(vb.to(device)[above:above + HC])
    if c.form == "tight":
        obuf = torch.full((rows, HC), SENTINEL, dtype=torch.bfloat16)
        r0 = 0
    else:
        obuf = torch.full((GUARD_ROWS + rows + GUARD_ROWS, HC + GUARD_COLS), SENTINEL, dtype=torch.bfloat16)
        r0 = GUARD_ROWS
    if ops["base"] is not None:
        for s in range(len(segs)):
            a = r0 + s * (c.pitch or 0)
            obuf[a:a + c.Lq, :HC] = ops["base"][a - r0:a - r0 + c.Lq]
    obuf = obuf.to(device)
    return {"q": q, "ks": ks, "vts": vts, "obuf": obuf, "o": obuf[r0:r0 + rows, :HC], "o_rows": (r0, rows)}


def run_case(c, ops, dev_ops=None):
    """one call into fresh operands (or `dev_ops`) -> the device operands; the result is in ["obuf"]"""
    from yume_amd import ops as yops
    d = dev_ops or device_operands(c, ops)
    scale = None if c.prescaled else SCALE
    if c.entry == "seg":
        yops.attn_fwd_seg(d["q"], d["ks"], d["vts"], d["o"], c.Lq, c.pitch, list(c.Lk), c.H, scale=scale, accumulate=c.acc, variant=c.variant,
                          q_prescaled=c.prescaled, kv_padded=c.padded, last_key_weights=list(c.weight))
    else:
        yops.attn_fwd(d["q"], d["ks"][0], d["vts"][0], d["o"], c.Lq, c.Lk, c.H, scale=scale, accumulate=c.acc, variant=c.variant,
                      use_workspace=c.workspace, q_prescaled=c.prescaled, kv_padded=c.padded, last_key_weight=c.weight)
    return d


def written(c, d):
    """(per-segment results [Lq, H, 128] fp64, everything else of obuf as one flat tensor: guard rows, guard columns, pitch gaps)"""
    r0, rows = d["o_rows"]
    HC = c.H * D
    obuf = d["obuf"]
    mask = torch.ones_like(obuf, dtype=torch.bool)
    res = []
    for s in range(len(d["ks"])):
        a = r0 + s * (c.pitch or 0)
        res.append(obuf[a:a + c.Lq, :HC].double().view(c.Lq, c.H, D))
        mask[a:a + c.Lq, :HC] = False
    return res, obuf[mask]


def route_of(line):
    """`[attn_fwd] v8 tail_qb=32 splits=2 nwg=256 Lq=...` -> ("v8", (32, 2)); the plan is None for the kernels that carry none"""
    f = line.split()
    kv = dict(t.split("=", 1) for t in f[2:] if "=" in t)
    plan = (int(kv["tail_qb"]), int(kv["splits"])) if "tail_qb" in kv else None
    return f[1], plan


def emulation_ratios(cases, kappa=KAPPA, out=sys.stdout):
    """the emulation's worst error / bound of every row at its own size, on the host (minutes: what KAPPA is settled from)"""
    for c in cases:
        ops = make_case(c)
        worst, outside, n = 0.0, 0, 0
        for got, r in zip(emulate(c, ops), reference(c, ops)):
            ratio = (got - (r["ref"] + r["base"])).abs() / bound(r, kappa)
            worst, outside, n = max(worst, ratio.max().item()), outside + int((ratio > 1).sum()), n + ratio.numel()
        out.write(f"{c.name}: worst error / bound {worst:.3f}, {outside} of {n} elements outside\n")
        out.flush()


def main(argv):
    if argv == ["--emulate"]:
        return emulation_ratios(CASES)
    if argv != ["--routes"]:
        sys.exit(__doc__)
    from yume_amd import ops as yops
    yops.ensure_counters(torch.device("cuda", torch.cuda.current_device()))      # (v8 draws its tickets from the registered counter workspace)
    for c in CASES:
        ops = make_case(c)
        d = device_operands(c, ops)
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {c.name}\n")
        sys.stderr.flush()
        run_case(c, ops, d)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main(sys.argv[1:])
