"""The case table of the sliding-window / causal attention entry point (yume_attn_fwd_band, yume_amd/csrc/attn_band.hpp), its fp64
reference, and a host emulation of the kernel's arithmetic with injected faults (no test functions in here). The per-element bound is
tests/attn_cases.py's `bound()` unchanged (KAPPA = 4.5 from r11, not re-fitted), the operand forms and guards are its `device_operands`.

    pos(i) = q_pos0 + i
    visible(i, j)  <=>  0 <= j < Lk  and  (left < 0 or j >= pos(i) - left)  and  (right < 0 or j <= pos(i) + right)
    O[i] = exact softmax over the visible keys;  O[i] = 0 where row i sees none (an accumulate call leaves the old O[i] as it is)

A hidden key has a_ij = 0, so a row without a visible key has ref = A = Q = 0 and its bound is 0 (+ the rounding of the old O, which a
correct kernel does not touch): it must be exact.

tests/test_attn_band_routes_gpu.py runs one call per CASES row and per NORMALISED row; tests/test_attn_band_cases_cpu.py proves the
reference, the Python mirror of attn_band_plan.hpp and the bound's reach over the faults on the host.

    python tests/attn_band_cases.py --routes      one call per CASES and NORMALISED row, `CASE <name>` on stderr before each
"""
import math
import os
import sys
import zlib
from collections import namedtuple

import torch

import attn_cases as ac
from attn_cases import D, GUARD_COLS, GUARD_ROWS, KAPPA, KT, LOG2E, PAD_VALUE, SCALE, SENTINEL, bound, device_operands, written  # noqa: F401

QB = 128                     # query rows per workgroup of attn_band_kernel (attn_band_plan.hpp)
# `ramp` / `ramp4`: the score of key j in the log2 domain is RAMP_STEP * (j % 64) for every query. The fault a ramp is there for — the row
# maximum taken before the mask — shows only where the base lies MORE than 126 above a row's visible scores: exp2(-126) is the smallest
# normal fp32 (and bf16) number, nothing is flushed at exactly 126, P, l and P V are all scaled by the same power of two and O / l comes
# out the same to 2^-22. Under the step of 2 the largest gap is 2 * 63 = 126: on those two rows the faulty emulation differs from the
# correct one by nothing the bound could see (tests/test_attn_band_cases_cpu.py prints the figures). They stay in the table as the rows
# they are (hidden scores far above the visible ones, which the kernel must not let into the base); the step of 4 (gaps up to 252, still
# bf16-exact) is where the fault flushes whole rows and must be flagged.
RAMP_STEP = {"ramp": 2, "ramp4": 4}

BandCase = namedtuple("BandCase", "name Lq Lk q_pos0 left right H pattern form prescaled padded acc", defaults=(3, "edge_probe", "engine_self",
                                                                                                              False, False, False))


def _table():
    rows = []
    forms = ("engine_self", "tight", "engine_cross")
    for n, (l, r) in enumerate(((0, 0), (63, 0), (64, 64), (1, 130), (-1, 0), (0, -1), (100, -1), (-1, 37))):
        tag = f"l{l}_r{r}".replace("-1", "inf")
        rows.append(BandCase(f"self_{tag}", 301, 301, 0, l, r, form=forms[n % 3], pattern="random" if n in (2, 6) else "edge_probe"))
    rows.append(BandCase("cross_k640_pos339", 301, 640, 339, 70, 70, form="engine_cross"))
    rows.append(BandCase("causal_k257_neg44", 301, 257, -44, -1, 0, form="engine_cross"))          # rows 0 ... 43 see no key
    rows.append(BandCase("causal_k100_neg201", 301, 100, -201, -1, 0, form="tight"))               # the whole first workgroup sees none
    rows.append(BandCase("trimmed_s128", 173, 301, 128, 70, 70))                                   # the trimmed last block: q_pos0 = s
    rows.append(BandCase("long_l300_r200", 1500, 1500, 0, 300, 200, H=2, pattern="random"))
    rows.append(BandCase("ramp_causal", 301, 301, 0, -1, 0, pattern="ramp", prescaled=True))
    rows.append(BandCase("ramp_l5", 301, 301, 0, 5, 0, pattern="ramp", prescaled=True))
    # (the same two windows under the steeper ramp: 4 (j % 64), hidden keys up to 252 above — see RAMP_STEP)
    rows.append(BandCase("ramp4_causal", 301, 301, 0, -1, 0, pattern="ramp4", prescaled=True))
    rows.append(BandCase("ramp4_l5", 301, 301, 0, 5, 0, pattern="ramp4", prescaled=True))
    rows.append(BandCase("acc_empty_rows", 301, 257, -44, -1, 0, form="engine_cross", acc=True))   # the old O of rows 0 ... 43 survives
    rows.append(BandCase("prescaled_l64_r64", 301, 301, 0, 64, 64, prescaled=True))
    rows.append(BandCase("plain_scale_l17_r5", 301, 301, 0, 17, 5, form="tight"))
    rows.append(BandCase("kv_padded_l70_r70", 301, 301, 0, 70, 70, prescaled=True, padded=True))   # PAD_VALUE junk behind Lk
    return rows


CASES = _table()
# calls that hide no (row, key) pair: the ordinary `[attn_fwd] ...` call, bit for bit
NORMALISED = [BandCase("norm_l300_r300", 301, 301, 0, 300, 300, pattern="random"),
              BandCase("norm_linf_r300", 301, 301, 0, -1, 300, pattern="random", form="tight"),
              BandCase("norm_trimmed", 173, 301, 128, 300, 172, pattern="random"),
              BandCase("norm_pre_padded", 301, 301, 0, 300, -1, pattern="random", prescaled=True, padded=True)]
# what the entry point must refuse: (name, keyword overrides of a valid call, error code, a word of the message)
EINVAL, EUNSUP = -1, -3
REFUSALS = [("left_minus_2", dict(left=-2), EINVAL, "win_left"), ("right_minus_7", dict(right=-7), EINVAL, "win_right"),
            ("variant_7", dict(variant=7), EUNSUP, "variant 7"), ("variant_2_flags", dict(variant=2 | 0x100 | 0x200), EUNSUP, "variant 2"),
            ("null_q", dict(Q=None), EINVAL, "NULL"), ("null_k", dict(K=None), EINVAL, "NULL"), ("null_vt", dict(Vt=None), EINVAL, "NULL"),
            ("null_o", dict(O=None), EINVAL, "NULL"), ("misaligned_q", dict(Q=4096 + 8), EINVAL, "alignment"),
            ("misaligned_k", dict(K=4096 + 2), EINVAL, "alignment"), ("misaligned_o", dict(O=4096 + 4), EINVAL, "alignment"),
            ("q_pos0_2_31", dict(q_pos0=2 ** 31), EINVAL, "q_pos0"), ("q_pos0_below", dict(q_pos0=-2 ** 31 - 1), EINVAL, "q_pos0"),
            ("ldvt_short", dict(ldvt=64), EINVAL, "ldvt"), ("empty", dict(Lq=0), EINVAL, "empty")]


def as_case(c):
    """the tests/attn_cases.py row whose operand-form helpers (device_operands, written, call_rows) serve this one"""
    return ac.Case(c.name, "fwd", 0, c.Lq, c.Lk, c.H, c.pattern, c.form, c.prescaled, c.padded, 1.0, c.acc, "band", None, None, False)


def shrink(c):
    """the same rows, keys and window (the band structure IS the case) on at most 2 heads"""
    return c._replace(name=c.name + "_small", H=min(c.H, 2))


# ---- the window: Python mirror of yume_amd/csrc/attn_band_plan.hpp --------------------------------------------------------------------------
def key_range(q_first, q_last, Lk, q_pos0, left, right):
    """(lo, hi) inclusive: the keys some row of q_first ... q_last sees; lo > hi: none"""
    lo = 0 if left < 0 else max(0, q_pos0 + q_first - left)
    hi = Lk - 1 if right < 0 else min(Lk - 1, q_pos0 + q_last + right)
    return lo, hi


def tile_range(q_first, q_last, Lk, q_pos0, left, right):
    lo, hi = key_range(q_first, q_last, Lk, q_pos0, left, right)
    return (0, -1) if lo > hi else (lo // KT, hi // KT)


def tile_is_interior(t, q_first, q_last, Lk, q_pos0, left, right):
    k0, k1 = t * KT, t * KT + KT - 1
    return k1 < Lk and (left < 0 or k0 >= q_pos0 + q_last - left) and (right < 0 or k1 <= q_pos0 + q_first + right)


def hides_nothing(Lq, Lk, q_pos0, left, right):
    return (left < 0 or q_pos0 + Lq - 1 - left <= 0) and (right < 0 or q_pos0 + right >= Lk - 1)


def block_tiles(c):
    """[(t_lo, t_hi)] of the 128-row workgroups of the call"""
    return [tile_range(q, min(q + QB, c.Lq) - 1, c.Lk, c.q_pos0, c.left, c.right) for q in range(0, c.Lq, QB)]


def tiles_min_max(c):
    n = [hi - lo + 1 for lo, hi in block_tiles(c)]
    return min(n), max(n)


def visible(Lq, Lk, q_pos0, left, right):
    """bool [Lq, Lk]"""
    pos = (q_pos0 + torch.arange(Lq)).view(Lq, 1)
    j = torch.arange(Lk).view(1, Lk)
    m = torch.ones(Lq, Lk, dtype=torch.bool)
    if left >= 0:
        m &= j >= pos - left
    if right >= 0:
        m &= j <= pos + right
    return m


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16)


def edge_targets(c):
    """j(i) of `edge_probe`: by i % 4 the row's first visible key, its last visible key, the first hidden key on the left, the first hidden
    key on the right — cut to [0, Lk - 1] (a row without a visible key aims at the key nearest to its position)"""
    t = []
    for i in range(c.Lq):
        lo, hi = key_range(i, i, c.Lk, c.q_pos0, c.left, c.right)
        if lo > hi:
            j = c.q_pos0 + i
        else:
            j = (lo, hi, lo - 1, hi + 1)[i % 4]
        t.append(min(max(j, 0), c.Lk - 1))
    return torch.tensor(t, dtype=torch.long)


def make_band_case(c):
    """seeded operands on the CPU in the form of attn_cases.make_case: {"segs": [{"q", "k", "v", "w": 1.0}], "base", "scale_log2"}.
      random      q, k, v ~ N(0, 1)
      edge_probe  q_i = 0.5 r_i + g k_j(i), j(i) = edge_targets: an off-by-one at either edge of the window moves real weight
      ramp        (pre-scaled q) feature 0 of q is 2, the others 0, feature 0 of k is j % 64: the score of key j in the log2 domain is
                  2 (j % 64), bf16-exact, the same for every query: under a causal window the hidden keys of a row's own tile lie up to 126
                  above its visible ones
      ramp4       the same with 4 (j % 64): up to 252 above (RAMP_STEP)"""
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.split("_small")[0].encode()))
    scale_log2 = 1.0 if c.prescaled else float(torch.tensor(SCALE, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    H, Lq, Lk = c.H, c.Lq, c.Lk
    r = torch.randn(Lq, H, D, generator=g)
    k = _bf16(torch.randn(Lk, H, D, generator=g)).float()
    v = _bf16(torch.randn(Lk, H, D, generator=g))
    q = r
    if c.pattern == "edge_probe":
        gain = (math.log(Lk) + 0.3) / (SCALE * D)
        q = 0.5 * r + gain * k[edge_targets(c)]
    if c.prescaled:
        q = q * (SCALE * LOG2E)
    q = _bf16(q).float()
    if c.pattern in RAMP_STEP:
        assert c.prescaled
        q = torch.zeros(Lq, H, D)
        q[:, :, 0] = float(RAMP_STEP[c.pattern])
        k[:, :, 0] = (torch.arange(Lk) % KT).view(Lk, 1).float()
    assert torch.equal(_bf16(q).float(), q) and torch.equal(_bf16(k).float(), k)
    base = _bf16(torch.randn(Lq, H * D, generator=g)) if c.acc else None
    return {"segs": [{"q": _bf16(q), "k": _bf16(k), "v": v, "w": 1.0}], "base": base, "scale_log2": scale_log2}


# ---- reference ---------------------------------------------------------------------------------------------------------------------------
def reference_band(c, ops, device="cpu"):
    """fp64 exact softmax over the visible keys, head by head: {"ref", "A" = sum_j a_ij |v_jd|, "Q" = sum_j (a_ij v_jd)^2 (fp64 [Lq, H, 128]; a_ij =
    0 for a hidden key, so all three are 0 on a row that sees none), "base" (the old O of an accumulate call, zeros otherwise)}"""
    sg = ops["segs"][0]
    q, k, v = sg["q"], sg["k"], sg["v"]
    vis = visible(c.Lq, c.Lk, c.q_pos0, c.left, c.right).to(device)
    out = {n: torch.empty(c.Lq, c.H, D, dtype=torch.float64, device=device) for n in ("ref", "A", "Q")}
    some = vis.any(dim=1, keepdim=True)
    for h in range(c.H):
        kh, vh = k[:, h].to(device, torch.float64), v[:, h].to(device, torch.float64)
        x = (q[:, h].to(device, torch.float64) @ kh.T) * ops["scale_log2"]
        x = torch.where(vis, x, torch.full_like(x, -float("inf")))
        m = torch.where(some, x.max(dim=1, keepdim=True).values, torch.zeros_like(x[:, :1]))
        a = torch.exp2(x - m)                                   # exactly 0 on a hidden key
        l = a.sum(dim=1, keepdim=True)
        a = a / torch.where(some, l, torch.ones_like(l))
        out["ref"][:, h] = a @ vh
        out["A"][:, h] = a @ vh.abs()
        out["Q"][:, h] = (a * a) @ (vh * vh)
    b = ops["base"]
    out["base"] = b.to(device, torch.float64).view(c.Lq, c.H, D) if b is not None else torch.zeros((), dtype=torch.float64, device=device)
    return out


def empty_rows(c):
    """bool [Lq]: rows that see no key"""
    return ~visible(c.Lq, c.Lk, c.q_pos0, c.left, c.right).any(dim=1)


# ---- host emulation of the kernel's arithmetic -----------------------------------------------------------------------------------------------
FAULTS = ("max_over_hidden", "left_off_by_one", "right_off_by_one", "top_left_aligned", "edge_tile_dropped", "empty_row_copies_v",
          "interior_masked_as_edge")
SAME_FUNCTION = ("interior_masked_as_edge",)        # must NOT be flagged: every tile through the masked body computes the same function


def fault_applies(c, fault):
    """does the corruption change what the kernel computes on this row of the table?
      * the base over hidden keys shows where a hidden key of a tile the row's workgroup walks lies MORE than 126 above every visible key
        of some row (RAMP_STEP): worked out from the ramp's integer scores — the `ramp4` rows, not the `ramp` rows (126 exactly);
      * an edge one key off needs a bounded edge and a row whose extra key exists (0 <= j < Lk);
      * the top-left alignment needs q_pos0 != 0;
      * a dropped edge tile takes visible keys from a row of every workgroup that sees any (the tile range is tight: its last key is
        visible to one of its rows);
      * a row without a visible key that copies a V row needs such a row;
      * the masked body on an interior tile is the same function."""
    pos = [c.q_pos0 + i for i in range(c.Lq)]
    rows = [key_range(i, i, c.Lk, c.q_pos0, c.left, c.right) for i in range(c.Lq)]
    return {"max_over_hidden": ramp_gap(c) > 126,
            "left_off_by_one": c.left >= 0 and any(0 <= p - c.left - 1 < c.Lk for p in pos),
            "right_off_by_one": c.right >= 0 and any(0 <= p + c.right + 1 < c.Lk for p in pos),
            "top_left_aligned": c.q_pos0 != 0,
            "edge_tile_dropped": any(lo <= hi for lo, hi in block_tiles(c)),
            "empty_row_copies_v": any(lo > hi for lo, hi in rows),
            "interior_masked_as_edge": True}[fault]


def ramp_gap(c):
    """the most a key of the tiles a row's workgroup walks lies above the row's best visible key, over the rows that see a key (log2 domain;
    0 for the patterns that are no ramp: their scores spread by far less than 126)"""
    if c.pattern not in RAMP_STEP:
        return 0
    score = RAMP_STEP[c.pattern] * (torch.arange(c.Lk) % KT)
    gap = 0
    tiles = block_tiles(c)
    for i in range(c.Lq):
        lo, hi = key_range(i, i, c.Lk, c.q_pos0, c.left, c.right)
        t_lo, t_hi = tiles[i // QB]
        if lo <= hi:
            gap = max(gap, int(score[t_lo * KT:(t_hi + 1) * KT].max() - score[lo:hi + 1].max()))
    return gap


def emulate_band(c, ops, fault=None):
    """what a correct attn_band_kernel stores, on the CPU in fp32 (attn_cases.emulate_one's arithmetic over the visible keys): scores from the
    bf16 operands, the mask BEFORE the row maximum, exp2 against the base (results under 2^-126 flushed), P of a hidden key 0, ONE bf16
    rounding of P, fp32 row sum and accumulation, one bf16 rounding of O / l (+ base); a row that sees no key stores 0 / keeps its old O.
    -> fp64 [Lq, H, 128]"""
    sg = ops["segs"][0]
    qf, kf, vf = sg["q"].float(), sg["k"].float(), sg["v"].float()
    Lq, Lk, H = c.Lq, c.Lk, c.H
    q_pos0, left, right = c.q_pos0, c.left, c.right
    if fault == "top_left_aligned":
        q_pos0 = 0
    if fault == "left_off_by_one" and left >= 0:
        left += 1
    if fault == "right_off_by_one" and right >= 0:
        right += 1
    vis = visible(Lq, Lk, q_pos0, left, right)
    walked = torch.zeros(Lq, Lk, dtype=torch.bool)              # the keys of the tiles the row's workgroup walks
    for b, (lo, hi) in enumerate(block_tiles(c._replace(q_pos0=q_pos0, left=left, right=right))):
        if lo <= hi:
            if fault == "edge_tile_dropped":
                vis[b * QB:(b + 1) * QB, hi * KT:] = False
                hi -= 1
            walked[b * QB:(b + 1) * QB, lo * KT:(hi + 1) * KT] = True
    some = vis.any(dim=1, keepdim=True)
    c2 = torch.tensor(ops["scale_log2"], dtype=torch.float32)
    out = torch.empty(Lq, H, D, dtype=torch.float32)
    for h in range(H):
        x = (qf[:, h] @ kf[:, h].T) * c2
        over = walked if fault == "max_over_hidden" else vis
        m = torch.where(over, x, torch.full_like(x, -float("inf"))).max(dim=1, keepdim=True).values
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        e = x - m
        p = torch.where(e < -126.0, torch.zeros_like(e), torch.exp2(e))
        p = torch.where(vis, p, torch.zeros_like(p))
        l = p.sum(dim=1, keepdim=True)
        o = ac._round_bf16(p) @ vf[:, h]
        out[:, h] = torch.where(l > 0, o / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(o))
        if fault == "empty_row_copies_v":
            j = (q_pos0 + torch.arange(Lq)).clamp(0, Lk - 1)
            out[:, h] = torch.where(some, out[:, h], vf[j, h])
    if ops["base"] is not None:
        out = out + ops["base"].float().view(Lq, H, D)
    return ac._round_bf16(out).double()


# ---- the call on the device ------------------------------------------------------------------------------------------------------------------
def run_band_case(c, ops, dev_ops=None, window=True):
    """one call into fresh operands (or `dev_ops`) -> the device operands; window=False: the global call on the same operands"""
    from yume_amd import ops as yops
    d = dev_ops or device_operands(as_case(c), ops)
    kw = dict(window=(c.left, c.right), q_pos0=c.q_pos0) if window else {}
    yops.attn_fwd(d["q"], d["ks"][0], d["vts"][0], d["o"], c.Lq, c.Lk, c.H, scale=None if c.prescaled else SCALE, accumulate=c.acc, variant=0,
                  q_prescaled=c.prescaled, kv_padded=c.padded, **kw)
    return d


def band_log(line):
    """`[attn_fwd_band] band q_pos0=.. left=.. right=.. tiles_min=.. tiles_max=.. Lq=.. ...` -> (route, {key: int})"""
    f = line.split()
    return f[1], {k: int(v) for k, v in (t.split("=", 1) for t in f[2:] if "=" in t)}


def main(argv):
    if argv != ["--routes"]:
        sys.exit(__doc__)
    from yume_amd import ops as yops
    yops.ensure_counters(torch.device("cuda", torch.cuda.current_device()))
    for c in CASES + NORMALISED:
        ops = make_band_case(c)
        d = device_operands(as_case(c), ops)
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {c.name}\n")
        sys.stderr.flush()
        run_band_case(c, ops, d)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main(sys.argv[1:])
