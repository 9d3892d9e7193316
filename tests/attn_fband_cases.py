"""The case tables of the frame-window / frame-causal attention entry point (yume_attn_fwd_fband, yume_amd/csrc/attn_fband.hpp), the Python
mirror of its visibility rule (yume_amd/csrc/attn_fband_plan.hpp: change both or neither), the fp64 masked-softmax reference, and a host
emulation of the kernel's arithmetic with injected faults (no test functions in here). The per-element bound is tests/attn_cases.py's
`bound()` unchanged (KAPPA = 4.5 from r11, not re-fitted), the operand forms and guards are its `device_operands`; H = 2, D = 128 throughout.

    spans = [(rows_g, nblk_g)]: span g starts at row0_g = sum_{g' < g} rows_g' nblk_g' and holds nblk_g blocks of rows_g rows; N rows, NB blocks
    b(p) = the block of position p;  pos(i) = q_pos0 + i
    visible(i, j)  <=>  0 <= j < Lk  and  (back < 0 or b(j) >= b(pos(i)) - back)  and  (ahead < 0 or b(j) <= b(pos(i)) + ahead)
    O[i] = exact softmax over the visible keys;  O[i] = 0 where row i sees none (an accumulate call leaves the old O[i] as it is)

tests/test_attn_fband_routes_gpu.py runs one call per row of CASES, NORMALISED and BAND_EQUIV; tests/test_attn_fband_cases_cpu.py proves the
mirror against the compiled header and a brute-force walk, and the bound's reach over the faults on the host.

    python tests/attn_fband_cases.py --routes      one call per CASES and NORMALISED row, `CASE <name>` on stderr before each
"""
import math
import sys
import zlib
from collections import namedtuple

import torch

import attn_cases as ac
from attn_cases import D, GUARD_COLS, GUARD_ROWS, KAPPA, KT, LOG2E, PAD_VALUE, SCALE, SENTINEL, bound, device_operands, written  # noqa: F401

QB = 128                     # query rows per workgroup of attn_fband_kernel (attn_fband_plan.hpp)
QW = 32                      # query rows per wave
MAX_SPANS = 16
RAMP_STEP = 4                # `ramp4`: the score of key j in the log2 domain is 4 (j % 64) for every query (tests/attn_band_cases.py RAMP_STEP: the
#                              row maximum taken before the mask shows only where a hidden key lies MORE than 126 above a row's visible ones)

FCase = namedtuple("FCase", "name spans Lq Lk q_pos0 back ahead H pattern form prescaled padded acc",
                   defaults=(2, "edge_probe", "engine_self", False, False, False))

ONE_SPAN = ((35, 9),)                                       # 315 rows: block edges on no tile, wave or workgroup boundary
PYRAMID = ((6, 1), (6, 3), (24, 4), (96, 2), (96, 3))       # 600 rows, 13 blocks: FramePack's coarse-to-fine shape


def _tag(back, ahead):
    return f"b{back}_a{ahead}".replace("-1", "inf")


def _table():
    rows = [FCase("tiny_blocks_b2_a1", ((5, 60),), 300, 300, 0, 2, 1)]
    for n, (b, a) in enumerate(((1, 1), (0, 0), (-1, 0), (0, -1))):
        rows.append(FCase(f"one_span_{_tag(b, a)}", ONE_SPAN, 315, 315, 0, b, a, form=("engine_self", "engine_cross")[n % 2],
                          pattern="random" if n == 1 else "edge_probe"))
    rows.append(FCase("big_blocks_b0_a0", ((300, 4),), 1200, 1200, 0, 0, 0))
    rows.append(FCase("big_blocks_binf_a0", ((300, 4),), 1200, 1200, 0, -1, 0, pattern="random"))
    rows.append(FCase("aligned_64x6_b1_a0", ((64, 6),), 384, 384, 0, 1, 0))
    rows.append(FCase("aligned_128x3_b1_a0", ((128, 3),), 384, 384, 0, 1, 0, form="engine_cross"))
    for n, (b, a) in enumerate(((1, 1), (2, 0), (-1, 0), (0, -1))):
        rows.append(FCase(f"pyramid_{_tag(b, a)}", PYRAMID, 600, 600, 0, b, a, form=("engine_self", "engine_cross")[n % 2]))
    # the engine's trimmed last block: the rows [s, L) of the sequence with q_pos0 = s; and Lk < N with the rest hidden (the rows of the
    # last block then see no key under (0, 0), the last workgroup none at all)
    rows.append(FCase("trimmed_s312", PYRAMID, 288, 600, 312, 1, 1))
    rows.append(FCase("trimmed_s401", PYRAMID, 199, 600, 401, 1, 1))
    rows.append(FCase("trimmed_lk500_b0_a0", PYRAMID, 288, 500, 312, 0, 0, form="engine_cross"))
    rows.append(FCase("trimmed_lk500_acc", PYRAMID, 288, 500, 312, 0, 0, form="engine_cross", acc=True))
    rows.append(FCase("l1500_b1_a1", ((125, 12),), 1500, 1500, 0, 1, 1, pattern="random"))
    # the ramp: hidden keys of a walked tile far above a row's visible ones
    rows.append(FCase("ramp4_one_span_binf_a0", ONE_SPAN, 315, 315, 0, -1, 0, pattern="ramp4", prescaled=True))
    rows.append(FCase("ramp4_one_span_b0_a0", ONE_SPAN, 315, 315, 0, 0, 0, pattern="ramp4", prescaled=True))
    rows.append(FCase("ramp4_pyramid_binf_a0", PYRAMID, 600, 600, 0, -1, 0, pattern="ramp4", prescaled=True))
    rows.append(FCase("ramp4_pyramid_b1_a1", PYRAMID, 600, 600, 0, 1, 1, pattern="ramp4", prescaled=True))
    # the modes, on the pyramid
    rows.append(FCase("pyramid_acc_b1_a1", PYRAMID, 600, 600, 0, 1, 1, acc=True))
    rows.append(FCase("pyramid_prescaled_b2_a0", PYRAMID, 600, 600, 0, 2, 0, prescaled=True))
    rows.append(FCase("pyramid_kv_padded_b1_a1", PYRAMID, 600, 600, 0, 1, 1, prescaled=True, padded=True))      # PAD_VALUE junk behind Lk
    return rows


CASES = _table()
# calls that hide no (row, key) pair: the ordinary `[attn_fwd] ...` call, bit for bit
NORMALISED = [FCase("norm_one_span_nb", ONE_SPAN, 315, 315, 0, 8, 8, pattern="random"),
              FCase("norm_one_span_inf", ONE_SPAN, 315, 315, 0, -1, -1, pattern="random", form="tight"),
              FCase("norm_pyramid_nb", PYRAMID, 600, 600, 0, 12, 40, pattern="random", prescaled=True, padded=True),
              FCase("norm_pyramid_inf", PYRAMID, 600, 600, 0, -1, -1, pattern="random")]
# one span of one-row blocks: yume_attn_fwd_band(left = back, right = ahead), bit for bit
BAND_EQUIV = [FCase("band_l17_r5", ((1, 300),), 300, 300, 0, 17, 5, pattern="random"),
              FCase("band_causal", ((1, 300),), 300, 300, 0, -1, 0, form="engine_cross")]
# what the entry point must refuse: (name, keyword overrides of a valid call, error code, a word of the message)
EINVAL, EUNSUP = -1, -3
REFUSALS = [("nspan_0", dict(spans=()), EINVAL, "nspan"), ("nspan_17", dict(spans=((1, 20),) * 17), EINVAL, "nspan"),
            ("rows_0", dict(spans=((0, 9), (35, 9))), EINVAL, "span_rows"), ("blocks_0", dict(spans=((35, 9), (35, 0))), EINVAL, "span_blocks"),
            ("n_2_31", dict(spans=((35, 9), (2 ** 20, 2 ** 11))), EINVAL, "2^31"), ("back_minus_2", dict(back=-2), EINVAL, "back"),
            ("ahead_minus_3", dict(ahead=-3), EINVAL, "ahead"), ("q_pos0_negative", dict(q_pos0=-1), EINVAL, "q_pos0"),
            ("rows_behind_n", dict(q_pos0=16), EINVAL, "q_pos0"), ("lk_over_n", dict(Lk=316, ldvt=320), EINVAL, "Lk"),
            ("variant_7", dict(variant=7), EUNSUP, "variant 7"), ("variant_11_flags", dict(variant=11 | 0x100 | 0x200), EUNSUP, "variant 11"),
            ("null_q", dict(Q=None), EINVAL, "NULL"), ("null_k", dict(K=None), EINVAL, "NULL"), ("null_vt", dict(Vt=None), EINVAL, "NULL"),
            ("null_o", dict(O=None), EINVAL, "NULL"), ("null_spans", dict(null_spans=True), EINVAL, "NULL"),
            ("misaligned_q", dict(Q=4096 + 8), EINVAL, "alignment"), ("misaligned_o", dict(O=4096 + 4), EINVAL, "alignment"),
            ("ldvt_short", dict(ldvt=64), EINVAL, "ldvt"), ("empty", dict(Lq=0), EINVAL, "empty")]


def as_case(c):
    """the tests/attn_cases.py row whose operand-form helpers (device_operands, written, call_rows) serve this one"""
    return ac.Case(c.name, "fwd", 0, c.Lq, c.Lk, c.H, c.pattern, c.form, c.prescaled, c.padded, 1.0, c.acc, "fband", None, None, False)


# ---- the rule: Python mirror of yume_amd/csrc/attn_fband_plan.hpp ---------------------------------------------------------------------------
def total_rows(spans):
    return sum(r * n for r, n in spans)


def total_blocks(spans):
    return sum(n for _, n in spans)


def block_of(pos, spans):
    """b(pos), 0 <= pos < N: the last span that starts at or below pos, one division inside it"""
    row0 = blk0 = 0
    s_row0, s_blk0, s_rows = 0, 0, spans[0][0]
    for rows, nblk in spans:
        if pos >= row0:
            s_row0, s_blk0, s_rows = row0, blk0, rows
        row0 += rows * nblk
        blk0 += nblk
    return s_blk0 + (pos - s_row0) // s_rows


def block_start(b, spans):
    """(start(b), end(b)), 0 <= b < NB"""
    row0 = blk0 = 0
    s_row0, s_blk0, s_rows = 0, 0, spans[0][0]
    for rows, nblk in spans:
        if b >= blk0:
            s_row0, s_blk0, s_rows = row0, blk0, rows
        row0 += rows * nblk
        blk0 += nblk
    start = s_row0 + (b - s_blk0) * s_rows
    return start, start + s_rows


def key_range(q_first, q_last, Lk, spans, q_pos0, back, ahead):
    """(lo, hi) inclusive: klo of the first row, khi of the last — the keys some row of q_first ... q_last sees; lo > hi: none"""
    nb = total_blocks(spans)
    b_first, b_last = block_of(q_pos0 + q_first, spans), block_of(q_pos0 + q_last, spans)
    b_lo = 0 if back < 0 else max(b_first - back, 0)
    b_hi = nb - 1 if ahead < 0 else min(b_last + ahead, nb - 1)
    return block_start(b_lo, spans)[0], min(block_start(b_hi, spans)[1], Lk) - 1


def tile_range(q_first, q_last, Lk, spans, q_pos0, back, ahead):
    lo, hi = key_range(q_first, q_last, Lk, spans, q_pos0, back, ahead)
    return (0, -1) if lo > hi else (lo // KT, hi // KT)


def tile_is_interior(t, q_first, q_last, Lk, spans, q_pos0, back, ahead):
    k0, k1 = t * KT, t * KT + KT - 1
    return (k1 < Lk and k0 >= key_range(q_last, q_last, Lk, spans, q_pos0, back, ahead)[0]
            and k1 <= key_range(q_first, q_first, Lk, spans, q_pos0, back, ahead)[1])


def hides_nothing(Lq, Lk, spans, q_pos0, back, ahead):
    return key_range(Lq - 1, Lq - 1, Lk, spans, q_pos0, back, ahead)[0] == 0 and key_range(0, 0, Lk, spans, q_pos0, back, ahead)[1] == Lk - 1


def rule(c):
    """the arguments of the mirror functions behind (rows, Lk)"""
    return tuple(c.spans), c.q_pos0, c.back, c.ahead


def block_index(spans):
    """long [N]: b(p) of every position"""
    return torch.cat([torch.arange(n).repeat_interleave(r) + b0 for (r, n), b0 in
                      zip(spans, [sum(n for _, n in spans[:g]) for g in range(len(spans))])])


def visible(Lq, Lk, spans, q_pos0, back, ahead, blk=None):
    """bool [Lq, Lk]; blk: another block index per position (the faults)"""
    blk = block_index(spans) if blk is None else blk
    bq = blk[q_pos0:q_pos0 + Lq].view(Lq, 1)
    bj = blk[:Lk].view(1, Lk)
    m = torch.ones(Lq, Lk, dtype=torch.bool)
    if back >= 0:
        m &= bj >= bq - back
    if ahead >= 0:
        m &= bj <= bq + ahead
    return m


def block_tiles(c):
    """[(t_lo, t_hi)] of the 128-row workgroups of the call"""
    return [tile_range(q, min(q + QB, c.Lq) - 1, c.Lk, *rule(c)) for q in range(0, c.Lq, QB)]


def tiles_min_max(c):
    n = [hi - lo + 1 for lo, hi in block_tiles(c)]
    return min(n), max(n)


def empty_rows(c):
    """bool [Lq]: rows that see no key"""
    return ~visible(c.Lq, c.Lk, *rule(c)).any(dim=1)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16)


def edge_targets(c):
    """j(i) of `edge_probe`: by i % 4 the row's first visible key, its last visible key, the first hidden key before, the first hidden key
    behind — cut to [0, Lk - 1] (a row without a visible key aims at the key nearest to its position)"""
    t = []
    for i in range(c.Lq):
        lo, hi = key_range(i, i, c.Lk, *rule(c))
        j = c.q_pos0 + i if lo > hi else (lo, hi, lo - 1, hi + 1)[i % 4]
        t.append(min(max(j, 0), c.Lk - 1))
    return torch.tensor(t, dtype=torch.long)


def make_fband_case(c):
    """seeded operands on the CPU in the form of attn_cases.make_case: {"segs": [{"q", "k", "v", "w": 1.0}], "base", "scale_log2"}.
      random      q, k, v ~ N(0, 1)
      edge_probe  q_i = 0.5 r_i + g k_j(i), j(i) = edge_targets: a block edge one key off moves real weight
      ramp4       (pre-scaled q) feature 0 of q is 4, the others 0, feature 0 of k is j % 64: the score of key j in the log2 domain is
                  4 (j % 64), bf16-exact, the same for every query"""
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.encode()))
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
    if c.pattern == "ramp4":
        assert c.prescaled
        q = torch.zeros(Lq, H, D)
        q[:, :, 0] = float(RAMP_STEP)
        k[:, :, 0] = (torch.arange(Lk) % KT).view(Lk, 1).float()
    assert torch.equal(_bf16(q).float(), q) and torch.equal(_bf16(k).float(), k)
    base = _bf16(torch.randn(Lq, H * D, generator=g)) if c.acc else None
    return {"segs": [{"q": _bf16(q), "k": _bf16(k), "v": v, "w": 1.0}], "base": base, "scale_log2": scale_log2}


# ---- reference ---------------------------------------------------------------------------------------------------------------------------
def reference_masked(vis, ops, H, device="cpu"):
    """fp64 exact softmax over the visible keys (vis bool [Lq, Lk]), head by head: {"ref", "A" = sum_j a_ij |v_jd|, "Q" = sum_j (a_ij v_jd)^2
    (fp64 [Lq, H, 128]; a_ij = 0 for a hidden key, so all three are 0 on a row that sees none), "base" (the old O of an accumulate call, zeros
    otherwise)}"""
    sg = ops["segs"][0]
    q, k, v = sg["q"], sg["k"], sg["v"]
    Lq = vis.shape[0]
    vis = vis.to(device)
    out = {n: torch.empty(Lq, H, D, dtype=torch.float64, device=device) for n in ("ref", "A", "Q")}
    some = vis.any(dim=1, keepdim=True)
    for h in range(H):
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
    out["base"] = b.to(device, torch.float64).view(Lq, H, D) if b is not None else torch.zeros((), dtype=torch.float64, device=device)
    return out


def reference_fband(c, ops, device="cpu"):
    return reference_masked(visible(c.Lq, c.Lk, *rule(c)), ops, c.H, device)


# ---- host emulation of the kernel's arithmetic -----------------------------------------------------------------------------------------------
# the faults, and the rows of CASES on which the bound flags each (worked out by tests/test_attn_fband_cases_cpu.py, which holds this record:
# every row named here must be flagged). What each needs in order to show:
#   no_span_offset      b(p) = blk0_g + p / rows_g, the span's first row forgotten: a partition of more than one span
#   first_span_rows     rows_0 used for every span: spans of different rows
#   back_ahead_swapped  back != ahead
#   end_off_by_one      end(b) one row short: a row aimed at its last visible key (edge_probe) — every row of the table has such rows
#   q_pos0_ignored      q_pos0 != 0: the trimmed rows
#   interior_first_klo  the unmasked body on the tiles inside [klo(first row of the wave), khi(first row)] instead of klo(last row): a wave
#                       that straddles a block edge with a whole tile between the two rows' klo. (The emulation takes the interior test as
#                       the only guard. The kernel has a second one — a wave takes the unmasked body only once all its rows have a base, and
#                       a row whose klo lies behind a tile's first key has none before that tile — so there this mistake alone stays hidden;
#                       the table still has to be able to see it.)
#   max_over_hidden     the row maximum over every key of the walked tiles: a hidden key MORE than 126 above a visible one that carries
#                       weight, so that exp2 flushes it — the ramp rows: on the pyramid the first block is 6 keys of a 64-key tile (its best
#                       visible key 232 below the tile's top), on one_span 35 keys (116 below, the row's lower keys more than 126)
FAULTS = ("no_span_offset", "first_span_rows", "back_ahead_swapped", "end_off_by_one", "q_pos0_ignored", "interior_first_klo", "max_over_hidden")
FAULT_ROWS = {
    "no_span_offset": ("pyramid_b1_a1", "pyramid_b2_a0", "pyramid_binf_a0", "pyramid_b0_ainf", "trimmed_s312", "trimmed_s401",
                       "trimmed_lk500_b0_a0", "trimmed_lk500_acc", "ramp4_pyramid_binf_a0", "ramp4_pyramid_b1_a1", "pyramid_acc_b1_a1",
                       "pyramid_prescaled_b2_a0", "pyramid_kv_padded_b1_a1"),
    "first_span_rows": ("pyramid_b1_a1", "pyramid_b2_a0", "pyramid_binf_a0", "pyramid_b0_ainf", "trimmed_s312", "trimmed_s401",
                        "trimmed_lk500_b0_a0", "trimmed_lk500_acc", "ramp4_pyramid_binf_a0", "ramp4_pyramid_b1_a1", "pyramid_acc_b1_a1",
                        "pyramid_prescaled_b2_a0", "pyramid_kv_padded_b1_a1"),
    "back_ahead_swapped": ("tiny_blocks_b2_a1", "one_span_binf_a0", "one_span_b0_ainf", "big_blocks_binf_a0", "aligned_64x6_b1_a0",
                           "aligned_128x3_b1_a0", "pyramid_b2_a0", "pyramid_binf_a0", "pyramid_b0_ainf", "ramp4_one_span_binf_a0",
                           "ramp4_pyramid_binf_a0", "pyramid_prescaled_b2_a0"),
    "end_off_by_one": tuple(c.name for c in CASES),
    "q_pos0_ignored": ("trimmed_s312", "trimmed_s401", "trimmed_lk500_b0_a0", "trimmed_lk500_acc"),
    "interior_first_klo": ("one_span_b1_a1", "one_span_b0_ainf", "big_blocks_b0_a0", "pyramid_b1_a1", "pyramid_b2_a0", "pyramid_b0_ainf",
                           "trimmed_s401", "l1500_b1_a1", "ramp4_pyramid_b1_a1", "pyramid_acc_b1_a1", "pyramid_prescaled_b2_a0",
                           "pyramid_kv_padded_b1_a1"),
    "max_over_hidden": ("ramp4_one_span_binf_a0", "ramp4_one_span_b0_a0", "ramp4_pyramid_binf_a0", "ramp4_pyramid_b1_a1"),
}


def ramp_gap(c):
    """the most a key of the tiles a row's workgroup walks lies above the row's best visible key, over the rows that see a key (log2 domain;
    0 for the patterns that are no ramp: their scores spread by far less than 126)"""
    if c.pattern != "ramp4":
        return 0
    score = RAMP_STEP * (torch.arange(c.Lk) % KT)
    gap = 0
    tiles = block_tiles(c)
    for i in range(c.Lq):
        lo, hi = key_range(i, i, c.Lk, *rule(c))
        t_lo, t_hi = tiles[i // QB]
        if lo <= hi:
            gap = max(gap, int(score[t_lo * KT:(t_hi + 1) * KT].max() - score[lo:hi + 1].max()))
    return gap


def _faulty_visible(c, fault):
    """what a kernel with the fault takes for visible: bool [Lq, Lk]"""
    spans, q_pos0, back, ahead = rule(c)
    N, nb = total_rows(spans), total_blocks(spans)
    blk = None
    if fault == "no_span_offset":
        pos = torch.arange(N)
        true = block_index(spans)
        blk0 = torch.cat([torch.full((r * n,), sum(m for _, m in spans[:g])) for g, (r, n) in enumerate(spans)])
        rows = torch.cat([torch.full((r * n,), r) for r, n in spans])
        blk = torch.minimum(blk0 + pos // rows, torch.tensor(nb - 1))
        assert blk.shape == true.shape
    if fault == "first_span_rows":
        blk = torch.minimum(torch.arange(N) // spans[0][0], torch.tensor(nb - 1))
    if fault == "back_ahead_swapped":
        back, ahead = ahead, back
    if fault == "q_pos0_ignored":
        q_pos0 = 0
    vis = visible(c.Lq, c.Lk, spans, q_pos0, back, ahead, blk)
    if fault == "end_off_by_one":
        for i in range(c.Lq):
            lo, hi = key_range(i, i, c.Lk, *rule(c))
            if lo <= hi:
                vis[i, hi] = False
    if fault == "interior_first_klo":
        for w0 in range(0, c.Lq, QW):
            w1 = min(w0 + QW, c.Lq) - 1
            t_lo, t_hi = tile_range(w0, w1, c.Lk, *rule(c))
            lo, hi = key_range(w0, w0, c.Lk, *rule(c))
            for t in range(t_lo, t_hi + 1):
                if t * KT >= lo and t * KT + KT - 1 <= hi:
                    vis[w0:w1 + 1, t * KT:(t + 1) * KT] = True
    return vis


def emulate_fband(c, ops, fault=None):
    """what a correct attn_fband_kernel stores, on the CPU in fp32 (attn_cases.emulate_one's arithmetic over the visible keys): scores from the
    bf16 operands, the mask BEFORE the row maximum, exp2 against the base (results under 2^-126 flushed), P of a hidden key 0, ONE bf16
    rounding of P, fp32 row sum and accumulation, one bf16 rounding of O / l (+ base); a row that sees no key stores 0 / keeps its old O.
    -> fp64 [Lq, H, 128]"""
    sg = ops["segs"][0]
    qf, kf, vf = sg["q"].float(), sg["k"].float(), sg["v"].float()
    Lq, Lk, H = c.Lq, c.Lk, c.H
    vis = visible(Lq, Lk, *rule(c)) if fault in (None, "max_over_hidden") else _faulty_visible(c, fault)
    walked = torch.zeros(Lq, Lk, dtype=torch.bool)              # the keys of the tiles the row's workgroup walks
    for b, (lo, hi) in enumerate(block_tiles(c)):
        if lo <= hi:
            walked[b * QB:(b + 1) * QB, lo * KT:(hi + 1) * KT] = True
    c2 = torch.tensor(ops["scale_log2"], dtype=torch.float32)
    out = torch.empty(Lq, H, D, dtype=torch.float32)
    for h in range(H):
        x = (qf[:, h] @ kf[:, h].T) * c2
        over = (walked | vis) if fault == "max_over_hidden" else vis
        m = torch.where(over, x, torch.full_like(x, -float("inf"))).max(dim=1, keepdim=True).values
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        e = x - m
        p = torch.where(e < -126.0, torch.zeros_like(e), torch.exp2(e))
        p = torch.where(vis, p, torch.zeros_like(p))
        l = p.sum(dim=1, keepdim=True)
        o = ac._round_bf16(p) @ vf[:, h]
        out[:, h] = torch.where(l > 0, o / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(o))
    if ops["base"] is not None:
        out = out + ops["base"].float().view(Lq, H, D)
    return ac._round_bf16(out).double()


# ---- the call on the device ------------------------------------------------------------------------------------------------------------------
def run_fband_case(c, ops, dev_ops=None, mode="fband"):
    """one call into fresh operands (or `dev_ops`) -> the device operands. The rows of O the call owns are pre-filled with NaN (the old O
    under accumulate): what the kernel does not write shows. mode: "fband", "global" (the ordinary call on the same operands) or "band"
    (yume_attn_fwd_band with left = back, right = ahead)"""
    from yume_amd import ops as yops
    d = dev_ops or device_operands(as_case(c), ops)
    if not c.acc:
        d["o"].fill_(float("nan"))
    kw = {"fband": dict(frame_window=(c.back, c.ahead), spans=list(c.spans), q_pos0=c.q_pos0), "global": {},
          "band": dict(window=(c.back, c.ahead), q_pos0=c.q_pos0)}[mode]
    yops.attn_fwd(d["q"], d["ks"][0], d["vts"][0], d["o"], c.Lq, c.Lk, c.H, scale=None if c.prescaled else SCALE, accumulate=c.acc, variant=0,
                  q_prescaled=c.prescaled, kv_padded=c.padded, **kw)
    return d


def fband_log(line):
    """`[attn_fwd_fband] fband q_pos0=.. back=.. ahead=.. nspan=.. nblocks=.. tiles_min=.. tiles_max=.. Lq=.. ...` -> (route, {key: int})"""
    f = line.split()
    return f[1], {k: int(v) for k, v in (t.split("=", 1) for t in f[2:] if "=" in t)}


def main(argv):
    if argv != ["--routes"]:
        sys.exit(__doc__)
    from yume_amd import ops as yops
    yops.ensure_counters(torch.device("cuda", torch.cuda.current_device()))
    for c in CASES + NORMALISED:
        ops = make_fband_case(c)
        d = device_operands(as_case(c), ops)
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {c.name}\n")
        sys.stderr.flush()
        run_fband_case(c, ops, d)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main(sys.argv[1:])
