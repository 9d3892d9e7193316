"""The case tables of the frame-window attention with a sink (yume_attn_fwd_fsink, yume_amd/csrc/attn_fsink.hpp), the Python mirror of its rule
(yume_amd/csrc/attn_fsink_plan.hpp: change both or neither), the fp64 masked-softmax reference, and a host emulation of the kernel's
arithmetic with injected faults (no test functions in here). Built like tests/attn_fband_cases.py, whose helpers serve here too; the
per-element bound is tests/attn_cases.py's `bound()` unchanged (KAPPA = 4.5), the operand forms and guards its `device_operands`; H = 2, D = 128.

    the partition, pos(i), b(p), back, ahead: tests/attn_fband_cases.py;  0 <= sink <= NB;  send = min(start(sink), Lk), start(NB) = N
    visible(i, j)  <=>  0 <= j < Lk  and  (j < send  or  the frame window's visible(i, j))
    a row sees [0, send) U [klo(i), khi(i)]: one interval where klo(i) <= send, two with a hidden gap otherwise
    a run of rows walks the tiles [0, ceil(send / 64)) and [max(t_lo, ceil(send / 64)), t_hi], ascending, each once

tests/test_attn_fsink_routes_gpu.py runs one call per row of CASES, NORMALISED and FBAND_EQUIV; tests/test_attn_fsink_cases_cpu.py proves the
mirror against the compiled header and a brute-force walk, and the bound's reach over the faults on the host.

    python tests/attn_fsink_cases.py --routes      one call per CASES, NORMALISED and FBAND_EQUIV row, `CASE <name>` on stderr before each
"""
import math
import sys
import zlib
from collections import namedtuple
from functools import lru_cache

import torch

import attn_cases as ac
import attn_fband_cases as fb
from attn_cases import D, GUARD_COLS, GUARD_ROWS, KAPPA, KT, LOG2E, PAD_VALUE, SCALE, SENTINEL, bound, device_operands, written  # noqa: F401
from attn_fband_cases import (MAX_SPANS, ONE_SPAN, PYRAMID, QB, QW, RAMP_STEP, as_case, block_index, block_of, block_start, fband_log,  # noqa: F401
                              reference_masked, total_blocks, total_rows)

SCase = namedtuple("SCase", "name spans Lq Lk q_pos0 back ahead sink H pattern form prescaled padded acc",
                   defaults=(2, "edge_probe", "engine_self", False, False, False))
ONE_SPAN30 = ((30, 10),)     # the ramp's own partition: see _table


def _table():
    rows = [SCase("tiny_blocks_s3_b1_a1", ((5, 60),), 300, 300, 0, 1, 1, 3)]              # block 8: keys 0-14, hidden 15-34, 35-49 in tile 0
    rows.append(SCase("pyramid_s1_b1_a1", PYRAMID, 600, 600, 0, 1, 1, 1))                   # sink inside tile 0; the last workgroup jumps 0 -> 6
    rows.append(SCase("pyramid_s1_b0_a0", PYRAMID, 600, 600, 0, 0, 0, 1, form="engine_cross"))
    rows.append(SCase("pyramid_s8_b0_a0", PYRAMID, 600, 600, 0, 0, 0, 8))                   # send = 120 inside tile 1; block 8 adjoins it, block 9 not
    rows.append(SCase("one_span_s1_b0_a0", ONE_SPAN, 315, 315, 0, 0, 0, 1, form="engine_cross"))
    rows.append(SCase("aligned_64x6_s1_b0_a0", ((64, 6),), 384, 384, 0, 0, 0, 1))           # send on a tile edge: no straddling sink tile
    rows.append(SCase("aligned_128x3_s1_b0_a0", ((128, 3),), 384, 384, 0, 0, 0, 1))         # send on a workgroup edge
    rows.append(SCase("big_blocks_s1_b0_a0", ((300, 4),), 1200, 1200, 0, 0, 0, 1))          # four interior sink tiles, one straddling
    rows.append(SCase("l1500_s2_b1_a1", ((125, 12),), 1500, 1500, 0, 1, 1, 2, pattern="random"))
    # the engine's trimmed last block, and Lk < N
    rows.append(SCase("trimmed_s312_s2", PYRAMID, 288, 600, 312, 1, 1, 2))
    rows.append(SCase("trimmed_s401_s2", PYRAMID, 199, 600, 401, 1, 1, 2))
    rows.append(SCase("trimmed_lk500_s8", PYRAMID, 288, 500, 312, 0, 0, 8, form="engine_cross"))
    # the sink's last tile is the ragged last tile of the key axis (the register path as the next tile of the list), and no row has a band
    # part. (Lk = 100, where Lk CUTS the sink, is no call of the kernel: send = Lk hides nothing — NORMALISED's norm_lk100_s8. Lk = 125
    # leaves the keys 120 ... 124 behind the sink, hidden from every row.)
    rows.append(SCase("trimmed_lk125_s8", PYRAMID, 288, 125, 312, 0, 0, 8, form="engine_cross"))
    # the ramp: the hidden keys of the sink's own tile far above a row's visible ones. On ONE_SPAN the sink is 35 keys of tile 0 and a row
    # of block 0 has its best key 116 below the tile's top (r28's figure; only its lower keys lie beyond exp2's 126); 30-row blocks put
    # the best key 136 below, which is what sink_tile_gap asks for.
    rows.append(SCase("ramp4_pyramid_s1_b1_a1", PYRAMID, 600, 600, 0, 1, 1, 1, pattern="ramp4", prescaled=True))
    rows.append(SCase("ramp4_one_span_s1_b0_a0", ONE_SPAN, 315, 315, 0, 0, 0, 1, pattern="ramp4", prescaled=True))
    rows.append(SCase("ramp4_one_span30_s1_b0_a0", ONE_SPAN30, 300, 300, 0, 0, 0, 1, pattern="ramp4", prescaled=True))
    # the modes, on the pyramid
    rows.append(SCase("pyramid_acc_s2_b1_a1", PYRAMID, 600, 600, 0, 1, 1, 2, acc=True))
    rows.append(SCase("pyramid_prescaled_s2_b1_a1", PYRAMID, 600, 600, 0, 1, 1, 2, prescaled=True))
    rows.append(SCase("pyramid_kv_padded_s2_b1_a1", PYRAMID, 600, 600, 0, 1, 1, 2, prescaled=True, padded=True))      # PAD_VALUE junk behind Lk
    return rows


CASES = _table()
# a sink that shows nothing the window hides (or none): yume_attn_fwd_fband with the same arguments, bit for bit, with its log line
FBAND_EQUIV = [SCase("equiv_sink0", PYRAMID, 600, 600, 0, 1, 1, 0),
               SCase("equiv_binf_s3", PYRAMID, 600, 600, 0, -1, 2, 3, pattern="random"),
               SCase("equiv_first_rows_s1", PYRAMID, 48, 600, 0, 4, 0, 1, form="engine_cross")]          # every row already sees block 0
# a sink that is the whole key axis (sink = NB, or cut by Lk): the ordinary `[attn_fwd] ...` call, bit for bit
NORMALISED = [SCase("norm_one_span_nb", ONE_SPAN, 315, 315, 0, 0, 0, 9, pattern="random"),
              SCase("norm_lk100_s8", PYRAMID, 288, 100, 312, 0, 0, 8, form="engine_cross"),
              SCase("norm_pyramid_nb", PYRAMID, 600, 600, 0, 1, 1, 13, pattern="random", prescaled=True, padded=True)]
# what the entry point must refuse: (name, keyword overrides of a valid call that reaches the kernel, error code, a word of the message, the
# entry that answers). fband's list through the new entry point, then the sink's own. Variant 13 IS the new kernel, with or without the
# flag bits; what refuses it is the frame-band entry, which a call with sink = 0 is handed to with the same arguments.
EINVAL, EUNSUP = fb.EINVAL, fb.EUNSUP
REFUSALS = [r + ("attn_fwd_fsink",) for r in fb.REFUSALS if not r[0].startswith("variant")] + [
    ("sink_minus_1", dict(sink=-1), EINVAL, "sink", "attn_fwd_fsink"), ("sink_nb_plus_1", dict(sink=10), EINVAL, "sink", "attn_fwd_fsink"),
    ("variant_7", dict(variant=7), EUNSUP, "variant 7", "attn_fwd_fsink"), ("variant_12", dict(variant=12), EUNSUP, "variant 12", "attn_fwd_fsink"),
    ("variant_11_flags", dict(variant=11 | 0x100 | 0x200), EUNSUP, "variant 11", "attn_fwd_fsink"),
    ("variant_13_flags_sink0", dict(variant=13 | 0x100 | 0x200, sink=0), EUNSUP, "variant 13", "attn_fwd_fband")]


# ---- the rule: Python mirror of yume_amd/csrc/attn_fsink_plan.hpp ---------------------------------------------------------------------------
def rule(c):
    """the arguments of the mirror functions behind (rows, Lk)"""
    return tuple(c.spans), c.q_pos0, c.back, c.ahead, c.sink


def send(Lk, spans, sink):
    if sink <= 0:
        return 0
    s = total_rows(spans) if sink >= total_blocks(spans) else block_start(sink, spans)[0]
    return min(s, Lk)


def visible(Lq, Lk, spans, q_pos0, back, ahead, sink):
    """bool [Lq, Lk]"""
    m = fb.visible(Lq, Lk, spans, q_pos0, back, ahead)
    m[:, :send(Lk, spans, sink)] = True
    return m


def adds_nothing(Lq, Lk, spans, q_pos0, back, ahead, sink):
    se = send(Lk, spans, sink)
    return se == 0 or (fb.key_range(Lq - 1, Lq - 1, Lk, spans, q_pos0, back, ahead)[0] == 0
                       and fb.key_range(0, 0, Lk, spans, q_pos0, back, ahead)[1] >= se - 1)


def hides_nothing(Lq, Lk, spans, q_pos0, back, ahead, sink):
    se = send(Lk, spans, sink)
    return se >= Lk or (fb.key_range(0, 0, Lk, spans, q_pos0, back, ahead)[1] == Lk - 1
                        and fb.key_range(Lq - 1, Lq - 1, Lk, spans, q_pos0, back, ahead)[0] <= se)


def tile_list(q_first, q_last, Lk, spans, q_pos0, back, ahead, sink):
    """(n_sink, b_lo, b_hi): the tiles [0, n_sink) and [b_lo, b_hi]; without band tiles behind the sink's b_lo = n_sink, b_hi = n_sink - 1"""
    ns = (send(Lk, spans, sink) + KT - 1) // KT
    lo, hi = fb.tile_range(q_first, q_last, Lk, spans, q_pos0, back, ahead)
    return ns, max(lo, ns), max(hi, ns - 1)


def tiles_of(tl):
    ns, b_lo, b_hi = tl
    return list(range(ns)) + list(range(b_lo, b_hi + 1))


def next_tile(t, tl):
    return tl[1] if t + 1 == tl[0] else t + 1


def tile_is_interior(t, q_first, q_last, Lk, spans, q_pos0, back, ahead, sink):
    k1 = t * KT + KT - 1
    return k1 < Lk and (k1 < send(Lk, spans, sink) or fb.tile_is_interior(t, q_first, q_last, Lk, spans, q_pos0, back, ahead))


@lru_cache(maxsize=None)
def block_lists(c):
    """[(n_sink, b_lo, b_hi)] of the 128-row workgroups of the call"""
    return [tile_list(q, min(q + QB, c.Lq) - 1, c.Lk, *rule(c)) for q in range(0, c.Lq, QB)]


def tiles_min_max(c):
    n = [len(tiles_of(tl)) for tl in block_lists(c)]
    return min(n), max(n)


@lru_cache(maxsize=None)
def row_ranges(c):
    """[(klo, khi)] of the frame window, row by row"""
    return [fb.key_range(i, i, c.Lk, *rule(c)[:4]) for i in range(c.Lq)]


def empty_rows(c):
    return ~visible(c.Lq, c.Lk, *rule(c)).any(dim=1)


# ---- what the tables must contain ----------------------------------------------------------------------------------------------------------
def split_tile_rows(c):
    """rows for which ONE tile holds the sink's end, a hidden gap and the band's start"""
    se = send(c.Lk, c.spans, c.sink)
    return [i for i, (lo, hi) in enumerate(row_ranges(c)) if se > 0 and lo <= hi and lo > se and lo // KT == (se - 1) // KT]


def has_gap(c):
    se = send(c.Lk, c.spans, c.sink)
    return any(lo <= hi and lo > se for lo, hi in row_ranges(c))


def jumps(c):
    """the workgroups whose list has a jump: (workgroup, from tile, to tile)"""
    return [(n, ns - 1, b_lo) for n, (ns, b_lo, b_hi) in enumerate(block_lists(c)) if ns > 0 and b_lo <= b_hi and b_lo > ns]


def meetings(c):
    """the workgroups whose sink run and band run share tiles: (workgroup, first shared tile, last shared tile)"""
    out = []
    for n, q in enumerate(range(0, c.Lq, QB)):
        ns = block_lists(c)[n][0]
        lo, hi = fb.tile_range(q, min(q + QB, c.Lq) - 1, c.Lk, *rule(c)[:4])
        if ns > 0 and lo <= hi and lo <= ns - 1:
            out.append((n, lo, min(hi, ns - 1)))
    return out


def sink_ends_in_ragged_last_tile(c):
    se = send(c.Lk, c.spans, c.sink)
    return se > 0 and c.Lk % KT != 0 and (se - 1) // KT == (c.Lk - 1) // KT


def sink_tile_gap(c):
    """`ramp4`: the most a hidden key of the sink's LAST tile lies above a row's best visible key, over the rows (log2 domain)"""
    if c.pattern != "ramp4":
        return 0
    se = send(c.Lk, c.spans, c.sink)
    t = (se - 1) // KT
    score = RAMP_STEP * (torch.arange(c.Lk) % KT)
    vis = visible(c.Lq, c.Lk, *rule(c))
    gap = 0
    for i in range(c.Lq):
        hidden = ~vis[i, t * KT:(t + 1) * KT]
        if bool(hidden.any()):
            gap = max(gap, int(score[t * KT:(t + 1) * KT][hidden].max() - score[vis[i]].max()))
    return gap


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16)


def edge_targets(c):
    """j(i) of `edge_probe`: by i % 6 the first and the last key of the row's band part, the hidden keys right before and right behind it,
    the sink's last key and the first key behind the sink — cut to [0, Lk - 1] (a row without a band part aims at the sink's two)"""
    se = send(c.Lk, c.spans, c.sink)
    t = []
    for i, (lo, hi) in enumerate(row_ranges(c)):
        j = (se - 1, se)[i % 2] if lo > hi else (lo, hi, lo - 1, hi + 1, se - 1, se)[i % 6]
        t.append(min(max(j, 0), c.Lk - 1))
    return torch.tensor(t, dtype=torch.long)


def make_fsink_case(c):
    """seeded operands on the CPU in the form of attn_fband_cases.make_fband_case (its patterns; edge_probe with this file's targets)"""
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


def reference_fsink(c, ops, device="cpu"):
    return reference_masked(visible(c.Lq, c.Lk, *rule(c)), ops, c.H, device)


# ---- host emulation of the kernel's arithmetic, and the faults -------------------------------------------------------------------------------
#   sink_ignored          the frame window alone
#   sink_counts_rows      send = sink * rows[0]: the sink counted in rows of the first span instead of blocks
#   gap_visible           a row's set taken as [0, khi]: the hidden gap between the sink and the band shown
#   sink_end_off_by_one   send one key short
#   sink_not_cut_at_lk    send = start(sink) where Lk cuts it: the keys behind Lk of the ragged last tile count (the register path fills them
#                         with copies of key Lk - 1, as v2's does). The entry hands no such call to the kernel (send = Lk hides nothing: the
#                         global call), so the kernel's own cut is a guard; the row that shows the table would see it is norm_lk100_s8.
#   jump_not_taken        the DMA pointers not advanced across the jump: the band tiles read from the tiles right behind the sink's
#   meeting_tile_twice    the tiles the sink run and the band run share walked by both: their keys count twice
#   max_over_hidden       the row maximum over every key of the walked tiles (r28's)
FAULT_CASES = CASES + [c for c in NORMALISED if c.name == "norm_lk100_s8"]          # the rows the faults are tried on
FAULTS = ("sink_ignored", "sink_counts_rows", "gap_visible", "sink_end_off_by_one", "sink_not_cut_at_lk", "jump_not_taken", "meeting_tile_twice",
          "max_over_hidden")


def fault_applies(fault, c):
    """the rows of CASES on which the bound must flag the fault, by what each needs in order to show. The ramp rows serve max_over_hidden
    alone: every score of theirs is one of 64 values that repeat tile after tile, and a far row's sink keys weigh 2^-232."""
    if c not in CASES:
        return fault == "sink_not_cut_at_lk" and send(total_rows(c.spans), c.spans, c.sink) > c.Lk and c.Lk % KT != 0
    ramp = c.pattern == "ramp4"
    se, start = send(c.Lk, c.spans, c.sink), send(total_rows(c.spans), c.spans, c.sink)
    if fault == "max_over_hidden":
        return ramp and sink_tile_gap(c) > 0
    if ramp:
        return False
    if fault == "sink_ignored":                 # every row of CASES has a sink that adds pairs
        return True
    if fault == "sink_counts_rows":             # the two counts differ
        return min(c.sink * c.spans[0][0], c.Lk) != se
    if fault == "gap_visible":                  # a row with a gap, aimed at the hidden key right before its band part
        return c.pattern == "edge_probe" and any(lo <= hi and lo - 1 >= se and i % 6 == 2 for i, (lo, hi) in enumerate(row_ranges(c)))
    if fault == "sink_end_off_by_one":          # a row aimed at the sink's last key that its band part does not hold
        return c.pattern == "edge_probe" and any(not (lo <= se - 1 <= hi) and (i % 6 == 4 or (lo > hi and i % 2 == 0))
                                                 for i, (lo, hi) in enumerate(row_ranges(c)))
    if fault == "sink_not_cut_at_lk":
        return start > c.Lk and c.Lk % KT != 0
    if fault == "jump_not_taken":
        return bool(jumps(c))
    if fault == "meeting_tile_twice":           # a row that sees keys of a shared tile and keys of another one
        for n, lo, hi in meetings(c):
            for i in range(n * QB, min(n * QB + QB, c.Lq)):
                klo, khi = row_ranges(c)[i]
                seen = [(0, se - 1)] + ([(klo, khi)] if klo <= khi else [])
                tiles = {t for a, b in seen for t in range(a // KT, b // KT + 1)}
                if any(lo <= t <= hi for t in tiles) and any(not (lo <= t <= hi) for t in tiles):
                    return True
        return False
    raise KeyError(fault)


def emulate_fsink(c, ops, fault=None):
    """what a correct attn_fsink_kernel stores, on the CPU in fp32 (attn_fband_cases.emulate_fband's arithmetic over the visible keys of the two
    intervals), workgroup by workgroup over the tiles of its list; with a fault, what a kernel with that mistake stores. -> fp64 [Lq, H, 128]"""
    sg = ops["segs"][0]
    qf, kf, vf = sg["q"].float(), sg["k"].float(), sg["v"].float()
    Lq, Lk, H = c.Lq, c.Lk, c.H
    spans, q_pos0, back, ahead, sink = rule(c)
    se = send(Lk, spans, sink)
    band = fb.visible(Lq, Lk, spans, q_pos0, back, ahead)
    vis = band.clone()
    if fault == "sink_counts_rows":
        se = min(sink * spans[0][0], Lk)
    if fault == "sink_end_off_by_one":
        se -= 1
    if fault != "sink_ignored":
        vis[:, :se] = True
    if fault == "gap_visible":
        for i, (lo, hi) in enumerate(row_ranges(c)):
            if lo <= hi:
                vis[i, :hi + 1] = True
    weight = torch.ones(Lq, Lk)                                 # how many times a key is summed
    if fault == "sink_not_cut_at_lk":
        uncut = send(total_rows(spans), spans, sink)
        weight[:, Lk - 1] += max(0, min(uncut, (Lk + KT - 1) // KT * KT) - Lk)
    src = torch.arange(Lk).repeat(Lq, 1)                        # the key whose K / V rows are read for key j
    walked = torch.zeros(Lq, Lk, dtype=torch.bool)              # the keys of the tiles the row's workgroup walks
    for n, tl in enumerate(block_lists(c)):
        r0, r1 = n * QB, min(n * QB + QB, Lq)
        for t in tiles_of(tl):
            walked[r0:r1, t * KT:(t + 1) * KT] = True
        if fault == "jump_not_taken" and tl[1] <= tl[2] and tl[1] > tl[0] > 0:
            j0 = tl[1] * KT
            src[r0:r1, j0:] -= (tl[1] - tl[0]) * KT
    if fault == "meeting_tile_twice":
        for n, lo, hi in meetings(c):
            weight[n * QB:min(n * QB + QB, Lq), lo * KT:(hi + 1) * KT] += 1
    c2 = torch.tensor(ops["scale_log2"], dtype=torch.float32)
    out = torch.empty(Lq, H, D, dtype=torch.float32)
    rows = torch.arange(Lq).view(Lq, 1)
    for h in range(H):
        x = (qf[:, h] @ kf[:, h].T) * c2
        if fault == "jump_not_taken":
            x = x.gather(1, src)
        over = (walked | vis) if fault == "max_over_hidden" else vis
        m = torch.where(over, x, torch.full_like(x, -float("inf"))).max(dim=1, keepdim=True).values
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        e = x - m
        p = torch.where(e < -126.0, torch.zeros_like(e), torch.exp2(e))
        p = torch.where(vis, p, torch.zeros_like(p))
        l = (p * weight).sum(dim=1, keepdim=True)
        pb = ac._round_bf16(p) * weight
        if fault == "jump_not_taken":
            o = torch.zeros(Lq, D).index_put_((rows.expand(Lq, Lk).reshape(-1),), (pb.reshape(-1, 1) * vf[:, h][src.reshape(-1)]), accumulate=True)
        else:
            o = pb @ vf[:, h]
        out[:, h] = torch.where(l > 0, o / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(o))
    if ops["base"] is not None:
        out = out + ops["base"].float().view(Lq, H, D)
    return ac._round_bf16(out).double()


# ---- the builder's own checks: the tables produce what they were built for ----------------------------------------------------------------------
def check_tables():
    by = {c.name: c for c in CASES}
    names = [c.name for c in CASES + FBAND_EQUIV + NORMALISED]
    assert len(set(names)) == len(names)
    for c in CASES + FBAND_EQUIV + NORMALISED:
        N, NB = total_rows(c.spans), total_blocks(c.spans)
        assert c.H == 2 and 1 <= len(c.spans) <= MAX_SPANS and c.q_pos0 >= 0 and c.q_pos0 + c.Lq <= N and c.Lk <= N and 0 <= c.sink <= NB, c.name
    for c in CASES:               # the new kernel
        assert not hides_nothing(c.Lq, c.Lk, *rule(c)) and c.sink > 0 and not adds_nothing(c.Lq, c.Lk, *rule(c)), c.name
        assert not bool(empty_rows(c).any()), c.name                       # with a sink no row is empty
    for c in FBAND_EQUIV:         # the frame-band call, which itself runs its kernel
        assert not hides_nothing(c.Lq, c.Lk, *rule(c)) and (c.sink == 0 or adds_nothing(c.Lq, c.Lk, *rule(c))), c.name
        assert not fb.hides_nothing(c.Lq, c.Lk, *rule(c)[:4]), c.name
    for c in NORMALISED:
        assert hides_nothing(c.Lq, c.Lk, *rule(c)) and (c.sink == total_blocks(c.spans) or send(c.Lk, c.spans, c.sink) == c.Lk), c.name
    # a tile with two visible pieces and a gap: the rows of block 8 see 0-14 and 35-49 of tile 0
    c = by["tiny_blocks_s3_b1_a1"]
    assert send(c.Lk, c.spans, c.sink) == 15 and 40 in split_tile_rows(c) and row_ranges(c)[40] == (35, 49)
    # the jump: the last workgroup of the pyramid walks tile 0, then 6 ... 9
    assert block_lists(by["pyramid_s1_b1_a1"])[-1] == (1, 6, 9) and (4, 0, 6) in jumps(by["pyramid_s1_b1_a1"])
    assert jumps(by["pyramid_s1_b0_a0"]) and send(600, PYRAMID, 1) == 6
    # send = 120 inside tile 1; block 8 (rows 120 ...) adjoins the sink: one interval; block 9 (rows 216 ...) does not
    c = by["pyramid_s8_b0_a0"]
    assert send(c.Lk, c.spans, 8) == 120 and row_ranges(c)[120][0] == 120 and row_ranges(c)[216][0] == 216 and meetings(c) and jumps(c)
    assert send(384, ((64, 6),), 1) == 64 and send(384, ((128, 3),), 1) == 128
    # four interior sink tiles and one straddling; the unmasked body on sink tiles for a wave far behind
    c = by["big_blocks_s1_b0_a0"]
    assert [tile_is_interior(t, 640, 671, c.Lk, *rule(c)) for t in range(5)] == [True] * 4 + [False] and block_lists(c)[5][0] == 5
    # the sink's last tile the ragged last tile of the key axis, and no band part for any row
    c = by["trimmed_lk125_s8"]
    assert send(c.Lk, c.spans, c.sink) == 120 < c.Lk and c.Lk % KT and all(lo > hi for lo, hi in row_ranges(c))
    assert all(tl == (2, 2, 1) for tl in block_lists(c)) and sink_ends_in_ragged_last_tile(c)
    assert any(c.Lk < total_rows(c.spans) for c in CASES) and any(c.q_pos0 for c in CASES)
    assert {c.prescaled for c in CASES} == {True, False} and any(c.padded for c in CASES) and any(c.acc for c in CASES)
    assert any(split_tile_rows(c) for c in CASES) and any(jumps(c) for c in CASES) and any(meetings(c) for c in CASES)
    # the ramp: the gap on the sink's own tile beyond exp2's 126 (one_span's 35-key block leaves 116, as in r28: its lower keys carry it)
    assert {c.name: sink_tile_gap(c) for c in CASES if c.pattern == "ramp4"} == {
        "ramp4_pyramid_s1_b1_a1": 208, "ramp4_one_span_s1_b0_a0": 116, "ramp4_one_span30_s1_b0_a0": 136}
    for f in FAULTS:
        assert any(fault_applies(f, c) for c in FAULT_CASES), f


check_tables()


# ---- the call on the device ------------------------------------------------------------------------------------------------------------------
def run_fsink_case(c, ops, dev_ops=None, mode="fsink", variant=0):
    """one call into fresh operands (or `dev_ops`) -> the device operands. The rows of O the call owns are pre-filled with NaN (the old O
    under accumulate): what the kernel does not write shows. mode: "fsink", "fband" (the same call without the sink) or "global"."""
    from yume_amd import ops as yops
    d = dev_ops or device_operands(as_case(c), ops)
    if not c.acc:
        d["o"].fill_(float("nan"))
    fw = dict(frame_window=(c.back, c.ahead), spans=list(c.spans), q_pos0=c.q_pos0)
    kw = {"fsink": dict(fw, frame_sink=c.sink), "fband": fw, "global": {}}[mode]
    if mode == "fsink" and (c.sink == 0 or variant != 0):         # (ops.attn_fwd makes the frame-band call itself for sink = 0: the entry directly)
        call_entry(c, d, variant)
        return d
    yops.attn_fwd(d["q"], d["ks"][0], d["vts"][0], d["o"], c.Lq, c.Lk, c.H, scale=None if c.prescaled else SCALE, accumulate=c.acc, variant=variant,
                  q_prescaled=c.prescaled, kv_padded=c.padded, **kw)
    return d


def call_entry(c, d, variant=0):
    """yume_attn_fwd_fsink itself on the device operands d"""
    import ctypes
    from yume_amd import _lib, ops as yops
    yops.ensure_counters(d["q"].device)
    (qp, ldq), (kp, ldk), (vp, ldv), (op, ldo) = (yops._rows(t, n) for t, n in ((d["q"], "q"), (d["ks"][0], "k"), (d["vts"][0], "vt"), (d["o"], "out")))
    arr = ctypes.c_int64 * len(c.spans)
    flags = variant | (0x100 if c.prescaled else 0) | (0x200 if c.padded else 0)
    rc = _lib.load().yume_attn_fwd_fsink(qp, ldq, kp, ldk, vp, ldv, op, ldo, c.Lq, c.Lk, c.H, SCALE, int(c.acc), flags, c.q_pos0, len(c.spans),
                                         arr(*[r for r, _ in c.spans]), arr(*[b for _, b in c.spans]), c.back, c.ahead, c.sink, None, 0,
                                         yops._stream())
    _lib.check(rc, "yume_attn_fwd_fsink")


def main(argv):
    if argv != ["--routes"]:
        sys.exit(__doc__)
    from yume_amd import ops as yops
    yops.ensure_counters(torch.device("cuda", torch.cuda.current_device()))
    for c in CASES + NORMALISED + FBAND_EQUIV:
        ops = make_fsink_case(c)
        d = device_operands(as_case(c), ops)
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {c.name}\n")
        sys.stderr.flush()
        run_fsink_case(c, ops, d)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main(sys.argv[1:])
