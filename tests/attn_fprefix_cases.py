"""The case tables of the frame-window attention over two key buffers (yume_attn_fwd_fprefix, yume_amd/csrc/attn_fprefix.hpp), the Python
mirror of its rule (yume_amd/csrc/attn_fprefix_plan.hpp: change both or neither), the fp64 masked-softmax reference, and a host emulation of the
kernel's arithmetic in its padded coordinate with injected faults (no test functions in here). Built on tests/attn_fsink_cases.py, whose
`bound()` (tests/attn_cases.py's, KAPPA = 4.5) and reference machinery serve unchanged; H = 2, D = 128.

    the suffix: the partition, pos(i), b(p), back, ahead, Lk of tests/attn_fband_cases.py, keys numbered from 0;  n_prefix >= 0 prefix keys
    visible(i, prefix j) for every 0 <= j < n_prefix;  visible(i, suffix j)  <=>  the frame window's visible(i, j)
    the logical key order of the softmax (and of every [.., n_prefix + Lk] tensor in here) is prefix, then suffix
    padded coordinate: prefix key j at j, suffix key j at P + j, P = 64 ceil(n_prefix / 64); n_prefix ... P - 1 is nobody's key
    a run of rows walks the padded tiles [0, P / 64) and [P / 64 + t_lo, P / 64 + t_hi], ascending, each once

tests/test_attn_fprefix_routes_gpu.py runs one call per row of CASES, ONE_BUFFER_EQUIV and NORMALISED; tests/test_attn_fprefix_cases_cpu.py
proves the mirror against the compiled header and a brute-force walk, and the bound's reach over the faults on the host.

    python tests/attn_fprefix_cases.py --routes      one call per CASES, ONE_BUFFER_EQUIV and NORMALISED row, `CASE <name>` on stderr before each
"""
import math
import sys
import zlib
from collections import namedtuple
from functools import lru_cache

import torch

import attn_cases as ac
import attn_fband_cases as fb
import attn_fsink_cases as sc
from attn_fsink_cases import (D, GUARD_ROWS, KT, LOG2E, QB, QW, RAMP_STEP, SCALE, SENTINEL, as_case, bound, device_operands, fband_log,  # noqa: F401
                              reference_masked, total_blocks, total_rows, written)

# pform: how the prefix lies in memory beside the suffix (`form`, tests/attn_cases.py device_operands: engine_self ldk = 2 HC, engine_cross 3 HC)
#   tight   Kp [ceil64(n_prefix), HC] (ldkp = HC), Vtp [HC, ceil64(n_prefix)]
#   wide    Kp the right half of a [.., 2 HC] buffer (ldkp = 2 HC), Vtp a row slice of a taller buffer with 64 columns more
# either way the rows behind n_prefix of Kp and the columns behind n_prefix of Vtp hold NaN up to the next multiple of 64 (and beyond)
PCase = namedtuple("PCase", "name n_prefix spans Lq Lk q_pos0 back ahead H pattern form pform prescaled padded acc",
                   defaults=(2, "edge_probe", "engine_self", "tight", True, False, False))
S24 = ((24, 5),)                 # 120 rows: one workgroup, a ragged last suffix tile
S40 = ((40, 4),)                 # 160 rows: two workgroups, a ragged last suffix tile; under (0, 0) the second one skips suffix tile 0
S2 = ((8, 3), (40, 3))           # 144 rows, two spans
S32 = ((32, 4),)                 # 128 rows: every suffix tile whole


def _table():
    rows = [PCase("p1_s24_causal", 1, S24, 120, 120, 0, -1, 0),                                      # a one-key prefix: 63 pad coordinates
            PCase("p1_s40_b0a0", 1, S40, 160, 160, 0, 0, 0, form="engine_cross"),
            PCase("p52_s40_causal", 52, S40, 160, 160, 0, -1, 0),
            PCase("p52_s2_b1a1", 52, S2, 144, 144, 0, 1, 1, pattern="random", pform="wide"),
            PCase("p64_s24_b0a0", 64, S24, 120, 120, 0, 0, 0),                                       # exact prefix tiles
            PCase("p64_s32_b0a0", 64, S32, 128, 128, 0, 0, 0, form="engine_cross"),                  # no ragged tile at all: every tile by DMA
            PCase("p64_s40_causal_same", 64, S40, 160, 160, 0, -1, 0, pform="wide"),                 # ldkp == ldk
            PCase("p116_s40_b1a1", 116, S40, 160, 160, 0, 1, 1),                                     # a whole and a ragged prefix tile
            PCase("p116_s2_causal", 116, S2, 144, 144, 0, -1, 0, form="engine_cross", pform="wide"),
            PCase("p128_s2_causal", 128, S2, 144, 144, 0, -1, 0),
            PCase("p128_s40_b1a1", 128, S40, 160, 160, 0, 1, 1, pattern="random", form="engine_cross"),
            PCase("p180_s40_b0a0", 180, S40, 160, 160, 0, 0, 0),
            PCase("p180_s24_inf", 180, S24, 120, 120, 0, -1, -1, form="engine_cross"),               # a suffix window that hides nothing: still the kernel
            PCase("p116_s40_qpos60", 116, S40, 100, 160, 60, -1, 0, form="engine_cross"),            # q_pos0 > 0: the trailing rows
            PCase("p52_s40_lq131_lk150", 52, S40, 131, 150, 0, 1, 1),                                # Lq ragged against the block, Lk < N
            PCase("p116_s24_acc", 116, S24, 120, 120, 0, 0, 0, acc=True),
            PCase("p52_s40_unscaled", 52, S40, 160, 160, 0, -1, 0, prescaled=False, pform="wide", form="engine_cross"),
            PCase("ramp4_p1_s24_b0a0", 1, S24, 120, 120, 0, 0, 0, pattern="ramp4"),
            PCase("ramp4_p1_s24_causal", 1, S24, 120, 120, 0, -1, 0, pattern="ramp4", form="engine_cross")]
    return rows


CASES = _table()
# n_prefix a whole number of tiles, prefix and suffix views of ONE [n_prefix + Lk] buffer: the one-buffer call with the prefix as one more
# leading block, frame_sink = 1 and q_pos0 moved by n_prefix walks the same tiles in the same order with the same per-tile body: equal bits,
# whichever of yume_attn_fwd_fsink / yume_attn_fwd_fband that call normalises to. (Not a window that hides nothing: that one-buffer call is
# the global one, another kernel.)
ONE_BUFFER_EQUIV = [PCase("one_p64_s40_causal", 64, S40, 160, 160, 0, -1, 0, pattern="random"),
                    PCase("one_p64_s24_b0a0", 64, S24, 120, 120, 0, 0, 0),
                    PCase("one_p128_s2_b1a1", 128, S2, 144, 144, 0, 1, 1),
                    PCase("one_p128_s40_qpos60_b0a0", 128, S40, 100, 160, 60, 0, 0, pattern="random")]
# n_prefix = 0: yume_attn_fwd_fband with the suffix arguments, bit for bit, with its log line
NORMALISED = [PCase("norm_p0_s40_causal", 0, S40, 160, 160, 0, -1, 0, pattern="random"),
              PCase("norm_p0_s2_b1a1", 0, S2, 144, 144, 0, 1, 1, form="engine_cross")]
# what the entry point must refuse: (name, keyword overrides of a valid call that reaches the kernel, error code, a word of the message, the
# entry that answers). fband's list on the suffix side through the new entry point, then the prefix's own. Variant 14 IS the new kernel; what
# refuses it is the frame-band entry, which a call with n_prefix = 0 is handed to.
EINVAL, EUNSUP = fb.EINVAL, fb.EUNSUP
REFUSALS = [r + ("attn_fwd_fprefix",) for r in fb.REFUSALS if not r[0].startswith("variant")] + [
    ("n_prefix_minus_1", dict(n_prefix=-1), EINVAL, "n_prefix", "attn_fwd_fprefix"),
    ("n_prefix_2_31", dict(n_prefix=2 ** 31 - 100, ldvtp=2 ** 31), EINVAL, "2^31", "attn_fwd_fprefix"),
    ("null_kp", dict(Kp=None), EINVAL, "NULL", "attn_fwd_fprefix"), ("null_vtp", dict(Vtp=None), EINVAL, "NULL", "attn_fwd_fprefix"),
    ("misaligned_kp", dict(Kp=4096 + 8), EINVAL, "alignment", "attn_fwd_fprefix"),
    ("misaligned_vtp", dict(Vtp=4096 + 2), EINVAL, "alignment", "attn_fwd_fprefix"),
    ("ldkp_odd", dict(ldkp=260), EINVAL, "ldkp", "attn_fwd_fprefix"), ("ldvtp_odd", dict(ldvtp=108), EINVAL, "ldvtp", "attn_fwd_fprefix"),
    ("ldvtp_short", dict(ldvtp=96), EINVAL, "ldvtp", "attn_fwd_fprefix"),
    ("variant_7", dict(variant=7), EUNSUP, "variant 7", "attn_fwd_fprefix"), ("variant_13", dict(variant=13), EUNSUP, "variant 13", "attn_fwd_fprefix"),
    ("variant_12_flags", dict(variant=12 | 0x100 | 0x200), EUNSUP, "variant 12", "attn_fwd_fprefix"),
    ("variant_14_flags_p0", dict(variant=14 | 0x100 | 0x200, n_prefix=0), EUNSUP, "variant 14", "attn_fwd_fband")]
REFUSAL_DEFAULT = dict(Lq=300, Lk=315, H=2, ldvt=320, variant=0, q_pos0=0, spans=fb.ONE_SPAN, back=1, ahead=0, ldkp=256, ldvtp=104, n_prefix=100)


# ---- the rule: Python mirror of yume_amd/csrc/attn_fprefix_plan.hpp --------------------------------------------------------------------------
def rule(c):
    """the arguments of the mirror functions behind (rows, Lk)"""
    return tuple(c.spans), c.q_pos0, c.back, c.ahead, c.n_prefix


def prefix_tiles(n_prefix):
    return (n_prefix + KT - 1) // KT


def pad(n_prefix):
    return prefix_tiles(n_prefix) * KT


def visible(Lq, Lk, spans, q_pos0, back, ahead, n_prefix):
    """bool [Lq, n_prefix + Lk] in the logical order"""
    return torch.cat([torch.ones(Lq, n_prefix, dtype=torch.bool), fb.visible(Lq, Lk, spans, q_pos0, back, ahead)], dim=1)


def visible_padded(Lq, Lk, spans, q_pos0, back, ahead, n_prefix):
    """bool [Lq, P + Lk] in the padded coordinate"""
    P = pad(n_prefix)
    m = torch.zeros(Lq, P + Lk, dtype=torch.bool)
    m[:, :n_prefix] = True
    m[:, P:] = fb.visible(Lq, Lk, spans, q_pos0, back, ahead)
    return m


def tile_list(q_first, q_last, Lk, spans, q_pos0, back, ahead, n_prefix):
    """(np, b_lo, b_hi) in padded tiles; without suffix tiles b_lo = np, b_hi = np - 1"""
    np_ = prefix_tiles(n_prefix)
    lo, hi = fb.tile_range(q_first, q_last, Lk, spans, q_pos0, back, ahead)
    return (np_, np_, np_ - 1) if lo > hi else (np_, np_ + lo, np_ + hi)


tiles_of, next_tile = sc.tiles_of, sc.next_tile


def tile_is_interior(t, q_first, q_last, Lk, spans, q_pos0, back, ahead, n_prefix):
    np_ = prefix_tiles(n_prefix)
    if t < np_:
        return t * KT + KT - 1 < n_prefix
    return fb.tile_is_interior(t - np_, q_first, q_last, Lk, spans, q_pos0, back, ahead)


@lru_cache(maxsize=None)
def block_lists(c):
    """[(np, b_lo, b_hi)] of the 128-row workgroups of the call"""
    return [tile_list(q, min(q + QB, c.Lq) - 1, c.Lk, *rule(c)) for q in range(0, c.Lq, QB)]


def tiles_min_max(c):
    n = [len(tiles_of(tl)) for tl in block_lists(c)]
    return min(n), max(n)


@lru_cache(maxsize=None)
def row_ranges(c):
    """[(klo, khi)] of the frame window on the suffix, row by row"""
    return [fb.key_range(i, i, c.Lk, *rule(c)[:4]) for i in range(c.Lq)]


def jumps(c):
    """the workgroups whose list skips suffix tiles behind the prefix: (workgroup, first suffix tile walked)"""
    return [(n, b_lo - np_) for n, (np_, b_lo, b_hi) in enumerate(block_lists(c)) if b_lo <= b_hi and b_lo > np_]


def ld_of(c):
    """(ldk, ldkp) the operand forms give"""
    HC = c.H * D
    return {"engine_self": 2 * HC, "engine_cross": 3 * HC, "tight": HC}[c.form], {"tight": HC, "wide": 2 * HC}[c.pform]


def ramp_gap(c):
    """`ramp4`: the most a hidden coordinate of a walked tile lies above a row's best visible key, over the rows (log2 domain)"""
    if c.pattern != "ramp4":
        return 0
    P = pad(c.n_prefix)
    score = RAMP_STEP * (torch.arange(P + c.Lk) % KT)
    score[c.n_prefix:P] = score[c.n_prefix - 1]                 # the pad: copies of the last prefix key
    vis = visible_padded(c.Lq, c.Lk, *rule(c))
    gap = 0
    for n, tl in enumerate(block_lists(c)):
        cols = torch.zeros(P + c.Lk, dtype=torch.bool)
        for t in tiles_of(tl):
            cols[t * KT:(t + 1) * KT] = True
        for i in range(n * QB, min(n * QB + QB, c.Lq)):
            hidden = cols & ~vis[i]
            if bool(hidden.any()):
                gap = max(gap, int(score[hidden].max() - score[vis[i]].max()))
    return gap


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16)


def edge_targets(c):
    """j(i) of `edge_probe` in the LOGICAL order: by i % 6 the first and the last key of the row's suffix interval, the suffix keys right before
    and right behind it, the last prefix key and prefix key 0 — the suffix ones cut to the suffix"""
    n, t = c.n_prefix, []
    for i, (lo, hi) in enumerate(row_ranges(c)):
        j = (n - 1, 0)[i % 2] if lo > hi else (n + lo, n + hi, n + max(lo - 1, 0), n + min(hi + 1, c.Lk - 1), n - 1, 0)[i % 6]
        t.append(j)
    return torch.tensor(t, dtype=torch.long)


def make_case(c):
    """seeded operands on the CPU: "q" [Lq, H, D], "k" / "v" [n_prefix + Lk, H, D] in the logical order (bf16), "base", "scale_log2"; "segs" is
    the one-segment form reference_masked reads"""
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c.name.encode()))
    scale_log2 = 1.0 if c.prescaled else float(torch.tensor(SCALE, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    H, Lq, L = c.H, c.Lq, c.n_prefix + c.Lk
    r = torch.randn(Lq, H, D, generator=g)
    k = _bf16(torch.randn(L, H, D, generator=g)).float()
    v = _bf16(torch.randn(L, H, D, generator=g))
    q = r
    if c.pattern == "edge_probe":
        gain = (math.log(L) + 0.3) / (SCALE * D)
        q = 0.5 * r + gain * k[edge_targets(c)]
    if c.prescaled:
        q = q * (SCALE * LOG2E)
    q = _bf16(q).float()
    if c.pattern == "ramp4":
        assert c.prescaled
        q = torch.zeros(Lq, H, D)
        q[:, :, 0] = float(RAMP_STEP)
        coord = torch.cat([torch.arange(c.n_prefix), pad(c.n_prefix) + torch.arange(c.Lk)])
        k[:, :, 0] = (coord % KT).view(L, 1).float()
    assert torch.equal(_bf16(q).float(), q) and torch.equal(_bf16(k).float(), k)
    base = _bf16(torch.randn(Lq, H * D, generator=g)) if c.acc else None
    return {"segs": [{"q": _bf16(q), "k": _bf16(k), "v": v, "w": 1.0}], "base": base, "scale_log2": scale_log2}


def reference(c, ops, device="cpu"):
    return reference_masked(visible(c.Lq, c.Lk, *rule(c)), ops, c.H, device)


# ---- host emulation of the kernel's arithmetic, and the faults -------------------------------------------------------------------------------
# The emulation works in the kernel's padded coordinate: K / V of coordinate c, the pad coordinates of either ragged tile being what the
# register path stores there (the K row of the segment's last key, V = 0).
#   suffix_shift_n_prefix   the suffix interval shifted by n_prefix instead of P
#   prefix_pad_unmasked     the pad coordinates of the ragged prefix tile visible
#   prefix_suffix_strides   the K rows of a prefix tile read with the suffix's row stride
#   jump_advances_prefix    the prefetch across the switch advancing the prefix pointers: the suffix tiles read from the prefix buffer
#   last_prefix_tile_skip   the last prefix tile not walked
#   interior_ignores_send   a prefix tile behind tile 0 taken for whole without looking at n_prefix: its pad coordinates count, unmasked
#   max_over_hidden         the row maximum over every coordinate of the walked tiles (r28's)
FAULTS = ("suffix_shift_n_prefix", "prefix_pad_unmasked", "prefix_suffix_strides", "jump_advances_prefix", "last_prefix_tile_skip",
          "interior_ignores_send", "max_over_hidden")


def fault_applies(fault, c):
    """the rows of CASES on which the bound must flag the fault, by what each needs in order to show. The ramp rows serve max_over_hidden
    alone (every score of theirs is one of 64 values, and a far key weighs nothing)."""
    ramp = c.pattern == "ramp4"
    n, ragged = c.n_prefix, c.n_prefix % KT != 0
    if fault == "max_over_hidden":
        return ramp and ramp_gap(c) > 126
    if ramp:
        return False
    probe = c.pattern == "edge_probe"
    if fault == "suffix_shift_n_prefix":        # the shift differs, and a row aims at an edge of its interval that moves
        return ragged and probe
    if fault == "prefix_pad_unmasked":          # a row aimed at the last prefix key, whose copies the pad holds
        return ragged and probe
    if fault == "prefix_suffix_strides":        # the strides differ: key j is read from row j ldk / ldkp
        ldk, ldkp = ld_of(c)
        return ldk != ldkp and n >= 2 and probe
    if fault == "jump_advances_prefix":
        return True
    if fault == "last_prefix_tile_skip":        # a row aimed at the last prefix key
        return probe
    if fault == "interior_ignores_send":
        return ragged and prefix_tiles(n) >= 2 and probe
    raise KeyError(fault)


def emulate(c, ops, fault=None):
    """what a correct attn_fprefix_kernel stores, on the CPU in fp32 (tests/attn_fsink_cases.py emulate_fsink's arithmetic) over the padded
    coordinate; with a fault, what a kernel with that mistake stores. -> fp64 [Lq, H, 128]"""
    sg = ops["segs"][0]
    qf, kl, vl = sg["q"].float(), sg["k"].float(), sg["v"].float()
    Lq, Lk, H, n = c.Lq, c.Lk, c.H, c.n_prefix
    spans, q_pos0, back, ahead, _ = rule(c)
    P, np_ = pad(n), prefix_tiles(n)
    Ls = (Lk + KT - 1) // KT * KT
    W = P + Ls
    # coordinate -> the logical key whose K row is read; has_v: its V row counts (pad: zeroed by the register path)
    src = torch.cat([torch.arange(P).clamp(max=n - 1), n + torch.arange(Ls).clamp(max=Lk - 1)])
    has_v = torch.cat([torch.arange(P) < n, torch.arange(Ls) < Lk])
    vis = torch.zeros(Lq, W, dtype=torch.bool)
    vis[:, :n] = True
    band = fb.visible(Lq, Lk, spans, q_pos0, back, ahead)
    shift = n if fault == "suffix_shift_n_prefix" else P
    vis[:, shift:shift + Lk] |= band
    if fault == "prefix_pad_unmasked" or (fault == "interior_ignores_send" and np_ >= 2):
        vis[:, n:P] = True
    if fault == "last_prefix_tile_skip":
        vis[:, (np_ - 1) * KT:P] = False
    ksrc = src.clone()
    if fault == "prefix_suffix_strides":
        ldk, ldkp = ld_of(c)
        ksrc[:P] = (src[:P] * ldk // ldkp) % n                 # (a row behind the buffer: emulated as a wrapped one)
    vsrc = src.clone()
    if fault == "jump_advances_prefix":
        ksrc[P:] = (P + torch.arange(Ls)) % n
        vsrc[P:] = ksrc[P:]
    kf, vf = kl[ksrc], vl[vsrc] * has_v.view(W, 1, 1).float()
    walked = torch.zeros(Lq, W, dtype=torch.bool)
    for b, tl in enumerate(block_lists(c)):
        for t in tiles_of(tl):
            walked[b * QB:min(b * QB + QB, Lq), t * KT:(t + 1) * KT] = True
    assert bool((walked | ~vis).all()) or fault is not None     # a correct walk covers every visible coordinate
    vis &= walked
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


# ---- the builder's own checks: the tables produce what they were built for ----------------------------------------------------------------------
def check_tables():
    by = {c.name: c for c in CASES}
    names = [c.name for c in CASES + ONE_BUFFER_EQUIV + NORMALISED]
    assert len(set(names)) == len(names)
    for c in CASES + ONE_BUFFER_EQUIV + NORMALISED:
        N = total_rows(c.spans)
        assert c.H == 2 and c.q_pos0 >= 0 and c.q_pos0 + c.Lq <= N and c.Lk <= N and c.n_prefix >= 0, c.name
    assert {c.n_prefix for c in CASES} == {1, 52, 64, 116, 128, 180}
    assert {tuple(c.spans) for c in CASES} >= {S24, S40, S2} and total_rows(S24) == 120 and total_rows(S40) == 160
    assert {(c.back, c.ahead) for c in CASES} == {(-1, 0), (0, 0), (1, 1), (-1, -1)}
    assert any(c.q_pos0 > 0 for c in CASES) and any(c.Lq % QB and c.Lq > QB for c in CASES) and any(c.acc for c in CASES)
    assert any(not c.prescaled for c in CASES) and any(c.Lk < total_rows(c.spans) for c in CASES)
    differ = [ld_of(c)[0] != ld_of(c)[1] for c in CASES]
    assert sum(differ) * 2 >= len(CASES) and not all(differ)
    assert all(c.n_prefix in (64, 128) and (c.back, c.ahead) != (-1, -1) for c in ONE_BUFFER_EQUIV) and {c.n_prefix for c in ONE_BUFFER_EQUIV} == {64, 128}
    assert all(c.n_prefix == 0 and not fb.hides_nothing(c.Lq, c.Lk, *rule(c)[:4]) for c in NORMALISED)
    # the second workgroup of the 160-row suffix under (0, 0) sees frame 3 alone: suffix tile 0 is skipped
    assert block_lists(by["p180_s40_b0a0"]) == [(3, 3, 5), (3, 4, 5)] and jumps(by["p180_s40_b0a0"]) == [(1, 1)]
    assert block_lists(by["p1_s24_causal"]) == [(1, 1, 2)] and tiles_min_max(by["p116_s40_b1a1"]) == (4, 5)
    # no ragged tile at all, and both ragged at once
    assert by["p64_s32_b0a0"].n_prefix % KT == 0 and by["p64_s32_b0a0"].Lk % KT == 0
    assert any(c.n_prefix % KT and c.Lk % KT for c in CASES) and any(c.n_prefix % KT == 0 and c.Lk % KT for c in CASES)
    # interior tiles of both kinds, for the last wave of p128_s40_b1a1: both prefix tiles; the whole suffix tile 1 (keys 64 ... 127) lies
    # inside frames 2 ... 3 = keys 80 ... 159 for no wave, so under (-1, 0) of the same suffix: tiles 0 and 1 for the last wave
    c = by["p128_s40_b1a1"]
    assert [tile_is_interior(t, 128, 159, c.Lk, *rule(c)) for t in range(5)] == [True, True, False, False, False]
    c = by["p64_s40_causal_same"]
    assert [tile_is_interior(t, 128, 159, c.Lk, *rule(c)) for t in range(4)] == [True, True, True, False]
    assert [tile_is_interior(t, 0, 31, c.Lk, *rule(c)) for t in range(4)] == [True, False, False, False]
    c = by["p116_s40_b1a1"]
    assert [tile_is_interior(t, 0, 31, c.Lk, *rule(c)) for t in range(2)] == [True, False]
    assert {c.name: ramp_gap(c) for c in CASES if c.pattern == "ramp4"} == {"ramp4_p1_s24_b0a0": 160, "ramp4_p1_s24_causal": 160}
    for f in FAULTS:
        assert any(fault_applies(f, c) for c in CASES), f


check_tables()


# ---- the call on the device ------------------------------------------------------------------------------------------------------------------
def device_operands_prefix(c, ops, device="cuda"):
    """the suffix, q and O in the row's `form` (tests/attn_cases.py device_operands: NaN behind Lk in K and V^T, guards around O), the prefix in
    its `pform` with NaN behind n_prefix -> device_operands' dict with "kp", "vtp" added. The suffix's V^T is replaced by one whose NaN
    columns reach the next multiple of 64."""
    nan = float("nan")
    sg = ops["segs"][0]
    n, H, HC = c.n_prefix, c.H, c.H * D
    sops = {"segs": [{"q": sg["q"], "k": sg["k"][n:], "v": sg["v"][n:], "w": 1.0}], "base": ops["base"], "scale_log2": ops["scale_log2"]}
    d = device_operands(as_case(c), sops, device)
    Ls = (c.Lk + KT - 1) // KT * KT
    vb = torch.full((HC + 2 * D, Ls), nan, dtype=torch.bfloat16)
    vb[D:D + HC, :c.Lk] = sg["v"][n:].reshape(c.Lk, HC).T
    d["vts"] = [vb.to(device)[D:D + HC]]
    if n == 0:
        d["kp"] = d["vtp"] = None
        return d
    P = pad(n)
    if c.pform == "tight":
        kb = torch.full((P, HC), nan, dtype=torch.bfloat16)
        kb[:n] = sg["k"][:n].reshape(n, HC)
        d["kp"] = kb.to(device)[:n]
        vb = torch.full((HC, P), nan, dtype=torch.bfloat16)
        vb[:, :n] = sg["v"][:n].reshape(n, HC).T
        d["vtp"] = vb.to(device)
    else:
        kb = torch.full((P + 8, 2 * HC), nan, dtype=torch.bfloat16)
        kb[:n, HC:] = sg["k"][:n].reshape(n, HC)
        d["kp"] = kb.to(device)[:n, HC:]
        vb = torch.full((D + HC + D, P + KT), nan, dtype=torch.bfloat16)
        vb[D:D + HC, :n] = sg["v"][:n].reshape(n, HC).T
        d["vtp"] = vb.to(device)[D:D + HC]
    return d


def run_case(c, ops, dev_ops=None, variant=0):
    """one call into fresh operands (or `dev_ops`) -> the device operands. The rows of O the call owns are pre-filled with NaN (the old O
    under accumulate): what the kernel does not write shows."""
    from yume_amd import ops as yops
    d = dev_ops or device_operands_prefix(c, ops)
    if not c.acc:
        d["o"].fill_(float("nan"))
    yops.attn_fwd(d["q"], d["ks"][0], d["vts"][0], d["o"], c.Lq, c.Lk, c.H, scale=None if c.prescaled else SCALE, accumulate=c.acc, variant=variant,
                  q_prescaled=c.prescaled, kv_padded=c.padded, frame_window=(c.back, c.ahead), spans=list(c.spans), q_pos0=c.q_pos0,
                  prefix=(d["kp"], d["vtp"], c.n_prefix))
    return d


def run_fband(c, ops):
    """the same suffix call without a prefix argument at all: yume_attn_fwd_fband"""
    from yume_amd import ops as yops
    d = device_operands_prefix(c, ops)
    d["o"].fill_(float("nan"))
    yops.attn_fwd(d["q"], d["ks"][0], d["vts"][0], d["o"], c.Lq, c.Lk, c.H, scale=None if c.prescaled else SCALE, q_prescaled=c.prescaled,
                  frame_window=(c.back, c.ahead), spans=list(c.spans), q_pos0=c.q_pos0)
    return d


def one_buffer_operands(c, ops, device="cuda"):
    """prefix and suffix as views of ONE K buffer [n_prefix + ceil64(Lk), 2 HC] (right half) and ONE V^T buffer [HC, n_prefix + ceil64(Lk)], NaN
    behind the last key; q and two O buffers with guards -> dict"""
    nan = float("nan")
    sg = ops["segs"][0]
    n, HC, L = c.n_prefix, c.H * D, c.n_prefix + c.Lk
    rows = n + (c.Lk + KT - 1) // KT * KT
    kb = torch.full((rows, 2 * HC), nan, dtype=torch.bfloat16)
    kb[:L, HC:] = sg["k"].reshape(L, HC)
    vb = torch.full((HC, rows), nan, dtype=torch.bfloat16)
    vb[:, :L] = sg["v"].reshape(L, HC).T
    kb, vb = kb.to(device), vb.to(device)
    q = sg["q"].reshape(c.Lq, HC).to(device)
    obuf = [torch.full((GUARD_ROWS + c.Lq + GUARD_ROWS, HC), SENTINEL, dtype=torch.bfloat16, device=device) for _ in range(2)]
    return {"q": q, "k_all": kb[:L, HC:], "vt_all": vb, "kp": kb[:n, HC:], "k": kb[n:L, HC:], "vtp": vb[:, :n], "vt": vb[:, n:], "obuf": obuf,
            "o": [o[GUARD_ROWS:GUARD_ROWS + c.Lq] for o in obuf]}


def run_one_buffer_pair(c, ops):
    """-> (obuf of the two-buffer call, obuf of the one-buffer call with the prefix as a leading block and frame_sink = 1)"""
    from yume_amd import ops as yops
    d = one_buffer_operands(c, ops)
    for o in d["o"]:
        o.fill_(float("nan"))
    kw = dict(scale=None if c.prescaled else SCALE, q_prescaled=c.prescaled, frame_window=(c.back, c.ahead))
    yops.attn_fwd(d["q"], d["k"], d["vt"], d["o"][0], c.Lq, c.Lk, c.H, spans=list(c.spans), q_pos0=c.q_pos0, prefix=(d["kp"], d["vtp"], c.n_prefix),
                  **kw)
    yops.attn_fwd(d["q"], d["k_all"], d["vt_all"], d["o"][1], c.Lq, c.n_prefix + c.Lk, c.H, spans=[(c.n_prefix, 1)] + list(c.spans),
                  q_pos0=c.n_prefix + c.q_pos0, frame_sink=1, **kw)
    return d["obuf"]


def main(argv):
    if argv != ["--routes"]:
        sys.exit(__doc__)
    from yume_amd import ops as yops
    yops.ensure_counters(torch.device("cuda", torch.cuda.current_device()))
    for c in CASES + NORMALISED:
        ops = make_case(c)
        d = device_operands_prefix(c, ops)
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {c.name}\n")
        sys.stderr.flush()
        run_case(c, ops, d)
        torch.cuda.synchronize()
    for c in ONE_BUFFER_EQUIV:
        ops = make_case(c)
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {c.name}\n")
        sys.stderr.flush()
        run_one_buffer_pair(c, ops)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main(sys.argv[1:])
