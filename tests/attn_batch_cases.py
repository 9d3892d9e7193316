"""The case table of yume_attn_fwd_batch (batched self-attention: nseg problems of one shape stacked in the same buffers) and its operands in
the stacked layout (no test functions in here). Inputs, the fp64 reference and the per-element bound are tests/attn_cases.py's: a batch case
is one of its segmented cases (every segment its own seeded q, k, v) whose segments all have Lk keys and a last-key weight of 1.

    python tests/attn_batch_cases.py --routes     one batch call per case and, for the persistent route, one ops.attn_fwd(variant=8) per segment
                                                  view; `CASE <name>` on stderr before each case (YUME_ATTN_LOG=1 names the kernels and the plans)
"""
import sys
from collections import namedtuple

import torch

import attn_cases as ac

D, KT = ac.D, ac.KT
GUARD_ROWS, GUARD_COLS = ac.GUARD_ROWS, ac.GUARD_COLS

# form: "split" = Q, K, V^T, O in buffers of their own; "engine" = Q and K are the two column halves of ONE [rows, 2 HC] buffer (what
# DiTEngine.forward_batch issues: q_pitch == k_pitch); "far" = row strides of 65536 elements and pitches of 32832 rows, so that segment 1's base
# lies beyond 4 GiB in Q, in K and in O (buffers from torch.empty, only the rows used are initialised).
# route / plan: what the YUME_ATTN_LOG line of the call must name; plan = attn_plan's for nseg * H heads (tests/test_attn_batch_cabi.py holds
# the table to attn_plan.hpp), None where the test does not pin it.
BCase = namedtuple("BCase", "name nseg H Lq Lk q_pitch k_pitch variant form route plan acc")


def _ceil(x, m):
    return (x + m - 1) // m * m


TABLE = [
    # whole blocks, ragged last query block, ragged last key tile, fewer virtual heads than XCDs
    BCase("b1_whole_2x1", 2, 1, 300, 520, 320, 576, 8, "split", "batch_v8", (2, 1), False),
    # 9 virtual heads: two on XCD 0; also accumulating
    BCase("b2_whole_3x3", 3, 3, 300, 520, 320, 576, 8, "split", "batch_v8", (2, 1), False),
    BCase("b2_whole_3x3_acc", 3, 3, 300, 520, 320, 576, 8, "split", "batch_v8", (2, 1), True),
    # key-range pieces and the merge
    BCase("b3_s2_2x1", 2, 1, 8442, 1030, _ceil(8442, 64), _ceil(1030, 64), 8, "split", "batch_v8", (32, 2), False),
    # ... with two virtual heads per XCD
    BCase("b4_s2_3x3", 3, 3, 4346, 1030, _ceil(4346, 64), _ceil(1030, 64), 8, "split", "batch_v8", (16, 2), False),
    # the automatic route, split in 4
    BCase("b5_s4_auto_2x1", 2, 1, 8442, 2100, _ceil(8442, 64), _ceil(2100, 64), 0, "split", "batch_v8", (32, 4), False),
    # too few keys for the persistent kernel: the segmented 4-wave kernel over views
    BCase("b6_segv2_2x4", 2, 4, 300, 300, 320, 320, 0, "split", "seg_v2", None, False),
    # what the engine issues
    BCase("b7_engine_2x4", 2, 4, 560, 560, 576, 576, 8, "engine", "batch_v8", None, False),
    # a segment base beyond 4 GiB
    BCase("b8_far_2x1", 2, 1, 300, 520, 32832, 32832, 8, "far", "batch_v8", (2, 1), False),
]
PATTERNS = ("probe", "random")
# `stairs` (tests/attn_cases.py: a score offset per key tile that leaves the base-free body's range) sends EVERY item of EVERY segment through
# the cold rerun on the robust body, whose K / V^T sources and partial-result slices must be the item's segment's: whole blocks with two
# virtual heads on one XCD, and key-range pieces with the merge
RERUN_CASES = [c for c in TABLE if c.name in ("b2_whole_3x3", "b3_s2_2x1")]
PROPERTY_CASES = [c for c in TABLE if c.name.startswith(("b1", "b2", "b3", "b4", "b5"))]
FAR_LD = 65536


def as_case(c, pattern):
    """the attn_cases.Case whose make_case / reference serve this batch case"""
    return ac.Case(f"{c.name}_{pattern}", "seg", c.variant, c.Lq, (c.Lk,) * c.nseg, c.H, pattern, "engine_self", True, True, (1.0,) * c.nseg,
                   c.acc, c.route, c.plan, c.q_pitch, True)


def device_operands(c, ops, device="cuda"):
    """the stacked buffers of one call. Everything a kernel must not use for a result holds NaN (q rows outside the segments, k rows >= Lk of
    a segment, the V^T columns between a segment's last whole key tile and the next segment), V^T's columns [Lk, ceil64(Lk)) hold PAD_VALUE,
    everything that must not be written SENTINEL (guard rows, guard columns, pitch gaps of O).
    -> {"q", "k", "vt", "o": the views the call gets, "obuf": O with its guards, "r0": first row of o in obuf}"""
    nan = float("nan")
    H, HC, n = c.H, c.H * D, c.nseg
    rows = (n - 1) * c.q_pitch + c.Lq
    Lp = _ceil(c.Lk, KT)
    krows = (n - 1) * c.k_pitch + Lp
    segs = ops["segs"]
    dev = torch.device(device)
    bf = torch.bfloat16
    if c.form == "far":
        qbuf = torch.empty(GUARD_ROWS + rows + GUARD_ROWS, FAR_LD, dtype=bf, device=dev)
        kbuf = torch.empty(krows, FAR_LD, dtype=bf, device=dev)
        obuf = torch.empty(GUARD_ROWS + rows + GUARD_ROWS, FAR_LD, dtype=bf, device=dev)
        q, k = qbuf[GUARD_ROWS:GUARD_ROWS + rows, :HC], kbuf[:, :HC]
        for s in range(n):                       # only the rows used (and their neighbours) are initialised
            a = GUARD_ROWS + s * c.q_pitch
            qbuf[a - GUARD_ROWS:a + c.Lq + GUARD_ROWS] = nan
            obuf[a - GUARD_ROWS:a + c.Lq + GUARD_ROWS] = ac.SENTINEL
            kbuf[s * c.k_pitch:s * c.k_pitch + Lp] = nan
    elif c.form == "engine":
        assert c.q_pitch == c.k_pitch
        qk = torch.full((max(GUARD_ROWS + rows + GUARD_ROWS, krows), 2 * HC), nan, dtype=bf, device=dev)
        q, k = qk[:rows, :HC], qk[:krows, HC:]
        obuf = torch.full((GUARD_ROWS + rows + GUARD_ROWS, HC + GUARD_COLS), ac.SENTINEL, dtype=bf, device=dev)
    else:
        qbuf = torch.full((GUARD_ROWS + rows + GUARD_ROWS, HC), nan, dtype=bf, device=dev)
        kbuf = torch.full((krows, HC + D), nan, dtype=bf, device=dev)
        q, k = qbuf[GUARD_ROWS:GUARD_ROWS + rows], kbuf[:, :HC]
        obuf = torch.full((GUARD_ROWS + rows + GUARD_ROWS, HC + GUARD_COLS), ac.SENTINEL, dtype=bf, device=dev)
    vb = torch.full((D + HC + D, krows), nan, dtype=bf, device=dev)
    vt = vb[D:D + HC]
    o = obuf[GUARD_ROWS:GUARD_ROWS + rows, :HC]
    for s, sg in enumerate(segs):
        q[s * c.q_pitch:s * c.q_pitch + c.Lq] = sg["q"].reshape(c.Lq, HC).to(dev)
        k[s * c.k_pitch:s * c.k_pitch + c.Lk] = sg["k"].reshape(c.Lk, HC).to(dev)
        vt[:, s * c.k_pitch:s * c.k_pitch + c.Lk] = sg["v"].reshape(c.Lk, HC).T.to(dev)
        vt[:, s * c.k_pitch + c.Lk:s * c.k_pitch + Lp] = ac.PAD_VALUE
        if ops["base"] is not None:
            o[s * c.q_pitch:s * c.q_pitch + c.Lq] = ops["base"][s * c.q_pitch:s * c.q_pitch + c.Lq].to(dev)
    return {"q": q, "k": k, "vt": vt, "o": o, "obuf": obuf, "r0": GUARD_ROWS}


def run_batch(c, d, nseg=None, variant=None):
    from yume_amd import ops as yops
    yops.attn_fwd_batch(d["q"], d["k"], d["vt"], d["o"], c.nseg if nseg is None else nseg, c.Lq, c.q_pitch, c.Lk, c.k_pitch, c.H,
                        accumulate=c.acc, variant=c.variant if variant is None else variant, q_prescaled=True, kv_padded=True)
    return d


def segment_views(c, d, s):
    """segment s as a problem of its own: (q, k, vt, o) views for ops.attn_fwd"""
    Lp = _ceil(c.Lk, KT)
    return (d["q"][s * c.q_pitch:s * c.q_pitch + c.Lq], d["k"][s * c.k_pitch:s * c.k_pitch + c.Lk],
            d["vt"][:, s * c.k_pitch:s * c.k_pitch + Lp], d["o"][s * c.q_pitch:s * c.q_pitch + c.Lq])


def run_single(c, d, s, variant=8):
    from yume_amd import ops as yops
    q, k, vt, o = segment_views(c, d, s)
    yops.attn_fwd(q, k, vt, o, c.Lq, c.Lk, c.H, accumulate=c.acc, variant=variant, q_prescaled=True, kv_padded=True)


def results(c, d):
    """per-segment results [Lq, H, 128] fp64"""
    return [d["o"][s * c.q_pitch:s * c.q_pitch + c.Lq].double().view(c.Lq, c.H, D) for s in range(c.nseg)]


def untouched(c, d):
    """everything of obuf (where it was initialised) that no segment owns: guard rows, guard columns, pitch gaps"""
    obuf, HC = d["obuf"], c.H * D
    if c.form == "far":
        parts = []
        for s in range(c.nseg):
            a = d["r0"] + s * c.q_pitch
            parts += [obuf[a - GUARD_ROWS:a].reshape(-1), obuf[a + c.Lq:a + c.Lq + GUARD_ROWS].reshape(-1),
                      obuf[a:a + c.Lq, HC:HC + GUARD_COLS].reshape(-1)]
        return torch.cat(parts)
    mask = torch.ones_like(obuf, dtype=torch.bool)
    for s in range(c.nseg):
        a = d["r0"] + s * c.q_pitch
        mask[a:a + c.Lq, :HC] = False
    return obuf[mask]


def main(argv):
    if argv != ["--routes"]:
        sys.exit(__doc__)
    from yume_amd import ops as yops
    yops.ensure_counters(torch.device("cuda", torch.cuda.current_device()))
    for c in TABLE:
        ops = ac.make_case(as_case(c, "random"))
        d = device_operands(c, ops)
        torch.cuda.synchronize()
        sys.stderr.write(f"CASE {c.name}\n")
        sys.stderr.flush()
        run_batch(c, d)
        if c.route == "batch_v8":
            for s in range(c.nseg):
                run_single(c, d, s)
        torch.cuda.synchronize()
        del d


if __name__ == "__main__":
    main(sys.argv[1:])
