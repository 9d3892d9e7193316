"""A pure-Python mirror of the host side of the GEMM's split-K tail (yume_amd/csrc/gemm_w4.hpp: w4_sk_plan, w4_applies; gemm_core.hpp:
use_256, tile_origin), for the tests to say what a shape is EXPECTED to do before the kernel is asked. tests/test_gemm_sk_plan.py holds
the constants below to the header's, so a change to the plan fails there, on the CPU, instead of silently detuning the GPU cases.

Vocabulary: T tiles of 256 x 256; R = T mod CUs tiles are left over after whole rounds; the plan cuts each of them into s slices along K
(K tiles of 64): slice 0 (the head, lh K tiles) finishes the tile, every other slice (a tail, lt K tiles; the last one takes what is
left) publishes a partial into scratch slot (j - 1) * R + t; a tail workgroup takes q slices one after the other."""
from collections import namedtuple

BK = 64
SK_MIN_KT = 4
SK_MAX_SLOTS = 256
SK_SLOT_BYTES = 64 * 256 * 16
SK_FLAG_STRIDE = 64
SK_MIN_NK = 96              # the default of YUME_GEMM_SK_MIN_NK
GROUP_M = 8                 # the default of YUME_GEMM_GROUPM
EPI_BF16, EPI_BF16_GELU, EPI_F32, EPI_RESID, EPI_BF16_SPLITT, EPI_BF16_GELU_ERF = 0, 1, 2, 3, 4, 5

Plan = namedtuple("Plan", "T R s q lh lt last slots nwg branch")


def workspace_bytes():
    return SK_MAX_SLOTS * (SK_SLOT_BYTES + SK_FLAG_STRIDE) + 64


FLAGS_OFFSET = SK_MAX_SLOTS * SK_SLOT_BYTES


def tiles(M, N):
    return (M + 255) // 256, (N + 255) // 256


def use_256(M, N):
    """the automatic variant's choice of the 256 x 256 tiling (worth = 1.25)"""
    tm, tn = tiles(M, N)
    if tm * tn < 192:
        return False
    t128 = ((M + 127) // 128) * ((N + 127) // 128)
    return tm * tn * 4.0 / 1.25 <= t128


def w4_applies(K, lda, ldw):
    return K >= 3 * BK and 255 * lda * 2 + 128 < (1 << 32) and 255 * ldw * 2 + 128 < (1 << 32)


def plan(M, N, K, ncu):
    """-> (Plan, None) where the tail is cut along K, else (None, reason): 'T<CUs', 'R=0', 'nk', 'lt', 'slots', 'nwg', 'ncu'"""
    if ncu < 64 or ncu > SK_MAX_SLOTS or ncu % 8:
        return None, "ncu"
    tm, tn = tiles(M, N)
    T, nk = tm * tn, K // BK
    R = T % ncu
    if T < ncu:
        return None, "T<CUs"
    if R == 0:
        return None, "R=0"
    if nk < SK_MIN_NK:
        return None, "nk"
    if 2 * R > ncu:
        branch, s = "A", 2
        q = (R + (ncu - R) - 1) // (ncu - R)
        lt = nk // (q + 1)
        lh = nk - lt
    else:
        branch, s = "B", min(ncu // R, nk // SK_MIN_KT)
        q = 1
        lt = lh = nk // s
    if s < 2 or lt < SK_MIN_KT or lh < SK_MIN_KT:
        return None, "lt"
    if (s - 1) * R > SK_MAX_SLOTS:
        return None, "slots"
    nwg = R + ((s - 1) * R + q - 1) // q
    if nwg > ncu:
        return None, "nwg"
    return Plan(T, R, s, q, lh, lt, nk - lh - (s - 2) * lt, (s - 1) * R, nwg, branch), None


def tile_origin(M, N, t, group_m=GROUP_M):
    """(m0, n0) of tile t of the grouped order: groups of group_m tile rows, walked row-fastest"""
    tm, tn = tiles(M, N)
    width = group_m * tn
    first_m = (t // width) * group_m
    gsz = min(tm - first_m, group_m)
    return (first_m + (t % width) % gsz) * 256, ((t % width) // gsz) * 256


def tail_tiles(M, N, p):
    """origins of the R tiles the plan cuts: the last R of the order"""
    return [tile_origin(M, N, t) for t in range(p.T - p.R, p.T)]


# The cases: (name, M, N, K). At 256 CUs they are, in this order, what the table in profiles/r8_gemm_splitk_tail_parity.md lists.
ACCEPTED = [
    ("5b_ffn2", 9460, 3072, 14336),             # A: R 188, q 3
    ("5b_ffn2_L12545", 12545, 3072, 14336),     # B: R 88, s 2
    ("14b_ffn2", 27810, 5120, 13824),           # A: R 132 (2 R = 264 > 256), q 2
    ("q2_ragged", 12467, 2040, 6144),           # A: q 2, ragged M and N
    ("q23_lt4_full", 42747, 768, 6144),         # A: q 23, lt = SK_MIN_KT, 256 workgroups
    ("s2_halves", 11005, 2048, 6144),           # B: s 2
    ("s3_ragged", 10366, 1988, 6400),           # B: s 3, nk = 100 not divisible, ragged M and N
    ("s4_full", 10240, 2048, 6144),             # B: s 4, 256 workgroups
    ("s10", 8960, 2048, 7168),                  # B: s 10, last slice 13
    ("r1_s24", 65783, 256, 6144),               # B: R 1, s clipped to nk / 4
    ("r5_s24", 66816, 256, 6144),               # B: R 5, s 24
]
REFUSED = [
    ("refused_lt", 64251, 512, 6144, "lt"),
    ("refused_nk", 9460, 3072, 6080, "nk"),
    ("refused_T", 65280, 256, 6144, "T<CUs"),
    ("refused_R0", 8192, 2048, 6144, "R=0"),
]

# what the plan gives at 256 CUs: name -> (T, R, s, q, lh, lt, last, slots)
AT_256 = {
    "5b_ffn2": (444, 188, 2, 3, 168, 56, 56, 188),
    "5b_ffn2_L12545": (600, 88, 2, 1, 112, 112, 112, 88),
    "14b_ffn2": (2180, 132, 2, 2, 144, 72, 72, 132),
    "q2_ragged": (392, 136, 2, 2, 64, 32, 32, 136),
    "q23_lt4_full": (501, 245, 2, 23, 92, 4, 4, 245),
    "s2_halves": (344, 88, 2, 1, 48, 48, 48, 88),
    "s3_ragged": (328, 72, 3, 1, 33, 33, 34, 144),
    "s4_full": (320, 64, 4, 1, 24, 24, 24, 192),
    "s10": (280, 24, 10, 1, 11, 11, 13, 216),
    "r1_s24": (257, 1, 24, 1, 4, 4, 4, 23),
    "r5_s24": (261, 5, 24, 1, 4, 4, 4, 115),
}


def check_coverage_at_256():
    """the case list reaches both branches of the plan, their edges and every refusal (asserted where the device has 256 CUs)"""
    plans = {}
    for name, M, N, K in ACCEPTED:
        p, why = plan(M, N, K, 256)
        assert p is not None, (name, why)
        assert use_256(M, N) and w4_applies(K, K, K), name
        assert tuple(p[:8]) == AT_256[name], (name, tuple(p[:8]), AT_256[name])
        plans[name] = p
    a = [p for p in plans.values() if p.branch == "A"]
    b = [p for p in plans.values() if p.branch == "B"]
    assert {2, 3, 23} <= {p.q for p in a}
    assert any(p.lt == SK_MIN_KT and p.nwg == 256 for p in a)
    assert {2, 3, 4, 10, 24} <= {p.s for p in b}
    assert any(p.last != p.lt for p in b), "no case whose K tiles do not divide by s"
    assert any(p.R == 1 for p in b)
    assert any(p.nwg == 256 for p in b)
    reasons = set()
    for name, M, N, K, why in REFUSED:
        p, got = plan(M, N, K, 256)
        assert p is None and got == why, (name, p, got)
        assert use_256(M, N) and w4_applies(K, K, K), name
        reasons.add(got)
    assert reasons == {"lt", "nk", "T<CUs", "R=0"}
    return plans
