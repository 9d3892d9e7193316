"""tests/gemm_sk_plan.py mirrors the split-K plan of yume_amd/csrc/gemm_w4.hpp for the GPU cases of tests/test_gemm_splitk_tail_gpu.py.
Here (no GPU) its constants are held to the header's and its case list to what the issue of round 8 set out to reach: a change to the
plan's constants fails on the CPU instead of silently moving the GPU cases off the branches they were chosen for."""
import os
import re

import gemm_sk_plan as skp
from conftest import ROOT

HPP = os.path.join(ROOT, "yume_amd", "csrc", "gemm_w4.hpp")


def _const(txt, name):
    m = re.search(r"constexpr\s+(?:int|unsigned)\s+" + name + r"\s*=\s*([^;]+);", txt)
    assert m, f"{name} is no longer a constexpr of gemm_w4.hpp"
    expr = m.group(1).strip()
    assert re.fullmatch(r"[0-9A-Za-z_ *+()<]+", expr), expr
    expr = re.sub(r"\b(\d+)u\b", r"\1", expr)
    return int(eval(expr, {"__builtins__": {}}, {"NTHR_W4": _const(txt, "NTHR_W4")} if "NTHR_W4" in expr else {}))


def test_mirror_constants_are_the_headers():
    txt = open(HPP).read()
    assert _const(txt, "SK_MIN_KT") == skp.SK_MIN_KT
    assert _const(txt, "SK_MAX_SLOTS") == skp.SK_MAX_SLOTS
    assert _const(txt, "SK_SLOT_BYTES") == skp.SK_SLOT_BYTES
    assert _const(txt, "SK_FLAG_STRIDE") == skp.SK_FLAG_STRIDE
    m = re.search(r'getenv\("YUME_GEMM_SK_MIN_NK"\);\s*return\s+v\s*\?\s*atoi\(v\)\s*:\s*(\d+)\s*;', txt)
    assert m and int(m.group(1)) == skp.SK_MIN_NK
    m = re.search(r"sk_workspace_bytes\(int slots\)\s*\{\s*return\s*\(int64_t\)slots \* \(SK_SLOT_BYTES \+ SK_FLAG_STRIDE\) \+ 64;", txt)
    assert m, "the layout of the scratch (slots, then flags, then the error word's line) changed"
    core = open(os.path.join(ROOT, "yume_amd", "csrc", "gemm_core.hpp")).read()
    m = re.search(r'getenv\("YUME_GEMM_GROUPM"\);\s*const int g = v \? atoi\(v\) : (\d+);', core)
    assert m and int(m.group(1)) == skp.GROUP_M


def test_workspace_bytes_through_the_library():
    from yume_amd import _lib
    n = int(_lib.load().yume_gemm_workspace_bytes())
    assert n == 256 * (skp.SK_SLOT_BYTES + skp.SK_FLAG_STRIDE) + 64 == skp.workspace_bytes()
    assert skp.FLAGS_OFFSET + 256 * skp.SK_FLAG_STRIDE == n - 64          # the error word sits behind the last flag's line


def test_case_list_reaches_both_branches_and_every_refusal_at_256_cus():
    plans = skp.check_coverage_at_256()
    # the two SPLITT shapes: the cut tiles hold a complete last group of the grouped order, so they lie on both sides of n_split = 1024
    for name, M, N, K in skp.ACCEPTED:
        if name in ("q2_ragged", "s3_ragged"):
            p = plans[name]
            assert p.R >= skp.GROUP_M * skp.tiles(M, N)[1]
            n0s = {n0 for _, n0 in skp.tail_tiles(M, N, p)}
            assert min(n0s) < 1024 <= max(n0s)
            assert M % 256 and N % 256


def test_plan_is_a_partition_of_k_for_other_cu_counts():
    """values only: whatever the CU count, an accepted plan's slices cover the K tiles once, each at least SK_MIN_KT long, within the slots"""
    for ncu in (64, 104, 128, 192, 224, 256):
        for name, M, N, K in skp.ACCEPTED + [c[:4] for c in skp.REFUSED]:
            p, why = skp.plan(M, N, K, ncu)
            if p is None:
                assert why
                continue
            assert p.lh + (p.s - 2) * p.lt + p.last == K // skp.BK
            assert min(p.lh, p.lt, p.last) >= skp.SK_MIN_KT and p.slots <= skp.SK_MAX_SLOTS and p.nwg <= ncu
            assert 0 < p.R < ncu and p.T % ncu == p.R
