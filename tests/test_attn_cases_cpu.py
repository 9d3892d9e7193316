"""Host proof of tests/attn_cases.py at a shrunken copy of every row of its table (fewer heads and queries, the same key structure): the
chunked fp64 reference against a plain torch.softmax over the explicit keys, the per-element bound against the host emulation of the
kernels' arithmetic (zero elements outside) and against ten injected faults (each flagged on every row it applies to), and the plan of
every v7 / v8 row against attn_plan::search, compiled from yume_amd/csrc/attn_plan.hpp into a small host program."""
import math
import os
import shutil
import subprocess

import pytest
import torch

import attn_cases as ac

SMALL = [ac.shrink(c) for c in ac.CASES]
IDS = [c.name for c in SMALL]


@pytest.fixture(scope="module")
def refs():
    """operands and references of every shrunken row, computed once and left unchanged"""
    return {c.name: (ops, ac.reference(c, ops)) for c in SMALL for ops in [ac.make_case(c)]}


def plain_softmax(sg, scale_log2):
    """fp64 softmax over the EXPLICIT keys (the weighted last key expanded into its copies), whole score matrix at once"""
    q, k, v = (t.double().transpose(0, 1) for t in (sg["q"], sg["k"], sg["v"]))        # [H, L, 128]
    n, w = k.shape[1] - 1, int(sg["w"])
    ke = torch.cat([k[:, :n], k[:, n:].expand(-1, w, -1)], dim=1)
    ve = torch.cat([v[:, :n], v[:, n:].expand(-1, w, -1)], dim=1)
    a = torch.softmax(q @ ke.transpose(1, 2) * (scale_log2 * math.log(2.0)), dim=-1)
    # A and Q of the folded key: its copies carry w a each
    a = torch.cat([a[:, :, :n], a[:, :, n:].sum(dim=-1, keepdim=True)], dim=-1)
    return {"ref": (a @ v).transpose(0, 1), "A": (a @ v.abs()).transpose(0, 1), "Q": ((a * a) @ (v * v)).transpose(0, 1)}


@pytest.mark.parametrize("c", SMALL, ids=IDS)
def test_the_chunked_reference_is_torchs_softmax_in_fp64(c, refs):
    ops, rs = refs[c.name]
    chunked = ac.reference(c, ops, chunk_bytes=8 * 37 * max(lk for lk, _ in ac.segments(c)))       # 37 queries per chunk: ragged chunks
    for sg, r, rc in zip(ops["segs"], rs, chunked):
        t = plain_softmax(sg, ops["scale_log2"])
        assert r["ref"].dtype == torch.float64 and r["ref"].shape == (c.Lq, c.H, ac.D)
        for key in ("ref", "A", "Q"):
            assert (r[key] - t[key]).abs().max().item() <= 1e-12, key
            assert (rc[key] - t[key]).abs().max().item() <= 1e-12, key


@pytest.mark.parametrize("c", SMALL, ids=IDS)
def test_the_emulation_of_a_correct_kernel_is_inside_the_bound_at_every_element(c, refs):
    ops, rs = refs[c.name]
    worst, outside = 0.0, 0
    for got, r in zip(ac.emulate(c, ops), rs):
        ratio = (got - (r["ref"] + r["base"])).abs() / ac.bound(r)
        worst, outside = max(worst, ratio.max().item()), outside + int((ratio > 1).sum())
    print(f"{c.name}: worst error / bound {worst:.3f}, {outside} elements outside")
    assert outside == 0, worst
    assert worst <= 0.95, worst


@pytest.mark.parametrize("fault", ac.FAULTS)
def test_the_bound_flags_the_injected_fault_on_every_row_it_applies_to(fault, refs):
    missed, report = [], []
    for c in SMALL:
        if not ac.fault_applies(c, fault):
            continue
        ops, rs = refs[c.name]
        n = sum(int(((got - (r["ref"] + r["base"])).abs() > ac.bound(r)).sum()) for got, r in zip(ac.emulate(c, ops, fault), rs))
        report.append(f"{c.name} {n}")
        if n == 0:
            missed.append(c.name)
    print(f"{fault}: elements outside the bound per row: " + ", ".join(report))
    assert report, "the fault applies to no row"
    assert not missed, (fault, missed)


def test_the_table_meets_the_abi_names_every_route_and_stays_small():
    names = [c.name for c in ac.CASES]
    assert len(set(names)) == len(names)
    assert {c.route for c in ac.CASES} == set(ac.ROUTES)
    for c in ac.CASES:
        work = sum(c.Lq * lk * c.H for lk, _ in ac.segments(c))
        assert work <= ac.MAX_WORK, c.name
        assert c.pattern in ("random", "probe", "levels", "halves", "peak", "stairs") and c.form in ("tight", "engine_self", "engine_cross"), c.name
        assert (c.plan is not None) == (c.route in ("v7", "v8")), c.name
        assert all(1.0 <= w <= 2 ** 20 for _, w in ac.segments(c)), c.name
        if c.pattern in ("levels", "halves"):
            assert c.prescaled and c.plan[1] >= 2, c.name
            lo, _ = ac.split_rows(c)
            values = ac.LEVELS if c.pattern == "levels" else ac.HALVES
            assert lo * c.H >= len(values) and (c.Lq - lo) * c.H >= len(values), c.name      # every value in whole blocks AND in the split tail
    assert ac.route_of("[attn_fwd] v8 tail_qb=32 splits=2 nwg=256 Lq=8442 Lk=1030 H=1 ldq=256") == ("v8", (32, 2))
    assert ac.route_of("[attn_fwd] v2w Lq=301 Lk=78 H=3 last_w=435") == ("v2w", None)
    assert ac.route_of("[attn_fwd_seg] seg_short nseg=2 Lq_seg=130 seg_pitch=192 H=3 Lk=78,5") == ("seg_short", None)
    # the probe walk starts with the weighted key and its neighbour, and reaches the first keys and the tile edges
    walk = ac.probe_walk(301, 257).tolist()
    assert walk[:2] == [256, 255] and {0, 65, 62, 63, 64, 66, 126, 130, 190, 194}.issubset(set(walk[:200]))


PLAN_MAIN = r"""
#include "attn_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char** argv) {
    for (int i = 1; i + 3 < argc; i += 4) {
        const attn_plan::Model m = (attn_plan::Model)atoi(argv[i]);
        const long long Lq = atoll(argv[i + 1]), Lk = atoll(argv[i + 2]), H = atoll(argv[i + 3]);
        const attn_plan::Plan a = attn_plan::search(attn_plan::MODELS[m], Lq, Lk, H), b = attn_plan::plan(m, Lq, Lk, H);
        printf("%d %lld %d %lld %d\n", attn_plan::applies(m, Lq, Lk) ? 1 : 0, (long long)a.tail_qb, a.splits, (long long)b.tail_qb, b.splits);
    }
    return 0;
}
"""


def test_every_v7_and_v8_row_names_the_plan_attn_plan_search_gives(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "plan_main.cpp", tmp_path / "plan_main"
    src.write_text(PLAN_MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ac.ROOT, "yume_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    rows = [c for c in ac.CASES if c.plan is not None]
    args = [str(x) for c in rows for x in (0 if c.route == "v7" else 1, c.Lq, c.Lk, c.H)]
    out = subprocess.run([str(exe)] + args, check=True, stdout=subprocess.PIPE, text=True, timeout=60).stdout.split("\n")
    planned = set()
    for c, line in zip(rows, out):
        applies, tq, sp, tq2, sp2 = (int(x) for x in line.split())
        assert applies == 1 and (tq, sp) == (tq2, sp2), c.name
        nqb = (c.Lq + ac.QBLOCK - 1) // ac.QBLOCK
        # variant 7 and a call without the scratch run whole blocks whatever the model plans
        want = (tq, sp) if (c.variant in (0, 8) and c.workspace) else (nqb, 1)
        assert c.plan == want, (c.name, c.plan, want)
        planned.add((c.route, c.plan[1], c.plan[0] > 0))
    # every splits value either model plans, each beside whole blocks (tail_qb > 0)
    assert {(r, s, True) for r in ("v7", "v8") for s in (1, 2, 3, 4)} <= planned
