"""Host proof of tests/attn_band_cases.py: the fp64 reference against a brute-force dense-mask softmax, attn_band_plan.hpp (compiled into a
small host program) against a brute-force walk over (row, key) pairs for every case and a few hundred seeded triples, the host emulation
of attn_band_kernel inside `bound()` at every element of every shrunken case, and every applicable injected fault flagged on every row it
applies to (the one that is the same function: not flagged)."""
import os
import random
import shutil
import subprocess

import pytest
import torch

import attn_band_cases as bc

SMALL = [bc.shrink(c) for c in bc.CASES]
IDS = [c.name for c in SMALL]


@pytest.fixture(scope="module")
def refs():
    """operands and references of every shrunken row, computed once and left unchanged"""
    return {c.name: (ops, bc.reference_band(c, ops)) for c in SMALL for ops in [bc.make_band_case(c)]}


def brute_visible(c):
    return [[0 <= j < c.Lk and (c.left < 0 or j >= c.q_pos0 + i - c.left) and (c.right < 0 or j <= c.q_pos0 + i + c.right) for j in range(c.Lk)]
            for i in range(c.Lq)]


@pytest.mark.parametrize("c", SMALL, ids=IDS)
def test_the_reference_is_a_dense_mask_softmax_in_fp64(c, refs):
    ops, r = refs[c.name]
    sg = ops["segs"][0]
    q, k, v = (t.double().transpose(0, 1) for t in (sg["q"], sg["k"], sg["v"]))          # [H, L, 128]
    mask = torch.tensor(brute_visible(c))
    assert torch.equal(mask, bc.visible(c.Lq, c.Lk, c.q_pos0, c.left, c.right))
    x = q @ k.transpose(1, 2) * (ops["scale_log2"] * 0.6931471805599453)
    a = torch.softmax(x.masked_fill(~mask, -float("inf")), dim=-1)
    a = torch.where(mask.any(dim=1).view(1, -1, 1), a, torch.zeros_like(a))             # (softmax of an all-hidden row is NaN: the row is 0)
    want = {"ref": a @ v, "A": a @ v.abs(), "Q": (a * a) @ (v * v)}
    for key in ("ref", "A", "Q"):
        assert r[key].dtype == torch.float64 and r[key].shape == (c.Lq, c.H, bc.D)
        assert (r[key] - want[key].transpose(0, 1)).abs().max().item() <= 1e-12, key
    empty = bc.empty_rows(c)
    assert torch.equal(empty, ~mask.any(dim=1))
    for key in ("ref", "A", "Q"):
        assert bool((r[key][empty] == 0).all())


@pytest.mark.parametrize("c", SMALL, ids=IDS)
def test_the_emulation_of_a_correct_kernel_is_inside_the_bound_at_every_element(c, refs):
    ops, r = refs[c.name]
    got = bc.emulate_band(c, ops)
    want = r["ref"] + r["base"]
    over = (got - want).abs() > bc.bound(r)
    ratio = torch.where(bc.bound(r) > 0, (got - want).abs() / bc.bound(r).clamp_min(1e-300), torch.zeros_like(got))
    print(f"{c.name}: worst error / bound {ratio.max().item():.3f}, {int(over.sum())} elements outside")
    assert int(over.sum()) == 0
    assert ratio.max().item() <= 0.95
    empty = bc.empty_rows(c)
    if ops["base"] is None:
        assert bool((got[empty] == 0).all())
    else:
        assert torch.equal(got[empty], ops["base"].double().view(c.Lq, c.H, bc.D)[empty])


@pytest.mark.parametrize("fault", bc.FAULTS)
def test_the_bound_flags_the_injected_fault_on_every_row_it_applies_to(fault, refs):
    missed, flagged, report = [], [], []
    for c in SMALL:
        if not bc.fault_applies(c, fault):
            continue
        ops, r = refs[c.name]
        n = int(((bc.emulate_band(c, ops, fault) - (r["ref"] + r["base"])).abs() > bc.bound(r)).sum())
        report.append(f"{c.name} {n}")
        (flagged if n else missed).append(c.name)
    print(f"{fault}: elements outside the bound per row: " + ", ".join(report))
    assert report, "the fault applies to no row"
    if fault in bc.SAME_FUNCTION:
        assert not flagged, (fault, flagged)
    else:
        assert not missed, (fault, missed)


def test_the_base_over_hidden_keys_at_a_gap_of_exactly_126_is_the_same_function(refs):
    """the figures behind attn_band_cases.RAMP_STEP: on the two rows of the ramp 2 (j % 64) the emulation with the row maximum taken before
    the mask stores what the correct one stores (nothing is flushed at exp2(-126)), so no bound can tell them apart there"""
    for c in SMALL:
        if c.pattern != "ramp":
            continue
        ops, r = refs[c.name]
        good, bad = bc.emulate_band(c, ops), bc.emulate_band(c, ops, "max_over_hidden")
        diff = (good - bad).abs()
        print(f"{c.name}: gap {bc.ramp_gap(c)}; faulty against correct emulation: max |diff| {diff.max().item():.3g}, "
              f"{int((diff > 0).sum())} of {diff.numel()} elements differ, {int(((bad - r['ref']).abs() > bc.bound(r)).sum())} outside the bound")
        assert bc.ramp_gap(c) == 126 and int(((bad - r["ref"]).abs() > bc.bound(r)).sum()) == 0


def test_the_faults_reach_the_rows_the_table_was_built_for():
    # the ramps: 2 (j % 64) reaches a gap of exactly 126 = exp2's last normal result, 4 (j % 64) goes beyond (attn_band_cases.RAMP_STEP)
    assert [(c.name, bc.ramp_gap(c)) for c in bc.CASES if c.pattern in bc.RAMP_STEP] == [("ramp_causal", 126), ("ramp_l5", 126),
                                                                                          ("ramp4_causal", 252), ("ramp4_l5", 252)]
    assert [c.name for c in bc.CASES if bc.fault_applies(c, "max_over_hidden")] == ["ramp4_causal", "ramp4_l5"]
    assert any(bc.fault_applies(c, "top_left_aligned") for c in bc.CASES)
    assert sum(bc.fault_applies(c, "empty_row_copies_v") for c in bc.CASES) >= 3
    names = [c.name for c in bc.CASES + bc.NORMALISED]
    assert len(set(names)) == len(names)
    for c in bc.CASES:
        assert not bc.hides_nothing(c.Lq, c.Lk, c.q_pos0, c.left, c.right), c.name
        assert c.pattern in ("edge_probe", "ramp", "ramp4", "random") and c.form in ("tight", "engine_self", "engine_cross"), c.name
    for c in bc.NORMALISED:
        assert bc.hides_nothing(c.Lq, c.Lk, c.q_pos0, c.left, c.right), c.name
    whole = [c for c in bc.CASES if bc.block_tiles(c)[0] == (0, -1)]
    assert whole, "no case whose first workgroup sees no key"
    assert any(c.acc and bool(bc.empty_rows(c).any()) for c in bc.CASES)
    assert {c.prescaled for c in bc.CASES} == {True, False} and any(c.padded for c in bc.CASES)
    assert bc.band_log("[attn_fwd_band] band q_pos0=-44 left=-1 right=0 tiles_min=0 tiles_max=4 Lq=301 Lk=257 H=3 ldq=384") == \
        ("band", {"q_pos0": -44, "left": -1, "right": 0, "tiles_min": 0, "tiles_max": 4, "Lq": 301, "Lk": 257, "H": 3, "ldq": 384})


PLAN_MAIN = r"""
#include "attn_band_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
// argv: groups of (Lq Lk q_pos0 left right). Per group one line `H <hides_nothing>`, then per 128-row block `B <t_lo> <t_hi>`, per 32-row
// wave and tile of its block's range `I <q_first> <t> <interior>`, per row `R <i> <first visible key> <last visible key> <count>` from visible().
int main(int argc, char** argv) {
    using namespace attn_band_plan;
    for (int a = 1; a + 4 < argc; a += 5) {
        const long long Lq = atoll(argv[a]), Lk = atoll(argv[a + 1]);
        const Window w{atoll(argv[a + 2]), atoll(argv[a + 3]), atoll(argv[a + 4])};
        printf("H %d\n", hides_nothing(Lq, Lk, w) ? 1 : 0);
        for (long long q = 0; q < Lq; q += QBLOCK) {
            const long long q1 = (q + QBLOCK < Lq ? q + QBLOCK : Lq) - 1;
            const TileRange r = tile_range(q, q1, Lk, w);
            printf("B %lld %lld\n", (long long)r.lo, (long long)r.hi);
            for (long long wq = q; wq <= q1; wq += QWAVE) {
                const long long wq1 = (wq + QWAVE - 1 < q1 ? wq + QWAVE - 1 : q1);
                for (long long t = r.lo; t <= r.hi; ++t) printf("I %lld %lld %d\n", wq, t, tile_is_interior(t, wq, wq1, Lk, w) ? 1 : 0);
            }
        }
        for (long long i = 0; i < Lq; ++i) {
            long long first = -1, last = -1, n = 0;
            for (long long j = -2; j < Lk + 2; ++j)
                if (visible(i, j, Lk, w)) { if (first < 0) first = j; last = j; ++n; }
            printf("R %lld %lld %lld %lld\n", i, first, last, n);
        }
    }
    return 0;
}
"""


def _triples():
    rng = random.Random(26)
    out = [(c.Lq, c.Lk, c.q_pos0, c.left, c.right) for c in bc.CASES + bc.NORMALISED]
    for _ in range(300):
        Lq, Lk = rng.choice((1, 31, 64, 129, 200, 257)), rng.choice((1, 63, 64, 65, 130, 300))
        side = lambda: rng.choice((-1, -1, 0, 1, 5, 63, 64, 65, 129, 400))
        out.append((Lq, Lk, rng.choice((0, 0, Lk - Lq, -70, 70, -400, 400, rng.randrange(-200, 200))), side(), side()))
    return out


def test_attn_band_plan_hpp_agrees_with_a_brute_force_walk(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "band_plan_main.cpp", tmp_path / "band_plan_main"
    src.write_text(PLAN_MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(bc.ac.ROOT, "yume_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    triples = _triples()
    hidden_seen = {True: 0, False: 0}
    for n0 in range(0, len(triples), 40):
        chunk = triples[n0:n0 + 40]
        lines = iter(subprocess.run([str(exe)] + [str(x) for t in chunk for x in t], check=True, stdout=subprocess.PIPE, text=True,
                                    timeout=120).stdout.split("\n"))
        for Lq, Lk, q_pos0, left, right in chunk:
            w = (q_pos0, left, right)
            vis = [[(left < 0 or j >= q_pos0 + i - left) and (right < 0 or j <= q_pos0 + i + right) for j in range(Lk)] for i in range(Lq)]
            nothing_hidden = all(all(row) for row in vis)
            hidden_seen[nothing_hidden] += 1
            assert next(lines) == f"H {int(nothing_hidden)}", (Lq, Lk, w)
            assert bc.hides_nothing(Lq, Lk, *w) == nothing_hidden
            for q in range(0, Lq, bc.QB):
                q1 = min(q + bc.QB, Lq) - 1
                keys = [j for i in range(q, q1 + 1) for j in range(Lk) if vis[i][j]]
                want = (min(keys) // bc.KT, max(keys) // bc.KT) if keys else (0, -1)
                assert next(lines) == f"B {want[0]} {want[1]}", (Lq, Lk, w, q)
                assert bc.tile_range(q, q1, Lk, *w) == want
                for wq in range(q, q1 + 1, 32):
                    wq1 = min(wq + 31, q1)
                    for t in range(want[0], want[1] + 1):
                        interior = all(j < Lk and vis[i][j] for i in range(wq, wq1 + 1) for j in range(t * bc.KT, t * bc.KT + bc.KT))
                        assert next(lines) == f"I {wq} {t} {int(interior)}", (Lq, Lk, w, wq, t)
                        assert bc.tile_is_interior(t, wq, wq1, Lk, *w) == interior
            for i in range(Lq):
                js = [j for j in range(Lk) if vis[i][j]]
                assert next(lines) == (f"R {i} {js[0]} {js[-1]} {len(js)}" if js else f"R {i} -1 -1 0"), (Lq, Lk, w, i)
                lo, hi = bc.key_range(i, i, Lk, *w)
                assert (list(range(lo, hi + 1)) if lo <= hi else []) == js
    assert hidden_seen[True] >= 10 and hidden_seen[False] >= 100
