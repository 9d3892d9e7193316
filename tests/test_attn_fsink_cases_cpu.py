"""Host proof of tests/attn_fsink_cases.py: attn_fsink_plan.hpp (compiled into a small host program) and its Python mirror against a brute-force
walk over every (row, key) pair of every case and of its partition at several q_pos0 and Lk; the tile lists held to "a tile is listed
exactly when some row of the run sees one of its keys, once, ascending"; the fp64 reference against a dense-mask softmax; the host
emulation of attn_fsink_kernel inside `bound()` at every element of every case, every injected fault flagged on every row its rule names;
the engine's span list with the sequence-parallel pad rows as one more block and a sink. (The C-ABI refusals: tests/test_attn_fsink_cabi.py.)"""
import os
import shutil
import subprocess

import pytest
import torch

import attn_fsink_cases as sc
from conftest import ROOT

ALL = sc.CASES + sc.NORMALISED + sc.FBAND_EQUIV


@pytest.fixture(scope="module")
def refs():
    """operands and references of every row the faults are tried on, computed once and left unchanged"""
    return {c.name: (ops, sc.reference_fsink(c, ops)) for c in sc.FAULT_CASES for ops in [sc.make_fsink_case(c)]}


def brute_blocks(spans):
    """the block of every position, by laying the blocks out one after the other"""
    out, b = [], 0
    for rows, nblk in spans:
        for _ in range(nblk):
            out += [b] * rows
            b += 1
    return torch.tensor(out)


def brute_visible(Lq, Lk, spans, q_pos0, back, ahead, sink):
    """(through the window, through the sink): bool [Lq, Lk] each, pair by pair from the laid-out blocks"""
    blk = brute_blocks(spans)
    bi, bj = blk[q_pos0:q_pos0 + Lq].view(Lq, 1), blk[:Lk].view(1, Lk)
    band = torch.ones(Lq, Lk, dtype=torch.bool)
    if back >= 0:
        band &= bj >= bi - back
    if ahead >= 0:
        band &= bj <= bi + ahead
    return band, (bj < sink).expand(Lq, Lk)


# ---- the rule: header == mirror == brute force -----------------------------------------------------------------------------------------------
PLAN_MAIN = r"""
#include "attn_fsink_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
// argv: groups of (Lq Lk q_pos0 back ahead sink nspan rows_0 nblk_0 ...). Per group `S <send> <hides_nothing> <adds_nothing>`, then per
// 128-row block `B <n_sink> <b_lo> <b_hi> <count>` and `L <the tiles by first_tile / next_tile>`, per 32-row wave of it `W <n_sink> <b_lo>
// <b_hi>` and per tile of the BLOCK's list `I <q_first> <t> <in the wave's list> <interior>`, per row `R <i> <first> <last> <count>` from visible().
int main(int argc, char** argv) {
    using namespace attn_fsink_plan;
    int a = 1;
    while (a + 6 < argc) {
        const long long Lq = atoll(argv[a]), Lk = atoll(argv[a + 1]);
        Plan w{};
        w.q_pos0 = atoll(argv[a + 2]); w.back = atoll(argv[a + 3]); w.ahead = atoll(argv[a + 4]);
        const long long sink = atoll(argv[a + 5]);
        w.nspan = atoi(argv[a + 6]);
        a += 7;
        for (int g = 0; g < w.nspan; ++g, a += 2) { w.rows[g] = atoi(argv[a]); w.nblk[g] = atoi(argv[a + 1]); }
        printf("S %lld %d %d\n", (long long)send(Lk, w, sink), hides_nothing(Lq, Lk, w, sink) ? 1 : 0, adds_nothing(Lq, Lk, w, sink) ? 1 : 0);
        for (long long q = 0; q < Lq; q += attn_fband_plan::QBLOCK) {
            const long long q1 = (q + attn_fband_plan::QBLOCK < Lq ? q + attn_fband_plan::QBLOCK : Lq) - 1;
            const TileList l = tile_list(q, q1, Lk, w, sink);
            printf("B %lld %lld %lld %lld\nL", (long long)l.n_sink, (long long)l.b_lo, (long long)l.b_hi, (long long)tile_count(l));
            for (long long t = first_tile(l); t <= l.b_hi; t = next_tile(t, l)) printf(" %lld", t);
            printf("\n");
            for (long long wq = q; wq <= q1; wq += attn_fband_plan::QWAVE) {
                const long long wq1 = (wq + attn_fband_plan::QWAVE - 1 < q1 ? wq + attn_fband_plan::QWAVE - 1 : q1);
                const TileList wl = tile_list(wq, wq1, Lk, w, sink);
                printf("W %lld %lld %lld\n", (long long)wl.n_sink, (long long)wl.b_lo, (long long)wl.b_hi);
                for (long long t = first_tile(l); t <= l.b_hi; t = next_tile(t, l))
                    printf("I %lld %lld %d %d\n", wq, t, in_list(t, wl) ? 1 : 0, tile_is_interior(t, wq, wq1, Lk, w, sink) ? 1 : 0);
            }
        }
        for (long long i = 0; i < Lq; ++i) {
            long long first = -1, last = -1, n = 0;
            for (long long j = -2; j < Lk + 2; ++j)
                if (visible(i, j, Lk, w, sink)) { if (first < 0) first = j; last = j; ++n; }
            printf("R %lld %lld %lld %lld\n", i, first, last, n);
        }
    }
    return 0;
}
"""


def _calls():
    """(Lq, Lk, spans, q_pos0, back, ahead, sink): every row of the tables as it is, and every (partition, window, sink) of them at q_pos0 in
    {0, 1, 64, 127, N - Lq} with up to 200 rows, at Lk = N, a little short, inside the sink and right behind it"""
    out, seen = [], set()
    for c in ALL:
        out.append((c.Lq, c.Lk) + sc.rule(c))
    for c in ALL:
        N = sc.total_rows(c.spans)
        key = (tuple(c.spans), c.back, c.ahead, c.sink)
        if key in seen or N > 700:
            continue
        seen.add(key)
        start = sc.send(N, c.spans, c.sink)
        for q_pos0 in (0, 1, 64, 127, max(N - 200, 0)):
            Lq = min(200, N - q_pos0)
            for Lk in {N, N - 37, max(start - 3, 1), min(start + 5, N)}:
                out.append((Lq, Lk, tuple(c.spans), q_pos0, c.back, c.ahead, c.sink))
    return sorted(set(out))


def test_attn_fsink_plan_hpp_and_its_mirror_agree_with_a_brute_force_walk(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "fsink_plan_main.cpp", tmp_path / "fsink_plan_main"
    src.write_text(PLAN_MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "yume_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    calls = _calls()
    assert len(calls) >= 150
    seen = {"hides_nothing": 0, "adds_nothing": 0, "kernel": 0, "two_intervals": 0, "jump": 0, "one_run": 0, "interior_sink": 0, "interior_band": 0,
            "edge": 0, "wave_skips": 0, "sink_cut": 0}
    for n0 in range(0, len(calls), 20):
        chunk = calls[n0:n0 + 20]
        argv = [str(x) for Lq, Lk, spans, q_pos0, back, ahead, sink in chunk
                for x in (Lq, Lk, q_pos0, back, ahead, sink, len(spans)) + tuple(v for s in spans for v in s)]
        lines = iter(subprocess.run([str(exe)] + argv, check=True, stdout=subprocess.PIPE, text=True, timeout=300).stdout.split("\n"))
        for Lq, Lk, spans, q_pos0, back, ahead, sink in chunk:
            w = (spans, q_pos0, back, ahead, sink)
            ctx = (Lq, Lk) + w
            band, through_sink = brute_visible(Lq, Lk, *w)
            vis = band | through_sink
            assert torch.equal(vis, sc.visible(Lq, Lk, *w)), ctx
            se = int(through_sink[0].sum())                              # the sink's keys are a prefix: their count is its end
            assert bool(through_sink[0, :se].all()) and se == sc.send(Lk, spans, sink), ctx
            seen["sink_cut"] += se == Lk and sink < sc.total_blocks(spans)
            nothing_hidden, nothing_added = bool(vis.all()), bool((band | ~through_sink).all())
            seen["hides_nothing" if nothing_hidden else "adds_nothing" if nothing_added else "kernel"] += 1
            assert next(lines) == f"S {se} {int(nothing_hidden)} {int(nothing_added)}", ctx
            assert sc.hides_nothing(Lq, Lk, *w) == nothing_hidden and sc.adds_nothing(Lq, Lk, *w) == nothing_added, ctx

            def tiles_seen(r0, r1):
                """the tiles of which some row of r0 ... r1 sees a key, ascending"""
                cols = vis[r0:r1 + 1].any(dim=0).nonzero().view(-1)
                return sorted(set((cols // sc.KT).tolist()))
            for q in range(0, Lq, sc.QB):
                q1 = min(q + sc.QB, Lq) - 1
                want = tiles_seen(q, q1)
                tl = sc.tile_list(q, q1, Lk, *w)
                assert sc.tiles_of(tl) == want, ctx + (q,)               # each once, ascending
                assert next(lines) == f"B {tl[0]} {tl[1]} {tl[2]} {len(want)}", ctx + (q,)
                assert next(lines) == "L" + "".join(f" {t}" for t in want), ctx + (q,)
                walk, t = [], (0 if tl[0] > 0 else tl[1])
                while t <= tl[2]:
                    walk.append(t)
                    t = sc.next_tile(t, tl)
                assert walk == want, ctx + (q,)
                seen["jump" if any(b - a > 1 for a, b in zip(want, want[1:])) else "one_run"] += 1
                for wq in range(q, q1 + 1, sc.QW):
                    wq1 = min(wq + sc.QW - 1, q1)
                    wl = sc.tile_list(wq, wq1, Lk, *w)
                    wave_tiles = tiles_seen(wq, wq1)
                    assert sc.tiles_of(wl) == wave_tiles and set(wave_tiles) <= set(want), ctx + (wq,)
                    assert next(lines) == f"W {wl[0]} {wl[1]} {wl[2]}", ctx + (wq,)
                    seen["wave_skips"] += len(wave_tiles) < len(want)
                    for t in want:
                        cols = slice(t * sc.KT, t * sc.KT + sc.KT)
                        whole = t * sc.KT + sc.KT <= Lk
                        by_sink = whole and bool(through_sink[wq:wq1 + 1, cols].all())
                        by_band = whole and bool(band[wq:wq1 + 1, cols].all())
                        interior = by_sink or by_band
                        seen["interior_sink" if by_sink else "interior_band" if by_band else "edge"] += 1
                        assert next(lines) == f"I {wq} {t} {int(t in wave_tiles)} {int(interior)}", ctx + (wq, t)
                        assert sc.tile_is_interior(t, wq, wq1, Lk, *w) == interior, ctx + (wq, t)
                        assert not interior or bool(vis[wq:wq1 + 1, cols].all()), ctx + (wq, t)
            for i in range(Lq):
                js = vis[i].nonzero().view(-1)
                assert next(lines) == (f"R {i} {int(js[0])} {int(js[-1])} {len(js)}" if len(js) else f"R {i} -1 -1 0"), ctx + (i,)
                seen["two_intervals"] += len(js) > 0 and int(js[-1]) - int(js[0]) + 1 > len(js)
    print(f"{len(calls)} calls: {seen}")
    assert seen["hides_nothing"] >= 5 and seen["adds_nothing"] >= 5 and seen["kernel"] >= 80 and seen["two_intervals"] >= 1000
    assert seen["jump"] >= 50 and seen["one_run"] >= 50 and min(seen["interior_sink"], seen["interior_band"], seen["edge"], seen["wave_skips"]) >= 50
    assert seen["sink_cut"] >= 5


# ---- the reference and the emulation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", sc.FAULT_CASES, ids=[c.name for c in sc.FAULT_CASES])
def test_the_reference_is_a_dense_mask_softmax_in_fp64_and_the_clean_emulation_is_inside_the_bound(c, refs):
    ops, r = refs[c.name]
    sg = ops["segs"][0]
    q, k, v = (t.double().transpose(0, 1) for t in (sg["q"], sg["k"], sg["v"]))          # [H, L, 128]
    band, through_sink = brute_visible(c.Lq, c.Lk, *sc.rule(c))
    mask = band | through_sink
    assert bool(mask.any(dim=1).all())                                                  # with a sink no row is empty
    x = q @ k.transpose(1, 2) * (ops["scale_log2"] * 0.6931471805599453)
    a = torch.softmax(x.masked_fill(~mask, -float("inf")), dim=-1)
    want = {"ref": a @ v, "A": a @ v.abs(), "Q": (a * a) @ (v * v)}
    for key in ("ref", "A", "Q"):
        assert r[key].dtype == torch.float64 and r[key].shape == (c.Lq, c.H, sc.D)
        assert (r[key] - want[key].transpose(0, 1)).abs().max().item() <= 1e-12, key
    got = sc.emulate_fsink(c, ops)
    bnd = sc.bound(r)
    err = (got - (r["ref"] + r["base"])).abs()
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.zeros_like(got))
    print(f"{c.name}: worst error / bound {ratio.max().item():.3f}, {int((err > bnd).sum())} elements outside")
    assert int((err > bnd).sum()) == 0 and ratio.max().item() <= 0.95


@pytest.mark.parametrize("fault", sc.FAULTS)
def test_the_bound_flags_the_injected_fault_on_every_row_its_rule_names(fault, refs):
    named, flagged, report = [], [], []
    for c in sc.FAULT_CASES:
        if not sc.fault_applies(fault, c):
            continue
        named.append(c.name)
        ops, r = refs[c.name]
        n = int(((sc.emulate_fsink(c, ops, fault) - (r["ref"] + r["base"])).abs() > sc.bound(r)).sum())
        report.append(f"{c.name} {n}")
        if n:
            flagged.append(c.name)
    print(f"{fault}: elements outside the bound per named row: " + ", ".join(report))
    assert named and flagged == named, (fault, sorted(set(named) - set(flagged)))


def test_the_tables_reach_what_they_were_built_for():
    sc.check_tables()
    assert len(sc.FAULTS) == 8 and len(sc.CASES) >= 19
    by = {c.name: c for c in sc.CASES}
    for situation in (sc.split_tile_rows, sc.jumps, sc.meetings, sc.sink_ends_in_ragged_last_tile):
        assert any(situation(c) for c in sc.CASES), situation.__name__
    # where every edge is a tile edge the sink has no straddling tile: every sink tile is interior for every wave
    for n in ("aligned_64x6_s1_b0_a0", "aligned_128x3_s1_b0_a0"):
        c = by[n]
        ns = sc.block_lists(c)[0][0]
        assert ns * sc.KT == sc.send(c.Lk, c.spans, c.sink)
        assert all(sc.tile_is_interior(t, w0, w0 + sc.QW - 1, c.Lk, *sc.rule(c)) for w0 in range(0, c.Lq, sc.QW) for t in range(ns))
    # the refusals: fband's list, the sink's range, the variants
    names = [r[0] for r in sc.REFUSALS]
    assert len(set(names)) == len(names) and {"sink_minus_1", "sink_nb_plus_1", "variant_7", "variant_12", "nspan_0", "lk_over_n"} <= set(names)
    assert sc.fband_log("[attn_fwd_fsink] fsink q_pos0=312 back=1 ahead=1 sink=2 sink_rows=12 nspan=5 nblocks=13 tiles_min=5 tiles_max=8 Lq=288 "
                        "Lk=600 H=2") == ("fsink", {"q_pos0": 312, "back": 1, "ahead": 1, "sink": 2, "sink_rows": 12, "nspan": 5, "nblocks": 13,
                                                    "tiles_min": 5, "tiles_max": 8, "Lq": 288, "Lk": 600, "H": 2})


# ---- the engine's arguments, without a GPU -----------------------------------------------------------------------------------------------------
def test_the_engine_hands_the_sink_on_through_frame_args_alone(monkeypatch):
    import __graft_entry__ as g
    g.build()
    from yume_amd.dit import DiTEngine

    class M:
        window_size = (-1, -1)
    e = DiTEngine(M(), "wan23")
    assert e.frame_sink == 0 and e._frame_args(5) == {}
    e.frame_sink = 1
    with pytest.raises(ValueError, match=r"(?s)frame_sink.*frame_window"):
        e._frame_args(0)
    e.frame_window = (1, 0)
    e._spans = [(6, 2), (24, 3)]
    assert e._frame_args(5) == {"frame_window": (1, 0), "spans": [(6, 2), (24, 3)], "q_pos0": 5, "frame_sink": 1}
    e.frame_sink = 0
    assert e._frame_args(5) == {"frame_window": (1, 0), "spans": [(6, 2), (24, 3)], "q_pos0": 5}       # r28's call, key for key
    e.frame_sink = -1
    with pytest.raises(ValueError, match=r"(?s)frame_sink.*frame_window"):
        e._frame_args(0)
    e.frame_sink = 40                                                   # more than the clip has: all of its frames
    assert e._frame_args(0)["frame_sink"] == 5
    # the sequence-parallel pad rows are one more block behind the clip; the sink is still counted in the clip's own frames, the pad rows see
    # the sink (and their own window's keys below Lk), and nobody sees a pad key: they lie behind Lk
    a = e._frame_args(0, 96)
    assert a["spans"] == [(6, 2), (24, 3), (12, 1)] and a["frame_sink"] == 5
    e.frame_sink = 1
    a = e._frame_args(0, 96)
    spans, n_tok = tuple(a["spans"]), 84
    vis = sc.visible(96, n_tok, spans, 0, 1, 0, a["frame_sink"])
    band, through_sink = brute_visible(96, n_tok, spans, 0, 1, 0, 1)
    assert torch.equal(vis, band | through_sink) and vis.shape == (96, n_tok)
    assert bool(vis[:, :6].all()) and vis[84:].sum(dim=1).tolist() == [6 + 24] * 12 and not sc.hides_nothing(96, n_tok, spans, 0, 1, 0, 1)
    assert sc.tile_list(0, 95, n_tok, spans, 0, 1, 0, 1) == (1, 1, 1)
    monkeypatch.setenv("YUME_FRAME_SINK", "2")
    assert DiTEngine(M(), "wan23").frame_sink == 2


def test_the_wrapper_refuses_a_sink_without_a_frame_window():
    import __graft_entry__ as g
    g.build()
    import inspect
    from yume_amd import attention, ops
    t = torch.zeros(8, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match=r"(?s)frame_sink.*frame_window"):
        ops.attn_fwd(t, t, t, t, 8, 8, 1, frame_sink=1)
    with pytest.raises(RuntimeError, match=r"(?s)frame_sink.*frame_window"):
        ops.attn_fwd(t, t, t, t, 8, 8, 1, window=(2, 0), frame_sink=1)
    assert inspect.signature(ops.attn_fwd).parameters["frame_sink"].default == 0
    assert list(inspect.signature(attention.frame_sink_attention).parameters) == ["q", "k", "v", "spans", "frame_window", "sink", "q_lens", "k_lens",
                                                                                  "softmax_scale"]
