"""Host proof of tests/attn_fprefix_cases.py: attn_fprefix_plan.hpp (compiled into a small host program) and its Python mirror against a
brute-force walk over every (row, key) pair of every case and of its partition at several q_pos0, Lk and n_prefix; the tile lists held to "a
padded tile is listed exactly when some row of the run sees one of its coordinates, once, ascending"; the fp64 reference against a dense-mask
softmax over the concatenated keys; the host emulation of attn_fprefix_kernel inside `bound()` at every element of every case, every injected
fault flagged on every row its rule names; the wrapper's refusals. (The C-ABI refusals: tests/test_attn_fprefix_cabi.py.)"""
import os
import shutil
import subprocess

import pytest
import torch

import attn_fprefix_cases as pc
from conftest import ROOT

ALL = pc.CASES + pc.ONE_BUFFER_EQUIV + pc.NORMALISED


@pytest.fixture(scope="module")
def refs():
    """operands and references of every row of CASES, computed once and left unchanged"""
    return {c.name: (ops, pc.reference(c, ops)) for c in pc.CASES for ops in [pc.make_case(c)]}


def brute_band(Lq, Lk, spans, q_pos0, back, ahead):
    """the suffix's window, pair by pair from the laid-out blocks: bool [Lq, Lk]"""
    blk, b = [], 0
    for rows, nblk in spans:
        for _ in range(nblk):
            blk += [b] * rows
            b += 1
    blk = torch.tensor(blk)
    bi, bj = blk[q_pos0:q_pos0 + Lq].view(Lq, 1), blk[:Lk].view(1, Lk)
    band = torch.ones(Lq, Lk, dtype=torch.bool)
    if back >= 0:
        band &= bj >= bi - back
    if ahead >= 0:
        band &= bj <= bi + ahead
    return band


# ---- the rule: header == mirror == brute force -----------------------------------------------------------------------------------------------
PLAN_MAIN = r"""
#include "attn_fprefix_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
// argv: groups of (Lq Lk q_pos0 back ahead n_prefix nspan rows_0 nblk_0 ...). Per group `S <prefix_tiles> <pad>`, then per 128-row block
// `B <np> <b_lo> <b_hi> <count>` and `L <the tiles by first_tile / next_tile>`, per 32-row wave of it `W <np> <b_lo> <b_hi>` and per tile of the
// BLOCK's list `I <q_first> <t> <in the wave's list> <interior>`, per row `R <i> <prefix keys seen> <first suffix key> <last> <count>` from
// visible() and `P <i> <first coordinate> <last> <count>` from visible_padded().
int main(int argc, char** argv) {
    using namespace attn_fprefix_plan;
    using namespace attn_fsink_plan;
    int a = 1;
    while (a + 6 < argc) {
        const long long Lq = atoll(argv[a]), Lk = atoll(argv[a + 1]);
        Plan w{};
        w.q_pos0 = atoll(argv[a + 2]); w.back = atoll(argv[a + 3]); w.ahead = atoll(argv[a + 4]);
        const long long n = atoll(argv[a + 5]);
        w.nspan = atoi(argv[a + 6]);
        a += 7;
        for (int g = 0; g < w.nspan; ++g, a += 2) { w.rows[g] = atoi(argv[a]); w.nblk[g] = atoi(argv[a + 1]); }
        printf("S %lld %lld\n", (long long)prefix_tiles(n), (long long)pad(n));
        for (long long q = 0; q < Lq; q += attn_fband_plan::QBLOCK) {
            const long long q1 = (q + attn_fband_plan::QBLOCK < Lq ? q + attn_fband_plan::QBLOCK : Lq) - 1;
            const TileList l = attn_fprefix_plan::tile_list(q, q1, Lk, w, n);
            printf("B %lld %lld %lld %lld\nL", (long long)l.n_sink, (long long)l.b_lo, (long long)l.b_hi, (long long)tile_count(l));
            for (long long t = first_tile(l); t <= l.b_hi; t = next_tile(t, l)) printf(" %lld", t);
            printf("\n");
            for (long long wq = q; wq <= q1; wq += attn_fband_plan::QWAVE) {
                const long long wq1 = (wq + attn_fband_plan::QWAVE - 1 < q1 ? wq + attn_fband_plan::QWAVE - 1 : q1);
                const TileList wl = attn_fprefix_plan::tile_list(wq, wq1, Lk, w, n);
                printf("W %lld %lld %lld\n", (long long)wl.n_sink, (long long)wl.b_lo, (long long)wl.b_hi);
                for (long long t = first_tile(l); t <= l.b_hi; t = next_tile(t, l))
                    printf("I %lld %lld %d %d\n", wq, t, in_list(t, wl) ? 1 : 0, attn_fprefix_plan::tile_is_interior(t, wq, wq1, Lk, w, n) ? 1 : 0);
            }
        }
        for (long long i = 0; i < Lq; ++i) {
            long long np = 0, first = -1, last = -1, cnt = 0;
            for (long long j = -2; j < n + 2; ++j) np += attn_fprefix_plan::visible(i, 0, j, Lk, w, n) ? 1 : 0;
            for (long long j = -2; j < Lk + 2; ++j)
                if (attn_fprefix_plan::visible(i, 1, j, Lk, w, n)) { if (first < 0) first = j; last = j; ++cnt; }
            printf("R %lld %lld %lld %lld %lld\n", i, np, first, last, cnt);
            first = last = -1; cnt = 0;
            for (long long c = 0; c < pad(n) + Lk + 2; ++c)
                if (visible_padded(i, c, Lk, w, n)) { if (first < 0) first = c; last = c; ++cnt; }
            printf("P %lld %lld %lld %lld\n", i, first, last, cnt);
        }
    }
    return 0;
}
"""


def _calls():
    """(Lq, Lk, spans, q_pos0, back, ahead, n_prefix): every row of the tables as it is, and every (partition, window) of them with every
    n_prefix of the tables and 0, 63, 65, at q_pos0 in {0, 1, 64, N - Lq} and Lk = N, a little short, and 30
    (where the later frames of a bounded window see no suffix key at all)"""
    out, seen = [], set()
    for c in ALL:
        out.append((c.Lq, c.Lk) + pc.rule(c))
    for c in ALL:
        N = pc.total_rows(c.spans)
        key = (tuple(c.spans), c.back, c.ahead)
        if key in seen:
            continue
        seen.add(key)
        for n in (0, 1, 52, 63, 64, 65, 116, 128, 180):
            for q_pos0 in (0, 1, 64, max(N - 50, 0)):
                for Lk in (N, N - 37, 30):
                    out.append((N - q_pos0, Lk, tuple(c.spans), q_pos0, c.back, c.ahead, n))
    return sorted(set(out))


def test_attn_fprefix_plan_hpp_and_its_mirror_agree_with_a_brute_force_walk(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "fprefix_plan_main.cpp", tmp_path / "fprefix_plan_main"
    src.write_text(PLAN_MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "yume_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    calls = _calls()
    assert len(calls) >= 300
    seen = {"jump": 0, "no_jump": 0, "interior_prefix": 0, "interior_suffix": 0, "edge": 0, "ragged_prefix_tile": 0, "wave_skips": 0,
            "no_suffix_tiles": 0}
    for n0 in range(0, len(calls), 20):
        chunk = calls[n0:n0 + 20]
        argv = [str(x) for Lq, Lk, spans, q_pos0, back, ahead, n in chunk
                for x in (Lq, Lk, q_pos0, back, ahead, n, len(spans)) + tuple(v for s in spans for v in s)]
        lines = iter(subprocess.run([str(exe)] + argv, check=True, stdout=subprocess.PIPE, text=True, timeout=300).stdout.split("\n"))
        for Lq, Lk, spans, q_pos0, back, ahead, n in chunk:
            w = (spans, q_pos0, back, ahead, n)
            ctx = (Lq, Lk) + w
            band = brute_band(Lq, Lk, spans, q_pos0, back, ahead)
            P, np_ = (n + 63) // 64 * 64, (n + 63) // 64
            vis = torch.zeros(Lq, P + Lk, dtype=torch.bool)              # the padded coordinate, laid out by hand
            vis[:, :n] = True
            vis[:, P:] = band
            assert torch.equal(vis, pc.visible_padded(Lq, Lk, *w)), ctx
            assert torch.equal(torch.cat([vis[:, :n], vis[:, P:]], dim=1), pc.visible(Lq, Lk, *w)), ctx
            assert next(lines) == f"S {np_} {P}" and (pc.prefix_tiles(n), pc.pad(n)) == (np_, P), ctx

            def tiles_seen(r0, r1):
                """the padded tiles of which some row of r0 ... r1 sees a coordinate, ascending"""
                cols = vis[r0:r1 + 1].any(dim=0).nonzero().view(-1)
                return sorted(set((cols // pc.KT).tolist()))
            for q in range(0, Lq, pc.QB):
                q1 = min(q + pc.QB, Lq) - 1
                want = tiles_seen(q, q1)
                tl = pc.tile_list(q, q1, Lk, *w)
                assert pc.tiles_of(tl) == want, ctx + (q,)               # each once, ascending
                assert next(lines) == f"B {tl[0]} {tl[1]} {tl[2]} {len(want)}", ctx + (q,)
                assert next(lines) == "L" + "".join(f" {t}" for t in want), ctx + (q,)
                walk, t = [], (0 if tl[0] > 0 else tl[1])
                while t <= tl[2]:
                    walk.append(t)
                    t = pc.next_tile(t, tl)
                assert walk == want, ctx + (q,)
                seen["jump" if any(b - a > 1 for a, b in zip(want, want[1:])) else "no_jump"] += 1
                seen["no_suffix_tiles"] += tl[1] > tl[2]
                for wq in range(q, q1 + 1, pc.QW):
                    wq1 = min(wq + pc.QW - 1, q1)
                    wl = pc.tile_list(wq, wq1, Lk, *w)
                    wave_tiles = tiles_seen(wq, wq1)
                    assert pc.tiles_of(wl) == wave_tiles and set(wave_tiles) <= set(want), ctx + (wq,)
                    assert next(lines) == f"W {wl[0]} {wl[1]} {wl[2]}", ctx + (wq,)
                    seen["wave_skips"] += len(wave_tiles) < len(want)
                    for t in want:
                        cols = slice(t * pc.KT, t * pc.KT + pc.KT)
                        interior = t * pc.KT + pc.KT <= P + Lk and bool(vis[wq:wq1 + 1, cols].all())
                        seen["interior_prefix" if interior and t < np_ else "interior_suffix" if interior else "edge"] += 1
                        seen["ragged_prefix_tile"] += t == np_ - 1 and n % 64 != 0
                        assert next(lines) == f"I {wq} {t} {int(t in wave_tiles)} {int(interior)}", ctx + (wq, t)
                        assert pc.tile_is_interior(t, wq, wq1, Lk, *w) == interior, ctx + (wq, t)
            for i in range(Lq):
                js = band[i].nonzero().view(-1)
                assert next(lines) == (f"R {i} {n} {int(js[0])} {int(js[-1])} {len(js)}" if len(js) else f"R {i} {n} -1 -1 0"), ctx + (i,)
                cs = vis[i].nonzero().view(-1)
                assert next(lines) == (f"P {i} {int(cs[0])} {int(cs[-1])} {len(cs)}" if len(cs) else f"P {i} -1 -1 0"), ctx + (i,)
    print(f"{len(calls)} calls: {seen}")
    assert min(seen.values()) >= 20, seen


# ---- the reference and the emulation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", pc.CASES, ids=[c.name for c in pc.CASES])
def test_the_reference_is_a_dense_mask_softmax_in_fp64_and_the_clean_emulation_is_inside_the_bound(c, refs):
    ops, r = refs[c.name]
    sg = ops["segs"][0]
    q, k, v = (t.double().transpose(0, 1) for t in (sg["q"], sg["k"], sg["v"]))          # [H, L, 128], the keys prefix then suffix
    mask = torch.cat([torch.ones(c.Lq, c.n_prefix, dtype=torch.bool), brute_band(c.Lq, c.Lk, c.spans, c.q_pos0, c.back, c.ahead)], dim=1)
    assert bool(mask.any(dim=1).all())                                                  # with a prefix no row is empty
    x = q @ k.transpose(1, 2) * (ops["scale_log2"] * 0.6931471805599453)
    a = torch.softmax(x.masked_fill(~mask, -float("inf")), dim=-1)
    want = {"ref": a @ v, "A": a @ v.abs(), "Q": (a * a) @ (v * v)}
    for key in ("ref", "A", "Q"):
        assert r[key].dtype == torch.float64 and r[key].shape == (c.Lq, c.H, pc.D)
        assert (r[key] - want[key].transpose(0, 1)).abs().max().item() <= 1e-12, key
    got = pc.emulate(c, ops)
    bnd = pc.bound(r)
    err = (got - (r["ref"] + r["base"])).abs()
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.zeros_like(got))
    print(f"{c.name}: worst error / bound {ratio.max().item():.3f}, {int((err > bnd).sum())} elements outside")
    assert int((err > bnd).sum()) == 0 and ratio.max().item() <= 0.95


@pytest.mark.parametrize("fault", pc.FAULTS)
def test_the_bound_flags_the_injected_fault_on_every_row_its_rule_names(fault, refs):
    named, flagged, report = [], [], []
    for c in pc.CASES:
        if not pc.fault_applies(fault, c):
            continue
        named.append(c.name)
        ops, r = refs[c.name]
        n = int(((pc.emulate(c, ops, fault) - (r["ref"] + r["base"])).abs() > pc.bound(r)).sum())
        report.append(f"{c.name} {n}")
        if n:
            flagged.append(c.name)
    print(f"{fault}: elements outside the bound per named row: " + ", ".join(report))
    assert named and flagged == named, (fault, sorted(set(named) - set(flagged)))


def test_the_tables_reach_what_they_were_built_for():
    pc.check_tables()
    assert len(pc.FAULTS) >= 7 and len(pc.CASES) >= 17
    names = [r[0] for r in pc.REFUSALS]
    assert len(set(names)) == len(names) and {"n_prefix_minus_1", "n_prefix_2_31", "null_kp", "null_vtp", "misaligned_kp", "misaligned_vtp",
                                              "ldvtp_odd", "ldvtp_short", "variant_7", "nspan_0", "lk_over_n"} <= set(names)
    assert pc.fband_log("[attn_fwd_fprefix] fprefix n_prefix=116 prefix_tiles=2 q_pos0=60 back=-1 ahead=0 nspan=1 nblocks=4 tiles_min=5 "
                        "tiles_max=5 Lq=100 Lk=160 H=2") == ("fprefix", {"n_prefix": 116, "prefix_tiles": 2, "q_pos0": 60, "back": -1, "ahead": 0,
                                                                           "nspan": 1, "nblocks": 4, "tiles_min": 5, "tiles_max": 5, "Lq": 100,
                                                                           "Lk": 160, "H": 2})


def test_the_wrapper_refuses_a_prefix_without_a_frame_window_and_beside_a_sink():
    import __graft_entry__ as g
    g.build()
    import inspect
    from yume_amd import ops
    t = torch.zeros(8, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=r"(?s)prefix.*frame_window"):
        ops.attn_fwd(t, t, t, t, 8, 8, 1, prefix=(t, t, 8))
    with pytest.raises(ValueError, match=r"(?s)prefix.*frame_sink"):
        ops.attn_fwd(t, t, t, t, 8, 8, 1, frame_window=(-1, 0), spans=[(8, 1)], frame_sink=1, prefix=(t, t, 8))
    assert inspect.signature(ops.attn_fwd).parameters["prefix"].default is None
