"""Host proof of tests/attn_fband_cases.py: attn_fband_plan.hpp (compiled into a small host program) and its Python mirror against a brute-force
walk over (row, key) pairs for every case's partition at several q_pos0, the fp64 reference against a dense-mask softmax, the host
emulation of attn_fband_kernel inside `bound()` at every element of every case, every injected fault flagged on the rows the table
records, framepack.frame_spans against a per-token frame index, and the C-ABI refusals of yume_attn_fwd_fband by name (no GPU: NULL
stream, pointers never dereferenced on the host)."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

import attn_fband_cases as fc
from conftest import ROOT

ALL = fc.CASES + fc.NORMALISED + fc.BAND_EQUIV
IDS = [c.name for c in fc.CASES]


@pytest.fixture(scope="module")
def refs():
    """operands and references of every row, computed once and left unchanged"""
    return {c.name: (ops, fc.reference_fband(c, ops)) for c in fc.CASES for ops in [fc.make_fband_case(c)]}


def brute_blocks(spans):
    """the block of every position, by laying the blocks out one after the other"""
    out, b = [], 0
    for rows, nblk in spans:
        for _ in range(nblk):
            out += [b] * rows
            b += 1
    return out


def brute_visible(Lq, Lk, spans, q_pos0, back, ahead):
    blk = brute_blocks(spans)
    return [[(back < 0 or blk[j] >= blk[q_pos0 + i] - back) and (ahead < 0 or blk[j] <= blk[q_pos0 + i] + ahead) for j in range(Lk)]
            for i in range(Lq)]


# ---- the rule: header == mirror == brute force -----------------------------------------------------------------------------------------------
PLAN_MAIN = r"""
#include "attn_fband_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
// argv: groups of (Lq Lk q_pos0 back ahead nspan rows_0 nblk_0 rows_1 nblk_1 ...). Per group one line `H <hides_nothing>`, then per 128-row
// block `B <t_lo> <t_hi>`, per 32-row wave and tile of its block's range `I <q_first> <t> <interior>`, per row `K <i> <klo> <khi>` from
// key_range and `R <i> <first visible key> <last visible key> <count>` from visible().
int main(int argc, char** argv) {
    using namespace attn_fband_plan;
    int a = 1;
    while (a + 5 < argc) {
        const long long Lq = atoll(argv[a]), Lk = atoll(argv[a + 1]);
        Plan w{};
        w.q_pos0 = atoll(argv[a + 2]); w.back = atoll(argv[a + 3]); w.ahead = atoll(argv[a + 4]); w.nspan = atoi(argv[a + 5]);
        a += 6;
        for (int g = 0; g < w.nspan; ++g, a += 2) { w.rows[g] = atoi(argv[a]); w.nblk[g] = atoi(argv[a + 1]); }
        printf("N %lld %lld\n", (long long)total_rows(w), (long long)total_blocks(w));
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
            const KeyRange kr = key_range(i, i, Lk, w);
            printf("K %lld %lld %lld\n", i, (long long)kr.lo, (long long)kr.hi);
            long long first = -1, last = -1, n = 0;
            for (long long j = -2; j < Lk + 2; ++j)
                if (visible(i, j, Lk, w)) { if (first < 0) first = j; last = j; ++n; }
            printf("R %lld %lld %lld %lld\n", i, first, last, n);
        }
    }
    return 0;
}
"""


def _calls():
    """(Lq, Lk, spans, q_pos0, back, ahead): every row of the tables as it is, and every partition and window of them at q_pos0 in
    {0, 1, 63, 64, 127, 128, N - Lq} with the rows that fit (up to 200 rows; up to the end where N <= 700), Lk = N and Lk a little short"""
    out, seen = [], set()
    for c in ALL:
        out.append((c.Lq, c.Lk, tuple(c.spans), c.q_pos0, c.back, c.ahead))
    for c in ALL:
        N = fc.total_rows(c.spans)
        if (tuple(c.spans), c.back, c.ahead) in seen:
            continue
        seen.add((tuple(c.spans), c.back, c.ahead))
        for Lq in (min(200, N),) + ((N,) if N <= 700 else ()):          # (the brute force is a Python walk over Lq x Lk pairs)
            for q_pos0 in (0, 1, 63, 64, 127, 128, N - Lq):
                if q_pos0 + Lq > N:
                    Lq2 = N - q_pos0
                else:
                    Lq2 = Lq
                for Lk in (N, N - 37):
                    out.append((Lq2, Lk, tuple(c.spans), q_pos0, c.back, c.ahead))
    return sorted(set(out))


def test_attn_fband_plan_hpp_and_its_mirror_agree_with_a_brute_force_walk(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "fband_plan_main.cpp", tmp_path / "fband_plan_main"
    src.write_text(PLAN_MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "yume_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    calls = _calls()
    assert len(calls) >= 200
    seen = {"hides_nothing": 0, "hides": 0, "empty_row": 0, "interior": 0, "edge": 0}
    for n0 in range(0, len(calls), 20):
        chunk = calls[n0:n0 + 20]
        argv = [str(x) for Lq, Lk, spans, q_pos0, back, ahead in chunk
                for x in (Lq, Lk, q_pos0, back, ahead, len(spans)) + tuple(v for s in spans for v in s)]
        lines = iter(subprocess.run([str(exe)] + argv, check=True, stdout=subprocess.PIPE, text=True, timeout=300).stdout.split("\n"))
        for Lq, Lk, spans, q_pos0, back, ahead in chunk:
            w = (spans, q_pos0, back, ahead)
            ctx = (Lq, Lk) + w
            blk = brute_blocks(spans)
            assert next(lines) == f"N {len(blk)} {blk[-1] + 1}", ctx
            assert (fc.total_rows(spans), fc.total_blocks(spans)) == (len(blk), blk[-1] + 1)
            assert [fc.block_of(p, spans) for p in range(len(blk))] == blk and fc.block_index(spans).tolist() == blk
            for b in range(blk[-1] + 1):
                assert fc.block_start(b, spans) == (blk.index(b), blk.index(b) + blk.count(b))
            vis = brute_visible(Lq, Lk, *w)
            assert torch.equal(torch.tensor(vis), fc.visible(Lq, Lk, *w)), ctx
            nothing_hidden = all(all(row) for row in vis)
            seen["hides_nothing" if nothing_hidden else "hides"] += 1
            assert next(lines) == f"H {int(nothing_hidden)}", ctx
            assert fc.hides_nothing(Lq, Lk, *w) == nothing_hidden, ctx
            for q in range(0, Lq, fc.QB):
                q1 = min(q + fc.QB, Lq) - 1
                keys = [j for i in range(q, q1 + 1) for j in range(Lk) if vis[i][j]]
                want = (min(keys) // fc.KT, max(keys) // fc.KT) if keys else (0, -1)        # the run's range is the union of its rows'
                assert next(lines) == f"B {want[0]} {want[1]}", ctx + (q,)
                assert fc.tile_range(q, q1, Lk, *w) == want, ctx + (q,)
                for wq in range(q, q1 + 1, fc.QW):
                    wq1 = min(wq + fc.QW - 1, q1)
                    for t in range(want[0], want[1] + 1):
                        interior = all(j < Lk and vis[i][j] for i in range(wq, wq1 + 1) for j in range(t * fc.KT, t * fc.KT + fc.KT))
                        seen["interior" if interior else "edge"] += 1
                        assert next(lines) == f"I {wq} {t} {int(interior)}", ctx + (wq, t)
                        assert fc.tile_is_interior(t, wq, wq1, Lk, *w) == interior, ctx + (wq, t)
            prev = (0, 0)
            for i in range(Lq):
                js = [j for j in range(Lk) if vis[i][j]]
                lo, hi = fc.key_range(i, i, Lk, *w)
                assert next(lines) == f"K {i} {lo} {hi}", ctx + (i,)
                assert next(lines) == (f"R {i} {js[0]} {js[-1]} {len(js)}" if js else f"R {i} -1 -1 0"), ctx + (i,)
                assert (list(range(lo, hi + 1)) if lo <= hi else []) == js, ctx + (i,)          # the visible set IS the interval
                assert lo >= prev[0] and hi >= prev[1], ctx + (i,)                               # both ends non-decreasing in the row
                prev = (lo, hi)
                seen["empty_row"] += not js
    print(f"{len(calls)} calls: {seen}")
    assert seen["hides_nothing"] >= 10 and seen["hides"] >= 100 and seen["empty_row"] >= 100 and seen["interior"] >= 100 and seen["edge"] >= 100


# ---- the reference and the emulation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", fc.CASES, ids=IDS)
def test_the_reference_is_a_dense_mask_softmax_in_fp64_and_the_clean_emulation_is_inside_the_bound(c, refs):
    ops, r = refs[c.name]
    sg = ops["segs"][0]
    q, k, v = (t.double().transpose(0, 1) for t in (sg["q"], sg["k"], sg["v"]))          # [H, L, 128]
    mask = torch.tensor(brute_visible(c.Lq, c.Lk, *fc.rule(c)))
    x = q @ k.transpose(1, 2) * (ops["scale_log2"] * 0.6931471805599453)
    a = torch.softmax(x.masked_fill(~mask, -float("inf")), dim=-1)
    a = torch.where(mask.any(dim=1).view(1, -1, 1), a, torch.zeros_like(a))             # (softmax of an all-hidden row is NaN: the row is 0)
    want = {"ref": a @ v, "A": a @ v.abs(), "Q": (a * a) @ (v * v)}
    for key in ("ref", "A", "Q"):
        assert r[key].dtype == torch.float64 and r[key].shape == (c.Lq, c.H, fc.D)
        assert (r[key] - want[key].transpose(0, 1)).abs().max().item() <= 1e-12, key
    empty = fc.empty_rows(c)
    assert torch.equal(empty, ~mask.any(dim=1))
    for key in ("ref", "A", "Q"):
        assert bool((r[key][empty] == 0).all())
    got = fc.emulate_fband(c, ops)
    bnd = fc.bound(r)
    err = (got - (r["ref"] + r["base"])).abs()
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.zeros_like(got))
    print(f"{c.name}: worst error / bound {ratio.max().item():.3f}, {int((err > bnd).sum())} elements outside")
    assert int((err > bnd).sum()) == 0 and ratio.max().item() <= 0.95
    if ops["base"] is None:
        assert bool((got[empty] == 0).all())
    else:
        assert torch.equal(got[empty], ops["base"].double().view(c.Lq, c.H, fc.D)[empty])


@pytest.mark.parametrize("fault", fc.FAULTS)
def test_the_bound_flags_the_injected_fault_on_the_rows_the_table_records(fault, refs):
    flagged, report = [], []
    for c in fc.CASES:
        ops, r = refs[c.name]
        n = int(((fc.emulate_fband(c, ops, fault) - (r["ref"] + r["base"])).abs() > fc.bound(r)).sum())
        report.append(f"{c.name} {n}")
        if n:
            flagged.append(c.name)
    print(f"{fault}: elements outside the bound per row: " + ", ".join(report))
    print(f"{fault}: flagged on {tuple(flagged)}")
    assert fc.FAULT_ROWS[fault], fault
    assert set(fc.FAULT_ROWS[fault]) <= set(flagged), (fault, sorted(set(fc.FAULT_ROWS[fault]) - set(flagged)))


def test_the_tables_reach_what_they_were_built_for():
    names = [c.name for c in ALL]
    assert len(set(names)) == len(names) and set(fc.FAULT_ROWS) == set(fc.FAULTS) and len(fc.FAULTS) == 7
    assert all(n in [c.name for c in fc.CASES] for rows in fc.FAULT_ROWS.values() for n in rows)
    for c in ALL:
        N = fc.total_rows(c.spans)
        assert c.H == 2 and 1 <= len(c.spans) <= fc.MAX_SPANS and c.q_pos0 >= 0 and c.q_pos0 + c.Lq <= N and c.Lk <= N, c.name
    for c in fc.CASES + fc.BAND_EQUIV:
        assert not fc.hides_nothing(c.Lq, c.Lk, *fc.rule(c)), c.name
    for c in fc.NORMALISED:
        assert fc.hides_nothing(c.Lq, c.Lk, *fc.rule(c)), c.name
    by = {c.name: c for c in fc.CASES}
    # the ramp: how far the walked tiles' top lies above a row's BEST visible key (its lower keys lie further down, beyond exp2's 126)
    assert {n: fc.ramp_gap(c) for n, c in by.items() if c.pattern == "ramp4"} == {
        "ramp4_one_span_binf_a0": 116, "ramp4_one_span_b0_a0": 116, "ramp4_pyramid_binf_a0": 232, "ramp4_pyramid_b1_a1": 208}
    # no masked tile at all where every edge is a tile edge; a workgroup without a key; empty rows under accumulate; Lk < N
    for n in ("aligned_64x6_b1_a0", "aligned_128x3_b1_a0"):
        c = by[n]
        for w0 in range(0, c.Lq, fc.QW):
            lo, hi = fc.tile_range(w0, w0 + fc.QW - 1, c.Lk, *fc.rule(c))
            assert all(fc.tile_is_interior(t, w0, w0 + fc.QW - 1, c.Lk, *fc.rule(c)) for t in range(lo, hi + 1)), (n, w0)
    assert fc.block_tiles(by["trimmed_lk500_b0_a0"])[-1] == (0, -1)
    assert by["trimmed_lk500_acc"].acc and bool(fc.empty_rows(by["trimmed_lk500_acc"]).any())
    assert any(c.Lk < fc.total_rows(c.spans) for c in fc.CASES)
    assert {c.prescaled for c in fc.CASES} == {True, False} and any(c.padded for c in fc.CASES) and any(c.acc for c in fc.CASES)
    # several blocks inside one tile and one wave; a block larger than a workgroup with interior tiles inside it
    assert by["tiny_blocks_b2_a1"].spans[0][0] * 6 < fc.QW and by["big_blocks_b0_a0"].spans[0][0] > fc.QB
    c = by["big_blocks_b0_a0"]
    assert any(fc.tile_is_interior(t, 320, 351, c.Lk, *fc.rule(c)) for t in range(*fc.tile_range(320, 351, c.Lk, *fc.rule(c))))
    # the band-equivalent rows ARE the token window: same visible set as tests/attn_band_cases.py's rule
    import attn_band_cases as bc
    for c in fc.BAND_EQUIV:
        assert torch.equal(fc.visible(c.Lq, c.Lk, *fc.rule(c)), bc.visible(c.Lq, c.Lk, c.q_pos0, c.back, c.ahead)), c.name
    assert fc.fband_log("[attn_fwd_fband] fband q_pos0=312 back=1 ahead=1 nspan=5 nblocks=13 tiles_min=3 tiles_max=5 Lq=288 Lk=600 H=2 ldq=512") == \
        ("fband", {"q_pos0": 312, "back": 1, "ahead": 1, "nspan": 5, "nblocks": 13, "tiles_min": 3, "tiles_max": 5, "Lq": 288, "Lk": 600, "H": 2,
                   "ldq": 512})


# ---- framepack.frame_spans ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hist", [1, 2, 4, 9, 22, 86])
def test_frame_spans_of_a_packed_plan_is_the_per_token_frame_index(n_hist):
    from yume_amd import framepack
    lfz, h, w = 8, 12, 16
    plan = framepack.pack_plan(n_hist + lfz, h, w, lfz)
    spans = framepack.frame_spans(plan)
    want, frame = [], 0                           # token by token: the groups in packed order, frame-major inside a group
    for g in plan.groups:
        for _ in range(g.nf):
            want += [frame] * (g.hp * g.wp)
            frame += 1
    assert len(spans) == len(plan.groups) and fc.total_rows(spans) == plan.seq_len == len(want)
    assert fc.block_index(spans).tolist() == want and [fc.block_of(p, spans) for p in range(len(want))] == want
    # the same frame counter the RoPE table's temporal index uses (plan_rope's f_off)
    assert fc.total_blocks(spans) == sum(g.nf for g in plan.groups)
    assert spans[-1] == (plan.new_grid[1] * plan.new_grid[2], lfz) and fc.total_rows(spans[:-1]) == plan.n_hist_tok


def test_frame_spans_of_a_plain_latent():
    from yume_amd import framepack
    F, H, W = 5, 12, 16
    assert framepack.frame_spans((F, H, W)) == [(48, 5)] == framepack.frame_spans(framepack.Group(0, F, 0, H // 2, W // 2))
    want = [f for f in range(F) for _ in range((H // 2) * (W // 2))]
    assert fc.block_index(framepack.frame_spans((F, H, W))).tolist() == want
    with pytest.raises(ValueError, match="even"):
        framepack.frame_spans((F, 13, W))


# ---- the C ABI and the Python layers, without a GPU --------------------------------------------------------------------------------------------
PTR = 4096            # any 16-byte aligned non-NULL value passes the common checks


def _lib():
    import __graft_entry__ as g
    g.build()
    from yume_amd import _lib
    return _lib


def _call(lib, Q=PTR, K=PTR, Vt=PTR, O=PTR, Lq=300, Lk=315, H=2, ldvt=320, variant=0, q_pos0=0, spans=fc.ONE_SPAN, back=1, ahead=0, null_spans=False):
    arr = ctypes.c_int64 * max(len(spans), 1)
    rows, blocks = arr(*[r for r, _ in spans]), arr(*[b for _, b in spans])
    return lib.yume_attn_fwd_fband(Q, H * 128, K, H * 128, Vt, ldvt, O, H * 128, Lq, Lk, H, 0.088, 0, variant, q_pos0, len(spans),
                                   None if null_spans else rows, blocks, back, ahead, None, 0, None)


def test_export_header_binding_and_wrapper_agree():
    _l = _lib()
    hdr = open(os.path.join(ROOT, "include", "yume_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    syms = sorted(set(re.findall(r"\b(yume_[a-z0-9_]+)\s*\(", src)))
    assert "yume_attn_fwd_fband" in syms
    assert "yume_attn_fwd_fband" in _l.SIGNATURES and len(_l.SIGNATURES["yume_attn_fwd_fband"]) == 23
    assert sorted(_l.SIGNATURES) == syms
    assert hasattr(ctypes.CDLL(_l.LIB_PATH), "yume_attn_fwd_fband")
    lib = _l.load()
    # an added export changes no argument list: the ABI number stays
    assert lib.yume_abi_version() == _l.ABI_VERSION == 9 == int(re.search(r"#define YUME_ABI_VERSION (\d+)", hdr).group(1))
    from yume_amd import attention, ops
    sig = inspect.signature(ops.attn_fwd).parameters
    assert sig["frame_window"].default is None and sig["spans"].default is None and sig["window"].default == (-1, -1)
    assert list(inspect.signature(attention.frame_window_attention).parameters) == ["q", "k", "v", "spans", "frame_window", "q_lens", "k_lens",
                                                                                    "softmax_scale"]
    assert "frame_window" not in inspect.signature(attention.flash_attention).parameters


@pytest.mark.parametrize("name,kw,code,word", fc.REFUSALS, ids=[r[0] for r in fc.REFUSALS])
def test_refusals_answer_by_name_before_any_launch(name, kw, code, word):
    lib = _lib().load()
    assert _call(lib, **kw) == code
    msg = lib.yume_last_error().decode()
    assert "attn_fwd_fband" in msg and word in msg, msg


def test_the_wrapper_refuses_what_does_not_combine():
    _lib()
    from yume_amd import ops
    t = torch.zeros(8, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="last_key_weight"):
        ops.attn_fwd(t, t, t, t, 8, 8, 1, last_key_weight=3.0, frame_window=(1, 0), spans=[(2, 4)])
    with pytest.raises(RuntimeError, match="window"):
        ops.attn_fwd(t, t, t, t, 8, 8, 1, window=(2, 0), frame_window=(1, 0), spans=[(2, 4)])
    with pytest.raises(RuntimeError, match="spans"):
        ops.attn_fwd(t, t, t, t, 8, 8, 1, frame_window=(1, 0))
    with pytest.raises(RuntimeError, match="spans"):
        ops.attn_fwd(t, t, t, t, 8, 8, 1, spans=[(2, 4)])


def test_the_engine_takes_the_attribute(monkeypatch):
    from yume_amd.dit import DiTEngine

    class M:
        window_size = (-1, -1)
    e = DiTEngine(M(), "wan23")
    assert e.frame_window is None and e._frame_args(5) == {}            # the default reaches nothing and passes nothing
    e.frame_window = (1, 0)
    with pytest.raises(NotImplementedError, match="frame_window"):     # no clip, no partition (block_forward's bare rows)
        e._frame_args(0)
    e._spans = [(6, 2), (24, 3)]
    assert e._frame_args(5) == {"frame_window": (1, 0), "spans": [(6, 2), (24, 3)], "q_pos0": 5}
    assert e._frame_args(0, 84) == e._frame_args(0)
    assert e._frame_args(0, 96)["spans"] == [(6, 2), (24, 3), (12, 1)]   # the sequence-parallel pad rows: one more block behind the clip
    for who in ("forward_pair / forward_cfg", "forward_batch"):
        with pytest.raises(NotImplementedError, match="frame_window"):
            e._refuse_frame_window(who)
        e._refuse_window(who)
    e.window_size = (4, 4)
    with pytest.raises(ValueError, match=r"(?s)frame_window.*window_size"):
        e._frame_args(0)
    e.window_size = (-1, -1)
    e.frame_window = (-2, 0)
    with pytest.raises(ValueError, match="frame_window"):
        e._frame_args(0)
    monkeypatch.setenv("YUME_FRAME_WINDOW", "-1,0")
    assert DiTEngine(M(), "wan23").frame_window == (-1, 0)
