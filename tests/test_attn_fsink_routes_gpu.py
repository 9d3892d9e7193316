"""yume_attn_fwd_fsink on the device, one call per row of tests/attn_fsink_cases.py: EVERY output element inside the per-element bound against
the fp64 masked reference (computed on the device), no NaN of the pre-filled O left, the guard rows and columns of O still the sentinel,
a second launch equal in its bits, variant 13 equal in its bits to variant 0; a sink that is the whole key axis equal in its bits to
the global call; a sink that adds nothing (or sink = 0) equal in its bits to yume_attn_fwd_fband; the refusals by code and name with O
untouched; and, from one child process with YUME_ATTN_LOG=1, the entry each call really took: `fsink` with the row's shape, sink_rows and
the tile counts the Python mirror of attn_fsink_plan::tile_list predicts, fband's line for the equivalent calls, the ordinary `[attn_fwd]`
line for the normalised ones."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attn_fsink_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", sc.CASES, ids=[c.name for c in sc.CASES])
def test_every_element_inside_the_bound_guards_intact_equal_bits_on_a_second_launch_and_under_variant_13(c):
    ops = sc.make_fsink_case(c)
    r = sc.reference_fsink(c, ops, DEV)
    d = sc.run_fsink_case(c, ops)
    (g,), guards = sc.written(sc.as_case(c), d)
    assert not torch.isnan(g).any() and torch.isfinite(g).all()      # nothing of the NaN pre-fill is left, and no NaN was read
    want = r["ref"] + r["base"]
    bnd = sc.bound(r)
    err = (g - want).abs()
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
    print(f"{c.name}: worst error / bound {ratio.reshape(-1)[worst].item():.3f} at (row, head, d) = {idx}: got {g[idx].item():.6g} "
          f"ref {want[idx].item():.6g}; {int((err > bnd).sum())} of {err.numel()} elements outside")
    assert int((err > bnd).sum()) == 0
    assert bool((guards == sc.SENTINEL).all())                   # guard rows, guard columns
    first = d["obuf"].clone()
    d2 = sc.run_fsink_case(c, ops, None if c.acc else d)
    assert torch.equal(first, d2["obuf"])
    d3 = sc.run_fsink_case(c, ops, None if c.acc else d, variant=13)          # the kernel by its own number, with the row's flag bits
    assert torch.equal(first, d3["obuf"])
    # and it is another function than the same window without the sink (not on the ramp: a sink key weighs 2^-72 or less there)
    if c.pattern != "ramp4":
        assert not torch.equal(first, sc.run_fsink_case(c, ops, mode="fband")["obuf"])


@pytest.mark.parametrize("c", sc.NORMALISED, ids=[c.name for c in sc.NORMALISED])
def test_a_sink_that_is_the_whole_key_axis_is_the_global_call_bit_for_bit(c):
    ops = sc.make_fsink_case(c)
    a = sc.run_fsink_case(c, ops)
    b = sc.run_fsink_case(c, ops, mode="global")
    assert torch.isfinite(a["o"].float()).all()
    assert torch.equal(a["obuf"], b["obuf"])


@pytest.mark.parametrize("c", sc.FBAND_EQUIV, ids=[c.name for c in sc.FBAND_EQUIV])
def test_a_sink_that_adds_nothing_is_the_frame_band_call_bit_for_bit(c):
    ops = sc.make_fsink_case(c)
    a = sc.run_fsink_case(c, ops)
    b = sc.run_fsink_case(c, ops, mode="fband")
    assert torch.isfinite(a["o"].float()).all()
    assert torch.equal(a["obuf"], b["obuf"])
    r = sc.reference_fsink(c, ops, DEV)
    (g,), _ = sc.written(sc.as_case(c), a)
    assert int(((g - r["ref"]).abs() > sc.bound(r)).sum()) == 0
    assert not torch.equal(a["obuf"], sc.run_fsink_case(c, ops, mode="global")["obuf"])


@pytest.mark.parametrize("name,kw,code,word,who", sc.REFUSALS, ids=[r[0] for r in sc.REFUSALS])
def test_refusals_return_their_codes_and_names_on_the_device(name, kw, code, word, who):
    from yume_amd import _lib
    lib = _lib.load()
    H, Lq, Lk = 2, kw.get("Lq", 300), kw.get("Lk", 315)
    t = torch.zeros(320, H * 128, dtype=torch.bfloat16, device=DEV)
    vt = torch.zeros(H * 128, 320, dtype=torch.bfloat16, device=DEV)
    o = torch.full((320, H * 128), 5.0, dtype=torch.bfloat16, device=DEV)
    ptr = dict(Q=t.data_ptr(), K=t.data_ptr(), Vt=vt.data_ptr(), O=o.data_ptr())
    for k in ptr:
        if k in kw:
            ptr[k] = None if kw[k] is None else ptr[k] + (kw[k] - 4096)          # the table's offsets from an aligned address
    spans = kw.get("spans", sc.ONE_SPAN)
    arr = ctypes.c_int64 * max(len(spans), 1)
    rows, blocks = arr(*[s[0] for s in spans]), arr(*[s[1] for s in spans])
    rc = lib.yume_attn_fwd_fsink(ptr["Q"], H * 128, ptr["K"], H * 128, ptr["Vt"], kw.get("ldvt", 320), ptr["O"], H * 128, Lq, Lk, H, 0.088, 0,
                                 kw.get("variant", 0), kw.get("q_pos0", 0), len(spans), None if kw.get("null_spans") else rows, blocks,
                                 kw.get("back", 1), kw.get("ahead", 0), kw.get("sink", 1), None, 0, None)
    assert rc == code
    msg = lib.yume_last_error().decode()
    assert msg.startswith(who + ":") and word in msg, msg
    torch.cuda.synchronize()
    assert bool((o == 5.0).all())                                                 # refused before any launch


def test_every_call_takes_the_entry_and_walks_the_tiles_its_row_predicts():
    """YUME_ATTN_LOG is read once per process: a fresh child makes every call of the three tables once"""
    env = dict(os.environ, YUME_ATTN_LOG="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_fsink_cases.py"), "--routes"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lines, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            lines[name] = []
        elif line.startswith("[attn_fwd") and name is not None:
            lines[name].append(line)
    print("\n".join(f"{c.name}: {' + '.join(lines.get(c.name, []))}" for c in sc.CASES + sc.NORMALISED + sc.FBAND_EQUIV))
    for c in sc.CASES:
        assert len(lines[c.name]) == 1 and lines[c.name][0].startswith("[attn_fwd_fsink] "), c.name
        route, kv = sc.fband_log(lines[c.name][0])
        tmin, tmax = sc.tiles_min_max(c)
        assert route == "fsink", c.name
        assert (kv["q_pos0"], kv["back"], kv["ahead"], kv["sink"], kv["sink_rows"], kv["nspan"], kv["nblocks"], kv["tiles_min"], kv["tiles_max"],
                kv["Lq"], kv["Lk"], kv["H"]) == (c.q_pos0, c.back, c.ahead, c.sink, sc.send(c.Lk, c.spans, c.sink), len(c.spans),
                                                 sc.total_blocks(c.spans), tmin, tmax, c.Lq, c.Lk, c.H), c.name
        assert (kv["prescaled"], kv["kv_padded"], kv["accumulate"]) == (int(c.prescaled), int(c.padded), int(c.acc)), c.name
    for c in sc.FBAND_EQUIV:
        assert len(lines[c.name]) == 1 and lines[c.name][0].startswith("[attn_fwd_fband] "), c.name
        route, kv = sc.fband_log(lines[c.name][0])
        assert route == "fband" and (kv["q_pos0"], kv["back"], kv["ahead"], kv["Lq"], kv["Lk"]) == (c.q_pos0, c.back, c.ahead, c.Lq, c.Lk), c.name
        assert (kv["tiles_min"], kv["tiles_max"]) == sc.fb.tiles_min_max(c), c.name
    for c in sc.NORMALISED:
        assert len(lines[c.name]) == 1 and lines[c.name][0].startswith("[attn_fwd] "), c.name
        assert sc.ac.route_of(lines[c.name][0])[0] in sc.ac.ROUTES, c.name
