"""yume_attn_fwd_fband on the device, one call per row of tests/attn_fband_cases.py: EVERY output element inside the per-element bound against
the fp64 masked reference (computed on the device), no NaN of the pre-filled O left, rows that see no key exactly 0 (exactly the old O
under accumulate), the guard rows and columns of O still the sentinel, a second launch equal in its bits; the calls that hide nothing
equal in their bits to the global call; one span of one-row blocks equal in its bits to yume_attn_fwd_band; the refusals by code and
name; and, from one child process with YUME_ATTN_LOG=1, the entry each call really took: `fband` with the row's shape and the tile
counts the Python mirror of attn_fband_plan::tile_range predicts, the ordinary `[attn_fwd]` line for the normalised calls."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attn_fband_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", fc.CASES, ids=[c.name for c in fc.CASES])
def test_every_element_inside_the_bound_empty_rows_exact_guards_intact_equal_bits_on_a_second_launch(c):
    ops = fc.make_fband_case(c)
    r = fc.reference_fband(c, ops, DEV)
    d = fc.run_fband_case(c, ops)
    (g,), guards = fc.written(fc.as_case(c), d)
    assert not torch.isnan(g).any() and torch.isfinite(g).all()      # nothing of the NaN pre-fill is left, and no NaN was read
    want = r["ref"] + r["base"]
    bnd = fc.bound(r)
    err = (g - want).abs()
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
    print(f"{c.name}: worst error / bound {ratio.reshape(-1)[worst].item():.3f} at (row, head, d) = {idx}: got {g[idx].item():.6g} "
          f"ref {want[idx].item():.6g}; {int((err > bnd).sum())} of {err.numel()} elements outside")
    assert int((err > bnd).sum()) == 0
    empty = fc.empty_rows(c).to(DEV)
    if c.acc:                                                    # the old O survives bit for bit
        assert torch.equal(g[empty], ops["base"].to(DEV).double().view(c.Lq, c.H, fc.D)[empty])
    else:
        assert bool((g[empty] == 0).all())
    assert bool((guards == fc.SENTINEL).all())                   # guard rows, guard columns
    first = d["obuf"].clone()
    d2 = fc.run_fband_case(c, ops, None if c.acc else d)
    assert torch.equal(first, d2["obuf"])


@pytest.mark.parametrize("c", fc.NORMALISED, ids=[c.name for c in fc.NORMALISED])
def test_a_frame_window_that_hides_nothing_is_the_global_call_bit_for_bit(c):
    ops = fc.make_fband_case(c)
    a = fc.run_fband_case(c, ops)
    b = fc.run_fband_case(c, ops, mode="global")
    assert torch.isfinite(a["o"].float()).all()
    assert torch.equal(a["obuf"], b["obuf"])


@pytest.mark.parametrize("c", fc.BAND_EQUIV, ids=[c.name for c in fc.BAND_EQUIV])
def test_one_span_of_one_row_blocks_is_the_band_call_bit_for_bit(c):
    ops = fc.make_fband_case(c)
    a = fc.run_fband_case(c, ops)
    b = fc.run_fband_case(c, ops, mode="band")
    assert torch.isfinite(a["o"].float()).all()
    assert torch.equal(a["obuf"], b["obuf"])
    # and it is the masked function, not the global one
    r = fc.reference_fband(c, ops, DEV)
    (g,), _ = fc.written(fc.as_case(c), a)
    assert int(((g - r["ref"]).abs() > fc.bound(r)).sum()) == 0
    assert not torch.equal(a["obuf"], fc.run_fband_case(c, ops, mode="global")["obuf"])


@pytest.mark.parametrize("name,kw,code,word", fc.REFUSALS, ids=[r[0] for r in fc.REFUSALS])
def test_refusals_return_their_codes_and_names_on_the_device(name, kw, code, word):
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
    spans = kw.get("spans", fc.ONE_SPAN)
    arr = ctypes.c_int64 * max(len(spans), 1)
    rows, blocks = arr(*[s[0] for s in spans]), arr(*[s[1] for s in spans])
    rc = lib.yume_attn_fwd_fband(ptr["Q"], H * 128, ptr["K"], H * 128, ptr["Vt"], kw.get("ldvt", 320), ptr["O"], H * 128, Lq, Lk, H, 0.088, 0,
                                 kw.get("variant", 0), kw.get("q_pos0", 0), len(spans), None if kw.get("null_spans") else rows, blocks,
                                 kw.get("back", 1), kw.get("ahead", 0), None, 0, None)
    assert rc == code
    msg = lib.yume_last_error().decode()
    assert "attn_fwd_fband" in msg and word in msg, msg
    torch.cuda.synchronize()
    assert bool((o == 5.0).all())                                                 # refused before any launch


def test_every_call_takes_the_entry_and_walks_the_tiles_its_row_predicts():
    """YUME_ATTN_LOG is read once per process: a fresh child makes every call of both tables once"""
    env = dict(os.environ, YUME_ATTN_LOG="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_fband_cases.py"), "--routes"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lines, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            lines[name] = []
        elif line.startswith("[attn_fwd") and name is not None:
            lines[name].append(line)
    print("\n".join(f"{c.name}: {' + '.join(lines.get(c.name, []))}" for c in fc.CASES + fc.NORMALISED))
    for c in fc.CASES:
        assert len(lines[c.name]) == 1 and lines[c.name][0].startswith("[attn_fwd_fband] "), c.name
        route, kv = fc.fband_log(lines[c.name][0])
        tmin, tmax = fc.tiles_min_max(c)
        assert route == "fband", c.name
        assert (kv["q_pos0"], kv["back"], kv["ahead"], kv["nspan"], kv["nblocks"], kv["tiles_min"], kv["tiles_max"], kv["Lq"], kv["Lk"], kv["H"]) == \
            (c.q_pos0, c.back, c.ahead, len(c.spans), fc.total_blocks(c.spans), tmin, tmax, c.Lq, c.Lk, c.H), c.name
        assert (kv["prescaled"], kv["kv_padded"], kv["accumulate"]) == (int(c.prescaled), int(c.padded), int(c.acc)), c.name
    for c in fc.NORMALISED:
        assert len(lines[c.name]) == 1 and lines[c.name][0].startswith("[attn_fwd] "), c.name
        assert fc.ac.route_of(lines[c.name][0])[0] in fc.ac.ROUTES, c.name
