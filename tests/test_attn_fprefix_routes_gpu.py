"""yume_attn_fwd_fprefix on the device, one call per row of tests/attn_fprefix_cases.py: EVERY output element inside the per-element bound
against the fp64 masked reference over the concatenated keys (computed on the device), no NaN of the pre-filled O left and none read from the
poisoned rows and columns behind n_prefix and Lk, the guard rows and columns of O still the sentinel, a second launch equal in its bits,
variant 14 equal in its bits to variant 0; prefix and suffix as views of one buffer equal in their bits to the one-buffer call with the
prefix as a sink block; n_prefix = 0 equal in its bits to yume_attn_fwd_fband; the refusals by code and name with O untouched; and, from one
child process with YUME_ATTN_LOG=1, the entry each call really took: `fprefix` with the row's shape, prefix_tiles and the tile counts the
Python mirror of attn_fprefix_plan::tile_list predicts, fband's line for the normalised calls."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attn_fprefix_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", pc.CASES, ids=[c.name for c in pc.CASES])
def test_every_element_inside_the_bound_guards_intact_equal_bits_on_a_second_launch_and_under_variant_14(c):
    ops = pc.make_case(c)
    r = pc.reference(c, ops, DEV)
    d = pc.run_case(c, ops)
    (g,), guards = pc.written(pc.as_case(c), d)
    assert not torch.isnan(g).any() and torch.isfinite(g).all()      # nothing of the NaN pre-fill is left, and no NaN was read
    want = r["ref"] + r["base"]
    bnd = pc.bound(r)
    err = (g - want).abs()
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
    print(f"{c.name}: worst error / bound {ratio.reshape(-1)[worst].item():.3f} at (row, head, d) = {idx}: got {g[idx].item():.6g} "
          f"ref {want[idx].item():.6g}; {int((err > bnd).sum())} of {err.numel()} elements outside")
    assert int((err > bnd).sum()) == 0
    assert bool((guards == pc.SENTINEL).all())                   # guard rows, guard columns
    first = d["obuf"].clone()
    d2 = pc.run_case(c, ops, None if c.acc else d)
    assert torch.equal(first, d2["obuf"])
    d3 = pc.run_case(c, ops, None if c.acc else d, variant=14)          # the kernel by its own number, with the row's flag bits
    assert torch.equal(first, d3["obuf"])
    # and it is another function than the same suffix call without the prefix (not on the ramp: the prefix key weighs 2^-92 or less there)
    if c.pattern != "ramp4" and not c.acc:
        assert not torch.equal(first, pc.run_fband(c, ops)["obuf"])


@pytest.mark.parametrize("c", pc.ONE_BUFFER_EQUIV, ids=[c.name for c in pc.ONE_BUFFER_EQUIV])
def test_views_of_one_buffer_give_the_bits_of_the_one_buffer_call_with_the_prefix_as_a_sink_block(c):
    ops = pc.make_case(c)
    two, one = pc.run_one_buffer_pair(c, ops)
    assert torch.isfinite(two.float()).all()
    assert torch.equal(two, one)
    r = pc.reference(c, ops, DEV)
    g = two[pc.GUARD_ROWS:pc.GUARD_ROWS + c.Lq].double().view(c.Lq, c.H, pc.D)
    assert int(((g - r["ref"]).abs() > pc.bound(r)).sum()) == 0


@pytest.mark.parametrize("c", pc.NORMALISED, ids=[c.name for c in pc.NORMALISED])
def test_an_empty_prefix_is_the_frame_band_call_bit_for_bit(c):
    ops = pc.make_case(c)
    a = pc.run_case(c, ops)
    b = pc.run_fband(c, ops)
    assert torch.isfinite(a["o"].float()).all()
    assert torch.equal(a["obuf"], b["obuf"])


@pytest.mark.parametrize("name,kw,code,word,who", pc.REFUSALS, ids=[r[0] for r in pc.REFUSALS])
def test_refusals_return_their_codes_and_names_on_the_device(name, kw, code, word, who):
    from yume_amd import _lib
    lib = _lib.load()
    a = dict(pc.REFUSAL_DEFAULT, **{k: v for k, v in kw.items() if k in pc.REFUSAL_DEFAULT})
    H = a["H"]
    t = torch.zeros(320, H * 128, dtype=torch.bfloat16, device=DEV)
    vt = torch.zeros(H * 128, 320, dtype=torch.bfloat16, device=DEV)
    o = torch.full((320, H * 128), 5.0, dtype=torch.bfloat16, device=DEV)
    ptr = dict(Q=t.data_ptr(), K=t.data_ptr(), Vt=vt.data_ptr(), O=o.data_ptr(), Kp=t.data_ptr(), Vtp=vt.data_ptr())
    for k in ptr:
        if k in kw:
            ptr[k] = None if kw[k] is None else ptr[k] + (kw[k] - 4096)          # the table's offsets from an aligned address
    spans = a["spans"]
    arr = ctypes.c_int64 * max(len(spans), 1)
    rows, blocks = arr(*[s[0] for s in spans]), arr(*[s[1] for s in spans])
    rc = lib.yume_attn_fwd_fprefix(ptr["Q"], H * 128, ptr["K"], H * 128, ptr["Vt"], a["ldvt"], ptr["O"], H * 128, a["Lq"], a["Lk"], H, 0.088, 0,
                                   a["variant"], a["q_pos0"], len(spans), None if kw.get("null_spans") else rows, blocks, a["back"], a["ahead"],
                                   ptr["Kp"], a["ldkp"], ptr["Vtp"], a["ldvtp"], a["n_prefix"], None, 0, None)
    assert rc == code
    msg = lib.yume_last_error().decode()
    assert msg.startswith(who + ":") and word in msg, msg
    torch.cuda.synchronize()
    assert bool((o == 5.0).all())                                                 # refused before any launch


def test_every_call_takes_the_entry_and_walks_the_tiles_its_row_predicts():
    """YUME_ATTN_LOG is read once per process: a fresh child makes every call of the three tables once"""
    env = dict(os.environ, YUME_ATTN_LOG="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_fprefix_cases.py"), "--routes"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lines, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            lines[name] = []
        elif line.startswith("[attn_fwd") and name is not None:
            lines[name].append(line)
    print("\n".join(f"{c.name}: {' + '.join(lines.get(c.name, []))}" for c in pc.CASES + pc.ONE_BUFFER_EQUIV + pc.NORMALISED))

    def held(c, line):
        assert line.startswith("[attn_fwd_fprefix] "), c.name
        route, kv = pc.fband_log(line)
        tmin, tmax = pc.tiles_min_max(c)
        assert route == "fprefix", c.name
        assert (kv["n_prefix"], kv["prefix_tiles"], kv["q_pos0"], kv["back"], kv["ahead"], kv["nspan"], kv["nblocks"], kv["tiles_min"],
                kv["tiles_max"], kv["Lq"], kv["Lk"], kv["H"]) == (c.n_prefix, pc.prefix_tiles(c.n_prefix), c.q_pos0, c.back, c.ahead, len(c.spans),
                                                                  pc.total_blocks(c.spans), tmin, tmax, c.Lq, c.Lk, c.H), c.name
        assert (kv["prescaled"], kv["kv_padded"], kv["accumulate"]) == (int(c.prescaled), int(c.padded), int(c.acc)), c.name
    for c in pc.CASES:
        assert len(lines[c.name]) == 1, c.name
        held(c, lines[c.name][0])
    for c in pc.ONE_BUFFER_EQUIV:          # the two-buffer call, then the one-buffer call under fsink's or fband's name
        assert len(lines[c.name]) == 2, c.name
        held(c, lines[c.name][0])
        assert lines[c.name][1].startswith(("[attn_fwd_fsink] ", "[attn_fwd_fband] ")), c.name
        assert pc.fband_log(lines[c.name][1])[1]["Lk"] == c.n_prefix + c.Lk, c.name
    for c in pc.NORMALISED:
        assert len(lines[c.name]) == 1 and lines[c.name][0].startswith("[attn_fwd_fband] "), c.name
        route, kv = pc.fband_log(lines[c.name][0])
        assert route == "fband" and (kv["q_pos0"], kv["back"], kv["ahead"], kv["Lq"], kv["Lk"]) == (c.q_pos0, c.back, c.ahead, c.Lq, c.Lk), c.name
