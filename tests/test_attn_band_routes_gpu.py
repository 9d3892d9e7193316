"""yume_attn_fwd_band on the device, one call per row of tests/attn_band_cases.py: EVERY output element finite and inside the per-element
bound against the fp64 masked reference (computed on the device), rows that see no key exactly 0 (exactly the old O under accumulate),
the guard rows and columns of O still the sentinel, a second launch equal in its bits; the calls whose window hides nothing equal in
their bits to the global call; and, from one child process with YUME_ATTN_LOG=1, the entry each call really took: `band` with the tile
counts the Python mirror of attn_band_plan::tile_range predicts, the ordinary `[attn_fwd]` line for the normalised calls."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attn_band_cases as bc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", bc.CASES, ids=[c.name for c in bc.CASES])
def test_every_element_inside_the_bound_empty_rows_exact_guards_intact_equal_bits_on_a_second_launch(c):
    ops = bc.make_band_case(c)
    r = bc.reference_band(c, ops, DEV)
    d = bc.run_band_case(c, ops)
    (g,), guards = bc.written(bc.as_case(c), d)
    assert torch.isfinite(g).all()                               # no NaN leaves the kernel (everything it must not read holds NaN)
    want = r["ref"] + r["base"]
    bnd = bc.bound(r)
    err = (g - want).abs()
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
    print(f"{c.name}: worst error / bound {ratio.reshape(-1)[worst].item():.3f} at (row, head, d) = {idx}: got {g[idx].item():.6g} "
          f"ref {want[idx].item():.6g}; {int((err > bnd).sum())} of {err.numel()} elements outside")
    assert int((err > bnd).sum()) == 0
    empty = bc.empty_rows(c).to(DEV)
    if c.acc:                                                    # the old O survives bit for bit
        assert torch.equal(g[empty], ops["base"].to(DEV).double().view(c.Lq, c.H, bc.D)[empty])
    else:
        assert bool((g[empty] == 0).all())
    assert bool((guards == bc.SENTINEL).all())                   # guard rows, guard columns
    first = d["obuf"].clone()
    d2 = bc.run_band_case(c, ops, None if c.acc else d)
    assert torch.equal(first, d2["obuf"])


@pytest.mark.parametrize("c", bc.NORMALISED, ids=[c.name for c in bc.NORMALISED])
def test_a_window_that_hides_nothing_is_the_global_call_bit_for_bit(c):
    ops = bc.make_band_case(c)
    a = bc.run_band_case(c, ops)
    b = bc.run_band_case(c, ops, window=False)
    assert torch.isfinite(a["o"].float()).all()
    assert torch.equal(a["obuf"], b["obuf"])


def test_every_call_takes_the_entry_and_walks_the_tiles_its_row_predicts():
    """YUME_ATTN_LOG is read once per process: a fresh child makes every call of both tables once"""
    env = dict(os.environ, YUME_ATTN_LOG="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_band_cases.py"), "--routes"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lines, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            lines[name] = []
        elif line.startswith("[attn_fwd") and name is not None:
            lines[name].append(line)
    print("\n".join(f"{c.name}: {' + '.join(lines.get(c.name, []))}" for c in bc.CASES + bc.NORMALISED))
    for c in bc.CASES:
        assert len(lines[c.name]) == 1 and lines[c.name][0].startswith("[attn_fwd_band] "), c.name
        route, kv = bc.band_log(lines[c.name][0])
        tmin, tmax = bc.tiles_min_max(c)
        assert route == "band", c.name
        assert (kv["q_pos0"], kv["left"], kv["right"], kv["tiles_min"], kv["tiles_max"], kv["Lq"], kv["Lk"], kv["H"]) == \
            (c.q_pos0, c.left, c.right, tmin, tmax, c.Lq, c.Lk, c.H), c.name
        assert (kv["prescaled"], kv["kv_padded"], kv["accumulate"]) == (int(c.prescaled), int(c.padded), int(c.acc)), c.name
    for c in bc.NORMALISED:
        assert len(lines[c.name]) == 1 and lines[c.name][0].startswith("[attn_fwd] "), c.name
        assert bc.ac.route_of(lines[c.name][0])[0] in bc.ac.ROUTES, c.name
