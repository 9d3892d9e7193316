"""yume_attn_fwd_f8mx and its two quantisers on the device, one call per row of tests/attn_f8_cases.py: EVERY output element finite and inside
the per-element bound against the fp64 reference on the very bytes the call got, the two pattern rows bit for bit, the guard rows and columns
of O still the sentinel, no NaN of the pre-fill left, a second launch equal in its bits; both quantisers bit-equal to the host MX quantiser,
their guards untouched; and, from one child process with YUME_ATTN_LOG=1 / YUME_NORM_LOG=1, the launch each call really made."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attn_f8_cases as fc
import conv_f8_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", fc.CASES, ids=[c.name for c in fc.CASES])
def test_every_element_inside_the_bound_guards_intact_equal_bits_on_a_second_launch(c):
    ops = fc.make_case(c)
    r = fc.reference(c, ops, DEV)
    dv = fc.run_case(c, ops)
    got, guards = fc.written(c, dv)
    assert torch.isfinite(got).all()                               # no NaN of the pre-fill left, nothing from a NaN byte
    ratio = (got - r["ref"]).abs() / fc.bound(r)
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
    print(f"{c.name}: worst error / bound {ratio.reshape(-1)[worst].item():.3f} at (row, head, d) = {idx}: got {got[idx].item():.6g} "
          f"ref {r['ref'][idx].item():.6g}; {int((ratio > 1).sum())} of {ratio.numel()} elements outside")
    assert int((ratio > 1).sum()) == 0
    if c.pattern == "pattern":
        want = fc.emulate(c, ops).to(DEV)
        print(f"{c.name}: {int((got != want).sum())} of {got.numel()} elements differ from the exact value")
        assert torch.equal(got, want)
    assert bool((guards == fc.SENTINEL).all())
    first = dv["obuf"].clone()
    dv2 = fc.run_case(c, ops, dv)
    assert torch.equal(first, dv2["obuf"])


@pytest.mark.parametrize("c", fc.QCASES, ids=[c.name for c in fc.QCASES])
def test_row_quantiser_is_bit_equal_to_the_host_mx_quantiser(c):
    x, q, e = fc.run_qcase(c)
    wq, we = cc.mx_quantise(x)
    assert torch.equal(q[:c.R, :c.K], wq) and torch.equal(e[:c.R, :c.K // 32], we)
    assert bool((q[c.R:] == fc.GUARD_BYTE).all()) and bool((q[:, c.K:] == fc.GUARD_BYTE).all())
    assert bool((e[c.R:] == fc.GUARD_BYTE).all()) and bool((e[:, c.K // 32:] == fc.GUARD_BYTE).all())
    assert int(we.max()) == 247 and not bool((wq & 0x7F == 0x7F).any())      # a block holding the largest bf16, no NaN byte
    assert c.R <= 2 or bool(((we == 127) & (wq.view(c.R, c.K // 32, 32) == 0).all(dim=2)).any())            # an all-zero block (rows > 2 carry one)


@pytest.mark.parametrize("c", fc.VCASES, ids=[c.name for c in fc.VCASES])
def test_vt_quantiser_is_bit_equal_to_the_host_through_vt8_offsets(c):
    vt, vt8, ev = fc.run_vcase(c)
    C, T = c.H * 128, fc.tiles(c.Lk)
    w8, wev = fc.vt_mx_quantise(vt, c.Lk)
    assert torch.equal(vt8[:C, :128 * T], w8) and torch.equal(ev[:T, :4 * C], wev)
    assert bool((vt8[:C, :128 * T][:, fc.vt8_offsets(c.Lk) >= c.Lk] == 0).all())                            # keys >= Lk: byte 0x00
    assert bool((vt8[C:] == fc.GUARD_BYTE).all()) and bool((vt8[:, 128 * T:] == fc.GUARD_BYTE).all())
    assert bool((ev[T:] == fc.GUARD_BYTE).all()) and bool((ev[:, 4 * C:] == fc.GUARD_BYTE).all())


def test_every_call_logs_the_launch_its_row_names():
    """YUME_ATTN_LOG and YUME_NORM_LOG are read once per process: a fresh child makes every call of the tables once"""
    env = dict(os.environ, YUME_ATTN_LOG="1", YUME_NORM_LOG="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_f8_cases.py"), "--routes"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = []
        elif line.startswith(("[attn] ", "[quant] ", "[attn_fwd")) and name is not None:
            seen[name].append(line.strip())
    want = {c.name: [f"[attn] f8mx Lq={c.Lq} Lk={c.Lk} H={c.H} tiles={fc.tiles(c.Lk)}"] for c in fc.CASES}
    for c in fc.QCASES:
        want[c.name] = [f"[quant] rows_mx R={c.R} K={c.K} ldx={c.K + c.ldx_x} ldq={c.K + c.ldq_x} lde={c.K // 32 + c.lde_x}"]
    for c in fc.VCASES:
        T = fc.tiles(c.Lk)
        want[c.name] = [f"[quant] vt_mx C={c.H * 128} Lk={c.Lk} tiles={T} ldvt={(c.Lk + c.ldvt_x + 3) // 4 * 4} ldvt8={128 * T + c.ldvt8_x} "
                        f"ldev={512 * c.H + c.ldev_x}"]
    assert want == seen
