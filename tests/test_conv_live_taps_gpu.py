"""The one-frame form of the causal 3x3x3 convolutions through the C-ABI, one 27-tap call and one (1,3,3) call per row of
tests/conv_live_taps_cases.py: EVERY element of both inside the bound of tests/conv_cases.py / tests/conv_f8_cases.py against the fp64
reference of the full 27-tap sum; the NaN the output held is gone and the guards are intact; a second launch gives equal bits; NaN
(0xFF bytes) in the dead weight columns of dt = 0, 1 does not reach the one-frame result; where the K tiles of the live tap fall on
the same boundaries (Cin % 64 == 0, f8 always) and the log names the same kernel, the two calls agree in their bits. From one child
process with YUME_CONV_LOG=1: the kernel family each call really ran on — conv_in and halo with k=1x3x3 (new in r24)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_cases as cc
import conv_f8_cases as f8
import conv_live_taps_cases as lt

pytestmark = pytest.mark.gpu
DEV = "cuda"

_ROUTES = {}


def routes():
    """{row: [(route, k) of the 27-tap call, (route, k) of the one-frame call]} — YUME_CONV_LOG is read once per process: a fresh child
    makes both calls of every row once (shared by the tests of this file)"""
    if not _ROUTES:
        env = dict(os.environ, YUME_CONV_LOG="1")
        p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_live_taps_cases.py"), "--routes"], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-4000:]
        name = None
        for line in p.stderr.splitlines():
            if line.startswith("CASE "):
                name = line.split()[1]
                _ROUTES[name] = []
            elif line.startswith("[conv3d_cl] ") and name is not None:
                _ROUTES[name].append(lt.parse_log(line))
    return _ROUTES


def _inside(name, got, ref, bnd):
    ratio = (got - ref).abs() / bnd
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
    print(f"{name}: worst error / bound {ratio.reshape(-1)[worst].item():.3f} at {idx}: got {got[idx].item():.6g} ref {ref[idx].item():.6g}; "
          f"{int((ratio > 1).sum())} of {ratio.numel()} elements outside")
    assert torch.isfinite(got).all(), name
    assert int((ratio > 1).sum()) == 0, name


@pytest.mark.parametrize("r", [r for r in lt.ROWS if r.kind == "bf16"], ids=[r.name for r in lt.ROWS if r.kind == "bf16"])
def test_bf16_row_both_calls_inside_the_bound_guards_equal_bits_dead_taps_poisoned(r):
    c = lt.case27(r)
    ops = cc.make_case(c, DEV)
    ref = cc.reference(c, ops, DEV)                         # the full 27-tap sum over the zero-padded input, fp64
    bnd = cc.bound(c, ref)
    w = ops["dev"]["w"]
    w1 = lt.live_weight(r, w)
    assert (w1.data_ptr() != w.data_ptr() and w1.stride(0) != w.stride(0)) == lt.uses_copy(r)          # the copy has rows of its own
    full = lt.run_bf16(r, ops, False, w)
    one = lt.run_bf16(r, ops, True, w1)
    for name, buf in (("27-tap", full), ("one-frame", one)):
        _inside(f"{r.name} {name}", buf[0, :, :, :r.cout].double(), ref["ref"][0], bnd[0])
        assert bool((buf[1] == lt.GUARD).all()) and bool((buf[..., r.cout:] == lt.GUARD).all()), name
    assert torch.equal(one, lt.run_bf16(r, ops, True, w1))
    # dead taps poisoned: NaN in the columns of dt = 0, 1 never reaches the one-frame call
    poison = lt.run_bf16(r, ops, True, lt.live_weight(r, lt.poisoned(r, w)))
    assert torch.isfinite(poison[0, :, :, :r.cout].float()).all()
    assert torch.equal(poison, one)
    seen = routes()[r.name]
    if lt.bit_equal_expected(r) and seen[0][0] == seen[1][0]:
        assert torch.equal(one, full), f"{r.name}: one-frame and 27-tap bits differ on {seen}"


@pytest.mark.parametrize("r", [r for r in lt.ROWS if r.kind == "f8"], ids=[r.name for r in lt.ROWS if r.kind == "f8"])
def test_f8_row_both_calls_inside_the_bound_guards_equal_bits_dead_taps_poisoned(r):
    c = lt.case27_f8(r)
    ops = f8.make_case(c, DEV)
    ref = f8.reference(c, ops)
    bnd = f8.bound(c, ref)
    wq = ops["dev"]["Wq"]
    full = lt.run_f8(r, ops, False, wq)
    one = lt.run_f8(r, ops, True, wq)
    for name, out in (("27-tap", full), ("one-frame", one)):
        _inside(f"{r.name} {name}", f8.gather(c, out).double().cpu(), ref["ref"], bnd)
        assert f8.guards_damaged(c, out) == 0, name
    assert torch.equal(one, lt.run_f8(r, ops, True, wq))
    poison = lt.run_f8(r, ops, True, lt.poisoned_f8(r, wq))
    assert torch.isfinite(f8.gather(c, poison).float()).all()
    assert torch.equal(poison, one)
    seen = routes()[r.name]
    if seen[0][0] == seen[1][0]:
        assert torch.equal(one, full), f"{r.name}: one-frame and 27-tap bits differ on {seen}"


def test_both_calls_of_every_row_run_on_the_family_the_row_names():
    """the one-frame call must land on the kernel family of the 27-tap call of the same layer; conv_in and halo refused k = (1,3,3) before
    r24 (the call fell to a gathering GEMM kernel)"""
    seen = routes()
    print("\n".join(f"{r.name}: {seen.get(r.name)}" for r in lt.ROWS))
    assert {r.name: [(r.route, "3x3x3"), (r.route, "1x3x3")] for r in lt.ROWS} == seen
