"""Every kernel route behind yume_conv3d_cl, one call per row of tests/conv_cases.py: EVERY output element inside the per-element bound
against the fp64 reference (computed on the device, oracle/devgold.py conv_taps), the guard frame and the guard channels untouched, a
second launch equal in its bits — and, from one child process with YUME_CONV_LOG=1, the kernel each of these calls really ran on."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", cc.CASES, ids=[c.name for c in cc.CASES])
def test_every_element_inside_the_bound_guards_intact_equal_bits_on_a_second_launch(c):
    ops = cc.make_case(c, DEV)
    r = cc.reference(c, ops, DEV)
    buf, t0 = cc.run_case(c, ops)
    fr, ho, wo, ch = cc.stored_shape(c)
    got = buf[t0:t0 + fr, :, :, :ch].double()
    ratio = (got - r["ref"]).abs() / cc.bound(c, r)
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
    print(f"{c.name}: worst error / bound {ratio.reshape(-1)[worst].item():.3f} at (t, h, w, c) = {idx}: got {got[idx].item():.6g} "
          f"ref {r['ref'][idx].item():.6g}; {int((ratio > 1).sum())} of {ratio.numel()} elements outside")
    assert torch.isfinite(got).all()
    assert int((ratio > 1).sum()) == 0
    assert bool((buf[:t0] == cc.GUARD).all()) and bool((buf[t0 + fr:] == cc.GUARD).all())          # the frames around the written ones
    assert bool((buf[..., ch:] == cc.GUARD).all())                                                  # the channel padding of a row
    buf2, _ = cc.run_case(c, ops)
    assert torch.equal(buf, buf2)


def test_every_case_runs_on_the_kernel_its_row_names():
    """YUME_CONV_LOG is read once per process: a fresh child makes every call of the table once and its log names the kernels."""
    env = dict(os.environ, YUME_CONV_LOG="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_cases.py"), "--routes"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = []
        elif line.startswith("[conv3d_cl] ") and name is not None:
            seen[name].append(cc.route_of(line))
    print("\n".join(f"{c.name}: {' + '.join(seen.get(c.name, []))}" for c in cc.CASES))
    assert {c.name: [c.route] for c in cc.CASES} == seen
