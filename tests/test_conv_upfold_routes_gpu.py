"""yume_conv_up2_fold, one call per row of tests/conv_upfold_cases.py: EVERY output element finite and inside the per-element bound against
the fp64 4-tap reference on the folded bytes (computed on the device, oracle/devgold.py conv_taps; the pattern rows bit-exact), the guard
frames and the guard columns untouched, a second launch equal in its bits — and, from one child process with YUME_CONV_LOG=1, the `w4fold`
line of each of these calls. Fails without the feature: the export does not exist."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_upfold_cases as cu

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", cu.CASES, ids=[c.name for c in cu.CASES])
def test_every_element_inside_the_bound_guards_intact_equal_bits_on_a_second_launch(c):
    ops = cu.make_case(c, DEV)
    r = cu.reference(c, ops, DEV)
    buf = cu.run_case(c, ops)
    got = buf[1:c.t + 1, :, :, :c.cout].double()
    assert torch.isfinite(got).all()                                           # every in-range element was written (NaN before the call)
    if c.pattern:
        bad = got != r["ref"]
        idx = tuple(int(i) for i in np.unravel_index(int(bad.int().argmax()), tuple(bad.shape)))
        print(f"{c.name}: {int(bad.sum())} of {bad.numel()} elements differ; first at (t, y, x, c) = {idx}: got {got[idx].item():.6g} ref {r['ref'][idx].item():.6g}")
        assert int(bad.sum()) == 0
    else:
        ratio = (got - r["ref"]).abs() / cu.bound(c, r)
        worst = int(ratio.argmax())
        idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
        print(f"{c.name}: worst error / bound {ratio.reshape(-1)[worst].item():.3f} at (t, y, x, c) = {idx}: got {got[idx].item():.6g} "
              f"ref {r['ref'][idx].item():.6g}; {int((ratio > 1).sum())} of {ratio.numel()} elements outside")
        assert int((ratio > 1).sum()) == 0
    assert bool((buf[0] == cu.GUARD).all()) and bool((buf[c.t + 1] == cu.GUARD).all())       # the frames around the written ones
    assert bool((buf[..., c.cout:] == cu.GUARD).all())                                        # the columns [Cout, ldo)
    buf2 = cu.run_case(c, ops)
    assert torch.equal(buf.view(torch.int16), buf2.view(torch.int16))


def test_every_call_of_the_table_logs_w4fold_with_its_shape():
    """YUME_CONV_LOG is read once per process: a fresh child makes every call of the table once"""
    env = dict(os.environ, YUME_CONV_LOG="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_upfold_cases.py"), "--routes"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = []
        elif line.startswith("[conv3d_cl] ") and name is not None:
            seen[name].append(line.split(None, 1)[1])
    print("\n".join(f"{k}: {v}" for k, v in seen.items()))
    want = {}
    for c in cu.CASES:
        tiles = c.t * 4 * ((c.hin * c.win + 255) // 256) * ((c.cout + 255) // 256)
        want[c.name] = [f"w4fold T={c.t} Hin={c.hin} Win={c.win} Cin={c.cin} Cout={c.cout} tiles={tiles}"]
    assert seen == want
