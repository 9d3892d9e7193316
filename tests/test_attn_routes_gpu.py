"""Every kernel route behind yume_attn_fwd / _ws / _kw / _seg, one call per row of tests/attn_cases.py: EVERY output element finite and
inside the per-element bound against the fp64 reference (computed on the device), the guard rows, guard columns and pitch gaps of O still
the sentinel, a second launch equal in its bits — and, from one child process with YUME_ATTN_LOG=1, the kernel and the plan each of these
calls really ran on."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", ac.CASES, ids=[c.name for c in ac.CASES])
def test_every_element_inside_the_bound_guards_intact_equal_bits_on_a_second_launch(c):
    ops = ac.make_case(c)
    rs = ac.reference(c, ops, DEV)
    d = ac.run_case(c, ops)
    got, guards = ac.written(c, d)
    outside = 0
    for s, (g, r) in enumerate(zip(got, rs)):
        ratio = (g - (r["ref"] + r["base"])).abs() / ac.bound(r)
        ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float("inf")))
        worst = int(ratio.argmax())
        idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
        outside += int((ratio > 1).sum())
        print(f"{c.name} segment {s}: worst error / bound {ratio.reshape(-1)[worst].item():.3f} at (row, head, d) = {idx}: got {g[idx].item():.6g} "
              f"ref {(r['ref'] + r['base'])[idx].item():.6g}; {int((ratio > 1).sum())} of {ratio.numel()} elements outside")
        assert torch.isfinite(g).all()
    assert outside == 0
    assert bool((guards == ac.SENTINEL).all())                  # guard rows, guard columns, pitch gaps
    first = d["obuf"].clone()
    if c.acc:                                                    # (an accumulate call reads O: the second launch starts from the same old O)
        d = None
    d2 = ac.run_case(c, ops, d)
    assert torch.equal(first, d2["obuf"])


def test_every_case_runs_on_the_kernel_and_the_plan_its_row_names():
    """YUME_ATTN_LOG is read once per process: a fresh child makes every call of the table once (it registers the counter workspace the
    persistent kernel draws its tickets from) and its log names the kernels."""
    env = dict(os.environ, YUME_ATTN_LOG="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_cases.py"), "--routes"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, lines, name = {}, {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name], lines[name] = [], []
        elif line.startswith(("[attn_fwd] ", "[attn_fwd_seg] ")) and name is not None:
            seen[name].append(ac.route_of(line))
            lines[name].append(line)
    print("\n".join(f"{c.name}: {' + '.join(lines.get(c.name, []))}" for c in ac.CASES))
    assert {c.name: [(c.route, c.plan)] for c in ac.CASES} == seen
