"""yume_attn_fwd_batch on the GPU, one call per row of tests/attn_batch_cases.py and input pattern: EVERY output element of every segment
finite and inside tests/attn_cases.py's per-element bound (KAPPA 4.5, no new tolerance) against its fp64 reference, the guard rows, guard
columns and pitch gaps of O still the sentinel — and the properties of a batch launch: equal bits run to run, every segment equal in its bits
to ops.attn_fwd(variant=8) on its views where both launches carry the same plan, no segment's bits depending on another segment's operands,
the ticket counters back at zero, one segment being the plain call. The kernels and the plans come from one child process with
YUME_ATTN_LOG=1."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attn_batch_cases as bc
import attn_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"
_memo = {}


def _case(c, pattern):
    """(operands, fp64 references): computed once per (case, pattern), shared and left unchanged"""
    key = (c.name, pattern)
    if key not in _memo:
        case = bc.as_case(c, pattern)
        ops = ac.make_case(case)
        _memo.clear()                       # (one case's references at a time: the large rows are 0.2 GB each)
        _memo[key] = (ops, ac.reference(case, ops, DEV))
    return _memo[key]


@pytest.fixture(scope="module")
def routes():
    """{case name: [(route, plan) of the batch call, then of the variant-8 call on each segment's views]}"""
    env = dict(os.environ, YUME_ATTN_LOG="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_batch_cases.py"), "--routes"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = []
        elif line.startswith(("[attn_fwd_batch] ", "[attn_fwd] ")) and name is not None:
            seen[name].append((ac.route_of(line), line))
    print("\n".join(f"{n}: {' | '.join(l for _, l in v)}" for n, v in seen.items()))
    return {n: [r for r, _ in v] for n, v in seen.items()}


@pytest.mark.parametrize("pattern", bc.PATTERNS)
@pytest.mark.parametrize("c", bc.TABLE, ids=[c.name for c in bc.TABLE])
def test_every_element_of_every_segment_inside_the_bound_and_nothing_else_written(c, pattern):
    _inside_the_bound(c, pattern)


@pytest.mark.parametrize("c", bc.RERUN_CASES, ids=[c.name for c in bc.RERUN_CASES])
def test_the_rerun_on_the_robust_body_stays_in_its_segment(c):
    """every item leaves the base-free range and is redone cold: the same bound, in every segment, and equal bits on a second launch"""
    d = _inside_the_bound(c, "stairs")
    ops, _ = _case(c, "stairs")
    assert torch.equal(d["obuf"], bc.run_batch(c, bc.device_operands(c, ops))["obuf"])


def _inside_the_bound(c, pattern):
    ops, rs = _case(c, pattern)
    d = bc.run_batch(c, bc.device_operands(c, ops))
    outside = 0
    for s, (g, r) in enumerate(zip(bc.results(c, d), rs)):
        ratio = (g - (r["ref"] + r["base"])).abs() / ac.bound(r)
        ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float("inf")))
        worst = int(ratio.argmax())
        idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
        outside += int((ratio > 1).sum())
        print(f"{c.name} {pattern} segment {s}: worst error / bound {ratio.reshape(-1)[worst].item():.3f} at (row, head, d) = {idx}: "
              f"got {g[idx].item():.6g} ref {(r['ref'] + r['base'])[idx].item():.6g}; {int((ratio > 1).sum())} of {ratio.numel()} elements outside")
        assert torch.isfinite(g).all()
    assert outside == 0
    assert bool((bc.untouched(c, d) == ac.SENTINEL).all())
    return d


def test_every_case_runs_on_the_kernel_and_the_plan_its_row_names(routes):
    for c in bc.TABLE:
        route, plan = routes[c.name][0]
        assert route == c.route, (c.name, routes[c.name])
        if c.plan is not None:
            assert plan == c.plan, (c.name, plan)
        if c.route == "batch_v8":
            assert [r for r, _ in routes[c.name][1:]] == ["v8"] * c.nseg


@pytest.mark.parametrize("c", bc.PROPERTY_CASES, ids=[c.name for c in bc.PROPERTY_CASES])
def test_batch_launch_properties(c, routes):
    from yume_amd import ops as yops
    ops, _ = _case(c, "random")
    fresh = lambda: bc.device_operands(c, ops)
    d = bc.run_batch(c, fresh())
    first = d["obuf"].clone()
    # ---- run to run
    assert torch.equal(first, bc.run_batch(c, fresh())["obuf"])
    # ---- the ticket counters are back at zero
    torch.cuda.synchronize()
    assert int(yops.ensure_counters(d["q"].device).abs().max()) == 0
    # ---- every segment against the plain persistent launch on its views, where the two carry the same plan
    same_plan = [s for s in range(c.nseg) if routes[c.name][1 + s] == ("v8", routes[c.name][0][1])]
    if c.plan == (2, 1):
        assert same_plan == list(range(c.nseg))            # whole blocks only: always
    print(f"{c.name}: batch plan {routes[c.name][0][1]}, single-launch plans {[p for _, p in routes[c.name][1:]]}")
    single = fresh()
    for s in same_plan:
        bc.run_single(c, single, s)
    got, ref = bc.results(c, d), bc.results(c, single)
    for s in same_plan:
        assert torch.equal(got[s], ref[s]), f"segment {s} differs from ops.attn_fwd(variant=8) on its views"
    # ---- no segment's bits depend on another segment's operands
    for changed in (c.nseg - 1, 0):
        other = fresh()
        sl_q = slice(changed * c.q_pitch, changed * c.q_pitch + c.Lq)
        sl_k = slice(changed * c.k_pitch, changed * c.k_pitch + c.Lk)
        other["q"][sl_q] = other["q"][sl_q].flip(0)
        other["k"][sl_k] = other["k"][sl_k].flip(0) * 0.5
        other["vt"][:, sl_k] = other["vt"][:, sl_k] + 1.0
        res = bc.results(c, bc.run_batch(c, other))
        for s in range(c.nseg):
            assert torch.equal(res[s], got[s]) == (s != changed), (changed, s)
    # ---- one segment is the plain call
    one, plain = fresh(), fresh()
    bc.run_batch(c, one, nseg=1)
    bc.run_single(c, plain, 0, variant=c.variant)
    assert torch.equal(one["obuf"], plain["obuf"])
