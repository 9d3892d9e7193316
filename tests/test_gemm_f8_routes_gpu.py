"""Every shape edge, epilogue and scale layout of the e4m3 GEMM, one call of the raw C-ABI per row of tests/gemm_f8_cases.py: EVERY output
element inside the per-element bound against the fp64 reference, every guard element around the stored [M, N] region untouched, the pattern
rows bit-exact (the instruction's operand map, established with exact integers), a second launch equal in its bits — and, from one child
process with YUME_GEMM_LOG=1, the f8 kernel named for every call."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_f8_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", fc.CASES, ids=[c.name for c in fc.CASES])
def test_every_element_inside_the_bound_guards_intact_equal_bits_on_a_second_launch(c):
    ops = fc.make_case(c, DEV)
    r = fc.reference(c, ops)
    bufs = fc.run_case(c, ops)
    torch.cuda.synchronize()
    got = fc.gather(c, bufs).double().cpu()
    ref = r["ref"]
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / fc.bound(c, r))
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
    print(f"{c.name}: worst error / bound {ratio.reshape(-1)[worst].item():.4f} at {idx}: got {got[idx].item():.6g} ref {ref[idx].item():.6g}; "
          f"{int((ratio > 1).sum())} of {ratio.numel()} elements outside")
    assert torch.isfinite(got).all()
    assert int((ratio > 1).sum()) == 0
    assert fc.guards_damaged(bufs) == 0
    if c.pattern:
        assert torch.equal(got, ref)
    bufs2 = fc.run_case(c, ops)
    assert torch.equal(bufs["out"][0], bufs2["out"][0])


def test_every_case_runs_on_the_f8_kernel():
    """YUME_GEMM_LOG is read once per process: a fresh child makes every call of the table once and its log names the kernel."""
    env = dict(os.environ, YUME_GEMM_LOG="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_f8_cases.py"), "--routes"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = []
        elif line.startswith("[gemm_") and name is not None:
            seen[name].append(line)
    for c in fc.CASES:
        assert len(seen.get(c.name, [])) == 1, (c.name, seen.get(c.name))
        tag, kernel, *fields = seen[c.name][0].split()
        assert (tag, kernel) == ("[gemm_f8]", "f8")
        f = {k: int(v) for k, v in (t.split("=") for t in fields)}
        lda, ldw, ldo = fc.strides(c)
        assert f == {"M": c.M, "N": c.N, "K": c.K, "epi": c.epi, "lda": lda, "ldw": ldw, "ldo": ldo}, seen[c.name][0]


def test_ops_wrapper_runs_the_same_call():
    from yume_amd import ops
    c = next(c for c in fc.CASES if c.name == "n516_gelu")
    o = fc.make_case(c, DEV)
    d = o["dev"]
    out = torch.empty(c.M, c.N, dtype=torch.bfloat16, device=DEV)
    ops.gemm_f8(d["Aq"][:, :c.K], d["sa"], d["Wq"][:, :c.K], d["sw"], d["bias"], out, fc.EPI_GELU)
    r = fc.reference(c, o)
    assert int(((out.double().cpu() - r["ref"]).abs() > fc.bound(c, r)).sum()) == 0
    with pytest.raises(RuntimeError):
        ops.gemm_f8(d["Aq"][:, :c.K], d["sa"][:-1], d["Wq"][:, :c.K], d["sw"], d["bias"], out, fc.EPI_GELU)
