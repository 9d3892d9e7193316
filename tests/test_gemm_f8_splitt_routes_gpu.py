"""The e4m3 QKV GEMM, one call of the raw C-ABI per row of tests/gemm_f8_splitt_cases.py: EVERY element of both outputs (q | k row-major,
V as the K-major V^T image) inside the per-element bound against the fp64 reference, every guard value around both outputs untouched (`out`
columns >= n_split, `outT` columns M .. ldt - 1, a row behind each), the pattern rows bit-exact, a second launch equal in its bits — and,
from one child process with YUME_GEMM_LOG=1, the f8 kernel named with epi=4 and the row's ldt / n_split for every call."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_f8_splitt_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", sc.CASES, ids=[c.name for c in sc.CASES])
def test_every_element_of_both_outputs_inside_the_bound_and_every_guard_intact(c):
    ops = sc.make_case(c, DEV)
    r = sc.reference(c, ops)
    bufs = sc.run_case(c, ops)
    torch.cuda.synchronize()
    host = tuple(b.cpu() for b in bufs)
    got = sc.gather(c, host).double()
    ref = r["ref"]
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / sc.bound(c, r))
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
    print(f"{c.name}: worst error / bound {ratio.reshape(-1)[worst].item():.4f} at {idx}: got {got[idx].item():.6g} ref {ref[idx].item():.6g}; "
          f"{int((ratio > 1).sum())} of {ratio.numel()} elements outside; {sc.guards_damaged(c, host)} guards damaged")
    assert got.shape == (c.M, c.N) and torch.isfinite(got).all()
    assert int((ratio > 1).sum()) == 0
    assert sc.guards_damaged(c, host) == 0
    if c.pattern:
        assert torch.equal(got, ref.bfloat16().double())
    bufs2 = sc.run_case(c, ops)
    assert torch.equal(bufs[0], bufs2[0]) and torch.equal(bufs[1], bufs2[1])


def test_every_case_runs_on_the_f8_kernel_with_the_split_epilogue():
    """YUME_GEMM_LOG is read once per process: a fresh child makes every call of the table once and its log names the kernel."""
    env = dict(os.environ, YUME_GEMM_LOG="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_f8_splitt_cases.py"), "--routes"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = []
        elif line.startswith("[gemm_") and name is not None:
            seen[name].append(line)
    for c in sc.CASES:
        assert len(seen.get(c.name, [])) == 1, (c.name, seen.get(c.name))
        tag, kernel, *fields = seen[c.name][0].split()
        assert (tag, kernel) == ("[gemm_f8]", "f8")
        f = {k: int(v) for k, v in (t.split("=") for t in fields)}
        lda, ldw, ldo, ldt = sc.strides(c)
        assert f == {"M": c.M, "N": c.N, "K": c.K, "epi": 4, "lda": lda, "ldw": ldw, "ldo": ldo, "ldt": ldt, "n_split": c.n_split}, seen[c.name][0]


def test_ops_wrapper_runs_the_same_call_and_gemm_f8_still_refuses_the_epilogue():
    from yume_amd import ops
    c = next(c for c in sc.CASES if c.name == "n772_split512")
    o = sc.make_case(c, DEV)
    d = o["dev"]
    out, vt = sc.buffers(c, DEV)
    ops.gemm_f8_splitt(d["Aq"][:, :c.K], d["sa"], d["Wq"][:, :c.K], d["sw"], d["bias"], out, vt, c.n_split)
    torch.cuda.synchronize()
    r = sc.reference(c, o)
    host = (out.cpu(), vt.cpu())
    assert int(((sc.gather(c, host).double() - r["ref"]).abs() > sc.bound(c, r)).sum()) == 0 and sc.guards_damaged(c, host) == 0
    with pytest.raises(RuntimeError):
        ops.gemm_f8_splitt(d["Aq"][:, :c.K], d["sa"], d["Wq"][:, :c.K], d["sw"], d["bias"], out, vt, 128)
    with pytest.raises(RuntimeError):
        ops.gemm_f8(d["Aq"][:, :c.K], d["sa"], d["Wq"][:, :c.K], d["sw"], d["bias"], out, ops.EPI_BF16_SPLITT)
