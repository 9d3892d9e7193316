"""Every shape edge, epilogue and scale layout of the int8 GEMM, one call of the raw C-ABI per row of tests/gemm_i8_cases.py (yume_gemm_i8 and
yume_gemm_i8_splitt): EVERY output element inside the per-element bound against the fp64 reference, the exact rows (F32, unit scales, no
bias: the pattern rows and the saturated one) equal to the host's integer product bit for bit, every guard element around the stored
regions untouched and no NaN of the pre-fill left where the call has to store, a second launch equal in its bits — and, from one child
process with YUME_GEMM_LOG=1, the i8 kernel named for every call."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_i8_cases as ic

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", ic.CASES, ids=[c.name for c in ic.CASES])
def test_every_element_inside_the_bound_guards_intact_equal_bits_on_a_second_launch(c):
    ops = ic.make_case(c, DEV)
    r = ic.reference(c, ops)
    bufs = ic.run_case(c, ops)
    torch.cuda.synchronize()
    host = tuple(b.cpu() if b is not None else None for b in bufs)
    got = ic.gather(c, host).double()
    ref = r["ref"]
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / ic.bound(c, r))
    worst = int(torch.nan_to_num(ratio, nan=float("inf")).argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
    print(f"{c.name}: worst error / bound {ratio.reshape(-1)[worst].item():.4f} at {idx}: got {got[idx].item():.9g} ref {ref[idx].item():.9g}; "
          f"{int((ratio > 1).sum())} of {ratio.numel()} elements outside; {ic.guards_damaged(c, host)} guards damaged")
    assert got.shape == (c.M, c.N) and torch.isfinite(got).all()
    assert int((ratio > 1).sum()) == 0
    assert ic.guards_damaged(c, host) == 0
    if ic.exact(c):
        want = r["acc"].float()
        print(f"{c.name}: {int((got.float() != want).sum())} elements differ from fp32(acc); max |acc| = {r['acc'].abs().max().item():.0f}")
        assert torch.equal(got.float(), want)
    if c.pattern and ic.is_splitt(c):
        assert torch.equal(got, ref.bfloat16().double())
    assert ic.violations(c, got.float(), r) == 0
    bufs2 = ic.run_case(c, ops)
    assert torch.equal(ic.gather(c, bufs), ic.gather(c, bufs2))


def test_every_case_runs_on_the_i8_kernel():
    """YUME_GEMM_LOG is read once per process: a fresh child makes every call of the table once and its log names the kernel."""
    env = dict(os.environ, YUME_GEMM_LOG="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_i8_cases.py"), "--routes"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = []
        elif line.startswith("[gemm_") and name is not None:
            seen[name].append(line)
    for c in ic.CASES:
        assert len(seen.get(c.name, [])) == 1, (c.name, seen.get(c.name))
        tag, kernel, *fields = seen[c.name][0].split()
        assert (tag, kernel) == ("[gemm_i8]", "i8")
        f = {k: int(v) for k, v in (t.split("=") for t in fields)}
        lda, ldw, ldo, ldt = ic.strides(c)
        want = {"M": c.M, "N": c.N, "K": c.K, "epi": c.epi, "lda": lda, "ldw": ldw, "ldo": ldo}
        if ic.is_splitt(c):
            want.update(ldt=ldt, n_split=c.n_split)
        assert f == want, seen[c.name][0]


def test_ops_wrappers_run_the_same_calls():
    from yume_amd import ops
    c = next(c for c in ic.CASES if c.name == "n516_bf16")
    o = ic.make_case(c, DEV)
    d = o["dev"]
    out = torch.empty(c.M, c.N, dtype=torch.bfloat16, device=DEV)
    ops.gemm_i8(d["Aq"][:, :c.K], d["sa"], d["Wq"][:, :c.K], d["sw"], d["bias"], out, ic.EPI_BF16)
    r = ic.reference(c, o)
    assert ic.violations(c, out.float().cpu(), r) == 0
    with pytest.raises(RuntimeError):
        ops.gemm_i8(d["Aq"][:, :c.K], d["sa"][:-1], d["Wq"][:, :c.K], d["sw"], d["bias"], out, ic.EPI_BF16)
    with pytest.raises(RuntimeError):
        ops.gemm_i8(d["Aq"][:, :c.K], d["sa"], d["Wq"][:, :c.K], d["sw"], d["bias"], out, ops.EPI_BF16_SPLITT)
    # uint8 views of the same bytes are read as signed bytes too
    out2 = torch.empty_like(out)
    ops.gemm_i8(d["Aq"][:, :c.K].view(torch.uint8), d["sa"], d["Wq"][:, :c.K].view(torch.uint8), d["sw"], d["bias"], out2, ic.EPI_BF16)
    assert torch.equal(out, out2)

    c = next(c for c in ic.CASES if c.name == "splitt_n772_split512")
    o = ic.make_case(c, DEV)
    d = o["dev"]
    out, vt = ic.buffers(c, DEV)
    ops.gemm_i8_splitt(d["Aq"][:, :c.K], d["sa"], d["Wq"][:, :c.K], d["sw"], d["bias"], out, vt, c.n_split)
    torch.cuda.synchronize()
    r = ic.reference(c, o)
    host = (out.cpu(), vt.cpu())
    assert ic.violations(c, ic.gather(c, host).float(), r) == 0 and ic.guards_damaged(c, host) == 0
    assert torch.isfinite(ic.gather(c, host).float()).all()
    with pytest.raises(RuntimeError):
        ops.gemm_i8_splitt(d["Aq"][:, :c.K], d["sa"], d["Wq"][:, :c.K], d["sw"], d["bias"], out, vt, 128)
