"""The MX pair on the device, one call of the raw C-ABI per row of tests/gemm_f8_mx_cases.py.
Consumer (yume_gemm_f8_mx): EVERY output element inside the per-element bound against the fp64 reference on the very bytes and scale bytes,
the guards around the stored region untouched, the two pattern rows bit-exact (a scale delivered to the wrong row or k-block changes the
integers), a second launch equal in its bits. Producer (yume_gemm_f8_mxout): every block's exponent admissible, every dequantised element
inside its bound, no NaN byte, the zero row with e = 0, bytes and scale bytes outside M / N untouched. The two chained reproduce the
fake-quantised product. One child process with YUME_GEMM_LOG=1 names the kernel of every call."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_f8_mx_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", mc.CASES, ids=[c.name for c in mc.CASES])
def test_consumer_every_element_inside_the_bound_guards_intact_equal_bits_on_a_second_launch(c):
    ops = mc.make_case(c, DEV)
    r = mc.reference(c, ops)
    bufs = mc.run_case(c, ops)
    torch.cuda.synchronize()
    got = mc.gather(c, bufs).double().cpu()
    ref = r["ref"]
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / mc.bound(c, r))
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
    print(f"{c.name}: worst error / bound {ratio.reshape(-1)[worst].item():.4f} at {idx}: got {got[idx].item():.6g} ref {ref[idx].item():.6g}; "
          f"{int((ratio > 1).sum())} of {ratio.numel()} elements outside; {int((err != 0).sum())} differ at all")
    assert torch.isfinite(got).all()
    assert int((ratio > 1).sum()) == 0
    assert mc.guards_damaged(bufs) == 0
    if c.pattern:
        assert torch.equal(got, ref)
    bufs2 = mc.run_case(c, ops)
    assert torch.equal(bufs["out"][0], bufs2["out"][0])


@pytest.mark.parametrize("c", mc.PCASES, ids=[c.name for c in mc.PCASES])
def test_producer_every_exponent_admissible_every_element_inside_nothing_written_outside(c):
    ops = mc.make_pcase(c, DEV)
    r = mc.preference(c, ops)
    q, eb = mc.run_pcase(c, ops)
    torch.cuda.synchronize()
    q, eb = q.cpu(), eb.cpu()
    nb = c.N // 32
    got = mc.check_producer(c, r, q[:c.M, :c.N].contiguous(), eb[:c.M, :nb].contiguous())
    print(f"{c.name}: {got}; scale bytes {int(eb[:c.M, :nb].min())} .. {int(eb[:c.M, :nb].max())}")
    assert got == {"exp_bad": 0, "val_bad": 0, "nan": 0}
    assert (q[c.M:] == mc.GUARD_BYTE).all() and (q[:, c.N:] == mc.GUARD_BYTE).all()
    assert (eb[c.M:] == mc.GUARD_BYTE).all() and (eb[:, nb:] == mc.GUARD_BYTE).all()
    if c.zero_row is not None:
        assert (eb[c.zero_row, :nb] == 127).all() and not (q[c.zero_row, :c.N] & 0x7f).any()
    q2, eb2 = mc.run_pcase(c, ops)
    assert torch.equal(q2.cpu(), q) and torch.equal(eb2.cpu(), eb)


def test_producer_into_consumer_through_the_ops_wrappers():
    """ffn.0 -> ffn.2 as the engine chains them: the consumer, fed the producer's own bytes and scale bytes, is held to ITS bound against the
    fp64 product of exactly those bytes"""
    from yume_amd import ops as yops
    g = torch.Generator().manual_seed(16)
    M, C, Fd = 130, 256, 512
    import gemm_f8_cases as fc
    _, hq = fc.e4m3_exact(torch.randn(M, C, generator=g))
    _, w1 = fc.e4m3_exact(torch.randn(Fd, C, generator=g) * C ** -0.5)
    W2, w2 = fc.e4m3_exact(torch.randn(C, Fd, generator=g) * Fd ** -0.5)
    sh, s1, s2 = torch.rand(M, generator=g) + 0.5, torch.rand(Fd, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5
    b1, b2 = torch.randn(Fd, generator=g), torch.randn(C, generator=g)
    fq = torch.empty(M, Fd, dtype=torch.uint8, device=DEV)
    fe = torch.empty(M, 16, dtype=torch.uint8, device=DEV)
    yops.gemm_f8_mxout(hq.to(DEV), sh.to(DEV), w1.to(DEV), s1.to(DEV), b1.to(DEV), fq, fe)
    out = torch.zeros(M, C, dtype=torch.float32, device=DEV)
    yops.gemm_f8_mx(fq, fe, w2.to(DEV), s2.to(DEV), b2.to(DEV), out, mc.EPI_F32)
    A = fq.cpu().view(torch.float8_e4m3fn).double() * mc.block_scale(fe.cpu(), Fd)
    y = (A @ W2.double().t()) * s2.double().view(1, -1)
    Q = ((A * A) @ (W2.double() ** 2).t()) * (s2.double() ** 2).view(1, -1)
    bnd = mc.C_SUM_MX * Q.sqrt() + 2.0 ** -21 * (y + b2.double()).abs() + 2.0 ** -22 * b2.double().abs()
    assert int(((out.double().cpu() - (y + b2.double())).abs() > bnd).sum()) == 0
    with pytest.raises(RuntimeError):
        yops.gemm_f8_mx(fq, fe[:, :8], w2.to(DEV), s2.to(DEV), b2.to(DEV), out, mc.EPI_F32)


def test_every_case_runs_on_its_kernel():
    """YUME_GEMM_LOG is read once per process: a fresh child makes every call of both tables once and its log names the kernel."""
    env = dict(os.environ, YUME_GEMM_LOG="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_f8_mx_cases.py"), "--routes"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = []
        elif line.startswith("[gemm_") and name is not None:
            seen[name].append(line)
    for c in mc.CASES:
        assert len(seen.get(c.name, [])) == 1, (c.name, seen.get(c.name))
        tag, kernel, *fields = seen[c.name][0].split()
        assert (tag, kernel) == ("[gemm_f8]", "mx")
        f = {k: int(v) for k, v in (t.split("=") for t in fields)}
        lda, ldw, ldo, ldea = mc.strides(c)
        assert f == {"M": c.M, "N": c.N, "K": c.K, "epi": c.epi, "lda": lda, "ldea": ldea, "ldw": ldw, "ldo": ldo}, seen[c.name][0]
    for c in mc.PCASES:
        assert len(seen.get(c.name, [])) == 1, (c.name, seen.get(c.name))
        tag, kernel, *fields = seen[c.name][0].split()
        assert (tag, kernel) == ("[gemm_f8]", "f8")
        f = {k: int(v) for k, v in (t.split("=") for t in fields)}
        lda, ldw, ldo, ldeo = mc.pstrides(c)
        assert f == {"M": c.M, "N": c.N, "K": c.K, "epi": mc.EPI_MX_GELU, "lda": lda, "ldw": ldw, "ldo": ldo, "ldeo": ldeo}, seen[c.name][0]
