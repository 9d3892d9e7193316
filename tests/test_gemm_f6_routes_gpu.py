"""The MXFP6 pair on the device, one call of the raw C-ABI per row of tests/gemm_f6_cases.py.
Consumer (yume_gemm_f6_mx): EVERY output element inside the per-element bound against the fp64 reference on the very bytes and scale bytes,
the guards around the stored region untouched (GUARD pre-filled), the two pattern rows bit-exact (a scale from the wrong row, k-block or
operand, or a wrong bit order, changes the integers), a second launch equal in its bits. Producer (yume_gemm_f6_mxout): every block's exponent
admissible, every dequantised element inside its bound, the zero row with e = 0 and zero codes, bytes and scale bytes outside M / N
untouched. The two chained through the ops wrappers reproduce the product of the producer's own bytes. One child process with
YUME_GEMM_LOG=1 names the kernel of every call."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_f6_cases as f6

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", f6.CASES, ids=[c.name for c in f6.CASES])
def test_consumer_every_element_inside_the_bound_guards_intact_equal_bits_on_a_second_launch(c):
    ops = f6.make_case(c, DEV)
    r = f6.reference(c, ops)
    bufs = f6.run_case(c, ops)
    torch.cuda.synchronize()
    got = f6.gather(c, bufs).double().cpu()
    ref = r["ref"]
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / f6.bound(c, r))
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
    print(f"{c.name}: worst error / bound {ratio.reshape(-1)[worst].item():.4f} at {idx}: got {got[idx].item():.6g} ref {ref[idx].item():.6g}; "
          f"{int((ratio > 1).sum())} of {ratio.numel()} elements outside; {int((err != 0).sum())} differ at all")
    assert torch.isfinite(got).all()
    assert int((ratio > 1).sum()) == 0
    assert f6.guards_damaged(bufs) == 0
    if c.pattern:
        assert torch.equal(got, ref)
    bufs2 = f6.run_case(c, ops)
    assert torch.equal(bufs["out"][0], bufs2["out"][0])


@pytest.mark.parametrize("c", f6.PCASES, ids=[c.name for c in f6.PCASES])
def test_producer_every_exponent_admissible_every_element_inside_nothing_written_outside(c):
    ops = f6.make_pcase(c, DEV)
    r = f6.preference(c, ops)
    q, eb = f6.run_pcase(c, ops)
    torch.cuda.synchronize()
    q, eb = q.cpu(), eb.cpu()
    nb, nq = c.N // 32, 3 * c.N // 4
    codes = f6.mx6_unpack_bits(q[:c.M], c.N)
    got = f6.check_producer(c, r, codes, eb[:c.M, :nb].contiguous())
    print(f"{c.name}: {got}; scale bytes {int(eb[:c.M, :nb].min())} .. {int(eb[:c.M, :nb].max())}")
    assert got == {"exp_bad": 0, "val_bad": 0}
    assert (q[c.M:] == f6.GUARD_BYTE).all() and (q[:, nq:] == f6.GUARD_BYTE).all()
    assert (eb[c.M:] == f6.GUARD_BYTE).all() and (eb[:, nb:] == f6.GUARD_BYTE).all()
    if c.zero_row is not None:
        assert (eb[c.zero_row, :nb] == 127).all() and not (codes[c.zero_row] & 0x1f).any()
    q2, eb2 = f6.run_pcase(c, ops)
    assert torch.equal(q2.cpu(), q) and torch.equal(eb2.cpu(), eb)


def test_producer_into_consumer_through_the_ops_wrappers():
    """ffn.0 -> ffn.2 as the engine chains them, weights from ops.mx6_pack: the consumer, fed the producer's own bytes and scale bytes, is held
    to ITS bound against the fp64 product of exactly those bytes"""
    from yume_amd import ops as yops
    g = torch.Generator().manual_seed(23)
    M, C, Fd = 130, 256, 512
    ca, ea = f6.mx6_quantise(torch.randn(M, C, generator=g))
    w1, w2 = (torch.randn(Fd, C, generator=g) * C ** -0.5).bfloat16(), (torch.randn(C, Fd, generator=g) * Fd ** -0.5).bfloat16()
    b1, b2 = torch.randn(Fd, generator=g), torch.randn(C, generator=g)
    w1p, e1 = yops.mx6_pack(w1.to(DEV))
    w2p, e2 = yops.mx6_pack(w2.to(DEV))
    h6 = f6.mx6_pack_bits(ca).to(DEV)
    he = torch.zeros(M, 16, dtype=torch.uint8)
    he[:, :C // 32] = ea
    he = he.to(DEV)[:, :C // 32]
    fq = torch.empty(M, 3 * Fd // 4, dtype=torch.uint8, device=DEV)
    fe = torch.empty(M, 16, dtype=torch.uint8, device=DEV)[:, :Fd // 32]
    yops.gemm_f6_mxout(h6, he, w1p, e1[:, :C // 32], b1.to(DEV), fq, fe)
    out = torch.zeros(M, C, dtype=torch.float32, device=DEV)
    yops.gemm_f6_mx(fq, fe, w2p, e2[:, :Fd // 32], b2.to(DEV), out, f6.EPI_F32)
    torch.cuda.synchronize()
    A = f6.mx6_dequantise(f6.mx6_unpack_bits(fq.cpu(), Fd), fe.cpu())
    W2 = f6.mx6_dequantise(f6.mx6_unpack_bits(w2p.cpu(), Fd), e2.cpu()[:, :Fd // 32])
    y = A @ W2.t() + b2.double()
    bnd = f6.C_SUM_F6 * ((A * A) @ (W2 * W2).t()).sqrt() + 2.0 ** -21 * y.abs() + 2.0 ** -22 * b2.double().abs()
    assert int(((out.double().cpu() - y).abs() > bnd).sum()) == 0
    # and the weights the device multiplied are the bf16 weights to half an e2m3 step of their block
    assert (W2 - w2.double()).abs().max() <= w2.double().abs().max() / 7.5 * 0.5
    with pytest.raises(RuntimeError):
        yops.gemm_f6_mx(fq, fe[:, :8], w2p, e2[:, :Fd // 32], b2.to(DEV), out, f6.EPI_F32)


def test_every_case_runs_on_its_kernel():
    """YUME_GEMM_LOG is read once per process: a fresh child makes every call of both tables once and its log names the kernel."""
    env = dict(os.environ, YUME_GEMM_LOG="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_f6_cases.py"), "--routes"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = []
        elif line.startswith("[gemm_") and name is not None:
            seen[name].append(line)
    for c in f6.CASES:
        assert len(seen.get(c.name, [])) == 1, (c.name, seen.get(c.name))
        tag, kernel, *fields = seen[c.name][0].split()
        assert (tag, kernel) == ("[gemm_f6]", "mx")
        f = {k: int(v) for k, v in (t.split("=") for t in fields)}
        lda, ldea, ldw, ldew, ldo = f6.strides(c)
        assert f == {"M": c.M, "N": c.N, "K": c.K, "epi": c.epi, "lda": lda, "ldea": ldea, "ldw": ldw, "ldew": ldew, "ldo": ldo}, seen[c.name][0]
    for c in f6.PCASES:
        assert len(seen.get(c.name, [])) == 1, (c.name, seen.get(c.name))
        tag, kernel, *fields = seen[c.name][0].split()
        assert (tag, kernel) == ("[gemm_f6]", "mxout")
        f = {k: int(v) for k, v in (t.split("=") for t in fields)}
        lda, ldea, ldw, ldew, ldo, ldeo = f6.pstrides(c)
        assert f == {"M": c.M, "N": c.N, "K": c.K, "epi": f6.EPI_MX6_GELU, "lda": lda, "ldea": ldea, "ldw": ldw, "ldew": ldew, "ldo": ldo,
                     "ldeo": ldeo}, seen[c.name][0]
