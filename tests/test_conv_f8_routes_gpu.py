"""The MX e4m3 convolution and its producer on the device, one call of the raw C-ABI per row of tests/conv_f8_cases.py.
Consumer (yume_conv3d_cl_f8mx): EVERY output element inside the per-element bound against the fp64 reference on the very bytes and scale
bytes, the guards around the stored region untouched, the two pattern rows bit-exact (a scale taken from the wrong tap, position, frame or
channel block changes the integers), a second launch equal in its bits. Producer (yume_vae_rmsnorm_silu_mx): bytes and scale bytes equal to
yume_vae_rmsnorm_silu followed by the host MX quantiser, nothing written outside. The two chained through the wrappers. One child process
with YUME_CONV_LOG=1 names the kernel of every call."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_f8_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", cc.CASES, ids=[c.name for c in cc.CASES])
def test_every_element_inside_the_bound_guards_intact_equal_bits_on_a_second_launch(c):
    ops = cc.make_case(c, DEV)
    r = cc.reference(c, ops)
    out = cc.run_case(c, ops)
    torch.cuda.synchronize()
    got = cc.gather(c, out).double().cpu()
    ref = r["ref"]
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / cc.bound(c, r))
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ratio.shape)))
    print(f"{c.name}: worst error / bound {ratio.reshape(-1)[worst].item():.4f} at {idx}: got {got[idx].item():.6g} ref {ref[idx].item():.6g}; "
          f"{int((ratio > 1).sum())} of {ratio.numel()} elements outside; {int((err != 0).sum())} differ at all")
    assert torch.isfinite(got).all()
    assert int((ratio > 1).sum()) == 0
    assert cc.guards_damaged(c, out) == 0
    if c.pattern:
        assert torch.equal(got, ref)
    out2 = cc.run_case(c, ops)
    assert torch.equal(out, out2)


@pytest.mark.parametrize("c", cc.PCASES, ids=[c.name for c in cc.PCASES])
def test_producer_equals_the_norm_followed_by_the_host_quantiser(c):
    ops = cc.make_pcase(c, DEV)
    q, e, y = cc.run_pcase(c, ops)
    torch.cuda.synchronize()
    q, e, y = q.cpu(), e.cpu(), y.cpu()
    nb = c.C // 32
    qh, eh = cc.mx_quantise(y.float())
    dq, de = int((q[:c.M, :c.C] != qh).sum()), int((e[:c.M, :nb] != eh).sum())
    print(f"{c.name}: {dq} bytes and {de} scale bytes differ; scale bytes {int(eh.min())} .. {int(eh.max())}")
    assert de == 0 and dq == 0
    assert (q[c.M:] == cc.GUARD_BYTE).all() and (q[:, c.C:] == cc.GUARD_BYTE).all()
    assert (e[c.M:] == cc.GUARD_BYTE).all() and (e[:, nb:] == cc.GUARD_BYTE).all()
    assert int(eh.max()) - int(eh.min()) >= 3 or c.M == 1
    q2, e2, _ = cc.run_pcase(c, ops)
    assert torch.equal(q2.cpu(), q) and torch.equal(e2.cpu(), e)


def test_producer_into_consumer_through_the_wrappers():
    """norm -> convolution as the engine chains them, with a cache pair: the convolution, fed the producer's own bytes and scale bytes, is
    held to ITS bound against the fp64 sum of exactly those bytes"""
    from yume_amd import ops as yops
    from yume_amd import vae_ops as V
    g = torch.Generator().manual_seed(19)
    T, H, W, C, Co = 2, 9, 7, 128, 136
    x = torch.randn(2 + T, H, W, C, generator=g).bfloat16().to(DEV)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    q = torch.empty((2 + T, H, W, C), dtype=torch.uint8, device=DEV)
    e = torch.empty((2 + T, H, W, C // 32), dtype=torch.uint8, device=DEV)
    V.rmsnorm_silu_mx(x, gamma, True, q, e)
    wb = (torch.randn(Co, 27 * C, generator=g) * (27 * C) ** -0.5).bfloat16().to(DEV)
    wq = torch.empty((Co, 27 * C), dtype=torch.uint8, device=DEV)
    sw = torch.empty(Co, dtype=torch.float32, device=DEV)
    yops.quant_rows_e4m3(wb, wq, sw)
    bias = torch.randn(Co, generator=g).to(DEV)
    out = torch.empty((T, H, W, Co), dtype=torch.bfloat16, device=DEV)
    zero = torch.zeros(64, dtype=torch.bfloat16, device=DEV)
    V.conv3d_cl_f8mx(q[2:], e[2:], (q[:2].contiguous(), e[:2].contiguous()), wq, sw, bias, Co, (3, 3, 3), out, V.EPI_BF16, zero_page=zero)
    torch.cuda.synchronize()
    c = cc.Case("chain", T, H, W, C, Co, cache=True)
    ops = {"x": q.cpu().view(torch.float8_e4m3fn).float(), "xe": e.cpu(), "W": wq.cpu().view(torch.float8_e4m3fn).float(), "sw": sw.cpu(),
           "bias": bias.cpu(), "add": None}
    r = cc.reference(c, ops)
    err = (out.double().cpu().view(-1, Co) - r["ref"]).abs()
    assert int((err > cc.bound(c, r)).sum()) == 0
    with pytest.raises(RuntimeError):
        V.conv3d_cl_f8mx(q[2:], e[2:], (q[:2].contiguous(), e[:1].contiguous()), wq, sw, bias, Co, (3, 3, 3), out, V.EPI_BF16, zero_page=zero)


def test_every_case_runs_on_the_f8mx_kernel():
    """YUME_CONV_LOG is read once per process: a fresh child makes every call of the table once and its log names the kernel and the shape."""
    env = dict(os.environ, YUME_CONV_LOG="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_f8_cases.py"), "--routes"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    seen, name = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("CASE "):
            name = line.split()[1]
            seen[name] = []
        elif line.startswith("[conv3d_cl]") and name is not None:
            seen[name].append(line)
    for c in cc.CASES:
        assert len(seen.get(c.name, [])) == 1, (c.name, seen.get(c.name))
        tag, kernel, *fields = seen[c.name][0].split()
        assert (tag, kernel) == ("[conv3d_cl]", "f8mx")
        f = dict(t.split("=") for t in fields)
        tiles = c.T * ((c.H * c.W + 255) // 256) * ((c.Cout + 255) // 256)
        assert f == {"M": str(c.T * c.H * c.W), "Cin": str(c.Cin), "Cout": str(c.Cout), "k": "%dx%dx%d" % c.k, "epi": str(c.epi),
                     "cache": "1" if c.cache else "0", "tiles": str(tiles)}, seen[c.name][0]
