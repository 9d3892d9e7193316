"""yume_quant_rows_e4m3 on the device against the reference and checks of tests/test_quant_rows_cpu.py: R in {1, 5, 300}, K in {16, 128, 3072},
rows longer than K on both sides, the four special rows (all zero; one huge element among tiny ones; bf16 subnormals; +amax and -amax).
The scale is bit-equal to amax / 448, every element inside half an e4m3 ulp (+ fp32 slack) of x / scale, the amax elements are +-448, no
byte is NaN, and the guard bytes beyond K and behind row R are untouched."""
import ctypes

import pytest
import torch

import test_quant_rows_cpu as qc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(x, ldx, ldq, R=None):
    """x bf16 [rows, K] on the host -> (q bytes [rows + 1, ldq], scale [rows + 1]) from ONE raw C-ABI call over the first R rows"""
    from yume_amd import _lib
    lib = _lib.load()
    rows, K = x.shape
    R = rows if R is None else R
    xb = torch.full((rows, ldx), 3.0, dtype=torch.bfloat16)
    xb[:, :K] = x
    xd = xb.to(DEV)
    q = torch.full((rows + 1, ldq), qc.GUARD_BYTE, dtype=torch.uint8, device=DEV)
    s = torch.full((rows + 1,), qc.GUARD_SCALE, dtype=torch.float32, device=DEV)
    rc = lib.yume_quant_rows_e4m3(ctypes.c_void_p(xd.data_ptr()), ldx, R, K, ctypes.c_void_p(q.data_ptr()), ldq, ctypes.c_void_p(s.data_ptr()),
                                  torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "yume_quant_rows_e4m3")
    torch.cuda.synchronize()
    return q.cpu(), s.cpu()


@pytest.mark.parametrize("R, K", qc.SHAPES)
def test_scale_bits_bound_amax_no_nan_and_guards(R, K):
    x = qc.make_input(R, K)
    q, s = _run(x, K + 8, K + 16)
    got = qc.check(x, q[:R, :K].contiguous(), s[:R].contiguous())
    print(f"R={R} K={K}: {got}")
    assert got == qc.CLEAN
    assert (q[:R, K:] == qc.GUARD_BYTE).all() and (q[R:] == qc.GUARD_BYTE).all() and s[R] == qc.GUARD_SCALE
    if R >= 5:
        z = qc.SPECIAL_ROWS["zero"]
        assert s[z] == 1.0 and not q[z, :K].any()
        want, _ = qc.ref_quant(x)
        # the reference forms x / scale by division, the kernel by a reciprocal: a value on a rounding boundary may fall to the other side
        # (both lie within half a step + slack of x / scale: never more than one step apart)
        assert ((q[:R, :K].int() - want.int()).abs() > 1).sum() == 0


def test_rows_behind_R_are_not_written_and_R0_launches_nothing():
    x = qc.make_input(5, 128)
    q, s = _run(x, 136, 144, R=3)
    assert (q[3:] == qc.GUARD_BYTE).all() and (s[3:] == qc.GUARD_SCALE).all()
    assert qc.check(x[:3], q[:3, :128].contiguous(), s[:3].contiguous()) == qc.CLEAN
    q, s = _run(x, 136, 144, R=0)
    assert (q == qc.GUARD_BYTE).all() and (s == qc.GUARD_SCALE).all()


def test_ops_wrapper_and_equal_bits_on_a_second_call():
    from yume_amd import ops
    x = qc.make_input(300, 3072).to(DEV)
    q1, s1 = torch.empty(300, 3072, dtype=torch.uint8, device=DEV), torch.empty(300, dtype=torch.float32, device=DEV)
    q2, s2 = torch.empty_like(q1), torch.empty_like(s1)
    ops.quant_rows_e4m3(x, q1, s1)
    ops.quant_rows_e4m3(x, q2, s2)
    assert torch.equal(q1, q2) and torch.equal(s1, s2)
    assert qc.check(x.cpu(), q1.cpu(), s1.cpu()) == qc.CLEAN
