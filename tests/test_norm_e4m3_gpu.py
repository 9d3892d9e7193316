"""yume_adaln_modulate_e4m3 on the device against its definition: yume_quant_rows_e4m3 applied to the bf16 rows of yume_adaln_modulate
(out_kind = 0), both run on the same device inputs — bytes and scales bit-equal, guard bytes beyond C and the guard row behind T untouched,
the exactly-zero row with scale 1 and zero bytes (tests/norm_e4m3_cases.py has the table). One child process with YUME_NORM_LOG=1 names the
instance every shape class ran on."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import norm_e4m3_cases as nc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _composite(x, tab, idx, add_one, T, C):
    from yume_amd import ops
    h = torch.empty(T, C, dtype=torch.bfloat16, device=DEV)
    ops.adaln_modulate(x[:, :C], tab[:, 0], tab[:, 1], 2 * C, idx, add_one, h, 0, 1e-6)
    q = torch.empty(T, C, dtype=torch.uint8, device=DEV)
    s = torch.empty(T, dtype=torch.float32, device=DEV)
    ops.quant_rows_e4m3(h, q, s)
    return h, q, s


def _fused_raw(x, tab, idx, add_one, T, C, ldq, rows=None):
    """ONE raw C-ABI call over the first `rows` rows into guarded buffers q [T + 1, ldq], scale [T + 1]"""
    from yume_amd import _lib
    lib = _lib.load()
    rows = T if rows is None else rows
    q = torch.full((T + 1, ldq), nc.GUARD_BYTE, dtype=torch.uint8, device=DEV)
    s = torch.full((T + 1,), nc.GUARD_SCALE, dtype=torch.float32, device=DEV)
    P = ctypes.c_void_p
    rc = lib.yume_adaln_modulate_e4m3(P(x.data_ptr()), x.stride(0), rows, C, 1e-6, P(tab[:, 0].data_ptr()), P(tab[:, 1].data_ptr()), 2 * C,
                                      P(idx.data_ptr()) if idx is not None else None, 1 if add_one else 0, P(q.data_ptr()), ldq,
                                      P(s.data_ptr()), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "yume_adaln_modulate_e4m3")
    torch.cuda.synchronize()
    return q, s


@pytest.mark.parametrize("name, T, C, use_idx, add_one, zero_add", nc.CASES, ids=nc.IDS)
def test_bytes_and_scales_equal_the_two_call_composite(name, T, C, use_idx, add_one, zero_add):
    x, tab, idx = nc.make_case(T, C, use_idx, add_one, zero_add)
    x, tab = x.to(DEV), tab.to(DEV)
    idx = idx.to(DEV) if idx is not None else None
    h, q_want, s_want = _composite(x, tab, idx, add_one, T, C)
    q, s = _fused_raw(x, tab, idx, add_one, T, C, C + 16)
    nq = (q[:T, :C] != q_want).sum().item()
    ns = (s[:T].view(torch.int32) != s_want.view(torch.int32)).sum().item()
    print(f"{name}: {nq} of {T * C} bytes and {ns} of {T} scales differ from the composite")
    assert nq == 0 and ns == 0
    assert (q[:T, C:] == nc.GUARD_BYTE).all() and (q[T:] == nc.GUARD_BYTE).all() and s[T].item() == nc.GUARD_SCALE
    assert (s[:T] > 0).all() and torch.isfinite(s[:T]).all()
    if use_idx or zero_add:
        z = nc.zero_row_of(T)
        assert not h[z].float().any()                              # the composite's bf16 row is zero: the case is what it claims to be
        assert s[z].item() == 1.0 and not (q[z, :C] & 0x7f).any()
        if T > 1:
            assert (s[:T] != 1.0).sum().item() >= T - 1             # ... and it is the only such row


def test_rows_behind_T_are_not_written_and_T0_launches_nothing():
    T, C = 1027, 512
    x, tab, idx = nc.make_case(T, C, True, True, False)
    x, tab, idx = x.to(DEV), tab.to(DEV), idx.to(DEV)
    _, q_want, s_want = _composite(x, tab, idx, True, T, C)
    q, s = _fused_raw(x, tab, idx, True, T, C, C + 16, rows=1025)      # the two-row instance with an odd count
    assert torch.equal(q[:1025, :C], q_want[:1025]) and torch.equal(s[:1025], s_want[:1025])
    assert (q[1025:] == nc.GUARD_BYTE).all() and (s[1025:] == nc.GUARD_SCALE).all() and (q[:, C:] == nc.GUARD_BYTE).all()
    q, s = _fused_raw(x, tab, idx, True, T, C, C + 16, rows=0)
    assert (q == nc.GUARD_BYTE).all() and (s == nc.GUARD_SCALE).all()


def test_ops_wrapper_and_equal_bits_on_a_second_call():
    from yume_amd import ops
    T, C = 1027, 3072
    x, tab, idx = nc.make_case(T, C, True, True, False)
    x, tab, idx = x.to(DEV), tab.to(DEV), idx.to(DEV)
    _, q_want, s_want = _composite(x, tab, idx, True, T, C)
    outs = []
    for _ in range(2):
        q, s = torch.empty(T, C, dtype=torch.uint8, device=DEV), torch.empty(T, dtype=torch.float32, device=DEV)
        ops.adaln_modulate_e4m3(x[:, :C], tab[:, 0], tab[:, 1], 2 * C, idx, True, q, s)
        outs.append((q, s))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][0], q_want) and torch.equal(outs[0][1], s_want)
    with pytest.raises(RuntimeError, match="do not fit"):
        ops.adaln_modulate_e4m3(x[:, :C], tab[:, 0], tab[:, 1], 2 * C, idx, True, outs[0][0][:5], outs[0][1])


def test_the_log_names_an_instance_of_its_own_per_shape_class():
    """YUME_NORM_LOG is read once per process: a child runs one call per (T, C) class"""
    env = dict(os.environ, YUME_NORM_LOG="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--log"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln.split() for ln in p.stderr.splitlines() if ln.startswith("[norm] ")]
    got = [(ln[1], int(ln[2].split("=")[1]), int(ln[3].split("=")[1])) for ln in lines]
    assert got == [(nc.instance(T, C), T, C) for T, C in LOG_SHAPES], got
    assert {g[0] for g in got} == {"adaln_e4m3<3>", "adaln2_e4m3", "adaln_e4m3<5>", "adaln_e4m3<8>"}


LOG_SHAPES = [(5, 512), (1027, 512), (1027, 3072), (1027, 5120), (5, 8192)]


def main():
    for T, C in LOG_SHAPES:
        x, tab, idx = nc.make_case(T, C, True, True, False)
        _fused_raw(x.to(DEV), tab.to(DEV), idx.to(DEV), True, T, C, C)


if __name__ == "__main__":
    if sys.argv[1:] != ["--log"]:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
