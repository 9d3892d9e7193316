"""yume_adaln_modulate_mx_e2m3 on the device against its definition: the host MX6 quantiser applied to the bf16 rows yume_adaln_modulate
(out_kind = 0) stores for the same device inputs — packed bytes and scale bytes bit-equal in both instances (one row and two rows per
workgroup), guard bytes beyond 3 C / 4 and C / 32 and the guard row behind T untouched (tests/norm_e2m3_cases.py has the table). One child
process with YUME_NORM_LOG=1 names the instance of every shape class."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import gemm_f6_cases as f6
import norm_e2m3_cases as n6

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _fused_raw(x, mul, add, ts, idx, add_one, T, C, rows=None):
    """ONE raw C-ABI call over the first `rows` rows into guarded buffers q [T + 1, ldq], e [T + 1, lde]"""
    from yume_amd import _lib
    lib = _lib.load()
    rows = T if rows is None else rows
    ldq, lde = n6.pitches(C)
    q = torch.full((T + 1, ldq), n6.GUARD_BYTE, dtype=torch.uint8, device=DEV)
    e = torch.full((T + 1, lde), n6.GUARD_BYTE, dtype=torch.uint8, device=DEV)
    P = ctypes.c_void_p
    rc = lib.yume_adaln_modulate_mx_e2m3(P(x.data_ptr()), x.stride(0), rows, C, 1e-6, P(mul.data_ptr()), P(add.data_ptr()), ts,
                                         P(idx.data_ptr()) if idx is not None else None, 1 if add_one else 0, P(q.data_ptr()), ldq,
                                         P(e.data_ptr()), lde, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "yume_adaln_modulate_mx_e2m3")
    torch.cuda.synchronize()
    return q.cpu(), e.cpu()


def _want(x, mul, add, ts, idx, add_one, T, C):
    from yume_amd import ops
    h = torch.empty(T, C, dtype=torch.bfloat16, device=DEV)
    ops.adaln_modulate(x[:, :C], mul, add, ts, idx, add_one, h, 0, 1e-6)
    codes, e = f6.mx6_quantise(h.cpu())
    return h.cpu(), f6.mx6_pack_bits(codes), e


def _device_case(T, C, form):
    x, mul, add, ts, idx, add_one = n6.make_case(T, C, form)
    base = mul._base if mul._base is not None else mul            # (mul and add are views of one table: move it once)
    tab = base.to(DEV)
    mul_d = tab.as_strided(mul.shape, mul.stride(), mul.storage_offset())
    add_d = tab.as_strided(add.shape, add.stride(), add.storage_offset())
    return x.to(DEV), mul_d, add_d, ts, idx.to(DEV) if idx is not None else None, add_one


@pytest.mark.parametrize("name, T, C, form", n6.CASES, ids=n6.IDS)
def test_bytes_and_scale_bytes_equal_adaln_then_the_host_quantiser(name, T, C, form):
    x, mul, add, ts, idx, add_one = _device_case(T, C, form)
    h, q_want, e_want = _want(x, mul, add, ts, idx, add_one, T, C)
    q, e = _fused_raw(x, mul, add, ts, idx, add_one, T, C)
    nq, ne = int((q[:T, :3 * C // 4] != q_want).sum()), int((e[:T, :C // 32] != e_want).sum())
    print(f"{name}: {nq} of {T * 3 * C // 4} bytes and {ne} of {T * C // 32} scale bytes differ from the composite; "
          f"scale bytes {int(e_want.min())} .. {int(e_want.max())}")
    assert nq == 0 and ne == 0
    assert (q[:T, 3 * C // 4:] == n6.GUARD_BYTE).all() and (q[T:] == n6.GUARD_BYTE).all()
    assert (e[:T, C // 32:] == n6.GUARD_BYTE).all() and (e[T:] == n6.GUARD_BYTE).all()
    if form == "idx":                                               # the exactly-zero row: every block e = 0, every code +0
        z = n6.nc.zero_row_of(T)
        assert not h[z].float().any() and (e[z, :C // 32] == 127).all() and not q[z, :3 * C // 4].any()


def test_rows_behind_T_are_not_written_T0_launches_nothing_and_the_ops_wrapper_repeats_its_bits():
    from yume_amd import ops
    T, C = 1030, 384
    x, mul, add, ts, idx, add_one = _device_case(T, C, "idx")
    _, q_want, e_want = _want(x, mul, add, ts, idx, add_one, T, C)
    q, e = _fused_raw(x, mul, add, ts, idx, add_one, T, C, rows=1025)      # the two-row instance with an odd count
    assert torch.equal(q[:1025, :288], q_want[:1025]) and torch.equal(e[:1025, :12], e_want[:1025])
    assert (q[1025:] == n6.GUARD_BYTE).all() and (e[1025:] == n6.GUARD_BYTE).all()
    q, e = _fused_raw(x, mul, add, ts, idx, add_one, T, C, rows=0)
    assert (q == n6.GUARD_BYTE).all() and (e == n6.GUARD_BYTE).all()
    outs = []
    for _ in range(2):
        qo = torch.empty(T, 288, dtype=torch.uint8, device=DEV)
        eo = torch.empty(T, 16, dtype=torch.uint8, device=DEV)[:, :12]
        ops.adaln_modulate_mx_e2m3(x[:, :C], mul, add, ts, idx, add_one, qo, eo)
        outs.append((qo.cpu(), eo.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][0], q_want) and torch.equal(outs[0][1], e_want)
    with pytest.raises(RuntimeError, match="do not fit"):
        ops.adaln_modulate_mx_e2m3(x[:, :C], mul, add, ts, idx, add_one, qo[:5], eo)


def test_the_log_names_an_instance_of_its_own_per_shape_class():
    """YUME_NORM_LOG is read once per process: a child runs one call per (T, C) class"""
    env = dict(os.environ, YUME_NORM_LOG="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--log"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln.split() for ln in p.stderr.splitlines() if ln.startswith("[norm] ")]
    got = [(ln[1], int(ln[2].split("=")[1]), int(ln[3].split("=")[1])) for ln in lines]
    assert got == [(n6.instance(T, C), T, C) for T, C in n6.LOG_SHAPES], got
    assert {g[0] for g in got} == {"adaln_e2m3<3>", "adaln2_e2m3"}


def main():
    for T, C in n6.LOG_SHAPES:
        x, mul, add, ts, idx, add_one = _device_case(T, C, "idx")
        _fused_raw(x, mul, add, ts, idx, add_one, T, C)


if __name__ == "__main__":
    if sys.argv[1:] != ["--log"]:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
