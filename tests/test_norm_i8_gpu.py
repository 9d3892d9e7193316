"""The int8 row format on the device (tests/norm_i8_cases.py has the mirror and the tables).
yume_quant_rows_i8 equals the host mirror bit for bit — bytes and scales — for K in {16, 128, 384, 3072}, ragged R, the zero row, the
largest bf16, the subnormal row, the exact .5 ties, with the pitch gaps and the rows beyond R untouched; the non-finite rule holds.
yume_adaln_modulate_i8 equals device yume_adaln_modulate followed by the mirror, AND followed by yume_quant_rows_i8, bit for bit, for C in
{512, 3072, 5120} (and 8192), T in {5, 1023, 1025}, both forms, with and without row_idx. One child process with YUME_NORM_LOG=1 names the
instance every shape class ran on."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import norm_i8_cases as nc

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = ctypes.c_void_p


def _quant_raw(xd, ldx, rows, K, ldq, alloc_rows):
    """ONE raw C-ABI call into guarded buffers q [alloc_rows + 1, ldq], scale [alloc_rows + 1]"""
    from yume_amd import _lib
    lib = _lib.load()
    q = torch.full((alloc_rows + 1, ldq), nc.GUARD_BYTE, dtype=torch.int8, device=DEV)
    s = torch.full((alloc_rows + 1,), nc.GUARD_SCALE, dtype=torch.float32, device=DEV)
    rc = lib.yume_quant_rows_i8(P(xd.data_ptr()), ldx, rows, K, P(q.data_ptr()), ldq, P(s.data_ptr()), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "yume_quant_rows_i8")
    torch.cuda.synchronize()
    return q.cpu(), s.cpu()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("R, K", nc.QUANT_SHAPES)
def test_quant_rows_i8_equals_the_mirror_bit_for_bit(R, K):
    x = nc.make_input(R, K)
    want_q, want_s = nc.mirror(x)
    ldx, ldq = K + 8, K + 16                                                      # pitch gaps on both sides
    xd = torch.full((R, ldx), 1e30, dtype=torch.bfloat16, device=DEV)            # what lies in the gap would change every amax
    xd[:, :K] = x.to(DEV)
    q, s = _quant_raw(xd, ldx, R, K, ldq, R)
    nq, ns = int((q[:R, :K] != want_q).sum()), int((s[:R].view(torch.int32) != want_s.view(torch.int32)).sum())
    print(f"R={R} K={K}: {nq} of {R * K} bytes and {ns} of {R} scales differ from the mirror; checks {nc.check(x, q[:R, :K].contiguous(), s[:R].contiguous())}")
    assert nq == 0 and ns == 0
    assert nc.check(x, q[:R, :K].contiguous(), s[:R].contiguous()) == nc.CLEAN
    assert (q[:R, K:] == nc.GUARD_BYTE).all() and (q[R:] == nc.GUARD_BYTE).all() and s[R].item() == nc.GUARD_SCALE
    if R >= 5:
        rows = nc.SPECIAL_ROWS
        assert s[rows["zero"]].item() == 1.0 and not q[rows["zero"], :K].any()
        assert s[rows["ties"]].item() == 2.0 ** nc.TIE_EXP and [int(t) for t in q[rows["ties"], 1:5]] == [0, 0, 2, -2]
        assert int(q[rows["huge"], K // 3]) == 127


def test_rows_beyond_R_are_not_written_and_R0_launches_nothing():
    R, K = 301, 128
    x = nc.make_input(R, K).to(DEV)
    want_q, want_s = nc.mirror(x.cpu())
    q, s = _quant_raw(x, K, 299, K, K + 16, R)                                    # 299 = 74 blocks of four waves + three rows
    assert torch.equal(q[:299, :K], want_q[:299]) and _same_bits(s[:299], want_s[:299])
    assert (q[299:] == nc.GUARD_BYTE).all() and (s[299:] == nc.GUARD_SCALE).all() and (q[:, K:] == nc.GUARD_BYTE).all()
    q, s = _quant_raw(x, K, 0, K, K + 16, R)
    assert (q == nc.GUARD_BYTE).all() and (s == nc.GUARD_SCALE).all()


def test_non_finite_rule_scale_nan_bytes_zero_other_rows_untouched():
    from yume_amd import ops
    x = nc.make_input(5, 384)
    x[1, 7] = float("inf")
    x[3, 300] = float("nan")
    want_q, want_s = nc.mirror(x)
    q = torch.full((5, 384), nc.GUARD_BYTE, dtype=torch.int8, device=DEV)
    s = torch.full((5,), nc.GUARD_SCALE, dtype=torch.float32, device=DEV)
    ops.quant_rows_i8(x.to(DEV), q, s)
    q, s = q.cpu(), s.cpu()
    assert torch.isnan(s[1]) and torch.isnan(s[3]) and not q[1].any() and not q[3].any()
    for r in (0, 2, 4):
        assert torch.equal(q[r], want_q[r]) and s[r] == want_s[r]
    assert torch.equal(q, want_q)


def _emit_raw(x, tab, idx, add_one, stride, T, C, ldq, rows=None):
    """ONE raw C-ABI call over the first `rows` rows into guarded buffers q [T + 1, ldq], scale [T + 1]"""
    from yume_amd import _lib
    lib = _lib.load()
    rows = T if rows is None else rows
    q = torch.full((T + 1, ldq), nc.GUARD_BYTE, dtype=torch.int8, device=DEV)
    s = torch.full((T + 1,), nc.GUARD_SCALE, dtype=torch.float32, device=DEV)
    rc = lib.yume_adaln_modulate_i8(P(x.data_ptr()), x.stride(0), rows, C, 1e-6, P(tab[:, 0].data_ptr()), P(tab[:, 1].data_ptr()), stride,
                                    P(idx.data_ptr()) if idx is not None else None, 1 if add_one else 0, P(q.data_ptr()), ldq,
                                    P(s.data_ptr()), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "yume_adaln_modulate_i8")
    torch.cuda.synchronize()
    return q, s


def _bf16_rows(x, tab, idx, add_one, stride, T, C):
    from yume_amd import ops
    h = torch.empty(T, C, dtype=torch.bfloat16, device=DEV)
    ops.adaln_modulate(x[:, :C], tab[:, 0], tab[:, 1], stride, idx, add_one, h, 0, 1e-6)
    return h


@pytest.mark.parametrize("name, T, C, use_idx, add_one", nc.EMIT_CASES, ids=nc.EMIT_IDS)
def test_emitter_equals_adaln_then_mirror_and_adaln_then_quant_rows_i8(name, T, C, use_idx, add_one):
    from yume_amd import ops
    x, tab, idx = nc.make_emit_case(T, C, use_idx, add_one)
    x, tab = x.to(DEV), tab.to(DEV)
    idx = idx.to(DEV) if idx is not None else None
    stride = nc.tab_stride(C, use_idx, add_one)
    h = _bf16_rows(x, tab, idx, add_one, stride, T, C)
    mq, ms = nc.mirror(h.cpu())                                                   # device adaLN, then the host mirror
    dq = torch.empty(T, C, dtype=torch.int8, device=DEV)
    ds = torch.empty(T, dtype=torch.float32, device=DEV)
    ops.quant_rows_i8(h, dq, ds)                                                  # device adaLN, then the device quantiser
    q, s = _emit_raw(x, tab, idx, add_one, stride, T, C, C + 16)
    qh, sh = q.cpu(), s.cpu()
    n_mq, n_ms = int((qh[:T, :C] != mq).sum()), int((sh[:T].view(torch.int32) != ms.view(torch.int32)).sum())
    n_dq, n_ds = int((q[:T, :C] != dq).sum()), int((s[:T].view(torch.int32) != ds.view(torch.int32)).sum())
    print(f"{name}: against the mirror {n_mq} of {T * C} bytes, {n_ms} of {T} scales differ; against quant_rows_i8 {n_dq} bytes, {n_ds} scales")
    assert n_mq == 0 and n_ms == 0 and n_dq == 0 and n_ds == 0
    assert (qh[:T, C:] == nc.GUARD_BYTE).all() and (qh[T:] == nc.GUARD_BYTE).all() and sh[T].item() == nc.GUARD_SCALE
    assert (sh[:T] > 0).all() and torch.isfinite(sh[:T]).all() and not (qh[:T, :C] == -128).any()
    assert (qh[:T, :C].abs().amax(dim=1)[sh[:T] != 1.0] == 127).all()             # every non-zero row reaches +-127
    if use_idx:
        z = nc.zero_row_of(T)
        assert not h[z].float().any()                                             # the bf16 row is zero: the case is what it claims to be
        assert sh[z].item() == 1.0 and not qh[z, :C].any()


def test_emitter_rows_behind_T_are_not_written_and_T0_launches_nothing():
    T, C = 1027, 512
    x, tab, idx = nc.make_emit_case(T, C, True, True)
    x, tab, idx = x.to(DEV), tab.to(DEV), idx.to(DEV)
    mq, ms = nc.mirror(_bf16_rows(x, tab, idx, True, 2 * C, T, C).cpu())
    q, s = _emit_raw(x, tab, idx, True, 2 * C, T, C, C + 16, rows=1025)           # the two-row instance with an odd count
    q, s = q.cpu(), s.cpu()
    assert torch.equal(q[:1025, :C], mq[:1025]) and _same_bits(s[:1025], ms[:1025])
    assert (q[1025:] == nc.GUARD_BYTE).all() and (s[1025:] == nc.GUARD_SCALE).all() and (q[:, C:] == nc.GUARD_BYTE).all()
    q, s = _emit_raw(x, tab, idx, True, 2 * C, T, C, C + 16, rows=0)
    assert (q == nc.GUARD_BYTE).all() and (s == nc.GUARD_SCALE).all()


def test_emitter_follows_the_non_finite_rule():
    """a non-finite x makes the whole LayerNorm row NaN: scale NaN, bytes zero, the other rows as before"""
    from yume_amd import ops
    T, C = 5, 512
    x, tab, idx = nc.make_emit_case(T, C, True, True)
    x, tab, idx = x.to(DEV), tab.to(DEV), idx.to(DEV)
    q0, s0 = torch.empty(T, C, dtype=torch.int8, device=DEV), torch.empty(T, dtype=torch.float32, device=DEV)
    ops.adaln_modulate_i8(x[:, :C], tab[:, 0], tab[:, 1], 2 * C, idx, True, q0, s0)
    x[1, 33] = float("inf")
    q, s = torch.empty_like(q0), torch.empty_like(s0)
    ops.adaln_modulate_i8(x[:, :C], tab[:, 0], tab[:, 1], 2 * C, idx, True, q, s)
    assert torch.isnan(s[1]).item() and not q[1].any()
    keep = [0, 2, 3, 4]
    assert torch.equal(q[keep], q0[keep]) and torch.equal(s[keep], s0[keep])


def test_ops_wrappers_and_equal_bits_on_a_second_call():
    from yume_amd import ops
    T, C = 1025, 3072
    x, tab, idx = nc.make_emit_case(T, C, True, True)
    x, tab, idx = x.to(DEV), tab.to(DEV), idx.to(DEV)
    outs = []
    for dt in (torch.int8, torch.uint8):                                          # both byte dtypes are taken
        q, s = torch.empty(T, C, dtype=dt, device=DEV), torch.empty(T, dtype=torch.float32, device=DEV)
        ops.adaln_modulate_i8(x[:, :C], tab[:, 0], tab[:, 1], 2 * C, idx, True, q, s)
        outs.append((q.view(torch.int8), s))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    with pytest.raises(RuntimeError, match="do not fit"):
        ops.adaln_modulate_i8(x[:, :C], tab[:, 0], tab[:, 1], 2 * C, idx, True, outs[0][0][:5], outs[0][1])
    with pytest.raises(RuntimeError, match="do not fit"):
        ops.quant_rows_i8(torch.zeros(5, 128, dtype=torch.bfloat16, device=DEV), outs[0][0][:5, :64], outs[0][1][:5])


LOG_SHAPES = [(5, 512), (1025, 512), (1025, 3072), (1025, 5120), (5, 8192)]


def test_the_log_names_an_instance_of_its_own_per_shape_class():
    """YUME_NORM_LOG is read once per process: a child runs one quantiser call and one emitter call per (T, C) class"""
    env = dict(os.environ, YUME_NORM_LOG="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--log"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln.split() for ln in p.stderr.splitlines() if ln.startswith("[norm] ")]
    got = [(ln[1], int(ln[2].split("=")[1]), int(ln[3].split("=")[1])) for ln in lines]
    assert got == [(nc.instance(T, C), T, C) for T, C in LOG_SHAPES], got
    assert {g[0] for g in got} == {"adaln_i8<3>", "adaln2_i8", "adaln_i8<5>", "adaln_i8<8>"}
    quant = [ln for ln in p.stderr.splitlines() if ln.startswith("[quant] ")]
    assert quant == ["[quant] rows_i8 R=5 K=128 ldx=128 ldq=144"], quant


def main():
    _quant_raw(nc.make_input(5, 128).to(DEV), 128, 5, 128, 144, 5)
    for T, C in LOG_SHAPES:
        x, tab, idx = nc.make_emit_case(T, C, True, True)
        _emit_raw(x.to(DEV), tab.to(DEV), idx.to(DEV), True, 2 * C, T, C, C)


if __name__ == "__main__":
    if sys.argv[1:] != ["--log"]:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
