"""yume_attn_fwd_kw on the GPU: a last key that counts `last_key_weight` times, on the 4-wave LDS-DMA kernel (variant 2), the short-key
kernel (variant 10, attn_short.hpp) and the automatic choice (variant 0).

The reference for every weighted case is the fp64 softmax over the EXPLICIT keys (n prompt keys followed by m = 512 - n copies of the pad
key: the reference models' formulation). Tolerances are the project's own for attention with P rounded to bf16 before P V
(tests/test_ops_gpu.py: max-abs <= 1.5e-2 of the value scale, rel-L2 < 6e-3 against fp64); between two bf16 formulations of the same
function rel-L2 < 1.2e-2 (test_attention_prescaled_q). A CPU model of the weighted path (one bf16 rounding of w e^s, fp32 accumulation, bf16
output) stays at rel-L2 <= 2.8e-3 and max-abs <= 5.8e-3 over these n, so the bounds leave room."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from yume_amd import ops  # noqa: E402

DEV = "cuda"
TEXT_LEN = 512
SHAPES = [(200, 2), (1030, 24), (2100, 5)]
CASES = [(n, v) for n in (0, 1, 62, 63, 64, 77, 126, 127) for v in (0, 2, 10)] + [(n, v) for n in (128, 191, 300, 511) for v in (0, 2)]


def rnd(*shape, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def attn_ref(q, k, v, scale):
    qd, kd, vd = (t.double().transpose(0, 1) for t in (q, k, v))      # [H, L, D]
    a = torch.softmax(qd @ kd.transpose(1, 2) * scale, dim=-1)
    return (a @ vd).transpose(0, 1)                                     # [Lq, H, D]


def prescale(q, scale=1 / math.sqrt(128)):
    return (q.double() * (scale * math.log2(math.e))).to(torch.bfloat16)


def run(q, k, v, weight=1.0, variant=0, padded=False, prescaled=False, scale=None, acc=None, use_ops_default=False):
    """one call; padded: the operands the engine hands over (K rows and V^T columns up to a whole 64-key tile, zeros); otherwise tight
    operands whose V^T padding columns hold NaN bits (they must never reach the result)."""
    Lq, H, D = q.shape
    Lk = k.shape[0]
    if padded:
        Lp = (Lk + 63) // 64 * 64
        kp = torch.zeros(Lp, H * D, dtype=torch.bfloat16, device=DEV)
        kp[:Lk] = k.reshape(Lk, H * D).to(DEV)
        kk = kp[:Lk]
        vt = torch.zeros(H * D, Lp, dtype=torch.bfloat16, device=DEV)
    else:
        kk = k.reshape(Lk, H * D).to(DEV)
        vt = torch.empty(H * D, (Lk + 7) // 8 * 8, dtype=torch.bfloat16, device=DEV).fill_(float("nan"))
    ops.transpose_bf16(v.reshape(Lk, H * D).to(DEV), vt)
    out = torch.empty(Lq, H * D, dtype=torch.bfloat16, device=DEV) if acc is None else acc
    kw = {} if use_ops_default else dict(last_key_weight=weight)
    ops.attn_fwd(q.reshape(Lq, H * D).to(DEV), kk, vt, out, Lq, Lk, H, scale=scale, accumulate=acc is not None, variant=variant,
                 q_prescaled=prescaled, kv_padded=padded, **kw)
    return out.cpu().view(Lq, H, D)


def explicit(k, v, n, m):
    """[n + 1] keys -> the n + m keys the reference attends over (key n repeated m times)"""
    H, D = k.shape[1:]
    return torch.cat([k[:n], k[n:n + 1].expand(m, H, D)]), torch.cat([v[:n], v[n:n + 1].expand(m, H, D)])


def check(got, want, what):
    e, mx, vs = rel_l2(got, want), (got.double() - want).abs().max().item(), max(want.abs().max().item(), 1e-3)
    print(f"{what}: rel-L2 {e:.3e} max-abs {mx:.3e} (value scale {vs:.3f})")
    assert torch.isfinite(got).all(), what
    assert mx <= 1.5e-2 * vs, (what, mx, vs)
    assert e < 6e-3, (what, e)


@pytest.mark.parametrize("Lq,H", SHAPES)
@pytest.mark.parametrize("n,variant", CASES)
def test_weighted_last_key_equals_explicit_copies(n, variant, Lq, H):
    m = TEXT_LEN - n
    scale = 1 / math.sqrt(128)
    q, k, v = (rnd(L, H, 128, seed=s, dtype=torch.bfloat16) for L, s in ((Lq, 1 + n), (n + 1, 2 + n), (n + 1, 3 + n)))
    tag = f"n={n} m={m} variant={variant} Lq={Lq} H={H}"
    for pad_key in ("random", "max", "low"):
        kk = k.clone()
        if pad_key == "max":                   # the pad key carries the row maximum for queries 3 and Lq - 1
            kk[n] = ((q[3].float() + q[Lq - 1].float()) * 1.5).to(torch.bfloat16)
        elif pad_key == "low":                 # far below the row maximum of query 7 (score about -34): m e^s is still a negligible share there
            kk[n] = (-3.0 * q[7].float()).to(torch.bfloat16)
        ke, ve = explicit(kk, v, n, m)
        want = attn_ref(q, ke, ve, scale)
        got = run(q, kk, v, weight=float(m), variant=variant)
        check(got, want, f"{tag} pad={pad_key} plain")
        if pad_key == "random":
            # the library's own plain call on the explicit keys: two bf16 formulations of one function
            lib_plain = run(q, ke, ve, variant=0, use_ops_default=True)
            assert rel_l2(got, lib_plain) < 1.2e-2
            assert torch.equal(run(q, kk, v, weight=float(m), variant=variant), got)      # run-to-run identical
        # the engine's form: prescaled q, padded operands
        qp = prescale(q)
        wantp = attn_ref(qp, ke, ve, math.log(2.0))
        gotp = run(qp, kk, v, weight=float(m), variant=variant, padded=True, prescaled=True)
        check(gotp, wantp, f"{tag} pad={pad_key} prescaled+padded")
    # prescaled without padding, plain with padding
    qp = prescale(q)
    ke, ve = explicit(k, v, n, m)
    check(run(qp, k, v, weight=float(m), variant=variant, prescaled=True), attn_ref(qp, ke, ve, math.log(2.0)), f"{tag} prescaled")
    check(run(q, k, v, weight=float(m), variant=variant, padded=True), attn_ref(q, ke, ve, scale), f"{tag} padded")
    # another scale
    check(run(q, k, v, weight=float(m), variant=variant, scale=0.3), attn_ref(q, ke, ve, 0.3), f"{tag} scale 0.3")
    # accumulate
    base = rnd(Lq, H * 128, seed=10, dtype=torch.bfloat16)
    want = attn_ref(q, ke, ve, scale) + base.view(Lq, H, 128).double()
    ga = run(q, k, v, weight=float(m), variant=variant, acc=base.to(DEV).clone())
    assert (ga.double() - want).abs().max() <= 2e-2 * want.abs().max()
    # asymmetric V (value = its own key index in d = 0, head index in d = 1, a pattern over the other features): catches key / head /
    # feature permutations and a weight on the wrong key
    v2 = torch.zeros(n + 1, H, 128)
    v2[:, :, 0] = torch.arange(n + 1).view(n + 1, 1) / 64.0
    v2[:, :, 1] = torch.arange(H).view(1, H) + 1.0
    v2[:, :, 2:] = (torch.arange(126).view(1, 1, 126) % 7) * 0.25 + (torch.arange(n + 1).view(n + 1, 1, 1) % 3) * 0.125
    v2 = v2.to(torch.bfloat16)
    ke2, ve2 = explicit(k, v2, n, m)
    w2 = attn_ref(q, ke2, ve2, scale)
    g2 = run(q, k, v2, weight=float(m), variant=variant)
    assert (g2.double() - w2).abs().max() <= 2e-2 * w2.abs().max()
    check(g2, w2, f"{tag} asymmetric V")


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("Lk", [78, 512, 2048])
def test_weight_one_through_the_new_export_is_todays_call(variant, Lk):
    """last_key_weight == 1 takes exactly the code path of yume_attn_fwd_ws: same kernel choice, same bits."""
    from yume_amd import _lib
    lib = _lib.load()
    for Lq, H in ((300, 3), (2100, 5)):
        q, k, v = (rnd(L, H, 128, seed=s, dtype=torch.bfloat16) for L, s in ((Lq, 1), (Lk, 2), (Lk, 3)))
        for prescaled, padded in ((False, False), (True, True)):
            qq = prescale(q) if prescaled else q
            # the raw export with weight 1 (ops.attn_fwd itself calls the old export at weight 1)
            Lp = (Lk + 63) // 64 * 64
            kp = torch.zeros(Lp, H * 128, dtype=torch.bfloat16, device=DEV)
            kp[:Lk] = k.reshape(Lk, H * 128).to(DEV)
            vt = torch.zeros(H * 128, Lp, dtype=torch.bfloat16, device=DEV)
            ops.transpose_bf16(v.reshape(Lk, H * 128).to(DEV), vt)
            qd = qq.reshape(Lq, H * 128).to(DEV)
            out = torch.empty(Lq, H * 128, dtype=torch.bfloat16, device=DEV)
            flags = variant | (ops.ATTN_Q_PRESCALED if prescaled else 0) | (ops.ATTN_KV_PADDED if padded else 0)
            rc = lib.yume_attn_fwd_kw(qd.data_ptr(), H * 128, kp.data_ptr(), H * 128, vt.data_ptr(), Lp, out.data_ptr(), H * 128, Lq, Lk, H,
                                      1 / math.sqrt(128), 0, flags, None, 0, 1.0, torch.cuda.current_stream().cuda_stream)
            _lib.check(rc, "yume_attn_fwd_kw")
            ref = torch.empty(Lq, H * 128, dtype=torch.bfloat16, device=DEV)
            rc = lib.yume_attn_fwd_ws(qd.data_ptr(), H * 128, kp.data_ptr(), H * 128, vt.data_ptr(), Lp, ref.data_ptr(), H * 128, Lq, Lk, H,
                                      1 / math.sqrt(128), 0, flags, None, 0, torch.cuda.current_stream().cuda_stream)
            _lib.check(rc, "yume_attn_fwd_ws")
            torch.cuda.synchronize()
            assert torch.equal(out, ref)
            # and ops.attn_fwd as it is called today (no workspace, as in the raw calls: with one, Lk >= 1536 may cut the last round into key ranges)
            today = torch.empty(Lq, H * 128, dtype=torch.bfloat16, device=DEV)
            ops.attn_fwd(qd, kp[:Lk], vt, today, Lq, Lk, H, variant=variant, use_workspace=False, q_prescaled=prescaled, kv_padded=padded)
            assert torch.equal(out, today)


@pytest.mark.parametrize("H", [1, 24, 40])
@pytest.mark.parametrize("Lk", [1, 5, 32, 33, 64, 100, 128])
def test_short_key_kernel_at_weight_one(Lk, H):
    """variant 10 without a weight against fp64: every key-block count, ragged Lq (one row, one short of / one over a 32-query unit, more units
    than waves), fewer units than waves, a head change inside one wave's range; run-to-run identical."""
    scale = 1 / math.sqrt(128)
    for Lq in (1, 31, 33, 4097):
        q, k, v = (rnd(L, H, 128, seed=s, dtype=torch.bfloat16) for L, s in ((Lq, 11), (Lk, 12), (Lk, 13)))
        want = attn_ref(q, k, v, scale)
        got = run(q, k, v, variant=10)
        check(got, want, f"variant 10 Lk={Lk} H={H} Lq={Lq}")
        assert torch.equal(run(q, k, v, variant=10), got)
        if Lq == 33:
            qp = prescale(q)
            check(run(qp, k, v, variant=10, prescaled=True, padded=True), attn_ref(qp, k, v, math.log(2.0)), f"variant 10 prescaled Lk={Lk} H={H}")
            assert rel_l2(got, run(q, k, v, variant=2)) < 6e-3          # the same function as the streaming kernel computes
