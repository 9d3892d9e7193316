"""Host proof of tests/gemm_cases.py: the table against the ABI's preconditions, the route mirror against its rows and against
gemm_sk_plan (the split-K tail is off everywhere), the four branches of w4_epilogue no earlier test reached, the fp64 reference against
torch's own linear, the per-element bound against an fp32 emulation of a correct kernel (zero violations) and against nine injected faults
(each flagged on every row it applies to), and the two activation allowances against an fp32 emulation of the kernels' formulas over a
dense grid. Every row runs at full size."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_cases as gc
import gemm_sk_plan as skp


SMALL = gc.CASES                                            # every row runs at full size on the host (the widest takes under three seconds)
IDS = [c.name for c in SMALL]


def emulate(c, ops, A=None, W=None, bias=None, idx=None, trunc=False, act=None, swap_geglu=False, drop_split=None):
    """what a correct kernel stores: an fp32 matmul (split-K: one per K slice, summed in order), bias in fp32, the epilogue in fp32, ONE
    rounding to nearest even for a bf16 output. The keyword arguments inject the faults."""
    A = (ops["A"] if A is None else A).float()
    W = (ops["W"] if W is None else W).float()
    if c.api == "splitk":
        Ks = c.K // c.splits
        parts = [A[:, s * Ks:(s + 1) * Ks] @ W[:, s * Ks:(s + 1) * Ks].t() for s in range(c.splits) if s != drop_split]
        y = parts[0]
        for p in parts[1:]:
            y = y + p
    else:
        y = A @ W.transpose(-1, -2)
    bias = ops["bias"] if bias is None else bias
    if bias is not None:
        y = y + bias
    if c.epi in (gc.EPI_GELU, gc.EPI_GELU_ERF):
        o = gc.gelu(y, act if act is not None else c.epi)
    elif c.epi == gc.EPI_GEGLU:
        g, v = y[..., 0::2], y[..., 1::2]
        if swap_geglu:
            g, v = v, g
        o = v * gc.gelu(g, c.epi)
    elif c.epi == gc.EPI_RESID:
        if ops["gate"] is not None:
            idx = ops["idx"] if idx is None else idx
            o = ops["x"] + y * (ops["gate"][idx.long()] if idx is not None else ops["gate"][0])
        else:
            o = ops["x"] + y
    else:
        o = y
    if c.epi in gc.BF16_OUT:
        o = (o.contiguous().view(torch.int32) & -65536).view(torch.float32) if trunc else o.bfloat16().float()
    return o.double()


@pytest.fixture(scope="module")
def made():
    cache = {}

    def get(c):
        if c.name not in cache:
            cache.clear()                                   # (one row at a time: the widest reference holds five [4231, 4096] fp64 arrays)
            ops = gc.make_case(c)
            cache[c.name] = (ops, gc.reference(c, ops))
        return cache[c.name]
    return get


def outside(c, r, got):
    return int(((got - r["ref"]).abs() > gc.bound(c, r)).sum())


# ------------------------------------------------------------------------------------------------ the table
def test_the_table_meets_the_abi_and_names_every_route():
    names = [c.name for c in gc.CASES]
    assert len(set(names)) == len(names)
    from yume_amd import ops as O
    assert (gc.EPI_BF16, gc.EPI_GELU, gc.EPI_F32, gc.EPI_RESID, gc.EPI_SPLITT, gc.EPI_GELU_ERF, gc.EPI_GEGLU) == \
        (O.EPI_BF16, O.EPI_BF16_GELU, O.EPI_F32, O.EPI_RESID, O.EPI_BF16_SPLITT, O.EPI_BF16_GELU_ERF, O.EPI_BF16_GEGLU)
    for c in gc.CASES:
        lda, ldw, ldo, ldt = gc.strides(c)
        assert c.route in gc.ROUTES, c.name
        assert c.K % 64 == 0 and c.N % 4 == 0 and lda % 8 == 0 and ldw % 8 == 0 and ldo % 4 == 0 and ldo >= gc.out_cols(c), c.name
        assert (c.row0 * ldo * gc.out_elem_bytes(c)) % 16 == 0, c.name                            # the out pointer: 16-byte aligned
        assert c.K in (64, 128, 192, 256) or (c.api == "splitk" and c.splits == 16), c.name
        if c.slices:
            assert (c.K * 2) % 16 == 0 and lda == ldw == 2 * c.K, c.name                          # W's pointer, K elements in
        if c.epi == gc.EPI_SPLITT:
            assert c.n_split % 128 == 0 and 0 < c.n_split < c.N and ldt >= c.M and ldt % 4 == 0, c.name
        if c.epi == gc.EPI_GEGLU:
            assert c.N % 8 == 0 and not c.bias and ldo > c.N // 2, c.name
        if c.epi == gc.EPI_RESID:
            assert c.N % 4 == 0 and (c.gate == "seg") == bool(c.seg) and all(0 < b < c.M for b in c.seg), c.name
        if c.api == "batched":
            assert c.epi in (gc.EPI_BF16, gc.EPI_F32), c.name
            ops = gc.make_case(c)
            if c.form != "pattern":
                assert ops["a_view"][0] % 8 == 0 and ops["w_view"][0] % 8 == 0 and ops["a_view"][1][0] % 8 == 0 and ops["w_view"][1][0] % 8 == 0
        if c.api == "splitk":
            assert 1 <= c.splits <= 64 and c.K % (c.splits * 64) == 0 and c.N % 8 == 0 and (c.M * c.N) % 4 == 0, c.name
            assert c.epi != gc.EPI_SPLITT
        if c.pattern or c.form == "pattern":
            assert not c.bias and c.epi == gc.EPI_F32, c.name
    assert {c.route for c in gc.CASES} == set(gc.ROUTES)
    # the encoder forms of yume_amd/t5.py: heads interleaved in a row (strideA = 64 < lda), N = 64 under a tile, strideO = 64 < ldo
    sc, va = (next(c for c in gc.CASES if c.form == f) for f in ("scores", "values"))
    assert gc.strides(sc)[:3] == (384, 384, 128) and (sc.M, sc.N, sc.K) == (77, 128, 64)
    assert gc.strides(va)[:3] == (128, 128, 192) and (va.M, va.N, va.K) == (77, 64, 128)
    # one bit-exact pattern row per kernel
    assert {c.route for c in gc.CASES if c.pattern or c.form == "pattern"} == {"g128", "g256", "w4", "batched", "batched splitk_reduce"}
    sk = [c for c in gc.CASES if c.api == "splitk"]
    assert {c.splits for c in sk} == {2, 4, 16} and {c.M for c in sk} >= {3, 77} and {c.N for c in sk} == {256, 264}
    assert {c.epi for c in sk} == {gc.EPI_BF16, gc.EPI_GELU, gc.EPI_GELU_ERF, gc.EPI_F32, gc.EPI_RESID, gc.EPI_GEGLU}
    assert gc.kernel_of("[gemm_bf16] w4 M=1 N=256 K=192 epi=0 variant=3 lda=192 ldw=192 ldo=256 ldt=0 n_split=0 ws=0 batch=1") == "w4"


@pytest.mark.parametrize("c", gc.CASES, ids=[c.name for c in gc.CASES])
def test_the_mirror_names_the_rows_route_and_the_split_k_tail_is_off(c):
    assert " ".join(gc.route(c)) == c.route
    for ncu in (64, 104, 256):
        # run_case hands over no workspace; and were one handed over (yume_amd.ops does so from 2^24 outputs on), the plan would refuse
        assert gc.tail_plan(c, ncu, workspace=False) is None and gc.tail_plan(c, ncu, workspace=True) is None
        assert " ".join(gc.route(c, ncu, workspace=True)) == c.route
    if c.api == "ws":
        p, why = skp.plan(c.M, c.N, c.K, 256)
        assert p is None and (why in ("T<CUs", "R=0") or c.K // skp.BK < skp.SK_MIN_NK), (c.name, p, why)


def test_every_kernel_gets_the_epilogues_it_takes():
    by = {}
    for c in gc.CASES:
        if c.api == "ws" and " " not in c.route:
            by.setdefault((c.route, c.variant != 0), set()).add((c.epi, c.bias))
    six = {gc.EPI_BF16, gc.EPI_GELU, gc.EPI_GELU_ERF, gc.EPI_F32, gc.EPI_RESID, gc.EPI_SPLITT}
    for k in ("g128", "g256", "w4"):
        for e in six:
            assert {(e, True), (e, False)} <= by[(k, True)], (k, gc.EPI_NAMES[e])
        gates = {c.gate for c in gc.CASES if c.route == k and c.variant and c.epi == gc.EPI_RESID}
        assert gates == {None, "one", "inter", "seg"}, (k, gates)
    assert any(c.epi == gc.EPI_GEGLU and c.route == "g256" and (c.N // 2) % 256 for c in gc.CASES)
    # variant 3 below three K tiles names the 8-wave kernel; K = 192 is exactly three
    assert any(c.variant == 3 and c.K == 128 and c.route == "g256" for c in gc.CASES)
    assert {c.K for c in gc.CASES if c.route == "w4" and c.variant == 3} == {192, 256}
    # the tile walk of the 256 kernels: a short last group of M tiles and a tile count that is no multiple of 8
    assert any(c.route == "g256" and (c.M + 255) // 256 == 10 and ((c.M + 255) // 256 * ((c.N + 255) // 256)) % 8 for c in gc.CASES)
    # both row-split pairs, and the epilogues the issue names for the w4 + g128 one
    assert {c.epi for c in gc.CASES if c.route == "w4 g128"} == {gc.EPI_F32, gc.EPI_RESID, gc.EPI_SPLITT, gc.EPI_GELU}
    for c in gc.CASES:
        if " " in c.route and c.api == "ws":
            M_main, rem = gc.row_split(c.M, c.N)
            assert (M_main, rem) == (4096, 135)
            if c.gate == "seg":
                assert any(b > M_main for b in c.seg), "no row_idx boundary inside the remainder rows"
    # use_256 refusing on padded work although 192 tiles stand
    c = next(c for c in gc.CASES if c.name == "v0_padded_work_refused")
    assert (c.M + 255) // 256 * ((c.N + 255) // 256) >= 192 and not skp.use_256(c.M, c.N) and 257 <= c.M <= 384


def test_the_four_branches_of_w4_epilogue_no_earlier_test_reached_are_reached():
    seen = {}
    for c in gc.CASES:
        for b in gc.w4_branches(c):
            seen.setdefault(b, []).append(c)
    assert set(seen) == {"T", "T_ragged_chunk", "image", "image_ragged_chunk", "resid_cols", "resid_same_row_ragged_m", "row4", "row4_bf16_ldo",
                         "row4_resid_n_edge"}, sorted(seen)
    assert any(gc.strides(c)[2] % 8 == 4 for c in seen["row4_bf16_ldo"])                            # bf16 out with ldo % 8 != 0
    assert any(c.N % 8 == 4 and gc.strides(c)[2] % 8 == 0 for c in seen["image_ragged_chunk"])      # col_left < 8 in w4_store_image
    assert {260, 516} <= {c.N for c in seen["row4_resid_n_edge"]}                                   # RESID on an N-edge tile
    assert any(c.gate == "seg" and c.M % 256 for c in seen["resid_same_row_ragged_m"])              # the "same row" shortcut on clamped rows
    assert any(c.M == 257 for c in seen["image"]) and any(c.M % 8 and gc.strides(c)[3] % 8 == 0 for c in seen["T_ragged_chunk"])


# ------------------------------------------------------------------------------------------------ reference and bound
@pytest.mark.parametrize("c", SMALL, ids=IDS)
def test_the_fp64_reference_is_torchs_linear(c, made):
    ops, r = made(c)
    b = ops["bias"].double() if ops["bias"] is not None else None
    A, W = ops["A"].double(), ops["W"].double()
    if A.dim() == 3:                                        # the batched forms: one linear per head
        y = torch.stack([F.linear(a, w) for a, w in zip(A, W)])
        q = torch.stack([F.linear(a ** 2, w ** 2) for a, w in zip(A, W)])
    else:
        y, q = F.linear(A, W, b), F.linear(A ** 2, W ** 2)
    assert r["y"].dtype == torch.float64 and r["y"].shape == y.shape
    assert (r["y"] - y).abs().max().item() <= 1e-12 * max(1.0, y.abs().max().item())
    assert (r["Q"] - q).abs().max().item() <= 1e-12 * max(1.0, q.abs().max().item())
    if c.pattern or c.form == "pattern":
        want = torch.zeros(c.M, c.N, dtype=torch.float64)              # A = I: out[m, n] = W[n, m]
        want[:min(c.M, c.K)] = ops["W"].double().t()[:min(c.M, c.K)]
        assert torch.equal(r["ref"], want)


@pytest.mark.parametrize("c", SMALL, ids=IDS)
def test_fp32_emulation_of_a_correct_kernel_is_inside_the_bound_at_every_element(c, made):
    ops, r = made(c)
    got = emulate(c, ops)
    err = (got - r["ref"]).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / gc.bound(c, r))
    print(f"{c.name}: worst error / bound {ratio.max().item():.3f}")
    assert int((ratio > 1).sum()) == 0, ratio.max().item()
    if c.pattern or c.form == "pattern":
        assert torch.equal(got, r["ref"])


@pytest.mark.parametrize("c", SMALL, ids=IDS)
def test_the_bound_flags_every_injected_fault(c, made):
    ops, r = made(c)
    M, N, K = c.M, c.N, c.K
    batched = c.api == "batched" and c.form != "pattern"
    if c.pattern or c.form == "pattern":
        # the identity-like A: a swapped pair of output rows and a W read with the wrong row stride both break bit-exactness
        got = emulate(c, ops)
        assert not torch.equal(got[[1, 0] + list(range(2, M))], r["ref"])
        return
    # 1. one 8-element K chunk of one row dropped
    A = ops["A"].clone()
    A[..., M // 2, 8:16] = 0
    assert outside(c, r, emulate(c, ops, A=A)) > 0, "dropped K chunk"
    # 2. two output rows swapped
    if M > 1:
        got = emulate(c, ops)
        perm = list(range(M))
        perm[0], perm[M - 1] = perm[M - 1], perm[0]
        assert outside(c, r, got[..., perm, :]) > 0, "swapped rows"
    # 3. the bias of the neighbouring column group
    if c.bias:
        assert outside(c, r, emulate(c, ops, bias=ops["bias"].roll(4))) > 0, "neighbouring bias"
    # 4. the gate row of the neighbouring segment on the rows next to a boundary
    if c.gate == "seg":
        for b in c.seg:
            idx = ops["idx"].clone()
            idx[b - 2:b] = idx[b]
            assert outside(c, r, emulate(c, ops, idx=idx)) > 0, ("gate row", b)
    # 5. truncation instead of round-to-nearest-even
    if c.epi in gc.BF16_OUT:
        assert outside(c, r, emulate(c, ops, trunc=True)) > 0, "truncation"
    # 6. the other GELU
    if c.epi in (gc.EPI_GELU, gc.EPI_GELU_ERF):
        assert outside(c, r, emulate(c, ops, act=gc.EPI_GELU_ERF if c.epi == gc.EPI_GELU else gc.EPI_GELU)) > 0, "the other GELU"
    # 7. GEGLU's two factors exchanged
    if c.epi == gc.EPI_GEGLU:
        assert outside(c, r, emulate(c, ops, swap_geglu=True)) > 0, "GEGLU factors"
    # 8. the row stride of a strided operand off by 8
    if ops["store"] is not None:
        for which in ("a", "w"):
            kw = {which.upper(): gc.operand_view(ops, which, ld_err=8)}
            assert outside(c, r, emulate(c, ops, **kw)) > 0, ("ld + 8", which)
    else:
        assert not batched
    # 9. one split's partial left out of the split-K sum
    if c.api == "splitk":
        for s in (0, c.splits - 1):
            assert outside(c, r, emulate(c, ops, drop_split=s)) > 0, ("split", s)


def test_the_reference_reads_strided_operands_where_the_call_does():
    """the operands as views of the flat storage equal the logical ones; the views of the two encoder forms are the strides of t5.py"""
    for c in gc.CASES:
        if c.slices or (c.api == "batched" and c.form != "pattern"):
            ops = gc.make_case(c)
            assert torch.equal(gc.operand_view(ops, "a"), ops["A"]) and torch.equal(gc.operand_view(ops, "w"), ops["W"])
            assert not torch.equal(gc.operand_view(ops, "a", 8), ops["A"])
            lda, ldw, _, _ = gc.strides(c)
            assert ops["a_view"][1][-2] == lda and ops["w_view"][1][-2] == ldw


# ------------------------------------------------------------------------------------------------ the activation allowances
def _worst(got, ref, allow):
    err = np.abs(got - ref)
    assert np.all(np.isfinite(err)) and np.all(allow >= 0)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(allow, 1e-300))))


def _f32(v):
    return np.asarray(v, dtype=np.float32)


def _ulp_step(v, k):
    """v moved by k ulps (fp32), infinities and zeros left alone"""
    out = v.copy()
    fin = np.isfinite(v) & (v != 0)
    out[fin] = np.nextafter(v[fin], np.float32(np.inf) if k > 0 else np.float32(-np.inf))
    return out


GRID = np.unique(np.concatenate([np.linspace(-12, 12, (1 << 21) + 1), np.linspace(-1, 1, (1 << 18) + 1) * 2.0 ** -6])).astype(np.float32)


def test_gelu_tanh_allowance_covers_the_kernels_formula_with_one_more_ulp_on_exp2_and_rcp():
    """common.hpp gelu_tanh in fp32 steps: x2 = x x; t = c1 x2 + c0 (fused or not); u = x t; e = exp2(u); d = e + 1; r = rcp(d); x r — with
    a correctly rounded exp2 and reciprocal each moved ONE ulp either way (the instructions are stated to 1 ulp)"""
    c0 = np.float32(-2.0) * np.float32(0.7978845608028654) * np.float32(1.4426950408889634)
    c1 = c0 * np.float32(0.044715)
    x = GRID
    x64 = x.astype(np.float64)
    ref = gc.gelu(torch.from_numpy(x64), gc.EPI_GELU).numpy()
    allow = gc.tanh_allowance(torch.from_numpy(x64), torch.from_numpy(ref)).numpy()
    x2 = x * x
    worst = 0.0
    with np.errstate(over="ignore", divide="ignore", under="ignore"):
        for fused in (True, False):
            t = _f32(c1.astype(np.float64) * x2.astype(np.float64) + np.float64(c0)) if fused else _f32(c1 * x2) + c0
            u = x * t
            e0 = _f32(np.exp2(u.astype(np.float64)))
            for ke in (-1, 1):
                d = _ulp_step(e0, ke) + np.float32(1.0)
                r0 = _f32(1.0 / d.astype(np.float64))
                for kr in (-1, 1):
                    got = (x * _ulp_step(r0, kr)).astype(np.float64)
                    worst = max(worst, _worst(got, ref, allow))
    print(f"gelu_tanh: worst error / allowance {worst:.3f} over {x.size} arguments in [-12, 12] (C_TANH = {gc.C_TANH})")
    assert worst <= 1.0


def test_gelu_erf_allowance_covers_the_kernels_formula_with_one_more_ulp_on_erff():
    """0.5f * x * (1.0f + erff(x * 0.70710678f)) in fp32 steps, erff correctly rounded and moved one ulp either way"""
    x = GRID
    x64 = x.astype(np.float64)
    ref = gc.gelu(torch.from_numpy(x64), gc.EPI_GELU_ERF).numpy()
    allow = gc.erf_allowance(torch.from_numpy(x64), torch.from_numpy(ref)).numpy()
    t = x * np.float32(0.7071067811865476)
    e0 = _f32(torch.erf(torch.from_numpy(t.astype(np.float64))).numpy())
    worst = 0.0
    for k in (-1, 1):
        e = np.clip(_ulp_step(e0, k), np.float32(-1), np.float32(1))
        got = ((np.float32(0.5) * x) * (np.float32(1.0) + e)).astype(np.float64)
        worst = max(worst, _worst(got, ref, allow))
    print(f"gelu_erf: worst error / allowance {worst:.3f} over {x.size} arguments in [-12, 12] (C_ERF = {gc.C_ERF})")
    assert worst <= 1.0


def test_the_references_gelu_is_torchs_and_the_slope_constant_holds():
    x = torch.linspace(-12, 12, (1 << 20) + 1, dtype=torch.float64, requires_grad=True)
    for approx, epi in (("tanh", gc.EPI_GELU), ("none", gc.EPI_GELU_ERF)):
        want = F.gelu(x, approximate=approx)
        assert (gc.gelu(x, epi) - want).abs().max().item() <= 1e-14          # (torch's loses the negative tail to cancellation)
        (g,) = torch.autograd.grad(gc.gelu(x, epi).sum(), x)
        assert 1.12 < g.abs().max().item() <= gc.GELU_SLOPE
