"""The split-K tail of the default GEMM (yume_gemm_bf16_ws / gemm_w4_kernel, yume_amd/csrc/gemm_w4.hpp) held to fp64, at shapes that reach
both branches of its plan, their edges and every refusal (tests/gemm_sk_plan.py mirrors the plan and names the cases). It is the one place
where workgroups exchange data inside a launch — partial tiles in a caller-owned scratch behind per-slot flags — and a whole-step
tolerance cannot see one wrong tile in 444, so:
  * the raw C-ABI is called with a workspace the test owns: after a launch the scratch itself says whether the path ran (the slots the plan
    uses hold partials, the others are still zero), whether it put its flags back, and whether a finisher gave up (the error word);
  * values are bounded per 256 x 256 tile as well as over the whole matrix (fp64 reference on the device, sample rows again on the host);
  * the tiles outside the cut tail are bit-identical to the same kernel without the plan (variant 3); launches repeat bit for bit, also on a
    scratch that holds another problem's partials.
One launch at a time, one process, no contention built on purpose: a starved finisher is the error word's business, not a test's."""
import math

import pytest
import torch

import gemm_sk_plan as skp

pytestmark = pytest.mark.gpu

from yume_amd import _lib, ops  # noqa: E402

DEV = "cuda"
SLOT, FLAGS_OFF = skp.SK_SLOT_BYTES, skp.FLAGS_OFFSET


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def bf(*shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * scale).to(torch.bfloat16)


def f32(*shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g) * scale


def operands(M, N, K, seed=1):
    return bf(M, K, seed=seed), bf(N, K, seed=seed + 1, scale=K ** -0.5), f32(N, seed=seed + 2)


def new_ws():
    n = int(_lib.load().yume_gemm_workspace_bytes())
    assert n == skp.workspace_bytes()
    return torch.zeros(n, dtype=torch.uint8, device=DEV)


def _p(t):
    return t.data_ptr() if t is not None else None


def raw_gemm(a, w, bias, out, epi, ws, variant=0, gate=None, gate_stride=0, row_idx=None, out_t=None, n_split=0):
    """yume_gemm_bf16_ws itself (no ops.gemm_bf16: the workspace is the caller's)"""
    lib = _lib.load()
    (M, K), N = a.shape, w.shape[0]
    rc = lib.yume_gemm_bf16_ws(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), _p(bias), M, N, K, epi, out.data_ptr(), out.stride(0),
                               _p(gate), gate_stride, _p(row_idx), _p(out_t), out_t.stride(0) if out_t is not None else 0, n_split, variant,
                               _p(ws), ws.numel() if ws is not None else 0, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "yume_gemm_bf16_ws")
    return out


def reference(a, w, bias):
    """fp64 on the device (the operands are exact bf16), in row blocks; ~8 sample rows are recomputed on the host so that the reference does
    not rest on one BLAS call alone: two fp64 sums of K <= 14336 products of magnitude O(1) differ by ~K * 2^-53 * |terms| < 1e-11, held
    to 1e-9 of the largest value"""
    M = a.shape[0]
    wd = w.double().t().contiguous()
    want = torch.empty(M, w.shape[0], dtype=torch.float64, device=DEV)
    for r0 in range(0, M, 8192):
        want[r0:r0 + 8192] = a[r0:r0 + 8192].double() @ wd
    if bias is not None:
        want += bias.double()
    rows = torch.tensor(sorted({0, 1, 255, 256, M // 2 + 1, max(0, M - 257), max(0, M - 245), M - 1}))
    host = a[rows.to(DEV)].double().cpu() @ w.double().cpu().t()
    if bias is not None:
        host += bias.double().cpu()
    assert (want[rows.to(DEV)].cpu() - host).abs().max().item() <= 1e-9 * max(1.0, host.abs().max().item()), "device and host fp64 disagree"
    return want


def tile_sums(x):
    """sum over every 256 x 256 tile of a [M, N] tensor -> [tiles_m, tiles_n]"""
    M, N = x.shape
    tm, tn = skp.tiles(M, N)
    p = torch.zeros(tm * 256, tn * 256, dtype=x.dtype, device=x.device)
    p[:M, :N] = x
    return p.view(tm, 256, tn, 256).sum(dim=(1, 3))


def check_values(got, want, K, what, report=None):
    """the GEMM bounds of test_ops_gpu.py::test_gemm_bf16_plain_and_f32 (fp32 accumulation of exact bf16 products), over the matrix and
    again per 256 x 256 tile: one wrong tile is not diluted by two thousand right ones"""
    d = got.double() - want
    bound = 2e-6 * math.sqrt(K) + 1e-6
    e2, w2 = tile_sums(d * d), tile_sums(want * want)
    per_tile = (e2 / w2.clamp_min(1e-300)).sqrt()
    worst = int(per_tile.argmax())
    tn = per_tile.shape[1]
    m0, n0 = worst // tn * 256, worst % tn * 256
    rel = math.sqrt(e2.sum().item() / w2.sum().item())
    mx, wmax = d.abs().max().item(), want.abs().max().item()
    print(f"{what}: rel-L2 {rel:.3e} max-abs {mx:.3e} (|want|max {wmax:.3f}) worst tile {per_tile.max().item():.3e} at (m0, n0) = ({m0}, {n0}); bound {bound:.3e}")
    if report is not None:
        report.update(rel_l2=rel, max_abs=mx, worst_tile=per_tile.max().item(), worst_at=(m0, n0))
    assert rel < bound, f"{what}: rel-L2 {rel:.3e} >= {bound:.3e}"
    assert mx < 1e-4 * max(1.0, wmax), f"{what}: max-abs {mx:.3e}"
    assert per_tile.max().item() < bound, f"{what}: tile (m0, n0) = ({m0}, {n0}) rel-L2 {per_tile.max().item():.3e} >= {bound:.3e}"


def check_scratch(ws, plan, what):
    """after a synchronize: the error word first (a finisher that timed out is another finding than a numeric mismatch), then the flags,
    then the slots: the plan's (s - 1) R hold partials, every other one is as it was handed over"""
    torch.cuda.synchronize()
    assert not bool(ws[-64:].any()), f"{what}: a finisher timed out (the scratch's error word is set)"
    assert not bool(ws[FLAGS_OFF:FLAGS_OFF + skp.SK_MAX_SLOTS * skp.SK_FLAG_STRIDE].any()), f"{what}: a flag was not returned to zero"
    used = (ws[:FLAGS_OFF].view(skp.SK_MAX_SLOTS, SLOT) != 0).any(dim=1).cpu()
    n = plan.slots if plan is not None else 0
    print(f"{what}: slots holding partials {int(used.sum())} (plan: {n})")
    assert bool(used[:n].all()), f"{what}: slots {[i for i in range(n) if not used[i]][:8]} of the plan's {n} were never written"
    assert not bool(used[n:].any()), f"{what}: slots beyond the plan's {n} were written: {[i for i in range(n, 256) if used[i]][:8]}"


def differing_tiles(x, y):
    """{(m0, n0)} of the 256 x 256 tiles in which any element differs bit for bit"""
    ne = tile_sums((x.view(torch.int32) != y.view(torch.int32)).to(torch.float32)).cpu()
    return {(int(i) * 256, int(j) * 256) for i, j in ne.nonzero()}


def plan_of(name, M, N, K):
    p, why = skp.plan(M, N, K, _ncu())
    if _ncu() == 256:
        assert p is not None and tuple(p[:8]) == skp.AT_256[name], (name, p, why)
    elif p is None:
        pytest.skip(f"{name}: the plan refuses this shape at {_ncu()} CUs ({why}); the case list is laid out for 256")
    return p


def test_case_list_covers_the_plan_space_on_this_device():
    if _ncu() != 256:
        pytest.skip(f"{_ncu()} CUs: the coverage of the case list is asserted at 256 (values are still checked per case)")
    skp.check_coverage_at_256()


# ------------------------------------------------------------------------------------------- every accepted case of the table
@pytest.mark.parametrize("name,M,N,K", skp.ACCEPTED, ids=[c[0] for c in skp.ACCEPTED])
def test_tail_values_scratch_and_untouched_tiles(name, M, N, K):
    plan = plan_of(name, M, N, K)
    print(f"{name}: M {M} N {N} K {K} -> {plan}")
    a, w, bias = operands(M, N, K)
    want = reference(a, w, bias)
    ws = new_ws()
    o0 = raw_gemm(a, w, bias, torch.empty(M, N, dtype=torch.float32, device=DEV), ops.EPI_F32, ws)
    check_scratch(ws, plan, name)                                          # 2. the path ran, and as the mirror says
    check_values(o0, want, K, name)                                        # 1. values, per tile too
    # 3. the same kernel without the plan: only cut tiles may differ (their K sum is split), and they do (another summation order)
    o3 = raw_gemm(a, w, bias, torch.empty(M, N, dtype=torch.float32, device=DEV), ops.EPI_F32, None, variant=3)
    diff = differing_tiles(o0, o3)
    print(f"{name}: tiles differing from the whole-tile launch {len(diff)} of R = {plan.R}")
    assert 1 <= len(diff) <= plan.R, (len(diff), plan.R)
    assert diff <= set(skp.tail_tiles(M, N, plan)), f"tiles outside the cut tail differ: {sorted(diff - set(skp.tail_tiles(M, N, plan)))[:8]}"
    # 4. run to run, on the scratch the first launch left
    o1 = raw_gemm(a, w, bias, torch.empty(M, N, dtype=torch.float32, device=DEV), ops.EPI_F32, ws)
    check_scratch(ws, plan, name + " (second launch)")
    assert torch.equal(o1, o0)


@pytest.mark.parametrize("name,M,N,K,why", skp.REFUSED, ids=[c[0] for c in skp.REFUSED])
def test_refused_shapes_leave_the_scratch_alone(name, M, N, K, why):
    p, got = skp.plan(M, N, K, _ncu())
    if _ncu() == 256:
        assert p is None and got == why
    elif p is not None:
        pytest.skip(f"{name}: accepted at {_ncu()} CUs")
    a, w, bias = operands(M, N, K)
    ws = new_ws()
    o0 = raw_gemm(a, w, bias, torch.empty(M, N, dtype=torch.float32, device=DEV), ops.EPI_F32, ws)
    torch.cuda.synchronize()
    assert not bool(ws.any()), "a refused shape wrote to the scratch"
    on = raw_gemm(a, w, bias, torch.empty(M, N, dtype=torch.float32, device=DEV), ops.EPI_F32, None)
    assert torch.equal(o0, on)


# ------------------------------------------------------------------------------------------- stale scratch
@pytest.mark.parametrize("name", ["q2_ragged", "s3_ragged"])               # branch A; branch B with s >= 3
def test_scratch_holding_another_problems_partials(name):
    """20 launches on ONE scratch, alternating two problems of one shape: every slot holds the other problem's partial when it is rewritten
    and every flag has been raised and lowered before. Each result equals, bit for bit, the same operands on a freshly zeroed scratch."""
    _, M, N, K = next(c for c in skp.ACCEPTED if c[0] == name)
    plan = plan_of(name, M, N, K)
    probs = []
    for seed in (11, 21):
        a, w, bias = operands(M, N, K, seed=seed)
        fresh_ws = new_ws()
        fresh = raw_gemm(a, w, bias, torch.empty(M, N, dtype=torch.float32, device=DEV), ops.EPI_F32, fresh_ws)
        check_scratch(fresh_ws, plan, f"{name} seed {seed}")
        probs.append((a, w, bias, fresh, reference(a, w, bias)))
    assert not torch.equal(probs[0][3], probs[1][3])
    ws = new_ws()
    for it in range(20):
        a, w, bias, fresh, want = probs[it & 1]
        got = raw_gemm(a, w, bias, torch.empty(M, N, dtype=torch.float32, device=DEV), ops.EPI_F32, ws)
        check_scratch(ws, plan, f"{name} launch {it}")
        assert torch.equal(got, fresh), f"launch {it}: differs from the freshly zeroed scratch in tiles {sorted(differing_tiles(got, fresh))[:8]}"
        check_values(got, want, K, f"{name} launch {it}")


# ------------------------------------------------------------------------------------------- epilogues
N_SPLIT = 1024


@pytest.mark.parametrize("epi", ["bf16", "gelu", "gelu_erf", "f32", "resid", "splitt"])
@pytest.mark.parametrize("name", ["q2_ragged", "s3_ragged"])
def test_tail_epilogues(name, epi):
    _, M, N, K = next(c for c in skp.ACCEPTED if c[0] == name)
    plan = plan_of(name, M, N, K)
    a, w, bias = operands(M, N, K, seed=5)
    want = reference(a, w, bias)
    ws = new_ws()
    tail = set(skp.tail_tiles(M, N, plan))
    if epi == "bf16":
        o = raw_gemm(a, w, bias, torch.empty(M, N, dtype=torch.bfloat16, device=DEV), ops.EPI_BF16, ws)
        assert (o.double() - want).abs().max() <= 2.0 ** -8 * want.abs().max() + 1e-6
    elif epi == "gelu":
        o = raw_gemm(a, w, bias, torch.empty(M, N, dtype=torch.bfloat16, device=DEV), ops.EPI_BF16_GELU, ws)
        wg = torch.nn.functional.gelu(want, approximate="tanh")
        assert (o.double() - wg).abs().max() <= 2.0 ** -7 * wg.abs().max() + 1e-5
    elif epi == "gelu_erf":
        o = raw_gemm(a, w, bias, torch.empty(M, N, dtype=torch.bfloat16, device=DEV), ops.EPI_BF16_GELU_ERF, ws)
        we = torch.nn.functional.gelu(want)
        assert (o.double() - we).abs().max() <= 2.0 ** -7 * we.abs().max() + 1e-5
    elif epi == "f32":
        o = raw_gemm(a, w, bias, torch.empty(M, N, dtype=torch.float32, device=DEV), ops.EPI_F32, ws)
        check_values(o, want, K, f"{name} f32")
    elif epi == "resid":
        # three gate rows in segments (the timesteps of a clip); both boundaries cross a tile of the cut tail, away from its edges
        bounds = (M - 700, M - 100)
        for b in bounds:
            assert b % 256 not in (0, 255) and all((b // 256 * 256, n0) in tail for n0 in range(0, N, 256)), "a segment boundary outside the cut tiles"
        idx = torch.zeros(M, dtype=torch.int32, device=DEV)
        idx[bounds[0]:] = 1
        idx[bounds[1]:] = 2
        x, tab = f32(M, N, seed=8), f32(3, 6, N, seed=9)
        o = raw_gemm(a, w, bias, x.clone(), ops.EPI_RESID, ws, gate=tab[:, 2], gate_stride=6 * N, row_idx=idx)
        wr = x.double() + want * tab[idx.long(), 2].double()
        assert (o.double() - wr).abs().max() < 1e-4 * max(1.0, wr.abs().max().item())
    else:
        # the cut tiles hold a complete last group of the grouped order: they lie on both sides of n_split, so the non-swapped operand order
        # (the K-major V^T tiles) is published and gathered too
        assert plan.R >= skp.GROUP_M * skp.tiles(M, N)[1] and {n0 < N_SPLIT for _, n0 in tail} == {True, False}
        Mp = (M + 7) // 8 * 8
        assert Mp > M
        qk = torch.empty(M, N_SPLIT, dtype=torch.bfloat16, device=DEV)
        vt = torch.zeros(N - N_SPLIT, Mp, dtype=torch.bfloat16, device=DEV)
        raw_gemm(a, w, bias, qk, ops.EPI_BF16_SPLITT, ws, out_t=vt, n_split=N_SPLIT)
        tol = 2.0 ** -8 * want.abs().max() + 1e-6
        assert (qk.double() - want[:, :N_SPLIT]).abs().max() <= tol
        assert (vt[:, :M].double() - want[:, N_SPLIT:].t()).abs().max() <= tol
        assert bool((vt[:, M:] == 0).all()), "padding columns of V^T were written"
    check_scratch(ws, plan, f"{name} {epi}")


# ------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("name", ["q23_lt4_full", "s10"])                  # one shape of each branch
def test_tail_scaling_by_two_is_exact(name):
    """A scaled by two (exact in bf16, in every fp32 partial sum and in their sum) doubles the result bit for bit — property (d) of
    test_fullsize_gpu.py::test_gemm_full_size_properties, here across published and gathered partials"""
    _, M, N, K = next(c for c in skp.ACCEPTED if c[0] == name)
    plan = plan_of(name, M, N, K)
    a, w, _ = operands(M, N, K, seed=7)
    ws = new_ws()
    o1 = raw_gemm(a, w, None, torch.empty(M, N, dtype=torch.float32, device=DEV), ops.EPI_F32, ws)
    check_scratch(ws, plan, name)
    o2 = raw_gemm((a.float() * 2).to(torch.bfloat16), w, None, torch.empty(M, N, dtype=torch.float32, device=DEV), ops.EPI_F32, ws)
    check_scratch(ws, plan, name + " (doubled)")
    assert torch.equal(o2, 2 * o1)


# ------------------------------------------------------------------------------------------- through ops.gemm_bf16
@pytest.mark.parametrize("name", ["5b_ffn2", "5b_ffn2_L12545", "14b_ffn2"])
def test_product_shapes_through_ops(name):
    """ffn.2 as the engine calls it (residual epilogue, gate rows by timestep segment) with the product's own workspace handling"""
    _, M, N, K = next(c for c in skp.ACCEPTED if c[0] == name)
    plan_of(name, M, N, K)
    a, w, bias = operands(M, N, K, seed=3)
    want = reference(a, w, bias)
    x, tab = f32(M, N, seed=8), f32(2, 6, N, seed=9)
    idx = (torch.arange(M, device=DEV) * 2 // M).to(torch.int32)
    got = ops.gemm_bf16(a, w, bias, x.clone(), ops.EPI_RESID, gate=tab[:, 5], gate_stride=6 * N, row_idx=idx)
    wr = x.double() + want * tab[idx.long(), 5].double()
    torch.cuda.synchronize()
    assert not ops.gemm_stream_k_error(), "a finisher timed out (ops.gemm_stream_k_error)"
    d = (got.double() - wr).abs()
    print(f"{name} through ops: max-abs {d.max().item():.3e} (|want|max {wr.abs().max().item():.3f})")
    assert d.max().item() < 1e-4 * max(1.0, wr.abs().max().item())
    # ... and per tile, on the GEMM's own term: (got - x) / gate against the fp64 product would divide by small gates; bound the error instead
    # by the tile's share: |got - wr| per tile in rel-L2 of the gated product
    g = tab[idx.long(), 5].double()
    e2, w2 = tile_sums((got.double() - wr) ** 2), tile_sums((want * g) ** 2)
    # the fp32 residual x (|x| ~ 1) is rounded once more when the product is added: 2^-24 |x + product| per element on top of the GEMM's bound
    bound = 2e-6 * math.sqrt(K) + 1e-6 + 2.0 ** -23
    per_tile = (e2 / w2.clamp_min(1e-300)).sqrt()
    worst = int(per_tile.argmax())
    assert per_tile.max().item() < bound, f"tile (m0, n0) = ({worst // per_tile.shape[1] * 256}, {worst % per_tile.shape[1] * 256}): {per_tile.max().item():.3e}"
    # the product's scratch is as a launch must leave it
    for (_, _), pws in ops._gemm_ws.items():
        assert not bool(pws[FLAGS_OFF:].any())
    assert not ops.gemm_stream_k_error()
