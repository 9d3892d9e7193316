"""yume_attn_fwd_seg on the GPU: several independent segments (own K / V^T / key count / last-key weight each) in ONE launch, on the segmented
short-key kernel (variant 10), the segmented 4-wave LDS-DMA kernel (variant 2) and the automatic choice (variant 0).

Reference: the fp64 softmax over each segment's EXPLICIT keys (the weighted key expanded into its copies, as in test_attn_key_weight_gpu.py).
Bounds: that file's, for attention with P rounded to bf16 before P V: max-abs <= 1.5e-2 of the value scale, rel-L2 < 6e-3 against fp64.

Shapes are the smallest at which the kernels can go wrong: one row, one over a 32-query unit, one over a 128-query block, several blocks;
a pitch equal to the segment and one rounded up to 64 rows (a gap that must keep its contents); key counts that leave whole key blocks of a
segment masked (78 beside 5), a full block (128), one key tile exactly (64), one over eight tiles (513); H = 1, where neighbouring units of
two segments have the same head. A wave of the short-key kernel walks more than one unit only beyond 4 x CU-count units, so the stale-K case
(the registers still hold the previous segment's keys) needs its own, long, case."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from yume_amd import ops  # noqa: E402

DEV = "cuda"
SCALE = 1 / math.sqrt(128)
# (Lk per segment, weight per segment); a third segment repeats the first one's shape with other data
SHORT_KEYS = [((78, 5), (434.0, 507.0)), ((5, 128), (1.0, 1.0)), ((128, 128), (1.0, 1.0))]
WAVE4_KEYS = [((512, 512), (1.0, 1.0)), ((78, 300), (434.0, 212.0)), ((64, 513), (1.0, 1.0))]
CASES = [(ks, v) for ks in SHORT_KEYS for v in (0, 2, 10)] + [(ks, v) for ks in WAVE4_KEYS for v in (0, 2)]
# (nseg, H, Lq_seg, pitch rounded up to 64): every value of every dimension, H = 1 with 2 and 3 segments, both pitches at every Lq_seg
COMBOS = [(2, 1, 1, False), (2, 3, 1, True), (2, 3, 33, True), (3, 1, 33, False), (3, 1, 130, True), (1, 3, 130, False),
          (3, 3, 300, False), (2, 1, 300, True)]
POISON = 77.0


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(torch.bfloat16)


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def attn_ref(q, k, v, scale):
    qd, kd, vd = (t.double().transpose(0, 1) for t in (q, k, v))      # [H, L, D]
    a = torch.softmax(qd @ kd.transpose(1, 2) * scale, dim=-1)
    return (a @ vd).transpose(0, 1)                                     # [Lq, H, D]


def prescale(q):
    return (q.double() * (SCALE * math.log2(math.e))).to(torch.bfloat16)


def explicit(k, v, w):
    """the keys the reference attends over: the last key repeated w times"""
    n, (H, D) = k.shape[0] - 1, k.shape[1:]
    return torch.cat([k[:n], k[n:].expand(int(w), H, D)]), torch.cat([v[:n], v[n:].expand(int(w), H, D)])


def check(got, want, what):
    e, mx, vs = rel_l2(got, want), (got.double() - want).abs().max().item(), max(want.abs().max().item(), 1e-3)
    print(f"{what}: rel-L2 {e:.3e} max-abs {mx:.3e} (value scale {vs:.3f})")
    assert torch.isfinite(got).all(), what
    assert mx <= 1.5e-2 * vs, (what, mx, vs)
    assert e < 6e-3, (what, e)


def seg_shapes(keys, nseg):
    Lks, ws = keys
    return (Lks + Lks[:1])[:nseg], (ws + ws[:1])[:nseg]


@functools.lru_cache(maxsize=None)
def problem(keys, nseg, H, Lq, seed=0):
    """inputs and fp64 references of one shape, computed once and shared by the variants: (q per segment, k, v, alternative k / v,
    reference, reference for the prescaled q)"""
    Lks, ws = seg_shapes(keys, nseg)
    qs = [rnd(Lq, H, 128, seed=seed + 10 * s + 1) for s in range(nseg)]
    ks = [rnd(Lk, H, 128, seed=seed + 10 * s + 2) for s, Lk in enumerate(Lks)]
    vs = [rnd(Lk, H, 128, seed=seed + 10 * s + 3) for s, Lk in enumerate(Lks)]
    k2 = [rnd(Lk, H, 128, seed=seed + 10 * s + 4) for s, Lk in enumerate(Lks)]
    v2 = [rnd(Lk, H, 128, seed=seed + 10 * s + 5) for s, Lk in enumerate(Lks)]
    ex = [explicit(k, v, w) for k, v, w in zip(ks, vs, ws)]
    ref = [attn_ref(q, ke, ve, SCALE) for q, (ke, ve) in zip(qs, ex)]
    refp = [attn_ref(prescale(q), ke, ve, math.log(2.0)) for q, (ke, ve) in zip(qs, ex)]
    return qs, ks, vs, k2, v2, ref, refp


def operands(ks, vs, H, padded):
    """device K / V^T of every segment with ONE row stride. padded: what the engine hands over (K rows and V^T columns up to a whole 64-key
    tile, zeros); otherwise tight K and V^T whose padding columns hold NaN bits (they must never reach the result)."""
    wmax = max(k.shape[0] for k in ks)
    kd, vd = [], []
    for k, v in zip(ks, vs):
        Lk = k.shape[0]
        if padded:
            kp = torch.zeros((Lk + 63) // 64 * 64, H * 128, dtype=torch.bfloat16, device=DEV)
            kp[:Lk] = k.reshape(Lk, H * 128).to(DEV)
            kd.append(kp[:Lk])
            vt = torch.zeros(H * 128, (wmax + 63) // 64 * 64, dtype=torch.bfloat16, device=DEV)
        else:
            kd.append(k.reshape(Lk, H * 128).to(DEV))
            vt = torch.full((H * 128, (wmax + 7) // 8 * 8), float("nan"), dtype=torch.bfloat16, device=DEV)
        ops.transpose_bf16(v.reshape(Lk, H * 128).to(DEV), vt)
        vd.append(vt)
    return kd, vd


def stack_q(qs, pitch):
    """the segments' queries at `pitch` rows; the rows of the gap hold NaN (nothing may read them into a result)"""
    Lq, H = qs[0].shape[:2]
    q = torch.full(((len(qs) - 1) * pitch + Lq, H * 128), float("nan"), dtype=torch.bfloat16)
    for s, x in enumerate(qs):
        q[s * pitch:s * pitch + Lq] = x.reshape(Lq, H * 128)
    return q.to(DEV)


def run(qd, kd, vd, Lq, pitch, Lks, ws, H, variant, out=None, **kw):
    o = torch.full_like(qd, POISON) if out is None else out
    ops.attn_fwd_seg(qd, kd, vd, o, Lq, pitch, list(Lks), H, variant=variant, last_key_weights=list(ws), accumulate=out is not None, **kw)
    return o


def segs(o, nseg, Lq, pitch, H):
    o = o.cpu()
    return [o[s * pitch:s * pitch + Lq].view(Lq, H, 128) for s in range(nseg)]


def gaps(o, nseg, Lq, pitch):
    return [o[s * pitch + Lq:(s + 1) * pitch] for s in range(nseg - 1)]


@pytest.mark.parametrize("keys,variant", CASES)
def test_segments_against_fp64(keys, variant):
    for nseg, H, Lq, pad64 in COMBOS:
        pitch = (Lq + 63) // 64 * 64 if pad64 else Lq
        Lks, ws = seg_shapes(keys, nseg)
        qs, ks, vs, k2, v2, ref, refp = problem(keys, nseg, H, Lq)
        tag = f"Lk={Lks} w={ws} variant={variant} nseg={nseg} H={H} Lq_seg={Lq} pitch={pitch}"
        qd = stack_q(qs, pitch)
        kd, vd = operands(ks, vs, H, padded=False)
        # 1. every segment within the bounds (tight operands, NaN bits behind Lk in V^T)
        o = run(qd, kd, vd, Lq, pitch, Lks, ws, H, variant)
        got = segs(o, nseg, Lq, pitch, H)
        for s in range(nseg):
            check(got[s], ref[s], f"{tag} segment {s} plain")
        # 4. the rows of the pitch gap keep what they held
        for g in gaps(o, nseg, Lq, pitch):
            assert (g == POISON).all(), tag
        # 2. run-to-run identical
        assert torch.equal(run(qd, kd, vd, Lq, pitch, Lks, ws, H, variant), o), tag
        # 5. one segment is the plain weighted call
        if nseg == 1:
            plain = torch.full_like(qd, POISON)
            ops.attn_fwd(qd, kd[0], vd[0], plain, Lq, Lks[0], H, variant=variant, last_key_weight=ws[0])
            assert torch.equal(plain, o), tag
        # 3. isolation: another K / V / weight in one segment leaves the other segments' bits alone
        for chg in range(min(nseg, 2) if nseg > 1 else 0):
            ka, va = list(ks), list(vs)
            ka[chg], va[chg] = k2[chg], v2[chg]
            wa = list(ws)
            wa[chg] = ws[chg] + 3.0
            kda, vda = operands(ka, va, H, padded=False)
            alt = segs(run(qd, kda, vda, Lq, pitch, Lks, wa, H, variant), nseg, Lq, pitch, H)
            for s in range(nseg):
                assert torch.equal(alt[s], got[s]) == (s != chg), (tag, chg, s)
        # the engine's form: prescaled q, padded operands; and prescaled q on the tight ones
        qpd = stack_q([prescale(q) for q in qs], pitch)
        kdp, vdp = operands(ks, vs, H, padded=True)
        op = run(qpd, kdp, vdp, Lq, pitch, Lks, ws, H, variant, q_prescaled=True, kv_padded=True)
        ot = run(qpd, kd, vd, Lq, pitch, Lks, ws, H, variant, q_prescaled=True)
        for s, (a, b) in enumerate(zip(segs(op, nseg, Lq, pitch, H), segs(ot, nseg, Lq, pitch, H))):
            check(a, refp[s], f"{tag} segment {s} prescaled+padded")
            check(b, refp[s], f"{tag} segment {s} prescaled")
        for g in gaps(op, nseg, Lq, pitch) + gaps(ot, nseg, Lq, pitch):
            assert (g == POISON).all(), tag
        if nseg == 1:
            plain = torch.full_like(qpd, POISON)
            ops.attn_fwd(qpd, kdp[0], vdp[0], plain, Lq, Lks[0], H, variant=variant, last_key_weight=ws[0], q_prescaled=True, kv_padded=True)
            assert torch.equal(plain, op), tag
        # accumulate: O += result, the gap rows keep the old O
        base = rnd(qd.shape[0], H * 128, seed=99)
        oa = run(qd, kdp, vdp, Lq, pitch, Lks, ws, H, variant, out=base.to(DEV).clone(), kv_padded=True)
        for s, a in enumerate(segs(oa, nseg, Lq, pitch, H)):
            want = ref[s] + base[s * pitch:s * pitch + Lq].view(Lq, H, 128).double()
            assert (a.double() - want).abs().max() <= 2e-2 * want.abs().max(), (tag, s)
        for s, g in enumerate(gaps(oa, nseg, Lq, pitch)):
            assert torch.equal(g.cpu(), base[s * pitch + Lq:(s + 1) * pitch]), tag


@pytest.mark.parametrize("variant", [0, 10])
def test_short_key_kernel_reloads_keys_at_a_segment_change_with_one_head(variant):
    """H = 1 and more (segment, query block) units than the launch has waves (4 per CU): a wave walks from the last unit of one segment
    into the first of the next with the SAME head — it has to reload K / V^T, and to take the new segment's key count and weight."""
    nseg, H, Lq = 3, 1, 32 * 1100 + 5
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert nseg * ((Lq + 31) // 32) >= 2 * 4 * cus, "the case no longer makes a wave walk several units"
    keys = ((37, 5), (3.0, 1.0))
    pitch = (Lq + 63) // 64 * 64
    Lks, ws = seg_shapes(keys, nseg)
    qs, ks, vs, _, _, ref, _ = problem(keys, nseg, H, Lq, seed=500)
    kd, vd = operands(ks, vs, H, padded=False)
    o = run(stack_q(qs, pitch), kd, vd, Lq, pitch, Lks, ws, H, variant)
    for s, a in enumerate(segs(o, nseg, Lq, pitch, H)):
        check(a, ref[s], f"H=1 long variant={variant} segment {s}")
    for g in gaps(o, nseg, Lq, pitch):
        assert (g == POISON).all()
