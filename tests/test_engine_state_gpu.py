"""One DiTEngine used the way a sampling job uses it: many calls, changing shapes, prompts and options, captured graphs alive in between.
None of the state the engine keeps across calls (yume_amd/dit.py: the `_buf` workspaces, the context caches, the plan cache, the packed
weights; yume_amd/ops.py: the scratch tensors per device and stream) may reach a result.

The yardstick is BIT EQUALITY WITH A FRESH ENGINE: the expected output of a call is what a newly built engine, making only that call with
the step's option settings from construction on, returns (torch.equal). The fresh engine is the reference, the warm engine the code under
test; no tolerance appears in this file. Agreement with the fp32 oracle at these shapes is held by tests/test_dit_gpu.py,
tests/test_forward_cfg_gpu.py and tests/test_forward_batch_gpu.py, whose tiny 2-layer models and helpers are imported here.

 (a) test_call_sequence_equals_fresh: a scripted table of steps (entry point, shape, prompts, options) on one warm model per family;
     test_plan_cache_empties_under_a_cached_packed_clip: more than 64 clip shapes beside a packed clip.
 (b) test_poisoned_workspaces_equal_fresh: a shorter table; between every two steps the engine's own workspaces are overwritten — every
     zero=False tensor with NaN / 0xFF, the zero=True tensors of POISON_TABLE with finite noise (what a longer call leaves behind).
 (c) test_graph_*: what a captured graph was handed stays alive (and untouched by anyone else) across shape changes and option flips of
     the engine it was captured from; c1 / c2 carry the host-only ownership assertion in front of their replays.

Shapes, plain latents (F, H, W) -> L = F (H/2) (W/2), padded rows ceil(L / 64) * 64: L120 -> 128, L70 -> 128, L90 -> 128, L64 -> 64 (no
padding), L300 -> 320, and the FramePack-packed clip of tests/test_forward_cfg_gpu.py per family. Prompts of 23, 9 and 0 tokens, text_len 64.

Whether a conditioning was recomputed is read from a call counter around DiTEngine._text_ctx (the existing cache tests compare the cache
keys; neither YUME_GEMM_LOG, read once per process, nor the _timed brackets, which the context GEMMs do not pass through, can tell)."""
import functools

import pytest
import torch

import test_forward_batch_gpu as fb
import test_forward_cfg_gpu as fc
from yume_amd import framepack, ops, synth
from yume_amd.dit import DiTEngine, _round_up

pytestmark = pytest.mark.gpu
DEV = fc.DEV
FAMILIES = ("wan23", "wan")
PLAIN = dict(fc.PLAIN, L120=(2, 10, 24), L70=(2, 10, 14))
N_PROMPT = {"a": 23, "a2": 23, "m": 23, "b": 9, "z": 0}      # a2: other values in a's shape; m: the tensor the script updates in place
T_OF = (250.0, 610.0)
# every switch of the engine a step can set; a step's options are these defaults with its own on top, on the warm and on the fresh engine
DEFAULTS = dict(cache_context=False, trim_last_block=False, dedup_pad_keys=False, q_prescale=True, fp8_ffn=False, fp8_ffn_fused=False,
                fp8_qkv=False, int8_qkv=False, fp6_ffn=False, fp8_attn=False, window_size=(-1, -1))


# ---------------------------------------------------------------------------------------------------------------- inputs, models, calls
def shape_of(family, kind):
    """(F, H, W, lfz, packed) of a kind"""
    if kind == "packed":
        return fc.PACKED[family] + (True,)
    return PLAIN[kind] + (8 if family == "wan23" else 9, False)


@functools.lru_cache(maxsize=None)
def prompts(family):
    """the prompts as device tensors: the SAME objects in every call of a family (the context caches key on address, version and shape)"""
    cfg = synth.tiny_cfg(family)
    g = torch.Generator().manual_seed(71)
    return {k: torch.randn((n, cfg["text_dim"]), generator=g).to(DEV) for k, n in N_PROMPT.items()}


@functools.lru_cache(maxsize=None)
def dev_case(family, kind):
    """the device inputs of one shape, made once: two samples (latents, timestep and, on the 14B architecture, y and CLIP tokens of their
    own), the keyword arguments of forward / forward_cfg (fc.kwargs) and those of forward_batch (fb.common)"""
    cfg = synth.tiny_cfg(family)
    F, H, W, lfz, packed = shape_of(family, kind)
    plan = framepack.pack_plan(F, H, W, lfz, (F - 9) if family == "wan" else None) if packed else None
    L = plan.seq_len if packed else F * (H // 2) * (W // 2)
    sm = []
    for s in range(2):
        inp = synth.make_dit_inputs(cfg, family, F, H, W, n_text=1, seed=72 + s)
        if family == "wan23" and packed:
            t = torch.cat([torch.zeros(plan.n_hist_tok), torch.full((plan.n_new_tok,), T_OF[s])]).unsqueeze(0).double()
        else:
            t = torch.tensor([T_OF[s]])
        sm.append(dict(inp, t=t))
    cs = dict(inp=sm[0], t=sm[0]["t"], L=L, lfz=lfz, packed=packed)
    one = fc.kwargs(family, cs)
    many = dict(fb.common(family, cs), t=torch.cat([v["t"] for v in sm]).to(DEV))
    if family == "wan":
        many.update(y=[v["y"].to(DEV) for v in sm], clip_fea=torch.cat([v["clip_fea"] for v in sm]).to(DEV))
    return dict(L=L, x=[v["x"].to(DEV) for v in sm], one=one, many=many, F=F, hp=H // 2, wp=W // 2)


@functools.lru_cache(maxsize=None)
def block_case(family, kind):
    """arguments of DiTEngine.block_forward at a plain shape: residual rows, one modulation row, the RoPE table, an embedded context"""
    cfg = synth.tiny_cfg(family)
    d = dev_case(family, kind)
    C, L = cfg["dim"], d["L"]
    n_img = 257 if family == "wan" else 0
    g = torch.Generator().manual_seed(73)
    x = torch.randn((L, C), generator=g).to(DEV)
    e = (0.1 * torch.randn((1, 6, C), generator=g)).to(DEV)
    ctx = torch.randn((n_img + cfg["text_len"], C), generator=g).to(DEV)
    rope = framepack.rope_cos_sin([(0, d["F"], d["hp"], d["wp"])], 128).to(DEV)
    return x, e, rope, ctx, n_img


def build(family):
    return fc._build(family)[2]


def set_options(eng, opts):
    assert set(opts) <= set(DEFAULTS), sorted(set(opts) - set(DEFAULTS))
    for k, v in DEFAULTS.items():
        setattr(eng, k, opts.get(k, v))


def call(m, family, kind, entry, who, x=None):
    """one call of an entry point on the device tensors of (family, kind) -> the list of its DEVICE outputs. x: latents to use instead of
    the case's (a list, one per sample: the static inputs of a captured graph)"""
    d = dev_case(family, kind)
    p = prompts(family)
    x = d["x"] if x is None else x
    if entry == "fwd":
        return [m([x[0]], context=[p[who[0]]], **d["one"])[0]]
    if entry == "cfg":
        return list(m.forward_cfg([x[0]], context=[p[who[0]]], context_null=[p[who[1]]], **d["one"]))
    if entry == "batch":
        return list(m.forward_batch([x[0], x[1]], context=[p[who[0]], p[who[1]]], **d["many"]))
    assert entry == "block", entry
    bx, e, rope, ctx, n_img = block_case(family, kind)
    return [m.engine.block_forward(1, bx, e, rope, ctx, n_img=n_img)]


_FRESH = {}
_FRESH_MODEL = {}


def fresh(family, kind, entry, who, opts, x=None):
    """the reference: a newly built engine (over a second module with the same parameters) with the step's options from construction on
    makes this one call -> CPU outputs. Kept per (call, options, version of every prompt it reads) where the latents are the case's."""
    key = (family, kind, entry, who, tuple(sorted(opts.items())), tuple(prompts(family)[w]._version for w in who))
    if x is None and key in _FRESH:
        return _FRESH[key]
    if family not in _FRESH_MODEL:
        _FRESH_MODEL[family] = build(family)
    m = _FRESH_MODEL[family]
    m._engine = None                                    # the engine property builds a new DiTEngine: no workspace, no cache, nothing packed
    eng = m.engine
    assert isinstance(eng, DiTEngine) and not eng._ws and eng._packed_key is None
    set_options(eng, opts)
    out = [o.cpu() for o in call(m, family, kind, entry, who, x=x)]
    m._engine = None
    assert all(torch.isfinite(o).all() for o in out), (family, kind, entry, who, opts)
    if x is None:
        _FRESH[key] = out
    return out


# ---------------------------------------------------------------------------------------------------------------- (a) the script
def S(entry, kind, who, hazard=None, ctx_calls=None, mutate=None, same_as=None, **opts):
    """one step. hazard: the token count of the longer call whose K rows / V^T columns this call must find in its padding (asserted in
    front of the call). ctx_calls: how many conditionings the call has to embed (DiTEngine._text_ctx calls). mutate: a prompt updated in
    place in front of the call. same_as: index of an earlier step whose warm output this one must repeat bit for bit."""
    return dict(entry=entry, kind=kind, who=who, hazard=hazard, ctx_calls=ctx_calls, mutate=mutate, same_as=same_as, opts=opts)


# the padded self-attention operands of each entry point: (q|k buffer, V^T buffer, stacked segments)
HAZARD_BUFS = {"fwd": ("qk", "vt", 1), "cfg": ("qk_p", "vt_p", 2), "batch": ("qk_b", "vt_b", 2)}
CC = dict(cache_context=True)
QKV8, FFN8 = dict(fp8_qkv=True), dict(fp8_ffn=True)

SCRIPT = [
    S("fwd", "L90", ("a",)),                                                     # 0: the very first call; the last step repeats it
    # --- same padded size (128 rows), L shrinking and growing: the shorter call finds the longer one's K rows and V^T columns in its padding
    S("fwd", "L120", ("a",)), S("fwd", "L70", ("a",), hazard=120), S("fwd", "L120", ("b",)), S("fwd", "L90", ("a",), hazard=120),
    S("fwd", "L70", ("z",), hazard=90),
    S("cfg", "L120", ("a", "b")), S("cfg", "L70", ("a", "b"), hazard=120), S("cfg", "L120", ("b", "z")), S("cfg", "L90", ("a", "b"), hazard=120),
    S("cfg", "L70", ("a", "z"), hazard=90),
    S("batch", "L120", ("a", "b")), S("batch", "L70", ("a", "b"), hazard=120), S("batch", "L120", ("z", "a")),
    S("batch", "L90", ("a", "b"), hazard=120), S("batch", "L70", ("b", "a"), hazard=90),
    # --- across padded sizes and back: every workspace is replaced, and replaced again
    S("fwd", "L64", ("a",)), S("fwd", "L300", ("a",)), S("fwd", "L64", ("b",)), S("fwd", "L120", ("a",)),
    S("cfg", "L64", ("a", "b")), S("cfg", "L300", ("a", "b")), S("cfg", "L64", ("a", "b")), S("cfg", "L120", ("a", "b")),
    S("batch", "L300", ("a", "b")), S("batch", "L64", ("a", "b")), S("batch", "L120", ("a", "b")),
    # --- the packed clip, trim_last_block on / off alternating at one shape; with the byte buffers of the 8-bit options the trimmed block
    #     takes row views (grow_rows) of the tensors the full blocks use
    S("fwd", "packed", ("a",)), S("fwd", "packed", ("a",), trim_last_block=True), S("fwd", "packed", ("b",)),
    S("fwd", "packed", ("a",), trim_last_block=True, fp8_qkv=True, fp8_ffn=True, fp8_ffn_fused=True),
    S("fwd", "packed", ("a",), fp8_qkv=True, fp8_ffn=True, fp8_ffn_fused=True),
    S("fwd", "packed", ("a",), trim_last_block=True, int8_qkv=True, fp6_ffn=True),
    S("fwd", "packed", ("a",), trim_last_block=True, fp8_ffn=True),
    S("fwd", "packed", ("a",), trim_last_block=True, fp8_attn=True), S("fwd", "packed", ("a",), trim_last_block=True),
    S("cfg", "packed", ("a", "b"), trim_last_block=True), S("batch", "packed", ("a", "b"), trim_last_block=True),
    # --- the entry points interleaved at one shape under cache_context, on the same device tensors: each keeps its own cache, and
    #     block_forward, which shares forward's K / V^T buffers, resets forward's key
    S("fwd", "L90", ("a",), ctx_calls=1, **CC), S("cfg", "L90", ("a", "b"), ctx_calls=2, **CC), S("fwd", "L90", ("a",), ctx_calls=0, **CC),
    S("batch", "L90", ("a", "b"), ctx_calls=2, **CC), S("fwd", "L90", ("a",), ctx_calls=0, **CC), S("block", "L90", (), ctx_calls=0, **CC),
    S("fwd", "L90", ("a",), ctx_calls=1, **CC), S("cfg", "L90", ("a", "b"), ctx_calls=0, **CC), S("batch", "L90", ("a", "b"), ctx_calls=0, **CC),
    # --- a prompt change under cache_context: the same object updated in place, another tensor of the same shape, another length with
    #     dedup_pad_keys off and on (another key count, other ctx_* / kc_* buffers)
    S("fwd", "L90", ("m",), ctx_calls=1, **CC), S("fwd", "L90", ("m",), ctx_calls=0, **CC), S("fwd", "L90", ("m",), ctx_calls=1, mutate="m", **CC),
    S("fwd", "L90", ("a2",), ctx_calls=1, **CC), S("fwd", "L90", ("a",), ctx_calls=1, **CC), S("fwd", "L90", ("b",), ctx_calls=1, **CC),
    S("fwd", "L90", ("b",), ctx_calls=1, dedup_pad_keys=True, **CC), S("fwd", "L90", ("a",), ctx_calls=1, dedup_pad_keys=True, **CC),
    S("fwd", "L90", ("a",), ctx_calls=0, dedup_pad_keys=True, **CC), S("fwd", "L90", ("z",), ctx_calls=1, dedup_pad_keys=True, **CC),
    S("fwd", "L90", ("a",), ctx_calls=1, **CC),
    S("cfg", "L90", ("m", "b"), ctx_calls=2, **CC), S("cfg", "L90", ("m", "b"), ctx_calls=2, mutate="m", **CC),
    S("cfg", "L90", ("a", "b"), ctx_calls=2, dedup_pad_keys=True, **CC), S("cfg", "L90", ("a", "z"), ctx_calls=2, dedup_pad_keys=True, **CC),
    S("cfg", "L90", ("a", "z"), ctx_calls=0, dedup_pad_keys=True, **CC),
    S("batch", "L90", ("b", "a"), ctx_calls=2, dedup_pad_keys=True, **CC), S("batch", "L90", ("b", "a2"), ctx_calls=2, dedup_pad_keys=True, **CC),
    S("batch", "L90", ("b", "a2"), ctx_calls=0, dedup_pad_keys=True, **CC), S("batch", "L90", ("b", "a2"), ctx_calls=2, **CC),
    # --- options flipped on the warm engine and flipped back (the pack options re-pack; fp8_ffn_fused, fp8_attn and window_size are not part
    #     of the pack key); under cache_context where the context caches carry the pack key
    S("fwd", "L90", ("a",), **FFN8), S("cfg", "L90", ("a", "b"), **FFN8), S("fwd", "L90", ("a",)),
    S("fwd", "L90", ("a",), fp8_ffn_fused=True), S("fwd", "L90", ("a",), fp8_ffn=True, fp8_ffn_fused=True),
    S("batch", "L90", ("a", "b"), fp8_ffn=True, fp8_ffn_fused=True), S("fwd", "L90", ("a",), **FFN8), S("fwd", "L90", ("a",)),
    S("fwd", "L90", ("a",), ctx_calls=1, **QKV8, **CC), S("fwd", "L90", ("a",), ctx_calls=0, **QKV8, **CC), S("fwd", "L90", ("a",), ctx_calls=1, **CC),
    S("cfg", "L90", ("a", "b"), **QKV8), S("fwd", "L90", ("a",)),
    S("fwd", "L90", ("a",), int8_qkv=True), S("batch", "L90", ("a", "b"), int8_qkv=True), S("fwd", "L90", ("a",)),
    S("fwd", "L90", ("a",), fp6_ffn=True), S("cfg", "L90", ("a", "b"), fp6_ffn=True), S("fwd", "L90", ("a",)),
    S("fwd", "L90", ("a",), fp8_attn=True), S("fwd", "L300", ("a",), fp8_attn=True), S("fwd", "L70", ("a",), fp8_attn=True),
    S("cfg", "L90", ("a", "b"), fp8_attn=True), S("fwd", "L90", ("a",)),
    S("fwd", "L90", ("b",), dedup_pad_keys=True), S("batch", "L90", ("a", "b"), dedup_pad_keys=True), S("fwd", "L90", ("b",)),
    S("fwd", "L90", ("a",), q_prescale=False), S("cfg", "L90", ("a", "b"), q_prescale=False), S("batch", "L90", ("a", "b"), q_prescale=False),
    S("fwd", "L90", ("a",)),
    S("fwd", "L90", ("a",), window_size=(16, 0)), S("fwd", "packed", ("a",), window_size=(16, 0), trim_last_block=True),
    S("fwd", "L90", ("a",), window_size=(16, 0), fp8_attn=True), S("fwd", "L90", ("a",)), S("cfg", "L90", ("a", "b")),
    S("fwd", "L90", ("a",), fp8_qkv=True, int8_qkv=True), S("cfg", "L90", ("a", "b"), fp8_qkv=True, int8_qkv=True), S("fwd", "L90", ("a",), **QKV8),
    S("fwd", "L90", ("a",), fp8_ffn=True, fp6_ffn=True), S("batch", "L90", ("a", "b"), fp8_ffn=True, fp6_ffn=True), S("fwd", "L90", ("a",), **FFN8),
    S("fwd", "L90", ("a",), same_as=0),                                          # after the last flip-back: the very first call's bits
]

# (b): every entry point and every option, a shrinking L per entry point, a cache hit over poisoned scratch
POISON_SCRIPT = [
    S("fwd", "L120", ("a",)), S("fwd", "L70", ("a",), hazard=120), S("cfg", "L120", ("a", "b")), S("cfg", "L70", ("a", "b"), hazard=120),
    S("batch", "L120", ("a", "b")), S("batch", "L70", ("a", "b"), hazard=120),
    S("fwd", "L90", ("a",), ctx_calls=1, **CC), S("fwd", "L90", ("a",), ctx_calls=0, **CC), S("block", "L90", (), **CC),
    S("cfg", "L90", ("a", "b"), ctx_calls=2, dedup_pad_keys=True, **CC), S("cfg", "L90", ("a", "b"), ctx_calls=0, dedup_pad_keys=True, **CC),
    S("batch", "L90", ("b", "a"), ctx_calls=2, dedup_pad_keys=True, **CC), S("batch", "L90", ("b", "a"), ctx_calls=0, dedup_pad_keys=True, **CC),
    S("fwd", "packed", ("a",), trim_last_block=True, fp8_qkv=True, fp8_ffn=True, fp8_ffn_fused=True),
    S("fwd", "packed", ("a",), trim_last_block=True, int8_qkv=True, fp6_ffn=True), S("cfg", "L90", ("a", "b"), fp8_ffn=True),
    S("fwd", "L90", ("a",), fp8_attn=True), S("fwd", "L70", ("a",), fp8_attn=True, q_prescale=False), S("fwd", "L90", ("a",), window_size=(16, 0)),
    S("fwd", "L300", ("z",)), S("fwd", "L64", ("a",)),
]

# (b): the zero=True floating workspaces whose padding an earlier call at the same padded size can reach — what that call leaves there is
# finite and of the size of the operands themselves, so the poisoner replaces their whole content by N(0, 1) clipped to +-8. Every other
# zero=True buffer is left alone: kc_* / vct_* carry their row count in the name, rope_p / rope_b / the selectors are replaced whenever L
# changes, so their padding can only ever hold the zeros of the allocation.
POISON_TABLE = {
    "qk": "forward at L = 120 leaves K rows 70..119 (columns C..2C) in front of forward at L = 70: both pad to 128 rows",
    "vt": "... and the V^T columns 70..119 of every channel row",
    "qk_p": "forward_cfg at L = 120 leaves K rows 70..119 of leg 0 and 198..247 of leg 1 in front of forward_cfg at L = 70 (pitch 128)",
    "vt_p": "... and the same V^T columns of both legs",
    "qk_b": "forward_batch (B = 2) at L = 120 leaves K rows 70..119 and 198..247 in front of forward_batch at L = 70 (pitch 128)",
    "vt_b": "... and the same V^T columns of both samples",
    "att_p": "forward_cfg leaves the image branch's sums in the gap rows L..pitch-1 in front of the next forward_cfg at that L (re-zeroed by hand)",
    "att_b": "forward_batch leaves them in every gap in front of the next forward_batch at that L and B (re-zeroed by hand)",
}


def assert_stale_padding(eng, entry, L, L_long):
    """the hazard is there: the buffers a call at L tokens is about to reuse hold a longer call's K rows and V^T columns L .. L_long - 1 of
    every stacked segment. A refactor that re-zeroes or re-keys these buffers has to update this assertion (and POISON_TABLE) on purpose."""
    qn, vn, nseg = HAZARD_BUFS[entry]
    C, pitch = eng.model.dim, _round_up(L, 64)
    assert _round_up(L_long, 64) == pitch and L < L_long
    qk, vt = eng._ws[qn], eng._ws[vn]
    assert tuple(qk.shape) == (nseg * pitch, 2 * C) and tuple(vt.shape) == (C, nseg * pitch), (qn, tuple(qk.shape), tuple(vt.shape))
    for s in range(nseg):
        assert bool(qk[s * pitch + L:s * pitch + L_long, C:].any()), f"{qn}: K rows {L}..{L_long - 1} of segment {s} are all zero"
        assert bool(vt[:, s * pitch + L:s * pitch + L_long].any()), f"{vn}: V^T columns {L}..{L_long - 1} of segment {s} are all zero"


def poison(eng, zero_of, gen):
    """overwrite the engine's workspaces -> (names filled with NaN / 0xFF, names filled with noise). int32 tensors (row selectors) are left."""
    nan_names, noise_names = [], []
    for name, t in eng._ws.items():
        assert name in zero_of, name
        if not zero_of[name]:
            if t.dtype == torch.int32:
                continue
            if t.is_floating_point():
                t.fill_(float("nan"))
            else:
                assert t.dtype in (torch.uint8, torch.int8), (name, t.dtype)
                t.view(torch.uint8).fill_(0xFF)                  # NaN as e4m3, NaN as an E8M0 scale
            nan_names.append(name)
        elif name in POISON_TABLE:
            t.copy_(torch.randn(t.shape, generator=gen, device=t.device).clamp_(-8, 8).to(t.dtype))
            noise_names.append(name)
    # the scratch of yume_amd.ops per device and stream (NOT _gemm_ws and the ticket counters: their zeros are a contract)
    for table in (ops._attn_ws, ops._attn_batch_ws, ops._splitk_ws):
        for t in table.values():
            if t.is_cuda:
                t.fill_(float("nan")) if t.is_floating_point() else t.fill_(0xFF)
    return nan_names, noise_names


def run_script(family, script, monkeypatch, poisoned=False):
    m = build(family)
    eng = m.engine
    L_of = {k: dev_case(family, k)["L"] for k in set(s["kind"] for s in script)}
    ctx_calls = [0]
    text_ctx = eng._text_ctx

    def counted_text_ctx(*a, **k):
        ctx_calls[0] += 1
        return text_ctx(*a, **k)
    monkeypatch.setattr(eng, "_text_ctx", counted_text_ctx)
    zero_of = {}
    buf = eng._buf

    def recorded_buf(name, shape, dtype, zero=False, grow_rows=False):
        assert zero_of.setdefault(name, zero) == zero, name
        return buf(name, shape, dtype, zero=zero, grow_rows=grow_rows)
    monkeypatch.setattr(eng, "_buf", recorded_buf)
    gen = torch.Generator(device=DEV).manual_seed(74)
    seen, outs = (set(), set()), []
    for i, st in enumerate(script):
        what = (i, st["entry"], st["kind"], st["who"], st["opts"])
        if st["mutate"]:
            prompts(family)[st["mutate"]].mul_(0.5)              # an in-place update: the version counter moves, the address stays
        if poisoned and i:
            nan_names, noise_names = poison(eng, zero_of, gen)
            assert nan_names and noise_names, (what, nan_names, noise_names)      # a poisoner that touches nothing must fail
            seen[0].update(nan_names), seen[1].update(noise_names)
        elif st["hazard"]:
            assert_stale_padding(eng, st["entry"], L_of[st["kind"]], st["hazard"])
        set_options(eng, st["opts"])
        ctx_calls[0] = 0
        got = [o.cpu() for o in call(m, family, st["kind"], st["entry"], st["who"])]
        if st["ctx_calls"] is not None:
            assert ctx_calls[0] == st["ctx_calls"], (what, ctx_calls[0])
        if st["entry"] == "block":
            assert eng._ctx_key is None                          # forward's K / V^T buffers were overwritten: its next call recomputes them
        want = fresh(family, st["kind"], st["entry"], st["who"], st["opts"])
        assert len(got) == len(want)
        for j, (g, w) in enumerate(zip(got, want)):
            assert torch.equal(g, w), (what, j, (g.double() - w.double()).abs().max().item())
        if st["same_as"] is not None:
            assert all(torch.equal(g, w) for g, w in zip(got, outs[st["same_as"]])), what
        outs.append(got)
    if poisoned:
        print(f"{family}: {len(script)} steps; NaN / 0xFF into {sorted(seen[0])}; noise into {sorted(seen[1])}")
        assert seen[1] >= {"qk", "vt", "qk_p", "vt_p", "qk_b", "vt_b"}, sorted(seen[1])
    return m


@pytest.mark.parametrize("family", FAMILIES)
def test_call_sequence_equals_fresh(family, monkeypatch):
    assert len(SCRIPT) >= 40
    run_script(family, SCRIPT, monkeypatch)


@pytest.mark.parametrize("family", FAMILIES)
def test_plan_cache_empties_under_a_cached_packed_clip(family):
    """more than 64 distinct (F, H, W) plans while a packed clip's tables are cached: _plan_cache empties itself under them; the packed
    call afterwards builds them again and returns the fresh bits"""
    m = build(family)
    eng = m.engine
    want = fresh(family, "packed", "fwd", ("a",), {})
    assert torch.equal(call(m, family, "packed", "fwd", ("a",))[0].cpu(), want[0])
    key = packed_plan_key(eng)
    many_plans(m, family)
    assert key not in eng._plan_cache                            # the cache did empty itself
    assert torch.equal(call(m, family, "packed", "fwd", ("a",))[0].cpu(), want[0])
    assert key in eng._plan_cache


def packed_plan_key(eng):
    keys = [k for k in eng._plan_cache if k[0] == "p"]
    assert len(keys) == 1
    return keys[0]


def many_plans(m, family):
    """one eager forward at each of 81 plain shapes F = 1, H, W in {2, 4, ..., 18}: more plans than _plan_cache holds"""
    d = dev_case(family, "L64")
    g = torch.Generator(device=DEV).manual_seed(75)
    shapes = [(1, H, W) for H in range(2, 20, 2) for W in range(2, 20, 2)]
    assert len(shapes) > 64
    for F, H, W in shapes:
        kw = dict(d["one"], seq_len=F * (H // 2) * (W // 2))
        x = torch.randn((d["x"][0].shape[0], F, H, W), generator=g, device=DEV)
        if family == "wan":
            kw["y"] = [torch.randn((d["one"]["y"][0].shape[0], F, H, W), generator=g, device=DEV)]
        out = m([x], context=[prompts(family)["a"]], **kw)[0]
        assert out.shape[1:] == (F, H, W) and bool(torch.isfinite(out).all()), (F, H, W)
    assert len(m.engine._plan_cache) < len(shapes)


# ---------------------------------------------------------------------------------------------------------------- (b) poisoned workspaces
@pytest.mark.parametrize("family", FAMILIES)
def test_poisoned_workspaces_equal_fresh(family, monkeypatch):
    """no kernel reads an element of a torch.empty workspace before a kernel of the same call has written it, and what a longer call leaves
    in the padding of the zero=True operands (finite values) reaches no result: every step equals fresh bit for bit"""
    assert set(e for s in POISON_SCRIPT for e in (s["entry"],)) == {"fwd", "cfg", "batch", "block"}
    assert set(k for s in POISON_SCRIPT for k in s["opts"]) == set(DEFAULTS)
    run_script(family, POISON_SCRIPT, monkeypatch, poisoned=True)


# ---------------------------------------------------------------------------------------------------------------- (c) graph lifetimes
def storages(obj, out=None):
    """{storage address: bytes} of every tensor reachable through dicts, lists and tuples"""
    out = {} if out is None else out
    if torch.is_tensor(obj):
        st = obj.untyped_storage()
        out[st.data_ptr()] = st.nbytes()
    elif isinstance(obj, dict):
        for v in obj.values():
            storages(v, out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            storages(v, out)
    return out


def owned(eng):
    """every storage the engine references: workspaces, packed weights, per-clip tables and what it keeps for captured graphs"""
    return storages([eng._ws, eng.P, eng._plan_cache, getattr(eng, "_captured", [])])


def new_latents(like, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(v.shape, generator=g).to(DEV) for v in like]


def warm_and_capture(fn):
    """as the existing capture tests: one eager call, one on a side stream, then the capture -> (graph, the graph's output tensors)"""
    fn()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


class Captured:
    """one graph of one entry point at one shape, with static latents of its own"""

    def __init__(self, m, family, kind, entry, who, opts, record=None):
        self.family, self.kind, self.entry, self.who, self.opts = family, kind, entry, who, dict(opts)
        self.x = [v.clone() for v in dev_case(family, kind)["x"]]
        set_options(m.engine, opts)
        fn = lambda: call(m, family, kind, entry, who, x=self.x)
        if record is None:
            self.graph, self.out = warm_and_capture(fn)
            return
        # the tensors _buf hands out DURING the capture (by storage), and the packed weights the capture runs on
        eng, buf, on = m.engine, m.engine._buf, [False]

        def recorded_buf(*a, **k):
            t = buf(*a, **k)
            if on[0] and torch.cuda.is_current_stream_capturing():
                storages(t, record["ws"])
            return t
        eng._buf = recorded_buf
        try:
            on[0] = True
            self.graph, self.out = warm_and_capture(fn)
        finally:
            del eng._buf
        storages(eng.P, record["P"])
        assert record["ws"] and record["P"]

    def replay_equals_fresh(self, seed):
        for dst, src in zip(self.x, new_latents(self.x, seed)):
            dst.copy_(src)
        self.graph.replay()
        torch.cuda.synchronize()
        got = [o.cpu() for o in self.out]
        want = fresh(self.family, self.kind, self.entry, self.who, self.opts, x=self.x)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert torch.equal(g, w), (self.kind, self.entry, seed, (g.double() - w.double()).abs().max().item())


def scratch_like(sizes):
    """tensors of the given byte counts, every byte 0xFF (all-NaN under any floating view): the allocator hands out freed blocks of a size
    first, so had the engine given one of these back it would be here"""
    return [torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV) for n in sizes]


def graph_model(family):
    m = build(family)
    ops.ensure_counters(torch.device(DEV, torch.cuda.current_device()))
    return m


def release(m, *graphs):
    for c in graphs:
        del c.graph
    m.engine.release_captured()
    ops.release_captured()
    assert not m.engine._captured and not ops._captured


@pytest.mark.parametrize("family", FAMILIES)
def test_graph_survives_eager_calls_at_other_shapes(family):
    """c1: graph A captured from forward at L = 90; eager forwards at L = 300 and L = 64 replace the engine's workspaces. The HOST-ONLY
    assertion comes first: every storage the capture was handed is still referenced by the engine (without the pinning of
    DiTEngine._buf it fails here, in front of the replay). Then scratch tensors of the replaced sizes, all 0xFF; the replay on new latents
    equals the fresh eager call and leaves every scratch byte alone."""
    m = graph_model(family)
    eng = m.engine
    rec = dict(ws={}, P={})
    A = Captured(m, family, "L90", "fwd", ("a",), {}, record=rec)
    call(m, family, "L300", "fwd", ("a",))
    call(m, family, "L64", "fwd", ("a",))
    replaced = {p: n for p, n in rec["ws"].items() if p not in storages(eng._ws)}
    assert replaced, "the eager calls at other shapes replaced no workspace of the capture: the test is vacuous"
    have = owned(eng)
    lost = [p for p in list(rec["ws"]) + list(rec["P"]) if p not in have]
    assert not lost, f"{len(lost)} of {len(rec['ws']) + len(rec['P'])} storages a live graph was handed are no longer referenced by the engine"
    scratch = scratch_like(replaced.values())
    A.replay_equals_fresh(81)
    A.replay_equals_fresh(82)
    assert all(bool((s == 0xFF).all()) for s in scratch)
    release(m, A)


@pytest.mark.parametrize("family", FAMILIES)
def test_graph_survives_an_option_flip_that_repacks(family):
    """c2: captured with fp8_ffn on; the option is flipped off and one eager forward re-packs the weights. Ownership first (host only),
    then scratch of the outgoing weights' sizes; the replay equals the fresh fp8_ffn-on call."""
    m = graph_model(family)
    eng = m.engine
    rec = dict(ws={}, P={})
    A = Captured(m, family, "L90", "fwd", ("a",), dict(fp8_ffn=True), record=rec)
    assert any("w1q" in d for d in eng.P["blocks"])
    set_options(eng, {})
    call(m, family, "L90", "fwd", ("a",))
    assert not any("w1q" in d for d in eng.P["blocks"])
    replaced = {p: n for p, n in rec["P"].items() if p not in storages(eng.P)}
    assert replaced, "the option flip replaced no packed weight of the capture: the test is vacuous"
    have = owned(eng)
    lost = [p for p in list(rec["ws"]) + list(rec["P"]) if p not in have]
    assert not lost, f"{len(lost)} of {len(rec['ws']) + len(rec['P'])} storages a live graph was handed are no longer referenced by the engine"
    scratch = scratch_like(replaced.values())
    A.replay_equals_fresh(83)
    assert all(bool((s == 0xFF).all()) for s in scratch)
    set_options(eng, {})
    assert torch.equal(call(m, family, "L90", "fwd", ("a",))[0].cpu(), fresh(family, "L90", "fwd", ("a",), {})[0])
    release(m, A)


@pytest.mark.parametrize("family", FAMILIES)
def test_two_graphs_of_one_engine_alive_together(family):
    """c3: graphs at L = 90 and L = 120 from one engine (they share the 128-row q|k and V^T operands and nothing else), replayed A, B, A, B
    with new latents each time and one eager forward_cfg at L = 90 in the middle"""
    m = graph_model(family)
    A = Captured(m, family, "L90", "fwd", ("a",), {})
    B = Captured(m, family, "L120", "fwd", ("b",), {})
    A.replay_equals_fresh(84)
    B.replay_equals_fresh(85)
    got = [o.cpu() for o in call(m, family, "L90", "cfg", ("a", "b"))]
    assert all(torch.equal(g, w) for g, w in zip(got, fresh(family, "L90", "cfg", ("a", "b"), {})))
    A.replay_equals_fresh(86)
    B.replay_equals_fresh(87)
    release(m, A, B)


@pytest.mark.parametrize("family", FAMILIES)
def test_captured_cfg_and_batch_survive_the_other_kind(family):
    """c4: forward_cfg and forward_batch (B = 2) captured at L = 90; one eager call of the other kind at another shape, then the replay"""
    m = graph_model(family)
    A = Captured(m, family, "L90", "cfg", ("a", "b"), {})
    call(m, family, "L120", "batch", ("a", "b"))
    A.replay_equals_fresh(88)
    B = Captured(m, family, "L90", "batch", ("a", "b"), {})
    call(m, family, "L300", "cfg", ("a", "b"))
    B.replay_equals_fresh(89)
    A.replay_equals_fresh(90)
    release(m, A, B)


@pytest.mark.parametrize("family", FAMILIES)
def test_graph_survives_the_plan_cache_emptying(family):
    """the per-clip RoPE table and row selector a captured step reads live in _plan_cache, which empties itself past 64 clips: ownership
    first (host only), then the replay of the packed clip's graph equals fresh"""
    m = graph_model(family)
    eng = m.engine
    A = Captured(m, family, "packed", "fwd", ("a",), {})
    key = packed_plan_key(eng)
    tables = storages(eng._plan_cache[key])
    assert tables
    many_plans(m, family)
    assert key not in eng._plan_cache
    have = owned(eng)
    assert all(p in have for p in tables), "the per-clip tables a live graph reads are no longer referenced by the engine"
    scratch = scratch_like(tables.values())
    A.replay_equals_fresh(91)
    assert all(bool((s == 0xFF).all()) for s in scratch)
    release(m, A)
