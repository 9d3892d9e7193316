"""The text and vision encoder MODULES (yume_amd/t5.py T5Engine.encode, yume_amd/clip.py ClipEngine.encode, CLIPModel.visual) as a case table
with plain-torch fp64 mirrors, a per-token-row yardstick, a host fault table and the closure of the production GEMM routes. No device is
touched here: tests/test_encoder_cases_cpu.py proves the table on the CPU, tests/test_encoder_modules_gpu.py runs it on the device.

Mirrors. `t5_mirror` / `clip_mirror` restate the two encode functions in fp64. With `rounded=False` they are the exact function of the
weights they are given (the reference; with unrounded weights it is oracle/t5.py / oracle/clip.py, which are pinned to the reference classes).
With `rounded=True` every tensor the device stores is rounded where the device stores it:
  T5    h, qk, vt, the normalised P, att, ff and the final output to bf16; S and the residual stream to fp32;
  CLIP  the patch matrix, h, qk, vt, P, att, ff to bf16; xs and x to fp32.
CLIP's P is rounded AFTER normalising with the exact row max and sum; the flash kernels round the unnormalised exponentials exp(s - m_tile)
and divide by the fp32 sum at the end. Both are one bf16 rounding of a number in [0, 1] per (query, key): the difference is second order
(the relative error of each term is the same 2^-9, only the position of the division differs).
`packed_sd` gives the bf16-rounded linears the engines pack (norm weights, biases, cls / pos tables, T5's position tables and the token
embedding stay as they are, as in `ensure_packed`).

Yardstick. row_err(a, ref)[r] = |a_r - ref_r|_2 / |ref_r|_2 per token row; E = max_r row_err(mirror(rounded=True), mirror(rounded=False)).
The device must keep row_err(dev, ref)[r] <= 2 E on every row: its output is one more draw of the same rounding process (other summation order,
other exp / tanh / erf forms, all below one bf16 rounding of a stage output) and a row's L2 over >= 128 elements concentrates.

Faults (FAULTS). Host emulations through `fault=` of the mirrors; a case SEES a fault when some row of the faulted rounded mirror has
row_err > 4 E. Every fault names the cases that must see it.

Routes. `t5_linears` / `clip_linears` list the GEMMs of one layer in launch order, `routes` turns them into (linear, epilogue, "splitk" | "plain")
through ops.small_m_splits; `production_routes()` must be a subset of `table_routes()`.
"""
import functools
import math

import torch
import torch.nn.functional as F

from conftest import load_golden
from yume_amd import ops, synth

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)          # OpenAI CLIP preprocessing constants
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
T5_LINEAR = ("attn.q.weight", "attn.k.weight", "attn.v.weight", "attn.o.weight", "ffn.gate.0.weight", "ffn.fc1.weight", "ffn.fc2.weight")
CLIP_LINEAR = ("patch_embedding.weight", "attn.to_qkv.weight", "attn.proj.weight", "mlp.0.weight", "mlp.2.weight")


def row_err(a, ref):
    a, ref = a.double().reshape(-1, a.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    return (a - ref).norm(dim=1) / ref.norm(dim=1)


def packed_sd(sd, linear):
    """the state dict with the linears the engine packs rounded to bf16 (held as fp32)"""
    return {k: (v.to(BF16).float() if k.endswith(linear) else v) for k, v in sd.items()}


def _rnd(on, dtype):
    return (lambda t: t.to(dtype).double()) if on else (lambda t: t)


# ------------------------------------------------------------------------------------------------------------------------------ T5
def t5_buckets(rel, num_buckets, max_dist=128):
    """T5RelativeEmbedding (bidirectional) of the reference: bucket of rel = j - i"""
    nb = num_buckets // 2
    out = (rel > 0).long() * nb
    rel = rel.abs()
    max_exact = nb // 2
    large = max_exact + (torch.log(rel.float() / max_exact) / math.log(max_dist / max_exact) * (nb - max_exact)).long()
    large = torch.min(large, torch.full_like(large, nb - 1))
    return out + torch.where(rel < max_exact, rel, large)


def _rms(x, w, eps=1e-6):
    return w * (x * torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps))


def _gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x.pow(3))))


T5_FAULTS = ("bias_shift", "drop_last_key", "geglu_swap", "stale_key", "head_v_shift")


def t5_mirror(sd, cfg, ids, rounded, fault=None, taps=None):
    """ids [n] -> fp64 [n, dim]. `taps` (a dict) receives the last layer's h, q, k, v, S, P, att, ff and x for bisecting a finding.
    faults: bias_shift      every logit takes the bias of slot j - i + n (the table read one slot to the right)
            drop_last_key   the softmax and P.V run over keys 0 .. n - 2
            geglu_swap      fc1 goes through the GELU and gate multiplies
            stale_key       a softmax over n + 1 keys: key row n (here a copy of row n // 2 with the value negated, bias 0) gets weight
            head_v_shift    head h multiplies head h + 1's V (cyclic)"""
    assert fault is None or fault in T5_FAULTS
    r16, r32 = _rnd(rounded, BF16), _rnd(rounded, F32)
    H = cfg["num_heads"]
    ids = ids.reshape(-1)
    n = ids.numel()
    x = sd["token_embedding.weight"].double()[ids]
    rel = torch.arange(n).unsqueeze(0) - torch.arange(n).unsqueeze(1)
    if fault == "bias_shift":
        rel = (rel + 1).clamp(max=n - 1)
    bk = t5_buckets(rel, cfg["num_buckets"])
    W = lambda k: sd[k].double()
    for i in range(cfg["num_layers"]):
        p = f"blocks.{i}."
        emb = W("pos_embedding.embedding.weight" if cfg.get("shared_pos", False) else p + "pos_embedding.embedding.weight")
        bias = emb[bk].permute(2, 0, 1)                                              # [H, n, n]
        h = r16(_rms(x, W(p + "norm1.weight")))
        q = r16(h @ W(p + "attn.q.weight").t()).view(n, H, -1).transpose(0, 1)       # [H, n, d]
        k = r16(h @ W(p + "attn.k.weight").t()).view(n, H, -1).transpose(0, 1)
        v = r16(h @ W(p + "attn.v.weight").t()).view(n, H, -1).transpose(0, 1)
        if fault == "stale_key":
            k = torch.cat([k, k[:, n // 2:n // 2 + 1]], dim=1)
            v = torch.cat([v, -v[:, n // 2:n // 2 + 1]], dim=1)
            bias = torch.cat([bias, torch.zeros(H, n, 1, dtype=F64)], dim=2)
        if fault == "drop_last_key" and n > 1:
            k, v, bias = k[:, :-1], v[:, :-1], bias[:, :, :-1]
        if fault == "head_v_shift":
            v = torch.roll(v, -1, dims=0)
        S = r32(q @ k.transpose(1, 2))                                               # no 1/sqrt(d)
        P = r16(torch.softmax(S + bias, dim=-1))
        att = r16(P @ v).transpose(0, 1).reshape(n, -1)
        x = r32(x + att @ W(p + "attn.o.weight").t())
        h2 = r16(_rms(x, W(p + "norm2.weight")))
        g, f1 = h2 @ W(p + "ffn.gate.0.weight").t(), h2 @ W(p + "ffn.fc1.weight").t()
        if fault == "geglu_swap":
            g, f1 = f1, g
        ff = r16(f1 * _gelu_tanh(g))
        x = r32(x + ff @ W(p + "ffn.fc2.weight").t())
        if taps is not None:
            taps.update(h=h, q=q, k=k, v=v, S=S, P=P, att=att, ff=ff, x=x)
    return r16(_rms(x, W("norm.weight")))


# ---------------------------------------------------------------------------------------------------------------------------- CLIP
CLIP_FAULTS = ("scale128", "drop_last_key", "no_cls", "no_pos", "quick_gelu")
PREPROCESS_FAULTS = ("mean_std_reversed", "no_half")


def clip_preprocess(videos, size, fault=None):
    """CLIPModel.visual's preprocessing of the reference in CPU fp32: videos a list of [3, T, H, W] in [-1, 1] -> [sum T, 3, size, size];
    the frames keep the order of torch.cat over the videos. faults: mean_std_reversed (channel order B, G, R of both), no_half (no *0.5+0.5)"""
    assert fault is None or fault in PREPROCESS_FAULTS
    v = torch.cat([F.interpolate(u.float().transpose(0, 1), size=(size, size), mode="bicubic", align_corners=False) for u in videos])
    if fault != "no_half":
        v = v * 0.5 + 0.5
    mean, std = (CLIP_MEAN[::-1], CLIP_STD[::-1]) if fault == "mean_std_reversed" else (CLIP_MEAN, CLIP_STD)
    return (v - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)


def clip_mirror(sd, cfg, x, nblk, rounded, fault=None):
    """x [B, 3, S, S] -> fp64 [B, 1 + patches, dim] after `nblk` blocks.
    faults: scale128 (softmax scale 128^-1/2, the padded head width), drop_last_key (key L - 1 left out), no_cls (row 0 without the class
    embedding), no_pos (no position table), quick_gelu (x sigmoid(1.702 x) in place of the erf GELU)"""
    assert fault is None or fault in CLIP_FAULTS
    r16, r32 = _rnd(rounded, BF16), _rnd(rounded, F32)
    C, H, ps, eps = cfg["dim"], cfg["num_heads"], cfg["patch_size"], cfg["norm_eps"]
    g = cfg["image_size"] // ps
    B, L, d = x.shape[0], g * g + 1, C // H
    W = lambda k: sd[k].double()
    ln = lambda t, name: F.layer_norm(t, (C,), W(name + ".weight"), W(name + ".bias"), eps)
    a = r16(x.double().view(B, 3, g, ps, g, ps).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, 3 * ps * ps))
    t = r32(a @ W("patch_embedding.weight").reshape(C, -1).t())
    cls = W("cls_embedding").expand(B, -1, -1)
    t = torch.cat([torch.zeros_like(cls) if fault == "no_cls" else cls, t], dim=1)
    if fault != "no_pos":
        t = r32(t + W("pos_embedding"))
    t = r32(ln(t, "pre_norm"))
    scale = (128 if fault == "scale128" else d) ** -0.5
    for i in range(nblk):
        p = f"transformer.{i}."
        h = r16(ln(t, p + "norm1"))
        qkv = r16(h @ W(p + "attn.to_qkv.weight").t() + W(p + "attn.to_qkv.bias")).view(B, L, 3, H, d)
        q, k, v = (u.transpose(1, 2) for u in qkv.unbind(2))                         # [B, H, L, d]
        if fault == "drop_last_key":
            k, v = k[:, :, :-1], v[:, :, :-1]
        P = r16(torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1))
        att = r16(P @ v).transpose(1, 2).reshape(B, L, C)
        t = r32(t + att @ W(p + "attn.proj.weight").t() + W(p + "attn.proj.bias"))
        h = r16(ln(t, p + "norm2"))
        u = h @ W(p + "mlp.0.weight").t() + W(p + "mlp.0.bias")
        ff = r16(u * torch.sigmoid(1.702 * u) if fault == "quick_gelu" else 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0))))
        t = r32(t + ff @ W(p + "mlp.2.weight").t() + W(p + "mlp.2.bias"))
    return t


# ---------------------------------------------------------------------------------------------------------------------------- table
T5_SPLITK_CFG = synth.tiny_t5_cfg(dim=512, heads=8, ffn=1024, layers=2, vocab=1000)
T5_SPLITK_SEED = 20
T5_SPLITK_N = (1, 64, 65, 128, 129, 300, 512, 1024)
CLIP_257_CFG = synth.tiny_clip_cfg(dim=640, heads=8, layers=2, image=224)
CLIP_257_SEED = 21
VISUAL_SIZE = (70, 90)


def t5_ids(cfg, n, seed):
    return torch.randint(1, cfg["vocab"], (n,), generator=torch.Generator().manual_seed(seed))


def _shared(sd, cfg):
    """the state dict of the shared_pos=True module tree: block 0's table at the top, none in the blocks"""
    out = {k: v for k, v in sd.items() if "pos_embedding" not in k}
    out["pos_embedding.embedding.weight"] = sd["blocks.0.pos_embedding.embedding.weight"]
    return out


def _gelu_probe(sd):
    return {k: (v * 4.0 if k.endswith("mlp.2.weight") else v - 2.0 if k.endswith("mlp.0.bias") else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _families():
    """family -> (kind, cfg, raw state dict)"""
    t5_tiny, clip_tiny = load_golden("t5_tiny"), load_golden("clip_tiny")
    live_t5 = synth.tiny_t5_cfg(dim=128, heads=2, ffn=192, layers=3, vocab=300)
    live_clip = synth.tiny_clip_cfg(dim=160, heads=2, layers=2, image=42)
    small_shared = dict(t5_tiny["cfg"], shared_pos=True)
    return {
        "t5_live": ("t5", live_t5, synth.make_t5_state_dict(live_t5, 9)),
        "t5_small": ("t5", t5_tiny["cfg"], synth.make_t5_state_dict(t5_tiny["cfg"], t5_tiny["seed"])),
        "t5_small_shared": ("t5", small_shared, _shared(synth.make_t5_state_dict(t5_tiny["cfg"], t5_tiny["seed"]), small_shared)),
        "t5_splitk": ("t5", T5_SPLITK_CFG, synth.make_t5_state_dict(T5_SPLITK_CFG, T5_SPLITK_SEED)),
        "clip_live": ("clip", live_clip, synth.make_clip_state_dict(live_clip, 2)),
        "clip_tiny": ("clip", clip_tiny["cfg"], synth.make_clip_state_dict(clip_tiny["cfg"], clip_tiny["seed"])),
        "clip_257": ("clip", CLIP_257_CFG, synth.make_clip_state_dict(CLIP_257_CFG, CLIP_257_SEED)),
        # No stock-weight case sees quick_gelu: with pre-activations ~ N(0, 1) the two forms differ by <= 0.021 where the GELU is O(1), 2.3 ..
        # 3.2 E at the output, and scaling mlp.2 alone (x 4 .. x 64) scales E with it (3.4 E). The forms differ RELATIVELY most on the negative
        # side (at u = -2: erf -0.0455, quick -0.0644): mlp.0's bias moved by -2 puts the pre-activations there, mlp.2 x 4 makes up for the
        # smaller GELU outputs. Measured: every row at >= 4 E, the worst at 19 E.
        "clip_tiny_gelu": ("clip", clip_tiny["cfg"], _gelu_probe(synth.make_clip_state_dict(clip_tiny["cfg"], clip_tiny["seed"]))),
    }


def family(name):
    return _families()[name]


def visual_videos(count):
    """`count` videos [3, 2, 70, 90] in [-1, 1] for CLIPModel.visual (frames 2 per video)"""
    g = torch.Generator().manual_seed(40)
    return [torch.rand((3, 2) + VISUAL_SIZE, generator=g) * 2 - 1 for _ in range(count)]


@functools.lru_cache(maxsize=None)
def _cases():
    """id -> dict(family, inp, nblk): `inp` is ids [n] (T5), images [B, 3, S, S] (CLIP); a visual case holds `videos` as well"""
    live_ids = torch.randint(1, 300, (2, 150), generator=torch.Generator().manual_seed(1))
    out = {"t5_live-150": dict(family="t5_live", inp=live_ids[0]), "t5_live-101of150": dict(family="t5_live", inp=live_ids[1, :101])}
    for n in (1, 63, 64, 65, 300):     # 300 (not asked for by the issue): the plain GEGLU kernel over two 256-row tiles, see test_route_closure
        out[f"t5_small-n{n}"] = dict(family="t5_small", inp=t5_ids(family("t5_small")[1], n, 100 + n))
    out["t5_small_shared-n65"] = dict(family="t5_small_shared", inp=out["t5_small-n65"]["inp"])
    for n in T5_SPLITK_N:
        out[f"t5_splitk-n{n}"] = dict(family="t5_splitk", inp=t5_ids(T5_SPLITK_CFG, n, 200 + n))
    # dim 160 is no multiple of 64 (the GEMMs' K tile): ClipEngine.ensure_packed refuses it, so this case ties the mirror to the reference
    # class on the CPU only, and the device test asserts the refusal
    out["clip_live"] = dict(family="clip_live", inp=torch.randn(1, 3, 42, 42, generator=torch.Generator().manual_seed(3)), use_31_block=True,
                            device=False)
    tiny_x = load_golden("clip_tiny")["x"]
    out["clip_tiny-31"] = dict(family="clip_tiny", inp=tiny_x, use_31_block=True)
    out["clip_tiny-all"] = dict(family="clip_tiny", inp=tiny_x, use_31_block=False)
    out["clip_tiny_gelu-31"] = dict(family="clip_tiny_gelu", inp=tiny_x, use_31_block=True)
    out["clip_257"] = dict(family="clip_257", inp=torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(5)), use_31_block=False)
    for count in (1, 2):
        videos = visual_videos(count)
        out[f"clip_visual-{count}"] = dict(family="clip_tiny", videos=videos, use_31_block=True,
                                           inp=clip_preprocess(videos, family("clip_tiny")[1]["image_size"]))
    return out


def case_ids(kind=None, device_only=False):
    return [c for c, d in _cases().items() if (kind is None or family(d["family"])[0] == kind) and (d.get("device", True) or not device_only)]


def case(cid):
    return _cases()[cid]


def nblk_of(cid):
    c = case(cid)
    cfg = family(c["family"])[1]
    return cfg["num_layers"] - 1 if c["use_31_block"] else cfg["num_layers"]


def mirror(cid, rounded, fault=None, packed=True):
    """the case's mirror; packed=False takes the raw (unrounded) weights: the function the oracles compute"""
    c = case(cid)
    kind, cfg, sd = family(c["family"])
    if kind == "t5":
        return t5_mirror(packed_sd(sd, T5_LINEAR) if packed else sd, cfg, c["inp"], rounded, fault)
    sd = packed_sd(sd, CLIP_LINEAR) if packed else sd
    if fault in PREPROCESS_FAULTS:
        return clip_mirror(sd, cfg, clip_preprocess(c["videos"], cfg["image_size"], fault), nblk_of(cid), rounded)
    return clip_mirror(sd, cfg, c["inp"], nblk_of(cid), rounded, fault)


@functools.lru_cache(maxsize=None)
def yardstick(cid):
    """(ref, E, row errors of the rounded mirror): computed once per case and process, shared, never written to"""
    ref = mirror(cid, False)
    err = row_err(mirror(cid, True), ref)
    return ref, err.max().item(), err


def sees(cid, fault):
    """-> (seen, rows above 4 E, rows, max row error)"""
    ref, E, _ = yardstick(cid)
    err = row_err(mirror(cid, True, fault), ref)
    return bool((err > 4 * E).any()), int((err > 4 * E).sum()), err.numel(), err.max().item()


# fault -> the cases that must see it (tests/test_encoder_cases_cpu.py measures the whole matrix and asserts these)
FAULTS = {
    "t5": {
        "bias_shift": ("t5_live-150", "t5_small-n65", "t5_splitk-n65", "t5_splitk-n300", "t5_splitk-n512", "t5_splitk-n1024"),
        "drop_last_key": ("t5_small-n65", "t5_splitk-n65", "t5_splitk-n300", "t5_splitk-n512"),
        "geglu_swap": ("t5_live-150", "t5_small-n1", "t5_small-n65", "t5_splitk-n1", "t5_splitk-n512", "t5_splitk-n1024"),
        "stale_key": ("t5_small-n63", "t5_small-n65", "t5_splitk-n65", "t5_splitk-n129"),
        "head_v_shift": ("t5_live-150", "t5_small-n65", "t5_splitk-n65", "t5_splitk-n1024"),
    },
    "clip": {
        "scale128": ("clip_tiny-31", "clip_257"),
        "drop_last_key": ("clip_tiny-31", "clip_257"),
        "no_cls": ("clip_live", "clip_tiny-31", "clip_257"),
        "no_pos": ("clip_live", "clip_tiny-31", "clip_257"),
        "quick_gelu": ("clip_tiny_gelu-31",),
        "mean_std_reversed": ("clip_visual-1", "clip_visual-2"),
        "no_half": ("clip_visual-1", "clip_visual-2"),
    },
}


# --------------------------------------------------------------------------------------------------------------------------- routes
EPI_NAME = {ops.EPI_BF16: "BF16", ops.EPI_F32: "F32", ops.EPI_RESID: "RESID", ops.EPI_BF16_SPLITT: "SPLITT", ops.EPI_BF16_GELU_ERF: "GELU_ERF",
            ops.EPI_BF16_GEGLU: "GEGLU"}


def t5_linears(cfg, n):
    """the dense GEMMs of one T5 layer in launch order: (linear, epilogue, M, N, K, small_m) — small_m: routed by ops.gemm_small_m"""
    C, Da, Dff = cfg["dim"], cfg["dim_attn"], cfg["dim_ffn"]
    return [("qkv", ops.EPI_BF16_SPLITT, n, 3 * Da, C, False), ("attn.o", ops.EPI_RESID, n, C, Da, True),
            ("gate|fc1", ops.EPI_BF16_GEGLU, n, 2 * Dff, C, True), ("fc2", ops.EPI_RESID, n, C, Dff, True)]


def clip_linears(cfg):
    """the dense GEMMs of one CLIP image: the patch embedding, then per block to_qkv, proj, mlp.0, mlp.2 (heads padded to 128 columns)"""
    C, H = cfg["dim"], cfg["num_heads"]
    L = (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1
    kp = (3 * cfg["patch_size"] ** 2 + 63) // 64 * 64
    M = int(C * cfg["mlp_ratio"])
    return [("patch_embedding", ops.EPI_F32, L - 1, C, kp, False), ("to_qkv", ops.EPI_BF16_SPLITT, L, 3 * H * 128, C, False),
            ("proj", ops.EPI_RESID, L, C, H * 128, True), ("mlp.0", ops.EPI_BF16_GELU_ERF, L, M, C, True), ("mlp.2", ops.EPI_RESID, L, C, M, True)]


def splits_of(lin):
    _, _, M, N, K, small_m = lin
    return ops.small_m_splits(M, N, K) if small_m else 1


def routes(linears):
    return {(lin[0], EPI_NAME[lin[1]], "splitk" if splits_of(lin) > 1 else "plain") for lin in linears}


def case_linears(cid):
    c = case(cid)
    kind, cfg, _ = family(c["family"])
    return t5_linears(cfg, c["inp"].numel()) if kind == "t5" else clip_linears(cfg)


def production_routes():
    out = routes(clip_linears(synth.CLIP_CFG_VIT_H))
    for n in range(1, 513):
        out |= routes(t5_linears(synth.T5_CFG_XXL, n))
    return out


def table_routes():
    """of the cases the device runs"""
    out = set()
    for cid in case_ids(device_only=True):
        out |= routes(case_linears(cid))
    return out
