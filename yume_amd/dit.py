"""DiT denoise engine: drives the HIP kernels (yume_amd.ops) for one WanModel forward.

The nn.Module classes in yume_amd/wan23/modules/model.py and yume_amd/wan/modules/model.py only hold the
parameters under the reference's state_dict key names and keep the reference call signatures; all compute
goes through this engine:

    pack (once)   q|k|v weights concatenated to one [3C, C] bf16 matrix, cross k|v to [2C, C], patch-embed
                  kernels flattened to GEMM operands, head weight split hi/lo for the fp32-accurate head GEMM,
                  block modulations stacked.
    per clip      FramePack plan, per-token RoPE (cos, sin) table and timestep-row selector, cached on device.
    per step      patch gather+GEMM -> fp32 residual stream; time MLP on the R distinct timesteps only
                  (R = 2 on the FramePack path: clean history and the current sigma) instead of all L tokens;
                  text MLP; per block: adaLN -> fused QKV GEMM (V written K-major) -> RMSNorm+RoPE ->
                  attention -> o-proj GEMM with gate*y+residual epilogue -> norm3 -> cross-attention ->
                  adaLN -> FFN (GELU fused) -> gate/residual epilogue; head; unpatchify.

HBM layout (L tokens, C hidden): residual stream x fp32 [L, C]; GEMM operands bf16 row-major [L, K];
q|k bf16 [L, 2C]; V^T bf16 [C, Lpad] (K-major, per head 128 rows); modulation tables fp32 [blocks, R, 6, C].
"""

import math
import os
import sys

import torch

from . import framepack, ops
from .ops import EPI_BF16, EPI_BF16_GELU, EPI_BF16_GELU_ERF, EPI_BF16_SPLITT, EPI_F32, EPI_RESID


def _round_up(a, b):
    return (a + b - 1) // b * b


class DiTEngine:
    def __init__(self, model, family):
        assert family in ("wan23", "wan")
        self.model = model
        self.family = family
        self._packed_key = None
        self._ws = {}
        self._plan_cache = {}
        self.prof = None   # dict kernel-group -> list of (start, end) HIP event pairs when bench.py profiles the timed steps
        self.prof_only = None   # set of group names: bracket only these (an event pair costs a few µs of queue time per call; ~330 calls per step)
        # the text / CLIP embeddings and every block's cross-attention K, V^T depend only on the
        # conditioning, not on the latent or the timestep; with cache_context they are computed once per conditioning
        # tensor (same object, same version) instead of once per denoise step. Off by default = the reference's work.
        self.cache_context = False
        # both families drop the history tokens before unpatchify (wan23/modules/model.py:860, wan/modules/model.py:1003-1005),
        # so in the LAST block the history rows only have to supply K / V to the self-attention: with trim_last_block their queries, o
        # projection, cross-attention and FFN are not computed (5B: 2420 of 9460 rows of one block). The returned velocity is unchanged
        # (GEMM / attention rows are independent). Off by default = the reference's work; bench.py reports it beside the headline.
        self.trim_last_block = os.environ.get("YUME_TRIM_LAST_BLOCK", "0") == "1"
        # r7: both families pad the prompt with ZERO rows up to text_len before text_embedding and attend over all text_len keys without a
        # key mask (wan23/modules/model.py:815-821, wan/modules/model.py:931-936). A zero row through Linear -> GELU -> Linear is one constant
        # vector, so for an n-token prompt the rows n .. text_len-1 of the embedded context, and of every block's cross-attention K and V, are
        # copies of one row. With dedup_pad_keys the engine embeds and projects n + 1 rows (the prompt and ONE zero row) and every text
        # cross-attention runs over n + 1 keys whose last one counts text_len - n times (yume_attn_fwd_kw): the same softmax, nothing
        # approximated, only the order of a few roundings changes. Off by default = the reference's work; env YUME_DEDUP_PAD_KEYS=1 turns it on.
        self.dedup_pad_keys = os.environ.get("YUME_DEDUP_PAD_KEYS", "0") == "1"
        # kernel selection passed to every GEMM / attention call: 0 = automatic (product setting); tests set (1, 1) to run the
        # whole model on the independent 128x128-tile GEMM and register-staged attention kernels as a cross-check (the register-staged
        # attention kernel takes no key weight: with dedup_pad_keys the text cross-attention of that mode runs variant 2)
        self.gemm_variant = 0
        self.attn_variant = 0
        # self-attention q leaves yume_rmsnorm_rope already multiplied by softmax scale * log2(e) (folded into the fp32 RMSNorm weight of q,
        # i.e. before q's one bf16 rounding) and yume_attn_fwd is told so (YUME_ATTN_Q_PRESCALED): the scores are the exponents.
        # YUME_ATTN_PRESCALE=0 keeps the scale inside the attention kernel (A/B and cross-checks).
        self.q_prescale = os.environ.get("YUME_ATTN_PRESCALE", "1") != "0"
        # a yume_amd.ulysses.SequenceParallel splits ONE chain's tokens over the ranks of its group
        self.sp = None
        self._ctx_key = None
        self._ctx_refs = None
        self._pair_ctx_key = None          # forward_pair's own conditioning cache (its K / V^T live in buffers of their own)
        self._pair_ctx_refs = None
        self._batch_ctx_key = None         # ... and forward_batch's
        self._batch_ctx_refs = None
        # forward_batch: the variant handed to ops.attn_fwd_batch for the self-attention of the stacked samples (0 = automatic: the persistent
        # kernel over (sample, head) pairs from 1536 keys on, the segmented 4-wave kernel below; 8 insists on the persistent kernel — tests
        # run it at a small L that way)
        self.batch_attn_variant = 0
        # forward_pair: issue the self-attention of the blocks >= 1 as ONE ops.attn_fwd_batch launch over the two legs instead of one
        # ops.attn_fwd launch per leg. Off by default = forward_pair as it was; env YUME_PAIR_SELF_BATCHED=1 turns it on (tools/batch_ab.py
        # measures both).
        self.pair_self_batched = os.environ.get("YUME_PAIR_SELF_BATCHED", "0") == "1"
        # r15: the two FFN linears of every block whose dim and ffn_dim are multiples of 128 in OCP e4m3 with one fp32 scale per token row and
        # per output channel (yume_quant_rows_e4m3 + yume_gemm_f8): weights quantised once at pack time, activations in front of each GEMM.
        # QKV, o and the cross projections stay bf16. Off by default = the bf16 calls, bit for bit; env YUME_FP8_FFN=1 turns it on. Part of
        # the pack key: flipping it re-packs.
        self.fp8_ffn = os.environ.get("YUME_FP8_FFN", "0") == "1"
        # r16: with fp8_ffn on (and only then), drop both quantiser passes: adaln_modulate_e4m3 -> gemm_f8 (MX_GELU) -> gemm_f8_mx (RESID), the
        # activations between the two GEMMs as e4m3 with power-of-two scales per 32 columns (_ffn_block). Off by default = fp8_ffn as r15
        # shipped it, bit for bit; env YUME_FP8_FFN_FUSED=1 turns it on. Not part of the pack key: the packed weights are the same.
        self.fp8_ffn_fused = os.environ.get("YUME_FP8_FFN_FUSED", "0") == "1"
        # r18: the self-attention QKV projection and the cross-attention q projection in e4m3. An adaLN launch feeds each of them, so there is
        # no quantiser pass: adaln_modulate_e4m3 -> gemm_f8_splitt (q | k row-major, V as the K-major V^T image) and adaln_modulate_e4m3
        # (norm3) -> gemm_f8 (_qkv_step, _cross_q_step). o and cross-o stay bf16 (their input is the attention output). Independent of the two
        # FFN options. Off by default = the bf16 calls, bit for bit; env YUME_FP8_QKV=1 turns it on. Part of the pack key: flipping it re-packs.
        self.fp8_qkv = os.environ.get("YUME_FP8_QKV", "0") == "1"
        # r22: the self-attention of the single-sample forward (_blocks and its trimmed last block) on MX e4m3 operands: behind rmsnorm_rope one
        # quantiser pass over qk [L, 2C], one over the V^T image, then yume_attn_fwd_f8mx (_self_attn_step). Cross-attention, forward_cfg /
        # forward_pair, forward_batch, the sequence-parallel path, a head_dim other than 128, YUME_ATTN_PRESCALE=0 and the cross-check variants
        # keep the bf16 calls (said once on stderr under YUME_ATTN_LOG=1). Independent of the other FP8 options; no weight is repacked, so it
        # is not part of the pack key. Off by default = the bf16 calls, bit for bit; env YUME_FP8_ATTN=1 turns it on.
        self.fp8_attn = os.environ.get("YUME_FP8_ATTN", "0") == "1"
        self._fp8_attn_said = set()
        # r23: the FFN adaLN and both FFN linears of every block whose dim and ffn_dim are multiples of 128 in OCP MXFP6 e2m3, BOTH operands of
        # both GEMMs with one E8M0 scale byte per row and 32 k: adaln_modulate_mx_e2m3 -> gemm_f6_mxout (GELU, MX6 out) -> gemm_f6_mx (RESID);
        # no quantiser pass, no bf16 ff (_ffn_block). The weights are packed once at pack time (ops.mx6_pack), the bf16 weights stay. Wins over
        # fp8_ffn / fp8_ffn_fused where both are on. Off by default = today's path, bit for bit; env YUME_FP6_FFN=1 turns it on. Part of the
        # pack key: flipping it re-packs.
        self.fp6_ffn = os.environ.get("YUME_FP6_FFN", "0") == "1"
        self._fp6_ffn_said = False
        # r25: the projections of fp8_qkv in symmetric int8 instead, one fp32 scale per token row and per output channel (csrc/i8.hpp): seven
        # bits under the row's largest value where e4m3 carries three mantissa bits, at the same MFMA rate on the same bytes.
        # adaln_modulate_i8 -> gemm_i8_splitt and adaln_modulate_i8 (norm3) -> gemm_i8 (_qkv_step, _cross_q_step); the weights are quantised
        # once at pack time (ops.quant_rows_i8), the bf16 weights stay. Wins over fp8_qkv where both are on (said once under YUME_GEMM_LOG).
        # Independent of the FFN and attention options. Off by default = today's path, bit for bit; env YUME_INT8_QKV=1 turns it on. Part of
        # the pack key: flipping it re-packs.
        self.int8_qkv = os.environ.get("YUME_INT8_QKV", "0") == "1"
        self._int8_qkv_said = False
        # r26: the model's window_size (left, right) — flash-attn's sliding window on the token axis, -1 = unbounded on that side — for the
        # self-attention of the single-sample forward (_blocks, its trimmed last block, the block_forward seam and the sequence-parallel call):
        # token i sees the keys i - left ... i + right (yume_attn_fwd_band). Taken from model.window_size and settable: setting it is how a
        # checkpoint shipped with (-1, -1) is tried with a window. Cross-attention is never windowed, as in the reference. With a window
        # fp8_attn keeps the bf16 self-attention, and forward_pair / forward_batch refuse. (-1, -1) = today's calls, bit for bit.
        self.window_size = tuple(int(v) for v in getattr(model, "window_size", (-1, -1)))
        # r28: a FRAME-aligned window for the same self-attention calls: None, or (back, ahead) — a token sees every token of the frames within
        # `back` frames before and `ahead` frames after its own, -1 = unbounded on that side, (-1, 0) = frame-causal (yume_attn_fwd_fband). The
        # frames are those of the clip's own plan (framepack.frame_spans of the object the RoPE table was built from): on a FramePack sequence
        # one span per group, a coarse history frame being a few tokens and a new frame hundreds — what window_size, counting tokens, cannot
        # say. Not combined with a window_size; fp8_attn keeps bf16 under it; forward_pair / forward_batch refuse. None = today's calls, bit
        # for bit (no new code is reached); env YUME_FRAME_WINDOW="back,ahead" sets it.
        fw = os.environ.get("YUME_FRAME_WINDOW", "").strip()
        self.frame_window = tuple(int(v) for v in fw.split(",")) if fw else None
        self._spans = None            # the current clip's (rows, blocks) spans, kept by _prologue while frame_window is set
        # r29: the frame window's sink — the first frame_sink frames of the clip stay visible to every token whatever the window
        # (yume_attn_fwd_fsink). Under FramePack frame 0 is the clip's first frame (framepack.history_groups puts it first): the conditioning
        # image of the I2V models, which a local window hides from every frame more than `back` frames on. Needs a frame_window; counts above
        # the clip's frames mean all of them. It reaches the kernel through _frame_args alone. 0 = r28's calls, bit for bit; env
        # YUME_FRAME_SINK sets it.
        self.frame_sink = int(os.environ.get("YUME_FRAME_SINK", "0").strip() or 0)
        # r30: under the frame-causal mask (frame_window = (-1, 0)) no history token of a FramePack sequence sees a token of the frames being
        # denoised; the 5B family gives the history rows the timestep t[0] and keeps their latents clean, and cross-attention and the FFN are
        # row-local: every history row of the residual stream, hence its K row and V^T column in every block, is the same at every denoise
        # step of a chunk. With cache_history the first qualifying forward_one after reset_history() (or after a change of the cache key:
        # clip shape, conditioning, pack, dedup_pad_keys) is a RECORD forward — today's forward, bit for bit, that also copies each block's
        # history K rows / V^T columns into engine-owned buffers — and every later one a REPLAY: the new frames' rows only, their
        # self-attention over the cached keys as an always-visible prefix (yume_attn_fwd_fprefix). The caller promises that the history
        # frames of u and t[0] are the recorded ones (sampling.make_velocity_5b's loop does; history_check compares them, with a sync).
        # Needs family wan23, the packed path, frame_window == (-1, 0), no window_size, no sequence parallelism, no block-residual cache.
        # Off by default = today's path, bit for bit; env YUME_CACHE_HISTORY=1 turns it on.
        self.cache_history = os.environ.get("YUME_CACHE_HISTORY", "0") == "1"
        self.history_check = os.environ.get("YUME_HISTORY_CHECK", "0") == "1"
        self._hist_key = None         # the cache key of the recorded history; None: the next qualifying forward records
        self._hist_refs = None        # the conditioning tensors of the key (their addresses stay theirs while the entry is live)
        self._hist_rec = None         # n_hist while a record forward is under way: _blocks / _trimmed_block copy K / V^T behind rmsnorm_rope
        self._hist_kept = None        # history_check: (the history frames of u, t[0]) at record time
        self._hist_said = False
        # r27: a captured hipGraph holds raw pointers to what the engine handed it — the _buf workspaces, the per-clip tables, the packed
        # weights — and knows nothing of _ws, _plan_cache or P. What a capture was handed is kept here (workspaces once per storage), so a later
        # eager call at another shape, a flipped pack option or the emptying plan cache replaces the engine's entry but frees nothing a replay
        # reads or writes. Held until release_captured(); empty, and never looked at, while nothing is captured.
        self._captured = []
        self._captured_ids = set()

    # ------------------------------------------------------------------ profiling (bench.py)
    def _timed(self, name, fn, *a, **k):
        """run one kernel call; with self.prof set, bracket it with HIP events recorded on the launch stream (torch's current
        stream IS the stream ops.* enqueue on)."""
        if self.prof is None or (self.prof_only is not None and name not in self.prof_only):
            return fn(*a, **k)
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        r = fn(*a, **k)
        ev[1].record()
        self.prof.setdefault(name, []).append(ev)
        return r

    # ------------------------------------------------------------------ weights
    def _param_key(self):
        # walked once per forward: (storage address, in-place version, dtype) of every parameter — a load_state_dict, an
        # optimizer step or a .to(dtype) re-packs; cheap next to one forward (≈1 k tensors), and cached per forward call
        return (self.q_prescale, bool(self.fp8_ffn), bool(self.fp8_qkv), bool(self.fp6_ffn), bool(self.int8_qkv)) + tuple((p.data_ptr(), p._version, p.dtype) for p in self.model.parameters())

    def _pack(self):
        m = self.model
        dev = m.patch_embedding.weight.device
        if dev.type != "cuda":
            raise RuntimeError("yume_amd WanModel must live on the GPU ('cuda') — there is no CPU path")
        C = m.dim

        def bf(w):
            return w.detach().to(torch.bfloat16).contiguous()

        def f32(w):
            return w.detach().to(torch.float32).contiguous()

        def padk(w2d):
            K = w2d.shape[1]
            Kp = _round_up(K, 64)
            if Kp != K:
                w2d = torch.cat([w2d, w2d.new_zeros(w2d.shape[0], Kp - K)], dim=1)
            return w2d.contiguous()

        P = {}
        # patch embeddings (levels 0..4 + the 2x_f pre-conv); only those attached to the module are packed
        P["pe"] = {}
        for lvl, suf in enumerate(framepack.LEVEL_SUFFIX):
            conv = getattr(m, "patch_embedding" + suf, None)
            if conv is not None:
                P["pe"][lvl] = (padk(bf(conv.weight.flatten(1))), f32(conv.bias))
        conv = getattr(m, "patch_embedding_2x_f", None)
        if conv is not None:
            P["pe"]["2x_f"] = (padk(bf(conv.weight.flatten(1))), f32(conv.bias))
        te, tm, tp = m.text_embedding, m.time_embedding, m.time_projection
        P["text"] = (bf(te[0].weight), f32(te[0].bias), bf(te[2].weight), f32(te[2].bias))
        # fp32 islands keep the parameter's own precision (bf16 if the model was cast, else fp32)
        keep = lambda w: w.detach().contiguous() if w.dtype in (torch.float32, torch.bfloat16) else f32(w)
        P["time"] = (keep(tm[0].weight), f32(tm[0].bias), keep(tm[2].weight), f32(tm[2].bias),
                     keep(tp[1].weight), f32(tp[1].bias))
        if self.family == "wan":
            pr = m.img_emb.proj
            P["img"] = (f32(pr[0].weight), f32(pr[0].bias), bf(pr[1].weight), f32(pr[1].bias), bf(pr[3].weight),
                        f32(pr[3].bias), f32(pr[4].weight), f32(pr[4].bias))
        blocks = []
        qs = math.log2(math.e) / math.sqrt(C // m.num_heads) if self.q_prescale else 1.0
        # qk_norm=False (reference model.py:175-176): norm_q / norm_k are nn.Identity — the RoPE / scale kernel runs with its normalisation off
        # (eps < 0, include/yume_hip.h) and a weight of ones (times the attention scale on the q side)
        self.qk_eps = m.eps if getattr(m.blocks[0], "qk_norm", True) else -1.0

        def nw(mod):
            w = getattr(mod, "weight", None)
            return (w if w is not None else torch.ones(C, device=dev)).double()

        for b in m.blocks:
            sa, ca = b.self_attn, b.cross_attn
            d = {
                "wqkv": bf(torch.cat([sa.q.weight, sa.k.weight, sa.v.weight], dim=0)),
                "bqkv": f32(torch.cat([sa.q.bias, sa.k.bias, sa.v.bias])),
                "nqk": f32(torch.cat([nw(sa.norm_q) * qs, nw(sa.norm_k)])),
                "wo": bf(sa.o.weight), "bo": f32(sa.o.bias),
                "wq_c": bf(ca.q.weight), "bq_c": f32(ca.q.bias), "nq_c": f32(nw(ca.norm_q) * qs),   # (cross q carries the scale too)
                "wo_c": bf(ca.o.weight), "bo_c": f32(ca.o.bias),
                "w1": bf(b.ffn[0].weight), "b1": f32(b.ffn[0].bias),
                "w2": bf(b.ffn[2].weight), "b2": f32(b.ffn[2].bias),
            }
            if getattr(b.norm3, "weight", None) is not None:
                d["n3w"], d["n3b"] = f32(b.norm3.weight), f32(b.norm3.bias)
            if self.fp8_ffn:
                if C % 128 == 0 and m.ffn_dim % 128 == 0:
                    for wk, qk_, sk_ in (("w1", "w1q", "s1"), ("w2", "w2q", "s2")):
                        d[qk_] = torch.empty(d[wk].shape, dtype=torch.uint8, device=dev)
                        d[sk_] = torch.empty(d[wk].shape[0], dtype=torch.float32, device=dev)
                        ops.quant_rows_e4m3(d[wk], d[qk_], d[sk_])
                elif os.environ.get("YUME_GEMM_LOG", "0") not in ("", "0"):
                    sys.stderr.write(f"[fp8_ffn] block {len(blocks)} keeps bf16 FFN linears: dim={C} ffn_dim={m.ffn_dim} are not both multiples of 128\n")
            if self.fp6_ffn:
                if C % 128 == 0 and m.ffn_dim % 128 == 0:
                    d["w1p"], d["e1"] = ops.mx6_pack(d["w1"])
                    d["w2p"], d["e2"] = ops.mx6_pack(d["w2"])
                elif os.environ.get("YUME_GEMM_LOG", "0") not in ("", "0"):
                    sys.stderr.write(f"[fp6_ffn] block {len(blocks)} keeps its FFN linears: dim={C} ffn_dim={m.ffn_dim} are not both multiples of 128\n")
            if self.fp8_qkv:
                log = os.environ.get("YUME_GEMM_LOG", "0") not in ("", "0")
                if C % 128 == 0:       # (K % 128 == 0 and n_split = 2 C a multiple of 256: every DiT the attention kernels take, head_dim 128)
                    for wk, qk_, sk_ in (("wqkv", "wqkvq", "sqkv"),) + ((("wq_c", "wq_cq", "sq_c"),) if "n3w" in d else ()):
                        d[qk_] = torch.empty(d[wk].shape, dtype=torch.uint8, device=dev)
                        d[sk_] = torch.empty(d[wk].shape[0], dtype=torch.float32, device=dev)
                        ops.quant_rows_e4m3(d[wk], d[qk_], d[sk_])
                    if "n3w" not in d and log and not blocks:
                        sys.stderr.write("[fp8_qkv] the blocks have no norm3 weights: the cross-attention q projection stays bf16\n")
                elif log and not blocks:
                    sys.stderr.write(f"[fp8_qkv] the blocks keep bf16 QKV / cross-q linears: dim={C} is not a multiple of 128\n")
            if self.int8_qkv:
                log = os.environ.get("YUME_GEMM_LOG", "0") not in ("", "0")
                if C % 128 == 0:       # (the condition of fp8_qkv: K % 128 == 0 and n_split = 2 C a multiple of 256)
                    for wk, qk_, sk_ in (("wqkv", "wqkvi", "sqkvi"),) + ((("wq_c", "wq_ci", "sq_ci"),) if "n3w" in d else ()):
                        d[qk_] = torch.empty(d[wk].shape, dtype=torch.int8, device=dev)
                        d[sk_] = torch.empty(d[wk].shape[0], dtype=torch.float32, device=dev)
                        ops.quant_rows_i8(d[wk], d[qk_], d[sk_])
                    if "n3w" not in d and log and not blocks:
                        sys.stderr.write("[int8_qkv] the blocks have no norm3 weights: the cross-attention q projection stays bf16\n")
                elif log and not blocks:
                    sys.stderr.write(f"[int8_qkv] the blocks keep bf16 QKV / cross-q linears: dim={C} is not a multiple of 128\n")
            blocks.append(d)
        P["blocks"] = blocks
        # cross-attention K / V projections of ALL blocks as one weight: the conditioning tokens are the same for every block,
        # so one [n_ctx, C] x [2*nb*C, C]^T GEMM (K rows of all blocks first, then V rows) replaces nb launches whose 128-wide
        # tiles each took a full K loop's latency; same products, same rounding. +2*nb*C*C bf16 of HBM (5B: 1.1 GB).
        cas = [b.cross_attn for b in m.blocks]
        P["wkv_c"] = bf(torch.cat([ca.k.weight for ca in cas] + [ca.v.weight for ca in cas], dim=0))
        P["bkv_c"] = f32(torch.cat([ca.k.bias for ca in cas] + [ca.v.bias for ca in cas]))
        P["nk_c"] = f32(torch.stack([nw(ca.norm_k) for ca in cas]))
        if self.family == "wan":
            P["wkv_i"] = bf(torch.cat([ca.k_img.weight for ca in cas] + [ca.v_img.weight for ca in cas], dim=0))
            P["bkv_i"] = f32(torch.cat([ca.k_img.bias for ca in cas] + [ca.v_img.bias for ca in cas]))
            P["nk_i"] = f32(torch.stack([nw(ca.norm_k_img) for ca in cas]))
        P["mod_all"] = f32(torch.cat([b.modulation.reshape(1, 6 * C) for b in m.blocks], dim=0))
        P["mod_head"] = f32(m.head.modulation.reshape(2, C))
        wh = m.head.head.weight.detach().float()
        hi = wh.to(torch.bfloat16)
        lo = (wh - hi.float()).to(torch.bfloat16)
        P["whead"] = torch.cat([hi, lo, hi], dim=1).contiguous()   # pairs with A' = [hi | hi | lo]
        P["bhead"] = f32(m.head.head.bias)
        self.P = P
        self.dev = dev

    def ensure_packed(self):
        key = self._param_key()
        if key != self._packed_key:
            if self._captured and getattr(self, "P", None) is not None:
                self._captured.append(self.P)      # (r27) a live graph may replay on the outgoing weights
            self._pack()
            self._packed_key = key

    # ------------------------------------------------------------------ what a graph capture was handed (r27)
    def _pin(self, obj, ident):
        if ident not in self._captured_ids:
            self._captured_ids.add(ident)
            self._captured.append(obj)

    def release_captured(self):
        """forget what stream captures were handed (workspaces, per-clip tables, replaced packed weights). Call it after deleting every
        graph captured from this engine: a graph replayed afterwards may run on memory the engine has given back."""
        self._captured.clear()
        self._captured_ids.clear()

    # ------------------------------------------------------------------ workspaces / per-clip tables
    def _buf(self, name, shape, dtype, zero=False, grow_rows=False):
        """a workspace tensor, kept across calls while its shape holds. zero: zero-filled when (re)allocated — for buffers whose padding
        (rows / columns no kernel writes) has to stay finite. grow_rows: a kept tensor with at least shape[0] rows (and the same other
        dims) serves as its first shape[0] rows — for callers whose row count alternates (the trimmed last block beside the full ones)."""
        t = self._ws.get(name)
        grown = grow_rows and t is not None and t.shape[0] >= shape[0] and tuple(t.shape[1:]) == tuple(shape[1:]) and t.dtype == dtype and t.device == self.dev
        if not grown and (t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != self.dev):
            t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.dev)
            self._ws[name] = t
        if torch.cuda.is_current_stream_capturing():
            self._pin(t, ("ws", t.untyped_storage().data_ptr()))     # (the base tensor, not the row view)
        return t[:shape[0]] if grown else t

    def _clip_tables(self, key, build):
        v = self._plan_cache.get(key)
        if v is None:
            if len(self._plan_cache) > 64:
                self._plan_cache.clear()
            v = build()
            self._plan_cache[key] = v
        if torch.cuda.is_current_stream_capturing():
            self._pin(v, ("plan", id(v)))         # (the cache empties itself past 64 clips; a graph still reads the RoPE / selector tables)
        return v

    # ------------------------------------------------------------------ pieces
    def _embed_group(self, u, g, xs_rows):
        """patch-embed frames [g.f0, g.f0+g.nf) of u [Cin,F,H,W] at level g.level into xs_rows (fp32 [ntok, C])."""
        P = self.P["pe"]
        if g.level == 5:
            w, b = P["2x_f"]
            Cin = u.shape[0]
            h4, w4 = -(-u.shape[2] // 4), -(-u.shape[3] // 4)
            a = self._buf("pe_a5", (g.nf * h4 * w4, w.shape[1]), torch.bfloat16)
            ops.patch_gather(u, g.f0, g.nf, 4, 4, a)
            mid = self._buf("pe_mid", (g.nf * h4 * w4, Cin), torch.float32)
            ops.gemm_bf16(a, w, b, mid, EPI_F32, variant=self.gemm_variant)
            # layout change only: token-major [f,h,w,c] -> [c,f,h,w] for the second gather
            u = mid.view(g.nf, h4, w4, Cin).permute(3, 0, 1, 2).contiguous()
            f0, lvl = 0, 4
        else:
            f0, lvl = g.f0, g.level
        if lvl not in P:
            raise RuntimeError(f"patch_embedding{framepack.LEVEL_SUFFIX[lvl]} is needed for this history length "
                               "but is not attached to the model")
        w, b = P[lvl]
        k = 2 << lvl
        a = self._buf(f"pe_a{lvl}_{g.ntok}", (g.ntok, w.shape[1]), torch.bfloat16)
        ops.patch_gather(u, f0, g.nf, k, k, a)
        ops.gemm_bf16(a, w, b, xs_rows, EPI_F32, variant=self.gemm_variant)

    def _time_rows(self, t64, t_index, R):
        """e [R, C], e0 [R, 6C] for the R distinct timesteps (fp32 islands of the reference)."""
        C = self.model.dim
        w0, b0, w2, b2, wp, bp = self.P["time"]
        e = self._buf("t_e", (R, C), torch.float32)
        e0 = self._buf("t_e0", (R, 6 * C), torch.float32)
        for r0 in range(0, R, 8):
            r1 = min(R, r0 + 8)
            n = r1 - r0
            s = self._buf("t_sin", (8, self.model.freq_dim), torch.float32)[:n]
            h = self._buf("t_h", (8, C), torch.float32)[:n]
            idx = t_index[r0:r1] if t_index is not None else None
            tt = t64 if t_index is not None else t64[r0:r1]
            ops.sinusoidal_embed(tt, idx, n, self.model.freq_dim, s)
            ops.linear_smallm_f32(s, w0, b0, h, in_act=0, out_act=1)          # Linear -> SiLU
            ops.linear_smallm_f32(h, w2, b2, e[r0:r1])                        # Linear
            ops.linear_smallm_f32(e[r0:r1], wp, bp, e0[r0:r1], in_act=1)      # SiLU -> Linear
        return e, e0

    def _text_ctx(self, context, out_rows):
        """text_embedding of the prompt padded with zero rows to out_rows' row count: text_len, or n + 1 with dedup_pad_keys (one zero row
        stands for all the pad rows; its weight goes to the attention calls)."""
        m = self.model
        w0, b0, w2, b2 = self.P["text"]
        n = context.shape[0]
        if n > m.text_len:
            raise RuntimeError(f"context has {n} tokens > text_len {m.text_len}")
        rows = out_rows.shape[0]
        sfx = "" if rows == m.text_len else f"_{rows}"
        cpad = self._buf("ctx_in" + sfx, (rows, m.text_dim), torch.bfloat16)
        if n:
            ops.cast_bf16(context.to(device=self.dev, dtype=torch.float32).contiguous(), n, cpad)
        else:
            cpad.zero_()                       # empty prompt: the reference pads [0, text_dim] to text_len zero rows (model.py:816-821)
        hid = self._buf("ctx_hid" + sfx, (rows, m.dim), torch.bfloat16)
        ops.gemm_bf16(cpad, w0, b0, hid, EPI_BF16_GELU, variant=self.gemm_variant)
        ops.gemm_bf16(hid, w2, b2, out_rows, EPI_BF16, variant=self.gemm_variant)

    def _img_ctx(self, clip_fea, out_rows):
        C = self.model.dim
        lw, lb, w1, b1, w3, b3, l4w, l4b = self.P["img"]
        x = clip_fea.to(device=self.dev, dtype=torch.float32).reshape(-1, clip_fea.shape[-1]).contiguous()
        n, d = x.shape
        a = self._buf("img_a", (n, d), torch.bfloat16)
        ops.adaln_modulate(x, lw, lb, 0, None, False, a, 0, eps=1e-5)         # nn.LayerNorm default eps
        h = self._buf("img_h", (n, d), torch.bfloat16)
        ops.gemm_bf16(a, w1, b1, h, EPI_BF16_GELU_ERF, variant=self.gemm_variant)
        y = self._buf("img_y", (n, C), torch.float32)
        ops.gemm_bf16(h, w3, b3, y, EPI_F32, variant=self.gemm_variant)
        ops.adaln_modulate(y, l4w, l4b, 0, None, False, out_rows, 0, eps=1e-5)

    def _cross_kv(self, tag, ctx_rows, nk, wkv, bkv, nk_w, fresh, cols=None):
        """K (RMS-normalised) and K-major V^T of all blocks for one conditioning stream: kc [nk, nb*C], vct [nb*C, nk8].
        Recomputed only when `fresh` (always, unless cache_context found the same conditioning tensors).
        cols: columns of vct where the caller needs more than nk's own whole tiles (forward_pair: both legs' V^T with one row stride)."""
        C, nb = self.model.dim, len(self.P["blocks"])
        # rows / columns up to a whole number of 64-key tiles exist and hold zeros: the attention kernels may fetch the ragged last key tile
        # like any other (YUME_ATTN_KV_PADDED); the GEMM below writes nk rows / columns only
        nk64 = _round_up(nk, 64)
        kc = self._buf(f"kc_{tag}_{nk}", (nk64, nb * C), torch.bfloat16, zero=True)[:nk]
        vct = self._buf(f"vct_{tag}_{nk}", (nb * C, nk64 if cols is None else cols), torch.bfloat16, zero=True)
        if fresh:
            ops.gemm_bf16(ctx_rows, wkv, bkv, kc, EPI_BF16_SPLITT, out_t=vct, n_split=nb * C, variant=self.gemm_variant)
            ops.rmsnorm_rows_periodic(kc.view(nk * nb, C), C, nk_w, self.qk_eps)
        return kc, vct

    def _blocks(self, xs, L, tab, row_idx, R, rope, n_rope, ctx, n_img, ctx_fresh=True, n_keys=None, only=None, cache=None, n_trim=0,
                txt_last_weight=1.0, hist=0):
        """xs fp32 [L, C] in/out. tab fp32 [nb, R, 6, C]; rope fp32 [n_rope, 64, 2] (n_rope == L here).
        txt_last_weight: how many keys the LAST text row of ctx stands for (dedup_pad_keys: text_len - n; 1 = every row is one key).
        n_trim: the first n_trim rows of the LAST block's output are not needed by the caller (history tokens in front of the head): that
        block computes K / V for every row but everything behind the QKV projection for the rows [n_trim, L) only; xs[:n_trim] is then stale.
        With sequence parallelism L is this rank's (padded) chunk and n_keys the true global token count.
        only: run just these block indices (tab[j] then belongs to only[j]) — the WanAttentionBlock.forward seam.
        cache: (mode, cache_list, tensors) block-residual cache of wan/modules/model.py:985-1000: mode 'record' appends
        bf16 (x_out - x_in) of the listed blocks, 'replay' adds the stored residual instead of running them.
        hist = n_hist > 0: a cache_history REPLAY. xs, row_idx and rope are the L = n_new_tok rows of the frames being denoised alone (row 0
        of every buffer is the first new token), in workspaces of the replay's own (`*_hr`: a longer eager forward never leaves its rows in
        their padding), and the self-attention runs over the recorded history keys as a prefix (_self_attn_history)."""
        m = self.model
        C, H, Fd, eps = m.dim, m.num_heads, m.ffn_dim, m.eps
        # q|k rows and V^T columns exist (zeros) up to a whole number of 64-key tiles: YUME_ATTN_KV_PADDED (see _cross_kv)
        Lp = _round_up(L, 64)
        sfx = "_hr" if hist else ""
        h = self._buf("h" + sfx, (L, C), torch.bfloat16)
        qk = self._buf("qk" + sfx, (Lp, 2 * C), torch.bfloat16, zero=True)[:L]
        vt = self._buf("vt" + sfx, (C, Lp), torch.bfloat16, zero=True)
        att = self._buf("att" + sfx, (L, C), torch.bfloat16)
        ff = self._buf("ff" + sfx, (L, Fd), torch.bfloat16)
        ts = 6 * C  # table row stride
        ntxt = ctx.shape[0] - n_img
        kc_t, vct_t = self._cross_kv("t", ctx[n_img:], ntxt, self.P["wkv_c"], self.P["bkv_c"], self.P["nk_c"], ctx_fresh)
        if n_img:
            kc_i, vct_i = self._cross_kv("i", ctx[:n_img], n_img, self.P["wkv_i"], self.P["bkv_i"], self.P["nk_i"], ctx_fresh)
        T = self._timed
        # (the register-staged kernel of the cross-check mode takes no key weight: variant 2 then)
        txt_variant = 2 if (txt_last_weight != 1.0 and self.attn_variant == 1) else self.attn_variant
        ids = range(len(self.P["blocks"])) if only is None else only
        for j, i in enumerate(ids):
            d = self.P["blocks"][i]
            if cache is not None and i in cache[1]:
                if cache[0] == "replay":
                    # reference: `x = x + cache[cache_list.index(cnt_blocks - 1)]` (fp32 + bf16), the block is not run
                    xs.add_(cache[2][cache[1].index(i)].reshape(L, C).to(torch.float32))
                    continue
                x_in = xs.clone()
            tb = tab[j if only is not None else i]                      # [R, 6, C]
            shift_sa, scale_sa, gate_sa = tb[:, 0], tb[:, 1], tb[:, 2]
            shift_ff, scale_ff, gate_ff = tb[:, 3], tb[:, 4], tb[:, 5]
            s = n_trim if j == len(ids) - 1 else 0                      # rows [s, L) are the ones whose output is wanted
            if s:
                self._trimmed_block(xs, L, s, d, i, tb, ts, row_idx, rope, eps, h, qk, vt, att, ff, kc_t, vct_t, ntxt,
                                    (kc_i, vct_i, n_img) if n_img else None, txt_last_weight, txt_variant)
                continue
            # --- self attention
            self._qkv_step(d, xs, scale_sa, shift_sa, ts, row_idx, h, qk, vt, eps)
            if n_rope == L:
                T("rmsnorm_rope", ops.rmsnorm_rope, qk, C, 2, d["nqk"], self.qk_eps, rope)
            elif n_rope == 0:
                ops.rmsnorm_rope(qk, C, 2, d["nqk"], self.qk_eps, None)
            else:
                ops.rmsnorm_rope(qk[:n_rope], C, 2, d["nqk"], self.qk_eps, rope)
                ops.rmsnorm_rope(qk[n_rope:], C, 2, d["nqk"], self.qk_eps, None)
            if self._hist_rec:
                self._hist_record(i, qk, vt)
            if hist:
                sa = self._self_attn_history(i, qk, vt, att, L, hist)
            elif self.sp is None:
                sa = self._self_attn_step(qk, vt, att, 0, L, n_keys if n_keys is not None else L)
            else:      # Ulysses: all tokens x this rank's heads, then back (2 collectives, yume_amd/ulysses.py)
                self._fp8_attn_notice("the sequence-parallel self-attention keeps the bf16 kernels")
                qf, kf, vtf = self.sp.exchange_qkv(qk, vt, C)
                of = self._buf("att_sp", (qf.shape[0], qf.shape[1]), torch.bfloat16)
                # (after the all-to-all this rank holds ALL tokens of its heads: row 0 is token 0)
                ops.attn_fwd(qf, kf, vtf, of, qf.shape[0], n_keys, H // self.sp.world, variant=self.attn_variant, q_prescaled=self.q_prescale,
                             **self._window_args(0), **self._frame_args(0, qf.shape[0]))
                sa = self.sp.exchange_out(of)
            T("gemm_o", ops.gemm_bf16, sa, d["wo"], d["bo"], xs, EPI_RESID, gate=gate_sa, gate_stride=ts, row_idx=row_idx, variant=self.gemm_variant)
            # --- cross attention
            self._cross_q_step(d, xs, h, qk[:, :C], eps)
            T("rmsnorm_rope", ops.rmsnorm_rope, qk[:, :C], C, 1, d["nq_c"], self.qk_eps)
            T("attn_cross", ops.attn_fwd, qk[:, :C], kc_t[:, i * C:(i + 1) * C], vct_t[i * C:(i + 1) * C], att, L, ntxt, H, variant=txt_variant,
              q_prescaled=self.q_prescale, kv_padded=True, last_key_weight=txt_last_weight)
            if n_img:
                T("attn_cross", ops.attn_fwd, qk[:, :C], kc_i[:, i * C:(i + 1) * C], vct_i[i * C:(i + 1) * C], att, L, n_img, H, accumulate=True,
                  variant=self.attn_variant, q_prescaled=self.q_prescale, kv_padded=True)
            T("gemm_cross_o", ops.gemm_bf16, att, d["wo_c"], d["bo_c"], xs, EPI_RESID, variant=self.gemm_variant)
            # --- FFN
            self._ffn_block(d, xs, h, ff, scale_ff, shift_ff, gate_ff, ts, row_idx, eps)
            if cache is not None and cache[0] == "record" and i in cache[1]:
                cache[2].append((xs - x_in).to(torch.bfloat16).unsqueeze(0))     # reference keeps [B, L, C] bf16

    def _fp8_attn_notice(self, why):
        """one stderr line per reason and engine (YUME_ATTN_LOG=1), in the style of the [fp8_qkv] notices"""
        if self.fp8_attn and why not in self._fp8_attn_said:
            self._fp8_attn_said.add(why)
            if os.environ.get("YUME_ATTN_LOG", "0") not in ("", "0"):
                sys.stderr.write(f"[fp8_attn] {why}\n")

    def _windowed(self):
        return tuple(self.window_size) != (-1, -1)

    def _window_args(self, q_pos0):
        """the window arguments of a self-attention ops.attn_fwd call whose first query row is token q_pos0; none without a window: the call
        is then the one it always was"""
        if not self._windowed():
            return {}
        left, right = (int(v) for v in self.window_size)
        if left < -1 or right < -1:
            raise ValueError(f"DiTEngine.window_size={self.window_size}: -1 (unbounded) or a non-negative width per side")
        return {"window": (left, right), "q_pos0": int(q_pos0)}

    def _frame_args(self, q_pos0, n_rows=None):
        """the frame-window arguments of a self-attention ops.attn_fwd call whose first query row is token q_pos0; none without a
        frame_window. n_rows: the call's query rows where they outnumber the clip's tokens (the sequence-parallel pad rows): the rows behind
        the last token are one more block, seen by nobody (they lie behind Lk). With a frame_sink, min(frame_sink, the clip's frames) of it."""
        sink = int(self.frame_sink)
        if sink != 0 and (sink < 0 or self.frame_window is None):
            raise ValueError(f"DiTEngine.frame_sink={self.frame_sink} with frame_window={self.frame_window}: the sink is a non-negative count of "
                             "leading frames beside a frame_window (set engine.frame_window, or engine.frame_sink = 0)")
        if self.frame_window is None:
            return {}
        if self._windowed():
            raise ValueError(f"DiTEngine.frame_window={tuple(self.frame_window)} and window_size={tuple(self.window_size)} do not combine: "
                             "one mask per self-attention (set one of them back to None / (-1, -1))")
        fw = tuple(int(v) for v in self.frame_window)
        if len(fw) != 2 or fw[0] < -1 or fw[1] < -1:
            raise ValueError(f"DiTEngine.frame_window={self.frame_window}: None, or (back, ahead) with -1 (unbounded) or a non-negative frame "
                             "count per side")
        if self._spans is None:
            raise NotImplementedError(f"frame_window={fw} needs the clip's frame partition, which block_forward's bare rows do not carry (run "
                                      "the model's forward, or set engine.frame_window = None)")
        spans = list(self._spans)
        n_tok = sum(r * b for r, b in spans)
        extra = {"frame_sink": min(sink, sum(b for _, b in spans))} if sink else {}
        if n_rows is not None and n_rows > n_tok:
            spans.append((n_rows - n_tok, 1))
        return {"frame_window": fw, "spans": spans, "q_pos0": int(q_pos0), **extra}

    def _refuse_frame_window(self, who):
        if self.frame_window is not None:
            raise NotImplementedError(f"{who} does not implement frame_window={tuple(self.frame_window)}: its self-attention kernels are dense "
                                      "(set engine.frame_window = None, or call the single-sample forward per leg / sample)")

    def _refuse_window(self, who):
        if self._windowed():
            raise NotImplementedError(f"{who} does not implement window_size={tuple(self.window_size)}: its self-attention kernels are dense "
                                      "(set engine.window_size = (-1, -1), or call the single-sample forward per leg / sample)")

    def _self_attn_step(self, qk, vt, out, s, L, n_keys):
        """the self-attention of one block of the single-sample forward behind rmsnorm_rope: the queries are the rows [s, L) of qk[:, :C], the
        keys the first n_keys rows of qk[:, C:] and columns of vt; out [L - s, C]. With fp8_attn: quant_rows_mx(qk) + attn_vt_mx(vt) ->
        attn_fwd_f8mx on engine-owned byte buffers (allocated by the first eager forward); otherwise today's bf16 call. With a window_size
        the bf16 call carries it with q_pos0 = s (row s of the call is token s), and fp8_attn keeps bf16; a frame_window likewise."""
        m = self.model
        C, H = m.dim, m.num_heads
        T = self._timed
        if self.fp8_attn:
            if self._windowed():
                self._fp8_attn_notice(f"self-attention stays bf16: window_size={tuple(self.window_size)} runs the bf16 band kernel")
            elif self.frame_window is not None:
                self._fp8_attn_notice(f"self-attention stays bf16: frame_window={tuple(self.frame_window)} runs the bf16 frame-band kernel")
            elif C != 128 * H:
                self._fp8_attn_notice(f"self-attention stays bf16: head_dim={C // H} is not 128")
            elif not self.q_prescale or self.attn_variant != 0:
                self._fp8_attn_notice("self-attention stays bf16: the e4m3 kernel takes pre-scaled q and the automatic variant only")
            else:
                self._fp8_attn_notice("cross-attention keeps the bf16 kernels")
                nt = (n_keys + 127) // 128
                qk8 = self._buf("qk8", (L, 2 * C), torch.uint8)
                qke = self._buf("qke", (L, 8 * H), torch.uint8)
                vt8 = self._buf("vt8", (C, 128 * nt), torch.uint8)
                ev = self._buf("vt8e", (nt, 4 * C), torch.uint8)
                T("quant_mx", ops.quant_rows_mx_e4m3, qk[:L], qk8, qke)
                T("quant_mx", ops.attn_vt_mx_e4m3, vt, n_keys, vt8, ev)
                T("attn_self", ops.attn_fwd_f8mx, qk8[s:, :C], qke[s:, :4 * H], qk8[:, C:], qke[:, 4 * H:], vt8, ev, out, L - s, n_keys, H)
                return out
        T("attn_self", ops.attn_fwd, qk[s:, :C], qk[:, C:], vt, out, L - s, n_keys, H, variant=self.attn_variant, q_prescaled=self.q_prescale,
          kv_padded=True, **self._window_args(s), **self._frame_args(s))
        return out

    # ------------------------------------------------------------------ the frame-causal history cache (r30)
    def reset_history(self):
        """forget the recorded history: the next qualifying forward_one records again (sampling.make_velocity_5b calls it once per chunk)"""
        self._hist_key = self._hist_refs = self._hist_kept = None

    def _hist_bufs(self, i, n_hist):
        """block i's cache: Kc [n_hist, C] and Vc [C, ceil8(n_hist)] (engine-owned workspaces: a capture that is handed them pins them)"""
        C = self.model.dim
        return (self._buf(f"hist_k{i}", (n_hist, C), torch.bfloat16),
                self._buf(f"hist_vt{i}", (C, _round_up(n_hist, 8)), torch.bfloat16, zero=True))

    def _hist_record(self, i, qk, vt):
        """behind block i's rmsnorm_rope of a record forward: the history tokens' K rows and V^T columns, as every later step will need them"""
        n, C = self._hist_rec, self.model.dim
        kc, vc = self._hist_bufs(i, n)
        kc.copy_(qk[:n, C:])
        vc[:, :n].copy_(vt[:, :n])

    def _self_attn_history(self, i, qk, vt, out, L, n_hist):
        """the self-attention of block i of a replay: the L new rows over the n_hist recorded keys (seen by every row) and their own keys
        under the frame-causal rule on the new group's span — yume_attn_fwd_fprefix. fp8_attn keeps this bf16 kernel."""
        C, H = self.model.dim, self.model.num_heads
        self._fp8_attn_notice("self-attention stays bf16: a cache_history replay runs the bf16 frame-prefix kernel")
        kc, vc = self._hist_bufs(i, n_hist)
        self._timed("attn_self", ops.attn_fwd, qk[:, :C], qk[:, C:], vt, out, L, L, H, variant=self.attn_variant, q_prescaled=self.q_prescale,
                    frame_window=(-1, 0), spans=[self._spans[-1]], q_pos0=0, prefix=(kc, vc, n_hist))
        return out

    def _history_mode(self, u, t, context, clip_fea, packed, lfz, n_sel, cache):
        """None with cache_history off; otherwise the preconditions (each refusal names the option and what it met), then ("record" | "replay",
        the cache key)"""
        if not self.cache_history:
            return None
        who = "DiTEngine.cache_history"
        if self.family != "wan23":
            raise NotImplementedError(f"{who} needs the wan23 (5B) family: the {self.family!r} family has one scalar t and re-noises its history "
                                      "every step, so its history rows are not step-invariant (set engine.cache_history = False)")
        if not packed or t.numel() < 2:
            raise ValueError(f"{who} needs the packed (FramePack) path with a per-token t (t[0] history, t[-1] new), got packed={packed} and "
                             f"{t.numel()} timestep(s)")
        fw = None if self.frame_window is None else tuple(int(v) for v in self.frame_window)
        if fw != (-1, 0):
            raise ValueError(f"{who} needs frame_window == (-1, 0) (frame-causal: no history token sees a new frame), got frame_window={fw}")
        if self._windowed():
            raise ValueError(f"{who} and window_size={tuple(self.window_size)} do not combine (needs window_size == (-1, -1))")
        if self.sp is not None:
            raise NotImplementedError(f"{who} is not combined with sequence parallelism (engine.sp must be None)")
        if cache is not None:
            raise NotImplementedError(f"{who} is not combined with the block-residual cache (forward_one's cache argument must be None)")
        Cin, F, H, W = u.shape
        key = (("p", F, H, W, lfz, n_sel),
               (context.data_ptr(), context._version, tuple(context.shape),
                None if clip_fea is None else (clip_fea.data_ptr(), clip_fea._version, tuple(clip_fea.shape)), self._packed_key,
                self.dedup_pad_keys), self._packed_key, self.dedup_pad_keys)
        if key == self._hist_key and not (self.history_check and self._hist_kept is None):      # (a check switched on later: record again)
            if self.history_check:
                hu, ht = self._hist_kept
                if not torch.equal(u[:, :F - lfz].to(hu.device, hu.dtype), hu):
                    raise RuntimeError(f"{who}: the history frames of u differ from the recorded ones (history_check; call "
                                       "engine.reset_history() when the history changes)")
                if float(t.reshape(-1)[0]) != ht:
                    raise RuntimeError(f"{who}: t[0]={float(t.reshape(-1)[0])} differs from the recorded {ht} (history_check; call "
                                       "engine.reset_history() when the history's timestep changes)")
            return "replay", key
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{who}: the record forward cannot run under a stream capture (run one eager forward of this clip, "
                               "conditioning and pack first; a replay captures)")
        return "record", key

    def _qkv_step(self, d, xs, scale_sa, shift_sa, ts, row_idx, h, qk, vt, eps):
        """the first adaLN of a block and its QKV projection, behind _blocks, _trimmed_block, _blocks_pair and _blocks_batch alike: q | k into
        qk [n, 2C], V as the K-major image vt[:, :n]. With fp8_qkv (and a block packed for it) the adaLN kernel emits the e4m3 rows and their
        scales itself and the e4m3 GEMM writes both outputs (yume_gemm_f8_splitt); h is then not written. Row-local: the callers' row ranges
        are handed on as they are. The byte and scale buffers are workspaces, allocated by the first eager forward. With int8_qkv the same pair
        runs on int8 rows (yume_adaln_modulate_i8 -> yume_gemm_i8_splitt), in front of the e4m3 branch where both options are on."""
        T = self._timed
        if "wqkvi" in d:
            # (r25) int8 rows in front of the e4m3 branch: the adaLN kernel emits the int8 rows and their scales, the int8 GEMM writes both outputs
            if self.fp8_qkv and not self._int8_qkv_said:
                self._int8_qkv_said = True
                if os.environ.get("YUME_GEMM_LOG", "0") not in ("", "0"):
                    sys.stderr.write("[int8_qkv] fp8_qkv is on too: the qualifying blocks run the int8 QKV / cross-q projections\n")
            n, C = h.shape
            hq = self._buf("qkv_hi8", (n, C), torch.int8, grow_rows=True)
            sh = self._buf("qkv_sh", (n,), torch.float32, grow_rows=True)
            T("adaln", ops.adaln_modulate_i8, xs, scale_sa, shift_sa, ts, row_idx, True, hq, sh, eps)
            T("gemm_qkv", ops.gemm_i8_splitt, hq, sh, d["wqkvi"], d["sqkvi"], d["bqkv"], qk, vt, 2 * C)
            return
        if "wqkvq" not in d:
            T("adaln", ops.adaln_modulate, xs, scale_sa, shift_sa, ts, row_idx, True, h, 0, eps)
            T("gemm_qkv", ops.gemm_bf16, h, d["wqkv"], d["bqkv"], qk, EPI_BF16_SPLITT, out_t=vt, n_split=2 * self.model.dim, variant=self.gemm_variant)
            return
        n, C = h.shape
        hq = self._buf("qkv_hq", (n, C), torch.uint8, grow_rows=True)
        sh = self._buf("qkv_sh", (n,), torch.float32, grow_rows=True)
        T("adaln", ops.adaln_modulate_e4m3, xs, scale_sa, shift_sa, ts, row_idx, True, hq, sh, eps)
        T("gemm_qkv", ops.gemm_f8_splitt, hq, sh, d["wqkvq"], d["sqkv"], d["bqkv"], qk, vt, 2 * C)

    def _cross_q_step(self, d, xs, h, q, eps):
        """norm3 (or, without its weights, the plain cast) of xs [n, C] and the cross-attention q projection into q [n, C], behind the same four
        bodies. With fp8_qkv (and norm3 weights: an adaLN launch has to be there to emit the bytes) the pair runs in e4m3 as _qkv_step's; with int8_qkv, in int8 (yume_adaln_modulate_i8 -> yume_gemm_i8), in front of it."""
        T = self._timed
        n, C = h.shape
        if "wq_ci" in d:
            hq = self._buf("qkv_hi8", (n, C), torch.int8, grow_rows=True)
            sh = self._buf("qkv_sh", (n,), torch.float32, grow_rows=True)
            T("adaln", ops.adaln_modulate_i8, xs, d["n3w"], d["n3b"], 0, None, False, hq, sh, eps)
            T("gemm_cross_q", ops.gemm_i8, hq, sh, d["wq_ci"], d["sq_ci"], d["bq_c"], q, EPI_BF16)
            return
        if "wq_cq" not in d:
            if "n3w" in d:
                T("adaln", ops.adaln_modulate, xs, d["n3w"], d["n3b"], 0, None, False, h, 0, eps)
            else:
                ops.cast_bf16(xs, n, h)
            T("gemm_cross_q", ops.gemm_bf16, h, d["wq_c"], d["bq_c"], q, EPI_BF16, variant=self.gemm_variant)
            return
        hq = self._buf("qkv_hq", (n, C), torch.uint8, grow_rows=True)
        sh = self._buf("qkv_sh", (n,), torch.float32, grow_rows=True)
        T("adaln", ops.adaln_modulate_e4m3, xs, d["n3w"], d["n3b"], 0, None, False, hq, sh, eps)
        T("gemm_cross_q", ops.gemm_f8, hq, sh, d["wq_cq"], d["sq_c"], d["bq_c"], q, EPI_BF16)

    def _ffn_block(self, d, xs, h, ff, scale_ff, shift_ff, gate_ff, ts, row_idx, eps):
        """the FFN adaLN and the FFN of a block, behind _blocks, _trimmed_block, _blocks_pair and _blocks_batch alike. With fp8_ffn_fused (where
        fp8_ffn is on and the block qualified at pack time, and ffn_dim % 32 == 0) neither quantiser pass exists: the adaLN kernel emits the
        e4m3 rows and their scales itself (bit-equal to adaln + quant_rows), ffn.0's GELU epilogue emits e4m3 with one E8M0 scale byte per row
        and 32 columns (OCP MX; no bf16 ff is written), and ffn.2 consumes those scales inside the MFMA. Everything is row-local; the byte and
        scale buffers are workspaces, allocated by the first eager forward."""
        T = self._timed
        if self.fp6_ffn and "w1p" in d:
            # (r23) MXFP6 e2m3, in front of the fp8 branch: adaLN emits packed e2m3 rows + E8M0 bytes, ffn.0's GELU epilogue emits the same, ffn.2
            # consumes them; the weights' block scales (e1 / e2) act inside the MFMA too. Row-local; the buffers are workspaces, allocated by the
            # first eager forward. Scale buffers have a pitch of whole 16-byte groups.
            if (self.fp8_ffn or self.fp8_ffn_fused) and not self._fp6_ffn_said and os.environ.get("YUME_GEMM_LOG", "0") not in ("", "0"):
                sys.stderr.write("[fp6_ffn] fp8_ffn is on too: the qualifying blocks run the MXFP6 FFN\n")
                self._fp6_ffn_said = True
            n, Cc, F = h.shape[0], h.shape[1], ff.shape[1]
            h6 = self._buf("ffn6_h", (n, 3 * Cc // 4), torch.uint8, grow_rows=True)
            he = self._buf("ffn6_he", (n, (Cc // 32 + 15) // 16 * 16), torch.uint8, grow_rows=True)[:, :Cc // 32]
            f6 = self._buf("ffn6_f", (n, 3 * F // 4), torch.uint8, grow_rows=True)
            fe = self._buf("ffn6_fe", (n, (F // 32 + 15) // 16 * 16), torch.uint8, grow_rows=True)[:, :F // 32]
            T("adaln", ops.adaln_modulate_mx_e2m3, xs, scale_ff, shift_ff, ts, row_idx, True, h6, he, eps)
            T("gemm_ffn0", ops.gemm_f6_mxout, h6, he, d["w1p"], d["e1"][:, :Cc // 32], d["b1"], f6, fe)
            T("gemm_ffn2", ops.gemm_f6_mx, f6, fe, d["w2p"], d["e2"][:, :F // 32], d["b2"], xs, EPI_RESID, gate=gate_ff, gate_stride=ts, row_idx=row_idx)
            return
        if not (self.fp8_ffn_fused and "w1q" in d and ff.shape[1] % 32 == 0):
            T("adaln", ops.adaln_modulate, xs, scale_ff, shift_ff, ts, row_idx, True, h, 0, eps)
            self._ffn(d, h, ff, xs, gate_ff, ts, row_idx)
            return
        n, F = h.shape[0], ff.shape[1]
        hq = self._buf("ffn_hq", (n, h.shape[1]), torch.uint8, grow_rows=True)
        sh = self._buf("ffn_sh", (n,), torch.float32, grow_rows=True)
        fq = self._buf("ffn_fq", (n, F), torch.uint8, grow_rows=True)
        fe = self._buf("ffn_fe", (n, (F // 32 + 15) // 16 * 16), torch.uint8, grow_rows=True)[:, :F // 32]     # (a pitch of whole 16-byte groups)
        T("adaln", ops.adaln_modulate_e4m3, xs, scale_ff, shift_ff, ts, row_idx, True, hq, sh, eps)
        T("gemm_ffn0", ops.gemm_f8_mxout, hq, sh, d["w1q"], d["s1"], d["b1"], fq, fe)
        T("gemm_ffn2", ops.gemm_f8_mx, fq, fe, d["w2q"], d["s2"], d["b2"], xs, EPI_RESID, gate=gate_ff, gate_stride=ts, row_idx=row_idx)

    def _ffn(self, d, h, ff, xs, gate_ff, ts, row_idx):
        """the block's FFN on h bf16 [n, C]: ff = gelu(h W1^T + b1), xs += (ff W2^T + b2) * gate. With fp8_ffn (and a block that qualified at
        pack time) both linears run in e4m3: quant_rows(h) -> gemm_f8 (GELU -> ff bf16) -> quant_rows(ff) -> gemm_f8 (RESID into xs). The byte
        and scale buffers are workspaces (nothing is allocated under a stream capture once they exist); the FFN is row-local, so sequence
        parallelism and the row-offset views of the trimmed block need nothing."""
        T = self._timed
        if "w1q" not in d:
            T("gemm_ffn0", ops.gemm_bf16, h, d["w1"], d["b1"], ff, EPI_BF16_GELU, variant=self.gemm_variant)
            T("gemm_ffn2", ops.gemm_bf16, ff, d["w2"], d["b2"], xs, EPI_RESID, gate=gate_ff, gate_stride=ts, row_idx=row_idx, variant=self.gemm_variant)
            return
        n = h.shape[0]
        hq = self._buf("ffn_hq", (n, h.shape[1]), torch.uint8, grow_rows=True)
        fq = self._buf("ffn_fq", (n, ff.shape[1]), torch.uint8, grow_rows=True)
        sh = self._buf("ffn_sh", (n,), torch.float32, grow_rows=True)
        sf = self._buf("ffn_sf", (n,), torch.float32, grow_rows=True)
        T("quant_rows", ops.quant_rows_e4m3, h, hq, sh)
        T("gemm_ffn0", ops.gemm_f8, hq, sh, d["w1q"], d["s1"], d["b1"], ff, EPI_BF16_GELU)
        T("quant_rows", ops.quant_rows_e4m3, ff, fq, sf)
        T("gemm_ffn2", ops.gemm_f8, fq, sf, d["w2q"], d["s2"], d["b2"], xs, EPI_RESID, gate=gate_ff, gate_stride=ts, row_idx=row_idx)

    def _trimmed_block(self, xs, L, s, d, i, tb, ts, row_idx, rope, eps, h, qk, vt, att, ff, kc_t, vct_t, ntxt, img, txt_last_weight=1.0,
                       txt_variant=0):
        """the block of _blocks with everything behind the QKV projection restricted to the rows [s, L) (trim_last_block): the same
        kernel calls on row-offset views, so the rows that are computed go through the same arithmetic."""
        m = self.model
        C, H = m.dim, m.num_heads
        T = self._timed
        shift_sa, scale_sa, gate_sa = tb[:, 0], tb[:, 1], tb[:, 2]
        shift_ff, scale_ff, gate_ff = tb[:, 3], tb[:, 4], tb[:, 5]
        xo, ho, ao, fo, qo = xs[s:], h[s:], att[s:], ff[s:], qk[s:, :C]
        ro = row_idx[s:] if row_idx is not None else None
        n = L - s
        self._qkv_step(d, xs, scale_sa, shift_sa, ts, row_idx, h, qk, vt, eps)
        T("rmsnorm_rope", ops.rmsnorm_rope, qk, C, 2, d["nqk"], self.qk_eps, rope)
        if self._hist_rec:
            self._hist_record(i, qk, vt)
        self._self_attn_step(qk, vt, ao, s, L, L)
        T("gemm_o", ops.gemm_bf16, ao, d["wo"], d["bo"], xo, EPI_RESID, gate=gate_sa, gate_stride=ts, row_idx=ro, variant=self.gemm_variant)
        self._cross_q_step(d, xo, ho, qo, eps)
        T("rmsnorm_rope", ops.rmsnorm_rope, qo, C, 1, d["nq_c"], self.qk_eps)
        T("attn_cross", ops.attn_fwd, qo, kc_t[:, i * C:(i + 1) * C], vct_t[i * C:(i + 1) * C], ao, n, ntxt, H, variant=txt_variant,
          q_prescaled=self.q_prescale, kv_padded=True, last_key_weight=txt_last_weight)
        if img is not None:
            kc_i, vct_i, n_img = img
            T("attn_cross", ops.attn_fwd, qo, kc_i[:, i * C:(i + 1) * C], vct_i[i * C:(i + 1) * C], ao, n, n_img, H, accumulate=True,
              variant=self.attn_variant, q_prescaled=self.q_prescale, kv_padded=True)
        T("gemm_cross_o", ops.gemm_bf16, ao, d["wo_c"], d["bo_c"], xo, EPI_RESID, variant=self.gemm_variant)
        self._ffn_block(d, xo, ho, fo, scale_ff, shift_ff, gate_ff, ts, ro, eps)

    # ------------------------------------------------------------------ one block through the engine (operator seam)
    @torch.no_grad()
    def block_forward(self, i, x, e, rope_cs, context, n_img=0):
        """WanAttentionBlock.forward for block i (reference wan23/modules/model.py:272-316, wan/modules/model.py:444-493):
        x [L, C] float; e fp32 [L, 6, C] (per token, 5B) or [1|6, C] (one row, 14B) — the time projection BEFORE the
        block's own modulation is added; rope_cs fp32 [n_rope, 64, 2] (cos, sin) of the first n_rope tokens or None;
        context [Lc, C] already embedded (the first n_img rows are CLIP image tokens). Returns fp32 [L, C].
        dedup_pad_keys does not reach this seam: an embedded context does not say how many of its rows came from pad rows, so every row is
        one key here, whatever the option says."""
        self.ensure_packed()
        C = self.model.dim
        L = x.shape[0]
        xs = self._buf("xs_blk", (L, C), torch.float32)
        xs.copy_(x.to(device=self.dev, dtype=torch.float32))
        e2 = e.to(device=self.dev, dtype=torch.float32).reshape(-1, 6 * C).contiguous()
        R = e2.shape[0]
        if R not in (1, L):
            raise RuntimeError(f"block modulation e has {R} rows for {L} tokens (expected 1 or one per token)")
        tab = self._buf("tab_blk", (1, R, 6 * C), torch.float32)
        ops.modulation_table(self.P["mod_all"][i:i + 1].contiguous(), e2, tab)
        row_idx = torch.arange(L, dtype=torch.int32, device=self.dev) if R > 1 else None
        ctx = context.to(device=self.dev, dtype=torch.bfloat16).contiguous()
        n_rope = 0 if rope_cs is None else rope_cs.shape[0]
        if n_rope == 0:
            rope_cs = torch.zeros((1, 64, 2), dtype=torch.float32, device=self.dev)
        self._ctx_key = None                                     # the per-conditioning cache belongs to forward_one
        self._spans = None                                       # (bare rows: no frame partition — a frame_window refuses by name)
        self._blocks(xs, L, tab.view(1, R, 6, C), row_idx, R, rope_cs.to(self.dev).contiguous(), n_rope, ctx, n_img, True, only=[i])
        return xs.clone()

    def _head(self, xs_new, row_idx_new, e, R, grid):
        """xs_new fp32 [Ln, C] -> fp32 [Cout, F, 2*Hp, 2*Wp]."""
        return self._unpatchify(self._head_rows(xs_new, row_idx_new, e, R), grid)

    def _unpatchify(self, y, grid):
        Co = self.model.out_dim
        Fr, Hp, Wp = grid
        out = torch.empty((Co, Fr, 2 * Hp, 2 * Wp), dtype=torch.float32, device=self.dev)
        ops.unpatchify(y, Fr, Hp, Wp, 2, 2, Co, out)
        return out

    def _head_rows(self, xs_new, row_idx_new, e, R):
        """xs_new fp32 [Ln, C] -> head output rows fp32 [Ln, 4*Cout] (model.py:344-347)."""
        m = self.model
        C, Co = m.dim, m.out_dim
        Ln = xs_new.shape[0]
        # (head.modulation [2, C] + e [R, C]) -> th[j, r, :]: j = 0 shift, 1 scale   (model.py:344)
        th = self._buf("tab_head", (2, R, C), torch.float32)
        ops.modulation_table(self.P["mod_head"], e, th)
        a3 = self._buf("head_a", (Ln, 3 * C), torch.bfloat16)
        ops.adaln_modulate(xs_new, th[1], th[0], C, row_idx_new, True, a3, 2, m.eps)
        y = self._buf("head_y", (Ln, 4 * Co), torch.float32)
        ops.gemm_bf16(a3, self.P["whead"], self.P["bhead"], y, EPI_F32, variant=self.gemm_variant)
        return y

    # ------------------------------------------------------------------ one sample forward
    def _prologue(self, u, t, packed, lfz, n_sel, pair=False, xs_rows=None, new_only=False):
        """what a forward does before the conditioning enters: the per-clip tables, the timestep rows, the patch embedding into the residual
        stream and the modulation table. Returns (xs, L, n_hist, grid, rope, R, row_idx, e, tab). pair: the residual stream is forward_pair's
        stacked buffer (the embedding fills its first L rows). xs_rows: a function L -> the rows of the residual stream the embedding fills
        (forward_batch: one sample's rows of its stacked buffer). new_only (a cache_history replay, packed): only the group of the frames being
        denoised is embedded, into a residual stream of n_new_tok rows; everything else returned is the whole clip's."""
        m = self.model
        C, D = m.dim, m.dim // m.num_heads
        if D != 128:
            raise RuntimeError("yume_amd attention kernels are built for head_dim 128")
        u = u.to(self.dev)
        if u.dtype not in (torch.float32, torch.bfloat16):
            u = u.float()
        u = u.contiguous()
        Cin, F, H, W = u.shape
        if Cin != m.in_dim:
            raise RuntimeError(f"input has {Cin} channels, model in_dim is {m.in_dim}")
        t64 = t.to(device=self.dev, dtype=torch.float64).reshape(-1).contiguous()

        if packed:
            def build():
                plan = framepack.pack_plan(F, H, W, lfz, n_sel)
                rope = framepack.plan_rope(plan, D).to(self.dev)
                ridx = torch.cat([torch.zeros(plan.n_hist_tok, dtype=torch.int32),
                                  torch.ones(plan.n_new_tok, dtype=torch.int32)]).to(self.dev)
                return plan, rope, ridx
            plan, rope, ridx = self._clip_tables(("p", F, H, W, lfz, n_sel), build)
            L, n_hist = plan.seq_len, plan.n_hist_tok
            groups, grid = plan.groups, plan.new_grid
            if self.frame_window is not None:
                self._spans = framepack.frame_spans(plan)
        else:
            def build():
                if H % 2 or W % 2:
                    # the base patch_embedding is an UNPADDED stride-2 Conv3d (model.py:455): odd sizes lose their last row / column
                    # there, while the pyramid levels pad (convpadd); no shipped resolution is odd — refuse instead of guessing
                    raise RuntimeError(f"latent H x W = {H} x {W} must be even for the (1, 2, 2) patch embedding")
                hp, wp = H // 2, W // 2
                rope = framepack.rope_cos_sin([(0, F, hp, wp)], D).to(self.dev)
                return framepack.Group(0, F, 0, hp, wp), rope
            g0, rope = self._clip_tables(("u", F, H, W), build)
            L, n_hist = g0.ntok, 0
            groups, grid = [g0], (F, g0.hp, g0.wp)
            if self.frame_window is not None:
                self._spans = framepack.frame_spans(g0)
            ridx = None

        # --- timestep rows
        if self.family == "wan":
            if t64.numel() != 1:
                raise RuntimeError("the 14B-arch model takes one scalar timestep per sample")
            R, t_index, row_idx = 1, None, None
        elif packed:
            if t64.numel() < 2:
                raise RuntimeError("FramePack path expects a per-token timestep vector (t[0] history, t[-1] new)")
            t_index = self._clip_tables(("ti", t64.numel()), lambda: torch.tensor(
                [0, t64.numel() - 1], dtype=torch.int32, device=self.dev))
            R, row_idx = 2, ridx
        elif t64.numel() == 1:
            R, t_index, row_idx = 1, None, None
        else:
            # arbitrary per-token timesteps (plain path): evaluate the distinct values only
            if t64.numel() < L:
                raise RuntimeError(f"per-token t has {t64.numel()} entries for {L} tokens")
            uniq, inv = torch.unique(t64[:L], return_inverse=True)
            t64, t_index, R = uniq.contiguous(), None, int(uniq.numel())
            row_idx = inv.to(torch.int32).contiguous()

        # --- embeddings
        if new_only:
            groups = groups[-1:]
            xs = self._buf("xs_hr", (groups[0].ntok, C), torch.float32)
        elif xs_rows is not None:
            xs = xs_rows(L)
        else:
            xs = self._buf("xs_p", (_round_up(L, 64) + L, C), torch.float32) if pair else self._buf("xs", (L, C), torch.float32)
        off = 0
        for g in groups:
            self._embed_group(u, g, xs[off:off + g.ntok])
            off += g.ntok
        e, e0 = self._time_rows(t64, t_index, R)
        nb = len(self.P["blocks"])
        tab = self._buf("tab", (nb, R, 6 * C), torch.float32)
        ops.modulation_table(self.P["mod_all"], e0, tab)
        return xs, L, n_hist, grid, rope, R, row_idx, e, tab

    @torch.no_grad()
    def forward_one(self, u, t, context, clip_fea=None, packed=True, lfz=8, n_sel=None, cache=None):
        """u [Cin, F, H, W] (fp32|bf16, x and y already concatenated); t tensor; context [Ltxt, text_dim].
        Returns fp32 [Cout, F', H, W]."""
        self.ensure_packed()
        m = self.model
        C = m.dim
        hist = self._history_mode(u, t, context, clip_fea, packed, lfz, n_sel, cache)
        replay = hist is not None and hist[0] == "replay"
        xs, L, n_hist, grid, rope, R, row_idx, e, tab = self._prologue(u, t, packed, lfz, n_sel, new_only=replay)
        nb = len(self.P["blocks"])
        n_img = 0
        if self.family == "wan":
            if clip_fea is None:
                raise RuntimeError("clip_fea is required by the i2v model")
            n_img = clip_fea.reshape(-1, clip_fea.shape[-1]).shape[0]
        # text rows of the context: text_len, or the prompt's n rows + one zero row that counts text_len - n times (dedup_pad_keys)
        n_txt, txt_w = m.text_len, 1.0
        if self.dedup_pad_keys and context.shape[0] < m.text_len:
            n_txt, txt_w = context.shape[0] + 1, float(m.text_len - context.shape[0])
        ctx = self._buf("ctx" if n_txt == m.text_len else f"ctx_{n_txt}", (n_img + n_txt, C), torch.bfloat16)
        ctx_fresh = True
        if self.cache_context:
            # storage address + version counter + shape (views of one tensor share all three); holding the references below
            # keeps those addresses from being handed to another tensor while the entry is live
            key = (context.data_ptr(), context._version, tuple(context.shape),
                   None if clip_fea is None else (clip_fea.data_ptr(), clip_fea._version, tuple(clip_fea.shape)),
                   self._packed_key, self.dedup_pad_keys)
            ctx_fresh = key != self._ctx_key
            self._ctx_key, self._ctx_refs = key, (context, clip_fea)
        else:
            self._ctx_key = None
        if ctx_fresh:
            if n_img:
                self._img_ctx(clip_fea, ctx[:n_img])
            self._text_ctx(context, ctx[n_img:])

        if self.sp is not None:
            if cache is not None:
                raise NotImplementedError("cache_sample is not combined with sequence parallelism")
            return self._forward_sp(xs, L, n_hist, tab.view(nb, R, 6, C), row_idx, R, rope, ctx, n_img, ctx_fresh, e, grid, txt_w)
        if replay:
            # the new rows alone, from row 0 of buffers of their own; nothing is left for trim_last_block to trim
            Ln, ridx_new = L - n_hist, row_idx[n_hist:]
            self._blocks(xs, Ln, tab.view(nb, R, 6, C), ridx_new, R, rope[n_hist:], Ln, ctx, n_img, ctx_fresh, txt_last_weight=txt_w, hist=n_hist)
            return self._head(xs, ridx_new, e, R, grid)
        n_trim = n_hist if (self.trim_last_block and cache is None) else 0
        if hist is not None:
            # a record forward: today's forward, and each block's history K rows / V^T columns kept behind its rmsnorm_rope
            self._hist_key = None
            self._hist_rec = n_hist
            self._hist_kept = (u[:, :u.shape[1] - lfz].detach().clone(), float(t.reshape(-1)[0])) if self.history_check else None
        try:
            self._blocks(xs, L, tab.view(nb, R, 6, C), row_idx, R, rope, L, ctx, n_img, ctx_fresh, cache=cache, n_trim=n_trim,
                         txt_last_weight=txt_w)
        finally:
            self._hist_rec = None
        if hist is not None:
            self._hist_key, self._hist_refs = hist[1], (context, clip_fea)
        ridx_new = row_idx[n_hist:] if row_idx is not None else None
        return self._head(xs[n_hist:], ridx_new, e, R, grid)

    # ------------------------------------------------------------------ a guided (classifier-free guidance) pair in one pass
    @torch.no_grad()
    def forward_pair(self, u, t, context, context_null, clip_fea=None, packed=True, lfz=8, n_sel=None):
        """The two forwards of a classifier-free-guidance step — same u, t and clip_fea, two prompts (fastvideo/sample/sample.py:774-779) — as
        ONE pass over the stacked rows of both legs. Returns (cond, uncond), each what forward_one returns for that context (fp32).

        Everything in front of block 0's first cross-attention does not depend on the prompt and runs once on L rows: patch embedding, time
        rows, modulation table, the CLIP image context with its K / V^T, and block 0's adaLN -> QKV -> RMSNorm+RoPE -> self-attention ->
        o projection. The residual stream is then copied to leg 1, `pitch` = ceil(L / 64) * 64 rows further on: the QKV GEMM writes V^T
        columns by stacked row and the self-attention kernels fetch K rows / V^T columns up to a whole 64-key tile, so leg 1 must start on
        a tile. The pitch - L rows between the legs are a token of their own (they start at zero, stay finite, are never keys and never
        returned). From there every adaLN, cast, GEMM and norm launch runs once over the pitch + L stacked rows with the row selector and
        RoPE table repeated per leg; self-attention is one launch per leg on row / column views; the CLIP image cross-attention one
        accumulating launch over all stacked queries (both legs share its keys); the text cross-attention ONE segmented launch
        (ops.attn_fwd_seg), each leg over its own K / V^T — with dedup_pad_keys its own n + 1 keys and last-key weight.

        cache_context keys on both contexts (and keeps its own K / V^T buffers: forward_one's cache is not disturbed). trim_last_block is
        ignored here: the last block runs on every row. Sequence parallelism and the block-residual cache are not implemented for the pair."""
        self._refuse_window("forward_pair / forward_cfg")
        self._refuse_frame_window("forward_pair / forward_cfg")
        if self.sp is not None:
            raise NotImplementedError("forward_pair is not implemented under sequence parallelism (enable_sequence_parallel)")
        self.ensure_packed()
        m = self.model
        C, H, nb = m.dim, m.num_heads, len(self.P["blocks"])
        xs, L, n_hist, grid, rope, R, row_idx, e, tab = self._prologue(u, t, packed, lfz, n_sel, pair=True)
        pitch = _round_up(L, 64)
        M = pitch + L                                                   # stacked rows: leg 0, the gap, leg 1
        n_img = 0
        if self.family == "wan":
            if clip_fea is None:
                raise RuntimeError("clip_fea is required by the i2v model")
            n_img = clip_fea.reshape(-1, clip_fea.shape[-1]).shape[0]
        legs = []
        for c in (context, context_null):
            n_txt, txt_w = m.text_len, 1.0
            if self.dedup_pad_keys and c.shape[0] < m.text_len:
                n_txt, txt_w = c.shape[0] + 1, float(m.text_len - c.shape[0])
            legs.append((c, n_txt, txt_w))
        ctx_fresh = True
        if self.cache_context:
            key = tuple((c.data_ptr(), c._version, tuple(c.shape)) for c in (context, context_null)) + (
                None if clip_fea is None else (clip_fea.data_ptr(), clip_fea._version, tuple(clip_fea.shape)), self._packed_key, self.dedup_pad_keys)
            ctx_fresh = key != self._pair_ctx_key
            self._pair_ctx_key, self._pair_ctx_refs = key, (context, context_null, clip_fea)
        else:
            self._pair_ctx_key = None
        cols = _round_up(max(n for _, n, _ in legs), 64)               # one V^T row stride for both legs
        kv_t = []
        for s, (c, n_txt, _) in enumerate(legs):
            ctx = self._buf(f"ctx_p{s}_{n_txt}", (n_txt, C), torch.bfloat16)
            if ctx_fresh:
                self._text_ctx(c, ctx)
            kv_t.append(self._cross_kv(f"p{s}c{cols}", ctx, n_txt, self.P["wkv_c"], self.P["bkv_c"], self.P["nk_c"], ctx_fresh, cols=cols))
        kv_i = None
        if n_img:
            ctx = self._buf("ctx_pi", (n_img, C), torch.bfloat16)
            if ctx_fresh:
                self._img_ctx(clip_fea, ctx)
            kv_i = self._cross_kv("pi", ctx, n_img, self.P["wkv_i"], self.P["bkv_i"], self.P["nk_i"], ctx_fresh)

        # --- stacked tables: the row selector and the RoPE rows once per leg (the gap: row 0 of the table, a zero rotation)
        ridx2 = None
        if row_idx is not None:
            ridx2 = self._buf("ridx_p", (M,), torch.int32, zero=True)
            ridx2[:L].copy_(row_idx)
            ridx2[pitch:].copy_(row_idx)
        rope2 = self._buf("rope_p", (M,) + tuple(rope.shape[1:]), torch.float32, zero=True)
        rope2[:L].copy_(rope)
        rope2[pitch:].copy_(rope)
        self._blocks_pair(xs, L, pitch, tab.view(nb, R, 6, C), row_idx, ridx2, rope, rope2, kv_t, [n for _, n, _ in legs],
                          [w for _, _, w in legs], kv_i, n_img)
        ridx_new = row_idx[n_hist:] if row_idx is not None else None
        return tuple(self._head(xs[o + n_hist:o + L], ridx_new, e, R, grid) for o in (0, pitch))

    def _blocks_pair(self, xs, L, pitch, tab, row_idx, ridx2, rope, rope2, kv_t, n_txt, txt_w, kv_i, n_img):
        """the blocks of forward_pair. xs fp32 [pitch + L, C]: rows [0, L) hold the embedded tokens on entry, both legs' outputs on exit
        (leg 1 at row `pitch`). The same kernel calls as _blocks, on the stacked rows."""
        m = self.model
        C, H, Fd, eps = m.dim, m.num_heads, m.ffn_dim, m.eps
        M = pitch + L
        self._fp8_attn_notice("forward_pair / forward_cfg keep the bf16 self-attention kernels")
        # rows and V^T columns exist up to a whole key tile behind leg 1 as well (zeros nobody writes): YUME_ATTN_KV_PADDED per leg
        h = self._buf("h_p", (M, C), torch.bfloat16)
        qk = self._buf("qk_p", (2 * pitch, 2 * C), torch.bfloat16, zero=True)
        vt = self._buf("vt_p", (C, 2 * pitch), torch.bfloat16, zero=True)
        att = self._buf("att_p", (M, C), torch.bfloat16, zero=True)
        ff = self._buf("ff_p", (M, Fd), torch.bfloat16)
        ts = 6 * C
        T = self._timed
        # (the register-staged kernel of the cross-check mode has no segmented form: the 4-wave LDS-DMA kernel then)
        txt_variant = 2 if self.attn_variant == 1 else self.attn_variant
        if pitch > L:
            xs[L:pitch].zero_()                                         # the gap starts every call as a zero token ...
            att[L:pitch].zero_()                                        # ... whose attention rows only the image branch adds to
        for i, d in enumerate(self.P["blocks"]):
            tb = tab[i]
            shift_sa, scale_sa, gate_sa = tb[:, 0], tb[:, 1], tb[:, 2]
            shift_ff, scale_ff, gate_ff = tb[:, 3], tb[:, 4], tb[:, 5]
            # --- self attention: block 0 once, on the L rows both legs share; later blocks over the stacked rows, one attention launch per leg
            n, ri, ro = (L, row_idx, rope) if i == 0 else (M, ridx2, rope2)
            self._qkv_step(d, xs[:n], scale_sa, shift_sa, ts, ri, h[:n], qk[:n], vt, eps)
            T("rmsnorm_rope", ops.rmsnorm_rope, qk[:n], C, 2, d["nqk"], self.qk_eps, ro)
            if i > 0 and self.pair_self_batched:
                T("attn_self", ops.attn_fwd_batch, qk[:M, :C], qk[:, C:], vt, att, 2, L, pitch, L, pitch, H, variant=self.batch_attn_variant,
                  q_prescaled=self.q_prescale, kv_padded=True)
            for o in (() if i > 0 and self.pair_self_batched else (0,) if i == 0 else (0, pitch)):
                T("attn_self", ops.attn_fwd, qk[o:o + L, :C], qk[o:o + L, C:], vt[:, o:o + pitch], att[o:o + L], L, L, H, variant=self.attn_variant,
                  q_prescaled=self.q_prescale, kv_padded=True)
            T("gemm_o", ops.gemm_bf16, att[:n], d["wo"], d["bo"], xs[:n], EPI_RESID, gate=gate_sa, gate_stride=ts, row_idx=ri, variant=self.gemm_variant)
            if i == 0:
                xs[pitch:].copy_(xs[:L])                                # the legs part here
            # --- cross attention
            self._cross_q_step(d, xs, h, qk[:M, :C], eps)
            T("rmsnorm_rope", ops.rmsnorm_rope, qk[:M, :C], C, 1, d["nq_c"], self.qk_eps)
            T("attn_cross", ops.attn_fwd_seg, qk[:M, :C], [kc[:, i * C:(i + 1) * C] for kc, _ in kv_t], [v[i * C:(i + 1) * C] for _, v in kv_t],
              att, L, pitch, n_txt, H, variant=txt_variant, q_prescaled=self.q_prescale, kv_padded=True, last_key_weights=txt_w)
            if n_img:
                T("attn_cross", ops.attn_fwd, qk[:M, :C], kv_i[0][:, i * C:(i + 1) * C], kv_i[1][i * C:(i + 1) * C], att, M, n_img, H, accumulate=True,
                  variant=self.attn_variant, q_prescaled=self.q_prescale, kv_padded=True)
            T("gemm_cross_o", ops.gemm_bf16, att, d["wo_c"], d["bo_c"], xs, EPI_RESID, variant=self.gemm_variant)
            # --- FFN
            self._ffn_block(d, xs, h, ff, scale_ff, shift_ff, gate_ff, ts, ridx2, eps)

    # ------------------------------------------------------------------ several samples in one pass
    @torch.no_grad()
    def forward_batch(self, us, ts, contexts, clip_feas=None, packed=True, lfz=8, n_sel=None, cache=None):
        """B (2 .. 8) samples of ONE shape in one pass over their stacked rows: us, ts, contexts lists of what forward_one takes (the
        timesteps, the prompts and their lengths are per sample), clip_feas a list or ONE tensor shared by all samples (14B); packed, lfz,
        n_sel common. Returns a list of fp32 outputs, each what forward_one returns for that sample. B == 1 calls forward_one.

        Sample s is at row s * pitch, pitch = ceil(L / 64) * 64 (the QKV GEMM writes V^T columns by stacked row and the attention kernels
        fetch K rows / V^T columns in whole 64-key tiles, as in forward_pair); the rows between two samples are zero tokens that are never
        keys and never returned. The prologue (patch embedding, time rows, modulation table) runs per sample into the stacked residual
        stream and a stacked modulation table whose rows the row selector picks per sample (an explicit selector also where forward_one
        passes none: t differs per sample). Every adaLN, cast, GEMM and RMSNorm+RoPE launch runs once over the stacked rows;
        self-attention is ONE ops.attn_fwd_batch launch per block; the text cross-attention one ops.attn_fwd_seg launch, each sample over
        its own K / V^T (with dedup_pad_keys its own n + 1 keys and last-key weight); the 14B image cross-attention one accumulating
        ops.attn_fwd over all stacked rows when every sample carries the same clip_fea tensor, one accumulating ops.attn_fwd_seg with
        per-sample image keys otherwise. Head and unpatchify run per sample.

        cache_context keys on all prompts and clip_feas (own buffers: forward_one's and forward_pair's caches are not disturbed);
        trim_last_block is ignored. Sequence parallelism and the block-residual cache are not implemented for the batch."""
        self._refuse_window("forward_batch")
        self._refuse_frame_window("forward_batch")
        B = len(us)
        if len(ts) != B or len(contexts) != B:
            raise RuntimeError(f"forward_batch: {B} samples, {len(ts)} timesteps, {len(contexts)} contexts")
        if isinstance(clip_feas, torch.Tensor):
            clip_feas = [clip_feas] * B
        if clip_feas is not None and len(clip_feas) != B:
            raise RuntimeError(f"forward_batch: {B} samples, {len(clip_feas)} clip_feas")
        if cache is not None:
            raise NotImplementedError("forward_batch does not implement the block-residual cache (cache_sample); use forward_one per sample")
        if self.sp is not None:
            raise NotImplementedError("forward_batch is not implemented under sequence parallelism (enable_sequence_parallel)")
        if B == 1:
            return [self.forward_one(us[0], ts[0], contexts[0], clip_fea=None if clip_feas is None else clip_feas[0], packed=packed, lfz=lfz,
                                     n_sel=n_sel)]
        if not 2 <= B <= 8:
            raise RuntimeError(f"forward_batch takes 1 .. 8 samples per pass, got {B}")
        if any(tuple(u.shape) != tuple(us[0].shape) for u in us):
            raise RuntimeError("forward_batch: the samples of one pass must have one shape: " + ", ".join(str(tuple(u.shape)) for u in us))
        self.ensure_packed()
        m = self.model
        C, nb = m.dim, len(self.P["blocks"])
        n_img = 0
        if self.family == "wan":
            if clip_feas is None or any(c is None for c in clip_feas):
                raise RuntimeError("clip_fea is required by the i2v model")
            n_img = clip_feas[0].reshape(-1, clip_feas[0].shape[-1]).shape[0]
            if any(c.reshape(-1, c.shape[-1]).shape[0] != n_img for c in clip_feas):
                raise RuntimeError("forward_batch: every clip_fea must have the same number of image tokens")

        # --- the prologue per sample, into the stacked residual stream, modulation table and time rows
        state = {}

        def rows_of(s):
            def get(L):
                pitch = _round_up(L, 64)
                xs = self._buf("xs_b", ((B - 1) * pitch + L, C), torch.float32)
                state["xs"] = xs
                return xs[s * pitch:s * pitch + L]
            return get
        per, r_off = [], 0
        for s in range(B):
            _, L, n_hist, grid, rope, R, row_idx, e, tab = self._prologue(us[s], ts[s], packed, lfz, n_sel, xs_rows=rows_of(s))
            # (e and tab are the engine's per-call buffers: the next sample's prologue overwrites them)
            per.append((R, r_off, row_idx, e.clone(), tab.view(nb, R, 6 * C).clone()))
            r_off += R
        xs, RT = state["xs"], r_off
        pitch = _round_up(L, 64)
        M = (B - 1) * pitch + L
        tabs = self._buf("tab_b", (nb, RT, 6 * C), torch.float32)
        ridx = self._buf("ridx_b", (M,), torch.int32, zero=True)            # (the gaps: row 0 of the table)
        ropes = self._buf("rope_b", (M,) + tuple(rope.shape[1:]), torch.float32, zero=True)    # (the gaps: a zero rotation)
        for s, (R, off, row_idx, _, tab) in enumerate(per):
            tabs[:, off:off + R].copy_(tab)
            if row_idx is None:
                ridx[s * pitch:s * pitch + L].fill_(off)
            else:
                torch.add(row_idx, off, out=ridx[s * pitch:s * pitch + L])
            ropes[s * pitch:s * pitch + L].copy_(rope)
            if s and pitch > L:
                xs[s * pitch - (pitch - L):s * pitch].zero_()               # the gap in front of sample s starts every call as a zero token

        # --- conditioning: every sample its own text K / V^T; the image K / V^T once when all samples share one clip_fea tensor
        legs = []
        for c in contexts:
            n_txt, txt_w = m.text_len, 1.0
            if self.dedup_pad_keys and c.shape[0] < m.text_len:
                n_txt, txt_w = c.shape[0] + 1, float(m.text_len - c.shape[0])
            legs.append((c, n_txt, txt_w))
        img_shared = n_img > 0 and all(c is clip_feas[0] for c in clip_feas)
        ctx_fresh = True
        if self.cache_context:
            ident = lambda c: None if c is None else (c.data_ptr(), c._version, tuple(c.shape))
            key = (tuple(ident(c) for c in contexts), None if clip_feas is None else tuple(ident(c) for c in clip_feas), img_shared,
                   self._packed_key, self.dedup_pad_keys)
            ctx_fresh = key != self._batch_ctx_key
            self._batch_ctx_key, self._batch_ctx_refs = key, (list(contexts), None if clip_feas is None else list(clip_feas))
        else:
            self._batch_ctx_key = None
        cols = _round_up(max(n for _, n, _ in legs), 64)                   # one V^T row stride for all samples
        kv_t = []
        for s, (c, n_txt, _) in enumerate(legs):
            ctx = self._buf(f"ctx_b{s}_{n_txt}", (n_txt, C), torch.bfloat16)
            if ctx_fresh:
                self._text_ctx(c, ctx)
            kv_t.append(self._cross_kv(f"b{s}c{cols}", ctx, n_txt, self.P["wkv_c"], self.P["bkv_c"], self.P["nk_c"], ctx_fresh, cols=cols))
        kv_i = []
        for s in range(1 if img_shared else B if n_img else 0):
            ctx = self._buf(f"ctx_bi{s}", (n_img, C), torch.bfloat16)
            if ctx_fresh:
                self._img_ctx(clip_feas[s], ctx)
            kv_i.append(self._cross_kv(f"bi{s}", ctx, n_img, self.P["wkv_i"], self.P["bkv_i"], self.P["nk_i"], ctx_fresh))

        self._blocks_batch(xs, B, L, pitch, tabs.view(nb, RT, 6, C), ridx, ropes, kv_t, [n for _, n, _ in legs], [w for _, _, w in legs],
                           kv_i, n_img)
        outs = []
        for s, (R, _, row_idx, e, _) in enumerate(per):
            ridx_new = row_idx[n_hist:] if row_idx is not None else None
            outs.append(self._head(xs[s * pitch + n_hist:s * pitch + L], ridx_new, e, R, grid))
        return outs

    def _blocks_batch(self, xs, B, L, pitch, tab, ridx, rope, kv_t, n_txt, txt_w, kv_i, n_img):
        """the blocks of forward_batch. xs fp32 [(B - 1) * pitch + L, C]: sample s at row s * pitch, in and out. The same kernel calls as
        _blocks, on the stacked rows. kv_i: one (K, V^T) of the image tokens shared by all samples, or one per sample."""
        m = self.model
        C, H, Fd, eps = m.dim, m.num_heads, m.ffn_dim, m.eps
        M = (B - 1) * pitch + L
        self._fp8_attn_notice("forward_batch keeps the bf16 self-attention kernels")
        # rows and V^T columns exist up to a whole key tile behind the last sample as well (zeros nobody writes): YUME_ATTN_KV_PADDED per sample
        h = self._buf("h_b", (M, C), torch.bfloat16)
        qk = self._buf("qk_b", (B * pitch, 2 * C), torch.bfloat16, zero=True)
        vt = self._buf("vt_b", (C, B * pitch), torch.bfloat16, zero=True)
        att = self._buf("att_b", (M, C), torch.bfloat16, zero=True)
        ff = self._buf("ff_b", (M, Fd), torch.bfloat16)
        ts = 6 * C
        T = self._timed
        # (the register-staged kernel of the cross-check mode has no segmented form: the 4-wave LDS-DMA kernel then)
        seg_variant = 2 if self.attn_variant == 1 else self.attn_variant
        if pitch > L:
            for s in range(1, B):
                att[s * pitch - (pitch - L):s * pitch].zero_()           # the gaps' attention rows: only a shared image branch adds to them
        for i, d in enumerate(self.P["blocks"]):
            tb = tab[i]
            shift_sa, scale_sa, gate_sa = tb[:, 0], tb[:, 1], tb[:, 2]
            shift_ff, scale_ff, gate_ff = tb[:, 3], tb[:, 4], tb[:, 5]
            # --- self attention: one launch over the (sample, head) pairs
            self._qkv_step(d, xs, scale_sa, shift_sa, ts, ridx, h, qk[:M], vt, eps)
            T("rmsnorm_rope", ops.rmsnorm_rope, qk[:M], C, 2, d["nqk"], self.qk_eps, rope)
            T("attn_self", ops.attn_fwd_batch, qk[:M, :C], qk[:, C:], vt, att, B, L, pitch, L, pitch, H, variant=self.batch_attn_variant,
              q_prescaled=self.q_prescale, kv_padded=True)
            T("gemm_o", ops.gemm_bf16, att, d["wo"], d["bo"], xs, EPI_RESID, gate=gate_sa, gate_stride=ts, row_idx=ridx, variant=self.gemm_variant)
            # --- cross attention
            self._cross_q_step(d, xs, h, qk[:M, :C], eps)
            T("rmsnorm_rope", ops.rmsnorm_rope, qk[:M, :C], C, 1, d["nq_c"], self.qk_eps)
            T("attn_cross", ops.attn_fwd_seg, qk[:M, :C], [kc[:, i * C:(i + 1) * C] for kc, _ in kv_t], [v[i * C:(i + 1) * C] for _, v in kv_t],
              att, L, pitch, n_txt, H, variant=seg_variant, q_prescaled=self.q_prescale, kv_padded=True, last_key_weights=txt_w)
            if len(kv_i) == 1:
                T("attn_cross", ops.attn_fwd, qk[:M, :C], kv_i[0][0][:, i * C:(i + 1) * C], kv_i[0][1][i * C:(i + 1) * C], att, M, n_img, H,
                  accumulate=True, variant=self.attn_variant, q_prescaled=self.q_prescale, kv_padded=True)
            elif kv_i:
                T("attn_cross", ops.attn_fwd_seg, qk[:M, :C], [kc[:, i * C:(i + 1) * C] for kc, _ in kv_i], [v[i * C:(i + 1) * C] for _, v in kv_i],
                  att, L, pitch, [n_img] * B, H, accumulate=True, variant=seg_variant, q_prescaled=self.q_prescale, kv_padded=True)
            T("gemm_cross_o", ops.gemm_bf16, att, d["wo_c"], d["bo_c"], xs, EPI_RESID, variant=self.gemm_variant)
            # --- FFN
            self._ffn_block(d, xs, h, ff, scale_ff, shift_ff, gate_ff, ts, ridx, eps)

    def _forward_sp(self, xs, L, n_hist, tab, row_idx, R, rope, ctx, n_img, ctx_fresh, e, grid, txt_last_weight=1.0):
        """Blocks + head on this rank's token chunk (sequence_parallel.py:121-152: chunk after the embeddings, gather
        after the head). The embeddings above were computed for all L tokens on every rank (< 0.1 % of the FLOPs)."""
        sp, C = self.sp, self.model.dim
        sp.check_heads(self.model.num_heads)
        Lp, lo, hi = sp.chunk(L)
        n = hi - lo
        xl = self._buf("xs_sp", (Lp, C), torch.float32)
        xl[:n].copy_(xs[lo:hi])
        xl[n:].zero_()                                   # pad tokens: finite rows, masked as keys, dropped at the end
        rl = self._buf("rope_sp", (Lp,) + tuple(rope.shape[1:]), torch.float32)
        rl[:n].copy_(rope[lo:hi])
        rl[n:].zero_()
        il = None
        if row_idx is not None:
            il = self._buf("ridx_sp", (Lp,), torch.int32)
            il[:n].copy_(row_idx[lo:hi])
            il[n:].zero_()
        self._blocks(xl, Lp, tab, il, R, rl, Lp, ctx, n_img, ctx_fresh, n_keys=L, txt_last_weight=txt_last_weight)
        y = sp.gather_rows(self._head_rows(xl, il, e, R))
        return self._unpatchify(y[n_hist:L].contiguous(), grid)
