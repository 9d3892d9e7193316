"""`flash_attention` operator seam (reference: wan/modules/attention.py:24-130 == wan23/modules/attention.py).

Same signature and return convention as the reference wrapper around flash-attn's varlen kernel: q,k,v are
[B, L, N, D] tensors of any float dtype on the GPU, output is [B, Lq, N, D] in q's dtype. Rebinding
`wan23.modules.model.flash_attention = yume_amd.attention.flash_attention` in the reference tree is enough to
route the reference model's attention through the gfx950 kernel.

`causal` and `window_size` carry flash-attn 2.7's meaning (bottom-right aligned; yume_attn_fwd_band): per sample, query row i sits at
(nk - nq) + i on the key axis and sees the keys within window_size[0] to its left and window_size[1] to its right (-1: unbounded; causal
sets the right side to 0). A row that sees no key is 0. A window that hides nothing is the global call, bit for bit.
"""
import math

import torch

from . import ops

__all__ = ["flash_attention", "attention", "frame_window_attention", "frame_sink_attention"]


def flash_attention(q, k, v, q_lens=None, k_lens=None, dropout_p=0., softmax_scale=None, q_scale=None, causal=False,
                    window_size=(-1, -1), deterministic=False, dtype=torch.bfloat16, version=None):
    assert dtype in (torch.float16, torch.bfloat16)
    assert q.device.type == "cuda" and q.size(-1) <= 256
    if dropout_p != 0.:
        raise NotImplementedError("yume_amd.flash_attention: dropout is not implemented (no Yume model uses it)")
    # flash-attn 2.7: causal is window_size[1] = 0; rows are bottom-right aligned, i.e. query row i of a sample sits at (nk - nq) + i
    left, right = int(window_size[0]), int(window_size[1])
    if left < -1 or right < -1:
        raise ValueError(f"yume_amd.flash_attention: window_size={tuple(window_size)}: -1 (unbounded) or a non-negative width per side")
    if causal:
        right = 0
    if dtype != torch.bfloat16:
        raise NotImplementedError("yume_amd.flash_attention computes in bf16 (the reference default)")
    return _attend(q, k, v, q_lens, k_lens, softmax_scale, q_scale, lambda nq, nk: dict(window=(left, right), q_pos0=nk - nq))


def _attend(q, k, v, q_lens, k_lens, softmax_scale, q_scale, mask):
    """the seam's body: per sample one ops.attn_fwd call with the mask arguments mask(nq, nk) gives"""
    b, lq, n, d = q.shape
    lk = k.size(1)
    if k.size(2) != n or v.size(-1) != d:
        raise NotImplementedError("yume_amd.flash_attention: equal q/k/v head counts and head dims only")
    if d > 128:
        raise NotImplementedError(f"yume_amd.flash_attention: head_dim {d} > 128 is not built (the reference accepts <= 256; "
                                  "no Yume model uses it)")
    d_in = d
    if d < 128:
        # zero columns add nothing to q.k and produce zero output columns: exact. (CLIP ViT-H/14 has head_dim 80.)
        pad = lambda t: torch.nn.functional.pad(t, (0, 128 - d_in))
        q, k, v = pad(q), pad(k), pad(v)
        d = 128
    out_dtype = q.dtype
    out = torch.empty((b, lq, n * d), dtype=torch.bfloat16, device=q.device)
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(d_in)
    for i in range(b):
        nq = int(q_lens[i]) if q_lens is not None else lq
        nk = int(k_lens[i]) if k_lens is not None else lk
        qi = q[i, :nq].reshape(nq, n * d)
        if q_scale is not None:
            qi = qi * q_scale
        qi = qi.to(torch.bfloat16).contiguous()
        ki = k[i, :nk].reshape(nk, n * d).to(torch.bfloat16).contiguous()
        vi = v[i, :nk].reshape(nk, n * d)
        if vi.dtype not in (torch.float32, torch.bfloat16):
            vi = vi.float()
        vt = torch.empty((n * d, (nk + 7) // 8 * 8), dtype=torch.bfloat16, device=q.device)
        ops.transpose_bf16(vi.contiguous(), vt)
        ops.attn_fwd(qi, ki, vt, out[i, :nq], nq, nk, n, scale=scale, **mask(nq, nk))
        if nq < lq:
            out[i, nq:].zero_()   # flash-attn's varlen packing leaves padded queries out; the reference never reads them
    return out.view(b, lq, n, d)[..., :d_in].type(out_dtype)


def frame_window_attention(q, k, v, spans, frame_window, q_lens=None, k_lens=None, softmax_scale=None):
    """flash_attention's tensor conventions (q [B, Lq, N, d], k / v [B, Lk, N, d], optional per-sample lengths, bf16 compute, the output in
    q's dtype) under a FRAME-aligned window: spans = [(rows, blocks), ...] partitions the key axis into frames (framepack.frame_spans), and a
    query sees every key of the frames within frame_window = (back, ahead) of its own (-1: unbounded; (-1, 0): frame-causal). Rows are
    bottom-right aligned per sample as in flash_attention: query row i sits at (nk - nq) + i. A row that sees no key is 0; a window that hides
    nothing is the global call, bit for bit. A function of its own: flash_attention's signature is the reference's."""
    return _frame_attend("frame_window_attention", q, k, v, spans, frame_window, 0, q_lens, k_lens, softmax_scale)


def frame_sink_attention(q, k, v, spans, frame_window, sink, q_lens=None, k_lens=None, softmax_scale=None):
    """frame_window_attention with an always-visible sink: every query also sees the first `sink` frames of the partition (0 <= sink <= the
    partition's frames; yume_attn_fwd_fsink) — the clip's first frame under FramePack, the anchor a local window would hide. sink = 0 is
    frame_window_attention, bit for bit. A function of its own: frame_window_attention's signature is held by its tests."""
    sink = int(sink)
    if sink < 0:
        raise ValueError(f"yume_amd.frame_sink_attention: sink={sink}: a non-negative count of leading frames")
    return _frame_attend("frame_sink_attention", q, k, v, spans, frame_window, sink, q_lens, k_lens, softmax_scale)


def _frame_attend(who, q, k, v, spans, frame_window, sink, q_lens, k_lens, softmax_scale):
    assert q.device.type == "cuda" and q.size(-1) <= 256
    back, ahead = int(frame_window[0]), int(frame_window[1])
    if back < -1 or ahead < -1:
        raise ValueError(f"yume_amd.{who}: frame_window={tuple(frame_window)}: -1 (unbounded) or a non-negative frame count "
                         "per side")
    spans = [(int(r), int(b)) for r, b in spans]
    extra = {"frame_sink": sink} if sink else {}
    return _attend(q, k, v, q_lens, k_lens, softmax_scale, None,
                   lambda nq, nk: dict(frame_window=(back, ahead), spans=spans, q_pos0=nk - nq, **extra))


def attention(q, k, v, q_lens=None, k_lens=None, dropout_p=0., softmax_scale=None, q_scale=None, causal=False,
              window_size=(-1, -1), deterministic=False, dtype=torch.bfloat16, fa_version=None):
    """reference attention.py:133-179: same as flash_attention when a flash kernel exists — here it always does."""
    return flash_attention(q, k, v, q_lens, k_lens, dropout_p, softmax_scale, q_scale, causal, window_size,
                           deterministic, dtype, fa_version)
