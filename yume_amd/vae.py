"""Causal 3D VAE engine (Wan2.2 and Wan2.1) on the HIP kernels: chunked encode / decode with the reference's
feat_cache semantics, on channels-last bf16 activations.

Reference behaviour reproduced (wan23/modules/vae2_2.py, wan/modules/vae.py):
  * decode walks the latent one frame at a time (vae2_2.py:839-857), encode in chunks of 1,4,4,... frames (:802-820) — a memory
    measure of the reference: a causal convolution fed [cache ++ chunk] computes the same outputs whatever the chunk length. Here the
    first chunk runs alone (it is the one with different arithmetic: no time_conv in the resamplers) and the following chunks run
    `group` at a time (default 8: 288 GB of HBM hold a 28-frame 704x1280 decode, ~20 GB): at one latent frame per pass the
    44x80 and 88x160 stages launch 56-tile GEMMs on a 256-CU chip, 13 % of the decode time for 3 % of its FLOPs;
  * every temporal conv keeps the last two input frames of the previous chunk (a [2,H,W,C] ring here, passed to the
    conv kernel as its `cache` operand instead of torch.cat + F.pad);
  * upsample3d's time_conv is skipped on the first chunk and starts from a zero cache ('Rep', :116-149);
    downsample3d's strided time_conv is skipped on the first chunk (:159-170);
  * Wan2.2 adds the parameter-free AvgDown3D / DupUp3D shortcuts (:322-418) and patchify(2) (:286-319).
Numerics: bf16 activations and weights, fp32 accumulation, fp32 RMS_norm statistics and softmax. The reference
runs this module in fp32; the stated tolerance is in tests/test_vae_gpu.py and DESIGN.md.
"""
import math
import os

import torch
import torch.nn as nn

from . import ops
from . import vae_ops as V


def _ru(a, b):
    return (a + b - 1) // b * b


def decode_passes(T, group):
    """[(first_latent, end_latent, first_chunk)] for a T-frame latent: the reference walks range(T) one frame per decoder call with
    first_chunk = (i == 0) (vae2_2.py:839-857); here frame 0 alone, then `group` frames per call."""
    return [(0, 1, True)] + [(i, min(T, i + group), False) for i in range(1, T, group)]


def encode_passes(T, group):
    """[(first_frame, end_frame, first_chunk)] for a T-frame video: the reference's chunks are frame 0, then 4 frames each for
    i = 1 .. (T-1)//4 (vae2_2.py:802-820; a ragged tail of < 4 frames is never encoded); here `group` of those chunks per call."""
    nchunk = 1 + (T - 1) // 4
    return [(0, 1, True)] + [(1 + 4 * (i - 1), 1 + 4 * (min(nchunk, i + group) - 1), False) for i in range(1, nchunk, group)]


def upfold_qualifies(cin, cout):
    """Does the engine's fold_upsample option run an upsample Resample's 3x3 convolution (cin -> cout) as four 2x2 phase convolutions?
    The only place the rule lives. It looks at the layer alone, never at the frame size or count of a call: a grouped pass and the
    one-latent walk take the same kernel. cout < 192 (the 192 -> 96 level) keeps conv_halo_n's folded-upsample instance: a 256-wide N tile
    would be 37 % full there."""
    return cin % 64 == 0 and cout >= 192


def live_tap_form(k, pad_t, T, has_cache, stride=(1, 1, 1)):
    """(k, pad_t, first_tap) a temporal convolution runs as under the engine's live_taps option. The only place the rule lives. A causal
    convolution with kt == 3, pt == 2 and stride 1 over ONE frame that has no cache entry yet reads the frames -2, -1, 0 for its only
    output frame; -2 and -1 are zeros, so the sum over dt = kt - 1 alone is the same number in real arithmetic: the call runs as the
    (1, kh, kw) convolution with pt = 0 on the K range of temporal tap first_tap = kt - 1. Everything else keeps today's call
    (first_tap = 0). The rule looks at the call's own frame count and cache, never at H, W, `group` or the length of the video."""
    kt, kh, kw = k
    if kt == 3 and pad_t == 2 and tuple(stride) == (1, 1, 1) and T == 1 and not has_cache:
        return (1, kh, kw), 0, kt - 1
    return (kt, kh, kw), pad_t, 0


def live_view_fits(k, cip):
    """May the live K range of a packed weight row be handed to the kernels as a VIEW (row stride unchanged)? A packed row holds
    K = kt kh kw cip elements ordered (dt, dh, dw, ci), zero padded to 64; the live slice starts at (kt - 1) kh kw cip and the
    dispatcher reads it up to its own padding to 64: legal only while that stays inside the row (the last row ends the buffer).
    True for cip = 32, 48, 64, 96, 128, 160, ...; False for cip = 8 and 16 (3x3x3), where _pack keeps a zero-padded copy instead."""
    kt, kh, kw = k
    return (kt - 1) * kh * kw * cip + _ru(kh * kw * cip, 64) <= _ru(kt * kh * kw * cip, 64)


_FOLD_TAPS = (((0,), (1, 2)), ((0, 1), (2,)))      # S(e, t): the 3x3 taps that phase parity e reads at 2x2 tap t


def fold_upsample_weight(w):
    """bf16-rounded Conv2d weight [co, ci, 3, 3] behind a nearest-2x upsample -> bf16 [4, co, 2, 2, ci]: the four 2x2 phase convolutions
    on the input-resolution image. Phase 2 e_h + e_w computes output (2a + e_h, 2b + e_w); its tap (th, tw) reads input
    (a + th - (1 - e_h), b + tw - (1 - e_w)) (zero outside) with the weight sum_{dh in S(e_h, th)} sum_{dw in S(e_w, tw)} w[co, ci, dh, dw],
    S(0, .) = ({0}, {1, 2}), S(1, .) = ({0, 1}, {2}); summed in fp32 in ascending (dh, dw), rounded once to bf16 (nearest even)."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise RuntimeError(f"fold_upsample_weight: expected a [co, ci, 3, 3] weight, got {tuple(w.shape)}")
    co, ci = w.shape[:2]
    w32 = w.float()
    out = torch.empty((4, co, 2, 2, ci), dtype=torch.float32, device=w.device)
    for eh in range(2):
        for ew in range(2):
            for th in range(2):
                for tw in range(2):
                    acc = None
                    for dh in _FOLD_TAPS[eh][th]:
                        for dw in _FOLD_TAPS[ew][tw]:
                            acc = w32[:, :, dh, dw] if acc is None else acc + w32[:, :, dh, dw]
                    out[2 * eh + ew, :, th, tw, :] = acc
    return out.to(torch.bfloat16)


class _Holder(nn.Module):
    """anonymous container; the tree of these reproduces the reference state_dict key names."""


def build_param_tree(shapes):
    root = _Holder()
    for key, shape in shapes.items():
        parts = key.split(".")
        mod = root
        for p in parts[:-1]:
            if not hasattr(mod, p):
                mod.add_module(p, _Holder())
            mod = getattr(mod, p)
        mod.register_parameter(parts[-1], nn.Parameter(torch.zeros(shape)))
    return root


class VaeEngine:
    def __init__(self, module, cfg):
        self.module = module
        self.cfg = cfg
        self._key = None
        self.P = None
        # reference chunks (latent frames in decode, 4-frame groups in encode) per pass after the first chunk; 1 = the reference's walk
        self.group = max(1, int(os.environ.get("YUME_VAE_GROUP", "8")))
        # r19 (env YUME_VAE_FP8=1, off by default): the ResidualBlock convolutions (residual.2 / residual.6, 3x3x3) whose input width is a
        # multiple of 128 run in e4m3 — the RMS_norm + SiLU launch in front of each emits OCP MX bytes (one E8M0 scale byte per position and
        # 32 channels, V.rmsnorm_silu_mx), the convolution takes them into the MFMA's scale operand (V.conv3d_cl_f8mx), weights are
        # quantised per output channel at pack time. About 10x the bf16 path's deviation on synthetic weights: a faster decode / encode
        # for preview and interactive use, to be judged on a real checkpoint. Selection looks at the layer only, never at the frame size or
        # count. Part of the pack key: toggling it repacks.
        self.fp8_conv = os.environ.get("YUME_VAE_FP8", "0") == "1"
        # r21 (env YUME_VAE_UPFOLD=1, off by default): the decoder's nearest-2x + Conv2d 3x3 of every upsample Resample that
        # upfold_qualifies runs as four 2x2 phase convolutions on the input-resolution image (V.conv_up2_fold; weights summed and rounded
        # to bf16 at pack time, fold_upsample_weight): 4 taps instead of 9. Not bit-equal to the 9-tap path (the summed weights are rounded
        # once more, 1.6-1.8e-3 rel-L2 per convolution). Independent of fp8_conv. Part of the pack key: toggling it repacks.
        self.fold_upsample = os.environ.get("YUME_VAE_UPFOLD", "0") == "1"
        # r24 (env YUME_VAE_LIVE_TAPS=1, off by default): the first pass of every encode / decode (one frame, an empty cache) runs its
        # 3x3x3 convolutions on the nine taps of dt = 2 alone — the 18 taps of the frames -2, -1 multiply zeros (live_tap_form). The same
        # value in real arithmetic; the fp32 sum can differ in its last bits where a K tile straddles taps. The weights are a view into
        # the packed rows, or a zero-padded copy packed beside them where the view would read past the row (live_view_fits: the
        # encoders' first convolution). Independent of fp8_conv and fold_upsample. Part of the pack key (the copies).
        self.live_taps = os.environ.get("YUME_VAE_LIVE_TAPS", "0") == "1"

    # ------------------------------------------------------------------ weights
    def _pack(self):
        sd = {k: v.detach() for k, v in self.module.state_dict().items()}
        dev = next(iter(sd.values())).device
        if dev.type != "cuda":
            raise RuntimeError("yume_amd VAE must live on the GPU ('cuda') — there is no CPU path")
        P = {}
        for k, w in sd.items():
            if k.endswith(".weight"):
                name = k[:-7]
                if w.dim() == 4:            # Conv2d -> kt = 1
                    w = w.unsqueeze(2)
                co, ci, kt, kh, kw = w.shape
                cip = _ru(ci, 8)
                cop = _ru(co, 4)
                wt = w.float().permute(0, 2, 3, 4, 1)                       # [co, kt, kh, kw, ci]
                if cip != ci:
                    wt = torch.cat([wt, wt.new_zeros(co, kt, kh, kw, cip - ci)], dim=-1)
                wt = wt.reshape(co, kt * kh * kw * cip)
                K = wt.shape[1]
                Kp = _ru(K, 64)
                full = torch.zeros(cop, Kp, dtype=torch.float32, device=dev)
                full[:co, :K] = wt
                b = torch.zeros(cop, dtype=torch.float32, device=dev)
                b[:co] = sd[name + ".bias"].float()
                P[name] = dict(w=full.to(torch.bfloat16).contiguous(), b=b, co=co, cop=cop, ci=ci, cip=cip, k=(kt, kh, kw))
                if self.live_taps and kt == 3 and not live_view_fits((kt, kh, kw), cip):
                    # the K range of dt = kt - 1 as rows of its own, zero padded to 64: a view would be read past the end of the row
                    Kl = kh * kw * cip
                    wl = torch.zeros(cop, _ru(Kl, 64), dtype=torch.bfloat16, device=dev)
                    wl[:, :Kl] = P[name]["w"][:, (kt - 1) * Kl:kt * Kl]
                    P[name]["wl"] = wl
                if self.fp8_conv and name.endswith((".residual.2", ".residual.6")) and ci % 128 == 0 and (kt, kh, kw) == (3, 3, 3):
                    # e4m3 bytes [cop, 27 ci] of the bf16 weights with one fp32 scale per output channel (amax / 448, 1 for a zero row)
                    wq = torch.empty((cop, K), dtype=torch.uint8, device=dev)
                    sw = torch.empty(cop, dtype=torch.float32, device=dev)
                    ops.quant_rows_e4m3(P[name]["w"][:, :K], wq, sw)
                    P[name].update(wq=wq, sw=sw)
                if (self.fold_upsample and name.startswith("decoder.") and name.endswith(".resample.1") and (kt, kh, kw) == (1, 3, 3)
                        and upfold_qualifies(ci, co)):
                    # the four 2x2 phase convolutions of nearest-2x + 3x3: bf16 [4, cop, 4 ci], K ordered (th, tw, ci)
                    wf = torch.zeros((4, cop, 4 * ci), dtype=torch.bfloat16, device=dev)
                    wf[:, :co] = fold_upsample_weight(w[:, :, 0].to(torch.bfloat16)).reshape(4, co, 4 * ci)
                    P[name]["wf"] = wf
            elif k.endswith(".gamma"):
                P[k] = w.float().reshape(-1).contiguous()
        self.P = P
        self.dev = dev
        self.zero = torch.zeros(64, dtype=torch.bfloat16, device=dev)

    def ensure_packed(self):
        key = tuple((p.data_ptr(), p._version) for p in self.module.parameters()) + (bool(self.fp8_conv), bool(self.fold_upsample), bool(self.live_taps))
        if key != self._key:
            self._pack()
            self._key = key

    # ------------------------------------------------------------------ primitives
    def _new(self, T, H, W, C):
        return torch.empty((T, H, W, C), dtype=torch.bfloat16, device=self.dev)

    def _update_cache(self, cache, name, x):
        """cache[name] <- last two frames of (previous cache ++ x); created zero-filled on first use."""
        if x.shape[0] >= 2:
            # no copy: the last two frames of this chunk's input ARE the next chunk's cache (x is never written again;
            # holding the view keeps it alive — 288 GB of HBM make that free)
            cache[name] = x[-2:]
            return
        c = cache.get(name)
        if c is None:
            c = torch.zeros((2,) + tuple(x.shape[1:]), dtype=x.dtype, device=self.dev)
        else:
            c = torch.stack((c[1], x[0]))      # [previous last frame, this frame] in fresh memory (c may be a view)
            cache[name] = c
            return
        c[1].copy_(x[0])
        cache[name] = c

    def _conv3(self, name, x, cache, add=None, norm=None):
        """CausalConv3d with a temporal kernel (3x3x3 or (3,1,1)), stride 1: reads cache[name], then updates it.
        norm: the name of an RMS_norm (+ SiLU) applied to the convolution's output inside the same C-ABI call (YUME_CONV_EPI_RMS_SILU)."""
        p = self.P[name]
        kt, kh, kw = p["k"]
        T, H, W, C = x.shape
        out = self._new(T, H, W, _ru(p["co"], 8))
        if out.shape[3] != p["cop"]:
            out.zero_()
        if norm is not None:
            if add is not None or out.shape[3] != p["cop"] or p["cop"] != p["co"]:
                raise RuntimeError("yume_amd.vae: the fused norm needs an unpadded channel row and no shortcut")
            epi, operand = V.EPI_RMS_SILU, self.P[norm + ".gamma"]
        else:
            epi, operand = (V.EPI_ADD if add is not None else V.EPI_BF16), add
        w, k, pt = p["w"], (kt, kh, kw), kt - 1
        if self.live_taps:
            k, pt, dt0 = live_tap_form(p["k"], kt - 1, T, cache.get(name) is not None)
            if dt0:
                # the K range of the live temporal tap: a view with the row stride of the packed rows, or the copy _pack kept
                w = p["wl"] if "wl" in p else p["w"][:, dt0 * kh * kw * p["cip"]:]
        V.conv3d_cl(x, cache.get(name), w, p["b"], p["cop"], k, (1, 1, 1), (pt, kh // 2, kw // 2), False,
                    out, epi, add=operand, zero_page=self.zero)
        self._update_cache(cache, name, x)
        return out

    def _conv1(self, name, x, add=None):
        """1x1x1 CausalConv3d / 1x1 Conv2d."""
        p = self.P[name]
        T, H, W, C = x.shape
        out = self._new(T, H, W, _ru(p["co"], 8))
        if out.shape[3] != p["cop"]:
            out.zero_()
        V.conv3d_cl(x, None, p["w"], p["b"], p["cop"], (1, 1, 1), (1, 1, 1), (0, 0, 0), False, out,
                    V.EPI_ADD if add is not None else V.EPI_BF16, add=add, zero_page=self.zero)
        return out

    def _norm(self, name, x, silu=True):
        out = torch.empty_like(x)
        return V.rmsnorm_silu(x, self.P[name + ".gamma"], silu, out)

    def _norm_mx(self, name, x):
        """RMS_norm + SiLU of x as OCP MX e4m3: (bytes [T,H,W,C], scale bytes [T,H,W,C/32])."""
        T, H, W, C = x.shape
        q = torch.empty((T, H, W, C), dtype=torch.uint8, device=self.dev)
        e = torch.empty((T, H, W, C // 32), dtype=torch.uint8, device=self.dev)
        return V.rmsnorm_silu_mx(x, self.P[name + ".gamma"], True, q, e)

    def _conv3_f8(self, name, qe, cache, add=None):
        """_conv3 for a convolution packed in e4m3: its input and its causal cache are (bytes, scale bytes) pairs, each half kept by the
        rules of _update_cache."""
        p = self.P[name]
        q, e = qe
        T, H, W, C = q.shape
        out = self._new(T, H, W, _ru(p["co"], 8))
        if out.shape[3] != p["cop"]:
            out.zero_()
        cq, ce = cache.get(name + "#q"), cache.get(name + "#e")
        wq, k = p["wq"], p["k"]
        if self.live_taps:
            k, _, dt0 = live_tap_form(p["k"], p["k"][0] - 1, T, cq is not None)
            if dt0:
                wq = p["wq"][:, dt0 * k[1] * k[2] * C:]      # e4m3 rows hold exactly K bytes: the live range ends the row, sw unchanged
        V.conv3d_cl_f8mx(q, e, None if cq is None else (cq, ce), wq, p["sw"], p["b"], p["cop"], k, out,
                         V.EPI_ADD if add is not None else V.EPI_BF16, add=add, zero_page=self.zero)
        self._update_cache(cache, name + "#q", q)
        self._update_cache(cache, name + "#e", e)
        return out

    def _res(self, name, x, cache):
        h = self._conv1(name + ".shortcut", x) if (name + ".shortcut") in self.P else x
        f2, f6 = "wq" in self.P[name + ".residual.2"], "wq" in self.P[name + ".residual.6"]
        if f2 or f6:
            # fp8_conv: each qualifying convolution reads the MX bytes its norm launch emitted; a block whose other convolution does not
            # qualify (Cin = in_dim for residual.2, out_dim for residual.6) keeps today's calls for that one
            if f2:
                y = self._conv3_f8(name + ".residual.2", self._norm_mx(name + ".residual.0", x), cache)
            else:
                y = self._conv3(name + ".residual.2", self._norm(name + ".residual.0", x), cache)
            if f6:
                return self._conv3_f8(name + ".residual.6", self._norm_mx(name + ".residual.3", y), cache, add=h)
            V.rmsnorm_silu(y, self.P[name + ".residual.3.gamma"], True, y)
            return self._conv3(name + ".residual.6", y, cache, add=h)
        # residual.3 (RMS_norm) + residual.4 (SiLU) ride in the epilogue of residual.2's call: conv -> norm -> SiLU is one C-ABI call
        # (fused in the kernel at the 96 / 160-channel levels, conv + in-place norm kernel elsewhere; include/yume_hip.h)
        yn = self._conv3(name + ".residual.2", self._norm(name + ".residual.0", x), cache, norm=name + ".residual.3")
        return self._conv3(name + ".residual.6", yn, cache, add=h)

    def _attn(self, name, x):
        """AttentionBlock: per frame, one head of width C over the H*W positions (two GEMMs + a row softmax)."""
        T, H, W, C = x.shape
        hw = H * W
        if C % 64:
            raise RuntimeError("yume_amd VAE attention needs C % 64 == 0")
        pq = self.P[name + ".to_qkv"]
        xn = self._norm(name + ".norm", x, silu=False)
        out = torch.empty_like(x)
        hwp, hw4 = _ru(hw, 64), _ru(hw, 4)     # K padding of the P.V product; N padding of the score GEMM (zero key rows)
        qk = torch.zeros((hw4, 2 * C), dtype=torch.bfloat16, device=self.dev)
        vt = torch.zeros((C, hwp), dtype=torch.bfloat16, device=self.dev)
        s = torch.empty((hw, hw4), dtype=torch.float32, device=self.dev)
        pm = torch.empty((hw, hwp), dtype=torch.bfloat16, device=self.dev)
        o = self._new(1, H, W, C)
        for t in range(T):
            ops.gemm_bf16(xn[t].view(hw, C), pq["w"], pq["b"], qk[:hw], ops.EPI_BF16_SPLITT, out_t=vt, n_split=2 * C)
            ops.gemm_bf16(qk[:hw, :C], qk[:, C:], None, s, ops.EPI_F32)
            V.softmax_rows(s, hw, 1.0 / math.sqrt(C), pm)
            ops.gemm_bf16(pm, vt, None, o.view(hw, C), ops.EPI_BF16)
            pp = self.P[name + ".proj"]
            V.conv3d_cl(o, None, pp["w"], pp["b"], pp["cop"], (1, 1, 1), (1, 1, 1), (0, 0, 0), False, out[t:t + 1],
                        V.EPI_ADD, add=x[t:t + 1], zero_page=self.zero)
        return out

    def _upsample(self, name, x, mode, cache, first_chunk):
        T, H, W, C = x.shape
        if mode == "upsample3d" and not first_chunk:
            tc = name + ".time_conv"
            p = self.P[tc]
            y = self._new(2 * T, H, W, C)
            V.conv3d_cl(x, cache.get(tc), p["w"], p["b"], p["cop"], (3, 1, 1), (1, 1, 1), (2, 0, 0), False, y, V.EPI_TSPLIT,
                        zero_page=self.zero)
            self._update_cache(cache, tc, x)
            x, T = y, 2 * T
        p = self.P[name + ".resample.1"]
        out = self._new(T, 2 * H, 2 * W, _ru(p["co"], 8))
        if "wf" in p:
            if out.shape[3] != p["cop"]:
                out.zero_()
            return V.conv_up2_fold(x, p["wf"], p["b"], p["cop"], out)
        V.conv3d_cl(x, None, p["w"], p["b"], p["cop"], (1, 3, 3), (1, 1, 1), (0, 1, 1), True, out, V.EPI_BF16, zero_page=self.zero)
        return out

    def _downsample(self, name, x, mode, cache, first_chunk):
        T, H, W, C = x.shape
        p = self.P[name + ".resample.1"]
        Ho, Wo = (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1
        y = self._new(T, Ho, Wo, C)
        V.conv3d_cl(x, None, p["w"], p["b"], p["cop"], (1, 3, 3), (1, 2, 2), (0, 0, 0), False, y, V.EPI_BF16, zero_page=self.zero)
        if mode == "downsample3d":
            tc = name + ".time_conv"
            if first_chunk:
                self._update_cache(cache, tc, y)          # pass through; remember the frame
                return y
            p = self.P[tc]
            To = (T + 1 - 3) // 2 + 1
            z = self._new(To, Ho, Wo, C)
            V.conv3d_cl(y, cache.get(tc), p["w"], p["b"], p["cop"], (3, 1, 1), (2, 1, 1), (1, 0, 0), False, z, V.EPI_BF16,
                        zero_page=self.zero)
            self._update_cache(cache, tc, y)
            return z
        return y

    def _dims(self, enc):
        m = self.cfg["dim_mult"]
        return [self.cfg["dim"] * u for u in [1] + m] if enc else [self.cfg["dec_dim"] * u for u in [m[-1]] + m[::-1]]

    # ------------------------------------------------------------------ passes
    def _encoder_pass(self, x, cache, first_chunk):
        cfg = self.cfg
        v22 = cfg["version"] == "2.2"
        dims, nres, tds = self._dims(True), cfg["num_res_blocks"], cfg["temperal_downsample"]
        x = self._conv3("encoder.conv1", x, cache)
        li = 0
        for i, (cin, cout) in enumerate(zip(dims[:-1], dims[1:])):
            down = i != len(cfg["dim_mult"]) - 1
            t_down = tds[i] if i < len(tds) else False
            mode = "downsample3d" if t_down else "downsample2d"
            if v22:
                x0, base = x, f"encoder.downsamples.{i}.downsamples"
                for j in range(nres):
                    x = self._res(f"{base}.{j}", x, cache)
                if down:
                    x = self._downsample(f"{base}.{nres}", x, mode, cache, first_chunk)
                V.avgdown_add(x0, x, 2 if t_down else 1, 2 if down else 1)
            else:
                for j in range(nres):
                    x = self._res(f"encoder.downsamples.{li}", x, cache)
                    li += 1
                if down:
                    x = self._downsample(f"encoder.downsamples.{li}", x, mode, cache, first_chunk)
                    li += 1
        x = self._res("encoder.middle.0", x, cache)
        x = self._attn("encoder.middle.1", x)
        x = self._res("encoder.middle.2", x, cache)
        return self._conv3("encoder.head.2", self._norm("encoder.head.0", x), cache)

    def _decoder_pass(self, x, cache, first_chunk):
        cfg = self.cfg
        v22 = cfg["version"] == "2.2"
        dims, nres = self._dims(False), cfg["num_res_blocks"]
        tus = cfg["temperal_downsample"][::-1]
        x = self._conv3("decoder.conv1", x, cache)
        x = self._res("decoder.middle.0", x, cache)
        x = self._attn("decoder.middle.1", x)
        x = self._res("decoder.middle.2", x, cache)
        li = 0
        for i, (cin, cout) in enumerate(zip(dims[:-1], dims[1:])):
            up = i != len(cfg["dim_mult"]) - 1
            t_up = tus[i] if i < len(tus) else False
            mode = "upsample3d" if t_up else "upsample2d"
            if v22:
                x0, base = x, f"decoder.upsamples.{i}.upsamples"
                for j in range(nres + 1):
                    x = self._res(f"{base}.{j}", x, cache)
                if up:
                    x = self._upsample(f"{base}.{nres + 1}", x, mode, cache, first_chunk)
                    ft = 2 if t_up else 1
                    V.dupup_add(x0, x, ft, 2, (ft - 1) if first_chunk else 0)
            else:
                for j in range(nres + 1):
                    x = self._res(f"decoder.upsamples.{li}", x, cache)
                    li += 1
                if up:
                    x = self._upsample(f"decoder.upsamples.{li}", x, mode, cache, first_chunk)
                    li += 1
        return self._conv3("decoder.head.2", self._norm("decoder.head.0", x), cache)

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def _vec(self, v, n):
        if v is None:
            return None
        if not isinstance(v, torch.Tensor):
            v = torch.full((n,), float(v))
        return v.to(device=self.dev, dtype=torch.float32).reshape(-1).expand(n).contiguous()

    def encode(self, video, sub=None, mul=None):
        """video [3, T, H, W] (fp32|bf16, [-1,1]) -> latent fp32 [z, 1+(T-1)//4, H/s, W/s] = (mu - sub) * mul —
        WanVAE_.encode (sub = mean, mul = 1/std)."""
        self.ensure_packed()
        cfg = self.cfg
        ps, z = cfg["patch"], cfg["z_dim"]
        v = video.to(self.dev)
        if v.dtype not in (torch.float32, torch.bfloat16):
            v = v.float()
        v = v.contiguous()
        C, T, H, W = v.shape
        cpad = _ru(C * ps * ps, 8)
        x = self._new(T, H // ps, W // ps, cpad)
        V.pack_input(v, ps, None, None, x)
        cache, outs = {}, []
        for a, b, first in encode_passes(T, self.group):
            outs.append(self._encoder_pass(x[a:b], cache, first))
        out = torch.cat(outs, dim=0)                                     # [T', h, w, 2z(pad)]
        mu = self._conv1("conv1", out)
        Tl, h, w, _ = mu.shape
        res = torch.empty((z, Tl, h, w), dtype=torch.float32, device=self.dev)
        if (sub is None) != (mul is None):
            sub, mul = (0.0 if sub is None else sub), (1.0 if mul is None else mul)
        V.unpack_output(mu, z, 1, self._vec(sub, z), self._vec(mul, z), 0.0, 0.0, res)
        return res

    @torch.no_grad()
    def decode(self, zlat, mul=None, add=None, clamp=True):
        """latent [z, T, h, w] -> video fp32 [3, 1+4(T-1), H, W] — WanVAE_.decode on z*mul + add (mul = std,
        add = mean), clamped to [-1,1] like the Wan*VAE wrappers when clamp."""
        self.ensure_packed()
        cfg = self.cfg
        ps, z = cfg["patch"], cfg["z_dim"]
        zl = zlat.to(self.dev)
        if zl.dtype not in (torch.float32, torch.bfloat16):
            zl = zl.float()
        zl = zl.contiguous()
        C, T, h, w = zl.shape
        if C != z:
            raise RuntimeError(f"latent has {C} channels, VAE z_dim is {z}")
        x = self._new(T, h, w, _ru(z, 8))
        if (mul is None) != (add is None):
            mul, add = (1.0 if mul is None else mul), (0.0 if add is None else add)
        V.pack_input(zl, 1, self._vec(mul, z), self._vec(add, z), x)
        x = self._conv1("conv2", x)
        cache, outs = {}, []
        for a, b, first in decode_passes(T, self.group):
            outs.append(self._decoder_pass(x[a:b], cache, first))
        out = torch.cat(outs, dim=0)                                     # [T_out, H/ps, W/ps, in_ch(pad)]
        To, Ho, Wo, _ = out.shape
        cv = cfg["in_ch"]
        res = torch.empty((cv // (ps * ps), To, Ho * ps, Wo * ps), dtype=torch.float32, device=self.dev)
        V.unpack_output(out, cv, ps, None, None, -1.0 if clamp else 0.0, 1.0 if clamp else 0.0, res)
        return res
