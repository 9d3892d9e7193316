"""Tensor-level wrappers over the VAE part of the C-ABI (include/yume_hip.h, "Causal 3D VAE" section).
Activations are bf16 channels-last tensors [T, H, W, C] (contiguous, C % 8 == 0)."""
import torch

from . import _lib
from .ops import _dev, _ptr, _stream, ensure_counters

EPI_BF16, EPI_F32, EPI_ADD, EPI_TSPLIT, EPI_RMS_SILU = 0, 2, 16, 17, 18


def _cl(t, name):
    _dev(t, name, torch.bfloat16)
    if t.dim() != 4 or not t.is_contiguous():
        raise RuntimeError(f"yume_amd.vae: {name} must be a contiguous bf16 [T,H,W,C] tensor, got {tuple(t.shape)}")
    return t


def conv3d_cl(x, cache, w, bias, cout, k, stride, pad, ups, out, epi=EPI_BF16, add=None, zero_page=None, cin=None):
    """out[To,Ho,Wo,>=cout] = conv(x [Tin,Hin,Win,C]) — geometry: k=(kt,kh,kw), stride=(st,sh,sw), pad=(pt,ph,pw)."""
    lib = _lib.load()
    _cl(x, "x")
    _cl(out, "out")
    ensure_counters(x.device)
    Tin, Hin, Win, C = x.shape
    To, Ho, Wo, Cl = out.shape
    if epi == EPI_TSPLIT:
        To = To // 2          # `out` holds the 2*To interleaved frames with cout/2 channels
    if cache is not None:
        _cl(cache, "cache")
        if tuple(cache.shape) != (2, Hin, Win, C):
            raise RuntimeError("yume_amd.vae: cache must be [2,Hin,Win,C]")
    ldadd = 0
    if epi == EPI_RMS_SILU:
        # `add` carries the fp32 gamma of the RMS_norm fused behind the convolution (include/yume_hip.h)
        _dev(add, "gamma", torch.float32)
        if add.numel() < cout or not add.is_contiguous():
            raise RuntimeError("yume_amd.vae: gamma must be a contiguous fp32 vector of >= cout elements")
    elif add is not None:
        _cl(add, "add")
        ldadd = add.shape[3]
    rc = lib.yume_conv3d_cl(x.data_ptr(), _ptr(cache), C, Tin, Hin, Win, cin if cin is not None else C, w.data_ptr(),
                            w.stride(0), _ptr(bias), cout, k[0], k[1], k[2], stride[0], stride[1], stride[2], pad[0],
                            pad[1], pad[2], 1 if ups else 0, To, Ho, Wo, epi, out.data_ptr(), Cl,
                            _ptr(add), ldadd, zero_page.data_ptr(), _stream())
    _lib.check(rc, "yume_conv3d_cl")
    return out


def rmsnorm_silu(x, gamma, silu, out, beta=None):
    lib = _lib.load()
    _cl(x, "x")
    _cl(out, "out")
    C = x.shape[3]
    M = x.numel() // C
    rc = lib.yume_vae_rmsnorm_silu(x.data_ptr(), C, M, C, gamma.data_ptr(), _ptr(beta), 1 if silu else 0, out.data_ptr(),
                                   C, _stream())
    _lib.check(rc, "yume_vae_rmsnorm_silu")
    return out


def _cl8(t, name):
    _dev(t, name, torch.uint8)
    if t.dim() != 4 or not t.is_contiguous():
        raise RuntimeError(f"yume_amd.vae: {name} must be a contiguous uint8 [T,H,W,C] tensor, got {tuple(t.shape)}")
    return t


def rmsnorm_silu_mx(x, gamma, silu, q, e, beta=None):
    """(q u8 [T,H,W,C], e u8 [T,H,W,C/32]) = the MX e4m3 quantisation of rmsnorm_silu(x), in one kernel, bit for bit (yume_hip.h)."""
    lib = _lib.load()
    _cl(x, "x")
    _cl8(q, "q")
    _cl8(e, "e")
    C = x.shape[3]
    M = x.numel() // C
    if tuple(q.shape) != tuple(x.shape) or tuple(e.shape) != tuple(x.shape[:3]) + (C // 32,) or C % 32:
        raise RuntimeError(f"yume_amd.vae.rmsnorm_silu_mx: x {tuple(x.shape)}, q {tuple(q.shape)}, e {tuple(e.shape)} do not fit")
    rc = lib.yume_vae_rmsnorm_silu_mx(x.data_ptr(), C, M, C, gamma.data_ptr(), _ptr(beta), 1 if silu else 0, q.data_ptr(), C,
                                      e.data_ptr(), C // 32, _stream())
    _lib.check(rc, "yume_vae_rmsnorm_silu_mx")
    return q, e


def conv3d_cl_f8mx(xq, xe, cache, wq, sw, bias, cout, k, out, epi=EPI_BF16, add=None, zero_page=None):
    """out[T,H,W,>=cout] = the stride-1 causal convolution of MX e4m3 activations (xq u8 [T,H,W,C], xe u8 [T,H,W,C/32]) with e4m3
    weights wq u8 [cout, >= kt*kh*kw*C] and their per-channel scales sw; cache = None or the (bytes, scales) pair of the previous chunk's
    last two frames (yume_hip.h)."""
    lib = _lib.load()
    _cl8(xq, "xq")
    _cl8(xe, "xe")
    _dev(wq, "wq", torch.uint8)
    _dev(sw, "sw", torch.float32)
    T, H, W, C = xq.shape
    if tuple(xe.shape[:3]) != (T, H, W) or tuple(out.shape[:3]) != (T, H, W) or not out.is_contiguous():
        raise RuntimeError("yume_amd.vae.conv3d_cl_f8mx: xq, xe and out must share [T,H,W]")
    _dev(out, "out", torch.float32 if epi == EPI_F32 else torch.bfloat16)
    cq = ce = None
    if cache is not None:
        cq, ce = cache
        _cl8(cq, "cacheq")
        _cl8(ce, "cachee")
        if tuple(cq.shape) != (2, H, W, C) or tuple(ce.shape) != (2, H, W, xe.shape[3]):
            raise RuntimeError("yume_amd.vae.conv3d_cl_f8mx: the cache pair must be [2,H,W,C] and [2,H,W,C/32]")
    ldadd = 0
    if add is not None:
        _cl(add, "add")
        ldadd = add.shape[3]
    rc = lib.yume_conv3d_cl_f8mx(xq.data_ptr(), xe.data_ptr(), _ptr(cq), _ptr(ce), C, xe.shape[3], T, H, W, C, wq.data_ptr(), wq.stride(0),
                                 sw.data_ptr(), _ptr(bias), cout, k[0], k[1], k[2], 1, 1, 1, k[0] - 1, k[1] // 2, k[2] // 2, 0, T, H, W, epi,
                                 out.data_ptr(), out.shape[3], _ptr(add), ldadd, zero_page.data_ptr(), _stream())
    _lib.check(rc, "yume_conv3d_cl_f8mx")
    return out


def conv_up2_fold(x, wf, bias, cout, out, cin=None):
    """out[T,2H,2W,>=cout] = Conv2d 3x3 (pad 1) of the nearest-2x upsampled x [T,H,W,C] as four 2x2 phase convolutions: wf bf16
    [4, cout, >= 4*cin], phase 2 e_h + e_w, K ordered (th, tw, ci) (yume_amd.vae.fold_upsample_weight; yume_hip.h)."""
    lib = _lib.load()
    _cl(x, "x")
    _cl(out, "out")
    _dev(wf, "wf", torch.bfloat16)
    T, H, W, C = x.shape
    if tuple(out.shape[:3]) != (T, 2 * H, 2 * W):
        raise RuntimeError(f"yume_amd.vae.conv_up2_fold: out {tuple(out.shape)} is not the 2x upsample of x {tuple(x.shape)}")
    if wf.dim() != 3 or wf.shape[0] != 4 or wf.shape[1] != cout or not wf.is_contiguous():
        raise RuntimeError(f"yume_amd.vae.conv_up2_fold: wf must be a contiguous [4, cout, >= 4*cin] tensor, got {tuple(wf.shape)}")
    rc = lib.yume_conv_up2_fold(x.data_ptr(), C, T, H, W, cin if cin is not None else C, wf.data_ptr(), wf.shape[2], _ptr(bias), cout,
                                out.data_ptr(), out.shape[3], _stream())
    _lib.check(rc, "yume_conv_up2_fold")
    return out


def dupup_add(x, y, ft, fs, toff):
    lib = _lib.load()
    _cl(x, "x")
    _cl(y, "y")
    Tin, Hin, Win, Cin = x.shape
    To, Ho, Wo, Cout = y.shape
    if (Ho, Wo) != (Hin * fs, Win * fs):
        raise RuntimeError("yume_amd.vae.dupup_add: spatial shape mismatch")
    rc = lib.yume_vae_dupup_add(x.data_ptr(), Cin, Tin, Hin, Win, Cin, y.data_ptr(), Cout, To, Cout, ft, fs, toff, _stream())
    _lib.check(rc, "yume_vae_dupup_add")
    return y


def avgdown_add(x, y, ft, fs):
    lib = _lib.load()
    _cl(x, "x")
    _cl(y, "y")
    Tin, Hin, Win, Cin = x.shape
    To, Ho, Wo, Cout = y.shape
    padt = (ft - Tin % ft) % ft
    if (To, Ho, Wo) != ((Tin + padt) // ft, Hin // fs, Win // fs):
        raise RuntimeError(f"yume_amd.vae.avgdown_add: shape mismatch {tuple(x.shape)} -> {tuple(y.shape)}")
    rc = lib.yume_vae_avgdown_add(x.data_ptr(), Cin, Tin, Hin, Win, Cin, y.data_ptr(), Cout, Cout, ft, fs, _stream())
    _lib.check(rc, "yume_vae_avgdown_add")
    return y


def softmax_rows(s, n, scale, p):
    lib = _lib.load()
    _dev(s, "s", torch.float32)
    _dev(p, "p", torch.bfloat16)
    rc = lib.yume_softmax_rows(s.data_ptr(), s.stride(0), s.shape[0], n, scale, p.data_ptr(), p.stride(0), _stream())
    _lib.check(rc, "yume_softmax_rows")
    return p


def pack_input(x, ps, mul, add, out):
    """x fp32|bf16 [C,T,H,W] -> out bf16 [T,H/ps,W/ps,Cpad]."""
    lib = _lib.load()
    _dev(x, "x")
    if x.dtype not in (torch.float32, torch.bfloat16) or not x.is_contiguous() or x.dim() != 4:
        raise RuntimeError("yume_amd.vae.pack_input: x must be contiguous fp32|bf16 [C,T,H,W]")
    C, T, H, W = x.shape
    _cl(out, "out")
    rc = lib.yume_vae_pack_input(x.data_ptr(), 1 if x.dtype == torch.bfloat16 else 0, C, T, H, W, ps, _ptr(mul), _ptr(add),
                                 out.data_ptr(), out.shape[3], _stream())
    _lib.check(rc, "yume_vae_pack_input")
    return out


def unpack_output(x, cv, ps, sub, mul, lo, hi, out):
    """x bf16 [T,H,W,ld] (first cv channels) -> out fp32 [cv/ps^2, T, H*ps, W*ps]."""
    lib = _lib.load()
    _cl(x, "x")
    _dev(out, "out", torch.float32)
    T, H, W, ld = x.shape
    rc = lib.yume_vae_unpack_output(x.data_ptr(), ld, T, H, W, cv, ps, _ptr(sub), _ptr(mul), lo, hi, out.data_ptr(), _stream())
    _lib.check(rc, "yume_vae_unpack_output")
    return out
