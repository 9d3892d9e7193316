"""Tensor-level wrappers over the C-ABI (include/yume_hip.h).

torch is used for device memory and the current HIP stream only: every function here validates
its tensors, passes raw device pointers + sizes to libyume_hip.so and raises RuntimeError on failure.
"""
import math
import os

import torch

from . import _lib

EPI_BF16, EPI_BF16_GELU, EPI_F32, EPI_RESID, EPI_BF16_SPLITT, EPI_BF16_GELU_ERF, EPI_BF16_GEGLU = 0, 1, 2, 3, 4, 5, 6


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t, name, dtype=None):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"yume_amd: {name} must be a device ('cuda') tensor — this path has no CPU fallback")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"yume_amd: {name} must be {dtype}, got {t.dtype}")
    return t


def _rows(t, name):
    """2-D view parameters (ptr, ld) of a tensor whose last dim is contiguous."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise RuntimeError(f"yume_amd: {name} must be 2-D with a contiguous last dim, got shape {tuple(t.shape)} stride {t.stride()}")
    return t.data_ptr(), t.stride(0)


def _ptr(t):
    return t.data_ptr() if t is not None else None


_counters = {}
_DEBUG_COUNTERS = os.environ.get("YUME_DEBUG_COUNTERS", "0") == "1"


def ensure_counters(device):
    """Register (once per device) the caller-owned ticket-counter workspace of include/yume_hip.h (yume_counter_workspace_init): kernels
    that hand out work by ticket — long convolutions' tails, the persistent attention kernel — draw their counters from it; the library
    itself allocates nothing. The tensor lives for the life of the process.
    The zeroing is enqueued on the current stream and the DEVICE is synchronised before the workspace counts as registered: the first
    ticketed launch may come from any stream. Inside a hipGraph capture the zeroing would be recorded, not executed — refused by name
    (call yume_amd.ops.ensure_counters(device) once before capturing). YUME_DEBUG_COUNTERS=1: every call checks that the sets read zero
    (every ticketed kernel puts its zeros back; a dirty set means a launch was killed half way)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    t = _counters.get(idx)
    if t is None:
        with torch.cuda.device(idx):                       # (the capture state of THAT device's current stream)
            capturing = torch.cuda.is_current_stream_capturing()
        if capturing:
            raise RuntimeError("yume_amd: the ticket-counter workspace must be registered before a stream capture begins "
                               "(call yume_amd.ops.ensure_counters(device) once outside the capture)")
        lib = _lib.load()
        n = int(lib.yume_counter_workspace_bytes())
        with torch.cuda.device(idx):
            t = torch.zeros(n // 4, dtype=torch.int32, device=torch.device("cuda", idx))
            _lib.check(lib.yume_counter_workspace_init(t.data_ptr(), n, _stream()), "yume_counter_workspace_init")
            torch.cuda.synchronize(idx)
        _counters[idx] = t
    elif _DEBUG_COUNTERS and not torch.cuda.is_current_stream_capturing():
        torch.cuda.synchronize(idx)
        if int(t.abs().max()) != 0:
            raise RuntimeError("yume_amd: the ticket-counter workspace is not zero between launches (YUME_DEBUG_COUNTERS=1)")
    return t


def adaln_modulate(x, mul, add, tab_stride, row_idx, add_one, out, out_kind=0, eps=1e-6):
    """out = LN(x) * (mul[row] + add_one) + add[row]; x fp32 [T,C]; mul/add fp32 table views (first row)."""
    lib = _lib.load()
    _dev(x, "x", torch.float32)
    xp, ldx = _rows(x, "x")
    T, C = x.shape
    op, ldo = _rows(out, "out")
    rc = lib.yume_adaln_modulate(xp, ldx, T, C, eps, mul.data_ptr(), add.data_ptr(), tab_stride, _ptr(row_idx),
                                 1 if add_one else 0, op, ldo, out_kind, _stream())
    _lib.check(rc, "yume_adaln_modulate")
    return out


def adaln_modulate_e4m3(x, mul, add, tab_stride, row_idx, add_one, q, scale, eps=1e-6):
    """q u8 [T, C], scale fp32 [T] = quant_rows_e4m3(adaln_modulate(x, ..., out bf16)) in one kernel, bit for bit (yume_hip.h)."""
    lib = _lib.load()
    _dev(x, "x", torch.float32)
    _dev(q, "q", torch.uint8)
    _dev(scale, "scale", torch.float32)
    xp, ldx = _rows(x, "x")
    qp, ldq = _rows(q, "q")
    T, C = x.shape
    if tuple(q.shape) != (T, C) or scale.dim() != 1 or scale.numel() != T or not scale.is_contiguous():
        raise RuntimeError(f"yume_amd.adaln_modulate_e4m3: x {tuple(x.shape)}, q {tuple(q.shape)}, scale {tuple(scale.shape)} do not fit")
    rc = lib.yume_adaln_modulate_e4m3(xp, ldx, T, C, eps, mul.data_ptr(), add.data_ptr(), tab_stride, _ptr(row_idx),
                                      1 if add_one else 0, qp, ldq, scale.data_ptr(), _stream())
    _lib.check(rc, "yume_adaln_modulate_e4m3")
    return q, scale


def rmsnorm_f32(x, w, out, eps=1e-6):
    """out bf16 [T, C] = x * rsqrt(mean(x^2) + eps) * w (T5LayerNorm: no mean subtraction, no shift); x fp32 [T, C], w fp32 [C]."""
    lib = _lib.load()
    _dev(x, "x", torch.float32)
    _dev(w, "w", torch.float32)
    _dev(out, "out", torch.bfloat16)
    xp, ldx = _rows(x, "x")
    op, ldo = _rows(out, "out")
    T, C = x.shape
    if tuple(out.shape) != (T, C) or w.numel() != C or not w.is_contiguous():
        raise RuntimeError(f"yume_amd.rmsnorm_f32: x {tuple(x.shape)}, w {tuple(w.shape)}, out {tuple(out.shape)} do not fit")
    rc = lib.yume_rmsnorm_f32(xp, ldx, T, C, eps, w.data_ptr(), op, ldo, _stream())
    _lib.check(rc, "yume_rmsnorm_f32")
    return out


def softmax_bias_rows(S, bias, P, n):
    """P[h, i, :n] = softmax_j(S[h, i, j] + bias[h, j - i + n - 1]), P[h, i, n:] = 0 (the T5 attention rows, no scaling). S fp32 [H, n, >= n],
    bias fp32 [H, >= 2n - 1], P bf16 [H, n, .] whose row stride ldp = P.stride(1), n <= ldp <= 1024, is zeroed up to; the last dim of each contiguous."""
    lib = _lib.load()
    _dev(S, "S", torch.float32)
    _dev(bias, "bias", torch.float32)
    _dev(P, "P", torch.bfloat16)
    if S.dim() != 3 or P.dim() != 3 or bias.dim() != 2 or S.stride(2) != 1 or P.stride(2) != 1 or bias.stride(1) != 1:
        raise RuntimeError("yume_amd.softmax_bias_rows: S and P must be 3-D, bias 2-D, each with a contiguous last dim")
    H = S.shape[0]
    if S.shape[1] != n or P.shape[:2] != (H, n) or bias.shape[0] != H:
        raise RuntimeError(f"yume_amd.softmax_bias_rows: S {tuple(S.shape)}, bias {tuple(bias.shape)}, P {tuple(P.shape)} do not fit n={n}")
    rc = lib.yume_softmax_bias_rows(S.data_ptr(), S.stride(1), S.stride(0), H, n, bias.data_ptr(), bias.stride(0), P.data_ptr(), P.stride(1), P.stride(0), _stream())
    _lib.check(rc, "yume_softmax_bias_rows")
    return P


# scratch of the GEMM's stream-K tail (yume_gemm_bf16_ws): one zero-initialised buffer per (device, stream) — launches sharing it are ordered
_gemm_ws = {}


def _gemm_workspace(t):
    key = _ws_key(t)
    ws = _gemm_ws.get(key)
    if ws is None:
        n = int(_lib.load().yume_gemm_workspace_bytes())
        ws = _gemm_ws[key] = torch.zeros(n, dtype=torch.uint8, device=t.device)
    return ws


def gemm_stream_k_error(device=None):
    """True if a stream-K finisher of any GEMM on `device` timed out waiting for a partial tile (the error word of the scratch)."""
    bad = False
    for (idx, _), ws in _gemm_ws.items():
        if device is None or torch.device(device).index in (None, idx):
            bad = bad or bool(ws[-64:].any().item())
    return bad


def gemm_bf16(a, w, bias, out, epi=EPI_BF16, gate=None, gate_stride=0, row_idx=None, out_t=None, n_split=0,
              variant=0):
    """acc = a @ w.T (a bf16 [M,K], w bf16 [N,K]); epilogue selected by `epi` (see yume_hip.h)."""
    lib = _lib.load()
    _dev(a, "a", torch.bfloat16)
    _dev(w, "w", torch.bfloat16)
    ap, lda = _rows(a, "a")
    wp, ldw = _rows(w, "w")
    M, K = a.shape
    N, K2 = w.shape
    if K != K2:
        raise RuntimeError(f"yume_amd.gemm_bf16: K mismatch {K} vs {K2}")
    op, ldo = _rows(out, "out")
    tp, ldt = (None, 0)
    if out_t is not None:
        tp, ldt = _rows(out_t, "out_t")
    # the scratch is handed over where the split-K plan can take the shape at all (big launches of the automatic variant). Under a stream
    # capture the first call on the capture stream allocates and zero-fills it inside the capture (the fill is replayed with the graph)
    ws = _gemm_workspace(a) if (variant == 0 and M * N >= 256 * 256 * 256) else None
    rc = lib.yume_gemm_bf16_ws(ap, lda, wp, ldw, _ptr(bias), M, N, K, epi, op, ldo, _ptr(gate), gate_stride,
                               _ptr(row_idx), tp, ldt, n_split, variant, _ptr(ws), ws.numel() if ws is not None else 0, _stream())
    _lib.check(rc, "yume_gemm_bf16")
    return out


def quant_rows_e4m3(x, q, scale):
    """q u8 [R, K] = e4m3(x / scale[r]) with scale[r] = max|x[r]| / 448 (1 for a zero row); x bf16 [R, K], scale fp32 [R] (yume_hip.h)."""
    lib = _lib.load()
    _dev(x, "x", torch.bfloat16)
    _dev(q, "q", torch.uint8)
    _dev(scale, "scale", torch.float32)
    xp, ldx = _rows(x, "x")
    qp, ldq = _rows(q, "q")
    R, K = x.shape
    if tuple(q.shape) != (R, K) or scale.dim() != 1 or scale.numel() != R or not scale.is_contiguous():
        raise RuntimeError(f"yume_amd.quant_rows_e4m3: x {tuple(x.shape)}, q {tuple(q.shape)}, scale {tuple(scale.shape)} do not fit")
    rc = lib.yume_quant_rows_e4m3(xp, ldx, R, K, qp, ldq, scale.data_ptr(), _stream())
    _lib.check(rc, "yume_quant_rows_e4m3")
    return q, scale


def gemm_f8(aq, sa, wq, sw, bias, out, epi=EPI_BF16, gate=None, gate_stride=0, row_idx=None):
    """acc = aq @ wq.T (e4m3 bytes: aq u8 [M,K], wq u8 [N,K]); y = acc * sa[m] * sw[n] + bias; epilogue `epi` as gemm_bf16 (BF16, GELU, F32, RESID)."""
    lib = _lib.load()
    _dev(aq, "aq", torch.uint8)
    _dev(wq, "wq", torch.uint8)
    _dev(sa, "sa", torch.float32)
    _dev(sw, "sw", torch.float32)
    ap, lda = _rows(aq, "aq")
    wp, ldw = _rows(wq, "wq")
    M, K = aq.shape
    N, K2 = wq.shape
    if K != K2:
        raise RuntimeError(f"yume_amd.gemm_f8: K mismatch {K} vs {K2}")
    if sa.dim() != 1 or sa.numel() != M or not sa.is_contiguous() or sw.dim() != 1 or sw.numel() != N or not sw.is_contiguous():
        raise RuntimeError(f"yume_amd.gemm_f8: scales sa {tuple(sa.shape)}, sw {tuple(sw.shape)} do not fit M={M}, N={N}")
    op, ldo = _rows(out, "out")
    rc = lib.yume_gemm_f8(ap, lda, sa.data_ptr(), wp, ldw, sw.data_ptr(), _ptr(bias), M, N, K, epi, op, ldo, _ptr(gate), gate_stride,
                          _ptr(row_idx), _stream())
    _lib.check(rc, "yume_gemm_f8")
    return out


def gemm_f8_splitt(aq, sa, wq, sw, bias, out, out_t, n_split):
    """gemm_f8's sum and scales with the QKV epilogue: columns n < n_split bf16 row-major into out [M, >= n_split], columns n >= n_split as
    the K-major V^T image out_t[n - n_split, m] (bf16 [>= N - n_split, ldt >= M]); n_split % 256 == 0 (yume_hip.h)."""
    lib = _lib.load()
    _dev(aq, "aq", torch.uint8)
    _dev(wq, "wq", torch.uint8)
    _dev(sa, "sa", torch.float32)
    _dev(sw, "sw", torch.float32)
    ap, lda = _rows(aq, "aq")
    wp, ldw = _rows(wq, "wq")
    M, K = aq.shape
    N, K2 = wq.shape
    if K != K2:
        raise RuntimeError(f"yume_amd.gemm_f8_splitt: K mismatch {K} vs {K2}")
    if sa.dim() != 1 or sa.numel() != M or not sa.is_contiguous() or sw.dim() != 1 or sw.numel() != N or not sw.is_contiguous():
        raise RuntimeError(f"yume_amd.gemm_f8_splitt: scales sa {tuple(sa.shape)}, sw {tuple(sw.shape)} do not fit M={M}, N={N}")
    op, ldo, tp, ldt = None, 0, None, 0
    if out is not None:
        _dev(out, "out", torch.bfloat16)
        op, ldo = _rows(out, "out")
        if out.shape[0] < M or out.shape[1] < n_split:
            raise RuntimeError(f"yume_amd.gemm_f8_splitt: out {tuple(out.shape)} does not hold [{M}, {n_split}]")
    if out_t is not None:
        _dev(out_t, "out_t", torch.bfloat16)
        tp, ldt = _rows(out_t, "out_t")
        if out_t.shape[0] < N - n_split:
            raise RuntimeError(f"yume_amd.gemm_f8_splitt: out_t {tuple(out_t.shape)} does not hold {N - n_split} rows")
    rc = lib.yume_gemm_f8_splitt(ap, lda, sa.data_ptr(), wp, ldw, sw.data_ptr(), _ptr(bias), M, N, K, op, ldo, tp, ldt, n_split, _stream())
    _lib.check(rc, "yume_gemm_f8_splitt")
    return out, out_t


def _bytes(t, name):
    """an int8 row tensor: torch.int8 or torch.uint8 (the kernels read signed bytes either way)"""
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype not in (torch.int8, torch.uint8):
        raise RuntimeError(f"yume_amd: {name} must be a device ('cuda') int8 / uint8 tensor")
    return t


def quant_rows_i8(x, q, scale):
    """q i8 [R, K] = rne(clamp(x / scale[r], +-127)) with scale[r] = max|x[r]| / 127 (1 for a zero row; NaN and zero bytes for a row with a
    non-finite value); x bf16 [R, K], scale fp32 [R] (yume_hip.h)."""
    lib = _lib.load()
    _dev(x, "x", torch.bfloat16)
    _bytes(q, "q")
    _dev(scale, "scale", torch.float32)
    xp, ldx = _rows(x, "x")
    qp, ldq = _rows(q, "q")
    R, K = x.shape
    if tuple(q.shape) != (R, K) or scale.dim() != 1 or scale.numel() != R or not scale.is_contiguous():
        raise RuntimeError(f"yume_amd.quant_rows_i8: x {tuple(x.shape)}, q {tuple(q.shape)}, scale {tuple(scale.shape)} do not fit")
    rc = lib.yume_quant_rows_i8(xp, ldx, R, K, qp, ldq, scale.data_ptr(), _stream())
    _lib.check(rc, "yume_quant_rows_i8")
    return q, scale


def adaln_modulate_i8(x, mul, add, tab_stride, row_idx, add_one, q, scale, eps=1e-6):
    """q i8 [T, C], scale fp32 [T] = quant_rows_i8(adaln_modulate(x, ..., out bf16)) in one kernel, bit for bit (yume_hip.h)."""
    lib = _lib.load()
    _dev(x, "x", torch.float32)
    _bytes(q, "q")
    _dev(scale, "scale", torch.float32)
    xp, ldx = _rows(x, "x")
    qp, ldq = _rows(q, "q")
    T, C = x.shape
    if tuple(q.shape) != (T, C) or scale.dim() != 1 or scale.numel() != T or not scale.is_contiguous():
        raise RuntimeError(f"yume_amd.adaln_modulate_i8: x {tuple(x.shape)}, q {tuple(q.shape)}, scale {tuple(scale.shape)} do not fit")
    rc = lib.yume_adaln_modulate_i8(xp, ldx, T, C, eps, mul.data_ptr(), add.data_ptr(), tab_stride, _ptr(row_idx),
                                    1 if add_one else 0, qp, ldq, scale.data_ptr(), _stream())
    _lib.check(rc, "yume_adaln_modulate_i8")
    return q, scale


def _i8_operands(what, aq, sa, wq, sw):
    _bytes(aq, "aq")
    _bytes(wq, "wq")
    _dev(sa, "sa", torch.float32)
    _dev(sw, "sw", torch.float32)
    ap, lda = _rows(aq, "aq")
    wp, ldw = _rows(wq, "wq")
    M, K = aq.shape
    N, K2 = wq.shape
    if K != K2:
        raise RuntimeError(f"yume_amd.{what}: K mismatch {K} vs {K2}")
    if sa.dim() != 1 or sa.numel() != M or not sa.is_contiguous() or sw.dim() != 1 or sw.numel() != N or not sw.is_contiguous():
        raise RuntimeError(f"yume_amd.{what}: scales sa {tuple(sa.shape)}, sw {tuple(sw.shape)} do not fit M={M}, N={N}")
    return ap, lda, wp, ldw, M, N, K


def gemm_i8(aq, sa, wq, sw, bias, out, epi=EPI_BF16):
    """acc = aq @ wq.T (signed bytes: aq i8 [M,K], wq i8 [N,K]; int32, exact); y = float(acc) * sa[m] * sw[n] + bias; epilogue BF16 or F32."""
    lib = _lib.load()
    ap, lda, wp, ldw, M, N, K = _i8_operands("gemm_i8", aq, sa, wq, sw)
    _dev(out, "out", torch.float32 if epi == EPI_F32 else torch.bfloat16)
    op, ldo = _rows(out, "out")
    if out.shape[0] < M or out.shape[1] < N:
        raise RuntimeError(f"yume_amd.gemm_i8: out {tuple(out.shape)} does not hold [{M}, {N}]")
    rc = lib.yume_gemm_i8(ap, lda, sa.data_ptr(), wp, ldw, sw.data_ptr(), _ptr(bias), M, N, K, epi, op, ldo, _stream())
    _lib.check(rc, "yume_gemm_i8")
    return out


def gemm_i8_splitt(aq, sa, wq, sw, bias, out, out_t, n_split):
    """gemm_i8's sum and scales with the QKV epilogue of gemm_f8_splitt: columns n < n_split bf16 row-major into out [M, >= n_split], columns
    n >= n_split as the K-major V^T image out_t[n - n_split, m] (bf16 [>= N - n_split, ldt >= M]); n_split % 256 == 0 (yume_hip.h)."""
    lib = _lib.load()
    ap, lda, wp, ldw, M, N, K = _i8_operands("gemm_i8_splitt", aq, sa, wq, sw)
    op, ldo, tp, ldt = None, 0, None, 0
    if out is not None:
        _dev(out, "out", torch.bfloat16)
        op, ldo = _rows(out, "out")
        if out.shape[0] < M or out.shape[1] < n_split:
            raise RuntimeError(f"yume_amd.gemm_i8_splitt: out {tuple(out.shape)} does not hold [{M}, {n_split}]")
    if out_t is not None:
        _dev(out_t, "out_t", torch.bfloat16)
        tp, ldt = _rows(out_t, "out_t")
        if out_t.shape[0] < N - n_split:
            raise RuntimeError(f"yume_amd.gemm_i8_splitt: out_t {tuple(out_t.shape)} does not hold {N - n_split} rows")
    rc = lib.yume_gemm_i8_splitt(ap, lda, sa.data_ptr(), wp, ldw, sw.data_ptr(), _ptr(bias), M, N, K, op, ldo, tp, ldt, n_split, _stream())
    _lib.check(rc, "yume_gemm_i8_splitt")
    return out, out_t


EPI_MX_GELU = 7


def gemm_f8_mxout(aq, sa, wq, sw, bias, out, eo, epi=EPI_MX_GELU):
    """the MX producer: out u8 [M, N] = e4m3(gelu_tanh(aq @ wq.T * sa[m] * sw[n] + bias) * 2^-e), eo u8 [M, N / 32] = e + 127 per row and
    32 columns, e the smallest exponent with the block's amax <= 448 * 2^e (yume_hip.h)."""
    lib = _lib.load()
    _dev(aq, "aq", torch.uint8)
    _dev(wq, "wq", torch.uint8)
    _dev(sa, "sa", torch.float32)
    _dev(sw, "sw", torch.float32)
    _dev(out, "out", torch.uint8)
    _dev(eo, "eo", torch.uint8)
    ap, lda = _rows(aq, "aq")
    wp, ldw = _rows(wq, "wq")
    M, K = aq.shape
    N, K2 = wq.shape
    if K != K2:
        raise RuntimeError(f"yume_amd.gemm_f8_mxout: K mismatch {K} vs {K2}")
    if sa.dim() != 1 or sa.numel() != M or not sa.is_contiguous() or sw.dim() != 1 or sw.numel() != N or not sw.is_contiguous():
        raise RuntimeError(f"yume_amd.gemm_f8_mxout: scales sa {tuple(sa.shape)}, sw {tuple(sw.shape)} do not fit M={M}, N={N}")
    op, ldo = _rows(out, "out")
    ep, ldeo = _rows(eo, "eo")
    if tuple(out.shape) != (M, N) or tuple(eo.shape) != (M, N // 32):
        raise RuntimeError(f"yume_amd.gemm_f8_mxout: out {tuple(out.shape)}, eo {tuple(eo.shape)} do not fit M={M}, N={N}")
    rc = lib.yume_gemm_f8_mxout(ap, lda, sa.data_ptr(), wp, ldw, sw.data_ptr(), _ptr(bias), M, N, K, epi, op, ldo, ep, ldeo, _stream())
    _lib.check(rc, "yume_gemm_f8_mxout")
    return out, eo


def gemm_f8_mx(aq, ea, wq, sw, bias, out, epi=EPI_F32, gate=None, gate_stride=0, row_idx=None):
    """the MX consumer: acc = sum over 32-k blocks of 2^(ea[m, b] - 127) * (aq @ wq.T restricted to the block); y = acc * sw[n] + bias;
    epilogue F32 or RESID. ea u8 [M, K / 32] with a row pitch that is a multiple of 16 bytes (yume_hip.h)."""
    lib = _lib.load()
    _dev(aq, "aq", torch.uint8)
    _dev(wq, "wq", torch.uint8)
    _dev(ea, "ea", torch.uint8)
    _dev(sw, "sw", torch.float32)
    ap, lda = _rows(aq, "aq")
    wp, ldw = _rows(wq, "wq")
    ep, ldea = _rows(ea, "ea")
    M, K = aq.shape
    N, K2 = wq.shape
    if K != K2:
        raise RuntimeError(f"yume_amd.gemm_f8_mx: K mismatch {K} vs {K2}")
    if tuple(ea.shape) != (M, K // 32) or sw.dim() != 1 or sw.numel() != N or not sw.is_contiguous():
        raise RuntimeError(f"yume_amd.gemm_f8_mx: scales ea {tuple(ea.shape)}, sw {tuple(sw.shape)} do not fit M={M}, N={N}, K={K}")
    op, ldo = _rows(out, "out")
    rc = lib.yume_gemm_f8_mx(ap, lda, ep, ldea, wp, ldw, sw.data_ptr(), _ptr(bias), M, N, K, epi, op, ldo, _ptr(gate), gate_stride,
                             _ptr(row_idx), _stream())
    _lib.check(rc, "yume_gemm_f8_mx")
    return out


# ---- (r23) OCP MXFP6 e2m3: packed values (32 per 24 bytes, value i at bits [6 i, 6 i + 6)) + one E8M0 byte per row and 32 k (yume_hip.h)
EPI_MX6_GELU = 8
E2M3_MAX = 7.5


def _ceil16(v):
    return (v + 15) // 16 * 16


def mx6_pack(w):
    """the host packer: w [N, K] (bf16 or any float, K % 32 == 0) -> (packed u8 [N, 3 K / 4], scale bytes u8 [N, round_up(K / 32, 16)] of which
    [:, :K / 32] are the scales, the rest 127). In torch on w's device; runs once, when the engine packs. Per row and 32 consecutive k:
    e = the smallest integer with amax <= 7.5 * 2^e (byte e + 127 clamped below at 0; 127 for a zero block), code = e2m3_rne(clamp(w * 2^-e,
    +-7.5)) with the sign bit of every w < 0."""
    N, K = w.shape
    if K % 32:
        raise RuntimeError(f"yume_amd.mx6_pack: K={K} must be a multiple of 32")
    x = w.detach().float()
    amax = x.abs().view(N, K // 32, 32).amax(dim=2)
    m, ex = torch.frexp(amax)                                      # amax = m 2^ex, m in [0.5, 1): 1.f = 2 m
    e = ex - 1 - 2 + (2 * m > 1.875).int()
    byte = torch.where(amax > 0, (e + 127).clamp(min=0), torch.full_like(e, 127))
    mult = torch.pow(2.0, 127 - byte.double()).repeat_interleave(32, dim=1)
    t = (x.double() * mult).clamp(-E2M3_MAX, E2M3_MAX)
    a = t.abs()
    step = torch.pow(2.0, torch.floor(torch.log2(a.clamp(min=1.0))) - 3)       # 1/8 below 2, 1/4 in [2, 4), 1/2 from 4
    r = torch.round(a / step) * step                                # torch.round: half to even
    ex2 = torch.floor(torch.log2(r.clamp(min=1.0)))
    code = torch.where(r < 1.0, r * 8, (ex2 + 1) * 8 + (r / torch.pow(2.0, ex2) - 1) * 8).to(torch.int64) | ((t < 0).to(torch.int64) << 5)
    c = code.view(N, K // 4, 4)
    word = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)            # four values = three bytes
    packed = torch.stack([word & 255, (word >> 8) & 255, (word >> 16) & 255], dim=2).to(torch.uint8).view(N, 3 * K // 4).contiguous()
    eb = torch.full((N, _ceil16(K // 32)), 127, dtype=torch.uint8, device=w.device)
    eb[:, :K // 32] = byte.to(torch.uint8)
    return packed, eb


def adaln_modulate_mx_e2m3(x, mul, add, tab_stride, row_idx, add_one, q, e, eps=1e-6):
    """q u8 [T, 3 C / 4], e u8 [T, C / 32] (a view whose row pitch is a multiple of 16) = the MX6 quantiser applied to
    adaln_modulate(x, ..., out bf16), in one kernel, bit for bit (yume_hip.h)."""
    lib = _lib.load()
    _dev(x, "x", torch.float32)
    _dev(q, "q", torch.uint8)
    _dev(e, "e", torch.uint8)
    xp, ldx = _rows(x, "x")
    qp, ldq = _rows(q, "q")
    ep, lde = _rows(e, "e")
    T, C = x.shape
    if tuple(q.shape) != (T, 3 * C // 4) or tuple(e.shape) != (T, C // 32):
        raise RuntimeError(f"yume_amd.adaln_modulate_mx_e2m3: x {tuple(x.shape)}, q {tuple(q.shape)}, e {tuple(e.shape)} do not fit")
    rc = lib.yume_adaln_modulate_mx_e2m3(xp, ldx, T, C, eps, mul.data_ptr(), add.data_ptr(), tab_stride, _ptr(row_idx),
                                         1 if add_one else 0, qp, ldq, ep, lde, _stream())
    _lib.check(rc, "yume_adaln_modulate_mx_e2m3")
    return q, e


def _f6_operands(who, a6, ea, w6, ew):
    for t, name in ((a6, "a6"), (ea, "ea"), (w6, "w6"), (ew, "ew")):
        _dev(t, name, torch.uint8)
    M, KB = a6.shape
    N, KB2 = w6.shape
    K = KB * 4 // 3
    if KB != KB2 or KB % 96:
        raise RuntimeError(f"yume_amd.{who}: packed rows of {KB} and {KB2} bytes (equal multiples of 96 needed)")
    if tuple(ea.shape) != (M, K // 32) or tuple(ew.shape) != (N, K // 32):
        raise RuntimeError(f"yume_amd.{who}: scales ea {tuple(ea.shape)}, ew {tuple(ew.shape)} do not fit M={M}, N={N}, K={K}")
    return M, N, K


def gemm_f6_mxout(a6, ea, w6, ew, bias, out, eo, epi=EPI_MX6_GELU):
    """the MX6 producer: out u8 [M, 3 N / 4], eo u8 [M, N / 32] = the MX6 quantiser applied to gelu_tanh(acc + bias), acc the block-scaled
    e2m3 x e2m3 sum of yume_gemm_f6_mx (yume_hip.h). ea / ew / eo: views [rows, K / 32] / [M, N / 32] with a row pitch that is a multiple of 16."""
    lib = _lib.load()
    M, N, K = _f6_operands("gemm_f6_mxout", a6, ea, w6, ew)
    _dev(out, "out", torch.uint8)
    _dev(eo, "eo", torch.uint8)
    if tuple(out.shape) != (M, 3 * N // 4) or tuple(eo.shape) != (M, N // 32):
        raise RuntimeError(f"yume_amd.gemm_f6_mxout: out {tuple(out.shape)}, eo {tuple(eo.shape)} do not fit M={M}, N={N}")
    (ap, lda), (eap, ldea), (wp, ldw), (ewp, ldew) = _rows(a6, "a6"), _rows(ea, "ea"), _rows(w6, "w6"), _rows(ew, "ew")
    (op, ldo), (eop, ldeo) = _rows(out, "out"), _rows(eo, "eo")
    rc = lib.yume_gemm_f6_mxout(ap, lda, eap, ldea, wp, ldw, ewp, ldew, _ptr(bias), M, N, K, epi, op, ldo, eop, ldeo, _stream())
    _lib.check(rc, "yume_gemm_f6_mxout")
    return out, eo


def gemm_f6_mx(a6, ea, w6, ew, bias, out, epi=EPI_F32, gate=None, gate_stride=0, row_idx=None):
    """the MX6 consumer: acc = sum over 32-k blocks of 2^(ea[m, b] - 127) 2^(ew[n, b] - 127) * (a6 @ w6.T restricted to the block);
    y = acc + bias; epilogue F32 or RESID (yume_hip.h)."""
    lib = _lib.load()
    M, N, K = _f6_operands("gemm_f6_mx", a6, ea, w6, ew)
    (ap, lda), (eap, ldea), (wp, ldw), (ewp, ldew) = _rows(a6, "a6"), _rows(ea, "ea"), _rows(w6, "w6"), _rows(ew, "ew")
    op, ldo = _rows(out, "out")
    rc = lib.yume_gemm_f6_mx(ap, lda, eap, ldea, wp, ldw, ewp, ldew, _ptr(bias), M, N, K, epi, op, ldo, _ptr(gate), gate_stride,
                             _ptr(row_idx), _stream())
    _lib.check(rc, "yume_gemm_f6_mx")
    return out


# Scratch buffers of the split-K GEMM and the attention key-range split are keyed by (device, stream): two callers on
# different HIP streams of one device (a VAE decode overlapped with the next chunk's denoise, say) never share partials.
_splitk_ws = {}
# r27: each of them (and _attn_ws / _attn_batch_ws below) is REPLACED when a bigger call arrives on its (device, stream), and a hipGraph
# captured from a smaller call holds the old tensor's raw pointer. The stream in the key does not save it: torch.cuda.graph captures on one
# shared side stream unless given another, so a second capture at a larger shape, or an eager call on the stream that was captured on, finds
# the same entry. What a capture was handed is therefore kept here until release_captured().
_captured = []


def _pin_if_capturing(ws):
    if torch.cuda.is_current_stream_capturing() and not any(ws is c for c in _captured):
        _captured.append(ws)
    return ws


def release_captured():
    """forget the scratch tensors stream captures were handed. Call it after deleting every graph captured through this module (the DiT
    engine's, the encoders'): a graph replayed afterwards may write partials into memory handed to someone else."""
    _captured.clear()


def _ws_key(t):
    return (t.device.index, _stream())


def small_m_splits(M, N, K, target_blocks=256):
    """The number of K slices `gemm_small_m` cuts an [M, K] x [N, K]^T product into; 1 means the plain `gemm_bf16` call. Pure
    host arithmetic (no device, no tensors): tests derive the route of every encoder linear from it."""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    splits = 1
    while splits < 16 and tiles * splits * 2 <= target_blocks and K % (splits * 2 * 64) == 0 and K // (splits * 2) >= 256:
        splits *= 2
    if splits == 1 or N % 8 or (M * N) % 4:
        return 1
    return splits


def gemm_small_m(a, w, bias, out, epi=EPI_BF16, target_blocks=256):
    """a @ w.T for a small number of rows against a large weight (encoders): split-K over enough slices to put ~target_blocks
    workgroups on the chip; falls back to the plain call when no split is possible or needed."""
    M, K = a.shape
    N = w.shape[0]
    splits = small_m_splits(M, N, K, target_blocks)
    if splits == 1:
        return gemm_bf16(a, w, bias, out, epi, variant=2 if epi == EPI_BF16_GEGLU else 0)
    lib = _lib.load()
    _dev(a, "a", torch.bfloat16)
    _dev(w, "w", torch.bfloat16)
    ap, lda = _rows(a, "a")
    wp, ldw = _rows(w, "w")
    op, ldo = _rows(out, "out")
    need = splits * M * N
    key = _ws_key(a)
    ws = _splitk_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, 1 << 22), dtype=torch.float32, device=a.device)
        _splitk_ws[key] = ws
    _pin_if_capturing(ws)
    rc = lib.yume_gemm_bf16_splitk(ap, lda, wp, ldw, _ptr(bias), M, N, K, epi, op, ldo, splits, ws.data_ptr(), _stream())
    _lib.check(rc, "yume_gemm_bf16_splitk")
    return out


def rmsnorm_rope(buf, C, nparts, w, eps=1e-6, rope=None, head_dim=128):
    """in-place RMSNorm over C (+RoPE) on the first nparts*C columns of bf16 `buf` [T, >=nparts*C]."""
    lib = _lib.load()
    _dev(buf, "buf", torch.bfloat16)
    bp, ld = _rows(buf, "buf")
    T = buf.shape[0]
    rc = lib.yume_rmsnorm_rope(bp, ld, T, C, nparts, w.data_ptr(), eps, _ptr(rope), head_dim, _stream())
    _lib.check(rc, "yume_rmsnorm_rope")
    return buf


def rmsnorm_rows_periodic(buf, C, w, eps=1e-6):
    """in-place RMSNorm over C of bf16 `buf` [T, C]; row t uses weight row t % w.shape[0] (w fp32 [period, C])."""
    lib = _lib.load()
    _dev(buf, "buf", torch.bfloat16)
    bp, ld = _rows(buf, "buf")
    rc = lib.yume_rmsnorm_rows_periodic(bp, ld, buf.shape[0], C, w.data_ptr(), w.shape[0], eps, _stream())
    _lib.check(rc, "yume_rmsnorm_rows_periodic")
    return buf


_attn_ws, _attn_ws_bytes = {}, {}


ATTN_Q_PRESCALED = 0x100     # YUME_ATTN_Q_PRESCALED
ATTN_KV_PADDED = 0x200       # YUME_ATTN_KV_PADDED


def attn_fwd(q, k, vt, out, Lq, Lk, H, scale=None, accumulate=False, variant=0, use_workspace=True, q_prescaled=False, kv_padded=False,
             last_key_weight=1.0, window=(-1, -1), q_pos0=0, frame_window=None, spans=None, frame_sink=0, prefix=None):
    """out[Lq, H*128] = softmax(q k^T * scale) v ; q,k token-major bf16 2-D views, vt K-major [H*128, >=Lk].
    q_prescaled: q already carries scale * log2(e) (`scale` is ignored): out = sum_j 2^(q.k_j) v_j / sum_j 2^(q.k_j).
    kv_padded: the caller guarantees that k's storage is readable up to ceil(Lk/64)*64 rows and that vt has that many columns with finite
    values behind column Lk (YUME_ATTN_KV_PADDED): with q_prescaled it opens the persistent kernel (attn_fwd8.hip).
    last_key_weight: key Lk - 1 stands for that many identical keys (yume_attn_fwd_kw; variants 0, 2 and 10 = the short-key kernel, Lk <= 128).
    The weighted export is called only for a weight other than 1 or variant 10; every other call is the one it always was.
    window = (left, right), q_pos0: query row i sits at q_pos0 + i on the key axis and sees the keys j with q_pos0 + i - left <= j <= q_pos0 + i +
    right (-1: unbounded on that side; causal is right = 0; yume_attn_fwd_band, variants 0 and 11, no weighted last key). The banded export is
    called only for a window other than (-1, -1), and runs the banded kernel only where the window hides a key from a row.
    frame_window = (back, ahead), spans = [(rows, blocks), ...], q_pos0: the key axis is partitioned into blocks (frames) by the spans in order,
    `blocks` blocks of `rows` rows each; query row i sits at q_pos0 + i and sees every key of the blocks within `back` before and `ahead` after
    its own (-1: unbounded on that side; (-1, 0) is frame-causal; yume_attn_fwd_fband, variants 0 and 12, no weighted last key, no token
    window beside it). None (the default): the call is the one it always was.
    frame_sink = n > 0, with a frame_window: the first n blocks of the partition are seen by every row as well (0 <= n <= the partition's
    blocks; yume_attn_fwd_fsink, variants 0 and 13). 0 (the default): the call is the one it always was.
    prefix = (kp, vtp, n_prefix), with a frame_window: n_prefix more keys that every row sees, in buffers of their own (kp token-major
    [>= n_prefix, H*128], vtp K-major [H*128, >= n_prefix]), in front of k / vt in the softmax's order; k, vt, Lk, spans, frame_window and
    q_pos0 then describe the suffix alone, numbered from 0 (yume_attn_fwd_fprefix, variants 0 and 14, no frame_sink beside it). None (the
    default): the call is the one it always was."""
    lib = _lib.load()
    window = (int(window[0]), int(window[1]))
    frame_sink = int(frame_sink)
    if prefix is not None:
        if frame_window is None:
            raise ValueError("yume_amd.attn_fwd: prefix= needs a frame_window= (the prefix is the frame window's: yume_attn_fwd_fprefix)")
        if frame_sink != 0:
            raise ValueError(f"yume_amd.attn_fwd: prefix= and frame_sink={frame_sink} do not combine (the prefix is the always-visible part)")
        pk, pvt, n_prefix = prefix
        n_prefix = int(n_prefix)
    if frame_sink != 0 and frame_window is None:
        raise RuntimeError(f"yume_amd.attn_fwd: frame_sink={frame_sink} needs a frame_window (the sink is the frame window's: yume_attn_fwd_fsink)")
    if frame_window is not None:
        if window != (-1, -1):
            raise RuntimeError("yume_amd.attn_fwd: frame_window and window do not combine (one mask per call)")
        if last_key_weight != 1.0:
            raise RuntimeError("yume_amd.attn_fwd: a frame_window and a last_key_weight != 1 do not combine (yume_attn_fwd_fband takes no weighted key)")
        if spans is None:
            raise RuntimeError("yume_amd.attn_fwd: frame_window needs spans = [(rows, blocks), ...] (yume_amd.framepack.frame_spans)")
        spans = [(int(r), int(b)) for r, b in spans]
    elif spans is not None:
        raise RuntimeError("yume_amd.attn_fwd: spans without a frame_window")
    if window != (-1, -1) and last_key_weight != 1.0:
        raise RuntimeError("yume_amd.attn_fwd: a window and a last_key_weight != 1 do not combine (yume_attn_fwd_band takes no weighted key)")
    _dev(q, "q", torch.bfloat16)
    _dev(k, "k", torch.bfloat16)
    _dev(vt, "vt", torch.bfloat16)
    _dev(out, "out", torch.bfloat16)
    ensure_counters(q.device)
    qp, ldq = _rows(q, "q")
    kp, ldk = _rows(k, "k")
    vp, ldv = _rows(vt, "vt")
    op, ldo = _rows(out, "out")
    if kv_padded:
        # the caller's word is checked where the tensors can tell: V^T must HAVE the padded columns, and k's storage must
        # cover the rows of the last whole tile (a tight view at the end of an allocation would be read out of bounds). That the padding
        # is finite stays the caller's contract — dit.py keeps it in zero-filled buffers.
        Lp = (Lk + 63) // 64 * 64
        if vt.shape[1] < Lp:
            raise RuntimeError(f"yume_amd.attn_fwd: kv_padded needs vt with >= {Lp} columns (ceil(Lk / 64) * 64), got {vt.shape[1]}")
        need = k.storage_offset() + (Lp - 1) * ldk + H * 128
        have = k.untyped_storage().nbytes() // k.element_size()
        if need > have:
            raise RuntimeError(f"yume_amd.attn_fwd: kv_padded needs k's storage to cover {Lp} rows (ceil(Lk / 64) * 64): the view ends "
                               f"{need - have} elements short")
    if scale is None:
        scale = 1.0 / math.sqrt(128.0)
    ws, nbytes = None, 0
    if variant in (0, 8) and use_workspace:
        key = (q.device.index, Lq, Lk, H)
        nbytes = _attn_ws_bytes.get(key)
        if nbytes is None:
            nbytes = _attn_ws_bytes[key] = int(lib.yume_attn_workspace_bytes(Lq, Lk, H))
        if nbytes:
            wkey = _ws_key(q)
            ws = _attn_ws.get(wkey)
            if ws is None or ws.numel() < nbytes:
                ws = _attn_ws[wkey] = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
            _pin_if_capturing(ws)
    flags = variant | (ATTN_Q_PRESCALED if q_prescaled else 0) | (ATTN_KV_PADDED if kv_padded else 0)
    if frame_window is not None:
        import ctypes
        arr = ctypes.c_int64 * max(len(spans), 1)          # host arrays: read during the call, handed to the kernel by value
        if prefix is not None:
            pkp, ldkp, pvp, ldvp = None, 0, None, 0
            if n_prefix > 0:
                _dev(pk, "prefix k", torch.bfloat16)
                _dev(pvt, "prefix vt", torch.bfloat16)
                if pk.shape[0] < n_prefix or pk.shape[1] < H * 128 or pvt.shape[0] < H * 128 or pvt.shape[1] < n_prefix:
                    raise RuntimeError(f"yume_amd.attn_fwd: prefix k {tuple(pk.shape)} / vt {tuple(pvt.shape)} do not hold {n_prefix} keys of "
                                       f"{H} heads")
                (pkp, ldkp), (pvp, ldvp) = _rows(pk, "prefix k"), _rows(pvt, "prefix vt")
            rc = lib.yume_attn_fwd_fprefix(qp, ldq, kp, ldk, vp, ldv, op, ldo, Lq, Lk, H, scale, 1 if accumulate else 0, flags, int(q_pos0),
                                           len(spans), arr(*[r for r, _ in spans]), arr(*[b for _, b in spans]), int(frame_window[0]),
                                           int(frame_window[1]), pkp, ldkp, pvp, ldvp, n_prefix, _ptr(ws), nbytes if ws is not None else 0,
                                           _stream())
            _lib.check(rc, "yume_attn_fwd_fprefix")
            return out
        if frame_sink != 0:
            rc = lib.yume_attn_fwd_fsink(qp, ldq, kp, ldk, vp, ldv, op, ldo, Lq, Lk, H, scale, 1 if accumulate else 0, flags, int(q_pos0), len(spans),
                                         arr(*[r for r, _ in spans]), arr(*[b for _, b in spans]), int(frame_window[0]), int(frame_window[1]),
                                         frame_sink, _ptr(ws), nbytes if ws is not None else 0, _stream())
            _lib.check(rc, "yume_attn_fwd_fsink")
            return out
        rc = lib.yume_attn_fwd_fband(qp, ldq, kp, ldk, vp, ldv, op, ldo, Lq, Lk, H, scale, 1 if accumulate else 0, flags, int(q_pos0), len(spans),
                                     arr(*[r for r, _ in spans]), arr(*[b for _, b in spans]), int(frame_window[0]), int(frame_window[1]),
                                     _ptr(ws), nbytes if ws is not None else 0, _stream())
        _lib.check(rc, "yume_attn_fwd_fband")
        return out
    if window != (-1, -1):
        rc = lib.yume_attn_fwd_band(qp, ldq, kp, ldk, vp, ldv, op, ldo, Lq, Lk, H, scale, 1 if accumulate else 0, flags, int(q_pos0), window[0],
                                    window[1], _ptr(ws), nbytes if ws is not None else 0, _stream())
        _lib.check(rc, "yume_attn_fwd_band")
        return out
    if last_key_weight != 1.0 or variant == 10:
        rc = lib.yume_attn_fwd_kw(qp, ldq, kp, ldk, vp, ldv, op, ldo, Lq, Lk, H, scale, 1 if accumulate else 0, flags, _ptr(ws),
                                  nbytes if ws is not None else 0, float(last_key_weight), _stream())
    else:
        rc = lib.yume_attn_fwd_ws(qp, ldq, kp, ldk, vp, ldv, op, ldo, Lq, Lk, H, scale, 1 if accumulate else 0, flags, _ptr(ws),
                                  nbytes if ws is not None else 0, _stream())
    _lib.check(rc, "yume_attn_fwd")
    return out


def attn_fwd_seg(q, ks, vts, out, Lq_seg, seg_pitch, Lks, H, scale=None, accumulate=False, variant=0, q_prescaled=False, kv_padded=False,
                 last_key_weights=None):
    """Segmented attention (yume_attn_fwd_seg): segment s = the rows [s * seg_pitch, s * seg_pitch + Lq_seg) of q and out, attending over
    ks[s] / vts[s] with Lks[s] keys whose last one counts last_key_weights[s] times (None: every weight 1). One launch for all segments;
    the rows of the pitch gap are neither read nor written. All ks (and all vts) share one row stride. kv_padded: as for attn_fwd, for
    every segment. variants 0, 2 (4-wave LDS-DMA kernel) and 10 (short-key kernel, every Lks[s] <= 128)."""
    lib = _lib.load()
    nseg = len(ks)
    if nseg < 1 or len(vts) != nseg or len(Lks) != nseg or (last_key_weights is not None and len(last_key_weights) != nseg):
        raise RuntimeError("yume_amd.attn_fwd_seg: ks, vts, Lks and last_key_weights must list the same number (>= 1) of segments")
    _dev(q, "q", torch.bfloat16)
    _dev(out, "out", torch.bfloat16)
    if nseg == 1:
        ensure_counters(q.device)          # (one segment is attn_fwd's call, with attn_fwd's kernel choice)
    qp, ldq = _rows(q, "q")
    op, ldo = _rows(out, "out")
    rows =(nseg - 1) * seg_pitch + Lq_seg
    if q.shape[0] < rows or out.shape[0] < rows or q.shape[1] < H * 128 or out.shape[1] < H * 128:
        raise RuntimeError(f"yume_amd.attn_fwd_seg: q {tuple(q.shape)} / out {tuple(out.shape)} do not hold {rows} rows of {H} heads")
    kps, vps, ldk, ldv = [], [], None, None
    for s, (k, vt, Lk) in enumerate(zip(ks, vts, Lks)):
        _dev(k, f"ks[{s}]", torch.bfloat16)
        _dev(vt, f"vts[{s}]", torch.bfloat16)
        kp, lk = _rows(k, f"ks[{s}]")
        vp, lv = _rows(vt, f"vts[{s}]")
        if (ldk, ldv) not in ((None, None), (lk, lv)):
            raise RuntimeError("yume_amd.attn_fwd_seg: every segment's k (and vt) must have the same row stride")
        ldk, ldv = lk, lv
        Lp = (Lk + 63) // 64 * 64 if kv_padded else Lk
        need = k.storage_offset() + (Lp - 1) * lk + H * 128
        if k.shape[0] < Lk or vt.shape[0] < H * 128 or vt.shape[1] < Lp or need > k.untyped_storage().nbytes() // k.element_size():
            raise RuntimeError(f"yume_amd.attn_fwd_seg: segment {s}: k {tuple(k.shape)} / vt {tuple(vt.shape)} do not hold {Lp} keys of {H} heads")
        kps.append(kp)
        vps.append(vp)
    if scale is None:
        scale = 1.0 / math.sqrt(128.0)
    import ctypes
    karr, varr = (ctypes.c_void_p * nseg)(*kps), (ctypes.c_void_p * nseg)(*vps)
    larr = (ctypes.c_int64 * nseg)(*[int(x) for x in Lks])
    warr = None if last_key_weights is None else (ctypes.c_float * nseg)(*[float(w) for w in last_key_weights])
    flags = variant | (ATTN_Q_PRESCALED if q_prescaled else 0) | (ATTN_KV_PADDED if kv_padded else 0)
    rc = lib.yume_attn_fwd_seg(qp, ldq, karr, ldk, varr, ldv, op, ldo, nseg, Lq_seg, seg_pitch, larr, H, scale, 1 if accumulate else 0, flags,
                               warr, _stream())
    _lib.check(rc, "yume_attn_fwd_seg")
    return out


_attn_batch_ws, _attn_batch_ws_bytes = {}, {}


def attn_fwd_batch(q, k, vt, out, nseg, Lq_seg, q_pitch, Lk_seg, k_pitch, H, scale=None, accumulate=False, variant=0, use_workspace=True,
                   q_prescaled=False, kv_padded=False):
    """Batched self-attention (yume_attn_fwd_batch): nseg problems of one shape stacked in q / k / vt / out. Segment s = the rows
    [s * q_pitch, s * q_pitch + Lq_seg) of q and out, the rows [s * k_pitch, s * k_pitch + Lk_seg) of k and the columns of vt from s * k_pitch
    on; the pitch gaps are neither read for a result nor written. One launch of the persistent kernel over (segment, head) pairs where it
    applies (variant 0 with both flags, Lk_seg >= 1536, Lq_seg >= 256; variant 8 insists, Lk_seg >= 512), otherwise one of the segmented
    4-wave kernel (variant 2 insists). q_prescaled / kv_padded: as for attn_fwd, for every segment. The scratch for key-range pieces is kept
    per (device, stream)."""
    lib = _lib.load()
    _dev(q, "q", torch.bfloat16)
    _dev(k, "k", torch.bfloat16)
    _dev(vt, "vt", torch.bfloat16)
    _dev(out, "out", torch.bfloat16)
    ensure_counters(q.device)
    qp, ldq = _rows(q, "q")
    kp, ldk = _rows(k, "k")
    vp, ldv = _rows(vt, "vt")
    op, ldo = _rows(out, "out")
    rows = (nseg - 1) * q_pitch + Lq_seg
    if nseg < 1 or q.shape[0] < rows or out.shape[0] < rows or q.shape[1] < H * 128 or out.shape[1] < H * 128:
        raise RuntimeError(f"yume_amd.attn_fwd_batch: q {tuple(q.shape)} / out {tuple(out.shape)} do not hold {nseg} segments of {Lq_seg} rows "
                           f"({q_pitch} apart) of {H} heads")
    # every segment's keys must be there: with kv_padded up to the last whole tile (as attn_fwd checks), in k's STORAGE and in vt's columns
    Lp = (Lk_seg + 63) // 64 * 64 if kv_padded else Lk_seg
    need = k.storage_offset() + ((nseg - 1) * k_pitch + Lp - 1) * ldk + H * 128
    have = k.untyped_storage().nbytes() // k.element_size()
    if k.shape[0] < (nseg - 1) * k_pitch + Lk_seg or k.shape[1] < H * 128 or need > have:
        raise RuntimeError(f"yume_amd.attn_fwd_batch: k {tuple(k.shape)} does not hold {nseg} segments of {Lp} keys ({k_pitch} apart) of {H} heads")
    if vt.shape[0] < H * 128 or vt.shape[1] < (nseg - 1) * k_pitch + Lp:
        raise RuntimeError(f"yume_amd.attn_fwd_batch: vt {tuple(vt.shape)} does not hold {nseg} segments of {Lp} key columns ({k_pitch} apart) "
                           f"of {H} heads")
    if scale is None:
        scale = 1.0 / math.sqrt(128.0)
    ws, nbytes = None, 0
    if variant in (0, 8) and use_workspace:
        key = (q.device.index, nseg, Lq_seg, Lk_seg, H)
        nbytes = _attn_batch_ws_bytes.get(key)
        if nbytes is None:
            nbytes = _attn_batch_ws_bytes[key] = int(lib.yume_attn_batch_workspace_bytes(nseg, Lq_seg, Lk_seg, H))
        if nbytes:
            wkey = _ws_key(q)
            ws = _attn_batch_ws.get(wkey)
            if ws is None or ws.numel() < nbytes:
                ws = _attn_batch_ws[wkey] = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
            _pin_if_capturing(ws)
    flags = variant | (ATTN_Q_PRESCALED if q_prescaled else 0) | (ATTN_KV_PADDED if kv_padded else 0)
    rc = lib.yume_attn_fwd_batch(qp, ldq, kp, ldk, vp, ldv, op, ldo, nseg, Lq_seg, q_pitch, Lk_seg, k_pitch, H, scale, 1 if accumulate else 0,
                                 flags, _ptr(ws), ws.numel() if ws is not None else 0, _stream())
    _lib.check(rc, "yume_attn_fwd_batch")
    return out


def quant_rows_mx_e4m3(x, q, e):
    """OCP MX quantiser (yume_quant_rows_mx_e4m3): x bf16 [R, K] -> q u8 [R, K] e4m3 bytes, e u8 [R, K / 32] E8M0 scale bytes, one per row
    and 32 consecutive columns."""
    lib = _lib.load()
    _dev(x, "x", torch.bfloat16)
    _dev(q, "q", torch.uint8)
    _dev(e, "e", torch.uint8)
    xp, ldx = _rows(x, "x")
    qp, ldq = _rows(q, "q")
    ep, lde = _rows(e, "e")
    R, K = x.shape
    if tuple(q.shape) != (R, K) or tuple(e.shape) != (R, K // 32):
        raise RuntimeError(f"yume_amd.quant_rows_mx_e4m3: x {tuple(x.shape)}, q {tuple(q.shape)}, e {tuple(e.shape)} do not fit")
    rc = lib.yume_quant_rows_mx_e4m3(xp, ldx, R, K, qp, ldq, ep, lde, _stream())
    _lib.check(rc, "yume_quant_rows_mx_e4m3")
    return q, e


def attn_vt_mx_e4m3(vt, Lk, vt8, ev):
    """The e4m3 V^T image of attn_fwd_f8mx (yume_attn_vt_mx_e4m3): vt bf16 [C, >= Lk] K-major -> vt8 u8 [C, >= 128 * tiles] in the kernel's key
    order, ev u8 [tiles, >= 4 * C], tiles = ceil(Lk / 128); keys >= Lk of the last tile are written as zeros."""
    lib = _lib.load()
    _dev(vt, "vt", torch.bfloat16)
    _dev(vt8, "vt8", torch.uint8)
    _dev(ev, "ev", torch.uint8)
    vp, ldvt = _rows(vt, "vt")
    v8p, ldvt8 = _rows(vt8, "vt8")
    evp, ldev = _rows(ev, "ev")
    C = vt.shape[0]
    tiles = (Lk + 127) // 128
    if vt.shape[1] < Lk or vt8.shape[0] != C or vt8.shape[1] < 128 * tiles or ev.shape[0] < tiles or ev.shape[1] < 4 * C:
        raise RuntimeError(f"yume_amd.attn_vt_mx_e4m3: vt {tuple(vt.shape)}, vt8 {tuple(vt8.shape)}, ev {tuple(ev.shape)} do not fit Lk={Lk}")
    rc = lib.yume_attn_vt_mx_e4m3(vp, ldvt, C, Lk, v8p, ldvt8, evp, ldev, _stream())
    _lib.check(rc, "yume_attn_vt_mx_e4m3")
    return vt8, ev


def attn_fwd_f8mx(q8, eq, k8, ek, vt8, ev, out, Lq, Lk, H):
    """out[Lq, H*128] bf16 = sum_j 2^(q.k_j) v_j / sum_j 2^(q.k_j) over MX e4m3 operands (yume_attn_fwd_f8mx): q8 / k8 u8 token-major 2-D views
    with their scale bytes eq / ek [rows, >= 4 H] (quant_rows_mx_e4m3), vt8 / ev from attn_vt_mx_e4m3. q already carries scale * log2(e)."""
    lib = _lib.load()
    for t, name in ((q8, "q8"), (eq, "eq"), (k8, "k8"), (ek, "ek"), (vt8, "vt8"), (ev, "ev")):
        _dev(t, name, torch.uint8)
    _dev(out, "out", torch.bfloat16)
    qp, ldq = _rows(q8, "q8")
    eqp, ldeq = _rows(eq, "eq")
    kp, ldk = _rows(k8, "k8")
    ekp, ldek = _rows(ek, "ek")
    vp, ldvt8 = _rows(vt8, "vt8")
    evp, ldev = _rows(ev, "ev")
    op, ldo = _rows(out, "out")
    tiles = (Lk + 127) // 128
    if (q8.shape[0] < Lq or eq.shape[0] < Lq or k8.shape[0] < Lk or ek.shape[0] < Lk or out.shape[0] < Lq or vt8.shape[0] < H * 128
            or vt8.shape[1] < 128 * tiles or ev.shape[0] < tiles or min(q8.shape[1], k8.shape[1], out.shape[1]) < H * 128
            or min(eq.shape[1], ek.shape[1]) < 4 * H or ev.shape[1] < 512 * H):
        raise RuntimeError(f"yume_amd.attn_fwd_f8mx: operands do not fit Lq={Lq} Lk={Lk} H={H}: q8 {tuple(q8.shape)} eq {tuple(eq.shape)} "
                           f"k8 {tuple(k8.shape)} ek {tuple(ek.shape)} vt8 {tuple(vt8.shape)} ev {tuple(ev.shape)} out {tuple(out.shape)}")
    rc = lib.yume_attn_fwd_f8mx(qp, ldq, eqp, ldeq, kp, ldk, ekp, ldek, vp, ldvt8, evp, ldev, op, ldo, Lq, Lk, H, _stream())
    _lib.check(rc, "yume_attn_fwd_f8mx")
    return out


def linear_smallm_f32(x, w, bias, out, in_act=0, out_act=0, add_table=None):
    lib = _lib.load()
    _dev(x, "x", torch.float32)
    R, K = x.shape
    N = w.shape[0]
    if not (x.is_contiguous() and w.is_contiguous() and out.is_contiguous()):
        raise RuntimeError("yume_amd.linear_smallm_f32: tensors must be contiguous")
    if w.dtype not in (torch.float32, torch.bfloat16) or w.shape[1] != K:
        raise RuntimeError("yume_amd.linear_smallm_f32: bad weight")
    rc = lib.yume_linear_smallm_f32(x.data_ptr(), R, K, w.data_ptr(), 1 if w.dtype == torch.bfloat16 else 0,
                                    _ptr(bias), N, in_act, out_act, _ptr(add_table), out.data_ptr(), _stream())
    _lib.check(rc, "yume_linear_smallm_f32")
    return out


def modulation_table(tab, e0, out):
    """out[b, r, :] = tab[b, :] + e0[r, :]  (fp32, contiguous)."""
    lib = _lib.load()
    _dev(tab, "tab", torch.float32)
    _dev(e0, "e0", torch.float32)
    B, W = tab.shape
    R = e0.shape[0]
    if not (tab.is_contiguous() and e0.is_contiguous() and out.is_contiguous()) or e0.shape[1] != W:
        raise RuntimeError("yume_amd.modulation_table: bad layout")
    rc = lib.yume_modulation_table(tab.data_ptr(), e0.data_ptr(), B, R, W, out.data_ptr(), _stream())
    _lib.check(rc, "yume_modulation_table")
    return out


def sinusoidal_embed(t, t_index, R, dim, out):
    lib = _lib.load()
    _dev(t, "t", torch.float64)
    rc = lib.yume_sinusoidal_embed(t.data_ptr(), _ptr(t_index), R, dim, out.data_ptr(), _stream())
    _lib.check(rc, "yume_sinusoidal_embed")
    return out


def patch_gather(x, f0, nf, kh, kw, out):
    """x [Cin,F,H,W] fp32|bf16 contiguous -> out bf16 [nf*ceil(H/kh)*ceil(W/kw), Kp]."""
    lib = _lib.load()
    _dev(x, "x")
    if not x.is_contiguous() or x.dim() != 4:
        raise RuntimeError("yume_amd.patch_gather: x must be contiguous [Cin,F,H,W]")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("yume_amd.patch_gather: x must be fp32 or bf16")
    Cin, F, H, W = x.shape
    op, Kp = _rows(out, "out")
    rc = lib.yume_patch_gather(x.data_ptr(), 1 if x.dtype == torch.bfloat16 else 0, Cin, F, H, W, f0, nf, kh, kw, op,
                               Kp, _stream())
    _lib.check(rc, "yume_patch_gather")
    return out


def unpatchify(x, Fr, Hp, Wp, ph, pw, Cout, out):
    lib = _lib.load()
    _dev(x, "x", torch.float32)
    xp, ldi = _rows(x, "x")
    rc = lib.yume_unpatchify(xp, ldi, Fr, Hp, Wp, ph, pw, Cout, out.data_ptr(), _stream())
    _lib.check(rc, "yume_unpatchify")
    return out


def cast_bf16(x, rows_valid, out):
    lib = _lib.load()
    _dev(x, "x", torch.float32)
    xp, ldi = _rows(x, "x")
    op, ldo = _rows(out, "out")
    rows, cols = out.shape
    rc = lib.yume_cast_bf16(xp, ldi, rows_valid, rows, cols, op, ldo, _stream())
    _lib.check(rc, "yume_cast_bf16")
    return out


def transpose_bf16(x, out):
    """x [rows, cols] fp32|bf16 -> out bf16 [cols, >=rows]."""
    lib = _lib.load()
    _dev(x, "x")
    xp, ldi = _rows(x, "x")
    op, ldo = _rows(out, "out")
    rows, cols = x.shape
    rc = lib.yume_transpose_bf16(xp, 1 if x.dtype == torch.bfloat16 else 0, ldi, rows, cols, op, ldo, _stream())
    _lib.check(rc, "yume_transpose_bf16")
    return out
