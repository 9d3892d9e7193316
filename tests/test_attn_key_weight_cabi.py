"""yume_attn_fwd_kw (ABI 9): a weighted last key. What can be said without a GPU: the export exists and is bound, its host-side validation
answers by name before any launch, and the identity the feature rests on (m copies of one key == that key once with weight m) holds in fp64."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import ROOT

N_LIST = [0, 1, 62, 63, 64, 77, 127, 128, 300, 511]
EINVAL, EUNSUP = -1, -3


def _lib():
    import __graft_entry__ as g
    g.build()
    from yume_amd import _lib
    return _lib


def test_export_header_and_binding_agree():
    _l = _lib()
    hdr = open(os.path.join(ROOT, "include", "yume_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    syms = sorted(set(re.findall(r"\b(yume_[a-z0-9_]+)\s*\(", src)))
    assert "yume_attn_fwd_kw" in syms
    assert sorted(_l.SIGNATURES) == syms
    raw = ctypes.CDLL(_l.LIB_PATH)
    for s in syms:
        assert hasattr(raw, s), f"{s} declared in yume_hip.h but not exported"
    # the new call is yume_attn_fwd_ws's argument list with `float last_key_weight` in front of the stream
    ws, kw = _l.SIGNATURES["yume_attn_fwd_ws"], _l.SIGNATURES["yume_attn_fwd_kw"]
    assert kw == ws[:-1] + [ctypes.c_float] + ws[-1:]
    lib = _l.load()
    assert lib.yume_abi_version() == _l.ABI_VERSION == 9 == int(re.search(r"#define YUME_ABI_VERSION (\d+)", hdr).group(1))


def _call(lib, Lk=78, variant=0, weight=2.0, Lq=64, H=2, ldvt=None):
    # pointers are never dereferenced on the host: any 16-byte aligned non-NULL value passes the common checks
    p = 4096
    ldvt = ldvt if ldvt is not None else (Lk + 7) // 8 * 8
    return lib.yume_attn_fwd_kw(p, H * 128, p, H * 128, p, ldvt, p, H * 128, Lq, Lk, H, 0.088, 0, variant, None, 0, weight, None)


@pytest.mark.parametrize("weight", [0.0, 0.5, -1.0, float("nan"), float("inf"), float(2 ** 21)])
@pytest.mark.parametrize("variant", [0, 2, 10])
def test_weight_out_of_range_is_einval_by_name(weight, variant):
    lib = _lib().load()
    assert _call(lib, variant=variant, weight=weight) == EINVAL
    assert b"last_key_weight" in lib.yume_last_error()


@pytest.mark.parametrize("variant", [1, 4, 7, 8, 9])
@pytest.mark.parametrize("flags", [0, 0x100 | 0x200])
def test_kernels_without_a_weight_are_eunsup_and_named(variant, flags):
    lib = _lib().load()
    for Lk, Lq in ((78, 64), (512, 2048), (2048, 2048)):
        assert _call(lib, Lk=Lk, Lq=Lq, variant=variant | flags, weight=2.0, ldvt=(Lk + 63) // 64 * 64) == EUNSUP
        msg = lib.yume_last_error().decode()
        assert f"variant {variant}" in msg and "last_key_weight" in msg


def test_short_key_kernel_refuses_more_than_128_keys():
    lib = _lib().load()
    for w in (1.0, 2.0):
        assert _call(lib, Lk=129, variant=10, weight=w) == EINVAL
        assert b"variant 10" in lib.yume_last_error() and b"128" in lib.yume_last_error()


def test_common_checks_still_come_first():
    lib = _lib().load()
    assert lib.yume_attn_fwd_kw(None, 128, None, 128, None, 8, None, 128, 4, 4, 1, 1.0, 0, 0, None, 0, 2.0, None) == EINVAL
    assert b"NULL" in lib.yume_last_error()
    assert _call(lib, Lk=78, variant=2, weight=2.0, ldvt=7) == EINVAL


@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("spike", [False, True])
def test_m_copies_of_a_key_are_one_key_with_weight_m(n, spike):
    """fp64 pin of the identity: softmax over n keys and m copies of key p == softmax over n + 1 keys in which key p counts m times."""
    g = torch.Generator().manual_seed(100 + n)
    m, D, Lq = 512 - n, 128, 33
    q = torch.randn(Lq, D, generator=g, dtype=torch.float64)
    k = torch.randn(n + 1, D, generator=g, dtype=torch.float64)
    v = torch.randn(n + 1, D, generator=g, dtype=torch.float64)
    if spike:
        k[n] = q[5] * 2.0                       # the pad key carries the row maximum of query 5
    scale = 1 / math.sqrt(D)
    k_exp = torch.cat([k[:n], k[n:].expand(m, D)])
    v_exp = torch.cat([v[:n], v[n:].expand(m, D)])
    want = torch.softmax(q @ k_exp.t() * scale, dim=-1) @ v_exp
    w = torch.ones(n + 1, dtype=torch.float64)
    w[n] = m
    e = torch.exp(q @ k.t() * scale - (q @ k.t() * scale).max(dim=-1, keepdim=True).values) * w
    got = (e @ v) / e.sum(dim=-1, keepdim=True)
    assert (got - want).abs().max() <= 1e-12 * max(want.abs().max().item(), 1.0)
