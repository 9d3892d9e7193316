"""yume_vae_rmsnorm_silu_mx and yume_conv3d_cl_f8mx without a GPU: the exports exist and are bound with the header's argument lists, the ABI
number did not move, and the host-side validation answers every refusal of tests/conv_f8_cases.py before any launch: on a host without a
device a launch would answer YUME_ELAUNCH instead."""
import ctypes
import os
import re

import pytest

import conv_f8_cases as cc
from conftest import ROOT

NAMES = ("yume_vae_rmsnorm_silu_mx", "yume_conv3d_cl_f8mx")


def _lib():
    import __graft_entry__ as g
    g.build()
    from yume_amd import _lib
    return _lib


def _header_kinds(src, name):
    decl = re.search(r"int %s\((.*?)\);" % name, src, flags=re.S).group(1)
    kinds = []
    for arg in decl.split(","):
        arg = arg.strip()
        kinds.append(ctypes.c_void_p if "*" in arg else {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}[arg.split()[0]])
    return kinds


def test_exports_header_and_binding_agree():
    _l = _lib()
    hdr = open(os.path.join(ROOT, "include", "yume_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    so = ctypes.CDLL(_l.LIB_PATH)
    for name in NAMES:
        assert name in _l.SIGNATURES and hasattr(so, name) and name not in _l._RES
        assert _header_kinds(src, name) == _l.SIGNATURES[name], name
    # the producer: yume_vae_rmsnorm_silu's list with (y, ldy) replaced by (q, ldq, e, lde)
    base, mx = _l.SIGNATURES["yume_vae_rmsnorm_silu"], _l.SIGNATURES["yume_vae_rmsnorm_silu_mx"]
    assert mx[:7] == base[:7] and mx[7:] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    # the consumer: yume_conv3d_cl's list with (x, cache, ldc) -> (xq, xe, cacheq, cachee, ldc, lde) and sw behind the weight pitch
    base, f8 = _l.SIGNATURES["yume_conv3d_cl"], _l.SIGNATURES["yume_conv3d_cl_f8mx"]
    assert f8[6:12] == base[3:9] and f8[13:] == base[9:] and len(f8) == len(base) + 4
    assert _l.load().yume_abi_version() == _l.ABI_VERSION == 9 == int(re.search(r"#define YUME_ABI_VERSION (\d+)", hdr).group(1))
    from yume_amd import vae_ops
    assert callable(vae_ops.rmsnorm_silu_mx) and callable(vae_ops.conv3d_cl_f8mx)


@pytest.mark.parametrize("name, kw, rc", cc.REFUSALS, ids=[r[0] for r in cc.REFUSALS])
def test_conv_refusals_answer_before_any_launch(name, kw, rc):
    lib = _lib().load()
    assert cc.refusal_call(lib, kw) == rc, lib.yume_last_error()
    assert b"conv3d_cl_f8mx" in lib.yume_last_error()


@pytest.mark.parametrize("name, kw", cc.PREFUSALS, ids=[r[0] for r in cc.PREFUSALS])
def test_producer_refusals_answer_before_any_launch(name, kw):
    lib = _lib().load()
    assert cc.prefusal_call(lib, kw) == cc.EINVAL, lib.yume_last_error()
    assert b"vae_rmsnorm_silu_mx" in lib.yume_last_error()
