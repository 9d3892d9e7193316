"""yume_quant_rows_e4m3 and yume_gemm_f8 (ABI 9 + two exports): what can be said without a GPU. The exports exist, are declared and bound
with the argument lists of the header, the ABI number did not move, and the host-side validation answers every refusal row of
tests/gemm_f8_cases.py (and the quantiser's) before any launch: on a host without a device a launch would answer YUME_ELAUNCH instead."""
import ctypes
import os
import re

import pytest

import gemm_f8_cases as fc
from conftest import ROOT

EINVAL, EUNSUP, OK = -1, -3, 0
PTR = 4096            # pointers are never dereferenced on the host: any 16-byte aligned non-NULL value passes the common checks
P = ctypes.c_void_p


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
    so = ctypes.CDLL(_l.LIB_PATH)
    assert sorted(_l.SIGNATURES) == syms
    for name in ("yume_quant_rows_e4m3", "yume_gemm_f8"):
        assert name in syms and name in _l.SIGNATURES and hasattr(so, name)
        decl = re.search(r"int %s\((.*?)\);" % name, src, flags=re.S).group(1)
        kinds = []
        for arg in decl.split(","):
            arg = arg.strip()
            kinds.append(ctypes.c_void_p if "*" in arg else {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}[arg.split()[0]])
        assert kinds == _l.SIGNATURES[name], name
        assert name not in _l._RES
    lib = _l.load()
    # added exports change no argument list: the ABI number stays
    assert lib.yume_abi_version() == _l.ABI_VERSION == 9 == int(re.search(r"#define YUME_ABI_VERSION (\d+)", hdr).group(1))
    from yume_amd import ops
    assert callable(ops.quant_rows_e4m3) and callable(ops.gemm_f8)


@pytest.mark.parametrize("name, kw, rc", fc.REFUSALS, ids=[r[0] for r in fc.REFUSALS])
def test_gemm_f8_refusals_answer_before_any_launch(name, kw, rc):
    lib = _lib().load()
    assert fc.refusal_call(lib, kw) == rc
    assert b"gemm_f8" in lib.yume_last_error()


def test_gemm_f8_refusals_name_what_is_wrong():
    lib = _lib().load()
    for kw, word in ((dict(epi=fc.EPI_SPLITT), b"epilogue 4"), (dict(K=192), b"K=192"), (dict(lda_x=8), b"lda"), (dict(a_off=8), b"aligned")):
        fc.refusal_call(lib, kw)
        assert word in lib.yume_last_error(), (kw, lib.yume_last_error())
    # NULL operands and scales
    assert lib.yume_gemm_f8(None, 256, P(PTR), P(PTR), 256, P(PTR), None, 256, 256, 256, 0, P(PTR), 256, None, 0, None, None) == EINVAL
    assert lib.yume_gemm_f8(P(PTR), 256, None, P(PTR), 256, P(PTR), None, 256, 256, 256, 0, P(PTR), 256, None, 0, None, None) == EINVAL
    assert b"NULL" in lib.yume_last_error()
    # RESID: the gate's stride and alignment
    assert lib.yume_gemm_f8(P(PTR), 256, P(PTR), P(PTR), 256, P(PTR), None, 256, 256, 256, 3, P(PTR), 256, P(PTR), 6 * 256 + 2, None, None) == EINVAL
    assert b"gate" in lib.yume_last_error()


def _quant(lib, x=PTR, ldx=136, R=5, K=128, q=PTR, ldq=144, scale=PTR):
    return lib.yume_quant_rows_e4m3(P(x) if x else None, ldx, R, K, P(q) if q else None, ldq, P(scale) if scale else None, None)


@pytest.mark.parametrize("kw, word", [(dict(K=120), b"K=120"), (dict(ldq=136), b"ldq"), (dict(ldq=112), b"ldq"), (dict(ldx=132), b"ldx"),
                                      (dict(x=PTR + 8), b"aligned"), (dict(q=PTR + 8), b"aligned"), (dict(x=None), b"NULL"), (dict(K=0), b"shape"),
                                      (dict(R=-1), b"shape")])
def test_quant_rows_refusals_answer_before_any_launch(kw, word):
    lib = _lib().load()
    assert _quant(lib, **kw) == EINVAL
    assert b"quant_rows_e4m3" in lib.yume_last_error() and word in lib.yume_last_error()


def test_quant_rows_of_no_rows_is_ok_without_a_launch():
    lib = _lib().load()
    assert _quant(lib, R=0) == OK
    assert _quant(lib, R=0, x=None, q=None, scale=None) == OK
