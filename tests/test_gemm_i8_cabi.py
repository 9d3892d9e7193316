"""yume_quant_rows_i8, yume_adaln_modulate_i8, yume_gemm_i8 and yume_gemm_i8_splitt (ABI 9 + four exports): what can be said without a GPU.
The exports exist, are declared and bound with the argument lists of the header, the ABI number did not move, and the host-side validation
answers every refusal row of tests/gemm_i8_cases.py (and the quantiser's and the emitter's) before any launch: on a host without a device
a launch would answer YUME_ELAUNCH instead."""
import ctypes
import os
import re

import pytest

import gemm_i8_cases as ic
from conftest import ROOT

EINVAL, EUNSUP, OK = -1, -3, 0
PTR = 4096            # pointers are never dereferenced on the host: any 16-byte aligned non-NULL value passes the common checks
P = ctypes.c_void_p
NAMES = ("yume_quant_rows_i8", "yume_adaln_modulate_i8", "yume_gemm_i8", "yume_gemm_i8_splitt")


def _lib():
    import __graft_entry__ as g
    g.build()
    from yume_amd import _lib
    return _lib


def test_export_header_and_binding_agree():
    _l = _lib()
    hdr = open(os.path.join(ROOT, "include", "yume_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    so = ctypes.CDLL(_l.LIB_PATH)
    for name in NAMES:
        assert name in _l.SIGNATURES and hasattr(so, name)
        decl = re.search(r"int %s\((.*?)\);" % name, src, flags=re.S).group(1)
        kinds = []
        for arg in decl.split(","):
            arg = arg.strip()
            kinds.append(ctypes.c_void_p if "*" in arg else {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}[arg.split()[0]])
        assert kinds == _l.SIGNATURES[name], name
        assert name not in _l._RES
    # the emitter and the QKV form take the argument lists of their e4m3 counterparts
    assert _l.SIGNATURES["yume_adaln_modulate_i8"] == _l.SIGNATURES["yume_adaln_modulate_e4m3"]
    assert _l.SIGNATURES["yume_quant_rows_i8"] == _l.SIGNATURES["yume_quant_rows_e4m3"]
    assert _l.SIGNATURES["yume_gemm_i8_splitt"] == _l.SIGNATURES["yume_gemm_f8_splitt"]
    lib = _l.load()
    # added exports change no argument list: the ABI number stays
    assert lib.yume_abi_version() == _l.ABI_VERSION == 9 == int(re.search(r"#define YUME_ABI_VERSION (\d+)", hdr).group(1))
    from yume_amd import ops
    assert callable(ops.quant_rows_i8) and callable(ops.adaln_modulate_i8) and callable(ops.gemm_i8) and callable(ops.gemm_i8_splitt)


@pytest.mark.parametrize("name, kw, rc", ic.REFUSALS, ids=[r[0] for r in ic.REFUSALS])
def test_gemm_i8_refusals_answer_before_any_launch(name, kw, rc):
    lib = _lib().load()
    assert ic.refusal_call(lib, kw) == rc
    assert b"gemm_i8:" in lib.yume_last_error()


@pytest.mark.parametrize("name, kw, rc", ic.REFUSALS_SPLITT, ids=[r[0] for r in ic.REFUSALS_SPLITT])
def test_gemm_i8_splitt_refusals_answer_before_any_launch(name, kw, rc):
    lib = _lib().load()
    assert ic.refusal_call_splitt(lib, kw) == rc
    assert b"gemm_i8_splitt:" in lib.yume_last_error()


def test_gemm_i8_refusals_name_what_is_wrong():
    lib = _lib().load()
    for kw, word in ((dict(epi=ic.EPI_SPLITT), b"epilogue 4"), (dict(epi=ic.EPI_RESID), b"epilogue 3"), (dict(K=192), b"K=192"),
                     (dict(K=ic.MAX_K + 128), b"int32"), (dict(lda_x=8), b"lda"), (dict(a_off=8), b"aligned"), (dict(sa=None), b"NULL")):
        ic.refusal_call(lib, kw)
        assert word in lib.yume_last_error(), (kw, lib.yume_last_error())
    for kw, word in ((dict(n_split=128), b"n_split=128"), (dict(ldt=248), b"ldt=248"), (dict(K=ic.MAX_K + 128), b"int32")):
        ic.refusal_call_splitt(lib, kw)
        assert word in lib.yume_last_error(), (kw, lib.yume_last_error())


def test_the_largest_k_passes_the_k_check():
    """K = 131072 itself is taken: the call gets as far as the next check (a misaligned operand)"""
    lib = _lib().load()
    assert ic.refusal_call(lib, dict(K=ic.MAX_K, a_off=8)) == EINVAL
    assert b"aligned" in lib.yume_last_error()


def _quant(lib, x=PTR, ldx=136, R=5, K=128, q=PTR, ldq=144, scale=PTR):
    return lib.yume_quant_rows_i8(P(x) if x else None, ldx, R, K, P(q) if q else None, ldq, P(scale) if scale else None, None)


@pytest.mark.parametrize("kw, word", [(dict(K=120), b"K=120"), (dict(ldq=136), b"ldq"), (dict(ldq=112), b"ldq"), (dict(ldx=132), b"ldx"),
                                      (dict(x=PTR + 8), b"aligned"), (dict(q=PTR + 8), b"aligned"), (dict(x=None), b"NULL"), (dict(K=0), b"shape"),
                                      (dict(R=-1), b"shape")])
def test_quant_rows_i8_refusals_answer_before_any_launch(kw, word):
    lib = _lib().load()
    assert _quant(lib, **kw) == EINVAL
    assert b"quant_rows_i8" in lib.yume_last_error() and word in lib.yume_last_error()


def test_quant_rows_i8_of_no_rows_is_ok_without_a_launch():
    lib = _lib().load()
    assert _quant(lib, R=0) == OK
    assert _quant(lib, R=0, x=None, q=None, scale=None) == OK


def _emit(lib, x=PTR, ldx=512, T=5, C=512, tab_stride=3072, q=PTR, ldq=512, scale=PTR, mul=PTR, add=PTR):
    p = lambda v: P(v) if v else None
    return lib.yume_adaln_modulate_i8(p(x), ldx, T, C, 1e-6, p(mul), p(add), tab_stride, None, 1, p(q), ldq, p(scale), None)


@pytest.mark.parametrize("kw, word", [(dict(C=520), b"C=520"), (dict(C=8704, ldq=8704, ldx=8704), b"C <= 8192"), (dict(ldq=520), b"ldq"),
                                      (dict(ldq=496), b"ldq"), (dict(ldx=514), b"strides"), (dict(tab_stride=3074), b"strides"),
                                      (dict(q=PTR + 8), b"aligned"), (dict(x=None), b"NULL"), (dict(scale=None), b"NULL")])
def test_adaln_modulate_i8_refusals_answer_before_any_launch(kw, word):
    lib = _lib().load()
    assert _emit(lib, **kw) == EINVAL
    assert b"adaln_modulate_i8" in lib.yume_last_error() and word in lib.yume_last_error(), lib.yume_last_error()


def test_adaln_modulate_i8_of_no_rows_is_ok_without_a_launch():
    lib = _lib().load()
    assert _emit(lib, T=0) == OK
    assert _emit(lib, T=0, x=None, q=None, scale=None) == OK
