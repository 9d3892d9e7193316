"""yume_adaln_modulate_e4m3 without a GPU: the export exists and is bound with the header's argument list, the ABI number did not move, and
the host-side validation answers the shape refusals (C % 16, ldq % 16, ldq >= C, as yume_quant_rows_e4m3 has them) before any launch: on a
host without a device a launch would answer YUME_ELAUNCH instead."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

EINVAL, OK = -1, 0
PTR = 4096            # never dereferenced on the host
P = ctypes.c_void_p


def _lib():
    import __graft_entry__ as g
    g.build()
    from yume_amd import _lib
    return _lib


def _call(lib, x=PTR, ldx=512, T=5, C=512, mul=PTR, add=PTR, tab_stride=1024, q=PTR, ldq=512, scale=PTR):
    p = lambda v: P(v) if v else None
    return lib.yume_adaln_modulate_e4m3(p(x), ldx, T, C, 1e-6, p(mul), p(add), tab_stride, None, 1, p(q), ldq, p(scale), None)


def test_export_header_and_binding_agree():
    _l = _lib()
    hdr = open(os.path.join(ROOT, "include", "yume_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    name = "yume_adaln_modulate_e4m3"
    so = ctypes.CDLL(_l.LIB_PATH)
    assert name in _l.SIGNATURES and hasattr(so, name) and name not in _l._RES
    decl = re.search(r"int %s\((.*?)\);" % name, src, flags=re.S).group(1)
    kinds = []
    for arg in decl.split(","):
        arg = arg.strip()
        kinds.append(ctypes.c_void_p if "*" in arg else {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}[arg.split()[0]])
    assert kinds == _l.SIGNATURES[name]
    # yume_adaln_modulate's list with (out, ldo, out_kind) replaced by (q, ldq, scale)
    base = _l.SIGNATURES["yume_adaln_modulate"]
    assert kinds[:10] == base[:10] and kinds[10:] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    assert _l.load().yume_abi_version() == _l.ABI_VERSION == 9 == int(re.search(r"#define YUME_ABI_VERSION (\d+)", hdr).group(1))
    from yume_amd import ops
    assert callable(ops.adaln_modulate_e4m3)


@pytest.mark.parametrize("kw, word", [(dict(C=520, ldq=528), b"C=520"), (dict(C=8, ldq=16), b"C=8"), (dict(ldq=520), b"ldq=520"),
                                      (dict(ldq=496), b"ldq=496"), (dict(C=8208, ldq=8208), b"C=8208"), (dict(ldx=514), b"strides"),
                                      (dict(q=PTR + 8), b"aligned"), (dict(x=None), b"NULL"), (dict(scale=None), b"NULL"), (dict(T=-1), b"shape")])
def test_refusals_answer_before_any_launch(kw, word):
    lib = _lib().load()
    assert _call(lib, **kw) == EINVAL
    assert b"adaln_modulate_e4m3" in lib.yume_last_error() and word in lib.yume_last_error(), lib.yume_last_error()


def test_no_rows_is_ok_without_a_launch():
    lib = _lib().load()
    assert _call(lib, T=0) == OK
    assert _call(lib, T=0, x=None, q=None, scale=None) == OK
