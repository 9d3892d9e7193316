"""The C ABI of yume_attn_fwd_fprefix without a GPU (NULL stream, pointers never dereferenced on the host): the export, the header and the
binding agree, the ABI number stays, and every row of tests/attn_fprefix_cases.py's REFUSALS is answered by code and by name before any launch."""
import ctypes
import os
import re

import pytest

import attn_fprefix_cases as pc
from conftest import ROOT

PTR = 4096            # any 16-byte aligned non-NULL value passes the common checks


def _lib():
    import __graft_entry__ as g
    g.build()
    from yume_amd import _lib
    return _lib


def _call(lib, Q=PTR, K=PTR, Vt=PTR, O=PTR, Kp=PTR, Vtp=PTR, null_spans=False, **kw):
    a = dict(pc.REFUSAL_DEFAULT, **kw)
    spans, H = a["spans"], a["H"]
    arr = ctypes.c_int64 * max(len(spans), 1)
    rows, blocks = arr(*[r for r, _ in spans]), arr(*[b for _, b in spans])
    return lib.yume_attn_fwd_fprefix(Q, H * 128, K, H * 128, Vt, a["ldvt"], O, H * 128, a["Lq"], a["Lk"], H, 0.088, 0, a["variant"], a["q_pos0"],
                                     len(spans), None if null_spans else rows, blocks, a["back"], a["ahead"], Kp, a["ldkp"], Vtp, a["ldvtp"],
                                     a["n_prefix"], None, 0, None)


def test_export_header_and_binding_agree_and_the_abi_number_stays():
    _l = _lib()
    hdr = open(os.path.join(ROOT, "include", "yume_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    syms = sorted(set(re.findall(r"\b(yume_[a-z0-9_]+)\s*\(", src)))
    assert "yume_attn_fwd_fprefix" in syms and sorted(_l.SIGNATURES) == syms
    # yume_attn_fwd_fband's argument list with the five prefix arguments behind `ahead`
    a, b = _l.SIGNATURES["yume_attn_fwd_fband"], _l.SIGNATURES["yume_attn_fwd_fprefix"]
    assert len(b) == len(a) + 5 and b[:20] == a[:20] and b[25:] == a[20:]
    assert b[20:25] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]
    decl = re.search(r"int yume_attn_fwd_fprefix\((.*?)\);", src, flags=re.S).group(1)
    assert re.search(r"int64_t back,\s*int64_t ahead,\s*const void\* Kp,\s*int64_t ldkp,\s*const void\* Vtp,\s*int64_t ldvtp,\s*int64_t n_prefix,"
                     r"\s*void\* workspace", decl)
    assert hasattr(ctypes.CDLL(_l.LIB_PATH), "yume_attn_fwd_fprefix")
    assert _l.load().yume_abi_version() == _l.ABI_VERSION == 9 == int(re.search(r"#define YUME_ABI_VERSION (\d+)", hdr).group(1))


def test_the_default_call_of_the_refusals_passes_every_check():
    """(NULL stream, no GPU: the launch itself fails or not, but no argument check answers)"""
    d = pc.REFUSAL_DEFAULT
    assert d["n_prefix"] >= 1 and d["ldvtp"] >= d["n_prefix"] and d["ldvtp"] % 8 == 0 and d["ldkp"] % 8 == 0
    assert d["q_pos0"] + d["Lq"] <= pc.total_rows(d["spans"]) and d["Lk"] <= pc.total_rows(d["spans"]) and d["ldvt"] >= d["Lk"]


@pytest.mark.parametrize("name,kw,code,word,who", pc.REFUSALS, ids=[r[0] for r in pc.REFUSALS])
def test_refusals_answer_by_name_before_any_launch(name, kw, code, word, who):
    lib = _lib().load()
    assert _call(lib, **kw) == code
    msg = lib.yume_last_error().decode()
    assert msg.startswith(who + ":") and word in msg, msg
