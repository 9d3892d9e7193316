"""The C ABI of yume_attn_fwd_fsink without a GPU (NULL stream, pointers never dereferenced on the host): the export, the header and the
binding agree, the ABI number stays, and every row of tests/attn_fsink_cases.py's REFUSALS is answered by code and by name before any launch."""
import ctypes
import os
import re

import pytest

import attn_fsink_cases as sc
from conftest import ROOT

PTR = 4096            # any 16-byte aligned non-NULL value passes the common checks


def _lib():
    import __graft_entry__ as g
    g.build()
    from yume_amd import _lib
    return _lib


def _call(lib, Q=PTR, K=PTR, Vt=PTR, O=PTR, Lq=300, Lk=315, H=2, ldvt=320, variant=0, q_pos0=0, spans=sc.ONE_SPAN, back=1, ahead=0, sink=1,
          null_spans=False):
    arr = ctypes.c_int64 * max(len(spans), 1)
    rows, blocks = arr(*[r for r, _ in spans]), arr(*[b for _, b in spans])
    return lib.yume_attn_fwd_fsink(Q, H * 128, K, H * 128, Vt, ldvt, O, H * 128, Lq, Lk, H, 0.088, 0, variant, q_pos0, len(spans),
                                   None if null_spans else rows, blocks, back, ahead, sink, None, 0, None)


def test_export_header_and_binding_agree_and_the_abi_number_stays():
    _l = _lib()
    hdr = open(os.path.join(ROOT, "include", "yume_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    syms = sorted(set(re.findall(r"\b(yume_[a-z0-9_]+)\s*\(", src)))
    assert "yume_attn_fwd_fsink" in syms and sorted(_l.SIGNATURES) == syms
    # yume_attn_fwd_fband's argument list with `int64_t sink` behind `ahead`
    a, b = _l.SIGNATURES["yume_attn_fwd_fband"], _l.SIGNATURES["yume_attn_fwd_fsink"]
    assert len(b) == 24 and b[:20] == a[:20] and b[20] is ctypes.c_int64 and b[21:] == a[20:]
    decl = re.search(r"int yume_attn_fwd_fsink\((.*?)\);", src, flags=re.S).group(1)
    assert re.search(r"int64_t back,\s*int64_t ahead,\s*int64_t sink,\s*void\* workspace", decl)
    assert hasattr(ctypes.CDLL(_l.LIB_PATH), "yume_attn_fwd_fsink")
    assert _l.load().yume_abi_version() == _l.ABI_VERSION == 9 == int(re.search(r"#define YUME_ABI_VERSION (\d+)", hdr).group(1))


def test_the_default_call_of_the_refusals_is_one_the_kernel_would_run():
    c = sc.SCase("refusal_default", sc.ONE_SPAN, 300, 315, 0, 1, 0, 1)
    assert not sc.hides_nothing(c.Lq, c.Lk, *sc.rule(c)) and not sc.adds_nothing(c.Lq, c.Lk, *sc.rule(c))


@pytest.mark.parametrize("name,kw,code,word,who", sc.REFUSALS, ids=[r[0] for r in sc.REFUSALS])
def test_refusals_answer_by_name_before_any_launch(name, kw, code, word, who):
    lib = _lib().load()
    assert _call(lib, **kw) == code
    msg = lib.yume_last_error().decode()
    assert msg.startswith(who + ":") and word in msg, msg
